// Checks charon_amd/csrc/parts/rowlog_entry.hpp -- the compact row-log entry, its chain mode and the walk k_count_wavelog does over a
// log -- against plain bit arithmetic on the rows themselves.  No GPU, no HIP:
//   g++ -std=c++14 -O1 -fsanitize=address,undefined -Icharon_amd/csrc/parts tools/rowlog_entry_check.cpp -o rowlog_entry_check && ./rowlog_entry_check
// Prints one line per fact and "ok"; exits 1 at the first mismatch.  (tests/test_rowlog_entry_cpu.py builds and runs it.)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rowlog_entry.hpp"

static void fail(const char *what, unsigned long long a, unsigned long long b, unsigned long long c) {
    std::fprintf(stderr, "FAILED: %s (%llu, %llu, %llu)\n", what, a, b, c);
    std::exit(1);
}
static uint64_t rnd_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() {
    uint64_t z = (rnd_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// the entry as it was before there were chains, restated: what `chain == 0` must still give, bit for bit
template <int W>
static uint32_t legacy_encode(const uint64_t *acc, uint32_t B, uint32_t owner, bool &escaped) {
    uint64_t m[W];
    uint32_t pc = 0;
    for (int w = 0; w < W; ++w) {
        m[w] = acc[w];
        if (w == W - 1 && (B & 63u)) m[w] &= (1ULL << (B & 63u)) - 1;
        for (int b = 0; b < 64; ++b) pc += (uint32_t)((m[w] >> b) & 1u);
    }
    escaped = pc > 3;
    if (escaped) return owner << 26;
    uint32_t e = pc | (owner << 26), slot = 0;
    for (int w = 0; w < W; ++w)
        for (uint32_t b = 0; b < 64; ++b)
            if ((m[w] >> b) & 1u) { e |= ((uint32_t)w * 64 + b) << (2 + 8 * slot); ++slot; }
    return e;
}

// a log that refuses to be read at or beyond its count
struct GuardedLog {
    const std::vector<uint32_t> &v;
    uint32_t count;
    uint32_t operator[](uint32_t i) const {
        if (i >= count) fail("read at or beyond count", i, count, 0);
        return v[i];
    }
};

template <int W>
struct Row { uint64_t w[W]; uint32_t owner; };

template <int W>
static bool bit(const uint64_t *w, uint32_t b) { return b < 64u * W && ((w[b >> 6] >> (b & 63u)) & 1ULL); }

// One wavefront's log of `rows` (the probe kernel's side), then the count kernel's two passes over it.
template <int W>
static void check_log(const std::vector<Row<W>> &rows, uint32_t B, bool chain, unsigned long long &n_chained, unsigned long long &n_escaped, unsigned long long &n_entries) {
    const uint64_t lastmask = (B & 63u) ? ((1ULL << (B & 63u)) - 1) : ~0ULL;
    std::vector<uint32_t> log;
    std::vector<uint64_t> esc;  // the escaped-row region
    std::vector<uint32_t> first_entry;  // of every row that has one
    std::vector<uint32_t> row_of_entry;
    for (size_t r = 0; r < rows.size(); ++r) {
        uint32_t e[2];
        bool escaped = false;
        const uint32_t n = rowlog_encode<W>(rows[r].w, B, rows[r].owner, chain, e, escaped);
        uint32_t pc = 0;
        for (uint32_t b = 0; b < B; ++b) pc += bit<W>(rows[r].w, b);
        const uint32_t want_n = pc == 0 ? 0u : (chain && pc >= 4 && pc <= 6) ? 2u : 1u;
        if (n != want_n || escaped != (pc > (chain ? 6u : 3u))) fail("entries per row", pc, n, escaped);
        if (!chain) {
            bool esc0 = false;
            const uint32_t old = legacy_encode<W>(rows[r].w, B, rows[r].owner, esc0);
            if (old != e[0] || esc0 != escaped) fail("chain == 0 encodes as before", old, e[0], pc);
        }
        if (n == 0) continue;
        first_entry.push_back((uint32_t)log.size());
        if (escaped) {
            for (int w = 0; w < W; ++w) esc.push_back(rows[r].w[w]);
            e[0] |= (uint32_t)(esc.size() / W) << 2;  // (index + 1) << 2
            ++n_escaped;
        }
        for (uint32_t i = 0; i < n; ++i) { log.push_back(e[i]); row_of_entry.push_back((uint32_t)r); }
        if (n == 2) {
            ++n_chained;
            if (!rowlog_has_tail(e[0], chain) || !rowlog_is_tail(e[1], chain) || rowlog_is_tail(e[0], chain) || rowlog_has_tail(e[1], chain)) fail("chain flags", e[0], e[1], 0);
            if ((e[0] >> 26) != (e[1] >> 26)) fail("both halves name the owner", e[0], e[1], 0);
        } else if (!escaped && (rowlog_has_tail(e[0], chain) || rowlog_is_tail(e[0], chain))) fail("a single entry carries no chain flag", e[0], 0, 0);
    }
    n_entries += log.size();
    const uint32_t count = (uint32_t)log.size();
    const GuardedLog glog{log, count};

    // decode: the bins an entry (with its tail) or its escaped row names are the row's set bins; pass A's bumps are those bits
    std::vector<uint32_t> tot(64 * 64u * W, 0), want_tot(64 * 64u * W, 0);
    for (const auto &row : rows)
        for (uint32_t b = 0; b < B; ++b) want_tot[row.owner * 64u * W + b] += bit<W>(row.w, b);
    for (uint32_t e = 0; e < count; ++e) {  // pass A: every entry on its own
        const uint32_t x = glog[e], o = x >> 26, pc = rowlog_count(x);
        if (pc) {
            uint32_t prev = 0;
            for (uint32_t j = 0; j < pc; ++j) {
                const uint32_t b = rowlog_bin(x, j, chain);
                if (b >= B || (j && b <= prev)) fail("bins ascend below B", x, j, b);
                prev = b;
                tot[o * 64u * W + b] += 1;
            }
        } else if (x & ROWLOG_ESC_MASK) {
            const size_t j = ((x & ROWLOG_ESC_MASK) >> 2) - 1;
            for (int w = 0; w < W; ++w) {
                uint64_t rw = esc[j * W + w];
                if (w == W - 1) rw &= lastmask;
                for (uint32_t b = 0; b < 64; ++b) tot[o * 64u * W + w * 64 + b] += (uint32_t)((rw >> b) & 1u);
            }
        } else fail("an entry that names nothing", x, e, 0);
    }
    if (tot != want_tot) fail("pass A totals", B, chain, count);

    // pass B under random chosen-bin masks: found / fbin per row against popcount(row & mask) / its bit
    for (int trial = 0; trial < 1000; ++trial) {
        uint64_t cm[64][W];
        const uint32_t density = (uint32_t)(rnd() % 5);  // from sparse to every other bin
        for (auto &o : cm)
            for (int w = 0; w < W; ++w) {
                uint64_t m = rnd();
                for (uint32_t d = 0; d < density; ++d) m &= rnd();
                if (w == W - 1) m &= lastmask;
                o[w] = m;
            }
        size_t nrow = 0;
        for (uint32_t e = 0; e < count; ++e) {
            const uint32_t x = glog[e], o = x >> 26, pc = rowlog_count(x);
            uint32_t found = 0, fbin = 0;
            if (pc) {
                if (rowlog_is_tail(x, chain)) continue;
                auto chosen = [&](uint32_t b) -> bool { return (cm[o][b >> 6] >> (b & 63u)) & 1ULL; };
                found = rowlog_match(x, chain, chosen, fbin);
                if (rowlog_has_tail(x, chain)) found += rowlog_match(rowlog_tail(glog, e, count, chain), chain, chosen, fbin);
            } else {
                const size_t j = ((x & ROWLOG_ESC_MASK) >> 2) - 1;
                for (int w = 0; w < W; ++w) {
                    const uint64_t rw = esc[j * W + w] & cm[o][w];
                    found += (uint32_t)__builtin_popcountll(rw);
                    if (rw) fbin = w * 64 + (uint32_t)__builtin_ctzll(rw);
                }
            }
            if (nrow >= first_entry.size() || first_entry[nrow] != e) fail("pass B meets every row once, at its first entry", e, nrow, 0);
            const Row<W> &row = rows[row_of_entry[e]];
            uint32_t want = 0, wbin = 0;
            for (int w = 0; w < W; ++w) {  // popcount(row & mask) and its bit (the masks hold no bin at or above B)
                const uint64_t hit = row.w[w] & cm[o][w];
                want += (uint32_t)__builtin_popcountll(hit);
                if (hit) wbin = w * 64 + (uint32_t)__builtin_ctzll(hit);
            }
            if (found != want || (want == 1 && fbin != wbin)) fail("pass B found / fbin", found, want, fbin);
            ++nrow;
        }
        if (nrow != first_entry.size()) fail("pass B row count", nrow, first_entry.size(), 0);
    }

    // a log cut behind a chain's first entry: the entry is judged on its own and nothing at or beyond the count is read
    for (uint32_t e = 0; e + 1 < count; ++e)
        if (rowlog_has_tail(log[e], chain)) {
            const GuardedLog cut{log, e + 1};
            if (rowlog_tail(cut, e, e + 1, chain) != 0) fail("cut log: no tail", e, 0, 0);
            uint32_t fbin = 0;
            auto all = [](uint32_t) -> bool { return true; };
            if (rowlog_match(cut[e], chain, all, fbin) != 3) fail("cut log: the head's own three bins", e, 0, 0);
            if (rowlog_tail(glog, e, count, chain) != log[e + 1]) fail("whole log: the tail is the next entry", e, 0, 0);
        }
}

template <int W>
static void check_B(uint32_t B, bool chain, unsigned long long &n_rows, unsigned long long &n_chained, unsigned long long &n_escaped, unsigned long long &n_entries) {
    std::vector<Row<W>> rows;
    for (uint32_t owner = 0; owner < 64; ++owner)
        for (uint32_t nb = 0; nb <= 12; ++nb) {
                const int rep = (int)((owner + nb) & 1u);
                Row<W> row;
                std::memset(&row, 0, sizeof row);
                row.owner = owner;
                const uint32_t want = nb < B ? nb : B;
                uint32_t have = 0;
                while (have < want) {
                    // (the second row of every kind crowds the top bins: indices with bit 6 set, the last word's edge)
                    const uint32_t b = rep ? B - 1 - (uint32_t)(rnd() % (B < 2 * want + 2 ? B : 2 * want + 2)) : (uint32_t)(rnd() % B);
                    if (!bit<W>(row.w, b)) { row.w[b >> 6] |= 1ULL << (b & 63u); ++have; }
                }
                // technical bins at and above B are set at random: they never count
                for (uint32_t b = B; b < 64u * W; ++b)
                    if (rnd() & 1u) row.w[b >> 6] |= 1ULL << (b & 63u);
                rows.push_back(row);
            }
    // shuffle, so that chains, escapes and single entries of different owners interleave
    for (size_t i = rows.size(); i > 1; --i) { const size_t j = (size_t)(rnd() % i); const Row<W> t = rows[i - 1]; rows[i - 1] = rows[j]; rows[j] = t; }
    n_rows += rows.size();
    check_log<W>(rows, B, chain, n_chained, n_escaped, n_entries);
}

int main() {
    unsigned long long n_rows = 0, n_chained = 0, n_escaped = 0, n_entries = 0;
    const uint32_t Bs[] = {1, 63, 64, 65, 100, 127, 128};
    for (uint32_t B : Bs) {
        if (!rowlog_chain_ok(B)) fail("chain mode allowed up to 128 bins", B, 0, 0);
        for (int chain = 0; chain < 2; ++chain) {
            if (B <= 64) check_B<1>(B, chain != 0, n_rows, n_chained, n_escaped, n_entries);  // (W = ceil(B / 64) words per row, as in every index)
            else check_B<2>(B, chain != 0, n_rows, n_chained, n_escaped, n_entries);
        }
    }
    if (rowlog_chain_ok(129)) fail("no chain mode above 128 bins", 129, 0, 0);
    check_B<3>(129, false, n_rows, n_chained, n_escaped, n_entries);
    std::printf("rows: %llu in %llu entries; %llu chained (two entries), %llu escaped\n", n_rows, n_entries, n_chained, n_escaped);
    if (!n_chained || !n_escaped) fail("both chains and escapes occur", n_chained, n_escaped, 0);

    // by hand: a first entry whose successor is no tail is judged on its own; flags of an escaped entry's index bits are not flags
    {
        const std::vector<uint32_t> log = {3u | ROWLOG_CHAIN_NEXT | (5u << 2) | (9u << 10) | (77u << 18) | (7u << 26), 1u | (4u << 2) | (7u << 26)};
        const GuardedLog g{log, 2};
        if (rowlog_tail(g, 0, 2, true) != 0) fail("successor without the flag is no tail", 0, 0, 0);
        const uint32_t escaped_entry = ((0x8080u + 1u) << 2) | (3u << 26);  // index bits that fall on bits 9 and 17
        if (rowlog_is_tail(escaped_entry, true) || rowlog_has_tail(escaped_entry, true)) fail("escaped entries carry no chain flags", escaped_entry, 0, 0);
        if (rowlog_bin(log[0], 0, true) != 5 || rowlog_bin(log[0], 1, true) != 9 || rowlog_bin(log[0], 2, true) != 77) fail("bins under the flags", log[0], 0, 0);
        const uint32_t wide = 2u | (200u << 2) | (255u << 10);  // chain == 0: bins up to 255, bits 9 and 17 are bin bits
        if (rowlog_bin(wide, 0, false) != 200 || rowlog_bin(wide, 1, false) != 255 || rowlog_is_tail(wide, false) || rowlog_has_tail(wide, false)) fail("unchained wide bins", wide, 0, 0);
    }
    std::printf("ok\n");
    return 0;
}
