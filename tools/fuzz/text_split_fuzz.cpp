// Fuzzer of the FASTQ record rule (charon_amd/csrc/parts/text_split.inc) on a CPU build under ASan / UBSan: tsp_host_job, the body of
// chn_text_split_host, which applies the very tsp_record that chn_text_split's kernels compile.  Every case is compared with a plain
// sequential parser written here from the rule in include/charon_hip.h: every descriptor, n_records, consumed, ids_bytes and the ids.
//   g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Icharon_amd/csrc tools/fuzz/text_split_fuzz.cpp -o /tmp/text_split_fuzz
//   /tmp/text_split_fuzz [cases] [seed]
// Cases: FASTQ texts of 0 - 40 short records (ids now and then empty, line ends \n, \r\n or mixed) with 0 - 4 mutations at line level:
// a line feed, \r, '@' or '+' dropped, inserted or doubled, a line dropped or doubled, a blank line, a truncation; a `start` at a record
// boundary or anywhere; a max_records at, below or above the count.  The text, every descriptor array and the id buffer are allocated
// at exactly their sizes, so ASan watches their ends.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "charon_hip.h"
#include "parts/text_split.inc"

static uint64_t g_x = 1;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }

struct Rec { uint64_t id_off, seq_off, qual_off; uint32_t id_len, seq_len; };

// the yardstick: one record after another, byte by byte
static bool line_end(const std::string &t, uint64_t from, uint64_t end, uint64_t &feed) {
    for (uint64_t i = from; i < end; ++i) if (t[i] == '\n') { feed = i; return true; }
    return false;
}
static uint64_t parse(const std::string &t, uint64_t start, uint64_t end, uint64_t max_records, std::vector<Rec> &out, std::string &ids) {
    uint64_t p = start;
    while (out.size() < max_records) {
        if (p >= end || t[p] != '@') break;
        uint64_t f[4], q = p;
        bool four = true;
        for (int k = 0; k < 4 && four; ++k) { four = line_end(t, q, end, f[k]); q = f[k] + 1; }
        if (!four) break;
        auto stripped = [&](uint64_t a, uint64_t b) { return b > a && t[b - 1] == '\r' ? b - 1 - a : b - a; };  // length of line [a, b) without one \r
        const uint64_t n1 = stripped(f[0] + 1, f[1]);
        if (n1 == 0 || t[f[0] + 1] == '+') break;
        if (t[f[1] + 1] != '+') break;  // (an empty third line holds its line feed there)
        if (stripped(f[2] + 1, f[3]) != n1) break;
        Rec r;
        r.id_off = p + 1; r.id_len = (uint32_t)stripped(p + 1, f[0]);
        r.seq_off = f[0] + 1; r.seq_len = (uint32_t)n1; r.qual_off = f[2] + 1;
        out.push_back(r);
        ids.append(t, r.id_off, r.id_len);
        p = f[3] + 1;
    }
    return p;
}

static std::string letters(const char *alphabet, size_t n) {
    std::string s(n, 'A');
    const size_t k = std::strlen(alphabet);
    for (size_t i = 0; i < n; ++i) s[i] = alphabet[rnd() % k];
    return s;
}

int main(int argc, char **argv) {
    const long cases = argc > 1 ? std::atol(argv[1]) : 200000;
    g_x = (argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1) * 0x9E3779B97F4A7C15ULL + 1;
    long bad = 0, refused = 0;
    uint64_t taken = 0, stopped_early = 0;
    for (long c = 0; c < cases; ++c) {
        // lines, each with its line end
        std::vector<std::string> lines;
        std::vector<uint64_t> bounds(1, 0);
        const unsigned n_recs = (unsigned)(rnd() % 41), eol_mode = (unsigned)(rnd() % 3);
        for (unsigned i = 0; i < n_recs; ++i) {
            const size_t len = 1 + rnd() % (rnd() % 8 ? 30 : 300);
            auto eol = [&]() { return std::string(eol_mode == 1 || (eol_mode == 2 && rnd() % 2) ? "\r\n" : "\n"); };
            lines.push_back("@" + (rnd() % 6 ? letters("abc019 /:_", rnd() % 20) : std::string()) + eol());
            lines.push_back(letters("ACGTN", len) + eol());
            lines.push_back("+" + (rnd() % 4 ? std::string() : letters("abc0", rnd() % 10)) + eol());
            lines.push_back(letters("FF:,#@+!~", len) + eol());
            uint64_t b = bounds.back();
            for (size_t k = lines.size() - 4; k < lines.size(); ++k) b += lines[k].size();
            bounds.push_back(b);
        }
        for (unsigned m = (unsigned)(rnd() % 5); m > 0 && !lines.empty(); --m) {
            const size_t i = rnd() % lines.size();
            std::string &l = lines[i];
            const char what = "\n\r@+"[rnd() % 4];
            switch (rnd() % 8) {
                case 0: { const size_t at = l.find(what); if (at != std::string::npos) l.erase(at, 1); break; }   // dropped
                case 1: l.insert(rnd() % (l.size() + 1), 1, what); break;                                          // inserted
                case 2: { const size_t at = l.find(what); if (at != std::string::npos) l.insert(at, 1, what); break; }  // doubled
                case 3: lines.erase(lines.begin() + (long)i); break;
                case 4: lines.insert(lines.begin() + (long)i, lines[i]); break;
                case 5: lines.insert(lines.begin() + (long)i, rnd() % 2 ? "\n" : "\r\n"); break;                   // a blank line
                case 6: l.insert(0, 1, what); break;
                default: lines.resize(i + 1); lines[i].resize(rnd() % (lines[i].size() + 1)); break;               // truncated
            }
        }
        std::string t;
        for (const std::string &l : lines) t += l;
        const uint64_t end = t.size();
        uint64_t start = 0;
        if (rnd() % 3 == 0) start = rnd() % 2 ? std::min<uint64_t>(bounds[rnd() % bounds.size()], end) : rnd() % (end + 1);
        uint64_t max_records = rnd() % 4 ? 1000 : rnd() % (n_recs + 2);
        const bool want_ids = rnd() % 4 != 0;

        std::vector<Rec> want;
        std::string want_ids_bytes;
        const uint64_t consumed = parse(t, start, end, max_records, want, want_ids_bytes);
        uint64_t ids_capacity = want_ids_bytes.size();
        const bool too_small = want_ids && ids_capacity && rnd() % 16 == 0;
        if (too_small) --ids_capacity;

        // the code under test, on buffers of exactly the sizes it may touch
        uint8_t *text = new uint8_t[end ? end : 1];
        if (end) std::memcpy(text, t.data(), end);
        const size_t m = (size_t)max_records;
        uint64_t *id_off = new uint64_t[m ? m : 1], *seq_off = new uint64_t[m ? m : 1], *qual_off = new uint64_t[m ? m : 1];
        uint32_t *id_len = new uint32_t[m ? m : 1], *seq_len = new uint32_t[m ? m : 1];
        uint8_t *ids = new uint8_t[ids_capacity ? ids_capacity : 1];
        chn_text_split_job j;
        std::memset(&j, 0, sizeof j);
        j.struct_size = sizeof j;
        j.text = text; j.text_bytes = end; j.start = start; j.max_records = max_records;
        j.id_offset = id_off; j.id_length = id_len; j.seq_offset = seq_off; j.seq_length = seq_len; j.qual_offset = qual_off;
        j.ids = want_ids ? ids : nullptr; j.ids_capacity = ids_capacity;
        j.n_records = j.consumed = j.ids_bytes = 0xDEAD;
        std::string why;
        const int rc = tsp_host_job(&j, why);
        bool ok;
        if (too_small) { ok = rc == CHN_E_CAPACITY && why.find(std::to_string(want_ids_bytes.size()) + " bytes") != std::string::npos; ++refused; }
        else {
            ok = rc == 0 && j.n_records == want.size() && j.consumed == consumed && j.ids_bytes == want_ids_bytes.size();
            for (size_t i = 0; ok && i < want.size(); ++i)
                ok = id_off[i] == want[i].id_off && id_len[i] == want[i].id_len && seq_off[i] == want[i].seq_off && seq_len[i] == want[i].seq_len && qual_off[i] == want[i].qual_off;
            if (ok && want_ids && !want_ids_bytes.empty()) ok = std::memcmp(ids, want_ids_bytes.data(), want_ids_bytes.size()) == 0;
            taken += want.size();
            stopped_early += want.size() < n_recs;
        }
        if (!ok && ++bad < 10) std::printf("case %ld: rc %d (%s), records %llu / %zu, consumed %llu / %llu, start %llu of %llu bytes\n", c, rc, why.c_str(),
                                           (unsigned long long)j.n_records, want.size(), (unsigned long long)j.consumed, (unsigned long long)consumed,
                                           (unsigned long long)start, (unsigned long long)end);
        delete[] text; delete[] id_off; delete[] seq_off; delete[] qual_off; delete[] id_len; delete[] seq_len; delete[] ids;
    }
    std::printf("%ld cases, %llu records taken, %llu cases stopped before their last record, %ld refused for ids_capacity, %ld disagreements\n", cases,
                (unsigned long long)taken, (unsigned long long)stopped_early, refused, bad);
    return bad ? 1 : 0;
}
