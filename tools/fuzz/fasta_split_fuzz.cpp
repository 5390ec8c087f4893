// Fuzzer of the FASTA record rule (charon_amd/csrc/parts/fasta_split.inc) on a CPU build under ASan / UBSan: fsp_host_job, the body of
// chn_fasta_split_host, which applies the very fsp_is_header / fsp_is_dropped / fsp_record that chn_fasta_split's kernels compile.
// Every case is compared with a straight restatement of BlockReader::parse_fasta (charon_amd/csrc/host/fastx_reader.inc) written here:
// its line loop, its clean-line shortcut and its byte loop, run over a copy of the text that it compacts in place as the reader does,
// stopped where the rule stops (an empty record, no header at the record's start, no header behind the record unless the input ends).
// Compared: every descriptor, n_records, consumed, ids_bytes, seq_bytes, the ids and the letters.
//   g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Icharon_amd/csrc tools/fuzz/fasta_split_fuzz.cpp -o /tmp/fasta_split_fuzz
//   /tmp/fasta_split_fuzz [cases] [seed]
// Cases: FASTA texts of 0 - 40 short records ('>' and ';' headers, ids now and then empty, sequences wrapped at 1 - 80 letters, line ends
// \n, \r\n or mixed, blanks / tabs / digits inside lines, blank lines) with 0 - 4 mutations at line level: a line feed, \r, '>' or ';'
// dropped, inserted or doubled, a line dropped or doubled, a blank line, a sequence line emptied, a truncation; a `start` at a record
// boundary or anywhere; a max_records at, below or above the count; the end-of-input flag on or off.  The text, every descriptor array,
// the id buffer and the letter buffer are allocated at exactly their sizes, so ASan watches their ends.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "charon_hip.h"
#include "parts/fasta_split.inc"

static uint64_t g_x = 1;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }

struct Rec { uint64_t id_off, seq_off; uint32_t id_len, seq_len; };

// the yardstick: parse_fasta from a record boundary on, over [p, end) of `buf` (compacted in place), `eof` as the reader's eof_.
// Returns the position behind the record, or null where the reader would wait for more text, skip blank lines or throw.
static char *parse_fasta(char *p, char *end, bool eof, const char *&id, uint32_t &id_len, const char *&seq, uint32_t &seq_len) {
    auto find_eol = [](const char *a, const char *b) { return static_cast<const char *>(std::memchr(a, '\n', (size_t)(b - a))); };
    if (p >= end) return nullptr;
    if (*p != '>' && *p != ';') return nullptr;  // (leading blank lines, which the reader skips, are the caller's business under the rule)
    const char *e0 = find_eol(p, end);
    if (!e0) { if (!eof) return nullptr; e0 = end; }
    char *q = (e0 < end) ? const_cast<char *>(e0) + 1 : end;
    char *rec_end = nullptr;
    for (char *l = q;;) {
        if (l >= end) { if (!eof) return nullptr; rec_end = end; break; }
        if (*l == '>' || *l == ';') { rec_end = l; break; }
        const char *e = find_eol(l, end);
        if (!e) { if (!eof) return nullptr; rec_end = end; break; }
        l = const_cast<char *>(e) + 1;
    }
    uint32_t idn = (uint32_t)(e0 - p - 1);
    if (idn && p[idn] == '\r') --idn;
    id = p + 1; id_len = idn;
    char *dst = q;
    for (char *c = q; c < rec_end;) {
        char *e = static_cast<char *>(std::memchr(c, '\n', (size_t)(rec_end - c)));
        if (!e) e = rec_end;
        const size_t len = (size_t)(e - c);
        bool clean = true;
        size_t i = 0;
        for (; i + 8 <= len; i += 8) {
            uint64_t x;
            std::memcpy(&x, c + i, 8);
            if (((x | (x << 1)) & 0x8080808080808080ULL) != 0x8080808080808080ULL) { clean = false; break; }
        }
        if (clean) for (; i < len; ++i) if ((unsigned char)c[i] < 0x40) { clean = false; break; }
        if (clean) {
            if (dst != c) std::memmove(dst, c, len);
            dst += len;
        } else {
            for (char *p2 = c; p2 < e; ++p2) {
                const char ch = *p2;
                if (ch == '\r' || ch == ' ' || ch == '\t' || (ch >= '0' && ch <= '9')) continue;
                if (dst != p2) *dst = ch;
                ++dst;
            }
        }
        c = e < rec_end ? e + 1 : rec_end;
    }
    seq = q; seq_len = (uint32_t)(dst - q);
    return rec_end;
}
static uint64_t parse(const std::string &t, uint64_t start, uint64_t end, uint64_t max_records, bool eof, std::vector<Rec> &out, std::string &ids, std::string &letters) {
    std::string buf(t, 0, (size_t)end);  // the reader compacts in place
    char *base = &buf[0], *p = base + start, *stop = base + end;
    if (buf.empty()) return start;
    while (out.size() < max_records) {
        const char *id = nullptr, *seq = nullptr;
        uint32_t id_len = 0, seq_len = 0;
        char *nx = parse_fasta(p, stop, eof, id, id_len, seq, seq_len);
        if (!nx || seq_len == 0) break;
        Rec r;
        r.id_off = (uint64_t)(id - base); r.id_len = id_len; r.seq_off = letters.size(); r.seq_len = seq_len;
        out.push_back(r);
        ids.append(t, r.id_off, r.id_len);  // (the id bytes are never moved)
        letters.append(seq, seq_len);
        p = nx;
    }
    return (uint64_t)(p - base);
}

static std::string letters_of(const char *alphabet, size_t n) {
    std::string s(n, 'A');
    const size_t k = std::strlen(alphabet);
    for (size_t i = 0; i < n; ++i) s[i] = alphabet[rnd() % k];
    return s;
}

int main(int argc, char **argv) {
    const long cases = argc > 1 ? std::atol(argv[1]) : 200000;
    g_x = (argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1) * 0x9E3779B97F4A7C15ULL + 1;
    long bad = 0, refused = 0;
    uint64_t taken = 0, stopped_early = 0, with_flag = 0;
    for (long c = 0; c < cases; ++c) {
        // lines, each with its line end
        std::vector<std::string> lines;
        std::vector<uint64_t> bounds(1, 0);
        const unsigned n_recs = (unsigned)(rnd() % 41), eol_mode = (unsigned)(rnd() % 3);
        auto eol = [&]() { return std::string(eol_mode == 1 || (eol_mode == 2 && rnd() % 2) ? "\r\n" : "\n"); };
        for (unsigned i = 0; i < n_recs; ++i) {
            const size_t first = lines.size();
            const size_t len = 1 + rnd() % (rnd() % 8 ? 60 : 600), width = 1 + rnd() % 80;
            lines.push_back(std::string(rnd() % 5 ? ">" : ";") + (rnd() % 6 ? letters_of("abc019 /:_>;", rnd() % 20) : std::string()) + eol());
            const std::string s = letters_of(rnd() % 4 ? "ACGTN" : "ACGTNacgtn*-RYKM", len);
            for (size_t a = 0; a < len; a += width) {
                std::string l = s.substr(a, width);
                if (rnd() % 6 == 0) l.insert(rnd() % (l.size() + 1), letters_of(" \t0123456789", 1 + rnd() % 4));
                if (rnd() % 20 == 0) lines.push_back(eol());  // a blank line inside the record
                lines.push_back(l + eol());
            }
            uint64_t b = bounds.back();
            for (size_t k = first; k < lines.size(); ++k) b += lines[k].size();
            bounds.push_back(b);
        }
        for (unsigned m = (unsigned)(rnd() % 5); m > 0 && !lines.empty(); --m) {
            const size_t i = rnd() % lines.size();
            std::string &l = lines[i];
            const char what = "\n\r>;"[rnd() % 4];
            switch (rnd() % 9) {
                case 0: { const size_t at = l.find(what); if (at != std::string::npos) l.erase(at, 1); break; }   // dropped
                case 1: l.insert(rnd() % (l.size() + 1), 1, what); break;                                          // inserted
                case 2: { const size_t at = l.find(what); if (at != std::string::npos) l.insert(at, 1, what); break; }  // doubled
                case 3: lines.erase(lines.begin() + (long)i); break;
                case 4: lines.insert(lines.begin() + (long)i, lines[i]); break;
                case 5: lines.insert(lines.begin() + (long)i, rnd() % 2 ? "\n" : "\r\n"); break;                   // a blank line
                case 6: l.insert(0, 1, what); break;
                case 7: if (l[0] != '>' && l[0] != ';') l = rnd() % 2 ? " 12\t" + eol() : eol(); break;            // a sequence line emptied
                default: lines.resize(i + 1); lines[i].resize(rnd() % (lines[i].size() + 1)); break;               // truncated
            }
        }
        std::string t;
        for (const std::string &l : lines) t += l;
        const uint64_t end = t.size();
        uint64_t start = 0;
        if (rnd() % 3 == 0) start = rnd() % 2 ? std::min<uint64_t>(bounds[rnd() % bounds.size()], end) : rnd() % (end + 1);
        uint64_t max_records = rnd() % 4 ? 1000 : rnd() % (n_recs + 2);
        const bool want_ids = rnd() % 4 != 0, eoi = rnd() % 2 != 0;
        with_flag += eoi;

        std::vector<Rec> want;
        std::string want_ids_bytes, want_letters;
        const uint64_t consumed = parse(t, start, end, max_records, eoi, want, want_ids_bytes, want_letters);
        uint64_t ids_capacity = want_ids_bytes.size();
        const bool too_small = want_ids && ids_capacity && rnd() % 16 == 0;
        if (too_small) --ids_capacity;
        const uint64_t seq_capacity = (end - start + 15) & ~(uint64_t)15;

        // the code under test, on buffers of exactly the sizes it may touch
        uint8_t *text = new uint8_t[end ? end : 1];
        if (end) std::memcpy(text, t.data(), end);
        const size_t m = (size_t)max_records;
        uint64_t *id_off = new uint64_t[m ? m : 1], *seq_off = new uint64_t[m ? m : 1];
        uint32_t *id_len = new uint32_t[m ? m : 1], *seq_len = new uint32_t[m ? m : 1];
        uint8_t *ids = new uint8_t[ids_capacity ? ids_capacity : 1];
        uint8_t *seq = new uint8_t[seq_capacity ? seq_capacity : 1];
        std::memset(seq, 0xA5, seq_capacity ? seq_capacity : 1);
        chn_fasta_split_job j;
        std::memset(&j, 0, sizeof j);
        j.struct_size = sizeof j; j.flags = eoi ? CHN_FASTA_SPLIT_END_OF_INPUT : 0;
        j.text = text; j.text_bytes = end; j.start = start; j.max_records = max_records;
        j.id_offset = id_off; j.id_length = id_len; j.seq_offset = seq_off; j.seq_length = seq_len;
        j.seq_text = seq_capacity ? seq : nullptr; j.seq_capacity = seq_capacity;
        j.ids = want_ids ? ids : nullptr; j.ids_capacity = ids_capacity;
        j.n_records = j.consumed = j.ids_bytes = j.seq_bytes = 0xDEAD;
        std::string why;
        const int rc = fsp_host_job(&j, why);
        bool ok;
        if (too_small) { ok = rc == CHN_E_CAPACITY && why.find(std::to_string(want_ids_bytes.size()) + " bytes") != std::string::npos; ++refused; }
        else {
            ok = rc == 0 && j.n_records == want.size() && j.consumed == consumed && j.ids_bytes == want_ids_bytes.size() && j.seq_bytes == want_letters.size();
            for (size_t i = 0; ok && i < want.size(); ++i)
                ok = id_off[i] == want[i].id_off && id_len[i] == want[i].id_len && seq_off[i] == want[i].seq_off && seq_len[i] == want[i].seq_len;
            if (ok && want_ids && !want_ids_bytes.empty()) ok = std::memcmp(ids, want_ids_bytes.data(), want_ids_bytes.size()) == 0;
            if (ok && !want_letters.empty()) ok = std::memcmp(seq, want_letters.data(), want_letters.size()) == 0;
            for (uint64_t i = want_letters.size(); ok && i < seq_capacity; ++i) ok = seq[i] == 0xA5;  // nothing behind the letters is written
            taken += want.size();
            stopped_early += want.size() < n_recs;
        }
        if (!ok && ++bad < 10) std::printf("case %ld: rc %d (%s), records %llu / %zu, consumed %llu / %llu, letters %llu / %zu, start %llu of %llu bytes, flag %d\n", c, rc,
                                           why.c_str(), (unsigned long long)j.n_records, want.size(), (unsigned long long)j.consumed, (unsigned long long)consumed,
                                           (unsigned long long)j.seq_bytes, want_letters.size(), (unsigned long long)start, (unsigned long long)end, (int)eoi);
        delete[] text; delete[] id_off; delete[] seq_off; delete[] id_len; delete[] seq_len; delete[] ids; delete[] seq;
    }
    std::printf("%ld cases (%llu with the end-of-input flag), %llu records taken, %llu cases stopped before their last record, %ld refused for ids_capacity, %ld disagreements\n",
                cases, (unsigned long long)with_flag, (unsigned long long)taken, (unsigned long long)stopped_early, refused, bad);
    return bad ? 1 : 0;
}
