// Fuzzer of the record rule of the extract files and of a chn_extract's piece-and-tail arithmetic (charon_amd/csrc/parts/extract_records.inc)
// on a CPU build under ASan / UBSan: xr_host_job, the body of chn_extract_records_host (the host policy of the source k_extract_records
// compiles), with the checks chn_extract_append_records makes on the same job before it queues anything; and xr_plan_append / xr_bound
// driving a model of the handle's buffer whose pieces go through dfl_member_host, the compressor of chn_deflate_run_host.
//   g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Icharon_amd/csrc tools/fuzz/extract_records_fuzz.cpp -o /tmp/extract_records_fuzz
//   /tmp/extract_records_fuzz [cases] [seed]
// Rule cases: random texts of 0 - 3000 bytes (any byte value; now and then letters only), 0 - 12 records whose id, sequence and quality
// string lie anywhere, at the text's start, end at its last byte, are empty or overlap; now and then one range that ends behind the text
// (by a byte, by far, with a sum that wraps) or a capacity one byte short.  Every record against a plain restatement written here (a
// 256-entry table built from the front end's letter classes).  The text, the arrays and the output are allocated at exactly their
// sizes, so ASan watches their ends; a refused job leaves the output untouched.
// Bookkeeping cases (one in 64, they compress): a file's text appended in 1 - 12 parts of 0 - 200 000 bytes to a model of the handle --
// the bytes behind the pending tail, every whole piece compressed in place, the tail moved to the front, xr_bound checked against
// what came out -- and `finish`; the members must equal the file's text cut at multiples of 65 280 and compressed piece by piece.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "charon_hip.h"
#include "parts/gzip_trees.inc"
#include "parts/inflate_members.inc"
#include "parts/deflate_members.inc"
#include "parts/extract_records.inc"

static uint64_t g_x = 1;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }

static uint8_t g_map[256];
static void make_map() {  // host/fastx_reader.inc's CodeTable through "ACGTN"[code & 7]; no letter: N
    std::memset(g_map, 'N', sizeof g_map);
    for (const char *c = "ACGT"; *c; ++c) { g_map[(unsigned char)*c] = (uint8_t)*c; g_map[(unsigned char)(*c + 32)] = (uint8_t)*c; }
    g_map[(unsigned char)'U'] = g_map[(unsigned char)'u'] = 'T';
}

static DflShared *g_sh;
static std::vector<uint32_t> g_tokens;
static std::vector<uint8_t> g_slot;
static void member(const uint8_t *p, uint32_t n, std::vector<uint8_t> &out) {
    uint32_t crc = 0;
    const uint32_t size = dfl_member_host(*g_sh, g_tokens.data(), p, n, DFL_F_BGZF, g_slot.data(), &crc);
    out.insert(out.end(), g_slot.begin(), g_slot.begin() + size);
}

static bool bookkeeping_case(long c) {
    const int parts = 1 + (int)(rnd() % 12);
    std::vector<uint8_t> file, got, buf;  // buf: the handle's buffer, `pending` bytes at its front
    uint64_t pending = 0;
    for (int p = 0; p <= parts; ++p) {
        const bool finish = p == parts;
        uint64_t n = 0;
        switch (rnd() % 6) {
            case 0: n = 0; break;
            case 1: n = rnd() % 300; break;
            case 2: n = XR_PIECE - pending + (rnd() % 3) - 1; break;  // the tail becomes 65 279, 0 or 1
            case 3: n = XR_PIECE * (1 + rnd() % 3) - pending; break;
            default: n = rnd() % 200001; break;
        }
        if (finish) n = 0;
        if (n > 3 * XR_PIECE + 70000) n = 0;
        const size_t before = got.size();
        const uint64_t bound = xr_bound(pending, n);
        if (finish) {
            if (pending) member(buf.data(), (uint32_t)pending, got);
            pending = 0;
        } else if (n) {
            const XrPlan plan = xr_plan_append(pending, n);
            buf.resize((size_t)(pending + n));
            for (uint64_t i = 0; i < n; ++i) { const uint8_t b = (uint8_t)("ACGT@+\nI#"[rnd() % 9]); buf[(size_t)(pending + i)] = b; file.push_back(b); }
            for (uint64_t k = 0; k < plan.pieces; ++k) member(buf.data() + k * XR_PIECE, (uint32_t)XR_PIECE, got);
            if (plan.pieces && plan.tail) std::memcpy(buf.data(), buf.data() + plan.pieces * XR_PIECE, (size_t)plan.tail);  // (memcpy: ASan reports an overlap)
            if (plan.pieces * XR_PIECE + plan.tail != pending + n || plan.tail >= XR_PIECE) { std::printf("case %ld: plan does not add up\n", c); return false; }
            pending = plan.tail;
        }
        if (got.size() - before > bound) { std::printf("case %ld: %zu bytes came out, xr_bound said %llu\n", c, got.size() - before, (unsigned long long)bound); return false; }
    }
    std::vector<uint8_t> want;
    for (size_t at = 0; at < file.size(); at += XR_PIECE) member(file.data() + at, (uint32_t)std::min<size_t>(XR_PIECE, file.size() - at), want);
    if (got != want) { std::printf("case %ld: the members differ from the file cut at multiples of the piece size (%zu bytes of text)\n", c, file.size()); return false; }
    return true;
}

int main(int argc, char **argv) {
    const long cases = argc > 1 ? std::atol(argv[1]) : 300000;
    g_x = (argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1) * 0x9E3779B97F4A7C15ULL + 1;
    make_map();
    g_sh = new DflShared;
    g_tokens.resize(DFL_MAX_IN); g_slot.resize(DFL_SLOT);
    long bad = 0, refused_range = 0, refused_capacity = 0, files = 0;
    uint64_t formed = 0;
    for (int w = 0; w < 256; ++w)  // the letter map, every byte at every place of a dword
        for (int k = 0; k < 4; ++k) {
            const uint32_t word = 0x61216121u ^ ((uint32_t)(w ^ 0x21 ^ (k & 1 ? 0x40 : 0)) << (8 * k));
            const uint32_t m = xr_map_word(word);
            for (int b = 0; b < 4; ++b) if ((uint8_t)(m >> (8 * b)) != g_map[(uint8_t)(word >> (8 * b))]) { ++bad; std::printf("xr_map_word(%08x) = %08x\n", word, m); }
        }
    for (long c = 0; c < cases; ++c) {
        if (c % 64 == 63) { ++files; if (!bookkeeping_case(c)) ++bad; continue; }
        const uint64_t end = rnd() % 8 ? rnd() % (rnd() % 4 ? 300 : 3001) : 0;
        const size_t n = (size_t)(rnd() % 13);
        uint8_t *text = new uint8_t[end ? end : 1];
        const bool letters = rnd() % 3 == 0;
        for (uint64_t i = 0; i < end; ++i) text[i] = letters ? (uint8_t)"ACGTUacgtuNRYSWKMBDHVnryswkmbdhv"[rnd() % 32] : (uint8_t)rnd();
        uint64_t *off[3];
        uint32_t *len[3];
        for (int m = 0; m < 3; ++m) { off[m] = new uint64_t[n ? n : 1]; len[m] = new uint32_t[n ? n : 1]; }
        for (size_t i = 0; i < n; ++i)
            for (int m = 0; m < 3; ++m) {
                uint64_t o = end ? rnd() % (end + 1) : 0;
                uint64_t l = rnd() % (end - o + 1);
                switch (rnd() % 8) {
                    case 0: o = 0; l = rnd() % (end + 1); break;
                    case 1: l = rnd() % (end + 1); o = end - l; break;  // ends at the last byte
                    case 2: l = 0; break;
                    case 3: l = std::min<uint64_t>(l, rnd() % 40); break;
                    case 4: if (m) { o = off[m - 1][i]; l = len[m - 1][i]; } break;  // the same bytes as the segment before
                    default: break;
                }
                off[m][i] = o; len[m][i] = (uint32_t)l;
            }
        long bad_rec = -1;
        if (n && rnd() % 10 == 0) {
            bad_rec = (long)(rnd() % n);
            const int m = (int)(rnd() % 3);
            switch (rnd() % 3) {
                case 0: off[m][bad_rec] = end - len[m][bad_rec] + 1; break;
                case 1: off[m][bad_rec] = end + 1 + rnd() % 1000; break;
                default: off[m][bad_rec] = ~(uint64_t)0 - rnd() % 4; len[m][bad_rec] = 5 + (uint32_t)(rnd() % 100); break;
            }
        }
        std::vector<uint8_t> want;
        for (size_t i = 0; i < n && bad_rec < 0; ++i) {  // the yardstick
            want.push_back('@');
            for (uint32_t b = 0; b < len[0][i]; ++b) want.push_back(text[off[0][i] + b]);
            want.push_back('\n');
            for (uint32_t b = 0; b < len[1][i]; ++b) want.push_back(g_map[text[off[1][i] + b]]);
            want.push_back('\n'); want.push_back('+'); want.push_back('\n');
            for (uint32_t b = 0; b < len[2][i]; ++b) want.push_back(text[off[2][i] + b]);
            want.push_back('\n');
        }
        uint64_t total = 0;
        for (size_t i = 0; i < n; ++i) total += (uint64_t)len[0][i] + len[1][i] + len[2][i] + 6;
        uint64_t capacity = total;
        const bool too_small = bad_rec < 0 && total && rnd() % 12 == 0;
        if (too_small) --capacity;
        else if (rnd() % 4 == 0) capacity += rnd() % 20;
        uint8_t *out = new uint8_t[capacity ? capacity : 1];
        std::memset(out, 0xA5, capacity ? capacity : 1);
        chn_extract_job j;
        std::memset(&j, 0, sizeof j);
        j.struct_size = sizeof j;
        j.text = text; j.text_bytes = end; j.n_records = n;
        j.id_offset = off[0]; j.id_length = len[0]; j.seq_offset = off[1]; j.seq_length = len[1]; j.qual_offset = off[2]; j.qual_length = len[2];
        uint64_t bytes = 0xDEAD;
        std::string why;
        const int rc = xr_host_job(&j, out, capacity, &bytes, why);
        bool ok;
        if (bad_rec >= 0) {
            ok = rc == CHN_E_INVALID && why.find("record " + std::to_string(bad_rec) + ":") != std::string::npos;
            ++refused_range;
        } else if (too_small) {
            ok = rc == CHN_E_CAPACITY && why.find("need " + std::to_string(total) + " bytes") != std::string::npos;
            ++refused_capacity;
        } else {
            ok = rc == 0 && bytes == total && want.size() == total && (total == 0 || std::memcmp(out, want.data(), total) == 0);
            for (uint64_t i = total; ok && i < capacity; ++i) ok = out[i] == 0xA5;
            formed += total;
        }
        if (rc != 0) { for (uint64_t i = 0; ok && i < capacity; ++i) ok = out[i] == 0xA5; ok = ok && bytes == 0xDEAD; }  // refused: nothing written
        if (!ok && ++bad < 10) std::printf("case %ld: rc %d (%s), %zu records of a text of %llu bytes, %llu / %llu bytes\n", c, rc, why.c_str(), n, (unsigned long long)end,
                                           (unsigned long long)bytes, (unsigned long long)total);
        delete[] text; delete[] out;
        for (int m = 0; m < 3; ++m) { delete[] off[m]; delete[] len[m]; }
    }
    delete g_sh;
    std::printf("%ld cases, %llu bytes of records formed, %ld refused for a range, %ld refused for capacity, %ld files through the piece-and-tail model, %ld disagreements\n",
                cases, (unsigned long long)formed, refused_range, refused_capacity, files, bad);
    return bad ? 1 : 0;
}
