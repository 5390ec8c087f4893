// Fuzzer of the pair-id rule (charon_amd/csrc/parts/text_pair.inc) on a CPU build under ASan / UBSan: tpi_host_job, the body of
// chn_text_pair_ids_host, with the checks (tpi_check_job) that chn_text_pair_ids makes on the same job before it queues anything.
// Every case is compared with a byte-wise restatement of the rule written here.
//   g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Icharon_amd/csrc tools/fuzz/text_pair_fuzz.cpp -o /tmp/text_pair_fuzz
//   /tmp/text_pair_fuzz [cases] [seed]
// Cases: two random texts of 0 - 3000 bytes over a small alphabet (so that equal stretches are common) and 0 - 60 pairs.  The id of
// mate 1 lies anywhere, at the text's start or ends at its last byte, with a length of 0 - 90 bytes, now and then up to 1200; the id
// of mate 2 is a copy written into text 2 at an offset of its own (any alignment) -- as it stands, with another last byte, with one
// compared byte changed (the first, the last, any), a byte longer or shorter -- or an unrelated stretch.  Now and then one id ends
// behind its text (by one byte, by far, with an offset whose sum with the length wraps).  The texts and the id arrays are allocated
// at exactly their sizes, so ASan watches their ends.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "charon_hip.h"
#include "parts/text_pair.inc"

static uint64_t g_x = 1;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }

// the yardstick: both ids lose their last byte, what is left must be equal
static bool agree(const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb) {
    if (la) --la;
    if (lb) --lb;
    if (la != lb) return false;
    for (uint32_t i = 0; i < la; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

int main(int argc, char **argv) {
    const long cases = argc > 1 ? std::atol(argv[1]) : 200000;
    g_x = (argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1) * 0x9E3779B97F4A7C15ULL + 1;
    long bad = 0, refused = 0, with_mismatch = 0;
    uint64_t pairs = 0, agreeing = 0;
    for (long c = 0; c < cases; ++c) {
        const uint64_t end1 = rnd() % 8 ? rnd() % (rnd() % 4 ? 300 : 3001) : 0, end2 = rnd() % 8 ? rnd() % (rnd() % 4 ? 300 : 3001) : 0;
        const size_t n = (size_t)(rnd() % 61);
        uint8_t *t1 = new uint8_t[end1 ? end1 : 1], *t2 = new uint8_t[end2 ? end2 : 1];
        const unsigned letters = rnd() % 3 ? 2 : 200;
        for (uint64_t i = 0; i < end1; ++i) t1[i] = (uint8_t)('A' + rnd() % letters);
        for (uint64_t i = 0; i < end2; ++i) t2[i] = (uint8_t)('A' + rnd() % letters);
        uint64_t *o1 = new uint64_t[n ? n : 1], *o2 = new uint64_t[n ? n : 1];
        uint32_t *l1 = new uint32_t[n ? n : 1], *l2 = new uint32_t[n ? n : 1];
        for (size_t i = 0; i < n; ++i) {
            uint64_t a = end1 ? rnd() % (end1 + 1) : 0;
            uint64_t la = std::min<uint64_t>(end1 - a, rnd() % 20 ? rnd() % 91 : rnd() % 1201);
            switch (rnd() % 6) {
                case 0: a = 0; la = std::min<uint64_t>(end1, la); break;
                case 1: la = std::min<uint64_t>(end1, la); a = end1 - la; break;  // ends at the last byte
                default: break;
            }
            // mate 2: a copy of mate 1's id somewhere in text 2 (later pairs may overwrite it: the yardstick reads what is there in the end)
            uint64_t lb = la;
            const unsigned kind = (unsigned)(rnd() % 9);
            if (kind == 4) ++lb;
            if (kind == 5 && lb) --lb;
            lb = std::min<uint64_t>(lb, end2);
            uint64_t b = end2 - lb ? rnd() % (end2 - lb + 1) : 0;
            if (rnd() % 6 == 0) b = end2 - lb;  // ends at the last byte
            if (kind != 8) {
                for (uint64_t k = 0; k < std::min(la, lb); ++k) t2[b + k] = t1[a + k];
                if (kind == 1 && lb) t2[b + lb - 1] ^= 1;                      // another last byte: agrees
                if (kind == 2 && lb >= 2) t2[b] ^= 1;                          // the first byte
                if (kind == 3 && lb >= 2) t2[b + lb - 2] ^= 1;                 // the last compared byte
                if (kind == 6 && lb >= 2) t2[b + rnd() % (lb - 1)] ^= 2;       // any compared byte
            }
            o1[i] = a; l1[i] = (uint32_t)la; o2[i] = b; l2[i] = (uint32_t)lb;
        }
        long bad_pair = -1;
        int bad_file = 0;
        if (n && rnd() % 10 == 0) {
            bad_pair = (long)(rnd() % n);
            bad_file = (int)(rnd() % 2);
            uint64_t *o = bad_file ? o2 : o1;
            uint32_t *l = bad_file ? l2 : l1;
            const uint64_t end = bad_file ? end2 : end1;
            switch (rnd() % 3) {
                case 0: o[bad_pair] = end - l[bad_pair] + 1; break;                                  // one byte too far
                case 1: o[bad_pair] = end + 1 + rnd() % 1000; break;                                 // offset behind the text
                default: o[bad_pair] = ~(uint64_t)0 - rnd() % 4; l[bad_pair] = 5 + (uint32_t)(rnd() % 100); break;  // the sum wraps
            }
        }
        uint64_t want = n;
        if (bad_pair < 0) {
            for (size_t i = 0; i < n; ++i)
                if (!agree(t1 + o1[i], l1[i], t2 + o2[i], l2[i])) { want = i; break; }
            pairs += n; agreeing += want;
            if (want < n) ++with_mismatch;
        }
        chn_text_pair_job j;
        std::memset(&j, 0, sizeof j);
        j.struct_size = sizeof j;
        j.text1 = t1; j.text1_bytes = end1; j.text2 = t2; j.text2_bytes = end2; j.n_pairs = n;
        j.id1_offset = o1; j.id1_length = l1; j.id2_offset = o2; j.id2_length = l2;
        j.first_mismatch = 0xDEAD;
        std::string why;
        const int rc = tpi_host_job(&j, why);
        bool ok;
        if (bad_pair >= 0) {
            ok = rc == CHN_E_INVALID && why.find("id " + std::to_string(bad_file + 1) + " of pair " + std::to_string(bad_pair) + " ") != std::string::npos &&
                 j.first_mismatch == 0xDEAD;
            ++refused;
        } else {
            ok = rc == 0 && j.first_mismatch == want;
        }
        if (!ok && ++bad < 10)
            std::printf("case %ld: rc %d (%s), %zu pairs, texts of %llu and %llu bytes, first_mismatch %llu, expected %llu\n", c, rc, why.c_str(), n,
                        (unsigned long long)end1, (unsigned long long)end2, (unsigned long long)j.first_mismatch, (unsigned long long)want);
        delete[] t1; delete[] t2; delete[] o1; delete[] o2; delete[] l1; delete[] l2;
    }
    std::printf("%ld cases, %llu pairs (%llu agreeing in front of the first mismatch), %ld cases with a mismatch, %ld refused for a range, %ld disagreements\n", cases,
                (unsigned long long)pairs, (unsigned long long)agreeing, with_mismatch, refused, bad);
    return bad ? 1 : 0;
}
