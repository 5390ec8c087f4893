// Fuzzer of the byte-range copy rule (charon_amd/csrc/parts/text_gather.inc) on a CPU build under ASan / UBSan: txg_host_job, the
// body of chn_text_fetch_host, with the checks (txg_check_job) that chn_text_fetch makes on the same job before it queues anything.
// Every case is compared with a plain byte loop written here.
//   g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Icharon_amd/csrc tools/fuzz/text_fetch_fuzz.cpp -o /tmp/text_fetch_fuzz
//   /tmp/text_fetch_fuzz [cases] [seed]
// Cases: random texts of 0 - 5000 bytes and 0 - 40 ranges: anywhere, at the text's start, ending at its last byte, empty, repeated,
// overlapping the one before; now and then one range that ends behind the text (by one byte, by far, with an offset whose sum with
// the length wraps) or an out_capacity one byte short.  The text, the range arrays and `out` are allocated at exactly their sizes, so
// ASan watches their ends; a refused job must leave `out` untouched.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "charon_hip.h"
#include "parts/text_gather.inc"

static uint64_t g_x = 1;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }

int main(int argc, char **argv) {
    const long cases = argc > 1 ? std::atol(argv[1]) : 200000;
    g_x = (argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1) * 0x9E3779B97F4A7C15ULL + 1;
    long bad = 0, refused_range = 0, refused_capacity = 0;
    uint64_t moved = 0;
    for (long c = 0; c < cases; ++c) {
        const uint64_t end = rnd() % 8 ? rnd() % (rnd() % 4 ? 200 : 5001) : 0;
        const size_t n = (size_t)(rnd() % 41);
        uint8_t *text = new uint8_t[end ? end : 1];
        for (uint64_t i = 0; i < end; ++i) text[i] = (uint8_t)rnd();
        uint64_t *off = new uint64_t[n ? n : 1];
        uint32_t *len = new uint32_t[n ? n : 1];
        for (size_t i = 0; i < n; ++i) {
            uint64_t o = end ? rnd() % (end + 1) : 0;
            uint64_t l = rnd() % (end - o + 1);
            switch (rnd() % 8) {
                case 0: o = 0; l = rnd() % (end + 1); break;
                case 1: l = rnd() % (end + 1); o = end - l; break;       // ends at the last byte
                case 2: l = 0; break;
                case 3: if (i) { o = off[i - 1]; l = len[i - 1]; } break;  // repeated
                case 4: if (i && len[i - 1]) { o = off[i - 1] + rnd() % len[i - 1]; l = rnd() % (end - o + 1); } break;  // overlapping
                default: break;
            }
            off[i] = o; len[i] = (uint32_t)l;
        }
        long bad_range = -1;
        if (n && rnd() % 10 == 0) {
            bad_range = (long)(rnd() % n);
            switch (rnd() % 3) {
                case 0: off[bad_range] = end - len[bad_range] + 1; break;                                // one byte too far
                case 1: off[bad_range] = end + 1 + rnd() % 1000; break;                                  // offset behind the text
                default: off[bad_range] = ~(uint64_t)0 - rnd() % 4; len[bad_range] = 5 + (uint32_t)(rnd() % 100); break;  // the sum wraps
            }
            for (long i = 0; i < bad_range; ++i)  // (the first bad range is the one the message names)
                if (off[i] > end || len[i] > end - off[i]) { bad_range = i; break; }
        }
        uint64_t total = 0;
        for (size_t i = 0; i < n; ++i) total += len[i];
        uint64_t capacity = total;
        const bool too_small = bad_range < 0 && total && rnd() % 12 == 0;
        if (too_small) --capacity;
        else if (rnd() % 4 == 0) capacity += rnd() % 20;

        std::vector<uint8_t> want;
        if (bad_range < 0 && !too_small)
            for (size_t i = 0; i < n; ++i)
                for (uint32_t b = 0; b < len[i]; ++b) want.push_back(text[off[i] + b]);  // the yardstick

        uint8_t *out = new uint8_t[capacity ? capacity : 1];
        std::memset(out, 0xA5, capacity ? capacity : 1);
        chn_text_fetch_job j;
        std::memset(&j, 0, sizeof j);
        j.struct_size = sizeof j;
        j.text = text; j.text_bytes = end; j.n_ranges = n; j.offset = off; j.length = len; j.out = out; j.out_capacity = capacity;
        j.out_bytes = 0xDEAD;
        std::string why;
        const int rc = txg_host_job(&j, why);
        bool ok;
        if (bad_range >= 0) {
            ok = rc == CHN_E_INVALID && why.find("range " + std::to_string(bad_range) + " ") != std::string::npos;
            ++refused_range;
        } else if (too_small) {
            ok = rc == CHN_E_CAPACITY && why.find("need " + std::to_string(total) + " bytes") != std::string::npos;
            ++refused_capacity;
        } else {
            ok = rc == 0 && j.out_bytes == total && (total == 0 || std::memcmp(out, want.data(), total) == 0);
            for (uint64_t i = total; ok && i < capacity; ++i) ok = out[i] == 0xA5;
            moved += total;
        }
        if (rc != 0) for (uint64_t i = 0; ok && i < capacity; ++i) ok = out[i] == 0xA5;  // refused: nothing written
        if (!ok && ++bad < 10) std::printf("case %ld: rc %d (%s), %zu ranges of a text of %llu bytes, out_bytes %llu / %llu\n", c, rc, why.c_str(), n,
                                           (unsigned long long)end, (unsigned long long)j.out_bytes, (unsigned long long)total);
        delete[] text; delete[] off; delete[] len; delete[] out;
    }
    std::printf("%ld cases, %llu bytes moved, %ld refused for a range, %ld refused for out_capacity, %ld disagreements\n", cases, (unsigned long long)moved,
                refused_range, refused_capacity, bad);
    return bad ? 1 : 0;
}
