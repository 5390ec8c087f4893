// Fuzzer of the Elias-Fano encode (charon_amd/csrc/parts/ef_encode.inc, abi_ef_encode.inc) on a CPU build under ASan / UBSan:
// chn_ef_layout_of and chn_index_encode_ef_host over random indexes, densities and slice sizes.  Runs on the CPU only.
//   g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Icharon_amd/csrc tools/fuzz/ef_encode_fuzz.cpp -o /tmp/ef_encode_fuzz
//   /tmp/ef_encode_fuzz [cases] [seed]
// Words and both arrays live in buffers of exactly their sizes (ASan watches both ends).  Every answer is compared with a serial encoder
// spelt out here (one set bit after the other into arrays of the layout's size, the layout computed with a loop for the logarithm), for a
// random slice size, for one row a slice and for one slice.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "charon_hip.h"
static std::string g_msg;
static int fail(int rc, const std::string &m) { g_msg = m; return rc; }
#include "parts/ef_encode.inc"
#include "parts/abi_ef_encode.inc"

static uint64_t g_x = 1;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }

static unsigned slow_hi(uint64_t x) { unsigned h = 0; while (x > 1) { x >>= 1; ++h; } return h; }

int main(int argc, char **argv) {
    const long cases = argc > 1 ? std::atol(argv[1]) : 2000;
    g_x = (argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1) * 0x9E3779B97F4A7C15ULL + 1;
    long bad = 0;
    uint64_t total_ones = 0;
    for (long c = 0; c < cases; ++c) {
        chn_index_desc d;
        std::memset(&d, 0, sizeof d);
        d.struct_size = sizeof d;
        d.bins = 1 + rnd() % 255; d.bin_words = (d.bins + 63) / 64; d.technical_bins = 64 * d.bin_words;
        d.bin_size = 1 + rnd() % (c % 7 == 0 ? 3000 : 200);
        const uint64_t n = d.bin_size * d.bin_words, m_size = n * 64;
        std::vector<uint64_t> words(n);
        const unsigned kind = (unsigned)(rnd() % 6);  // 0 empty | 1 full | 2 .. 5 thinner and thinner noise, with empty stretches
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t w = kind == 0 ? 0 : kind == 1 ? ~0ULL : rnd();
            for (unsigned t = 2; t < kind; ++t) w &= rnd();
            if (kind >= 2 && (i / 97) % 3 == 1) w = 0;
            words[i] = w;
        }
        uint64_t ones = 0;
        for (uint64_t w : words) ones += (uint64_t)__builtin_popcountll(w);
        total_ones += ones;
        // the serial encoder
        unsigned logm = slow_hi(ones) + 1;
        const unsigned logn = slow_hi(m_size) + 1;
        if (logm == logn) --logm;
        const unsigned wl = logn - logm;
        const uint64_t high_bits = ones + (1ULL << logm);
        std::vector<uint64_t> want_low((ones * wl + 63) / 64, 0), want_high((high_bits + 63) / 64, 0);
        uint64_t k = 0;
        for (uint64_t p = 0; p < m_size; ++p) {
            if (!((words[p >> 6] >> (p & 63)) & 1)) continue;
            for (unsigned b = 0; b < wl; ++b)
                if ((p >> b) & 1) { const uint64_t at = k * wl + b; want_low[at >> 6] |= 1ULL << (at & 63); }
            const uint64_t hp = (p >> wl) + k;
            want_high[hp >> 6] |= 1ULL << (hp & 63);
            ++k;
        }
        chn_ef_layout lay;
        if (chn_ef_layout_of(m_size, ones, &lay) != CHN_OK || lay.wl != wl || lay.high_bits != high_bits || lay.low_bits != ones * wl ||
            lay.n_low_words != want_low.size() || lay.n_high_words != want_high.size()) {
            std::printf("case %ld: layout of (%llu, %llu) differs\n", c, (unsigned long long)m_size, (unsigned long long)ones);
            ++bad;
            continue;
        }
        const uint64_t slices[3] = {1 + rnd() % (d.bin_size + 3), 1, 0};
        for (uint64_t slice_rows : slices) {
            std::vector<uint64_t> low(want_low.size(), ~0ULL), high(want_high.size(), ~0ULL);
            chn_ef_encode_job job;
            std::memset(&job, 0, sizeof job);
            job.struct_size = sizeof job; job.slice_rows = slice_rows; job.layout = &lay;
            job.low = low.empty() ? nullptr : low.data(); job.n_low_words = low.size(); job.high = high.data(); job.n_high_words = high.size();
            const int rc = chn_index_encode_ef_host(&d, words.data(), &job);
            if (rc != CHN_OK || job.ones_written != ones || low != want_low || high != want_high) {
                std::printf("case %ld (bins %llu, rows %llu, ones %llu, wl %u, slice %llu): rc %d %s\n", c, (unsigned long long)d.bins, (unsigned long long)d.bin_size,
                            (unsigned long long)ones, wl, (unsigned long long)slice_rows, rc, rc ? g_msg.c_str() : "arrays differ");
                ++bad;
            }
        }
    }
    std::printf("%ld cases, %llu set bits, %ld bad\n", cases, (unsigned long long)total_ones, bad);
    return bad ? 1 : 0;
}
