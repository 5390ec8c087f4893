// Fuzzer of the block-start search (charon_amd/csrc/parts/inflate_search.inc, abi_inflate_search.inc) on a CPU build under ASan / UBSan:
// chn_inflate_stream_search_host over noise, zlib streams (untouched and mutated) and truncations.  Runs on the CPU only.
//   g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Icharon_amd/csrc tools/fuzz/inflate_search_fuzz.cpp -lz -o /tmp/inflate_search_fuzz
//   /tmp/inflate_search_fuzz [cases] [seed]
// The input lives in a buffer of exactly its size (ASan watches both ends); ranges are random, unordered and overlapping, some empty, some
// one bit long, some to the last bit.  Every answer is compared with a brute-force walk: every position of the range in order, R0 spelt
// out here, infs_filter for that position's byte, infs_trial at the position -- the front end's find_block cannot be compiled in (it
// lives in a class that maps files and needs the library and OpenMP), tests/test_inflate_search_cpu.py compares with it through the CLI.
// Where a range begins on a sync-flush point of an untouched text stream whose next block is dynamic, the answer must be that point.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>
#include <zlib.h>

#include "charon_hip.h"
static int fail(int rc, const std::string &) { return rc; }
#include "parts/inflate_members.inc"
#include "parts/inflate_stream.inc"
#include "parts/inflate_search.inc"
#include "parts/abi_inflate_search.inc"

static uint64_t g_x = 1;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }

static uint64_t brute(InfShared &sh, const uint8_t *in, uint64_t n, uint64_t from, uint64_t to) {
    for (uint64_t p = from; p < to; ++p) {
        const uint64_t b = p >> 3;
        if (b + 8 > n || ((p + 17) >> 3) + 9 > n) continue;  // R0
        uint8_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (uint64_t i = 0; i < 12 && b + i < n; ++i) w[i] = in[b + i];
        uint64_t lo;
        uint32_t hi;
        std::memcpy(&lo, w, 8);
        std::memcpy(&hi, w + 8, 4);
        if (!((infs_filter(lo, hi, b, p, p + 1, n) >> (p & 7)) & 1u)) continue;
        InfChunkHostPolicy pol;
        pol.in = in + b; pol.len = n - b; pol.bit0 = (uint32_t)(p & 7);
        if (infs_trial(pol, sh)) return p;
    }
    return INFS_NONE;
}

int main(int argc, char **argv) {
    const long cases = argc > 1 ? std::atol(argv[1]) : 2000;
    g_x = (argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1) * 0x9E3779B97F4A7C15ULL + 1;
    long bad = 0, ranges = 0, found = 0, flush_hits = 0;
    InfShared *sh = new InfShared;
    for (long c = 0; c < cases; ++c) {
        const unsigned kind = (unsigned)(rnd() % 4);  // 0 noise | 1 .. 3 a zlib stream of text
        std::vector<uint8_t> m;
        std::vector<size_t> flushes;
        bool clean = true, dynamic_text = false;
        if (kind == 0) {
            m.resize(rnd() % 20000);
            for (uint8_t &b : m) b = (uint8_t)rnd();
        } else {
            const size_t n = 200 + rnd() % 60000;
            std::vector<uint8_t> text(n);
            for (size_t i = 0; i < n; ++i) text[i] = (i >= 150 && rnd() % 8) ? text[i - 150] : (uint8_t)"ACGT\nF:@+,#"[rnd() % 11];
            z_stream zs;
            std::memset(&zs, 0, sizeof zs);
            const int level = (int)(rnd() % 10), strategy = rnd() % 6 == 0 ? Z_FIXED : Z_DEFAULT_STRATEGY;
            const int mem = 1 + (int)(rnd() % 9);
            dynamic_text = level > 0 && strategy == Z_DEFAULT_STRATEGY && mem >= 8;  // (blocks of thousands of symbols: zlib writes them dynamic)
            deflateInit2(&zs, level, Z_DEFLATED, -15, mem, strategy);
            m.resize(deflateBound(&zs, (uLong)n) + 4096);
            zs.next_out = m.data(); zs.avail_out = (uInt)m.size();
            std::vector<size_t> steps;
            for (size_t left = n; left;) { steps.push_back(std::min<size_t>(left, 2000 + rnd() % 20000)); left -= steps.back(); }
            size_t at = 0;
            for (size_t k = 0; k < steps.size(); ++k) {
                zs.next_in = text.data() + at; zs.avail_in = (uInt)steps[k];
                at += steps[k];
                deflate(&zs, k + 1 < steps.size() ? Z_SYNC_FLUSH : Z_FINISH);
                if (k + 2 < steps.size() && steps[k + 1] >= 8000) flushes.push_back(m.size() - zs.avail_out);  // (a non-final piece of 8 000 bytes and more follows)
            }
            m.resize(m.size() - zs.avail_out);
            deflateEnd(&zs);
            for (unsigned k = (unsigned)(rnd() % 3) * (unsigned)(rnd() % 2); k > 0 && !m.empty(); --k) { m[rnd() % m.size()] ^= (uint8_t)(1 + rnd() % 255); clean = false; }
            if (rnd() % 8 == 0 && m.size() > 1) { m.resize(1 + rnd() % (m.size() - 1)); clean = false; }
        }
        const uint64_t n = m.size(), end = 8 * n;
        uint8_t *in = new uint8_t[n ? n : 1];
        if (n) std::memcpy(in, m.data(), n);
        std::vector<uint64_t> from, to;
        for (unsigned k = 1 + (unsigned)(rnd() % 6); k > 0; --k) {
            const uint64_t f = end ? rnd() % (end + 1) : 0;
            const unsigned how = (unsigned)(rnd() % 5);
            from.push_back(f);
            to.push_back(how == 0 ? f : how == 1 ? std::min(end, f + 1) : how == 2 ? end : std::min(end, f + 1 + rnd() % 30000));
        }
        const size_t own = from.size();
        if (clean && dynamic_text)
            for (size_t f : flushes) { from.push_back(8 * (uint64_t)f); to.push_back(std::min(end, 8 * (uint64_t)f + 1 + rnd() % 5000)); }
        std::vector<uint64_t> got(from.size(), 0xA5A5A5A5A5A5A5A5ull);
        chn_inflate_search_job j;
        std::memset(&j, 0, sizeof j);
        j.struct_size = sizeof j; j.n_ranges = from.size();
        j.in = n ? in : nullptr; j.in_bytes = n; j.from_bit = from.data(); j.to_bit = to.data(); j.found_bit = got.data();
        std::string what;
        if (chn_inflate_stream_search_host(&j) != CHN_OK) what = "the call failed";
        for (size_t k = 0; k < from.size() && what.empty(); ++k) {
            // the brute-force walk is slow on long ranges of streams that hold candidates only far in: cut what it looks at to 40 000 positions
            const uint64_t upto = got[k] != INFS_NONE ? std::min(to[k], got[k] + 1) : std::min(to[k], from[k] + 40000);
            const uint64_t want = brute(*sh, in, n, from[k], upto);
            if (got[k] != INFS_NONE && (got[k] < from[k] || got[k] >= to[k])) what = "a position outside its range";
            else if (want != (got[k] != INFS_NONE || upto == to[k] ? got[k] : INFS_NONE)) what = "differs from the brute-force walk";
            else if (k >= own && got[k] != from[k]) what = "a sync-flush point in front of a dynamic text block was not found";
            found += got[k] != INFS_NONE;
            flush_hits += k >= own;
        }
        ranges += (long)from.size();
        if (!what.empty() && ++bad < 10) std::printf("case %ld: %s (kind %u, %llu bytes, %zu ranges, clean %d)\n", c, what.c_str(), kind, (unsigned long long)n, from.size(), (int)clean);
        delete[] in;
    }
    delete sh;
    std::printf("%ld cases, %ld ranges, %ld with a position found, %ld of them sync-flush points asked for, %ld disagreements\n", cases, ranges, found, flush_hits, bad);
    return bad ? 1 : 0;
}
