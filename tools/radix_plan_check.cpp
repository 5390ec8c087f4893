// Checks charon_amd/csrc/parts/radix_plan.hpp -- keys per tile, tiles for n keys, the scratch of a chn_hashset_unique call and the
// largest set -- against the figures worked out by hand below.  No GPU, no HIP:
//   g++ -std=c++14 -O1 -Wall -Icharon_amd/csrc/parts tools/radix_plan_check.cpp -o radix_plan_check && ./radix_plan_check
// Prints one line per n and "ok"; exits 1 at the first mismatch.  (tests/test_hashset_cpu.py builds and runs it.)
#include <cstdio>
#include <cstdlib>

#include "radix_plan.hpp"

static void fail(const char *what, unsigned long long a, unsigned long long b, unsigned long long c) {
    std::fprintf(stderr, "FAILED: %s (%llu, %llu, %llu)\n", what, a, b, c);
    std::exit(1);
}

// n keys at `tile`: so many tiles, so many bytes of scratch
static void expect(uint64_t n, uint32_t tile, uint64_t tiles, uint64_t scratch) {
    if (!radix_n_ok(n, tile)) fail("n is refused", n, tile, 0);
    if (radix_tiles(n, tile) != tiles) fail("tiles", n, radix_tiles(n, tile), tiles);
    if (radix_scratch_bytes(n, tile) != scratch) fail("scratch bytes", n, radix_scratch_bytes(n, tile), scratch);
    std::printf("n %llu tile %u: %llu tiles, %llu bytes of scratch\n", (unsigned long long)n, tile, (unsigned long long)tiles, (unsigned long long)scratch);
}

int main() {
    const uint32_t T = RADIX_TILE_DEFAULT;
    if (T != 4096 || RADIX_THREADS != 256 || RADIX_DIGITS != 256 || RADIX_PASSES * RADIX_BITS != 64) fail("the constants", T, RADIX_THREADS, RADIX_DIGITS);
    // 8 histograms of 256 64-bit counters, 256 64-bit digit bases, the distinct count
    const uint64_t tail = 8 * 256 * 8 + 256 * 8 + 8;
    if (tail != 18440 || radix_tail_bytes() != tail) fail("histograms, bases and the count", radix_tail_bytes(), tail, 0);
    // nothing to sort: no scratch at all
    expect(0, T, 0, 0);
    expect(1, T, 1, 0);
    // one tile: the second key buffer, 256 counters of 4 bytes, the tail
    expect(T - 1, T, 1, 4095ULL * 8 + 1024 + tail);
    expect(T, T, 1, 4096ULL * 8 + 1024 + tail);
    expect(T + 1, T, 2, 4097ULL * 8 + 2048 + tail);
    // the largest set: 2^32 - 1 keys in 2^20 tiles; 1 GiB of counters beside 32 GiB of keys
    expect(0xFFFFFFFFULL, T, 1ULL << 20, 0xFFFFFFFFULL * 8 + (1ULL << 30) + tail);
    if (radix_n_ok(1ULL << 32, T)) fail("2^32 keys are refused", 0, 0, 0);
    if (radix_max_keys(T) != 0xFFFFFFFFULL) fail("the largest set at the default tile", radix_max_keys(T), 0, 0);
    // the test hook's smallest tile: one workgroup a tile bounds the set at 2^22 tiles
    expect(256, 256, 1, 256ULL * 8 + 1024 + tail);
    expect(257, 256, 2, 257ULL * 8 + 2048 + tail);
    expect(1025ULL * 256 + 7, 256, 1026, (1025ULL * 256 + 7) * 8 + 1026 * 1024 + tail);
    if (radix_max_keys(256) != (1ULL << 30) || radix_n_ok((1ULL << 30) + 1, 256) || !radix_n_ok(1ULL << 30, 256)) fail("the largest set at tile 256", radix_max_keys(256), 0, 0);
    // tile_keys: multiples of 256 from 256 to 65 536
    const uint32_t good[] = {256, 512, 4096, 65536}, bad[] = {0, 1, 255, 257, 4097, 65536 + 256, 0xFFFFFF00u};
    for (uint32_t t : good) if (!radix_tile_ok(t)) fail("a legal tile is refused", t, 0, 0);
    for (uint32_t t : bad) if (radix_tile_ok(t)) fail("an illegal tile is accepted", t, 0, 0);
    // the counters never fall short of what the unique pass reuses them for (tiles + 1 words)
    for (uint64_t n = 2; n < 70000; n += 257)
        for (uint32_t t : good) if (radix_counts_bytes(n, t) < (radix_tiles(n, t) + 1) * 4) fail("room for the unique pass's tile counts", n, t, 0);
    std::printf("ok\n");
    return 0;
}
