// radix_plan.hpp -- the geometry of the device-resident minimiser set's sort and unique passes (parts/radix_sort.inc): keys per tile,
// tiles for n keys, the scratch a chn_hashset_unique call takes, and the largest n a set may hold.
// Header-only and free of HIP: included by the translation unit charon_hip.hip (before the kernels), by the host front end (which
// weighs a unique call's scratch against its budget before it asks for it) and by tools/radix_plan_check.cpp.
#ifndef CHN_RADIX_PLAN_HPP
#define CHN_RADIX_PLAN_HPP

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RADIX_HD __host__ __device__ __forceinline__
#else
#define RADIX_HD static inline
#endif

#define RADIX_BITS 8u                    // bits of a digit
#define RADIX_DIGITS 256u                // values of a digit
#define RADIX_PASSES 8u                  // digits of a 64-bit key
#define RADIX_THREADS 256u               // workgroup of every kernel of radix_sort.inc: one thread a digit, four wavefronts
#define RADIX_TILE_DEFAULT 4096u         // keys per tile (chn_hashset_cfg.tile_keys == 0)
#define RADIX_TILE_MAX 65536u            // the largest tile_keys
#define RADIX_MAX_TILES (1u << 22)       // one workgroup a tile: 2^22 * 256 threads stay below the 2^32 threads of one launch
#define RADIX_MAX_KEYS 0xFFFFFFFFULL     // a set holds fewer than 2^32 values: counters per tile and digit, and ranks, are 32 bits wide

// Is `tile` a legal tile_keys?  A wavefront owns tile / 4 consecutive keys and walks them 64 at a time.
RADIX_HD bool radix_tile_ok(uint32_t tile) { return tile >= RADIX_THREADS && tile <= RADIX_TILE_MAX && tile % RADIX_THREADS == 0; }

// The largest n at this tile: RADIX_MAX_KEYS at the default tile, less where a small tile (the test hook) would need too many workgroups.
RADIX_HD uint64_t radix_max_keys(uint32_t tile) {
    const uint64_t by_tiles = (uint64_t)tile * RADIX_MAX_TILES;
    return by_tiles < RADIX_MAX_KEYS ? by_tiles : RADIX_MAX_KEYS;
}
RADIX_HD bool radix_n_ok(uint64_t n, uint32_t tile) { return n <= radix_max_keys(tile); }

RADIX_HD uint64_t radix_tiles(uint64_t n, uint32_t tile) { return (n + tile - 1) / tile; }

// The scratch of one unique call over n keys, in the order it is laid out:
//   the second key buffer                      n * 8
//   counts[digit][tile], 32 bits each          256 * tiles * 4    (the unique pass's tile counts reuse the first `tiles + 1` of them)
//   the 8 * 256 digit histograms, 64 bits      16 384
//   the 256 digit bases of a pass, 64 bits     2 048
//   the distinct count, 64 bits                8
// The buffer the distinct values are compacted into is not scratch: it becomes the set's.
RADIX_HD uint64_t radix_counts_bytes(uint64_t n, uint32_t tile) {
    const uint64_t per_digit = radix_tiles(n, tile) * RADIX_DIGITS, unique = radix_tiles(n, tile) + 1;
    return (per_digit > unique ? per_digit : unique) * 4;
}
RADIX_HD uint64_t radix_hist_bytes() { return (uint64_t)RADIX_PASSES * RADIX_DIGITS * 8; }
RADIX_HD uint64_t radix_tail_bytes() { return radix_hist_bytes() + RADIX_DIGITS * 8 + 8; }
RADIX_HD uint64_t radix_scratch_bytes(uint64_t n, uint32_t tile) { return n < 2 ? 0 : n * 8 + radix_counts_bytes(n, tile) + radix_tail_bytes(); }

#endif  // CHN_RADIX_PLAN_HPP
