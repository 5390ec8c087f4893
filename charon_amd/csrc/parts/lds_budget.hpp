// lds_budget.hpp -- host arithmetic of the LDS that k_minimise_probe and k_count_wavelog take: the ring-packing rule, the probe kernel's
// LDS size, the count kernel's table size and the budget it is given beside the probe wavefronts of a CU.
// Header-only and free of HIP: included by the translation unit charon_hip.hip (before the kernels) and by tools/lds_budget_check.cpp.
#ifndef CHN_LDS_BUDGET_HPP
#define CHN_LDS_BUDGET_HPP

#include <cstddef>
#include <cstdint>

#ifndef WAVE
#define WAVE 64
#endif
#ifndef QCAP
#define QCAP 128
#endif
#ifndef CHN_LOG_BATCH
#define CHN_LOG_BATCH 4
#endif
#ifndef K1_COND_MAX_BINS
#define K1_COND_MAX_BINS 4u
#endif
#ifndef FUSED_ROUNDS
#define FUSED_ROUNDS 2u
#endif

enum { MODE_FUSED = 0, MODE_ROWS = 1, MODE_EMPLACE = 2, MODE_LIST = 3 };

static inline uint32_t bits_u64(uint64_t x) { uint32_t n = 0; while (x) { ++n; x >>= 1; } return n; }
static inline uint64_t pow5_u64(uint32_t e) { uint64_t p = 1; while (e--) p *= 5; return p; }

// ---- ring words that carry their own offset ----------------------------------------------------------------------------------------
// A slot of the probe kernel's window ring holds (v << pb) | (wn - 1 - u): v the canonical value, u the slot's offset in its block,
// pb = bits(wn - 1).  The kernel XORs the k-mer ranks (below 5^k) with the index's 64-bit seed, so every bit of v above
// bits(5^k - 1) is a constant of the launch: shifting pb of them out loses nothing as long as the bits that do vary stay, and the
// order of two words is the order of (v, complemented offset).  The rule also holds for a seed that was shifted down to 2k bits
// beforehand (seqan3's adjust_seed), hence the second term.  k in 1..27, wn >= 1.
static inline uint32_t ring_offset_bits(uint32_t wn) { return bits_u64((uint64_t)wn - 1); }
static inline uint32_t ring_value_bits(uint32_t k, uint64_t seed) {
    const uint64_t a = pow5_u64(k) - 1, b = seed >> (64 - 2 * k);
    return bits_u64(a > b ? a : b);
}
static inline bool ring_pack_ok(uint32_t k, uint32_t wn, uint64_t seed) { return ring_value_bits(k, seed) + ring_offset_bits(wn) <= 64; }

// conditional probing (k1_minimise_probe.inc): MODE_FUSED indexes of few bins
static inline bool k1_cond(int mode, uint32_t B) { return mode == MODE_FUSED && B <= K1_COND_MAX_BINS; }

// dynamic LDS of one probe wavefront.  pack: the ring words carry their offsets (ring_pack_ok), there is no [wn][64] byte plane of offsets
static inline size_t k1_lds_bytes(uint32_t wn, uint32_t C, int mode, uint32_t h, uint32_t W, uint32_t B, bool pack) {
    const bool cond = k1_cond(mode, B);  // conditional probing: one row per round, a longer queue with the ANDs so far
    const size_t qc = cond ? QCAP + WAVE : QCAP;
    size_t b = (size_t)wn * WAVE * 8 + qc * 8 + qc * 4 + (cond ? qc * 8 : 0) + (mode == MODE_EMPLACE ? WAVE * 8 : 0) + (pack ? 0 : (size_t)wn * WAVE);
    if (mode == MODE_FUSED) b += (size_t)2 * C * WAVE * 4;
    if (cond) b += (size_t)FUSED_ROUNDS * 1024;
    else if (mode == MODE_FUSED || mode == MODE_ROWS) b += (size_t)2 * h * (W <= 2 ? 1 : 2) * 1024;  // probe buffer: two rounds of h x NBLK x 1 KiB
    b = (b + 15) & ~(size_t)15;
    if (mode == MODE_ROWS) b += (size_t)(CHN_LOG_BATCH + 1) * WAVE * 4;  // staged row-log entries (+ the at most 64 behind a full store)
    return b;
}

// dynamic LDS of one k_count_wavelog workgroup that counts G owners per sweep
static inline size_t k2_lds_bytes(uint32_t B, uint32_t C, uint32_t W, uint32_t G, bool t16) {
    const size_t tb = t16 ? (B + 1) / 2 : B;
    return (size_t)G * tb * 4 + ((size_t)G * C + ((G * C) & 1u)) * 4 + (size_t)G * W * 8 + (size_t)G * C + 16;
}

// ---- what the probe wavefronts of a CU leave for a count workgroup -------------------------------------------------------------------
#define CU_LDS_BYTES 163840u     // 160 KB per CU (gfx950)
#define LDS_GRANULE 256u         // unit a workgroup's LDS is rounded up to in this estimate
#define K2_LDS_STATIC 256u       // k_count_wavelog's static LDS (s_b2c)
#define K2_LDS_MARGIN 1024u      // the count workgroup's static 256 B, the rounding of its own allocation to the granule, and as much again in hand
#define K2_LDS_BUDGET_MIN 7680u  // never below the figure the kernel was sized with before the budget was derived (32 owners of 100 bins)
// The count kernel is to run UNDER the next batch's probe kernel: its tables get what floor(160 KB / probe LDS) probe wavefronts of the
// stream's probe configuration leave of the CU, less the margin.  (With more LDS than that it still runs, but only where a CU is short
// of a probe wavefront.)  At the default k = 19, w = 41, W <= 2: 20 736 B per packed probe wavefront, seven per CU, 18 688 B left,
// budget 17 664 B -- 64 owners of 100 bins with 16-bit totals take 14 480 B (of 128 bins 18 064 B: 32 owners).  Without packing:
// 22 208 B, 8 384 B left, the floor holds.
static inline size_t k2_lds_budget(size_t probe_lds) {
#ifdef K2_LDS_BUDGET  // diagnostics builds (tools/build_diag.sh k2big): a fixed budget
    (void)probe_lds;
    return K2_LDS_BUDGET;
#else
    size_t p = (probe_lds + LDS_GRANULE - 1) / LDS_GRANULE * LDS_GRANULE;
    if (p == 0 || p > CU_LDS_BYTES) return K2_LDS_BUDGET_MIN;
    const size_t left = CU_LDS_BYTES - CU_LDS_BYTES / p * p;
    const size_t b = left > K2_LDS_MARGIN ? left - K2_LDS_MARGIN : 0;
    return b > K2_LDS_BUDGET_MIN ? b : K2_LDS_BUDGET_MIN;
#endif
}
// owners per sweep: as many (64, 32, 16, 8) as keep the tables within the budget
static inline uint32_t k2_group(uint32_t B, uint32_t C, uint32_t W, bool t16, size_t budget) {
    uint32_t G = WAVE;
    while (G > 8 && k2_lds_bytes(B, C, W, G, t16) > budget) G >>= 1;
    return G;
}

#endif  // CHN_LDS_BUDGET_HPP
