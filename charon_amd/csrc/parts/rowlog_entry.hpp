// rowlog_entry.hpp -- the compact row-log entry: how k_minimise_probe writes a probed row (the AND of a minimiser's h rows) and how
// k_count_wavelog reads it back.  The rule is written once, here.
// Header-only and free of HIP: included by the translation unit charon_hip.hip (before the kernels) and by tools/rowlog_entry_check.cpp.
//
// An entry is 32 bits: bits 0-1 the number of set bins it names (0..3), bits 2-9 / 10-17 / 18-25 their indices in ascending order,
// bits 26-31 the owner lane.  A row without a set bin gets no entry.  A row with more set bins than the entries can name ESCAPES:
// count = 0 with a non-zero 24-bit field (bits 2-25) = 1 + index of its W full words in the wavefront's escaped-row region.
//
// Chain mode (B <= 128, so that a bin index needs 7 bits and the top bit of each 8-bit bin field is free): a row with 4..6 set bins
// becomes TWO consecutive entries of the same owner -- three bins, then the other one to three, still in ascending order.  Bit 9 (the top
// bit of the first bin field) of the first says "this row continues in the next entry", bit 17 (of the second bin field) of the second
// says "this entry continues the previous one".  Both flags are read only where the count is non-zero (in an escaped entry the bits belong
// to the index); a row with seven or more set bins still escapes.  Without chain mode the encoding is what it was before there were chains.
#ifndef CHN_ROWLOG_ENTRY_HPP
#define CHN_ROWLOG_ENTRY_HPP

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ROWLOG_HD __host__ __device__ __forceinline__
#else
#define ROWLOG_HD static inline
#endif

#define ROWLOG_ESC_MASK 0x03fffffcu
#define ROWLOG_ESC_MAX 0x00fffffeu       // largest escaped-row index one entry can name
#define ROWLOG_CHAIN_NEXT (1u << 9)      // chain mode: the row continues in the next entry
#define ROWLOG_CHAIN_PREV (1u << 17)     // chain mode: this entry continues the previous one
#define ROWLOG_CHAIN_MAX_BINS 128u       // chain mode needs the top bit of the bin fields

ROWLOG_HD bool rowlog_chain_ok(uint32_t B) { return B <= ROWLOG_CHAIN_MAX_BINS; }
ROWLOG_HD uint32_t rowlog_bin_mask(bool chain) { return chain ? 0x7fu : 0xffu; }

// Encode the row acc[0..W) of `owner`.  Returns the number of entries (0: no set bin; 1; 2: a chain) and writes them to e[0], e[1].
// escaped: the one entry lacks the escape index -- the caller stores the full row and adds (index + 1) << 2.
template <int W>
ROWLOG_HD uint32_t rowlog_encode(const uint64_t *acc, uint32_t B, uint32_t owner, bool chain, uint32_t e[2], bool &escaped) {
    uint64_t m[W];
    uint32_t pc = 0;
    for (int w = 0; w < W; ++w) {
        m[w] = acc[w];
        if (w == W - 1 && (B & 63u)) m[w] &= (1ULL << (B & 63u)) - 1;  // technical bins >= B never count
        pc += (uint32_t)__builtin_popcountll(m[w]);
    }
    e[0] = e[1] = owner << 26;
    escaped = pc > (chain ? 6u : 3u);
    if (escaped) return 1;
    if (pc == 0) return 0;
    const uint32_t n = pc > 3 ? 2u : 1u;
    e[0] |= pc > 3 ? 3u | ROWLOG_CHAIN_NEXT : pc;
    if (n == 2) e[1] |= (pc - 3) | ROWLOG_CHAIN_PREV;
    uint32_t slot = 0;
    for (int w = 0; w < W; ++w) {
        uint64_t x = m[w];
        while (x) {
            const uint32_t b = (uint32_t)w * 64 + (uint32_t)__builtin_ctzll(x);
            x &= x - 1;
            if (slot < 3) e[0] |= b << (2 + 8 * slot); else e[1] |= b << (2 + 8 * (slot - 3));
            ++slot;
        }
    }
    return n;
}

// ---- the walk (k_count_wavelog) ----
// number of bins entry x names (0: an escaped row if x & ROWLOG_ESC_MASK, else nothing) and bin j < that number
ROWLOG_HD uint32_t rowlog_count(uint32_t x) { return x & 3u; }
ROWLOG_HD uint32_t rowlog_bin(uint32_t x, uint32_t j, bool chain) { return (x >> (2 + 8 * j)) & rowlog_bin_mask(chain); }
// Pass A (per-bin totals) takes every entry on its own: bump rowlog_bin(x, j) for j < rowlog_count(x).
// Pass B (one decision per ROW): the second entry of a chain is skipped, the first is judged together with its successor.
ROWLOG_HD bool rowlog_is_tail(uint32_t x, bool chain) { return chain && (x & 3u) != 0 && (x & ROWLOG_CHAIN_PREV) != 0; }
ROWLOG_HD bool rowlog_has_tail(uint32_t x, bool chain) { return chain && (x & 3u) != 0 && (x & ROWLOG_CHAIN_NEXT) != 0; }
// Entry e of a log of `count` entries, x = log[e] with rowlog_has_tail(x): the successor to judge with it, or 0 (names nothing) if the log
// ends here or the next entry is no tail -- nothing at or beyond `count` is read.
template <class Log>
ROWLOG_HD uint32_t rowlog_tail(const Log &log, uint32_t e, uint32_t count, bool chain) {
    if (e + 1 >= count) return 0;
    const uint32_t y = log[e + 1];
    return rowlog_is_tail(y, chain) ? y : 0u;
}
// how many of the bins x names are chosen (chosen(b) -> bool); fbin: the last such bin
template <class Chosen>
ROWLOG_HD uint32_t rowlog_match(uint32_t x, bool chain, const Chosen &chosen, uint32_t &fbin) {
    uint32_t found = 0;
    const uint32_t pc = rowlog_count(x);
    for (uint32_t j = 0; j < pc; ++j) {
        const uint32_t b = rowlog_bin(x, j, chain);
        if (chosen(b)) { ++found; fbin = b; }
    }
    return found;
}

#endif  // CHN_ROWLOG_ENTRY_HPP
