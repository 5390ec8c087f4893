// ef_encode.inc -- Elias-Fano (sd_vector) encode for the index writer: the layout rule, a set bit's place in m_low / m_high, the slice
// ranges, and the kernel k_ef_encode
// Part of the single translation unit charon_hip.hip (included in order, behind ef_decode.inc); not a stand-alone source.
// Builds for the CPU alone as well (tools/fuzz/ef_encode_fuzz.cpp): everything but the kernel is __host__ __device__.
//
// The layout is sdsl's sd_vector (SURVEY A.5; the front end's EliasFanoWriter::begin states it too, oracle/pyref.py: ef_encode is the
// independent restatement the tests compare with).  The set bit of rank k (counted from 0 over the whole vector) at plain position pos puts
// its low wl bits at bit k * wl of m_low and sets bit (pos >> wl) + k of m_high: its place depends on nothing but pos and k, so any piece
// of the plain vector is encoded on its own once the number of set bits in front of it is known.

#ifndef __HIPCC__  // a CPU build of the rule and of chn_index_encode_ef_host
#define __host__
#define __device__
#endif

struct EfLayoutRule {
    uint32_t wl;
    uint64_t low_bits, high_bits, n_low_words, n_high_words;
};
__host__ __device__ static inline uint32_t ef_hi(uint64_t x) { return x ? 63u - (uint32_t)__builtin_clzll(x) : 0u; }  // floor(log2 x), hi(0) = 0
// 1 <= ones_max is not asked for: ones == 0 gives logm = 1, no low words, two high bits.  The caller keeps m_size below 2^57 (ones * wl fits).
__host__ __device__ static inline EfLayoutRule ef_layout_rule(uint64_t m_size, uint64_t ones) {
    uint32_t logm = ef_hi(ones) + 1;
    const uint32_t logn = ef_hi(m_size) + 1;
    if (logm == logn) --logm;
    EfLayoutRule r;
    r.wl = logn - logm;
    r.low_bits = ones * r.wl;
    r.high_bits = ones + (1ULL << logm);
    r.n_low_words = (r.low_bits + 63) / 64;
    r.n_high_words = (r.high_bits + 63) / 64;
    return r;
}

// The words of m_low and m_high that the set bits of plain positions [pos_begin, pos_end) can touch, given that `before` set bits precede
// them and they hold `ones` > 0 set bits: ranks before .. before + ones - 1; the first possible high bit belongs to (pos_begin, before), the
// last to (pos_end - 1, before + ones - 1).  Neighbouring pieces share at most the word at each seam.
struct EfRange {
    uint64_t low_w0, n_low, high_w0, n_high;
};
__host__ __device__ static inline EfRange ef_slice_range(uint32_t wl, uint64_t pos_begin, uint64_t pos_end, uint64_t before, uint64_t ones) {
    EfRange r;
    r.low_w0 = (before * wl) >> 6;
    r.n_low = (((before + ones) * wl + 63) >> 6) - r.low_w0;
    r.high_w0 = ((pos_begin >> wl) + before) >> 6;
    r.n_high = ((((pos_end - 1) >> wl) + before + ones - 1) >> 6) + 1 - r.high_w0;
    return r;
}

// Where a piece's encode writes: zeroed words [low_w0, low_w0 + n_low) of m_low at `low`, [high_w0, high_w0 + n_high) of m_high at `high`.
struct EfOut {
    uint64_t *low, *high;
    uint64_t low_w0, n_low, high_w0, n_high;
};
struct EfOrPlain {
    __host__ __device__ void operator()(uint64_t *p, uint64_t v) const { *p |= v; }
};

// One word under construction: bits meant for word `w` are gathered in `v` and ORed into the array when the next bit belongs to another
// word (ranks and positions ascend within a plain word, so a word is left for good).  A word outside the piece's range is counted, not
// written: it cannot happen with the ranges of ef_slice_range and true ranks, and the count says so to the caller.
template <class Or> struct EfPending {
    uint64_t w = ~0ULL, v = 0;
    __host__ __device__ void put(uint64_t word, uint64_t bits, uint64_t *arr, uint64_t w0, uint64_t n, Or &or_, uint32_t &bad) {
        if (word != w) { flush(arr, w0, n, or_, bad); w = word; v = 0; }
        v |= bits;
    }
    __host__ __device__ void flush(uint64_t *arr, uint64_t w0, uint64_t n, Or &or_, uint32_t &bad) {
        if (w == ~0ULL) return;
        const uint64_t i = w - w0;  // (wraps to a huge value in front of the range)
        if (i < n) or_(arr + i, v); else ++bad;
    }
};

// The set bits of plain word x, which covers positions [pos0, pos0 + 64) and whose first set bit has rank k.  Returns the number of words it
// would have written outside the piece's range (0).  At most 64 rounds.
template <class Or> __host__ __device__ static inline uint32_t ef_encode_word(uint64_t x, uint64_t pos0, uint64_t k, uint32_t wl, const EfOut &o, Or or_) {
    uint32_t bad = 0;
    EfPending<Or> lo, hi;
    const uint64_t lowmask = (1ULL << wl) - 1;  // 1 <= wl <= 63
    while (x) {
        const uint64_t pos = pos0 + (uint64_t)__builtin_ctzll(x);
        x &= x - 1;
        const uint64_t v = pos & lowmask, bit = k * wl, wd = bit >> 6, sh = bit & 63;
        lo.put(wd, v << sh, o.low, o.low_w0, o.n_low, or_, bad);
        if (sh + wl > 64) lo.put(wd + 1, v >> (64 - sh), o.low, o.low_w0, o.n_low, or_, bad);  // the element straddles two words
        const uint64_t hp = (pos >> wl) + k;
        hi.put(hp >> 6, 1ULL << (hp & 63), o.high, o.high_w0, o.n_high, or_, bad);
        ++k;
    }
    lo.flush(o.low, o.low_w0, o.n_low, or_, bad);
    hi.flush(o.high, o.high_w0, o.n_high, or_, bad);
    return bad;
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------------
// Elias-Fano encode on the device (writer)
// ------------------------------------------------------------------------------------------------
// One slice of rows: k_ef_block_counts and k_ef_block_prefix (ef_decode.inc) over the PLAIN words give the set bits in front of every block
// of 256 words; here a thread takes a word, a workgroup scan gives the rank of its first set bit, and the thread walks its set bits.  What it
// has gathered for one word of m_low / m_high goes out in one relaxed device-scope atomic OR (words are shared between threads, workgroups
// and -- through the host's OR -- slices).  No workgroup waits for another.
struct EfOrAtomic {
    __device__ void operator()(uint64_t *p, uint64_t v) const {
        (void)__hip_atomic_fetch_or((unsigned long long *)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
struct EfEncArgs {
    const uint64_t *words;  // the slice's plain words
    uint64_t n_words, pos0, ones_before;  // pos0: plain position of bit 0 of words[0]; ones_before: set bits of the index in front of the slice
    EfOut out;              // zeroed device scratch
    unsigned long long *bad;
    uint32_t wl;
};
__global__ __launch_bounds__(256) void k_ef_encode(const EfEncArgs a, const uint64_t *block_prefix /* exclusive, per 256-word block */) {
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    const uint64_t word = i < a.n_words ? a.words[i] : 0ULL;
    uint32_t block_ones;
    const uint32_t before = block_scan<256>((uint32_t)__popcll(word), block_ones);  // ones of the block's words in front of this one
    if (!word) return;
    const uint64_t k = a.ones_before + block_prefix[blockIdx.x] + before;  // 64-bit: the high ranks of a large index pass 2^32
    const uint32_t bad = ef_encode_word(word, a.pos0 + i * 64, k, a.wl, a.out, EfOrAtomic());
    if (bad) atomicAdd(a.bad, (unsigned long long)bad);
}
#endif
