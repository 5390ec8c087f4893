// ef_decode.inc -- Elias-Fano (sd_vector) decode and per-bin popcounts for the index loader
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.

// ------------------------------------------------------------------------------------------------
// Elias-Fano decode on the device (loader)
// ------------------------------------------------------------------------------------------------
struct EfArgs {
    const uint64_t *high, *low;
    uint64_t n_high_words, high_bit0, ones_before, low_elem0, m_size, row_begin, row_end;
    uint64_t *words;
    unsigned long long *bad;
    uint32_t wl, W, B, TB;
};
__global__ __launch_bounds__(256) void k_ef_block_counts(const uint64_t *high, uint64_t n, uint32_t *block_ones) {
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    uint32_t ones;
    block_scan<256>(i < n ? (uint32_t)__popcll(high[i]) : 0u, ones);
    if (threadIdx.x == 0) block_ones[blockIdx.x] = ones;
}
// exclusive prefix of the per-block counts, by one workgroup (a slice has some 10^4 blocks: n < 2^32): keeps a slice's whole chain on the device
__global__ __launch_bounds__(SCAN_THREADS) void k_ef_block_prefix(const uint32_t *counts, uint64_t n, uint64_t *prefix) {
    array_scan<SCAN_THREADS, uint64_t>((uint32_t)n, [&](uint32_t i) { return counts[i]; }, [&](uint32_t i, uint64_t at) { prefix[i] = at; });
}
__global__ __launch_bounds__(256) void k_ef_decode(const EfArgs a, const uint64_t *block_prefix /* exclusive, per 256-word block */) {
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    const uint64_t word = i < a.n_high_words ? a.high[i] : 0ULL;
    uint32_t block_ones;
    const uint32_t before = block_scan<256>((uint32_t)__popcll(word), block_ones);  // ones of the block's words in front of this one
    uint64_t k = a.ones_before + block_prefix[blockIdx.x] + before;  // rank of this word's first one
    uint64_t x = word;
    const uint64_t bit0 = a.high_bit0 + i * 64;
    const uint64_t lowmask = a.wl >= 64 ? ~0ULL : ((1ULL << a.wl) - 1);
    while (x) {
        const uint32_t j = (uint32_t)__ffsll((long long)x) - 1;
        x &= x - 1;
        const uint64_t z = bit0 + j - k;  // zeros before this one = its high part
        uint64_t lo = 0;
        if (a.wl) {
            const uint64_t bit = (k - a.low_elem0) * a.wl, wd = bit >> 6, sh = bit & 63;
            lo = a.low[wd] >> sh;
            if (sh + a.wl > 64) lo |= a.low[wd + 1] << (64 - sh);
            lo &= lowmask;
        }
        const uint64_t pos = (a.wl >= 64 ? 0 : (z << a.wl)) | lo;
        ++k;
        if (pos >= a.m_size) { atomicAdd(a.bad, 1ULL); continue; }
        const uint64_t row = pos / a.TB;
        const uint32_t bin = (uint32_t)(pos % a.TB);
        if (bin >= a.B) { atomicAdd(a.bad, 1ULL); continue; }
        if (row < a.row_begin || row >= a.row_end) continue;
        atomicOr((unsigned long long *)&a.words[(row - a.row_begin) * a.W + (bin >> 6)], 1ULL << (bin & 63));
    }
}
// Set bits per technical bin over the whole index (loader self-checks: the decoded vector lost no bit; fill per bin).  A thread walks words of
// ONE column of the rows (its stride is a multiple of W), so bit j of everything it reads is the same bin.  The eight bits of a byte go to
// eight accumulators whose BYTES count (x >> j) & 0x0101..01: three 64-bit operations per accumulator and word, emptied every 255 words --
// the kernel runs at HBM speed (a thread per bit and row, as before, took 16 ms per GB).
__global__ __launch_bounds__(256) void k_bin_popcounts(const uint64_t *words, uint64_t n_rows, uint32_t W, unsigned long long *out /* [W*64] */) {
    __shared__ uint32_t s[256];
    s[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t n_words = n_rows * W;
    const uint64_t T = ((uint64_t)gridDim.x * blockDim.x / W) * W;  // threads in use: a multiple of W, so a thread keeps its column
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < T) {
        const uint32_t col = (uint32_t)(t % W);
        const uint64_t M = 0x0101010101010101ULL;
        uint64_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t pending = 0;
        auto flush = [&]() {
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
#pragma unroll
                for (uint32_t k = 0; k < 8; ++k) {
                    const uint32_t c = (uint32_t)(acc[j] >> (8 * k)) & 0xffu;
                    if (c) atomicAdd(&s[col * 64 + 8 * k + j], c);
                }
                acc[j] = 0;
            }
            pending = 0;
        };
        for (uint64_t i = t; i < n_words; i += T) {
            const uint64_t x = __builtin_nontemporal_load(words + i);
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) acc[j] += (x >> j) & M;
            if (++pending == 255) flush();
        }
        flush();
    }
    __syncthreads();
    if (threadIdx.x < W * 64 && s[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)s[threadIdx.x]);
}
