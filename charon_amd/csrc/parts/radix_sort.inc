// radix_sort.inc -- sort and unique of the 64-bit values of a device-resident minimiser set (chn_hashset_unique, abi_hashset.inc)
// Part of the single translation unit charon_hip.hip (included in order, behind scan.inc and radix_plan.hpp); not a stand-alone source.
//
// An LSD radix sort, 8-bit digits, ping-pong between two buffers, and a unique pass over the sorted keys.  No workgroup waits for
// another: what one kernel needs of the whole array is there when it starts, written by the kernel in front of it.  Every loop is
// bounded by the key count, the tile or the 8 passes.
//   k_radix_hist      once: the 8 digit histograms of all keys (LDS counters a workgroup, 64-bit atomics to the global ones).  The host reads
//                     them: a pass whose keys all share the digit moves nothing and is not run
//   per pass that runs:
//   k_radix_count     one workgroup a tile: counts[digit][tile]
//   k_radix_offsets   one workgroup a digit: array_scan in place over the digit's tile counts; the digit's base (keys of smaller digits,
//                     from the histogram) goes to base[digit].  256 workgroups, none needs another's result
//   k_radix_scatter   one workgroup a tile: the stable rank of a key among the tile's keys of its digit, then dst[base + offset + rank]
//   k_unique_count    one workgroup a tile: heads (v[i] != v[i - 1]) of the tile
//   k_unique_offsets  one workgroup: array_scan over the tile counts, the distinct count
//   k_unique_compact  one workgroup a tile: block_scan of the head flags, 256 keys a round, heads to out[offset + prefix]
// A tile is `tile` keys (radix_plan.hpp; a run-time value: chn_hashset_cfg.tile_keys is a test hook); wavefront w of the workgroup owns
// keys [w, w + 1) * tile / 4 of it and walks them 64 at a time, so the order "wavefront, round, lane" is the order of the keys: ranks
// counted in that order keep equal digits in their order (the sort is stable, which is what makes LSD passes add up).
// Counters per tile and digit are 32 bits (a set holds fewer than 2^32 values), global offsets 64 bits.

__device__ __forceinline__ void wave_lds_sync() {  // LDS written by some lanes of the wavefront is read by others behind this
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the live lanes of the wavefront whose digit is this lane's (8 ballots); 0 for a lane that is not live
__device__ __forceinline__ uint64_t wave_match_digit(uint32_t digit, bool live) {
    uint64_t m = __ballot(live ? 1 : 0);
#pragma unroll
    for (uint32_t b = 0; b < RADIX_BITS; ++b) {
        const bool one = (digit >> b) & 1u;
        const uint64_t with = __ballot(live && one ? 1 : 0);
        m &= one ? with : ~with;
    }
    return live ? m : 0;
}

__global__ __launch_bounds__(RADIX_THREADS) void k_radix_hist(const uint64_t *keys, uint64_t n, unsigned long long *hist /* [8][256] */) {
    __shared__ uint32_t s_hist[RADIX_PASSES * RADIX_DIGITS];  // a workgroup sees fewer than 2^32 keys
    for (uint32_t i = threadIdx.x; i < RADIX_PASSES * RADIX_DIGITS; i += RADIX_THREADS) s_hist[i] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * RADIX_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RADIX_THREADS) {
        const uint64_t key = keys[i];
#pragma unroll
        for (uint32_t p = 0; p < RADIX_PASSES; ++p) atomicAdd(&s_hist[p * RADIX_DIGITS + ((uint32_t)(key >> (p * RADIX_BITS)) & 255u)], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < RADIX_PASSES * RADIX_DIGITS; i += RADIX_THREADS)
        if (s_hist[i]) atomicAdd(&hist[i], (unsigned long long)s_hist[i]);
}

// The digit counts of every wavefront's quarter of tile `blockIdx.x` into s_wave[wavefront][digit] (zeroed here).  One lane of every group
// of equal digits adds the group's size: the lanes that write in one step write different counters, and the steps of a wavefront follow
// each other, so no atomic is needed.  Ends with a barrier.
__device__ __forceinline__ void tile_wave_counts(const uint64_t *keys, uint64_t n, uint32_t tile, uint32_t shift, uint32_t (*s_wave)[RADIX_DIGITS]) {
    const uint32_t wv = threadIdx.x / WAVE, per_wave = tile / (RADIX_THREADS / WAVE);
    const uint64_t first = (uint64_t)blockIdx.x * tile + (uint64_t)wv * per_wave;
#pragma unroll
    for (uint32_t w = 0; w < RADIX_THREADS / WAVE; ++w) s_wave[w][threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t r = 0; r < per_wave; r += WAVE) {
        const uint64_t i = first + r + lane_id();
        const bool live = i < n;
        const uint32_t digit = live ? (uint32_t)(keys[i] >> shift) & 255u : 0u;
        const uint64_t m = wave_match_digit(digit, live);
        if (live && (m & ((1ULL << lane_id()) - 1)) == 0) s_wave[wv][digit] += (uint32_t)__popcll(m);
        wave_lds_sync();
    }
    __syncthreads();
}

__global__ __launch_bounds__(RADIX_THREADS) void k_radix_count(const uint64_t *keys, uint64_t n, uint32_t tile, uint32_t shift, uint32_t *counts /* [256][tiles] */) {
    __shared__ uint32_t s_wave[RADIX_THREADS / WAVE][RADIX_DIGITS];
    tile_wave_counts(keys, n, tile, shift, s_wave);
    uint32_t c = 0;
#pragma unroll
    for (uint32_t w = 0; w < RADIX_THREADS / WAVE; ++w) c += s_wave[w][threadIdx.x];
    counts[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] = c;
}

// workgroup d: counts[d][t] becomes the number of keys of digit d in the tiles in front of t; base[d] the number of keys of smaller digits
__global__ __launch_bounds__(RADIX_THREADS) void k_radix_offsets(uint32_t *counts, uint32_t tiles, const unsigned long long *hist /* of this pass */,
                                                                 unsigned long long *base /* [256] */) {
    const uint32_t d = blockIdx.x;
    uint64_t all;
    const uint64_t smaller = block_scan<RADIX_THREADS, uint64_t>((uint64_t)hist[threadIdx.x], all);
    if (threadIdx.x == d) base[d] = smaller;
    uint32_t *row = counts + (uint64_t)d * tiles;
    (void)array_scan<RADIX_THREADS, uint32_t>(tiles, [&](uint32_t i) { return row[i]; }, [&](uint32_t i, uint32_t v) { row[i] = v; });
}

__global__ __launch_bounds__(RADIX_THREADS) void k_radix_scatter(const uint64_t *keys, uint64_t n, uint32_t tile, uint32_t shift, const uint32_t *offsets /* [256][tiles] */,
                                                                 const unsigned long long *base /* [256] */, uint64_t *dst) {
    __shared__ uint32_t s_wave[RADIX_THREADS / WAVE][RADIX_DIGITS];
    __shared__ uint64_t s_at[RADIX_DIGITS];
    tile_wave_counts(keys, n, tile, shift, s_wave);
    {   // thread = digit: where the tile's keys of this digit go, and where each wavefront's begin among them
        uint32_t before = 0;
#pragma unroll
        for (uint32_t w = 0; w < RADIX_THREADS / WAVE; ++w) { const uint32_t c = s_wave[w][threadIdx.x]; s_wave[w][threadIdx.x] = before; before += c; }
        s_at[threadIdx.x] = (uint64_t)base[threadIdx.x] + offsets[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x];
    }
    __syncthreads();
    const uint32_t wv = threadIdx.x / WAVE, per_wave = tile / (RADIX_THREADS / WAVE);
    const uint64_t first = (uint64_t)blockIdx.x * tile + (uint64_t)wv * per_wave;
    for (uint32_t r = 0; r < per_wave; r += WAVE) {
        const uint64_t i = first + r + lane_id();
        const bool live = i < n;
        const uint64_t key = live ? keys[i] : 0;
        const uint32_t digit = (uint32_t)(key >> shift) & 255u;
        const uint64_t m = wave_match_digit(digit, live);
        const uint32_t rank = (uint32_t)__popcll(m & ((1ULL << lane_id()) - 1));
        const uint32_t taken = s_wave[wv][digit];  // by the rounds in front of this one
        wave_lds_sync();
        if (live && rank == 0) s_wave[wv][digit] = taken + (uint32_t)__popcll(m);
        wave_lds_sync();
        const uint64_t at = s_at[digit] + taken + rank;
        if (live && at < n) dst[at] = key;  // (at < n holds by construction: the counts are of these keys)
    }
}

// ---- unique over sorted keys ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool unique_head(const uint64_t *keys, uint64_t i, uint64_t key) { return i == 0 || keys[i - 1] != key; }

__global__ __launch_bounds__(RADIX_THREADS) void k_unique_count(const uint64_t *keys, uint64_t n, uint32_t tile, uint32_t *tile_counts) {
    const uint64_t first = (uint64_t)blockIdx.x * tile, end = first + tile < n ? first + tile : n;
    uint32_t c = 0;
    for (uint64_t i = first + threadIdx.x; i < end; i += RADIX_THREADS) c += unique_head(keys, i, keys[i]) ? 1u : 0u;
    uint32_t all;
    (void)block_scan<RADIX_THREADS, uint32_t>(c, all);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = all;
}

__global__ __launch_bounds__(RADIX_THREADS) void k_unique_offsets(uint32_t *tile_counts, uint32_t tiles, unsigned long long *distinct) {
    const uint32_t all = array_scan<RADIX_THREADS, uint32_t>(tiles, [&](uint32_t i) { return tile_counts[i]; }, [&](uint32_t i, uint32_t v) { tile_counts[i] = v; });
    if (threadIdx.x == 0) *distinct = all;
}

__global__ __launch_bounds__(RADIX_THREADS) void k_unique_compact(const uint64_t *keys, uint64_t n, uint32_t tile, const uint32_t *tile_offsets, uint64_t distinct,
                                                                  uint64_t *out) {
    const uint64_t first = (uint64_t)blockIdx.x * tile;
    uint64_t at = tile_offsets[blockIdx.x];
    for (uint32_t r = 0; r < tile && first + r < n; r += RADIX_THREADS) {  // (the same rounds for every thread: block_scan holds barriers)
        const uint64_t i = first + r + threadIdx.x;
        const bool live = i < n;
        const uint64_t key = live ? keys[i] : 0;
        const uint32_t head = live && unique_head(keys, i, key) ? 1u : 0u;
        uint32_t all;
        const uint64_t to = at + block_scan<RADIX_THREADS, uint32_t>(head, all);
        if (head && to < distinct) out[to] = key;  // (to < distinct holds by construction)
        at += all;
    }
}
