// scan.inc -- sums and prefix sums over a wavefront, a workgroup and an array: the one place where "sizes -> offsets" is written
// Part of the single translation unit charon_hip.hip (included in order, right behind common.inc); not a stand-alone source.
//
//   wave_sum, wave_scan, wave_max_*   over the 64 lanes of a wavefront, by shuffles, no LDS
//   block_scan<THREADS>               one value a thread: its exclusive prefix over the workgroup, and the workgroup's total to every thread
//   array_scan<THREADS, T>            n values by ONE workgroup: four values a thread and round (THREADS * 4 a round: 1024 with 256 threads),
//                                     the carry from round to round in a register
// Every thread of the workgroup calls block_scan / array_scan, with the same n: both hold barriers.  The sums are unsigned and wrap; a
// caller that wants 64-bit sums of 32-bit values asks for T = uint64_t and converts in its load.
// Callers: k_split_scan, k_deflate_scan, k_ef_block_prefix, k_scan_u64, k_scan_meta, k_radix_offsets, k_unique_offsets (array_scan);
// k_ef_block_counts, k_ef_decode, k_ef_encode, k_radix_offsets, k_unique_count, k_unique_compact (block_scan); k_wave_caps, the text / FASTA splitters, DflWavePolicy (the wave forms).  tools/scan_check.hip checks all of it.

// sum over the lanes, to every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((long long)v, o);
    return v;
}
// inclusive scan over the lanes: lane l gets the sum of lanes 0 .. l
__device__ __forceinline__ uint32_t wave_scan(uint32_t v) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)v, o); if (lane_id() >= (uint32_t)o) v += t; }
    return v;
}
__device__ __forceinline__ uint64_t wave_scan(uint64_t v) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) { const uint64_t t = (uint64_t)__shfl_up((long long)v, o); if (lane_id() >= (uint32_t)o) v += t; }
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        uint64_t t = (uint64_t)__shfl_xor((long long)v, o);
        v = t > v ? t : v;
    }
    return v;
}

// The block step.  Returns the sum of `v` over the threads in front of this one; `total` becomes the sum over all THREADS threads.
// A wave scan, one partial a wavefront in LDS, two barriers (the second frees the partials for the next call).
template <uint32_t THREADS, class T>
__device__ __forceinline__ T block_scan(T v, T &total) {
    static_assert(THREADS % WAVE == 0 && THREADS >= WAVE && THREADS <= 1024, "whole wavefronts, one workgroup");
    constexpr uint32_t NW = THREADS / WAVE;
    __shared__ T part[NW];
    const uint32_t wv = threadIdx.x / WAVE;
    const T incl = wave_scan(v);
    if (lane_id() == WAVE - 1) part[wv] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < NW; ++k) { const T p = part[k]; if (k < wv) before += p; all += p; }
    __syncthreads();
    total = all;
    return before + incl - v;
}

// The one-workgroup array scan: store(i, sum of load(0 .. i - 1)) for every i < n, and the sum of all n values to every thread.
// A thread loads its four values of a round before it stores their prefixes and no other thread touches them, so `store` may write
// where `load` reads (in place).  n == 0: no load, no store, 0.  n <= 2^32 - 4 * THREADS (the round counter is 32 bits wide).
#define SCAN_THREADS 256  // the workgroup of every scan kernel of the library: a round is 1024 values
template <uint32_t THREADS, class T, class Load, class Store>
__device__ __forceinline__ T array_scan(uint32_t n, Load load, Store store) {
    T carry = 0;
    for (uint32_t base = 0; base < n; base += THREADS * 4) {
        const uint32_t i = base + threadIdx.x * 4;
        T v[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) v[k] = i + k < n ? (T)load(i + k) : (T)0;
        T all;
        T at = carry + block_scan<THREADS, T>(v[0] + v[1] + v[2] + v[3], all);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) { if (i + k < n) store(i + k, at); at += v[k]; }
        carry += all;
    }
    return carry;
}
