// len_order.inc -- length-class ordering (stable counting sort) and the algorithmic byte counter
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.

// ------------------------------------------------------------------------------------------------
// length-class ordering (counting sort on an 8-steps-per-octave bucket of the total read length)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t len_bucket(uint32_t len) {
    if (len < 8) return len;
    const uint32_t e = 31u - (uint32_t)__clz((int)len);
    return (e - 2) * 8 + ((len >> (e - 3)) & 7u);  // 8..247
}
// Stable (deterministic) counting sort: the read -> wavefront assignment must be identical on every rank of the
// row-sharded mode, and reproducible run to run.  LEN_BLOCKS workgroups each own a contiguous chunk of reads.
#define LEN_BLOCKS 256
// Per-slot control words on the device (zeroed by k_len_hist at the head of every batch chain).  CTL_GATE: workgroups of the ordinary probe
// launch that have started (the probe gate, k1_minimise_probe.inc); a re-run after a log overflow, which has no gate, sums lengths there.
enum { CTL_BYTES = 0, CTL_MINIMISERS = 1, CTL_LOG_CURSOR = 2, CTL_ESC_CURSOR = 3, CTL_STATUS = 4, CTL_NLONG = 5, CTL_FETCHES = 6, CTL_GATE = 7, CTL_WORDS = 8,
       CTL_SUM_LEN = CTL_WORDS - 1 };  // k_sum_len's scratch word in such a re-run: the last word, which is the gate's
// Reads of at least 2^15 bases (bucket 104 and up; the order lists them first) are split over the lanes of a wavefront by the SPLIT
// launch of k_minimise_probe.  CHN_STREAM_SPLIT_BUCKET(b) overrides the bucket for testing (255: never split).
#define LONG_BUCKET_DEFAULT 104u
__host__ __device__ __forceinline__ uint32_t len_bucket_floor(uint32_t bucket) {  // smallest length in `bucket` (bucket >= 8)
    const uint32_t e = bucket / 8 + 2, sub = bucket & 7u;
    return (1u << e) + (sub << (e - 3));
}
// Two launches order a batch: k_len_hist (per-block bucket counts; also clears the slot's control words) and k_len_scatter (every block derives its own start positions from the block histograms -- no separate scan launch).
__global__ __launch_bounds__(256) void k_len_hist(const uint32_t *len1, const uint32_t *len2, uint32_t n, uint32_t *blockhist /* [LEN_BLOCKS][256] */,
                                                  unsigned long long *ctl) {
    __shared__ uint32_t sh[256];
    sh[threadIdx.x] = 0;
    if (blockIdx.x == 0 && threadIdx.x < CTL_WORDS) ctl[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t chunk = (n + LEN_BLOCKS - 1) / LEN_BLOCKS, lo = blockIdx.x * chunk, hi = min(n, lo + chunk);
    for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) atomicAdd(&sh[len_bucket(len1[i] + (len2 ? len2[i] : 0u))], 1u);
    __syncthreads();
    blockhist[blockIdx.x * 256 + threadIdx.x] = sh[threadIdx.x];
}
// long_bucket < 256: block 0 also publishes the number of reads in buckets >= long_bucket (ctl[CTL_NLONG]; single-end batches only; at most split_cap)
__global__ __launch_bounds__(256) void k_len_scatter(const uint32_t *len1, const uint32_t *len2, uint32_t n, const uint32_t *blockhist, uint32_t *order,
                                                     unsigned long long *ctl, uint32_t long_bucket, uint32_t split_cap) {
    __shared__ uint32_t cursor[256], tot[256];
    __shared__ uint16_t tile[256];
    {   // start of (this block, bucket b): buckets are laid out longest first, blocks in index order inside a bucket
        const uint32_t b = threadIdx.x;
        uint32_t t = 0, pre = 0;
        for (uint32_t k = 0; k < LEN_BLOCKS; ++k) { const uint32_t c = blockhist[k * 256 + b]; t += c; if (k < blockIdx.x) pre += c; }
        tot[b] = t;
        __syncthreads();
        uint32_t start = 0;
        for (uint32_t x = b + 1; x < 256; ++x) start += tot[x];
        cursor[b] = start + pre;
        // (more long reads than the caller's buffers can hold -- a device batch with overlapping segments -- : none is split)
        if (blockIdx.x == 0 && b == long_bucket && !len2 && start + tot[b] <= split_cap) ctl[CTL_NLONG] = (unsigned long long)start + tot[b];
    }
    const uint32_t chunk = (n + LEN_BLOCKS - 1) / LEN_BLOCKS, lo = blockIdx.x * chunk, hi = min(n, lo + chunk);
    for (uint32_t base = lo; base < hi; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t bk = i < hi ? len_bucket(len1[i] + (len2 ? len2[i] : 0u)) : 0xffffu;
        __syncthreads();
        tile[threadIdx.x] = (uint16_t)bk;
        __syncthreads();
        uint32_t rank = 0, same = 0;
        // uniform-length batches put the whole tile into one bucket: rank = thread index, no counting needed
        const bool uniform_tile = __syncthreads_and(tile[threadIdx.x] == tile[0] && bk != 0xffffu) != 0;
        if (uniform_tile) {
            rank = threadIdx.x; same = 256;
            order[cursor[bk] + rank] = i;
        } else if (i < hi) {
            for (uint32_t j = 0; j < 256; ++j) { const bool eq = tile[j] == bk; same += eq; rank += eq && j < threadIdx.x; }
            order[cursor[bk] + rank] = i;
        }
        __syncthreads();
        if (i < hi && rank == same - 1) cursor[bk] += same;  // the last read of each bucket in this tile advances the cursor
    }
}

// sum of the segment lengths of a batch (sizing of the worst-case re-run after a log overflow)
__global__ void k_sum_len(const uint32_t *len1, const uint32_t *len2, uint32_t n, unsigned long long *out) {
    unsigned long long s = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) s += (unsigned long long)len1[i] + (len2 ? len2[i] : 0u);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor((long long)s, o);
    if (lane_id() == 0 && s) atomicAdd(out, s);
}

// algorithmic bytes of a batch (SURVEY 8(d)): sum ceil(L/4) + M*h*W*8 + (8 + 8C)
__global__ void k_batch_bytes(const uint32_t *len1, const uint32_t *len2, const uint32_t *num_hashes, uint32_t n,
                              uint32_t hW8, uint32_t outb, unsigned long long *acc /* [2]: bytes, minimisers */) {
    unsigned long long b = 0, m = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t L = len1[i] + (len2 ? len2[i] : 0u);
        b += (L + 3) / 4 + (unsigned long long)num_hashes[i] * hW8 + outb;
        m += num_hashes[i];
    }
    for (int o = 32; o > 0; o >>= 1) { b += __shfl_xor((long long)b, o); m += __shfl_xor((long long)m, o); }
    if (lane_id() == 0) { atomicAdd(&acc[0], b); atomicAdd(&acc[1], m); }
}
