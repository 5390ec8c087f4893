// shard_kernels.inc -- row-range sharded probing kernels (k_probe_partial, k_and_partial, list compaction, emplace)
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.

// ------------------------------------------------------------------------------------------------
// row-sharded ("hash-bin" sharded) probing: every rank holds rows [row_begin, row_end) of the IBF.  A probe word is
// written by exactly one rank (all others write 0), so one sum all-reduce of the partial buffer reconstructs it
// exactly (SURVEY 8(e)); the AND over the h hash functions happens afterwards.
// ------------------------------------------------------------------------------------------------
struct ShardArgs {
    const uint64_t *list;        // minimiser values, wavefront log layout
    const WaveMeta *wave_meta;   // start of wavefront g's region in `list` / `rowlog` (base) and in `rows` (esc_base)
    const uint64_t *cbase;       // start of wavefront g's entries in the COMPACT partial buffer
    const uint32_t *wave_count;
    const uint64_t *words;
    uint64_t S, row_begin, row_end;
    uint32_t shift, h, W;
    uint64_t *partial;           // [entry][h][W]
    uint64_t *rows;              // escaped-row regions of the wavefront logs (k_and_partial)
    uint32_t *rowlog;            // compact row log (owner in bits 26-31 on entry to k_and_partial)
    uint32_t B, n_waves;
    uint64_t esc_capacity;       // extent of `rows` in rows
    uint32_t *status;
};
template <int W>
__global__ __launch_bounds__(256) void k_probe_partial(const ShardArgs a) {
    const uint32_t g = blockIdx.x, count = a.wave_count[g];
    const uint64_t *list = a.list + a.wave_meta[g].base;
    uint64_t *out = a.partial + a.cbase[g] * a.h * W;
    for (uint32_t e = threadIdx.x; e < count; e += blockDim.x) {
        const uint64_t val = list[e];
        for (uint32_t i = 0; i < a.h; ++i) {
            const uint64_t row = hash_and_fit_row(val, c_ibf_seeds[i], a.S, a.shift);
            const bool mine = row >= a.row_begin && row < a.row_end;
            const uint64_t *p = a.words + (mine ? (row - a.row_begin) * W : 0);
#pragma unroll
            for (int w = 0; w < W; ++w) out[((size_t)e * a.h + i) * W + w] = mine ? __builtin_nontemporal_load(p + w) : 0ULL;
        }
    }
}
// The AND of a minimiser's h rows becomes entry e of the wavefront's log (k_and_partial, k_shx_and): an escaped row claims a slot of the
// wavefront's region `rows` (ecap rows) from the workgroup's counter s_esc, or raises status bit 0 when the region is full.
template <int W>
__device__ __forceinline__ void store_row_entry(const uint64_t *row, uint32_t B, uint32_t *log, uint32_t e, uint64_t *rows, uint32_t ecap, uint32_t *s_esc, uint32_t *status) {
    bool esc;
    uint32_t entry = encode_row<W>(row, B, log[e] >> 26, esc);
    if (esc) {
        const uint32_t slot = atomicAdd(s_esc, 1u);
        if (slot < ecap) {
#pragma unroll
            for (int w = 0; w < W; ++w) rows[(size_t)slot * W + w] = row[w];
            entry |= (slot + 1) << 2;
        } else {
            atomicOr(status, 1u);
        }
    }
    log[e] = entry;
}
template <int W>
__global__ __launch_bounds__(256) void k_and_partial(const ShardArgs a) {
    __shared__ uint32_t s_esc;
    const uint32_t g = blockIdx.x, count = a.wave_count[g];
    const uint64_t *in = a.partial + a.cbase[g] * a.h * W;
    const uint64_t ebase = a.wave_meta[g].esc_base;
    const uint32_t ecap = a.wave_meta[g].esc_cap;  // written by k_minimise_probe (MODE_LIST) for its region
    uint64_t *rows = a.rows + ebase * W;
    uint32_t *log = a.rowlog + a.wave_meta[g].base;
    if (threadIdx.x == 0) s_esc = 0;
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < count; e += blockDim.x) {
        uint64_t acc[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            acc[w] = ~0ULL;
            for (uint32_t i = 0; i < a.h; ++i) acc[w] &= in[((size_t)e * a.h + i) * W + w];
        }
        store_row_entry<W>(acc, a.B, log, e, rows, ecap, &s_esc, a.status);
    }
}
__global__ __launch_bounds__(256) void k_compact_list(const ShardArgs a, uint64_t *out) {
    const uint32_t g = blockIdx.x, count = a.wave_count[g];
    const uint64_t *list = a.list + a.wave_meta[g].base;
    uint64_t *dst = out + a.cbase[g];
    for (uint32_t e = threadIdx.x; e < count; e += blockDim.x) dst[e] = list[e];
}
__global__ void k_emplace_values(uint64_t *words, const uint64_t *values, uint64_t n, uint32_t bin, uint64_t S, uint64_t row_begin, uint64_t row_end,
                                 uint32_t shift, uint32_t h, uint32_t W) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t v = values[i];
        for (uint32_t j = 0; j < h; ++j) {
            const uint64_t row = hash_and_fit_row(v, c_ibf_seeds[j], S, shift);
            if (row >= row_begin && row < row_end) atomicOr((unsigned long long *)&words[(row - row_begin) * W + (bin >> 6)], 1ULL << (bin & 63));
        }
    }
}
__global__ void k_counts_to_u64(const uint32_t *c, uint32_t n, uint64_t *out /* n + 1 */) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = c[i];
    else if (i == n) out[i] = 0;
}
