// shardx_kernels.inc -- sparse row-sharded probing: query / response exchange between the ranks that own the rows
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.

// ------------------------------------------------------------------------------------------------
// Row-range sharded index, sparse exchange (north-star config 4).  Rank r holds rows [splits[r], splits[r+1]).  Every rank
// minimises only ITS OWN reads; each probe (minimiser e, hash function i) becomes a 4-byte query -- the row number local to
// the owning rank -- in a buffer grouped by owner; one all-to-all carries the queries to the owners, k_shx_serve gathers the
// W words of every queried row, a second all-to-all carries them back in the same order, and k_shx_and ANDs the h rows of each
// minimiser into the usual compact row log.  Per probe 4 bytes go out and 8 W come back (the dense scheme of
// shard_kernels.inc all-reduces 8 W bytes per probe through every rank and minimises every read on every rank).
//
// The query order must be reproducible, because the responses are matched to their probes by position only: queries are
// ordered by (owner rank, wavefront log g, chunk of 256 entries, hash function i, entry), and k_shx_scatter / k_shx_and walk
// the log with the same code (shx_walk).
// ------------------------------------------------------------------------------------------------
#define SHX_MAX_RANKS 16
#define SHX_THREADS 256
struct ShxArgs {
    const uint64_t *list;        // minimiser values, wavefront log layout (MODE_LIST)
    const WaveMeta *wave_meta;
    const uint32_t *wave_count;
    uint32_t n_waves, n_ranks, h, shift;
    uint64_t S;
    uint64_t splits[SHX_MAX_RANKS + 1];
    uint64_t *cnt;               // [n_ranks][n_waves + 1]: probes of wavefront g owned by rank r; scanned in place to offsets
    uint64_t send_base[SHX_MAX_RANKS + 1];  // start of rank r's group in the query / response buffers
    uint32_t *queries;           // k_shx_scatter out
    const uint64_t *resp;        // k_shx_and in: [probe position][W]
    uint32_t *rowlog;
    uint64_t *rows;
    uint64_t esc_capacity;
    uint32_t *status;
    uint32_t B;
};

__device__ __forceinline__ uint32_t shx_owner(const ShxArgs &a, uint64_t row) {
    uint32_t o = 0;
    for (uint32_t r = 1; r < a.n_ranks; ++r) o += row >= a.splits[r];
    return o;
}

__global__ __launch_bounds__(SHX_THREADS) void k_shx_count(const ShxArgs a) {
    __shared__ uint32_t c[SHX_THREADS / WAVE][SHX_MAX_RANKS];
    const uint32_t g = blockIdx.x, count = a.wave_count[g], wv = threadIdx.x / WAVE;
    uint32_t mine = 0;  // lane r of every wave counts owner r (n_ranks <= 16 <= 64)
    const uint64_t *list = a.list + a.wave_meta[g].base;
    for (uint32_t base = 0; base < count; base += SHX_THREADS) {
        const uint32_t e = base + threadIdx.x;
        const bool valid = e < count;
        const uint64_t val = valid ? list[e] : 0;
        for (uint32_t i = 0; i < a.h; ++i) {
            const uint32_t owner = shx_owner(a, hash_and_fit_row(val, c_ibf_seeds[i], a.S, a.shift));
            for (uint32_t r = 0; r < a.n_ranks; ++r) {
                const uint64_t m = __ballot(valid && owner == r);
                if (lane_id() == r) mine += (uint32_t)__popcll(m);
            }
        }
    }
    if (lane_id() < SHX_MAX_RANKS) c[wv][lane_id()] = mine;
    __syncthreads();
    if (threadIdx.x < a.n_ranks) {
        uint32_t t = 0;
        for (uint32_t w2 = 0; w2 < SHX_THREADS / WAVE; ++w2) t += c[w2][threadIdx.x];
        a.cnt[(size_t)threadIdx.x * (a.n_waves + 1) + g] = t;
        if (g == 0) a.cnt[(size_t)threadIdx.x * (a.n_waves + 1) + a.n_waves] = 0;
    }
}
// (k_scan_u64 with one workgroup per rank then scans that rank's n_waves + 1 counts in place: the total lands in element n_waves)

// Walk wavefront log g in the canonical probe order and hand every probe to `f(e, i, k, valid, row, owner, gpos)`, gpos = its
// position in the query / response buffers (send_base[owner] + offset of (owner, g) + rank inside (owner, g)).  A chunk is
// SHX_EPT x 256 entries (entry e = base + k * 256 + tid); inside (chunk, hash function i) probes are ordered by (k, tid).  One
// barrier per (chunk, i): per-(k, wave) owner counts and the running per-owner totals are double-buffered in LDS.
#define SHX_EPT 4
template <class F>
__device__ __forceinline__ void shx_walk(const ShxArgs &a, uint32_t g, F &&f) {
    constexpr uint32_t NW = SHX_THREADS / WAVE;
    __shared__ uint32_t wcnt[2][SHX_EPT * NW][SHX_MAX_RANKS];
    __shared__ uint32_t run[2][SHX_MAX_RANKS];
    __shared__ uint64_t gbase[SHX_MAX_RANKS];  // where (owner, g) starts in the buffers
    const uint32_t count = a.wave_count[g], tid = threadIdx.x, wv = tid / WAVE;
    const uint64_t *list = a.list + a.wave_meta[g].base;
    if (tid < SHX_MAX_RANKS) {
        run[0][tid] = 0;
        gbase[tid] = tid < a.n_ranks ? a.send_base[tid] + a.cnt[(size_t)tid * (a.n_waves + 1) + g] : 0;
    }
    uint32_t buf = 0;
    for (uint32_t base = 0; base < count; base += SHX_EPT * SHX_THREADS) {
        uint64_t val[SHX_EPT];
#pragma unroll
        for (uint32_t k = 0; k < SHX_EPT; ++k) { const uint32_t e = base + k * SHX_THREADS + tid; val[k] = e < count ? list[e] : 0; }
        for (uint32_t i = 0; i < a.h; ++i) {
            uint64_t row[SHX_EPT];
            uint32_t owner[SHX_EPT], rank_in_wave[SHX_EPT];
#pragma unroll
            for (uint32_t k = 0; k < SHX_EPT; ++k) {
                const bool valid = base + k * SHX_THREADS + tid < count;
                row[k] = hash_and_fit_row(val[k], c_ibf_seeds[i], a.S, a.shift);
                owner[k] = shx_owner(a, row[k]);
                rank_in_wave[k] = 0;
                for (uint32_t r = 0; r < a.n_ranks; ++r) {
                    const uint64_t m = __ballot(valid && owner[k] == r);
                    if (owner[k] == r) rank_in_wave[k] = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    if (lane_id() == 0) wcnt[buf][k * NW + wv][r] = (uint32_t)__popcll(m);
                }
            }
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < SHX_EPT; ++k) {
                const uint32_t e = base + k * SHX_THREADS + tid;
                uint32_t before = run[buf][owner[k]];
                for (uint32_t s2 = 0; s2 < k * NW + wv; ++s2) before += wcnt[buf][s2][owner[k]];
                f(e, i, k, e < count, row[k], owner[k], gbase[owner[k]] + before + rank_in_wave[k]);
            }
            if (tid < a.n_ranks) {
                uint32_t t = run[buf][tid];
                for (uint32_t s2 = 0; s2 < SHX_EPT * NW; ++s2) t += wcnt[buf][s2][tid];
                run[buf ^ 1][tid] = t;
            }
            buf ^= 1;
        }
    }
}

__global__ __launch_bounds__(SHX_THREADS) void k_shx_scatter(const ShxArgs a) {
    shx_walk(a, blockIdx.x, [&](uint32_t, uint32_t, uint32_t, bool valid, uint64_t row, uint32_t owner, uint64_t gpos) {
        if (valid) a.queries[gpos] = (uint32_t)(row - a.splits[owner]);
    });
}

// the owner's side: out[j][w] = word w of local row queries[j] of this shard (random 8 W-byte gathers: HBM-bound).  Four
// queries per thread and pass: the query reads, the gathers and the stores of a pass are each issued back to back.
template <int W> struct ShxRow { uint64_t w[W]; };
typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));
template <int W>
__global__ __launch_bounds__(256) void k_shx_serve(const uint64_t *words, const uint32_t *queries, uint64_t n, uint64_t rows_local, uint64_t *out, uint32_t *status) {
    constexpr int U = 4;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j0 = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j0 < n; j0 += stride * U) {
        uint64_t q[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t j = j0 + u * stride;
            q[u] = j < n ? queries[j] : 0;
            ok[u] = j < n;
        }
        ShxRow<W> r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (q[u] >= rows_local) { if (ok[u]) atomicOr(status, 4u); q[u] = 0; }  // a row this shard does not hold: bookkeeping error upstream
            if (W == 2) {
                const u64x2_t v = __builtin_nontemporal_load(reinterpret_cast<const u64x2_t *>(words + q[u] * W));
                r[u].w[0] = v.x; r[u].w[W > 1 ? 1 : 0] = v.y;
            } else if (W == 4) {
                const u64x2_t v0 = __builtin_nontemporal_load(reinterpret_cast<const u64x2_t *>(words + q[u] * W));
                const u64x2_t v1 = __builtin_nontemporal_load(reinterpret_cast<const u64x2_t *>(words + q[u] * W + 2));
                r[u].w[0] = v0.x; r[u].w[W > 1 ? 1 : 0] = v0.y; r[u].w[W > 2 ? 2 : 0] = v1.x; r[u].w[W > 3 ? 3 : 0] = v1.y;
            } else {
#pragma unroll
                for (int w = 0; w < W; ++w) r[u].w[w] = __builtin_nontemporal_load(words + q[u] * W + w);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t j = j0 + u * stride;
            if (!ok[u]) continue;
            if (W == 2) {
                *reinterpret_cast<ulonglong2 *>(out + j * W) = make_ulonglong2(r[u].w[0], r[u].w[W > 1 ? 1 : 0]);
            } else if (W == 4) {
                *reinterpret_cast<ulonglong2 *>(out + j * W) = make_ulonglong2(r[u].w[0], r[u].w[W > 1 ? 1 : 0]);
                *reinterpret_cast<ulonglong2 *>(out + j * W + 2) = make_ulonglong2(r[u].w[W > 2 ? 2 : 0], r[u].w[W > 3 ? 3 : 0]);
            } else {
#pragma unroll
                for (int w = 0; w < W; ++w) out[j * W + w] = r[u].w[w];
            }
        }
    }
}

template <int W>
__global__ __launch_bounds__(SHX_THREADS) void k_shx_and(const ShxArgs a) {
    __shared__ uint32_t s_esc;
    const uint32_t g = blockIdx.x, tid = threadIdx.x;
    const uint64_t ebase = a.wave_meta[g].esc_base;
    const uint32_t ecap = a.wave_meta[g].esc_cap;  // written by k_minimise_probe when it claimed the region
    uint64_t *rows = a.rows + ebase * W;
    uint32_t *log = a.rowlog + a.wave_meta[g].base;
    if (tid == 0) s_esc = 0;
    uint64_t acc[SHX_EPT][W];  // running AND of this thread's entries of the current chunk
    shx_walk(a, g, [&](uint32_t e, uint32_t i, uint32_t k, bool valid, uint64_t, uint32_t, uint64_t gpos) {
        if (valid) {
            const uint64_t *r = a.resp + gpos * W;
            uint64_t v[W];
#pragma unroll
            for (int w = 0; w < W; ++w) v[w] = r[w];
#pragma unroll
            for (uint32_t kk = 0; kk < SHX_EPT; ++kk)
                if (kk == k) {
#pragma unroll
                    for (int w = 0; w < W; ++w) { acc[kk][w] = (i == 0 ? ~0ULL : acc[kk][w]) & v[w]; v[w] = acc[kk][w]; }
                }
            if (i + 1 == a.h) store_row_entry<W>(v, a.B, log, e, rows, ecap, &s_esc, a.status);
        }
    });
}
