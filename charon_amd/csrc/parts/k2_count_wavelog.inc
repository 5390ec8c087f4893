// k2_count_wavelog.inc -- k_count_wavelog: ReadEntry::get_counts on a wavefront's row log; row-log capacity kernels
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.

// ------------------------------------------------------------------------------------------------
// k_count_wavelog: ReadEntry::get_counts (include/read_entry.hpp:92-138) on the row log of one wavefront of
// k_minimise_probe (64 reads).  One workgroup per log; all per-read state lives in LDS.
// ------------------------------------------------------------------------------------------------
struct K2Args {
    const uint64_t *rows;      // escaped full rows
    const uint32_t *rowlog;
    const WaveMeta *wave_meta;
    const uint32_t *wave_count;
    const uint32_t *order;
    uint32_t *counts, *unique;
    uint32_t n_reads, B, C, W;
    uint8_t b2c[256];
    // reads split over a wavefront (k_minimise_probe's SPLIT launch): the first *n_long_ptr entries of `order`; their logs are the
    // wave slots wave_slot0 .. and are counted by k_count_longlog -- k_count_wavelog leaves those reads' rows alone
    const unsigned long long *n_long_ptr;
    uint32_t wave_slot0;
    uint32_t group;            // k_count_wavelog: owners counted per sweep over the log (64, 32, 16 or 8)
    uint32_t chain;            // k_count_wavelog: the logs were written in chain mode (K1Args::chain, rowlog_entry.hpp); k_count_longlog's never are
};

#define K2_THREADS 512
#define K2_UNROLL 4
// T16: totals are 16 bits wide, two to a word (a read of fewer than 2^16 minimisers: the ordinary launch when longer reads go to the SPLIT
// launch).  a.group owners are counted per sweep over the log (64 / a.group sweeps of two passes each; under the probe kernel an XCD's L2 turns
// over between them, so count every sweep as a read of the log from HBM).  The host gives the tables what the probe wavefronts leave of a CU's
// LDS (k2_lds_budget, lds_budget.hpp): at the default k, w and W <= 2 a probe wavefront with a packed ring takes 20 736 B, seven leave 18 688 B,
// and all 64 owners of 100 bins (14 480 B + 256 B static) fit -- one sweep, the log read twice; where the ring is not packed (22 208 B, 8 384 B
// left) 32 owners (7.2 KB) do, as before.  Either way the kernel runs UNDER the next batch's probe kernel instead of waiting for the boundary
// between two of them (the 27 KB of 64 owners x 32-bit totals never fitted).
template <int W, bool T16>
__global__ __launch_bounds__(K2_THREADS) void k_count_wavelog(const K2Args a) {
    extern __shared__ __align__(16) unsigned char smem2[];
    __builtin_amdgcn_s_setprio(3);  // (runs under the next batch's probe kernel: see k_model_call)
    const uint32_t B = a.B, C = a.C, G = a.group;
    const bool chain = a.chain != 0;
    const uint32_t TB = T16 ? (B + 1) / 2 : B;                            // words of totals per owner
    uint32_t *tot = reinterpret_cast<uint32_t *>(smem2);                 // [G][TB] total_bits_per_bin (:96-99)
    uint32_t *unq = tot + (size_t)G * TB;                                // [G][C]
    uint64_t *cmask = reinterpret_cast<uint64_t *>(unq + (size_t)G * C + ((G * C) & 1u));  // [G][W] chosen-bin mask
    uint8_t *chosen = reinterpret_cast<uint8_t *>(cmask + G * W);        // [G][C]
    __shared__ uint8_t s_b2c[256];
    const uint32_t tid = threadIdx.x, g = blockIdx.x;
    const uint32_t n_long = a.n_long_ptr ? (uint32_t)*a.n_long_ptr : 0u;
    if ((g + 1) * WAVE <= n_long) return;  // every lane of this wavefront belongs to a split read: nothing was logged
    if (tid < 256) s_b2c[tid] = a.b2c[tid];
    const uint32_t count = a.wave_count[g];
    const uint64_t *rows = a.rows + a.wave_meta[g].esc_base * W;
    const uint32_t *log = a.rowlog + a.wave_meta[g].base;
    const uint64_t lastmask = (B & 63u) ? ((1ULL << (B & 63u)) - 1) : ~0ULL;
    const uint4 *log4 = reinterpret_cast<const uint4 *>(log);
    const uint32_t count4 = (count + 3) / 4;
    auto bump = [&](uint32_t o, uint32_t b) {
        if (T16) atomicAdd(&tot[o * TB + (b >> 1)], 1u << (16u * (b & 1u)));
        else atomicAdd(&tot[o * TB + b], 1u);
    };
    auto total = [&](uint32_t o, uint32_t b) -> uint32_t { return T16 ? (tot[o * TB + (b >> 1)] >> (16u * (b & 1u))) & 0xffffu : tot[o * TB + b]; };
    // Four compact entries per load and K2_UNROLL loads in flight per thread: the loop is latency-bound per thread, not bandwidth-bound.
    auto sweep = [&](auto f) {
        for (uint32_t i4 = tid; i4 < count4; i4 += K2_THREADS * K2_UNROLL) {
            uint4 v[K2_UNROLL];
#pragma unroll
            for (int u = 0; u < K2_UNROLL; ++u) {
                const uint32_t j = i4 + u * K2_THREADS;
                v[u] = j < count4 ? log4[j] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < K2_UNROLL; ++u) {
                const uint32_t xs[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if ((i4 + u * K2_THREADS) * 4 + q < count) f(xs[q], (i4 + u * K2_THREADS) * 4 + q);
            }
        }
    };
    for (uint32_t o0 = 0; o0 < WAVE; o0 += G) {  // owners o0 .. o0 + G - 1
        __syncthreads();
        for (uint32_t i = tid; i < G * TB; i += K2_THREADS) tot[i] = 0;
        for (uint32_t i = tid; i < G * C; i += K2_THREADS) { unq[i] = 0; chosen[i] = 255; }
        for (uint32_t i = tid; i < G * W; i += K2_THREADS) cmask[i] = 0;
        __syncthreads();
        // pass A: per-bin totals of each read
        sweep([&](uint32_t x, uint32_t) {
            const uint32_t o = (x >> 26) - o0, pc = rowlog_count(x);
            if (o >= G) return;
            if (pc) {  // (both entries of a chained row come by here, each with its own bins)
                bump(o, rowlog_bin(x, 0, chain));
                if (pc > 1) bump(o, rowlog_bin(x, 1, chain));
                if (pc > 2) bump(o, rowlog_bin(x, 2, chain));
            } else if (x & ROWLOG_ESC_MASK) {  // escaped: more set bins than entries can name, full row in the wavefront's escaped-row region
                const size_t j = ((x & ROWLOG_ESC_MASK) >> 2) - 1;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    uint64_t r = rows[j * W + w];
                    if (w == W - 1) r &= lastmask;
                    while (r) {
                        const uint32_t b = (uint32_t)__ffsll((long long)r) - 1;
                        r &= r - 1;
                        bump(o, w * 64 + b);
                    }
                }
            }
        });
        __syncthreads();
        // first bin with the strictly largest total per category (:102-115): one thread per (read, category), bins scanned in
        // ascending order with the running best in registers
        for (uint32_t i = tid; i < G * C; i += K2_THREADS) {
            const uint32_t o = i / C, c = i % C;
            uint32_t best = 255, bestv = 0;
            for (uint32_t b = 0; b < B; ++b) {
                const uint32_t t = total(o, b);
                if (s_b2c[b] == c && (best == 255 || t > bestv)) { best = b; bestv = t; }
            }
            chosen[i] = (uint8_t)best;
            if (best != 255) atomicOr((unsigned long long *)&cmask[o * W + (best >> 6)], 1ULL << (best & 63u));
            const uint32_t gi = g * WAVE + o0 + o;
            if (gi < a.n_reads && gi >= n_long) a.counts[(size_t)a.order[gi] * C + c] = best == 255 ? 0u : bestv;  // a category without bins keeps 0
        }
        __syncthreads();
        // pass B: a minimiser is a unique hit if exactly one category's chosen bin contains it (:121-136)
        sweep([&](uint32_t x, uint32_t e) {
            const uint32_t o = (x >> 26) - o0, pc = rowlog_count(x);
            if (o >= G) return;
            uint32_t found = 0, fbin = 0;
            if (pc) {
                if (rowlog_is_tail(x, chain)) return;  // judged with the entry before it
                auto is_chosen = [&](uint32_t b) -> bool { return (cmask[o * W + (b >> 6)] >> (b & 63u)) & 1ULL; };
                found = rowlog_match(x, chain, is_chosen, fbin);
                // a chained row: its other bins are in the next entry (never read at or beyond `count`: rowlog_tail)
                if (rowlog_has_tail(x, chain)) found += rowlog_match(rowlog_tail(log, e, count, chain), chain, is_chosen, fbin);
            } else if (x & ROWLOG_ESC_MASK) {
                const size_t j = ((x & ROWLOG_ESC_MASK) >> 2) - 1;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const uint64_t r = rows[j * W + w] & cmask[o * W + w];
                    found += (uint32_t)__popcll(r);
                    if (r) fbin = w * 64 + (uint32_t)__ffsll((long long)r) - 1;
                }
            }
            if (found == 1) atomicAdd(&unq[o * C + s_b2c[fbin]], 1u);
        });
        __syncthreads();
        for (uint32_t i = tid; i < G * C; i += K2_THREADS) {
            const uint32_t o = i / C, c = i % C, gi = g * WAVE + o0 + o;
            if (gi < a.n_reads && gi >= n_long) a.unique[(size_t)a.order[gi] * C + c] = unq[i];
        }
    }
}
// The same counts for the reads that k_minimise_probe's SPLIT launch cut over a wavefront: one read per log (every entry has owner
// slot 0), workgroup x takes the reads x, x + gridDim.x, ... of the first *n_long_ptr entries of `order`.
#define K2L_THREADS 256
template <int W>
__global__ __launch_bounds__(K2L_THREADS) void k_count_longlog(const K2Args a) {
    __shared__ uint32_t tot[256], unq[256];
    __shared__ uint64_t cmask[4];
    __shared__ uint8_t s_b2c[256];
    const uint32_t B = a.B, C = a.C, tid = threadIdx.x;
    const uint32_t n_long = a.n_long_ptr ? (uint32_t)*a.n_long_ptr : 0u;
    s_b2c[tid] = a.b2c[tid];
    const uint64_t lastmask = (B & 63u) ? ((1ULL << (B & 63u)) - 1) : ~0ULL;
    for (uint32_t item = blockIdx.x; item < n_long; item += gridDim.x) {
        const uint32_t g = a.wave_slot0 + item, r = a.order[item];
        __syncthreads();
        tot[tid] = 0; unq[tid] = 0;
        if (tid < 4) cmask[tid] = 0;
        __syncthreads();
        const uint32_t count = a.wave_count[g];
        const uint64_t *rows = a.rows + a.wave_meta[g].esc_base * W;
        const uint32_t *log = a.rowlog + a.wave_meta[g].base;
        for (uint32_t e = tid; e < count; e += K2L_THREADS) {  // per-bin totals (include/read_entry.hpp:96-99)
            const uint32_t x = log[e], pc = x & 3u;
            if (pc) {
                atomicAdd(&tot[(x >> 2) & 0xffu], 1u);
                if (pc > 1) atomicAdd(&tot[(x >> 10) & 0xffu], 1u);
                if (pc > 2) atomicAdd(&tot[(x >> 18) & 0xffu], 1u);
            } else if (x & ROWLOG_ESC_MASK) {
                const size_t j = ((x & ROWLOG_ESC_MASK) >> 2) - 1;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    uint64_t rw = rows[j * W + w];
                    if (w == W - 1) rw &= lastmask;
                    while (rw) { const uint32_t b = (uint32_t)__ffsll((long long)rw) - 1; rw &= rw - 1; atomicAdd(&tot[w * 64 + b], 1u); }
                }
            }
        }
        __syncthreads();
        if (tid < C) {  // first bin with the strictly largest total per category (:102-115)
            uint32_t best = 255, bestv = 0;
            for (uint32_t b = 0; b < B; ++b) {
                const uint32_t t = tot[b];
                if (s_b2c[b] == tid && (best == 255 || t > bestv)) { best = b; bestv = t; }
            }
            if (best != 255) atomicOr((unsigned long long *)&cmask[best >> 6], 1ULL << (best & 63u));
            a.counts[(size_t)r * C + tid] = best == 255 ? 0u : bestv;
        }
        __syncthreads();
        for (uint32_t e = tid; e < count; e += K2L_THREADS) {  // unique hits: exactly one category's chosen bin holds the minimiser (:121-136)
            const uint32_t x = log[e], pc = x & 3u;
            uint32_t found = 0, fbin = 0;
            if (pc) {
                for (uint32_t j = 0; j < pc; ++j) {
                    const uint32_t b = (x >> (2 + 8 * j)) & 0xffu;
                    if ((cmask[b >> 6] >> (b & 63u)) & 1ULL) { ++found; fbin = b; }
                }
            } else if (x & ROWLOG_ESC_MASK) {
                const size_t j = ((x & ROWLOG_ESC_MASK) >> 2) - 1;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const uint64_t rw = rows[j * W + w] & cmask[w];
                    found += (uint32_t)__popcll(rw);
                    if (rw) fbin = w * 64 + (uint32_t)__ffsll((long long)rw) - 1;
                }
            }
            if (found == 1) atomicAdd(&unq[s_b2c[fbin]], 1u);
        }
        __syncthreads();
        if (tid < C) a.unique[(size_t)r * C + tid] = unq[tid];
    }
}
// (LDS of one workgroup counting `G` owners at a time: k2_lds_bytes, lds_budget.hpp)

// Deterministic log layout (dense row-sharded mode, chn_minimisers): region sizes per wavefront, then an exclusive scan.
// (The default path lets every k_minimise_probe wavefront claim its region from an atomic cursor instead.)
__global__ void k_wave_caps(const uint32_t *order, const uint32_t *len1, const uint32_t *len2, uint32_t n, uint32_t cap_num, uint32_t esc_shift, WaveMeta *meta) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t v = 0;
    if (i < n) { const uint32_t r = order[i]; v = len1[r] + (len2 ? len2[r] : 0u); }
    const uint64_t sum = wave_sum((uint64_t)v);
    if (lane_id() == 0 && i < n) {
        const uint64_t cap = wave_log_cap(sum, cap_num);
        meta[i / WAVE].base = cap;
        meta[i / WAVE].esc_base = wave_esc_cap(cap, esc_shift);
    }
}
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_meta(WaveMeta *v, uint32_t n) {  // in place exclusive scan of both fields, single workgroup
    array_scan<SCAN_THREADS, uint64_t>(n, [&](uint32_t i) { return v[i].base; }, [&](uint32_t i, uint64_t at) { v[i].base = at; });
    array_scan<SCAN_THREADS, uint64_t>(n, [&](uint32_t i) { return v[i].esc_base; }, [&](uint32_t i, uint64_t at) { v[i].esc_base = at; });
}
// in place exclusive scan of the rows of n values at v, one workgroup a row
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_u64(uint64_t *v, uint32_t n) {
    uint64_t *row = v + (size_t)blockIdx.x * n;
    array_scan<SCAN_THREADS, uint64_t>(n, [&](uint32_t i) { return row[i]; }, [&](uint32_t i, uint64_t at) { row[i] = at; });
}
