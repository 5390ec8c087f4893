// abi_synth_memory.inc -- chn_synth_* and pinned / device memory helpers
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.

// ---- synthetic workloads ------------------------------------------------------------------------
extern "C" int chn_synth_genomes(int device, uint64_t seed, uint64_t n_genomes, uint64_t genome_len, uint32_t **dev_bases2) {
    if (!dev_bases2 || genome_len % 64 || n_genomes == 0) return fail(CHN_E_INVALID, "chn_synth_genomes: bad argument");
    HIPCHK(hipSetDevice(device));
    const uint64_t nd = n_genomes * genome_len / 16;
    uint32_t *p = nullptr;
    HIPCHK(hipMalloc((void **)&p, nd * 4));
    hipLaunchKernelGGL(k_synth_genomes, dim3((uint32_t)std::min<uint64_t>(65535, (nd + 255) / 256)), dim3(256), 0, 0, p, nd, seed);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    *dev_bases2 = p;
    return CHN_OK;
}
// pure random row fetches from the index's words: what the chip gives the probe pattern when nothing else is going on.
// U fetches per thread in flight (the default measurement uses 1 and 32 wavefronts per CU; the others are diagnostics:
// CHN_ROOF_UNROLL, CHN_ROOF_BLOCKS_PER_CU, CHN_ROOF_LDS -- how does the rate go with wavefronts per CU and fetches per wavefront?)
template <int W, int NT, int U>
__global__ __launch_bounds__(256) void k_gather_roof(const uint64_t *words, uint64_t rows, uint32_t iters, uint64_t *sink) {
    extern __shared__ unsigned char roof_lds[];  // only its size matters (occupancy diagnostic)
    uint64_t s = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) * 0x9E3779B97F4A7C15ULL + 1;
    uint64_t acc = 0;
    typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));
    for (uint32_t it = 0; it < iters; it += U) {
        ull2 v[U];
        uint64_t v1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // a chain per thread (s -> mix(s)): a counter shared across threads would make neighbours fetch each other's lines one
            // step later and measure the cache instead of the memory system
            uint64_t z = s + 0x9E3779B97F4A7C15ULL;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; z ^= z >> 31;
            s = z;
            const uint64_t *p = words + __umul64hi(z, rows) * W;
            v[u] = ull2{0, 0}; v1[u] = 0;
            if (W >= 2) { const ull2 *q = reinterpret_cast<const ull2 *>(p); v[u] = NT ? __builtin_nontemporal_load(q) : *q; }
            if (W == 4) { const ull2 *q = reinterpret_cast<const ull2 *>(p + 2); const ull2 t = NT ? __builtin_nontemporal_load(q) : *q; v[u].x ^= t.x; v[u].y ^= t.y; }
            if (W & 1) v1[u] = NT ? __builtin_nontemporal_load(p + W - 1) : p[W - 1];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // U fetches in flight per thread: the rate is set by the memory system
#pragma unroll
        for (int u = 0; u < U; ++u) acc ^= v[u].x ^ v[u].y ^ v1[u];
    }
    if (acc == 0x123456789ULL) *sink = acc;
    if (iters == 0xFFFFFFFFu) *sink = roof_lds[threadIdx.x];
}
template <int W, int NT, int U> static void launch_gather_roof_u(uint32_t blocks, size_t lds, const uint64_t *words, uint64_t rows, uint32_t iters, uint64_t *sink) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)k_gather_roof<W, NT, U>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((k_gather_roof<W, NT, U>), dim3(blocks), dim3(256), lds, 0, words, rows, iters, sink);
}
template <int W> static void launch_gather_roof(int nt, int unroll, uint32_t blocks, size_t lds, const uint64_t *words, uint64_t rows, uint32_t iters, uint64_t *sink) {
#define CHN_ROOF_CASE(U) if (unroll == U) { if (nt) launch_gather_roof_u<W, 1, U>(blocks, lds, words, rows, iters, sink); else launch_gather_roof_u<W, 0, U>(blocks, lds, words, rows, iters, sink); return; }
    CHN_ROOF_CASE(2) CHN_ROOF_CASE(4) CHN_ROOF_CASE(6) CHN_ROOF_CASE(12)
#undef CHN_ROOF_CASE
    if (nt) launch_gather_roof_u<W, 1, 1>(blocks, lds, words, rows, iters, sink); else launch_gather_roof_u<W, 0, 1>(blocks, lds, words, rows, iters, sink);
}
extern "C" int chn_index_gather_roof(chn_index *idx, int nt, double *fetches_per_s) {
    if (!idx || !fetches_per_s) return fail(CHN_E_INVALID, "chn_index_gather_roof: null argument");
    HIPCHK(hipSetDevice(idx->d.device));
    const uint32_t W = (uint32_t)idx->d.bin_words;
    uint64_t *sink = nullptr;
    HIPCHK(hipMalloc((void **)&sink, 8));
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
    uint32_t iters = 600, blocks = 256 * 8;
    int unroll = 1;
    size_t lds = 0;
    if (const char *e = diag_env("CHN_ROOF_ITERS")) iters = (uint32_t)std::max(8, std::atoi(e));  // diagnostics
    if (const char *e = diag_env("CHN_ROOF_UNROLL")) unroll = std::atoi(e);
    if (const char *e = diag_env("CHN_ROOF_BLOCKS_PER_CU")) blocks = 256u * (uint32_t)std::max(1, std::atoi(e));
    if (const char *e = diag_env("CHN_ROOF_LDS")) lds = (size_t)std::atol(e);
    iters = iters / 12 * 12;
    if (const char *e = diag_env("CHN_ROOF_MEMSET")) HIPCHK(hipMemset(idx->words, std::atoi(e), idx->rows_local * W * 8));  // diagnostic: DESTROYS the index content
    auto go = [&](uint32_t it) {
        by_words(W, [&](auto w) { launch_gather_roof<decltype(w)::value>(nt, unroll, blocks, lds, idx->words, idx->rows_local, it, sink); });
    };
    go(iters / 12 / 8 * 12 + 12);  // warm-up
    HIPCHK(hipEventRecord(a, 0));
    go(iters);
    HIPCHK(hipEventRecord(b, 0));
    HIPCHK(hipEventSynchronize(b));
    HIPCHK(hipGetLastError());
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a); (void)hipEventDestroy(b); (void)hipFree(sink);
    *fetches_per_s = (double)blocks * 256.0 * iters / (ms * 1e-3);
    return CHN_OK;
}
extern "C" int chn_synth_fill_index(chn_index *idx, uint64_t seed, double density) {
    if (!idx || density < 0 || density > 1) return fail(CHN_E_INVALID, "chn_synth_fill_index: bad argument");
    HIPCHK(hipSetDevice(idx->d.device));
    const uint32_t thr = (uint32_t)std::lround(density * 65536.0);
    hipLaunchKernelGGL(k_synth_fill, dim3(8192), dim3(256), 0, 0, idx->words, idx->rows_local, idx->d.row_begin, (uint32_t)idx->d.bin_words, (uint32_t)idx->d.bins, seed, thr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return CHN_OK;
}
extern "C" int chn_synth_plant(chn_index *idx, const uint32_t *dev_bases2, uint64_t n_genomes, uint64_t genome_len, const uint8_t *genome_bin) {
    if (!idx || !dev_bases2 || !genome_bin || genome_len % 64) return fail(CHN_E_INVALID, "chn_synth_plant: bad argument");
    const chn_index_desc &d = idx->d;
    HIPCHK(hipSetDevice(d.device));
    // The set of minimisers of a sequence equals the union over overlapping chunks (every window lies in one chunk),
    // so genomes are cut into chunks of 4096 bases overlapping by w-1 and each chunk is treated as one "read".
    const uint32_t chunk = 4096, overlap = d.window_size - 1;
    const uint64_t cpg = (genome_len + chunk - 1) / chunk, n = n_genomes * cpg;
    if (n > 0xFFFFFF00ULL) return fail(CHN_E_INVALID, "too many chunks");
    uint64_t *off = nullptr; uint32_t *len = nullptr; uint8_t *bin = nullptr;
    HIPCHK(hipMalloc((void **)&off, n * 8));
    HIPCHK(hipMalloc((void **)&len, n * 4));
    HIPCHK(hipMalloc((void **)&bin, n));
    std::vector<uint8_t> hb(n);
    for (uint64_t i = 0; i < n; ++i) {
        hb[i] = genome_bin[i / cpg];
        if (hb[i] >= d.bins) { (void)hipFree(off); (void)hipFree(len); (void)hipFree(bin); return fail(CHN_E_INVALID, "genome_bin out of range"); }
    }
    HIPCHK(hipMemcpy(bin, hb.data(), n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_chunk_layout, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, 0, n_genomes, genome_len, chunk, overlap, cpg, off, len);
    K1Args a;
    std::memset(&a, 0, sizeof(a));
    a.words = idx->words; a.words_rw = idx->words; a.S = d.bin_size; a.row_begin = d.row_begin; a.row_end = d.row_end; a.seed = d.minimiser_seed; a.powk1 = pow5(d.kmer_size - 1);
    a.shift = (uint32_t)d.hash_shift; a.h = d.hash_funs; a.k = d.kmer_size; a.wn = d.window_size - d.kmer_size + 1;
    a.n_reads = (uint32_t)n; a.nseg = 1; a.B = (uint32_t)d.bins; a.C = d.num_categories;
    a.bases = dev_bases2; a.off1 = off; a.len1 = len; a.read_bin = bin; a.n_bases = n_genomes * genome_len;
    a.pack = ring_pack_ok(a.k, a.wn, a.seed) ? 1u : 0u;
    const size_t lds = k1_lds_bytes(a.wn, d.num_categories, MODE_EMPLACE, a.h, (uint32_t)d.bin_words, (uint32_t)d.bins, a.pack != 0);
    hipError_t e = by_words(d.bin_words, [&](auto w) { return launch_k1_as<decltype(w)::value, MODE_EMPLACE, false, false>(a, lds, 0, 0); });
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipFree(off); (void)hipFree(len); (void)hipFree(bin);
    if (e != hipSuccess) return fail(CHN_E_HIP, std::string("plant: ") + hipGetErrorString(e));
    return CHN_OK;
}
extern "C" int chn_synth_reads(int device, uint64_t seed, const uint32_t *dev_genomes, uint64_t n_genomes, uint64_t genome_len,
                               uint64_t first_read_id, uint64_t n_reads, uint32_t read_len_min, uint32_t read_len_max, double sub_rate, double random_fraction,
                               float mean_quality, chn_synth_reads_out *out) {
    if (!out || n_reads == 0 || read_len_min == 0 || read_len_max < read_len_min) return fail(CHN_E_INVALID, "chn_synth_reads: bad argument");
    if (n_genomes && (!dev_genomes || genome_len < read_len_max)) return fail(CHN_E_INVALID, "genomes shorter than reads");
    HIPCHK(hipSetDevice(device));
    std::memset(out, 0, sizeof(*out));
    uint64_t *d_total = nullptr;
    HIPCHK(hipMalloc((void **)&out->seg1_length, n_reads * 4));
    HIPCHK(hipMalloc((void **)&out->seg1_offset, n_reads * 8));
    HIPCHK(hipMalloc((void **)&out->mean_quality, n_reads * 4));
    HIPCHK(hipMalloc((void **)&out->compression, n_reads * 4));
    HIPCHK(hipMalloc((void **)&d_total, 8));
    const dim3 g1((uint32_t)((n_reads + 255) / 256)), b1(256);
    hipLaunchKernelGGL(k_synth_read_layout, g1, b1, 0, 0, seed, first_read_id, n_reads, read_len_min, read_len_max, out->seg1_length);
    uint64_t total = 0;
    if (read_len_min == read_len_max) {
        const uint64_t pad = ((uint64_t)read_len_min + 63) & ~63ULL;
        std::vector<uint64_t> h(n_reads);
        for (uint64_t i = 0; i < n_reads; ++i) h[i] = i * pad;
        HIPCHK(hipMemcpy(out->seg1_offset, h.data(), n_reads * 8, hipMemcpyHostToDevice));
        total = n_reads * pad;
    } else {
        hipLaunchKernelGGL(k_synth_offsets, dim3(1), dim3(64), 0, 0, out->seg1_length, n_reads, out->seg1_offset, d_total);
        HIPCHK(hipMemcpy(&total, d_total, 8, hipMemcpyDeviceToHost));
    }
    (void)hipFree(d_total);
    out->n_bases = total;
    HIPCHK(hipMalloc((void **)&out->bases2, total / 4 + 16));
    HIPCHK(hipMemset(out->bases2, 0, total / 4 + 16));
    hipLaunchKernelGGL(k_fill_f32, g1, b1, 0, 0, out->mean_quality, n_reads, mean_quality);
    hipLaunchKernelGGL(k_fill_f32, g1, b1, 0, 0, out->compression, n_reads, 0.3f);
    SynthReadsArgs a;
    a.genomes = dev_genomes; a.n_genomes = n_genomes; a.genome_len = genome_len; a.seed = seed; a.n_reads = n_reads; a.first_id = first_read_id;
    a.len_min = read_len_min; a.len_max = read_len_max;
    a.sub_thr32 = (uint32_t)std::min<double>(4294967295.0, sub_rate * 4294967296.0);
    a.rand_thr32 = (uint32_t)std::min<double>(4294967295.0, random_fraction * 4294967296.0);
    a.bases = out->bases2; a.off = out->seg1_offset; a.len = out->seg1_length;
    const uint32_t gy = (uint32_t)std::min<uint64_t>(n_reads, 32768), gz = (uint32_t)((n_reads + gy - 1) / gy);
    const uint32_t max_dwords = (read_len_max + 63) / 64 * 4;
    hipLaunchKernelGGL(k_synth_reads, dim3((max_dwords + 63) / 64, gy, gz), dim3(64), 0, 0, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return CHN_OK;
}
extern "C" int chn_host_alloc(uint64_t bytes, void **ptr) {
    if (!ptr) return fail(CHN_E_INVALID, "null argument");
    HIPCHK(hipHostMalloc(ptr, bytes ? bytes : 16, hipHostMallocDefault));
    return CHN_OK;
}
extern "C" int chn_host_free(void *ptr) {
    if (ptr) HIPCHK(hipHostFree(ptr));
    return CHN_OK;
}
extern "C" int chn_device_malloc(int device, uint64_t bytes, void **ptr) {
    if (!ptr) return fail(CHN_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipMalloc(ptr, bytes ? bytes : 16));
    return CHN_OK;
}
extern "C" int chn_device_upload(int device, void *dev_dst, const void *host_src, uint64_t bytes) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipMemcpy(dev_dst, host_src, bytes, hipMemcpyHostToDevice));
    return CHN_OK;
}
extern "C" int chn_device_free(int device, void *ptr) {
    HIPCHK(hipSetDevice(device));
    if (ptr) HIPCHK(hipFree(ptr));
    return CHN_OK;
}
extern "C" int chn_device_download(int device, void *host_dst, const void *dev_src, uint64_t bytes) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost));
    return CHN_OK;
}
