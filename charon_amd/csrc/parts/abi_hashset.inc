// abi_hashset.inc -- chn_hashset: a set of 64-bit values that lives in device memory (the minimisers of one bin of `charon index`), and
// the two calls that fill it from a batch and empty it into an index (chn_minimisers_into, chn_index_emplace_set)
// Part of the single translation unit charon_hip.hip (behind abi_shard_wait.inc, whose chn_shard_minimise and shard_args it uses).
//
// Memory rule.  The set owns ONE buffer of `cap` values; `n` of them are in use.  An append that does not fit allocates max(need, 2 * cap)
// values (the need alone where the doubled size is refused), copies device to device and frees the old buffer.  chn_hashset_unique
// allocates its scratch (radix_scratch_bytes: the second key buffer, the counters), sorts, frees whichever of the two key buffers does not
// hold the sorted keys and, the distinct count being known, allocates a buffer of exactly that many values, which becomes the set's;
// everything else is freed before the call returns.  So bytes_held is 8 * cap at any time and 8 * n right behind a unique call, and the
// peak of a unique call is 8 * cap + the scratch.
// Every refusal, a failed allocation included, leaves the set holding the values it held (after a failed unique call possibly sorted).

struct chn_hashset {
    int device = 0;
    uint32_t tile = RADIX_TILE_DEFAULT;
    hipStream_t q = nullptr;
    uint64_t *buf = nullptr;
    uint64_t cap = 0, n = 0;
    bool distinct = true;  // the n values are distinct and ascending: nothing was appended since the last unique call
};

static int hashset_alloc(uint64_t **p, uint64_t values, const char *who) {
    const hipError_t e = hipMalloc((void **)p, values * 8);
    if (e == hipSuccess) return CHN_OK;
    (void)hipGetLastError();
    *p = nullptr;
    return fail(e == hipErrorOutOfMemory ? CHN_E_NOMEM : CHN_E_HIP, std::string(who) + ": " + std::to_string(values * 8) + " bytes of device memory: " + hipGetErrorString(e));
}

// room for `more` values behind the n in use (the device is selected)
static int hashset_reserve(chn_hashset *h, uint64_t more, const char *who) {
    const uint64_t need = h->n + more;
    if (need > radix_max_keys(h->tile))
        return fail(CHN_E_CAPACITY, std::string(who) + ": the set would hold " + std::to_string(need) + " values, more than the " + std::to_string(radix_max_keys(h->tile)) + " it may");
    if (need <= h->cap) return CHN_OK;
    uint64_t *p = nullptr;
    uint64_t cap = std::max(need, 2 * h->cap);
    if (hashset_alloc(&p, cap, who) != CHN_OK) {
        cap = need;
        if (const int rc = hashset_alloc(&p, cap, who)) return rc;
    }
    if (h->n) {
        hipError_t e = hipMemcpyAsync(p, h->buf, h->n * 8, hipMemcpyDeviceToDevice, h->q);
        if (e == hipSuccess) e = hipStreamSynchronize(h->q);
        if (e != hipSuccess) { (void)hipFree(p); return fail(CHN_E_HIP, std::string(who) + ": " + hipGetErrorString(e)); }
    }
    if (h->buf) HIPCHK(hipFree(h->buf));
    h->buf = p; h->cap = cap;
    return CHN_OK;
}

extern "C" int chn_hashset_create(const chn_hashset_cfg *cfg, chn_hashset **out) {
    if (!cfg || !out) return fail(CHN_E_INVALID, "chn_hashset_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(chn_hashset_cfg)) return fail(CHN_E_INVALID, "chn_hashset_create: struct_size mismatch");
    const uint32_t tile = cfg->tile_keys ? cfg->tile_keys : RADIX_TILE_DEFAULT;
    if (!radix_tile_ok(tile))
        return fail(CHN_E_INVALID, "chn_hashset_create: tile_keys " + std::to_string(cfg->tile_keys) + " is not 0 or a multiple of 256 up to " + std::to_string(RADIX_TILE_MAX));
    if (cfg->reserved != 0) return fail(CHN_E_INVALID, "chn_hashset_create: reserved must be 0");
    int count = 0;
    HIPCHK(hipGetDeviceCount(&count));
    if (cfg->device < 0 || cfg->device >= count)
        return fail(CHN_E_INVALID, "chn_hashset_create: device " + std::to_string(cfg->device) + " is not below the device count " + std::to_string(count));
    HIPCHK(hipSetDevice(cfg->device));
    chn_hashset *h = new (std::nothrow) chn_hashset;
    if (!h) return fail(CHN_E_NOMEM, "chn_hashset_create: no memory");
    h->device = cfg->device; h->tile = tile;
    const hipError_t e = hipStreamCreateWithFlags(&h->q, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(CHN_E_HIP, std::string("chn_hashset_create: ") + hipGetErrorString(e)); }
    *out = h;
    return CHN_OK;
}

extern "C" int chn_hashset_destroy(chn_hashset *h) {
    if (!h) return CHN_OK;
    (void)hipSetDevice(h->device);
    if (h->q) { (void)hipStreamSynchronize(h->q); (void)hipStreamDestroy(h->q); }
    if (h->buf) (void)hipFree(h->buf);
    delete h;
    return CHN_OK;
}

extern "C" int chn_hashset_append(chn_hashset *h, const uint64_t *host_values, uint64_t n) {
    if (!h || (!host_values && n)) return fail(CHN_E_INVALID, "chn_hashset_append: null argument");
    if (n == 0) return CHN_OK;
    HIPCHK(hipSetDevice(h->device));
    if (const int rc = hashset_reserve(h, n, "chn_hashset_append")) return rc;
    HIPCHK(hipMemcpy(h->buf + h->n, host_values, n * 8, hipMemcpyHostToDevice));
    h->n += n; h->distinct = false;
    return CHN_OK;
}

extern "C" int chn_hashset_size(const chn_hashset *h, uint64_t *n, uint64_t *bytes_held) {
    if (!h || !n || !bytes_held) return fail(CHN_E_INVALID, "chn_hashset_size: null argument");
    *n = h->n; *bytes_held = h->cap * 8;
    return CHN_OK;
}

extern "C" int chn_hashset_download(const chn_hashset *h, uint64_t first, uint64_t n, uint64_t *host_values) {
    if (!h || (!host_values && n)) return fail(CHN_E_INVALID, "chn_hashset_download: null argument");
    if (first > h->n || n > h->n - first)
        return fail(CHN_E_INVALID, "chn_hashset_download: values [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") of a set of " + std::to_string(h->n));
    if (n == 0) return CHN_OK;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy(host_values, h->buf + first, n * 8, hipMemcpyDeviceToHost));
    return CHN_OK;
}

// The sort of chn_hashset_unique over the n values of h->buf and the count of the distinct ones, all scratch in hand.  *sorted_in is where
// the sorted keys are: h->buf after an even number of passes that ran, alt after an odd one.
static int hashset_sort_count(chn_hashset *h, uint64_t *alt, uint32_t *counts, unsigned long long *tail, uint64_t **sorted_in, uint64_t *distinct) {
    const uint64_t n = h->n;
    const uint32_t tile = h->tile, tiles = (uint32_t)radix_tiles(n, tile);
    unsigned long long *hist = tail, *base = tail + RADIX_PASSES * RADIX_DIGITS, *d_distinct = base + RADIX_DIGITS;
    uint64_t *src = h->buf, *dst = alt;
    HIPCHK(hipMemsetAsync(hist, 0, radix_hist_bytes(), h->q));
    hipLaunchKernelGGL(k_radix_hist, dim3((uint32_t)std::min<uint64_t>(2048, (n + RADIX_THREADS * 16 - 1) / (RADIX_THREADS * 16))), dim3(RADIX_THREADS), 0, h->q, src, n, hist);
    HIPCHK(hipGetLastError());
    std::vector<unsigned long long> host_hist(RADIX_PASSES * RADIX_DIGITS);
    HIPCHK(hipMemcpyAsync(host_hist.data(), hist, radix_hist_bytes(), hipMemcpyDeviceToHost, h->q));
    HIPCHK(hipStreamSynchronize(h->q));
    for (uint32_t p = 0; p < RADIX_PASSES; ++p) {
        bool one_digit = false;  // all keys share this digit: the pass would copy the keys as they lie
        for (uint32_t d = 0; d < RADIX_DIGITS; ++d) one_digit = one_digit || host_hist[p * RADIX_DIGITS + d] == n;
        if (one_digit) continue;
        const uint32_t shift = p * RADIX_BITS;
        hipLaunchKernelGGL(k_radix_count, dim3(tiles), dim3(RADIX_THREADS), 0, h->q, src, n, tile, shift, counts);
        hipLaunchKernelGGL(k_radix_offsets, dim3(RADIX_DIGITS), dim3(RADIX_THREADS), 0, h->q, counts, tiles, hist + p * RADIX_DIGITS, base);
        hipLaunchKernelGGL(k_radix_scatter, dim3(tiles), dim3(RADIX_THREADS), 0, h->q, src, n, tile, shift, counts, base, dst);
        HIPCHK(hipGetLastError());
        std::swap(src, dst);
    }
    hipLaunchKernelGGL(k_unique_count, dim3(tiles), dim3(RADIX_THREADS), 0, h->q, src, n, tile, counts);
    hipLaunchKernelGGL(k_unique_offsets, dim3(1), dim3(RADIX_THREADS), 0, h->q, counts, tiles, d_distinct);
    HIPCHK(hipGetLastError());
    unsigned long long d = 0;
    HIPCHK(hipMemcpyAsync(&d, d_distinct, 8, hipMemcpyDeviceToHost, h->q));
    HIPCHK(hipStreamSynchronize(h->q));
    if (d == 0 || d > n) return fail(CHN_E_HIP, "chn_hashset_unique: internal error: " + std::to_string(d) + " distinct values among " + std::to_string(n));
    *sorted_in = src; *distinct = d;
    return CHN_OK;
}

extern "C" int chn_hashset_unique(chn_hashset *h, uint64_t *n_distinct) {
    if (!h || !n_distinct) return fail(CHN_E_INVALID, "chn_hashset_unique: null argument");
    if (h->distinct || h->n < 2) { h->distinct = true; *n_distinct = h->n; return CHN_OK; }
    HIPCHK(hipSetDevice(h->device));
    const uint64_t n = h->n;
    const uint32_t tiles = (uint32_t)radix_tiles(n, h->tile);
    uint64_t *alt = nullptr, *out = nullptr, *sorted_in = nullptr, distinct = 0;
    uint32_t *counts = nullptr;
    unsigned long long *tail = nullptr;
    int rc = hashset_alloc(&alt, n, "chn_hashset_unique");
    if (rc == CHN_OK) rc = hashset_alloc(reinterpret_cast<uint64_t **>(&counts), radix_counts_bytes(n, h->tile) / 8 + 1, "chn_hashset_unique");
    if (rc == CHN_OK) rc = hashset_alloc(reinterpret_cast<uint64_t **>(&tail), radix_tail_bytes() / 8, "chn_hashset_unique");
    if (rc == CHN_OK) rc = hashset_sort_count(h, alt, counts, tail, &sorted_in, &distinct);
    if (rc == CHN_OK) {
        // the buffer that does not hold the sorted keys goes first: from here on the set owns the sorted keys, whatever follows
        if (sorted_in == alt) { (void)hipFree(h->buf); h->buf = alt; h->cap = n; } else (void)hipFree(alt);
        alt = nullptr;
        rc = hashset_alloc(&out, distinct, "chn_hashset_unique");
    }
    if (rc == CHN_OK) {
        hipLaunchKernelGGL(k_unique_compact, dim3(tiles), dim3(RADIX_THREADS), 0, h->q, h->buf, n, h->tile, counts, distinct, out);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(h->q);
        if (e != hipSuccess) rc = fail(CHN_E_HIP, std::string("chn_hashset_unique: ") + hipGetErrorString(e));
    }
    const std::string why = rc ? g_err : std::string();
    if (rc) (void)hipStreamSynchronize(h->q);  // nothing of a failed call still runs on what is freed here
    if (rc == CHN_OK) { (void)hipFree(h->buf); h->buf = out; h->cap = h->n = distinct; h->distinct = true; }
    else if (out) (void)hipFree(out);
    if (alt) (void)hipFree(alt);
    if (counts) (void)hipFree(counts);
    if (tail) (void)hipFree(tail);
    if (rc) return fail(rc, why);
    *n_distinct = distinct;
    return CHN_OK;
}

extern "C" int chn_minimisers_into(chn_stream *s, const chn_batch *b, chn_hashset *h, uint64_t *n_values) {
    if (!s || !b || !h || !n_values) return fail(CHN_E_INVALID, "chn_minimisers_into: null argument");
    if (s->idx->d.device != h->device)
        return fail(CHN_E_INVALID, "chn_minimisers_into: the stream is on device " + std::to_string(s->idx->d.device) + ", the set on device " + std::to_string(h->device));
    uint64_t total = 0;
    int rc = chn_shard_minimise(s, b, &total);
    if (rc) return rc;
    s->shard_open = false;  // nothing else of the sharded chain follows
    *n_values = total;
    if (total == 0) return CHN_OK;
    if ((rc = hashset_reserve(h, total, "chn_minimisers_into"))) return rc;
    // compact the per-wavefront logs straight behind the set's values
    const Slot &sl = s->slot[s->head];
    const uint32_t n_waves = (uint32_t)waves_of(sl.n_reads);
    const ShardArgs sa = shard_args(s, s->idx, nullptr, sl);
    hipLaunchKernelGGL(k_compact_list, dim3(n_waves), dim3(256), 0, s->q_probe[0], sa, h->buf + h->n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->q_probe[0]));
    h->n += total; h->distinct = false;
    return CHN_OK;
}

extern "C" int chn_index_emplace_set(chn_index *idx, const chn_hashset *h, uint32_t bin) {
    if (!idx || !h) return fail(CHN_E_INVALID, "chn_index_emplace_set: null argument");
    if (bin >= idx->d.bins) return fail(CHN_E_INVALID, "chn_index_emplace_set: bin out of range");
    const chn_index_desc &d = idx->d;
    if (d.device != h->device)
        return fail(CHN_E_INVALID, "chn_index_emplace_set: the index is on device " + std::to_string(d.device) + ", the set on device " + std::to_string(h->device));
    if (h->n == 0) return CHN_OK;
    HIPCHK(hipSetDevice(d.device));
    if (const int rc = index_wait_queued(idx)) return rc;
    hipLaunchKernelGGL(k_emplace_values, dim3((uint32_t)std::min<uint64_t>(65535, (h->n + 255) / 256)), dim3(256), 0, 0, idx->words, h->buf, h->n, bin,
                       d.bin_size, d.row_begin, d.row_end, (uint32_t)d.hash_shift, (uint32_t)d.hash_funs, (uint32_t)d.bin_words);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return CHN_OK;
}

extern "C" int chn_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes) {
    if (!free_bytes || !total_bytes) return fail(CHN_E_INVALID, "chn_device_memory: null argument");
    int count = 0;
    HIPCHK(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(CHN_E_INVALID, "chn_device_memory: device " + std::to_string(device) + " is not below the device count " + std::to_string(count));
    HIPCHK(hipSetDevice(device));
    size_t f = 0, t = 0;
    HIPCHK(hipMemGetInfo(&f, &t));
    *free_bytes = f; *total_bytes = t;
    return CHN_OK;
}
