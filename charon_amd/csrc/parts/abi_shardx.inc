// abi_shardx.inc -- sparse row-sharded entry points (chn_shardx_*): query / response exchange between the ranks that own the rows
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.

extern "C" int chn_shardx_minimise(chn_stream *s, const chn_batch *b) {
    if (!s || !b) return fail(CHN_E_INVALID, "chn_shardx_minimise: null argument");
    if (s->shx_stage != 0 || s->shard_open) return fail(CHN_E_STATE, "chn_shardx_minimise: previous sharded batch not finished");
    HIPCHK(hipSetDevice(s->idx->d.device));
    const uint64_t nw = waves_of(s->cfg.max_reads);
    int rc;
    // density-sized regions (as the per-slot logs of the replica path); an overrun is reported by chn_shardx_counts, not re-run
    if ((rc = s->shx.ensure(s->cfg.max_bases, nw, (uint32_t)s->idx->d.bin_words, s->cap_num, s->esc_shift))) return rc;
    if ((rc = s->d_list.ensure(s->shx.log_cap * 8))) return rc;
    if ((rc = submit_impl(s, b, LIST_SPARSE))) return rc;
    s->shx_stage = 1;
    return CHN_OK;
}

extern "C" int chn_shardx_counts(chn_stream *s, uint32_t n_ranks, const uint64_t *row_splits, uint64_t *n_probes, uint64_t *send_counts) {
    if (!s || !row_splits || !n_probes || !send_counts) return fail(CHN_E_INVALID, "chn_shardx_counts: null argument");
    if (s->shx_stage != 1) return fail(CHN_E_STATE, "chn_shardx_counts: call chn_shardx_minimise first");
    if (n_ranks < 1 || n_ranks > SHX_MAX_RANKS) return fail(CHN_E_INVALID, "chn_shardx_counts: 1..16 ranks");
    const chn_index_desc &d = s->idx->d;
    if (row_splits[0] != 0 || row_splits[n_ranks] != d.bin_size) return fail(CHN_E_INVALID, "chn_shardx_counts: row_splits must cover [0, bin_size)");
    for (uint32_t r = 0; r < n_ranks; ++r)
        if (row_splits[r] > row_splits[r + 1] || row_splits[r + 1] - row_splits[r] > 0xFFFFFFFFULL)
            return fail(CHN_E_INVALID, "chn_shardx_counts: row_splits must ascend and a shard may hold at most 2^32 - 1 rows");
    HIPCHK(hipSetDevice(d.device));
    Slot &sl = s->slot[s->head];
    const uint32_t n_waves = (uint32_t)waves_of(sl.n_reads);
    int rc;
    if ((rc = s->d_shx_cnt.ensure((size_t)n_ranks * (n_waves + 1) * 8))) return rc;
    ShxArgs &a = s->shx_args;
    std::memset(&a, 0, sizeof a);
    a.list = s->d_list.as<uint64_t>(); a.wave_meta = s->shx.meta.as<WaveMeta>(); a.wave_count = s->shx.wcount.as<uint32_t>();
    a.n_waves = n_waves; a.n_ranks = n_ranks; a.h = d.hash_funs; a.shift = (uint32_t)d.hash_shift; a.S = d.bin_size;
    for (uint32_t r = 0; r <= n_ranks; ++r) a.splits[r] = row_splits[r];
    a.cnt = s->d_shx_cnt.as<uint64_t>();
    a.rowlog = s->shx.log.as<uint32_t>(); a.rows = s->shx.rows.as<uint64_t>(); a.esc_capacity = s->shx.esc_cap;
    a.status = reinterpret_cast<uint32_t *>(sl.d_ctl.as<unsigned long long>() + CTL_STATUS); a.B = (uint32_t)d.bins;
    hipLaunchKernelGGL(k_shx_count, dim3(n_waves), dim3(SHX_THREADS), 0, s->q_probe[0], a);
    hipLaunchKernelGGL(k_scan_u64, dim3(n_ranks), dim3(SCAN_THREADS), 0, s->q_probe[0], a.cnt, n_waves + 1);
    HIPCHK(hipGetLastError());
    std::vector<uint64_t> tot(n_ranks);
    for (uint32_t r = 0; r < n_ranks; ++r)
        HIPCHK(hipMemcpyAsync(&tot[r], a.cnt + (size_t)r * (n_waves + 1) + n_waves, 8, hipMemcpyDeviceToHost, s->q_probe[0]));
    unsigned long long st = 0;
    HIPCHK(hipMemcpyAsync(&st, sl.d_ctl.as<unsigned long long>() + CTL_STATUS, 8, hipMemcpyDeviceToHost, s->q_probe[0]));
    HIPCHK(hipStreamSynchronize(s->q_probe[0]));
    if (st & 2) { s->shx_stage = 0; return fail(CHN_E_INVALID, "a segment of the batch is misaligned or lies outside the base buffer"); }
    if (st & 1) { s->shx_stage = 0; return fail(CHN_E_CAPACITY, "minimiser log overflow in the sparse row-sharded chain: submit the reads in smaller batches or create the stream with a larger max_bases"); }
    uint64_t run = 0;
    for (uint32_t r = 0; r < n_ranks; ++r) { a.send_base[r] = run; send_counts[r] = tot[r]; run += tot[r]; }
    a.send_base[n_ranks] = run;
    *n_probes = run;
    s->shard_entries = run;
    s->shx_stage = 2;
    return CHN_OK;
}

extern "C" int chn_shardx_queries(chn_stream *s, uint32_t *dev_queries, uint64_t capacity) {
    if (!s || (!dev_queries && capacity)) return fail(CHN_E_INVALID, "chn_shardx_queries: null argument");
    if (s->shx_stage != 2) return fail(CHN_E_STATE, "chn_shardx_queries: call chn_shardx_counts first");
    if (capacity < s->shard_entries) return fail(CHN_E_CAPACITY, "chn_shardx_queries: query buffer too small");
    HIPCHK(hipSetDevice(s->idx->d.device));
    ShxArgs a = s->shx_args;
    a.queries = dev_queries;
    hipLaunchKernelGGL(k_shx_scatter, dim3(a.n_waves), dim3(SHX_THREADS), 0, s->q_probe[0], a);
    HIPCHK(hipGetLastError());
    s->shx_stage = 3;
    return CHN_OK;
}

extern "C" int chn_shardx_serve(chn_stream *s, const chn_index *shard, const uint32_t *dev_queries_in, uint64_t n_in, uint64_t *dev_rows_out) {
    if (!s || !shard || (n_in && (!dev_queries_in || !dev_rows_out))) return fail(CHN_E_INVALID, "chn_shardx_serve: null argument");
    if (shard->d.device != s->idx->d.device) return fail(CHN_E_INVALID, "chn_shardx_serve: shard lives on another device");
    if (n_in == 0) return CHN_OK;
    HIPCHK(hipSetDevice(shard->d.device));
    Slot &sl = s->slot[s->head];
    uint32_t *status = reinterpret_cast<uint32_t *>(sl.d_ctl.as<unsigned long long>() + CTL_STATUS);
    // Two workgroups (eight wavefronts) per CU, each looping over its share of the queries: enough loads in flight to reach the device's
    // random-fetch rate (profiles/r02/gather_roof_sweep.txt: 4 wavefronts per CU already do), and the CU's other wave slots stay free for
    // the next batch's minimise kernel, which the caller queues beside this one (a grid of 16 384 workgroups filled every slot: 59 -> 54 ms
    // per step at N = 1).  CHN_SERVE_BLOCKS overrides (diagnostic).
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, shard->d.device);
    static const long serve_blocks_env = []() { const char *e = diag_env("CHN_SERVE_BLOCKS"); return e ? std::atol(e) : 0L; }();
    const uint64_t serve_blocks = serve_blocks_env > 0 ? (uint64_t)serve_blocks_env : (uint64_t)std::max(1, cus) * 2;
    const dim3 grid((uint32_t)std::min<uint64_t>((n_in + 255) / 256, serve_blocks)), block(256);
    by_words(shard->d.bin_words, [&](auto w) { hipLaunchKernelGGL(k_shx_serve<decltype(w)::value>, grid, block, 0, s->q_probe[0], shard->words, dev_queries_in, n_in, shard->rows_local, dev_rows_out, status); });
    HIPCHK(hipGetLastError());
    return CHN_OK;
}

extern "C" int chn_shardx_finish(chn_stream *s, const uint64_t *dev_rows_back) {
    if (!s || (!dev_rows_back && s->shard_entries)) return fail(CHN_E_INVALID, "chn_shardx_finish: null argument");
    if (s->shx_stage != 3) return fail(CHN_E_STATE, "chn_shardx_finish: call chn_shardx_queries first");
    HIPCHK(hipSetDevice(s->idx->d.device));
    Slot &sl = s->slot[s->head];
    ShxArgs a = s->shx_args;
    a.resp = dev_rows_back;
    by_words(s->idx->d.bin_words, [&](auto w) { hipLaunchKernelGGL(k_shx_and<decltype(w)::value>, dim3(a.n_waves), dim3(SHX_THREADS), 0, s->q_probe[0], a); });
    HIPCHK(hipGetLastError());
    s->shx_stage = 0;
    HIPCHK(hipEventRecord(sl.k1_done, s->q_probe[0]));
    HIPCHK(hipStreamWaitEvent(s->q_side, sl.k1_done, 0));
    int rc = launch_tail(s, sl, s->shx, TAIL_BATCH);
    if (rc) return rc;
    s->head = (s->head + 1) % chn_stream::N_SLOTS;
    s->inflight += 1;
    return CHN_OK;
}
