// abi_shard_wait.inc -- row-sharded entry points, chn_minimisers / chn_index_emplace, chn_batch_wait, chn_classify_counts, profiling
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.

// ---- row-sharded mode -----------------------------------------------------------------------------
// A slot's status word (CTL_STATUS) as an error.  What an overflow of the row log (bit 1) means is the caller's to say; null: the
// caller deals with it (chn_batch_wait re-runs the batch).  chn_shard_minimise hands in bits 1 and 2 only, the two it has always tested.
static int status_error(unsigned long long status, const char *overflow) {
    if (status & 2) return fail(CHN_E_INVALID, "a segment of the batch is misaligned or lies outside the base buffer");
    if (status & 4)  // k_shx_serve answered such a query with row 0: the counts of whoever asked are wrong
        return fail(CHN_E_INVALID, "chn_shardx_serve was asked for rows this shard does not hold: the queries were built from other row_splits than the shards' "
                                   "(or went to the wrong owner)");
    if ((status & 1) && overflow) return fail(CHN_E_CAPACITY, overflow);
    return CHN_OK;
}

static int ensure_shard_buffers(chn_stream *s) {
    // the dense row-sharded chain cannot be re-run behind the caller's collective, so it is laid out for the worst case
    // (one minimiser per base, every row escaped), deterministically
    const uint64_t nw = waves_of(s->cfg.max_reads);
    int rc;
    if ((rc = s->big.ensure(s->cfg.max_bases, nw, (uint32_t)s->idx->d.bin_words, 65536, 0))) return rc;
    if ((rc = s->d_list.ensure(s->big.log_cap * 8)) || (rc = s->d_cbase.ensure((nw + 1) * 8))) return rc;
    return CHN_OK;
}
static ShardArgs shard_args(chn_stream *s, const chn_index *shard, uint64_t *partial, const Slot &sl) {
    ShardArgs a;
    std::memset(&a, 0, sizeof a);
    const chn_index_desc &d = shard->d;
    a.list = s->d_list.as<uint64_t>(); a.wave_meta = s->big.meta.as<WaveMeta>(); a.cbase = s->d_cbase.as<uint64_t>();
    a.wave_count = s->big.wcount.as<uint32_t>(); a.words = shard->words; a.S = d.bin_size; a.row_begin = d.row_begin; a.row_end = d.row_end;
    a.shift = (uint32_t)d.hash_shift; a.h = d.hash_funs; a.W = (uint32_t)d.bin_words; a.partial = partial; a.rows = s->big.rows.as<uint64_t>();
    a.rowlog = s->big.log.as<uint32_t>(); a.B = (uint32_t)d.bins;
    a.n_waves = (uint32_t)waves_of(sl.n_reads); a.esc_capacity = s->big.esc_cap;
    a.status = reinterpret_cast<uint32_t *>(const_cast<Slot &>(sl).d_ctl.as<unsigned long long>() + CTL_STATUS);
    return a;
}

extern "C" int chn_shard_minimise(chn_stream *s, const chn_batch *b, uint64_t *n_entries) {
    if (!s || !b || !n_entries) return fail(CHN_E_INVALID, "chn_shard_minimise: null argument");
    if (s->shard_open || s->shx_stage != 0) return fail(CHN_E_STATE, "chn_shard_minimise: previous sharded batch not finished");  // (it would take the open batch's slot)
    HIPCHK(hipSetDevice(s->idx->d.device));
    int rc = ensure_shard_buffers(s);
    if (rc) return rc;
    if ((rc = submit_impl(s, b, LIST_DENSE))) return rc;
    const uint32_t n_waves = (uint32_t)waves_of(b->n_reads);
    hipLaunchKernelGGL(k_counts_to_u64, dim3((n_waves + 1 + 255) / 256), dim3(256), 0, s->q_probe[0], s->big.wcount.as<uint32_t>(), n_waves, s->d_cbase.as<uint64_t>());
    hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(SCAN_THREADS), 0, s->q_probe[0], s->d_cbase.as<uint64_t>(), n_waves + 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->q_probe[0]));
    uint64_t total = 0;
    HIPCHK(hipMemcpy(&total, s->d_cbase.as<uint64_t>() + n_waves, 8, hipMemcpyDeviceToHost));
    unsigned long long st = 0;
    HIPCHK(hipMemcpy(&st, s->slot[s->head].d_ctl.as<unsigned long long>() + CTL_STATUS, 8, hipMemcpyDeviceToHost));
    if ((rc = status_error(st & 3, "minimiser log overflow (batch larger than the stream's max_bases?)"))) return rc;
    s->shard_entries = total;
    s->shard_open = true;
    *n_entries = total;
    return CHN_OK;
}

extern "C" int chn_minimisers(chn_stream *s, const chn_batch *b, uint64_t *host_values, uint64_t capacity, uint64_t *n_values) {
    if (!s || !b || !n_values) return fail(CHN_E_INVALID, "chn_minimisers: null argument");
    uint64_t total = 0;
    int rc = chn_shard_minimise(s, b, &total);
    if (rc) return rc;
    s->shard_open = false;  // nothing else of the sharded chain follows
    *n_values = total;
    if (total == 0) return CHN_OK;
    if (!host_values || capacity < total) return fail(CHN_E_CAPACITY, "chn_minimisers: output buffer too small (need " + std::to_string(total) + " values)");
    // compact the per-wavefront logs into the (unused here) escaped-row buffer, then copy out
    if ((rc = s->big.rows.ensure(total * 8))) return rc;
    const Slot &sl = s->slot[s->head];
    const uint32_t n_waves = (uint32_t)waves_of(sl.n_reads);
    const ShardArgs sa = shard_args(s, s->idx, nullptr, sl);
    hipLaunchKernelGGL(k_compact_list, dim3(n_waves), dim3(256), 0, s->q_probe[0], sa, s->big.rows.as<uint64_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host_values, s->big.rows.p, total * 8, hipMemcpyDeviceToHost, s->q_probe[0]));
    HIPCHK(hipStreamSynchronize(s->q_probe[0]));
    return CHN_OK;
}

extern "C" int chn_index_emplace(chn_index *idx, const uint64_t *host_values, uint64_t n_values, uint32_t bin) {
    if (!idx || (!host_values && n_values)) return fail(CHN_E_INVALID, "chn_index_emplace: null argument");
    if (bin >= idx->d.bins) return fail(CHN_E_INVALID, "chn_index_emplace: bin out of range");
    if (n_values == 0) return CHN_OK;
    const chn_index_desc &d = idx->d;
    HIPCHK(hipSetDevice(d.device));
    if (const int rc = index_wait_queued(idx)) return rc;
    uint64_t *dv = nullptr;
    const uint64_t chunk = 1ULL << 26;  // 512 MiB of values at a time
    HIPCHK(hipMalloc((void **)&dv, std::min(chunk, n_values) * 8));
    for (uint64_t o = 0; o < n_values; o += chunk) {
        const uint64_t m = std::min(chunk, n_values - o);
        hipError_t e = hipMemcpy(dv, host_values + o, m * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_emplace_values, dim3((uint32_t)std::min<uint64_t>(65535, (m + 255) / 256)), dim3(256), 0, 0, idx->words, dv, m, bin,
                               d.bin_size, d.row_begin, d.row_end, (uint32_t)d.hash_shift, (uint32_t)d.hash_funs, (uint32_t)d.bin_words);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) { (void)hipFree(dv); return fail(CHN_E_HIP, std::string("chn_index_emplace: ") + hipGetErrorString(e)); }
    }
    HIPCHK(hipFree(dv));
    return CHN_OK;
}

extern "C" int chn_shard_probe(chn_stream *s, const chn_index *shard, uint64_t *dev_partial, uint64_t capacity_words) {
    if (!s || !shard) return fail(CHN_E_INVALID, "chn_shard_probe: null argument");
    if (!s->shard_open) return fail(CHN_E_STATE, "chn_shard_probe: call chn_shard_minimise first");
    if (!dev_partial && s->shard_entries) return fail(CHN_E_INVALID, "chn_shard_probe: null argument");  // (a batch without a minimiser has no partial words)
    const chn_index_desc &a = s->idx->d, &c = shard->d;
    if (a.bin_size != c.bin_size || a.bin_words != c.bin_words || a.hash_funs != c.hash_funs || a.device != c.device)
        return fail(CHN_E_INVALID, "chn_shard_probe: shard does not belong to the stream's index");
    if (capacity_words < s->shard_entries * c.hash_funs * c.bin_words) return fail(CHN_E_CAPACITY, "chn_shard_probe: partial buffer too small");
    HIPCHK(hipSetDevice(a.device));
    const Slot &sl = s->slot[s->head];
    const uint32_t n_waves = (uint32_t)waves_of(sl.n_reads);
    const ShardArgs sa = shard_args(s, shard, dev_partial, sl);
    by_words(c.bin_words, [&](auto w) { hipLaunchKernelGGL(k_probe_partial<decltype(w)::value>, dim3(n_waves), dim3(256), 0, s->q_probe[0], sa); });
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->q_probe[0]));  // the caller's collective runs on its own stream
    return CHN_OK;
}

extern "C" int chn_shard_finish(chn_stream *s, const uint64_t *dev_partial) {
    if (!s) return fail(CHN_E_INVALID, "chn_shard_finish: null argument");
    if (!s->shard_open) return fail(CHN_E_STATE, "chn_shard_finish: no sharded batch open");
    if (!dev_partial && s->shard_entries) return fail(CHN_E_INVALID, "chn_shard_finish: null argument");
    HIPCHK(hipSetDevice(s->idx->d.device));
    Slot &sl = s->slot[s->head];
    const uint32_t n_waves = (uint32_t)waves_of(sl.n_reads);
    const ShardArgs sa = shard_args(s, s->idx, const_cast<uint64_t *>(dev_partial), sl);
    by_words(s->idx->d.bin_words, [&](auto w) { hipLaunchKernelGGL(k_and_partial<decltype(w)::value>, dim3(n_waves), dim3(256), 0, s->q_probe[0], sa); });
    HIPCHK(hipGetLastError());
    s->shard_open = false;
    HIPCHK(hipEventRecord(sl.k1_done, s->q_probe[0]));
    HIPCHK(hipStreamWaitEvent(s->q_side, sl.k1_done, 0));
    int rc = launch_tail(s, sl, s->big, TAIL_BATCH);
    if (rc) return rc;
    s->head = (s->head + 1) % chn_stream::N_SLOTS;
    s->inflight += 1;
    return CHN_OK;
}

extern "C" int chn_stream_sync(chn_stream *s) {
    if (!s) return fail(CHN_E_INVALID, "null stream");
    HIPCHK(hipSetDevice(s->idx->d.device));
    for (const StreamRole &r : stream_roles(s)) if (r.synced) HIPCHK(hipStreamSynchronize(*r.q));
    return CHN_OK;
}

// A wavefront's log region (sized for twice the minimiser density of random sequence) overflowed: run the batch again on the
// stream's worst-case buffers (one entry per base, every row escaped), synchronously.  Inputs are still in place: host batches
// sit in the slot's staging, device batches are owned by the caller until chn_batch_wait returns.
// Later batches may be running meanwhile, on either probe stream and on the side stream: they work on their own slots (control words,
// order, row log, results) and on the caller's or their slot's inputs; s->big belongs to this call (the list modes, its other users,
// refuse to run with batches in flight), and s->d_hist is only touched by the ordering kernels on the copy stream, which do not run here.
static int rerun_worst_case(chn_stream *s, Slot &sl) {
    const chn_index_desc &d = s->idx->d;
    unsigned long long *ctl = sl.d_ctl.as<unsigned long long>();
    const uint64_t n = sl.n_reads, nw = waves_of(n) + sl.split_bound;
    HIPCHK(hipMemsetAsync(ctl, 0, CTL_NLONG * 8, s->q_probe[0]));  // (the number of split reads stays)
    HIPCHK(hipMemsetAsync(ctl + CTL_FETCHES, 0, (CTL_WORDS - CTL_FETCHES) * 8, s->q_probe[0]));
    hipLaunchKernelGGL(k_sum_len, dim3((uint32_t)std::min<uint64_t>(1024, (n + 255) / 256)), dim3(256), 0, s->q_probe[0], sl.len1, sl.len2, (uint32_t)n, ctl + CTL_SUM_LEN);
    HIPCHK(hipGetLastError());
    unsigned long long total = 0;
    HIPCHK(hipMemcpyAsync(&total, ctl + CTL_SUM_LEN, 8, hipMemcpyDeviceToHost, s->q_probe[0]));
    HIPCHK(hipStreamSynchronize(s->q_probe[0]));
    int rc = s->big.ensure(total, waves_of(n) + std::min<uint64_t>(sl.split_bound, total / len_bucket_floor(std::min(s->long_bucket, 247u)) + 1), (uint32_t)d.bin_words, 65536, 0, nw);
    if (rc) return rc;
    sl.k1.chain = 0;  // worst-case regions are one entry per base: no chained second entries (launch_tail reads the flag from the slot)
    K1Args a = sl.k1;
    a.gate_started = a.gate_signal = nullptr;  // no probe gate: the slot's counter has counted this grid once already, and nothing waits for it
    fill_k1_log(a, sl, s->big, true);
    const size_t lds = k1_rows_lds(d);
    hipError_t e = launch_k1(MODE_ROWS, (uint32_t)d.bin_words, a, lds, s->q_probe[0]);
    if (e == hipSuccess && sl.split_bound) e = launch_k1(MODE_ROWS, (uint32_t)d.bin_words, a, lds, s->q_probe[0], split_grid(sl.split_bound));
    if (e != hipSuccess) return fail(CHN_E_HIP, std::string("k_minimise_probe re-run: ") + hipGetErrorString(e));
    if ((rc = launch_tail(s, sl, s->big, TAIL_RERUN))) return rc;
    HIPCHK(hipStreamSynchronize(s->q_probe[0]));
    s->overflow_reruns += 1;
    return CHN_OK;
}

// Profiling streams, at a batch's wait: its brackets' times into the stream's sums.
// The probe kernel counts only with what lies behind the end of the probe kernels before it (they overlap, on two streams) -- the sum
// over batches is the time some probe kernel was running, and one batch at a time gives the bracket time.  That end is kept as
// milliseconds behind the stream's time anchor (chn_stream::prof_anchor); a batch behind whose probe kernel the next anchor was
// recorded moves the stream on to it.
static int prof_collect(chn_stream *s, Slot &sl) {
    const EvBracket *const brackets[4] = {&sl.t_probe, &sl.t_count, &sl.t_model, &sl.t_chain};  // PROF_PROBE .. PROF_CHAIN
    for (int i = 0; i < 4; ++i) {
        const EvBracket &t = *brackets[i];
        if (!t.used) continue;
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, t.begin, t.end));
        if (i == PROF_PROBE) {
            float t0 = 0, t1 = 0;
            HIPCHK(hipEventElapsedTime(&t0, s->prof_anchor[s->prof_cur], t.begin));
            HIPCHK(hipEventElapsedTime(&t1, s->prof_anchor[s->prof_cur], t.end));
            if (s->prof_have_end && s->prof_prev_end > (double)t0) ms = (float)std::max(0.0, (double)t1 - s->prof_prev_end);
            if (!s->prof_have_end || (double)t1 > s->prof_prev_end) s->prof_prev_end = t1;
            s->prof_have_end = true;
            if (sl.new_anchor) {
                float off = 0;
                HIPCHK(hipEventElapsedTime(&off, s->prof_anchor[s->prof_cur], s->prof_anchor[s->prof_cur ^ 1]));
                s->prof_prev_end -= off; s->prof_cur ^= 1;
                sl.new_anchor = s->prof_anchor_pending = false;
            }
        }
        s->prof_ms[i] += ms; s->prof_n[i] += 1;
    }
    return CHN_OK;
}

// one result column into the caller's memory: from the slot's page-locked copy, filled in stream, or (null) from the device
static int copy_out(void *dst, const void *staged, const void *dev, size_t bytes) {
    if (staged) std::memcpy(dst, staged, bytes);
    else HIPCHK(hipMemcpy(dst, dev, bytes, hipMemcpyDeviceToHost));
    return CHN_OK;
}

// CHN_DIAG_WAIT: one line per chn_batch_wait, printed as the call returns
struct WaitDiag {
    bool on;
    double at, done, gz;
    ~WaitDiag() { if (on) std::fprintf(stderr, "chn_batch_wait: at %.4f  done-event %.2f ms  gz-event %.2f ms  rest %.2f ms\n", at, (done - at) * 1e3, (gz - done) * 1e3, (wall_now() - gz) * 1e3); }
};

extern "C" int chn_batch_wait(chn_stream *s, chn_result *r) {
    if (!s || !r || r->struct_size != sizeof(chn_result)) return fail(CHN_E_INVALID, "chn_batch_wait: bad argument");
    if (s->inflight == 0) return fail(CHN_E_STATE, "no batch in flight");
    HIPCHK(hipSetDevice(s->idx->d.device));
    Slot &sl = s->slot[(s->head + chn_stream::N_SLOTS - s->inflight) % chn_stream::N_SLOTS];  // oldest batch in flight
    static const bool diag_wait = diag_env("CHN_DIAG_WAIT") != nullptr;
    const double at = diag_wait ? wall_now() : 0;
    HIPCHK(hipEventSynchronize(sl.done));
    const double done = diag_wait ? wall_now() : 0;
    if (sl.want_gzt) HIPCHK(hipEventSynchronize(sl.gz_done));
    const WaitDiag diag{diag_wait, at, done, diag_wait ? wall_now() : 0};
    s->inflight -= 1;
    int rc = prof_collect(s, sl);
    if (rc) return rc;
    unsigned long long ctl[CTL_WORDS];
    const uint64_t n = sl.n_reads, C = s->idx->d.num_categories;
    const ResLayout L(n, C);
    const char *staged = sl.staged ? sl.h_res.as<char>() : nullptr;  // the slot's page-locked copy, filled in stream
    if ((rc = copy_out(ctl, staged ? staged + L.ctl : nullptr, sl.d_ctl.p, sizeof ctl))) return rc;
    if ((rc = status_error(ctl[CTL_STATUS], sl.list_mode ? "row log overflow in the row-sharded chain" : nullptr))) return rc;
    if (ctl[CTL_STATUS] & 1) {
        if ((rc = rerun_worst_case(s, sl))) return rc;
        staged = nullptr;  // the re-run's results are in the device arrays only
        if ((rc = copy_out(ctl, nullptr, sl.d_ctl.p, sizeof ctl))) return rc;
        if (ctl[CTL_STATUS] & 1) return fail(CHN_E_CAPACITY, "row log overflow at worst-case capacity (a wavefront of 64 reads with more than 2^24 escaped rows)");
    }
    s->last_bytes = ctl[CTL_BYTES]; s->last_min = ctl[CTL_MINIMISERS]; s->last_fetches = ctl[CTL_FETCHES];
    if (!sl.list_mode) s->last_had_long = ctl[CTL_NLONG] != 0;  // (decides the next batches' probe stream: pick_probe_stream)
    if (r->on_device) {  // valid until the third-next chn_batch_submit
        r->num_hashes = sl.d_num_hashes.as<uint32_t>(); r->counts = sl.d_counts.as<uint32_t>(); r->unique_counts = sl.d_unique.as<uint32_t>();
        r->probabilities = sl.d_prob.as<double>(); r->call = sl.d_call.as<uint8_t>(); r->confidence = sl.d_conf.as<uint8_t>();
        r->flags = sl.d_flags.as<uint8_t>();
        r->gzip_tallies = sl.want_gzt ? sl.d_gzt.as<uint16_t>() : nullptr;
        r->gzip_sizes = sl.want_gzt && sl.gz_output != CHN_GZIP_TALLIES ? sl.d_gzsize.as<uint32_t>() : nullptr;
        return CHN_OK;
    }
    auto fetch = [&](void *dst, const void *dev, size_t off, size_t bytes) { return copy_out(dst, staged ? staged + off : nullptr, dev, bytes); };
    int frc = CHN_OK;
    if (sl.want_gzt && r->gzip_tallies) {
        if (sl.gz_output == CHN_GZIP_SIZES || sl.gz_output == CHN_GZIP_SIZES_ALL) return fail(CHN_E_INVALID, "chn_result.gzip_tallies: the batch asked for sizes only");
        if ((frc = copy_out(r->gzip_tallies, sl.gz_staged ? sl.h_gzt.p : nullptr, sl.d_gzt.p, n * GZT_WORDS * 2))) return frc;
    }
    if (sl.want_gzt && r->gzip_sizes) {
        if (sl.gz_output == CHN_GZIP_TALLIES) return fail(CHN_E_INVALID, "chn_result.gzip_sizes: the batch asked for tallies only");
        if ((frc = copy_out(r->gzip_sizes, sl.gz_staged ? sl.h_gzsize.p : nullptr, sl.d_gzsize.p, n * 4))) return frc;
    }
    if (r->num_hashes && (frc = fetch(r->num_hashes, sl.d_num_hashes.p, L.nh, n * 4))) return frc;
    if (r->counts && (frc = fetch(r->counts, sl.d_counts.p, L.counts, n * C * 4))) return frc;
    if (r->unique_counts && (frc = fetch(r->unique_counts, sl.d_unique.p, L.unique, n * C * 4))) return frc;
    if (sl.model_ran) {
        if (r->probabilities && (frc = fetch(r->probabilities, sl.d_prob.p, L.prob, n * C * 8))) return frc;
        if (r->call && (frc = fetch(r->call, sl.d_call.p, L.call, n))) return frc;
        if (r->confidence && (frc = fetch(r->confidence, sl.d_conf.p, L.conf, n))) return frc;
        std::vector<uint8_t> flags(n);
        if ((frc = fetch(flags.data(), sl.d_flags.p, L.flags, n))) return frc;
        if (r->flags) std::memcpy(r->flags, flags.data(), n);
        // borderline reads: re-evaluate with the host libm so that `call` never depends on a last-ulp exp() difference
        if (sl.host_batch && r->num_hashes && r->counts && r->unique_counts && r->call && r->confidence && r->probabilities) {
            std::vector<double> p(C);
            // gamma / beta models: the reference evaluates stats::dgamma / dbeta in float, the device forms the log-density in
            // double -- the probability column then agrees to ~1e-5 only, so host results are always taken from the float path
            const bool all = s->model.dist != CHN_DIST_KDE;
            for (uint64_t i = 0; i < n; ++i)
                if (all || flags[i] || r->num_hashes[i] == 0) {
                    const uint32_t length = sl.h_len1[i] + (sl.h_len2.empty() ? 0u : sl.h_len2[i]);
                    host_model_call(s->model, r->num_hashes[i], r->counts + i * C, r->unique_counts + i * C,
                                    sl.h_mq.empty() ? 0.0f : sl.h_mq[i],
                                    sl.want_gzt ? std::numeric_limits<float>::infinity() : (sl.h_comp.empty() ? 0.0f : sl.h_comp[i]),  // gate left to the caller
                                    length, p.data(),
                                    &r->call[i], &r->confidence[i]);
                    for (uint64_t c = 0; c < C; ++c) r->probabilities[i * C + c] = p[c];
                }
        }
    }
    return CHN_OK;
}

extern "C" int chn_classify_counts_raw(chn_stream *s, uint64_t n, const uint32_t *num_hashes, const uint32_t *counts,
                                       const uint32_t *unique_counts, const uint32_t *lengths, const float *mean_quality,
                                       const float *compression, double *probabilities, uint8_t *call, uint8_t *confidence,
                                       uint8_t *flags) {
    if (!s || !num_hashes || !counts || !unique_counts || !lengths || !probabilities || !call || !confidence || !flags)
        return fail(CHN_E_INVALID, "chn_classify_counts: null argument");
    if (!s->model.set) return fail(CHN_E_STATE, "chn_classify_counts: no model set");
    if (s->inflight) return fail(CHN_E_STATE, "chn_classify_counts: a batch is in flight");
    if (n == 0) return CHN_OK;
    if (n > s->cfg.max_reads) return fail(CHN_E_CAPACITY, "chn_classify_counts: more reads than the stream's max_reads");
    HIPCHK(hipSetDevice(s->idx->d.device));
    const uint64_t C = s->idx->d.num_categories, m = s->cfg.max_reads;
    chn_stream::CountsBufs &b = s->cc;  // never a batch slot's buffers (device-resident results of waited batches live there)
    int rc;
    if ((rc = b.num_hashes.ensure(m * 4)) || (rc = b.counts.ensure(m * C * 4)) || (rc = b.unique.ensure(m * C * 4)) ||
        (rc = b.prob.ensure(m * C * 8)) || (rc = b.call.ensure(m)) || (rc = b.conf.ensure(m)) || (rc = b.flags.ensure(m)))
        return rc;
    if ((rc = upload(b.len1, lengths, n * 4, s->q_probe[0], m * 4))) return rc;
    if (mean_quality && (rc = upload(b.mq, mean_quality, n * 4, s->q_probe[0], m * 4))) return rc;
    if (compression && (rc = upload(b.comp, compression, n * 4, s->q_probe[0], m * 4))) return rc;
    HIPCHK(hipMemcpyAsync(b.num_hashes.p, num_hashes, n * 4, hipMemcpyHostToDevice, s->q_probe[0]));
    HIPCHK(hipMemcpyAsync(b.counts.p, counts, n * C * 4, hipMemcpyHostToDevice, s->q_probe[0]));
    HIPCHK(hipMemcpyAsync(b.unique.p, unique_counts, n * C * 4, hipMemcpyHostToDevice, s->q_probe[0]));
    K3Args k3 = s->k3;
    k3.num_hashes = b.num_hashes.as<uint32_t>(); k3.counts = b.counts.as<uint32_t>(); k3.unique = b.unique.as<uint32_t>();
    k3.len1 = b.len1.as<uint32_t>(); k3.len2 = nullptr;
    k3.mean_quality = mean_quality ? b.mq.as<float>() : nullptr; k3.compression = compression ? b.comp.as<float>() : nullptr;
    k3.prob = b.prob.as<double>(); k3.call = b.call.as<uint8_t>(); k3.conf = b.conf.as<uint8_t>(); k3.flags = b.flags.as<uint8_t>();
    k3.n_reads = (uint32_t)n;
    hipLaunchKernelGGL(k_model_call, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s->q_probe[0], k3);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->q_probe[0]));
    HIPCHK(hipMemcpy(probabilities, b.prob.p, n * C * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(call, b.call.p, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(confidence, b.conf.p, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(flags, b.flags.p, n, hipMemcpyDeviceToHost));
    return CHN_OK;
}

extern "C" int chn_classify_counts(chn_stream *s, uint64_t n, const uint32_t *num_hashes, const uint32_t *counts,
                                   const uint32_t *unique_counts, const uint32_t *lengths, const float *mean_quality,
                                   const float *compression, double *probabilities, uint8_t *call, uint8_t *confidence) {
    std::vector<uint8_t> flags(std::max<uint64_t>(n, 1));
    int rc = chn_classify_counts_raw(s, n, num_hashes, counts, unique_counts, lengths, mean_quality, compression, probabilities, call,
                                     confidence, flags.data());
    if (rc) return rc;
    const uint64_t C = s->idx->d.num_categories;
    std::vector<double> p(C);
    const bool all = s->model.dist != CHN_DIST_KDE;  // gamma / beta: always the float path of the reference (see chn_batch_wait)
    for (uint64_t i = 0; i < n; ++i)
        if (all || flags[i] || num_hashes[i] == 0) {  // borderline or NaN rows: host libm / host NaN sign
            host_model_call(s->model, num_hashes[i], counts + i * C, unique_counts + i * C, mean_quality ? mean_quality[i] : 0.0f,
                            compression ? compression[i] : 0.0f, lengths[i], p.data(), &call[i], &confidence[i]);
            for (uint64_t c = 0; c < C; ++c) probabilities[i * C + c] = p[c];
        }
    return CHN_OK;
}

extern "C" int chn_stream_profile(chn_stream *s, int which, double *total_ms, uint64_t *launches, int reset) {
    if (!s || !profile_which_ok(which)) return fail(CHN_E_INVALID, "chn_stream_profile: bad argument");
    // a counter without a time
    auto count_of = [&](uint64_t &counter, double ms, bool resets) {
        if (total_ms) *total_ms = ms;
        if (launches) *launches = counter;
        if (reset && resets) counter = 0;
        return CHN_OK;
    };
    switch ((ProfileWhich)which) {
        case PROF_FASTA_SPLIT: s->fsp.timer.report(total_ms, launches, reset); return CHN_OK;  // chn_fasta_split: its kernels in front of the first wait
        case PROF_PAIR_IDS: s->tpi.timer.report(total_ms, launches, reset); return CHN_OK;     // chn_text_pair_ids: k_pair_ids
        case PROF_TEXT_FETCH: s->txg.timer.report(total_ms, launches, reset); return CHN_OK;   // chn_text_fetch: k_text_gather
        case PROF_TEXT_SPLIT: s->tsp.timer.report(total_ms, launches, reset); return CHN_OK;   // chn_text_split: its kernels in front of the first wait
        case PROF_GATED:  // batches whose ordinary probe launch was queued behind a probe-gate wait (no time: whether this stream gates at all)
            return count_of(s->gated_batches, s->gate_signal ? 1.0 : 0.0, true);
        case PROF_TEXT_UPLOAD:
        case PROF_TEXT_PACK: {  // text batches: upload of the text, k_text_pack + k_text_mq
            double &ms = s->text_ms[which - PROF_TEXT_UPLOAD];
            if (total_ms) *total_ms = ms;
            if (launches) *launches = s->text_n;
            if (reset) { ms = 0; if (which == PROF_TEXT_PACK) s->text_n = 0; }
            return CHN_OK;
        }
        case PROF_FETCHES: return count_of(s->last_fetches, 0, false);    // row fetches the last batch's probe kernel issued
        case PROF_RERUNS: return count_of(s->overflow_reruns, 0, true);   // batches re-run on worst-case buffers after a row-log overflow
        case PROF_PROBE: case PROF_COUNT: case PROF_MODEL: case PROF_CHAIN: break;  // a slot's brackets, summed by prof_collect
    }
    if (total_ms) *total_ms = s->prof_ms[which];
    if (launches) *launches = s->prof_n[which];
    if (reset) { s->prof_ms[which] = 0; s->prof_n[which] = 0; }
    if (reset && which == PROF_PROBE && s->prof_anchor[0]) {  // no earlier probe kernel to count behind; idle streams: a fresh anchor as well
        s->prof_have_end = false;
        if (s->inflight == 0) {
            HIPCHK(hipSetDevice(s->idx->d.device));
            HIPCHK(prof_anchor_now(s));
        }
    }
    return CHN_OK;
}
extern "C" int chn_stream_last_batch_bytes(chn_stream *s, uint64_t *bytes, uint64_t *total_minimisers) {
    if (!s) return fail(CHN_E_INVALID, "null stream");
    if (bytes) *bytes = s->last_bytes;
    if (total_minimisers) *total_minimisers = s->last_min;
    return CHN_OK;
}
