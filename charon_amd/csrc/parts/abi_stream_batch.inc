// abi_stream_batch.inc -- chn_stream_create/destroy, chn_model_set, batch submission (submit_impl, launch_tail)
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.

// ---- stream -------------------------------------------------------------------------------------
// (ResLayout, the layout of a slot's page-locked result block: batch_plan.inc)

// The streams of a chn_stream, in the order they are made.
// Two probe streams, used alternately: batch i + 1's probe kernel does not wait for the last wavefront of batch i's, its workgroups
// take the slots that batch i's retiring wavefronts free once batch i has none left to dispatch (equal-length reads leave a last
// generation of one wavefront per CU; a front end's 65 536-read batches never fill the device at all).  Batch i + 2 queues behind
// batch i, so at most two probe grids are on the device.
// Priorities: the probe kernels' streams are the ordinary ones.  The side stream (count, model + call, result download of batch i)
// and the copy stream (uploads and the two tiny ordering kernels of batch i+1) run ABOVE it: their short kernels must get
// workgroup slots as the probe kernel of the neighbouring batch retires waves, or batch i only completes when batch i+1's probe
// kernel does and a caller with host buffers cannot start the next upload in time.  The tally stream runs BELOW it: the
// latency-bound deflate pass fills in beside the probe kernel, and so does the long-gzip stream, which the first CHN_GZIP_SIZES_ALL
// batch makes.  (The runtime also keeps a separate set of hardware queues per priority level, so a long tally kernel never sits in
// front of a copy or a probe launch in the same queue.)
// synced: chn_stream_sync waits for it (the two gzip streams are waited for through a batch's gz_done event only).
enum StreamPrio { PRIO_ORDINARY, PRIO_ABOVE, PRIO_BELOW };
struct StreamRole { hipStream_t *q; StreamPrio prio; bool at_create, synced; };
enum { N_STREAM_ROLES = 7 };
static std::array<StreamRole, N_STREAM_ROLES> stream_roles(chn_stream *s) {
    return {{{&s->q_probe[0], PRIO_ORDINARY, true, true}, {&s->q_probe[1], PRIO_ORDINARY, true, true}, {&s->q_side, PRIO_ABOVE, true, true},
             {&s->q_copy, PRIO_ABOVE, true, true}, {&s->q_tally, PRIO_BELOW, true, false}, {&s->q_split, PRIO_ORDINARY, true, true},
             {&s->q_gzlong, PRIO_BELOW, false, false}}};
}
// the list's entry for one of the streams (the long-gzip stream is opened late, by its first batch)
static StreamRole stream_role(chn_stream *s, const hipStream_t *q) {
    const auto roles = stream_roles(s);
    for (const StreamRole &r : roles) if (r.q == q) return r;
    return roles[0];  // (not reached: every stream of a chn_stream is in the list)
}
static hipError_t stream_open(const StreamRole &r) {
    if (r.prio == PRIO_ORDINARY) return hipStreamCreateWithFlags(r.q, hipStreamNonBlocking);
    int prio_least = 0, prio_greatest = 0;
    const hipError_t e = hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    return e != hipSuccess ? e : hipStreamCreateWithPriority(r.q, hipStreamNonBlocking, r.prio == PRIO_ABOVE ? prio_greatest : prio_least);
}

// A slot's events: the ones that order the streams, and the profiling brackets of the chain (a text batch's brackets are made by the
// first profiled text batch, abi_text_batch.inc; they are destroyed here with the others)
static int slot_events_create(Slot &sl) {
    return events_create("hipEventCreate", {&sl.k1_done, &sl.split_done, &sl.done, &sl.uploaded, &sl.bases_up, &sl.gz_done, &sl.gzt_done},
                         {&sl.t_probe.begin, &sl.t_probe.end, &sl.t_count.begin, &sl.t_count.end, &sl.t_model.begin, &sl.t_model.end, &sl.t_chain.begin, &sl.t_chain.end});
}
static void slot_events_destroy(Slot &sl) {
    events_destroy({&sl.k1_done, &sl.split_done, &sl.done, &sl.uploaded, &sl.bases_up, &sl.gz_done, &sl.gzt_done,
                    &sl.t_probe.begin, &sl.t_probe.end, &sl.t_count.begin, &sl.t_count.end, &sl.t_model.begin, &sl.t_model.end, &sl.t_chain.begin, &sl.t_chain.end,
                    &sl.t_text_upload.begin, &sl.t_text_upload.end, &sl.t_text_pack.begin, &sl.t_text_pack.end});
}

// Profiling streams: the age from which the time anchor is replaced at the next submit (at 10 s a float of milliseconds still resolves 0.001 ms)
static const int PROF_ANCHOR_SECONDS = 8;
// Profiling streams, with no batch in flight (the streams are idle): a fresh anchor, and no probe kernel behind which the next one counts
static hipError_t prof_anchor_now(chn_stream *s) {
    for (Slot &sl : s->slot) sl.new_anchor = false;
    s->prof_cur = 0; s->prof_anchor_pending = false; s->prof_have_end = false; s->prof_prev_end = 0;
    hipError_t e = hipEventRecord(s->prof_anchor[0], s->q_probe[0]);
    if (e == hipSuccess) e = hipEventSynchronize(s->prof_anchor[0]);
    s->prof_anchor_at = std::chrono::steady_clock::now();
    return e;
}

extern "C" int chn_stream_create(chn_index *idx, const chn_stream_cfg *cfg, chn_stream **out) {
    if (!idx || !cfg || !out || cfg->struct_size != sizeof(chn_stream_cfg)) return fail(CHN_E_INVALID, "chn_stream_create: bad argument");
    if (cfg->max_reads == 0 || cfg->max_reads > 0xFFFFFF00ULL) return fail(CHN_E_INVALID, "max_reads out of range");
    HIPCHK(hipSetDevice(idx->d.device));
    idx->ef_release();  // the loader's decode buffers: the index is complete by now
    chn_stream *s = new (std::nothrow) chn_stream();
    if (!s) return fail(CHN_E_NOMEM, "host allocation failed");
    s->idx = idx; s->cfg = *cfg;
    hipError_t e = hipSuccess;
    for (const StreamRole &r : stream_roles(s)) if (r.at_create && e == hipSuccess) e = stream_open(r);
    {   // long reads are cut over the lanes of a wavefront from this length class on (testing: CHN_STREAM_SPLIT_BUCKET)
        const uint32_t ob = (cfg->flags >> 8) & 0xffu;
        s->long_bucket = ob == 0 ? LONG_BUCKET_DEFAULT : ob == 255 ? 256u : std::max(64u, ob);
    }
    if (e != hipSuccess) { chn_stream_destroy(s); return fail(CHN_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e)); }
    {   // The probe gate's signal word (chn_stream::gate_signal), where the device's queues can wait for a value in memory.  Without it, or
        // with CHN_STREAM_NO_PROBE_GATE, consecutive probe grids share the device from their first workgroup on.  Diagnostics builds:
        // CHN_PROBE_GATE=0 does the same, for the A/B.
        int can_wait = 0;
        const char *off = diag_env("CHN_PROBE_GATE");
        if (!(cfg->flags & CHN_STREAM_NO_PROBE_GATE) && !(off && std::atoi(off) == 0) &&
            hipDeviceGetAttribute(&can_wait, hipDeviceAttributeCanUseStreamWaitValue, idx->d.device) == hipSuccess && can_wait) {
            e = hipExtMallocWithFlags((void **)&s->gate_signal, 8, hipMallocSignalMemory);
            if (e == hipSuccess) e = hipMemset(s->gate_signal, 0, 8);
            if (e != hipSuccess) { chn_stream_destroy(s); return fail(CHN_E_HIP, std::string("probe gate signal: ") + hipGetErrorString(e)); }
        }
    }
    const uint64_t n = cfg->max_reads, C = idx->d.num_categories;
    int rc = CHN_OK;
    const bool sharded = idx->d.row_begin != 0 || idx->d.row_end != idx->d.bin_size;
    const bool fused = !sharded && idx->single_bin_categories && C <= 8 && idx->d.bin_words == 1;
    // Row-log sizing: random sequence emits 2 / (wn + 1) minimisers per base; regions hold twice that (worst case: one per
    // base).  Escaped rows (more than three set bins): an eighth of the entries up to 128 bins, half of them beyond.
    const uint32_t wn = (uint32_t)idx->d.window_size - idx->d.kmer_size + 1;
    s->cap_num = (uint32_t)std::min<uint64_t>(65536, (4ULL * 65536 + wn) / (wn + 1));
    s->esc_shift = idx->d.bins <= 128 ? 3u : 1u;
    if (cfg->flags & CHN_STREAM_TINY_LOG) { s->cap_num = 64; s->esc_shift = 6; }  // testing: force the overflow -> re-run path
    // wavefront logs: one per 64 reads + one per read the SPLIT launch may take
    const uint64_t nw = waves_of(n) + (s->long_bucket < 256 ? std::min<uint64_t>(n, cfg->max_bases / len_bucket_floor(s->long_bucket)) : 0);
    for (Slot &sl : s->slot) {
        if ((rc = slot_events_create(sl))) { chn_stream_destroy(s); return rc; }
        if ((rc = sl.d_num_hashes.ensure(n * 4)) || (rc = sl.d_counts.ensure(n * C * 4)) || (rc = sl.d_unique.ensure(n * C * 4)) ||
            (rc = sl.d_prob.ensure(n * C * 8)) || (rc = sl.d_call.ensure(n)) || (rc = sl.d_conf.ensure(n)) || (rc = sl.d_flags.ensure(n)) ||
            (rc = sl.d_ctl.ensure(CTL_WORDS * 8)) || (rc = sl.d_order.ensure(n * 4))) {
            chn_stream_destroy(s);
            return rc;
        }
        if (!fused && !sharded && (rc = sl.lb.ensure(cfg->max_bases, nw, (uint32_t)idx->d.bin_words, s->cap_num, s->esc_shift, waves_of(n) + n))) { chn_stream_destroy(s); return rc; }
    }
    if ((rc = s->d_hist.ensure(LEN_BLOCKS * 256 * 4))) { chn_stream_destroy(s); return rc; }
    if (cfg->flags & CHN_STREAM_PROFILE) {  // the anchor the probe kernels' times are taken against (chn_stream_profile, which = 0)
        for (hipEvent_t &a : s->prof_anchor) if (e == hipSuccess) e = hipEventCreate(&a);
        if (e == hipSuccess) e = prof_anchor_now(s);
        if (e != hipSuccess) { chn_stream_destroy(s); return fail(CHN_E_HIP, std::string("profiling anchor: ") + hipGetErrorString(e)); }
    }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, idx->d.device) == hipSuccess && cus > 0) s->n_cus = (uint32_t)cus;
    }
    {   // result staging of all slots in ONE page-locked block when it is small (a front end's 65 536-read batches: 3 x 3 MB)
        const size_t res = (ResLayout(n, C).total + 255) & ~(size_t)255, gzs = (n * 4 + 255) & ~(size_t)255;
        if ((res + gzs) * chn_stream::N_SLOTS <= ((size_t)64 << 20) && s->h_block.ensure((res + gzs) * chn_stream::N_SLOTS) == CHN_OK) {
            char *base = s->h_block.as<char>();
            for (int i = 0; i < chn_stream::N_SLOTS; ++i) {
                s->slot[i].h_res.lend(base + (size_t)i * (res + gzs), res);
                s->slot[i].h_gzsize.lend(base + (size_t)i * (res + gzs) + res, gzs);
            }
        }
    }
    *out = s;
    return CHN_OK;
}

extern "C" int chn_stream_destroy(chn_stream *s) {
    if (!s) return CHN_OK;
    (void)hipSetDevice(s->idx->d.device);
    for (const StreamRole &r : stream_roles(s)) if (*r.q) (void)hipStreamSynchronize(*r.q);
    for (const StreamRole &r : stream_roles(s)) if (*r.q) (void)hipStreamDestroy(*r.q);
    if (s->gate_signal) (void)hipFree(s->gate_signal);
    for (hipEvent_t a : s->prof_anchor) if (a) (void)hipEventDestroy(a);
    for (Slot &sl : s->slot) {
        slot_events_destroy(sl);
        sl.h_res.release(); sl.h_gzt.release(); sl.h_gzsize.release(); sl.d_gzsize.release();
        sl.h_text.release(); sl.d_text.release(); sl.d_tdesc.release(); sl.d_tctl.release();
        DevBuf *bufs[] = {&sl.d_num_hashes, &sl.d_counts, &sl.d_unique, &sl.d_prob, &sl.d_call, &sl.d_conf, &sl.d_flags, &sl.d_ctl, &sl.d_order, &sl.d_gzt, &sl.d_gzidx, &sl.d_gzctr, &sl.d_gzlong,
                          &sl.d_len1, &sl.d_len2, &sl.d_mq, &sl.d_comp, &sl.d_bases, &sl.d_nmask, &sl.d_off1, &sl.d_off2};
        for (DevBuf *b : bufs) b->release();
        sl.lb.release();
    }
    DevBuf *bufs[] = {&s->d_hist, &s->d_model, &s->d_list, &s->d_cbase, &s->d_memo, &s->d_shx_cnt, &s->d_gzscratch, &s->d_gzlscratch[0], &s->d_gzlscratch[1],
                      &s->cc.num_hashes, &s->cc.counts, &s->cc.unique, &s->cc.len1, &s->cc.mq, &s->cc.comp, &s->cc.prob, &s->cc.call,
                      &s->cc.conf, &s->cc.flags};
    for (DevBuf *b : bufs) b->release();
    s->h_block.release();  // (behind the slots: they may have borrowed pieces of it)
    s->big.release();
    s->shx.release();
    s->tsp.release();
    s->fsp.release();
    s->txg.release();
    s->tpi.release();
    delete s;
    return CHN_OK;
}

extern "C" int chn_model_set(chn_stream *s, const chn_model *m) {
    // every check first: a rejected call leaves the stream's current model untouched
    if (!s || !m || m->struct_size != sizeof(chn_model)) return fail(CHN_E_INVALID, "chn_model_set: bad argument");
    const uint32_t C = m->num_categories;
    if (C != s->idx->d.num_categories) return fail(CHN_E_INVALID, "model category count differs from the index");
    if (!m->paired && (C < 2 || m->host_index > 1))
        return fail(CHN_E_INVALID, "single-end dehost (call_host) needs the host category at index 0 or 1 of a >= 2 category index");
    if (m->paired && C < 2) return fail(CHN_E_INVALID, "call_category needs at least 2 categories");
    if (m->dist > CHN_DIST_BETA) return fail(CHN_E_INVALID, "chn_model_set: unknown dist");
    const bool kde = m->dist == CHN_DIST_KDE;
    if (kde) {
        if (!m->pos_data || !m->neg_data || !m->pos_n || !m->neg_n) return fail(CHN_E_INVALID, "null KDE dataset table");
        for (uint32_t c = 0; c < C; ++c)
            if ((!m->pos_data[c] && m->pos_n[c]) || (!m->neg_data[c] && m->neg_n[c])) return fail(CHN_E_INVALID, "null KDE dataset");
    } else if (!m->pos_params || !m->neg_params) {
        return fail(CHN_E_INVALID, "chn_model_set: gamma / beta models need pos_params and neg_params");
    }
    if (s->inflight) return fail(CHN_E_STATE, "chn_model_set: batches are in flight");
    HIPCHK(hipSetDevice(s->idx->d.device));
    HostModel M;
    M.C = C;
    size_t total = 0;
    M.dist = m->dist;
    for (uint32_t c = 0; c < C; ++c) {
        if (kde) {
            M.pos.emplace_back(m->pos_data[c], m->pos_data[c] + m->pos_n[c]);
            M.neg.emplace_back(m->neg_data[c], m->neg_data[c] + m->neg_n[c]);
            total += m->pos_n[c] + m->neg_n[c];
        } else {
            M.pos.emplace_back(); M.neg.emplace_back();
            for (int j = 0; j < 3; ++j) M.dparams.push_back(m->pos_params[3 * c + j]);
            for (int j = 0; j < 3; ++j) M.dparams.push_back(m->neg_params[3 * c + j]);
        }
    }
    M.h_pos = m->h_pos; M.h_neg = m->h_neg; M.rate = m->err_rate;
    M.min_quality = m->min_quality; M.min_length = m->min_length; M.min_compression = m->min_compression;
    M.conf_thr = m->confidence_threshold; M.min_hits = m->min_hits; M.paired = m->paired; M.host_index = m->host_index;
    M.cpt = m->confidence_probability_threshold; M.lo_thr = m->host_unique_prop_lo_threshold;
    M.min_pd = m->min_proportion_difference; M.min_prd = m->min_prob_difference;
    std::vector<float> flat;
    flat.reserve(total);
    std::vector<uint32_t> tab(4 * (size_t)C);
    for (uint32_t c = 0; c < C; ++c) {
        tab[c] = (uint32_t)flat.size(); tab[C + c] = (uint32_t)M.pos[c].size();
        flat.insert(flat.end(), M.pos[c].begin(), M.pos[c].end());
        tab[2 * C + c] = (uint32_t)flat.size(); tab[3 * C + c] = (uint32_t)M.neg[c].size();
        flat.insert(flat.end(), M.neg[c].begin(), M.neg[c].end());
    }
    HIPCHK(hipStreamSynchronize(s->q_probe[0]));
    HIPCHK(hipStreamSynchronize(s->q_probe[1]));
    HIPCHK(hipStreamSynchronize(s->q_side));
    // From here on the device tables are being replaced: a failure leaves the stream WITHOUT a model (never with a torn one).
    s->model.set = false;
    const size_t tab_bytes = tab.size() * 4, flat_bytes = std::max<size_t>(flat.size() * 4, 4), par_bytes = M.dparams.size() * 4;
    int rc = s->d_model.ensure(tab_bytes + flat_bytes + std::max<size_t>(par_bytes, 4));
    if (rc) return rc;
    HIPCHK(hipMemcpy(s->d_model.p, tab.data(), tab_bytes, hipMemcpyHostToDevice));
    if (!flat.empty()) HIPCHK(hipMemcpy(static_cast<char *>(s->d_model.p) + tab_bytes, flat.data(), flat.size() * 4, hipMemcpyHostToDevice));
    if (par_bytes) HIPCHK(hipMemcpy(static_cast<char *>(s->d_model.p) + tab_bytes + flat_bytes, M.dparams.data(), par_bytes, hipMemcpyHostToDevice));
    const uint32_t memo_entries = 1u << 21;  // 32 MiB
    if ((rc = s->d_memo.ensure((size_t)memo_entries * 16))) return rc;
    HIPCHK(hipMemset(s->d_memo.p, 0, (size_t)memo_entries * 16));
    K3Args k;
    std::memset(&k, 0, sizeof(k));
    k.memo = s->d_memo.as<ulonglong2>(); k.memo_mask = memo_entries - 1;
    k.tab = s->d_model.as<uint32_t>();
    k.data = reinterpret_cast<const float *>(static_cast<char *>(s->d_model.p) + tab_bytes);
    k.C = C; k.h_pos = M.h_pos; k.h_neg = M.h_neg; k.rate = M.rate; k.log_rate = std::log(M.rate);
    k.min_quality = M.min_quality; k.min_compression = M.min_compression; k.cpt = M.cpt; k.lo_thr = M.lo_thr;
    k.min_pd = M.min_pd; k.min_prd = M.min_prd; k.min_length = M.min_length; k.conf_thr = (int32_t)M.conf_thr;
    k.min_hits = M.min_hits; k.paired = M.paired; k.host_index = M.host_index;
    k.dist = M.dist;
    k.dparams = reinterpret_cast<const float *>(static_cast<char *>(s->d_model.p) + tab_bytes + flat_bytes);
    s->k3 = k;
    s->model = std::move(M);
    s->model.set = true;
    return CHN_OK;
}

// (k1_cond, k1_lds_bytes, ring_pack_ok: lds_budget.hpp)
// One instance of the probe kernel.  blocks = 0: the ordinary launch, one wavefront per 64 reads; else the SPLIT launch (one long read per
// wavefront), `blocks` looping workgroups
template <int W, int MODE, bool SPLIT, bool COND>
static hipError_t launch_k1_as(const K1Args &a, size_t lds, hipStream_t st, uint32_t blocks) {
    if (!SPLIT) blocks = (uint32_t)waves_of(a.n_reads);
    if (lds > 48 * 1024) {  // long windows: opt in to large dynamic LDS
        hipError_t e = hipFuncSetAttribute((const void *)k_minimise_probe<W, MODE, 0, SPLIT, COND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    // w=41, k=19: the defaults every real Charon index uses (include/index_arguments.hpp:16-17).  The fixed-window instance has a packed ring and
    // nothing else: a window of 23 with k >= 26, where the ring words have no room for the offsets, goes to the general instance.
    if (a.wn == 23 && a.pack)
        hipLaunchKernelGGL((k_minimise_probe<W, MODE, 23, SPLIT, COND>), dim3(blocks), dim3(WAVE), lds, st, a);
    else
        hipLaunchKernelGGL((k_minimise_probe<W, MODE, 0, SPLIT, COND>), dim3(blocks), dim3(WAVE), lds, st, a);
    return hipGetLastError();
}
// The probe kernel's launch: the instance for `mode` and W = bin_words, on `st`.  split_blocks = 0: the ordinary launch; else the SPLIT
// launch with that many workgroups.  MODE_FUSED and MODE_LIST are W = 1 by definition; the list modes never split a read.
// (MODE_EMPLACE is no batch's: chn_synth_plant takes its instance itself.)
static hipError_t launch_k1(int mode, uint32_t W, const K1Args &a, size_t lds, hipStream_t st, uint32_t split_blocks = 0) {
    const bool cond = k1_cond(mode, a.B);
    if (split_blocks) {
        if (mode == MODE_FUSED) return cond ? launch_k1_as<1, MODE_FUSED, true, true>(a, lds, st, split_blocks) : launch_k1_as<1, MODE_FUSED, true, false>(a, lds, st, split_blocks);
        return by_words(W, [&](auto w) { return launch_k1_as<decltype(w)::value, MODE_ROWS, true, false>(a, lds, st, split_blocks); });
    }
    if (mode == MODE_LIST) return launch_k1_as<1, MODE_LIST, false, false>(a, lds, st, 0);
    if (mode == MODE_FUSED) return cond ? launch_k1_as<1, MODE_FUSED, false, true>(a, lds, st, 0) : launch_k1_as<1, MODE_FUSED, false, false>(a, lds, st, 0);
    return by_words(W, [&](auto w) { return launch_k1_as<decltype(w)::value, MODE_ROWS, false, false>(a, lds, st, 0); });
}
// the probe kernel's LDS for this index in MODE_ROWS: what the count kernel's budget is taken from, and what a re-run launches with
static size_t k1_rows_lds(const chn_index_desc &d) {
    const uint32_t wn = d.window_size - d.kmer_size + 1;
    return k1_lds_bytes(wn, d.num_categories, MODE_ROWS, d.hash_funs, (uint32_t)d.bin_words, (uint32_t)d.bins, ring_pack_ok(d.kmer_size, wn, d.minimiser_seed));
}
// Workgroups of a SPLIT launch: they loop over the long reads in strides of the grid.  More than the device holds at once (1 792 at seven
// per CU) on purpose: the reads a workgroup meets differ in length, and with four times as many workgroups as slots the dispatcher evens
// that out as slots fall free.  A grid of exactly what is resident was measured on 500 b - 50 kb reads: the step 3 ms (4 %) longer
// (profiles/r06/probe_overlap_ab.txt).  A device batch's bound is all its reads; its workgroups beyond the long reads return at once.
static uint32_t split_grid(uint32_t bound) { return std::min<uint32_t>(bound, 8192u); }

// (reserve: the most this buffer will ever hold -- allocated at first use, so that a later, larger batch never re-allocates:
//  hipFree waits for the device, i.e. for whatever kernels of the batches in flight are running)
static int upload(DevBuf &buf, const void *src, size_t bytes, hipStream_t st, size_t reserve = 0) {
    int rc = buf.ensure(std::max<size_t>(std::max(bytes, reserve), 16));
    if (rc) return rc;
    if (bytes) HIPCHK(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, st));
    return CHN_OK;
}

// What the stages of a submit know of the batch on the device: a host batch in the slot's staging, a device batch where the caller has
// it.  (The lengths, mean quality and compression are the slot's: sl.len1, sl.len2, sl.mq, sl.comp -- the tail reads them too.)
struct DevBatch {
    const uint32_t *bases, *nmask;  // nmask null: no N in the batch
    const uint64_t *off1, *off2;    // off2 null: single reads
    uint64_t n, n_bases;
    bool paired, on_device;
};

// ---- the gzip column: deflate tallies / gzip member sizes of a batch's reads (k_gzip_tally, k_gzip_long, k_gzip_size) ----
// What a launch of either deflate kernel needs beside its arguments.  A launch is as many wavefronts as the device holds at once (a CU's
// LDS over the launch's LDS per wavefront, max_wpc at most), each taking the next read from a counter, each with stride32 words of
// scratch for its class arrays.  The launches of a stream run one after the other, so they share the scratch; it only grows (hipFree
// waits for the kernels in flight), with a quarter to spare if `spare`.  lds beyond the default limit: the kernels' limit is raised,
// once, to the whole CU.  no_room: how a failed growth is reported (null: as the allocation reports it).
static int gz_launch_room(const chn_stream *s, size_t lds, uint32_t max_wpc, uint32_t count, size_t stride32, DevBuf &scratch, bool spare, const char *no_room,
                          const void *k4, const void *k2, bool &whole_cu, uint32_t &grid) {
    const uint32_t wpc = (uint32_t)std::min<size_t>(max_wpc, std::max<size_t>(1, (size_t)160 * 1024 / lds));
    grid = (uint32_t)std::min<uint64_t>(count, (uint64_t)s->n_cus * wpc);
    const size_t need = (size_t)grid * stride32 * 4;
    if (need > scratch.cap) {
        const int rc = scratch.ensure(need + (spare ? need / 4 : 0));
        if (rc) return no_room ? fail(CHN_E_NOMEM, std::string(no_room) + ": no room for " + std::to_string(need >> 20) + " MiB of deflate scratch (" + g_err + ")") : rc;
    }
    if (lds > 48 * 1024 && !whole_cu) {
        HIPCHK(hipFuncSetAttribute(k4, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        HIPCHK(hipFuncSetAttribute(k2, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        whole_cu = true;
    }
    return CHN_OK;
}

// The kernel's LDS (and with it the number of reads a CU works on at once) goes with the longest read of a launch, so a host batch is
// cut into occupancy classes (gz_plan, batch_plan.inc), one launch per class in use; a device batch is one launch sized by the caller's
// bound.  Reads: plan, upload, launches longest class first, sizes, downloads.
static int submit_gzip_column(chn_stream *s, Slot &sl, const DevBatch &db, uint32_t gzip_tallies, uint32_t gzip_output) {
    sl.want_gzt = gzip_tallies != 0 && !sl.list_mode;
    if (sl.want_gzt && gzip_output > CHN_GZIP_SIZES_ALL) return fail(CHN_E_INVALID, "chn_batch.gzip_output: unknown value");
    if (sl.want_gzt && gzip_output == CHN_GZIP_SIZES_ALL && db.on_device)
        return fail(CHN_E_INVALID, "chn_batch.gzip_output = CHN_GZIP_SIZES_ALL: host batches only");
    sl.gz_output = gzip_output;
    if (!sl.want_gzt) return CHN_OK;
    const uint64_t n = db.n;
    int rc = sl.d_gzt.ensure((size_t)s->cfg.max_reads * GZT_WORDS * 2);
    if (rc) return rc;
    const int bits = db.nmask ? 4 : 2;
    const uint32_t bound = std::min<uint32_t>(gzip_tallies, GZT_MAX_LEN);
    // CHN_GZIP_SIZES_ALL: k_gzip_long sizes the reads beyond the tally kernel's reach -- longer than GZT_MAX_LEN (on its own stream,
    // beside the tally launches) and those the tallies hand back for a second deflate block (behind the tally launches)
    const bool all_sizes = sl.gz_output == CHN_GZIP_SIZES_ALL;
    const uint32_t long_bound = gzip_tallies;
    const size_t cap_n = (size_t)s->cfg.max_reads;
    bool long_launch = false;  // a k_gzip_long launch on the long-gzip stream: the sizes are formed there, behind it and behind the tallies
    if (all_sizes) {
        if (!s->q_gzlong) HIPCHK(stream_open(stream_role(s, &s->q_gzlong)));
        if ((rc = sl.d_gzlong.ensure((cap_n + 64) * 4))) return rc;
        HIPCHK(hipMemsetAsync(sl.d_gzlong.p, 0, n * 4, s->q_copy));  // 0: not sized (yet)
        HIPCHK(hipMemsetAsync(sl.d_gzlong.as<uint32_t>() + cap_n, 0, 64 * 4, s->q_copy));
    }
    // one k_gzip_long launch
    auto launch_long = [&](hipStream_t st, DevBuf &scratch, uint32_t ctr, uint32_t filter, const uint32_t *index, uint32_t count) -> int {
        if (count == 0) return CHN_OK;
        const size_t lds = gzl_lds_bytes(bits);
        uint32_t grid = 0;
        if (int rc2 = gz_launch_room(s, lds, ~0u, count, GZL_STRIDE32, scratch, false, "gzip sizes of long reads", (const void *)k_gzip_long<4>, (const void *)k_gzip_long<2>,
                                     s->gzl_big_lds, grid))
            return rc2;
        GzlArgs gl;
        std::memset(&gl, 0, sizeof gl);
        gl.bases = db.bases; gl.nmask = db.nmask; gl.off1 = db.off1; gl.off2 = db.off2; gl.len1 = sl.len1; gl.len2 = sl.len2; gl.n_bases = db.n_bases;
        gl.bound = long_bound; gl.short_max = bound; gl.filter = filter; gl.tallies = sl.d_gzt.as<uint16_t>();
        gl.index = index; gl.count = count; gl.sizes = sl.d_gzlong.as<uint32_t>();
        gl.scratch = scratch.as<uint32_t>(); gl.counter = sl.d_gzlong.as<uint32_t>() + cap_n + ctr;
        gz_by_bits(bits, [&](auto B) { hipLaunchKernelGGL(k_gzip_long<decltype(B)::value>, dim3(grid), dim3(WAVE), lds, st, gl); });
        HIPCHK(hipGetLastError());
        return CHN_OK;
    };
    HIPCHK(hipMemsetAsync(sl.d_gzt.p, 1, n * GZT_WORDS * 2, s->q_tally));  // status word != 0: "not tallied" unless a launch says otherwise
    GztArgs g;
    std::memset(&g, 0, sizeof g);
    g.bases = db.bases; g.nmask = db.nmask; g.off1 = db.off1; g.off2 = db.off2; g.len1 = sl.len1; g.len2 = sl.len2;
    g.n_reads = (uint32_t)n; g.out = sl.d_gzt.as<uint16_t>(); g.n_bases = db.n_bases;
    // every launch of the batch takes its reads from a counter of its own
    if ((rc = sl.d_gzctr.ensure(32 * 4))) return rc;
    HIPCHK(hipMemsetAsync(sl.d_gzctr.p, 0, 32 * 4, s->q_tally));
    uint32_t n_launch = 0;
    // one k_gzip_tally launch (LDS: half a byte per letter; scratch: 6 bytes per letter)
    auto launch = [&](const uint32_t *index, uint32_t count, uint32_t max_len) -> int {
        if (count == 0) return CHN_OK;
        size_t glds = gzt_lds_bytes(max_len, bits);
        if (const char *pad = diag_env("CHN_GZT_LDS_PAD")) glds += (size_t)std::atoi(pad);  // occupancy-sensitivity diagnostic
        if (glds > 160 * 1024) return fail(CHN_E_INVALID, "deflate tallies: read too long for a CU's LDS");
        uint32_t max_wpc = GZT_WAVES_PER_CU;
        if (const char *w = diag_env("CHN_GZT_WAVES_PER_CU")) max_wpc = (uint32_t)std::max(1, std::min((int)max_wpc, std::atoi(w)));
        g.index = index; g.count = count; g.max_len = max_len;
        g.stride32 = gzt_stride32(max_len);
        uint32_t grid = 0;
        if (int rc2 = gz_launch_room(s, glds, max_wpc, count, g.stride32, s->d_gzscratch, true, nullptr, (const void *)k_gzip_tally<4>, (const void *)k_gzip_tally<2>,
                                     s->gzt_big_lds, grid))
            return rc2;
        g.scratch = s->d_gzscratch.as<uint32_t>();
        g.counter = sl.d_gzctr.as<uint32_t>() + (n_launch++ & 31u);
        gz_by_bits(bits, [&](auto B) { hipLaunchKernelGGL(k_gzip_tally<decltype(B)::value>, dim3(grid), dim3(WAVE), glds, s->q_tally, g); });
        HIPCHK(hipGetLastError());
        return CHN_OK;
    };
    if (!db.on_device) {
        const GzPlan p = gz_plan(sl.h_len1.data(), db.paired ? sl.h_len2.data() : nullptr, n, bits, bound, long_bound, all_sizes, sl.h_gzidx);
        // (on the copy stream: a pageable upload on the tally stream would wait for the previous batch's tally kernels)
        if ((rc = upload(sl.d_gzidx, sl.h_gzidx.data(), sl.h_gzidx.size() * 4, s->q_copy, (size_t)s->cfg.max_reads * 4 * (all_sizes ? 2 : 1)))) return rc;
        HIPCHK(hipEventRecord(sl.bases_up, s->q_copy));
        HIPCHK(hipStreamWaitEvent(s->q_tally, sl.bases_up, 0));
        const uint32_t *d_index = sl.d_gzidx.as<uint32_t>();
        if (all_sizes && p.rerun_at > p.long_at) {
            HIPCHK(hipStreamWaitEvent(s->q_gzlong, sl.bases_up, 0));
            if ((rc = launch_long(s->q_gzlong, s->d_gzlscratch[0], 0, GZL_ALL, d_index + p.long_at, (uint32_t)(p.rerun_at - p.long_at)))) return rc;
            long_launch = true;
        }
        for (uint32_t c = 1; c < GZ_NCLS; ++c)  // longest first: the slow, low-occupancy launches start early
            if ((rc = launch(d_index + p.start[c], p.start[c + 1] - p.start[c], p.cmax[c]))) return rc;
        if (all_sizes && (rc = launch_long(s->q_tally, s->d_gzlscratch[1], 1, GZL_HANDED_BACK, d_index + p.rerun_at, (uint32_t)(sl.h_gzidx.size() - p.rerun_at)))) return rc;
    } else {
        HIPCHK(hipEventRecord(sl.bases_up, s->q_copy));
        HIPCHK(hipStreamWaitEvent(s->q_tally, sl.bases_up, 0));
        if ((rc = launch(nullptr, (uint32_t)n, bound))) return rc;
    }
    // where the sizes are formed and downloaded: behind the tallies on the tally stream, or -- with a long-read launch -- on the long-gzip
    // stream behind both, so that the next batch's tally launches do not queue behind this batch's longest read
    hipStream_t zs = s->q_tally;
    if (long_launch) {
        HIPCHK(hipEventRecord(sl.gzt_done, s->q_tally));
        HIPCHK(hipStreamWaitEvent(s->q_gzlong, sl.gzt_done, 0));
        zs = s->q_gzlong;
    }
    if (sl.gz_output != CHN_GZIP_TALLIES) {  // the sizes from the tallies, one lane per read
        if ((rc = sl.d_gzsize.ensure((size_t)s->cfg.max_reads * 4))) return rc;
        GzSizeArgs gs;
        gs.tallies = sl.d_gzt.as<uint16_t>(); gs.len1 = sl.len1; gs.len2 = sl.len2; gs.n_reads = (uint32_t)n; gs.sizes = sl.d_gzsize.as<uint32_t>();
        gs.long_sizes = all_sizes ? sl.d_gzlong.as<uint32_t>() : nullptr;  // k_gzip_long's sizes fill in where the tallies hand a read back
        hipLaunchKernelGGL(k_gzip_size, dim3((uint32_t)waves_of(n)), dim3(WAVE), 0, zs, gs);
        HIPCHK(hipGetLastError());
    }
    sl.gz_staged = false;
    if (!db.on_device) {
        if (sl.gz_output == CHN_GZIP_TALLIES || sl.gz_output == CHN_GZIP_BOTH) {
            if ((rc = sl.h_gzt.ensure(n * GZT_WORDS * 2))) return rc;
            HIPCHK(hipMemcpyAsync(sl.h_gzt.p, sl.d_gzt.p, n * GZT_WORDS * 2, hipMemcpyDeviceToHost, s->q_tally));
        }
        if (sl.gz_output != CHN_GZIP_TALLIES) {
            if ((rc = sl.h_gzsize.ensure(n * 4))) return rc;
            HIPCHK(hipMemcpyAsync(sl.h_gzsize.p, sl.d_gzsize.p, n * 4, hipMemcpyDeviceToHost, zs));
        }
        sl.gz_staged = true;
    }
    HIPCHK(hipEventRecord(sl.gz_done, zs));
    return CHN_OK;
}

// ---- a batch's submit, stage by stage (submit_impl below is the driver) ----
// list_kind != 0: stop after logging the minimiser VALUES -- LIST_DENSE (dense row-sharded mode, chn_minimisers: deterministic
// worst-case layout on s->big) or LIST_SPARSE (sparse row-sharded mode: density-sized regions claimed from the cursor on s->shx);
// 0: the whole chain
enum { LIST_NONE = 0, LIST_DENSE = 1, LIST_SPARSE = 2 };
// which caller launch_tail serves: a batch's own tail on the side stream, or the synchronous re-run after a row-log overflow on the
// first probe stream (no profiling, no result download, no `done` event: chn_batch_wait is already past them)
enum TailFor { TAIL_BATCH, TAIL_RERUN };
// count (general layouts) + model/call + byte counter; closes the batch in slot `sl`
static int launch_tail(chn_stream *s, Slot &sl, LogBuf &lb, TailFor who);

// Stage 1: is this a batch the stream can take now?  Nothing is queued before it has passed (the stream's device is selected).
static int check_batch(const chn_stream *s, const chn_batch *b, bool list_mode) {
    if (!s || !b || b->struct_size != sizeof(chn_batch)) return fail(CHN_E_INVALID, "chn_batch_submit: bad argument");
    if (!list_mode && (s->idx->d.row_begin != 0 || s->idx->d.row_end != s->idx->d.bin_size))
        return fail(CHN_E_INVALID, "chn_batch_submit needs an index object holding all rows; use the chn_shard_* calls with a row shard");
    if (list_mode && s->inflight) return fail(CHN_E_STATE, "chn_shard_minimise: batches are in flight");
    if (s->inflight >= chn_stream::N_SLOTS) return fail(CHN_E_STATE, "three batches already in flight: call chn_batch_wait first");
    if (b->n_reads == 0) return fail(CHN_E_INVALID, "empty batch");
    if (b->n_reads > s->cfg.max_reads || b->n_bases > s->cfg.max_bases) return fail(CHN_E_CAPACITY, "batch exceeds stream capacity");
    if (!b->bases2 || !b->seg1_offset || !b->seg1_length) return fail(CHN_E_INVALID, "missing batch arrays");
    if ((b->seg2_offset == nullptr) != (b->seg2_length == nullptr)) return fail(CHN_E_INVALID, "seg2_offset/seg2_length must both be set or both NULL");
    if (b->n_bases % 64) return fail(CHN_E_INVALID, "n_bases must be a multiple of 64");
    HIPCHK(hipSetDevice(s->idx->d.device));
    return CHN_OK;
}
// ... and, for a host batch, the shapes of its operands before anything is launched (device batches are validated by the kernel itself)
static int check_segments(const chn_batch *b) {
    if (b->on_device) return CHN_OK;
    const bool paired = b->seg2_offset != nullptr;
    for (uint64_t i = 0; i < b->n_reads; ++i) {
        const uint64_t o1 = b->seg1_offset[i], l1 = b->seg1_length[i];
        if ((o1 & 63) || o1 + l1 > b->n_bases) return fail(CHN_E_INVALID, "segment 1 of read " + std::to_string(i) + " is misaligned or out of range");
        if (paired) {
            const uint64_t o2 = b->seg2_offset[i], l2 = b->seg2_length[i];
            if ((o2 & 63) || o2 + l2 > b->n_bases) return fail(CHN_E_INVALID, "segment 2 of read " + std::to_string(i) + " is misaligned or out of range");
        }
    }
    return CHN_OK;
}

// Stage 2: the batch's inputs where the kernels read them.  A host batch is uploaded into the slot's staging on the COPY stream (the
// probe stream waits on the slot's `uploaded` event, stage 5) and its small columns are kept on the host for chn_batch_wait; the slot's
// previous batch was waited for before this submit could happen (at most N_SLOTS batches in flight), so its staging is free.
// born_on_device: a text batch (abi_text_batch.inc) -- a host batch whose bases, N mask, layout and mean quality k_text_pack has
// already written into the slot's buffers (b->bases2 / nmask only say which of them exist, b->mean_quality is the host copy).
// A device batch stays where the caller has it.
static int stage_inputs(chn_stream *s, Slot &sl, const chn_batch *b, bool born_on_device, DevBatch &db) {
    const uint64_t n = b->n_reads;
    db.n = n; db.n_bases = b->n_bases; db.paired = b->seg2_offset != nullptr; db.on_device = b->on_device != 0;
    sl.host_batch = !b->on_device;
    sl.is_text = born_on_device;
    sl.n_reads = n;
    if (b->on_device) {
        db.bases = b->bases2; db.nmask = b->nmask; db.off1 = b->seg1_offset; sl.len1 = b->seg1_length;
        db.off2 = b->seg2_offset; sl.len2 = b->seg2_length; sl.mq = b->mean_quality; sl.comp = b->compression;
        return CHN_OK;
    }
    int rc;
    const bool paired = db.paired;
    const size_t cap_b = (size_t)s->cfg.max_bases, cap_n = (size_t)s->cfg.max_reads;
    if (!born_on_device) {
        if ((rc = upload(sl.d_bases, b->bases2, b->n_bases / 4, s->q_copy, cap_b / 4))) return rc;
        if (b->nmask && (rc = upload(sl.d_nmask, b->nmask, b->n_bases / 8, s->q_copy, cap_b / 8))) return rc;
        if ((rc = upload(sl.d_off1, b->seg1_offset, n * 8, s->q_copy, cap_n * 8)) || (rc = upload(sl.d_len1, b->seg1_length, n * 4, s->q_copy, cap_n * 4))) return rc;
        if (paired && ((rc = upload(sl.d_off2, b->seg2_offset, n * 8, s->q_copy, cap_n * 8)) || (rc = upload(sl.d_len2, b->seg2_length, n * 4, s->q_copy, cap_n * 4)))) return rc;
        if (b->mean_quality && (rc = upload(sl.d_mq, b->mean_quality, n * 4, s->q_copy, cap_n * 4))) return rc;
    }
    if (b->compression && (rc = upload(sl.d_comp, b->compression, n * 4, s->q_copy, cap_n * 4))) return rc;
    db.bases = sl.d_bases.as<uint32_t>();
    db.nmask = b->nmask ? sl.d_nmask.as<uint32_t>() : nullptr;
    db.off1 = sl.d_off1.as<uint64_t>(); sl.len1 = sl.d_len1.as<uint32_t>();
    db.off2 = paired ? sl.d_off2.as<uint64_t>() : nullptr; sl.len2 = paired ? sl.d_len2.as<uint32_t>() : nullptr;
    sl.mq = b->mean_quality ? sl.d_mq.as<float>() : nullptr;
    sl.comp = b->compression ? sl.d_comp.as<float>() : nullptr;
    sl.h_len1.assign(b->seg1_length, b->seg1_length + n);
    if (paired) sl.h_len2.assign(b->seg2_length, b->seg2_length + n); else sl.h_len2.clear();
    if (b->mean_quality) sl.h_mq.assign(b->mean_quality, b->mean_quality + n); else sl.h_mq.clear();
    if (b->compression) sl.h_comp.assign(b->compression, b->compression + n); else sl.h_comp.clear();
    return CHN_OK;
}

// Stage 3: this batch's PROBE stream -- the ordinary launch and everything that brackets it.  The list modes run with nothing in flight
// and keep to the first.  So do the batches of a caller whose reads are long enough for the SPLIT launch (judged by the batch waited for
// last: a front end's length distribution does not change from batch to batch): there the SPLIT launches carry most of the bases, the
// length order already fills the ordinary grid's tail with its shortest reads, and a second ordinary grid beside them measured
// 1 - 2 % SLOWER (DESIGN section 5).  Diagnostics builds: CHN_PROBE_STREAMS=1 puts every batch on the first stream (the schedule
// before there were two), CHN_PROBE_STREAMS=2 alternates whatever the reads.
// Profiling streams: the chain's bracket opens on it, behind a fresh time anchor where the old one has aged.
struct ProbeStream { hipStream_t q; bool alternate; };
static int pick_probe_stream(chn_stream *s, Slot &sl, bool prof, ProbeStream &ps) {
    static const int probe_streams = [] { const char *v = diag_env("CHN_PROBE_STREAMS"); return v ? std::atoi(v) : 0; }();
    ps.alternate = probe_streams == 2 || (probe_streams != 1 && !s->last_had_long);
    ps.q = s->q_probe[sl.list_mode || !ps.alternate ? 0 : s->batch_seq & 1];
    for (EvBracket *t : {&sl.t_probe, &sl.t_count, &sl.t_model, &sl.t_chain}) t->used = false;
    if (sl.new_anchor) { sl.new_anchor = false; s->prof_anchor_pending = false; }  // (left by a submit that failed half-way)
    if (prof) {
        // nothing in flight and the time anchor is old (the caller paused): a fresh one, or this batch's times would be floats of the
        // milliseconds since before the pause (the anchor otherwise only moves on behind a running batch, launch_probe)
        if (s->inflight == 0 && std::chrono::steady_clock::now() - s->prof_anchor_at > std::chrono::seconds(PROF_ANCHOR_SECONDS)) HIPCHK(prof_anchor_now(s));
        HIPCHK(hipEventRecord(sl.t_chain.begin, ps.q));
    }
    return CHN_OK;
}

// (stage 4, the gzip column, is submit_gzip_column above: the TALLY stream, and the LONG-GZIP stream, behind the uploads on the copy stream)

// Stage 5: length-class ordering, two launches (the first also clears the slot's control words).  They run on the COPY stream, behind
// this batch's uploads and beside the previous batch's minimise+probe kernel (they depend on neither), so that a small batch's
// critical path is just that kernel; the probe stream picks up at the slot's `uploaded` event.
static int order_reads(chn_stream *s, Slot &sl, const DevBatch &db, hipStream_t probe_q) {
    unsigned long long *ctl = sl.d_ctl.as<unsigned long long>();
    hipLaunchKernelGGL(k_len_hist, dim3(LEN_BLOCKS), dim3(256), 0, s->q_copy, sl.len1, sl.len2, (uint32_t)db.n, s->d_hist.as<uint32_t>(), ctl);
    // (list modes -- row-sharded chains, chn_minimisers -- never split a read: every rank must log the same entries in the same order)
    sl.split_bound = sl.list_mode ? 0u : split_bound(s->long_bucket, db.paired, sl.host_batch ? &sl.h_len1 : nullptr, db.n);
    hipLaunchKernelGGL(k_len_scatter, dim3(LEN_BLOCKS), dim3(256), 0, s->q_copy, sl.len1, sl.len2, (uint32_t)db.n, s->d_hist.as<uint32_t>(), sl.d_order.as<uint32_t>(),
                       ctl, sl.split_bound ? s->long_bucket : 256u, sl.split_bound);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(sl.uploaded, s->q_copy));
    HIPCHK(hipStreamWaitEvent(probe_q, sl.uploaded, 0));
    return CHN_OK;
}

// Stage 6: the probe kernel's arguments from the index and the slot (kept in the slot: a re-run after a log overflow starts from them).
// The row log, the probe gate and the chain flag are not set here: fill_k1_log, launch_probe.
static void fill_k1(K1Args &a, const chn_index *idx, Slot &sl, const DevBatch &db) {
    const chn_index_desc &d = idx->d;
    unsigned long long *ctl = sl.d_ctl.as<unsigned long long>();
    std::memset(&a, 0, sizeof(a));
    a.words = idx->words; a.S = d.bin_size; a.row_begin = d.row_begin; a.row_end = d.row_end; a.seed = d.minimiser_seed; a.powk1 = pow5(d.kmer_size - 1);
    a.shift = (uint32_t)d.hash_shift; a.h = d.hash_funs; a.k = d.kmer_size; a.wn = d.window_size - d.kmer_size + 1;
    a.n_reads = (uint32_t)db.n; a.nseg = db.paired ? 2 : 1; a.B = (uint32_t)d.bins; a.C = d.num_categories;
    a.pack = ring_pack_ok(a.k, a.wn, a.seed) ? 1u : 0u;  // decided once here; k1_lds_bytes and the launch follow it
    for (uint32_t bb = 0; bb < 8 && bb < d.bins; ++bb) a.b2c_packed |= (uint64_t)d.bin_to_category[bb] << (8 * bb);
    a.bases = db.bases; a.nmask = db.nmask; a.off1 = db.off1; a.off2 = db.off2; a.len1 = sl.len1; a.len2 = sl.len2; a.n_bases = db.n_bases;
    a.order = sl.d_order.as<uint32_t>();
    a.status = reinterpret_cast<uint32_t *>(ctl + CTL_STATUS);
    if (const char *ab = diag_env("CHN_ABLATE")) a.ablate = (uint32_t)std::atoi(ab);  // (diagnostics builds: skipping the row fetches gives wrong results by design)
    a.nt_probes = idx->rows_local * d.bin_words * 8 > (4ULL << 30) ? 1u : 0u;
    if (const char *nt = diag_env("CHN_NT_PROBES")) a.nt_probes = (uint32_t)std::atoi(nt);  // A/B diagnostic
    a.num_hashes = sl.d_num_hashes.as<uint32_t>(); a.counts = sl.d_counts.as<uint32_t>(); a.unique = sl.d_unique.as<uint32_t>();
    a.n_long_ptr = sl.split_bound ? ctl + CTL_NLONG : nullptr; a.wave_slot0 = (uint32_t)waves_of(db.n);
    a.fetches = ctl + CTL_FETCHES;
}
static void fill_k1_log(K1Args &a, Slot &sl, LogBuf &lb, bool dynamic) {
    a.rowlog = lb.log.as<uint32_t>(); a.rows = lb.rows.as<uint64_t>(); a.wave_meta = lb.meta.as<WaveMeta>(); a.wave_count = lb.wcount.as<uint32_t>();
    a.log_capacity = lb.log_cap; a.esc_capacity = lb.esc_cap; a.cap_num = lb.cap_num; a.esc_shift = lb.esc_shift;
    a.cursor = dynamic ? sl.d_ctl.as<unsigned long long>() + CTL_LOG_CURSOR : nullptr;
}
// ... and where the kernel logs: the slot's own row log (general layouts), or for the list modes the minimiser values on the stream's
// buffers -- LIST_DENSE with its region table laid out on the probe stream first
static int choose_log(chn_stream *s, Slot &sl, int list_kind, hipStream_t probe_q) {
    K1Args &a = sl.k1;
    if (list_kind == LIST_SPARSE) {
        fill_k1_log(a, sl, s->shx, true);
        a.rows = s->d_list.as<uint64_t>();
    } else if (list_kind == LIST_DENSE) {
        // deterministic worst-case layout on the stream's big buffers (every rank of the dense row-sharded mode must log its
        // minimisers at the same positions)
        fill_k1_log(a, sl, s->big, false);
        a.rows = s->d_list.as<uint64_t>();
        hipLaunchKernelGGL(k_wave_caps, dim3((uint32_t)((sl.n_reads + 255) / 256)), dim3(256), 0, probe_q, sl.d_order.as<uint32_t>(), sl.len1, sl.len2,
                           (uint32_t)sl.n_reads, s->big.cap_num, s->big.esc_shift, s->big.meta.as<WaveMeta>());
        hipLaunchKernelGGL(k_scan_meta, dim3(1), dim3(SCAN_THREADS), 0, probe_q, s->big.meta.as<WaveMeta>(), (uint32_t)waves_of(sl.n_reads));
        HIPCHK(hipGetLastError());
    } else if (!sl.fused) {
        fill_k1_log(a, sl, sl.lb, true);
    }
    return CHN_OK;
}

// Stage 7: the probe kernel.  The long reads first, on the SPLIT stream; then, on the batch's PROBE stream, the gate wait, the ordinary
// launch and (profiling streams) the end of its bracket and the stream's next time anchor.  gated: the launch takes part in the probe gate.
static int launch_probe(chn_stream *s, Slot &sl, int mode, size_t lds, const ProbeStream &ps, bool prof, bool &gated) {
    K1Args &a = sl.k1;
    const uint32_t W = (uint32_t)s->idx->d.bin_words;
    unsigned long long *ctl = sl.d_ctl.as<unsigned long long>();
    if (sl.split_bound) {
        // the long reads first, on a stream of their own: a few wavefronts that run beside the ordinary launch instead of holding it up
        HIPCHK(hipStreamWaitEvent(s->q_split, sl.uploaded, 0));
        hipError_t e4 = launch_k1(mode, W, a, lds, s->q_split, split_grid(sl.split_bound));
        if (e4 != hipSuccess) return fail(CHN_E_HIP, std::string("k_minimise_probe (split) launch: ") + hipGetErrorString(e4));
        HIPCHK(hipEventRecord(sl.split_done, s->q_split));
    }
    // The probe gate.  A batch that alternates no longer starts beside its predecessor's grid for that grid's whole life (both then run at
    // half speed for twice as long, and the predecessor's side kernels starve under two grids): its launch waits, in its queue and not on a
    // CU, until the gated batch before it has dispatched its last workgroup, and so fills that grid's thinning last generation.  It still
    // queues behind batch i - 2 by stream order.  The value waited for is the last one whose writers (the grid, and k_gate_release behind
    // it) are already enqueued: batches that launch no gated grid -- list modes, long-read batches on the first stream, re-runs --
    // write nothing and use up no value, and this batch's own value counts only once its launch has succeeded.
    gated = !sl.list_mode && ps.alternate && s->gate_signal != nullptr;
    if (gated) {
        if (s->gate_seq) {
            HIPCHK(hipStreamWaitValue64(ps.q, s->gate_signal, s->gate_seq, hipStreamWaitValueGte, ~0ull));
            s->gated_batches += 1;
        }
        a.gate_started = ctl + CTL_GATE; a.gate_signal = s->gate_signal; a.gate_value = s->gate_seq + 1;
    }
    if (prof) { HIPCHK(hipEventRecord(sl.t_probe.begin, ps.q)); }
    // Chained row-log entries (rowlog_entry.hpp): the ordinary launch of a whole-index MODE_ROWS batch only.  The SPLIT launch above went
    // out unchained (k_count_longlog reads its logs), the list modes never chain, and a re-run after an overflow clears the flag again.
    a.chain = (mode == MODE_ROWS && rowlog_chain_ok(a.B)) ? 1u : 0u;
    hipError_t e = launch_k1(mode, W, a, lds, ps.q);
    if (e != hipSuccess) return fail(CHN_E_HIP, std::string("k_minimise_probe launch: ") + hipGetErrorString(e));
    if (gated) s->gate_seq += 1;
    if (prof) {
        // (profiling streams: the probe kernel's time is the time until BOTH its launches are done -- with long reads in the batch the SPLIT launch may
        //  carry most of the bases)
        if (sl.split_bound) HIPCHK(hipStreamWaitEvent(ps.q, sl.split_done, 0));
        HIPCHK(hipEventRecord(sl.t_probe.end, ps.q)); sl.t_probe.used = true;
        // the stream's time anchor moves on every few seconds: the next one behind this kernel, in use from this batch's wait on
        if (!s->prof_anchor_pending && std::chrono::steady_clock::now() - s->prof_anchor_at > std::chrono::seconds(PROF_ANCHOR_SECONDS)) {
            HIPCHK(hipEventRecord(s->prof_anchor[s->prof_cur ^ 1], ps.q));
            s->prof_anchor_at = std::chrono::steady_clock::now();
            sl.new_anchor = s->prof_anchor_pending = true;
        }
    }
    return CHN_OK;
}

// Stage 8: hand over to the tail.  The SIDE stream waits for both probe launches; behind the ordinary one, on the probe stream, the
// gate's backstop; then count, model + call and the result download on the side stream (launch_tail).
static int hand_over(chn_stream *s, Slot &sl, hipStream_t probe_q, bool gated) {
    HIPCHK(hipEventRecord(sl.k1_done, probe_q));
    HIPCHK(hipStreamWaitEvent(s->q_side, sl.k1_done, 0));
    if (sl.split_bound) HIPCHK(hipStreamWaitEvent(s->q_side, sl.split_done, 0));
    if (gated) {  // the backstop: a grid that died still releases its successor (a max: the successor's grid may have written already)
        hipLaunchKernelGGL(k_gate_release, dim3(1), dim3(1), 0, probe_q, s->gate_signal, (unsigned long long)s->gate_seq);
        HIPCHK(hipGetLastError());
    }
    return launch_tail(s, sl, sl.lb, TAIL_BATCH);
}

// The driver.  A stage that refuses leaves the slot not in flight: the next submit takes it again, and whatever was queued for it drains.
static int submit_impl(chn_stream *s, const chn_batch *b, int list_kind, bool born_on_device = false) {
    static const bool diag_sub = diag_env("CHN_DIAG_SUBMIT") != nullptr;
    const bool list_mode = list_kind != LIST_NONE;
    int rc;
    if ((rc = check_batch(s, b, list_mode))) return rc;
    const double t_start = wall_now();
    if ((rc = check_segments(b))) return rc;
    const chn_index_desc &d = s->idx->d;
    const uint32_t W = (uint32_t)d.bin_words, C = d.num_categories;
    const bool prof = (s->cfg.flags & CHN_STREAM_PROFILE) != 0;
    Slot &sl = s->slot[s->head];
    sl.list_mode = list_mode;
    sl.fused = !list_mode && s->idx->single_bin_categories && C <= 8 && W == 1;
    DevBatch db;
    if ((rc = stage_inputs(s, sl, b, born_on_device, db))) return rc;
    const double t_staged = wall_now();
    ProbeStream ps;
    if ((rc = pick_probe_stream(s, sl, prof, ps))) return rc;
    if ((rc = submit_gzip_column(s, sl, db, b->gzip_tallies, b->gzip_output))) return rc;
    const double t_gzip = wall_now();
    if ((rc = order_reads(s, sl, db, ps.q))) return rc;
    fill_k1(sl.k1, s->idx, sl, db);
    if ((rc = choose_log(s, sl, list_kind, ps.q))) return rc;
    const int mode = list_mode ? MODE_LIST : sl.fused ? MODE_FUSED : MODE_ROWS;
    size_t lds = k1_lds_bytes(sl.k1.wn, C, mode, sl.k1.h, W, sl.k1.B, sl.k1.pack != 0);
    if (const char *pad = diag_env("CHN_LDS_PAD")) lds += (size_t)std::atoi(pad);  // occupancy-sensitivity diagnostic
    if (lds > 160 * 1024) return fail(CHN_E_INVALID, "window too large for LDS");
    bool gated = false;
    if ((rc = launch_probe(s, sl, mode, lds, ps, prof, gated))) return rc;
    if (list_mode) return CHN_OK;  // the caller continues with chn_shard_probe / chn_shard_finish
    const double t_probe = wall_now();
    if ((rc = hand_over(s, sl, ps.q, gated))) return rc;
    if (diag_sub) std::fprintf(stderr, "submit: validate + uploads %.2f ms, deflate tallies %.2f, ordering + probe launch %.2f, tail %.2f\n",
                               (t_staged - t_start) * 1e3, (t_gzip - t_staged) * 1e3, (t_probe - t_gzip) * 1e3, (wall_now() - t_probe) * 1e3);
    s->head = (s->head + 1) % chn_stream::N_SLOTS;
    s->inflight += 1;
    s->batch_seq += 1;
    return CHN_OK;
}

// 3. counts from the row log (general bin layouts), 4. model + call (+ the algorithmic byte counter): a batch's own tail on the side
// stream, with its profiling brackets, the in-stream result download of a host batch and the slot's `done` event; a re-run's on the
// first probe stream, with none of them
static int launch_tail(chn_stream *s, Slot &sl, LogBuf &lb, TailFor who) {
    const chn_index_desc &d = s->idx->d;
    const hipStream_t st = who == TAIL_BATCH ? s->q_side : s->q_probe[0];
    const uint64_t n = sl.n_reads;
    const uint32_t W = (uint32_t)d.bin_words, C = d.num_categories;
    const uint32_t n_waves = (uint32_t)waves_of(n);
    const bool prof = (s->cfg.flags & CHN_STREAM_PROFILE) != 0 && who == TAIL_BATCH;
    unsigned long long *ctl = sl.d_ctl.as<unsigned long long>();
    if (!sl.fused) {
        K2Args k2;
        std::memset(&k2, 0, sizeof(k2));
        k2.rows = lb.rows.as<uint64_t>(); k2.rowlog = lb.log.as<uint32_t>();
        k2.wave_meta = lb.meta.as<WaveMeta>(); k2.wave_count = lb.wcount.as<uint32_t>(); k2.order = sl.d_order.as<uint32_t>();
        k2.counts = sl.d_counts.as<uint32_t>(); k2.unique = sl.d_unique.as<uint32_t>();
        k2.n_reads = (uint32_t)n; k2.B = (uint32_t)d.bins; k2.C = C; k2.W = W;
        std::memcpy(k2.b2c, d.bin_to_category, 256);
        k2.n_long_ptr = sl.split_bound && !sl.list_mode ? ctl + CTL_NLONG : nullptr; k2.wave_slot0 = n_waves;
        k2.chain = sl.list_mode ? 0u : sl.k1.chain;  // as the ordinary probe launch of this batch wrote its logs
        const dim3 grid(n_waves), block(K2_THREADS);
        // 16-bit totals when no read of this launch can have 2^16 minimisers (reads of 2^15 bases and more go to the SPLIT launch); as many
        // owners per sweep as keep the tables within what the probe wavefronts of this stream's probe configuration leave of a CU's LDS
        // (k2_lds_budget, lds_budget.hpp), so that the kernel runs under the next batch's probe kernel
        const bool t16 = !sl.list_mode && sl.len2 == nullptr && s->long_bucket <= LONG_BUCKET_DEFAULT;
        const uint32_t G = k2_group((uint32_t)d.bins, C, W, t16, k2_lds_budget(k1_rows_lds(d)));
        k2.group = G;
        const size_t lds2 = k2_lds_bytes((uint32_t)d.bins, C, W, G, t16);
        if (lds2 > 150 * 1024) return fail(CHN_E_INVALID, "bins x categories too large for the count kernel's LDS");
        const void *fn = t16 ? by_words(W, [](auto w) { return (const void *)k_count_wavelog<decltype(w)::value, true>; })
                             : by_words(W, [](auto w) { return (const void *)k_count_wavelog<decltype(w)::value, false>; });
        if (lds2 > 48 * 1024) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));  // opt in to large dynamic LDS
        if (prof) HIPCHK(hipEventRecord(sl.t_count.begin, st));
        {
            void *args[] = {(void *)&k2};
            HIPCHK(hipLaunchKernel(fn, grid, block, args, lds2, st));
        }
        if (k2.n_long_ptr) {  // the logs of the reads that were split over a wavefront: one read per log
            const dim3 lgrid(std::min<uint32_t>(sl.split_bound, 4096u)), lblock(K2L_THREADS);
            by_words(W, [&](auto w) { hipLaunchKernelGGL(k_count_longlog<decltype(w)::value>, lgrid, lblock, 0, st, k2); });
        }
        HIPCHK(hipGetLastError());
        if (prof) { HIPCHK(hipEventRecord(sl.t_count.end, st)); sl.t_count.used = true; }
    }
    sl.model_ran = s->model.set;
    const uint32_t hW8 = (uint32_t)(d.hash_funs * W * 8), outb = (uint32_t)(8 + 8 * C);
    if (s->model.set) {
        K3Args k3 = s->k3;
        k3.num_hashes = sl.d_num_hashes.as<uint32_t>(); k3.counts = sl.d_counts.as<uint32_t>(); k3.unique = sl.d_unique.as<uint32_t>();
        k3.len1 = sl.len1; k3.len2 = sl.len2; k3.mean_quality = sl.mq; k3.compression = sl.comp;
        k3.prob = sl.d_prob.as<double>(); k3.call = sl.d_call.as<uint8_t>(); k3.conf = sl.d_conf.as<uint8_t>(); k3.flags = sl.d_flags.as<uint8_t>();
        k3.n_reads = (uint32_t)n;
        k3.acc = ctl + CTL_BYTES; k3.hW8 = hW8; k3.outb = outb;
        k3.open_compression_gate = sl.want_gzt ? 1u : 0u;
        if (prof) HIPCHK(hipEventRecord(sl.t_model.begin, st));
        hipLaunchKernelGGL(k_model_call, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, k3);
        HIPCHK(hipGetLastError());
        if (prof) { HIPCHK(hipEventRecord(sl.t_model.end, st)); sl.t_model.used = true; }
    } else {
        hipLaunchKernelGGL(k_batch_bytes, dim3((uint32_t)std::min<uint64_t>(1024, (n + 255) / 256)), dim3(256), 0, st, sl.len1, sl.len2,
                           sl.d_num_hashes.as<uint32_t>(), (uint32_t)n, hW8, outb, ctl + CTL_BYTES);
        HIPCHK(hipGetLastError());
    }
    if (prof) { HIPCHK(hipEventRecord(sl.t_chain.end, st)); sl.t_chain.used = true; }
    sl.staged = false;
    if (who == TAIL_RERUN) return CHN_OK;  // chn_batch_wait fetches the re-run's results from the device arrays
    if (sl.host_batch) {
        const ResLayout L(n, C);
        int rc = sl.h_res.ensure(L.total);
        if (rc) return rc;
        char *h = sl.h_res.as<char>();
        HIPCHK(hipMemcpyAsync(h + L.ctl, ctl, CTL_WORDS * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h + L.nh, sl.d_num_hashes.p, n * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h + L.counts, sl.d_counts.p, n * C * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h + L.unique, sl.d_unique.p, n * C * 4, hipMemcpyDeviceToHost, st));
        if (sl.model_ran) {
            HIPCHK(hipMemcpyAsync(h + L.prob, sl.d_prob.p, n * C * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h + L.call, sl.d_call.p, n, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h + L.conf, sl.d_conf.p, n, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h + L.flags, sl.d_flags.p, n, hipMemcpyDeviceToHost, st));
        }
        sl.staged = true;
    }
    HIPCHK(hipEventRecord(sl.done, st));
    return CHN_OK;
}

extern "C" int chn_batch_submit(chn_stream *s, const chn_batch *b) {
    static const bool diag = diag_env("CHN_DIAG_WAIT") != nullptr;
    if (!diag) return submit_impl(s, b, LIST_NONE);
    const double t0 = wall_now();
    const int rc = submit_impl(s, b, LIST_NONE);
    const double t1 = wall_now();
    std::fprintf(stderr, "chn_batch_submit: at %.4f  %.2f ms\n", t0, (t1 - t0) * 1e3);
    return rc;
}
