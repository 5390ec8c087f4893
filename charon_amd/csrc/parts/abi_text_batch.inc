// abi_text_batch.inc -- chn_text_submit / chn_text_wait / chn_text_pack: batches of reads handed over as plain text
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.
//
// A text batch is a HOST batch whose large arrays are born on the device: the text and its descriptors are uploaded on the copy
// stream, k_text_pack (text_pack.inc) writes the slot's d_bases / d_nmask / d_mq behind them, and the host waits for the kernel's
// three words -- N seen, illegal bytes, first read with one -- because the chain is shaped on the host by whether there is an N mask.
// From there on it is submit_impl with the uploads of those arrays left out.
// With CHN_TEXT_ON_DEVICE the text is the caller's device memory (the contract of text_split.inc): no staging, no upload, k_text_pack
// reads the caller's buffer -- it fetches only aligned dwords that hold a wanted byte -- and the wait for its verdict frees the buffer.

static const size_t TEXT_PAD = 64;      // bytes in front of and behind the text on the device
static const size_t TEXT_MQ_AT = 64;    // the mean-quality column in a slot's h_text, behind k_text_pack's words

static uint64_t text_pad64(uint64_t x) { return (x + 63) & ~(uint64_t)63; }

// everything up to and including the wait for k_text_pack on slot `sl`; the packed batch is then in the slot's device buffers, the
// words and the mean quality in sl.h_text.  A failure leaves nothing queued that matters (the copy stream drains on its own).
static int text_pack_run(chn_stream *s, Slot &sl, const chn_text_batch *t, const char *who) {
    const std::string W(who);
    // chn_text_batch is the form without text2 (nothing behind gzip_output is read), chn_text_batch2 the form with it
    static_assert(offsetof(chn_text_batch2, text2) == sizeof(chn_text_batch), "text2 lies right behind the batch");
    if (t->struct_size != sizeof(chn_text_batch) && t->struct_size != sizeof(chn_text_batch2)) return fail(CHN_E_INVALID, W + ": bad struct_size");
    const chn_text_batch2 *t2 = t->struct_size == sizeof(chn_text_batch2) ? reinterpret_cast<const chn_text_batch2 *>(t) : nullptr;
    const uint8_t *text2 = t2 ? t2->text2 : nullptr;
    if (t->flags & ~(CHN_TEXT_DNA5_RANKS | CHN_TEXT_ON_DEVICE)) return fail(CHN_E_INVALID, W + ": unknown flag");
    const uint64_t n = t->n_reads;
    if (n == 0) return fail(CHN_E_INVALID, "empty batch");
    if (n > s->cfg.max_reads) return fail(CHN_E_CAPACITY, "batch exceeds stream capacity (reads)");
    if (!t->seq1_offset || !t->seq1_length) return fail(CHN_E_INVALID, W + ": missing seq1_offset / seq1_length");
    if (!t->text && t->text_bytes) return fail(CHN_E_INVALID, W + ": text is NULL");
    if ((t->qual1_offset == nullptr) != (t->qual1_length == nullptr)) return fail(CHN_E_INVALID, W + ": qual1_offset / qual1_length must both be set or both NULL");
    if ((t->seq2_offset == nullptr) != (t->seq2_length == nullptr)) return fail(CHN_E_INVALID, W + ": seq2_offset / seq2_length must both be set or both NULL");
    if ((t->qual2_offset == nullptr) != (t->qual2_length == nullptr)) return fail(CHN_E_INVALID, W + ": qual2_offset / qual2_length must both be set or both NULL");
    if (t->qual2_offset && !t->seq2_offset) return fail(CHN_E_INVALID, W + ": qual2_* without seq2_*");
    const bool paired = t->seq2_offset != nullptr;
    if (text2 && !(t->flags & CHN_TEXT_ON_DEVICE)) return fail(CHN_E_INVALID, W + ": text2 needs CHN_TEXT_ON_DEVICE");
    if (text2 && !paired) return fail(CHN_E_INVALID, W + ": text2 without seq2_*");
    const bool q1 = t->qual1_offset != nullptr, q2 = t->qual2_offset != nullptr;
    // range check of every descriptor and the segment layout (pack.py::pack_reads, HostBatch::pack)
    const uint64_t tb = t->text_bytes, tb2 = text2 ? t2->text2_bytes : tb;  // mate 2 lies in text2 where there is one
    auto inside = [tb](uint64_t o, uint32_t l) { return o <= tb && l <= tb - o; };
    auto inside2 = [tb2](uint64_t o, uint32_t l) { return o <= tb2 && l <= tb2 - o; };
    sl.h_toff1.resize(n);
    if (paired) sl.h_toff2.resize(n); else sl.h_toff2.clear();
    uint64_t cur = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (!inside(t->seq1_offset[i], t->seq1_length[i]) || (q1 && !inside(t->qual1_offset[i], t->qual1_length[i])) ||
            (paired && !inside2(t->seq2_offset[i], t->seq2_length[i])) || (q2 && !inside2(t->qual2_offset[i], t->qual2_length[i])))
            return fail(CHN_E_INVALID, W + ": a stretch of read " + std::to_string(i) + " reaches beyond " + (text2 ? "text_bytes / text2_bytes" : "text_bytes"));
        sl.h_toff1[i] = cur; cur += text_pad64(t->seq1_length[i]);
        if (paired) { sl.h_toff2[i] = cur; cur += text_pad64(t->seq2_length[i]); }
    }
    const uint64_t n_bases = std::max<uint64_t>(cur, 64);
    if (n_bases > s->cfg.max_bases) return fail(CHN_E_CAPACITY, "batch exceeds stream capacity (bases)");
    sl.text_n_bases = n_bases;

    HIPCHK(hipSetDevice(s->idx->d.device));
    const bool on_device = (t->flags & CHN_TEXT_ON_DEVICE) != 0;
    int rc;
    if (on_device && (rc = device_text_check(t->text, tb, s->idx->d.device, W + ": CHN_TEXT_ON_DEVICE"))) return rc;  // before any launch
    if (text2 && (rc = device_text_check(text2, tb2, s->idx->d.device, W + ": CHN_TEXT_ON_DEVICE: text2"))) return rc;
    const size_t cap_b = (size_t)s->cfg.max_bases, cap_n = (size_t)s->cfg.max_reads;
    // the slot's batch buffers at the sizes stage_inputs (abi_stream_batch.inc) reserves for them (they never re-allocate afterwards)
    if ((rc = sl.d_bases.ensure(std::max<size_t>(cap_b / 4, 16))) || (rc = sl.d_nmask.ensure(std::max<size_t>(cap_b / 8, 16))) ||
        (rc = sl.d_mq.ensure(std::max<size_t>(cap_n * 4, 16))) || (rc = sl.d_tctl.ensure(TXT_CTL_WORDS * 4)) ||
        (rc = sl.h_text.ensure(TEXT_MQ_AT + cap_n * 4)))
        return rc;
    if (!on_device) {  // text staging: grow-only, with some slack so that batches of slightly different sizes do not re-allocate
        const size_t need = (size_t)tb + 2 * TEXT_PAD;
        if (need > sl.d_text.cap && (rc = sl.d_text.ensure(need + need / 8)))
            return fail(CHN_E_NOMEM, W + ": no room for " + std::to_string(need >> 20) + " MiB of device text staging (" + g_err + ")");
    }
    const bool prof = (s->cfg.flags & CHN_STREAM_PROFILE) != 0;
    if (prof)
        for (hipEvent_t *e : {&sl.t_text_upload.begin, &sl.t_text_upload.end, &sl.t_text_pack.begin, &sl.t_text_pack.end}) if (!*e) HIPCHK(hipEventCreate(e));
    const uint8_t *d_text = on_device ? t->text : sl.d_text.as<uint8_t>() + TEXT_PAD;
    if (prof) HIPCHK(hipEventRecord(sl.t_text_upload.begin, s->q_copy));
    if (tb && !on_device) HIPCHK(hipMemcpyAsync(sl.d_text.as<uint8_t>() + TEXT_PAD, t->text, tb, hipMemcpyHostToDevice, s->q_copy));
    if (prof) HIPCHK(hipEventRecord(sl.t_text_upload.end, s->q_copy));
    if ((rc = upload(sl.d_off1, sl.h_toff1.data(), n * 8, s->q_copy, cap_n * 8)) || (rc = upload(sl.d_len1, t->seq1_length, n * 4, s->q_copy, cap_n * 4))) return rc;
    if (paired && ((rc = upload(sl.d_off2, sl.h_toff2.data(), n * 8, s->q_copy, cap_n * 8)) || (rc = upload(sl.d_len2, t->seq2_length, n * 4, s->q_copy, cap_n * 4)))) return rc;
    // descriptors: four columns of byte offsets, then two of quality lengths
    if ((rc = sl.d_tdesc.ensure(cap_n * 40))) return rc;
    uint64_t *d_o = sl.d_tdesc.as<uint64_t>();
    uint32_t *d_q = reinterpret_cast<uint32_t *>(d_o + 4 * cap_n);
    HIPCHK(hipMemcpyAsync(d_o, t->seq1_offset, n * 8, hipMemcpyHostToDevice, s->q_copy));
    if (q1) {
        HIPCHK(hipMemcpyAsync(d_o + cap_n, t->qual1_offset, n * 8, hipMemcpyHostToDevice, s->q_copy));
        HIPCHK(hipMemcpyAsync(d_q, t->qual1_length, n * 4, hipMemcpyHostToDevice, s->q_copy));
    }
    if (paired) HIPCHK(hipMemcpyAsync(d_o + 2 * cap_n, t->seq2_offset, n * 8, hipMemcpyHostToDevice, s->q_copy));
    if (q2) {
        HIPCHK(hipMemcpyAsync(d_o + 3 * cap_n, t->qual2_offset, n * 8, hipMemcpyHostToDevice, s->q_copy));
        HIPCHK(hipMemcpyAsync(d_q + cap_n, t->qual2_length, n * 4, hipMemcpyHostToDevice, s->q_copy));
    }
    HIPCHK(hipMemsetAsync(sl.d_tctl.p, 0, 2 * 4, s->q_copy));
    HIPCHK(hipMemsetAsync(sl.d_tctl.as<uint32_t>() + TXT_FIRST_BAD, 0xFF, 4, s->q_copy));
    HIPCHK(hipMemsetAsync(sl.d_mq.p, 0, n * 4, s->q_copy));

    TextPackArgs a;
    std::memset(&a, 0, sizeof a);
    a.text = d_text; a.text2 = text2 ? text2 : d_text;
    a.off1 = sl.d_off1.as<uint64_t>(); a.len1 = sl.d_len1.as<uint32_t>();
    a.off2 = paired ? sl.d_off2.as<uint64_t>() : nullptr; a.len2 = paired ? sl.d_len2.as<uint32_t>() : nullptr;
    a.so1 = d_o; a.qo1 = q1 ? d_o + cap_n : nullptr; a.so2 = paired ? d_o + 2 * cap_n : nullptr; a.qo2 = q2 ? d_o + 3 * cap_n : nullptr;
    a.ql1 = q1 ? d_q : nullptr; a.ql2 = q2 ? d_q + cap_n : nullptr;
    a.n_reads = (uint32_t)n; a.n_bases = n_bases;
    a.bases = sl.d_bases.as<uint32_t>(); a.nmask = sl.d_nmask.as<uint32_t>(); a.qsum = sl.d_mq.as<int>(); a.ctl = sl.d_tctl.as<uint32_t>();
    const uint64_t blocks = (n_bases / 16 + 255) / 256;
    if (blocks > 0x7FFFFFFFULL) return fail(CHN_E_CAPACITY, W + ": batch too large for one launch");
    if (prof) HIPCHK(hipEventRecord(sl.t_text_pack.begin, s->q_copy));
    if (t->flags & CHN_TEXT_DNA5_RANKS) hipLaunchKernelGGL(k_text_pack<true>, dim3((uint32_t)blocks), dim3(256), 0, s->q_copy, a);
    else hipLaunchKernelGGL(k_text_pack<false>, dim3((uint32_t)blocks), dim3(256), 0, s->q_copy, a);
    HIPCHK(hipGetLastError());
    if (q1 || q2) {
        hipLaunchKernelGGL(k_text_mq, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s->q_copy, sl.d_mq.as<int>(), a.ql1, a.ql2, (uint32_t)n);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(sl.h_text.as<char>() + TEXT_MQ_AT, sl.d_mq.p, n * 4, hipMemcpyDeviceToHost, s->q_copy));
    }
    if (prof) HIPCHK(hipEventRecord(sl.t_text_pack.end, s->q_copy));
    HIPCHK(hipMemcpyAsync(sl.h_text.p, sl.d_tctl.p, TXT_CTL_WORDS * 4, hipMemcpyDeviceToHost, s->q_copy));
    HIPCHK(hipStreamSynchronize(s->q_copy));
    if (prof) {
        float up = 0, pk = 0;
        HIPCHK(hipEventElapsedTime(&up, sl.t_text_upload.begin, sl.t_text_upload.end));
        HIPCHK(hipEventElapsedTime(&pk, sl.t_text_pack.begin, sl.t_text_pack.end));
        s->text_ms[0] += up; s->text_ms[1] += pk; s->text_n += 1;
    }
    const uint32_t *ctl = sl.h_text.as<uint32_t>();
    if (ctl[TXT_ILLEGAL])
        return fail(CHN_E_INVALID, W + ": illegal byte in the sequence of read " + std::to_string(ctl[TXT_FIRST_BAD]) + " (" + std::to_string(ctl[TXT_ILLEGAL]) +
                                       " illegal byte(s) in the batch; " + ((t->flags & CHN_TEXT_DNA5_RANKS) ? "dna5 ranks are 0 .. 4" : "only IUPAC nucleotide letters are accepted") + ")");
    sl.text_has_n = ctl[TXT_HAS_N] ? 1u : 0u;
    return CHN_OK;
}

extern "C" int chn_text_submit(chn_stream *s, const chn_text_batch *t) {
    if (!s || !t) return fail(CHN_E_INVALID, "chn_text_submit: null argument");
    if (s->idx->d.row_begin != 0 || s->idx->d.row_end != s->idx->d.bin_size)
        return fail(CHN_E_INVALID, "chn_text_submit needs an index object holding all rows");
    if (s->inflight >= chn_stream::N_SLOTS) return fail(CHN_E_STATE, "three batches already in flight: call chn_batch_wait first");
    if (s->shard_open || s->shx_stage) return fail(CHN_E_STATE, "chn_text_submit: a sharded batch is open");
    Slot &sl = s->slot[s->head];
    int rc = text_pack_run(s, sl, t, "chn_text_submit");
    if (rc) return rc;
    const bool quals = t->qual1_offset || t->qual2_offset;
    chn_batch b;
    std::memset(&b, 0, sizeof b);
    b.struct_size = sizeof b; b.n_reads = t->n_reads; b.n_bases = sl.text_n_bases;
    b.bases2 = sl.d_bases.as<uint32_t>();
    b.nmask = sl.text_has_n ? sl.d_nmask.as<uint32_t>() : nullptr;
    b.seg1_offset = sl.h_toff1.data(); b.seg1_length = t->seq1_length;
    if (t->seq2_offset) { b.seg2_offset = sl.h_toff2.data(); b.seg2_length = t->seq2_length; }
    b.mean_quality = quals ? reinterpret_cast<const float *>(sl.h_text.as<char>() + TEXT_MQ_AT) : nullptr;
    b.compression = t->compression; b.gzip_tallies = t->gzip_tallies; b.gzip_output = t->gzip_output;
    return submit_impl(s, &b, LIST_NONE, true);
}

extern "C" int chn_text_wait(chn_stream *s, chn_result *r, chn_text_result *t) {
    if (!s || !r || !t || t->struct_size != sizeof(chn_text_result)) return fail(CHN_E_INVALID, "chn_text_wait: bad argument");
    if (r->struct_size != sizeof(chn_result)) return fail(CHN_E_INVALID, "chn_text_wait: bad argument");
    if (s->inflight == 0) return fail(CHN_E_STATE, "no batch in flight");
    Slot &sl = s->slot[(s->head + chn_stream::N_SLOTS - s->inflight) % chn_stream::N_SLOTS];  // oldest batch in flight
    if (!sl.is_text) return fail(CHN_E_STATE, "chn_text_wait: the oldest batch in flight is not a text batch (use chn_batch_wait)");
    const int rc = chn_batch_wait(s, r);
    if (rc) return rc;
    t->has_n = sl.text_has_n; t->n_bases = sl.text_n_bases;
    if (t->mean_quality) {
        if (sl.h_mq.empty()) std::memset(t->mean_quality, 0, sl.n_reads * 4);
        else std::memcpy(t->mean_quality, sl.h_mq.data(), sl.n_reads * 4);
    }
    return CHN_OK;
}

extern "C" int chn_text_pack(chn_stream *s, const chn_text_batch *t, uint32_t *bases2, uint32_t *nmask, uint64_t *seg1_offset,
                             uint64_t *seg2_offset, float *mean_quality, uint64_t *n_bases, uint32_t *has_n) {
    if (!s || !t) return fail(CHN_E_INVALID, "chn_text_pack: null argument");
    if (s->inflight >= chn_stream::N_SLOTS) return fail(CHN_E_STATE, "chn_text_pack: three batches in flight, no free slot");
    if (s->shard_open || s->shx_stage) return fail(CHN_E_STATE, "chn_text_pack: a sharded batch is open");
    Slot &sl = s->slot[s->head];
    int rc = text_pack_run(s, sl, t, "chn_text_pack");
    if (rc) return rc;
    const uint64_t n = t->n_reads, nb = sl.text_n_bases;
    if (bases2) HIPCHK(hipMemcpy(bases2, sl.d_bases.p, nb / 4, hipMemcpyDeviceToHost));
    if (nmask) HIPCHK(hipMemcpy(nmask, sl.d_nmask.p, nb / 8, hipMemcpyDeviceToHost));
    if (seg1_offset) std::memcpy(seg1_offset, sl.h_toff1.data(), n * 8);
    if (seg2_offset && t->seq2_offset) std::memcpy(seg2_offset, sl.h_toff2.data(), n * 8);
    if (mean_quality) {
        if (t->qual1_offset || t->qual2_offset) std::memcpy(mean_quality, sl.h_text.as<char>() + TEXT_MQ_AT, n * 4);
        else std::memset(mean_quality, 0, n * 4);
    }
    if (n_bases) *n_bases = nb;
    if (has_n) *has_n = sl.text_has_n;
    return CHN_OK;
}
