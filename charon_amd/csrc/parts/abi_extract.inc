// abi_extract.inc -- chn_extract_*: the records of one --extract file formed and deflated in device memory
// Part of the single translation unit charon_hip.hip (included in order, behind abi_deflate.inc); not a stand-alone source.
//
// A chn_extract owns a chn_deflate (its three streams, its two sets of compressor buffers) and `pend`, a grow-only device buffer that
// holds the file's text behind the last cut: `pending` bytes at its front between calls.  An append
//   1. writes its bytes at pend + pending on the upload stream: k_extract_records out of the caller's device text (44 bytes of
//      descriptors a record go up first), or one copy of the caller's host bytes;
//   2. hands every whole piece to deflate_launch in groups, as chn_deflate_run does -- the group's descriptors (piece k at
//      k * 65 280) follow the bytes on the upload stream, the compressor reads `pend` in place, group g is collected when group g + 1
//      has been issued (deflate_collect) -- and downloads the members behind one another into `out`;
//   3. moves the tail to the front on the run stream, behind the last group's kernels, and waits for everything.
// `pend` always has 16 readable bytes behind the text (DeflateArgs::in); k_deflate_members ignores what they hold.

struct chn_extract {
    int device = 0;
    chn_deflate *dfl = nullptr;
    DevBuf pend, d_desc;
    PinBuf h_desc, h_bytes;
    uint64_t pending = 0;         // bytes of text at the front of `pend`
    hipEvent_t r0 = nullptr, r1 = nullptr;
    double kernel_ms = 0;
    bool broken = false;          // a HIP call failed with work queued: the buffer's content is not known any more
};

extern "C" int chn_extract_destroy(chn_extract *h) {
    if (!h) return CHN_OK;
    (void)hipSetDevice(h->device);
    if (h->dfl) (void)chn_deflate_destroy(h->dfl);  // (waits for the streams)
    h->pend.release(); h->d_desc.release(); h->h_desc.release(); h->h_bytes.release();
    for (hipEvent_t ev : {h->r0, h->r1}) if (ev) (void)hipEventDestroy(ev);
    delete h;
    return CHN_OK;
}

extern "C" int chn_extract_create(int32_t device, chn_extract **out) {
    if (!out) return fail(CHN_E_INVALID, "chn_extract_create: null argument");
    *out = nullptr;
    chn_extract *h = new (std::nothrow) chn_extract;
    if (!h) return fail(CHN_E_NOMEM, "chn_extract_create: no memory");
    int rc = chn_deflate_create(device, &h->dfl);  // (checks `device` and selects it)
    if (rc) { delete h; return rc; }
    h->device = device;
    hipError_t e = hipEventCreate(&h->r0);
    if (e == hipSuccess) e = hipEventCreate(&h->r1);
    if (e != hipSuccess) {
        const std::string msg = std::string("chn_extract_create: ") + hipGetErrorString(e);
        chn_extract_destroy(h);
        return fail(CHN_E_HIP, msg);
    }
    *out = h;
    return CHN_OK;
}

extern "C" int chn_extract_bound(const chn_extract *h, uint64_t appended_bytes, uint64_t *out_bytes) {
    if (!h || !out_bytes) return fail(CHN_E_INVALID, "chn_extract_bound: null argument");
    *out_bytes = xr_bound(h->pending, appended_bytes);
    return CHN_OK;
}

extern "C" int chn_extract_records_host(chn_extract_job *job, uint8_t *text_out, uint64_t capacity, uint64_t *bytes) {
    std::string why;
    const int rc = xr_host_job(job, text_out, capacity, bytes, why);
    return rc ? fail(rc, why) : CHN_OK;
}

// room for `have` bytes of text in `pend` (and 16 readable bytes behind them); what is pending moves along
static int extract_reserve(chn_extract *h, uint64_t have) {
    const size_t need = (size_t)((have + 15) & ~(uint64_t)15) + 16;
    if (need <= h->pend.cap) return CHN_OK;
    DevBuf bigger;
    const int rc = bigger.ensure(need + need / 4);
    if (rc) return rc;
    if (h->pending) {
        const hipError_t e = hipMemcpy(bigger.p, h->pend.p, h->pending, hipMemcpyDeviceToDevice);
        const hipError_t w = hipStreamSynchronize(nullptr);  // (a device-to-device hipMemcpy may return early)
        if (e != hipSuccess || w != hipSuccess) { bigger.release(); return fail(CHN_E_HIP, std::string("chn_extract: ") + hipGetErrorString(e != hipSuccess ? e : w)); }
    }
    h->pend.release();
    h->pend = bigger;
    return CHN_OK;
}

// Steps 2 and 3 of an append, and chn_extract_finish: `have` bytes of text lie at the front of `pend`, the last of them written by work
// queued on the upload stream.  Compress `pieces` whole pieces -- or, `last` set, the `have` < XR_PIECE bytes as one shorter member --
// into out, and keep the `tail` bytes behind the pieces.  Returns with nothing queued.
static int extract_compress(chn_extract *h, uint64_t have, uint64_t pieces, uint64_t tail, bool last, uint8_t *out, uint64_t out_capacity, uint64_t *out_used) {
    chn_deflate *d = h->dfl;
    const bool out_pinned = out && out_capacity && page_locked_host(out, out_capacity);
    const uint64_t members = last ? 1 : pieces;
    uint64_t first = 0, g = 0, used = 0;
    int rc = CHN_OK;
    // (not run_groups: the tail moves between the last issue and the last collect, and the streams are waited for whatever happened)
    const auto collect = [&](DeflateSet &st) {
        return deflate_collect(d, st, st.n * XR_PIECE, CHN_DEFLATE_BGZF, out, out_pinned, &used, &h->kernel_ms, "chn_extract", "piece", " of the call");
    };
    while (first < members) {
        const uint64_t n = std::min<uint64_t>(d->group_members, members - first);
        const uint64_t in_total = last ? have : n * XR_PIECE;
        DeflateSet &st = d->set[g & 1];  // (free: its last group was collected when the one after it was issued)
        st.first = first; st.n = n;
        if ((rc = deflate_ensure(d, st, n, in_total, CHN_DEFLATE_BGZF))) break;
        uint64_t *in_off = st.h_desc.as<uint64_t>();
        uint32_t *in_len = reinterpret_cast<uint32_t *>(in_off + n);
        for (uint64_t k = 0; k < n; ++k) { in_off[k] = (first + k) * XR_PIECE; in_len[k] = last ? (uint32_t)have : (uint32_t)XR_PIECE; }
        hipError_t e = hipMemcpyAsync(st.d_desc.p, st.h_desc.p, (size_t)n * 12, hipMemcpyHostToDevice, d->s_up);
        if (e == hipSuccess) e = hipMemsetAsync(st.d_cursor.p, 0, 4, d->s_up);
        if (e == hipSuccess) e = hipEventRecord(st.up, d->s_up);
        if (e != hipSuccess) { rc = fail(CHN_E_HIP, std::string("chn_extract: ") + hipGetErrorString(e)); break; }
        rc = deflate_launch(d, st, h->pend.as<uint8_t>(), n, in_total, CHN_DEFLATE_BGZF);
        if (rc == CHN_OK && g > 0) rc = collect(d->set[(g - 1) & 1]);
        if (rc) break;
        first += n; ++g;
    }
    if (rc == CHN_OK && !last && pieces && tail) {  // behind the last group's kernels; old and new place cannot overlap (tail < XR_PIECE <= pieces * XR_PIECE)
        const hipError_t e = hipMemcpyAsync(h->pend.p, h->pend.as<uint8_t>() + pieces * XR_PIECE, tail, hipMemcpyDeviceToDevice, d->s_run);
        if (e != hipSuccess) rc = fail(CHN_E_HIP, std::string("chn_extract: ") + hipGetErrorString(e));
    }
    if (rc == CHN_OK && g > 0) rc = collect(d->set[(g - 1) & 1]);
    // nothing of this call stays queued, whatever happened
    const hipError_t w0 = hipStreamSynchronize(d->s_up), w1 = hipStreamSynchronize(d->s_run), w2 = hipStreamSynchronize(d->s_down);
    d->set[0].busy = d->set[1].busy = false;
    if (rc == CHN_OK)
        for (hipError_t w : {w0, w1, w2}) if (w != hipSuccess) { rc = fail(CHN_E_HIP, std::string("chn_extract: ") + hipGetErrorString(w)); break; }
    if (rc) { h->broken = true; return rc; }
    h->pending = last ? 0 : tail;
    *out_used = used;
    return CHN_OK;
}

static int extract_usable(const chn_extract *h, const char *who) {
    if (!h) return fail(CHN_E_INVALID, std::string(who) + ": null handle");
    if (h->broken) return fail(CHN_E_INVALID, std::string(who) + ": an earlier call on this handle failed inside the device work: destroy it");
    return CHN_OK;
}

static int extract_capacity(const chn_extract *h, const char *who, uint64_t appended, const uint8_t *out, uint64_t out_capacity) {
    const uint64_t need = xr_bound(h->pending, appended);
    if (out_capacity < need)
        return fail(CHN_E_CAPACITY, std::string(who) + ": the members may need " + std::to_string(need) + " bytes (chn_extract_bound), out_capacity is " + std::to_string(out_capacity));
    if (need && !out) return fail(CHN_E_INVALID, std::string(who) + ": out is NULL");
    return CHN_OK;
}

extern "C" int chn_extract_append_records(chn_extract *h, chn_extract_job *j) {
    const char *who = "chn_extract_append_records";
    int rc = extract_usable(h, who);
    if (rc) return rc;
    std::string why;
    uint64_t total = 0;
    if ((rc = xr_check_job(j, who, why, total))) return fail(rc, why);
    HIPCHK(hipSetDevice(h->device));
    if ((rc = device_text_check(j->text, j->text_bytes, h->device, who))) return rc;
    if ((rc = extract_capacity(h, who, total, j->out, j->out_capacity))) return rc;
    h->kernel_ms = 0;
    j->out_used = 0;
    const uint64_t n = j->n_records;
    if (n == 0) return CHN_OK;
    chn_deflate *d = h->dfl;
    const XrPlan plan = xr_plan_append(h->pending, total);
    // descriptors in one block: id_off seq_off qual_off dst_off [n] (64-bit), id_len seq_len qual_len [n] (32-bit)
    const size_t desc_bytes = (size_t)n * 44;
    if ((rc = extract_reserve(h, h->pending + total)) || (rc = h->h_desc.ensure(desc_bytes)) || (rc = h->d_desc.ensure(desc_bytes))) return rc;
    uint64_t *h_off = h->h_desc.as<uint64_t>();
    uint32_t *h_len = reinterpret_cast<uint32_t *>(h_off + 4 * n);
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; ++i) {
        h_off[i] = j->id_offset[i]; h_off[n + i] = j->seq_offset[i]; h_off[2 * n + i] = j->qual_offset[i]; h_off[3 * n + i] = at;
        h_len[i] = j->id_length[i]; h_len[n + i] = j->seq_length[i]; h_len[2 * n + i] = j->qual_length[i];
        at += xr_record_bytes(j->id_length[i], j->seq_length[i], j->qual_length[i]);
    }
    XrArgs a;
    const uint64_t *d_off = h->d_desc.as<uint64_t>();
    const uint32_t *d_len = reinterpret_cast<const uint32_t *>(d_off + 4 * n);
    a.text = j->text;
    a.id_off = d_off; a.seq_off = d_off + n; a.qual_off = d_off + 2 * n; a.dst_off = d_off + 3 * n;
    a.id_len = d_len; a.seq_len = d_len + n; a.qual_len = d_len + 2 * n;
    a.n = n; a.out = h->pend.as<uint8_t>(); a.out_base = h->pending;
    // a looping grid; the cap of 16 wavefronts a CU is a guess (k_text_gather's), not a measured optimum
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(n, (uint64_t)std::max(1, d->cus) * 16);
    hipError_t e = hipMemcpyAsync(h->d_desc.p, h->h_desc.p, desc_bytes, hipMemcpyHostToDevice, d->s_up);
    if (e == hipSuccess) e = hipEventRecord(h->r0, d->s_up);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_extract_records, dim3(blocks), dim3(WAVE), 0, d->s_up, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(h->r1, d->s_up);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(d->s_up);
        h->broken = true;
        return fail(CHN_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    if ((rc = extract_compress(h, h->pending + total, plan.pieces, plan.tail, false, j->out, j->out_capacity, &j->out_used))) return rc;
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, h->r0, h->r1));
    h->kernel_ms += ms;
    return CHN_OK;
}

extern "C" int chn_extract_append_bytes(chn_extract *h, const uint8_t *bytes, uint64_t n, uint8_t *out, uint64_t out_capacity, uint64_t *out_used) {
    const char *who = "chn_extract_append_bytes";
    int rc = extract_usable(h, who);
    if (rc) return rc;
    if (!out_used) return fail(CHN_E_INVALID, std::string(who) + ": out_used is NULL");
    if (n && !bytes) return fail(CHN_E_INVALID, std::string(who) + ": bytes is NULL");
    if ((rc = extract_capacity(h, who, n, out, out_capacity))) return rc;
    h->kernel_ms = 0;
    *out_used = 0;
    if (n == 0) return CHN_OK;
    HIPCHK(hipSetDevice(h->device));
    chn_deflate *d = h->dfl;
    const XrPlan plan = xr_plan_append(h->pending, n);
    if ((rc = extract_reserve(h, h->pending + n))) return rc;
    const uint8_t *src = bytes;
    if (!page_locked_host(bytes, n)) {  // through page-locked staging, so that the copy is a stream's like everything behind it
        if ((rc = h->h_bytes.ensure_grow((size_t)n, (size_t)(n / 4)))) return rc;
        std::memcpy(h->h_bytes.p, bytes, n);
        src = h->h_bytes.as<uint8_t>();
    }
    const hipError_t e = hipMemcpyAsync(h->pend.as<uint8_t>() + h->pending, src, n, hipMemcpyHostToDevice, d->s_up);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(d->s_up);
        h->broken = true;
        return fail(CHN_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    return extract_compress(h, h->pending + n, plan.pieces, plan.tail, false, out, out_capacity, out_used);
}

extern "C" int chn_extract_finish(chn_extract *h, uint8_t *out, uint64_t out_capacity, uint64_t *out_used) {
    const char *who = "chn_extract_finish";
    int rc = extract_usable(h, who);
    if (rc) return rc;
    if (!out_used) return fail(CHN_E_INVALID, std::string(who) + ": out_used is NULL");
    if ((rc = extract_capacity(h, who, 0, out, out_capacity))) return rc;
    h->kernel_ms = 0;
    *out_used = 0;
    if (h->pending == 0) return CHN_OK;
    HIPCHK(hipSetDevice(h->device));
    return extract_compress(h, h->pending, 0, 0, true, out, out_capacity, out_used);
}

extern "C" int chn_extract_kernel_ms(chn_extract *h, double *ms) {
    if (!h || !ms) return fail(CHN_E_INVALID, "chn_extract_kernel_ms: null argument");
    *ms = h->kernel_ms;
    return CHN_OK;
}
