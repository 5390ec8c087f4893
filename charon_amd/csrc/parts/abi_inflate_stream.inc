// abi_inflate_stream.inc -- chn_inflate_stream_run / chn_inflate_stream_run_host: chunks of one deflate stream (inflate_stream.inc)
// Part of the single translation unit charon_hip.hip (included in order, behind abi_inflate.inc); not a stand-alone source.
//
// chn_inflate_stream_run is one pass on the handle's run stream with two waits.  Up: the input from the 16-byte boundary in front of
// chunk 0 to its end, the begin / target bits and the caller's window (padded in front to 32 KiB).  k_inflate_chunks.  Down: 20 bytes a
// chunk -- boundary, symbols, status, BFINAL.  The host walks the counting rule over them (which chunks are proven, where their bytes go,
// which one does not fit) and cuts the proven chunks into pieces.  Up: the plan.  k_inflate_windows, k_inflate_bytes.  Down: a CRC-32 a
// piece and the smallest marker a chunk -- and the bytes, unless `out` is the caller's device memory.  The host applies the distance rule
// and joins the CRCs (infs_crc_join).  The buffers are the handle's, grow-only, apart from those of chn_inflate_run.

#ifdef __HIPCC__
struct InflateStreamState {
    DevBuf d_in, d_desc, d_res, d_sym, d_win, d_plan, d_pres, d_out, d_cursor;
    PinBuf h_desc, h_res, h_plan, h_pres;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // around step 1, around steps 2 and 3
};
static void inflate_stream_release(InflateStreamState *s) {
    if (!s) return;
    for (DevBuf *b : {&s->d_in, &s->d_desc, &s->d_res, &s->d_sym, &s->d_win, &s->d_plan, &s->d_pres, &s->d_out, &s->d_cursor}) b->release();
    for (PinBuf *b : {&s->h_desc, &s->h_res, &s->h_plan, &s->h_pres}) b->release();
    for (hipEvent_t e : s->ev) if (e) (void)hipEventDestroy(e);
    delete s;
}

#endif  // (what follows up to chn_inflate_stream_run also builds for the CPU alone: tools/fuzz/inflate_stream_fuzz.cpp)

static int inflate_stream_check(const chn_inflate_stream_job *j, const char *who, bool host_call) {
    const std::string W(who);
    if (!j) return fail(CHN_E_INVALID, W + ": null job");
    if (j->struct_size != sizeof(chn_inflate_stream_job)) return fail(CHN_E_INVALID, W + ": bad struct_size");
    if (j->flags & ~CHN_INFLATE_OUT_DEVICE) return fail(CHN_E_INVALID, W + ": unknown flag");
    if (host_call && j->flags) return fail(CHN_E_INVALID, W + ": CHN_INFLATE_OUT_DEVICE is for chn_inflate_stream_run (the CPU decoder writes host memory)");
    const uint64_t n = j->n_chunks;
    if (n > CHN_INFLATE_STREAM_MAX_CHUNKS) return fail(CHN_E_INVALID, W + ": n_chunks is above CHN_INFLATE_STREAM_MAX_CHUNKS");
    if (!j->n_counted || !j->out_used) return fail(CHN_E_INVALID, W + ": n_counted / out_used is NULL");
    if (n == 0) return CHN_OK;
    if (!j->begin_bit || !j->target_bit || !j->end_bit || !j->out_length || !j->status || !j->final) return fail(CHN_E_INVALID, W + ": a descriptor array is NULL");
    if (!j->in || (!j->out && j->out_bytes) || (!j->window && j->window_bytes)) return fail(CHN_E_INVALID, W + ": in / out / window is NULL");
    if (j->window_bytes > INFS_WIN) return fail(CHN_E_INVALID, W + ": window_bytes is above 32768");
    if (j->sym_capacity < CHN_INFLATE_STREAM_MIN_SYMS) return fail(CHN_E_INVALID, W + ": sym_capacity is below CHN_INFLATE_STREAM_MIN_SYMS");
    for (uint64_t i = 0; i < n; ++i) {
        const std::string M = W + ": chunk " + std::to_string(i);
        if (j->begin_bit[i] / 8 >= j->in_bytes) return fail(CHN_E_INVALID, M + " begins at or beyond the end of in");
        if (i && j->begin_bit[i] <= j->begin_bit[i - 1]) return fail(CHN_E_INVALID, M + " does not begin behind the chunk in front of it");
        if (j->target_bit[i] < j->begin_bit[i]) return fail(CHN_E_INVALID, M + " has its target in front of its begin");
    }
    return CHN_OK;
}

// the caller's window at the end of 32 KiB (zero bytes in front: never read -- the distance rule refuses what would resolve there)
static void infs_first_window(const chn_inflate_stream_job *j, uint8_t *w) {
    std::memset(w, 0, INFS_WIN - j->window_bytes);
    if (j->window_bytes) std::memcpy(w + INFS_WIN - j->window_bytes, j->window, j->window_bytes);
}
// window positions below this are in front of the member's first byte for a chunk with `before` bytes of the member in front of it
static inline uint32_t infs_lowest(uint64_t before) { return before >= INFS_WIN ? 0u : INFS_WIN - (uint32_t)before; }
static inline void infs_no_progress(const chn_inflate_stream_job *j, uint64_t k, uint32_t status) {
    j->status[k] = status; j->out_length[k] = 0; j->end_bit[k] = j->begin_bit[k]; j->final[k] = 0;
    if (j->crc32) j->crc32[k] = 0;
}

extern "C" int chn_inflate_stream_run_host(const chn_inflate_stream_job *j) {
    const char *who = "chn_inflate_stream_run_host";
    int rc = inflate_stream_check(j, who, true);
    if (rc) return rc;
    *j->n_counted = 0; *j->out_used = 0;
    const uint64_t n = j->n_chunks;
    if (n == 0) return CHN_OK;
    const uint32_t cap = (uint32_t)std::min<uint64_t>(j->sym_capacity, INFS_MAX_CAP);
    InfShared *sh = new (std::nothrow) InfShared;
    uint16_t *sym = static_cast<uint16_t *>(std::malloc((size_t)infs_stride(cap) * 2));  // (untouched pages cost nothing)
    std::vector<uint8_t> win(2 * INFS_WIN), buf(INFS_PIECE + 16);
    if (!sh || !sym) { delete sh; std::free(sym); return fail(CHN_E_NOMEM, std::string(who) + ": no memory for the decoder's tables and symbols"); }
    infs_first_window(j, win.data());
    uint64_t used = 0, counted = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t byte = j->begin_bit[k] >> 3;
        InfChunkHostPolicy pol;
        pol.in = j->in + byte; pol.len = j->in_bytes - byte; pol.bit0 = (uint32_t)(j->begin_bit[k] & 7);
        const InfsChunkResult r = infs_chunk(pol, *sh, sym, cap, k == 0 ? (uint32_t)j->window_bytes : INFS_WIN, byte, j->begin_bit[k], j->target_bit[k]);
        counted = k + 1;
        if (r.n_sym > j->out_bytes - used) { infs_no_progress(j, k, CHN_INFLATE_E_ROOM); break; }
        uint8_t *dst = j->out + used;
        uint32_t low = INFS_WIN, crc = 0;
        for (uint32_t f = 0; f < r.n_sym; f += INFS_PIECE) {
            const uint32_t len = std::min(r.n_sym - f, INFS_PIECE);
            const uint32_t l = infs_bytes(pol, sym + f, len, win.data(), buf.data());
            low = std::min(low, l);
            crc = infs_crc_join(crc, inf_crc32_at(pol, sh->ll, buf.data(), 0, len), len);
            std::memcpy(dst + f, buf.data(), len);
        }
        if (k > 0 && low < infs_lowest(j->window_bytes + used)) { infs_no_progress(j, k, INF_E_SYMBOL); break; }
        j->end_bit[k] = r.end_bit; j->out_length[k] = r.n_sym; j->status[k] = r.status; j->final[k] = (uint8_t)r.final;
        if (j->crc32) j->crc32[k] = crc;
        // the next chunk's window: the last 32 KiB of (window | these bytes)
        if (r.n_sym >= INFS_WIN) std::memcpy(win.data(), dst + r.n_sym - INFS_WIN, INFS_WIN);
        else if (r.n_sym) { std::memmove(win.data(), win.data() + r.n_sym, INFS_WIN - r.n_sym); std::memcpy(win.data() + INFS_WIN - r.n_sym, dst, r.n_sym); }
        used += r.n_sym;
        if (r.status != 0 || r.final || k + 1 == n || r.end_bit != j->begin_bit[k + 1]) break;
    }
    delete sh;
    std::free(sym);
    *j->n_counted = counted; *j->out_used = used;
    return CHN_OK;
}

#ifdef __HIPCC__
extern "C" int chn_inflate_stream_run(chn_inflate *h, const chn_inflate_stream_job *j) {
    const char *who = "chn_inflate_stream_run";
    if (!h) return fail(CHN_E_INVALID, std::string(who) + ": null handle");
    int rc = inflate_stream_check(j, who, false);
    if (rc) return rc;
    const uint64_t n = j->n_chunks;
    const bool dev_out = (j->flags & CHN_INFLATE_OUT_DEVICE) != 0;
    HIPCHK(hipSetDevice(h->device));
    if (n && dev_out && j->out_bytes) {  // before anything is launched
        std::string why;
        if (!device_memory_of(j->out, j->out_bytes, h->device, why)) return fail(CHN_E_INVALID, std::string(who) + ": CHN_INFLATE_OUT_DEVICE: out " + why);
    }
    *j->n_counted = 0; *j->out_used = 0;
    h->kernel_ms = 0;
    if (n == 0) return CHN_OK;
    if (!h->ss) {
        h->ss = new (std::nothrow) InflateStreamState;
        if (!h->ss) return fail(CHN_E_NOMEM, std::string(who) + ": no memory");
        for (hipEvent_t &e : h->ss->ev)
            if (hipEventCreate(&e) != hipSuccess) { inflate_stream_release(h->ss); h->ss = nullptr; return fail(CHN_E_HIP, std::string(who) + ": hipEventCreate failed"); }
    }
    InflateStreamState &s = *h->ss;
    hipStream_t q = h->s_run;
    const uint32_t cap = (uint32_t)std::min<uint64_t>(j->sym_capacity, INFS_MAX_CAP);
    const uint64_t stride = infs_stride(cap);
    const uint64_t first = (j->begin_bit[0] >> 3) & ~15ull, up = j->in_bytes - first;
    const size_t desc_bytes = (size_t)n * 16 + INFS_WIN, res_bytes = (size_t)n * 20;
    if ((rc = s.d_in.ensure_grow((size_t)up + INF_PAD, (size_t)(up / 4))) || (rc = s.h_desc.ensure(desc_bytes)) || (rc = s.d_desc.ensure(desc_bytes)) ||
        (rc = s.h_res.ensure(res_bytes)) || (rc = s.d_res.ensure(res_bytes)) || (rc = s.d_sym.ensure((size_t)(n * stride * 2))) ||
        (rc = s.d_win.ensure((size_t)(n + 1) * INFS_WIN)) || (rc = s.d_cursor.ensure(16)))
        return rc;
    // step 1
    uint64_t *hb = s.h_desc.as<uint64_t>();
    std::memcpy(hb, j->begin_bit, (size_t)n * 8);
    std::memcpy(hb + n, j->target_bit, (size_t)n * 8);
    infs_first_window(j, reinterpret_cast<uint8_t *>(hb + 2 * n));
    HIPCHK(hipMemcpyAsync(s.d_in.p, j->in + first, up, hipMemcpyHostToDevice, q));
    HIPCHK(hipMemsetAsync(s.d_in.as<uint8_t>() + up, 0, INF_PAD, q));
    HIPCHK(hipMemcpyAsync(s.d_desc.p, hb, (size_t)n * 16, hipMemcpyHostToDevice, q));
    HIPCHK(hipMemcpyAsync(s.d_win.p, hb + 2 * n, INFS_WIN, hipMemcpyHostToDevice, q));
    HIPCHK(hipMemsetAsync(s.d_cursor.p, 0, 4, q));
    InflateChunkArgs a;
    a.in = s.d_in.as<uint8_t>(); a.first = first; a.in_bytes = j->in_bytes;
    a.begin_bit = s.d_desc.as<uint64_t>(); a.target_bit = a.begin_bit + n;
    a.sym = s.d_sym.as<uint16_t>(); a.cap = cap; a.before0 = (uint32_t)j->window_bytes;
    a.end_bit = s.d_res.as<uint64_t>();
    a.n_sym = reinterpret_cast<uint32_t *>(a.end_bit + n); a.status = a.n_sym + n; a.final = a.status + n;
    a.cursor = s.d_cursor.as<uint32_t>(); a.n = (uint32_t)n;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(n, (uint64_t)std::max(1, h->cus) * 2);  // two workgroups fit a CU's LDS
    HIPCHK(hipEventRecord(s.ev[0], q));
    hipLaunchKernelGGL(k_inflate_chunks, dim3(blocks), dim3(WAVE), 0, q, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s.ev[1], q));
    HIPCHK(hipMemcpyAsync(s.h_res.p, s.d_res.p, res_bytes, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
    h->kernel_ms = ms;
    const uint64_t *r_end = s.h_res.as<uint64_t>();
    const uint32_t *r_sym = reinterpret_cast<const uint32_t *>(r_end + n), *r_status = r_sym + n, *r_final = r_status + n;
    // the counting rule: chunks [0, counted) are proven, the bytes of chunks [0, made) are made
    uint64_t counted = 0, made = 0, used = 0, no_room = n, pieces = 0;
    std::vector<uint64_t> off((size_t)n);
    for (uint64_t k = 0; k < n; ++k) {
        counted = k + 1;
        if (r_sym[k] > j->out_bytes - used) { no_room = k; break; }
        off[(size_t)k] = used; used += r_sym[k]; made = k + 1;
        pieces += (r_sym[k] + INFS_PIECE - 1) / INFS_PIECE;
        if (r_status[k] != 0 || r_final[k] || k + 1 == n || r_end[k] != j->begin_bit[k + 1]) break;
    }
    // steps 2 and 3
    const size_t plan_bytes = (size_t)(made + pieces) * 8, pres_bytes = (size_t)(pieces + made) * 4;
    const uint32_t *p_crc = nullptr, *p_low = nullptr;
    if (pieces) {
        if ((rc = s.h_plan.ensure(plan_bytes + plan_bytes / 4)) || (rc = s.d_plan.ensure(s.h_plan.cap)) || (rc = s.h_pres.ensure(pres_bytes + pres_bytes / 4)) ||
            (rc = s.d_pres.ensure(s.h_pres.cap)) || (!dev_out && (rc = s.d_out.ensure_grow((size_t)used, (size_t)(used / 4)))))
            return rc;
        uint64_t *plan = s.h_plan.as<uint64_t>(), *pc = plan + made;
        for (uint64_t k = 0; k < made; ++k) {
            plan[k] = off[(size_t)k];
            for (uint32_t f = 0; f < r_sym[k]; f += INFS_PIECE) *pc++ = (k << 32) | f;
        }
        HIPCHK(hipMemcpyAsync(s.d_plan.p, plan, plan_bytes, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemsetAsync(s.d_pres.p, 0xFF, pres_bytes, q));
        HIPCHK(hipEventRecord(s.ev[2], q));
        if (made > 1) {
            InflateWindowArgs w;
            w.sym = s.d_sym.as<uint16_t>(); w.stride = stride; w.n_sym = a.n_sym; w.win = s.d_win.as<uint8_t>(); w.n = (uint32_t)(made - 1);
            hipLaunchKernelGGL(k_inflate_windows, dim3(1), dim3(INFS_WIN_THREADS), 0, q, w);
            HIPCHK(hipGetLastError());
        }
        InflateBytesArgs b;
        b.sym = s.d_sym.as<uint16_t>(); b.stride = stride; b.win = s.d_win.as<uint8_t>();
        b.out = dev_out ? j->out : s.d_out.as<uint8_t>();
        b.out_off = s.d_plan.as<uint64_t>(); b.piece = b.out_off + made; b.n_sym = a.n_sym;
        b.crc = s.d_pres.as<uint32_t>(); b.low = b.crc + pieces;
        hipLaunchKernelGGL(k_inflate_bytes, dim3((uint32_t)pieces), dim3(WAVE), 0, q, b);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(s.ev[3], q));
        HIPCHK(hipMemcpyAsync(s.h_pres.p, s.d_pres.p, pres_bytes, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        HIPCHK(hipEventElapsedTime(&ms, s.ev[2], s.ev[3]));
        h->kernel_ms += ms;
        p_crc = s.h_pres.as<uint32_t>(); p_low = p_crc + pieces;
    }
    // the distance rule, over the chunks behind the first
    uint64_t far = n;
    for (uint64_t k = 1; k < made; ++k)
        if (p_low && p_low[k] < infs_lowest(j->window_bytes + off[(size_t)k])) { far = k; counted = k + 1; made = k; used = off[(size_t)k]; no_room = n; break; }
    for (uint64_t k = 0; k < n; ++k) {  // (the unproven chunks: what their wavefronts found)
        j->end_bit[k] = r_end[k]; j->out_length[k] = r_sym[k]; j->status[k] = r_status[k]; j->final[k] = (uint8_t)r_final[k];
    }
    if (j->crc32) {
        uint64_t pi = 0;
        for (uint64_t k = 0; k < made; ++k) {
            uint32_t crc = 0;
            for (uint32_t f = 0; f < r_sym[k]; f += INFS_PIECE) crc = infs_crc_join(crc, p_crc[pi++], std::min(r_sym[k] - f, INFS_PIECE));
            j->crc32[k] = crc;
        }
    }
    if (no_room < n) infs_no_progress(j, no_room, CHN_INFLATE_E_ROOM);
    if (far < n) infs_no_progress(j, far, INF_E_SYMBOL);
    if (!dev_out && used) {
        HIPCHK(hipMemcpyAsync(j->out, s.d_out.p, used, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
    }
    *j->n_counted = counted; *j->out_used = used;
    return CHN_OK;
}
#endif
