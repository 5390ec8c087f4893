// abi_inflate.inc -- chn_inflate_create / chn_inflate_run[_crc] / chn_inflate_run_host[_crc] / chn_inflate_destroy: raw deflate members on the device
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.
//
// chn_inflate_run works through a job in groups of members (about 32 MiB of output each) on three streams of the handle's own:
// while group g is decoded, the compressed bytes of group g + 1 are packed into page-locked staging (member by member, each on a
// 16-byte boundary, so nothing of `in` between or around the members is uploaded) and uploaded, and the output of group g - 1 is
// downloaded -- straight into `out` where that is page-locked and the group's members lie back to back there, through staging otherwise.
// Two sets of grow-only buffers take turns.  The handle is a CodecPipe and the loop is run_groups (abi_device_call.inc).
// With a chn_inflate_crc that names an array, the CRC form of the kernel runs: `expected` travels behind the descriptors in their
// upload, the CRCs behind the statuses in their download -- no further copy, launch or wait.
// With CHN_INFLATE_OUT_DEVICE `out` is the caller's device memory: the kernel writes every member to out + out_offset[i] itself (its
// write-out handles any misalignment and never leaves the member's stretch), nothing of the output is staged or downloaded, and the
// wait for the statuses is the wait for the bytes.

static const uint64_t INF_GROUP_OUT = 32ull << 20, INF_GROUP_IN = 64ull << 20;
static const uint32_t INF_GROUP_MEMBERS = 1u << 16;

struct InflateSet {
    DevBuf d_in, d_out, d_desc, d_status, d_cursor;
    PinBuf h_in, h_out, h_desc, h_status;
    hipEvent_t up = nullptr, done = nullptr, down = nullptr, k0 = nullptr, k1 = nullptr;
    uint64_t first = 0, n = 0, out_bytes = 0;  // the group in this set
    bool direct = false, busy = false, crc = false, dev_out = false;
    int make_events(const char *who) { return events_create(who, {&up, &done, &down}, {&k0, &k1}); }
    void release() {
        for (DevBuf *b : {&d_in, &d_out, &d_desc, &d_status, &d_cursor}) b->release();
        for (PinBuf *b : {&h_in, &h_out, &h_desc, &h_status}) b->release();
        events_destroy({&up, &done, &down, &k0, &k1});
    }
};
struct InflateStreamState;  // chn_inflate_stream_run's buffers (abi_inflate_stream.inc), made by its first call
static void inflate_stream_release(InflateStreamState *s);
struct chn_inflate : CodecPipe {
    InflateSet set[2];
    double kernel_ms = 0;  // device time of the last run's kernels
    InflateStreamState *ss = nullptr;
};

static int inflate_check_job(const chn_inflate_job *j, const char *who, bool host_call) {
    const std::string W(who);
    if (!j) return fail(CHN_E_INVALID, W + ": null job");
    if (j->struct_size != sizeof(chn_inflate_job)) return fail(CHN_E_INVALID, W + ": bad struct_size");
    if (j->flags & ~CHN_INFLATE_OUT_DEVICE) return fail(CHN_E_INVALID, W + ": unknown flag");
    if (host_call && j->flags) return fail(CHN_E_INVALID, W + ": CHN_INFLATE_OUT_DEVICE is for chn_inflate_run / chn_inflate_run_crc (the CPU decoder writes host memory)");
    const uint64_t n = j->n_members;
    if (n == 0) return CHN_OK;
    if (!j->in_offset || !j->in_length || !j->out_offset || !j->out_length || !j->status) return fail(CHN_E_INVALID, W + ": a descriptor array is NULL");
    if ((!j->in && j->in_bytes) || (!j->out && j->out_bytes)) return fail(CHN_E_INVALID, W + ": in / out is NULL");
    uint64_t out_end = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const std::string M = W + ": member " + std::to_string(i);
        if (j->in_offset[i] > j->in_bytes || j->in_length[i] > j->in_bytes - j->in_offset[i]) return fail(CHN_E_INVALID, M + " reaches beyond in_bytes");
        if (j->out_length[i] > CHN_INFLATE_MAX_OUT) return fail(CHN_E_INVALID, M + " has out_length above CHN_INFLATE_MAX_OUT");
        if (j->out_offset[i] > j->out_bytes || j->out_length[i] > j->out_bytes - j->out_offset[i]) return fail(CHN_E_INVALID, M + " reaches beyond out_bytes");
        if (j->out_offset[i] < out_end) return fail(CHN_E_INVALID, M + " overlaps the output of the member in front of it");
        out_end = j->out_offset[i] + j->out_length[i];
    }
    return CHN_OK;
}

static int inflate_check_crc(const chn_inflate_crc *c, const char *who) {
    if (!c) return CHN_OK;
    if (c->struct_size != sizeof(chn_inflate_crc)) return fail(CHN_E_INVALID, std::string(who) + ": bad struct_size of the chn_inflate_crc");
    if (c->reserved) return fail(CHN_E_INVALID, std::string(who) + ": chn_inflate_crc.reserved is not 0");
    return CHN_OK;
}

static int inflate_run_host(const chn_inflate_job *j, const chn_inflate_crc *c, const char *who) {
    int rc = inflate_check_crc(c, who);
    if (rc == CHN_OK) rc = inflate_check_job(j, who, true);
    if (rc || j->n_members == 0) return rc;
    const bool want = c && (c->expected || c->crc32);
    InfShared *sh = new (std::nothrow) InfShared;
    if (!sh) return fail(CHN_E_NOMEM, std::string(who) + ": no memory for the decoder's tables");
    for (uint64_t i = 0; i < j->n_members; ++i) {
        uint32_t crc = 0;
        uint32_t st = (uint32_t)inf_member_host(*sh, j->in + j->in_offset[i], j->in_length[i], j->out + j->out_offset[i], j->out_length[i], want ? &crc : nullptr);
        if (want && st == 0) {
            if (c->expected && crc != c->expected[i]) st = CHN_INFLATE_E_CRC;
            if (c->crc32) c->crc32[i] = crc;
        }
        j->status[i] = st;
    }
    delete sh;
    return CHN_OK;
}
extern "C" int chn_inflate_run_host(const chn_inflate_job *j) { return inflate_run_host(j, nullptr, "chn_inflate_run_host"); }
extern "C" int chn_inflate_run_host_crc(const chn_inflate_job *j, const chn_inflate_crc *c) { return inflate_run_host(j, c, "chn_inflate_run_host_crc"); }

extern "C" int chn_inflate_create(int32_t device, chn_inflate **out) { return codec_create(device, out, "chn_inflate_create", chn_inflate_destroy); }

extern "C" int chn_inflate_destroy(chn_inflate *h) {
    if (!h) return CHN_OK;
    (void)hipSetDevice(h->device);
    h->drain();
    for (InflateSet &st : h->set) st.release();
    inflate_stream_release(h->ss);
    h->destroy();
    delete h;
    return CHN_OK;
}

// pack, upload, decode and start the download of members [first, first + n) in set `st`
static int inflate_issue(chn_inflate *h, InflateSet &st, const chn_inflate_job *j, const chn_inflate_crc *c, uint64_t first, uint64_t n, bool out_pinned) {
    uint64_t in_bytes = 0, out_bytes = 0;
    bool contiguous = true;
    for (uint64_t i = first; i < first + n; ++i) {
        in_bytes += ((uint64_t)j->in_length[i] + 15) & ~15ull;
        if (i > first && j->out_offset[i] != j->out_offset[i - 1] + j->out_length[i - 1]) contiguous = false;
        out_bytes += j->out_length[i];
    }
    st.dev_out = (j->flags & CHN_INFLATE_OUT_DEVICE) != 0;
    st.first = first; st.n = n; st.out_bytes = out_bytes; st.direct = st.dev_out || (out_pinned && contiguous);
    st.crc = c != nullptr;
    const bool expect = c && c->expected;
    int rc;
    // descriptors in one block: in_off[n] out_off[n] (64-bit), in_len[n] out_len[n] (32-bit), and expected[n] where CRCs are compared;
    // statuses in one block: status[n], and crc[n] behind them where CRCs are taken
    const size_t desc_bytes = (size_t)n * (expect ? 28 : 24), status_bytes = (size_t)n * (st.crc ? 8 : 4);
    if ((rc = st.h_desc.ensure(desc_bytes + desc_bytes / 4)) || (rc = st.d_desc.ensure(st.h_desc.cap)) ||
        (rc = st.h_in.ensure_grow((size_t)in_bytes + 2 * INF_PAD, (size_t)(in_bytes / 4))) || (rc = st.d_in.ensure(st.h_in.cap)) ||
        (!st.dev_out && (rc = st.d_out.ensure_grow((size_t)out_bytes + 64, (size_t)(out_bytes / 4)))) ||
        (rc = st.h_status.ensure_grow(status_bytes, status_bytes / 4)) || (rc = st.d_status.ensure(st.h_status.cap)) || (rc = st.d_cursor.ensure(16)))
        return rc;
    if (!st.direct && (rc = st.h_out.ensure(st.d_out.cap))) return rc;
    uint64_t *in_off = st.h_desc.as<uint64_t>(), *out_off = in_off + n;
    uint32_t *in_len = reinterpret_cast<uint32_t *>(out_off + n), *out_len = in_len + n;
    uint8_t *stage = st.h_in.as<uint8_t>();
    std::memset(stage, 0, INF_PAD);
    uint64_t ip = INF_PAD, op = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t i = first + k;
        in_off[k] = ip; in_len[k] = j->in_length[i];
        out_off[k] = st.dev_out ? j->out_offset[i] : op; out_len[k] = j->out_length[i];
        if (j->in_length[i]) std::memcpy(stage + ip, j->in + j->in_offset[i], j->in_length[i]);
        ip += ((uint64_t)j->in_length[i] + 15) & ~15ull;
        op += j->out_length[i];
    }
    std::memset(stage + ip, 0, INF_PAD);
    if (expect) std::memcpy(out_len + n, c->expected + first, (size_t)n * 4);
    HIPCHK(hipMemcpyAsync(st.d_in.p, stage, ip + INF_PAD, hipMemcpyHostToDevice, h->s_up));
    HIPCHK(hipMemcpyAsync(st.d_desc.p, st.h_desc.p, desc_bytes, hipMemcpyHostToDevice, h->s_up));
    HIPCHK(hipMemsetAsync(st.d_cursor.p, 0, 4, h->s_up));
    HIPCHK(hipEventRecord(st.up, h->s_up));
    HIPCHK(hipStreamWaitEvent(h->s_run, st.up, 0));
    InflateArgs a;
    a.in = st.d_in.as<uint8_t>();
    a.in_off = st.d_desc.as<uint64_t>(); a.out_off = a.in_off + n;
    a.in_len = reinterpret_cast<const uint32_t *>(a.out_off + n); a.out_len = a.in_len + n;
    a.out = st.dev_out ? j->out : st.d_out.as<uint8_t>(); a.status = st.d_status.as<uint32_t>(); a.cursor = st.d_cursor.as<uint32_t>();
    a.n = (uint32_t)n;
    a.expected = expect ? a.out_len + n : nullptr;
    a.crc = st.crc ? a.status + n : nullptr;
    // a looping grid: two workgroups of one wavefront fit a CU's LDS; the cursor hands out members
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(n, (uint64_t)std::max(1, h->cus) * 2);
    HIPCHK(hipEventRecord(st.k0, h->s_run));
    if (st.crc) hipLaunchKernelGGL(k_inflate_members<true>, dim3(blocks), dim3(WAVE), 0, h->s_run, a);
    else hipLaunchKernelGGL(k_inflate_members<false>, dim3(blocks), dim3(WAVE), 0, h->s_run, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st.k1, h->s_run));
    HIPCHK(hipEventRecord(st.done, h->s_run));
    HIPCHK(hipStreamWaitEvent(h->s_down, st.done, 0));
    if (out_bytes && !st.dev_out) {
        void *dst = st.direct ? static_cast<void *>(j->out + j->out_offset[first]) : st.h_out.p;
        HIPCHK(hipMemcpyAsync(dst, st.d_out.p, out_bytes, hipMemcpyDeviceToHost, h->s_down));
    }
    HIPCHK(hipMemcpyAsync(st.h_status.p, st.d_status.p, status_bytes, hipMemcpyDeviceToHost, h->s_down));
    HIPCHK(hipEventRecord(st.down, h->s_down));
    st.busy = true;
    return CHN_OK;
}

// wait for the group in set `st` and hand its output and statuses to the caller
static int inflate_collect(chn_inflate *h, InflateSet &st, const chn_inflate_job *j, const chn_inflate_crc *c) {
    if (!st.busy) return CHN_OK;
    st.busy = false;
    HIPCHK(hipEventSynchronize(st.down));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, st.k0, st.k1));
    h->kernel_ms += ms;
    std::memcpy(j->status + st.first, st.h_status.p, st.n * 4);
    if (st.crc && c->crc32)  // defined where the status is 0 or CHN_INFLATE_E_CRC; the kernel leaves the others unwritten
        std::memcpy(c->crc32 + st.first, st.h_status.as<uint32_t>() + st.n, st.n * 4);
    if (!st.direct) {
        const uint8_t *src = st.h_out.as<uint8_t>();
        for (uint64_t i = st.first; i < st.first + st.n; ++i) {
            if (j->out_length[i]) std::memcpy(j->out + j->out_offset[i], src, j->out_length[i]);
            src += j->out_length[i];
        }
    }
    return CHN_OK;
}

static int inflate_run(chn_inflate *h, const chn_inflate_job *j, const chn_inflate_crc *c, const char *who) {
    if (!h) return fail(CHN_E_INVALID, std::string(who) + ": null handle");
    int rc = inflate_check_crc(c, who);
    if (rc == CHN_OK) rc = inflate_check_job(j, who, false);
    if (rc || j->n_members == 0) return rc;
    if (c && !c->expected && !c->crc32) c = nullptr;  // decode only: the plain kernel
    HIPCHK(hipSetDevice(h->device));
    const bool dev_out = (j->flags & CHN_INFLATE_OUT_DEVICE) != 0;
    if (dev_out && j->out_bytes) {  // before anything is launched
        std::string why;
        if (!device_memory_of(j->out, j->out_bytes, h->device, why)) return fail(CHN_E_INVALID, std::string(who) + ": CHN_INFLATE_OUT_DEVICE: out " + why);
    }
    h->kernel_ms = 0;
    const bool out_pinned = !dev_out && j->out_bytes && page_locked_host(j->out, j->out_bytes);  // (no bytes: the staged path, which then moves none)
    return run_groups(*h, h->set, j->n_members,
        [&](InflateSet &st, uint64_t first, uint64_t &n) {
            uint64_t ob = 0, ib = 0;
            while (first + n < j->n_members && n < INF_GROUP_MEMBERS && (n == 0 || (ob + j->out_length[first + n] <= INF_GROUP_OUT && ib + j->in_length[first + n] <= INF_GROUP_IN))) {
                ob += j->out_length[first + n]; ib += j->in_length[first + n]; ++n;
            }
            return inflate_issue(h, st, j, c, first, n, out_pinned);
        },
        [&](InflateSet &st) { return inflate_collect(h, st, j, c); });
}
extern "C" int chn_inflate_run(chn_inflate *h, const chn_inflate_job *j) { return inflate_run(h, j, nullptr, "chn_inflate_run"); }
extern "C" int chn_inflate_run_crc(chn_inflate *h, const chn_inflate_job *j, const chn_inflate_crc *c) { return inflate_run(h, j, c, "chn_inflate_run_crc"); }

extern "C" int chn_inflate_kernel_ms(chn_inflate *h, double *ms) {
    if (!h || !ms) return fail(CHN_E_INVALID, "chn_inflate_kernel_ms: null argument");
    *ms = h->kernel_ms;
    return CHN_OK;
}
