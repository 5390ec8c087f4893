// abi_deflate.inc -- chn_deflate_create / chn_deflate_run / chn_deflate_run_host / chn_deflate_bound / chn_deflate_destroy: pieces deflated on the device
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.
//
// chn_deflate_run works through a job in groups of members (at most 1 024, about 64 MiB of input) on three streams of the handle's own,
// as chn_inflate_run does: while group g is compressed, the pieces of group g + 1 are packed into page-locked staging (each on a 16-byte
// boundary) and uploaded, and the members of group g - 1 are downloaded.  Two sets of grow-only buffers take turns.  The handle is a
// CodecPipe and the loop is run_groups (abi_device_call.inc); deflate_launch, deflate_ensure and deflate_collect also serve chn_extract.
// k_deflate_members leaves member i in its own stretch of DFL_SLOT bytes; k_deflate_scan turns the sizes into offsets and
// k_deflate_gather moves the members back to back, so one copy of exactly the group's bytes brings them to the host -- straight into
// `out` where that is page-locked, through staging otherwise.  The sizes travel first (a few bytes a member): the host needs their sum
// to size that copy.

static const uint32_t DFL_GROUP_MEMBERS = 1024;

struct DeflateSet {
    DevBuf d_in, d_desc, d_slots, d_res, d_packed, d_cursor;
    PinBuf h_in, h_desc, h_res, h_out;
    hipEvent_t up = nullptr, done = nullptr, sized = nullptr, down = nullptr, k0 = nullptr, k1 = nullptr;
    uint64_t first = 0, n = 0;  // the group in this set
    bool busy = false;
    int make_events(const char *who) { return events_create(who, {&up, &done, &sized, &down}, {&k0, &k1}); }
    void release() {
        for (DevBuf *b : {&d_in, &d_desc, &d_slots, &d_res, &d_packed, &d_cursor}) b->release();
        for (PinBuf *b : {&h_in, &h_desc, &h_res, &h_out}) b->release();
        events_destroy({&up, &done, &sized, &down, &k0, &k1});
    }
};
struct chn_deflate : CodecPipe {
    DeflateSet set[2];
    DevBuf d_tokens;       // the workgroups' token scratch (one kernel runs at a time)
    double kernel_ms = 0;  // device time of the last run's kernels
    uint32_t group_members = DFL_GROUP_MEMBERS;
};

static uint64_t deflate_bound(uint64_t n, uint64_t in_total, uint32_t flags) {
    return in_total + n * (5 + ((flags & CHN_DEFLATE_BGZF) ? DFL_BGZF_HEAD + DFL_BGZF_TAIL : 0));
}
extern "C" int chn_deflate_bound(uint64_t n_members, uint64_t in_bytes_total, uint32_t flags, uint64_t *bytes) {
    if (!bytes) return fail(CHN_E_INVALID, "chn_deflate_bound: null argument");
    if (flags & ~CHN_DEFLATE_BGZF) return fail(CHN_E_INVALID, "chn_deflate_bound: unknown flag");
    *bytes = deflate_bound(n_members, in_bytes_total, flags);
    return CHN_OK;
}

static int deflate_check_job(const chn_deflate_job *j, const char *who) {
    const std::string W(who);
    if (!j) return fail(CHN_E_INVALID, W + ": null job");
    if (j->struct_size != sizeof(chn_deflate_job)) return fail(CHN_E_INVALID, W + ": bad struct_size");
    if (j->flags & ~CHN_DEFLATE_BGZF) return fail(CHN_E_INVALID, W + ": unknown flag");
    if (!j->out_used) return fail(CHN_E_INVALID, W + ": out_used is NULL");
    const uint64_t n = j->n_members;
    if (n == 0) return CHN_OK;
    if (!j->in_offset || !j->in_length || !j->out_offset || !j->out_length) return fail(CHN_E_INVALID, W + ": a descriptor array is NULL");
    if ((!j->in && j->in_bytes) || !j->out) return fail(CHN_E_INVALID, W + ": in / out is NULL");
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const std::string M = W + ": member " + std::to_string(i);
        if (j->in_length[i] > CHN_DEFLATE_MAX_IN) return fail(CHN_E_INVALID, M + " has in_length above CHN_DEFLATE_MAX_IN");
        if (j->in_offset[i] > j->in_bytes || j->in_length[i] > j->in_bytes - j->in_offset[i]) return fail(CHN_E_INVALID, M + " reaches beyond in_bytes");
        total += j->in_length[i];
    }
    const uint64_t need = deflate_bound(n, total, j->flags);
    if (j->out_bytes < need)
        return fail(CHN_E_INVALID, W + ": member " + std::to_string(n - 1) + " may end at " + std::to_string(need) + " (chn_deflate_bound), out_bytes is " + std::to_string(j->out_bytes));
    return CHN_OK;
}

extern "C" int chn_deflate_run_host(const chn_deflate_job *j) {
    const char *who = "chn_deflate_run_host";
    const int rc = deflate_check_job(j, who);
    if (rc) return rc;
    *j->out_used = 0;
    if (j->n_members == 0) return CHN_OK;
    DflShared *sh = new (std::nothrow) DflShared;
    std::vector<uint32_t> tokens;
    std::vector<uint8_t> slot;
    try { tokens.resize(DFL_MAX_IN); slot.resize(DFL_SLOT); } catch (const std::bad_alloc &) { delete sh; sh = nullptr; }
    if (!sh) return fail(CHN_E_NOMEM, std::string(who) + ": no memory for the compressor's tables");
    uint64_t at = 0;
    for (uint64_t i = 0; i < j->n_members; ++i) {
        uint32_t crc = 0;
        const uint32_t size = dfl_member_host(*sh, tokens.data(), j->in + j->in_offset[i], j->in_length[i], j->flags, slot.data(), &crc);
        if (size > DFL_SLOT) { delete sh; return fail(CHN_E_INVALID, std::string(who) + ": member " + std::to_string(i) + " did not come out at its planned size"); }
        std::memcpy(j->out + at, slot.data(), size);
        j->out_offset[i] = at; j->out_length[i] = size;
        if (j->crc32) j->crc32[i] = crc;
        at += size;
    }
    *j->out_used = at;
    delete sh;
    return CHN_OK;
}

extern "C" int chn_deflate_create(int32_t device, chn_deflate **out) { return codec_create(device, out, "chn_deflate_create", chn_deflate_destroy); }

extern "C" int chn_deflate_destroy(chn_deflate *h) {
    if (!h) return CHN_OK;
    (void)hipSetDevice(h->device);
    h->drain();
    for (DeflateSet &st : h->set) st.release();
    h->d_tokens.release();
    h->destroy();
    delete h;
    return CHN_OK;
}

extern "C" int chn_deflate_group_members(chn_deflate *h, uint32_t members) {
    if (!h || members == 0 || members > DFL_GROUP_MEMBERS) return fail(CHN_E_INVALID, "chn_deflate_group_members: null handle, or members not in 1 .. 1024");
    h->group_members = members;
    return CHN_OK;
}

// the results of a group in one block: out_off[n + 1] (64-bit), out_len[n], crc[n]
static size_t deflate_res_bytes(uint64_t n) { return (size_t)(n + 1) * 8 + (size_t)n * 8; }

// compress the n pieces that lie in device memory at d_in + in_off[k] (in_off / in_len: d_desc, uploaded on s_up like the pieces and
// the zeroed cursor, in front of the event st.up that the caller has recorded) in set `st`, and start the download of their sizes.
// `d_in` is the set's own staging (chn_deflate_run) or a buffer of the caller's that is already in place (chn_extract).
static int deflate_launch(chn_deflate *h, DeflateSet &st, const uint8_t *d_in, uint64_t n, uint64_t in_total, uint32_t flags) {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(n, (uint64_t)std::max(1, h->cus) * 2);
    const size_t res_bytes = deflate_res_bytes(n);
    const size_t packed_bytes = (size_t)deflate_bound(n, in_total, flags) + 16;
    HIPCHK(hipStreamWaitEvent(h->s_run, st.up, 0));
    DeflateArgs a;
    a.in = d_in;
    a.in_off = st.d_desc.as<uint64_t>();
    a.in_len = reinterpret_cast<const uint32_t *>(a.in_off + n);
    a.slots = st.d_slots.as<uint8_t>();
    uint64_t *d_off = st.d_res.as<uint64_t>();
    a.out_len = reinterpret_cast<uint32_t *>(d_off + n + 1); a.crc = a.out_len + n;
    a.tokens = h->d_tokens.as<uint32_t>(); a.cursor = st.d_cursor.as<uint32_t>();
    a.n = (uint32_t)n; a.flags = flags;
    // a looping grid: two workgroups of one wavefront fit a CU's LDS; the cursor hands out members
    HIPCHK(hipEventRecord(st.k0, h->s_run));
    hipLaunchKernelGGL(k_deflate_members, dim3(blocks), dim3(WAVE), 0, h->s_run, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_deflate_scan, dim3(1), dim3(SCAN_THREADS), 0, h->s_run, a.out_len, d_off, (uint32_t)n);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_deflate_gather, dim3((uint32_t)n), dim3(256), 0, h->s_run, a.slots, a.out_len, d_off, st.d_packed.as<uint8_t>(), (uint64_t)packed_bytes);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st.k1, h->s_run));
    HIPCHK(hipEventRecord(st.done, h->s_run));
    HIPCHK(hipStreamWaitEvent(h->s_down, st.done, 0));
    HIPCHK(hipMemcpyAsync(st.h_res.p, st.d_res.p, res_bytes, hipMemcpyDeviceToHost, h->s_down));
    HIPCHK(hipEventRecord(st.sized, h->s_down));
    st.busy = true;
    return CHN_OK;
}

// the set's buffers for n pieces of in_total bytes altogether, all but the staging of the pieces themselves
static int deflate_ensure(chn_deflate *h, DeflateSet &st, uint64_t n, uint64_t in_total, uint32_t flags) {
    const size_t desc_bytes = (size_t)n * 12, res_bytes = deflate_res_bytes(n);
    const size_t packed_bytes = (size_t)deflate_bound(n, in_total, flags) + 16;
    int rc;
    if ((rc = st.h_desc.ensure(desc_bytes)) || (rc = st.d_desc.ensure(st.h_desc.cap)) ||
        (rc = st.d_slots.ensure((size_t)n * DFL_SLOT + 16)) || (rc = st.h_res.ensure(res_bytes)) || (rc = st.d_res.ensure(st.h_res.cap)) ||
        (rc = st.d_packed.ensure_grow(packed_bytes, packed_bytes / 4)) || (rc = st.d_cursor.ensure(16)) ||
        (rc = h->d_tokens.ensure((size_t)std::max(1, h->cus) * 2 * DFL_MAX_IN * 4)))  // (for the widest grid at once: a kernel may be running on it)
        return rc;
    return CHN_OK;
}

// pack, upload and compress members [first, first + n) in set `st`, and start the download of their sizes
static int deflate_issue(chn_deflate *h, DeflateSet &st, const chn_deflate_job *j, uint64_t first, uint64_t n) {
    uint64_t in_bytes = 0, in_total = 0;
    for (uint64_t i = first; i < first + n; ++i) { in_bytes += ((uint64_t)j->in_length[i] + 15) & ~15ull; in_total += j->in_length[i]; }
    st.first = first; st.n = n;
    const size_t desc_bytes = (size_t)n * 12;
    int rc;
    if ((rc = deflate_ensure(h, st, n, in_total, j->flags)) ||
        (rc = st.h_in.ensure_grow((size_t)in_bytes + 16, (size_t)(in_bytes / 4))) || (rc = st.d_in.ensure(st.h_in.cap)))
        return rc;
    uint64_t *in_off = st.h_desc.as<uint64_t>();
    uint32_t *in_len = reinterpret_cast<uint32_t *>(in_off + n);
    uint8_t *stage = st.h_in.as<uint8_t>();
    uint64_t ip = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t i = first + k;
        in_off[k] = ip; in_len[k] = j->in_length[i];
        if (j->in_length[i]) std::memcpy(stage + ip, j->in + j->in_offset[i], j->in_length[i]);
        ip += ((uint64_t)j->in_length[i] + 15) & ~15ull;
    }
    HIPCHK(hipMemcpyAsync(st.d_in.p, stage, ip + 16, hipMemcpyHostToDevice, h->s_up));
    HIPCHK(hipMemcpyAsync(st.d_desc.p, st.h_desc.p, desc_bytes, hipMemcpyHostToDevice, h->s_up));
    HIPCHK(hipMemsetAsync(st.d_cursor.p, 0, 4, h->s_up));
    HIPCHK(hipEventRecord(st.up, h->s_up));
    return deflate_launch(h, st, st.d_in.as<uint8_t>(), n, in_total, j->flags);
}

// Wait for the sizes of the group in set `st`, check them against DFL_SLOT and the bound of `in_total` bytes of input, and download the
// group's members to out + *used: straight there where `out` is page-locked, through staging otherwise.  `*kernel_ms` takes the group's
// device time; `who`, `member` and `of_what` word the two refusals.  The offsets, sizes and CRCs stay in st.h_res for the caller.
static int deflate_collect(chn_deflate *h, DeflateSet &st, uint64_t in_total, uint32_t flags, uint8_t *out, bool out_pinned, uint64_t *used, double *kernel_ms,
                           const char *who, const char *member, const char *of_what) {
    if (!st.busy) return CHN_OK;
    st.busy = false;
    HIPCHK(hipEventSynchronize(st.sized));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, st.k0, st.k1));
    *kernel_ms += ms;
    const uint64_t n = st.n, *off = st.h_res.as<uint64_t>();
    const uint32_t *len = reinterpret_cast<const uint32_t *>(off + n + 1);
    for (uint64_t k = 0; k < n; ++k)
        if (len[k] > DFL_SLOT) return fail(CHN_E_HIP, std::string(who) + ": " + member + " " + std::to_string(st.first + k) + of_what + " did not come out at its planned size");
    const uint64_t bytes = off[n];
    if (bytes > deflate_bound(n, in_total, flags)) return fail(CHN_E_HIP, std::string(who) + ": a group came out above its bound");
    if (bytes) {
        if (!out_pinned) { const int rc = st.h_out.ensure_grow((size_t)bytes, (size_t)(bytes / 4)); if (rc) return rc; }
        HIPCHK(hipMemcpyAsync(out_pinned ? static_cast<void *>(out + *used) : st.h_out.p, st.d_packed.p, bytes, hipMemcpyDeviceToHost, h->s_down));
        HIPCHK(hipEventRecord(st.down, h->s_down));
        HIPCHK(hipEventSynchronize(st.down));
        if (!out_pinned) std::memcpy(out + *used, st.h_out.p, bytes);
    }
    *used += bytes;
    return CHN_OK;
}

extern "C" int chn_deflate_run(chn_deflate *h, const chn_deflate_job *j) {
    if (!h) return fail(CHN_E_INVALID, "chn_deflate_run: null handle");
    h->kernel_ms = 0;
    int rc = deflate_check_job(j, "chn_deflate_run");
    if (rc) return rc;
    *j->out_used = 0;
    if (j->n_members == 0) return CHN_OK;
    HIPCHK(hipSetDevice(h->device));
    const bool out_pinned = page_locked_host(j->out, j->out_bytes);
    uint64_t used = 0;
    rc = run_groups(*h, h->set, j->n_members,
        [&](DeflateSet &st, uint64_t first, uint64_t &n) {
            n = std::min<uint64_t>(h->group_members, j->n_members - first);
            return deflate_issue(h, st, j, first, n);
        },
        [&](DeflateSet &st) {  // the group's members behind `used`; offsets, sizes and CRCs to the caller
            if (!st.busy) return CHN_OK;
            uint64_t in_total = 0;
            for (uint64_t k = 0; k < st.n; ++k) in_total += j->in_length[st.first + k];
            const uint64_t base = used;
            const int r = deflate_collect(h, st, in_total, j->flags, j->out, out_pinned, &used, &h->kernel_ms, "chn_deflate_run", "member", "");
            if (r) return r;
            const uint64_t *off = st.h_res.as<uint64_t>();
            const uint32_t *len = reinterpret_cast<const uint32_t *>(off + st.n + 1), *crc = len + st.n;
            for (uint64_t k = 0; k < st.n; ++k) {
                j->out_offset[st.first + k] = base + off[k];
                j->out_length[st.first + k] = len[k];
                if (j->crc32) j->crc32[st.first + k] = crc[k];
            }
            return CHN_OK;
        });
    if (rc) return rc;
    *j->out_used = used;
    return CHN_OK;
}

extern "C" int chn_deflate_kernel_ms(chn_deflate *h, double *ms) {
    if (!h || !ms) return fail(CHN_E_INVALID, "chn_deflate_kernel_ms: null argument");
    *ms = h->kernel_ms;
    return CHN_OK;
}
