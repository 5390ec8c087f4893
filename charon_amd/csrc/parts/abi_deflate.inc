// abi_deflate.inc -- chn_deflate_create / chn_deflate_run / chn_deflate_run_host / chn_deflate_bound / chn_deflate_destroy: pieces deflated on the device
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.
//
// chn_deflate_run works through a job in groups of members (at most 1 024, about 64 MiB of input) on three streams of the handle's own,
// as chn_inflate_run does: while group g is compressed, the pieces of group g + 1 are packed into page-locked staging (each on a 16-byte
// boundary) and uploaded, and the members of group g - 1 are downloaded.  Two sets of grow-only buffers take turns.
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
};
struct chn_deflate {
    int device = 0;
    hipStream_t s_up = nullptr, s_run = nullptr, s_down = nullptr;
    DeflateSet set[2];
    DevBuf d_tokens;       // the workgroups' token scratch (one kernel runs at a time)
    double kernel_ms = 0;  // device time of the last run's kernels
    int cus = 0;
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

extern "C" int chn_deflate_create(int32_t device, chn_deflate **out) {
    if (!out) return fail(CHN_E_INVALID, "chn_deflate_create: null argument");
    *out = nullptr;
    int count = 0;
    HIPCHK(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(CHN_E_INVALID, "chn_deflate_create: device " + std::to_string(device) + " is not below the device count " + std::to_string(count));
    HIPCHK(hipSetDevice(device));
    chn_deflate *h = new (std::nothrow) chn_deflate;
    if (!h) return fail(CHN_E_NOMEM, "chn_deflate_create: no memory");
    h->device = device;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->s_up, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->s_run, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->s_down, hipStreamNonBlocking);
    for (int s = 0; s < 2 && e == hipSuccess; ++s) {
        DeflateSet &st = h->set[s];
        if (e == hipSuccess) e = hipEventCreateWithFlags(&st.up, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&st.done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&st.sized, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&st.down, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreate(&st.k0);
        if (e == hipSuccess) e = hipEventCreate(&st.k1);
    }
    if (e != hipSuccess) {
        const std::string msg = std::string("chn_deflate_create: ") + hipGetErrorString(e);
        chn_deflate_destroy(h);
        return fail(CHN_E_HIP, msg);
    }
    h->cus = prop.multiProcessorCount;
    *out = h;
    return CHN_OK;
}

extern "C" int chn_deflate_destroy(chn_deflate *h) {
    if (!h) return CHN_OK;
    (void)hipSetDevice(h->device);
    if (h->s_up) (void)hipStreamSynchronize(h->s_up);
    if (h->s_run) (void)hipStreamSynchronize(h->s_run);
    if (h->s_down) (void)hipStreamSynchronize(h->s_down);
    for (DeflateSet &st : h->set) {
        st.d_in.release(); st.d_desc.release(); st.d_slots.release(); st.d_res.release(); st.d_packed.release(); st.d_cursor.release();
        st.h_in.release(); st.h_desc.release(); st.h_res.release(); st.h_out.release();
        for (hipEvent_t ev : {st.up, st.done, st.sized, st.down, st.k0, st.k1}) if (ev) (void)hipEventDestroy(ev);
    }
    h->d_tokens.release();
    if (h->s_up) (void)hipStreamDestroy(h->s_up);
    if (h->s_run) (void)hipStreamDestroy(h->s_run);
    if (h->s_down) (void)hipStreamDestroy(h->s_down);
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
    hipLaunchKernelGGL(k_deflate_scan, dim3(1), dim3(WAVE), 0, h->s_run, a.out_len, d_off, (uint32_t)n);
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
        (rc = st.d_packed.ensure(packed_bytes + (st.d_packed.cap < packed_bytes ? packed_bytes / 4 : 0))) || (rc = st.d_cursor.ensure(16)) ||
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
        (rc = st.h_in.ensure((size_t)in_bytes + 16 + (st.h_in.cap < in_bytes + 16 ? in_bytes / 4 : 0))) || (rc = st.d_in.ensure(st.h_in.cap)))
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

// wait for the group in set `st`, download its members behind `*used` and hand offsets, sizes and CRCs to the caller
static int deflate_collect(chn_deflate *h, DeflateSet &st, const chn_deflate_job *j, bool out_pinned, uint64_t *used) {
    if (!st.busy) return CHN_OK;
    st.busy = false;
    HIPCHK(hipEventSynchronize(st.sized));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, st.k0, st.k1));
    h->kernel_ms += ms;
    const uint64_t n = st.n, *off = st.h_res.as<uint64_t>();
    const uint32_t *len = reinterpret_cast<const uint32_t *>(off + n + 1), *crc = len + n;
    uint64_t in_total = 0;
    for (uint64_t k = 0; k < n; ++k) {
        if (len[k] > DFL_SLOT) return fail(CHN_E_HIP, "chn_deflate_run: member " + std::to_string(st.first + k) + " did not come out at its planned size");
        in_total += j->in_length[st.first + k];
    }
    const uint64_t bytes = off[n];
    if (bytes > deflate_bound(n, in_total, j->flags)) return fail(CHN_E_HIP, "chn_deflate_run: a group came out above its bound");
    if (bytes) {
        if (!out_pinned) { const int rc = st.h_out.ensure((size_t)bytes + (st.h_out.cap < bytes ? bytes / 4 : 0)); if (rc) return rc; }
        HIPCHK(hipMemcpyAsync(out_pinned ? static_cast<void *>(j->out + *used) : st.h_out.p, st.d_packed.p, bytes, hipMemcpyDeviceToHost, h->s_down));
        HIPCHK(hipEventRecord(st.down, h->s_down));
        HIPCHK(hipEventSynchronize(st.down));
        if (!out_pinned) std::memcpy(j->out + *used, st.h_out.p, bytes);
    }
    for (uint64_t k = 0; k < n; ++k) {
        j->out_offset[st.first + k] = *used + off[k];
        j->out_length[st.first + k] = len[k];
        if (j->crc32) j->crc32[st.first + k] = crc[k];
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
    const bool out_pinned = inflate_is_pinned(j->out, j->out_bytes);
    uint64_t first = 0, g = 0, used = 0;
    while (first < j->n_members) {
        const uint64_t n = std::min<uint64_t>(h->group_members, j->n_members - first);
        // the set's staging and device buffers are free: its last group was collected when the one after it was issued
        rc = deflate_issue(h, h->set[g & 1], j, first, n);
        if (rc == CHN_OK && g > 0) rc = deflate_collect(h, h->set[(g - 1) & 1], j, out_pinned, &used);
        if (rc) break;
        first += n; ++g;
    }
    if (rc == CHN_OK) rc = deflate_collect(h, h->set[(g - 1) & 1], j, out_pinned, &used);
    if (rc) {  // nothing of this call may still be on its way into the caller's memory
        (void)hipStreamSynchronize(h->s_up); (void)hipStreamSynchronize(h->s_run); (void)hipStreamSynchronize(h->s_down);
        h->set[0].busy = h->set[1].busy = false;
        return rc;
    }
    *j->out_used = used;
    return CHN_OK;
}

extern "C" int chn_deflate_kernel_ms(chn_deflate *h, double *ms) {
    if (!h || !ms) return fail(CHN_E_INVALID, "chn_deflate_kernel_ms: null argument");
    *ms = h->kernel_ms;
    return CHN_OK;
}
