// abi_device_call.inc -- what every device call of the C ABI is written against: grow-only buffers (DevBuf, PinBuf), the pointer-kind
// predicates, the member codecs' pipeline (CodecPipe, events_create, run_groups) and the profiling bracket of a call (CallTimer)
// Part of the single translation unit charon_hip.hip (in front of every abi_*.inc); tools/abi_helpers_check.hip includes it alone.

// ------------------------------------------------------------------------------------------------
// grow-only buffers
// ------------------------------------------------------------------------------------------------
// what ensure_grow asks for: `slack` more than needed where the buffer has to grow at all, so that sizes creeping up do not reallocate every call
static inline size_t grown_size(size_t cap, size_t need, size_t slack) { return need > cap ? need + slack : need; }

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return CHN_OK;
        if (p) { HIPCHK(hipFree(p)); p = nullptr; cap = 0; }
        HIPCHK(hipMalloc(&p, bytes));
        cap = bytes;
        return CHN_OK;
    }
    int ensure_grow(size_t need, size_t slack) { return ensure(grown_size(cap, need, slack)); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() { return reinterpret_cast<T *>(p); }
};

struct PinBuf {  // page-locked host memory (targets of in-stream result downloads)
    void *p = nullptr;
    size_t cap = 0;
    bool borrowed = false;  // a piece of the stream's one block (hipHostMalloc costs ~20 ms a call whatever the size)
    int ensure(size_t bytes) {
        if (bytes <= cap) return CHN_OK;
        if (p && !borrowed) HIPCHK(hipHostFree(p));
        p = nullptr; cap = 0; borrowed = false;
        HIPCHK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        cap = bytes;
        return CHN_OK;
    }
    int ensure_grow(size_t need, size_t slack) { return ensure(grown_size(cap, need, slack)); }
    void lend(void *piece, size_t bytes) { release(); p = piece; cap = bytes; borrowed = true; }
    void release() { if (p && !borrowed) (void)hipHostFree(p); p = nullptr; cap = 0; borrowed = false; }
    template <class T> T *as() { return reinterpret_cast<T *>(p); }
};

// ------------------------------------------------------------------------------------------------
// what kind of memory is a caller's pointer?
// ------------------------------------------------------------------------------------------------
// Is [p, p + bytes) page-locked host memory the runtime knows?  (bytes == 0 asks about p alone.)
static bool page_locked_host(const void *p, uint64_t bytes) {
    for (int k = 0; k < 2; ++k) {
        const void *q = k == 0 ? p : static_cast<const char *>(p) + (bytes ? bytes - 1 : 0);
        hipPointerAttribute_t a;
        std::memset(&a, 0, sizeof a);
        if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (a.type != hipMemoryTypeHost) return false;
    }
    return true;
}

// Is [p, p + bytes) device memory of `device`?  `why` says what it is instead.  (The runtime answers a pageable pointer with an
// error, which is cleared: it is "not device memory".)
static bool device_memory_of(const void *p, uint64_t bytes, int device, std::string &why) {
    for (int k = 0; k < 2; ++k) {
        const void *q = k == 0 ? p : static_cast<const char *>(p) + (bytes ? bytes - 1 : 0);
        hipPointerAttribute_t a;
        std::memset(&a, 0, sizeof a);
        if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); why = "is not device memory (pageable host memory, or a pointer the runtime does not know)"; return false; }
        if (a.type == hipMemoryTypeHost) { why = "is page-locked host memory, not device memory"; return false; }
        if (a.type != hipMemoryTypeDevice) { why = "is not device memory"; return false; }
        if (a.device != device) { why = "is memory of device " + std::to_string(a.device) + ", not of device " + std::to_string(device); return false; }
    }
    return true;
}

// the device text contract of chn_text_split and CHN_TEXT_ON_DEVICE
static int device_text_check(const uint8_t *text, uint64_t text_bytes, int device, const std::string &who) {
    if (!text_bytes) return CHN_OK;  // nothing is read
    if (reinterpret_cast<uintptr_t>(text) & 15) return fail(CHN_E_INVALID, who + ": device text must be 16-byte aligned");
    std::string why;
    if (!device_memory_of(text, (text_bytes + 15) & ~(uint64_t)15, device, why)) return fail(CHN_E_INVALID, who + ": text " + why);
    return CHN_OK;
}

// ------------------------------------------------------------------------------------------------
// the member codecs' pipeline (chn_inflate, chn_deflate and through it chn_extract)
// ------------------------------------------------------------------------------------------------
// The events of one buffer set: `ordering` events only order the streams (no timing), `timed` ones bracket the kernels.
static int events_create(const char *who, std::initializer_list<hipEvent_t *> ordering, std::initializer_list<hipEvent_t *> timed) {
    hipError_t e = hipSuccess;
    for (hipEvent_t *ev : ordering) if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    for (hipEvent_t *ev : timed) if (e == hipSuccess) e = hipEventCreate(ev);
    return e == hipSuccess ? CHN_OK : fail(CHN_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
}
static void events_destroy(std::initializer_list<hipEvent_t *> events) {
    for (hipEvent_t *ev : events) { if (*ev) (void)hipEventDestroy(*ev); *ev = nullptr; }
}

// A device and three streams of the handle's own: uploads, kernels, downloads.  A handle embeds one and keeps two sets of buffers and
// events that take turns (run_groups).
struct CodecPipe {
    int device = 0;
    hipStream_t s_up = nullptr, s_run = nullptr, s_down = nullptr;
    int cus = 0;
    // checks and selects `device`; leaves no stream behind where it fails
    int create(int32_t device, const char *who) {
        int count = 0;
        HIPCHK(hipGetDeviceCount(&count));
        if (device < 0 || device >= count) return fail(CHN_E_INVALID, std::string(who) + ": device " + std::to_string(device) + " is not below the device count " + std::to_string(count));
        HIPCHK(hipSetDevice(device));
        this->device = device;
        hipDeviceProp_t prop;
        hipError_t e = hipGetDeviceProperties(&prop, device);
        for (hipStream_t *q : {&s_up, &s_run, &s_down}) if (e == hipSuccess) e = hipStreamCreateWithFlags(q, hipStreamNonBlocking);
        if (e != hipSuccess) { destroy(); return fail(CHN_E_HIP, std::string(who) + ": " + hipGetErrorString(e)); }
        cus = prop.multiProcessorCount;
        return CHN_OK;
    }
    // nothing of the handle's work stays queued: nothing is on its way into the caller's memory any more
    void drain() { for (hipStream_t q : {s_up, s_run, s_down}) if (q) (void)hipStreamSynchronize(q); }
    void destroy() {
        drain();
        for (hipStream_t *q : {&s_up, &s_run, &s_down}) { if (*q) (void)hipStreamDestroy(*q); *q = nullptr; }
    }
};

// chn_X_create for a handle H that embeds a CodecPipe and has set[2], each with make_events(who)
template <class H> static int codec_create(int32_t device, H **out, const char *who, int (*destroy)(H *)) {
    if (!out) return fail(CHN_E_INVALID, std::string(who) + ": null argument");
    *out = nullptr;
    H *h = new (std::nothrow) H;
    if (!h) return fail(CHN_E_NOMEM, std::string(who) + ": no memory");
    int rc = h->create(device, who);
    if (rc) { delete h; return rc; }
    for (auto &st : h->set) if (rc == CHN_OK) rc = st.make_events(who);
    if (rc) { (void)destroy(h); return rc; }  // (destroy leaves the message alone)
    *out = h;
    return CHN_OK;
}

// The run loop of a job that is worked through in groups of members on the two sets of a pipe: issue group g into set g & 1, then
// collect group g - 1 from the other set (so a set is free when its turn comes again: its last group was collected when the one after
// it was issued), and collect the last group at the end.
//   issue(set, first, n)   queues members [first, first + n) -- it chooses n >= 1 -- and sets set.busy
//   collect(set)           waits for the set's group and hands it to the caller; a set that is not busy is none of its business
// Whatever fails, the pipe is drained before the error is returned and neither set is busy.
template <class Pipe, class Set, class Issue, class Collect>
static int run_groups(Pipe &pipe, Set (&set)[2], uint64_t members, Issue issue, Collect collect) {
    int rc = CHN_OK;
    uint64_t first = 0, g = 0;
    for (; rc == CHN_OK && first < members; ++g) {
        uint64_t n = 0;
        rc = issue(set[g & 1], first, n);
        if (rc == CHN_OK && g > 0) rc = collect(set[(g - 1) & 1]);
        first += n;
    }
    if (rc == CHN_OK && g > 0) rc = collect(set[(g - 1) & 1]);
    if (rc) { pipe.drain(); set[0].busy = set[1].busy = false; }
    return rc;
}

// ------------------------------------------------------------------------------------------------
// the profiling bracket of a call on a chn_stream (chn_stream_profile)
// ------------------------------------------------------------------------------------------------
// Two events around a call's kernels, made by the first profiled call; `prof` is the stream's CHN_STREAM_PROFILE.  Without it no event
// is created, nothing is recorded and nothing counted.
struct CallTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms = 0;
    uint64_t calls = 0;
    hipError_t begin(bool prof, hipStream_t q) {
        if (!prof) return hipSuccess;
        for (hipEvent_t &e : ev)
            if (!e) { const hipError_t c = hipEventCreate(&e); if (c != hipSuccess) return c; }
        return hipEventRecord(ev[0], q);
    }
    hipError_t end(bool prof, hipStream_t q) { return prof ? hipEventRecord(ev[1], q) : hipSuccess; }
    // behind the wait for `q`: the call counts, with its time
    hipError_t collect(bool prof) {
        if (!prof) return hipSuccess;
        float t = 0;
        const hipError_t e = hipEventElapsedTime(&t, ev[0], ev[1]);
        if (e == hipSuccess) { ms += t; calls += 1; }
        return e;
    }
    void count_only() { calls += 1; }  // a profiled call that had nothing to run
    void report(double *total_ms, uint64_t *launches, int reset) {
        if (total_ms) *total_ms = ms;
        if (launches) *launches = calls;
        if (reset) { ms = 0; calls = 0; }
    }
    void release() { for (hipEvent_t &e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; } }
};
