// text_gather.inc -- byte ranges of a text that lies in device memory gathered back to back (chn_text_fetch), and the same copy rule
// on the CPU (chn_text_fetch_host)
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.
//
// THE COPY RULE: range i is text[offset[i] .. + length[i]); it goes to out + sum(length[0 .. i)).  Ranges may overlap, repeat and be
// empty; every one lies inside [0, text_bytes).  txg_check_job makes the checks both calls make; txg_host_job is the body of
// chn_text_fetch_host.
//
// The device does what k_inflate_members' write-out does, the other way round.  One wavefront takes one range at a time.  Source and
// destination are mutually misaligned in general: every whole 16-byte piece of the DESTINATION is one aligned vector store of one lane,
// built from the one or two aligned 16-byte pieces of the source that hold its bytes (the byte shift between them is the same for every
// piece of a range, so the funnel is wave-uniform); the ragged ends in front of the first and behind the last whole piece go byte by
// byte.  Only aligned pieces that hold a wanted byte are loaded: the second piece of a pair is not touched when the shift is zero, and
// with a shift its first byte is wanted.  So the kernel needs what the device text contract grants (16-byte alignment, readable up to
// text_bytes rounded up to 16) and nothing more.  Every store is a plain store; no LDS.

#ifndef __HIPCC__  // a CPU build of the checks and the host copy alone (tools/fuzz/text_fetch_fuzz.cpp)
#ifndef __host__
#define __host__
#define __device__
#endif
#endif

// The checks both calls make on a job before anything else; `why` names the first that fails and `total` is the sum of the lengths.
// 0 or a CHN_E_* code.
static int txg_check_job(const chn_text_fetch_job *j, const char *who, std::string &why, uint64_t &total) {
    const std::string W(who);
    total = 0;
    if (!j) { why = W + ": null job"; return CHN_E_INVALID; }
    if (j->struct_size != sizeof(chn_text_fetch_job)) { why = W + ": bad struct_size"; return CHN_E_INVALID; }
    if (j->flags) { why = W + ": unknown flag"; return CHN_E_INVALID; }
    if (j->n_ranges && (!j->offset || !j->length)) { why = W + ": a range array is NULL"; return CHN_E_INVALID; }
    if (!j->text && j->text_bytes) { why = W + ": text is NULL"; return CHN_E_INVALID; }
    for (uint64_t i = 0; i < j->n_ranges; ++i) {
        if (j->offset[i] > j->text_bytes || j->length[i] > j->text_bytes - j->offset[i]) {
            why = W + ": range " + std::to_string(i) + " (offset " + std::to_string(j->offset[i]) + ", length " + std::to_string(j->length[i]) + ") ends behind text_bytes " +
                  std::to_string(j->text_bytes);
            return CHN_E_INVALID;
        }
        total += j->length[i];  // (n < 2^64 / 2^32 ranges of a real array: no wrap)
    }
    if (total > j->out_capacity) {
        why = W + ": the ranges need " + std::to_string(total) + " bytes, out_capacity is " + std::to_string(j->out_capacity);
        return CHN_E_CAPACITY;
    }
    if (total && !j->out) { why = W + ": out is NULL"; return CHN_E_INVALID; }
    return CHN_OK;
}

// chn_text_fetch_host: one range after another
static int txg_host_job(chn_text_fetch_job *j, std::string &why) {
    uint64_t total = 0;
    const int rc = txg_check_job(j, "chn_text_fetch_host", why, total);
    if (rc) return rc;
    uint64_t at = 0;
    for (uint64_t i = 0; i < j->n_ranges; ++i) {
        if (j->length[i]) std::memcpy(j->out + at, j->text + j->offset[i], j->length[i]);
        at += j->length[i];
    }
    j->out_bytes = total;
    return CHN_OK;
}

#ifdef __HIPCC__
// range i: text[src_off[i] .. + len[i]) to out + dst_off[i].  `out` is 16-byte aligned; dst_off is the exclusive scan of len (the host's).
// A looping grid of one-wavefront workgroups.
__global__ void __launch_bounds__(64) k_text_gather(const uint8_t *__restrict__ text, const uint64_t *__restrict__ src_off, const uint64_t *__restrict__ dst_off,
                                                    const uint32_t *__restrict__ len, uint64_t n, uint8_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x;
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {  // (wave-uniform)
        const uint64_t so = src_off[i], dpos = dst_off[i];
        const uint32_t l = len[i];
        if (l == 0) continue;
        const uint8_t *src = text + so;
        uint8_t *dst = out + dpos;
        const uint32_t to16 = (uint32_t)(16 - (dpos & 15)) & 15u;
        const uint32_t head = to16 < l ? to16 : l;        // bytes in front of the first whole piece of the destination
        const uint32_t pieces = (l - head) / 16;          // whole pieces
        const uint32_t tail = (l - head) & 15u;           // bytes behind the last
        if (lane < head) dst[lane] = src[lane];
        if (lane < tail) dst[head + pieces * 16 + lane] = src[head + pieces * 16 + lane];
        // piece p holds source bytes [s, s + 16), s = so + head + 16 p: with sh = s & 15 the last 16 - sh bytes of the aligned piece at
        // s - sh and, if sh != 0, the first sh bytes of the next (whose first byte is wanted, so it lies inside the text)
        const uint32_t sh = (uint32_t)((so + head) & 15), q = sh >> 2, r8 = (sh & 3u) * 8;
        const uint8_t *abase = src + head - sh;           // 16-byte aligned
        u32x4_t *dbase = reinterpret_cast<u32x4_t *>(dst + head);
        for (uint32_t p = lane; p < pieces; p += WAVE) {
            const u32x4_t a = *reinterpret_cast<const u32x4_t *>(abase + (uint64_t)p * 16);
            u32x4_t o = a;
            if (sh) {
                const u32x4_t b = *reinterpret_cast<const u32x4_t *>(abase + (uint64_t)p * 16 + 16);
                // the eight words moved down by q words (named values, constant indices: no array a lane would index at run time) ...
                uint32_t x0 = a.x, x1 = a.y, x2 = a.z, x3 = a.w, x4 = b.x, x5 = b.y, x6 = b.z, x7 = b.w;
                if (q & 2u) { x0 = x2; x1 = x3; x2 = x4; x3 = x5; x4 = x6; x5 = x7; }
                if (q & 1u) { x0 = x1; x1 = x2; x2 = x3; x3 = x4; x4 = x5; }
                // ... and by the 0 .. 3 bytes left (a funnel shift by 0 gives the low word)
                o.x = __funnelshift_r(x0, x1, r8); o.y = __funnelshift_r(x1, x2, r8);
                o.z = __funnelshift_r(x2, x3, r8); o.w = __funnelshift_r(x3, x4, r8);
            }
            dbase[p] = o;
        }
    }
}
#endif
