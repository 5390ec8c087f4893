// extract_records.inc -- the FASTQ records of the --extract files formed out of a text that lies in device memory
// (chn_extract_append_records), the same rule on the CPU (chn_extract_records_host), and the piece-and-tail arithmetic of a chn_extract
// Part of the single translation unit charon_hip.hip (included in order, behind text_gather.inc); not a stand-alone source.
//
// THE RECORD RULE is Result::write_record's (host/result.inc) for FASTQ:  '@' id '\n' SEQ '\n' '+' '\n' qual '\n'
//   id, qual   the bytes of text[id_offset .. + id_length) and text[qual_offset .. + qual_length) as they stand
//   SEQ        the bytes of text[seq_offset .. + seq_length), each through the letter map "ACGTN"[g_codes.t[c] & 7] of the front end
//              (host/fastx_reader.inc, CodeTable): A C G T and their lower case stay / become upper case, U and u become T, the IUPAC
//              letters N R Y S W K M B D H V and their lower case become N.  Every other byte is no letter and cannot get here, because
//              chn_text_submit refuses the batch of such a read; for a table without a hole it maps to N as well ("ACGTN"[255 & 7]
//              would be past the string's end: the front end never evaluates it).
// Record i is id_length + seq_length + qual_length + 6 bytes long and goes to the sum of the lengths of the records before it.
//
// The rule is written once, as __host__ __device__ code over a policy (xr_record): on the device the policy is a wavefront whose lanes
// share the bytes of a record, on the host it has one lane.  A record is three SEGMENTS (id, sequence, quality) with six FIXED bytes
// around them.  Every segment is copied the way k_text_gather copies a range: every whole 16-byte piece of the DESTINATION that lies
// inside the segment is one aligned vector store of one lane, built from the one or two aligned 16-byte pieces of the source that hold
// its bytes (the sequence's then go through the letter map, four letters a dword); the bytes of a segment in front of its first and
// behind its last whole piece go byte by byte, and so do the six fixed bytes.  So a destination piece that holds a SEAM -- the end of
// one segment, fixed bytes, the start of the next, or the end of one record and the start of the next -- is written byte by byte by
// up to 15 + 15 + 5 lanes, every byte by exactly one lane, and every other piece is one store.  Only aligned source pieces that hold
// a wanted byte are loaded (the device text contract: readable to text_bytes rounded up to 16).  Plain stores only; no LDS: the letter
// map is arithmetic on the four bytes of a dword at once (xr_map_word), about 40 integer operations a dword.

#ifndef __HIPCC__  // a CPU build of the checks, the rule and the bookkeeping alone (tools/fuzz/extract_records_fuzz.cpp)
#ifndef __host__
#define __host__
#define __device__
#endif
#endif

// 0x80 in every byte of the result whose byte of x is zero, 0 elsewhere (exact: the sum cannot carry from byte to byte)
__host__ __device__ static inline uint32_t xr_zero_bytes(uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); }
// 0x80 flags widened to 0xFF
__host__ __device__ static inline uint32_t xr_byte_mask(uint32_t f) { return (f - (f >> 7)) | f; }
// THE LETTER MAP on four bytes at once.  u clears the case bit; a byte of u that is A, C, G or T stays, U becomes T, all else N.
__host__ __device__ static inline uint32_t xr_map_word(uint32_t w) {
    const uint32_t u = w & 0xDFDFDFDFu;
    const uint32_t keep = xr_byte_mask(xr_zero_bytes(u ^ 0x41414141u) | xr_zero_bytes(u ^ 0x43434343u) | xr_zero_bytes(u ^ 0x47474747u) | xr_zero_bytes(u ^ 0x54545454u));
    const uint32_t isu = xr_byte_mask(xr_zero_bytes(u ^ 0x55555555u));
    return (u & keep) | (0x54545454u & isu) | (0x4E4E4E4Eu & ~(keep | isu));
}
__host__ __device__ static inline uint8_t xr_map_byte(uint8_t c) { return (uint8_t)xr_map_word(c); }

// one lane, host text and host destination of any alignment: a piece is its 16 bytes and nothing else
struct XrHostPolicy {
    static const uint32_t LANES = 1;
    __host__ __device__ uint32_t lane() const { return 0; }
    __host__ __device__ void load16(const uint8_t *text, uint64_t s, uint32_t w[4]) const {
        for (uint32_t k = 0; k < 4; ++k) w[k] = (uint32_t)text[s + 4 * k] | (uint32_t)text[s + 4 * k + 1] << 8 | (uint32_t)text[s + 4 * k + 2] << 16 | (uint32_t)text[s + 4 * k + 3] << 24;
    }
    __host__ __device__ void store16(uint8_t *dst, const uint32_t w[4]) const {
        for (uint32_t j = 0; j < 16; ++j) dst[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
};

// text[so .. + l) to out + dpos, through the letter map if MAP.  Which bytes are "a whole piece" depends on dpos & 15 alone, so `out`
// itself is 16-byte aligned on the device and of any alignment on the host.
template <bool MAP, class P>
__host__ __device__ static inline void xr_segment(const P &pol, const uint8_t *text, uint64_t so, uint32_t l, uint8_t *out, uint64_t dpos) {
    if (l == 0) return;
    const uint8_t *src = text + so;
    uint8_t *dst = out + dpos;
    const uint32_t to16 = (uint32_t)(16 - (dpos & 15)) & 15u;
    const uint32_t head = to16 < l ? to16 : l;        // bytes in front of the first whole piece of the destination
    const uint32_t pieces = (l - head) / 16;          // whole pieces
    const uint32_t tail = (l - head) & 15u;           // bytes behind the last
    const uint32_t rest = head + pieces * 16;
    for (uint32_t k = pol.lane(); k < head; k += P::LANES) dst[k] = MAP ? xr_map_byte(src[k]) : src[k];
    for (uint32_t k = pol.lane(); k < tail; k += P::LANES) dst[rest + k] = MAP ? xr_map_byte(src[rest + k]) : src[rest + k];
    for (uint32_t p = pol.lane(); p < pieces; p += P::LANES) {
        uint32_t w[4];
        pol.load16(text, so + head + (uint64_t)p * 16, w);
        if (MAP) { w[0] = xr_map_word(w[0]); w[1] = xr_map_word(w[1]); w[2] = xr_map_word(w[2]); w[3] = xr_map_word(w[3]); }
        pol.store16(dst + head + (uint64_t)p * 16, w);
    }
}

// the rule (above) for one record, to out + dpos
template <class P>
__host__ __device__ static inline void xr_record(const P &pol, const uint8_t *text, uint64_t id_off, uint32_t id_len, uint64_t seq_off, uint32_t seq_len,
                                                 uint64_t qual_off, uint32_t qual_len, uint8_t *out, uint64_t dpos) {
    const uint64_t mid = (uint64_t)id_len + seq_len;
    // the six fixed bytes: '@' at 0, '\n' behind the id, '\n' '+' '\n' behind the sequence, '\n' behind the quality string
    for (uint32_t k = pol.lane(); k < 6; k += P::LANES) {
        const uint64_t at = k == 0 ? 0 : k == 1 ? (uint64_t)id_len + 1 : k < 5 ? mid + k : mid + qual_len + 5;
        out[dpos + at] = k == 0 ? (uint8_t)'@' : k == 3 ? (uint8_t)'+' : (uint8_t)'\n';
    }
    xr_segment<false>(pol, text, id_off, id_len, out, dpos + 1);
    xr_segment<true>(pol, text, seq_off, seq_len, out, dpos + 2 + id_len);
    xr_segment<false>(pol, text, qual_off, qual_len, out, dpos + 5 + mid);
}

__host__ __device__ static inline uint64_t xr_record_bytes(uint32_t id_len, uint32_t seq_len, uint32_t qual_len) { return (uint64_t)id_len + seq_len + qual_len + 6; }

// The checks that need no device, for both calls; `why` names the first that fails, `total` is the sum of the records' lengths.
static int xr_check_job(const chn_extract_job *j, const char *who, std::string &why, uint64_t &total) {
    const std::string W(who);
    total = 0;
    if (!j) { why = W + ": null job"; return CHN_E_INVALID; }
    if (j->struct_size != sizeof(chn_extract_job)) { why = W + ": bad struct_size"; return CHN_E_INVALID; }
    if (j->flags) { why = W + ": unknown flag"; return CHN_E_INVALID; }
    if (j->n_records && (!j->id_offset || !j->id_length || !j->seq_offset || !j->seq_length || !j->qual_offset || !j->qual_length)) {
        why = W + ": a descriptor array is NULL";
        return CHN_E_INVALID;
    }
    if (!j->text && j->text_bytes) { why = W + ": text is NULL"; return CHN_E_INVALID; }
    for (uint64_t i = 0; i < j->n_records; ++i) {
        for (int m = 0; m < 3; ++m) {
            const uint64_t o = m == 0 ? j->id_offset[i] : m == 1 ? j->seq_offset[i] : j->qual_offset[i];
            const uint32_t l = m == 0 ? j->id_length[i] : m == 1 ? j->seq_length[i] : j->qual_length[i];
            if (o > j->text_bytes || l > j->text_bytes - o) {
                why = W + ": record " + std::to_string(i) + ": its " + (m == 0 ? "id" : m == 1 ? "sequence" : "quality string") + " (offset " + std::to_string(o) + ", length " +
                      std::to_string(l) + ") ends behind text_bytes " + std::to_string(j->text_bytes);
                return CHN_E_INVALID;
            }
        }
        total += xr_record_bytes(j->id_length[i], j->seq_length[i], j->qual_length[i]);  // (n < 2^64 / 2^34 records of a real array: no wrap)
    }
    return CHN_OK;
}

// chn_extract_records_host: one record after another
static int xr_host_job(const chn_extract_job *j, uint8_t *text_out, uint64_t capacity, uint64_t *bytes, std::string &why) {
    const char *who = "chn_extract_records_host";
    uint64_t total = 0;
    const int rc = xr_check_job(j, who, why, total);
    if (rc) return rc;
    if (!bytes) { why = std::string(who) + ": bytes is NULL"; return CHN_E_INVALID; }
    if (total > capacity) { why = std::string(who) + ": the records need " + std::to_string(total) + " bytes, capacity is " + std::to_string(capacity); return CHN_E_CAPACITY; }
    if (total && !text_out) { why = std::string(who) + ": text_out is NULL"; return CHN_E_INVALID; }
    const XrHostPolicy pol;
    uint64_t at = 0;
    for (uint64_t i = 0; i < j->n_records; ++i) {
        xr_record(pol, j->text, j->id_offset[i], j->id_length[i], j->seq_offset[i], j->seq_length[i], j->qual_offset[i], j->qual_length[i], text_out, at);
        at += xr_record_bytes(j->id_length[i], j->seq_length[i], j->qual_length[i]);
    }
    *bytes = total;
    return CHN_OK;
}

// THE PIECE-AND-TAIL ARITHMETIC of a chn_extract.  A file's text is cut at multiples of XR_PIECE from its start, whatever the appends
// were.  The handle's buffer holds the `pending` bytes behind the last cut (fewer than XR_PIECE) at its front; an append of `bytes`
// goes behind them, the `pieces` whole pieces that are there then are compressed in place -- piece k at k * XR_PIECE, a multiple of
// 16 -- and the `tail` bytes behind them move to the front.  With pieces >= 1 the tail's old place [pieces * XR_PIECE, + tail) and its
// new one [0, tail) cannot overlap, because tail < XR_PIECE.
static const uint64_t XR_PIECE = CHN_DEFLATE_MAX_IN;
struct XrPlan { uint64_t pieces, tail; };
__host__ __device__ static inline XrPlan xr_plan_append(uint64_t pending, uint64_t bytes) {
    const uint64_t have = pending + bytes;
    return XrPlan{have / XR_PIECE, have % XR_PIECE};
}
// bytes a piece may take as a BGZF member: the piece, a stored block's 5 bytes, header and trailer
static const uint64_t XR_MEMBER_EXTRA = 5 + 18 + 8;
static inline uint64_t xr_bound(uint64_t pending, uint64_t appended) {
    if (appended == 0) return pending ? pending + XR_MEMBER_EXTRA : 0;  // what chn_extract_finish needs
    const XrPlan p = xr_plan_append(pending, appended);
    return p.pieces * (XR_PIECE + XR_MEMBER_EXTRA);
}

#ifdef __HIPCC__
// a wavefront; device text under the device text contract and a 16-byte aligned destination
struct XrWavePolicy {
    static const uint32_t LANES = WAVE;
    __device__ __forceinline__ uint32_t lane() const { return threadIdx.x; }
    // the 16 bytes at text + s, all wanted: with sh = s & 15 the last 16 - sh bytes of the aligned piece at s - sh and, if sh != 0, the
    // first sh bytes of the next (whose first byte is wanted, so it lies inside the text).  sh is the same for every piece of a segment.
    __device__ __forceinline__ void load16(const uint8_t *text, uint64_t s, uint32_t w[4]) const {
        const uint32_t sh = (uint32_t)(s & 15), q = sh >> 2, r8 = (sh & 3u) * 8;
        const uint8_t *ap = text + (s - sh);
        const u32x4_t a = *reinterpret_cast<const u32x4_t *>(ap);
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
        if (sh) {
            const u32x4_t b = *reinterpret_cast<const u32x4_t *>(ap + 16);
            // the eight words moved down by q words (named values, constant indices: no array a lane would index at run time) ...
            uint32_t x0 = a.x, x1 = a.y, x2 = a.z, x3 = a.w, x4 = b.x, x5 = b.y, x6 = b.z, x7 = b.w;
            if (q & 2u) { x0 = x2; x1 = x3; x2 = x4; x3 = x5; x4 = x6; x5 = x7; }
            if (q & 1u) { x0 = x1; x1 = x2; x2 = x3; x3 = x4; x4 = x5; }
            // ... and by the 0 .. 3 bytes left (a funnel shift by 0 gives the low word)
            w[0] = __funnelshift_r(x0, x1, r8); w[1] = __funnelshift_r(x1, x2, r8);
            w[2] = __funnelshift_r(x2, x3, r8); w[3] = __funnelshift_r(x3, x4, r8);
        }
    }
    __device__ __forceinline__ void store16(uint8_t *dst, const uint32_t w[4]) const {
        u32x4_t o;
        o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
        *reinterpret_cast<u32x4_t *>(dst) = o;
    }
};

struct XrArgs {
    const uint8_t *text;
    const uint64_t *id_off, *seq_off, *qual_off, *dst_off;  // [n]; ranges checked on the host, dst_off the exclusive scan of the records' lengths
    const uint32_t *id_len, *seq_len, *qual_len;            // [n]
    uint64_t n;
    uint8_t *out;         // 16-byte aligned
    uint64_t out_base;    // record i goes to out + out_base + dst_off[i]
};

// A looping grid of one-wavefront workgroups; a wavefront takes one record at a time.
__global__ void __launch_bounds__(64) k_extract_records(const XrArgs a) {
    const XrWavePolicy pol;
    for (uint64_t i = blockIdx.x; i < a.n; i += gridDim.x)  // (wave-uniform)
        xr_record(pol, a.text, a.id_off[i], a.id_len[i], a.seq_off[i], a.seq_len[i], a.qual_off[i], a.qual_len[i], a.out, a.out_base + a.dst_off[i]);
}
#endif
