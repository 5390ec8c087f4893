// inflate_search.inc -- where does a dynamic-Huffman block start?  The block-start search of a one-stream .gz round (phase A)
// Part of the single translation unit charon_hip.hip (included in order, behind inflate_stream.inc); not a stand-alone source.
//
// THE RULE.  The answer for a range [from, to) of bit positions (LSB first, from bit 0 of the input of in_bytes bytes) is the first
// position p in it that passes all of:
//   R0  (p >> 3) + 8 <= in_bytes, and with at = p + 17: (at >> 3) + 9 <= in_bytes
//   R1  the 3 bits at p are BFINAL = 0, BTYPE = 2 (value 4); the HLIT field <= 29 and the HDIST field <= 29
//   R2  128 >> l summed over the non-zero ones of the HCLEN + 4 three-bit lengths l at p + 17 is exactly 128
//   R3  the dynamic header parses by InfDecoder::dynamic_tables (zlib's acceptance rules)
//   R4  the block decodes until end-of-block or until at least 32 768 symbols are out -- the count is looked at in front of every
//       literal/length code, a match counts as its length, nothing is read once the count is reached; every literal is text (9, 10, 13,
//       32 .. 126), every code valid, no more bits consumed than the input holds; a distance is never refused (the window is unknown)
//   R5  at least 32 symbols came out
//   R6  behind an end-of-block stands a block header that parses, BFINAL either way: stored with LEN == ~NLEN behind the byte boundary,
//       fixed, or dynamic as under R3 (InfDecoder::header_only)
// R0 - R2 are integer tests on 96 bits of input (infs_filter), the eight positions of a byte at a time.  R3 - R6 are a TRIAL: the decoder
// of inflate_members.inc with an output side that stores nothing (InfProbeOut).  Filter, output side and trial are __host__ __device__
// and templated on the decoder's policy like the rest of it; what is built on them today is the host's walk (infs_search_host, one
// lane).  A kernel over them (a wavefront a range, a lane a byte, survivors tried by the whole wavefront) is not part of this file:
// DESIGN 7l says why.  A found position is only a candidate: the counting rule of chn_inflate_stream_run proves or refutes it.

static const uint32_t INFS_PROBE_SYMS = 32768;  // symbols a trial decodes at most (R4)
static const uint32_t INFS_PROBE_MIN = 32;      // and at least (R5)
static const uint64_t INFS_NONE = ~0ull;

struct InfProbeOut {
    static const bool ASKS_FIRST = true;  // R4: the count is looked at in front of a code, so nothing behind symbol 32 768 is read
    uint32_t pos;   // symbols so far
    bool bad;       // a literal that is not text
    __host__ __device__ bool room(uint32_t) const { return !bad && pos < INFS_PROBE_SYMS; }
    __host__ __device__ bool reach(uint32_t) const { return true; }
    template <class P> __host__ __device__ void lit(P &, uint32_t b) {
        if (!(b == 9 || b == 10 || b == 13 || (b >= 32 && b < 127))) bad = true;
        ++pos;
    }
    template <class P> __host__ __device__ void put(P &, uint32_t, uint32_t n) { pos += n; }
    template <class P> __host__ __device__ void match(P &, uint32_t, uint32_t len) { pos += len; }
    __host__ __device__ bool block_end(uint64_t, bool) { return true; }
    __host__ __device__ int finish() const { return INF_OK; }
};

// R0's second half, R1 and R2 for the eight positions of byte b, and the range: bit r is set if position 8 b + r passes.  lo = the
// eight bytes from b, hi = the four behind them (bytes behind the input: zero -- R0 keeps every bit that decides inside it); the caller
// has checked b + 8 <= in_bytes.
__host__ __device__ static inline uint32_t infs_filter(uint64_t lo, uint32_t hi, uint64_t b, uint64_t from, uint64_t to, uint64_t in_bytes) {
    uint32_t pass = 0;
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) {
        const uint64_t pos = b * 8 + r;
        const uint32_t v = (uint32_t)(lo >> r);
        if ((v & 7) != 4 || ((v >> 3) & 31) > 29 || ((v >> 8) & 31) > 29) continue;
        if (pos < from || pos >= to || ((pos + 17) >> 3) + 9 > in_bytes) continue;
        const uint32_t ncode = ((v >> 13) & 15) + 4;
        const uint64_t x = (lo >> (r + 17)) | ((uint64_t)hi << (47 - r));  // the 64 bits from p + 17 on (57 are looked at)
        uint32_t kraft = 0;
        for (uint32_t i = 0; i < ncode; ++i) {
            const uint32_t l = (uint32_t)(x >> (3 * i)) & 7;
            if (l) kraft += 128u >> l;
        }
        if (kraft == 128) pass |= 1u << r;
    }
    return pass;
}

// R3 - R6 at the position the policy stands on
template <class P> __host__ __device__ static bool infs_trial(P &pol, InfShared &sh) {
    InfProbeOut o;
    o.pos = 0; o.bad = false;
    InfDecoder<P, InfProbeOut> d(pol, sh, o);
    d.refill();
    d.drop(3);  // BFINAL = 0, BTYPE = 2 (R1)
    if (d.dynamic_tables() != INF_OK) return false;
    const int st = d.symbols();
    if (o.bad || o.pos < INFS_PROBE_MIN) return false;
    if (st == INF_E_OVER) return true;  // (the only source of it here: the count was reached)
    if (st != INF_OK) return false;
    return d.header_only() == INF_OK;
}

// the host's walk of one range, byte by byte
static uint64_t infs_search_host(InfShared &sh, const uint8_t *in, uint64_t in_bytes, uint64_t from, uint64_t to) {
    for (uint64_t b = from >> 3; b * 8 < to && b + 8 <= in_bytes; ++b) {
        uint8_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        std::memcpy(w, in + b, (size_t)std::min<uint64_t>(12, in_bytes - b));
        uint64_t lo;
        uint32_t hi;
        std::memcpy(&lo, w, 8);
        std::memcpy(&hi, w + 8, 4);
        uint32_t pass = infs_filter(lo, hi, b, from, to, in_bytes);
        for (; pass; pass &= pass - 1) {
            const uint32_t r = (uint32_t)__builtin_ctz(pass);
            InfChunkHostPolicy pol;
            pol.in = in + b; pol.len = in_bytes - b; pol.bit0 = r;
            if (infs_trial(pol, sh)) return b * 8 + r;
        }
    }
    return INFS_NONE;
}
