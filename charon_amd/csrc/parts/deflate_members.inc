// deflate_members.inc -- raw deflate (RFC 1951) compressor for small independent pieces (BGZF members), one wavefront per piece
// Part of the single translation unit charon_hip.hip (included in order, behind gzip_trees.inc and inflate_members.inc); not a stand-alone source.
//
// ONE compressor source for the device and the host, as the decoder in inflate_members.inc: everything that decides a byte of the output is
// __host__ __device__ code templated on a small policy.  On the device the policy is a wavefront, on the host it has one lane and walks
// the 64 slots of a group serially.  The bytes are the same under both: chn_deflate_run_host, the CPU tests and the fuzzer check the
// statements the kernel runs, and tests/test_gpu_deflate.py compares the two byte for byte.
//
// A piece (at most 65 280 bytes, bgzip's block size) becomes ONE deflate block with BFINAL = 1:
//   crc     CRC-32 of the piece while it lies in LDS (inf_crc32_at: 64 slices and the exact join)
//   parse   groups of 64 positions, one a lane.  Candidates of position p: the position one byte back (runs), the nearest earlier lane of
//           the group with the same 4-byte hash, and the hash table's entry (a position of an earlier group).  The longest wins, the
//           nearer on a tie; it is kept if it pays (dfl_accept: by length and distance).  A left-to-right walk over the group picks
//           the tokens (greedy, one step lazy).  Tokens go to the workgroup's global scratch, their code frequencies to LDS.
//   trees   lane 0: gztrees::plan_block (zlib's build_tree / build_bl_tree and its stored / static / dynamic choice), the block header
//           (gztrees::send_tree), canonical codes.  A piece that does not compress leaves as a stored block.
//   encode  64 tokens a round: a lane's token is at most 48 bits, a wave scan gives its bit offset, the bits are OR-ed into a 4 KiB ring
//           in LDS whose finished halves go out as aligned 16-byte stores.
// Determinism: nothing depends on the order in which lanes reach LDS.  Hash-table inserts: of the lanes of a group that share a hash only
// the highest stores (the 64-step sweep that finds the nearest earlier lane finds that too), so every store of a round has its own
// slot; the table is read before the round's inserts.  Frequencies are sums, the ring is OR-ed: both commute.
// Every loop is bounded by the piece's length (positions, tokens) or by 258 (a match), so the kernel terminates on any input.

#ifndef __HIPCC__  // a CPU build of the compressor alone (tools/fuzz/deflate_members_fuzz.cpp)
#define __host__
#define __device__
#endif

static const uint32_t DFL_MAX_IN = 65280;
static const uint32_t DFL_GROUP = 64;                   // positions / tokens a round
static const uint32_t DFL_HASH_BITS = 12;
static const uint32_t DFL_NIL = 0xFFFFu;                // empty hash-table entry (no position is that high)
static const uint32_t DFL_NOHASH = 0xFFFFFFFFu;         // a position with fewer than 4 bytes behind it
static const uint32_t DFL_WINDOW = 32768;               // the farthest distance deflate can name
static const uint32_t DFL_RING_WORDS = 1024, DFL_HALF = 2048;  // the output ring: 4 KiB, flushed in halves
static const uint32_t DFL_BGZF_HEAD = 18, DFL_BGZF_TAIL = 8;
static const uint32_t DFL_SLOT = 65312;                 // a member's stretch of the kernel's output: 18 + 65 280 + 5 + 8, rounded up to 16
static const uint32_t DFL_F_BGZF = 1u;
// the acceptance rule: a match must be at least this long to pay for its length and distance codes
static const uint32_t DFL_MIN_NEAR = 4, DFL_MIN_MID = 5, DFL_MIN_FAR = 7, DFL_NEAR = 64, DFL_MID = 4096;

struct alignas(16) DflShared {
    uint8_t in[DFL_MAX_IN + 32];   // the piece; reads of 4 bytes at a time may reach 3 bytes behind it
    union {
        uint32_t crc_tab[1024];                  // crc
        uint16_t hash[1u << DFL_HASH_BITS];      // parse
        gztrees::Work work;                      // trees
    } u;
    uint32_t lf[288], df[32];      // frequencies, then codes: length << 16 | the code's bits in sending order
    uint32_t blc[20];              // codes of the bit-length tree
    uint32_t ring[DFL_RING_WORDS]; // image byte q lives at byte q % 4096
    uint32_t info[4];              // lane 0 to all: block type, bit position behind the header, the planned size
};
static_assert(sizeof(DflShared) <= 81920, "two workgroups per CU");

__host__ __device__ static inline uint32_t dfl_load32(const uint8_t *p) { uint32_t w; __builtin_memcpy(&w, p, 4); return w; }
__host__ __device__ static inline uint32_t dfl_hash(uint32_t w) { return (w * 0x9E3779B1u) >> (32 - DFL_HASH_BITS); }
// bytes that agree between positions a < pos, at most maxlen (<= 258, and no more than the piece has behind pos)
__host__ __device__ static inline uint32_t dfl_match(const uint8_t *in, uint32_t a, uint32_t pos, uint32_t maxlen) {
    uint32_t l = 0;
    while (l < maxlen) {
        const uint32_t x = dfl_load32(in + a + l) ^ dfl_load32(in + pos + l);
        if (x) { l += (uint32_t)__builtin_ctz(x) >> 3; break; }
        l += 4;
    }
    return l < maxlen ? l : maxlen;
}
__host__ __device__ static inline bool dfl_accept(uint32_t len, uint32_t dist) {
    return len >= (dist <= DFL_NEAR ? DFL_MIN_NEAR : dist <= DFL_MID ? DFL_MIN_MID : DFL_MIN_FAR);
}
__host__ __device__ static inline uint32_t dfl_reverse(uint32_t code, uint32_t bits) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < bits; ++i) r |= ((code >> i) & 1u) << (bits - 1 - i);
    return r;
}
// canonical codes (RFC 1951 3.2.2) of n code lengths, as length << 16 | reversed code (deflate sends a code's first bit first)
// cnt, next: 16 values of scratch each.  Only lens[0 .. used) count (behind them lies the guard of scan_tree / send_tree)
template <class L> __host__ __device__ static inline void dfl_gen_codes(const L *lens, uint32_t used, uint32_t n, uint32_t *out, uint16_t *cnt, uint16_t *next) {
    for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
    for (uint32_t s = 0; s < used; ++s) cnt[lens[s]]++;
    cnt[0] = 0; next[0] = 0;
    for (uint32_t l = 1; l < 16; ++l) next[l] = (next[l - 1] + cnt[l - 1]) << 1;
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = s < used ? lens[s] : 0;
        out[s] = l ? (l << 16) | dfl_reverse(next[l], l) : 0u;
        if (l) next[l]++;
    }
}

// ---- policies --------------------------------------------------------------------------------------------------------------------
// A group's 64 slots: lane l holds slots l, l + LANES, ... in arrays of 64 / LANES values
struct DflHostPolicy {
    static const uint32_t LANES = 1;
    uint32_t lane() const { return 0; }
    uint32_t uni(uint32_t v) const { return v; }
    void sync() const {}
    uint32_t get(const uint32_t *a, uint32_t j) const { return a[j]; }  // slot j's value
    void add32(uint32_t *p, uint32_t v) const { *p += v; }
    void or32(uint32_t *p, uint32_t v) const { *p |= v; }
    uint32_t excl_scan(uint32_t *a) const {  // a[] becomes the sum of the slots in front; returns the sum of all
        uint32_t s = 0;
        for (uint32_t j = 0; j < DFL_GROUP; ++j) { const uint32_t v = a[j]; a[j] = s; s += v; }
        return s;
    }
    void store16(uint8_t *dst, const uint32_t *src) const { __builtin_memcpy(dst, src, 16); }
    uint32_t slice_down(const uint32_t *part, uint32_t k, uint32_t d) const { return k + d < INF_CRC_SLICES ? part[k + d] : 0u; }
};
#ifdef __HIPCC__
struct DflWavePolicy {
    static const uint32_t LANES = WAVE;
    __device__ uint32_t lane() const { return lane_id(); }
    __device__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    // one wavefront per workgroup: its LDS and global operations execute in order, the fence keeps the compiler from moving them across
    __device__ void sync() const { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); }
    __device__ uint32_t get(const uint32_t *a, uint32_t j) const { return (uint32_t)__builtin_amdgcn_readlane((int)a[0], (int)j); }  // j is wave-uniform
    __device__ void add32(uint32_t *p, uint32_t v) const { atomicAdd(p, v); }
    __device__ void or32(uint32_t *p, uint32_t v) const { atomicOr(p, v); }
    __device__ uint32_t excl_scan(uint32_t *a) const {
        const uint32_t own = a[0], s = wave_scan(own);
        a[0] = s - own;
        return (uint32_t)__builtin_amdgcn_readlane((int)s, WAVE - 1);
    }
    __device__ void store16(uint8_t *dst, const uint32_t *src) const { *reinterpret_cast<u32x4_t *>(dst) = *reinterpret_cast<const u32x4_t *>(src); }
    __device__ uint32_t slice_down(const uint32_t *part, uint32_t, uint32_t d) const {
        const uint32_t v = (uint32_t)__shfl_down((int)part[0], d);
        return lane_id() + d < INF_CRC_SLICES ? v : 0u;
    }
};
#endif

// ---- the compressor --------------------------------------------------------------------------------------------------------------
template <class P> struct DflCoder {
    static const uint32_t SLOTS = DFL_GROUP / P::LANES;
    P &p;
    DflShared &sh;
    uint32_t n;          // bytes of the piece, in sh.in
    uint32_t *tokens;    // [DFL_MAX_IN] scratch: a literal's byte, or 1 << 31 | (length - 3) << 16 | distance - 1
    uint8_t *dst;        // the member's image, 16-byte aligned, DFL_SLOT bytes
    uint32_t flushed = 0;

    __host__ __device__ DflCoder(P &p_, DflShared &sh_, uint32_t n_, uint32_t *tokens_, uint8_t *dst_) : p(p_), sh(sh_), n(n_), tokens(tokens_), dst(dst_) {}

    // -- bits into the ring: `bp` is the bit position in the member's image
    __host__ __device__ void put(uint32_t &bp, uint32_t v, uint32_t nb) {  // nb <= 16, one lane
        const uint32_t w = (bp >> 5) & (DFL_RING_WORDS - 1), s = bp & 31;
        sh.ring[w] |= v << s;
        if (s + nb > 32) sh.ring[(w + 1) & (DFL_RING_WORDS - 1)] |= v >> (32 - s);
        bp += nb;
    }
    struct TreeSink {  // what gztrees::send_tree writes through
        DflCoder &c;
        uint32_t &bp;
        __host__ __device__ void bl(int sym) { const uint32_t e = c.sh.blc[sym]; c.put(bp, e & 0xFFFFu, e >> 16); }
        __host__ __device__ void bits(uint32_t v, int nb) { c.put(bp, v, (uint32_t)nb); }
    };
    // image bytes [flushed, flushed + bytes) leave the ring, 16 at a time; the ring is zero behind them
    __host__ __device__ void flush(uint32_t bytes) {
        const uint32_t lane = p.lane(), chunks = (bytes + 15) / 16;
        for (uint32_t c = lane; c < chunks; c += P::LANES) {
            uint32_t *src = sh.ring + (((flushed >> 2) + c * 4) & (DFL_RING_WORDS - 1));
            if (flushed + c * 16 + 16 <= DFL_SLOT) p.store16(dst + flushed + c * 16, src);  // (always: a member is at most its planned size)
            src[0] = src[1] = src[2] = src[3] = 0;
        }
        flushed += bytes;
        p.sync();
    }

    // -- parse: tokens and frequencies; returns the number of tokens
    __host__ __device__ uint32_t parse() {
        const uint32_t lane = p.lane();
        for (uint32_t i = lane; i < (1u << DFL_HASH_BITS) / 2; i += P::LANES) reinterpret_cast<uint32_t *>(sh.u.hash)[i] = DFL_NIL | (DFL_NIL << 16);
        for (uint32_t i = lane; i < 288; i += P::LANES) sh.lf[i] = 0;
        for (uint32_t i = lane; i < 32; i += P::LANES) sh.df[i] = 0;
        p.sync();
        uint32_t ntok = 0, covered = 0;  // positions below `covered` lie inside a token already
        for (uint32_t b = 0; b < n; b += DFL_GROUP) {
            const uint32_t cnt = n - b < DFL_GROUP ? n - b : DFL_GROUP;
            uint32_t h[SLOTS], w4[SLOTS], near[SLOTS], lose[SLOTS], ml[SLOTS], md[SLOTS];
            for (uint32_t k = 0, i = lane; k < SLOTS; ++k, i += P::LANES) {
                const uint32_t pos = b + i;
                w4[k] = dfl_load32(sh.in + (pos < n ? pos : 0));
                h[k] = pos + 4 <= n ? dfl_hash(w4[k]) : DFL_NOHASH;
                near[k] = DFL_GROUP; lose[k] = 0; ml[k] = 0; md[k] = 0;
            }
            // the sweep: the nearest earlier slot with this hash, and whether a later one has it (then that one is inserted, not this)
            for (uint32_t j = 0; j < cnt; ++j) {
                const uint32_t hj = p.get(h, j);
                for (uint32_t k = 0, i = lane; k < SLOTS; ++k, i += P::LANES)
                    if (hj == h[k] && hj != DFL_NOHASH) { if (j < i) near[k] = j; else if (j > i) lose[k] = 1; }
            }
            const bool search = covered < b + cnt;  // (wave-uniform) a match reaching over the whole group leaves nothing to look for
            if (search)
                for (uint32_t k = 0, i = lane; k < SLOTS; ++k, i += P::LANES) {
                    const uint32_t pos = b + i;
                    if (i >= cnt || pos < covered) continue;
                    const uint32_t maxlen = n - pos < 258 ? n - pos : 258;
                    uint32_t best = 0, dist = 0;
                    if (pos >= 1) { best = dfl_match(sh.in, pos - 1, pos, maxlen); dist = 1; }
                    if (near[k] < DFL_GROUP && best < maxlen) {
                        const uint32_t c = b + near[k];
                        if (dfl_load32(sh.in + c) == w4[k]) { const uint32_t l = dfl_match(sh.in, c, pos, maxlen); if (l > best) { best = l; dist = pos - c; } }
                    }
                    if (h[k] != DFL_NOHASH && best < maxlen) {
                        const uint32_t c = sh.u.hash[h[k]];
                        if (c != DFL_NIL && pos - c <= DFL_WINDOW && dfl_load32(sh.in + c) == w4[k]) {
                            const uint32_t l = dfl_match(sh.in, c, pos, maxlen);
                            if (l > best) { best = l; dist = pos - c; }
                        }
                    }
                    if (best >= 3 && dfl_accept(best, dist)) { ml[k] = best; md[k] = dist; }
                }
            p.sync();  // the table was read
            for (uint32_t k = 0; k < SLOTS; ++k)
                if (h[k] != DFL_NOHASH && !lose[k]) sh.u.hash[h[k]] = (uint16_t)(b + k * P::LANES + lane);
            // the walk: which positions start a token (wave-uniform)
            uint64_t starts = 0, matches = 0;
            uint32_t r = covered > b ? covered - b : 0;
            while (r < cnt) {
                uint32_t l = p.get(ml, r);
                if (l && r + 1 < cnt && p.get(ml, r + 1) > l) l = 0;  // one step lazy: the next position has the longer match
                starts |= 1ull << r;
                if (l) { matches |= 1ull << r; r += l; } else r += 1;
            }
            covered = b + r;
            for (uint32_t k = 0, i = lane; k < SLOTS; ++k, i += P::LANES) {
                if (!((starts >> i) & 1)) continue;
                const uint32_t at = ntok + inf_popc64(starts & ((1ull << i) - 1));
                if ((matches >> i) & 1) {
                    const uint32_t lc = ml[k] - 3, d = md[k] - 1;
                    tokens[at] = 0x80000000u | (lc << 16) | d;
                    p.add32(&sh.lf[257 + gztrees::length_code(lc)], 1);
                    p.add32(&sh.df[gztrees::dist_code(d)], 1);
                } else {
                    const uint32_t c = sh.in[b + i];
                    tokens[at] = c;
                    p.add32(&sh.lf[c], 1);
                }
            }
            ntok += inf_popc64(starts);
            p.sync();  // the inserts are visible to the next group
        }
        return ntok;
    }

    // -- a token's bits, in sending order: code, extra bits, distance code, extra bits (at most 15 + 5 + 15 + 13)
    __host__ __device__ uint64_t token_bits(uint32_t tok, uint32_t &nb) const {
        if (!(tok & 0x80000000u)) { const uint32_t e = sh.lf[tok]; nb = e >> 16; return e & 0xFFFFu; }
        const uint32_t lc = (tok >> 16) & 255u, d = tok & 0x7FFFu;
        const uint32_t c = gztrees::length_code(lc), dc = gztrees::dist_code(d);
        const uint32_t xl = (uint32_t)gztrees::extra_bits(0, (int)c), xd = (uint32_t)gztrees::extra_bits(1, (int)dc);
        const uint32_t el = sh.lf[257 + c], ed = sh.df[dc];
        uint64_t v = el & 0xFFFFu;
        uint32_t at = el >> 16;
        v |= (uint64_t)(lc & ((1u << xl) - 1)) << at; at += xl;
        v |= (uint64_t)(ed & 0xFFFFu) << at; at += ed >> 16;
        v |= (uint64_t)(d & ((1u << xd) - 1)) << at; at += xd;
        nb = at;
        return v;
    }

    // -- one member: returns its size; *crc_out is the piece's CRC-32
    __host__ __device__ uint32_t run(uint32_t flags, uint32_t *crc_out) {
        const uint32_t lane = p.lane();
        const uint32_t head = (flags & DFL_F_BGZF) ? DFL_BGZF_HEAD : 0, tail = (flags & DFL_F_BGZF) ? DFL_BGZF_TAIL : 0;
        for (uint32_t i = lane; i < DFL_RING_WORDS; i += P::LANES) sh.ring[i] = 0;
        const uint32_t crc = inf_crc32_at(p, sh.u.crc_tab, sh.in, 0, n);
        *crc_out = crc;
        p.sync();
        const uint32_t ntok = parse();
        if (lane == 0) {
            gztrees::Work &w = sh.u.work;  // (the hash table is dead)
            const gztrees::BlockPlan plan = gztrees::plan_block(w, sh.lf, sh.df);
            const uint32_t type = (uint64_t)n + 4 <= plan.opt_lenb ? 0u : plan.static_lenb == plan.opt_lenb ? 1u : 2u;
            const uint32_t body = type == 0 ? n + 5 : (uint32_t)plan.opt_lenb, total = head + body + tail;
            uint32_t bp = 0;
            if (head) {
                const uint32_t hw[9] = {0x8B1F, 0x0408, 0, 0, 0xFF00, 0x0006, 0x4342, 0x0002, total - 1};  // gzip, FEXTRA, the BC subfield, BSIZE
                for (uint32_t i = 0; i < 9; ++i) put(bp, hw[i], 16);
            }
            if (type == 0) {
                put(bp, 1, 8); put(bp, n, 16); put(bp, n ^ 0xFFFFu, 16);  // BFINAL, type 0, padded to a byte; LEN, NLEN
            } else {
                put(bp, 1u | (type << 1), 3);
                if (type == 2) {
                    dfl_gen_codes(w.bllen, gztrees::BL_CODES, gztrees::BL_CODES, sh.blc, w.heap, w.heap + 16);  // (the heap is dead)
                    const uint8_t order[gztrees::BL_CODES] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                    put(bp, (uint32_t)plan.max_l + 1 - 257, 5); put(bp, (uint32_t)plan.max_d, 5); put(bp, (uint32_t)plan.max_blindex + 1 - 4, 4);  // send_all_trees
                    for (int r = 0; r <= plan.max_blindex; ++r) put(bp, w.bllen[order[r]], 3);
                    TreeSink sink{*this, bp};
                    gztrees::send_tree(sink, w.llen, plan.max_l);
                    gztrees::send_tree(sink, w.dlen, plan.max_d);
                    dfl_gen_codes(w.llen, (uint32_t)plan.max_l + 1, gztrees::L_CODES, sh.lf, w.heap, w.heap + 16);
                    dfl_gen_codes(w.dlen, (uint32_t)plan.max_d + 1, gztrees::D_CODES, sh.df, w.heap, w.heap + 16);
                } else {
                    for (uint32_t s = 0; s < 288; ++s) {  // RFC 1951 3.2.6
                        const uint32_t l = (uint32_t)gztrees::static_len_of(0, (int)s);
                        const uint32_t code = s < 144 ? 0x30 + s : s < 256 ? 0x190 + (s - 144) : s < 280 ? s - 256 : 0xC0 + (s - 280);
                        sh.lf[s] = (l << 16) | dfl_reverse(code, l);
                    }
                    for (uint32_t s = 0; s < 30; ++s) sh.df[s] = (5u << 16) | dfl_reverse(s, 5);
                }
            }
            sh.info[0] = type; sh.info[1] = bp; sh.info[2] = total;
        }
        p.sync();
        const uint32_t type = p.uni(sh.info[0]), total = p.uni(sh.info[2]);
        uint32_t bp = p.uni(sh.info[1]);
        if (type == 0) {
            // stored: the piece itself behind the header; image byte q is piece byte q - at
            const uint32_t at = bp >> 3;
            const uint8_t *hdr = reinterpret_cast<const uint8_t *>(sh.ring);  // what lane 0 wrote: `at` bytes (both targets are little-endian)
            for (uint32_t q = lane * 16; q < at + n + tail; q += P::LANES * 16) {
                alignas(16) uint32_t v[4] = {0, 0, 0, 0};
                for (uint32_t i = 0; i < 16; ++i) {
                    const uint32_t o = q + i;
                    uint32_t byte = 0;
                    if (o < at) byte = hdr[o];
                    else if (o < at + n) byte = sh.in[o - at];
                    else if (o < at + n + 4) byte = (crc >> (8 * (o - at - n))) & 255u;
                    else if (o < at + n + 8) byte = (n >> (8 * (o - at - n - 4))) & 255u;
                    v[i >> 2] |= byte << (8 * (i & 3));
                }
                p.store16(dst + q, v);
            }
            p.sync();
            return total;
        }
        // encode: DFL_GROUP tokens a round, the end-of-block code behind the last
        for (uint32_t t0 = 0; t0 <= ntok; t0 += DFL_GROUP) {
            uint64_t v[SLOTS];
            uint32_t nb[SLOTS];
            for (uint32_t k = 0, i = lane; k < SLOTS; ++k, i += P::LANES) {
                const uint32_t t = t0 + i;
                v[k] = 0; nb[k] = 0;
                if (t < ntok) v[k] = token_bits(tokens[t], nb[k]);
                else if (t == ntok) { const uint32_t e = sh.lf[gztrees::END_BLOCK]; v[k] = e & 0xFFFFu; nb[k] = e >> 16; }
            }
            uint32_t off[SLOTS];
            for (uint32_t k = 0; k < SLOTS; ++k) off[k] = nb[k];
            const uint32_t sum = p.excl_scan(off);
            for (uint32_t k = 0; k < SLOTS; ++k) {
                if (!nb[k]) continue;
                const uint32_t at = bp + off[k], wd = at >> 5, s = at & 31;
                const uint64_t hi = (v[k] >> 1) >> (31 - s);  // what does not fit the first word
                p.or32(&sh.ring[wd & (DFL_RING_WORDS - 1)], (uint32_t)(v[k] << s));
                if ((uint32_t)hi) p.or32(&sh.ring[(wd + 1) & (DFL_RING_WORDS - 1)], (uint32_t)hi);
                if (hi >> 32) p.or32(&sh.ring[(wd + 2) & (DFL_RING_WORDS - 1)], (uint32_t)(hi >> 32));
            }
            bp += sum;
            p.sync();
            while ((bp >> 3) - flushed >= DFL_HALF) flush(DFL_HALF);  // (wave-uniform) at most 384 bytes a round: never more than once
        }
        bp = (bp + 7) & ~7u;
        if (tail) {  // CRC-32 and ISIZE
            uint32_t t = bp;
            if (lane == 0) { put(t, crc & 0xFFFFu, 16); put(t, crc >> 16, 16); put(t, n & 0xFFFFu, 16); put(t, n >> 16, 16); }
            bp += tail * 8;
        }
        p.sync();
        const uint32_t made = bp >> 3;
        while (made - flushed >= DFL_HALF) flush(DFL_HALF);
        flush(made - flushed);
        return made == total ? total : 0xFFFFFFFFu;  // (cannot differ: plan_block counted the bits that were sent)
    }
};

// host entry: one member of `len` bytes; `sh` and `tokens` ([DFL_MAX_IN]) are the caller's scratch, `slot` has DFL_SLOT bytes; returns its size
static uint32_t dfl_member_host(DflShared &sh, uint32_t *tokens, const uint8_t *in, uint32_t len, uint32_t flags, uint8_t *slot, uint32_t *crc) {
    if (len) std::memcpy(sh.in, in, len);
    std::memset(sh.in + len, 0, sizeof(sh.in) - len);
    DflHostPolicy pol;
    DflCoder<DflHostPolicy> c(pol, sh, len, tokens, slot);
    return c.run(flags, crc);
}

#ifdef __HIPCC__
// ---- kernels ---------------------------------------------------------------------------------------------------------------------
struct DeflateArgs {
    const uint8_t *in;        // packed pieces, each on a 16-byte boundary, 16 readable bytes behind the last
    const uint64_t *in_off;   // [n] from `in`, multiples of 16
    const uint32_t *in_len;   // <= DFL_MAX_IN (checked on the host)
    uint8_t *slots;           // [n] stretches of DFL_SLOT bytes
    uint32_t *out_len;        // [n]
    uint32_t *crc;            // [n]
    uint32_t *tokens;         // [gridDim.x][DFL_MAX_IN]
    uint32_t *cursor;
    uint32_t n, flags;
};

__global__ void __launch_bounds__(WAVE) k_deflate_members(DeflateArgs a) {
    __shared__ DflShared sh;
    const uint32_t lane = lane_id();
    uint32_t *tokens = a.tokens + (size_t)blockIdx.x * DFL_MAX_IN;
    DflWavePolicy pol;
    for (;;) {
        uint32_t m = 0;
        if (lane == 0) m = atomicAdd(a.cursor, 1u);
        m = (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
        if (m >= a.n) break;
        const uint8_t *src = a.in + a.in_off[m];
        const uint32_t len = min(a.in_len[m], DFL_MAX_IN);
        for (uint32_t c = lane * 16; c < len; c += WAVE * 16) *reinterpret_cast<u32x4_t *>(sh.in + c) = *reinterpret_cast<const u32x4_t *>(src + c);
        pol.sync();
        for (uint32_t i = len + lane; i < ((len + 15) & ~15u) + 16; i += WAVE) sh.in[i] = 0;  // nothing behind the piece is the staging's
        pol.sync();
        DflCoder<DflWavePolicy> c(pol, sh, len, tokens, a.slots + (size_t)m * DFL_SLOT);
        uint32_t crc;
        const uint32_t size = c.run(a.flags, &crc);
        if (lane == 0) { a.out_len[m] = size; a.crc[m] = crc; }
        pol.sync();  // LDS and the token scratch are the next member's from here
    }
}

// out_off[i] = the sizes in front of member i, out_off[n] = their sum; one workgroup (array_scan, scan.inc)
__global__ void __launch_bounds__(SCAN_THREADS) k_deflate_scan(const uint32_t *out_len, uint64_t *out_off, uint32_t n) {
    const uint64_t sum = array_scan<SCAN_THREADS, uint64_t>(
        n, [&](uint32_t i) { const uint32_t len = out_len[i]; return len <= DFL_SLOT ? len : 0u; },  // (a member that failed its size check takes no room)
        [&](uint32_t i, uint64_t at) { out_off[i] = at; });
    if (threadIdx.x == 0) out_off[n] = sum;
}

// the members back to back: member blockIdx.x from its slot to packed + out_off; whole destination words where it can
__global__ void __launch_bounds__(256) k_deflate_gather(const uint8_t *slots, const uint32_t *out_len, const uint64_t *out_off, uint8_t *packed, uint64_t packed_bytes) {
    const uint32_t m = blockIdx.x, len = out_len[m];
    if (len > DFL_SLOT || out_off[m] + len > packed_bytes) return;  // (a member that failed its size check: nothing of it is copied)
    const uint8_t *src = slots + (size_t)m * DFL_SLOT;
    uint8_t *dst = packed + out_off[m];
    const uint32_t lead = min(len, (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3));  // bytes in front of the first whole word
    const uint32_t words = (len - lead) / 4;
    for (uint32_t i = threadIdx.x; i < lead; i += blockDim.x) dst[i] = src[i];
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(src);
    const uint32_t sh = lead * 8;  // source byte lead + 4 k + j is byte j of destination word k
    for (uint32_t k = threadIdx.x; k < words; k += blockDim.x) {
        const uint32_t lo = sw[k], hi = sw[k + 1];  // (inside the slot: 4 k + 8 <= len + 4 <= DFL_SLOT)
        reinterpret_cast<uint32_t *>(dst + lead)[k] = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
    }
    for (uint32_t i = lead + words * 4 + threadIdx.x; i < len; i += blockDim.x) dst[i] = src[i];
}
#endif
