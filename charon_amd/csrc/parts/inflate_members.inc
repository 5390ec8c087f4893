// inflate_members.inc -- raw deflate (RFC 1951) decoder for small independent members (BGZF), one wavefront per member
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.
//
// ONE decoder source for the device and the host.  Everything that decides what is accepted -- the bit reader, the block headers, the
// code-length parsing, the table construction, the symbol loop and every bounds check -- is __host__ __device__ code templated on a
// small policy.  On the device the policy is a wavefront: the decoder state (bit buffer, positions, table entries) is wave-uniform, the
// 64 lanes share the table construction and the match copy, and nothing diverges.  On the host the policy has one lane and the same
// loops run serially.  chn_inflate_run_host and the CPU tests therefore exercise the logic the kernel runs.
//
// Layout of a member's work in LDS (InfShared, 78 KiB -- two workgroups of one wavefront per CU):
//   win    the member's whole output (at most 64 KiB): a back-reference is an LDS read; it is written out once at the end, 16 bytes a lane
//   stage  two 1 KiB chunks of input: chunk c + 1 waits in registers (one 16-byte vector load per lane) while chunk c is consumed
//   ll/dd  literal/length table (10-bit first level + sub-tables) and distance table (8-bit first level + sub-tables), one word an entry
//
// What is accepted is what zlib's inflate accepts: over-subscribed code sets and incomplete ones are rejected (except a literal/length or
// distance set that is a single 1-bit code, and an empty distance set), as are a missing end-of-block code, HLIT > 286, HDIST > 30, block
// type 3, a stored LEN/NLEN mismatch, a distance reaching before the member's first byte; bytes behind the final block are ignored.
// Every loop consumes input bits, and consuming more than the member holds ends the decode, so it terminates on any input.
//
// CRC-32 (inf_crc32, behind chn_inflate_run_crc / chn_inflate_run_host_crc): taken over the finished window, before it is written out.
// The member is cut into 64 slices of equal length S = ceil(n / 64) by OUTPUT byte position, zero bytes imagined in front of the first
// byte where 64 S > n (zero bytes in front of everything leave a CRC register of 0 at 0); every slice goes through a slice-by-4 loop
// whose four tables the lanes build in `ll` (dead once decoding has ended), and the 64 registers are joined exactly in a six-round tree:
// left * x^(8 S 2^r) + right modulo the reflected polynomial, the multiplier wave-uniform.  The host policy walks the same 64 slices and
// the same tree serially.

#ifndef __HIPCC__  // a CPU build of the decoder alone (tools/fuzz/inflate_fuzz.cpp)
#define __host__
#define __device__
#endif

enum { INF_OK = 0, INF_E_INPUT = 1, INF_E_HEADER = 2, INF_E_LENGTHS = 3, INF_E_SYMBOL = 4, INF_E_OVER = 5, INF_E_SHORT = 6 };

static const uint32_t INF_MAX_OUT = 65536;
static const uint32_t INF_LL_ROOT = 10, INF_LL_CAP = 2048;  // zlib's `enough 286 10 15` is 1334 entries
static const uint32_t INF_DD_ROOT = 8, INF_DD_CAP = 512;    // `enough 30 8 15` is 402
static const uint32_t INF_PRE_ROOT = 7, INF_PRE_CAP = 128;  // code-length codes are at most 7 bits: no sub-tables
static const uint32_t INF_CHUNK_WORDS = 256;                // 64 lanes x 16 bytes
static const uint32_t INF_PAD = 64;                         // bytes the library keeps in front of and behind the device input
static const uint32_t INF_CRC_SLICES = 64;                  // slices a member's CRC-32 is taken in (the wavefront's lanes)
static const uint32_t INF_CRC_POLY = 0xEDB88320u;           // the gzip polynomial, reflected: bit 31 is x^0

struct alignas(16) InfShared {
    uint8_t win[INF_MAX_OUT + 16];  // output byte k lives at win[wmis + k], wmis = the destination's misalignment to 16 bytes
    uint32_t ll[INF_LL_CAP];
    uint32_t dd[INF_DD_CAP];
    uint32_t pre[INF_PRE_CAP];
    uint32_t stage[2 * INF_CHUNK_WORDS];
    uint32_t alloc;                 // sub-table allocation cursor of the table under construction
    uint8_t lens[320];              // code lengths: literal/length symbols, then distance symbols
    uint8_t plens[32];              // code lengths of the code-length code
};

// table entry: bits 0-3 code bits to drop, 4-7 kind, 8-12 extra bits (or sub-table index bits), 16-31 base value (or sub-table offset)
enum { INF_K_INVALID = 0, INF_K_LIT = 1, INF_K_LEN = 2, INF_K_EOB = 3, INF_K_SUB = 4 };
enum { INF_T_PRE = 0, INF_T_LL = 1, INF_T_DD = 2 };
__host__ __device__ static inline uint32_t inf_entry(uint32_t kind, uint32_t bits, uint32_t extra, uint32_t base) {
    return bits | (kind << 4) | (extra << 8) | (base << 16);
}
__host__ __device__ static inline uint32_t inf_symbol_entry(int table, uint32_t sym, uint32_t bits) {
    if (table == INF_T_PRE) return inf_entry(INF_K_LIT, bits, 0, sym);
    if (table == INF_T_LL) {
        if (sym < 256) return inf_entry(INF_K_LIT, bits, 0, sym);
        if (sym == 256) return inf_entry(INF_K_EOB, bits, 0, 0);
        if (sym > 285) return inf_entry(INF_K_INVALID, bits, 0, 0);
        const uint32_t i = sym - 257;
        if (i < 8) return inf_entry(INF_K_LEN, bits, 0, 3 + i);
        if (i == 28) return inf_entry(INF_K_LEN, bits, 0, 258);
        const uint32_t x = (i >> 2) - 1;
        return inf_entry(INF_K_LEN, bits, x, 3 + ((4 + (i & 3)) << x));
    }
    if (sym > 29) return inf_entry(INF_K_INVALID, bits, 0, 0);
    if (sym < 4) return inf_entry(INF_K_LEN, bits, 0, sym + 1);
    const uint32_t x = (sym >> 1) - 1;
    return inf_entry(INF_K_LEN, bits, x, 1 + ((2 + (sym & 1)) << x));
}
__host__ __device__ static inline uint32_t inf_reverse(uint32_t code, uint32_t bits) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < bits; ++i) r |= ((code >> i) & 1u) << (bits - 1 - i);
    return r;
}
__host__ __device__ static inline uint32_t inf_popc64(uint64_t m) {
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)__popcll(m);
#else
    return (uint32_t)__builtin_popcountll(m);
#endif
}

// ---- policies --------------------------------------------------------------------------------------------------------------------
// host: one lane, the member's bytes read in place (bytes behind the member read as zero)
struct InfHostPolicy {
    static const uint32_t LANES = 1;
    const uint8_t *in;
    uint64_t len;
    uint32_t lane() const { return 0; }
    uint32_t uni(uint32_t v) const { return v; }
    uint64_t ballot(bool p) const { return p ? 1u : 0u; }
    uint32_t below(uint64_t) const { return 0; }  // lanes below this one that are set in a ballot
    void sync() const {}
    uint32_t first_word() const { return 0; }
    uint64_t bit_begin() const { return 0; }
    uint64_t bit_end() const { return len * 8; }
    uint32_t word(uint32_t w) const {
        const uint64_t b = (uint64_t)w * 4;
        uint32_t v = 0;
        for (uint32_t i = 0; i < 4; ++i) if (b + i < len) v |= (uint32_t)in[b + i] << (8 * i);
        return v;
    }
    uint32_t fetch_add(uint32_t *p, uint32_t n) const { const uint32_t o = *p; *p = o + n; return o; }
    void fetch_max(uint32_t *p, uint32_t v) const { if (v > *p) *p = v; }
    // CRC join: the register of slice k + d (0 behind the last slice); this lane holds every slice, in order
    uint32_t slice_down(const uint32_t *part, uint32_t k, uint32_t d) const { return k + d < INF_CRC_SLICES ? part[k + d] : 0u; }
};

#ifdef __HIPCC__
// device: one wavefront.  The input is read from `abase` (the member's first byte rounded down to 16 bytes) in chunks of 1 KiB, each
// lane one aligned 16-byte load; bytes in front of the member are skipped, bytes behind it are masked to zero, and no load starts at or
// behind the member's end -- so at most 15 bytes on either side are touched, inside the padding the library allocates.
struct InfWavePolicy {
    static const uint32_t LANES = WAVE;
    const uint8_t *abase;
    uint64_t begin, end;  // the member's bytes are [begin, end) from abase; begin < 16
    uint32_t *stage;
    uint32_t staged;      // chunks written to `stage` so far; chunk `staged` waits in `reg`
    u32x4_t reg;
    __device__ uint32_t lane() const { return lane_id(); }
    __device__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ uint64_t ballot(bool p) const { return __ballot(p ? 1 : 0); }
    __device__ uint32_t below(uint64_t m) const { return (uint32_t)__popcll(m & ((1ull << lane_id()) - 1)); }
    // one wavefront per workgroup: its LDS operations execute in order, the fence keeps the compiler from moving them across
    __device__ void sync() const { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); }
    __device__ uint32_t first_word() const { return (uint32_t)(begin >> 2); }
    __device__ uint64_t bit_begin() const { return begin * 8; }
    __device__ uint64_t bit_end() const { return end * 8; }
    __device__ u32x4_t load_chunk(uint32_t c) const {
        const uint64_t off = (uint64_t)c * (INF_CHUNK_WORDS * 4) + (uint64_t)lane_id() * 16;
        u32x4_t v = {0u, 0u, 0u, 0u};
        if (off < end) {
            v = *reinterpret_cast<const u32x4_t *>(abase + off);
            if (end - off < 16) {
                const uint32_t keep = (uint32_t)(end - off);  // 1 .. 15 bytes of this lane's 16 belong to the member
                uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    const uint32_t k = keep > 4 * q ? keep - 4 * q : 0;
                    if (k < 4) w[q] = k ? (w[q] & ((1u << (8 * k)) - 1)) : 0u;
                }
                v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
            }
        }
        return v;
    }
    __device__ void start() { staged = 0; reg = load_chunk(0); }
    __device__ void advance() {
        uint32_t *slot = stage + (staged & 1u) * INF_CHUNK_WORDS + lane_id() * 4;
        *reinterpret_cast<u32x4_t *>(slot) = reg;
        ++staged;
        reg = load_chunk(staged);  // consumed a kilobyte from now
        sync();
    }
    __device__ uint32_t word(uint32_t w) {
        while ((w / INF_CHUNK_WORDS) >= staged) advance();  // w is wave-uniform and grows by one: at most one round
        return uni(stage[w & (2 * INF_CHUNK_WORDS - 1)]);
    }
    __device__ uint32_t fetch_add(uint32_t *p, uint32_t n) const { return atomicAdd(p, n); }
    __device__ void fetch_max(uint32_t *p, uint32_t v) const { atomicMax(p, v); }
    // CRC join: lane l holds slice l alone; the register of slice l + d comes from lane l + d
    __device__ uint32_t slice_down(const uint32_t *part, uint32_t, uint32_t d) const {
        const uint32_t v = (uint32_t)__shfl_down((int)part[0], d);
        return lane_id() + d < INF_CRC_SLICES ? v : 0u;
    }
};
#endif

// ---- output sides ----------------------------------------------------------------------------------------------------------------
// What the decoder does with a literal, a stored byte and a match is its output side O: room(n) -- may n more come?  reach(dist) -- is
// that far back still the stream's?  lit / put / match -- the writes (the decoder's p.sync() stand around match);  block_end(bit, final)
// -- a block is complete at that bit position: stop here?  finish() -- the status of a decode that stopped there.
// InfMemberOut: a member of known size, whole in `win` (sh.win + the destination's misalignment); a back-reference is an LDS read.
// (inflate_stream.inc has the other one: an unbounded stream of 16-bit symbols behind a ring.)
struct InfMemberOut {
    static const bool ASKS_FIRST = false;  // room() is asked for what a code produced, behind the code (true: also in front of every literal/length code)
    uint8_t *win;  // output byte k lives at win[k]
    uint32_t out_len, opos;
    __host__ __device__ bool room(uint32_t n) const { return opos + n <= out_len; }
    __host__ __device__ bool reach(uint32_t dist) const { return dist <= opos; }  // not before the member's first byte
    template <class P> __host__ __device__ void lit(P &p, uint32_t b) {
        if (p.lane() == 0) win[opos] = (uint8_t)b;
        ++opos;
    }
    template <class P> __host__ __device__ void put(P &p, uint32_t v, uint32_t n) {  // the low n <= 4 bytes of v
        for (uint32_t i = p.lane(); i < n; i += P::LANES) win[opos + i] = (uint8_t)(v >> (8 * i));
        opos += n;
    }
    // lane j copies byte j; an overlapping copy (dist < len) repeats the dist bytes in front of it
    template <class P> __host__ __device__ void match(P &p, uint32_t dist, uint32_t len) {
        const uint32_t lane = p.lane();
        uint8_t *to = win + opos;
        const uint8_t *from = to - dist;
        if (dist >= len) for (uint32_t k = lane; k < len; k += P::LANES) to[k] = from[k];
        else if (dist == 1) { const uint8_t b = from[0]; for (uint32_t k = lane; k < len; k += P::LANES) to[k] = b; }
        else for (uint32_t k = lane; k < len; k += P::LANES) to[k] = from[k % dist];
        opos += len;
    }
    __host__ __device__ bool block_end(uint64_t, bool final) { return final; }
    __host__ __device__ int finish() const { return opos == out_len ? INF_OK : INF_E_SHORT; }
};

// ---- the decoder -----------------------------------------------------------------------------------------------------------------
template <class P, class O = InfMemberOut> struct InfDecoder {
    P &p;
    InfShared &sh;
    O &o;
    uint64_t bb = 0;      // bit buffer
    uint32_t bc = 0;      // bits in it
    uint32_t wpos = 0;    // next input word
    uint64_t bit_end;     // the member's last bit, counted like wpos * 32 - bc

    __host__ __device__ InfDecoder(P &p_, InfShared &sh_, O &o_) : p(p_), sh(sh_), o(o_), bit_end(p_.bit_end()) {
        wpos = p.first_word();
        refill(); refill();
        const uint32_t skip = (uint32_t)(p.bit_begin() - (uint64_t)p.first_word() * 32);  // 0, 8, 16 or 24 bits in front of the member
        drop(skip);
    }
    __host__ __device__ void refill() {  // at least 33 bits afterwards
        if (bc <= 32) { bb |= (uint64_t)p.word(wpos) << bc; ++wpos; bc += 32; }
    }
    __host__ __device__ uint32_t peek(uint32_t n) const { return (uint32_t)(bb & ((1ull << n) - 1)); }
    __host__ __device__ void drop(uint32_t n) { bb >>= n; bc -= n; }
    __host__ __device__ uint32_t bits(uint32_t n) { const uint32_t v = peek(n); drop(n); return v; }
    // more bits consumed than the member holds (bits behind its end read as zero, so nothing is decided by them unnoticed)
    __host__ __device__ bool over() const { return (uint64_t)wpos * 32 - bc > bit_end; }

    // Build the decode table of `n` code lengths.  Lanes take symbols: a symbol's canonical code is the first code of its length plus the
    // number of symbols of that length in front of it.
    __host__ __device__ int build(const uint8_t *lens, uint32_t n, uint32_t *tab, uint32_t root, uint32_t cap, int table) {
        const uint32_t lane = p.lane();
        uint32_t cnt[16];
#pragma unroll
        for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
        for (uint32_t base = 0; base < n; base += P::LANES) {
            const uint32_t s = base + lane, L = s < n ? lens[s] : 0;
#pragma unroll
            for (uint32_t l = 1; l < 16; ++l) cnt[l] += inf_popc64(p.ballot(L == l));
        }
        for (uint32_t i = lane; i < cap; i += P::LANES) tab[i] = 0;  // every entry invalid
        if (lane == 0) sh.alloc = 1u << root;
        int left = 1;
        uint32_t max = 0;
#pragma unroll
        for (uint32_t l = 1; l < 16; ++l) {
            left = (left << 1) - (int)cnt[l];
            if (left < 0) return INF_E_LENGTHS;  // over-subscribed
            if (cnt[l]) max = l;
        }
        p.sync();
        if (max == 0) return table == INF_T_DD ? INF_OK : INF_E_LENGTHS;     // no code at all: only a distance set may be empty
        if (left > 0 && (table == INF_T_PRE || max != 1)) return INF_E_LENGTHS;  // incomplete (zlib lets a single 1-bit code pass)
        uint32_t next[16];
        next[0] = 0; next[1] = 0;
#pragma unroll
        for (uint32_t l = 2; l < 16; ++l) next[l] = (next[l - 1] + cnt[l - 1]) << 1;
        // pass 1: codes; symbols longer than the first level leave the longest length of their first-level slot there
        const uint32_t rmask = (1u << root) - 1;
        for (uint32_t base = 0; base < n; base += P::LANES) {
            const uint32_t s = base + lane, L = s < n ? lens[s] : 0;
            uint32_t code = 0;
#pragma unroll
            for (uint32_t l = 1; l < 16; ++l) {
                const uint64_t m = p.ballot(L == l);
                if (L == l) code = next[l] + p.below(m);
                next[l] += inf_popc64(m);
            }
            if (L > root) p.fetch_max(&tab[inf_reverse(code, L) & rmask], L);
        }
        p.sync();
        // pass 2: a sub-table of 2^(longest - root) entries for every such slot
        bool bad = false;
        if (max > root)
            for (uint32_t i = lane; i <= rmask; i += P::LANES) {
                const uint32_t m = tab[i];
                if (m == 0) continue;
                const uint32_t sub = m - root, off = p.fetch_add(&sh.alloc, 1u << sub);
                if (off + (1u << sub) > cap) { bad = true; tab[i] = 0; }
                else tab[i] = inf_entry(INF_K_SUB, root, sub, off);
            }
        if (p.ballot(bad) != 0) return INF_E_LENGTHS;  // (cannot happen: the capacities are above zlib's `enough` bounds)
        p.sync();
        // pass 3: fill.  The codes are computed again (cheaper than keeping them)
        next[1] = 0;
#pragma unroll
        for (uint32_t l = 2; l < 16; ++l) next[l] = (next[l - 1] + cnt[l - 1]) << 1;
        for (uint32_t base = 0; base < n; base += P::LANES) {
            const uint32_t s = base + lane, L = s < n ? lens[s] : 0;
            uint32_t code = 0;
#pragma unroll
            for (uint32_t l = 1; l < 16; ++l) {
                const uint64_t m = p.ballot(L == l);
                if (L == l) code = next[l] + p.below(m);
                next[l] += inf_popc64(m);
            }
            if (L == 0) continue;
            const uint32_t r = inf_reverse(code, L);
            if (L <= root) {
                const uint32_t e = inf_symbol_entry(table, s, L);
                for (uint32_t i = r; i <= rmask; i += 1u << L) tab[i] = e;
            } else {
                const uint32_t link = tab[r & rmask], sub = (link >> 8) & 31, off = link >> 16;
                const uint32_t e = inf_symbol_entry(table, s, L - root);
                for (uint32_t i = r >> root; i < (1u << sub); i += 1u << (L - root)) tab[off + i] = e;
            }
        }
        p.sync();
        return INF_OK;
    }

    // one symbol of table `tab`: the entry (its code bits dropped).  The caller has refilled.
    __host__ __device__ uint32_t symbol(const uint32_t *tab, uint32_t root) {
        uint32_t e = p.uni(tab[peek(root)]);
        if (((e >> 4) & 15) == INF_K_SUB) {
            drop(root);
            e = p.uni(tab[(e >> 16) + peek((e >> 8) & 31)]);
        }
        drop(e & 15);
        return e;
    }

    __host__ __device__ int stored() {
        drop(bc & 7);  // to the byte boundary (wpos * 32 is one)
        refill();
        const uint32_t len = bits(16), nlen = bits(16);
        if (over()) return INF_E_INPUT;
        if ((len ^ nlen) != 0xFFFFu) return INF_E_HEADER;
        if (!o.room(len)) return INF_E_OVER;
        if ((bit_end - ((uint64_t)wpos * 32 - bc)) / 8 < len) return INF_E_INPUT;
        uint32_t left = len;
        while (left >= 4) {
            refill();
            o.put(p, bits(32), 4);
            left -= 4;
        }
        while (left) {
            refill();
            o.lit(p, bits(8));
            --left;
        }
        p.sync();
        return INF_OK;
    }

    __host__ __device__ int fixed_tables() {
        const uint32_t lane = p.lane();
        for (uint32_t s = lane; s < 288; s += P::LANES) sh.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
        for (uint32_t s = lane; s < 32; s += P::LANES) sh.lens[288 + s] = 5;
        p.sync();
        int rc = build(sh.lens, 288, sh.ll, INF_LL_ROOT, INF_LL_CAP, INF_T_LL);
        if (rc) return rc;
        return build(sh.lens + 288, 32, sh.dd, INF_DD_ROOT, INF_DD_CAP, INF_T_DD);
    }

    __host__ __device__ int dynamic_tables() {
        const uint32_t lane = p.lane();
        refill();
        const uint32_t hlit = bits(5) + 257, hdist = bits(5) + 1, hclen = bits(4) + 4;
        if (over()) return INF_E_INPUT;
        if (hlit > 286 || hdist > 30) return INF_E_LENGTHS;
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        for (uint32_t i = lane; i < 19; i += P::LANES) sh.plens[i] = 0;
        p.sync();
        for (uint32_t i = 0; i < hclen; ++i) {
            refill();
            const uint32_t v = bits(3);
            if (lane == 0) sh.plens[order[i]] = (uint8_t)v;
        }
        if (over()) return INF_E_INPUT;
        p.sync();
        int rc = build(sh.plens, 19, sh.pre, INF_PRE_ROOT, INF_PRE_CAP, INF_T_PRE);
        if (rc) return rc;
        const uint32_t total = hlit + hdist;
        uint32_t i = 0, prev = 0;
        while (i < total) {
            refill();
            const uint32_t e = symbol(sh.pre, INF_PRE_ROOT);
            if (((e >> 4) & 15) != INF_K_LIT) return over() ? INF_E_INPUT : INF_E_LENGTHS;
            const uint32_t s = e >> 16;
            uint32_t rep = 1, val = s;
            if (s == 16) { if (i == 0) return over() ? INF_E_INPUT : INF_E_LENGTHS; val = prev; rep = 3 + bits(2); }
            else if (s == 17) { val = 0; rep = 3 + bits(3); }
            else if (s == 18) { val = 0; rep = 11 + bits(7); }
            if (over()) return INF_E_INPUT;
            if (i + rep > total) return INF_E_LENGTHS;
            if (lane == 0) for (uint32_t k = 0; k < rep; ++k) sh.lens[i + k] = (uint8_t)val;
            i += rep; prev = val;
        }
        p.sync();
        if (p.uni(sh.lens[256]) == 0) return INF_E_LENGTHS;  // no end-of-block code
        rc = build(sh.lens, hlit, sh.ll, INF_LL_ROOT, INF_LL_CAP, INF_T_LL);
        if (rc) return rc;
        return build(sh.lens + hlit, hdist, sh.dd, INF_DD_ROOT, INF_DD_CAP, INF_T_DD);
    }

    __host__ __device__ int symbols() {
        for (;;) {
            if (O::ASKS_FIRST && !o.room(1)) return INF_E_OVER;  // (a compile-time constant: only the search's side stops in front of a code)
            refill();
            const uint32_t e = symbol(sh.ll, INF_LL_ROOT);
            const uint32_t kind = (e >> 4) & 15;
            if (over()) return INF_E_INPUT;
            if (kind == INF_K_LIT) {
                if (!o.room(1)) return INF_E_OVER;
                o.lit(p, e >> 16);
                continue;
            }
            if (kind == INF_K_EOB) return INF_OK;
            if (kind != INF_K_LEN) return INF_E_SYMBOL;
            const uint32_t len = (e >> 16) + bits((e >> 8) & 31);
            refill();
            const uint32_t d = symbol(sh.dd, INF_DD_ROOT);
            if (((d >> 4) & 15) != INF_K_LEN) return over() ? INF_E_INPUT : INF_E_SYMBOL;
            const uint32_t dist = (d >> 16) + bits((d >> 8) & 31);
            if (over()) return INF_E_INPUT;
            if (!o.reach(dist)) return INF_E_SYMBOL;  // reaches before the member's first byte
            if (!o.room(len)) return INF_E_OVER;
            p.sync();  // the literals written so far are visible to every lane
            o.match(p, dist, len);
            p.sync();
        }
    }

    // the header of the block that starts here and nothing of its data: the three bits, a stored block's LEN / NLEN behind the byte
    // boundary, a dynamic block's code sets (inflate_search.inc: what follows an end-of-block must be a block again)
    __host__ __device__ int header_only() {
        refill();
        const uint32_t hdr = bits(3);
        if (over()) return INF_E_INPUT;
        const uint32_t type = hdr >> 1;
        if (type == 1) return INF_OK;
        if (type == 2) return dynamic_tables();
        if (type == 3) return INF_E_HEADER;
        drop(bc & 7);
        refill();
        const uint32_t len = bits(16), nlen = bits(16);
        if (over()) return INF_E_INPUT;
        return (len ^ nlen) != 0xFFFFu ? INF_E_HEADER : INF_OK;
    }

    __host__ __device__ int run() {
        for (;;) {
            refill();
            const uint32_t hdr = bits(3);
            if (over()) return INF_E_INPUT;
            const uint32_t type = hdr >> 1;
            int rc;
            if (type == 0) rc = stored();
            else if (type == 3) return INF_E_HEADER;
            else {
                rc = type == 1 ? fixed_tables() : dynamic_tables();
                if (rc == INF_OK) rc = symbols();
            }
            if (rc) return rc;
            if (o.block_end((uint64_t)wpos * 32 - bc, (hdr & 1) != 0)) break;
        }
        return o.finish();
    }
};

// ---- CRC-32 of a decoded member ----------------------------------------------------------------------------------------------------
// a * b modulo the polynomial, both reflected (bit 31 is x^0, so 0x80000000 is 1): what zlib's crc32_combine multiplies with
__host__ __device__ static inline uint32_t inf_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32; ++i) {
        p ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = (b >> 1) ^ (INF_CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}
// x^(8 n) modulo the polynomial: what n zero bytes do to a register
__host__ __device__ static inline uint32_t inf_crc_shift(uint32_t n) {
    uint32_t r = 0x80000000u, sq = 0x00800000u;  // 1, x^8
    for (; n; n >>= 1) {
        if (n & 1u) r = inf_crc_mul(r, sq);
        sq = inf_crc_mul(sq, sq);
    }
    return r;
}
// the register after window bytes [a, e), slice-by-4: bytes up to a 4-byte boundary of the window, whole words (both targets are
// little-endian), the rest.  tab[j * 256 + v] is what byte v does to the register j + 1 bytes later.
__host__ __device__ static inline uint32_t inf_crc_slice(const uint32_t *tab, const uint8_t *win, uint32_t a, uint32_t e, uint32_t reg) {
    for (; a < e && (a & 3u); ++a) reg = tab[(reg ^ win[a]) & 255u] ^ (reg >> 8);
    for (; a + 4 <= e; a += 4) {
        uint32_t w;
        __builtin_memcpy(&w, __builtin_assume_aligned(win + a, 4), 4);
        reg ^= w;
        reg = tab[768 + (reg & 255u)] ^ tab[512 + ((reg >> 8) & 255u)] ^ tab[256 + ((reg >> 16) & 255u)] ^ tab[reg >> 24];
    }
    for (; a < e; ++a) reg = tab[(reg ^ win[a]) & 255u] ^ (reg >> 8);
    return reg;
}
// zlib's crc32(0, data, n) of output bytes [0, n), which live at win[wmis ..).  Overwrites `ll`: the decode has ended.  Wave-uniform result.
// inf_crc32_at is the same over any byte array `win` with 1 024 words of scratch `tab` (deflate_members.inc: the input piece in LDS).
template <class P> __host__ __device__ static uint32_t inf_crc32_at(P &p, uint32_t *tab, const uint8_t *win, uint32_t wmis, uint32_t n) {
    if (n == 0) return 0;
    const uint32_t lane = p.lane();
    for (uint32_t v = lane; v < 256; v += P::LANES) {
        uint32_t c = v;
        for (uint32_t k = 0; k < 8; ++k) c = (c >> 1) ^ (INF_CRC_POLY & (0u - (c & 1u)));
        tab[v] = c;
    }
    p.sync();
    for (uint32_t v = lane; v < 256; v += P::LANES) {
        uint32_t c = tab[v];
        for (uint32_t j = 1; j < 4; ++j) { c = tab[c & 255u] ^ (c >> 8); tab[j * 256 + v] = c; }
    }
    p.sync();
    // slice s covers output positions [s S - pad, (s + 1) S - pad), cut at 0; the one that holds position 0 starts from gzip's register of ones
    const uint32_t S = (n + INF_CRC_SLICES - 1) / INF_CRC_SLICES, pad = INF_CRC_SLICES * S - n;
    uint32_t part[INF_CRC_SLICES / P::LANES];
    for (uint32_t k = 0; k < INF_CRC_SLICES / P::LANES; ++k) {
        const uint32_t s = k * P::LANES + lane, end = (s + 1) * S;
        const uint32_t a = s * S > pad ? s * S - pad : 0, e = end > pad ? end - pad : 0;
        part[k] = e ? inf_crc_slice(tab, win, wmis + a, wmis + e, s * S <= pad ? 0xFFFFFFFFu : 0u) : 0u;
    }
    uint32_t mult = inf_crc_shift(S);  // x^(8 S 2^r) in round r
    for (uint32_t r = 0; r < 6; ++r) {
        for (uint32_t k = 0; k < INF_CRC_SLICES / P::LANES; ++k) part[k] = inf_crc_mul(part[k], mult) ^ p.slice_down(part, k, 1u << r);
        mult = inf_crc_mul(mult, mult);
    }
    return ~p.uni(part[0]);
}
template <class P> __host__ __device__ static uint32_t inf_crc32(P &p, InfShared &sh, uint32_t wmis, uint32_t n) {
    return inf_crc32_at(p, sh.ll, sh.win, wmis, n);  // 4 x 256 words of its 2 048
}

// host entry: one member, `sh` is the caller's scratch; writes min(produced, out_len) bytes; *crc (if asked for) is set where the status is 0
static int inf_member_host(InfShared &sh, const uint8_t *in, uint64_t in_len, uint8_t *out, uint32_t out_len, uint32_t *crc = nullptr) {
    InfHostPolicy pol{in, in_len};
    InfMemberOut o{sh.win, out_len, 0};
    InfDecoder<InfHostPolicy> d(pol, sh, o);
    const int st = d.run();
    if (o.opos) std::memcpy(out, sh.win, std::min(o.opos, out_len));
    if (crc && st == INF_OK) *crc = inf_crc32(pol, sh, 0, out_len);
    return st;
}

#ifdef __HIPCC__
// ---- kernel ----------------------------------------------------------------------------------------------------------------------
struct InflateArgs {
    const uint8_t *in;          // packed members, INF_PAD bytes of padding in front and behind
    const uint64_t *in_off;     // [n] from `in`
    const uint32_t *in_len;
    uint8_t *out;               // packed outputs
    const uint64_t *out_off;
    const uint32_t *out_len;    // <= INF_MAX_OUT (checked on the host)
    uint32_t *status;
    uint32_t *cursor;
    uint32_t n;
    const uint32_t *expected;   // CRC kernel only: [n] or NULL
    uint32_t *crc;              // CRC kernel only: [n]
};

// CRC = false is the plain decode; CRC = true also takes the member's CRC-32 from the window and compares it with `expected`
template <bool CRC> __global__ void __launch_bounds__(WAVE) k_inflate_members(InflateArgs a) {
    __shared__ InfShared sh;
    const uint32_t lane = lane_id();
    for (;;) {
        uint32_t m = 0;
        if (lane == 0) m = atomicAdd(a.cursor, 1u);
        m = (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
        if (m >= a.n) break;
        const uint8_t *src = a.in + a.in_off[m];
        uint8_t *dst = a.out + a.out_off[m];
        const uint32_t out_len = min(a.out_len[m], INF_MAX_OUT);
        const uint32_t wmis = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15);
        InfWavePolicy pol;
        const uint64_t mis = reinterpret_cast<uintptr_t>(src) & 15;
        pol.abase = src - mis; pol.begin = mis; pol.end = mis + a.in_len[m]; pol.stage = sh.stage;
        pol.start();
        int st;
        uint32_t produced;
        {
            InfMemberOut o{sh.win + wmis, out_len, 0};
            InfDecoder<InfWavePolicy> d(pol, sh, o);
            st = d.run();
            produced = min(o.opos, out_len);
        }
        pol.sync();
        if (CRC && st == INF_OK) {  // (wave-uniform) only a member that decoded completely has a CRC
            const uint32_t crc = inf_crc32(pol, sh, wmis, produced);
            if (a.expected && crc != a.expected[m]) st = CHN_INFLATE_E_CRC;
            if (lane == 0) a.crc[m] = crc;
        }
        // write the window out: whole 16-byte pieces as one vector store per lane, the ragged ends byte by byte
        uint8_t *abase = dst - wmis;
        const uint32_t lo = wmis, hi = wmis + produced;  // window bytes [lo, hi)
        for (uint32_t b = lane * 16; b < hi; b += WAVE * 16) {
            if (b >= lo && b + 16 <= hi) *reinterpret_cast<u32x4_t *>(abase + b) = *reinterpret_cast<const u32x4_t *>(sh.win + b);
            else for (uint32_t i = b > lo ? b : lo; i < b + 16 && i < hi; ++i) abase[i] = sh.win[i];
        }
        if (lane == 0) a.status[m] = (uint32_t)st;
        pol.sync();  // the window and the tables are the next member's from here
    }
}
#endif
