// gzip_walk.inc -- the deflate_slow walk that k_gzip_tally (gzip_tally.inc) and k_gzip_long (gzip_tally_long.inc) both instantiate
// Part of the single translation unit charon_hip.hip (included in order, behind gzip_trees.inc and before gzip_tally.inc); not a stand-alone source.

// ------------------------------------------------------------------------------------------------
// One wavefront restates zlib's level-6 deflate_slow for one read (the scheme is described at the head of gzip_tally.inc).  What the
// two kernels do alike lives here, once: the packed codes and how they are read, the trigram classes as arrays, the wave-parallel
// longest_match, the tally of a step's symbol, the tallies' way into LDS.  Everything is force-inlined and templated on BITS (4 = dna5
// codes with 0xF behind the data, 2 = a batch without N); where the kernels differ they pass a value or a code store (flat / ring).
// What differs for good reason stays in the kernels: where the candidates come from, NIL and the window's limit, what a step's best
// candidate decodes to, blocks and output.
// ------------------------------------------------------------------------------------------------
template <int BITS>
struct GzCodes {
    static constexpr uint32_t CPW = 32 / BITS, LOGC = BITS == 4 ? 3 : 4, CMASK = (1u << BITS) - 1u;  // codes per word
    static constexpr uint32_t FIRST = CPW;                // codes the first comparison covers behind the trigram
    static constexpr uint32_t CSH = BITS == 4 ? 2 : 1;    // bit index -> code index
    static constexpr uint32_t PAD = BITS == 4 ? 0xFu : 0u;  // the code behind the data
};

// wave-wide unsigned max by DPP (row shifts inside the rows of 16, then the two row broadcasts of GFX9): no LDS traffic, result uniform
__device__ __forceinline__ uint32_t gz_wave_umax(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));  // row_shr:1
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));  // row_shr:2
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));  // row_shr:4
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));  // row_shr:8  -> lane 15 of a row holds the row's max
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));  // row_bcast:15 into rows 1 and 3
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));  // row_bcast:31 into rows 2 and 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

template <int BITS>
__device__ __forceinline__ uint32_t gz_key_of(uint32_t v) {  // the trigram's class: 125 of them with N, 64 without
    return BITS == 4 ? (v & 15u) * 25u + ((v >> 4) & 15u) * 5u + ((v >> 8) & 15u) : v & 63u;
}
// the tallies' word (= the letter) of the literal lane c counts: A C G T N
__device__ __forceinline__ uint32_t gz_letter_of(uint32_t c) { return c == 0 ? 65u : c == 1 ? 67u : c == 2 ? 71u : c == 3 ? 84u : 78u; }

// a read's segments against the batch, as k_minimise_probe checks them (a device batch is not checked by the host)
__device__ __forceinline__ bool gz_segments_outside(const uint64_t *off1, const uint64_t *off2, uint32_t l1, uint32_t l2, uint64_t n_bases, uint32_t r) {
    const uint64_t o1 = off1[r], o2 = off2 ? off2[r] : 0;
    return (o1 & 63u) || o1 > n_bases || l1 > n_bases - o1 || (off2 && ((o2 & 63u) || o2 > n_bases || l2 > n_bases - o2));
}

// the word of codes at word index gw of a read (mate 1 of l1 letters, then mate 2; n letters in all), from the batch's packed bases and
// N masks; PAD behind the data
template <int BITS>
__device__ __forceinline__ uint32_t gz_pack_codes(uint32_t gw, const uint32_t *b1, const uint32_t *b2, const uint32_t *m1, const uint32_t *m2, uint32_t l1, uint32_t n) {
    using C = GzCodes<BITS>;
    uint32_t word = 0;
    for (uint32_t j = 0; j < C::CPW; ++j) {
        const uint32_t p = gw * C::CPW + j;
        uint32_t c = C::PAD;
        if (p < n) {
            const bool second = p >= l1;
            const uint32_t q = second ? p - l1 : p;
            const uint32_t *bw = second ? b2 : b1, *mw = second ? m2 : m1;
            c = (bw[q >> 4] >> ((q & 15u) * 2)) & 3u;
            if (BITS == 4 && mw && ((mw[q >> 5] >> (q & 31u)) & 1u)) c = 4;
        }
        word |= c << (BITS * j);
    }
    return word;
}

// Where the codes lie in LDS: the word index of position p -- the whole read from word 0 on, or a ring of RMASK + 1 words
template <int BITS>
struct GzFlatStore {
    static __device__ __forceinline__ uint32_t word(uint32_t p) { return p >> GzCodes<BITS>::LOGC; }
};
template <int BITS, uint32_t RMASK>
struct GzRingStore {
    static __device__ __forceinline__ uint32_t word(uint32_t p) { return (p >> GzCodes<BITS>::LOGC) & RMASK; }
};
__device__ __forceinline__ uint32_t gz_lds_u32(uint32_t byte_addr) { return *(const __attribute__((address_space(3))) uint32_t *)(size_t)byte_addr; }
template <int BITS, class STORE>
struct GzCodeReader {
    const uint32_t *words;  // the store in LDS
    uint32_t csb;           // its LDS byte address, for the walk (pin_base)
    // the codes starting at position p, one word of them (position p in the low bits)
    __device__ __forceinline__ uint32_t get8(uint32_t p) const {
        const uint32_t w = STORE::word(p);
        return (uint32_t)__builtin_amdgcn_alignbit(words[w + 1], words[w], p * BITS);
    }
    // before the walk: the base address in a vector register the compiler knows nothing about (it would re-derive it as two additions per use)
    __device__ __forceinline__ void pin_base() {
        csb = (uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t *)words;
        asm volatile("" : "+v"(csb));
    }
    __device__ __forceinline__ uint32_t word_addr(uint32_t p) const {  // LDS address of the word holding code p: one shift (and the ring's mask), one shift-add
        uint32_t w = STORE::word(p);
        asm("" : "+v"(w));
        return (w << 2) + csb;
    }
    __device__ __forceinline__ uint32_t codes8(uint32_t p) const {  // get8 with two vector instructions of address arithmetic
        const uint32_t ad = word_addr(p);
        return (uint32_t)__builtin_amdgcn_alignbit(gz_lds_u32(ad + 4), gz_lds_u32(ad), p * BITS);
    }
    // the codes at the walk's position (Sv: S, per lane), three words from one address
    __device__ __forceinline__ void fetch(uint32_t Sv, uint32_t &here, uint32_t &next8) const {
        const uint32_t cwa = word_addr(Sv), sh = Sv * BITS;
        const uint32_t w0 = gz_lds_u32(cwa), w1 = gz_lds_u32(cwa + 4), w2 = gz_lds_u32(cwa + 8);
        here = (uint32_t)__builtin_amdgcn_alignbit(w1, w0, sh);                      // codes S .. S + 7
        const uint32_t mid = (uint32_t)__builtin_amdgcn_alignbit(w2, w1, sh);        // codes S + 8 .. S + 15
        next8 = (uint32_t)__builtin_amdgcn_alignbit(mid, here, 3 * BITS);            // codes S + 3 onwards, a word of them
    }
};

// The class arrays of positions [P0, P1) (at most 65 536 of them; their trigrams are in the store): class sizes -> class starts ->
// every position p into occ[] (positions by class, as p - P0, ascending inside a class) and pinfo[p - P0] = slot | rank inside the
// class << 16.  ccur[128] (zero on entry; the class ends on return) and cst[128] (the class starts on return) are in LDS.
template <int BITS, class CODES>
__device__ __forceinline__ void gz_build_classes(const CODES &codes, uint32_t lane, uint32_t P0, uint32_t P1, uint16_t *occ, uint32_t *pinfo, uint32_t *ccur, uint32_t *cst) {
    for (uint32_t p = P0 + lane; p < P1; p += WAVE) atomicAdd(&ccur[gz_key_of<BITS>(codes.get8(p))], 1u);
    __syncthreads();
    {   // exclusive scan over the classes: two per lane, once per build (no class beyond 124: slots 125 .. 127 hold zeros and get the total)
        const uint32_t k0 = lane * 2, c0 = ccur[k0], c1 = ccur[k0 + 1];
        uint32_t incl = c0 + c1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, o); if (lane >= (uint32_t)o) incl += t; }
        const uint32_t ex = incl - (c0 + c1);
        ccur[k0] = ex; cst[k0] = ex;
        ccur[k0 + 1] = ex + c0; cst[k0 + 1] = ex + c0;
    }
    __syncthreads();
    // positions into their classes, in position order: per tile of 64 positions every lane finds the lanes holding the same trigram
    // (seven ballots, one per key bit), its rank among them, and the class's lowest lane moves the cursor on
    for (uint32_t p0 = P0; p0 < P1; p0 += WAVE) {
        const uint32_t p = p0 + lane;
        const bool valid = p < P1;
        const uint32_t k = valid ? gz_key_of<BITS>(codes.get8(p)) : 127u;  // 127: no class
        uint64_t same = ~0ULL;
#pragma unroll
        for (uint32_t bit = 0; bit < 7; ++bit) {
            const uint64_t bm = __ballot((k >> bit) & 1u);
            same &= ((k >> bit) & 1u) ? bm : ~bm;
        }
        const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u));
        if (valid) {
            const uint32_t before = ccur[k], slot = before + rk;
            occ[slot] = (uint16_t)(p - P0);
            pinfo[p - P0] = slot | ((slot - cst[k]) << 16);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every lane of the class has read the cursor before its lowest lane moves it
            if (rk == 0) ccur[k] = before + (uint32_t)__popcll(same);
        }
    }
    // occ[] and pinfo[] are read back by this wavefront only: its stores went through the CU's vector cache (write-through, shared by the CU's
    // wavefronts, so coherent for them) and the barrier below waits for them.  A device-scope fence here (round 2 had one) writes the XCD's
    // whole L2 back to memory and empties the vector cache, per read: a third of the kernel's time on 5 kb reads.
    __syncthreads();
}

// longest_match at position S, by the whole wavefront: lane j holds the j-th most recent same-trigram candidate in curA (okA: it is in
// the window) and, with more than 64 of the kk candidates looked at, the (64 + j)-th in curB / okB.  Returns the wave's maximum over
// (length - 3) << 16 | pack: packA / packB say which candidate it was, the more recent the larger (16 bits), so that the most recent
// candidate of maximal length wins; 0: none.  next8: the codes from S + 3 on; PL: prev_length; look: the lookahead.
// The common case -- no candidate agrees beyond the first comparison's FIRST letters, the read is not about to end, nothing is out of
// the window -- is decided by ONE max-reduction; the reduction's own result says whether it was the common case (a length of 3 + FIRST:
// some candidate may go on), and only then, or when the caller says so (force_general: nice_match = lookahead within reach of the
// first comparison, candidates beyond the window), the general rule is evaluated: longer comparisons, the walk ending at the first
// candidate of nice_match.
template <int BITS, class CODES>
__device__ __forceinline__ uint32_t gz_longest_match(const CODES &codes, uint32_t lane, uint32_t S, uint32_t next8, uint32_t curA, uint32_t curB, uint32_t packA,
                                                     uint32_t packB, bool okA, bool okB, uint32_t kk, uint32_t PL, uint32_t look, bool force_general) {
    constexpr uint32_t FIRST = GzCodes<BITS>::FIRST, CSH = GzCodes<BITS>::CSH, MAX_MATCH = gztrees::MAX_MATCH;
    // common prefix: same class = same trigram, then a word of codes at once (the 0xF behind the data ends every match at n).
    // (lanes without a candidate read position 3 onwards: in range, ignored)
    const uint32_t xa = next8 ^ codes.codes8(curA + 3u);
    const uint32_t qa = (xa ? (uint32_t)__builtin_ctz(xa) : 32u) >> CSH;  // agreeing codes behind the trigram, at most FIRST
    uint32_t v = okA ? (qa << 16) | packA : 0u;
    if (kk > 64u) {
        const uint32_t xb = next8 ^ codes.codes8(curB + 3u);
        const uint32_t qb = (xb ? (uint32_t)__builtin_ctz(xb) : 32u) >> CSH;
        v = max(v, okB ? (qb << 16) | packB : 0u);
    }
    uint32_t mx = gz_wave_umax(v);
    if (mx >= (FIRST << 16) || force_general) {
        asm volatile("" ::: "memory");  // (a branch, not selects: one step in some hundreds comes here)
        const uint32_t xb = kk > 64u ? next8 ^ codes.codes8(curB + 3u) : 1u;
        // the general rule.  Further codes a word at a time while some candidate still agrees: those lanes all stand at the same
        // length, so the current string's codes are one uniform read per step
        uint32_t lenA = 3u + qa, lenB = 3u + ((xb ? (uint32_t)__builtin_ctz(xb) : 32u) >> CSH);
        bool goA = okA && xa == 0, goB = okB && xb == 0;
        uint32_t at = 3u + FIRST;
        while (at < MAX_MATCH && __builtin_amdgcn_ballot_w64(goA || goB)) {
            const uint32_t mine = codes.codes8(S + at);
            if (goA) {
                const uint32_t y = mine ^ codes.codes8(curA + at);
                lenA = at + ((y ? (uint32_t)__builtin_ctz(y) : 32u) >> CSH);
                goA = y == 0;
            }
            if (goB) {
                const uint32_t y = mine ^ codes.codes8(curB + at);
                lenB = at + ((y ? (uint32_t)__builtin_ctz(y) : 32u) >> CSH);
                goB = y == 0;
            }
            at += FIRST;
        }
        lenA = min(lenA, MAX_MATCH); lenB = min(lenB, MAX_MATCH);
        if (BITS == 2) { lenA = min(lenA, look); lenB = min(lenB, look); }  // no 0xF behind the data: the match ends at n all the same
        // the walk ends behind the first candidate reaching T (nice_match, and above prev_length), at the first candidate outside
        // the window, or when the chain runs out; the most recent candidate of maximal length wins
        const uint32_t nice = look < 128u ? look : 128u;
        const uint32_t T = nice > PL + 1 ? nice : PL + 1;
        v = okA ? ((lenA - 3u) << 16) | packA : 0u;
        const uint64_t stopA = __builtin_amdgcn_ballot_w64(okA && lenA >= T);
        if (stopA) { if (lane > (uint32_t)__builtin_ctzll(stopA)) v = 0; }
        else if (kk > 64u && __builtin_amdgcn_ballot_w64(okA) == ~0ULL) {  // the chain went on through all of the first 64
            uint32_t vb = okB ? ((lenB - 3u) << 16) | packB : 0u;
            const uint64_t stopB = __builtin_amdgcn_ballot_w64(okB && lenB >= T);
            if (stopB) { if (lane > (uint32_t)__builtin_ctzll(stopB)) vb = 0; }
            v = max(v, vb);
        }
        mx = gz_wave_umax(v);
    }
    return mx;
}

// The symbol tallies of a block, in registers: lane c counts the literals of code c, lane j the matches of length j + 3 (lengths from
// 67 on: at once into tall[], by gz_emit), lane d the matches of distance code d
struct GzTallies {
    uint32_t lit_cnt, len_cnt, dist_cnt;
    uint32_t code_prev;  // the literal waiting for the lazy evaluation (255: none -- match_available is false)
};
enum { GZ_NOTHING = 0, GZ_LITERAL = 1, GZ_MATCH = 2, GZ_LONG_MATCH = 3 };  // what gz_emit tallied (GZ_LONG_MATCH: a match of 67 letters and more)
// The end of a deflate_slow step at S (= Sv per lane; `here`: the codes at S), with this step's match length in ML and the previous
// step's in PL / PM (prev_length, prev_match): either the previous position's match is emitted and the walk moves behind it, or the
// waiting literal is, if there is one, and the walk moves one on.  (INSERT_STRING: nothing to do -- the class arrays hold every position.)
template <int BITS>
__device__ __forceinline__ uint32_t gz_emit(GzTallies &t, uint32_t *tall, uint32_t lane, uint32_t PL, uint32_t PM, uint32_t here, uint32_t &S, uint32_t &Sv, uint32_t &ML) {
    if (PL >= gztrees::MIN_MATCH && ML <= PL) {
        // length PL, distance S - 1 - PM (tally_dist counts dist - 1)
        const uint32_t lc = PL - gztrees::MIN_MATCH;
        uint32_t kind = GZ_MATCH;
        t.len_cnt += lane == lc ? 1u : 0u;
        if (lc >= 64u) {
            asm volatile("" ::: "memory");
            kind = GZ_LONG_MATCH;
            if (lane == 0) atomicAdd(&tall[257 + gztrees::length_code(lc)], 1u);
        }
        // d_code(d): the exponent and the first mantissa bit of d as a float (exact below 2^24), d itself below 2
        const uint32_t d = Sv - (PM + 2u);
        const uint32_t dc = d < 2u ? d : (__float_as_uint((float)d) >> 22) - 254u;
        t.dist_cnt += lane == dc ? 1u : 0u;
        S += PL - 1; Sv += PL - 1;
        t.code_prev = 255;
        ML = gztrees::MIN_MATCH - 1;
        return kind;
    }
    const uint32_t kind = t.code_prev != 255u ? GZ_LITERAL : GZ_NOTHING;
    t.lit_cnt += lane == t.code_prev ? 1u : 0u;  // the waiting literal, if there is one (no lane is 255)
    t.code_prev = here & GzCodes<BITS>::CMASK;
    S++; Sv++;
    return kind;
}
// the register tallies into a block's record in LDS: tall[0, 286) literal/length frequencies, tall[286, 316) distance frequencies
__device__ __forceinline__ void gz_store_tallies(const GzTallies &t, uint32_t *tall, uint32_t lane) {
    if (lane < 5) tall[gz_letter_of(lane)] = t.lit_cnt;
    if (t.len_cnt) atomicAdd(&tall[257 + gztrees::length_code(lane)], t.len_cnt);
    if (lane < 30) tall[286 + lane] = t.dist_cnt;
}
