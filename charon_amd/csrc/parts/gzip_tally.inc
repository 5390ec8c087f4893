// gzip_tally.inc -- k_gzip_tally: zlib level-6 deflate_slow of every read of a batch, as symbol TALLIES (SURVEY 8(f) item 3)
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.

// ------------------------------------------------------------------------------------------------
// The `compression` column (get_compression_ratio, src/utils.cpp:114-124) needs the exact SIZE of the gzip member zlib would write
// for the read's letters.  The size is a function of the literal/length and distance code FREQUENCIES of the deflate block
// (_tr_flush_block builds the Huffman trees from them); the frequencies come out of deflate_slow's lazy-match decisions, which are
// sequential per read.  One wavefront works on one read at a time (a launch is as many wavefronts as the device holds at once; each
// takes the next read from a counter until none is left):
//   1. the read's dna5 codes into LDS (4 bits each); the 125 trigram classes (= zlib's 15-bit hash classes for DNA letters, checked
//      on the host) are counted and every position p gets its slot in the positions-by-class array occ[] (= zlib's hash chains as
//      arrays, ascending inside a class) and its info word pinfo[p] = slot | rank inside the class << 16.  deflate_slow enters EVERY
//      position up to n - 3 into the dictionary, in position order, exactly once (INSERT_STRING at strstart, and the positions inside
//      an emitted match), so when the walk stands at position p the chain of its trigram is simply the rank(p) entries below slot(p):
//      no cursor has to be moved while deflate runs.  occ[] and pinfo[] live in global memory (6 bytes per letter and wavefront; LDS
//      holds only the codes, half a byte per letter, so a CU keeps its full 32 wavefronts up to ~9 000 letters);
//   2. deflate_slow runs with wave-uniform control flow; each longest_match is evaluated by the whole wavefront: lane j takes the
//      j-th most recent same-trigram candidate and measures its common prefix; one max-reduction over (length << 16 | position)
//      reproduces the sequential rule exactly (the most recent candidate of maximal length above prev_length wins; the first
//      candidate reaching nice_match ends the walk; max_chain 128, a quarter of it after a good match; MAX_DIST; TOO_FAR).  The
//      symbol tallies are kept in registers: lane c counts the literals of code c, lane j the matches of length j + 3, lane d the
//      matches of distance code d;
//   3. the tallies (286 literal/length + 30 distance frequencies) leave as 16-bit words; the host turns them into the block size
//      with the same _tr_flush_block restatement it uses for its own emulator (charon_amd/csrc/host/gzip_size.hpp) -- a few
//      microseconds per read instead of ~70 -- or k_gzip_size does on the device.
// Scope: A/C/G/T/N letters, 1 <= n <= GZT_MAX_LEN, one deflate block (fewer than 16 383 symbols), no window slide
// (n < 65 274 is implied).  Anything else is flagged and sized on the host.  Exactness is established against the host
// emulator (itself checked against zlib on millions of inputs): tests/test_gpu_parity.py::test_gzip_tallies_equal_the_host_emulator.
// ------------------------------------------------------------------------------------------------
#define GZT_MAX_LEN 61440u  // half a byte of LDS per letter: five wavefronts per CU at this length (and below 65 274, where zlib's window starts to slide)
#define GZT_WORDS 320u      // per read: [0, 286) literal/length freqs, [286, 316) distance freqs, [316] status (0 ok, 1 = size on the host), pad
#define GZT_WIN 64u         // info words fetched at once (one per lane)
#ifndef GZT_SYMBOL_LIMIT
#define GZT_SYMBOL_LIMIT 16383u  // lit_bufsize - 1: a block is flushed when it holds this many symbols (a DIAGNOSTICS build may lower it to test the hand-back)
#endif
#ifndef GZT_WAVES_PER_CU
#define GZT_WAVES_PER_CU 32u  // wavefronts a launch puts on a CU at most (LDS permitting)
#endif
struct GztArgs {
    const uint32_t *bases, *nmask;
    const uint64_t *off1, *off2;
    const uint32_t *len1, *len2;
    uint32_t n_reads, max_len;   // LDS and the scratch stride are sized for max_len
    uint64_t n_bases;            // size of `bases` in letters (a device batch is not checked by the host: a segment outside it is not tallied)
    const uint32_t *index;       // reads of this launch (an occupancy class), or null = reads 0 .. count - 1
    uint32_t count;              // reads of this launch
    uint16_t *out;               // [n_reads of the batch][GZT_WORDS]
    uint32_t *scratch;           // [blocks][stride32]: per wavefront pinfo[cap + GZT_WIN] (32 bits each), then occ[cap] (16 bits each), cap = max_len rounded up to 8
    uint32_t stride32;
    uint32_t *counter;           // next read of the launch (zero when the launch starts)
};
__device__ __constant__ uint8_t c_gz_extra_lbits[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};

__device__ __forceinline__ uint32_t gz_length_code(uint32_t lc) {  // _length_code[lc], lc = match length - 3 (trees.c tr_static_init)
    if (lc == 255) return 28;
    if (lc < 8) return lc;
    const uint32_t hb = 31u - (uint32_t)__clz((int)lc);  // lc in [2^hb, 2^(hb+1)); 4 codes per power of two from 8 on
    return (hb - 1) * 4 + ((lc >> (hb - 2)) & 3u);
}
__device__ __forceinline__ uint32_t gz_dist_code(uint32_t d) {  // d_code(dist), dist = match distance - 1
    if (d < 4) return d;
    const uint32_t hb = 31u - (uint32_t)__clz((int)d);
    return hb * 2 + ((d >> (hb - 1)) & 1u);
}

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

// BITS: 4 = dna5 codes (A C G T N) with 0xF behind the data; 2 = a batch without N: the codes as they are packed in the batch, sixteen to a word --
// half the LDS (twice the wavefronts on a CU for reads beyond 9 000 letters) and sixteen letters per comparison; nothing marks the end of
// the data, so the general rule cuts every candidate's length at the lookahead (zlib compares against the zeroed window behind the data: a
// mismatch at n, whatever the candidate holds there).
template <int BITS>
__global__ __launch_bounds__(WAVE) void k_gzip_tally(const GztArgs a) {
    constexpr uint32_t CPW = 32 / BITS, LOGC = BITS == 4 ? 3 : 4, CMASK = (1u << BITS) - 1u;  // codes per word
    constexpr uint32_t FIRST = CPW;  // codes the first comparison covers behind the trigram
    constexpr uint32_t CSH = BITS == 4 ? 2 : 1;  // bit index -> code index
    extern __shared__ __align__(16) unsigned char gsm[];
    const uint32_t lane = lane_id();
    // LDS (sized for max_len on the host): 1 280 bytes + half a byte per letter
    uint32_t *tall = reinterpret_cast<uint32_t *>(gsm);  // [320] the tallies as they leave; while the classes are built: class cursors [0, 128), class starts [128, 256)
    uint32_t *ccnt = tall, *cstart = tall + 128;
    uint32_t *cs4 = tall + GZT_WORDS;                    // the codes, BITS each (4: 0xF behind the data; 2: zeros)
    const uint32_t cap = (a.max_len + 7u) & ~7u;
    uint32_t *pinfo = a.scratch + (size_t)blockIdx.x * a.stride32;
    uint16_t *occ = reinterpret_cast<uint16_t *>(pinfo + cap + GZT_WIN);
    for (;;) {
        uint32_t item = 0;
        if (lane == 0) item = atomicAdd(a.counter, 1u);
        item = (uint32_t)__builtin_amdgcn_readfirstlane((int)item);
        if (item >= a.count) break;
        const uint32_t r = a.index ? a.index[item] : item;
        uint16_t *out = a.out + (size_t)r * GZT_WORDS;
        const uint32_t l1 = a.len1[r], l2 = a.len2 ? a.len2[r] : 0u, n = l1 + l2;
        bool outside = false;  // as k_minimise_probe checks its segments
        {
            const uint64_t o1 = a.off1[r], o2 = a.off2 ? a.off2[r] : 0;
            outside = (o1 & 63u) || o1 > a.n_bases || l1 > a.n_bases - o1 || (a.off2 && ((o2 & 63u) || o2 > a.n_bases || l2 > a.n_bases - o2));
        }
        if (n == 0 || n > a.max_len || n > GZT_MAX_LEN || outside) {
            // EVERY lane stores the word: the wavefront must come round the loop whole.  With `if (lane == 0)` in front of the store the
            // compiler sent lanes 1 .. 63 round on their own; their `item` is 0 and lane 0 is not there to fetch one, so they tallied read 0
            // once more, without lane 0's candidate and counters, over the proper tallies of read 0 (and for ever, if read 0 is skipped itself).
            // Only a device batch comes here: a host batch's launches list the reads to tally.
            out[316] = 1;
            continue;
        }
        for (uint32_t i = lane; i < 256; i += WAVE) tall[i] = 0;
        // 1a. codes
        const uint32_t *b1 = a.bases + (a.off1[r] >> 4), *b2 = a.off2 ? a.bases + (a.off2[r] >> 4) : nullptr;
        const uint32_t *m1 = a.nmask ? a.nmask + (a.off1[r] >> 5) : nullptr, *m2 = (a.nmask && a.off2) ? a.nmask + (a.off2[r] >> 5) : nullptr;
        // room for the reads of three words that start at the last position (4 bits) / for a comparison running MAX_MATCH past the end (2 bits)
        const uint32_t nwords = BITS == 4 ? (n + 7) / 8 + 3 : (n + 15) / 16 + 19;
        for (uint32_t wi = lane; wi < nwords; wi += WAVE) {
            uint32_t word = 0;
            for (uint32_t j = 0; j < CPW; ++j) {
                const uint32_t p = wi * CPW + j;
                uint32_t c = BITS == 4 ? 0xFu : 0u;
                if (p < n) {
                    const bool second = p >= l1;
                    const uint32_t q = second ? p - l1 : p;
                    const uint32_t *bw = second ? b2 : b1, *mw = second ? m2 : m1;
                    c = (bw[q >> 4] >> ((q & 15u) * 2)) & 3u;
                    if (BITS == 4 && mw && ((mw[q >> 5] >> (q & 31u)) & 1u)) c = 4;
                }
                word |= c << (BITS * j);
            }
            cs4[wi] = word;
        }
        __syncthreads();
        // the codes starting at position p, one word of them (position p in the low bits)
        auto get8 = [&](uint32_t p) -> uint32_t {
            const uint32_t w = p >> LOGC;
            return (uint32_t)__builtin_amdgcn_alignbit(cs4[w + 1], cs4[w], p * BITS);
        };
        const uint32_t m = n >= 3 ? n - 2 : 0;  // positions 0 .. n-3 enter the dictionary
        auto key_of = [](uint32_t v) -> uint32_t {  // the trigram's class: 125 of them with N, 64 without
            return BITS == 4 ? (v & 15u) * 25u + ((v >> 4) & 15u) * 5u + ((v >> 8) & 15u) : v & 63u;
        };
        // 1b. class sizes -> class starts
        for (uint32_t p = lane; p < m; p += WAVE) atomicAdd(&ccnt[key_of(get8(p))], 1u);
        __syncthreads();
        {   // exclusive scan over the 125 classes: two classes per lane (once per read)
            const uint32_t k0 = lane * 2, c0 = k0 < 125 ? ccnt[k0] : 0u, c1 = k0 + 1 < 125 ? ccnt[k0 + 1] : 0u;
            uint32_t incl = c0 + c1;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, o); if (lane >= (uint32_t)o) incl += t; }
            const uint32_t ex = incl - (c0 + c1);
            if (k0 < 125) { ccnt[k0] = ex; cstart[k0] = ex; }
            if (k0 + 1 < 125) { ccnt[k0 + 1] = ex + c0; cstart[k0 + 1] = ex + c0; }
        }
        __syncthreads();
        // 1c. positions into their classes, in position order: per tile of 64 positions every lane finds the lanes holding the same trigram
        // (seven ballots, one per key bit), its rank among them, and the class's lowest lane moves the cursor on
        for (uint32_t p0 = 0; p0 < m; p0 += WAVE) {
            const uint32_t p = p0 + lane;
            const bool valid = p < m;
            const uint32_t k = valid ? key_of(get8(p)) : 127u;  // 127: no class
            uint64_t same = ~0ULL;
#pragma unroll
            for (uint32_t bit = 0; bit < 7; ++bit) {
                const uint64_t bm = __ballot((k >> bit) & 1u);
                same &= ((k >> bit) & 1u) ? bm : ~bm;
            }
            const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u));
            if (valid) {
                const uint32_t before = ccnt[k], slot = before + rk;
                occ[slot] = (uint16_t)p;
                pinfo[p] = slot | ((slot - cstart[k]) << 16);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every lane of the class has read the cursor before its lowest lane moves it
                if (rk == 0) ccnt[k] = before + (uint32_t)__popcll(same);
            }
        }
        __syncthreads();
        for (uint32_t i = lane; i < GZT_WORDS; i += WAVE) tall[i] = 0;  // the builder's cursors lived here
        // occ[] and pinfo[] are read back by this wavefront only: its stores went through the CU's vector cache (write-through, shared by the CU's
        // wavefronts, so coherent for them) and the barrier below waits for them.  A device-scope fence here (round 2 had one) writes the XCD's
        // whole L2 back to memory and empties the vector cache, per read: a third of the kernel's time on 5 kb reads.
        __syncthreads();

        // 2. deflate_slow (deflate.c), level 6: max_lazy 16, good_match 8, nice_match 128, max_chain 128.  The walk is wave-uniform and instruction
        // issue is what bounds it (scalar and vector instructions alike), so the step is written for few instructions:
        //  * whatever costs nothing extra per lane is done per lane (the position again in a vector register for LDS addresses and shift counts,
        //    the distance code, the tallies);
        //  * the common case -- no candidate agrees beyond the first eleven letters, the read is not about to end, nothing is out of the
        //    window -- is decided by ONE max-reduction over (length - 3) << 16 | position; the reduction's own result says whether it was the
        //    common case (a length of eleven: some candidate may go on), and only then the general rule (longer comparisons, the walk ending
        //    at the first candidate of nice_match, candidates out of the window) is evaluated.
        const uint32_t MIN_MATCH = 3, MAX_MATCH = 258, MAX_DIST = 32768 - 262, TOO_FAR = 4096;
        const uint32_t cs4_lds = (uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t *)cs4;  // LDS byte address of the codes
        auto lds_u32 = [](uint32_t byte_addr) -> uint32_t { return *(const __attribute__((address_space(3))) uint32_t *)(size_t)byte_addr; };
        uint32_t csb = cs4_lds;  // ... in a vector register the compiler knows nothing about (it would re-derive it as two additions per use)
        asm volatile("" : "+v"(csb));
        auto word_addr = [&](uint32_t p) -> uint32_t {  // LDS address of the word holding code p: one shift, one shift-add
            uint32_t w = p >> LOGC;
            asm("" : "+v"(w));
            return (w << 2) + csb;
        };
        auto codes8 = [&](uint32_t p) -> uint32_t {  // get8 with two vector instructions of address arithmetic
            const uint32_t ad = word_addr(p);
            return (uint32_t)__builtin_amdgcn_alignbit(lds_u32(ad + 4), lds_u32(ad), p * BITS);
        };
        // steps that need the general rule whatever the candidates look like: the last eleven positions (nice_match = lookahead there) and
        // steps that need the general rule whatever the candidates look like: the last positions (nice_match = lookahead, within reach of the
        // first comparison there) and positions with candidates beyond the window
        const uint32_t rare_from = n >= FIRST + 4u ? min(n - (FIRST + 4u), MAX_DIST) : 0u;
        uint32_t S = 0, ML = MIN_MATCH - 1, MS = 0, W0 = 0, n_long = 0;
        uint32_t Sv = 0;                                  // S, per lane
        asm volatile("" : "+v"(Sv));
        uint32_t lit_cnt = 0, len_cnt = 0, dist_cnt = 0;  // lane c: literals of code c; lane j: matches of length j + 3; lane d: matches of distance code d
        uint32_t code_prev = 255;                        // the literal waiting for the lazy evaluation (255: none -- match_available is false)
        uint32_t pw = lane < m ? pinfo[lane] : 0u;       // info words of positions W0 .. W0 + 63
#ifdef GZT_DIAG_BUILD_ONLY  // DIAGNOSTICS BUILD ONLY (tools/build_diag.sh): what do the class arrays cost without the walk?
        S = n;
#endif
        while (S < n) {
            const uint32_t look = n - S;
            if (S - W0 >= GZT_WIN) {
                W0 = S;
                const uint32_t p = S + lane;
                pw = p < m ? pinfo[p] : 0u;
            }
            const uint32_t pi = (uint32_t)__builtin_amdgcn_readlane((int)pw, (int)(S - W0));
            const uint32_t top = pi & 0xFFFFu, rs = pi >> 16;  // rs earlier positions share this trigram; the most recent one is occ[top - 1]
            const uint32_t PL = ML, PM = MS;                   // prev_length, prev_match
            ML = MIN_MATCH - 1;
            // the codes at S: three words from one address
            const uint32_t cwa = word_addr(Sv), sh = Sv * BITS;
            const uint32_t w0 = lds_u32(cwa), w1 = lds_u32(cwa + 4), w2 = lds_u32(cwa + 8);
            const uint32_t here = (uint32_t)__builtin_amdgcn_alignbit(w1, w0, sh);      // codes S .. S + 7
            const uint32_t mid = (uint32_t)__builtin_amdgcn_alignbit(w2, w1, sh);       // codes S + 8 .. S + 15
            const uint32_t next8 = (uint32_t)__builtin_amdgcn_alignbit(mid, here, 3 * BITS);  // codes S + 3 onwards, a word of them
            // longest_match, by the whole wavefront: lane j measures the j-th and (more than 64 candidates) the (64 + j)-th most recent one.
            // kk candidates are looked at: none beyond max_lazy (prev_length >= 16), a quarter of the chain after a good match.  Every lane
            // loads (an index below the array is clamped; the value is dropped), so the loads need no exec masking.
            uint32_t kk = PL >= 8u ? 32u : 128u;
            kk = rs < kk ? rs : kk;
            if (PL >= 16u) kk = 0;
            const int32_t ia = (int32_t)(top - 1u - lane);
            uint32_t curA = occ[ia > 0 ? ia : 0];
            curA = lane < kk ? curA : 0u;
            uint32_t curB = 0;
            if (kk > 64u) {
                curB = occ[(int32_t)(top - 65u - lane) > 0 ? top - 65u - lane : 0u];
                curB = lane + 64u < kk ? curB : 0u;
            }
            const uint32_t head = (uint32_t)__builtin_amdgcn_readfirstlane((int)curA);
            const uint32_t limit = S > MAX_DIST ? S - MAX_DIST : 0u;
            // (hash_head != NIL -- position 0 doubles as NIL, as in zlib -- and strstart - hash_head <= MAX_DIST)
            if (head >= (limit ? limit : 1u)) {
                // candidates along the chain lie further and further back: those in the window are a prefix; the head may lie ON the limit
                const bool okA = curA > limit || lane == 0, okB = curB > limit;
                // common prefix: same class = same trigram, then eight codes at once (the 0xF behind the data ends every match at n).
                // (lanes without a candidate read position 3 onwards: in range, ignored)
                const uint32_t xa = next8 ^ codes8(curA + 3u);
                const uint32_t qa = (xa ? (uint32_t)__builtin_ctz(xa) : 32u) >> CSH;  // agreeing codes behind the trigram, at most FIRST
                uint32_t v = okA ? (qa << 16) | curA : 0u;
                if (kk > 64u) {
                    const uint32_t xb = next8 ^ codes8(curB + 3u);
                    const uint32_t qb = (xb ? (uint32_t)__builtin_ctz(xb) : 32u) >> CSH;
                    v = max(v, okB ? (qb << 16) | curB : 0u);
                }
                uint32_t mx = gz_wave_umax(v);
                if (mx >= (FIRST << 16) || S > rare_from) {
                    asm volatile("" ::: "memory");  // (a branch, not selects: one step in some hundreds comes here)
                    const uint32_t xb = kk > 64u ? next8 ^ codes8(curB + 3u) : 1u;
                    // the general rule.  Further codes eight at a time while some candidate still agrees: those lanes all stand at the same
                    // length, so the current string's codes are one uniform read per step
                    uint32_t lenA = 3u + qa, lenB = 3u + ((xb ? (uint32_t)__builtin_ctz(xb) : 32u) >> CSH);
                    bool goA = okA && xa == 0, goB = okB && xb == 0;
                    uint32_t at = 3u + FIRST;
                    while (at < MAX_MATCH && __builtin_amdgcn_ballot_w64(goA || goB)) {
                        const uint32_t mine = codes8(S + at);
                        if (goA) {
                            const uint32_t y = mine ^ codes8(curA + at);
                            lenA = at + ((y ? (uint32_t)__builtin_ctz(y) : 32u) >> CSH);
                            goA = y == 0;
                        }
                        if (goB) {
                            const uint32_t y = mine ^ codes8(curB + at);
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
                    v = okA ? ((lenA - 3u) << 16) | curA : 0u;
                    const uint64_t stopA = __builtin_amdgcn_ballot_w64(okA && lenA >= T);
                    if (stopA) { if (lane > (uint32_t)__builtin_ctzll(stopA)) v = 0; }
                    else if (kk > 64u && __builtin_amdgcn_ballot_w64(okA) == ~0ULL) {  // the chain went on through all of the first 64
                        uint32_t vb = okB ? ((lenB - 3u) << 16) | curB : 0u;
                        const uint64_t stopB = __builtin_amdgcn_ballot_w64(okB && lenB >= T);
                        if (stopB) { if (lane > (uint32_t)__builtin_ctzll(stopB)) vb = 0; }
                        v = max(v, vb);
                    }
                    mx = gz_wave_umax(v);
                }
                uint32_t best = PL;
                if ((mx >> 16) + 3u > best) { best = (mx >> 16) + 3u; MS = mx & 0xFFFFu; }
                ML = best <= look ? best : look;
                if (ML == MIN_MATCH) { if (S - MS > TOO_FAR) ML = MIN_MATCH - 1; }
            }
            // (INSERT_STRING: nothing to do -- see 1.)
            if (PL >= MIN_MATCH && ML <= PL) {
                // the previous position's match is emitted: length PL, distance S - 1 - PM (tally_dist counts dist - 1)
                const uint32_t lc = PL - MIN_MATCH;
                len_cnt += lane == lc ? 1u : 0u;
                if (lc >= 64u) {
                    asm volatile("" ::: "memory");
                    ++n_long;
                    if (lane == 0) atomicAdd(&tall[257 + gz_length_code(lc)], 1u);
                }
                // d_code(d): the exponent and the first mantissa bit of d as a float (exact below 2^24), d itself below 2
                const uint32_t d = Sv - (PM + 2u);
                const uint32_t dc = d < 2u ? d : (__float_as_uint((float)d) >> 22) - 254u;
                dist_cnt += lane == dc ? 1u : 0u;
                S += PL - 1; Sv += PL - 1;
                code_prev = 255;
                ML = MIN_MATCH - 1;
            } else {
                lit_cnt += lane == code_prev ? 1u : 0u;  // the waiting literal, if there is one
                code_prev = here & CMASK;
                S++; Sv++;
            }
        }
        // 3. out: a second deflate block (lit_bufsize - 1 = 16 383 symbols reached inside the loop) is sized on the host
        uint32_t nsym = lit_cnt + len_cnt;
        for (int o = 32; o > 0; o >>= 1) nsym += (uint32_t)__shfl_xor((int)nsym, o);
        const bool too_many = nsym + n_long >= GZT_SYMBOL_LIMIT;
        lit_cnt += lane == code_prev ? 1u : 0u;  // the literal still waiting at the end
        if (lane < 5) tall[lane == 0 ? 65u : lane == 1 ? 67u : lane == 2 ? 71u : lane == 3 ? 84u : 78u] = lit_cnt;  // A C G T N
        if (lane == 5) tall[256] = 1;  // END_BLOCK
        if (len_cnt) atomicAdd(&tall[257 + gz_length_code(lane)], len_cnt);
        if (lane < 30) tall[286 + lane] = dist_cnt;
        __syncthreads();
        for (uint32_t i = lane; i < 316; i += WAVE) out[i] = (uint16_t)tall[i];
        if (lane == 0) out[316] = too_many ? 1 : 0;
        __syncthreads();  // the next read re-uses the LDS
    }
}
static size_t gzt_lds_bytes(uint32_t max_len, int bits) {
    return GZT_WORDS * 4 + (bits == 4 ? ((size_t)max_len + 7) / 8 + 4 : ((size_t)max_len + 15) / 16 + 20) * 4;
}
static uint32_t gzt_stride32(uint32_t max_len) {
    const uint32_t cap = (max_len + 7u) & ~7u;
    return (cap + GZT_WIN + cap / 2 + 31u) & ~31u;  // whole 128-byte lines: two wavefronts never write into one
}
