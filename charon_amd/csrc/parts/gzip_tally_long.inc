// gzip_tally_long.inc -- k_gzip_long: zlib level-6 deflate_slow of reads of ANY length (window slide, any number of deflate blocks),
// each block sized in place: the gzip member size of every read (chn_batch.gzip_output = CHN_GZIP_SIZES_ALL)
// Part of the single translation unit charon_hip.hip (included in order, after gzip_tally.inc and gzip_size_dev.inc); not a stand-alone source.

// ------------------------------------------------------------------------------------------------
// k_gzip_tally's walk (one wavefront per read, the trigram classes as arrays, the wave-parallel longest_match with one DPP
// max-reduction, the tallies in registers, 4-bit codes with an N in the batch and 2-bit codes without), extended to what a read of
// any length needs.  Every statement follows the host emulator's deflate_slow (charon_amd/csrc/host/gzip_size.hpp, run()):
//  * EPOCHS of 32 768 positions.  The chain at p only reaches back MAX_DIST = 32 506 < 32 768, so the candidates of a position of
//    epoch e lie in epochs e and e - 1.  The class arrays are built per epoch when the walk enters it (occ[] of the epoch: positions
//    by class, 16-bit offsets, two buffers used in turn; pinfo[] of the epoch: slot | rank inside the class << 16), and the class
//    ranges of the previous epoch are kept in LDS: candidate j of p is the j-th entry below slot(p) while j < rank(p), then the
//    (j - rank(p))-th entry from the top of the class in epoch e - 1.
//  * The codes stream through a RING in LDS holding four epochs (the walk in epoch e reads e - 1 .. e + 1; epoch e + 1 is loaded
//    from the batch's packed bases and N mask as the walk enters e), with the first words mirrored behind its end so that a
//    three-word read never wraps.
//  * zlib's window slide: fill_window advances the base by w_size whenever strstart - base >= w_size + MAX_DIST (also near the end
//    of the input); a head at or below the base is NIL; the head may lie exactly MAX_DIST back, the other candidates strictly above
//    limit = max(strstart - MAX_DIST, base).  Positions are absolute; the reduction packs a candidate as (length - 3) << 16 |
//    (candidate + 65 536 - strstart): inside the window that is 16 bits, and larger means more recent.
//  * Block flushes: a scalar symbol counter; when the 16 383rd symbol of a block is tallied (match branch or lazy-literal branch)
//    the block record (the 286 + 30 frequencies in LDS, stored_len = strstart - block_start, buf = block_start >= base) is sized
//    at once by lane 0 with _tr_flush_block's arithmetic (gzsize_dev::flush_block_bits, shared with k_gzip_size; its heap in LDS),
//    the running bit count carries the stored blocks' byte padding, and the tallies restart.  The final block (the pending literal
//    first, then the flush with last = 1; it may be empty) closes the member: size = 18 + bits / 8.
// Per wavefront: LDS 3 328 B of tallies and class ranges + 7 088 B of tree work + the ring (64 KiB with 4-bit codes, 32 KiB with
// 2-bit codes) + 16 B of mirror: 75 968 / 43 200 bytes, two / three wavefronts per CU.  Scratch in global memory: occ[2][32 768]
// (16 bits) + pinfo[32 768 + 64] (32 bits) = 262 400 bytes.  Neither grows with the read's length.
// ------------------------------------------------------------------------------------------------
#define GZL_EPOCH 32768u        // positions per class-array epoch (= zlib's w_size)
#define GZL_RING_EPOCHS 4u      // epochs of codes in the LDS ring
#define GZL_GUARD 4u            // ring words mirrored behind its end
#define GZL_HEAD_WORDS 832u     // LDS: tallies [320], class cursors / starts of this epoch, class starts / ends of the previous one [4][128]
#define GZL_BLOCK_SYMBOLS 16383u  // lit_bufsize - 1 (memLevel 8): zlib flushes a block when it holds this many symbols
#define GZL_MAX_READ 0xFFF00000u  // the walk's absolute positions stay below 2^32 (two epochs of codes are loaded ahead)
enum { GZL_ALL = 0, GZL_HANDED_BACK = 1 };
struct GzlArgs {
    const uint32_t *bases, *nmask;
    const uint64_t *off1, *off2;
    const uint32_t *len1, *len2;
    uint64_t n_bases;            // size of `bases` in letters (a segment outside it is not sized)
    uint32_t bound;              // longest read to size (both mates together)
    uint32_t short_max;          // GZL_HANDED_BACK: the tally launches' bound (only reads of at most this many letters)
    uint32_t filter;             // GZL_ALL: every listed read; GZL_HANDED_BACK: the listed reads whose tally status (tallies[316]) is not 0
    const uint16_t *tallies;     // [n_reads][GZT_WORDS] (GZL_HANDED_BACK)
    const uint32_t *index;       // reads of this launch
    uint32_t count;
    uint32_t *sizes;             // [n_reads]: the gzip member size of every read this launch sizes (others untouched)
    uint32_t *scratch;           // [blocks][GZL_STRIDE32]
    uint32_t *counter;           // next read of the launch (zero when the launch starts)
};
#define GZL_STRIDE32 (GZL_EPOCH + GZL_EPOCH + GZT_WIN)  // occ[2][GZL_EPOCH] 16-bit, pinfo[GZL_EPOCH + GZT_WIN]: a multiple of 32 words

__host__ __device__ constexpr size_t gzl_work_bytes() { return (sizeof(gzsize_dev::Work) + 15) & ~(size_t)15; }
static size_t gzl_lds_bytes(int bits) {
    return (size_t)GZL_HEAD_WORDS * 4 + gzl_work_bytes() + ((size_t)GZL_EPOCH * GZL_RING_EPOCHS * bits / 32 + GZL_GUARD) * 4;
}

template <int BITS>
__global__ __launch_bounds__(WAVE) void k_gzip_long(const GzlArgs a) {
    constexpr uint32_t CPW = 32 / BITS, LOGC = BITS == 4 ? 3 : 4, CMASK = (1u << BITS) - 1u;  // codes per word
    constexpr uint32_t FIRST = CPW;  // codes the first comparison covers behind the trigram
    constexpr uint32_t CSH = BITS == 4 ? 2 : 1;
    constexpr uint32_t EPW = GZL_EPOCH / CPW, RWORDS = EPW * GZL_RING_EPOCHS, RMASK = RWORDS - 1u;
    constexpr uint32_t PAD = BITS == 4 ? 0xFu : 0u;  // the code behind the data
    extern __shared__ __align__(16) unsigned char gsm[];
    const uint32_t lane = lane_id();
    uint32_t *tall = reinterpret_cast<uint32_t *>(gsm);  // [320] the block's tallies (long match lengths during the walk, everything at a flush)
    uint32_t *ccur = tall + GZT_WORDS, *cst = ccur + 128, *pst = cst + 128, *pen = pst + 128;
    gzsize_dev::Work *work = reinterpret_cast<gzsize_dev::Work *>(gsm + GZL_HEAD_WORDS * 4);
    uint32_t *ring = reinterpret_cast<uint32_t *>(gsm + GZL_HEAD_WORDS * 4 + gzl_work_bytes());
    uint16_t *occ = reinterpret_cast<uint16_t *>(a.scratch + (size_t)blockIdx.x * GZL_STRIDE32);  // [2][GZL_EPOCH]
    uint32_t *pinfo = a.scratch + (size_t)blockIdx.x * GZL_STRIDE32 + GZL_EPOCH;                  // [GZL_EPOCH + GZT_WIN]
    for (uint32_t i = lane; i < GZT_WORDS; i += WAVE) tall[i] = 0;
    __syncthreads();
    for (;;) {
        uint32_t item = 0;
        if (lane == 0) item = atomicAdd(a.counter, 1u);
        item = (uint32_t)__builtin_amdgcn_readfirstlane((int)item);
        if (item >= a.count) break;
        const uint32_t r = a.index[item];
        const uint32_t l1 = a.len1[r], l2 = a.len2 ? a.len2[r] : 0u;
        const uint64_t n64 = (uint64_t)l1 + l2;
        const uint64_t o1 = a.off1[r], o2 = a.off2 ? a.off2[r] : 0;
        const bool outside = (o1 & 63u) || o1 > a.n_bases || l1 > a.n_bases - o1 || (a.off2 && ((o2 & 63u) || o2 > a.n_bases || l2 > a.n_bases - o2));
        bool take = !outside && n64 != 0 && n64 <= a.bound && n64 <= GZL_MAX_READ;
        if (a.filter == GZL_HANDED_BACK) take = take && n64 <= a.short_max && a.tallies[(size_t)r * GZT_WORDS + 316] != 0;
        if (!take) continue;
        const uint32_t n = (uint32_t)n64;
        const uint32_t *b1 = a.bases + (o1 >> 4), *b2 = a.off2 ? a.bases + (o2 >> 4) : nullptr;
        const uint32_t *m1 = a.nmask ? a.nmask + (o1 >> 5) : nullptr, *m2 = (a.nmask && a.off2) ? a.nmask + (o2 >> 5) : nullptr;
        // the codes of epoch e into the ring (the batch's packed bases and N mask; PAD behind the data)
        auto load_epoch = [&](uint32_t e) {
            for (uint32_t wi = lane; wi < EPW; wi += WAVE) {
                const uint32_t gw = e * EPW + wi;
                uint32_t word = 0;
                for (uint32_t j = 0; j < CPW; ++j) {
                    const uint32_t p = gw * CPW + j;
                    uint32_t c = PAD;
                    if (p < n) {
                        const bool second = p >= l1;
                        const uint32_t q = second ? p - l1 : p;
                        const uint32_t *bw = second ? b2 : b1, *mw = second ? m2 : m1;
                        c = (bw[q >> 4] >> ((q & 15u) * 2)) & 3u;
                        if (BITS == 4 && mw && ((mw[q >> 5] >> (q & 31u)) & 1u)) c = 4;
                    }
                    word |= c << (BITS * j);
                }
                const uint32_t w = gw & RMASK;
                ring[w] = word;
                if (w < GZL_GUARD) ring[RWORDS + w] = word;
            }
        };
        auto get8 = [&](uint32_t p) -> uint32_t {  // the codes starting at position p, one word of them
            const uint32_t w = (p >> LOGC) & RMASK;
            return (uint32_t)__builtin_amdgcn_alignbit(ring[w + 1], ring[w], p * BITS);
        };
        auto key_of = [](uint32_t v) -> uint32_t {  // the trigram's class: 125 of them with N, 64 without
            return BITS == 4 ? (v & 15u) * 25u + ((v >> 4) & 15u) * 5u + ((v >> 8) & 15u) : v & 63u;
        };
        const uint32_t m = n >= 3 ? n - 2 : 0;  // positions 0 .. n-3 enter the dictionary
        // the class arrays of epoch e (its codes and the first two of epoch e + 1 are in the ring); the previous epoch's class
        // ranges move to pst / pen
        auto build_epoch = [&](uint32_t e) {
            const uint32_t E0 = e * GZL_EPOCH, P1 = min(m, E0 + GZL_EPOCH);
            uint16_t *occE = occ + (e & 1u) * GZL_EPOCH;
            for (uint32_t k = lane; k < 128; k += WAVE) {
                pst[k] = e ? cst[k] : 0u;
                pen[k] = e ? ccur[k] : 0u;  // (the cursor ended at the class's end)
                ccur[k] = 0;
            }
            __syncthreads();
            for (uint32_t p = E0 + lane; p < P1; p += WAVE) atomicAdd(&ccur[key_of(get8(p))], 1u);
            __syncthreads();
            {   // exclusive scan over the classes: two per lane
                const uint32_t k0 = lane * 2, c0 = ccur[k0], c1 = ccur[k0 + 1];
                uint32_t incl = c0 + c1;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, o); if (lane >= (uint32_t)o) incl += t; }
                const uint32_t ex = incl - (c0 + c1);
                ccur[k0] = ex; cst[k0] = ex;
                ccur[k0 + 1] = ex + c0; cst[k0 + 1] = ex + c0;
            }
            __syncthreads();
            for (uint32_t p0 = E0; p0 < P1; p0 += WAVE) {
                const uint32_t p = p0 + lane;
                const bool valid = p < P1;
                const uint32_t k = valid ? key_of(get8(p)) : 127u;  // 127: no class
                uint64_t same = ~0ULL;
#pragma unroll
                for (uint32_t bit = 0; bit < 7; ++bit) {
                    const uint64_t bm = __ballot((k >> bit) & 1u);
                    same &= ((k >> bit) & 1u) ? bm : ~bm;
                }
                const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u));
                if (valid) {
                    const uint32_t before = ccur[k], slot = before + rk;
                    occE[slot] = (uint16_t)(p - E0);
                    pinfo[p - E0] = slot | ((slot - cst[k]) << 16);
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every lane of the class has read the cursor before its lowest lane moves it
                    if (rk == 0) ccur[k] = before + (uint32_t)__popcll(same);
                }
            }
            __syncthreads();  // (occ[] and pinfo[] are read back by this wavefront only: see k_gzip_tally)
        };

        const uint32_t MIN_MATCH = 3, MAX_MATCH = 258, W_SIZE = GZL_EPOCH, MAX_DIST = 32768 - 262, TOO_FAR = 4096, MIN_LOOKAHEAD = 262;
        const uint32_t ring_lds = (uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t *)ring;
        auto lds_u32 = [](uint32_t byte_addr) -> uint32_t { return *(const __attribute__((address_space(3))) uint32_t *)(size_t)byte_addr; };
        uint32_t csb = ring_lds;
        asm volatile("" : "+v"(csb));
        auto word_addr = [&](uint32_t p) -> uint32_t {  // LDS address of the ring word holding code p
            uint32_t w = (p >> LOGC) & RMASK;
            asm("" : "+v"(w));
            return (w << 2) + csb;
        };
        auto codes8 = [&](uint32_t p) -> uint32_t {
            const uint32_t ad = word_addr(p);
            return (uint32_t)__builtin_amdgcn_alignbit(lds_u32(ad + 4), lds_u32(ad), p * BITS);
        };
        uint32_t S = 0, ML = MIN_MATCH - 1, MS = 0, W0 = 0;
        uint32_t Sv = 0;  // S, per lane
        asm volatile("" : "+v"(Sv));
        uint32_t lit_cnt = 0, len_cnt = 0, dist_cnt = 0;  // lane c: literals of code c; lane j: matches of length j + 3; lane d: matches of distance code d
        uint32_t code_prev = 255;                        // the literal waiting for the lazy evaluation (255: none)
        uint32_t nsym = 0, block_start = 0;               // symbols of the current block; where it starts
        uint32_t base = 0, loaded_end = min(n, 2u * W_SIZE);  // zlib's window: its start, the end of what fill_window has read
        uint32_t ep_end = 0, E0 = 0, P1 = 0, ebuf = 0, pbuf = 0;  // the epoch of the class arrays: [E0, ep_end), positions entered below P1
        uint32_t pw = 0;
        uint64_t bits = 0;  // the member's deflate bits so far (lane 0)
        // a block's record into LDS, sized by lane 0 (_tr_flush_block), tallies cleared
        auto flush = [&](uint32_t stored_len, bool buf, bool last) {
            if (lane < 5) tall[lane == 0 ? 65u : lane == 1 ? 67u : lane == 2 ? 71u : lane == 3 ? 84u : 78u] = lit_cnt;  // A C G T N
            if (len_cnt) atomicAdd(&tall[257 + gz_length_code(lane)], len_cnt);
            if (lane < 30) tall[286 + lane] = dist_cnt;
            __syncthreads();
            if (lane == 0) gzsize_dev::flush_block_bits(*work, tall, tall + 286, stored_len, buf, last, bits);
            __syncthreads();
            for (uint32_t i = lane; i < GZT_WORDS; i += WAVE) tall[i] = 0;
            __syncthreads();
            lit_cnt = len_cnt = dist_cnt = 0;
            nsym = 0;
        };
        load_epoch(0);
        for (;;) {
            if (loaded_end - S < MIN_LOOKAHEAD) {  // fill_window: the slide (even with no input left), then as much input as fits
                if (S - base >= W_SIZE + MAX_DIST) base += W_SIZE;
                loaded_end = (uint32_t)min((uint64_t)n, (uint64_t)base + 2u * W_SIZE);
            }
            if (S >= loaded_end) break;
            const uint32_t look = loaded_end - S;
            if (S >= ep_end) {  // the walk enters a new epoch: codes of the next one, then this one's class arrays
                const uint32_t e = S / GZL_EPOCH;
                load_epoch(e + 1);
                __syncthreads();
                build_epoch(e);
                E0 = e * GZL_EPOCH; ep_end = E0 + GZL_EPOCH; P1 = min(m, ep_end);
                ebuf = (e & 1u) * GZL_EPOCH; pbuf = GZL_EPOCH - ebuf;
                W0 = S;
                pw = S + lane < P1 ? pinfo[S + lane - E0] : 0u;
            } else if (S - W0 >= GZT_WIN) {
                W0 = S;
                pw = S + lane < P1 ? pinfo[S + lane - E0] : 0u;
            }
            const uint32_t pi = (uint32_t)__builtin_amdgcn_readlane((int)pw, (int)(S - W0));
            const uint32_t top = pi & 0xFFFFu, rsE = pi >> 16;  // rsE earlier positions of this epoch share the trigram; the most recent is occ[top - 1]
            const uint32_t PL = ML, PM = MS;
            ML = MIN_MATCH - 1;
            const uint32_t cwa = word_addr(Sv), sh = Sv * BITS;
            const uint32_t w0 = lds_u32(cwa), w1 = lds_u32(cwa + 4), w2 = lds_u32(cwa + 8);
            const uint32_t here = (uint32_t)__builtin_amdgcn_alignbit(w1, w0, sh);
            const uint32_t mid = (uint32_t)__builtin_amdgcn_alignbit(w2, w1, sh);
            const uint32_t next8 = (uint32_t)__builtin_amdgcn_alignbit(mid, here, 3 * BITS);
            // the chain: rsE entries of this epoch, then the class's entries of the previous epoch (older ones are beyond MAX_DIST)
            const bool enters = S < m;
            const uint32_t k = enters ? key_of(here) : 0u;
            const uint32_t pend_k = pen[k], pcount = enters ? pend_k - pst[k] : 0u;
            uint32_t kk = PL >= 8u ? 32u : 128u;
            kk = min(rsE + pcount, kk);
            if (PL >= 16u) kk = 0;
            auto cand = [&](uint32_t j) -> uint32_t {
                const bool inE = j < rsE;
                const uint32_t idx = inE ? ebuf + top - 1u - j : pbuf + pend_k - 1u - (j - rsE);
                const uint32_t v = occ[j < kk ? idx : 0u];
                return j < kk ? v + (inE ? E0 : E0 - GZL_EPOCH) : 0u;
            };
            uint32_t curA = cand(lane);
            uint32_t curB = 0;
            if (kk > 64u) curB = cand(lane + 64u);
            const uint32_t head = (uint32_t)__builtin_amdgcn_readfirstlane((int)curA);
            const uint32_t limit = S - base > MAX_DIST ? S - MAX_DIST : base;
            // hash_head: not NIL (at or below the base), within MAX_DIST
            if (kk != 0 && head > base && S - head <= MAX_DIST) {
                const bool okA = curA > limit || lane == 0, okB = curB > limit;
                const uint32_t relA = curA + 65536u - S, relB = curB + 65536u - S;
                const uint32_t xa = next8 ^ codes8(curA + 3u);
                const uint32_t qa = (xa ? (uint32_t)__builtin_ctz(xa) : 32u) >> CSH;
                uint32_t v = okA ? (qa << 16) | relA : 0u;
                if (kk > 64u) {
                    const uint32_t xb = next8 ^ codes8(curB + 3u);
                    const uint32_t qb = (xb ? (uint32_t)__builtin_ctz(xb) : 32u) >> CSH;
                    v = max(v, okB ? (qb << 16) | relB : 0u);
                }
                uint32_t mx = gz_wave_umax(v);
                if (mx >= (FIRST << 16) || look < FIRST + 4u) {
                    asm volatile("" ::: "memory");
                    const uint32_t xb = kk > 64u ? next8 ^ codes8(curB + 3u) : 1u;
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
                    if (BITS == 2) { lenA = min(lenA, look); lenB = min(lenB, look); }
                    const uint32_t nice = look < 128u ? look : 128u;
                    const uint32_t T = nice > PL + 1 ? nice : PL + 1;
                    v = okA ? ((lenA - 3u) << 16) | relA : 0u;
                    const uint64_t stopA = __builtin_amdgcn_ballot_w64(okA && lenA >= T);
                    if (stopA) { if (lane > (uint32_t)__builtin_ctzll(stopA)) v = 0; }
                    else if (kk > 64u && __builtin_amdgcn_ballot_w64(okA) == ~0ULL) {
                        uint32_t vb = okB ? ((lenB - 3u) << 16) | relB : 0u;
                        const uint64_t stopB = __builtin_amdgcn_ballot_w64(okB && lenB >= T);
                        if (stopB) { if (lane > (uint32_t)__builtin_ctzll(stopB)) vb = 0; }
                        v = max(v, vb);
                    }
                    mx = gz_wave_umax(v);
                }
                uint32_t best = PL;
                if ((mx >> 16) + 3u > best) { best = (mx >> 16) + 3u; MS = S + (mx & 0xFFFFu) - 65536u; }
                ML = best <= look ? best : look;
                if (ML == MIN_MATCH) { if (S - MS > TOO_FAR) ML = MIN_MATCH - 1; }
            }
            if (PL >= MIN_MATCH && ML <= PL) {
                const uint32_t lc = PL - MIN_MATCH;
                len_cnt += lane == lc ? 1u : 0u;
                if (lc >= 64u) {
                    asm volatile("" ::: "memory");
                    if (lane == 0) atomicAdd(&tall[257 + gz_length_code(lc)], 1u);
                }
                const uint32_t d = Sv - (PM + 2u);
                const uint32_t dc = d < 2u ? d : (__float_as_uint((float)d) >> 22) - 254u;
                dist_cnt += lane == dc ? 1u : 0u;
                S += PL - 1; Sv += PL - 1;
                code_prev = 255;
                ML = MIN_MATCH - 1;
                if (++nsym == GZL_BLOCK_SYMBOLS) { flush(S - block_start, block_start >= base, false); block_start = S; }
            } else {
                if (code_prev != 255u) {
                    lit_cnt += lane == code_prev ? 1u : 0u;
                    if (++nsym == GZL_BLOCK_SYMBOLS) { flush(S - block_start, block_start >= base, false); block_start = S; }
                }
                code_prev = here & CMASK;
                S++; Sv++;
            }
        }
        if (code_prev != 255u) lit_cnt += lane == code_prev ? 1u : 0u;  // the literal still waiting at the end
        flush(S - block_start, block_start >= base, true);
        if (lane == 0) a.sizes[r] = (uint32_t)(18 + (bits >> 3));
    }
}
