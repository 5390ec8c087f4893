// gzip_tally_long.inc -- k_gzip_long: zlib level-6 deflate_slow of reads of ANY length (window slide, any number of deflate blocks),
// each block sized in place: the gzip member size of every read (chn_batch.gzip_output = CHN_GZIP_SIZES_ALL)
// Part of the single translation unit charon_hip.hip (included in order, after gzip_trees.inc, gzip_walk.inc, gzip_tally.inc and gzip_size_dev.inc); not a stand-alone source.

// ------------------------------------------------------------------------------------------------
// The walk of gzip_walk.inc, which k_gzip_tally instantiates too (one wavefront per read, the trigram classes as arrays, the
// wave-parallel longest_match with one DPP max-reduction, the tallies in registers, 4-bit codes with an N in the batch and 2-bit
// codes without), with what a read of any length needs around it.  Every statement follows the host emulator's deflate_slow (charon_amd/csrc/host/gzip_size.hpp, run()):
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
//    at once by lane 0 with _tr_flush_block's arithmetic (gztrees::flush_block_bits, the one k_gzip_size and the host emulator run; its heap in LDS),
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

__host__ __device__ constexpr size_t gzl_work_bytes() { return (sizeof(gztrees::Work) + 15) & ~(size_t)15; }
constexpr size_t gzl_lds_bytes(int bits) {
    return (size_t)GZL_HEAD_WORDS * 4 + gzl_work_bytes() + ((size_t)GZL_EPOCH * GZL_RING_EPOCHS * bits / 32 + GZL_GUARD) * 4;
}
// the figures of the head comment: they decide two / three wavefronts per CU
static_assert(gzl_work_bytes() == 7088 && gzl_lds_bytes(4) == 75968 && gzl_lds_bytes(2) == 43200, "k_gzip_long's LDS must not move");

template <int BITS>
__global__ __launch_bounds__(WAVE) void k_gzip_long(const GzlArgs a) {
    constexpr uint32_t MIN_MATCH = gztrees::MIN_MATCH, MAX_DIST = gztrees::MAX_DIST, W_SIZE = GZL_EPOCH, MIN_LOOKAHEAD = gztrees::MIN_LOOKAHEAD;
    constexpr uint32_t FIRST = GzCodes<BITS>::FIRST;
    constexpr uint32_t EPW = GZL_EPOCH / GzCodes<BITS>::CPW, RWORDS = EPW * GZL_RING_EPOCHS, RMASK = RWORDS - 1u;
    extern __shared__ __align__(16) unsigned char gsm[];
    const uint32_t lane = lane_id();
    uint32_t *tall = reinterpret_cast<uint32_t *>(gsm);  // [320] the block's tallies (long match lengths during the walk, everything at a flush)
    uint32_t *ccur = tall + GZT_WORDS, *cst = ccur + 128, *pst = cst + 128, *pen = pst + 128;
    gztrees::Work *work = reinterpret_cast<gztrees::Work *>(gsm + GZL_HEAD_WORDS * 4);
    uint32_t *ring = reinterpret_cast<uint32_t *>(gsm + GZL_HEAD_WORDS * 4 + gzl_work_bytes());
    GzCodeReader<BITS, GzRingStore<BITS, RMASK>> codes{ring, 0u};
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
        bool take = !gz_segments_outside(a.off1, a.off2, l1, l2, a.n_bases, r) && n64 != 0 && n64 <= a.bound && n64 <= GZL_MAX_READ;
        if (a.filter == GZL_HANDED_BACK) take = take && n64 <= a.short_max && a.tallies[(size_t)r * GZT_WORDS + 316] != 0;
        if (!take) continue;
        const uint32_t n = (uint32_t)n64;
        const uint64_t o1 = a.off1[r], o2 = a.off2 ? a.off2[r] : 0;
        const uint32_t *b1 = a.bases + (o1 >> 4), *b2 = a.off2 ? a.bases + (o2 >> 4) : nullptr;
        const uint32_t *m1 = a.nmask ? a.nmask + (o1 >> 5) : nullptr, *m2 = (a.nmask && a.off2) ? a.nmask + (o2 >> 5) : nullptr;
        // the codes of epoch e into the ring (the first words again behind its end)
        auto load_epoch = [&](uint32_t e) {
            for (uint32_t wi = lane; wi < EPW; wi += WAVE) {
                const uint32_t gw = e * EPW + wi, word = gz_pack_codes<BITS>(gw, b1, b2, m1, m2, l1, n);
                const uint32_t w = gw & RMASK;
                ring[w] = word;
                if (w < GZL_GUARD) ring[RWORDS + w] = word;
            }
        };
        const uint32_t m = n >= 3 ? n - 2 : 0;  // positions 0 .. n-3 enter the dictionary
        // the class arrays of epoch e (its codes and the first two of epoch e + 1 are in the ring); the previous epoch's class
        // ranges move to pst / pen
        auto build_epoch = [&](uint32_t e) {
            for (uint32_t k = lane; k < 128; k += WAVE) {
                pst[k] = e ? cst[k] : 0u;
                pen[k] = e ? ccur[k] : 0u;  // (the cursor ended at the class's end)
                ccur[k] = 0;
            }
            __syncthreads();
            gz_build_classes<BITS>(codes, lane, e * GZL_EPOCH, min(m, e * GZL_EPOCH + GZL_EPOCH), occ + (e & 1u) * GZL_EPOCH, pinfo, ccur, cst);
        };

        codes.pin_base();
        uint32_t S = 0, ML = MIN_MATCH - 1, MS = 0, W0 = 0;
        uint32_t Sv = 0;  // S, per lane
        asm volatile("" : "+v"(Sv));
        GzTallies t = {0, 0, 0, 255};
        uint32_t nsym = 0, block_start = 0;               // symbols of the current block; where it starts
        uint32_t base = 0, loaded_end = min(n, 2u * W_SIZE);  // zlib's window: its start, the end of what fill_window has read
        uint32_t ep_end = 0, E0 = 0, P1 = 0, ebuf = 0, pbuf = 0;  // the epoch of the class arrays: [E0, ep_end), positions entered below P1
        uint32_t pw = 0;
        uint64_t bits = 0;  // the member's deflate bits so far (lane 0)
        // a block's record into LDS, sized by lane 0 (_tr_flush_block), tallies cleared
        auto flush = [&](uint32_t stored_len, bool buf, bool last) {
            gz_store_tallies(t, tall, lane);
            __syncthreads();
            if (lane == 0) gztrees::flush_block_bits(*work, tall, tall + 286, stored_len, buf, last, bits);
            __syncthreads();
            for (uint32_t i = lane; i < GZT_WORDS; i += WAVE) tall[i] = 0;
            __syncthreads();
            t.lit_cnt = t.len_cnt = t.dist_cnt = 0;
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
            uint32_t here, next8;
            codes.fetch(Sv, here, next8);
            // the chain: rsE entries of this epoch, then the class's entries of the previous epoch (older ones are beyond MAX_DIST)
            const bool enters = S < m;
            const uint32_t k = enters ? gz_key_of<BITS>(here) : 0u;
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
                // (positions are absolute: a candidate is packed as its distance from the bottom of the 16 bits, the more recent the larger)
                const uint32_t mx = gz_longest_match<BITS>(codes, lane, S, next8, curA, curB, curA + 65536u - S, curB + 65536u - S, okA, okB, kk, PL, look, look < FIRST + 4u);
                uint32_t best = PL;
                if ((mx >> 16) + 3u > best) { best = (mx >> 16) + 3u; MS = S + (mx & 0xFFFFu) - 65536u; }
                ML = best <= look ? best : look;
                if (ML == MIN_MATCH) { if (S - MS > gztrees::TOO_FAR) ML = MIN_MATCH - 1; }
            }
            const uint32_t kind = gz_emit<BITS>(t, tall, lane, PL, PM, here, S, Sv, ML);
            if (kind != GZ_NOTHING && ++nsym == gztrees::LIT_BUFSIZE - 1) {
                // zlib flushes right behind the tally: a match has moved strstart on by then, a literal has not yet
                const uint32_t at = kind == GZ_LITERAL ? S - 1u : S;
                flush(at - block_start, block_start >= base, false);
                block_start = at;
            }
        }
        if (t.code_prev != 255u) t.lit_cnt += lane == t.code_prev ? 1u : 0u;  // the literal still waiting at the end
        flush(S - block_start, block_start >= base, true);
        if (lane == 0) a.sizes[r] = (uint32_t)(18 + (bits >> 3));
    }
}
