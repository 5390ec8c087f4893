// gzip_tally.inc -- k_gzip_tally: zlib level-6 deflate_slow of every read of a batch, as symbol TALLIES (SURVEY 8(f) item 3)
// Part of the single translation unit charon_hip.hip (included in order, after gzip_walk.inc: the walk itself, shared with k_gzip_long);
// not a stand-alone source.

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
//      with the one _tr_flush_block restatement (gzip_trees.inc, through GzipSizer::size_from_tallies of host/gzip_size.hpp) -- a
//      few microseconds per read instead of ~70 -- or k_gzip_size does on the device.
// Scope: A/C/G/T/N letters, 1 <= n <= GZT_MAX_LEN, one deflate block (fewer than 16 383 symbols), no window slide
// (n < 65 274 is implied).  Anything else is flagged and sized on the host.  Exactness is established against zlib:
// tests/test_gpu_parity.py::test_gzip_sizes_on_the_device_equal_zlib, tests/test_gpu_gzip_any_length.py.
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

// BITS: 4 = dna5 codes (A C G T N) with 0xF behind the data; 2 = a batch without N: the codes as they are packed in the batch, sixteen to a word --
// half the LDS (twice the wavefronts on a CU for reads beyond 9 000 letters) and sixteen letters per comparison; nothing marks the end of
// the data, so the general rule cuts every candidate's length at the lookahead (zlib compares against the zeroed window behind the data: a
// mismatch at n, whatever the candidate holds there).
template <int BITS>
__global__ __launch_bounds__(WAVE) void k_gzip_tally(const GztArgs a) {
    constexpr uint32_t FIRST = GzCodes<BITS>::FIRST, MIN_MATCH = gztrees::MIN_MATCH, MAX_DIST = gztrees::MAX_DIST;
    extern __shared__ __align__(16) unsigned char gsm[];
    const uint32_t lane = lane_id();
    // LDS (sized for max_len on the host): 1 280 bytes + half a byte per letter
    uint32_t *tall = reinterpret_cast<uint32_t *>(gsm);  // [320] the tallies as they leave; while the classes are built: class cursors [0, 128), class starts [128, 256)
    uint32_t *cs4 = tall + GZT_WORDS;                    // the codes, BITS each (4: 0xF behind the data; 2: zeros), the whole read from word 0 on
    GzCodeReader<BITS, GzFlatStore<BITS>> codes{cs4, 0u};
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
        if (n == 0 || n > a.max_len || n > GZT_MAX_LEN || gz_segments_outside(a.off1, a.off2, l1, l2, a.n_bases, r)) {
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
        for (uint32_t wi = lane; wi < nwords; wi += WAVE) cs4[wi] = gz_pack_codes<BITS>(wi, b1, b2, m1, m2, l1, n);
        __syncthreads();
        const uint32_t m = n >= 3 ? n - 2 : 0;  // positions 0 .. n-3 enter the dictionary
        // 1b, 1c. the classes of the whole read (cursors and starts where the tallies will be)
        gz_build_classes<BITS>(codes, lane, 0u, m, occ, pinfo, tall, tall + 128);
        for (uint32_t i = lane; i < GZT_WORDS; i += WAVE) tall[i] = 0;  // the builder's cursors lived here
        __syncthreads();

        // 2. deflate_slow (deflate.c), level 6: max_lazy 16, good_match 8, nice_match 128, max_chain 128.  The walk is wave-uniform and instruction
        // issue is what bounds it (scalar and vector instructions alike), so the step is written for few instructions: whatever costs nothing
        // extra per lane is done per lane (the position again in a vector register for LDS addresses and shift counts, the distance code, the
        // tallies), and the common case of longest_match is one max-reduction (gz_longest_match).
        codes.pin_base();
        // steps that need the general rule whatever the candidates look like: the last positions (nice_match = lookahead, within reach of the
        // first comparison there) and positions with candidates beyond the window
        const uint32_t rare_from = n >= FIRST + 4u ? min(n - (FIRST + 4u), MAX_DIST) : 0u;
        uint32_t S = 0, ML = MIN_MATCH - 1, MS = 0, W0 = 0, n_long = 0;
        uint32_t Sv = 0;                                  // S, per lane
        asm volatile("" : "+v"(Sv));
        GzTallies t = {0, 0, 0, 255};
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
            uint32_t here, next8;
            codes.fetch(Sv, here, next8);
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
                const uint32_t mx = gz_longest_match<BITS>(codes, lane, S, next8, curA, curB, curA, curB, okA, okB, kk, PL, look, S > rare_from);
                uint32_t best = PL;
                if ((mx >> 16) + 3u > best) { best = (mx >> 16) + 3u; MS = mx & 0xFFFFu; }
                ML = best <= look ? best : look;
                if (ML == MIN_MATCH) { if (S - MS > gztrees::TOO_FAR) ML = MIN_MATCH - 1; }
            }
            if (gz_emit<BITS>(t, tall, lane, PL, PM, here, S, Sv, ML) == GZ_LONG_MATCH) ++n_long;  // (not in len_cnt)
        }
        // 3. out: a second deflate block (lit_bufsize - 1 = 16 383 symbols reached inside the loop) is sized on the host
        uint32_t nsym = t.lit_cnt + t.len_cnt;
        for (int o = 32; o > 0; o >>= 1) nsym += (uint32_t)__shfl_xor((int)nsym, o);
        const bool too_many = nsym + n_long >= GZT_SYMBOL_LIMIT;
        t.lit_cnt += lane == t.code_prev ? 1u : 0u;  // the literal still waiting at the end
        gz_store_tallies(t, tall, lane);
        if (lane == 5) tall[256] = 1;  // END_BLOCK
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
