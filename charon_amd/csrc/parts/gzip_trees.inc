// gzip_trees.inc -- zlib's trees.c as arithmetic: the bits of one deflate block from its symbol frequencies
// Part of the single translation unit charon_hip.hip (included in order, before gzip_walk.inc), and of host/gzip_size.hpp.
//
// ONE source for the device and the host, as in inflate_members.inc.  The size of a gzip member is a deflate_slow walk, which exists
// twice for good reason (serial and chain-based in host/gzip_size.hpp, wave-parallel in gzip_walk.inc), followed by what is here, once:
// zlib's constants (level 6, memLevel 8), the code maps of tr_static_init as functions, build_tree / gen_bitlen / scan_tree /
// build_bl_tree and the stored / static / dynamic choice of _tr_flush_block.  k_gzip_size runs it with one lane per read, lane 0 of
// k_gzip_long at every block flush, GzipSizer at every block flush of the host walk -- so every CPU comparison of GzipSizer with zlib
// (tests/test_cli_cpu.py, tools/gzip_size_check.cpp) checks the statements the kernels run.  zlib is the yardstick on both sides.
// deflate_members.inc, which writes blocks instead of sizing them, takes its trees and its choice from here too (plan_block) and its
// block header through send_tree.

#ifndef __HIPCC__  // a CPU build (the host front end, tools/gzip_size_check.cpp)
#define __host__
#define __device__
#endif

namespace gztrees {
enum {
    MIN_MATCH = 3, MAX_MATCH = 258, W_SIZE = 32768, MIN_LOOKAHEAD = MAX_MATCH + MIN_MATCH + 1, MAX_DIST = W_SIZE - MIN_LOOKAHEAD,
    TOO_FAR = 4096, GOOD_MATCH = 8, MAX_LAZY = 16, NICE_MATCH = 128, MAX_CHAIN = 128,  // configuration_table[6], deflate_slow
    LIT_BUFSIZE = 1 << (8 + 6),  // memLevel 8: a block is flushed when it holds LIT_BUFSIZE - 1 symbols
    L_CODES = 286, D_CODES = 30, BL_CODES = 19, LITERALS = 256, END_BLOCK = 256, MAX_BITS = 15, MAX_BL_BITS = 7,
    HEAP_SIZE = 2 * L_CODES + 1, REP_3_6 = 16, REPZ_3_10 = 17, REPZ_11_138 = 18
};

__host__ __device__ static inline uint32_t length_code(uint32_t lc) {  // _length_code[lc], lc = match length - MIN_MATCH
    if (lc == 255) return 28;
    if (lc < 8) return lc;
    const uint32_t hb = 31u - (uint32_t)__builtin_clz(lc);  // lc in [2^hb, 2^(hb+1)); 4 codes per power of two from 8 on
    return (hb - 1) * 4 + ((lc >> (hb - 2)) & 3u);
}
__host__ __device__ static inline uint32_t dist_code(uint32_t d) {  // d_code(d), d = match distance - 1; 2 codes per power of two from 4 on
    if (d < 4) return d;
    const uint32_t hb = 31u - (uint32_t)__builtin_clz(d);
    return hb * 2 + ((d >> (hb - 1)) & 1u);
}
// kind 0 literal/length tree (n = symbol - 257), 1 distance tree, 2 bit-length tree: extra_lbits / extra_dbits / extra_blbits
__host__ __device__ static inline int extra_bits(int kind, int n) {
    if (kind == 0) return n < 8 || n == 28 ? 0 : (n >> 2) - 1;
    if (kind == 1) return n < 2 ? 0 : (n >> 1) - 1;
    return n < 16 ? 0 : n == 16 ? 2 : n == 17 ? 3 : 7;
}
__host__ __device__ static inline int static_len_of(int kind, int n) {  // static_ltree / static_dtree code lengths
    if (kind == 0) return n <= 143 ? 8 : n <= 255 ? 9 : n <= 279 ? 7 : 8;
    return 5;
}

struct Work {
    uint32_t freq[HEAP_SIZE];  // the tree being built: leaves, then internal nodes
    uint16_t len[HEAP_SIZE], dad[HEAP_SIZE], heap[HEAP_SIZE];
    uint8_t depth[HEAP_SIZE];
    uint16_t llen[L_CODES + 2], dlen[D_CODES + 2], bllen[BL_CODES + 2];
    uint32_t blfreq[BL_CODES];
    uint64_t opt_len, static_len;
    int heap_len, heap_max;
};
__host__ __device__ static inline bool smaller(const Work &w, int n, int m) {
    return w.freq[n] < w.freq[m] || (w.freq[n] == w.freq[m] && w.depth[n] <= w.depth[m]);
}
__host__ __device__ static inline void pqdownheap(Work &w, int k) {
    const int v = w.heap[k];
    int j = k << 1;
    while (j <= w.heap_len) {
        if (j < w.heap_len && smaller(w, w.heap[j + 1], w.heap[j])) j++;
        if (smaller(w, v, w.heap[j])) break;
        w.heap[k] = w.heap[j];
        k = j;
        j <<= 1;
    }
    w.heap[k] = (uint16_t)v;
}
// build_tree + gen_bitlen: w.freq[0 .. elems) holds the frequencies; the code lengths go to outlen[0 .. elems); returns max_code.
__host__ __device__ static inline int build_tree(Work &w, int kind, int elems, int max_length, int extra_base, uint16_t *outlen) {
    int max_code = -1, node;
    w.heap_len = 0;
    w.heap_max = HEAP_SIZE;
    for (int n = 0; n < elems; ++n) {
        if (w.freq[n] != 0) { w.heap[++w.heap_len] = (uint16_t)(max_code = n); w.depth[n] = 0; }
        else w.len[n] = 0;
    }
    while (w.heap_len < 2) {  // force at least two codes of non-zero frequency
        node = w.heap[++w.heap_len] = (uint16_t)(max_code < 2 ? ++max_code : 0);
        w.freq[node] = 1;
        w.depth[node] = 0;
        w.opt_len--;
        if (kind != 2) w.static_len -= (uint64_t)static_len_of(kind, node);
    }
    for (int n = w.heap_len / 2; n >= 1; --n) pqdownheap(w, n);
    node = elems;
    do {
        const int n = w.heap[1];
        w.heap[1] = w.heap[w.heap_len--];
        pqdownheap(w, 1);
        const int m = w.heap[1];
        w.heap[--w.heap_max] = (uint16_t)n;
        w.heap[--w.heap_max] = (uint16_t)m;
        w.freq[node] = w.freq[n] + w.freq[m];
        w.depth[node] = (uint8_t)((w.depth[n] >= w.depth[m] ? w.depth[n] : w.depth[m]) + 1);
        w.dad[n] = w.dad[m] = (uint16_t)node;
        w.heap[1] = (uint16_t)node++;
        pqdownheap(w, 1);
    } while (w.heap_len >= 2);
    w.heap[--w.heap_max] = w.heap[1];
    // gen_bitlen
    uint16_t bl_count[MAX_BITS + 1];
    int h, overflow = 0;
    for (int bits = 0; bits <= MAX_BITS; ++bits) bl_count[bits] = 0;
    w.len[w.heap[w.heap_max]] = 0;
    for (h = w.heap_max + 1; h < HEAP_SIZE; ++h) {
        const int n = w.heap[h];
        int bits = w.len[w.dad[n]] + 1;
        if (bits > max_length) { bits = max_length; overflow++; }
        w.len[n] = (uint16_t)bits;
        if (n > max_code) continue;  // not a leaf
        bl_count[bits]++;
        int xbits = 0;
        if (n >= extra_base) xbits = extra_bits(kind, n - extra_base);
        w.opt_len += (uint64_t)w.freq[n] * (unsigned)(bits + xbits);
        if (kind != 2) w.static_len += (uint64_t)w.freq[n] * (unsigned)(static_len_of(kind, n) + xbits);
    }
    if (overflow != 0) {
        do {
            int bits = max_length - 1;
            while (bl_count[bits] == 0) bits--;
            bl_count[bits]--;
            bl_count[bits + 1] += 2;
            bl_count[max_length]--;
            overflow -= 2;
        } while (overflow > 0);
        for (int bits = max_length; bits != 0; --bits) {
            int n = bl_count[bits];
            while (n != 0) {
                const int m = w.heap[--h];
                if (m > max_code) continue;
                if ((unsigned)w.len[m] != (unsigned)bits) {
                    w.opt_len += ((uint64_t)bits - w.len[m]) * w.freq[m];
                    w.len[m] = (uint16_t)bits;
                }
                n--;
            }
        }
    }
    for (int n = 0; n <= max_code; ++n) outlen[n] = w.len[n];
    for (int n = max_code + 1; n < elems; ++n) outlen[n] = 0;
    return max_code;
}
__host__ __device__ static inline void scan_tree(Work &w, uint16_t *tlen, int max_code) {
    int prevlen = -1, curlen, nextlen = tlen[0], count = 0, max_count = 7, min_count = 4;
    if (nextlen == 0) { max_count = 138; min_count = 3; }
    tlen[max_code + 1] = (uint16_t)0xffff;  // guard
    for (int n = 0; n <= max_code; ++n) {
        curlen = nextlen;
        nextlen = tlen[n + 1];
        if (++count < max_count && curlen == nextlen) continue;
        else if (count < min_count) w.blfreq[curlen] += (uint32_t)count;
        else if (curlen != 0) {
            if (curlen != prevlen) w.blfreq[curlen]++;
            w.blfreq[REP_3_6]++;
        } else if (count <= 10) w.blfreq[REPZ_3_10]++;
        else w.blfreq[REPZ_11_138]++;
        count = 0;
        prevlen = curlen;
        if (nextlen == 0) { max_count = 138; min_count = 3; }
        else if (curlen == nextlen) { max_count = 6; min_count = 3; }
        else { max_count = 7; min_count = 4; }
    }
}
// send_tree: the code-length sequence tlen[0 .. max_code] as scan_tree counted it, sent through `s`: s.bl(sym) sends the bit-length
// code of sym, s.bits(value, n) n plain bits (deflate_members.inc writes them; the sizers only count and never call this)
template <class S> __host__ __device__ static inline void send_tree(S &s, uint16_t *tlen, int max_code) {
    int prevlen = -1, curlen, nextlen = tlen[0], count = 0, max_count = 7, min_count = 4;
    if (nextlen == 0) { max_count = 138; min_count = 3; }
    tlen[max_code + 1] = (uint16_t)0xffff;  // guard, as scan_tree left it
    for (int n = 0; n <= max_code; ++n) {
        curlen = nextlen;
        nextlen = tlen[n + 1];
        if (++count < max_count && curlen == nextlen) continue;
        else if (count < min_count) { do { s.bl(curlen); } while (--count != 0); }
        else if (curlen != 0) {
            if (curlen != prevlen) { s.bl(curlen); count--; }
            s.bl(REP_3_6); s.bits((uint32_t)(count - 3), 2);
        } else if (count <= 10) { s.bl(REPZ_3_10); s.bits((uint32_t)(count - 3), 3); }
        else { s.bl(REPZ_11_138); s.bits((uint32_t)(count - 11), 7); }
        count = 0;
        prevlen = curlen;
        if (nextlen == 0) { max_count = 138; min_count = 3; }
        else if (curlen == nextlen) { max_count = 6; min_count = 3; }
        else { max_count = 7; min_count = 4; }
    }
}
// The steps of flush_block_bits (below) up to its choice, for a caller that goes on to WRITE the block (deflate_members.inc): the
// block's frequencies are lf [L_CODES] without END_BLOCK's count, which is set here, and df [D_CODES].  Leaves the code lengths in
// w.llen / w.dlen / w.bllen and the bit counts in w.opt_len / w.static_len (both without the 3 header bits); opt_lenb is the smaller of
// the two byte counts, as in zlib.  (flush_block_bits keeps its own statement of these calls: the sizers' kernels are tuned around
// the code it compiles to.)
struct BlockPlan { int max_l, max_d, max_blindex; uint64_t opt_lenb, static_lenb; };
template <typename T>
__host__ __device__ static inline BlockPlan plan_block(Work &w, const T *lf, const T *df) {
    BlockPlan b;
    w.opt_len = w.static_len = 0;
    for (int i = 0; i < BL_CODES; ++i) w.blfreq[i] = 0;
    // literal/length tree
    for (int i = 0; i < L_CODES; ++i) w.freq[i] = lf[i];
    w.freq[END_BLOCK] = 1;
    b.max_l = build_tree(w, 0, L_CODES, MAX_BITS, LITERALS + 1, w.llen);
    // distance tree
    for (int i = 0; i < D_CODES; ++i) w.freq[i] = df[i];
    b.max_d = build_tree(w, 1, D_CODES, MAX_BITS, 0, w.dlen);
    // bit-length tree over the two code-length sequences
    scan_tree(w, w.llen, b.max_l);
    scan_tree(w, w.dlen, b.max_d);
    for (int i = 0; i < BL_CODES; ++i) w.freq[i] = w.blfreq[i];
    (void)build_tree(w, 2, BL_CODES, MAX_BL_BITS, 0, w.bllen);
    const uint8_t order[BL_CODES] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (b.max_blindex = BL_CODES - 1; b.max_blindex >= 3; --b.max_blindex)
        if (w.bllen[order[b.max_blindex]] != 0) break;
    w.opt_len += 3 * ((uint64_t)b.max_blindex + 1) + 5 + 5 + 4;
    b.opt_lenb = (w.opt_len + 3 + 7) >> 3;
    b.static_lenb = (w.static_len + 3 + 7) >> 3;
    if (b.static_lenb <= b.opt_lenb) b.opt_lenb = b.static_lenb;
    return b;
}
// _tr_flush_block for one block of a deflate stream: the trees of the block's frequencies (lf [L_CODES] without END_BLOCK's count,
// which is set here; df [D_CODES]), the stored / static / dynamic choice, and the block's bits added to `bits`, the running bit count
// of the stream: a stored block pads its 3-bit header to a byte from there (buf: zlib still holds the block's bytes, `buf != NULL`);
// `last` closes the stream with bi_windup.
template <typename T>
__host__ __device__ static inline void flush_block_bits(Work &w, const T *lf, const T *df, uint64_t stored_len, bool buf, bool last, uint64_t &bits) {
    w.opt_len = w.static_len = 0;
    for (int i = 0; i < BL_CODES; ++i) w.blfreq[i] = 0;
    // literal/length tree
    for (int i = 0; i < L_CODES; ++i) w.freq[i] = lf[i];
    w.freq[END_BLOCK] = 1;
    const int max_l = build_tree(w, 0, L_CODES, MAX_BITS, LITERALS + 1, w.llen);
    // distance tree
    for (int i = 0; i < D_CODES; ++i) w.freq[i] = df[i];
    const int max_d = build_tree(w, 1, D_CODES, MAX_BITS, 0, w.dlen);
    // bit-length tree over the two code-length sequences
    scan_tree(w, w.llen, max_l);
    scan_tree(w, w.dlen, max_d);
    for (int i = 0; i < BL_CODES; ++i) w.freq[i] = w.blfreq[i];
    (void)build_tree(w, 2, BL_CODES, MAX_BL_BITS, 0, w.bllen);
    const uint8_t bl_order[BL_CODES] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int max_blindex;
    for (max_blindex = BL_CODES - 1; max_blindex >= 3; --max_blindex)
        if (w.bllen[bl_order[max_blindex]] != 0) break;
    w.opt_len += 3 * ((uint64_t)max_blindex + 1) + 5 + 5 + 4;
    uint64_t opt_lenb = (w.opt_len + 3 + 7) >> 3;
    const uint64_t static_lenb = (w.static_len + 3 + 7) >> 3;
    if (static_lenb <= opt_lenb) opt_lenb = static_lenb;
    if (stored_len + 4 <= opt_lenb && buf) bits = ((bits + 3 + 7) & ~7ULL) + 32 + 8 * stored_len;  // 3 header bits padded to a byte, LEN + NLEN, the bytes
    else if (static_lenb == opt_lenb) bits += 3 + w.static_len;
    else bits += 3 + w.opt_len;
    if (last) bits = (bits + 7) & ~7ULL;  // bi_windup
}
}  // namespace gztrees
