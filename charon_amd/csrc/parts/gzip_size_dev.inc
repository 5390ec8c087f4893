// gzip_size_dev.inc -- k_gzip_size: _tr_flush_block's arithmetic on the deflate tallies of k_gzip_tally, one lane per read
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.

// ------------------------------------------------------------------------------------------------
// The size of the gzip member zlib would write for a read = 18 bytes of header and trailer + the bits of ONE deflate block whose
// symbol frequencies k_gzip_tally counted: trees.c's build_tree / gen_bitlen / scan_tree / build_bl_tree and the stored / static /
// dynamic choice of _tr_flush_block, restated (as in charon_amd/csrc/host/gzip_size.hpp, which stays the checker:
// tests/test_gpu_parity.py::test_gzip_sizes_on_the_device_equal_the_host_arithmetic).  The algorithm is a sequential heap walk per
// read with data-dependent control flow, so it runs one LANE per read with its arrays in private memory -- some 10 000 divergent
// instructions per read, a millisecond or two per batch beside the tally kernel's 20+, and it takes 1.7 us per read off the host
// (the whole of the main thread's sizing loop at -t 1) and 640 bytes per read off the download.
// ------------------------------------------------------------------------------------------------
struct GzSizeArgs {
    const uint16_t *tallies;  // [n][GZT_WORDS]
    const uint32_t *len1, *len2;
    uint32_t n_reads;
    uint32_t *sizes;          // [n]: gzip member size in bytes, 0 = not tallied on the device (size it on the host)
    const uint32_t *long_sizes;  // [n] or null: what k_gzip_long found for the reads the tallies hand back (CHN_GZIP_SIZES_ALL)
};

namespace gzsize_dev {
enum { L_CODES = 286, D_CODES = 30, BL_CODES = 19, HEAP_SIZE = 2 * L_CODES + 1, MAX_BITS = 15, MAX_BL_BITS = 7, END_BLOCK = 256,
       REP_3_6 = 16, REPZ_3_10 = 17, REPZ_11_138 = 18 };
struct Work {
    uint32_t freq[HEAP_SIZE];  // the tree being built: leaves, then internal nodes
    uint16_t len[HEAP_SIZE], dad[HEAP_SIZE], heap[HEAP_SIZE];
    uint8_t depth[HEAP_SIZE];
    uint16_t llen[L_CODES + 2], dlen[D_CODES + 2], bllen[BL_CODES + 2];
    uint32_t blfreq[BL_CODES];
    uint64_t opt_len, static_len;
    int heap_len, heap_max;
};
__device__ __forceinline__ int extra_bits(int kind, int n) {  // n = symbol - extra_base
    if (kind == 0) return c_gz_extra_lbits[n];
    if (kind == 1) return n < 2 ? 0 : (n >> 1) - 1;
    return n < 16 ? 0 : n == 16 ? 2 : n == 17 ? 3 : 7;
}
__device__ __forceinline__ int static_len_of(int kind, int n) {  // static_ltree / static_dtree code lengths (trees.c tr_static_init)
    if (kind == 0) return n <= 143 ? 8 : n <= 255 ? 9 : n <= 279 ? 7 : 8;
    return 5;
}
__device__ __forceinline__ bool smaller(const Work &w, int n, int m) {
    return w.freq[n] < w.freq[m] || (w.freq[n] == w.freq[m] && w.depth[n] <= w.depth[m]);
}
__device__ void pqdownheap(Work &w, int k) {
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
// build_tree + gen_bitlen (trees.c): kind 0 literal/length, 1 distance, 2 bit-length tree.  w.freq[0 .. elems) holds the frequencies;
// the code lengths go to outlen[0 .. elems); returns max_code.
__device__ int build_tree(Work &w, int kind, int elems, int max_length, int extra_base, uint16_t *outlen) {
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
__device__ void scan_tree(Work &w, uint16_t *tlen, int max_code) {
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
// _tr_flush_block for one block of a deflate stream: the trees of the block's frequencies (lf [L_CODES] without END_BLOCK's count,
// which is set here; df [D_CODES]), the stored / static / dynamic choice, and the block's bits added to `bits`, the running bit count
// of the stream: a stored block pads its 3-bit header to a byte from there (buf: zlib still holds the block's bytes, `buf != NULL`);
// `last` closes the stream with bi_windup.
template <typename T>
__device__ void flush_block_bits(Work &w, const T *lf, const T *df, uint64_t stored_len, bool buf, bool last, uint64_t &bits) {
    w.opt_len = w.static_len = 0;
    for (int i = 0; i < BL_CODES; ++i) w.blfreq[i] = 0;
    // literal/length tree
    for (int i = 0; i < L_CODES; ++i) w.freq[i] = lf[i];
    w.freq[END_BLOCK] = 1;
    const int max_l = build_tree(w, 0, L_CODES, MAX_BITS, 257, w.llen);
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
}  // namespace gzsize_dev

__global__ __launch_bounds__(WAVE) void k_gzip_size(const GzSizeArgs a) {
    using namespace gzsize_dev;
    const uint32_t r = blockIdx.x * WAVE + threadIdx.x;
    if (r >= a.n_reads) return;
    const uint16_t *t = a.tallies + (size_t)r * GZT_WORDS;
    if (t[316] != 0) { a.sizes[r] = a.long_sizes ? a.long_sizes[r] : 0u; return; }
    const uint64_t stored_len = (uint64_t)a.len1[r] + (a.len2 ? a.len2[r] : 0u);
    Work w;
    uint64_t bits = 0;
    flush_block_bits(w, t, t + 286, stored_len, true, true, bits);
    a.sizes[r] = (uint32_t)(18 + (bits >> 3));
}
