// text_pack.inc -- k_text_pack / k_text_mq: reads as plain text (one byte per base, phred characters) -> the packed batch
// (2-bit codes, N mask, mean quality) that the chain reads; what the host packers (charon_amd/pack.py::pack_reads,
// HostBatch::pack in host/dehost.inc) write, bit for bit.
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.
//
// Work is mapped by OUTPUT: one lane per 16 bases = one dword of `bases2`, four lanes per 64-base chunk, two neighbouring lanes
// per dword of `nmask`.  Every dword of both arrays up to n_bases is written, the padding behind a segment as zero, so a recycled
// buffer keeps nothing of the batch before.  The read a lane belongs to is found by binary search in the padded segment offsets:
// once per wavefront for its first and its last lane (all lanes fetch the same one or two addresses), then per lane between those
// two results -- no step at all where the wavefront lies inside one long read, about four where it spans 16 short ones.
// A read's letters start at any byte offset: a lane fetches the (at most five) ALIGNED dwords that cover its 16 bytes and shifts
// them into place (v_alignbit), so it touches at most 3 bytes before and behind its stretch -- the text buffer carries 64 bytes
// of padding at both ends.  Descriptors are range-checked on the host before the launch.
// Two texts (chn_text_batch2.text2: the two files of paired input in two device buffers): mate 2's letters and qualities are read from
// TextPackArgs.text2, which the host sets to `text` for a batch with one text -- one code path, the mate picks the base pointer.
// Qualities: the lane of bases [p, p + 16) of a mate sums the quality bytes [p, p + 16) of that mate; a quality string longer than
// its sequence (or one without a sequence) is finished by the read's first lane, byte by byte.  The partial sums of a read are
// added up over the lanes of the wavefront that hold it (segmented shuffle reduction) before the one integer atomic per read and
// wavefront; k_text_mq then divides once per read.

struct TextPackArgs {
    const uint8_t *text;                 // 4-byte aligned, 64 bytes of padding before and behind
    const uint8_t *text2;                // the text that holds mate 2: `text` again unless the batch has two texts
    const uint64_t *off1, *off2;         // padded segment offsets in bases (off2 NULL: single-end)
    const uint32_t *len1, *len2;
    const uint64_t *so1, *so2;           // byte offsets of the letters
    const uint64_t *qo1, *qo2;           // byte offsets of the qualities (NULL: none)
    const uint32_t *ql1, *ql2;
    uint32_t n_reads;
    uint64_t n_bases;
    uint32_t *bases, *nmask;
    int *qsum;                           // [n_reads], zeroed: sum of (signed char)q - 33
    uint32_t *ctl;                       // [0] has_n, [1] illegal bytes, [2] smallest read index with one (0xFFFFFFFF: none)
};
enum { TXT_HAS_N = 0, TXT_ILLEGAL = 1, TXT_FIRST_BAD = 2, TXT_CTL_WORDS = 4 };

// the 16 bytes at text + addr as four dwords; only dwords that hold one of the `count` bytes are fetched
__device__ __forceinline__ void text_fetch16(const uint8_t *text, uint64_t addr, uint32_t count, uint32_t w[4]) {
    const uint32_t *a = reinterpret_cast<const uint32_t *>(text + (addr & ~(uint64_t)3));
    const uint32_t skew = (uint32_t)addr & 3u, span = skew + count;
    uint32_t d[5];
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k) d[k] = 4 * k < span ? a[k] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) w[k] = __funnelshift_r(d[k], d[k + 1], 8 * skew);
}

// last i in [lo, hi] with off[i] <= b (off[lo] <= b holds)
__device__ __forceinline__ uint32_t text_find(const uint64_t *off, uint32_t lo, uint32_t hi, uint64_t b) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// letters A C G T U N R Y S W K M B D H V as bits of (letter - 'A')
#define TXT_BIT(c) (1u << ((c) - 'A'))
#define TXT_ACGTU (TXT_BIT('A') | TXT_BIT('C') | TXT_BIT('G') | TXT_BIT('T') | TXT_BIT('U'))
#define TXT_AMBIG (TXT_BIT('N') | TXT_BIT('R') | TXT_BIT('Y') | TXT_BIT('S') | TXT_BIT('W') | TXT_BIT('K') | TXT_BIT('M') | TXT_BIT('B') | \
                   TXT_BIT('D') | TXT_BIT('H') | TXT_BIT('V'))

template <bool RANKS>
__global__ __launch_bounds__(256) void k_text_pack(const TextPackArgs a) {
    const uint64_t lane_g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t n_lanes = a.n_bases >> 4;
    const bool active = lane_g < n_lanes;
    const uint64_t b = (active ? lane_g : n_lanes - 1) << 4;  // first base of this lane
    // the wavefront's first and last lane (wavefronts are aligned to 64 lanes)
    const uint64_t wave_b0 = (lane_g & ~(uint64_t)63) << 4;
    const uint64_t wave_b1 = ((lane_g | 63) < n_lanes ? (lane_g | 63) : n_lanes - 1) << 4;
    const uint32_t ends = text_find(a.off1, 0, a.n_reads - 1, lane_id() < 32 ? wave_b0 : wave_b1);
    const uint32_t r_lo = (uint32_t)__shfl((int)ends, 0), r_hi = (uint32_t)__shfl((int)ends, 63);
    const uint32_t r = text_find(a.off1, r_lo, r_hi, b);

    // segment of this lane: mate 2 from off2[r] on
    uint64_t so = a.off1[r], to = a.so1[r];
    uint32_t L = a.len1[r], mate = 0;
    if (a.off2 && b >= a.off2[r]) { so = a.off2[r]; to = a.so2[r]; L = a.len2[r]; mate = 1; }
    const uint64_t p = b - so;  // a multiple of 16; >= L in the padding
    const uint32_t count = active && p < L ? (L - p < 16 ? (uint32_t)(L - p) : 16u) : 0u;
    const uint8_t *tx = mate ? a.text2 : a.text;  // the text this lane's mate lies in

    uint32_t codes = 0, nb = 0, bad = 0;
    if (count) {
        uint32_t w[4];
        text_fetch16(tx, to + p, count, w);
#pragma unroll
        for (uint32_t j = 0; j < 16; ++j) {
            const uint32_t c = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
            if (j < count) {
                if (RANKS) {  // seqan3 dna5 ranks: 0 A, 1 C, 2 G, 3 N, 4 T
                    if (c == 3) nb |= 1u << j;
                    else if (c <= 4) codes |= (c == 4 ? 3u : c) << (2 * j);
                    else ++bad;
                } else {
                    const uint32_t u = (c & 0xDFu) - 'A';  // either case -> 0 .. 25 for a letter ((c & 0xDF) == X only for X and x)
                    const uint32_t bit = u < 26 ? 1u << u : 0u;
                    if (bit & TXT_ACGTU) { const uint32_t t = (c >> 1) & 3u; codes |= (t ^ (t >> 1)) << (2 * j); }  // A0 C1 T2 G3 -> A0 C1 G2 T3; U as T
                    else if (bit & TXT_AMBIG) nb |= 1u << j;
                    else ++bad;
                }
            }
        }
    }
    if (active) a.bases[lane_g] = codes;
    const uint32_t nb_hi = (uint32_t)__shfl_xor((int)nb, 1);
    if (active && !(lane_g & 1)) a.nmask[lane_g >> 1] = nb | (nb_hi << 16);
    if (__ballot(nb != 0) && lane_id() == 0) a.ctl[TXT_HAS_N] = 1u;  // (every writer stores the same value)
    if (bad) {
        atomicAdd(&a.ctl[TXT_ILLEGAL], bad);
        atomicMin(&a.ctl[TXT_FIRST_BAD], r);
    }

    if (!a.qo1 && !a.qo2) return;
    // ---- quality sums ----
    int sum = 0;
    const uint64_t *qo = mate ? a.qo2 : a.qo1;
    const uint32_t *ql = mate ? a.ql2 : a.ql1;
    const uint32_t Q = (active && qo) ? ql[r] : 0u;
    // (p < L: only lanes that hold bases take a piece; the rest of a longer quality string goes to the read's first lane below)
    const uint32_t nq = count && p < Q ? (Q - p < 16 ? (uint32_t)(Q - p) : 16u) : 0u;
    if (nq) {
        uint32_t w[4];
        text_fetch16(tx, qo[r] + p, nq, w);
#pragma unroll
        for (uint32_t j = 0; j < 16; ++j)
            if (j < nq) sum += (int)(signed char)((w[j >> 2] >> (8 * (j & 3))) & 0xffu) - 33;
    }
    // the read's first lane: mate 1's first piece, or mate 2's where mate 1 has no letters
    if (count && p == 0 && (mate == 0 || a.len1[r] == 0)) {
        for (uint32_t m = 0; m < (a.off2 ? 2u : 1u); ++m) {
            const uint64_t *xo = m ? a.qo2 : a.qo1;
            if (!xo) continue;
            const uint32_t xq = (m ? a.ql2 : a.ql1)[r], xl = (m ? a.len2 : a.len1)[r];
            const uint64_t covered = ((uint64_t)xl + 15) & ~(uint64_t)15;
            const uint8_t *q = (m ? a.text2 : a.text) + xo[r];
            for (uint64_t j = covered; j < xq; ++j) sum += (int)(signed char)q[j] - 33;
        }
    }
    // add up over the lanes of this wavefront that hold the same segment (they are contiguous; the segment's first base names it), then
    // one atomic by the first of them
    const unsigned long long key = count ? (unsigned long long)so : ~0ull;
#pragma unroll
    for (uint32_t o = 1; o < WAVE; o <<= 1) {
        const int t = __shfl_down(sum, o);
        const unsigned long long k = __shfl_down(key, o);
        if (lane_id() + o < WAVE && k == key) sum += t;
    }
    const unsigned long long prev = __shfl_up(key, 1);
    if (count && (lane_id() == 0 || prev != key) && sum != 0) atomicAdd(&a.qsum[r], sum);
}

// mean quality of every read, in place: int sum -> float(sum) / float(count) (src/dehost_main.cpp:355-360), 0 without qualities
__global__ __launch_bounds__(256) void k_text_mq(int *qsum, const uint32_t *ql1, const uint32_t *ql2, uint32_t n_reads) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_reads) return;
    const uint64_t cnt = (uint64_t)(ql1 ? ql1[i] : 0u) + (ql2 ? ql2[i] : 0u);
    const int s = qsum[i];
    reinterpret_cast<float *>(qsum)[i] = cnt ? static_cast<float>(s) / static_cast<float>(cnt) : 0.0f;
}
