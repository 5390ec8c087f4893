// text_split.inc -- FASTQ records found in a text that lies in device memory (chn_text_split), and the same rule on the CPU
// (chn_text_split_host)
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.
//
// ONE rule source for the device and the host, as the decoder (inflate_members.inc) and the compressor are written: tsp_record is
// __host__ __device__ code that decides from the starts of five consecutive lines whether the four lines between them are a plain
// four-line record, and fills its descriptor.  It accepts exactly what BlockReader::dry_record (host/fastx_reader.inc) accepts:
//   - the first byte is '@';
//   - the sequence line, after dropping one trailing '\r', has length n >= 1 and does not begin with '+';
//   - the third line begins with '+';
//   - the fourth line, after dropping one trailing '\r', has length n;
//   - the id is what follows '@' up to the line end, minus one trailing '\r' (it may be empty).
// That four line feeds follow inside [start, text_bytes) is what having five line starts means.  Records are taken one behind the
// other from `start` until the rule fails or max_records is reached; what lies behind is the caller's business.
//
// The host applies the rule record by record (tsp_host_job, the body of chn_text_split_host).  The device finds every line start
// first -- count the line feeds per 4 KiB tile, scan the counts, rank the line feeds -- and then lets one lane per CANDIDATE record r
// judge lines 4r .. 4r + 3.  A candidate behind the first failing one is not aligned to real records and is ignored: record r is real
// if records 0 .. r - 1 are, which is the induction split_in_parallel (host/fastx_reader.inc) uses for its pieces.
//
// Device text contract (also CHN_TEXT_ON_DEVICE): `text` is 16-byte aligned and readable up to text_bytes rounded up to 16, so every
// lane may fetch the aligned 16-byte piece that holds a wanted byte.  Bytes outside [start, text_bytes) are masked, never judged.
// Every store is a plain store; every loop runs over tiles, pieces or records, none over data.

#ifndef __HIPCC__  // a CPU build of the rule and the host walk alone (tools/fuzz/text_split_fuzz.cpp)
#define __host__
#define __device__
#endif

static const uint32_t TSP_TILE = 4096;  // bytes a wavefront counts and ranks at a time: four rounds of 64 lanes x 16 bytes

struct TspRecord {
    uint64_t id_off, seq_off, qual_off;
    uint32_t id_len, seq_len;
};

// the rule.  ls[k] is the first byte of line k of the candidate, ls[k + 1] - 1 its line feed (k = 0 .. 3); all five lie in the text
__host__ __device__ static inline bool tsp_record(const uint8_t *text, const uint64_t ls[5], TspRecord &r) {
    if (text[ls[0]] != '@') return false;  // (an empty first line holds its line feed here)
    uint64_t idn = ls[1] - 1 - ls[0] - 1;
    if (idn && text[ls[0] + idn] == '\r') --idn;
    const uint64_t raw1 = ls[2] - 1 - ls[1];
    uint64_t n1 = raw1;
    if (n1 && text[ls[1] + n1 - 1] == '\r') --n1;
    if (n1 == 0 || text[ls[1]] == '+' || raw1 > 0xFFFFFFF0ull) return false;
    if (text[ls[2]] != '+') return false;
    uint64_t n3 = ls[4] - 1 - ls[3];
    if (n3 && text[ls[3] + n3 - 1] == '\r') --n3;
    if (n3 != n1) return false;
    r.id_off = ls[0] + 1; r.id_len = (uint32_t)idn;
    r.seq_off = ls[1]; r.seq_len = (uint32_t)n1;
    r.qual_off = ls[3];
    return true;
}

// The checks both calls make on a job before anything else; `why` names the first that fails.  0 or a CHN_E_* code.
static int tsp_check_job(const chn_text_split_job *j, const char *who, std::string &why) {
    const std::string W(who);
    if (!j) { why = W + ": null job"; return CHN_E_INVALID; }
    if (j->struct_size != sizeof(chn_text_split_job)) { why = W + ": bad struct_size"; return CHN_E_INVALID; }
    if (j->flags) { why = W + ": unknown flag"; return CHN_E_INVALID; }
    if (j->start > j->text_bytes) { why = W + ": start lies behind text_bytes"; return CHN_E_INVALID; }
    if (j->max_records && (!j->id_offset || !j->id_length || !j->seq_offset || !j->seq_length || !j->qual_offset)) { why = W + ": a descriptor array is NULL"; return CHN_E_INVALID; }
    if (!j->text && j->text_bytes) { why = W + ": text is NULL"; return CHN_E_INVALID; }
    if (j->text_bytes > CHN_TEXT_SPLIT_MAX_BYTES) {
        why = W + ": text_bytes " + std::to_string(j->text_bytes) + " is above CHN_TEXT_SPLIT_MAX_BYTES (" + std::to_string(CHN_TEXT_SPLIT_MAX_BYTES) + " bytes)";
        return CHN_E_CAPACITY;
    }
    return CHN_OK;
}
// a record is at least "@\nA\n+\nA\n": more candidates than this cannot be met, whatever max_records says
static uint64_t tsp_record_bound(const chn_text_split_job *j) { return std::min<uint64_t>(j->max_records, (j->text_bytes - j->start) / 8); }

static int tsp_ids_too_small(const chn_text_split_job *j, uint64_t need, const char *who, std::string &why) {
    why = std::string(who) + ": the ids need " + std::to_string(need) + " bytes, ids_capacity is " + std::to_string(j->ids_capacity);
    return CHN_E_CAPACITY;
}

// chn_text_split_host: the rule applied from `start` one record after another
static int tsp_host_job(chn_text_split_job *j, std::string &why) {
    const char *who = "chn_text_split_host";
    int rc = tsp_check_job(j, who, why);
    if (rc) return rc;
    const uint8_t *text = j->text;
    const uint64_t end = j->text_bytes, bound = tsp_record_bound(j);
    uint64_t n = 0, ids_bytes = 0, ls[5];
    ls[0] = j->start;
    while (n < bound) {
        bool four = true;
        for (int k = 0; k < 4 && four; ++k) {
            const void *nl = ls[k] < end ? std::memchr(text + ls[k], '\n', (size_t)(end - ls[k])) : nullptr;
            if (nl) ls[k + 1] = (uint64_t)(static_cast<const uint8_t *>(nl) - text) + 1; else four = false;
        }
        TspRecord r;
        if (!four || !tsp_record(text, ls, r)) break;
        j->id_offset[n] = r.id_off; j->id_length[n] = r.id_len;
        j->seq_offset[n] = r.seq_off; j->seq_length[n] = r.seq_len;
        j->qual_offset[n] = r.qual_off;
        ids_bytes += r.id_len;
        ls[0] = ls[4];
        ++n;
    }
    if (j->ids) {
        if (ids_bytes > j->ids_capacity) return tsp_ids_too_small(j, ids_bytes, who, why);
        uint64_t at = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (j->id_length[i]) std::memcpy(j->ids + at, text + j->id_offset[i], j->id_length[i]);
            at += j->id_length[i];
        }
    }
    j->n_records = n; j->consumed = ls[0]; j->ids_bytes = ids_bytes;
    return CHN_OK;
}

#ifdef __HIPCC__
// ---- kernels ---------------------------------------------------------------------------------------------------------------------
// control words of one call
enum { TSP_LINES = 0, TSP_FIRST_BAD = 1, TSP_N = 2, TSP_CONSUMED = 3, TSP_IDS_BYTES = 4, TSP_CTL_WORDS = 8 };

// which of the 16 bytes of the aligned piece at byte `p` of the text are line feeds inside [start, end): bit j is byte p + j.
// SWAR: a byte of x = w ^ 0x0A0A0A0A is zero exactly where the high bit of ~(((x & 0x7F..) + 0x7F..) | x | 0x7F..) is set.
__device__ __forceinline__ uint32_t tsp_piece_feeds(const uint8_t *text, uint64_t p, uint64_t start, uint64_t end) {
    if (p >= end || p + 16 <= start) return 0u;
    const u32x4_t v = *reinterpret_cast<const u32x4_t *>(text + p);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t x = w[q] ^ 0x0A0A0A0Au;
        const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);  // 0x80 in every byte that is a line feed
        m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * q);
    }
    const uint32_t hi = end - p < 16 ? (uint32_t)(end - p) : 16u, lo = start > p ? (uint32_t)(start - p) : 0u;  // lo < 16, hi >= 1
    return m & ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// 1. count: tile t is bytes [(tile0 + t) * TSP_TILE, + TSP_TILE) of the text; one wavefront a tile, a looping grid
__global__ void __launch_bounds__(256) k_split_count(const uint8_t *text, uint64_t start, uint64_t end, uint64_t tile0, uint32_t n_tiles, uint32_t *tile_count) {
    const uint32_t wave = (blockIdx.x * 256 + threadIdx.x) / WAVE, n_waves = gridDim.x * (256 / WAVE);
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {
        const uint64_t base = (tile0 + t) * TSP_TILE + lane_id() * 16;
        uint32_t c = 0;
#pragma unroll
        for (uint32_t k = 0; k < TSP_TILE / (WAVE * 16); ++k) c += (uint32_t)__popc(tsp_piece_feeds(text, base + k * WAVE * 16, start, end));
        c = wave_sum(c);
        if (lane_id() == 0) tile_count[t] = c;
    }
}

// 2. exclusive scan of in[0 .. n) into out, the sum into *total; ONE workgroup (array_scan, scan.inc).
// n is min(*n_dev, n_max) where n_dev is given (the number of records is known on the device only).  The sum stays below 2^32: it
// counts bytes of a text of at most 2^31.
__global__ void __launch_bounds__(SCAN_THREADS) k_split_scan(const uint32_t *in, uint32_t *out, const uint32_t *n_dev, uint32_t n_max, uint32_t *total) {
    const uint32_t n = n_dev ? min(*n_dev, n_max) : n_max;
    const uint32_t sum = array_scan<SCAN_THREADS, uint32_t>(n, [&](uint32_t i) { return in[i]; }, [&](uint32_t i, uint32_t at) { out[i] = at; });
    if (threadIdx.x == 0) *total = sum;
}

// 3. line starts: line feed number `rank` of [start, end) ends line `rank`; line rank + 1 starts behind it.  Only the first `cap` line
// starts behind line_start[0] = start are kept (cap = 4 x the record bound), so a text of nothing but line feeds needs no more room.
__global__ void __launch_bounds__(256) k_split_lines(const uint8_t *text, uint64_t start, uint64_t end, uint64_t tile0, uint32_t n_tiles, const uint32_t *tile_off,
                                                     uint32_t *line_start, uint32_t cap) {
    const uint32_t wave = (blockIdx.x * 256 + threadIdx.x) / WAVE, n_waves = gridDim.x * (256 / WAVE);
    if (wave == 0 && lane_id() == 0) line_start[0] = (uint32_t)start;
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {
        uint32_t rank0 = tile_off[t];  // (wave-uniform)
        if (rank0 >= cap) continue;
        const uint64_t base = (tile0 + t) * TSP_TILE + lane_id() * 16;
#pragma unroll
        for (uint32_t k = 0; k < TSP_TILE / (WAVE * 16); ++k) {
            const uint64_t p = base + k * WAVE * 16;
            uint32_t m = tsp_piece_feeds(text, p, start, end);
            const uint32_t c = (uint32_t)__popc(m), incl = wave_scan(c);
            uint32_t rank = rank0 + incl - c;
            for (uint32_t b = 0; b < 16; ++b)  // (sixteen rounds whatever the bytes are)
                if (m & (1u << b)) {
                    if (rank < cap) line_start[rank + 1] = (uint32_t)(p + b + 1);
                    ++rank;
                }
            rank0 += (uint32_t)__shfl((int)incl, WAVE - 1);
        }
    }
}

struct TspRecArgs {
    const uint8_t *text;
    const uint32_t *line_start;
    uint32_t *ctl;          // reads TSP_LINES, lowers TSP_FIRST_BAD
    uint32_t bound;         // most records to take
    uint64_t *id_off, *seq_off, *qual_off;
    uint32_t *id_len, *seq_len;
};
// 4. records: one lane per candidate r < min(lines / 4, bound); the first failing candidate of the launch is the minimum over the
// wavefronts of their lowest failing lane
__global__ void __launch_bounds__(256) k_split_records(TspRecArgs a) {
    const uint32_t n_cand = min(a.ctl[TSP_LINES] / 4, a.bound);
    const uint32_t stride = gridDim.x * 256;
    for (uint32_t r0 = blockIdx.x * 256 + (threadIdx.x & ~(WAVE - 1)); r0 < n_cand; r0 += stride) {  // (wave-uniform)
        const uint32_t r = r0 + lane_id();
        bool bad = false;
        if (r < n_cand) {
            uint64_t ls[5];
#pragma unroll
            for (uint32_t k = 0; k < 5; ++k) ls[k] = a.line_start[4 * (uint64_t)r + k];
            TspRecord rec;
            if (tsp_record(a.text, ls, rec)) {
                a.id_off[r] = rec.id_off; a.seq_off[r] = rec.seq_off; a.qual_off[r] = rec.qual_off;
                a.id_len[r] = rec.id_len; a.seq_len[r] = rec.seq_len;
            } else bad = true;
        }
        const uint64_t m = __ballot(bad ? 1 : 0);
        if (m && lane_id() == 0) atomicMin(&a.ctl[TSP_FIRST_BAD], r0 + (uint32_t)__ffsll((unsigned long long)m) - 1);
    }
}

// ... and what follows from it: the number of records taken and where the last of them ends
__global__ void k_split_close(const uint32_t *line_start, uint32_t *ctl, uint32_t bound) {
    if (threadIdx.x || blockIdx.x) return;
    const uint32_t n = min(min(ctl[TSP_LINES] / 4, bound), ctl[TSP_FIRST_BAD]);
    ctl[TSP_N] = n;
    ctl[TSP_CONSUMED] = line_start[4 * (uint64_t)n];
}

// 5. ids: record i's id bytes to ids + id_pos[i]; sixteen lanes a record, a looping grid
__global__ void __launch_bounds__(256) k_split_ids(const uint8_t *text, const uint64_t *id_off, const uint32_t *id_len, const uint32_t *id_pos, uint32_t n, uint8_t *ids) {
    const uint32_t g = threadIdx.x & 15u, stride = gridDim.x * 16;
    for (uint32_t i = blockIdx.x * 16 + threadIdx.x / 16; i < n; i += stride) {
        const uint8_t *src = text + id_off[i];
        uint8_t *dst = ids + id_pos[i];
        const uint32_t len = id_len[i];
        for (uint32_t b = g; b < len; b += 16) dst[b] = src[b];
    }
}
#endif
