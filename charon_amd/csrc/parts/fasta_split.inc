// fasta_split.inc -- FASTA records found and unwrapped in a text that lies in device memory (chn_fasta_split), and the same rule on
// the CPU (chn_fasta_split_host)
// Part of the single translation unit charon_hip.hip (included in order, behind text_split.inc); not a stand-alone source.
//
// ONE rule source for the device and the host, as text_split.inc has it: fsp_is_header, fsp_is_dropped and fsp_record are
// __host__ __device__ code.  Together they are exactly what BlockReader::parse_fasta (host/fastx_reader.inc) produces from a record
// boundary on.  Lines end at '\n' inside [start, text_bytes).
//   - a HEADER LINE is a line whose first byte is '>' or ';'; record i runs from header line i up to the next header line;
//   - the id is what follows the first byte up to the line feed, minus one trailing '\r' (it may be empty);
//   - the sequence is the bytes of the lines between the two header lines, in order, without '\n', '\r', ' ', '\t' and '0' .. '9'
//     (what seqan3 skips inside FASTA sequence lines; parse_fasta's clean-line shortcut moves a line of bytes >= 0x40 as one piece,
//     which is the same thing because every dropped byte is below 0x40);
//   - a record is taken if and only if its first byte begins a header line, the header's line feed lies in the text, the next header
//     line begins inside the text and the compacted sequence has length >= 1.
// With CHN_FASTA_SPLIT_END_OF_INPUT the end of the text counts as a following header line (and as the line end of a last line without
// a line feed), which is parse_fasta under eof_.  Records are taken from `start` one behind the other until the rule fails or
// max_records is reached; an empty record, a text that does not begin with a header (leading blank lines included) and a record with
// no header behind it end the run and are the caller's business.
//
// The host walks record by record (fsp_host_job, the body of chn_fasta_split_host).  The device does not walk: everything follows
// from per-byte predicates and prefix sums.
//   a. k_fasta_tiles    a wavefront per 4 KiB tile: per byte whether it is a line feed, a line start that is a header, a byte the
//                       sequence keeps.  Whether a byte lies in a header line depends on the line that runs INTO the tile, so the
//                       tile's summary keeps the bytes in front of its first line start apart (FspTile).
//   b. k_fasta_resolve  one workgroup: the state that runs into every tile (a last-writer-wins scan, associative), and with it the
//                       tile's header-ending line feeds and kept bytes; k_split_scan (text_split.inc) then gives the three exclusive sums.
//   c. k_fasta_headers  the header of rank r stores its position and the number of kept bytes in front of it, the line feed that ends
//                       it stores its own position (and whether a '\r' stands before it) under the same rank: only the last header
//                       of a text can lack its line feed, so the ranks agree.
//   d. k_fasta_records  one lane per candidate record applies fsp_record; k_fasta_close: how many are taken, where they end, how many
//                       letters they hold.
//   e. k_fasta_compact  every lane ranks the kept bytes of its 16-byte piece (popcount, wave scan, tile base); the letters of the taken
//                       records are staged in LDS so that whole 16-byte pieces of the destination are single aligned vector stores.
//                       Only the ragged ends of a tile's stretch go byte by byte.  Kept bytes at or behind seq_bytes are not stored.
//   f. k_split_ids      (text_split.inc) the ids.
// Device text contract as text_split.inc: aligned 16-byte loads only, bytes outside [start, text_bytes) are masked, never judged;
// every store is a plain store; every loop runs over tiles, pieces or records, none over data.

#ifndef __HIPCC__  // a CPU build of the rule and the host walk alone (tools/fuzz/fasta_split_fuzz.cpp)
#ifndef __host__
#define __host__
#define __device__
#endif
#endif

__host__ __device__ static inline bool fsp_is_header(uint8_t c) { return c == '>' || c == ';'; }
__host__ __device__ static inline bool fsp_is_dropped(uint8_t c) { return c == '\n' || c == '\r' || c == ' ' || c == '\t' || (uint8_t)(c - '0') < 10; }

struct FspRecord {
    uint64_t id_off, seq_off;
    uint32_t id_len, seq_len;
};
// the rule, given what the text says about one record: its header line starts at `hdr` and ends with the line feed at `feed`, `cr`
// says whether the byte in front of that line feed is '\r'; kept0 / kept1 are the kept bytes of the text in front of this header and
// in front of the next (or of the end of the text, where that counts as one)
__host__ __device__ static inline bool fsp_record(uint64_t hdr, uint64_t feed, bool cr, uint64_t kept0, uint64_t kept1, FspRecord &r) {
    uint64_t idn = feed - hdr - 1;
    if (idn && cr) --idn;
    if (kept1 == kept0) return false;  // an empty record
    r.id_off = hdr + 1; r.id_len = (uint32_t)idn;
    r.seq_off = kept0; r.seq_len = (uint32_t)(kept1 - kept0);
    return true;
}

static uint64_t fsp_up16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }

// The checks both calls make on a job before anything else; `why` names the first that fails.  0 or a CHN_E_* code.
static int fsp_check_job(const chn_fasta_split_job *j, const char *who, std::string &why) {
    const std::string W(who);
    if (!j) { why = W + ": null job"; return CHN_E_INVALID; }
    if (j->struct_size != sizeof(chn_fasta_split_job)) { why = W + ": bad struct_size"; return CHN_E_INVALID; }
    if (j->flags & ~(uint32_t)CHN_FASTA_SPLIT_END_OF_INPUT) { why = W + ": unknown flag"; return CHN_E_INVALID; }
    if (j->start > j->text_bytes) { why = W + ": start lies behind text_bytes"; return CHN_E_INVALID; }
    if (j->max_records && (!j->id_offset || !j->id_length || !j->seq_offset || !j->seq_length)) { why = W + ": a descriptor array is NULL"; return CHN_E_INVALID; }
    if (!j->text && j->text_bytes) { why = W + ": text is NULL"; return CHN_E_INVALID; }
    if (j->text_bytes > CHN_TEXT_SPLIT_MAX_BYTES) {
        why = W + ": text_bytes " + std::to_string(j->text_bytes) + " is above CHN_TEXT_SPLIT_MAX_BYTES (" + std::to_string(CHN_TEXT_SPLIT_MAX_BYTES) + " bytes)";
        return CHN_E_CAPACITY;
    }
    const uint64_t need = fsp_up16(j->text_bytes - j->start);
    if (j->seq_capacity < need) {
        why = W + ": the letters may need " + std::to_string(need) + " bytes, seq_capacity is " + std::to_string(j->seq_capacity);
        return CHN_E_CAPACITY;
    }
    if (!j->seq_text && j->seq_capacity) { why = W + ": seq_text is NULL"; return CHN_E_INVALID; }
    if (j->seq_capacity && j->text_bytes) {
        const uintptr_t t0 = reinterpret_cast<uintptr_t>(j->text), t1 = t0 + fsp_up16(j->text_bytes), s0 = reinterpret_cast<uintptr_t>(j->seq_text), s1 = s0 + j->seq_capacity;
        if (s0 < t1 && t0 < s1) { why = W + ": seq_text and text overlap"; return CHN_E_INVALID; }
    }
    return CHN_OK;
}
// a record is at least ">\nA": more candidates than this cannot be met, whatever max_records says
static uint64_t fsp_record_bound(const chn_fasta_split_job *j) { return std::min<uint64_t>(j->max_records, (j->text_bytes - j->start) / 3); }

static int fsp_ids_too_small(const chn_fasta_split_job *j, uint64_t need, const char *who, std::string &why) {
    why = std::string(who) + ": the ids need " + std::to_string(need) + " bytes, ids_capacity is " + std::to_string(j->ids_capacity);
    return CHN_E_CAPACITY;
}

// chn_fasta_split_host: the rule applied from `start` one record after another
static int fsp_host_job(chn_fasta_split_job *j, std::string &why) {
    const char *who = "chn_fasta_split_host";
    int rc = fsp_check_job(j, who, why);
    if (rc) return rc;
    const uint8_t *text = j->text;
    const uint64_t end = j->text_bytes, bound = fsp_record_bound(j);
    const bool eoi = (j->flags & CHN_FASTA_SPLIT_END_OF_INPUT) != 0;
    uint64_t n = 0, ids_bytes = 0, kept = 0, p = j->start;
    while (n < bound) {
        if (p >= end || !fsp_is_header(text[p])) break;
        const void *nl = std::memchr(text + p, '\n', (size_t)(end - p));
        if (!nl) break;  // (at the end of the input too: no byte is left for the sequence)
        const uint64_t feed = (uint64_t)(static_cast<const uint8_t *>(nl) - text);
        // the next header line, or the end of the input
        uint64_t next = feed + 1;
        bool found = false;
        for (;;) {
            if (next >= end) { found = eoi; next = end; break; }
            if (fsp_is_header(text[next])) { found = true; break; }
            const void *e = std::memchr(text + next, '\n', (size_t)(end - next));
            if (!e) { found = eoi; next = end; break; }
            next = (uint64_t)(static_cast<const uint8_t *>(e) - text) + 1;
        }
        if (!found) break;
        uint64_t at = kept;
        for (uint64_t q = feed + 1; q < next; ++q)
            if (!fsp_is_dropped(text[q])) j->seq_text[at++] = text[q];
        FspRecord r;
        if (!fsp_record(p, feed, feed > p && text[feed - 1] == '\r', kept, at, r)) break;
        j->id_offset[n] = r.id_off; j->id_length[n] = r.id_len;
        j->seq_offset[n] = r.seq_off; j->seq_length[n] = r.seq_len;
        ids_bytes += r.id_len;
        kept = at;
        p = next;
        ++n;
    }
    if (j->ids) {
        if (ids_bytes > j->ids_capacity) return fsp_ids_too_small(j, ids_bytes, who, why);
        uint64_t at = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (j->id_length[i]) std::memcpy(j->ids + at, text + j->id_offset[i], j->id_length[i]);
            at += j->id_length[i];
        }
    }
    j->n_records = n; j->consumed = p; j->ids_bytes = ids_bytes; j->seq_bytes = kept;
    return CHN_OK;
}

#ifdef __HIPCC__
// ---- kernels ---------------------------------------------------------------------------------------------------------------------
// control words of one call
enum { FSP_HDRS = 0, FSP_FEEDS = 1, FSP_KEPT = 2, FSP_FIRST_BAD = 3, FSP_N = 4, FSP_CONSUMED = 5, FSP_SEQ_BYTES = 6, FSP_IDS_BYTES = 7, FSP_CTL_WORDS = 8 };

// what a tile knows of itself.  state: 2 | h if the tile has a line start (h: the last of them is a header), else 0.  The bytes in
// front of the first line start belong to the line that runs into the tile: kept_pre of them are no dropped bytes, feed_pre (0 or 1)
// is a line feed.  Behind it the tile knows the lines: kept_in kept bytes in other than header lines, feed_in line feeds of header lines.
struct FspTile { uint32_t state, n_hdr, kept_pre, feed_pre, kept_in, feed_in; };

// the aligned 16-byte piece at byte `p` of the text: its words, and which of its bytes lie inside [start, end) (bit j is byte p + j),
// are line feeds, '\r', '>' or ';', dropped bytes -- all inside [start, end) only
struct FspPiece { uint32_t w[4], valid, lf, cr, hb, drop; };
__device__ __forceinline__ FspPiece fsp_piece(const uint8_t *text, uint64_t p, uint64_t start, uint64_t end) {
    FspPiece m;
    m.w[0] = m.w[1] = m.w[2] = m.w[3] = 0; m.valid = m.lf = m.cr = m.hb = m.drop = 0;
    if (p >= end || p + 16 <= start) return m;
    const u32x4_t v = *reinterpret_cast<const u32x4_t *>(text + p);
    m.w[0] = v.x; m.w[1] = v.y; m.w[2] = v.z; m.w[3] = v.w;
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b) {
        const uint8_t c = (uint8_t)(m.w[b >> 2] >> (8 * (b & 3)));
        m.lf |= (uint32_t)(c == '\n') << b;
        m.cr |= (uint32_t)(c == '\r') << b;
        m.hb |= (uint32_t)fsp_is_header(c) << b;
        m.drop |= (uint32_t)fsp_is_dropped(c) << b;
    }
    const uint32_t hi = end - p < 16 ? (uint32_t)(end - p) : 16u, lo = start > p ? (uint32_t)(start - p) : 0u;  // lo < 16, hi >= 1
    m.valid = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
    m.lf &= m.valid; m.cr &= m.valid; m.hb &= m.valid; m.drop &= m.valid;
    return m;
}

// a wavefront going through one tile, a round of 64 pieces at a time
struct FspWalk {
    uint32_t tail;    // wave-uniform: bit 0 / 1: the byte in front of the round's first piece is a line feed / a '\r' of the text
    uint32_t state;   // wave-uniform: 2 | h once a line start has been met, h saying whether that line is a header line; else 0
    // one lane's piece, from step()
    FspPiece m;
    uint32_t ls, hs;  // line starts; those that begin a header line
    uint32_t crp;     // bytes that stand behind a '\r'
    uint32_t inhdr;   // bytes of header lines, as far as the state is known
    uint32_t pre;     // bytes in front of the first line start since begin(): their line is not known (never set when begin() knew it)

    __device__ __forceinline__ void begin(const uint8_t *text, uint64_t tile_base, uint64_t start, uint64_t end, uint32_t state_in) {
        state = state_in; tail = 0;
        if (tile_base > start) {  // (so tile_base >= 16; every lane loads the same piece)
            const FspPiece b = fsp_piece(text, tile_base - 16, start, end);
            tail = ((b.lf >> 15) & 1u) | (((b.cr >> 15) & 1u) << 1);
        }
    }
    __device__ __forceinline__ void step(const uint8_t *text, uint64_t p, uint64_t start, uint64_t end) {
        m = fsp_piece(text, p, start, end);
        const uint32_t mine = ((m.lf >> 15) & 1u) | (((m.cr >> 15) & 1u) << 1);
        uint32_t up = (uint32_t)__shfl_up((int)mine, 1);
        if (lane_id() == 0) up = tail;
        ls = (((m.lf << 1) | (up & 1u)) & 0xFFFFu) & m.valid;
        if (start >= p && start < p + 16 && start < end) ls |= 1u << (uint32_t)(start - p);
        crp = ((m.cr << 1) | (up >> 1)) & 0xFFFFu;
        hs = ls & m.hb;
        // the state behind this piece, last writer wins: over the lanes, then over what came before
        uint32_t incl = ls ? (2u | ((hs >> (31 - __clz((int)ls))) & 1u)) : 0u;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, o); if (lane_id() >= (uint32_t)o && !(incl & 2u)) incl = t; }
        uint32_t in = (uint32_t)__shfl_up((int)incl, 1);
        if (lane_id() == 0 || !(in & 2u)) in = state;
        uint32_t h = in & 1u, known = in >> 1;
        inhdr = 0; pre = 0;
#pragma unroll
        for (uint32_t b = 0; b < 16; ++b) {  // (sixteen rounds whatever the bytes are)
            if (ls & (1u << b)) { known = 1u; h = (hs >> b) & 1u; }
            inhdr |= h << b;
            pre |= (known ^ 1u) << b;
        }
        tail = (uint32_t)__shfl((int)mine, WAVE - 1);
        const uint32_t last = (uint32_t)__shfl((int)incl, WAVE - 1);
        if (last & 2u) state = last;
    }
    __device__ __forceinline__ uint32_t kept() const { return m.valid & ~m.drop & ~inhdr & ~pre; }  // (with a known state: pre == 0)
    __device__ __forceinline__ uint32_t header_feeds() const { return m.lf & inhdr & ~pre; }
};

// a. tiles: tile t is bytes [(tile0 + t) * TSP_TILE, + TSP_TILE) of the text; one wavefront a tile, a looping grid
__global__ void __launch_bounds__(256) k_fasta_tiles(const uint8_t *text, uint64_t start, uint64_t end, uint64_t tile0, uint32_t n_tiles, FspTile *tiles) {
    const uint32_t wave = (blockIdx.x * 256 + threadIdx.x) / WAVE, n_waves = gridDim.x * (256 / WAVE);
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {
        const uint64_t tile_base = (tile0 + t) * TSP_TILE;
        FspWalk x;
        x.begin(text, tile_base, start, end, 0u);
        uint32_t n_hdr = 0, kept_pre = 0, feed_pre = 0, kept_in = 0, feed_in = 0;
#pragma unroll
        for (uint32_t k = 0; k < TSP_TILE / (WAVE * 16); ++k) {
            x.step(text, tile_base + k * WAVE * 16 + lane_id() * 16, start, end);
            n_hdr += (uint32_t)__popc(x.hs);
            kept_pre += (uint32_t)__popc(x.m.valid & ~x.m.drop & x.pre);
            feed_pre += (uint32_t)__popc(x.m.lf & x.pre);
            kept_in += (uint32_t)__popc(x.kept());
            feed_in += (uint32_t)__popc(x.header_feeds());
        }
        n_hdr = wave_sum(n_hdr); kept_pre = wave_sum(kept_pre); feed_pre = wave_sum(feed_pre);
        kept_in = wave_sum(kept_in); feed_in = wave_sum(feed_in);
        if (lane_id() == 0) {
            FspTile o;
            o.state = x.state; o.n_hdr = n_hdr; o.kept_pre = kept_pre; o.feed_pre = feed_pre; o.kept_in = kept_in; o.feed_in = feed_in;
            tiles[t] = o;
        }
    }
}

__device__ __forceinline__ uint32_t fsp_later(uint32_t before, uint32_t after) { return (after & 2u) ? after : before; }

// b. resolve: tile_state[t] = is the line that runs into tile t a header line (0 for the first tile: `start` is a line start), and the
// tile's counts under that state.  ONE workgroup of 256 threads, four tiles a thread and round.
__global__ void __launch_bounds__(256) k_fasta_resolve(const FspTile *tiles, uint32_t n, uint32_t *tile_state, uint32_t *tile_hdr, uint32_t *tile_feed, uint32_t *tile_kept) {
    __shared__ uint32_t part[256 / WAVE];
    const uint32_t wv = threadIdx.x / WAVE;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + threadIdx.x * 4;
        FspTile v[4];
        uint32_t mine = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (i + k < n) v[k] = tiles[i + k]; else { v[k].state = v[k].n_hdr = v[k].kept_pre = v[k].feed_pre = v[k].kept_in = v[k].feed_in = 0; }
            mine = fsp_later(mine, v[k].state);
        }
        uint32_t incl = mine;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, o); if (lane_id() >= (uint32_t)o) incl = fsp_later(t, incl); }
        if (lane_id() == WAVE - 1) part[wv] = incl;
        __syncthreads();
        uint32_t before = carry, all = carry;
#pragma unroll
        for (uint32_t k = 0; k < 256 / WAVE; ++k) { if (k < wv) before = fsp_later(before, part[k]); all = fsp_later(all, part[k]); }
        uint32_t up = (uint32_t)__shfl_up((int)incl, 1);
        if (lane_id() == 0) up = 0;
        uint32_t cur = fsp_later(before, up);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (i + k < n) {
                const uint32_t h = cur & 1u;
                tile_state[i + k] = h;
                tile_hdr[i + k] = v[k].n_hdr;
                tile_feed[i + k] = v[k].feed_in + (h ? v[k].feed_pre : 0u);
                tile_kept[i + k] = v[k].kept_in + (h ? 0u : v[k].kept_pre);
            }
            cur = fsp_later(cur, v[k].state);
        }
        carry = all;
        __syncthreads();  // part[] is the next round's
    }
}

// c. headers.  Only the first `cap` ranks are kept (cap = the record bound + 1), so a text of nothing but '>' needs no more room.
// feed_pos carries in bit 31 whether a '\r' stands in front of the line feed (positions are below 2^31).  Entry H = the number of
// headers stands for the end of the text: hdr_pos[H] = end, kept_before[H] = all kept bytes.
__global__ void __launch_bounds__(256) k_fasta_headers(const uint8_t *text, uint64_t start, uint64_t end, uint64_t tile0, uint32_t n_tiles, const uint32_t *tile_state,
                                                       const uint32_t *hdr_off, const uint32_t *feed_off, const uint32_t *kept_off, const uint32_t *ctl,
                                                       uint32_t *hdr_pos, uint32_t *feed_pos, uint32_t *kept_before, uint32_t cap) {
    const uint32_t wave = (blockIdx.x * 256 + threadIdx.x) / WAVE, n_waves = gridDim.x * (256 / WAVE);
    if (wave == 0 && lane_id() == 0) {
        const uint32_t H = ctl[FSP_HDRS];
        if (H < cap) { hdr_pos[H] = (uint32_t)end; kept_before[H] = ctl[FSP_KEPT]; }
    }
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {
        uint32_t hr = hdr_off[t], fr = feed_off[t], kr = kept_off[t];  // (wave-uniform)
        if (hr >= cap && fr >= cap) continue;
        const uint64_t tile_base = (tile0 + t) * TSP_TILE;
        FspWalk x;
        x.begin(text, tile_base, start, end, 2u | tile_state[t]);
#pragma unroll
        for (uint32_t k = 0; k < TSP_TILE / (WAVE * 16); ++k) {
            const uint64_t p = tile_base + k * WAVE * 16 + lane_id() * 16;
            x.step(text, p, start, end);
            const uint32_t kept = x.kept(), hf = x.header_feeds();
            const uint32_t c2 = (uint32_t)__popc(x.hs) | ((uint32_t)__popc(hf) << 16), ck = (uint32_t)__popc(kept);  // (at most 1024 each a round)
            const uint32_t i2 = wave_scan(c2), ik = wave_scan(ck);
            uint32_t rank_h = hr + ((i2 - c2) & 0xFFFFu), rank_f = fr + ((i2 - c2) >> 16);
            const uint32_t kb = kr + ik - ck;
            for (uint32_t b = 0; b < 16; ++b) {  // (sixteen rounds whatever the bytes are)
                if (x.hs & (1u << b)) {
                    if (rank_h < cap) { hdr_pos[rank_h] = (uint32_t)(p + b); kept_before[rank_h] = kb + (uint32_t)__popc(kept & ((1u << b) - 1u)); }
                    ++rank_h;
                }
                if (hf & (1u << b)) {
                    if (rank_f < cap) feed_pos[rank_f] = (uint32_t)(p + b) | (((x.crp >> b) & 1u) << 31);
                    ++rank_f;
                }
            }
            const uint32_t t2 = (uint32_t)__shfl((int)i2, WAVE - 1);
            hr += t2 & 0xFFFFu; fr += t2 >> 16; kr += (uint32_t)__shfl((int)ik, WAVE - 1);
        }
    }
}

struct FspRecArgs {
    const uint32_t *hdr_pos, *feed_pos, *kept_before;
    uint32_t *ctl;          // reads FSP_HDRS and FSP_FEEDS, lowers FSP_FIRST_BAD
    uint32_t start, bound;  // most records to take
    uint32_t eoi;           // CHN_FASTA_SPLIT_END_OF_INPUT
    uint64_t *id_off, *seq_off;
    uint32_t *id_len, *seq_len;
};
// the headers that have a successor, if the text begins with one
__device__ __forceinline__ uint32_t fsp_candidates(const FspRecArgs &a) {
    const uint32_t H = a.ctl[FSP_HDRS];
    if (H == 0 || a.hdr_pos[0] != a.start) return 0;
    return min(a.bound, a.eoi ? H : H - 1);
}
// d. records: one lane per candidate; the first failing candidate of the launch is the minimum over the wavefronts of their lowest
// failing lane
__global__ void __launch_bounds__(256) k_fasta_records(FspRecArgs a) {
    const uint32_t n_cand = fsp_candidates(a), n_feeds = a.ctl[FSP_FEEDS];
    const uint32_t stride = gridDim.x * 256;
    for (uint32_t r0 = blockIdx.x * 256 + (threadIdx.x & ~(WAVE - 1)); r0 < n_cand; r0 += stride) {  // (wave-uniform)
        const uint32_t r = r0 + lane_id();
        bool bad = false;
        if (r < n_cand) {
            FspRecord rec;
            const uint32_t f = r < n_feeds ? a.feed_pos[r] : 0u;
            if (r < n_feeds && fsp_record(a.hdr_pos[r], f & 0x7FFFFFFFu, (f >> 31) != 0, a.kept_before[r], a.kept_before[r + 1], rec)) {
                a.id_off[r] = rec.id_off; a.seq_off[r] = rec.seq_off;
                a.id_len[r] = rec.id_len; a.seq_len[r] = rec.seq_len;
            } else bad = true;
        }
        const uint64_t m = __ballot(bad ? 1 : 0);
        if (m && lane_id() == 0) atomicMin(&a.ctl[FSP_FIRST_BAD], r0 + (uint32_t)__ffsll((unsigned long long)m) - 1);
    }
}

// ... and what follows from it: the number of records taken, where the last of them ends, how many letters they hold
__global__ void k_fasta_close(FspRecArgs a) {
    if (threadIdx.x || blockIdx.x) return;
    const uint32_t n = min(fsp_candidates(a), a.ctl[FSP_FIRST_BAD]);
    a.ctl[FSP_N] = n;
    a.ctl[FSP_CONSUMED] = n ? a.hdr_pos[n] : a.start;
    a.ctl[FSP_SEQ_BYTES] = n ? a.kept_before[n] : 0u;
}

// e. compaction: kept byte number g of the text goes to seq[g] if g < seq_bytes.  A tile's kept bytes are the stretch [g0, g0 + count)
// of the destination: they are laid out in LDS from byte g0 & 15 on, so that LDS piece i is destination piece (g0 & ~15) / 16 + i.
__global__ void __launch_bounds__(256) k_fasta_compact(const uint8_t *text, uint64_t start, uint64_t end, uint64_t tile0, uint32_t n_tiles, const uint32_t *tile_state,
                                                       const uint32_t *kept_off, const uint32_t *ctl, uint8_t *seq) {
    __shared__ u32x4_t stage[256 / WAVE][TSP_TILE / 16 + 1];
    const uint32_t wave = (blockIdx.x * 256 + threadIdx.x) / WAVE, n_waves = gridDim.x * (256 / WAVE);
    const uint32_t seq_bytes = ctl[FSP_SEQ_BYTES];
    u32x4_t *mine = stage[threadIdx.x / WAVE];
    uint8_t *lds = reinterpret_cast<uint8_t *>(mine);
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {
        const uint32_t g0 = kept_off[t];  // (wave-uniform)
        if (g0 >= seq_bytes) continue;
        const uint64_t tile_base = (tile0 + t) * TSP_TILE;
        const uint32_t sh = g0 & 15u;
        uint32_t at = sh;
        FspWalk x;
        x.begin(text, tile_base, start, end, 2u | tile_state[t]);
#pragma unroll
        for (uint32_t k = 0; k < TSP_TILE / (WAVE * 16); ++k) {
            x.step(text, tile_base + k * WAVE * 16 + lane_id() * 16, start, end);
            const uint32_t kept = x.kept(), c = (uint32_t)__popc(kept), incl = wave_scan(c);
            uint32_t pos = at + incl - c;
#pragma unroll
            for (uint32_t b = 0; b < 16; ++b)
                if (kept & (1u << b)) lds[pos++] = (uint8_t)(x.m.w[b >> 2] >> (8 * (b & 3)));
            at += (uint32_t)__shfl((int)incl, WAVE - 1);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the stretch [g0, g1) of the destination, g1 <= seq_bytes: [g0, a0) and [a1, g1) byte by byte, the whole pieces between them
        const uint32_t g1 = min(g0 + (at - sh), seq_bytes), base = g0 - sh;
        const uint32_t a0 = (g0 + 15u) & ~15u, a1 = g1 & ~15u;
        const uint32_t head_end = min(a0, g1);
        if (lane_id() < head_end - g0) seq[g0 + lane_id()] = lds[sh + lane_id()];
        if (a1 >= a0) {
            const uint32_t pieces = (a1 - a0) / 16, first = (a0 - base) / 16;
            u32x4_t *dst = reinterpret_cast<u32x4_t *>(seq + a0);
            for (uint32_t i = lane_id(); i < pieces; i += WAVE) dst[i] = mine[first + i];
            if (lane_id() < g1 - a1) seq[a1 + lane_id()] = lds[a1 - base + lane_id()];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the stage is the next tile's
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}
#endif
