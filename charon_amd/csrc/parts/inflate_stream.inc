// inflate_stream.inc -- chunks of ONE deflate stream decoded side by side: 16-bit symbols behind a ring, window hand-down, symbols to bytes
// Part of the single translation unit charon_hip.hip (included in order, behind inflate_members.inc); not a stand-alone source.
//
// A chunk starts at a block header somewhere inside a stream, so the 32 KiB of output in front of it are unknown while it is decoded.
// The decoder is inflate_members.inc's -- bit reader, block headers, code-length parsing, build(), symbol() and every acceptance check --
// with another output side (InfRingOut): what it produces are 16-bit SYMBOLS, 0-255 for a byte that is known, 0x8000 | w for "the byte at
// position w of the window in front of this chunk" (w = 32768 + p - d for the element at chunk position p of a match of distance d with
// p - d < 0; w = 32767 is the byte right in front of the chunk).  A match whose source lies inside the chunk copies the symbol as it
// stands, marker or not.  The symbols have no known number, so they pass through a RING of 32 Ki symbols in LDS (64 KiB, where the member
// decoder keeps its window) and leave it for the chunk's stretch of a symbol scratch in global memory in groups of 512 -- one 16-byte store
// per lane -- before their slot is used again.  Ring positions p and p - 32768 share a slot: a match of distance 32 705 .. 32 768 reads
// slots that the same match writes.  Element k's source is the slot element k + 32768 - d (>= k) writes, a wavefront's 64 loads of a round
// come before its 64 stores, and the one-lane host policy goes through k in order: every read comes before the write to its slot, and the
// groups behind the write position are stored before the match begins (make_room).
// Three steps, the same rules on the device (three kernels) and on the host (infs_run_host, serially):
//   1 k_inflate_chunks   one wavefront per chunk, drawn from a cursor: whole blocks until the chunk stands at or behind its target bit or
//                        behind a final block; the last complete block boundary (bit, symbols) and the reason it stopped go out
//   2 k_inflate_windows  one workgroup over the proven chunks in stream order: window[k + 1] = the last 32 768 bytes of (window[k]
//                        followed by chunk k's symbols resolved against window[k]); every chunk's incoming window stays in global memory
//   3 k_inflate_bytes    one wavefront per piece of INFS_PIECE symbols of a chunk: the chunk's window is a 32 KiB table in LDS, the bytes
//                        are put together in LDS, their CRC-32 taken there (inf_crc32_at) and written out 16 bytes a lane; the smallest
//                        marker of the chunk goes out (the distance rule: a marker below 32768 - bytes of the member so far is zlib's
//                        "invalid distance too far back")
// Every loop of step 1 consumes input bits or symbol capacity, so it ends on any input -- a falsely started chunk decodes noise.

static const uint32_t INFS_WIN = 32768;    // bytes of window, symbols of ring
static const uint32_t INFS_GROUP = 512;    // symbols that leave the ring at once on the device: 64 lanes x 16 bytes
static const uint32_t INFS_PIECE = 32768;  // bytes one workgroup of k_inflate_bytes makes (window + piece + CRC tables: 68 KiB, two per CU)
static const uint32_t INFS_MAX_CAP = 1u << 30;

struct alignas(16) Inf16 { uint32_t w[4]; };  // one 16-byte load / store on either side

// symbols of one chunk's stretch of the scratch: the capacity rounded up to whole groups
__host__ __device__ static inline uint64_t infs_stride(uint32_t cap) { return ((uint64_t)cap + INFS_GROUP - 1) / INFS_GROUP * INFS_GROUP; }

struct InfRingOut {
    static const bool ASKS_FIRST = false;
    uint16_t *ring;     // INFS_WIN symbols: symbol p lives at ring[p % INFS_WIN] until it is stored
    uint16_t *sym;      // the chunk's stretch of the scratch, 16-byte aligned, infs_stride(cap) symbols
    uint32_t cap;       // symbols the chunk may produce
    uint32_t before;    // bytes a distance may reach in front of the chunk (chunk 0: the caller's window; others: unknown, all 32 768)
    uint64_t target;    // stop at the first block boundary at or behind this bit (counted like the decoder's wpos * 32 - bc)
    uint32_t pos, stored;       // symbols produced; symbols [0, stored) are in `sym` (a multiple of INFS_GROUP)
    uint64_t end_bit;           // the last complete block boundary ...
    uint32_t end_sym;           // ... and the symbols up to it
    bool final, far;            // that block had BFINAL; a distance reached in front of `before`

    __host__ __device__ bool room(uint32_t n) const { return pos + n <= cap; }
    __host__ __device__ bool reach(uint32_t dist) {
        if (dist <= before + pos) return true;
        far = true;
        return false;
    }
    // symbols [stored, to) -- whole groups -- from the ring to the scratch
    template <class P> __host__ __device__ void store(P &p, uint32_t to) {
        p.sync();  // what lane 0 wrote is visible
        for (uint32_t g = stored + p.lane() * 8; g < to; g += P::LANES * 8)
            *reinterpret_cast<Inf16 *>(sym + g) = *reinterpret_cast<const Inf16 *>(ring + (g & (INFS_WIN - 1)));
        if (to > stored) stored = to;
        p.sync();
    }
    // the slots of symbols [pos, pos + n), n <= 258, are free: what they held is in the scratch
    template <class P> __host__ __device__ void make_room(P &p, uint32_t n) {
        if (pos + n - stored > INFS_WIN) store(p, pos & ~(INFS_GROUP - 1));  // fewer than a group stay behind: 511 + 258 fit
    }
    template <class P> __host__ __device__ void lit(P &p, uint32_t b) {
        make_room(p, 1);
        if (p.lane() == 0) ring[pos & (INFS_WIN - 1)] = (uint16_t)b;
        ++pos;
    }
    template <class P> __host__ __device__ void put(P &p, uint32_t v, uint32_t n) {  // the low n <= 4 bytes of v
        make_room(p, n);
        for (uint32_t i = p.lane(); i < n; i += P::LANES) ring[(pos + i) & (INFS_WIN - 1)] = (uint16_t)((v >> (8 * i)) & 255u);
        pos += n;
    }
    // element k comes from chunk position s + k (overlapping: s + k % dist): a ring slot as it stands, or the marker of a window position
    template <class P> __host__ __device__ void match(P &p, uint32_t dist, uint32_t len) {
        make_room(p, len);
        const int32_t s = (int32_t)pos - (int32_t)dist;
        for (uint32_t k = p.lane(); k < len; k += P::LANES) {
            const int32_t q = s + (int32_t)(dist >= len ? k : k % dist);
            const uint16_t v = q >= 0 ? ring[(uint32_t)q & (INFS_WIN - 1)] : (uint16_t)(0x8000u | (uint32_t)((int32_t)INFS_WIN + q));
            ring[(pos + k) & (INFS_WIN - 1)] = v;
        }
        pos += len;
    }
    __host__ __device__ bool block_end(uint64_t bit, bool fin) {
        end_bit = bit; end_sym = pos; final = fin;
        return fin || bit >= target;
    }
    __host__ __device__ int finish() const { return INF_OK; }
};

// One chunk: decodes from bit `begin` (of policy `pol`, whose first byte is byte `base` of the job's input) and leaves the symbols up
// to its last complete block in `sym`.  What goes out: the boundary's bit position in the job's input, the symbols, the status, BFINAL.
struct InfsChunkResult { uint64_t end_bit; uint32_t n_sym, status, final; };
template <class P> __host__ __device__ static InfsChunkResult infs_chunk(P &pol, InfShared &sh, uint16_t *sym, uint32_t cap, uint32_t before,
                                                                         uint64_t base, uint64_t begin_bit, uint64_t target_bit) {
    InfRingOut o;
    o.ring = reinterpret_cast<uint16_t *>(sh.win); o.sym = sym; o.cap = cap; o.before = before;
    o.target = target_bit - base * 8;
    o.pos = 0; o.stored = 0; o.end_bit = begin_bit - base * 8; o.end_sym = 0; o.final = false; o.far = false;
    int st;
    {
        InfDecoder<P, InfRingOut> d(pol, sh, o);
        st = d.run();
    }
    InfsChunkResult r;
    if (o.far) {  // in front of the member's first byte: nothing of this chunk counts
        r.end_bit = begin_bit; r.n_sym = 0; r.status = INF_E_SYMBOL; r.final = 0;
    } else {
        o.store(pol, (o.end_sym + INFS_GROUP - 1) & ~(INFS_GROUP - 1));  // (the ring still holds everything behind `stored`)
        r.end_bit = base * 8 + o.end_bit; r.n_sym = o.end_sym; r.status = (uint32_t)st; r.final = o.final ? 1u : 0u;
    }
    return r;
}

// Symbols [first, first + n) of a chunk to bytes at buf[0 .. n) through the chunk's window; returns the smallest marker among this
// lane's symbols (INFS_WIN: none).  Lanes take eight symbols at a time; `sym + first` is 16-byte aligned and whole eights may be read.
template <class P> __host__ __device__ static uint32_t infs_bytes(P &p, const uint16_t *sym, uint32_t n, const uint8_t *win, uint8_t *buf) {
    uint32_t low = INFS_WIN;
    for (uint32_t g = p.lane() * 8; g < n; g += P::LANES * 8) {
        const Inf16 v = *reinterpret_cast<const Inf16 *>(sym + g);
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            if (g + j >= n) break;
            const uint32_t s = (v.w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
            uint32_t b = s & 255u;
            if (s & 0x8000u) { const uint32_t w = s & (INFS_WIN - 1); low = w < low ? w : low; b = win[w]; }
            buf[g + j] = (uint8_t)b;
        }
    }
    return low;
}

// host policy of a chunk: InfHostPolicy from the chunk's first byte, the block header `bit0` bits into it
struct InfChunkHostPolicy : InfHostPolicy {
    uint32_t bit0;
    uint64_t bit_begin() const { return bit0; }
};

// the joined CRC-32 of a front piece (crc a) and the n bytes behind it (crc b): zlib's crc32_combine
static inline uint32_t infs_crc_join(uint32_t a, uint32_t b, uint64_t n) {
    uint32_t m = 0x80000000u;
    for (; n; n -= std::min<uint64_t>(n, 1u << 30)) m = inf_crc_mul(m, inf_crc_shift((uint32_t)std::min<uint64_t>(n, 1u << 30)));
    return inf_crc_mul(a, m) ^ b;
}

#ifdef __HIPCC__
// device policy of a chunk: InfWavePolicy from the 16-byte boundary in front of the chunk's first byte; `end` is the end of the job's
// input (bytes behind it read as zero), so the decoder's word position counts from the chunk's own start and stays 32-bit
struct InfChunkWavePolicy : InfWavePolicy {
    uint32_t bit0;
    __device__ uint64_t bit_begin() const { return begin * 8 + bit0; }
};

struct InflateChunkArgs {
    const uint8_t *in;          // byte `first` of the job's input, 16-byte aligned (first is a multiple of 16), INF_PAD bytes behind the end
    uint64_t first, in_bytes;
    const uint64_t *begin_bit, *target_bit;  // [n]
    uint16_t *sym;              // [n] stretches of infs_stride(cap) symbols
    uint32_t cap, before0;      // before0: the window bytes in front of chunk 0
    uint64_t *end_bit;          // [n] out
    uint32_t *n_sym, *status, *final;
    uint32_t *cursor;
    uint32_t n;
};

__global__ void __launch_bounds__(WAVE) k_inflate_chunks(InflateChunkArgs a) {
    __shared__ InfShared sh;
    const uint32_t lane = lane_id();
    const uint64_t stride = infs_stride(a.cap);
    for (;;) {
        uint32_t m = 0;
        if (lane == 0) m = atomicAdd(a.cursor, 1u);
        m = (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
        if (m >= a.n) break;
        const uint64_t bit = a.begin_bit[m], byte = bit >> 3, base = byte & ~15ull;  // byte < in_bytes (checked on the host)
        InfChunkWavePolicy pol;
        pol.abase = a.in + (base - a.first); pol.begin = byte - base; pol.end = a.in_bytes - base; pol.stage = sh.stage;
        pol.bit0 = (uint32_t)(bit & 7);
        pol.start();
        const InfsChunkResult r = infs_chunk(pol, sh, a.sym + (uint64_t)m * stride, a.cap, m == 0 ? a.before0 : INFS_WIN, base, bit, a.target_bit[m]);
        if (lane == 0) { a.end_bit[m] = r.end_bit; a.n_sym[m] = r.n_sym; a.status[m] = r.status; a.final[m] = r.final; }
        pol.sync();  // the ring and the tables are the next chunk's from here
    }
}

// windows down the first n chunks (the proven ones, decided on the host): win[0] is the caller's, win[k + 1] is written here
struct InflateWindowArgs {
    const uint16_t *sym;
    uint64_t stride;
    const uint32_t *n_sym;
    uint8_t *win;  // [n + 1][INFS_WIN]
    uint32_t n;
};
static const uint32_t INFS_WIN_THREADS = 1024;
__global__ void __launch_bounds__(INFS_WIN_THREADS) k_inflate_windows(InflateWindowArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t w[2][INFS_WIN];
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t * 16; i < INFS_WIN; i += INFS_WIN_THREADS * 16) *reinterpret_cast<Inf16 *>(&w[0][i]) = *reinterpret_cast<const Inf16 *>(a.win + i);
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t k = 0; k < a.n; ++k) {
        const uint32_t n = a.n_sym[k], take = n < INFS_WIN ? n : INFS_WIN, keep = INFS_WIN - take;
        const uint16_t *s = a.sym + (uint64_t)k * a.stride + (n - take);
        const uint8_t *old = w[cur];
        uint8_t *nw = w[cur ^ 1];
        for (uint32_t i = t; i < INFS_WIN; i += INFS_WIN_THREADS) {
            uint32_t b;
            if (i < keep) b = old[i + take];
            else { const uint32_t v = s[i - keep]; b = (v & 0x8000u) ? old[v & (INFS_WIN - 1)] : (v & 255u); }
            nw[i] = (uint8_t)b;
        }
        __syncthreads();  // everybody has read `old` (the buffer after next's writes go there) and written `nw`
        uint8_t *dst = a.win + (uint64_t)(k + 1) * INFS_WIN;
        for (uint32_t i = t * 16; i < INFS_WIN; i += INFS_WIN_THREADS * 16) *reinterpret_cast<Inf16 *>(dst + i) = *reinterpret_cast<const Inf16 *>(nw + i);
        cur ^= 1;
    }
}

struct InflateBytesArgs {
    const uint16_t *sym;
    uint64_t stride;
    const uint8_t *win;         // [chunks][INFS_WIN]: every chunk's incoming window
    uint8_t *out;
    const uint64_t *piece;      // [n_pieces] chunk << 32 | first symbol (a multiple of INFS_PIECE)
    const uint64_t *out_off;    // [chunks] where the chunk's bytes go in out
    const uint32_t *n_sym;      // [chunks]
    uint32_t *crc;              // [n_pieces] out
    uint32_t *low;              // [chunks] smallest marker (atomicMin; starts at 0xFFFFFFFF)
};
struct alignas(16) InfsBytesShared {
    uint8_t win[INFS_WIN];
    uint8_t buf[INFS_PIECE + 16];  // byte k of the piece at buf[wmis + k], wmis = the destination's misalignment to 16 bytes
    uint32_t tab[1024];
};
__global__ void __launch_bounds__(WAVE) k_inflate_bytes(InflateBytesArgs a) {
    __shared__ InfsBytesShared sh;
    const uint32_t lane = lane_id();
    const uint64_t pc = a.piece[blockIdx.x];
    const uint32_t c = (uint32_t)(pc >> 32), first = (uint32_t)pc;
    const uint32_t total = a.n_sym[c], n = total - first < INFS_PIECE ? total - first : INFS_PIECE;  // first < total (host)
    const uint8_t *win = a.win + (uint64_t)c * INFS_WIN;
    for (uint32_t i = lane * 16; i < INFS_WIN; i += WAVE * 16) *reinterpret_cast<Inf16 *>(sh.win + i) = *reinterpret_cast<const Inf16 *>(win + i);
    uint8_t *dst = a.out + a.out_off[c] + first;
    const uint32_t wmis = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15);
    InfWavePolicy pol;  // lane(), sync() and the CRC join are what is used of it
    pol.sync();
    uint32_t low = infs_bytes(pol, a.sym + (uint64_t)c * a.stride + first, n, sh.win, sh.buf + wmis);
    for (int o = 32; o > 0; o >>= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)low, o); low = t < low ? t : low; }
    if (lane == 0 && low < INFS_WIN) atomicMin(a.low + c, low);
    pol.sync();
    const uint32_t crc = inf_crc32_at(pol, sh.tab, sh.buf, wmis, n);
    if (lane == 0) a.crc[blockIdx.x] = crc;
    // whole 16-byte pieces as one vector store per lane, the ragged ends byte by byte: never outside [dst, dst + n)
    uint8_t *abase = dst - wmis;
    const uint32_t lo = wmis, hi = wmis + n;
    for (uint32_t b = lane * 16; b < hi; b += WAVE * 16) {
        if (b >= lo && b + 16 <= hi) *reinterpret_cast<Inf16 *>(abase + b) = *reinterpret_cast<const Inf16 *>(sh.buf + b);
        else for (uint32_t i = b > lo ? b : lo; i < b + 16 && i < hi; ++i) abase[i] = sh.buf[i];
    }
}
#endif
