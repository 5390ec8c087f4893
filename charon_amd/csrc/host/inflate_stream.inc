// inflate_stream.inc -- gzip (RFC 1952) / deflate (RFC 1951) decoder for one-stream .gz read files
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a
// stand-alone header.
//
// A read file that is ONE deflate stream has no seams: zlib's single inflate on the reader thread (0.45 GB/s of FASTQ) bounds
// `.gz` input at a tenth of what the rest of the pipeline takes.  This decoder splits the stream anyway:
//   * the compressed file is mapped and cut into chunks; for every chunk but the first a thread SEARCHES the bit position of a
//     dynamic-Huffman block header (a header that parses -- complete code-length, literal/length and distance codes -- and whose
//     block decodes to text) and all chunks are decoded AT ONCE from their block starts without knowing the 32 KiB of output in
//     front of them: a match reaching in front of the chunk leaves 16-bit MARKER symbols that name window positions;
//   * a chunk decodes on until it stands at a block boundary at or behind the next chunk's start position.  Standing EXACTLY on it
//     proves that start was a real block boundary (the first chunk starts at a known one: induction); overshooting it means the
//     search was fooled -- the round then ends with this chunk and the rest is decoded again from where it stands.  So what comes
//     out is what a sequential inflate writes, by construction, not by luck; the CRC32 / ISIZE trailer is checked on top;
//   * windows are passed down the chunks in order (the last 32 KiB of each, markers resolved: cheap), then every chunk's symbols
//     become bytes in parallel and the CRCs of the pieces are joined with crc32_combine.
// (The idea is that of pugz / rapidgzip; the code is this build's own.)  With one thread, or when no block starts are found
// (not text), the same decoder runs sequentially: 64-bit bit buffer refilled eight bytes at a time, two-level tables (11-bit
// literal/length, 9-bit distance first level), output into one buffer that doubles as the window.  It checks what zlib checks:
// code sets (over-subscribed, incomplete, missing end-of-block), distances beyond the member's output, stored-block length
// complements, header flags, CRC32 + ISIZE of every member.  Concatenated members decode as one stream; bytes behind the last
// member that are not a gzip header are ignored, as gzread does.  Anything wrong is a "gzip read error" exception -- never a
// short file (ADVICE r1).

// Slabs of inflated text: byte vectors whose resize() does not zero-fill (every byte is written by an inflate right afterwards;
// zero-filling 256 MB per block on the reader thread is time the other threads wait for).
// CHARON_TEXT_BATCHES=1: slabs of a megabyte and more are page-locked (chn_host_alloc), so that the upload of a batch's text straight out
// of its slab is an asynchronous DMA; g_pinned_slabs remembers which allocations are, for deallocate.  Off: plain operator new as before.
bool g_pin_slabs = false;
struct PinnedSlabs {
    std::mutex m;
    std::unordered_set<void *> v;
    void *take(size_t bytes) {
        void *p = nullptr;
        if (chn_host_alloc(bytes, &p) != CHN_OK || !p) return nullptr;
        std::lock_guard<std::mutex> lk(m);
        v.insert(p);
        return p;
    }
    bool give(void *p) {
        { std::lock_guard<std::mutex> lk(m); if (!v.erase(p)) return false; }
        (void)chn_host_free(p);
        return true;
    }
};
PinnedSlabs g_pinned_slabs;
template <class T> struct NoInitAlloc : std::allocator<T> {
    template <class U> struct rebind { typedef NoInitAlloc<U> other; };
    NoInitAlloc() = default;
    template <class U> NoInitAlloc(const NoInitAlloc<U> &) {}
    T *allocate(size_t n) {
        if (g_pin_slabs && n * sizeof(T) >= ((size_t)1 << 20))
            if (void *p = g_pinned_slabs.take(n * sizeof(T))) return static_cast<T *>(p);
        return std::allocator<T>::allocate(n);
    }
    void deallocate(T *p, size_t n) {
        if (n * sizeof(T) >= ((size_t)1 << 20) && g_pinned_slabs.give(p)) return;
        std::allocator<T>::deallocate(p, n);
    }
    template <class U> void construct(U *p) noexcept { ::new (static_cast<void *>(p)) U; }  // default-initialise: nothing for char
    template <class U, class... A> void construct(U *p, A &&...a) { ::new (static_cast<void *>(p)) U(std::forward<A>(a)...); }
};
typedef std::vector<char, NoInitAlloc<char>> Slab;

// ---- CRC-32 (the gzip trailer's) ------------------------------------------------------------------------------------------
// zlib 1.2.11's crc32() runs at about 1 GB/s; on x86-64 with PCLMULQDQ the same CRC folds 64 bytes per step with carry-less
// multiplies (Gopal et al., "Fast CRC Computation for Generic Polynomials Using PCLMULQDQ Instruction", Intel 2009; fold constants
// for the reflected polynomial 0xEDB88320).  The routine is checked against zlib's crc32() on first use -- lengths that exercise
// every tail -- and zlib's is used if it is absent or disagrees.
#if defined(__x86_64__)
__attribute__((target("pclmul,sse4.1"))) inline uint32_t crc32_clmul_blocks(uint32_t crc, const uint8_t *p, size_t len) {
    // len >= 64 and a multiple of 16; crc is the running value in zlib's convention (pre- and post-inverted by the caller)
    static const uint64_t __attribute__((aligned(16))) k1k2[2] = {0x0154442bd4ULL, 0x01c6e41596ULL};
    static const uint64_t __attribute__((aligned(16))) k3k4[2] = {0x01751997d0ULL, 0x00ccaa009eULL};
    static const uint64_t __attribute__((aligned(16))) k5k0[2] = {0x0163cd6124ULL, 0x0000000000ULL};
    static const uint64_t __attribute__((aligned(16))) poly[2] = {0x01db710641ULL, 0x01f7011641ULL};
    __m128i x0, x1, x2, x3, x4, x5, x6, x7, x8, y5, y6, y7, y8;
    x1 = _mm_loadu_si128(reinterpret_cast<const __m128i *>(p + 0x00));
    x2 = _mm_loadu_si128(reinterpret_cast<const __m128i *>(p + 0x10));
    x3 = _mm_loadu_si128(reinterpret_cast<const __m128i *>(p + 0x20));
    x4 = _mm_loadu_si128(reinterpret_cast<const __m128i *>(p + 0x30));
    x1 = _mm_xor_si128(x1, _mm_cvtsi32_si128((int)crc));
    x0 = _mm_load_si128(reinterpret_cast<const __m128i *>(k1k2));
    p += 64; len -= 64;
    while (len >= 64) {  // four 128-bit lanes, each folded 512 bits forward
        x5 = _mm_clmulepi64_si128(x1, x0, 0x00); x6 = _mm_clmulepi64_si128(x2, x0, 0x00);
        x7 = _mm_clmulepi64_si128(x3, x0, 0x00); x8 = _mm_clmulepi64_si128(x4, x0, 0x00);
        x1 = _mm_clmulepi64_si128(x1, x0, 0x11); x2 = _mm_clmulepi64_si128(x2, x0, 0x11);
        x3 = _mm_clmulepi64_si128(x3, x0, 0x11); x4 = _mm_clmulepi64_si128(x4, x0, 0x11);
        y5 = _mm_loadu_si128(reinterpret_cast<const __m128i *>(p + 0x00)); y6 = _mm_loadu_si128(reinterpret_cast<const __m128i *>(p + 0x10));
        y7 = _mm_loadu_si128(reinterpret_cast<const __m128i *>(p + 0x20)); y8 = _mm_loadu_si128(reinterpret_cast<const __m128i *>(p + 0x30));
        x1 = _mm_xor_si128(_mm_xor_si128(x1, x5), y5); x2 = _mm_xor_si128(_mm_xor_si128(x2, x6), y6);
        x3 = _mm_xor_si128(_mm_xor_si128(x3, x7), y7); x4 = _mm_xor_si128(_mm_xor_si128(x4, x8), y8);
        p += 64; len -= 64;
    }
    x0 = _mm_load_si128(reinterpret_cast<const __m128i *>(k3k4));  // the four lanes into one
    x5 = _mm_clmulepi64_si128(x1, x0, 0x00); x1 = _mm_clmulepi64_si128(x1, x0, 0x11); x1 = _mm_xor_si128(_mm_xor_si128(x1, x2), x5);
    x5 = _mm_clmulepi64_si128(x1, x0, 0x00); x1 = _mm_clmulepi64_si128(x1, x0, 0x11); x1 = _mm_xor_si128(_mm_xor_si128(x1, x3), x5);
    x5 = _mm_clmulepi64_si128(x1, x0, 0x00); x1 = _mm_clmulepi64_si128(x1, x0, 0x11); x1 = _mm_xor_si128(_mm_xor_si128(x1, x4), x5);
    while (len >= 16) {  // remaining whole 16-byte blocks
        x2 = _mm_loadu_si128(reinterpret_cast<const __m128i *>(p));
        x5 = _mm_clmulepi64_si128(x1, x0, 0x00); x1 = _mm_clmulepi64_si128(x1, x0, 0x11); x1 = _mm_xor_si128(_mm_xor_si128(x1, x2), x5);
        p += 16; len -= 16;
    }
    // 128 -> 64 bits
    x2 = _mm_clmulepi64_si128(x1, x0, 0x10);
    x3 = _mm_setr_epi32(~0, 0, ~0, 0);
    x1 = _mm_srli_si128(x1, 8);
    x1 = _mm_xor_si128(x1, x2);
    x0 = _mm_loadl_epi64(reinterpret_cast<const __m128i *>(k5k0));
    x2 = _mm_srli_si128(x1, 4);
    x1 = _mm_and_si128(x1, x3);
    x1 = _mm_clmulepi64_si128(x1, x0, 0x00);
    x1 = _mm_xor_si128(x1, x2);
    // Barrett reduction to 32 bits
    x0 = _mm_load_si128(reinterpret_cast<const __m128i *>(poly));
    x2 = _mm_and_si128(x1, x3);
    x2 = _mm_clmulepi64_si128(x2, x0, 0x10);
    x2 = _mm_and_si128(x2, x3);
    x2 = _mm_clmulepi64_si128(x2, x0, 0x00);
    x1 = _mm_xor_si128(x1, x2);
    return (uint32_t)_mm_extract_epi32(x1, 1);
}
#endif
// crc32() of zlib, faster where the CPU allows it (same arguments and result)
bool g_crc_clmul = false;  // diagnostic: which routine fast_crc32 settled on
inline uint32_t fast_crc32(uint32_t crc, const uint8_t *p, size_t n) {
#if defined(__x86_64__)
    static const bool usable = []() {
        if (std::getenv("CHARON_ZLIB_CRC") || !__builtin_cpu_supports("pclmul") || !__builtin_cpu_supports("sse4.1")) return false;
        std::vector<uint8_t> t(4096 + 77);
        uint32_t x = 0x9E3779B9u;
        for (auto &b : t) { x = x * 1664525u + 1013904223u; b = (uint8_t)(x >> 24); }
        for (size_t len : {(size_t)64, (size_t)80, (size_t)128, (size_t)1024, (size_t)4096 + 64}) {
            const uint32_t start = 0x12345678u ^ (uint32_t)len;
            const uint32_t want = (uint32_t)crc32(start, t.data() + 3, (uInt)len);
            if ((~crc32_clmul_blocks(~start, t.data() + 3, len)) != want) return false;
        }
        g_crc_clmul = true;
        return true;
    }();
    if (usable && n >= 256) {
        const size_t body = n & ~(size_t)15;
        crc = ~crc32_clmul_blocks(~crc, p, body);
        p += body; n -= body;
    }
#endif
    while (n) {  // zlib takes a uInt length
        const size_t step = std::min<size_t>(n, (size_t)1 << 30);
        crc = (uint32_t)crc32(crc, p, (uInt)step);
        p += step; n -= step;
    }
    return crc;
}

int g_reader_threads = 1;  // threads the reader may use (BGZF members, chunks of a deflate stream, bzip2 blocks, FASTQ pieces, CRC slices)
// -t is the reference's OpenMP team for the per-read loop (src/dehost_main.cpp:341); its input streams have threads of their own (seqan3's
// bgzf stream decompresses on several threads whatever -t says).  Here the reader gets the -t threads, and never fewer than four (or the
// CPUs this process may run on) for decompressing and splitting its input: the default -t 1 would otherwise inflate a .gz at a third and
// decode a .bz2 at a quarter of the rate.  The records are the same by construction.  CHARON_READER_THREADS overrides.
// CPUs this process can really keep busy: its affinity mask, cut by the cgroup's CPU quota where there is one (a container may see 256 hardware
// threads and be allowed 16 CPUs' worth of time: teams sized by the former trample each other)
int usable_cpus() {
    int cpus = 1;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) cpus = std::max(1, CPU_COUNT(&set));
    long long quota = -1, period = 0;
    if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "max 100000" or "<quota> <period>"
        char q[32] = {0};
        if (std::fscanf(f, "%31s %lld", q, &period) == 2 && std::strcmp(q, "max") != 0) quota = std::atoll(q);
        std::fclose(f);
    } else {  // cgroup v1
        if (FILE *g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (std::fscanf(g, "%lld", &quota) != 1) quota = -1; std::fclose(g); }
        if (FILE *g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (std::fscanf(g, "%lld", &period) != 1) period = 0; std::fclose(g); }
    }
    if (quota > 0 && period > 0) cpus = std::max(1, std::min<int>(cpus, (int)((quota + period - 1) / period)));
    return cpus;
}
// The reader's team: the -t threads, never fewer than four (eight where half of the usable CPUs are that many).  For PLAIN text input never more than half of the CPUs this process can keep busy,
// since the packing team works beside it and splitting text is cheap (-t 16 on a 16-CPU share: sixteen splitting threads next to sixteen
// packing threads gave 1.36 M reads/s, eight 1.89 M); compressed input is bound by its decompression and gets them all.
int reader_threads_for(int t, bool compressed_input = true) {
    if (const char *e = std::getenv("CHARON_READER_THREADS")) return std::max(1, std::atoi(e));
    const int cpus = usable_cpus();
    const int want = compressed_input ? std::max(1, t) : std::min(std::max(1, t), std::max(1, cpus / 2));
    return std::max(want, std::min(8, std::max(std::min(4, cpus), cpus / 2)));  // never fewer than four -- eight where half the CPUs are that many
}
// does the file start like a gzip member or a bzip2 stream?
bool looks_compressed(const std::string &path) {
    unsigned char m[3] = {0, 0, 0};
    if (FILE *f = std::fopen(path.c_str(), "rb")) { size_t got = std::fread(m, 1, 3, f); std::fclose(f); if (got < 2) return false; }
    return (m[0] == 0x1f && m[1] == 0x8b) || (m[0] == 'B' && m[1] == 'Z' && m[2] == 'h');
}

namespace inflate_core {
enum { WSIZE = 32768, LBITS = 11, DBITS = 9, LIT_CAP = (1 << LBITS) + 288 * 16, DIST_CAP = (1 << DBITS) + 32 * 64 };
// table entry: bits 0-7 codeword bits to consume (link: index bits of the second level), 8-11 kind, 12-15 extra bits, 16-31 value
enum Kind { LITERAL = 0, BASE = 1, END_BLOCK = 2, LINK = 3, INVALID = 4 };
inline uint32_t entry(uint32_t nbits, uint32_t kind, uint32_t extra, uint32_t value) { return nbits | (kind << 8) | (extra << 12) | (value << 16); }
const char *const E_SHORT = "unexpected end of the compressed stream";

struct BitIn {  // least significant bit first
    const uint8_t *ip = nullptr, *end = nullptr;
    uint64_t bb = 0;
    unsigned bc = 0;
    inline void refill() {
        if (end - ip >= 8) {
            uint64_t w;
            std::memcpy(&w, ip, 8);
            bb |= w << bc;
            ip += (63 - bc) >> 3;
            bc |= 56;
        } else {
            while (bc <= 56 && ip < end) { bb |= (uint64_t)*ip++ << bc; bc += 8; }
        }
    }
    void start(const uint8_t *file, const uint8_t *file_end, uint64_t bitpos) {
        ip = file + (bitpos >> 3); end = file_end; bb = 0; bc = 0;
        refill();
        const unsigned r = (unsigned)(bitpos & 7);
        if (bc >= r) { bb >>= r; bc -= r; } else { bb = 0; bc = 0; }
    }
    uint64_t bitpos(const uint8_t *file) const { return (uint64_t)(ip - file) * 8 - bc; }
    inline bool take(unsigned n, uint32_t &v) {  // n <= 32; the caller has refilled
        if (n > bc) return false;
        v = (uint32_t)(bb & ((1ULL << n) - 1));
        bb >>= n; bc -= n;
        return true;
    }
    void byte_align() { const unsigned r = bc & 7; bb >>= r; bc -= r; }
    void unread_bytes() { ip -= bc >> 3; bb = 0; bc = 0; }  // whole bytes in the bit buffer go back to the input pointer
};

struct Tables { uint32_t lit[LIT_CAP], dist[DIST_CAP]; };

inline uint32_t reverse_bits(uint32_t code, unsigned len) {
    uint32_t r = 0;
    for (unsigned i = 0; i < len; ++i) { r = (r << 1) | (code & 1); code >>= 1; }
    return r;
}
// Canonical code from `lens` (RFC 1951 3.2.2) into a two-level table indexed by the next bits of the stream.  sym_entry(s)
// gives kind / extra bits / value of symbol s.  False for a code set zlib rejects: over-subscribed, or incomplete unless it is
// the one-code-of-length-1 case (never for the code-length code); an all-zero set is accepted and decodes nothing.
template <class SymEntry>
bool build(const uint8_t *lens, unsigned n, unsigned root, uint32_t *table, unsigned cap, SymEntry sym_entry, bool may_be_single = true) {
    unsigned count[16] = {0};
    for (unsigned s = 0; s < n; ++s) count[lens[s]]++;
    unsigned maxlen = 15;
    while (maxlen > 0 && count[maxlen] == 0) --maxlen;
    const uint32_t bad = entry(1, INVALID, 0, 0);
    for (unsigned i = 0; i < (1u << root); ++i) table[i] = bad;
    if (maxlen == 0) return true;
    int left = 1;
    for (unsigned l = 1; l <= 15; ++l) { left <<= 1; left -= (int)count[l]; if (left < 0) return false; }
    if (left > 0 && (maxlen != 1 || !may_be_single)) return false;
    unsigned next_code[16], code = 0;
    count[0] = 0;
    for (unsigned l = 1; l <= 15; ++l) { code = (code + count[l - 1]) << 1; next_code[l] = code; }
    // second-level tables: one per first-level prefix that long codes share, as wide as the longest of them
    unsigned used = 1u << root;
    if (maxlen > root) {
        uint8_t sub_bits[1 << LBITS];
        std::memset(sub_bits, 0, (size_t)1 << root);
        unsigned nc[16];
        std::memcpy(nc, next_code, sizeof nc);
        for (unsigned s = 0; s < n; ++s) {
            const unsigned l = lens[s];
            if (l == 0) continue;
            const uint32_t r = reverse_bits(nc[l]++, l);
            if (l > root) { uint8_t &b = sub_bits[r & ((1u << root) - 1)]; b = (uint8_t)std::max<unsigned>(b, l - root); }
        }
        for (unsigned i = 0; i < (1u << root); ++i)
            if (sub_bits[i]) {
                if (used + (1u << sub_bits[i]) > cap) return false;
                table[i] = entry(sub_bits[i], LINK, 0, used);
                for (unsigned j = 0; j < (1u << sub_bits[i]); ++j) table[used + j] = bad;
                used += 1u << sub_bits[i];
            }
    }
    for (unsigned s = 0; s < n; ++s) {
        const unsigned l = lens[s];
        if (l == 0) continue;
        const uint32_t r = reverse_bits(next_code[l]++, l), se = sym_entry(s);
        if (l <= root) {
            for (uint32_t i = r; i < (1u << root); i += 1u << l) table[i] = se | l;
        } else {
            const uint32_t link = table[r & ((1u << root) - 1)];
            const unsigned sb = link & 0xFF, start = link >> 16, rem = l - root;
            for (uint32_t i = r >> root; i < (1u << sb); i += 1u << rem) table[start + i] = se | rem;
        }
    }
    return true;
}
inline uint32_t litlen_entry(unsigned s) {
    static const uint16_t base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    if (s < 256) return entry(0, LITERAL, 0, s);
    if (s == 256) return entry(0, END_BLOCK, 0, 0);
    if (s < 286) return entry(0, BASE, extra[s - 257], base[s - 257]);
    return entry(0, INVALID, 0, 0);
}
inline uint32_t dist_entry(unsigned s) {
    static const uint16_t base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static const uint8_t extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    if (s < 30) return entry(0, BASE, extra[s], base[s]);
    return entry(0, INVALID, 0, 0);
}
inline const Tables &fixed_tables() {
    static const Tables *t = []() {
        Tables *f = new Tables();
        uint8_t lens[288];
        for (unsigned s = 0; s < 288; ++s) lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
        build(lens, 288, LBITS, f->lit, LIT_CAP, litlen_entry);
        for (unsigned s = 0; s < 32; ++s) lens[s] = 5;
        build(lens, 32, DBITS, f->dist, DIST_CAP, dist_entry);
        return f;
    }();
    return *t;
}

// The dynamic block's code tables (the three header bits are already taken).
inline const char *dynamic_header(BitIn &in, Tables &t) {
    uint32_t v;
    in.refill();
    if (!in.take(14, v)) return E_SHORT;
    const unsigned nlen = (v & 31) + 257, ndist = ((v >> 5) & 31) + 1, ncode = (v >> 10) + 4;
    if (nlen > 286 || ndist > 30) return "too many length or distance symbols";
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19] = {0};
    bool any = false;
    for (unsigned i = 0; i < ncode; ++i) {
        if (in.bc < 3) in.refill();
        if (!in.take(3, v)) return E_SHORT;
        cl[order[i]] = (uint8_t)v;
        any = any || v;
    }
    uint32_t cltab[128];
    if (!any || !build(cl, 19, 7, cltab, 128, [](unsigned s) { return entry(0, LITERAL, 0, s); }, false)) return "invalid code lengths set";
    uint8_t lens[286 + 30 + 138];
    unsigned have = 0;
    while (have < nlen + ndist) {
        in.refill();
        const uint32_t e = cltab[in.bb & 127];
        if (((e >> 8) & 0xF) != LITERAL) return "invalid code lengths set";
        if (!in.take(e & 0xFF, v)) return E_SHORT;
        const unsigned sym = e >> 16;
        if (sym < 16) { lens[have++] = (uint8_t)sym; continue; }
        unsigned rep, val = 0;
        if (sym == 16) {
            if (have == 0) return "invalid bit length repeat";
            val = lens[have - 1];
            if (!in.take(2, v)) return E_SHORT;
            rep = 3 + v;
        } else if (sym == 17) {
            if (!in.take(3, v)) return E_SHORT;
            rep = 3 + v;
        } else {
            if (!in.take(7, v)) return E_SHORT;
            rep = 11 + v;
        }
        if (have + rep > nlen + ndist) return "invalid bit length repeat";
        while (rep--) lens[have++] = (uint8_t)val;
    }
    if (lens[256] == 0) return "invalid code -- missing end-of-block";
    if (!build(lens, nlen, LBITS, t.lit, LIT_CAP, litlen_entry)) return "invalid literal/lengths set";
    if (!build(lens + nlen, ndist, DBITS, t.dist, DIST_CAP, dist_entry)) return "invalid distances set";
    return nullptr;
}
// Block header at the reader's position.  type 0: stored_len set and the reader stands byte-aligned on the data; 1 / 2: lt / dt set.
inline const char *block_header(BitIn &in, Tables &dyn, const uint32_t *&lt, const uint32_t *&dt, unsigned &type, bool &final, uint32_t &stored_len) {
    uint32_t v;
    in.refill();
    if (!in.take(3, v)) return E_SHORT;
    final = (v & 1) != 0;
    type = v >> 1;
    if (type == 0) {
        in.byte_align();
        in.refill();
        uint32_t len, nlen;
        if (!in.take(16, len) || !in.take(16, nlen)) return E_SHORT;
        if ((len ^ 0xFFFFu) != nlen) return "invalid stored block lengths";
        stored_len = len;
        return nullptr;
    }
    if (type == 1) { lt = fixed_tables().lit; dt = fixed_tables().dist; return nullptr; }
    if (type == 2) {
        const char *e = dynamic_header(in, dyn);
        lt = dyn.lit; dt = dyn.dist;
        return e;
    }
    return "invalid block type";
}

// Huffman-coded data from the reader's position into base[op ..], until the end of the block (eob) or until op >= lim (then the
// caller makes room or hands the piece on, and calls again).  Output may pass lim by one match (258) plus a wide copy's slack.
//   MARK = false: bytes; the window lies physically in front of `base`; a match may reach reach_before + op bytes back.
//   MARK = true : 16-bit symbols; a match reaching in front of base[0] leaves markers 0x8000 | window index (0 = WSIZE bytes in
//                 front of the chunk, WSIZE - 1 = the byte right in front of it).
//   TEXT        : literals must be text (the block-start search's plausibility test).
template <bool MARK, bool TEXT, class Out>
const char *huffman(BitIn &in_, const uint32_t *lt, const uint32_t *dt, Out *base, size_t &op_, size_t lim, uint64_t reach_before, bool &eob) {
    const uint64_t lmask = (1u << LBITS) - 1, dmask = (1u << DBITS) - 1;
    // the bit reader lives in locals for the length of the loop: stores through `out` may alias anything
    uint64_t bb = in_.bb;
    unsigned bc = in_.bc;
    const uint8_t *ip = in_.ip, *const in_end = in_.end;
    Out *out = base + op_, *const out_lim = base + lim;
    const char *err = nullptr;
    eob = false;
    auto text_ok = [](uint32_t c) { return c == 10 || c == 13 || c == 9 || (c >= 32 && c < 127); };
#define CHN_REFILL()                                                                          \
    do {                                                                                      \
        if (in_end - ip >= 8) {                                                               \
            uint64_t w_; std::memcpy(&w_, ip, 8);                                             \
            bb |= w_ << bc; ip += (63 - bc) >> 3; bc |= 56;                                   \
        } else {                                                                              \
            while (bc <= 56 && ip < in_end) { bb |= (uint64_t)*ip++ << bc; bc += 8; }         \
        }                                                                                     \
    } while (0)
    while (out < out_lim) {
        CHN_REFILL();
        uint32_t e = lt[bb & lmask];
        if ((e & 0xF00) == (LITERAL << 8)) {
            // up to three literals out of one refill (a literal code is at most 15 bits)
            unsigned nb = e & 0xFF;
            if (nb > bc) { err = E_SHORT; break; }
            bb >>= nb; bc -= nb;
            if (TEXT && !text_ok(e >> 16)) { err = "not text"; break; }
            *out++ = (Out)(e >> 16);
            e = lt[bb & lmask];
            if ((e & 0xF00) == (LITERAL << 8) && (nb = e & 0xFF) <= bc) {
                bb >>= nb; bc -= nb;
                if (TEXT && !text_ok(e >> 16)) { err = "not text"; break; }
                *out++ = (Out)(e >> 16);
                e = lt[bb & lmask];
                if ((e & 0xF00) == (LITERAL << 8) && (nb = e & 0xFF) <= bc) {
                    bb >>= nb; bc -= nb;
                    if (TEXT && !text_ok(e >> 16)) { err = "not text"; break; }
                    *out++ = (Out)(e >> 16);
                }
            }
            continue;
        }
        unsigned kind = (e >> 8) & 0xF;
        if (kind == LINK) {
            const unsigned sb = e & 0xFF;
            if (bc < LBITS) { err = E_SHORT; break; }
            bb >>= LBITS; bc -= LBITS;
            e = lt[(e >> 16) + (bb & ((1u << sb) - 1))];
            kind = (e >> 8) & 0xF;
        }
        unsigned nb = e & 0xFF;
        if (nb > bc) { err = E_SHORT; break; }
        bb >>= nb; bc -= nb;
        if (kind == LITERAL) {
            if (TEXT && !text_ok(e >> 16)) { err = "not text"; break; }
            *out++ = (Out)(e >> 16);
            continue;
        }
        if (kind == END_BLOCK) { eob = true; break; }
        if (kind != BASE) { err = "invalid literal/length code"; break; }
        unsigned xb = (e >> 12) & 0xF;
        if (xb > bc) { err = E_SHORT; break; }
        const unsigned len = (e >> 16) + (unsigned)(bb & ((1u << xb) - 1));
        bb >>= xb; bc -= xb;
        if (bc < 32) CHN_REFILL();
        e = dt[bb & dmask];
        kind = (e >> 8) & 0xF;
        if (kind == LINK) {
            const unsigned sb = e & 0xFF;
            if (bc < DBITS) { err = E_SHORT; break; }
            bb >>= DBITS; bc -= DBITS;
            e = dt[(e >> 16) + (bb & ((1u << sb) - 1))];
            kind = (e >> 8) & 0xF;
        }
        if (kind != BASE) { err = "invalid distance code"; break; }
        nb = e & 0xFF;
        xb = (e >> 12) & 0xF;
        if (nb + xb > bc) { err = E_SHORT; break; }
        bb >>= nb;
        const unsigned dist = (e >> 16) + (unsigned)(bb & ((1u << xb) - 1));
        bb >>= xb; bc -= nb + xb;
        Out *const end = out + len;
        if (!MARK) {
            // how far back a match may reach: what this member has produced so far (the window holds WSIZE of it)
            if (dist > reach_before + (uint64_t)(out - base)) { err = "invalid distance too far back"; break; }
            const Out *src = out - dist;
            if (dist >= 8) {
                do { uint64_t w; std::memcpy(&w, src, 8); std::memcpy(out, &w, 8); src += 8; out += 8; } while (out < end);
            } else if (dist == 1) {
                std::memset(out, *src, len);  // a run
            } else {
                // a short period: eight bytes one by one, then eight at a time from a whole number of periods (>= 8 bytes) back
                unsigned i = 0;
                for (; i < 8 && i < len; ++i) out[i] = out[(int)i - (int)dist];
                if (len > 8) {
                    const unsigned back = dist * ((7 + dist) / dist);
                    Out *o = out + 8;
                    const Out *s2 = o - back;
                    do { uint64_t w; std::memcpy(&w, s2, 8); std::memcpy(o, &w, 8); s2 += 8; o += 8; } while (o < end);
                }
            }
        } else {
            const ptrdiff_t s = (out - base) - (ptrdiff_t)dist;
            if (s >= 0) {
                const Out *src = base + s;
                if (dist >= 4) {
                    do { uint64_t w; std::memcpy(&w, src, 8); std::memcpy(out, &w, 8); src += 4; out += 4; } while (out < end);
                } else {
                    // a short period: four symbols one by one, then four at a time from a whole number of periods (>= 4 symbols) back
                    unsigned i = 0;
                    for (; i < 4 && i < len; ++i) out[i] = src[i];
                    if (len > 4) {
                        const unsigned back = dist * ((3 + dist) / dist);
                        Out *o = out + 4;
                        const Out *s2 = o - back;
                        do { uint64_t w; std::memcpy(&w, s2, 8); std::memcpy(o, &w, 8); s2 += 4; o += 4; } while (o < end);
                    }
                }
            } else {
                for (ptrdiff_t q = s; out < end; ++q) *out++ = q >= 0 ? base[q] : (Out)(0x8000u | (uint32_t)(WSIZE + q));
            }
        }
        out = end;
    }
#undef CHN_REFILL
    in_.bb = bb; in_.bc = bc; in_.ip = ip;
    op_ = (size_t)(out - base);
    return err;
}
}  // namespace inflate_core

// CHARON_GPU_INFLATE_STREAM=1 (with CHARON_GPU_INFLATE=1): phases B-D of a parallel round -- decode, windows, bytes and CRC -- are one
// chn_inflate_stream_run on this device; the block-start search stays on the reader's threads
bool g_gpu_inflate_stream = false;
int g_gpu_inflate_stream_device = 0;

class FastInflate {
    typedef inflate_core::BitIn BitIn;
    enum { WSIZE = inflate_core::WSIZE };
public:
    explicit FastInflate(const std::string &path) : path_(path) {}
    ~FastInflate() {
        if (std::getenv("CHARON_DIAG_INFLATE") && t_fill_ > 0)  // (a reader that was opened only to be asked what it is says nothing)
            std::fprintf(stderr, "inflate totals: fill %.3f s; rounds: search %.3f  decode %.3f  windows %.3f  bytes+crc %.3f  (round calls %.3f)\n", t_fill_, t_ph_[0], t_ph_[1], t_ph_[2], t_ph_[3], t_round_);
        if (gpu_) (void)chn_inflate_destroy(gpu_);
        if (map_) ::munmap(const_cast<uint8_t *>(map_), map_size_);
    }
    FastInflate(const FastInflate &) = delete;
    FastInflate &operator=(const FastInflate &) = delete;

    // Maps the file.  False: not a regular file / cannot be mapped / does not start with a gzip header (the caller falls back to
    // zlib's gzopen, which also reads plain files and pipes).
    bool open() {
        const int fd = ::open(path_.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (::fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 18) { ::close(fd); return false; }
        void *m = ::mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        ::close(fd);
        if (m == MAP_FAILED) return false;
        map_ = static_cast<const uint8_t *>(m); map_size_ = (size_t)st.st_size;
        (void)::madvise(m, map_size_, MADV_SEQUENTIAL);
        if (map_[0] != 0x1f || map_[1] != 0x8b) { ::munmap(m, map_size_); map_ = nullptr; return false; }
        in_.ip = map_; in_.end = map_ + map_size_;
        state_ = MEMBER_HEADER;
        work_.assign(WSIZE + 8, 0);
        if (const char *c = std::getenv("CHARON_INFLATE_CHUNK")) chunk_bytes_ = std::max<size_t>(1024, (size_t)std::atol(c));  // tests
        serial_only_ = std::getenv("CHARON_SERIAL_INFLATE") != nullptr;
        gpu_stream_ = g_gpu_inflate_stream && !serial_only_;
        if (gpu_stream_) {
            // more and smaller chunks than the host path's -t chunks of 1 MiB: a chunk is one wavefront's work, and a device has LDS for
            // two workgroups a CU.  Both defaults are guesses that no measurement stands behind.
            if (!std::getenv("CHARON_INFLATE_CHUNK")) chunk_bytes_ = (size_t)256 << 10;
            if (const char *c = std::getenv("CHARON_GPU_INFLATE_ROUND")) gpu_round_ = std::min<size_t>(CHN_INFLATE_STREAM_MAX_CHUNKS, std::max<size_t>(2, (size_t)std::atol(c)));  // tests
        }
        return true;
    }
    // hidden diagnostic (charon _find_blocks): find_block over the mapped file from byte `first` on in ranges of `chunk` bytes, one line
    // a range: from to found, in bits of the file, "-" for none
    void find_blocks_dump(size_t chunk, size_t first, std::ostream &os) const {
        std::vector<uint16_t> scratch;
        for (uint64_t from = (uint64_t)first * 8, end = (uint64_t)map_size_ * 8; from < end; from += (uint64_t)chunk * 8) {
            const uint64_t to = std::min(end, from + (uint64_t)chunk * 8), at = find_block(from, to, scratch);
            os << from << " " << to << " ";
            if (at == NONE) os << "-\n"; else os << at << "\n";
        }
    }
    bool at_end() const { return state_ == DONE && pend_pos_ >= pend_len_; }
    uint64_t parallel_rounds() const { return rounds_; }
    uint64_t chunks_accepted() const { return chunks_ok_; }
    uint64_t chunks_discarded() const { return chunks_lost_; }

    // Appends the next piece of the inflated data to `out`: about max_out bytes (at most 65 KiB more), fewer only when the data ends.
    void fill(Slab &out, size_t max_out) {
        if (max_out < 1) max_out = 1;
        const double t_fill0 = omp_get_wtime();
        struct Lap { double &acc; double t0; ~Lap() { acc += omp_get_wtime() - t0; } } lap{t_fill_, t_fill0};
        out.reserve(out.size() + max_out + 65536 + 400);  // one allocation per slab: growing it round by round copies it again and again
        size_t produced = 0;
        bool parallel_failed = false;
        while (produced < max_out) {
            if (pend_pos_ < pend_len_) {  // what a parallel round left
                const size_t n = std::min(max_out - produced, pend_len_ - pend_pos_);
                out.insert(out.end(), reinterpret_cast<char *>(pending_.data()) + pend_pos_, reinterpret_cast<char *>(pending_.data()) + pend_pos_ + n);
                pend_pos_ += n; produced += n;
                if (pend_pos_ >= pend_len_) { pend_len_ = 0; pend_pos_ = 0; }
                continue;
            }
            if (state_ == DONE) break;
            if (state_ == MEMBER_HEADER) member_header();
            const bool want_parallel = !serial_only_ && (g_reader_threads > 1 || gpu_stream_) && !parallel_failed;
            if (want_parallel && state_ == BLOCK_HEADER) {
                const double tr0 = omp_get_wtime();
                const bool did = gpu_stream_ ? gpu_round(out, max_out - produced, produced) : parallel_round(out, max_out - produced, produced);
                t_round_ += omp_get_wtime() - tr0;
                if (did) continue;
                parallel_failed = true;  // too close to the end, or no block starts found: the rest of this call sequentially
            }
            // a sequential stretch: to the next block boundary if a parallel round is to follow, else as far as the call goes
            produced += sequential(out, max_out - produced, want_parallel && !parallel_failed);
        }
    }

private:
    enum State { MEMBER_HEADER, BLOCK_HEADER, STORED, HUFFMAN, MEMBER_TRAILER, DONE };

    std::string path_;
    const uint8_t *map_ = nullptr;
    size_t map_size_ = 0;
    BitIn in_;
    State state_ = DONE;
    bool final_block_ = false, serial_only_ = false;
    uint32_t stored_left_ = 0;
    uint32_t crc_ = 0;
    uint64_t member_out_ = 0;  // bytes of the current member produced so far
    size_t crc_done_ = 0;
    std::vector<uint8_t> work_;
    inflate_core::Tables dyn_;
    const uint32_t *lt_ = nullptr, *dt_ = nullptr;
    // parallel rounds
    size_t chunk_bytes_ = (size_t)1 << 20;
    std::vector<uint8_t> pending_;   // the last round's bytes (kept allocated from round to round, like the symbol buffers)
    size_t pend_pos_ = 0, pend_len_ = 0;
    std::vector<std::vector<uint16_t>> sym_pool_;
    uint64_t rounds_ = 0, chunks_ok_ = 0, chunks_lost_ = 0;
    unsigned poor_rounds_ = 0;
    double t_fill_ = 0, t_round_ = 0, t_ph_[4] = {0, 0, 0, 0};
    // CHARON_GPU_INFLATE_STREAM=1
    bool gpu_stream_ = false;
    size_t gpu_round_ = 256;  // chunks per round
    chn_inflate *gpu_ = nullptr;

    [[noreturn]] void fail(const char *what) const { throw std::runtime_error("gzip read error in " + path_ + ": " + what); }

    // the last WSIZE bytes of [old window | n new bytes at p] become the window (work_[0 .. WSIZE))
    void keep_window(const uint8_t *p, size_t n) {
        if (n >= WSIZE) std::memcpy(work_.data(), p + n - WSIZE, WSIZE);
        else { std::memmove(work_.data(), work_.data() + n, WSIZE - n); std::memmove(work_.data() + WSIZE - n, p, n); }
    }


    // Sequential decoding of up to about `budget` bytes, appended to out; with to_block_end it stops at the first block boundary.
    // work_ = [last WSIZE bytes of what was produced before | this call's output | slack]: matches read straight out of it.
    size_t sequential(Slab &out, size_t budget, bool to_block_end) {
        work_.resize(WSIZE + budget + 65536 + 320 + 8);
        uint8_t *const base = work_.data() + WSIZE;
        size_t op = 0;
        while (state_ != DONE && op < budget) {
            if (to_block_end && op > 0 && state_ == BLOCK_HEADER) break;
            switch (state_) {
                case MEMBER_HEADER: member_header(); break;
                case BLOCK_HEADER: {
                    unsigned type;
                    const char *e = inflate_core::block_header(in_, dyn_, lt_, dt_, type, final_block_, stored_left_);
                    if (e) fail(e);
                    state_ = type == 0 ? STORED : HUFFMAN;
                    break;
                }
                case STORED: {
                    in_.unread_bytes();  // whole bytes still in the bit buffer belong to the block
                    const size_t want = std::min<size_t>(stored_left_, budget + 65536 - op);
                    if ((size_t)(in_.end - in_.ip) < want) fail(inflate_core::E_SHORT);
                    std::memcpy(base + op, in_.ip, want);
                    in_.ip += want; op += want; stored_left_ -= (uint32_t)want;
                    if (stored_left_ == 0) state_ = final_block_ ? MEMBER_TRAILER : BLOCK_HEADER;
                    break;
                }
                case HUFFMAN: {
                    bool eob = false;
                    const char *e = inflate_core::huffman<false, false, uint8_t>(in_, lt_, dt_, base, op, budget, member_out_ - crc_done_, eob);
                    if (e) fail(e);
                    if (eob) state_ = final_block_ ? MEMBER_TRAILER : BLOCK_HEADER;
                    break;
                }
                case MEMBER_TRAILER:
                    crc_piece(base + crc_done_, op - crc_done_);  // the trailer needs the CRC of everything up to here
                    crc_done_ = op;
                    member_trailer();
                    break;
                default: break;
            }
        }
        crc_piece(base + crc_done_, op - crc_done_);
        crc_done_ = 0;
        out.insert(out.end(), reinterpret_cast<char *>(base), reinterpret_cast<char *>(base) + op);
        keep_window(base, op);
        return op;
    }

    // ---- gzip framing --------------------------------------------------------------------------------------------------
    void member_header() {
        in_.unread_bytes();
        const uint8_t *p = in_.ip;
        const size_t avail = (size_t)(in_.end - p);
        if (avail < 10) fail(inflate_core::E_SHORT);
        if (p[0] != 0x1f || p[1] != 0x8b) fail("incorrect header check");
        if (p[2] != 8) fail("unknown compression method");
        const unsigned flg = p[3];
        if (flg & 0xE0) fail("unknown header flags set");
        size_t q = 10;
        auto need = [&](size_t n) { if (q + n > avail) fail(inflate_core::E_SHORT); };
        if (flg & 4) { need(2); const size_t xlen = (size_t)p[q] | ((size_t)p[q + 1] << 8); q += 2; need(xlen); q += xlen; }
        for (unsigned bit : {8u, 16u})  // FNAME, FCOMMENT: zero-terminated
            if (flg & bit) { for (;;) { need(1); if (p[q++] == 0) break; } }
        if (flg & 2) {  // FHCRC: the low half of the CRC32 of the header so far
            need(2);
            const uint32_t want = (uint32_t)p[q] | ((uint32_t)p[q + 1] << 8);
            if (((uint32_t)crc32(crc32(0L, Z_NULL, 0), p, (uInt)q) & 0xFFFFu) != want) fail("header crc mismatch");
            q += 2;
        }
        in_.ip = p + q;
        crc_ = (uint32_t)crc32(0L, Z_NULL, 0);
        member_out_ = 0;
        state_ = BLOCK_HEADER;
    }
    void member_trailer() {
        in_.byte_align();
        in_.unread_bytes();
        if (in_.end - in_.ip < 8) fail(inflate_core::E_SHORT);
        const uint8_t *t = in_.ip;
        const uint32_t want_crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        const uint32_t want_len = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
        in_.ip += 8;
        if (want_crc != crc_ && !std::getenv("CHARON_DIAG_NO_CRC")) fail("incorrect data check");
        if (want_len != (uint32_t)(member_out_ & 0xFFFFFFFFu)) fail("incorrect length check");
        // another member, or the end (bytes that are not a gzip header are ignored, as gzread does)
        state_ = (in_.end - in_.ip >= 2 && in_.ip[0] == 0x1f && in_.ip[1] == 0x8b) ? MEMBER_HEADER : DONE;
    }
    void crc_piece(const uint8_t *p, size_t n) {
        if (n == 0) return;
        member_out_ += n;
        static const bool skip = std::getenv("CHARON_DIAG_NO_CRC") != nullptr;  // timing diagnostic only
        if (skip) return;
        const int nt = (int)std::min<size_t>((size_t)std::max(1, g_reader_threads), n >> 20);
        if (nt <= 1) { crc_ = fast_crc32(crc_, p, n); return; }
        std::vector<uint32_t> part((size_t)nt);
        const size_t slice = (n + (size_t)nt - 1) / (size_t)nt;
#pragma omp parallel for num_threads(nt) schedule(static, 1)
        for (int t = 0; t < nt; ++t) {
            const size_t b = std::min(n, slice * (size_t)t), e = std::min(n, b + slice);
            part[(size_t)t] = fast_crc32((uint32_t)crc32(0L, Z_NULL, 0), p + b, e - b);
        }
        for (int t = 0; t < nt; ++t) {
            const size_t b = std::min(n, slice * (size_t)t), e = std::min(n, b + slice);
            crc_ = (uint32_t)crc32_combine(crc_, part[(size_t)t], (z_off_t)(e - b));
        }
    }

    // ---- parallel rounds -------------------------------------------------------------------------------------------------
    static const uint64_t NONE = ~0ULL;
    struct Chunk {
        uint64_t begin = ~0ULL, target = 0, end_pos = 0;  // bit positions: start, where the next chunk starts, where this one stopped
        bool last = false, landed = false, final_seen = false;
        const char *err = nullptr;
        std::vector<uint16_t> *symv = nullptr;  // pooled buffer
        size_t n = 0;        // symbols
        size_t out_off = 0;  // where its bytes go in pending_
        uint32_t crc = 0;
        const char *bad_marker = nullptr;
    };

    // First bit position in [from, to) where a dynamic-Huffman block seems to start: the header parses (complete code sets), the
    // block decodes -- as text, with valid codes -- to its end or for 32 Ki symbols, and what follows an end looks like a block
    // header again.  Only a candidate: the chunk in front of it proves or refutes it by where it comes to stand.
    uint64_t find_block(uint64_t from, uint64_t to, std::vector<uint16_t> &scratch) const {
        using namespace inflate_core;
        const uint8_t *const end = map_ + map_size_;
        std::unique_ptr<Tables> t(new Tables());
        scratch.resize(32768 + 600);
        for (uint64_t byte = from >> 3; byte * 8 < to && byte + 8 <= map_size_; ++byte) {
            uint64_t w;
            std::memcpy(&w, map_ + byte, 8);
            for (unsigned r = 0; r < 8; ++r) {
                const uint64_t pos = byte * 8 + r;
                if (pos < from || pos >= to) continue;
                const uint32_t v = (uint32_t)(w >> r);
                // not final, dynamic, at most 286 literal/length and 30 distance codes
                if ((v & 7) != 4 || ((v >> 3) & 31) > 29 || ((v >> 8) & 31) > 29) continue;
                {   // the code-length code must be complete (Kraft sum of its 3-bit lengths exactly 1): few of the survivors pass
                    const unsigned ncode = ((v >> 13) & 15) + 4;
                    const uint64_t at = pos + 17;
                    if ((at >> 3) + 9 > map_size_) continue;
                    uint64_t lo;
                    std::memcpy(&lo, map_ + (at >> 3), 8);
                    const uint64_t x = (lo >> (at & 7)) | ((at & 7) ? (uint64_t)map_[(at >> 3) + 8] << (64 - (at & 7)) : 0);
                    unsigned kraft = 0;
                    for (unsigned i = 0; i < ncode; ++i) { const unsigned l = (unsigned)(x >> (3 * i)) & 7; if (l) kraft += 128u >> l; }
                    if (kraft != 128) continue;
                }
                BitIn in;
                in.start(map_, end, pos + 3);
                if (dynamic_header(in, *t)) continue;
                size_t op = 0;
                bool eob = false;
                if (huffman<true, true, uint16_t>(in, t->lit, t->dist, scratch.data(), op, 32768, 0, eob)) continue;
                if (op < 32) continue;
                if (eob) {  // the next header must be one, too
                    const uint32_t *a, *b;
                    unsigned type; bool fin; uint32_t sl;
                    if (block_header(in, *t, a, b, type, fin, sl)) continue;
                }
                return pos;
            }
        }
        return NONE;
    }

    void decode_chunk(Chunk &c) const {
        using namespace inflate_core;
        BitIn in;
        in.start(map_, map_ + map_size_, c.begin);
        std::unique_ptr<Tables> t(new Tables());
        std::vector<uint16_t> &sym = *c.symv;
        if (sym.size() < chunk_bytes_ * 6 + 70000) sym.resize(chunk_bytes_ * 6 + 70000);
        size_t op = 0;
        for (;;) {
            const uint32_t *lt = nullptr, *dt = nullptr;
            unsigned type; bool fin; uint32_t slen = 0;
            if ((c.err = block_header(in, *t, lt, dt, type, fin, slen))) break;
            if (type == 0) {
                in.unread_bytes();
                if ((size_t)(in.end - in.ip) < slen) { c.err = E_SHORT; break; }
                if (sym.size() < op + slen + 600) sym.resize((op + slen) * 3 / 2 + 70000);
                for (uint32_t i = 0; i < slen; ++i) sym[op + i] = in.ip[i];
                in.ip += slen; op += slen;
            } else {
                for (;;) {
                    if (sym.size() < op + 66000) sym.resize(op * 3 / 2 + 70000);
                    bool eob = false;
                    if ((c.err = huffman<true, false, uint16_t>(in, lt, dt, sym.data(), op, sym.size() - 600, 0, eob))) break;
                    if (eob) break;
                }
                if (c.err) break;
            }
            const uint64_t pos = in.bitpos(map_);
            if (fin) { c.final_seen = true; c.end_pos = pos; break; }
            if (pos >= c.target) { c.end_pos = pos; c.landed = c.last || pos == c.target; break; }
            // a chunk that blows up (a fooled search decoding noise, or extremely repetitive data) stops at this block boundary:
            // the round ends with it and the next one starts here
            if (op > chunk_bytes_ * 32) { c.end_pos = pos; c.landed = false; break; }
        }
        c.n = op;
    }

    // One round: the next chunks of the stream decoded at once.  False: not worth it (the caller decodes on sequentially).
    // The first `budget` bytes of the round go straight to the end of `out` (`produced` grows by them), the rest waits in pending_.
    bool parallel_round(Slab &out, size_t budget, size_t &produced) {
        using namespace inflate_core;
        const uint64_t pos0 = in_.bitpos(map_);
        const size_t byte0 = (size_t)(pos0 >> 3);
        if (map_size_ < byte0 + 8 + 2 * chunk_bytes_) return false;
        const size_t room = map_size_ - 8 - byte0;
        const int nchunks = (int)std::min<size_t>((size_t)g_reader_threads, room / chunk_bytes_);
        if (nchunks < 2) return false;
        std::vector<Chunk> ch((size_t)nchunks);
        if (sym_pool_.size() < (size_t)nchunks) sym_pool_.resize((size_t)nchunks);
        for (int i = 0; i < nchunks; ++i) ch[(size_t)i].symv = &sym_pool_[(size_t)i];
        ch[0].begin = pos0;
        static const bool diag = std::getenv("CHARON_DIAG_INFLATE") != nullptr;
        const double tA = omp_get_wtime();
        const uint64_t round_end = (uint64_t)(byte0 + (size_t)nchunks * chunk_bytes_) * 8;
        // A: block starts
#pragma omp parallel num_threads(nchunks)
        {
            std::vector<uint16_t> scratch;
#pragma omp for schedule(static, 1)
            for (int i = 1; i < nchunks; ++i)
                ch[(size_t)i].begin = find_block((uint64_t)(byte0 + (size_t)i * chunk_bytes_) * 8, (uint64_t)(byte0 + (size_t)(i + 1) * chunk_bytes_) * 8, scratch);
        }
        std::vector<int> order;  // chunks with a start, in stream order
        for (int i = 0; i < nchunks; ++i) if (ch[(size_t)i].begin != NONE) order.push_back(i);
        if (order.size() < 2) {
            // nothing that looks like a block start (stored blocks, not text?): the plain sequential decoder is faster -- and after three such
            // searches (every byte of every chunk, bit by bit) the stream is taken for what it is and no further search is made (ADVICE r2:
            // the search used to repeat on every fill(); 1.2 s against 0.006 s for a 9.5 MB level-0 .gz in 20 kB chunks)
            if (++poor_rounds_ >= 3) serial_only_ = true;
            return false;
        }
        for (size_t k = 0; k < order.size(); ++k) {
            Chunk &c = ch[(size_t)order[k]];
            c.last = k + 1 == order.size();
            c.target = c.last ? round_end : ch[(size_t)order[k + 1]].begin;
        }
        const double tB = omp_get_wtime();
        // B: all chunks at once, markers for what lies in front of them
#pragma omp parallel for num_threads((int)order.size()) schedule(static, 1)
        for (int k = 0; k < (int)order.size(); ++k) decode_chunk(ch[(size_t)order[(size_t)k]]);
        const double tC = omp_get_wtime();
        // C: in order -- a chunk counts if the one before it came to stand exactly on its start
        std::vector<Chunk *> ok;
        for (size_t k = 0; k < order.size(); ++k) {
            Chunk &c = ch[(size_t)order[k]];
            if (c.err) fail(c.err);  // its start is proven (chunk 0: known; others: the predecessor stood on it), so the data is bad
            ok.push_back(&c);
            if (c.final_seen || !c.landed) break;
        }
        chunks_ok_ += ok.size(); chunks_lost_ += order.size() - ok.size(); rounds_ += 1;
        // rounds that keep counting a single chunk (output that expands beyond the cap: data far more repetitive than read files are;
        // or a search that keeps being fooled) cost more than they bring: after three of them the stream goes on sequentially
        if (ok.size() == 1 && order.size() > 1 && ++poor_rounds_ >= 3) serial_only_ = true;
        // windows down the chunks: window[k + 1] = last WSIZE bytes of (window[k] | chunk k), markers resolved against window[k]
        std::vector<std::vector<uint8_t>> win(ok.size() + 1);
        std::vector<uint64_t> reach(ok.size() + 1);
        win[0].assign(work_.data(), work_.data() + WSIZE);
        reach[0] = std::min<uint64_t>(member_out_, WSIZE);
        size_t total = 0;
        for (size_t k = 0; k < ok.size(); ++k) {
            const Chunk &c = *ok[k];
            ok[k]->out_off = total;
            total += c.n;
            std::vector<uint8_t> &nw = win[k + 1];
            nw.resize(WSIZE);
            const size_t take = std::min<size_t>(c.n, WSIZE);
            if (take < WSIZE) std::memcpy(nw.data(), win[k].data() + take, WSIZE - take);
            for (size_t i = 0; i < take; ++i) {
                const uint16_t s = (*c.symv)[c.n - take + i];
                nw[WSIZE - take + i] = (s & 0x8000u) ? win[k][s & 0x7FFFu] : (uint8_t)s;
            }
            reach[k + 1] = std::min<uint64_t>(reach[k] + c.n, WSIZE);
        }
        const double tD = omp_get_wtime();
        // D: symbols to bytes (straight into the caller's buffer as far as its budget goes), CRC per chunk
        const size_t direct = std::min(total, budget), old_size = out.size();
        out.resize(old_size + direct);
        if (pending_.size() < total - direct) pending_.resize(total - direct);
        pend_pos_ = 0; pend_len_ = total - direct;
        uint8_t *const out_base = reinterpret_cast<uint8_t *>(out.data()) + old_size;
        static const bool skip_crc = std::getenv("CHARON_DIAG_NO_CRC") != nullptr;
#pragma omp parallel for num_threads((int)ok.size()) schedule(static, 1)
        for (int k = 0; k < (int)ok.size(); ++k) {
            Chunk &c = *ok[(size_t)k];
            const uint8_t *w = win[(size_t)k].data();
            const uint32_t lowest = (uint32_t)(WSIZE - reach[(size_t)k]);  // window positions below this are not the member's data
            uint32_t min_marker = WSIZE;
            const uint16_t *s = c.symv->data();
            // Where the whole window is the member's data (always, but for a member's first 32 KiB) no marker can be out of range and
            // symbols go through one table: repetitive reads keep markers alive for the length of a chunk (a quality line copied
            // from the line before it, which was copied from ...), so the marker path has to be as cheap as the literal path.
            const bool whole_window = lowest == 0;
            std::vector<uint8_t> lut_store;
            const uint8_t *lut = nullptr;
            if (whole_window) {
                lut_store.resize(65536);
                for (unsigned v = 0; v < 256; ++v) lut_store[v] = (uint8_t)v;
                std::memcpy(lut_store.data() + 0x8000, w, WSIZE);
                lut = lut_store.data();
            }
            // the chunk's bytes [0, n) lie at round offsets [out_off, out_off + n): those below `direct` in out, the others in pending_
            const size_t n_out = c.out_off >= direct ? 0 : std::min(c.n, direct - c.out_off);
            uint32_t crc = (uint32_t)crc32(0L, Z_NULL, 0);
            for (int part = 0; part < 2; ++part) {
                const size_t b = part == 0 ? 0 : n_out, e = part == 0 ? n_out : c.n;
                if (e <= b) continue;
                uint8_t *dst = part == 0 ? out_base + c.out_off : pending_.data() + (c.out_off + b - direct);
                // 32 KiB at a time: bytes, then their CRC while they are still in the cache
                for (size_t blk = b; blk < e; blk += 32768) {
                    const size_t blk_end = std::min(e, blk + 32768);
                    size_t i = blk;
                    while (i < blk_end) {
#if defined(__x86_64__)
                        // sixteen symbols at a time while none of them is a marker (markers thin out behind a chunk's first 32 KiB)
                        if (i + 16 <= blk_end) {
                            const __m128i lo = _mm_loadu_si128(reinterpret_cast<const __m128i *>(s + i)), hi = _mm_loadu_si128(reinterpret_cast<const __m128i *>(s + i + 8));
                            if ((_mm_movemask_epi8(_mm_or_si128(lo, hi)) & 0xAAAA) == 0) {
                                _mm_storeu_si128(reinterpret_cast<__m128i *>(dst + (i - b)), _mm_packus_epi16(lo, hi));
                                i += 16;
                                continue;
                            }
                            if (whole_window) {  // markers among them: sixteen look-ups, no test in between
                                for (unsigned j = 0; j < 16; ++j) dst[i - b + j] = lut[s[i + j]];
                                i += 16;
                                continue;
                            }
                        }
#endif
                        const uint16_t v = s[i];
                        if (whole_window) {
                            dst[i - b] = lut[v];  // one unconditional look-up: literals map to themselves, markers to the window's byte
                        } else if (v & 0x8000u) {
                            const uint32_t idx = v & 0x7FFFu; min_marker = std::min(min_marker, idx); dst[i - b] = w[idx];
                        } else {
                            dst[i - b] = (uint8_t)v;
                        }
                        ++i;
                    }
                    if (!skip_crc) crc = fast_crc32(crc, dst + (blk - b), blk_end - blk);
                }
            }
            if (min_marker < lowest) c.bad_marker = "invalid distance too far back";
            c.crc = crc;
        }
        produced += direct;
        for (Chunk *c : ok) {
            if (c->bad_marker) fail(c->bad_marker);
            if (!skip_crc && c->n) crc_ = (uint32_t)crc32_combine(crc_, c->crc, (z_off_t)c->n);
        }
        t_ph_[0] += tB - tA; t_ph_[1] += tC - tB; t_ph_[2] += tD - tC; t_ph_[3] += omp_get_wtime() - tD;
        if (diag && std::getenv("CHARON_DIAG_INFLATE_ROUNDS")) std::fprintf(stderr, "inflate round: %d chunks, %zu with a start, %zu counted; search %.1f ms, decode %.1f ms, windows %.1f ms, bytes+crc %.1f ms; %zu bytes out\n",
                               nchunks, order.size(), ok.size(), (tB - tA) * 1e3, (tC - tB) * 1e3, (tD - tC) * 1e3, (omp_get_wtime() - tD) * 1e3, total);
        member_out_ += total;
        std::memcpy(work_.data(), win[ok.size()].data(), WSIZE);
        // the stream stands where the last counted chunk stopped
        const Chunk &lastc = *ok.back();
        in_.start(map_, map_ + map_size_, lastc.end_pos);
        final_block_ = lastc.final_seen;
        state_ = lastc.final_seen ? MEMBER_TRAILER : BLOCK_HEADER;
        return true;
    }

    // One round with phases B-D on the device (CHARON_GPU_INFLATE_STREAM=1): the search as in parallel_round, then ONE
    // chn_inflate_stream_run over the round's stretch of the mapped file -- its counting rule is the induction of phase C, its window the
    // reader's kept window, its per-chunk CRCs are joined as phase D's.  The round's bytes arrive in pending_; the first `budget` of them
    // are copied to the end of `out`.  False: no progress possible this way (fewer than two starts; chunk 0 stopped for want of input,
    // symbol capacity or room, or on corrupt data, without a complete block) -- the caller decodes on sequentially, and it is the
    // sequential decoder that names what is wrong with a corrupt stream, in the words and with the exit status of the host path.
    bool gpu_round(Slab &out, size_t budget, size_t &produced) {
        const uint64_t pos0 = in_.bitpos(map_);
        const size_t byte0 = (size_t)(pos0 >> 3);
        if (map_size_ < byte0 + 8 + 2 * chunk_bytes_) return false;
        const size_t room = map_size_ - 8 - byte0;
        const int nchunks = (int)std::min<size_t>(gpu_round_, room / chunk_bytes_);
        if (nchunks < 2) return false;
        const double tA = omp_get_wtime();
        std::vector<uint64_t> found((size_t)nchunks, NONE);
        found[0] = pos0;
#pragma omp parallel num_threads(std::max(1, std::min(g_reader_threads, nchunks - 1)))
        {
            std::vector<uint16_t> scratch;
#pragma omp for schedule(dynamic, 1)
            for (int i = 1; i < nchunks; ++i)
                found[(size_t)i] = find_block((uint64_t)(byte0 + (size_t)i * chunk_bytes_) * 8, (uint64_t)(byte0 + (size_t)(i + 1) * chunk_bytes_) * 8, scratch);
        }
        std::vector<uint64_t> begin, target;  // bit positions from byte0
        for (int i = 0; i < nchunks; ++i) if (found[(size_t)i] != NONE) begin.push_back(found[(size_t)i] - (uint64_t)byte0 * 8);
        if (begin.size() < 2) {
            if (++poor_rounds_ >= 3) serial_only_ = true;
            return false;
        }
        const size_t n = begin.size();
        const uint64_t round_end = (uint64_t)nchunks * chunk_bytes_ * 8;
        for (size_t k = 0; k < n; ++k) target.push_back(k + 1 < n ? begin[k + 1] : round_end);
        const double tB = omp_get_wtime();
        if (!gpu_ && chn_inflate_create(g_gpu_inflate_stream_device, &gpu_) != CHN_OK)
            throw std::runtime_error(std::string("CHARON_GPU_INFLATE_STREAM: ") + chn_last_error());
        // the last chunk decodes on to a block boundary behind the round's end: a block more of input.  What a chunk may produce and what
        // the round may produce are bounds: a chunk or a round beyond them ends the chain there (status 5 / CHN_INFLATE_E_ROOM)
        const size_t stretch = std::min(map_size_ - byte0, (size_t)nchunks * chunk_bytes_ + std::max<size_t>(chunk_bytes_, (size_t)256 << 10));
        const size_t out_room = (size_t)nchunks * chunk_bytes_ * 6 + 65536;
        if (pending_.size() < out_room) pending_.resize(out_room);
        std::vector<uint64_t> end_bit(n), out_length(n);
        std::vector<uint32_t> status(n), crc(n);
        std::vector<uint8_t> fin(n);
        uint64_t counted = 0, used = 0;
        const uint64_t reach = std::min<uint64_t>(member_out_, WSIZE);
        chn_inflate_stream_job job;
        std::memset(&job, 0, sizeof job);
        job.struct_size = sizeof job; job.n_chunks = n;
        job.in = map_ + byte0; job.in_bytes = stretch;
        job.begin_bit = begin.data(); job.target_bit = target.data();
        job.window = work_.data() + WSIZE - reach; job.window_bytes = reach;
        job.sym_capacity = std::max<uint64_t>(CHN_INFLATE_STREAM_MIN_SYMS, (uint64_t)chunk_bytes_ * 12);
        job.out = pending_.data(); job.out_bytes = out_room;
        job.end_bit = end_bit.data(); job.out_length = out_length.data(); job.status = status.data(); job.final = fin.data(); job.crc32 = crc.data();
        job.n_counted = &counted; job.out_used = &used;
        if (chn_inflate_stream_run(gpu_, &job) != CHN_OK) throw std::runtime_error(std::string("CHARON_GPU_INFLATE_STREAM: ") + chn_last_error());
        const double tC = omp_get_wtime();
        // the stream stands where the last counted chunk that came forward at all stopped
        size_t last = 0;
        bool any = false;
        for (size_t k = 0; k < counted; ++k) if (end_bit[k] > begin[k]) { last = k; any = true; }
        const uint32_t why = status[counted ? counted - 1 : 0];
        if (why == 2 || why == 3 || why == 4) serial_only_ = true;  // corrupt where its start is proven: the sequential decoder says what it is
        if (!any) {
            if (++poor_rounds_ >= 3) serial_only_ = true;
            return false;
        }
        chunks_ok_ += last + 1; chunks_lost_ += n - (last + 1); rounds_ += 1;
        if (last == 0 && ++poor_rounds_ >= 3) serial_only_ = true;
        static const bool skip_crc = std::getenv("CHARON_DIAG_NO_CRC") != nullptr;
        size_t total = 0;
        for (size_t k = 0; k <= last; ++k) {
            if (!skip_crc && out_length[k]) crc_ = (uint32_t)crc32_combine(crc_, crc[k], (z_off_t)out_length[k]);
            total += (size_t)out_length[k];
        }
        const size_t direct = std::min(total, budget);
        out.insert(out.end(), reinterpret_cast<char *>(pending_.data()), reinterpret_cast<char *>(pending_.data()) + direct);
        pend_pos_ = direct; pend_len_ = total;
        if (pend_pos_ >= pend_len_) { pend_pos_ = 0; pend_len_ = 0; }
        produced += direct;
        member_out_ += total;
        keep_window(pending_.data(), total);
        in_.start(map_, map_ + map_size_, (uint64_t)byte0 * 8 + end_bit[last]);
        final_block_ = fin[last] != 0;
        state_ = final_block_ ? MEMBER_TRAILER : BLOCK_HEADER;
        t_ph_[0] += tB - tA; t_ph_[1] += tC - tB; t_ph_[3] += omp_get_wtime() - tC;
        static const bool diag = std::getenv("CHARON_DIAG_INFLATE") != nullptr;
        if (diag && std::getenv("CHARON_DIAG_INFLATE_ROUNDS")) {
            double ms = 0;
            (void)chn_inflate_kernel_ms(gpu_, &ms);
            std::fprintf(stderr, "inflate round (device): %d chunks, %zu with a start, %zu counted; search %.1f ms, chn_inflate_stream_run %.1f ms (kernels %.1f ms); %zu bytes out\n",
                         nchunks, n, last + 1, (tB - tA) * 1e3, (tC - tB) * 1e3, ms, total);
        }
        return true;
    }
};
