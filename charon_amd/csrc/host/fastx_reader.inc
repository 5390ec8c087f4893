// fastx_reader.inc -- FASTA/FASTQ(.gz, .bz2) block reader, dna5 code table, per-thread deflater
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a
// stand-alone header.

// ---------------------------------------------------------------------------------------------------
// FASTA / FASTQ block reader (seqan3::sequence_file_input<my_traits> semantics, include/utils.hpp:17-19): format by
// extension, optional .gz, dna5 alphabet (IUPAC -> N, lower case accepted, anything else is a parse error).
// A block is a large slab of the (inflated) file holding whole records; records are views into the slab (multi-line
// sequences are compacted in place), so nothing is copied per record and blocks can be parsed on a reader thread while
// the previous block is packed / compressed / classified.
// ---------------------------------------------------------------------------------------------------
struct RecView {
    const char *id = nullptr, *seq = nullptr, *qual = nullptr;
    uint32_t id_len = 0, seq_len = 0, qual_len = 0;
};
// A mapped read file's identity: ranges handed back for release name it, so that a range can never be applied to another mapping
// that happens to live at the same addresses later (a FASTA mapping holds in-place compacted -- private, dirty -- pages).
struct MapToken { std::atomic<bool> alive{true}; };
struct RawBlock {
    Slab buf;
    std::vector<RecView> recs;
    char *map_begin = nullptr;  // mapped input: the stretch of the mapping these records are views into
    size_t map_len = 0;
    std::shared_ptr<MapToken> map_token;
};

// Stretches of a mapped read file whose records are all printed: the reader thread (idle most of the time) drops their pages
// while the run goes on, instead of the kernel doing it page by page after the last row (0.1 s for a 4 GB file).
struct DeadRanges {
    struct Range { std::shared_ptr<MapToken> token; char *p; size_t n; };
    std::mutex m;
    std::vector<Range> v;
    void add(const std::shared_ptr<MapToken> &token, char *p, size_t n) {
        if (token && p && n) { std::lock_guard<std::mutex> lk(m); v.push_back(Range{token, p, n}); }
    }
    // the ranges of this mapping: taken off the list and released (whole pages strictly inside each range); ranges of mappings
    // that are gone are dropped on the way
    void release_for(const std::shared_ptr<MapToken> &token) {
        std::vector<Range> mine;
        {
            std::lock_guard<std::mutex> lk(m);
            for (size_t i = 0; i < v.size();) {
                if (v[i].token == token) mine.push_back(v[i]);
                if (v[i].token == token || !v[i].token->alive.load()) { v[i] = v.back(); v.pop_back(); } else ++i;
            }
        }
        const uintptr_t page = (uintptr_t)::sysconf(_SC_PAGESIZE);
        for (auto &r : mine) {
            const uintptr_t b = ((uintptr_t)r.p + page - 1) & ~(page - 1), e = ((uintptr_t)r.p + r.n) & ~(page - 1);
            if (e > b) (void)::madvise(reinterpret_cast<void *>(b), e - b, MADV_DONTNEED);
        }
    }
};
DeadRanges g_dead_ranges;

// Slabs of inflated text go round: a batch's slab returns here when its rows are printed and the reader thread fills it again
// (a fresh 256 MB vector per block is 65 000 page faults on the thread the others wait for).
struct SlabPool {
    std::mutex m;
    std::vector<Slab> v;
    void give(Slab &b) {
        if (b.capacity() < ((size_t)1 << 20)) return;
        std::lock_guard<std::mutex> lk(m);
        if (v.size() < 8) { b.clear(); v.emplace_back(std::move(b)); }
    }
    Slab take() {
        std::lock_guard<std::mutex> lk(m);
        if (v.empty()) return Slab();
        Slab b = std::move(v.back());
        v.pop_back();
        return b;
    }
};
SlabPool g_slab_pool;

// BGZF input (bgzip / htslib / Illumina BCL Convert output): a series of gzip members of at most 64 KiB, each carrying its own
// compressed size in a 'BC' extra subfield (SAM specification, section 4.1).  Members are therefore found without inflating anything
// and inflated in parallel -- what seqan3's bgzf input stream does for the reference's reader (src/dehost_main.cpp:324,335-339).
// An ordinary .gz is ONE deflate stream and stays on zlib's single inflate (about 0.4 GB/s).
// CHARON_GPU_INFLATE=1: the members of a block are inflated on the device (chn_inflate_run_crc) instead of in the OpenMP loop below; the
// size and the CRC-32 of every member are checked there too, against the trailers' values, and come back as the member's status.
bool g_gpu_inflate = false;
int g_gpu_inflate_device = 0;
double g_gpu_inflate_s = 0;  // reader-thread seconds inside chn_inflate_run_crc (CHARON_TIMING)

// CHARON_GPU_TEXT=1 (single-end BGZF FASTQ): the members of a block are inflated into DEVICE memory (CHN_INFLATE_OUT_DEVICE) and the text
// stays there; the main thread finds the records (chn_text_split), submits them (CHN_TEXT_ON_DEVICE) and fetches the letters of the few
// reads the host still needs (chn_text_fetch).  A block's buffer keeps `headroom` bytes free in front of member 0: the tail the block
// before left over is copied there, device to device, so that it ends exactly where member 0 begins.
bool g_gpu_text = false;
int g_gpu_text_device = 0;
size_t g_gpu_text_headroom = (size_t)4 << 20;  // longer than any read but the rarest (those take a fresh buffer); CHARON_GPU_TEXT_HEADROOM: test hook
uint64_t g_gpu_text_inflated = 0;              // text bytes inflated into device memory (CHARON_TIMING)
// CHARON_GPU_TEXT_PAIRS=1 (with CHARON_GPU_TEXT=1; paired BGZF FASTQ): each file has a reader thread of its own that fills device
// buffers, so the counters the readers add to are guarded, and twice as many buffers exist (below)
bool g_gpu_text_pairs = false;
// CHARON_GPU_TEXT_FASTA=1 (with CHARON_GPU_TEXT=1; single-end BGZF FASTA): the same loop with chn_fasta_split in place of chn_text_split.
// Every block has a second buffer of the pool for the unwrapped letters, which is the text the batches are submitted and fetched from.
bool g_gpu_text_fasta = false;
std::mutex g_reader_stat_m;
// The buffers go round: the reader fills one while two wait in the queue, the main thread splits one and up to two batches in flight
// refer to theirs.  All have one size, so any free one fits; more than four free ones are not kept.
struct DevTextPool {
    std::mutex m;
    std::vector<void *> v;
    size_t bytes = 0;  // size of every pooled buffer
    size_t keep = 4;   // free buffers kept (eight with two readers: CHARON_GPU_TEXT_PAIRS=1)
    void *take(size_t want) {
        {
            std::lock_guard<std::mutex> lk(m);
            if (bytes != want) { for (void *p : v) (void)chn_device_free(g_gpu_text_device, p); v.clear(); bytes = want; }
            if (!v.empty()) { void *p = v.back(); v.pop_back(); return p; }
        }
        void *p = nullptr;
        if (chn_device_malloc(g_gpu_text_device, want, &p) != CHN_OK || !p) throw std::runtime_error(std::string("CHARON_GPU_TEXT: ") + chn_last_error());
        return p;
    }
    void give(void *p, size_t n) {
        {
            std::lock_guard<std::mutex> lk(m);
            if (n == bytes && v.size() < keep) { v.push_back(p); return; }
        }
        (void)chn_device_free(g_gpu_text_device, p);
    }
    void drain() { std::lock_guard<std::mutex> lk(m); for (void *p : v) (void)chn_device_free(g_gpu_text_device, p); v.clear(); }
};
DevTextPool g_dev_text_pool;
// One block of inflated text in device memory: the tail of the block before in [start, member0), this block's members in
// [member0, text_bytes).  Byte x of it is byte file_offset + (x - member0) of the inflated file.
struct DevBlock {
    uint8_t *buf = nullptr;
    size_t cap = 0;
    bool pooled = false;
    uint64_t member0 = 0, text_bytes = 0, file_offset = 0;
    size_t z_end = 0;   // offset in the compressed file behind this block's last member
    bool last = false;  // no member follows
    DevBlock() = default;
    DevBlock(const DevBlock &) = delete;
    DevBlock &operator=(const DevBlock &) = delete;
    ~DevBlock() {
        if (!buf) return;
        if (pooled) g_dev_text_pool.give(buf, cap); else (void)chn_device_free(g_gpu_text_device, buf);
    }
};

class BgzfSource {
    chn_inflate *gpu_ = nullptr;  // one handle per source, created on first use
    const unsigned char *z_ = nullptr;
    size_t size_ = 0, pos_ = 0;
    std::string path_;
    struct Member { const unsigned char *cdata; uint32_t clen, isize, crc; size_t out; };
    // total size of the member starting at p (0: not a BGZF member / not enough bytes), and where its deflate data starts
    static size_t member(const unsigned char *p, size_t avail, size_t &data_off) {
        if (avail < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return 0;  // FLG: FEXTRA and nothing else
        const size_t xlen = (size_t)p[10] | ((size_t)p[11] << 8);
        if (avail < 12 + xlen) return 0;
        for (size_t q = 12; q + 4 <= 12 + xlen;) {
            const size_t slen = (size_t)p[q + 2] | ((size_t)p[q + 3] << 8);
            if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2 && q + 6 <= 12 + xlen) {
                const size_t total = ((size_t)p[q + 4] | ((size_t)p[q + 5] << 8)) + 1;
                if (total < 12 + xlen + 8) return 0;
                data_off = 12 + xlen;
                return total;
            }
            q += 4 + slen;
        }
        return 0;
    }
public:
    ~BgzfSource() {
        if (gpu_) (void)chn_inflate_destroy(gpu_);
        if (z_) ::munmap(const_cast<unsigned char *>(z_), size_);
    }
    // true if `path` starts with a BGZF member (the file is then mapped)
    bool open(const std::string &path) {
        path_ = path;
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        unsigned char head[64];
        size_t off = 0;
        const ssize_t got = ::pread(fd, head, sizeof head, 0);
        if (::fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || got < 18 || member(head, (size_t)got, off) == 0) { ::close(fd); return false; }
        void *m = ::mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        ::close(fd);
        if (m == MAP_FAILED) return false;
        z_ = static_cast<const unsigned char *>(m); size_ = (size_t)st.st_size;
        (void)::madvise(m, size_, MADV_SEQUENTIAL);
        return true;
    }
    bool at_end() const { return pos_ >= size_; }
    void seek(size_t pos) { pos_ = pos; }  // to a member boundary (DevBlock::z_end)
    // The next members, as many as fit max_out bytes (at least one non-empty one while there is data); returns the bytes they inflate to.
    size_t scan(std::vector<Member> &ms, size_t max_out) {
        size_t total = 0;
        while (pos_ < size_) {
            size_t off = 0;
            const size_t len = member(z_ + pos_, size_ - pos_, off);
            if (len == 0 || len > size_ - pos_)
                throw std::runtime_error("gzip read error in " + path_ + ": " + (len ? "unexpected end of the compressed stream" : "not a BGZF member where one is expected"));
            const unsigned char *tail = z_ + pos_ + len - 8;
            Member mb;
            mb.cdata = z_ + pos_ + off; mb.clen = (uint32_t)(len - off - 8);
            mb.crc = (uint32_t)tail[0] | ((uint32_t)tail[1] << 8) | ((uint32_t)tail[2] << 16) | ((uint32_t)tail[3] << 24);
            mb.isize = (uint32_t)tail[4] | ((uint32_t)tail[5] << 8) | ((uint32_t)tail[6] << 16) | ((uint32_t)tail[7] << 24);
            if (mb.isize > 65536) throw std::runtime_error("gzip read error in " + path_ + ": BGZF member larger than 64 KiB");
            if (total && total + mb.isize > max_out) break;
            mb.out = total; total += mb.isize;
            ms.push_back(mb);
            pos_ += len;
        }
        return total;
    }
    // CHARON_GPU_TEXT=1: the next members inflated into a device buffer of the pool, member 0 at `headroom`; size and CRC-32 of every
    // member are checked on the device as under CHARON_GPU_INFLATE=1.  Null when no member is left.
    std::shared_ptr<DevBlock> fill_device(size_t max_out, size_t headroom, uint64_t file_offset) {
        if (pos_ >= size_) return nullptr;
        std::vector<Member> ms;
        const size_t total = scan(ms, max_out);
        std::shared_ptr<DevBlock> b(new DevBlock());
        b->cap = (headroom + max_out + 65536 + 15) & ~(size_t)15;
        b->buf = static_cast<uint8_t *>(g_dev_text_pool.take(b->cap)); b->pooled = true;
        b->member0 = headroom; b->text_bytes = headroom + total; b->file_offset = file_offset;
        b->z_end = pos_; b->last = pos_ >= size_;
        if (!gpu_ && chn_inflate_create(g_gpu_text_device, &gpu_) != CHN_OK) throw std::runtime_error(std::string("CHARON_GPU_TEXT: ") + chn_last_error());
        const size_t n = ms.size();
        std::vector<uint64_t> in_off(n), out_off(n);
        std::vector<uint32_t> in_len(n), out_len(n), status(n, 0), expected(n);
        for (size_t i = 0; i < n; ++i) {
            in_off[i] = (uint64_t)(ms[i].cdata - z_); in_len[i] = ms[i].clen;
            out_off[i] = headroom + ms[i].out; out_len[i] = ms[i].isize;
            expected[i] = ms[i].crc;
        }
        chn_inflate_job job;
        std::memset(&job, 0, sizeof job);
        job.struct_size = sizeof job; job.flags = CHN_INFLATE_OUT_DEVICE; job.n_members = n;
        job.in = z_; job.in_bytes = size_; job.in_offset = in_off.data(); job.in_length = in_len.data();
        job.out = b->buf; job.out_bytes = b->text_bytes; job.out_offset = out_off.data(); job.out_length = out_len.data();
        job.status = status.data();
        chn_inflate_crc crc;
        std::memset(&crc, 0, sizeof crc);
        crc.struct_size = sizeof crc; crc.expected = expected.data();
        const double t0 = omp_get_wtime();
        if (chn_inflate_run_crc(gpu_, &job, &crc) != CHN_OK) throw std::runtime_error(std::string("CHARON_GPU_TEXT: ") + chn_last_error());
        {
            std::lock_guard<std::mutex> lk(g_reader_stat_m);
            g_gpu_inflate_s += omp_get_wtime() - t0;
            g_gpu_text_inflated += total;
        }
        for (size_t i = 0; i < n; ++i)
            if (status[i] != 0) throw std::runtime_error("gzip read error in " + path_ + ": a BGZF member is corrupt (inflate, size or CRC32 mismatch)");
        return b;
    }
    // Append the next members' data to buf: as many members as fit max_out bytes (at least one non-empty one while there is data).
    void fill(Slab &buf, size_t max_out) {
        std::vector<Member> ms;
        buf.reserve(buf.size() + max_out + 65536);
        const size_t total = scan(ms, max_out);
        const size_t old = buf.size();
        buf.resize(old + total);
        char *dst = buf.data() + old;
        bool bad = false;
        const int nt = std::max(1, std::min<int>(g_reader_threads, (int)ms.size()));
        if (g_gpu_inflate) {
            if (!gpu_ && chn_inflate_create(g_gpu_inflate_device, &gpu_) != CHN_OK)
                throw std::runtime_error(std::string("CHARON_GPU_INFLATE: ") + chn_last_error());
            const size_t n = ms.size();
            std::vector<uint64_t> in_off(n), out_off(n);
            std::vector<uint32_t> in_len(n), out_len(n), status(n, 0), expected(n);
            for (size_t i = 0; i < n; ++i) {
                in_off[i] = (uint64_t)(ms[i].cdata - z_); in_len[i] = ms[i].clen;
                out_off[i] = ms[i].out; out_len[i] = ms[i].isize;
                expected[i] = ms[i].crc;
            }
            chn_inflate_job job;
            std::memset(&job, 0, sizeof job);
            job.struct_size = sizeof job; job.n_members = n;
            job.in = z_; job.in_bytes = size_; job.in_offset = in_off.data(); job.in_length = in_len.data();
            job.out = reinterpret_cast<uint8_t *>(dst); job.out_bytes = total; job.out_offset = out_off.data(); job.out_length = out_len.data();
            job.status = status.data();
            chn_inflate_crc crc;
            std::memset(&crc, 0, sizeof crc);
            crc.struct_size = sizeof crc; crc.expected = expected.data();
            const double t0 = omp_get_wtime();
            if (chn_inflate_run_crc(gpu_, &job, &crc) != CHN_OK) throw std::runtime_error(std::string("CHARON_GPU_INFLATE: ") + chn_last_error());
            g_gpu_inflate_s += omp_get_wtime() - t0;
            for (size_t i = 0; i < n; ++i) bad = bad || status[i] != 0;  // a decode failure, a wrong size, or CHN_INFLATE_E_CRC
        } else {
#pragma omp parallel num_threads(nt)
        {
            z_stream zs;
            std::memset(&zs, 0, sizeof zs);
            bool ready = inflateInit2(&zs, -15) == Z_OK, mine_bad = !ready;
#pragma omp for schedule(dynamic, 16)
            for (long i = 0; i < (long)ms.size(); ++i) {
                if (mine_bad) continue;
                const Member &mb = ms[(size_t)i];
                if (inflateReset(&zs) != Z_OK) { mine_bad = true; continue; }
                unsigned char sink = 0;
                zs.next_in = const_cast<unsigned char *>(mb.cdata); zs.avail_in = mb.clen;
                zs.next_out = mb.isize ? reinterpret_cast<unsigned char *>(dst + mb.out) : &sink; zs.avail_out = mb.isize ? mb.isize : 1;
                const int rc = inflate(&zs, Z_FINISH);
                if (rc != Z_STREAM_END || zs.total_out != mb.isize ||
                    fast_crc32((uint32_t)crc32(0L, Z_NULL, 0), reinterpret_cast<const unsigned char *>(dst + mb.out), mb.isize) != mb.crc)
                    mine_bad = true;
            }
            if (ready) inflateEnd(&zs);
            if (mine_bad) {
#pragma omp critical(bgzf_bad)
                bad = true;
            }
        }
        }
        if (bad) throw std::runtime_error("gzip read error in " + path_ + ": a BGZF member is corrupt (inflate, size or CRC32 mismatch)");
    }
};

uint64_t g_split_pieces = 0, g_split_records = 0;  // pieces / records taken by the several-thread FASTQ splitter (diagnostic)
double g_reader_fill_s = 0, g_reader_parse_s = 0;  // reader-thread seconds in inflate / in record splitting (CHARON_TIMING)
class BlockReader {
    std::unique_ptr<BgzfSource> bgzf_;
    std::unique_ptr<Bz2Source> bz_;     // .bz2: blocks decoded side by side (bz2_stream.inc)
    std::unique_ptr<FastInflate> gz_;   // one-stream .gz: this build's decoder (inflate_stream.inc); zlib's gzread otherwise
    gzFile f_ = nullptr;
    bool fastq_ = false, eof_ = false;
    Slab carry_;
    double rec_bytes_ = 0;  // bytes of text per record in the last block (sizes the next decode)
    uint64_t device_offset_ = 0;  // inflated bytes handed out by next_device so far
    std::string path_;
    // Uncompressed files are mapped (MAP_PRIVATE, so that the in-place compaction of multi-line records stays possible): records
    // become views straight into the page cache -- no read() copies, no slab to zero-fill -- and the reader thread only has to find
    // line ends.  (.gz input still goes through zlib: one inflate stream, ~0.4 GB/s.)
    char *map_ = nullptr;
    size_t map_size_ = 0, map_pos_ = 0;
    std::shared_ptr<MapToken> map_token_;

    static const char *find_eol(const char *p, const char *end) { return static_cast<const char *>(std::memchr(p, '\n', (size_t)(end - p))); }

    // Parse one record starting at p (non-destructively first).  Returns the position after the record, or nullptr if the
    // data in [p, end) does not hold the whole record yet.
    char *parse_fastq(char *p, char *end, RecView &r) {
        while (p < end && (*p == '\n' || *p == '\r')) ++p;  // blank lines between records
        if (p >= end) return nullptr;
        if (*p != '@') throw std::runtime_error("FASTQ parse error in " + path_ + ": record does not start with '@'");
        const char *e0 = find_eol(p, end);
        if (!e0) return nullptr;
        // pass 1: locate the line structure
        struct Span { char *b; uint32_t n; };
        Span seq_first{nullptr, 0}; bool multi = false;
        uint64_t seq_len = 0;
        char *q = const_cast<char *>(e0) + 1, *plus = nullptr;
        for (;;) {
            if (q >= end) { if (!eof_) return nullptr; throw std::runtime_error("FASTQ parse error in " + path_ + ": unexpected end of file"); }
            const char *e = find_eol(q, end);
            if (!e) { if (!eof_) return nullptr; e = end; }
            uint32_t n = (uint32_t)(e - q);
            if (n && q[n - 1] == '\r') --n;
            if (n && q[0] == '+') { plus = q; q = (e < end) ? const_cast<char *>(e) + 1 : end; break; }
            if (!seq_first.b) seq_first = Span{q, n}; else if (n) multi = true;
            seq_len += n;
            q = (e < end) ? const_cast<char *>(e) + 1 : end;
        }
        (void)plus;
        char *qual_begin = q;
        uint64_t qual_len = 0; bool qmulti = false; bool first_q = true;
        while (qual_len < seq_len) {
            if (q >= end) { if (!eof_) return nullptr; throw std::runtime_error("FASTQ parse error in " + path_ + ": qualities shorter than sequence"); }
            const char *e = find_eol(q, end);
            if (!e) { if (!eof_) return nullptr; e = end; }
            uint32_t n = (uint32_t)(e - q);
            if (n && q[n - 1] == '\r') --n;
            if (!first_q && n) qmulti = true;
            first_q = false;
            qual_len += n;
            q = (e < end) ? const_cast<char *>(e) + 1 : end;
        }
        if (seq_len == 0 && q < end && *q != '@') {  // zero-length read: its (empty) quality line
            const char *e = find_eol(q, end);
            if (e && (e == q || (e == q + 1 && *q == '\r'))) q = const_cast<char *>(e) + 1;
        }
        // pass 2: views (compacting multi-line records in place)
        uint32_t idn = (uint32_t)(e0 - p - 1);
        if (idn && p[idn] == '\r') --idn;
        r.id = p + 1; r.id_len = idn;
        auto compact = [&](char *from, uint64_t want, bool is_multi) -> const char * {
            if (!is_multi) return from;
            char *dst = from, *src = from;
            uint64_t got = 0;
            while (got < want) {
                const char *e = find_eol(src, end);
                if (!e) e = end;
                uint32_t n = (uint32_t)(e - src);
                if (n && src[n - 1] == '\r') --n;
                if (dst != src) std::memmove(dst, src, n);
                dst += n; got += n;
                src = (e < end) ? const_cast<char *>(e) + 1 : end;
            }
            return from;
        };
        r.seq = seq_first.b ? compact(seq_first.b, seq_len, multi) : p; r.seq_len = (uint32_t)seq_len;
        r.qual = compact(qual_begin, qual_len, qmulti); r.qual_len = (uint32_t)qual_len;
        if (seq_len > 0xFFFFFFFFull) throw std::runtime_error("read longer than 2^32 bases");
        return q;
    }
    char *parse_fasta(char *p, char *end, RecView &r) {
        while (p < end && (*p == '\n' || *p == '\r')) ++p;
        if (p >= end) return nullptr;
        if (*p != '>' && *p != ';') throw std::runtime_error("FASTA parse error in " + path_ + ": record does not start with '>'");
        const char *e0 = find_eol(p, end);
        if (!e0) { if (!eof_) return nullptr; e0 = end; }
        // the record ends at the next line that starts with '>' / ';', or at end of file
        char *q = (e0 < end) ? const_cast<char *>(e0) + 1 : end;
        char *rec_end = nullptr;
        for (char *l = q;;) {
            if (l >= end) { if (!eof_) return nullptr; rec_end = end; break; }
            if (*l == '>' || *l == ';') { rec_end = l; break; }
            const char *e = find_eol(l, end);
            if (!e) { if (!eof_) return nullptr; rec_end = end; break; }
            l = const_cast<char *>(e) + 1;
        }
        uint32_t idn = (uint32_t)(e0 - p - 1);
        if (idn && p[idn] == '\r') --idn;
        r.id = p + 1; r.id_len = idn;
        // seqan3 skips blanks and digits inside FASTA sequence lines.  Line by line: a line of nothing but letters (every byte >= 0x40; the
        // characters to skip are all below) moves as one piece -- 2.2 x the byte loop on a chromosome in 60-letter lines --, any other line
        // goes byte by byte
        char *dst = q;
        for (char *c = q; c < rec_end;) {
            char *e = static_cast<char *>(std::memchr(c, '\n', (size_t)(rec_end - c)));
            if (!e) e = rec_end;
            const size_t len = (size_t)(e - c);
            bool clean = true;
            size_t i = 0;
            for (; i + 8 <= len; i += 8) {  // eight bytes at a time: bit 7 or bit 6 set in every one of them
                uint64_t x;
                std::memcpy(&x, c + i, 8);
                if (((x | (x << 1)) & 0x8080808080808080ULL) != 0x8080808080808080ULL) { clean = false; break; }
            }
            if (clean) for (; i < len; ++i) if ((unsigned char)c[i] < 0x40) { clean = false; break; }
            if (clean) {
                if (dst != c) std::memmove(dst, c, len);  // (a mapped file's pages are only copied where something actually moves)
                dst += len;
            } else {
                for (char *p2 = c; p2 < e; ++p2) {
                    const char ch = *p2;
                    if (ch == '\r' || ch == ' ' || ch == '\t' || (ch >= '0' && ch <= '9')) continue;
                    if (dst != p2) *dst = ch;
                    ++dst;
                }
            }
            c = e < rec_end ? e + 1 : rec_end;
        }
        r.seq = q; r.seq_len = (uint32_t)(dst - q); r.qual = nullptr; r.qual_len = 0;
        return rec_end;
    }

    // ---- several threads on one mapped FASTQ file ------------------------------------------------------------------------
    // The stretch of a block is cut into as many pieces as there are reader threads; every piece but the first starts at a GUESSED
    // record start (a line beginning with '@' from which two plain four-line records parse).  All pieces are parsed at once; a piece
    // counts if the piece in front of it came to stand exactly on its start -- the first piece starts at a known record boundary, so
    // by induction every counted record is one the sequential parser would have produced.  Only plain four-line records are taken
    // here (nothing is compacted in place, nothing throws): anything else -- wrapped lines, an empty read, a damaged record -- ends the
    // piece, and the sequential parser takes over from there with its own error handling.
    bool no_split_ = false;
    enum DryStatus { DRY_OK, DRY_END, DRY_OTHER };
    static DryStatus dry_record(char *p, char *end, RecView &r, char *&next) {
        if (p >= end) return DRY_END;
        if (*p != '@') return DRY_OTHER;
        const char *e0 = find_eol(p, end);
        if (!e0) return DRY_OTHER;
        char *q1 = const_cast<char *>(e0) + 1;
        const char *e1 = q1 < end ? find_eol(q1, end) : nullptr;
        if (!e1) return DRY_OTHER;
        uint32_t n1 = (uint32_t)(e1 - q1);
        if (n1 && q1[n1 - 1] == '\r') --n1;
        if (n1 == 0 || q1[0] == '+' || (uint64_t)(e1 - q1) > 0xFFFFFFF0ull) return DRY_OTHER;
        char *q2 = const_cast<char *>(e1) + 1;
        if (q2 >= end || *q2 != '+') return DRY_OTHER;
        const char *e2 = find_eol(q2, end);
        if (!e2) return DRY_OTHER;
        char *q3 = const_cast<char *>(e2) + 1;
        if (q3 >= end) return DRY_OTHER;
        const char *e3 = find_eol(q3, end);
        if (!e3) return DRY_OTHER;  // (the last line of a file without a final newline is left to the sequential parser)
        uint32_t n3 = (uint32_t)(e3 - q3);
        if (n3 && q3[n3 - 1] == '\r') --n3;
        if (n3 != n1) return DRY_OTHER;
        uint32_t idn = (uint32_t)(e0 - p - 1);
        if (idn && p[idn] == '\r') --idn;
        r.id = p + 1; r.id_len = idn; r.seq = q1; r.seq_len = n1; r.qual = q3; r.qual_len = n3;
        next = const_cast<char *>(e3) + 1;
        return DRY_OK;
    }
    // Fills blk.recs with the records of [base, ...) that could be taken this way and returns where the sequential parser goes on.
    char *split_in_parallel(RawBlock &blk, char *base, char *end, size_t max_recs, size_t max_bytes) {
        const size_t span = std::min<size_t>(max_bytes, (size_t)(end - base));
        const int T = (int)std::min<size_t>((size_t)g_reader_threads, span >> 20);
        if (T < 2 || max_recs < 4096) return base;
        struct Piece { char *start = nullptr, *stop = nullptr, *landed = nullptr; std::vector<RecView> recs; std::vector<char *> ends; bool other = false; };
        std::vector<Piece> pc((size_t)T);
        pc[0].start = base;
#pragma omp parallel for num_threads(T) schedule(static, 1)
        for (int i = 1; i < T; ++i) {  // guessed starts
            char *g = base + span / (size_t)T * (size_t)i, *lim = std::min(end, g + ((size_t)1 << 20));
            for (char *c = g; c < lim;) {
                const char *nl = find_eol(c, lim);
                if (!nl) break;
                char *cand = const_cast<char *>(nl) + 1, *n1 = nullptr, *n2 = nullptr;
                RecView r;
                if (cand < end && *cand == '@' && dry_record(cand, end, r, n1) == DRY_OK && dry_record(n1, end, r, n2) == DRY_OK) { pc[(size_t)i].start = cand; break; }
                c = cand;
            }
        }
        std::vector<int> order;
        for (int i = 0; i < T; ++i) if (pc[(size_t)i].start) order.push_back(i);
        if (order.size() < 2) return base;
        for (size_t k = 0; k < order.size(); ++k) pc[(size_t)order[k]].stop = k + 1 < order.size() ? pc[(size_t)order[k + 1]].start : base + span;
#pragma omp parallel for num_threads((int)order.size()) schedule(static, 1)
        for (int k = 0; k < (int)order.size(); ++k) {
            Piece &x = pc[(size_t)order[(size_t)k]];
            char *p = x.start;
            x.recs.reserve((size_t)(x.stop - x.start) / 256 + 16);
            while (p < x.stop) {
                RecView r;
                char *nx = nullptr;
                const DryStatus st = dry_record(p, end, r, nx);
                if (st != DRY_OK) { x.other = st == DRY_OTHER; break; }
                x.recs.push_back(r); x.ends.push_back(nx);
                p = nx;
            }
            x.landed = p;
        }
        // in order: a piece counts if its predecessor stands exactly on its start
        char *at = base;
        for (size_t k = 0; k < order.size(); ++k) {
            Piece &x = pc[(size_t)order[k]];
            if (x.start != at) break;
            size_t take = x.recs.size();
            if (blk.recs.size() >= max_recs) break;
            if (blk.recs.size() + take > max_recs) take = max_recs - blk.recs.size();
            blk.recs.insert(blk.recs.end(), x.recs.begin(), x.recs.begin() + (long)take);
            g_split_pieces += 1; g_split_records += take;
            if (take < x.recs.size()) { at = x.ends[take - 1]; break; }
            at = x.landed;
            if (x.other) { if (x.recs.empty() && k == 0) no_split_ = true; break; }  // a record of another shape: sequentially from here
            if (take == 0 && x.recs.empty()) break;
        }
        return at;
    }

public:
    explicit BlockReader(const std::string &path) : path_(path) {
        std::string p = path;
        const bool is_bz2 = ends_with(p, ".bz2");
        if (is_bz2) p.resize(p.size() - 4);
        else if (ends_with(p, ".gz")) p.resize(p.size() - 3);
        fastq_ = ends_with(p, ".fastq") || ends_with(p, ".fq");
        if (!fastq_ && !(ends_with(p, ".fasta") || ends_with(p, ".fa") || ends_with(p, ".fna") || ends_with(p, ".ffn") ||
                         ends_with(p, ".faa") || ends_with(p, ".frn") || ends_with(p, ".fas")))
            throw std::runtime_error("unknown sequence file extension: " + path);
        if (is_bz2) {  // this build's block-parallel decoder (bz2_stream.inc); throws on anything that is not a bzip2 stream
            bz_.reset(new Bz2Source());
            bz_->open(path);
            return;
        }
        if (!ends_with(path, ".gz") && !std::getenv("CHARON_NO_MMAP")) {
            const int fd = ::open(path.c_str(), O_RDONLY);
            struct stat st;
            if (fd >= 0 && ::fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
                if (st.st_size == 0) { ::close(fd); eof_ = true; map_ = const_cast<char *>(""); return; }
                void *m = ::mmap(nullptr, (size_t)st.st_size, PROT_READ | PROT_WRITE, MAP_PRIVATE, fd, 0);
                if (m != MAP_FAILED) {
                    ::close(fd);
                    map_ = static_cast<char *>(m); map_size_ = (size_t)st.st_size; eof_ = true;  // the parsers see the whole file
                    map_token_ = std::make_shared<MapToken>();
                    (void)::madvise(m, map_size_, MADV_SEQUENTIAL);
                    return;
                }
            }
            if (fd >= 0) ::close(fd);
        }
        if (ends_with(path, ".gz") && !std::getenv("CHARON_NO_BGZF")) {
            std::unique_ptr<BgzfSource> b(new BgzfSource());
            if (b->open(path)) { bgzf_ = std::move(b); return; }
        }
        if (ends_with(path, ".gz") && !std::getenv("CHARON_ZLIB_INFLATE")) {
            std::unique_ptr<FastInflate> g(new FastInflate(path));
            if (g->open()) { gz_ = std::move(g); return; }
        }
        f_ = gzopen(path.c_str(), "rb");
        if (!f_) throw std::runtime_error("cannot open " + path);
        gzbuffer(f_, 1 << 20);
    }
    ~BlockReader() {
        if (f_) gzclose(f_);
        if (map_token_) map_token_->alive.store(false);  // ranges still on their way back must not touch whatever is mapped here next
        if (map_ && map_size_) ::munmap(map_, map_size_);
    }
    BlockReader(const BlockReader &) = delete;
    BlockReader &operator=(const BlockReader &) = delete;

    // CHARON_GPU_INFLATE_STREAM=1 applies to a one-stream .gz that this build's decoder reads in parallel rounds; empty if it does,
    // else why it does not
    std::string gpu_inflate_stream_note() const {
        if (bgzf_) return "the input is BGZF (its members are inflated on the device under CHARON_GPU_INFLATE=1)";
        if (bz_) return "the input is bzip2";
        if (gz_) return std::getenv("CHARON_SERIAL_INFLATE") ? "CHARON_SERIAL_INFLATE is set (one sequential inflate, no chunks)" : "";
        if (ends_with(path_, ".gz")) return std::getenv("CHARON_ZLIB_INFLATE") ? "CHARON_ZLIB_INFLATE is set (zlib reads the file)" : "zlib reads the file (it is not a mappable gzip file)";
        return "the input is not compressed";
    }
    // CHARON_GPU_TEXT=1 applies to BGZF input in FASTQ form only
    bool is_bgzf_fastq() const { return bgzf_ && fastq_; }
    // the next block of the file as text in device memory (null at the end of the file)
    std::shared_ptr<DevBlock> next_device(size_t max_bytes, size_t headroom) {
        const double t0 = omp_get_wtime();
        std::shared_ptr<DevBlock> b = bgzf_->fill_device(max_bytes, headroom, device_offset_);
        { std::lock_guard<std::mutex> lk(g_reader_stat_m); g_reader_fill_s += omp_get_wtime() - t0; }
        if (b) device_offset_ += b->text_bytes - b->member0;
        return b;
    }
    // go on as next() does from a member boundary of the compressed file, with `carry` (text in front of that member) still to parse
    void resume(size_t z_pos, Slab &carry) {
        bgzf_->seek(z_pos);
        carry_.swap(carry);
        eof_ = false;
    }

    // Fill `blk` with up to max_recs whole records (reading about max_bytes of new data at a time).  Returns false when
    // the file is exhausted and nothing was produced.
    bool next(RawBlock &blk, size_t max_recs, size_t max_bytes) {
        blk.recs.clear();
        if (map_) {  // mapped file: parse in place, at most max_recs records / about max_bytes of text
            blk.buf.clear();
            g_dead_ranges.release_for(map_token_);
            char *base = map_ + map_pos_, *end = map_ + map_size_, *p = base;
            if (fastq_ && !no_split_ && g_reader_threads > 1) p = split_in_parallel(blk, base, end, max_recs, max_bytes);
            while (blk.recs.size() < max_recs && (size_t)(p - base) < max_bytes) {
                RecView r;
                char *nx = fastq_ ? parse_fastq(p, end, r) : parse_fasta(p, end, r);
                if (!nx) break;
                blk.recs.push_back(r);
                p = nx;
            }
            map_pos_ = (size_t)(p - map_);
            blk.map_begin = base; blk.map_len = (size_t)(p - base); blk.map_token = map_token_;
            if (!blk.recs.empty()) return true;
            for (char *c = p; c < end; ++c)
                if (*c != '\n' && *c != '\r') throw std::runtime_error("parse error in " + path_ + ": trailing data is not a whole record");
            return false;
        }
        // The new slab starts with what the last block left over (carry_: already a slab of its own, so the tail is copied once).
        if (carry_.empty()) { Slab fresh = g_slab_pool.take(); fresh.clear(); blk.buf.swap(fresh); }
        else { blk.buf.swap(carry_); Slab none; carry_.swap(none); }
        // How much to decode: what max_recs records take, judged by the last block's records (+ 1/8), and never more than max_bytes beyond
        // what is already there.  Decoding max_bytes on every call whatever the carry holds made the carry grow by (max_bytes - consumed)
        // per call: the whole inflated file in memory and copied again and again with short reads (ADVICE r2).
        size_t parsed_to = 0;
        for (bool first = true;; first = false) {
            // (re)parsing only ever starts from scratch while no record has been produced, because producing a record may
            // compact it in place
            size_t want = max_bytes;
            if (first) {
                const size_t target = rec_bytes_ ? std::min<size_t>(max_bytes, (size_t)(rec_bytes_ * (double)max_recs * 1.125) + (64u << 10)) : std::min<size_t>(max_bytes, (size_t)32 << 20);
                want = blk.buf.size() < target ? target - blk.buf.size() : 0;
            }
            const double t_fill0 = omp_get_wtime();
            if (want == 0 || eof_) {
            } else if (bgzf_) {
                bgzf_->fill(blk.buf, want);
                eof_ = bgzf_->at_end();
            } else if (gz_) {
                gz_->fill(blk.buf, want);
                eof_ = gz_->at_end();
            } else if (bz_) {
                bz_->fill(blk.buf, want);
                eof_ = bz_->at_end();
            } else {
                const size_t old = blk.buf.size();
                blk.buf.resize(old + want);
                size_t got = 0;
                while (got < want) {
                    const int n = gzread(f_, blk.buf.data() + old + got, (unsigned)std::min<size_t>(want - got, 1u << 30));
                    if (n <= 0) {
                        // end of data -- or a truncated / corrupt stream, which must not pass for a short file (the reference's
                        // seqan3 / zlib stream throws there)
                        int errnum = Z_OK;
                        const char *msg = gzerror(f_, &errnum);
                        if (n < 0 || (errnum != Z_OK && errnum != Z_STREAM_END) || !gzeof(f_))
                            throw std::runtime_error("gzip read error in " + path_ + ": " + (msg && *msg ? msg : "unexpected end of the compressed stream"));
                        eof_ = true;
                        break;
                    }
                    got += (size_t)n;
                }
                blk.buf.resize(old + got);
            }
            const double t_parse0 = omp_get_wtime();
            g_reader_fill_s += t_parse0 - t_fill0;
            char *base = blk.buf.data(), *end = base + blk.buf.size(), *p = base;
            while (blk.recs.size() < max_recs) {
                RecView r;
                char *nx = fastq_ ? parse_fastq(p, end, r) : parse_fasta(p, end, r);
                if (!nx) break;
                blk.recs.push_back(r);
                p = nx;
            }
            parsed_to = (size_t)(p - base);
            g_reader_parse_s += omp_get_wtime() - t_parse0;
            if (!blk.recs.empty() || eof_) break;
            // not even one whole record yet: read more and parse again
        }
        if (!blk.recs.empty()) rec_bytes_ = (double)parsed_to / (double)blk.recs.size();
        // whatever was not consumed goes to the next block
        if (parsed_to < blk.buf.size()) {
            bool only_ws = true;
            for (size_t i = parsed_to; i < blk.buf.size() && only_ws; ++i) only_ws = (blk.buf[i] == '\n' || blk.buf[i] == '\r');
            if (!only_ws) {
                carry_ = g_slab_pool.take();
                carry_.assign(blk.buf.begin() + (long)parsed_to, blk.buf.end());
            }
        }
        if (blk.recs.empty() && eof_ && carry_.empty()) return false;
        if (blk.recs.empty() && eof_) throw std::runtime_error("parse error in " + path_ + ": trailing data is not a whole record");
        return true;
    }
};

inline int dna_code(char c) {  // 0..3 = ACGT, 4 = N (seqan3 dna5: every other IUPAC letter folds to N)
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': case 'U': case 'u': return 3;
        default: return 4;
    }
}
struct CodeTable {  // 0..3 ACGT, 4 N (other IUPAC letters), 255 illegal
    uint8_t t[256];
    CodeTable() {
        std::memset(t, 255, sizeof t);
        for (const char *c = "NRYSWKMBDHVnryswkmbdhv"; *c; ++c) t[(unsigned char)*c] = 4;
        for (const char *c = "ACGTUacgtu"; *c; ++c) t[(unsigned char)*c] = (uint8_t)dna_code(*c);
    }
};
const CodeTable g_codes;

// get_compression_ratio (src/utils.cpp:114-124) of sequence_to_string(seq) (upper-case dna5 letters, :105-112).
// One z_stream per thread, deflateReset between reads (same output as a fresh deflateInit2, without its allocations).
struct Deflater {
    z_stream zs;
    bool init = false;
    std::vector<unsigned char> out;
    std::string up;
    gzsize::GzipSizer sizer;
    ~Deflater() { if (init) deflateEnd(&zs); }
    // the linked zlib itself: gzip::compress(up).size()
    size_t zlib_size(size_t n) {
        if (!init) {
            std::memset(&zs, 0, sizeof zs);
            if (deflateInit2(&zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw std::runtime_error("deflateInit2 failed");
            init = true;
        } else {
            deflateReset(&zs);
        }
        const size_t bound = deflateBound(&zs, (uLong)n) + 64;
        if (out.size() < bound) out.resize(bound);
        zs.next_in = (Bytef *)up.data(); zs.avail_in = (uInt)n;
        zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
        deflate(&zs, Z_FINISH);
        return out.size() - zs.avail_out;
    }
    // size of the gzip member of up[0..n): the bit-exact size emulator (host/gzip_size.hpp) when it is enabled and the input is in
    // its scope, the linked zlib otherwise.  `up` carries GzipSizer::PAD zero bytes behind the data.
    size_t gzip_size(size_t n) {
        if (g_gzip_emulator) {
            const uint32_t s = sizer.size_padded(reinterpret_cast<const uint8_t *>(up.data()), n);
            if (s) return s;
        }
        return zlib_size(n);
    }
    void load(const RecView &a, const RecView *b) {
        const size_t n = (size_t)a.seq_len + (b ? b->seq_len : 0);
        up.clear();
        up.reserve(n + gzsize::GzipSizer::PAD);
        for (uint32_t i = 0; i < a.seq_len; ++i) up.push_back("ACGTNNNN"[g_codes.t[(unsigned char)a.seq[i]] & 7]);
        if (b) for (uint32_t i = 0; i < b->seq_len; ++i) up.push_back("ACGTNNNN"[g_codes.t[(unsigned char)b->seq[i]] & 7]);
        up.append(gzsize::GzipSizer::PAD, '\0');
    }
    float ratio(const RecView &a, const RecView *b) {
        load(a, b);
        const size_t n = up.size() - gzsize::GzipSizer::PAD;
        return static_cast<float>(static_cast<double>(gzip_size(n)) / static_cast<double>(n));
    }
};

// Start-up cross-check of the size emulator against the zlib this binary is linked with (a different zlib build could take
// different decisions): a handful of deterministic sequences; on any disagreement the emulator is switched off for the run.
bool gzip_emulator_self_check() {
    Deflater d;
    uint64_t x = 0x9E3779B97F4A7C15ULL;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    const size_t lens[] = {1, 2, 3, 7, 40, 150, 301, 1000, 5000, 20000, 59999, 70001};  // the last one slides zlib's window
    for (size_t L : lens)
        for (int kind = 0; kind < 3; ++kind) {
            d.up.clear();
            for (size_t i = 0; i < L; ++i)
                d.up.push_back(kind == 0 ? "ACGT"[next() & 3] : kind == 1 ? "ACGTN"[next() % 5] : "ACGT"[(i / 5 + (next() % 31 == 0)) & 3]);
            d.up.append(gzsize::GzipSizer::PAD, '\0');
            const uint32_t e = d.sizer.size_padded(reinterpret_cast<const uint8_t *>(d.up.data()), L);
            if (e == 0 || e != d.zlib_size(L)) return false;
        }
    return true;
}

