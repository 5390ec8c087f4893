// host_batch.inc -- host batches (2-bit packing, quality, gzip column) and the reader queue that hands them to dehost_main
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a
// stand-alone header.

// ---------------------------------------------------------------------------------------------------
// batching: pack reads into the 2-bit layout of include/charon_hip.h
// ---------------------------------------------------------------------------------------------------
#if defined(__x86_64__)
const bool g_has_avx2 = __builtin_cpu_supports("avx2");
#endif
// Array of 32-bit words, zero-filled (assign_zero) or left for the caller to write (assign_raw); page-locked on request (chn_host_alloc), so that chn_batch_submit's upload of it is an asynchronous
// DMA instead of a staged copy on the caller's thread.  Grows, never shrinks (batches go round).
struct WordBuf {
    uint32_t *p = nullptr;
    size_t n = 0, cap = 0;
    bool pinned = false, want_pinned = false;
    WordBuf() = default;
    WordBuf(const WordBuf &) = delete;
    WordBuf &operator=(const WordBuf &) = delete;
    ~WordBuf() { release(); }
    void release() {
        if (p) { if (pinned) (void)chn_host_free(p); else std::free(p); }
        p = nullptr; n = cap = 0;
    }
    // room for `count` words, contents undefined (the packing loop writes every word of a read's span itself, thread by thread: clearing
    // 50 MB per batch on the main thread first was 0.75 s of a 1.2 s packing phase on 4 M reads)
    void assign_raw(size_t count) { grow(count); }
    void assign_zero(size_t count) { grow(count); std::memset(p, 0, count * 4); }
    uint32_t *data() { return p; }
    const uint32_t *data() const { return p; }
private:
    void grow(size_t count) {
        if (count > cap) {
            release();
            const size_t c = count + count / 8 + 16;
            void *q = nullptr;
            if (want_pinned && chn_host_alloc(c * 4, &q) == CHN_OK && q) pinned = true;
            else { q = std::malloc(c * 4); pinned = false; if (!q) throw std::bad_alloc(); }
            p = static_cast<uint32_t *>(q); cap = c;
        }
        n = count;
    }
};

// The default routing of reads beyond CHN_GZIP_MAX_LEN letters (CHN_GZIP_SIZES_ALL): the device sizes every read of the batch of at
// most the returned length (0: none of them).  One wavefront walks one such read, at about DEV_NS per letter (a lone wavefront's
// deflate_slow: 0.1-0.2 ms per kb, profiles/r03/sq_gzip_tally.txt), and the device holds WAVES of them at once; the host emulator
// takes HOST_NS per letter on one thread (about 70 us per 5 kb, DESIGN 6b).  A long read only pays on the device when its walk hides
// under what the batch costs anyway: the batch's other device work (BATCH_NS per letter of the batch) or the host time of the long
// reads the device takes off `threads` threads.  So a batch of short reads never waits for one lone 2 Mb read (0.3 s on the device,
// 28 ms on one host thread), while a batch with many ultra-long reads sends them to the device at -t 1.  Applied only where every read
// up to CHN_GZIP_MAX_LEN is sized on the device already (fewer than 12 threads): the routing never moves a read below that length.
static uint32_t gzip_long_device_limit(std::vector<uint32_t> long_lens, uint64_t batch_letters, int threads) {
    const double DEV_NS = 150.0, HOST_NS = 14.0, BATCH_NS = 0.1, WAVES = 512.0;
    std::sort(long_lens.begin(), long_lens.end());
    double rest = 0;  // letters of the reads at most long_lens[i]
    std::vector<double> upto(long_lens.size());
    for (size_t i = 0; i < long_lens.size(); ++i) upto[i] = rest += long_lens[i];
    for (size_t i = long_lens.size(); i-- > 0;) {  // the longest limit that pays
        const double dev = DEV_NS * std::max<double>(long_lens[i], upto[i] / WAVES);
        const double hidden = std::max(BATCH_NS * (double)batch_letters, HOST_NS * upto[i] / std::max(1, threads));
        if (dev <= hidden) return long_lens[i];
    }
    return 0;
}

struct HostBatch {
    RawBlock blk1, blk2;               // records of this batch (views into the blocks' slabs)
    std::vector<Slab> extra;  // further slabs of mate records when one block did not hold enough of them
    std::vector<uint32_t> keep;        // indices of the records that are classified (zero-length reads are skipped)
    WordBuf bases, nmask;              // 2-bit codes, N mask
    std::vector<uint32_t> len1, len2;
    std::vector<uint64_t> off1, off2;
    std::vector<float> mq, comp;
    bool any_n = false;
    uint64_t n_bases = 0;
    // CHARON_TEXT_BATCHES=1: the batch as chn_text_batch describes it -- `text` is the stretch of the block's slab that holds the kept
    // records (single-end input that was decoded into a slab: nothing is copied) or `tcopy`, a page-locked copy of the letters and
    // qualities alone (mapped files, whose pages cannot be page-locked, and pairs, whose mates live in two slabs)
    const uint8_t *text = nullptr;
    uint64_t text_bytes = 0;
    std::vector<uint64_t> so1, qo1, so2, qo2;
    std::vector<uint32_t> ql1, ql2;
    std::vector<uint64_t> io1, io2;    // CHARON_GPU_EXTRACT=1: where the ids lie in dtext / dtext2, and their lengths (mate 2's ids do not come down)
    std::vector<uint32_t> il1, il2;
    bool text_quals = false, text_from_slab = false;
    WordBuf tcopy;
    // CHARON_GPU_TEXT=1: the block's text in device memory (so1 / qo1 are offsets into it; the records' seq / qual pointers stay null
    // until chn_text_fetch has brought a read's letters into `arena`) and the id bytes chn_text_split handed back (the records' ids)
    std::shared_ptr<DevBlock> dtext;
    std::shared_ptr<DevBlock> dtext2;  // CHARON_GPU_TEXT_PAIRS=1: the block of file 2 that holds the mates (so2 / qo2 are offsets into it)
    std::unique_ptr<char[]> ids;
    WordBuf arena;
    ~HostBatch() {
        g_dead_ranges.add(blk1.map_token, blk1.map_begin, blk1.map_len); g_dead_ranges.add(blk2.map_token, blk2.map_begin, blk2.map_len);
        g_slab_pool.give(blk1.buf); g_slab_pool.give(blk2.buf);
        for (auto &e : extra) g_slab_pool.give(e);
    }

    static uint64_t pad64(uint64_t x) { return (x + 63) & ~63ULL; }
    // returns false on an illegal character
    bool put(const RecView &r, uint64_t off, bool &saw_n) {
        uint32_t *bw = bases.data() + (off >> 4);
        uint32_t *nw = nmask.data() + (off >> 5);
        // the segment's span (a multiple of 64 letters) is this call's to initialise: the N mask is OR-ed into, the code words behind the
        // last letter are never written below
        std::memset(nw, 0, (size_t)(pad64(r.seq_len) >> 5) * 4);
        for (uint64_t wdx = ((uint64_t)r.seq_len + 15) >> 4; wdx < (pad64(r.seq_len) >> 4); ++wdx) bw[wdx] = 0;
        const unsigned char *sq = reinterpret_cast<const unsigned char *>(r.seq);
        bool ok = true;
        uint32_t i = 0;
#if defined(__x86_64__)
        if (g_has_avx2) i = put_avx2(sq, r.seq_len, bw, nw, ok, saw_n);
#endif
        for (; i < r.seq_len; i += 16) {
            uint32_t w = 0, nb = 0;
            const uint32_t m = std::min<uint32_t>(16, r.seq_len - i);
            for (uint32_t j = 0; j < m; ++j) {
                const uint8_t c = g_codes.t[sq[i + j]];
                if (c < 4) w |= (uint32_t)c << (2 * j);
                else if (c == 4) nb |= 1u << j;
                else ok = false;
            }
            bw[i >> 4] = w;
            if (nb) { nw[i >> 5] |= nb << (i & 16); saw_n = true; }
        }
        return ok;
    }
#if defined(__x86_64__)
    // 32 letters per step: A/C/G/T in either case pack by arithmetic ((c >> 1) & 3 gives A0 C1 T2 G3; x ^ (x >> 1) swaps the last
    // two); a chunk holding anything else goes through the table.  Returns the number of letters done (a multiple of 32).
    __attribute__((target("avx2"))) static uint32_t put_avx2(const unsigned char *sq, uint32_t len, uint32_t *bw, uint32_t *nw, bool &ok, bool &saw_n) {
        const __m256i upper = _mm256_set1_epi8((char)0xDF), three = _mm256_set1_epi8(3), one = _mm256_set1_epi8(1);
        const __m256i lA = _mm256_set1_epi8('A'), lC = _mm256_set1_epi8('C'), lG = _mm256_set1_epi8('G'), lT = _mm256_set1_epi8('T');
        const __m256i w16 = _mm256_set1_epi16(0x0401), w32 = _mm256_set1_epi32(0x00100001);
        const __m256i pick = _mm256_setr_epi8(0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1);
        uint32_t i = 0;
        for (; i + 32 <= len; i += 32) {
            const __m256i c = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(sq + i));
            const __m256i u = _mm256_and_si256(c, upper);
            const __m256i valid = _mm256_or_si256(_mm256_or_si256(_mm256_cmpeq_epi8(u, lA), _mm256_cmpeq_epi8(u, lC)),
                                                  _mm256_or_si256(_mm256_cmpeq_epi8(u, lG), _mm256_cmpeq_epi8(u, lT)));
            if (_mm256_movemask_epi8(valid) != -1) {  // N, other IUPAC letters, U, or an illegal character somewhere in the chunk
                for (uint32_t h = 0; h < 32; h += 16) {
                    uint32_t w = 0, nb = 0;
                    for (uint32_t j = 0; j < 16; ++j) {
                        const uint8_t cc = g_codes.t[sq[i + h + j]];
                        if (cc < 4) w |= (uint32_t)cc << (2 * j);
                        else if (cc == 4) nb |= 1u << j;
                        else ok = false;
                    }
                    bw[(i + h) >> 4] = w;
                    if (nb) { nw[i >> 5] |= nb << h; saw_n = true; }
                }
                continue;
            }
            const __m256i t = _mm256_and_si256(_mm256_srli_epi16(c, 1), three);
            const __m256i code = _mm256_xor_si256(t, _mm256_and_si256(_mm256_srli_epi16(t, 1), one));
            const __m256i b4 = _mm256_madd_epi16(_mm256_maddubs_epi16(code, w16), w32);  // one byte (four letters) per 32-bit lane
            const __m256i packed = _mm256_shuffle_epi8(b4, pick);
            bw[i >> 4] = (uint32_t)_mm256_extract_epi32(packed, 0);
            bw[(i >> 4) + 1] = (uint32_t)_mm256_extract_epi32(packed, 4);
        }
        return i;
    }
    // sum of the bytes of p read as SIGNED chars (what `(int)qual[j]` sees; bytes above 127 do not occur in a valid FASTQ)
    __attribute__((target("avx2,popcnt"))) static int64_t char_sum_avx2(const char *q, size_t n) {
        const unsigned char *p = reinterpret_cast<const unsigned char *>(q);
        __m256i acc = _mm256_setzero_si256();
        size_t i = 0;
        int64_t high = 0;
        for (; i + 32 <= n; i += 32) {
            const __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(p + i));
            acc = _mm256_add_epi64(acc, _mm256_sad_epu8(v, _mm256_setzero_si256()));
            high += __builtin_popcount((unsigned)_mm256_movemask_epi8(v));
        }
        int64_t s = (int64_t)((uint64_t)_mm256_extract_epi64(acc, 0) + (uint64_t)_mm256_extract_epi64(acc, 1) + (uint64_t)_mm256_extract_epi64(acc, 2) + (uint64_t)_mm256_extract_epi64(acc, 3)) - 256 * high;
        for (; i < n; ++i) s += (int)q[i];
        return s;
    }
#endif
    // sum of (phred character - 33) over a quality string, as the int the reference accumulates (src/dehost_main.cpp:355-360)
    static int phred_sum(const char *q, uint32_t n) {
#if defined(__x86_64__)
        if (g_has_avx2) return (int)(char_sum_avx2(q, n) - 33 * (int64_t)n);
#endif
        int sum = 0;
        for (uint32_t j = 0; j < n; ++j) sum += (int)q[j] - 33;
        return sum;
    }
    // the kept records as (offset, length) pairs into one buffer
    void describe_text(bool paired, const Slab *slab, int copy_threads) {
        const size_t n = keep.size();
        so1.assign(n, 0); qo1.assign(n, 0); ql1.assign(n, 0);
        if (paired) { so2.assign(n, 0); qo2.assign(n, 0); ql2.assign(n, 0); } else { so2.clear(); qo2.clear(); ql2.clear(); }
        text_quals = false;
        for (size_t i = 0; i < n && !text_quals; ++i) text_quals = blk1.recs[keep[i]].qual_len != 0 || (paired && blk2.recs[keep[i]].qual_len != 0);
        text = nullptr; text_bytes = 0; text_from_slab = false;
        if (n == 0) return;
        if (!paired && slab && !slab->empty()) {
            // the slab as it stands: from the first kept stretch to the end of the last (ids and `+` lines ride along)
            const char *lo = slab->data() + slab->size(), *hi = slab->data();
            bool inside = true;
            for (size_t i = 0; i < n; ++i) {
                const RecView &a = blk1.recs[keep[i]];
                lo = std::min(lo, a.seq); hi = std::max(hi, a.seq + a.seq_len);
                if (a.qual_len) { lo = std::min(lo, a.qual); hi = std::max(hi, a.qual + a.qual_len); }
            }
            inside = lo >= slab->data() && hi <= slab->data() + slab->size() && lo <= hi;
            if (inside) {
                for (size_t i = 0; i < n; ++i) {
                    const RecView &a = blk1.recs[keep[i]];
                    so1[i] = (uint64_t)(a.seq - lo);
                    if (a.qual_len) { qo1[i] = (uint64_t)(a.qual - lo); ql1[i] = a.qual_len; }
                }
                text = reinterpret_cast<const uint8_t *>(lo); text_bytes = (uint64_t)(hi - lo); text_from_slab = true;
                return;
            }
        }
        // a copy of the letters and qualities alone: per read sequence, quality, mate sequence, mate quality
        uint64_t cur = 0;
        for (size_t i = 0; i < n; ++i) {
            const RecView &a = blk1.recs[keep[i]];
            so1[i] = cur; cur += a.seq_len;
            qo1[i] = cur; ql1[i] = a.qual_len; cur += a.qual_len;
            if (paired) {
                const RecView &b = blk2.recs[keep[i]];
                so2[i] = cur; cur += b.seq_len;
                qo2[i] = cur; ql2[i] = b.qual_len; cur += b.qual_len;
            }
        }
        tcopy.want_pinned = true;
        tcopy.assign_raw((size_t)((cur + 3) / 4) + 1);
        char *dst = reinterpret_cast<char *>(tcopy.data());
#pragma omp parallel for num_threads(copy_threads) schedule(dynamic, 64)
        for (long i = 0; i < (long)n; ++i) {
            const RecView &a = blk1.recs[keep[i]];
            std::memcpy(dst + so1[i], a.seq, a.seq_len);
            if (a.qual_len) std::memcpy(dst + qo1[i], a.qual, a.qual_len);
            if (paired) {
                const RecView &b = blk2.recs[keep[i]];
                std::memcpy(dst + so2[i], b.seq, b.seq_len);
                if (b.qual_len) std::memcpy(dst + qo2[i], b.qual, b.qual_len);
            }
        }
        text = reinterpret_cast<const uint8_t *>(dst); text_bytes = cur;
    }
    // layout + parallel packing, mean quality and gzip ratio of the records in blk1 (/blk2)
    // gz_gpu_max > 0: reads of at most that many letters get their gzip size from the device (finish_compression); gz_route_long: and
    // the reads beyond CHN_GZIP_MAX_LEN that gzip_long_device_limit gives the device in this batch
    std::vector<uint8_t> gz_pending;   // per kept read: its compression ratio is still to come
    uint32_t gz_gpu_len = 0;           // longest such read (what chn_batch.gzip_tallies asks for)
    // as_text: lay the batch out and form the host-side gzip ratios as ever, but neither pack the letters nor sum the qualities -- the
    // device does both (chn_text_submit); `slab`: the slab the records are views into, if they all are
    // resident (with as_text): the letters are in device memory and the caller has filled so1 / qo1 / ql1 from chn_text_split's
    // descriptors.  No ratio can be formed here, so every read's is "still to come": the device sizes those the routing gives it and
    // leaves 0 for the others, which finish_rows sizes on the host once their letters are fetched.
    void pack(bool paired, int threads, bool skip_compression, uint32_t gz_gpu_max = 0, bool gz_route_long = false, bool as_text = false,
              const Slab *slab = nullptr, bool resident = false) {
        const size_t nrec = blk1.recs.size();
        keep.clear();
        for (size_t i = 0; i < nrec; ++i) {
            const uint64_t L = (uint64_t)blk1.recs[i].seq_len + (paired ? blk2.recs[i].seq_len : 0);
            if (L == 0) { g_log.warn("Ignoring read " + std::string(blk1.recs[i].id, blk1.recs[i].id_len) + " as has zero length!"); continue; }  // src/dehost_main.cpp:351-354
            if (L > std::numeric_limits<uint32_t>::max()) { g_log.warn("Ignoring read as too long!"); continue; }
            keep.push_back((uint32_t)i);
        }
        const size_t n = keep.size();
        off1.assign(n, 0); len1.assign(n, 0); mq.assign(n, 0); comp.assign(n, 0);
        if (paired) { off2.assign(n, 0); len2.assign(n, 0); }
        uint64_t cur = 0;
        for (size_t i = 0; i < n; ++i) {
            const uint32_t k = keep[i];
            off1[i] = cur; len1[i] = blk1.recs[k].seq_len; cur += pad64(len1[i]);
            if (paired) { off2[i] = cur; len2[i] = blk2.recs[k].seq_len; cur += pad64(len2[i]); }
        }
        n_bases = std::max<uint64_t>(cur, 64);
        if (as_text) {}
        else if (cur == 0) { bases.assign_zero(n_bases / 16); nmask.assign_zero(n_bases / 32); }
        else { bases.assign_raw(n_bases / 16); nmask.assign_raw(n_bases / 32); }
        gz_pending.assign(n, 0); gz_gpu_len = 0;
        // (only where every read up to CHN_GZIP_MAX_LEN goes to the device already: the device then sizes every read up to the limit)
        if (gz_gpu_max >= CHN_GZIP_MAX_LEN && gz_route_long && !skip_compression) {
            std::vector<uint32_t> long_lens;
            uint64_t letters = 0;
            for (size_t i = 0; i < n; ++i) {
                const uint64_t L = (uint64_t)len1[i] + (paired ? len2[i] : 0);
                letters += L;
                if (L > CHN_GZIP_MAX_LEN) long_lens.push_back((uint32_t)L);
            }
            gz_gpu_max = std::max(gz_gpu_max, gzip_long_device_limit(long_lens, letters, threads));
        }
        if (gz_gpu_max && !skip_compression)
            for (size_t i = 0; i < n; ++i) {
                const uint64_t L = (uint64_t)len1[i] + (paired ? len2[i] : 0);
                if (L <= gz_gpu_max) { gz_pending[i] = 1; gz_gpu_len = std::max<uint32_t>(gz_gpu_len, (uint32_t)L); }
            }
        if (resident && !skip_compression) {  // (a length of 1 when nothing is routed to the device: the compression gate is then finish_rows')
            gz_pending.assign(n, 1);
            gz_gpu_len = std::max<uint32_t>(gz_gpu_len, 1);
        }
        bool saw_n = false, bad = false;
        // Letters -> 2-bit codes + N mask and the quality sums: what seqan3's READER does while it parses (sequence_file_input hands out dna5 ranks and
        // phred values), so it runs on the reader's threads -- `-t`, but never fewer than four -- like the decompression and the record splitting.
        // With the default `-t 1` the main thread used to pack for 3.6 of a 4.8 s read loop (4 M reads of 5 kb).
        const int conv_threads = std::max(threads, g_reader_threads);
        if (as_text && !resident) describe_text(paired, slab, conv_threads);
#pragma omp parallel num_threads(conv_threads) if (!as_text)
        {
            bool my_n = false, my_bad = false;
#pragma omp for schedule(dynamic, 16)
            for (long i = 0; i < (long)(as_text ? 0 : n); ++i) {
                const RecView &a = blk1.recs[keep[i]];
                const RecView *b = paired ? &blk2.recs[keep[i]] : nullptr;
                if (!put(a, off1[i], my_n)) my_bad = true;
                if (b && !put(*b, off2[i], my_n)) my_bad = true;
                // mean quality (src/dehost_main.cpp:355-360 / :441-450): int sum of phred (char - 33) / count, as float
                int sum = phred_sum(a.qual, a.qual_len);
                size_t cnt = a.qual_len;
                if (b) { cnt += b->qual_len; sum += phred_sum(b->qual, b->qual_len); }
                mq[i] = cnt ? static_cast<float>(sum) / static_cast<float>(cnt) : 0.0f;
            }
#pragma omp critical(batch_flags)
            { saw_n = saw_n || my_n; bad = bad || my_bad; }
        }
        // the gzip ratio of the reads the device does not size (src/dehost_main.cpp:363): per-read work of the reference's loop, on the -t threads
        bool host_gzip = false;
        if (!skip_compression && !bad)
            for (size_t i = 0; i < n && !host_gzip; ++i) host_gzip = !gz_pending[i];
        if (host_gzip) {
#pragma omp parallel num_threads(threads)
            {
                Deflater defl;
#pragma omp for schedule(dynamic, 16)
                for (long i = 0; i < (long)n; ++i)
                    if (!gz_pending[i]) comp[i] = defl.ratio(blk1.recs[keep[i]], paired ? &blk2.recs[keep[i]] : nullptr);
            }
        }
        any_n = saw_n;
        if (bad) throw std::runtime_error("parse error: illegal character in a sequence (only IUPAC nucleotide letters are accepted)");
    }
};

// bounded hand-over of parsed blocks from the reader thread
struct BlockQueue {
    std::mutex m;
    std::condition_variable cv;
    std::deque<std::shared_ptr<HostBatch>> q;
    bool done = false, aborted = false;
    std::string error;
    // false: the consumer has gone away (an error before or inside the read loop); the reader stops
    bool push(std::shared_ptr<HostBatch> b) {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return q.size() < 2 || aborted; });
        if (aborted) return false;
        q.push_back(std::move(b));
        cv.notify_all();
        return true;
    }
    void abort() { std::lock_guard<std::mutex> lk(m); aborted = true; q.clear(); cv.notify_all(); }
    void finish(const std::string &err) { std::lock_guard<std::mutex> lk(m); done = true; error = err; cv.notify_all(); }
    // for a second reader thread, once the first has been aborted and joined
    void reopen() { std::lock_guard<std::mutex> lk(m); q.clear(); done = aborted = false; error.clear(); }
    std::shared_ptr<HostBatch> pop() {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return !q.empty() || done; });
        if (q.empty()) return nullptr;
        std::shared_ptr<HostBatch> b = std::move(q.front());
        q.pop_front();
        cv.notify_all();
        return b;
    }
};
