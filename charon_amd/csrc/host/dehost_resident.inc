// dehost_resident.inc -- CHARON_GPU_TEXT=1: the read loop while the text stays in device memory
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a stand-alone header.

// Everything that touches the stream -- split, submit, wait, fetch -- runs on the main thread (one stream per host thread), so the
// replica threads are not used: up to two batches are in flight while the next is split and submitted.  The side readers' threads
// reach their SideReader alone (dehost_readers.inc); everything in here is the main thread's.
//
// The loop over `n_sides` files: one (single-end) or two (CHARON_GPU_TEXT_PAIRS=1).  Each side (file) keeps its current block, the
// descriptors of the records that are split but not yet in a batch, and `consumed`.  A side with no such record left takes its next
// block (the tail of the block before carried in front of it); a side that still has some does not, so files with records of unequal
// size never pile up text and no record is split twice.  The records at hand -- with two sides the pairs: the shorter of the two
// lists -- therefore lie in ONE block of either file, and a batch of them is a chn_text_batch (chn_text_batch2) over it (them).  The
// ids of a batch of pairs are compared on the device before the submit; the ids of file 2 come down with the split under --extract only.
class ResidentLoop {
public:
    uint64_t dt_split_records = 0;
    double t_split = 0;
    uint64_t dp_pairs_checked = 0;  // CHARON_GPU_TEXT_PAIRS=1: pairs through chn_text_pair_ids
    double t_pair = 0;

    ResidentLoop(MainThread &mt, const RunModes &modes, SideReader (&readers)[2], HostReader &host_reader)
        : mt_(mt), opt_(mt.opt), stream_(mt.stream), n_sides_(modes.n_sides), two_(modes.n_sides == 2), fasta_(modes.fasta_side),
          block_bytes_(modes.resident_block_bytes), dev_(g_gpu_text_device), readers_(readers), host_reader_(host_reader) {}

    // To the end of the files -- then the host reader's queue is finished (with the error a side reader met, if one did) and the host
    // loop finds nothing to do -- or until a side meets text the device cannot go on splitting: then the host reader runs from there.
    void run() {
        // what the loop holds is let go when it is left; by an exception: the device is done with the flying flights' arrays before they are freed
        auto let_go = scope_exit([this] {
            if (!flying_.empty()) (void)chn_stream_sync(stream_);
            flying_.clear();
            side_[0] = Side(); side_[1] = Side();
        });
        Side &s1 = side_[0], &s2 = side_[1];
        for (;;) {
            // Leaving the mode is noted here and done once the records at hand are submitted: side `leaving` met text the device cannot
            // go on splitting.
            int leaving = -1;
            for (int k = 0; k < n_sides_ && leaving < 0; ++k)
                while (side_[k].unpaired() == 0 && !side_[k].eof)  // (a block may end inside its first record and yield none)
                    if (take_block(k)) { leaving = k; break; }
            size_t avail = two_ ? std::min(s1.unpaired(), s2.unpaired()) : s1.unpaired();
            if (avail == 0 && leaving < 0) break;  // a file has run out: the records submitted so far are all there are
            while (avail) {
                const size_t cnt = cut_batch(opt_, 0, avail, [&](size_t i) {
                    return HostBatch::pad64(s1.seq_len[s1.head + i]) + (two_ ? HostBatch::pad64(s2.seq_len[s2.head + i]) : 0);
                });
                if (two_) check_pair_ids(cnt);
                std::unique_ptr<Flight> fl = mt_.pool.take();
                fill_flight(*fl, cnt);
                avail -= cnt;
                if (fl->sub.keep.empty()) { fl->sub.dtext.reset(); fl->sub.dtext2.reset(); continue; }
                submit(fl);
            }
            if (leaving >= 0) { leave(leaving); return; }
        }
        while (!flying_.empty()) retire_front();
        stop_side_readers();
        host_reader_.queue.finish(reader_failure_);
    }

private:
    struct Side {
        std::shared_ptr<HostBatch> hb;   // the block's holder: owns the id bytes its records' views point into
        std::shared_ptr<DevBlock> blk;   // the current block (kept at the end of the file: leaving the mode resumes behind it)
        std::shared_ptr<DevBlock> letters;  // CHARON_GPU_TEXT_FASTA=1: the unwrapped letters of blk's records; seq_off are offsets into it
        std::vector<uint64_t> id_off, seq_off, qual_off;  // records split from `blk`; those from `head` on are not yet paired
        std::vector<uint32_t> id_len, seq_len;
        std::vector<const char *> id;    // the id bytes (null where they did not come down)
        size_t head = 0;
        uint64_t consumed = 0;           // behind the last split record
        uint64_t paired_end = 0;         // behind the last PAIRED record (one side: the last record in a batch)
        bool eof = false;
        size_t unpaired() const { return id_off.size() - head; }
        void clear_records() { id_off.clear(); seq_off.clear(); qual_off.clear(); id_len.clear(); seq_len.clear(); id.clear(); head = 0; }
    };
    static const uint64_t kSplitRecords = 1u << 18;  // per split call (its scratch is 52 bytes per record of this bound); a block with more takes several

    MainThread &mt_;
    const DehostArguments &opt_;
    chn_stream *const stream_;
    const int n_sides_;
    const bool two_, fasta_;
    const size_t block_bytes_;
    const int dev_;
    SideReader (&readers_)[2];
    HostReader &host_reader_;
    Side side_[2];
    std::deque<std::unique_ptr<Flight>> flying_;  // submitted, oldest first
    std::string reader_failure_;
    std::vector<uint64_t> ido_, sqo_, qlo_;  // split scratch (sized by the first call: a run that is not resident never pays for them)
    std::vector<uint32_t> idl_, sql_;

    void retire_front() {
        std::unique_ptr<Flight> f = std::move(flying_.front());
        flying_.pop_front();
        mt_.wait_here(*f);
        // CHARON_GPU_EXTRACT=1: with final models and a current version every read of the flight is classified and written at once, so
        // its records can be formed where the text is; otherwise (training, or a version the models have moved on from) today's path
        f->device_records = g_gpu_extract && opt_.run_extract && mt_.result.models_final() && mt_.result.current_model_version() == f->version;
        const double tk = now();
        mt_.rows.fetch_letters(*f);
        mt_.t_fetch += now() - tk;
        mt_.writer.hand_on(f);
    }
    // a packed resident flight on its way: at most two in flight, the models pushed while they train, one batch at a time until they are final
    void submit(std::unique_ptr<Flight> &fl) {
        while (flying_.size() >= 2) retire_front();
        // (while the models are in training every batch is retired before the next is submitted, so nothing is in flight here)
        mt_.submit_here(*fl);
        flying_.push_back(std::move(fl));
        if (!mt_.result.models_final()) retire_front();
    }
    // the side readers are done with (one may still wait to hand over a block nobody wants)
    void stop_side_readers() {
        for (int s = 0; s < n_sides_; ++s) readers_[s].queue.abort();
        for (int s = 0; s < n_sides_; ++s) if (readers_[s].t.joinable()) readers_[s].t.join();
        for (int s = 0; s < n_sides_; ++s) { side_[s].hb.reset(); side_[s].blk.reset(); side_[s].letters.reset(); }
    }
    // Leaving the mode because of side k: every flight retired, each side's text from behind its last paired record downloaded, the
    // side readers stopped, and the host reader started with every file resumed.  That text and the rest of the files go through the
    // host's splitter and sequential parser, which produce today's rows and today's messages.
    void leave(int k) {
        while (!flying_.empty()) retire_front();
        for (int s = 0; s < n_sides_; ++s) {
            Side &sd = side_[s];
            host_reader_.resumed[s] = true;
            if (!sd.blk) continue;  // (no block of this file was taken: it starts from its first member)
            host_reader_.resume_z[s] = sd.blk->z_end;
            const uint64_t from = sd.paired_end, end = sd.blk->text_bytes;
            host_reader_.resume_carry[s].resize((size_t)(end - from));
            if (end > from) CHN_CHECK(chn_device_download(dev_, host_reader_.resume_carry[s].data(), sd.blk->buf + from, end - from));
        }
        const Side &sk = side_[k];
        g_log.info("CHARON_GPU_TEXT=1: leaving the device-resident path at byte " + std::to_string(sk.blk->file_offset + sk.consumed - sk.blk->member0) +
                   " of the inflated file " + (two_ ? (k ? opt_.read_file2 : opt_.read_file) + " " : "") +
                   (fasta_ ? "(text that is no FASTA record the device takes, or a record longer than a block)" : "(text that is no plain four-line record)") +
                   ": the host parser goes on from there");
        stop_side_readers();
        g_gpu_inflate = true; g_gpu_inflate_device = dev_; g_pin_slabs = true;  // inflate as under CHARON_GPU_INFLATE=1 from here on
        host_reader_.start(opt_);
    }
    // The tail [prev_from, prev->text_bytes) of the block before copied in front of member 0 of `blk`, so that it ends where member 0
    // begins; a tail longer than the gap (a record longer than the headroom) gets a fresh buffer for the two, which replaces `blk` (and
    // hb.dtext).  Returns where the text of `blk` now starts.
    uint64_t carry_tail(const std::shared_ptr<DevBlock> &prev, uint64_t prev_from, std::shared_ptr<DevBlock> &blk, HostBatch &hb) {
        const uint64_t tail = prev->text_bytes - prev_from, body = blk->text_bytes - blk->member0;
        if (tail > blk->member0) {
            std::shared_ptr<DevBlock> fresh(new DevBlock());
            void *p = nullptr;
            fresh->cap = (size_t)((tail + body + 15) & ~15ULL);
            CHN_CHECK(chn_device_malloc(dev_, fresh->cap, &p));
            fresh->buf = static_cast<uint8_t *>(p);
            fresh->member0 = tail; fresh->text_bytes = tail + body; fresh->file_offset = blk->file_offset;
            fresh->z_end = blk->z_end; fresh->last = blk->last;
            if (body) CHN_CHECK(chn_device_copy(dev_, fresh->buf + tail, blk->buf + blk->member0, body));
            blk = fresh;
            hb.dtext = fresh;
        }
        if (tail) CHN_CHECK(chn_device_copy(dev_, blk->buf + blk->member0 - tail, prev->buf + prev_from, tail));
        return blk->member0 - tail;
    }
    // what chn_text_split_job and chn_fasta_split_job have in common
    template <class Job>
    Job split_job(const DevBlock &blk, uint64_t from, uint8_t *ids, uint64_t ids_capacity) {
        Job job = abi_struct<Job>();
        job.text = blk.buf; job.text_bytes = blk.text_bytes; job.start = from; job.max_records = kSplitRecords;
        job.id_offset = ido_.data(); job.id_length = idl_.data(); job.seq_offset = sqo_.data(); job.seq_length = sql_.data();
        job.ids = ids; job.ids_capacity = ids_capacity;
        return job;
    }
    // The records of blk's text from `start` on, appended to sd's lists: descriptors and (want_ids) id bytes come back, letters and
    // qualities stay where they are.  The id bytes go to hb.ids.  Returns the offset behind the last record; *ids_bytes the id bytes
    // that came down.  A block with more than kSplitRecords records takes several calls.
    // `letters` (CHARON_GPU_TEXT_FASTA=1): chn_fasta_split unwraps the letters of the records it takes into that buffer, of blk's
    // capacity, and sd gets sequence offsets into THAT buffer (and no quality offset); each call writes behind the letters of the one
    // before, from the next multiple of 16 on.  (Room: a call that stops at the bound has dropped at least ">\n" of each of its 2^18
    // records, so the letters end more than 512 KiB below the text they came from.)  `eoi`: no text follows, the end counts as the
    // last record's end.
    uint64_t split_block(const DevBlock &blk, DevBlock *letters, bool eoi, uint64_t start, bool want_ids, HostBatch &hb, Side &sd, uint64_t *ids_bytes) {
        const uint64_t end = blk.text_bytes;
        uint64_t consumed = start, ids_used = 0, base = 0;
        if (want_ids) hb.ids.reset(new char[end - start + 1]);
        if (ido_.empty()) { ido_.resize(kSplitRecords); sqo_.resize(kSplitRecords); qlo_.resize(kSplitRecords); idl_.resize(kSplitRecords); sql_.resize(kSplitRecords); }
        if (letters) letters->text_bytes = 0;
        for (;;) {
            uint8_t *ids = want_ids ? reinterpret_cast<uint8_t *>(hb.ids.get()) + ids_used : nullptr;
            const uint64_t ids_capacity = want_ids ? end - start - ids_used : 0;
            uint64_t n_records = 0, got_ids = 0, next_base = 0;
            if (letters) {
                chn_fasta_split_job job = split_job<chn_fasta_split_job>(blk, consumed, ids, ids_capacity);
                job.flags = eoi ? CHN_FASTA_SPLIT_END_OF_INPUT : 0;
                job.seq_text = letters->buf + base; job.seq_capacity = letters->cap - base;
                CHN_CHECK(chn_fasta_split(stream_, &job));
                n_records = job.n_records; got_ids = job.ids_bytes; consumed = job.consumed;
                letters->text_bytes = base + job.seq_bytes;
                next_base = base + ((job.seq_bytes + 15) & ~15ULL);
            } else {
                chn_text_split_job job = split_job<chn_text_split_job>(blk, consumed, ids, ids_capacity);
                job.qual_offset = qlo_.data();
                CHN_CHECK(chn_text_split(stream_, &job));
                n_records = job.n_records; got_ids = job.ids_bytes; consumed = job.consumed;
            }
            const char *id = reinterpret_cast<const char *>(ids);
            for (uint64_t i = 0; i < n_records; ++i) {
                sd.id.push_back(id); sd.id_len.push_back(idl_[i]); sd.seq_len.push_back(sql_[i]);
                sd.id_off.push_back(ido_[i]); sd.seq_off.push_back(base + sqo_[i]); sd.qual_off.push_back(letters ? 0 : qlo_[i]);
                if (id) id += idl_[i];
            }
            if (want_ids) ids_used += got_ids;
            base = next_base;
            if (n_records < kSplitRecords) break;
        }
        if (ids_bytes) *ids_bytes = ids_used;
        return consumed;
    }
    // the next block of side k, the tail of the block before in front of it, split into records.  true: the mode has to be left
    bool take_block(int k) {
        Side &sd = side_[k];
        const double tp = now();
        std::shared_ptr<HostBatch> hbp = readers_[k].queue.pop();
        mt_.t_pop += now() - tp;
        if (!hbp) {  // the end of the file, or the reader's error
            sd.eof = true;
            if (!readers_[k].queue.error.empty()) reader_failure_ = readers_[k].queue.error;
            return false;
        }
        HostBatch &hb = *hbp;
        std::shared_ptr<DevBlock> blk = hb.dtext;
        const double tk = now();
        uint64_t start = blk->member0;
        // (every record of the block before is paired: its tail is [consumed, text_bytes))
        if (sd.blk) start = carry_tail(sd.blk, sd.consumed, blk, hb);
        const uint64_t end = blk->text_bytes;
        // the TSV prints the id of mate 1; mate 2's is written under --extract only -- and under CHARON_GPU_EXTRACT=1 out of the device
        // text, or (a flight on the host path) fetched with its letters
        const bool want_ids = k == 0 || (opt_.run_extract && !g_gpu_extract);
        sd.clear_records();
        uint64_t ids_bytes = 0;
        if (fasta_) {  // a buffer of the block's size for the letters: of the pool where the block's is
            sd.letters.reset(new DevBlock());
            DevBlock &lt = *sd.letters;
            lt.cap = blk->cap;
            if (blk->pooled) { lt.buf = static_cast<uint8_t *>(g_dev_text_pool.take(lt.cap)); lt.pooled = true; }
            else { void *p = nullptr; CHN_CHECK(chn_device_malloc(dev_, lt.cap, &p)); lt.buf = static_cast<uint8_t *>(p); }
        }
        const uint64_t consumed = split_block(*blk, fasta_ ? sd.letters.get() : nullptr, blk->last, start, want_ids, hb, sd, &ids_bytes);
        if (k == 1) mt_.rows.dp_id2_bytes += ids_bytes;
        t_split += now() - tk;
        dt_split_records += sd.id_off.size();
        sd.hb = hbp; sd.blk = blk; sd.consumed = consumed; sd.paired_end = start;
        if (fasta_) {
            // At the end of the file everything is taken unless the rule failed.  Before it, text is left over behind the last record
            // taken (at least its successor's header), which the next block completes -- unless no record was taken at all: then
            // the text at `consumed` is no header line, or its record is empty (a second header line follows), or the record does
            // not end in this text; that one is carried on while it is shorter than a block
            if (consumed >= end) return false;
            if (blk->last) return true;
            if (!sd.id_off.empty()) return false;
            Slab tail_text((size_t)(end - consumed));
            CHN_CHECK(chn_device_download(dev_, tail_text.data(), blk->buf + consumed, end - consumed));
            const char *t = tail_text.data(), *te = t + tail_text.size();
            if (*t != '>' && *t != ';') return true;
            for (const char *nl = static_cast<const char *>(std::memchr(t, '\n', (size_t)(te - t))); nl && nl + 1 < te;
                 nl = static_cast<const char *>(std::memchr(nl + 1, '\n', (size_t)(te - nl - 1))))
                if (nl[1] == '>' || nl[1] == ';') return true;
            return end - consumed >= block_bytes_;
        }
        // no record although four line feeds follow `start` (a wrapped record, a blank line, a damaged record), or bytes behind the
        // last record at the end of the file (a last line without a line feed)
        if (consumed < end && (sd.id_off.empty() || blk->last)) {
            if (blk->last) return true;
            Slab tail_text((size_t)(end - consumed));
            CHN_CHECK(chn_device_download(dev_, tail_text.data(), blk->buf + consumed, end - consumed));
            if (std::count(tail_text.begin(), tail_text.end(), '\n') >= 4) return true;
        }
        return false;
    }
    // the ids of the next `cnt` pairs must agree after dropping the last character (src/dehost_main.cpp:423-430): on the device
    void check_pair_ids(size_t cnt) {
        Side &s1 = side_[0], &s2 = side_[1];
        const double tk = now();
        chn_text_pair_job pj = abi_struct<chn_text_pair_job>();
        pj.text1 = s1.blk->buf; pj.text1_bytes = s1.blk->text_bytes; pj.text2 = s2.blk->buf; pj.text2_bytes = s2.blk->text_bytes;
        pj.n_pairs = cnt; pj.id1_offset = s1.id_off.data() + s1.head; pj.id1_length = s1.id_len.data() + s1.head;
        pj.id2_offset = s2.id_off.data() + s2.head; pj.id2_length = s2.id_len.data() + s2.head;
        CHN_CHECK(chn_text_pair_ids(stream_, &pj));
        t_pair += now() - tk;
        dp_pairs_checked += cnt;
        if (pj.first_mismatch >= cnt) return;
        const size_t a = s1.head + (size_t)pj.first_mismatch, b = s2.head + (size_t)pj.first_mismatch;
        while (!flying_.empty()) retire_front();
        mt_.writer.drain();
        const uint32_t la = s1.id_len[a] ? s1.id_len[a] - 1 : 0, lb = s2.id_len[b] ? s2.id_len[b] - 1 : 0;
        std::string id2(lb, '\0');
        if (lb) {  // the one id of file 2 this run needs on the host
            chn_text_fetch_job job = abi_struct<chn_text_fetch_job>();
            const uint64_t o = s2.id_off[b];
            job.text = s2.blk->buf; job.text_bytes = s2.blk->text_bytes;
            job.n_ranges = 1; job.offset = &o; job.length = &lb;
            job.out = reinterpret_cast<uint8_t *>(&id2[0]); job.out_capacity = lb;
            CHN_CHECK(chn_text_fetch(stream_, &job));
        }
        pairs_do_not_match(s1.id[a], la, id2.data(), lb);
    }
    // the record views of the next `cnt` records of a side
    void views(const Side &sd, size_t cnt, std::vector<RecView> &recs) const {
        recs.resize(cnt);
        for (size_t i = 0; i < cnt; ++i) {
            RecView r;
            r.id = sd.id[sd.head + i]; r.id_len = r.id ? sd.id_len[sd.head + i] : 0; r.seq_len = sd.seq_len[sd.head + i];
            r.qual_len = fasta_ ? 0 : r.seq_len;
            recs[i] = r;
        }
    }
    // where the letters, qualities and ids of the reads a flight keeps lie in a side's text
    static void columns(const Side &sd, const HostBatch &sub, const std::vector<uint32_t> &len, std::vector<uint64_t> &so, std::vector<uint64_t> &qo,
                        std::vector<uint32_t> &ql, std::vector<uint64_t> &io, std::vector<uint32_t> &il) {
        const size_t n = sub.keep.size();
        so.resize(n); qo.resize(n); ql = len;
        if (g_gpu_extract) { io.resize(n); il.resize(n); }
        for (size_t i = 0; i < n; ++i) {
            const size_t a = sd.head + sub.keep[i];
            so[i] = sd.seq_off[a]; qo[i] = sd.qual_off[a];
            if (g_gpu_extract) { io[i] = sd.id_off[a]; il[i] = sd.id_len[a]; }
        }
    }
    // The next `cnt` records of every side as one flight: record views and pack, then where their letters, qualities and ids lie in
    // the texts (with one side the second halves stay cleared); every side moves on by `cnt`.
    void fill_flight(Flight &fl, size_t cnt) {
        Side &s1 = side_[0], &s2 = side_[1];
        fl.parent = s1.hb;
        if (two_) fl.parent2 = s2.hb;
        fl.resident = true;
        HostBatch &sub = fl.sub;
        views(s1, cnt, sub.blk1.recs);
        if (two_) views(s2, cnt, sub.blk2.recs);
        const double tk = now();
        sub.pack(two_, opt_.threads, mt_.plan.skip_compression, mt_.plan.gz_gpu_max, mt_.plan.gz_route_long, true, nullptr, true);
        columns(s1, sub, sub.len1, sub.so1, sub.qo1, sub.ql1, sub.io1, sub.il1);
        if (two_) columns(s2, sub, sub.len2, sub.so2, sub.qo2, sub.ql2, sub.io2, sub.il2);
        else { sub.so2.clear(); sub.qo2.clear(); sub.ql2.clear(); }
        sub.text_quals = !fasta_; sub.text_from_slab = false;
        if (fasta_) sub.ql1.assign(sub.keep.size(), 0);  // (no quality string: the ranges fetch_letters asks for them are empty)
        sub.dtext = fasta_ ? s1.letters : s1.blk;
        if (two_) sub.dtext2 = s2.blk;
        mt_.t_pack += now() - tk;
        for (int k = 0; k < n_sides_; ++k) {
            Side &sd = side_[k];
            sd.head += cnt;
            sd.paired_end = sd.unpaired() ? sd.id_off[sd.head] - 1 : sd.consumed;  // ('@' stands in front of an id)
        }
    }
};
const uint64_t ResidentLoop::kSplitRecords;
