// dehost_rows.inc -- from a waited flight to its rows: the gzip column, the fast path, the --extract path, the letters a resident flight
// still needs on the host
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a stand-alone header.

// finish_rows() runs on the row writer's thread or on the main thread, never on both at once (RowWriter's rule, row_writer.inc): the
// members below are whoever's turn it is.  fetch_letters() is the main thread's, before the flight is handed on.
class RowStage {
public:
    uint64_t gz_on_device = 0, gz_long_on_device = 0;  // reads sized from the device's deflate tallies / by its long-read pass
    double t_gz = 0, t_rows = 0;                       // CHARON_TIMING: tallies -> sizes; rows
    uint64_t dt_fetched_records = 0, dt_fetched_bytes = 0;  // CHARON_GPU_TEXT=1: what chn_text_fetch brought down
    uint64_t dp_id2_bytes = 0;  // CHARON_GPU_TEXT_PAIRS=1: id bytes of file 2 that came down (with the split, or here with the letters)

    RowStage(const DehostArguments &opt, const IndexMeta &meta, Result &result, chn_stream *stream)
        : opt_(opt), meta_(meta), C_(meta.categories.size()), result_(result), stream_(stream),
          // (rows are FORMATTED by the reader's team as well -- -t, but never fewer than four: text out is the mirror of text in; the reference prints inside its
          //  critical section whatever -t is.  With the default -t 1 the main thread formatted rows for 1.0 of a 2.3 s read loop on 4 M reads.)
          rowbuf_((size_t)std::max<int>(1, std::max<int>((int)opt.threads, g_reader_threads))) {}

    // Fast path (models final, nothing to extract -- i.e. every plain `charon dehost` run after its first read): rows are formatted in
    // parallel straight from the result arrays into one buffer per thread and emitted in order; no per-read objects.  Otherwise the
    // reference's add_read state machine, read by read.
    void finish_rows(Flight &fl) {
        if (fl.sub.gz_gpu_len != 0) sizes_from_tallies(fl);
        const double t0 = now();
        auto lap_rows = scope_exit([this, t0] { t_rows += now() - t0; });
        if (opt_.run_extract) extract_rows(fl);
        else plain_rows(fl);
    }

    // After chn_text_wait: ONE chn_text_fetch for the reads whose letters the host needs -- the sequence of a read the device left
    // unsized, sequence and quality of every read under --extract (make_entry copies them; without --extract it reads the id alone,
    // in training too) -- into the flight's arena; the record views point there.  The block's buffer is let go afterwards.
    void fetch_letters(Flight &fl) {
        HostBatch &sub = fl.sub;
        const size_t n = sub.keep.size();
        const bool tallied = sub.gz_gpu_len != 0;
        // under --extract, sequence and quality of every read -- unless the flight's records are formed on the device (CHARON_GPU_EXTRACT=1)
        const bool letters = opt_.run_extract && !fl.device_records;
        const bool two = sub.dtext2 != nullptr;  // pairs over two texts: the same reads' mates out of file 2's block -- one fetch per text
        const bool ids2 = letters && g_gpu_extract && two;  // the ids of mate 2 did not come down with the split: with the letters, then
        std::vector<uint64_t> off[2];
        std::vector<uint32_t> len[2], who;
        uint64_t total[2] = {0, 0};
        auto range = [&](int k, uint64_t o, uint32_t l) { off[k].push_back(o); len[k].push_back(l); total[k] += l; };
        for (size_t i = 0; i < n; ++i) {
            if (!letters && !(tallied && sub.gz_pending[i] && fl.gz_sizes[i] == 0)) continue;
            who.push_back((uint32_t)i);
            range(0, sub.so1[i], sub.len1[i]);
            if (letters) range(0, sub.qo1[i], sub.ql1[i]);
            if (two) range(1, sub.so2[i], sub.len2[i]);
            if (two && letters) range(1, sub.qo2[i], sub.ql2[i]);
            if (ids2) { range(1, sub.io2[i], sub.il2[i]); dp_id2_bytes += sub.il2[i]; }
        }
        if (!who.empty()) {
            sub.arena.want_pinned = true;
            sub.arena.assign_raw((size_t)((total[0] + total[1]) / 4) + 2);
            uint8_t *arena = reinterpret_cast<uint8_t *>(sub.arena.data());
            for (int k = 0; k < (two ? 2 : 1); ++k) {  // mate 2's bytes behind mate 1's
                chn_text_fetch_job job = abi_struct<chn_text_fetch_job>();
                const DevBlock &blk = k ? *sub.dtext2 : *sub.dtext;
                job.text = blk.buf; job.text_bytes = blk.text_bytes;
                job.n_ranges = off[k].size(); job.offset = off[k].data(); job.length = len[k].data();
                job.out = arena + (k ? total[0] : 0); job.out_capacity = total[k];
                CHN_CHECK(chn_text_fetch(stream_, &job));
            }
            const char *at = reinterpret_cast<const char *>(arena), *at2 = at + total[0];
            for (uint32_t i : who) {
                RecView &r = sub.blk1.recs[sub.keep[i]];
                r.seq = at; at += sub.len1[i];
                if (letters) { r.qual = at; at += sub.ql1[i]; }
                if (!two) continue;
                RecView &m = sub.blk2.recs[sub.keep[i]];
                m.seq = at2; at2 += sub.len2[i];
                if (letters) { m.qual = at2; at2 += sub.ql2[i]; }
                if (ids2) { m.id = at2; m.id_len = sub.il2[i]; at2 += sub.il2[i]; }
            }
            dt_fetched_records += who.size(); dt_fetched_bytes += total[0] + total[1];
        }
        if (!fl.device_records) { sub.dtext.reset(); sub.dtext2.reset(); }
    }

private:
    const DehostArguments &opt_;
    const IndexMeta &meta_;
    const size_t C_;
    Result &result_;
    chn_stream *const stream_;  // stream 0 (fetch_letters)
    std::vector<std::string> rowbuf_;
    std::vector<Entry> entries_;

    uint32_t length_of(const HostBatch &sub, size_t i) const { return sub.len1[i] + (opt_.is_paired ? sub.len2[i] : 0u); }

    // the gzip column from the device's deflate tallies (exact: _tr_flush_block's arithmetic on the same frequencies), the host
    // emulator / zlib for the reads the device left out; then the compression gate the call kernel left open
    // (include/read_entry.hpp:189-191,250-252: no call below min_compression; the confidence score is unaffected)
    void sizes_from_tallies(Flight &fl) {
        HostBatch &sub = fl.sub;
        const std::vector<uint32_t> &gz_sizes = fl.gz_sizes;
        std::vector<uint8_t> &call = fl.call;
        const long n = (long)sub.keep.size();
        const bool paired = opt_.is_paired;
        const float min_compression = opt_.min_compression;
        uint64_t on_device = 0, long_on_device = 0;
        const double tt = now();
#pragma omp parallel num_threads(opt_.threads) reduction(+ : on_device, long_on_device)
        {
            Deflater defl;
#pragma omp for schedule(dynamic, 64)
            for (long i = 0; i < n; ++i) {
                const uint64_t L = (uint64_t)sub.len1[i] + (paired ? sub.len2[i] : 0);
                if (sub.gz_pending[i]) {
                    if (gz_sizes[i] != 0) {
                        sub.comp[i] = static_cast<float>(static_cast<double>(gz_sizes[i]) / static_cast<double>(L));
                        if (L <= CHN_GZIP_MAX_LEN) on_device += 1; else long_on_device += 1;
                    } else {
                        sub.comp[i] = defl.ratio(sub.blk1.recs[sub.keep[i]], paired ? &sub.blk2.recs[sub.keep[i]] : nullptr);
                    }
                }
                if (sub.comp[i] < min_compression) call[i] = 255;
            }
        }
        gz_on_device += on_device; gz_long_on_device += long_on_device;
        t_gz += now() - tt;
    }

    void make_entry(Flight &fl, size_t i, Entry &e) const {
        const HostBatch &sub = fl.sub;
        const size_t C = C_;
        const RecView &a = sub.blk1.recs[sub.keep[i]];
        e.read_id = first_token(a.id, a.id_len);
        e.length = length_of(sub, i);
        e.num_hashes = fl.nh[i]; e.mean_quality = sub.mq[i]; e.compression = sub.comp[i];
        e.counts.assign(fl.cnt.begin() + i * C, fl.cnt.begin() + (i + 1) * C);
        e.unique.assign(fl.unq.begin() + i * C, fl.unq.begin() + (i + 1) * C);
        e.prob.assign(fl.prob.begin() + i * C, fl.prob.begin() + (i + 1) * C);
        e.call = fl.call[i]; e.conf = fl.conf[i]; e.model_version = fl.version; e.row_version = fl.version;
        format_row(meta_, e, e.row);
        if (fl.device_records) {
            e.rec_index = (uint32_t)i;  // Result::extract notes the index; the letters stay on the device
        } else if (opt_.run_extract) {
            e.rec_id.assign(a.id, a.id_len); e.rec_seq.assign(a.seq, a.seq_len); e.rec_qual.assign(a.qual ? a.qual : "", a.qual_len);
            if (opt_.is_paired) {
                const RecView &b = sub.blk2.recs[sub.keep[i]];
                e.rec2_id.assign(b.id, b.id_len); e.rec2_seq.assign(b.seq, b.seq_len); e.rec2_qual.assign(b.qual ? b.qual : "", b.qual_len);
            }
        }
    }

    // nothing to extract
    void plain_rows(Flight &fl) {
        HostBatch &sub = fl.sub;
        const size_t C = C_, n = sub.keep.size();
        size_t i0 = 0;
        // until the models are final (the first read of a run, which the reference drops: include/result.hpp:139-151) go read by read
        while (i0 < n && !result_.models_final()) {
            Entry e;
            make_entry(fl, i0, e);
            result_.add_read(e);
            ++i0;
        }
        if (i0 == n) return;
        if (result_.current_model_version() != fl.version) {
            // the models changed while this batch was on the device (gamma: force_ready moves the neg distribution's location,
            // include/classify_stats.hpp:306-312): bring the rest of the batch up to date in one device call
            std::vector<uint32_t> lens(n - i0);
            for (size_t i = i0; i < n; ++i) lens[i - i0] = length_of(sub, i);
            result_.reclassify_raw(n - i0, fl.nh.data() + i0, fl.cnt.data() + i0 * C, fl.unq.data() + i0 * C, lens.data(), sub.mq.data() + i0, sub.comp.data() + i0,
                                   fl.prob.data() + i0 * C, fl.call.data() + i0, fl.conf.data() + i0);
        }
        const int T = (int)rowbuf_.size();
        std::vector<std::vector<uint64_t>> per_call((size_t)T, std::vector<uint64_t>(C + 1, 0));
#pragma omp parallel num_threads(T)
        {
#ifdef _OPENMP
            const int tid = omp_get_thread_num(), nt = omp_get_num_threads();
#else
            const int tid = 0, nt = 1;
#endif
            const size_t span = n - i0, lo = i0 + span * (size_t)tid / (size_t)nt, hi = i0 + span * (size_t)(tid + 1) / (size_t)nt;
            std::string &out = rowbuf_[(size_t)tid];
            out.clear();
            for (size_t i = lo; i < hi; ++i) {
                const RecView &a = sub.blk1.recs[sub.keep[i]];
                const void *sp = std::memchr(a.id, ' ', a.id_len);  // read_id = id up to the first space (src/dehost_main.cpp:345)
                const size_t idn = sp ? (size_t)(static_cast<const char *>(sp) - a.id) : (size_t)a.id_len;
                format_row_raw(meta_, a.id, idn, fl.call[i], length_of(sub, i), fl.nh[i], sub.mq[i], fl.conf[i], sub.comp[i],
                               fl.cnt.data() + i * C, fl.unq.data() + i * C, fl.prob.data() + i * C, out);
                per_call[(size_t)tid][fl.call[i] < 255 ? fl.call[i] : C] += 1;
            }
        }
        for (int t = 0; t < T; ++t) result_.bulk(rowbuf_[(size_t)t], per_call[(size_t)t]);
    }

    // --extract: build the entries and format their rows in parallel, then critical(add_read_to_results): serial, in input order (what
    // the reference does at -t 1).  When a model finishes training in the middle of the batch, the rest of the batch is brought up to
    // date in one device call.
    void extract_rows(Flight &fl) {
        HostBatch &sub = fl.sub;
        const size_t n = sub.keep.size();
        entries_.assign(n, Entry());
#pragma omp parallel for num_threads(opt_.threads) schedule(static)
        for (long i = 0; i < (long)n; ++i) make_entry(fl, (size_t)i, entries_[(size_t)i]);
        if (fl.device_records) result_.begin_device_records();
        for (size_t i = 0; i < n; ++i) {
            if (result_.models_final() && entries_[i].model_version != result_.current_model_version()) result_.refresh(entries_, i);
            result_.add_read(entries_[i]);
        }
        if (!fl.device_records) return;
        // every read went through classify_read at once (the models are final and this flight's version is current): one
        // chn_extract_append_records per extract file that got records, mate 1's out of the flight's text, mate 2's out of its second
        Result::DeviceRecords dr;
        dr.text[0] = sub.dtext->buf; dr.text_bytes[0] = sub.dtext->text_bytes;
        dr.id_off[0] = sub.io1.data(); dr.id_len[0] = sub.il1.data(); dr.seq_off[0] = sub.so1.data(); dr.seq_len[0] = sub.len1.data();
        dr.qual_off[0] = sub.qo1.data(); dr.qual_len[0] = sub.ql1.data();
        if (sub.dtext2) {
            dr.text[1] = sub.dtext2->buf; dr.text_bytes[1] = sub.dtext2->text_bytes;
            dr.id_off[1] = sub.io2.data(); dr.id_len[1] = sub.il2.data(); dr.seq_off[1] = sub.so2.data(); dr.seq_len[1] = sub.len2.data();
            dr.qual_off[1] = sub.qo2.data(); dr.qual_len[1] = sub.ql2.data();
        }
        auto let_go = scope_exit([&sub] { sub.dtext.reset(); sub.dtext2.reset(); });  // the blocks' buffers, once the calls have returned
        result_.append_device_records(dr);
    }
};
