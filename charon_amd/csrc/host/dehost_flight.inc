// dehost_flight.inc -- one GPU batch on its way through the pipeline, and the three things done to it that touch nothing else: cut,
// submit, wait
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a stand-alone header.

// One GPU batch on its way through the pipeline: its host arrays stay alive until chn_batch_wait has returned.
struct Flight {
    std::shared_ptr<HostBatch> parent;  // owns the slabs the record views point into
    std::shared_ptr<HostBatch> parent2; // CHARON_GPU_TEXT_PAIRS=1: owns the id bytes of the mates' records (file 2's block)
    HostBatch sub;
    uint32_t version = 0;
    uint64_t seq = 0;  // replica mode: position in input order (the ordered merge releases flights by it)
    bool resident = false;  // CHARON_GPU_TEXT=1: a text batch whose text is sub.dtext, in device memory
    bool device_records = false;  // CHARON_GPU_EXTRACT=1: the records of its called reads are formed on the device (decided after the wait)
    // what chn_batch_wait fills (per flight: the rows of batch i are written by another thread while batch i + 1 is waited for)
    std::vector<uint32_t> nh, cnt, unq;
    std::vector<double> prob;
    std::vector<uint8_t> call, conf, flags;
    std::vector<uint32_t> gz_sizes;

    size_t reads() const { return sub.keep.size(); }
    void let_go() { parent.reset(); parent2.reset(); device_records = false; }  // (FlightPool::recycle)
};

// How a batch is packed, the same for every batch of a run.
struct PackPlan {
    bool skip_compression = false;  // diagnostics build only
    // the gzip column's deflate pass on the GPU for reads up to CHN_GZIP_MAX_LEN letters (CHARON_GZIP_ON_HOST=1 / CHARON_ZLIB_ONLY=1: all on the host)
    // Long reads run few wavefronts per CU there (five for a 60 kb read, its class arrays in global memory): about what sixteen host threads
    // make of them with the size emulator -- so with that many host threads the longest reads (beyond 40 000 letters) stay on the host, in the
    // packing loop beside the GPU; with fewer threads everything up to the device's limit goes to the GPU (sweep: profiles/r02/cli_long_reads.txt).
    // Reads beyond CHN_GZIP_MAX_LEN are sized by the device's long-read pass (CHN_GZIP_SIZES_ALL) where gzip_long_device_limit says
    // it pays; CHARON_GZIP_GPU_MAX sets one length limit for everything instead (61440: every longer read on the host).
    uint32_t gz_gpu_max = 0;
    bool gz_route_long = false;

    explicit PackPlan(const DehostArguments &opt) {
#ifdef CHARON_DIAG  // diagnostics build only (make CXXFLAGS_EXTRA=-DCHARON_DIAG): a knob that changes the output has no place in the product binary
        skip_compression = std::getenv("CHARON_SKIP_COMPRESSION") != nullptr;  // NOT reference behaviour: prints 0
        if (skip_compression) g_log.warn("CHARON_SKIP_COMPRESSION set: the compression column is 0 (differs from the reference)");
#endif
        gz_gpu_max = (std::getenv("CHARON_GZIP_ON_HOST") || std::getenv("CHARON_ZLIB_ONLY") || !g_gzip_emulator) ? 0u : (opt.threads >= 12 ? 40000u : CHN_GZIP_MAX_LEN);
        gz_route_long = gz_gpu_max != 0;
        if (gz_gpu_max)
            if (const char *e = std::getenv("CHARON_GZIP_GPU_MAX")) {
                gz_gpu_max = (uint32_t)std::min<unsigned long long>(CHN_GZIP_ANY_LEN, std::max<unsigned long long>(1, std::strtoull(e, nullptr, 10)));
                gz_route_long = false;
            }
    }
};

// CHARON_TEXT_BATCHES=1: batches sent as their slab / as a page-locked copy (counted by whichever thread submits)
struct TextBatchCounts { std::atomic<uint64_t> slab{0}, copy{0}; };

// The end of the GPU batch that starts at record `begin` of `limit`: at most batch_reads records and batch_bases padded bases, the
// stream's capacity (need_of(i): the padded bases of record i, both mates of a pair)
template <class NeedOf>
size_t cut_batch(const DehostArguments &opt, size_t begin, size_t limit, NeedOf need_of) {
    uint64_t bases = 0;
    size_t end = begin;
    while (end < limit && end - begin < opt.batch_reads) {
        const uint64_t need = need_of(end);
        if (need > opt.batch_bases) throw std::runtime_error("a read is longer than CHARON_BATCH_BASES");
        if (bases + need > opt.batch_bases) break;
        bases += need; ++end;
    }
    return end;
}

// deflate pass and tree arithmetic on the device: four bytes per read come back (reads beyond CHN_GZIP_MAX_LEN: the long-read pass)
inline uint32_t gzip_output_for(const HostBatch &sub) { return sub.gz_gpu_len > CHN_GZIP_MAX_LEN ? CHN_GZIP_SIZES_ALL : CHN_GZIP_SIZES; }

chn_batch fill_batch(const DehostArguments &opt, Flight &fl) {
    HostBatch &sub = fl.sub;
    chn_batch bt = abi_struct<chn_batch>();
    bt.on_device = 0; bt.n_reads = sub.keep.size(); bt.n_bases = sub.n_bases;
    bt.bases2 = sub.bases.data(); bt.nmask = sub.any_n ? sub.nmask.data() : nullptr;
    bt.seg1_offset = sub.off1.data(); bt.seg1_length = sub.len1.data();
    bt.seg2_offset = opt.is_paired ? sub.off2.data() : nullptr; bt.seg2_length = opt.is_paired ? sub.len2.data() : nullptr;
    bt.mean_quality = sub.mq.data(); bt.compression = sub.comp.data();
    bt.gzip_tallies = sub.gz_gpu_len;  // > 0: the call kernel leaves the compression gate to finish()
    bt.gzip_output = gzip_output_for(sub);
    return bt;
}

// a packed batch through chn_batch_submit, or (CHARON_TEXT_BATCHES=1, a resident flight) the text itself through chn_text_submit.
// Any thread: reaches the flight, the stream and `counts` (atomic) alone.
void submit_flight(const DehostArguments &opt, TextBatchCounts &counts, chn_stream *st, Flight &fl) {
    if (!opt.text_batches && !fl.resident) {
        chn_batch bt = fill_batch(opt, fl);
        CHN_CHECK(chn_batch_submit(st, &bt));
        return;
    }
    HostBatch &sub = fl.sub;
    chn_text_batch2 tb2;  // (a chn_text_batch with the text of file 2 behind it: used as such by paired resident batches only)
    std::memset(&tb2, 0, sizeof tb2);
    chn_text_batch &tb = tb2.batch;
    tb.struct_size = sizeof tb; tb.n_reads = sub.keep.size(); tb.text = sub.text; tb.text_bytes = sub.text_bytes;
    tb.seq1_offset = sub.so1.data(); tb.seq1_length = sub.len1.data();
    if (sub.text_quals) { tb.qual1_offset = sub.qo1.data(); tb.qual1_length = sub.ql1.data(); }
    if (opt.is_paired) {
        tb.seq2_offset = sub.so2.data(); tb.seq2_length = sub.len2.data();
        if (sub.text_quals) { tb.qual2_offset = sub.qo2.data(); tb.qual2_length = sub.ql2.data(); }
    }
    tb.compression = sub.comp.data();
    tb.gzip_tallies = sub.gz_gpu_len;
    tb.gzip_output = gzip_output_for(sub);
    if (fl.resident) { tb.flags = CHN_TEXT_ON_DEVICE; tb.text = sub.dtext->buf; tb.text_bytes = sub.dtext->text_bytes; }
    if (fl.resident && sub.dtext2) { tb.struct_size = sizeof tb2; tb2.text2 = sub.dtext2->buf; tb2.text2_bytes = sub.dtext2->text_bytes; }
    else (sub.text_from_slab ? counts.slab : counts.copy) += 1;
    const int rc = chn_text_submit(st, &tb);
    // (the device met a byte that is no IUPAC nucleotide letter: what HostBatch::pack reports for a packed batch)
    if (rc == CHN_E_INVALID && std::strstr(chn_last_error(), "illegal byte"))
        throw InputError("parse error: illegal character in a sequence (only IUPAC nucleotide letters are accepted)");
    if (rc != CHN_OK) throw std::runtime_error(std::string("chn_text_submit failed: ") + chn_last_error());
}

// chn_batch_wait (chn_text_wait) into the flight's own arrays; `acc_wait` gets the seconds inside the call.
// Any thread: reaches the flight and the stream alone.
void wait_flight(const DehostArguments &opt, size_t C, chn_stream *st, Flight &fl, double &acc_wait) {
    HostBatch &sub = fl.sub;
    const size_t n = sub.keep.size();
    fl.nh.resize(n); fl.cnt.resize(n * C); fl.unq.resize(n * C); fl.prob.resize(n * C); fl.call.resize(n); fl.conf.resize(n); fl.flags.resize(n);
    chn_result rs = abi_struct<chn_result>();
    rs.on_device = 0;
    rs.num_hashes = fl.nh.data(); rs.counts = fl.cnt.data(); rs.unique_counts = fl.unq.data(); rs.probabilities = fl.prob.data();
    rs.call = fl.call.data(); rs.confidence = fl.conf.data(); rs.flags = fl.flags.data();
    if (sub.gz_gpu_len != 0) { fl.gz_sizes.resize(n); rs.gzip_sizes = fl.gz_sizes.data(); }
    const double tt = now();
    if (opt.text_batches || fl.resident) {  // the mean-quality column comes back with the results
        chn_text_result tr = abi_struct<chn_text_result>();
        tr.mean_quality = sub.mq.data();
        CHN_CHECK(chn_text_wait(st, &rs, &tr));
        sub.any_n = tr.has_n != 0;
    } else {
        CHN_CHECK(chn_batch_wait(st, &rs));
    }
    acc_wait += now() - tt;
}
