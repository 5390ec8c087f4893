// dehost_setup.inc -- from the index file to streams with their models: the index in HBM, its replicas, the self-checks
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a stand-alone header.

// loader self-check (v), SURVEY 8(c): if a reference FASTA recorded in the index (filepath_to_bin) is still readable, every
// minimiser of it must be found in its bin.  This is the first-contact test for the third-party behaviour this build
// only recalls (seqan3's hash_and_fit fastrange vs the older modulo variant, seeds, alphabet): a miss is reported loudly
// in the log and on stderr, never guessed around.  Only the first 200 kb of at most 8 files are probed.
void self_check_reference_files(const IndexMeta &meta, chn_stream *stream, const DehostArguments &opt) {
    size_t checked = 0;
    for (const auto &fb : meta.filepath_to_bin) {
        if (checked >= 8) break;
        if (!is_file(fb.first)) continue;
        try {
            BlockReader in(fb.first);
            RawBlock blk;
            if (!in.next(blk, 4, 1 << 20)) continue;
            HostBatch hb;
            // the first 200 kb of each record, in pieces of 4 kb: every window of a piece is a window of the record, so a piece's
            // minimisers are minimisers of the record -- and 50 short reads fill a wavefront where one long read keeps a single lane
            // busy for 40 ms
            for (const RecView &r : blk.recs) {
                const uint32_t take = std::min<uint32_t>(r.seq_len, 200000);
                for (uint32_t o = 0; o < take; o += 4096) {
                    RecView piece = r;
                    piece.seq = r.seq + o; piece.seq_len = std::min<uint32_t>(4096, take - o);
                    piece.qual = nullptr; piece.qual_len = 0;
                    hb.blk1.recs.push_back(piece);
                }
            }
            hb.pack(false, 1, true);
            const size_t n = hb.keep.size();
            if (n == 0 || n > opt.batch_reads || hb.n_bases > opt.batch_bases) continue;
            chn_batch bt = abi_struct<chn_batch>();
            bt.n_reads = n; bt.n_bases = hb.n_bases; bt.bases2 = hb.bases.data();
            bt.nmask = hb.any_n ? hb.nmask.data() : nullptr; bt.seg1_offset = hb.off1.data(); bt.seg1_length = hb.len1.data();
            CHN_CHECK(chn_batch_submit(stream, &bt));
            const size_t C = meta.categories.size();
            std::vector<uint32_t> nh(n), cnt(n * C), unq(n * C);
            chn_result rs = abi_struct<chn_result>();
            rs.num_hashes = nh.data(); rs.counts = cnt.data(); rs.unique_counts = unq.data();
            CHN_CHECK(chn_batch_wait(stream, &rs));
            const uint8_t cat = meta.category_index(meta.bin_to_category.at(fb.second));
            for (size_t i = 0; i < n; ++i) {
                // counts_[cat] is the best bin of the category: it must be at least what the file's own bin holds = all of them
                if (cnt[i * C + cat] != nh[i]) {
                    const std::string msg = "self-check FAILED: only " + std::to_string(cnt[i * C + cat]) + " of " + std::to_string(nh[i]) +
                                            " minimisers of " + fb.first + " are found in the index -- the hash / alphabet conventions of this build do not match the program that wrote the index";
                    g_log.error(msg);
                    std::fprintf(stderr, "charon: %s\n", msg.c_str());
                    return;
                }
            }
            ++checked;
        } catch (std::exception &e) {
            g_log.debug(std::string("self-check skipped for ") + fb.first + ": " + e.what());
        }
    }
    if (checked) g_log.info("self-check: minimisers of " + std::to_string(checked) + " reference file(s) all found in their bins");
}

// What the options ask of this index: the category to extract exists, the extract files' names, a supported distribution.
// false: refused (the message is in the log); the caller returns 1.
bool settle_outputs(DehostArguments &opt, const IndexMeta &meta) {
    opt.run_extract = !opt.category_to_extract.empty();
    if (opt.run_extract && opt.category_to_extract != "all" &&
        std::find(meta.categories.begin(), meta.categories.end(), opt.category_to_extract) == meta.categories.end()) {
        std::string options;
        for (auto &c : meta.categories) options += c + " ";
        g_log.error("Cannot extract " + opt.category_to_extract + ", please chose one of [ all " + options + "]");
        return false;  // the reference's callback drops this value: exit status stays 0 (src/dehost_main.cpp:311,513-514)
    }
    if (opt.run_extract) {  // src/dehost_main.cpp:515-536
        if (opt.prefix.empty()) opt.prefix = "charon";
        std::vector<std::string> to_extract;
        if (opt.category_to_extract == "all") to_extract = meta.categories; else to_extract.push_back(opt.category_to_extract);
        // get_extension (src/utils.cpp:126-133): extension of the read file, looking through a trailing .gz
        std::string base = opt.read_file;
        const size_t slash = base.find_last_of('/');
        if (slash != std::string::npos) base = base.substr(slash + 1);
        auto ext_of = [](const std::string &f) { const size_t d = f.find_last_of('.'); return (d == std::string::npos || d == 0) ? std::string() : f.substr(d); };
        std::string extension = ext_of(base);
        if (extension == ".gz") extension = ext_of(base.substr(0, base.size() - 3));
        for (const std::string &category : to_extract) {
            const uint8_t ci = meta.category_index(category);
            if (opt.is_paired) {
                opt.extract_category_to_file[ci].push_back(opt.prefix + "_" + category + "_1" + extension + ".gz");
                opt.extract_category_to_file[ci].push_back(opt.prefix + "_" + category + "_2" + extension + ".gz");
            } else {
                opt.extract_category_to_file[ci].push_back(opt.prefix + "_" + category + extension + ".gz");
            }
        }
    }
    if (opt.classify_mode) {  // src/classify_main.cpp:338-341
        if (opt.dist != "gamma" && opt.dist != "beta") {
            g_log.error("Supported distributions are [gamma , beta]");
            return false;
        }
    } else if (opt.dist != "gamma" && opt.dist != "beta" && opt.dist != "kde") {  // src/dehost_main.cpp:538-541
        g_log.error("Supported distributions are [gamma , beta, kde]");
        return false;
    }
    return true;
}

// The index file and what is made of it on the devices.  Built in three steps, as the run's messages come: the constructor reads the
// file's head and starts the select-block check; settle_outputs() (above) may still refuse the run; load() puts the index into HBM,
// replicates it, and creates one stream per replica with the options' model on stream 0.
// The destructor is what every way out of dehost_main passes: the streams of replicas 1.. are destroyed (they wait for their batches),
// then those replicas' indexes, then the select check is waited for.  Stream 0 and index 0 are destroyed by destroy_first() alone, at
// the end of a run that succeeded -- the tear-down its timing line measures; a run that fails exits with them.
class DeviceSetup {
public:
    IndexFile file;
    const IndexMeta &meta;
    uint8_t host_index;
    std::vector<int> devices;          // one index replica per entry; replica 0 is the index decoded from the file, the others device copies
    std::vector<chn_index *> index;    // per replica
    std::vector<chn_stream *> stream;  // per replica
    chn_model model;
    double t_meta = 0, t_hip = 0, t_sc0 = 0, t_ready = 0;  // CHARON_TIMING: index file read | device + index created | self-check begins | ready

    DeviceSetup(const DehostArguments &opt) : file(opt.db), meta(file.meta), host_index(file.meta.host_category_index()) {
        g_log.info("Loading index from file " + opt.db);
        // The two select blocks behind m_high are checked (a pass over m_high and over the blocks) WHILE the device is set up and the vector
        // decoded: decoding does not need them.  The check is over, and has thrown if it had to, before the first read is classified.
        if (file.has_select_blocks()) {
            IndexFile *f = &file;
            std::exception_ptr *failure = &select_failure_;
            const int threads = g_reader_threads;
            select_check_ = std::thread([f, failure, threads]() {
                try { f->verify_select_blocks(threads); } catch (...) { *failure = std::current_exception(); }
            });
        } else {
            g_log.info("index file ends behind m_high (written by an earlier build of this program: upstream charon expects two select blocks there)");
        }
        if (opt.classify_mode) {
            if (host_index == 255) host_index = 0;  // classify never asks for the host category (src/classify_main.cpp:303-345)
        } else {
            if (host_index == 255) {
                g_log.error("Index does not contain 'host' or 'human' as a category ");
                join_select_check();
                throw std::runtime_error("index does not contain 'host' or 'human' as a category");  // assert in the reference (include/index.hpp:76-78)
            }
            g_log.info("Found host at index " + std::to_string(host_index) + " in the index categories");
        }
    }
    DeviceSetup(const DeviceSetup &) = delete;
    DeviceSetup &operator=(const DeviceSetup &) = delete;
    ~DeviceSetup() {
        for (size_t r = 1; r < stream.size(); ++r) chn_stream_destroy(stream[r]);
        for (size_t r = 1; r < index.size(); ++r) chn_index_destroy(index[r]);
        join_select_check();
    }
    void destroy_first() {
        chn_stream_destroy(stream[0]);
        chn_index_destroy(index[0]);
    }

    // `warm` brings the HIP runtime up meanwhile: waited for before the first device call.  resident: the device-resident loop will run.
    void load(const DehostArguments &opt, std::thread &warm, bool resident) {
        chn_index_desc d = index_desc(opt);
        t_meta = now();
        warm.join();
        choose_devices(opt, resident);
        d.device = devices[0];
        const size_t n_rep = devices.size();
        index.assign(n_rep, nullptr);
        stream.assign(n_rep, nullptr);
        CHN_CHECK(chn_index_create(&d, &index[0]));
        t_hip = now();
        {
            uint64_t slice = 0;  // test hook: words of m_high per decode slice (default: some 64 MB of staging per buffer)
            if (const char *e = std::getenv("CHARON_INDEX_SLICE")) slice = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
            file.decode_on_device(index[0], g_reader_threads, slice);
        }
        if (select_check_.joinable()) {
            select_check_.join();
            if (select_failure_) std::rethrow_exception(select_failure_);
            g_log.info("self-check: the sd_vector's two select_support_mcl blocks answer select exactly as m_high does");
        }
        g_log.info("Index loaded");
        check_bin_fill();
        // the other replicas: queued device copies of replica 0, each checked against the set bits per bin the loader counted
        for (size_t r = 1; r < n_rep; ++r) CHN_CHECK(chn_index_replicate(index[0], devices[r], &index[r]));
        for (size_t r = 1; r < n_rep; ++r) {
            std::vector<uint64_t> bits(meta.technical_bins, 0);
            CHN_CHECK(chn_index_bin_popcounts(index[r], bits.data()));
            if (bits != file.bits_per_bin)
                throw std::runtime_error("replica " + std::to_string(r) + " (device " + std::to_string(devices[r]) + "): its set bits per bin differ from the decoded index");
        }
        chn_stream_cfg cfg = abi_struct<chn_stream_cfg>();
        cfg.max_reads = opt.batch_reads; cfg.max_bases = opt.batch_bases;
        for (size_t r = 0; r < n_rep; ++r) CHN_CHECK(chn_stream_create(index[r], &cfg, &stream[r]));
        // call_category for paired dehost and for every classify run (include/read_entry.hpp:281-285), call_host otherwise
        CHN_CHECK(chn_model_default(&model, d.num_categories, host_index, (opt.is_paired || opt.classify_mode) ? 1 : 0));
        model.host_index = opt.classify_mode ? 0 : host_index;
        model.min_quality = opt.min_quality; model.min_length = opt.min_length; model.min_compression = opt.min_compression;
        model.confidence_threshold = (int8_t)opt.confidence_threshold;  // narrowing as in StatsModel (include/classify_stats.hpp:404,497)
        model.confidence_probability_threshold = opt.confidence_probability_threshold;
        model.host_unique_prop_lo_threshold = opt.host_unique_prop_lo_threshold;
        model.min_proportion_difference = opt.min_proportion_difference; model.min_prob_difference = opt.min_prob_difference;
        model.min_hits = opt.min_hits;
        CHN_CHECK(chn_model_set(stream[0], &model));
        t_sc0 = now();
        self_check_reference_files(meta, stream[0], opt);
        t_ready = now();
    }

private:
    std::exception_ptr select_failure_;
    std::thread select_check_;

    void join_select_check() { if (select_check_.joinable()) select_check_.join(); }
    chn_index_desc index_desc(const DehostArguments &opt) const {
        chn_index_desc d = abi_struct<chn_index_desc>();
        d.device = opt.device;
        d.kmer_size = meta.kmer_size; d.window_size = meta.window_size; d.hash_funs = (uint8_t)meta.hash_funs;
        d.num_categories = (uint8_t)meta.categories.size(); d.host_index = host_index;
        d.minimiser_seed = 0x8F3F73B5CF1C9ADEULL;
        d.bins = meta.bins; d.technical_bins = meta.technical_bins; d.bin_size = meta.bin_size; d.hash_shift = meta.hash_shift; d.bin_words = meta.bin_words;
        for (uint64_t b = 0; b < meta.bins; ++b) d.bin_to_category[b] = meta.category_index(meta.bin_to_category.at((uint8_t)b));
        return d;
    }
    // CHARON_DEVICES: the list, checked against the devices there are
    void choose_devices(const DehostArguments &opt, bool resident) {
        devices.assign(1, opt.device);
        if (opt.devices_all || !opt.devices.empty()) {
            int count = 0;
            CHN_CHECK(chn_device_count(&count));
            if (opt.devices_all) {
                devices.clear();
                for (int i = 0; i < count && i < 64; ++i) devices.push_back(i);
                if (devices.empty()) throw std::runtime_error("CHARON_DEVICES=all: no device is visible");
            } else {
                devices = opt.devices;
                for (int dv : devices)
                    if (dv >= count) throw std::runtime_error("CHARON_DEVICES: device " + std::to_string(dv) + " is not below the device count " + std::to_string(count));
            }
            if (resident && devices.size() > 1) throw std::runtime_error("CHARON_GPU_TEXT: cannot be set together with CHARON_DEVICES=all on several devices (the text lives on one device)");
        }
        std::string list;
        for (int dv : devices) list += (list.empty() ? "" : ",") + std::to_string(dv);
        g_log.info("replicas: " + std::to_string(devices.size()) + " (devices " + list + ")");
    }
    // loader self-check (iv), SURVEY 8(c): a bin that received n distinct values through h hash functions should have
    // about S * (1 - exp(-h n / S)) set bits.  Reported, never fatal (hashes_per_bin counts are what `charon index` stored).
    void check_bin_fill() const {
        for (uint64_t b = 0; b < meta.bins; ++b) {
            auto it = meta.hashes_per_bin.find((uint8_t)b);
            if (it == meta.hashes_per_bin.end() || it->second == 0) continue;
            const double expect = (double)meta.bin_size * (1.0 - std::exp(-(double)meta.hash_funs * (double)it->second / (double)meta.bin_size));
            const double got = (double)file.bits_per_bin[b];
            if (std::fabs(got - expect) > 0.02 * expect + 64)
                g_log.warn("self-check: bin " + std::to_string(b) + " has " + std::to_string((uint64_t)got) + " set bits, expected about " +
                           std::to_string((uint64_t)expect) + " for its " + std::to_string(it->second) + " hashes");
        }
    }
};
