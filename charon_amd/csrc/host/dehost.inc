// dehost.inc -- reference-file self-check, dehost_main (src/dehost_main.cpp:314-550)
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a
// stand-alone header.

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
            chn_batch bt;
            std::memset(&bt, 0, sizeof bt);
            bt.struct_size = sizeof bt; bt.n_reads = n; bt.n_bases = hb.n_bases; bt.bases2 = hb.bases.data();
            bt.nmask = hb.any_n ? hb.nmask.data() : nullptr; bt.seg1_offset = hb.off1.data(); bt.seg1_length = hb.len1.data();
            CHN_CHECK(chn_batch_submit(stream, &bt));
            const size_t C = meta.categories.size();
            std::vector<uint32_t> nh(n), cnt(n * C), unq(n * C);
            chn_result rs;
            std::memset(&rs, 0, sizeof rs);
            rs.struct_size = sizeof rs; rs.num_hashes = nh.data(); rs.counts = cnt.data(); rs.unique_counts = unq.data();
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

// The ids of a pair differ after dropping their last characters (src/dehost_main.cpp:423-430): the two ids behind the rows printed so
// far, and the end the reference's uncaught exception gives.  The caller has drained whatever still had rows to print.
[[noreturn]] void pairs_do_not_match(const char *id1, size_t len1, const char *id2, size_t len2) {
    std::cout.flush();
    std::cout << std::string(id1, len1) << " " << std::string(id2, len2);
    std::cout.flush();
    std::fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n  what():  Your pairs don't match for read ids.\n");
    std::abort();
}

// CHARON_TIMING=1: one line to the log and, behind "charon: ", to stderr
__attribute__((format(printf, 1, 2))) void timing_line(const char *fmt, ...) {
    char tb[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(tb, sizeof tb, fmt, ap);
    va_end(ap);
    g_log.info(tb);
    std::fprintf(stderr, "charon: %s\n", tb);
}

int dehost_main(DehostArguments &opt) {
    const double t_entry = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    g_log.open(opt.log_file, opt.verbosity);
    g_reader_threads = reader_threads_for(opt.threads, looks_compressed(opt.read_file) || (!opt.read_file2.empty() && looks_compressed(opt.read_file2)));
    if (!ends_with(opt.db, ".idx")) opt.db += ".idx";                 // src/dehost_main.cpp:489-491
    if (!opt.read_file2.empty()) { opt.is_paired = true; opt.min_length = 80; }  // :493-496
    g_log.info(std::string(opt.classify_mode ? "Running charon classify\n\nCharon version: " : "Running charon dehost\n\nCharon version: ") + CHARON_VERSION);
    if (std::getenv("CHARON_ZLIB_ONLY")) g_gzip_emulator = false;
    else if (!gzip_emulator_self_check()) {
        g_gzip_emulator = false;
        g_log.warn(std::string("gzip size emulator disagrees with the linked zlib ") + zlibVersion() + "; using zlib for the compression column");
    }

    // CHARON_TEXT_BATCHES=1: slabs are page-locked from the first one on (the reader thread below allocates them); those left in the pool
    // are released when this function is left, after everything that hands slabs back, while the HIP runtime is certainly still up
    g_pin_slabs = opt.text_batches || g_gpu_inflate;  // (CHARON_GPU_INFLATE=1 downloads straight into the slab)
    struct SlabPoolDrain { ~SlabPoolDrain() { std::lock_guard<std::mutex> lk(g_slab_pool.m); g_slab_pool.v.clear(); } } slab_pool_drain;
    struct DevTextPoolDrain { ~DevTextPoolDrain() { g_dev_text_pool.drain(); } } dev_text_pool_drain;  // (CHARON_GPU_TEXT=1) likewise
    if (g_gpu_inflate) g_log.info("CHARON_GPU_INFLATE=1: BGZF members are inflated on device " + std::to_string(g_gpu_inflate_device) + " (size and CRC-32 are checked on the device)");
    if (g_gpu_inflate_stream) {  // one line per input file: on (and where), or why not; the kind of input is what a reader makes of the file
        for (const std::string &f : {opt.read_file, opt.read_file2}) {
            if (f.empty()) continue;
            std::string why;
            try { why = BlockReader(f).gpu_inflate_stream_note(); } catch (std::exception &) { continue; }  // (the reader thread reports what is wrong with it)
            if (why.empty()) g_log.info("CHARON_GPU_INFLATE_STREAM=1: the chunks of the one-stream .gz are inflated on device " + std::to_string(g_gpu_inflate_stream_device) + " (chn_inflate_stream_run; block starts are searched on the reader's threads)");
            else g_log.info("CHARON_GPU_INFLATE_STREAM=1 does not apply: " + why);
        }
    }
    if (g_gpu_deflate) g_log.info("CHARON_GPU_DEFLATE=1: extract files are compressed on device " + std::to_string(g_gpu_deflate_device) + " (BGZF members of 65280 bytes)");
    if (opt.text_batches) g_log.info("CHARON_TEXT_BATCHES=1: reads go to the device as text (letters -> codes and mean quality on the GPU)");
    // reader thread: parses whole-record blocks while the previous batch is packed / compressed / classified / printed.  It starts
    // before the device is touched, so the first block is parsed while the HIP runtime initialises and the index is decoded.
    BlockQueue queue;
    // the readers outlive the reader thread: records of a mapped file are views into the mapping until their rows are printed
    std::unique_ptr<BlockReader> in1p, in2;
    // CHARON_GPU_TEXT=1: while the run is device-resident, each of its `n_sides` files (one, or with CHARON_GPU_TEXT_PAIRS=1 the two of
    // a pair) has a reader thread and a queue of its own (side_reader / side_queue), each with its own BlockReader, hence its own
    // BgzfSource and inflate handle, which hand over blocks of text in device memory.  The host reader (reader_body) is then started
    // only when the main thread leaves the mode: from `resume_z` of either compressed file with `resume_carry` in front.
    // A device block is 64 MiB of text (a thousand members per chn_inflate_run: four wavefronts for each of the device's 256 CUs, and
    // some 13 000 reads of 5 kb per chn_text_split) instead of the 256 MB of a slab.  Device buffers: each reader fills one while two
    // wait in its queue, the main thread holds one per side and up to two batches in flight refer to one per side -- at most seven
    // exist per side; of a pair's fourteen, eight free ones are kept.
    int n_sides = 0;
    bool resumed[2] = {false, false};
    size_t resume_z[2] = {0, 0};
    Slab resume_carry[2];
    BlockQueue side_queue[2];
    std::thread side_reader[2];
    // (CHARON_GPU_TEXT_BLOCK: test hook, a smaller block -- down to one BGZF member's 64 KiB)
    size_t resident_block_bytes = std::min<size_t>((size_t)std::min<uint64_t>(256ULL << 20, std::max<uint64_t>(1 << 20, opt.batch_bases)), (size_t)64 << 20);
    if (const char *e = std::getenv("CHARON_GPU_TEXT_BLOCK")) resident_block_bytes = (size_t)std::min<unsigned long long>(resident_block_bytes, std::max<unsigned long long>(65536, std::strtoull(e, nullptr, 10)));
    auto side_reader_body = [&](int k) {
        BlockQueue &q = side_queue[k];
        try {
            BlockReader in(k ? opt.read_file2 : opt.read_file);
            const size_t block_bytes = resident_block_bytes;
            for (;;) {
                std::shared_ptr<HostBatch> hb(new HostBatch());
                hb->dtext = in.next_device(block_bytes, g_gpu_text_headroom);
                if (!hb->dtext) break;
                if (!q.push(std::move(hb))) return;
            }
            q.finish("");
        } catch (std::exception &e) {
            q.finish(e.what());
        }
    };
    auto reader_body = [&]() {
        try {
            in1p.reset(new BlockReader(opt.read_file));
            BlockReader &in1 = *in1p;
            if (opt.is_paired) in2.reset(new BlockReader(opt.read_file2));
            const size_t max_bytes = (size_t)std::min<uint64_t>(256ULL << 20, std::max<uint64_t>(1 << 20, opt.batch_bases));
            if (resumed[0]) in1.resume(resume_z[0], resume_carry[0]);
            if (resumed[1]) in2->resume(resume_z[1], resume_carry[1]);
            for (;;) {
                std::shared_ptr<HostBatch> hb(new HostBatch());
                // a batch may hold at most batch_bases padded bases: bound the record count by the byte budget as well
                if (!in1.next(hb->blk1, opt.batch_reads, max_bytes)) break;
                if (opt.is_paired) {
                    // the second file is simply `take`n in step with the first (src/dehost_main.cpp:413-415)
                    if (!in2->next(hb->blk2, hb->blk1.recs.size(), max_bytes)) break;
                    while (hb->blk2.recs.size() < hb->blk1.recs.size()) {
                        // the byte budget cut the mate block short: read further mate blocks until the counts agree
                        RawBlock more;
                        if (!in2->next(more, hb->blk1.recs.size() - hb->blk2.recs.size(), max_bytes)) break;
                        // moving a vector keeps its heap buffer, so the views into `more.buf` stay valid
                        hb->blk2.recs.insert(hb->blk2.recs.end(), more.recs.begin(), more.recs.end());
                        if (more.map_begin && hb->blk2.map_begin) hb->blk2.map_len = (size_t)(more.map_begin + more.map_len - hb->blk2.map_begin);
                        hb->extra.emplace_back(std::move(more.buf));
                    }
                    if (hb->blk2.recs.size() < hb->blk1.recs.size()) hb->blk1.recs.resize(hb->blk2.recs.size());
                }
                if (!queue.push(std::move(hb))) return;
            }
            queue.finish("");
        } catch (std::exception &e) {
            queue.finish(e.what());
        }
    };
    // why CHARON_GPU_TEXT=1 cannot take `f` (empty: it can)
    auto not_resident_because = [](const std::string &f) -> std::string {
        const std::string stem = f.substr(0, f.size() - std::min<size_t>(3, f.size()));
        if (!ends_with(f, ".gz")) return "not a .gz file";
        if (std::getenv("CHARON_NO_BGZF")) return "CHARON_NO_BGZF is set";
        if (!ends_with(stem, ".fastq") && !ends_with(stem, ".fq")) return "not FASTQ";
        if (!BgzfSource().open(f)) return "one deflate stream, not BGZF";
        return "";
    };
    // why CHARON_GPU_TEXT_FASTA=1 cannot take `f` (empty: it can): FASTA by name, as BlockReader decides it
    auto not_resident_fasta_because = [](const std::string &f) -> std::string {
        const std::string stem = f.substr(0, f.size() - std::min<size_t>(3, f.size()));
        if (!ends_with(f, ".gz")) return "not a .gz file";
        if (std::getenv("CHARON_NO_BGZF")) return "CHARON_NO_BGZF is set";
        bool fasta = false;
        for (const char *x : {".fasta", ".fa", ".fna", ".ffn", ".faa", ".frn", ".fas"}) fasta = fasta || ends_with(stem, x);
        if (!fasta) return "not FASTA";
        if (!BgzfSource().open(f)) return "one deflate stream, not BGZF";
        return "";
    };
    bool fasta_side = false;  // CHARON_GPU_TEXT_FASTA=1 took the input: the one side is a FASTA file
    // no side, one (single-end input) or two (CHARON_GPU_TEXT_PAIRS=1 and a pair of files)
    if (g_gpu_text) {
        bool two = false;
        if (g_gpu_text_pairs && !opt.is_paired)
            g_log.info("CHARON_GPU_TEXT_PAIRS=1 does not apply to " + opt.read_file + " (single-end input): CHARON_GPU_TEXT=1 alone decides");
        if (g_gpu_text_pairs && opt.is_paired) {
            std::string why = not_resident_because(opt.read_file), file = opt.read_file;
            if (why.empty()) { why = not_resident_because(opt.read_file2); file = opt.read_file2; }
            two = why.empty();
            if (!two) g_log.info("CHARON_GPU_TEXT_PAIRS=1 does not apply to " + file + " (" + why + "; both files must be BGZF FASTQ): the run goes on without it");
        }
        std::string why = two ? "" : opt.is_paired ? "paired input" : not_resident_because(opt.read_file);
        if (g_gpu_text_fasta) {
            const std::string fwhy = opt.is_paired ? "paired input" : not_resident_fasta_because(opt.read_file);
            fasta_side = fwhy.empty();
            if (fasta_side) why.clear();
            else g_log.info("CHARON_GPU_TEXT_FASTA=1 does not apply to " + opt.read_file + " (" + fwhy + "; single-end BGZF FASTA only): the run goes on as under CHARON_GPU_TEXT=1 alone");
        }
        if (why.empty()) {
            n_sides = two ? 2 : 1;
            if (const char *e = std::getenv("CHARON_GPU_TEXT_HEADROOM")) g_gpu_text_headroom = (size_t)std::min<unsigned long long>(1ULL << 30, std::strtoull(e, nullptr, 10));
            if (two || fasta_side) g_dev_text_pool.keep = 8;
            g_log.info("CHARON_GPU_TEXT=1: BGZF text is inflated into the memory of device " + std::to_string(g_gpu_text_device) +
                       " and stays there (records split and packed on the device; headroom " + std::to_string(g_gpu_text_headroom) + " bytes)");
            if (fasta_side) g_log.info("CHARON_GPU_TEXT_FASTA=1: FASTA records are found and unwrapped on the device (a second buffer per block holds the letters)");
            if (two) g_log.info("CHARON_GPU_TEXT_PAIRS=1: both files of the pair stay in device memory (two texts a batch; the ids of a pair are compared on the device)");
        } else {
            g_log.info("CHARON_GPU_TEXT=1 does not apply to " + opt.read_file + " (" + why + "; single-end BGZF FASTQ only): the run goes on without it");
        }
    }
    if (g_gpu_extract) {
        if (opt.category_to_extract.empty()) {
            g_log.info("CHARON_GPU_EXTRACT=1 does nothing without --extract: the run goes on without it");
            g_gpu_extract = false;
        } else if (!n_sides) {
            g_log.info("CHARON_GPU_EXTRACT=1 does not apply (the input is not taken by the device-resident loop of CHARON_GPU_TEXT=1): the run goes on without it");
            g_gpu_extract = false;
        } else if (fasta_side) {
            g_log.info("CHARON_GPU_EXTRACT=1 does not apply (FASTA input: extract records are formed on the device for FASTQ only): the run goes on without it");
            g_gpu_extract = false;
        } else {
            g_log.info("CHARON_GPU_EXTRACT=1: the records of the extract files are formed and compressed in the memory of device " + std::to_string(g_gpu_text_device));
        }
    }
    std::thread reader;
    for (int k = 0; k < n_sides; ++k) side_reader[k] = std::thread(side_reader_body, k);
    if (!n_sides) reader = std::thread(reader_body);

    struct ReaderJoin {  // whatever way this function is left: stop the reader and wait for it
        BlockQueue &q; std::thread &t;
        ~ReaderJoin() { if (t.joinable()) { q.abort(); t.join(); } }
    } reader_join{queue, reader}, side_reader_join0{side_queue[0], side_reader[0]}, side_reader_join1{side_queue[1], side_reader[1]};
    // the HIP runtime takes 0.1-0.2 s to come up: let it do so while this thread reads the index file
    std::thread warm([]() { void *p = nullptr; if (chn_host_alloc(64, &p) == CHN_OK) chn_host_free(p); });
    struct WarmJoin { std::thread &t; ~WarmJoin() { if (t.joinable()) t.join(); } } warm_join{warm};

    IndexFile file(opt.db);
    const IndexMeta &meta = file.meta;
    g_log.info("Loading index from file " + opt.db);
    // The two select blocks behind m_high are checked (a pass over m_high and over the blocks) WHILE the device is set up and the vector
    // decoded: decoding does not need them.  The check is over, and has thrown if it had to, before the first read is classified.
    std::exception_ptr select_failure;
    std::thread select_check;
    struct SelectJoin { std::thread &t; ~SelectJoin() { if (t.joinable()) t.join(); } } select_join{select_check};
    if (file.has_select_blocks()) {
        select_check = std::thread([&]() {
            try { file.verify_select_blocks(g_reader_threads); } catch (...) { select_failure = std::current_exception(); }
        });
    } else {
        g_log.info("index file ends behind m_high (written by an earlier build of this program: upstream charon expects two select blocks there)");
    }
    uint8_t host_index = meta.host_category_index();
    if (opt.classify_mode) {
        if (host_index == 255) host_index = 0;  // classify never asks for the host category (src/classify_main.cpp:303-345)
    } else {
        if (host_index == 255) {
            g_log.error("Index does not contain 'host' or 'human' as a category ");
            throw std::runtime_error("index does not contain 'host' or 'human' as a category");  // assert in the reference (include/index.hpp:76-78)
        }
        g_log.info("Found host at index " + std::to_string(host_index) + " in the index categories");
    }

    opt.run_extract = !opt.category_to_extract.empty();
    if (opt.run_extract && opt.category_to_extract != "all" &&
        std::find(meta.categories.begin(), meta.categories.end(), opt.category_to_extract) == meta.categories.end()) {
        std::string options;
        for (auto &c : meta.categories) options += c + " ";
        g_log.error("Cannot extract " + opt.category_to_extract + ", please chose one of [ all " + options + "]");
        return 1;  // the reference's callback drops this value: exit status stays 0 (src/dehost_main.cpp:311,513-514)
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
            return 1;
        }
    } else if (opt.dist != "gamma" && opt.dist != "beta" && opt.dist != "kde") {  // src/dehost_main.cpp:538-541
        g_log.error("Supported distributions are [gamma , beta, kde]");
        return 1;
    }

    // index -> HBM
    chn_index_desc d;
    std::memset(&d, 0, sizeof d);
    d.struct_size = sizeof d; d.device = opt.device;
    d.kmer_size = meta.kmer_size; d.window_size = meta.window_size; d.hash_funs = (uint8_t)meta.hash_funs;
    d.num_categories = (uint8_t)meta.categories.size(); d.host_index = host_index;
    d.minimiser_seed = 0x8F3F73B5CF1C9ADEULL;
    d.bins = meta.bins; d.technical_bins = meta.technical_bins; d.bin_size = meta.bin_size; d.hash_shift = meta.hash_shift; d.bin_words = meta.bin_words;
    for (uint64_t b = 0; b < meta.bins; ++b) d.bin_to_category[b] = meta.category_index(meta.bin_to_category.at((uint8_t)b));
    chn_index *index = nullptr;
    const double t_meta = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    warm.join();
    // CHARON_DEVICES: one index replica per entry; replica 0 is the index decoded from the file, the others are device copies of it
    std::vector<int> devices(1, opt.device);
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
        d.device = devices[0];
        if (n_sides && devices.size() > 1) throw std::runtime_error("CHARON_GPU_TEXT: cannot be set together with CHARON_DEVICES=all on several devices (the text lives on one device)");
    }
    {
        std::string list;
        for (int dv : devices) list += (list.empty() ? "" : ",") + std::to_string(dv);
        g_log.info("replicas: " + std::to_string(devices.size()) + " (devices " + list + ")");
    }
    CHN_CHECK(chn_index_create(&d, &index));
    const double t_hip = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    {
        uint64_t slice = 0;  // test hook: words of m_high per decode slice (default: some 64 MB of staging per buffer)
        if (const char *e = std::getenv("CHARON_INDEX_SLICE")) slice = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
        file.decode_on_device(index, g_reader_threads, slice);
    }
    if (select_check.joinable()) {
        select_check.join();
        if (select_failure) std::rethrow_exception(select_failure);
        g_log.info("self-check: the sd_vector's two select_support_mcl blocks answer select exactly as m_high does");
    }
    g_log.info("Index loaded");
    // loader self-check (iv), SURVEY 8(c): a bin that received n distinct values through h hash functions should have
    // about S * (1 - exp(-h n / S)) set bits.  Reported, never fatal (hashes_per_bin counts are what `charon index` stored).
    for (uint64_t b = 0; b < meta.bins; ++b) {
        auto it = meta.hashes_per_bin.find((uint8_t)b);
        if (it == meta.hashes_per_bin.end() || it->second == 0) continue;
        const double expect = (double)meta.bin_size * (1.0 - std::exp(-(double)meta.hash_funs * (double)it->second / (double)meta.bin_size));
        const double got = (double)file.bits_per_bin[b];
        if (std::fabs(got - expect) > 0.02 * expect + 64)
            g_log.warn("self-check: bin " + std::to_string(b) + " has " + std::to_string((uint64_t)got) + " set bits, expected about " +
                       std::to_string((uint64_t)expect) + " for its " + std::to_string(it->second) + " hashes");
    }

    // the other replicas: queued device copies of replica 0, each checked against the set bits per bin the loader counted
    const size_t n_rep = devices.size();
    std::vector<chn_index *> rep_index(n_rep, nullptr);
    std::vector<chn_stream *> rep_stream(n_rep, nullptr);
    struct ReplicaObjects {  // destroyed whatever way this function is left (streams first: they wait for their batches)
        std::vector<chn_index *> &idx; std::vector<chn_stream *> &st;
        ~ReplicaObjects() { for (size_t r = 1; r < st.size(); ++r) chn_stream_destroy(st[r]); for (size_t r = 1; r < idx.size(); ++r) chn_index_destroy(idx[r]); }
    } replica_objects{rep_index, rep_stream};
    rep_index[0] = index;
    for (size_t r = 1; r < n_rep; ++r) CHN_CHECK(chn_index_replicate(index, devices[r], &rep_index[r]));
    for (size_t r = 1; r < n_rep; ++r) {
        std::vector<uint64_t> bits(meta.technical_bins, 0);
        CHN_CHECK(chn_index_bin_popcounts(rep_index[r], bits.data()));
        if (bits != file.bits_per_bin)
            throw std::runtime_error("replica " + std::to_string(r) + " (device " + std::to_string(devices[r]) + "): its set bits per bin differ from the decoded index");
    }

    chn_stream_cfg cfg;
    cfg.struct_size = sizeof cfg; cfg.flags = 0; cfg.max_reads = opt.batch_reads; cfg.max_bases = opt.batch_bases;
    chn_stream *stream = nullptr;
    CHN_CHECK(chn_stream_create(index, &cfg, &stream));
    rep_stream[0] = stream;
    for (size_t r = 1; r < n_rep; ++r) CHN_CHECK(chn_stream_create(rep_index[r], &cfg, &rep_stream[r]));
    chn_model model;
    // call_category for paired dehost and for every classify run (include/read_entry.hpp:281-285), call_host otherwise
    CHN_CHECK(chn_model_default(&model, d.num_categories, host_index, (opt.is_paired || opt.classify_mode) ? 1 : 0));
    model.host_index = opt.classify_mode ? 0 : host_index;
    model.min_quality = opt.min_quality; model.min_length = opt.min_length; model.min_compression = opt.min_compression;
    model.confidence_threshold = (int8_t)opt.confidence_threshold;  // narrowing as in StatsModel (include/classify_stats.hpp:404,497)
    model.confidence_probability_threshold = opt.confidence_probability_threshold;
    model.host_unique_prop_lo_threshold = opt.host_unique_prop_lo_threshold;
    model.min_proportion_difference = opt.min_proportion_difference; model.min_prob_difference = opt.min_prob_difference;
    model.min_hits = opt.min_hits;
    CHN_CHECK(chn_model_set(stream, &model));

    const double t_sc0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    self_check_reference_files(meta, stream, opt);
    const double t_ready = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();

    std::ios::sync_with_stdio(false);
    Result result(meta, opt, stream, model, std::cout);
    result.push_initial_model();
    g_log.info(std::string(opt.classify_mode ? "Classifying file " : "Dehosting file ") + opt.read_file + (opt.is_paired ? " and " + opt.read_file2 : ""));

    const size_t C = meta.categories.size();
#ifdef CHARON_DIAG  // diagnostics build only (make CXXFLAGS_EXTRA=-DCHARON_DIAG): a knob that changes the output has no place in the product binary
    const bool skip_compression = std::getenv("CHARON_SKIP_COMPRESSION") != nullptr;  // NOT reference behaviour: prints 0
    if (skip_compression) g_log.warn("CHARON_SKIP_COMPRESSION set: the compression column is 0 (differs from the reference)");
#else
    const bool skip_compression = false;
#endif

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
    };
    uint64_t gz_on_device = 0, gz_long_on_device = 0;
    std::atomic<uint64_t> text_slab_batches{0}, text_copy_batches{0};  // CHARON_TEXT_BATCHES=1: batches sent as their slab / as a page-locked copy
    // CHARON_TIMING=1: wall seconds per phase of the main thread, to the log (where does the CLI's time go?)
    const bool timing = std::getenv("CHARON_TIMING") != nullptr;
    double t_pop = 0, t_pack = 0, t_submit = 0, t_wait = 0, t_gz = 0, t_rows = 0;
    auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    // the gzip column's deflate pass on the GPU for reads up to CHN_GZIP_MAX_LEN letters (CHARON_GZIP_ON_HOST=1 / CHARON_ZLIB_ONLY=1: all on the host)
    // Long reads run few wavefronts per CU there (five for a 60 kb read, its class arrays in global memory): about what sixteen host threads
    // make of them with the size emulator -- so with that many host threads the longest reads (beyond 40 000 letters) stay on the host, in the
    // packing loop beside the GPU; with fewer threads everything up to the device's limit goes to the GPU (sweep: profiles/r02/cli_long_reads.txt).
    // Reads beyond CHN_GZIP_MAX_LEN are sized by the device's long-read pass (CHN_GZIP_SIZES_ALL) where gzip_long_device_limit says
    // it pays; CHARON_GZIP_GPU_MAX sets one length limit for everything instead (61440: every longer read on the host).
    uint32_t gz_gpu_max = (std::getenv("CHARON_GZIP_ON_HOST") || std::getenv("CHARON_ZLIB_ONLY") || !g_gzip_emulator) ? 0u : (opt.threads >= 12 ? 40000u : CHN_GZIP_MAX_LEN);
    bool gz_route_long = gz_gpu_max != 0;
    if (gz_gpu_max)
        if (const char *e = std::getenv("CHARON_GZIP_GPU_MAX")) {
            gz_gpu_max = (uint32_t)std::min<unsigned long long>(CHN_GZIP_ANY_LEN, std::max<unsigned long long>(1, std::strtoull(e, nullptr, 10)));
            gz_route_long = false;
        }
    std::vector<Entry> entries;
    // (rows are FORMATTED by the reader's team as well -- -t, but never fewer than four: text out is the mirror of text in; the reference prints inside its
    //  critical section whatever -t is.  With the default -t 1 the main thread formatted rows for 1.0 of a 2.3 s read loop on 4 M reads.)
    std::vector<std::string> rowbuf((size_t)std::max<int>(1, std::max<int>((int)opt.threads, g_reader_threads)));
    std::string failure;

    // chn_batch_wait + rows.  Fast path (models final, nothing to extract -- i.e. every plain `charon dehost` run after its
    // first read): rows are formatted in parallel straight from the result arrays into one buffer per thread and emitted in
    // order; no per-read objects.  Otherwise the reference's add_read state machine, read by read.
    auto finish_wait = [&](Flight &fl, chn_stream *st, double &acc_wait) {
        HostBatch &sub = fl.sub;
        std::vector<uint32_t> &nh = fl.nh, &cnt = fl.cnt, &unq = fl.unq, &gz_sizes = fl.gz_sizes;
        std::vector<double> &prob = fl.prob;
        std::vector<uint8_t> &call = fl.call, &conf = fl.conf, &flags = fl.flags;
        const size_t n = sub.keep.size();
        nh.resize(n); cnt.resize(n * C); unq.resize(n * C); prob.resize(n * C); call.resize(n); conf.resize(n); flags.resize(n);
        chn_result rs;
        std::memset(&rs, 0, sizeof rs);
        rs.struct_size = sizeof rs; rs.on_device = 0;
        rs.num_hashes = nh.data(); rs.counts = cnt.data(); rs.unique_counts = unq.data(); rs.probabilities = prob.data();
        rs.call = call.data(); rs.confidence = conf.data(); rs.flags = flags.data();
        const bool tallied = sub.gz_gpu_len != 0;
        if (tallied) { gz_sizes.resize(n); rs.gzip_sizes = gz_sizes.data(); }
        double tt = now();
        if (opt.text_batches || fl.resident) {  // the mean-quality column comes back with the results
            chn_text_result tr;
            std::memset(&tr, 0, sizeof tr);
            tr.struct_size = sizeof tr; tr.mean_quality = sub.mq.data();
            CHN_CHECK(chn_text_wait(st, &rs, &tr));
            sub.any_n = tr.has_n != 0;
        } else {
            CHN_CHECK(chn_batch_wait(st, &rs));
        }
        acc_wait += now() - tt;
    };
    auto finish_rows = [&](Flight &fl) {
        HostBatch &sub = fl.sub;
        std::vector<uint32_t> &nh = fl.nh, &cnt = fl.cnt, &unq = fl.unq, &gz_sizes = fl.gz_sizes;
        std::vector<double> &prob = fl.prob;
        std::vector<uint8_t> &call = fl.call, &conf = fl.conf;
        const size_t n = sub.keep.size();
        const bool tallied = sub.gz_gpu_len != 0;
        double tt = now();
        struct Lap { double &acc; double t0; std::function<double()> clk; ~Lap() { acc += clk() - t0; } } lap_rows{t_rows, 0, now};
        if (tallied) {
            // the gzip column from the device's deflate tallies (exact: _tr_flush_block's arithmetic on the same frequencies), the host
            // emulator / zlib for the reads the device left out; then the compression gate the call kernel left open
            // (include/read_entry.hpp:189-191,250-252: no call below min_compression; the confidence score is unaffected)
#pragma omp parallel num_threads(opt.threads)
            {
                Deflater defl;
#pragma omp for schedule(dynamic, 64)
                for (long i = 0; i < (long)n; ++i) {
                    const uint64_t L = (uint64_t)sub.len1[i] + (opt.is_paired ? sub.len2[i] : 0);
                    if (sub.gz_pending[i]) {
                        if (gz_sizes[i] != 0) {
                            sub.comp[i] = static_cast<float>(static_cast<double>(gz_sizes[i]) / static_cast<double>(L));
                            if (L <= CHN_GZIP_MAX_LEN) {
#pragma omp atomic
                                gz_on_device += 1;
                            } else {
#pragma omp atomic
                                gz_long_on_device += 1;
                            }
                        } else {
                            sub.comp[i] = defl.ratio(sub.blk1.recs[sub.keep[i]], opt.is_paired ? &sub.blk2.recs[sub.keep[i]] : nullptr);
                        }
                    }
                    if (sub.comp[i] < opt.min_compression) call[i] = 255;
                }
            }
            t_gz += now() - tt;
        }
        lap_rows.t0 = now();
        const uint32_t version = fl.version;
        auto make_entry = [&](size_t i, Entry &e) {
            const RecView &a = sub.blk1.recs[sub.keep[i]];
            e.read_id = first_token(a.id, a.id_len);
            e.length = sub.len1[i] + (opt.is_paired ? sub.len2[i] : 0u);
            e.num_hashes = nh[i]; e.mean_quality = sub.mq[i]; e.compression = sub.comp[i];
            e.counts.assign(cnt.begin() + i * C, cnt.begin() + (i + 1) * C);
            e.unique.assign(unq.begin() + i * C, unq.begin() + (i + 1) * C);
            e.prob.assign(prob.begin() + i * C, prob.begin() + (i + 1) * C);
            e.call = call[i]; e.conf = conf[i]; e.model_version = version; e.row_version = version;
            format_row(meta, e, e.row);
            if (fl.device_records) {
                e.rec_index = (uint32_t)i;  // Result::extract notes the index; the letters stay on the device
            } else if (opt.run_extract) {
                e.rec_id.assign(a.id, a.id_len); e.rec_seq.assign(a.seq, a.seq_len); e.rec_qual.assign(a.qual ? a.qual : "", a.qual_len);
                if (opt.is_paired) {
                    const RecView &b = sub.blk2.recs[sub.keep[i]];
                    e.rec2_id.assign(b.id, b.id_len); e.rec2_seq.assign(b.seq, b.seq_len); e.rec2_qual.assign(b.qual ? b.qual : "", b.qual_len);
                }
            }
        };
        size_t i0 = 0;
        if (!opt.run_extract) {
            // until the models are final (the first read of a run, which the reference drops: include/result.hpp:139-151) go read by read
            while (i0 < n && !result.models_final()) {
                Entry e;
                make_entry(i0, e);
                result.add_read(e);
                ++i0;
            }
            if (i0 == n) return;
            if (result.current_model_version() != version) {
                // the models changed while this batch was on the device (gamma: force_ready moves the neg distribution's location,
                // include/classify_stats.hpp:306-312): bring the rest of the batch up to date in one device call
                std::vector<uint32_t> lens(n - i0);
                for (size_t i = i0; i < n; ++i) lens[i - i0] = sub.len1[i] + (opt.is_paired ? sub.len2[i] : 0u);
                result.reclassify_raw(n - i0, nh.data() + i0, cnt.data() + i0 * C, unq.data() + i0 * C, lens.data(), sub.mq.data() + i0, sub.comp.data() + i0,
                                      prob.data() + i0 * C, call.data() + i0, conf.data() + i0);
            }
            const int T = (int)rowbuf.size();
            std::vector<std::vector<uint64_t>> per_call((size_t)T, std::vector<uint64_t>(C + 1, 0));
#pragma omp parallel num_threads(T)
            {
#ifdef _OPENMP
                const int tid = omp_get_thread_num(), nt = omp_get_num_threads();
#else
                const int tid = 0, nt = 1;
#endif
                const size_t span = n - i0, lo = i0 + span * (size_t)tid / (size_t)nt, hi = i0 + span * (size_t)(tid + 1) / (size_t)nt;
                std::string &out = rowbuf[(size_t)tid];
                out.clear();
                for (size_t i = lo; i < hi; ++i) {
                    const RecView &a = sub.blk1.recs[sub.keep[i]];
                    const void *sp = std::memchr(a.id, ' ', a.id_len);  // read_id = id up to the first space (src/dehost_main.cpp:345)
                    const size_t idn = sp ? (size_t)(static_cast<const char *>(sp) - a.id) : (size_t)a.id_len;
                    format_row_raw(meta, a.id, idn, call[i], sub.len1[i] + (opt.is_paired ? sub.len2[i] : 0u), nh[i], sub.mq[i], conf[i], sub.comp[i],
                                   cnt.data() + i * C, unq.data() + i * C, prob.data() + i * C, out);
                    per_call[(size_t)tid][call[i] < 255 ? call[i] : C] += 1;
                }
            }
            for (int t = 0; t < T; ++t) result.bulk(rowbuf[(size_t)t], per_call[(size_t)t]);
            return;
        }
        // --extract: build the entries and format their rows in parallel ...
        entries.assign(n, Entry());
#pragma omp parallel for num_threads(opt.threads) schedule(static)
        for (long i = 0; i < (long)n; ++i) make_entry((size_t)i, entries[(size_t)i]);
        // ... then critical(add_read_to_results): serial, in input order (what the reference does at -t 1).  When a model finishes
        // training in the middle of the batch, the rest of the batch is brought up to date in one device call.
        if (fl.device_records) result.begin_device_records();
        for (size_t i = 0; i < n; ++i) {
            if (result.models_final() && entries[i].model_version != result.current_model_version()) result.refresh(entries, i);
            result.add_read(entries[i]);
        }
        if (fl.device_records) {
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
            struct LetGo { HostBatch &s; ~LetGo() { s.dtext.reset(); s.dtext2.reset(); } } let_go{sub};  // the blocks' buffers, once the calls have returned
            result.append_device_records(dr);
        }
    };

    // Flight objects go round (their vectors keep their capacity: no fresh pages per batch)
    std::vector<std::unique_ptr<Flight>> flight_pool;
    std::mutex pool_m;
    auto recycle = [&](std::unique_ptr<Flight> &f) {
        f->parent.reset();
        f->parent2.reset();
        f->device_records = false;
        std::lock_guard<std::mutex> lk(pool_m);
        flight_pool.push_back(std::move(f));
    };
    auto take_flight = [&]() {
        std::unique_ptr<Flight> fl;
        {
            std::lock_guard<std::mutex> lk(pool_m);
            if (!flight_pool.empty()) { fl = std::move(flight_pool.back()); flight_pool.pop_back(); }
        }
        if (!fl) fl.reset(new Flight());
        return fl;
    };
    // The end of the GPU batch that starts at record `begin` of `limit`: at most batch_reads records and batch_bases padded bases, the
    // stream's capacity (need_of(i): the padded bases of record i, both mates of a pair)
    auto cut_batch = [&](size_t begin, size_t limit, auto need_of) -> size_t {
        uint64_t bases = 0;
        size_t end = begin;
        while (end < limit && end - begin < opt.batch_reads) {
            const uint64_t need = need_of(end);
            if (need > opt.batch_bases) throw std::runtime_error("a read is longer than CHARON_BATCH_BASES");
            if (bases + need > opt.batch_bases) break;
            bases += need; ++end;
        }
        return end;
    };
    // The rows of a batch are formatted and written by a thread of their own once the models are final and nothing is extracted (every plain
    // `charon dehost` run after its first read): the main thread packs and submits batch i + 1 meanwhile -- with the default -t 1 it used to
    // alternate between packing (1.2 s of a 2.1 s loop on 4 M reads) and rows (0.8 s).  Batches go through in order; at most two wait.
    // (with as many -t threads as the process has CPUs the reader's, the packing and the formatting teams already take every core: one more stage
    //  beside them only adds contention -- -t 16 on a 16-CPU share: 1.67 instead of 1.89 M reads/s.  CHARON_ROW_WRITER=0 / 1 overrides.)
    bool use_row_writer = 2 * (int)opt.threads <= usable_cpus();
    if (const char *e = std::getenv("CHARON_ROW_WRITER")) use_row_writer = std::atoi(e) != 0;
    struct RowWriter {
        std::mutex m;
        std::condition_variable cv;
        std::deque<std::unique_ptr<Flight>> q;
        bool busy = false, stop = false;
        std::string error;
        std::thread t;
    } writer;
    auto writer_drain = [&]() {  // everything handed over has been written (or has failed)
        std::unique_lock<std::mutex> lk(writer.m);
        writer.cv.wait(lk, [&] { return (writer.q.empty() && !writer.busy) || !writer.error.empty(); });
        if (!writer.error.empty()) throw std::runtime_error(writer.error);
    };
    auto writer_body = [&]() {
        for (;;) {
            std::unique_ptr<Flight> f;
            {
                std::unique_lock<std::mutex> lk(writer.m);
                writer.cv.wait(lk, [&] { return !writer.q.empty() || writer.stop; });
                if (writer.q.empty()) return;
                f = std::move(writer.q.front());
                writer.q.pop_front();
                writer.busy = true;
                writer.cv.notify_all();
            }
            std::string err;
            try { finish_rows(*f); } catch (std::exception &e) { err = e.what(); }
            recycle(f);
            std::lock_guard<std::mutex> lk(writer.m);
            writer.busy = false;
            if (!err.empty() && writer.error.empty()) writer.error = err;
            writer.cv.notify_all();
            if (!err.empty()) return;
        }
    };
    struct WriterJoin {
        RowWriter &w;
        ~WriterJoin() {
            { std::lock_guard<std::mutex> lk(w.m); w.stop = true; w.cv.notify_all(); }
            if (w.t.joinable()) w.t.join();
        }
    } writer_join{writer};
    // a waited flight on to its rows: the row writer's queue, or here behind everything handed over before
    auto hand_on = [&](std::unique_ptr<Flight> &f) {
        const bool hand_over = use_row_writer && !opt.run_extract && result.models_final() && result.current_model_version() == f->version;
        if (!hand_over) {  // the reference's read-by-read state machine: here, behind everything handed over before
            if (writer.t.joinable()) writer_drain();
            finish_rows(*f);
            recycle(f);
            return;
        }
        if (!writer.t.joinable()) writer.t = std::thread(writer_body);
        std::unique_lock<std::mutex> lk(writer.m);
        writer.cv.wait(lk, [&] { return writer.q.size() < 2 || !writer.error.empty(); });
        if (!writer.error.empty()) throw std::runtime_error(writer.error);
        writer.q.push_back(std::move(f));
        writer.cv.notify_all();
    };
    auto retire = [&](std::unique_ptr<Flight> &f) {
        finish_wait(*f, stream, t_wait);
        hand_on(f);
    };
    auto fill_batch = [&](Flight &fl, chn_batch &bt) {
        HostBatch &sub = fl.sub;
        std::memset(&bt, 0, sizeof bt);
        bt.struct_size = sizeof bt; bt.on_device = 0; bt.n_reads = sub.keep.size(); bt.n_bases = sub.n_bases;
        bt.bases2 = sub.bases.data(); bt.nmask = sub.any_n ? sub.nmask.data() : nullptr;
        bt.seg1_offset = sub.off1.data(); bt.seg1_length = sub.len1.data();
        bt.seg2_offset = opt.is_paired ? sub.off2.data() : nullptr; bt.seg2_length = opt.is_paired ? sub.len2.data() : nullptr;
        bt.mean_quality = sub.mq.data(); bt.compression = sub.comp.data();
        bt.gzip_tallies = sub.gz_gpu_len;  // > 0: the call kernel leaves the compression gate to finish()
        // deflate pass and tree arithmetic on the device: four bytes per read come back (reads beyond CHN_GZIP_MAX_LEN: the long-read pass)
        bt.gzip_output = sub.gz_gpu_len > CHN_GZIP_MAX_LEN ? CHN_GZIP_SIZES_ALL : CHN_GZIP_SIZES;
    };

    // a packed batch through chn_batch_submit, or (CHARON_TEXT_BATCHES=1) the text itself through chn_text_submit
    auto submit_flight = [&](chn_stream *st, Flight &fl) {
        if (!opt.text_batches && !fl.resident) {
            chn_batch bt;
            fill_batch(fl, bt);
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
        tb.gzip_output = sub.gz_gpu_len > CHN_GZIP_MAX_LEN ? CHN_GZIP_SIZES_ALL : CHN_GZIP_SIZES;
        if (fl.resident) { tb.flags = CHN_TEXT_ON_DEVICE; tb.text = sub.dtext->buf; tb.text_bytes = sub.dtext->text_bytes; }
        if (fl.resident && sub.dtext2) { tb.struct_size = sizeof tb2; tb2.text2 = sub.dtext2->buf; tb2.text2_bytes = sub.dtext2->text_bytes; }
        else (sub.text_from_slab ? text_slab_batches : text_copy_batches) += 1;
        const int rc = chn_text_submit(st, &tb);
        // (the device met a byte that is no IUPAC nucleotide letter: what HostBatch::pack reports for a packed batch)
        if (rc == CHN_E_INVALID && std::strstr(chn_last_error(), "illegal byte"))
            throw InputError("parse error: illegal character in a sequence (only IUPAC nucleotide letters are accepted)");
        if (rc != CHN_OK) throw std::runtime_error(std::string("chn_text_submit failed: ") + chn_last_error());
    };

    // Replica mode, once the models are final (before that every batch runs on replica 0, retired one by one: the models may change with
    // every read).  The main thread reads, splits and packs as before and deals the packed batches round-robin, numbered in input order;
    // each replica's thread submits them on its own stream and waits for them, and the ordered merge hands them back to the row writer
    // strictly in input order.  One replica (CHARON_DEVICES unset) is the same loop with N = 1.
    static const size_t kMaxOutstanding = 3;  // flights per replica between dealing and release (the writer holds two more)
    struct Replica {
        size_t index = 0;
        int device = 0;
        chn_stream *stream = nullptr;
        uint32_t model_version = 0;   // the models on its stream (every flight it submits must have been packed for them)
        std::mutex m;
        std::condition_variable cv;
        std::deque<std::unique_ptr<Flight>> in;  // dealt, not yet submitted
        uint64_t need = 0;            // flights up to this sequence number are wanted back (need_set: any)
        bool need_set = false, closing = false, stop = false;
        size_t outstanding = 0;       // main thread: dealt and not yet released by the merge
        uint64_t batches = 0, reads = 0;
        double t_submit = 0, t_wait = 0;
        std::thread t;
    };
    std::vector<std::unique_ptr<Replica>> reps;
    for (size_t r = 0; r < n_rep; ++r) {
        reps.emplace_back(new Replica());
        reps[r]->index = r; reps[r]->device = devices[r]; reps[r]->stream = rep_stream[r];
    }
    OrderedMerge<std::unique_ptr<Flight>> merge;
    bool dealing = false;  // the replica threads run
    uint64_t next_seq = 0;
    auto replica_body = [&](Replica &rp) {
        std::deque<std::unique_ptr<Flight>> flying;  // submitted, oldest first
        try {
            for (;;) {
                std::unique_ptr<Flight> f;
                {
                    std::unique_lock<std::mutex> lk(rp.m);
                    auto wait_oldest = [&] {
                        return !flying.empty() && (rp.closing || flying.size() >= kMaxOutstanding || (rp.need_set && flying.front()->seq <= rp.need));
                    };
                    rp.cv.wait(lk, [&] { return rp.stop || (!rp.in.empty() && flying.size() < kMaxOutstanding) || wait_oldest() || (rp.closing && rp.in.empty()); });
                    if (rp.stop) break;
                    if (!rp.in.empty() && flying.size() < kMaxOutstanding) {
                        f = std::move(rp.in.front());
                        rp.in.pop_front();
                    } else if (flying.empty()) {
                        return;  // closing, and everything has been handed back
                    }
                }
                if (f) {
                    if (f->version != rp.model_version)
                        throw std::runtime_error("batch packed for model version " + std::to_string(f->version) + ", stream holds " + std::to_string(rp.model_version));
                    const double tk = now();
                    submit_flight(rp.stream, *f);
                    rp.t_submit += now() - tk;
                    rp.batches += 1; rp.reads += f->sub.keep.size();
                    flying.push_back(std::move(f));
                    continue;
                }
                std::unique_ptr<Flight> g = std::move(flying.front());
                flying.pop_front();
                finish_wait(*g, rp.stream, rp.t_wait);
                const uint64_t seq = g->seq;
                merge.put(seq, std::move(g));
            }
        } catch (InputError &e) {
            merge.fail(e.what());  // the input's fault, not the replica's: the message a run without replicas gives
        } catch (std::exception &e) {
            merge.fail("replica " + std::to_string(rp.index) + " (device " + std::to_string(rp.device) + "): " + e.what());
        }
        if (!flying.empty()) (void)chn_stream_sync(rp.stream);  // the uploads out of these flights' buffers are over before they are freed
    };
    auto stop_replicas = [&]() {
        for (auto &rp : reps) { std::lock_guard<std::mutex> lk(rp->m); rp->stop = true; rp->cv.notify_all(); }
        for (auto &rp : reps) if (rp->t.joinable()) rp->t.join();
    };
    struct ReplicaJoin { std::function<void()> f; ~ReplicaJoin() { f(); } } replica_join{stop_replicas};
    // the next flight in input order, back from its replica, on to its rows
    auto release_next = [&]() {
        const uint64_t s = merge.next_seq();
        Replica &owner = *reps[(size_t)(s % n_rep)];
        { std::lock_guard<std::mutex> lk(owner.m); if (!owner.need_set || owner.need < s) { owner.need = s; owner.need_set = true; } owner.cv.notify_all(); }
        std::unique_ptr<Flight> f = merge.take();
        owner.outstanding -= 1;
        hand_on(f);
    };
    auto release_ready = [&]() {  // whatever has come back in order already, without waiting
        std::unique_ptr<Flight> f;
        while (merge.try_take(f)) {
            reps[(size_t)(f->seq % n_rep)]->outstanding -= 1;
            hand_on(f);
        }
    };
    auto drain_replicas = [&]() {  // every dealt flight back and on to its rows, in order
        while (merge.next_seq() < next_seq) release_next();
    };
    auto start_replicas = [&]() {
        // the final models on every replica's stream (replica 0's may lag behind the last change in training)
        result.ensure_device_model();
        reps[0]->model_version = result.current_model_version();
        for (size_t r = 1; r < n_rep; ++r) reps[r]->model_version = result.push_model_to_device(reps[r]->stream);
        for (auto &rp : reps) { Replica *p = rp.get(); p->t = std::thread([&replica_body, p]() { replica_body(*p); }); }
        dealing = true;
    };
    auto deal = [&](std::unique_ptr<Flight> &f) {
        const uint64_t s = next_seq++;
        Replica &rp = *reps[(size_t)(s % n_rep)];
        while (rp.outstanding >= kMaxOutstanding) release_next();
        f->seq = s;
        rp.outstanding += 1;
        std::lock_guard<std::mutex> lk(rp.m);
        rp.in.push_back(std::move(f));
        // its earlier flights are wanted back: it waits for them while this one runs (submit i + 1, wait i)
        if (s >= n_rep && (!rp.need_set || rp.need < s - n_rep)) { rp.need = s - n_rep; rp.need_set = true; }
        rp.cv.notify_all();
    };

    // ---- CHARON_GPU_TEXT=1: the read loop while the text stays in device memory ---------------------------------------------------
    // Everything that touches the stream -- split, submit, wait, fetch -- runs on this thread (one stream per host thread), so the
    // replica threads are not used: up to two batches are in flight while the next is split and submitted.
    uint64_t dt_split_records = 0, dt_fetched_records = 0, dt_fetched_bytes = 0;
    double t_split = 0, t_fetch = 0;
    uint64_t dp_pairs_checked = 0, dp_id2_bytes = 0;  // CHARON_GPU_TEXT_PAIRS=1: pairs through chn_text_pair_ids; id bytes of file 2 that came down
    double t_pair = 0;
    // After chn_text_wait: ONE chn_text_fetch for the reads whose letters the host needs -- the sequence of a read the device left
    // unsized, sequence and quality of every read under --extract (make_entry copies them; without --extract it reads the id alone,
    // in training too) -- into the flight's arena; the record views point there.  The block's buffer is let go afterwards.
    auto fetch_letters = [&](Flight &fl) {
        HostBatch &sub = fl.sub;
        const size_t n = sub.keep.size();
        const bool tallied = sub.gz_gpu_len != 0;
        // under --extract, sequence and quality of every read -- unless the flight's records are formed on the device (CHARON_GPU_EXTRACT=1)
        const bool letters = opt.run_extract && !fl.device_records;
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
                chn_text_fetch_job job;
                std::memset(&job, 0, sizeof job);
                const DevBlock &blk = k ? *sub.dtext2 : *sub.dtext;
                job.struct_size = sizeof job; job.text = blk.buf; job.text_bytes = blk.text_bytes;
                job.n_ranges = off[k].size(); job.offset = off[k].data(); job.length = len[k].data();
                job.out = arena + (k ? total[0] : 0); job.out_capacity = total[k];
                CHN_CHECK(chn_text_fetch(stream, &job));
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
    };
    typedef std::deque<std::unique_ptr<Flight>> Flying;  // submitted, oldest first
    struct SyncOnThrow {  // the device is done with these flights' arrays before they are freed
        Flying &f; chn_stream *s;
        ~SyncOnThrow() { if (!f.empty()) (void)chn_stream_sync(s); }
    };
    auto retire_front = [&](Flying &flying) {
        std::unique_ptr<Flight> f = std::move(flying.front());
        flying.pop_front();
        finish_wait(*f, stream, t_wait);
        // CHARON_GPU_EXTRACT=1: with final models and a current version every read of the flight is classified and written at once, so
        // its records can be formed where the text is; otherwise (training, or a version the models have moved on from) today's path
        f->device_records = g_gpu_extract && opt.run_extract && result.models_final() && result.current_model_version() == f->version;
        const double tk = now();
        fetch_letters(*f);
        t_fetch += now() - tk;
        hand_on(f);
    };
    // a packed resident flight on its way: at most two in flight, the models pushed while they train, one batch at a time until they are final
    bool final_pushed = false;
    auto submit_resident = [&](Flying &flying, std::unique_ptr<Flight> &fl) {
        const size_t n = fl->sub.keep.size();
        while (flying.size() >= 2) retire_front(flying);
        // (while the models are in training every batch is retired before the next is submitted, so nothing is in flight here)
        if (!final_pushed) { result.ensure_device_model(); final_pushed = result.models_final(); }
        fl->version = result.current_model_version();
        const double tk = now();
        submit_flight(stream, *fl);
        t_submit += now() - tk;
        reps[0]->batches += 1; reps[0]->reads += n;
        flying.push_back(std::move(fl));
        if (!result.models_final()) retire_front(flying);
    };
    // The tail [prev_from, prev->text_bytes) of the block before copied in front of member 0 of `blk`, so that it ends where member 0
    // begins; a tail longer than the gap (a record longer than the headroom) gets a fresh buffer for the two, which replaces `blk` (and
    // hb.dtext).  Returns where the text of `blk` now starts.
    auto carry_tail = [&](const std::shared_ptr<DevBlock> &prev, uint64_t prev_from, std::shared_ptr<DevBlock> &blk, HostBatch &hb) -> uint64_t {
        const int dev = g_gpu_text_device;
        const uint64_t tail = prev->text_bytes - prev_from, body = blk->text_bytes - blk->member0;
        if (tail > blk->member0) {
            std::shared_ptr<DevBlock> fresh(new DevBlock());
            void *p = nullptr;
            fresh->cap = (size_t)((tail + body + 15) & ~15ULL);
            CHN_CHECK(chn_device_malloc(dev, fresh->cap, &p));
            fresh->buf = static_cast<uint8_t *>(p);
            fresh->member0 = tail; fresh->text_bytes = tail + body; fresh->file_offset = blk->file_offset;
            fresh->z_end = blk->z_end; fresh->last = blk->last;
            if (body) CHN_CHECK(chn_device_copy(dev, fresh->buf + tail, blk->buf + blk->member0, body));
            blk = fresh;
            hb.dtext = fresh;
        }
        if (tail) CHN_CHECK(chn_device_copy(dev, blk->buf + blk->member0 - tail, prev->buf + prev_from, tail));
        return blk->member0 - tail;
    };
    // The records of blk's text from `start` on: descriptors and (want_ids) id bytes come back, letters and qualities stay where they
    // are.  The id bytes go to hb.ids; `sink` gets every record: its id bytes (null without want_ids), id length, sequence length, and
    // the offsets of id, sequence and quality string in the text.  Returns the offset behind the last record; *ids_bytes the id bytes
    // that came down.
    const uint64_t kSplitRecords = 1u << 18;  // per chn_text_split (its scratch is 52 bytes per record of this bound); a block with more takes several
    std::vector<uint64_t> ido, sqo, qlo;  // (sized by the first call: a run that is not resident never pays for them)
    std::vector<uint32_t> idl, sql;
    auto split_block = [&](const DevBlock &blk, uint64_t start, bool want_ids, HostBatch &hb,
                           const std::function<void(const char *, uint32_t, uint32_t, uint64_t, uint64_t, uint64_t)> &sink, uint64_t *ids_bytes) -> uint64_t {
        const uint64_t end = blk.text_bytes;
        uint64_t consumed = start, ids_used = 0;
        if (want_ids) hb.ids.reset(new char[end - start + 1]);
        if (ido.empty()) { ido.resize(kSplitRecords); sqo.resize(kSplitRecords); qlo.resize(kSplitRecords); idl.resize(kSplitRecords); sql.resize(kSplitRecords); }
        for (;;) {
            chn_text_split_job job;
            std::memset(&job, 0, sizeof job);
            job.struct_size = sizeof job; job.text = blk.buf; job.text_bytes = end; job.start = consumed; job.max_records = kSplitRecords;
            job.id_offset = ido.data(); job.id_length = idl.data(); job.seq_offset = sqo.data(); job.seq_length = sql.data(); job.qual_offset = qlo.data();
            if (want_ids) { job.ids = reinterpret_cast<uint8_t *>(hb.ids.get()) + ids_used; job.ids_capacity = end - start - ids_used; }
            CHN_CHECK(chn_text_split(stream, &job));
            const char *id = want_ids ? hb.ids.get() + ids_used : nullptr;
            for (uint64_t i = 0; i < job.n_records; ++i) {
                sink(id, idl[i], sql[i], ido[i], sqo[i], qlo[i]);
                if (id) id += idl[i];
            }
            if (want_ids) ids_used += job.ids_bytes;
            consumed = job.consumed;
            if (job.n_records < kSplitRecords) break;
        }
        if (ids_bytes) *ids_bytes = ids_used;
        return consumed;
    };
    // The same for a FASTA block (CHARON_GPU_TEXT_FASTA=1): chn_fasta_split unwraps the letters of the records it takes into `letters`,
    // a buffer of blk's capacity, and `sink` gets sequence offsets into THAT buffer (and no quality offset).  A block with more than
    // kSplitRecords records takes several calls; each writes behind the letters of the one before, from the next multiple of 16 on.
    // (Room: a call that stops at the bound has dropped at least ">\n" of each of its 2^18 records, so the letters end more than
    // 512 KiB below the text they came from.)  `eoi`: no text follows, the end counts as the last record's end.
    auto split_fasta_block = [&](const DevBlock &blk, DevBlock &letters, uint64_t start, bool eoi, HostBatch &hb,
                                 const std::function<void(const char *, uint32_t, uint32_t, uint64_t, uint64_t, uint64_t)> &sink, uint64_t *ids_bytes) -> uint64_t {
        const uint64_t end = blk.text_bytes;
        uint64_t consumed = start, ids_used = 0, base = 0;
        hb.ids.reset(new char[end - start + 1]);
        if (ido.empty()) { ido.resize(kSplitRecords); sqo.resize(kSplitRecords); qlo.resize(kSplitRecords); idl.resize(kSplitRecords); sql.resize(kSplitRecords); }
        letters.text_bytes = 0;
        for (;;) {
            chn_fasta_split_job job;
            std::memset(&job, 0, sizeof job);
            job.struct_size = sizeof job; job.flags = eoi ? CHN_FASTA_SPLIT_END_OF_INPUT : 0;
            job.text = blk.buf; job.text_bytes = end; job.start = consumed; job.max_records = kSplitRecords;
            job.id_offset = ido.data(); job.id_length = idl.data(); job.seq_offset = sqo.data(); job.seq_length = sql.data();
            job.seq_text = letters.buf + base; job.seq_capacity = letters.cap - base;
            job.ids = reinterpret_cast<uint8_t *>(hb.ids.get()) + ids_used; job.ids_capacity = end - start - ids_used;
            CHN_CHECK(chn_fasta_split(stream, &job));
            const char *id = hb.ids.get() + ids_used;
            for (uint64_t i = 0; i < job.n_records; ++i) {
                sink(id, idl[i], sql[i], ido[i], base + sqo[i], 0);
                id += idl[i];
            }
            ids_used += job.ids_bytes;
            consumed = job.consumed;
            letters.text_bytes = base + job.seq_bytes;
            base += (job.seq_bytes + 15) & ~15ULL;
            if (job.n_records < kSplitRecords) break;
        }
        if (ids_bytes) *ids_bytes = ids_used;
        return consumed;
    };
    // The loop over `n_sides` files: one (single-end) or two (CHARON_GPU_TEXT_PAIRS=1).  Each side (file) keeps its current block, the
    // descriptors of the records that are split but not yet in a batch, and `consumed`.  A side with no such record left takes its next
    // block (the tail of the block before carried in front of it); a side that still has some does not, so files with records of unequal
    // size never pile up text and no record is split twice.  The records at hand -- with two sides the pairs: the shorter of the two
    // lists -- therefore lie in ONE block of either file, and a batch of them is a chn_text_batch (chn_text_batch2) over it (them).  The
    // ids of a batch of pairs are compared on the device before the submit; the ids of file 2 come down with the split under --extract only.
    auto run_resident = [&]() {
        Flying flying;
        SyncOnThrow sync_on_throw{flying, stream};
        const int dev = g_gpu_text_device;
        const bool two = n_sides == 2;
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
        } side[2];
        Side &s1 = side[0], &s2 = side[1];
        std::string reader_failure;
        // the side readers are done with (one may still wait to hand over a block nobody wants)
        auto stop_side_readers = [&]() {
            for (int s = 0; s < n_sides; ++s) side_queue[s].abort();
            for (int s = 0; s < n_sides; ++s) if (side_reader[s].joinable()) side_reader[s].join();
            for (int s = 0; s < n_sides; ++s) { side[s].hb.reset(); side[s].blk.reset(); side[s].letters.reset(); }
        };
        // Leaving the mode because of side k: every flight retired, each side's text from behind its last paired record downloaded, the
        // side readers stopped, and the host reader started with every file resumed.  That text and the rest of the files go through the
        // host's splitter and sequential parser, which produce today's rows and today's messages.
        auto leave = [&](int k) {
            while (!flying.empty()) retire_front(flying);
            for (int s = 0; s < n_sides; ++s) {
                Side &sd = side[s];
                resumed[s] = true;
                if (!sd.blk) continue;  // (no block of this file was taken: it starts from its first member)
                resume_z[s] = sd.blk->z_end;
                const uint64_t from = sd.paired_end, end = sd.blk->text_bytes;
                resume_carry[s].resize((size_t)(end - from));
                if (end > from) CHN_CHECK(chn_device_download(dev, resume_carry[s].data(), sd.blk->buf + from, end - from));
            }
            const Side &sk = side[k];
            g_log.info("CHARON_GPU_TEXT=1: leaving the device-resident path at byte " + std::to_string(sk.blk->file_offset + sk.consumed - sk.blk->member0) +
                       " of the inflated file " + (two ? (k ? opt.read_file2 : opt.read_file) + " " : "") +
                       (fasta_side ? "(text that is no FASTA record the device takes, or a record longer than a block)" : "(text that is no plain four-line record)") +
                       ": the host parser goes on from there");
            stop_side_readers();
            g_gpu_inflate = true; g_gpu_inflate_device = dev; g_pin_slabs = true;  // inflate as under CHARON_GPU_INFLATE=1 from here on
            reader = std::thread(reader_body);
        };
        // the next block of side k, the tail of the block before in front of it, split into records.  true: the mode has to be left
        auto take_block = [&](int k) -> bool {
            Side &sd = side[k];
            const double tp = now();
            std::shared_ptr<HostBatch> hbp = side_queue[k].pop();
            t_pop += now() - tp;
            if (!hbp) {  // the end of the file, or the reader's error
                sd.eof = true;
                if (!side_queue[k].error.empty()) reader_failure = side_queue[k].error;
                return false;
            }
            HostBatch &hb = *hbp;
            std::shared_ptr<DevBlock> blk = hb.dtext;
            double tk = now();
            uint64_t start = blk->member0;
            // (every record of the block before is paired: its tail is [consumed, text_bytes))
            if (sd.blk) start = carry_tail(sd.blk, sd.consumed, blk, hb);
            const uint64_t end = blk->text_bytes;
            // the TSV prints the id of mate 1; mate 2's is written under --extract only -- and under CHARON_GPU_EXTRACT=1 out of the device
            // text, or (a flight on the host path) fetched with its letters
            const bool want_ids = k == 0 || (opt.run_extract && !g_gpu_extract);
            sd.id_off.clear(); sd.seq_off.clear(); sd.qual_off.clear(); sd.id_len.clear(); sd.seq_len.clear(); sd.id.clear(); sd.head = 0;
            uint64_t ids_bytes = 0;
            const auto sink = [&](const char *id, uint32_t id_len, uint32_t seq_len, uint64_t io, uint64_t so, uint64_t qo) {
                sd.id.push_back(id); sd.id_len.push_back(id_len); sd.seq_len.push_back(seq_len);
                sd.id_off.push_back(io); sd.seq_off.push_back(so); sd.qual_off.push_back(qo);
            };
            if (fasta_side) {  // a buffer of the block's size for the letters: of the pool where the block's is
                sd.letters.reset(new DevBlock());
                DevBlock &lt = *sd.letters;
                lt.cap = blk->cap;
                if (blk->pooled) { lt.buf = static_cast<uint8_t *>(g_dev_text_pool.take(lt.cap)); lt.pooled = true; }
                else { void *p = nullptr; CHN_CHECK(chn_device_malloc(dev, lt.cap, &p)); lt.buf = static_cast<uint8_t *>(p); }
            }
            const uint64_t consumed = fasta_side ? split_fasta_block(*blk, *sd.letters, start, blk->last, hb, sink, &ids_bytes)
                                                 : split_block(*blk, start, want_ids, hb, sink, &ids_bytes);
            if (k == 1) dp_id2_bytes += ids_bytes;
            t_split += now() - tk;
            dt_split_records += sd.id_off.size();
            sd.hb = hbp; sd.blk = blk; sd.consumed = consumed; sd.paired_end = start;
            if (fasta_side) {
                // At the end of the file everything is taken unless the rule failed.  Before it, text is left over behind the last record
                // taken (at least its successor's header), which the next block completes -- unless no record was taken at all: then
                // the text at `consumed` is no header line, or its record is empty (a second header line follows), or the record does
                // not end in this text; that one is carried on while it is shorter than a block
                if (consumed >= end) return false;
                if (blk->last) return true;
                if (!sd.id_off.empty()) return false;
                Slab tail_text((size_t)(end - consumed));
                CHN_CHECK(chn_device_download(dev, tail_text.data(), blk->buf + consumed, end - consumed));
                const char *t = tail_text.data(), *te = t + tail_text.size();
                if (*t != '>' && *t != ';') return true;
                for (const char *nl = static_cast<const char *>(std::memchr(t, '\n', (size_t)(te - t))); nl && nl + 1 < te;
                     nl = static_cast<const char *>(std::memchr(nl + 1, '\n', (size_t)(te - nl - 1))))
                    if (nl[1] == '>' || nl[1] == ';') return true;
                return end - consumed >= resident_block_bytes;
            }
            // no record although four line feeds follow `start` (a wrapped record, a blank line, a damaged record), or bytes behind the
            // last record at the end of the file (a last line without a line feed)
            if (consumed < end && (sd.id_off.empty() || blk->last)) {
                if (blk->last) return true;
                Slab tail_text((size_t)(end - consumed));
                CHN_CHECK(chn_device_download(dev, tail_text.data(), blk->buf + consumed, end - consumed));
                if (std::count(tail_text.begin(), tail_text.end(), '\n') >= 4) return true;
            }
            return false;
        };
        // the ids of the next `cnt` pairs must agree after dropping the last character (src/dehost_main.cpp:423-430): on the device
        auto check_pair_ids = [&](size_t cnt) {
            const double tk = now();
            chn_text_pair_job pj;
            std::memset(&pj, 0, sizeof pj);
            pj.struct_size = sizeof pj; pj.text1 = s1.blk->buf; pj.text1_bytes = s1.blk->text_bytes; pj.text2 = s2.blk->buf; pj.text2_bytes = s2.blk->text_bytes;
            pj.n_pairs = cnt; pj.id1_offset = s1.id_off.data() + s1.head; pj.id1_length = s1.id_len.data() + s1.head;
            pj.id2_offset = s2.id_off.data() + s2.head; pj.id2_length = s2.id_len.data() + s2.head;
            CHN_CHECK(chn_text_pair_ids(stream, &pj));
            t_pair += now() - tk;
            dp_pairs_checked += cnt;
            if (pj.first_mismatch >= cnt) return;
            const size_t a = s1.head + (size_t)pj.first_mismatch, b = s2.head + (size_t)pj.first_mismatch;
            while (!flying.empty()) retire_front(flying);
            if (writer.t.joinable()) writer_drain();
            const uint32_t la = s1.id_len[a] ? s1.id_len[a] - 1 : 0, lb = s2.id_len[b] ? s2.id_len[b] - 1 : 0;
            std::string id2(lb, '\0');
            if (lb) {  // the one id of file 2 this run needs on the host
                chn_text_fetch_job job;
                std::memset(&job, 0, sizeof job);
                const uint64_t o = s2.id_off[b];
                job.struct_size = sizeof job; job.text = s2.blk->buf; job.text_bytes = s2.blk->text_bytes;
                job.n_ranges = 1; job.offset = &o; job.length = &lb;
                job.out = reinterpret_cast<uint8_t *>(&id2[0]); job.out_capacity = lb;
                CHN_CHECK(chn_text_fetch(stream, &job));
            }
            pairs_do_not_match(s1.id[a], la, id2.data(), lb);
        };
        // The next `cnt` records of every side as one flight: record views and pack, then where their letters, qualities and ids lie in
        // the texts (with one side the second halves stay cleared); every side moves on by `cnt`.
        auto fill_flight = [&](Flight &fl, size_t cnt) {
            fl.parent = s1.hb;
            if (two) fl.parent2 = s2.hb;
            fl.resident = true;
            HostBatch &sub = fl.sub;
            auto views = [&](const Side &sd, std::vector<RecView> &recs) {
                recs.resize(cnt);
                for (size_t i = 0; i < cnt; ++i) {
                    RecView r;
                    r.id = sd.id[sd.head + i]; r.id_len = r.id ? sd.id_len[sd.head + i] : 0; r.seq_len = sd.seq_len[sd.head + i];
                    r.qual_len = fasta_side ? 0 : r.seq_len;
                    recs[i] = r;
                }
            };
            views(s1, sub.blk1.recs);
            if (two) views(s2, sub.blk2.recs);
            const double tk = now();
            sub.pack(two, opt.threads, skip_compression, gz_gpu_max, gz_route_long, true, nullptr, true);
            const size_t n = sub.keep.size();
            auto columns = [&](const Side &sd, const std::vector<uint32_t> &len, std::vector<uint64_t> &so, std::vector<uint64_t> &qo, std::vector<uint32_t> &ql,
                               std::vector<uint64_t> &io, std::vector<uint32_t> &il) {
                so.resize(n); qo.resize(n); ql = len;
                if (g_gpu_extract) { io.resize(n); il.resize(n); }
                for (size_t i = 0; i < n; ++i) {
                    const size_t a = sd.head + sub.keep[i];
                    so[i] = sd.seq_off[a]; qo[i] = sd.qual_off[a];
                    if (g_gpu_extract) { io[i] = sd.id_off[a]; il[i] = sd.id_len[a]; }
                }
            };
            columns(s1, sub.len1, sub.so1, sub.qo1, sub.ql1, sub.io1, sub.il1);
            if (two) columns(s2, sub.len2, sub.so2, sub.qo2, sub.ql2, sub.io2, sub.il2);
            else { sub.so2.clear(); sub.qo2.clear(); sub.ql2.clear(); }
            sub.text_quals = !fasta_side; sub.text_from_slab = false;
            if (fasta_side) sub.ql1.assign(n, 0);  // (no quality string: the ranges fetch_letters asks for them are empty)
            sub.dtext = fasta_side ? s1.letters : s1.blk;
            if (two) sub.dtext2 = s2.blk;
            t_pack += now() - tk;
            for (int k = 0; k < n_sides; ++k) {
                Side &sd = side[k];
                sd.head += cnt;
                sd.paired_end = sd.unpaired() ? sd.id_off[sd.head] - 1 : sd.consumed;  // ('@' stands in front of an id)
            }
        };
        for (;;) {
            // Leaving the mode is noted here and done once the records at hand are submitted: side `leaving` met text the device cannot
            // go on splitting.
            int leaving = -1;
            for (int k = 0; k < n_sides && leaving < 0; ++k)
                while (side[k].unpaired() == 0 && !side[k].eof)  // (a block may end inside its first record and yield none)
                    if (take_block(k)) { leaving = k; break; }
            size_t avail = two ? std::min(s1.unpaired(), s2.unpaired()) : s1.unpaired();
            if (avail == 0 && leaving < 0) break;  // a file has run out: the records submitted so far are all there are
            while (avail) {
                // GPU batches that respect the stream's capacity, as below
                const size_t cnt = cut_batch(0, avail, [&](size_t i) {
                    return HostBatch::pad64(s1.seq_len[s1.head + i]) + (two ? HostBatch::pad64(s2.seq_len[s2.head + i]) : 0);
                });
                if (two) check_pair_ids(cnt);
                std::unique_ptr<Flight> fl = take_flight();
                fill_flight(*fl, cnt);
                avail -= cnt;
                if (fl->sub.keep.empty()) { fl->sub.dtext.reset(); fl->sub.dtext2.reset(); continue; }
                submit_resident(flying, fl);
            }
            if (leaving >= 0) { leave(leaving); return; }
        }
        while (!flying.empty()) retire_front(flying);
        // nothing was left: the loop below, which reads the host reader's queue, finds it finished -- with the error a side reader met,
        // if one did
        stop_side_readers();
        queue.finish(reader_failure);
    };
    try {
        if (n_sides) run_resident();
        for (;;) {
            double tp = now();
            std::shared_ptr<HostBatch> hbp = queue.pop();
            t_pop += now() - tp;
            if (!hbp) break;
            HostBatch &hb = *hbp;
            const size_t nrec = hb.blk1.recs.size();
            if (opt.is_paired) {
                for (size_t i = 0; i < nrec; ++i) {  // pair ids must agree after dropping the last character (:423-430)
                    const RecView &a = hb.blk1.recs[i], &b = hb.blk2.recs[i];
                    const uint32_t la = a.id_len ? a.id_len - 1 : 0, lb = b.id_len ? b.id_len - 1 : 0;
                    if (la != lb || std::memcmp(a.id, b.id, la) != 0) {
                        if (dealing) drain_replicas();
                        if (writer.t.joinable()) writer_drain();
                        pairs_do_not_match(a.id, la, b.id, lb);
                    }
                }
            }
            // split the block into GPU batches that respect the stream's capacity
            size_t begin = 0;
            while (begin < nrec) {
                const size_t endi = cut_batch(begin, nrec, [&](size_t i) {
                    return HostBatch::pad64(hb.blk1.recs[i].seq_len) + (opt.is_paired ? HostBatch::pad64(hb.blk2.recs[i].seq_len) : 0);
                });
                if (dealing) release_ready();
                std::unique_ptr<Flight> fl = take_flight();
                fl->parent = hbp;
                fl->resident = false;
                HostBatch &sub = fl->sub;
                sub.bases.want_pinned = sub.nmask.want_pinned = true;  // three of these go round: uploads straight out of them
                sub.blk1.recs.assign(hb.blk1.recs.begin() + (long)begin, hb.blk1.recs.begin() + (long)endi);
                if (opt.is_paired) sub.blk2.recs.assign(hb.blk2.recs.begin() + (long)begin, hb.blk2.recs.begin() + (long)endi);
                begin = endi;
                double tk = now();
                sub.pack(opt.is_paired, opt.threads, skip_compression, gz_gpu_max, gz_route_long, opt.text_batches,
                         (!opt.is_paired && !hb.blk1.map_begin) ? &hb.blk1.buf : nullptr);  // batch i+1 is packed while the GPU works on batch i
                t_pack += now() - tk;
                const size_t n = sub.keep.size();
                if (n == 0) continue;
                if (result.models_final()) {
                    // (nothing is in flight on replica 0 when the models become final: every training batch is retired before the next)
                    if (!dealing) start_replicas();
                    fl->version = result.current_model_version();
                    deal(fl);
                    release_ready();
                    continue;
                }
                // a model still in training may change with every read added below: every batch is retired before the next is submitted
                result.ensure_device_model();
                fl->version = result.current_model_version();
                tk = now();
                submit_flight(stream, *fl);
                t_submit += now() - tk;
                reps[0]->batches += 1; reps[0]->reads += n;
                retire(fl);
            }
        }
        if (dealing) {
            drain_replicas();
            for (auto &rp : reps) { std::lock_guard<std::mutex> lk(rp->m); rp->closing = true; rp->cv.notify_all(); }
            for (auto &rp : reps) if (rp->t.joinable()) rp->t.join();
        }
        if (writer.t.joinable()) writer_drain();
        if (!queue.error.empty()) failure = queue.error;
    } catch (std::exception &e) {
        failure = e.what();
        queue.abort();  // the reader thread stops at its next block
        stop_replicas();
    }
    if (reader.joinable()) reader.join();
    if (!failure.empty()) { std::cout.flush(); throw std::runtime_error(failure); }
    result.complete();
    std::cout.flush();
    if (timing) {
        timing_line("timing (main thread, s): wait-for-reader %.3f  pack %.3f  submit %.3f  wait-for-gpu %.3f  tallies->sizes %.3f  rows %.3f",
                    t_pop, t_pack, t_submit, t_wait, t_gz, t_rows);
        timing_line("timing (reader thread, s): inflate %.3f  record splitting %.3f", g_reader_fill_s, g_reader_parse_s);
        if (g_gpu_inflate) timing_line("timing (reader thread, s): inside chn_inflate_run %.3f (part of inflate)", g_gpu_inflate_s);
        if (n_sides)
            timing_line("timing (CHARON_GPU_TEXT=1): records split %llu  records fetched %llu  text bytes inflated %llu  text bytes fetched %llu  "
                        "seconds in inflate %.3f  seconds in split %.3f  seconds in fetch %.3f",
                        (unsigned long long)dt_split_records, (unsigned long long)dt_fetched_records, (unsigned long long)g_gpu_text_inflated,
                        (unsigned long long)dt_fetched_bytes, g_gpu_inflate_s, t_split, t_fetch);
        if (n_sides == 2)
            timing_line("timing (CHARON_GPU_TEXT_PAIRS=1): pairs checked %llu  id bytes of file 2 downloaded %llu  seconds in pair check %.3f",
                        (unsigned long long)dp_pairs_checked, (unsigned long long)dp_id2_bytes, t_pair);
        if (g_gpu_deflate) timing_line("timing (main thread, s): inside chn_deflate_run %.3f (extract files)", g_gpu_deflate_s);
        if (g_gpu_extract)
            timing_line("timing (CHARON_GPU_EXTRACT=1): records formed on the device %llu  bytes appended from the host %llu  compressed bytes down %llu  "
                        "seconds in chn_extract calls %.3f", (unsigned long long)g_gpu_extract_records, (unsigned long long)g_gpu_extract_host_bytes,
                        (unsigned long long)g_gpu_extract_down, g_gpu_extract_s);
        timing_line("timing (start-up, s): index file read %.3f  device + index create %.3f  index decode, stream, models %.3f (of which reference self-check %.3f)  read loop %.3f",
                    t_meta - t_entry, t_hip - t_meta, t_ready - t_hip, t_ready - t_sc0, now() - t_ready);
        timing_line("timing (index decode, s): select blocks checked %.3f  page-locked staging %.3f  slices staged %.3f  waited for the device %.3f  bin popcounts %.3f",
                    file.t_verify, file.t_stage_alloc, file.t_stage_fill, file.t_device_wait, file.t_popcounts);
    }
    for (auto &rp : reps) {
        g_log.info("replica " + std::to_string(rp->index) + " (device " + std::to_string(rp->device) + "): " + std::to_string(rp->batches) + " batches, " +
                   std::to_string(rp->reads) + " reads");
        if (timing && dealing)
            timing_line("timing (replica %zu, device %d, s): submit %.3f  wait-for-gpu %.3f", rp->index, rp->device, rp->t_submit, rp->t_wait);
    }
    if (opt.text_batches)
        g_log.info("text batches: " + std::to_string(text_slab_batches.load()) + " sent as the block's slab, " + std::to_string(text_copy_batches.load()) +
                   " as a page-locked copy of letters and qualities");
    if (gz_gpu_max) g_log.info("gzip column: " + std::to_string(gz_on_device) + " reads sized from device deflate tallies (the rest on the host)");
    if (gz_gpu_max) g_log.info("gzip column: " + std::to_string(gz_long_on_device) + " reads beyond " + std::to_string(CHN_GZIP_MAX_LEN) + " letters sized by the device's long-read deflate pass");
    result.print_summary();
    // the process is about to exit: unmapping gigabytes of read file page by page is time nobody needs
    (void)in1p.release(); (void)in2.release();
    const double t_tear = now();
    chn_stream_destroy(stream);
    chn_index_destroy(index);
    if (timing) {
        const double wall = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
        std::fprintf(stderr, "charon: timing (tear-down, s): stream + index destroy %.3f; dehost_main %.3f in all, returning at wall clock %.3f\n", now() - t_tear, now() - t_entry, wall);
    }
    return 0;
}
