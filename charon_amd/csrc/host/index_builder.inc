// index_builder.inc -- `charon index`: arguments, Elias-Fano / cereal writers, index_main (src/index_main.cpp, include/store_index.hpp)
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a
// stand-alone header.

// ===================================================================================================
// charon index  (src/index_main.cpp; include/index_arguments.hpp:9-27; include/store_index.hpp:12-17)
// ===================================================================================================
struct IndexArguments {
    std::string input_file, prefix, tmp_dir, log_file = "charon.log";
    uint8_t window_size = 41, kmer_size = 19;
    uint64_t bits = 4294967293ULL;  // numeric_limits<uint32_t>::max() - 2
    uint8_t num_hash = 3;
    double max_fpr = 0.01;
    uint8_t threads = 1, verbosity = 0;
    bool optimize = false;
    int device = 0;
    bool gpu_ef = false;  // CHARON_GPU_INDEX_EF=1: the Elias-Fano arrays are encoded on the device (chn_index_encode_ef)
    bool gpu_sets = false;  // CHARON_GPU_INDEX_SETS=1: the bins' minimisers stay in device memory (chn_hashset), sorted and made distinct there
};

bool parse_index(int argc, char **argv, IndexArguments &opt) {
    std::vector<std::string> pos;
    for (int i = 0; i < argc; ++i) {
        std::string a = argv[i], val;
        bool has_val = false;
        if (a.size() > 2 && a[0] == '-' && a[1] == '-') {
            const size_t eq = a.find('=');
            if (eq != std::string::npos) { val = a.substr(eq + 1); a = a.substr(0, eq); has_val = true; }
        }
        auto need = [&]() -> std::string {
            if (has_val) return val;
            if (i + 1 >= argc) throw ParseError(a + ": 1 required");
            return argv[++i];
        };
        if (a == "-h" || a == "--help") {
            std::cout << "Build an index (IBF) for a number of references split into a small number of bins.\n"
                         "Usage: charon index [OPTIONS] <input>\n\nPositionals:\n  <input> FILE REQUIRED   Tab separated file with columns for filename and category\n\n"
                         "Options:\n  -w INT=41               Window size for (w,k,s)-minimers (must be <=k).\n  -k INT=19               K-mer size for (w,k,s)-minimers.\n"
                         "  -t,--threads INT=1      Maximum number of threads to use.\n  -p,--prefix FILE        Prefix for the output index.\n"
                         "  --temp DIR              Temporary directory for index construction files.\n  --log FILE              File for log\n"
                         "  --optimize              Compress the number of bins for improved classification run time\n  -v                      Verbosity of logging.\n\n"
                         "Note (MI355X build): the .idx is laid out as upstream charon's (cereal binary archive, sdsl sd_vector with its two\n"
                         "select_support_mcl blocks) per the published sdsl-lite v3 / cereal formats; no upstream-written file was available\n"
                         "to compare with (parity unpinned).\n";
            return false;
        }
        else if (a == "-w") opt.window_size = (uint8_t)parse_uint("w", need(), 255);
        else if (a == "-k") opt.kmer_size = (uint8_t)parse_uint("k", need(), 255);
        else if (a == "-t" || a == "--threads") opt.threads = (uint8_t)parse_uint("threads", need(), 255);
        else if (a == "-p" || a == "--prefix") opt.prefix = need();
        else if (a == "--temp") opt.tmp_dir = need();
        else if (a == "--log") opt.log_file = need();
        else if (a == "--optimize") opt.optimize = true;
        else if (a.size() >= 2 && a[0] == '-' && a.find_first_not_of('v', 1) == std::string::npos) opt.verbosity = (uint8_t)std::min<size_t>(255, opt.verbosity + a.size() - 1);
        else if (!a.empty() && a[0] == '-' && a.size() > 1) throw ParseError("The following argument was not expected: " + a);
        else pos.push_back(a);
    }
    if (pos.empty()) throw ParseError("<input> is required");
    if (pos.size() > 1) throw ParseError("The following argument was not expected: " + pos[1]);
    if (!is_file(pos[0])) throw ParseError("<input>: File does not exist: " + pos[0]);
    if (!opt.prefix.empty() && path_exists(opt.prefix)) throw ParseError("--prefix: Path already exists: " + opt.prefix);
    opt.input_file = pos[0];
    return true;
}

std::string make_absolute(const std::string &p) {
    if (!p.empty() && p[0] == '/') return p;
    char buf[4096];
    if (!::getcwd(buf, sizeof buf)) return p;
    return std::string(buf) + "/" + p;
}

// bin_size_in_bits (src/utils.cpp:75-90)
uint64_t bin_size_in_bits(const IndexArguments &opt, uint64_t num_elements) {
    const double numerator = -static_cast<double>(num_elements * opt.num_hash);
    const double denominator = std::log(1 - std::exp(std::log(opt.max_fpr) / opt.num_hash));
    const double result = std::ceil(numerator / denominator);
    if (result > (double)opt.bits) { g_log.warn("Require more bits than available for max_fpr"); return opt.bits; }
    return (uint64_t)result;
}

// sdsl::sd_vector construction (SURVEY App. A.5) from ascending set-bit positions delivered block-wise, and the cereal
// binary archive of Index::serialize (include/index.hpp:122-131).  The two trailing select_support_mcl structures of
// sd_vector are written by selmcl::build (sdsl_select.inc).
struct EliasFanoWriter {
    uint64_t size = 0, ones = 0, high_bits = 0, k = 0;
    uint8_t wl = 0;
    std::vector<uint64_t> low, high;
    static unsigned hi(uint64_t x) { return x ? 63u - (unsigned)__builtin_clzll(x) : 0u; }
    void begin(uint64_t universe, uint64_t n_ones) {
        size = universe; ones = n_ones; k = 0;
        unsigned logm = hi(ones) + 1;
        const unsigned logn = hi(size) + 1;
        if (logm == logn) --logm;
        wl = (uint8_t)(logn - logm);
        high_bits = ones + (1ULL << logm);
        low.assign((ones * wl + 63) / 64 + 1, 0);
        high.assign((high_bits + 63) / 64, 0);
    }
    void add(uint64_t pos) {
        if (wl) {
            const uint64_t v = pos & ((1ULL << wl) - 1), bit = k * wl, wd = bit >> 6, sh = bit & 63;
            low[wd] |= v << sh;
            if (sh + wl > 64) low[wd + 1] |= v >> (64 - sh);
        }
        const uint64_t hp = (pos >> wl) + k;
        high[hp >> 6] |= 1ULL << (hp & 63);
        ++k;
    }
    // the i-th set bit (i counted from 0 over the whole vector) at position pos, from any thread: the words at the seams between
    // two threads' stretches are shared, hence the atomic ORs
    void add_at(uint64_t pos, uint64_t i) {
        if (wl) {
            const uint64_t v = pos & ((1ULL << wl) - 1), bit = i * wl, wd = bit >> 6, sh = bit & 63;
            __atomic_fetch_or(&low[wd], v << sh, __ATOMIC_RELAXED);
            if (sh + wl > 64) __atomic_fetch_or(&low[wd + 1], v >> (64 - sh), __ATOMIC_RELAXED);
        }
        const uint64_t hp = (pos >> wl) + i;
        __atomic_fetch_or(&high[hp >> 6], 1ULL << (hp & 63), __ATOMIC_RELAXED);
    }
};

// The set bits of words[0 .. nwords) -- word i covers positions [bit0 + 64 i, bit0 + 64 i + 64) -- written into `ef` by `threads` threads at
// once: the block is cut into one stretch per thread, the set bits of every stretch are counted, and each thread then writes its bits at
// their final places (a set bit's place in the Elias-Fano arrays depends only on its position and on how many set bits precede it;
// `before` = set bits in front of this block).  Returns the number of set bits of the block.
uint64_t ef_add_block(EliasFanoWriter &ef, const uint64_t *words, uint64_t nwords, uint64_t bit0, uint64_t before, int threads) {
    std::vector<uint64_t> first((size_t)std::max(1, threads) + 1, 0);
    uint64_t team = 1;
#pragma omp parallel num_threads(std::max(1, threads))
    {
        // (the runtime may give fewer threads than asked for: the stretches are cut by the size of the team that is really there)
        const uint64_t T = (uint64_t)omp_get_num_threads(), per = (nwords + T - 1) / T;
        const uint64_t t = (uint64_t)omp_get_thread_num(), lo = std::min(nwords, t * per), hi = std::min(nwords, lo + per);
        uint64_t c = 0;
        for (uint64_t i = lo; i < hi; ++i) c += (uint64_t)__builtin_popcountll(words[i]);
        first[t + 1] = c;
#pragma omp barrier
#pragma omp single
        { team = T; first[0] = before; for (uint64_t q = 0; q < T; ++q) first[(size_t)q + 1] += first[(size_t)q]; }
        uint64_t k = first[t];
        for (uint64_t i = lo; i < hi; ++i) {
            uint64_t x = words[i];
            const uint64_t base = bit0 + i * 64;
            while (x) { ef.add_at(base + (uint64_t)__builtin_ctzll(x), k++); x &= x - 1; }
        }
    }
    return first[(size_t)team] - before;
}

struct BinWriter {
    std::ofstream os;
    explicit BinWriter(const std::string &path) : os(path, std::ios::binary) { if (!os) throw std::runtime_error("cannot create " + path); }
    template <class T> void pod(const T &v) { os.write(reinterpret_cast<const char *>(&v), sizeof(T)); }
    void str(const std::string &s) { pod<uint64_t>(s.size()); os.write(s.data(), (std::streamsize)s.size()); }
    void int_vector(uint8_t width, uint64_t bit_size, const std::vector<uint64_t> &words) {
        const uint64_t n_words = (bit_size + 63) >> 6;
        pod<uint8_t>(width); pod<float>(1.5f); pod<uint64_t>(n_words); pod<uint64_t>(bit_size);
        os.write(reinterpret_cast<const char *>(words.data()), (std::streamsize)(n_words * 8));
    }
};

// distinct values in ascending order; the sort runs on the -t threads (a bin of a human-sized reference holds some 10^8 minimisers:
// seconds on one thread, and the GPU that produced them waits)
void sort_unique(std::vector<uint64_t> &v, int threads) {
    static const size_t par_min = []() { const char *e = std::getenv("CHARON_PSORT_MIN"); return e ? (size_t)std::strtoull(e, nullptr, 10) : (size_t)1 << 16; }();  // test hook
    if (threads > 1 && v.size() > par_min) __gnu_parallel::sort(v.begin(), v.end(), __gnu_parallel::multiway_mergesort_tag((unsigned)threads));
    else std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
}

// CHARON_GPU_INDEX_SETS=1: the bins' minimiser sets in device memory and the budget of bytes they share.  The sets must not end a run
// that the host path would have finished: when the set being filled would pass the budget, cannot get its memory or reaches 2^32
// values, it comes down into the bin's host vector and that bin and every later one take the host path (spill); the sets of the
// bins done stay where they are.
struct DeviceSets {
    bool on = false;                    // the bin being read, and those behind it, still go to the device
    uint64_t budget = 0;                // bytes; default: half of what the device had free at the start (a guess, not a tuned value)
    uint64_t compact_at = 1ULL << 26;   // values appended to a set before it is made distinct inside the loop, as on the host path
    uint64_t held_done = 0;             // bytes the sets of the bins done hold
    std::vector<chn_hashset *> set;     // per bin; null: the bin's minimisers are in its host vector
    std::vector<uint64_t> appended;     // per bin: values that went from the minimiser kernel's log into the set
    uint64_t held_with(const chn_hashset *h, uint64_t *n = nullptr) const {
        uint64_t nn = 0, bytes = 0;
        CHN_CHECK(chn_hashset_size(h, &nn, &bytes));
        if (n) *n = nn;
        return held_done + bytes;
    }
    // chn_hashset_unique if its scratch fits the budget and the device has it; false: it did not run, the set is as it was
    bool unique(chn_hashset *h, uint64_t &distinct) const {
        uint64_t n = 0;
        const uint64_t held = held_with(h, &n);
        if (held + radix_scratch_bytes(n, RADIX_TILE_DEFAULT) > budget) return false;
        const int rc = chn_hashset_unique(h, &distinct);
        if (rc == CHN_E_NOMEM) return false;
        if (rc != CHN_OK) throw std::runtime_error(std::string("chn_hashset_unique failed: ") + chn_last_error());
        return true;
    }
    // the set of `bin` comes down behind the values `host` holds; from here on every bin takes the host path
    void spill(uint8_t bin, std::vector<uint64_t> &host, const std::string &why) {
        chn_hashset *h = set[bin];
        uint64_t n = 0;
        (void)unique(h, n);  // fewer values to bring down, if it can be done
        (void)held_with(h, &n);
        const size_t old = host.size();
        host.resize(old + n);
        CHN_CHECK(chn_hashset_download(h, 0, n, host.data() + old));
        chn_hashset_destroy(h);
        set[bin] = nullptr; appended[bin] = 0; on = false;
        g_log.info("CHARON_GPU_INDEX_SETS=1: bin " + std::to_string(bin) + " and the bins behind it take the host path (" + why + "); " + std::to_string(n) +
                   " values of its set came down");
    }
};

int index_main(IndexArguments &opt) {
    g_log.open(opt.log_file, opt.verbosity);
    g_reader_threads = reader_threads_for(opt.threads);
    // src/index_main.cpp:274-291
    if (opt.window_size < opt.kmer_size) throw std::logic_error("W must be greater than K");
    if (opt.kmer_size == 0) throw std::logic_error("K must be a positive integer");
    if (opt.kmer_size > 27) throw std::logic_error("K must be at most 27 for the dna5 alphabet (5^k has to fit 64 bits)");
    opt.input_file = make_absolute(opt.input_file);
    if (!opt.prefix.empty()) opt.prefix += ".idx"; else opt.prefix = opt.input_file + ".idx";
    g_log.info(std::string("Running charon index\n\nCharon version: ") + CHARON_VERSION);

    // parse_input_file (:75-116).  Category order = iteration order of an unordered_set<string>, reproduced by using the same
    // container of the same standard library (libstdc++) -- quirk A.9.
    IndexMeta meta;
    meta.window_size = opt.window_size; meta.kmer_size = opt.kmer_size; meta.max_fpr = opt.max_fpr;
    {
        std::ifstream in(opt.input_file);
        if (!in) { g_log.error("Error opening file " + opt.input_file); return 1; }
        std::unordered_set<std::string> categories;
        std::string line;
        uint8_t next_bin = 0;
        while (std::getline(in, line)) {
            if (line.empty()) continue;
            const size_t tab = line.find('\t');
            if (tab == std::string::npos) continue;
            const std::string path = make_absolute(line.substr(0, tab));
            std::string name = line.substr(tab + 1);
            const size_t tab2 = name.find('\t');
            if (tab2 != std::string::npos) name.resize(tab2);
            meta.bin_to_category[next_bin] = name;
            categories.insert(name);
            meta.filepath_to_bin.emplace_back(path, next_bin);
            if (next_bin == 255) { g_log.warn("User has reached the maximum number of files which is 255 - ignoring any additional lines!"); break; }
            next_bin++;
        }
        meta.num_bins = next_bin;
        meta.categories.insert(meta.categories.end(), categories.begin(), categories.end());
    }
    if (meta.num_bins == 0) throw std::runtime_error("no 'path<TAB>category' lines in " + opt.input_file);
    g_log.info("Found " + std::to_string(meta.filepath_to_bin.size()) + " files corresponding to " + std::to_string(meta.categories.size()) + " categories");

    // count_and_store_hashes (:118-160) with the minimisers computed on the GPU.  A throw-away 1-bin index object carries k, w.
    chn_index_desc d0;
    std::memset(&d0, 0, sizeof d0);
    d0.struct_size = sizeof d0; d0.device = opt.device; d0.kmer_size = opt.kmer_size; d0.window_size = opt.window_size; d0.hash_funs = opt.num_hash;
    d0.num_categories = 1; d0.host_index = 255; d0.minimiser_seed = 0x8F3F73B5CF1C9ADEULL;
    d0.bins = 1; d0.technical_bins = 64; d0.bin_size = 64; d0.hash_shift = (uint64_t)__builtin_clzll(64ULL); d0.bin_words = 1;
    DeviceSets sets;
    sets.set.assign(meta.num_bins, nullptr); sets.appended.assign(meta.num_bins, 0);
    if (opt.gpu_sets) {
        sets.on = true;
        uint64_t free_bytes = 0, total_bytes = 0;
        CHN_CHECK(chn_device_memory(opt.device, &free_bytes, &total_bytes));
        sets.budget = free_bytes / 2;
        if (const char *e = std::getenv("CHARON_INDEX_SETS_BUDGET")) sets.budget = std::strtoull(e, nullptr, 10);  // test hook
        if (const char *e = std::getenv("CHARON_INDEX_SETS_COMPACT")) sets.compact_at = std::strtoull(e, nullptr, 10);  // test hook
    }
    chn_index *probe_index = nullptr;
    CHN_CHECK(chn_index_create(&d0, &probe_index));
    const uint64_t max_bases = 1ULL << 28;
    const uint32_t chunk = 4096;
    chn_stream_cfg cfg;
    cfg.struct_size = sizeof cfg; cfg.flags = 0; cfg.max_reads = max_bases / chunk + 65536; cfg.max_bases = max_bases;
    chn_stream *stream = nullptr;
    CHN_CHECK(chn_stream_create(probe_index, &cfg, &stream));

    double t_read = 0, t_pack = 0, t_min = 0, t_sort = 0, t_emplace = 0, t_ef = 0, t_mark = omp_get_wtime();
    auto lap = [&](double &acc) { const double now = omp_get_wtime(); acc += now - t_mark; t_mark = now; };
    std::vector<std::vector<uint64_t>> hashes(meta.num_bins);  // distinct minimisers per bin (the reference spills them to <tmp>/<bin>.min)
    for (const auto &fb : meta.filepath_to_bin) {
        const uint8_t bin = fb.second;
        meta.records_per_bin[bin] += 0;
        BlockReader in(fb.first);
        meta.num_files += 1;
        std::vector<uint64_t> &set = hashes[bin];
        uint64_t record_count = 0;
        std::vector<uint64_t> values;
        uint64_t since_unique = 0, distinct = 0;  // of the bin's device set
        if (sets.on) {
            chn_hashset_cfg hc;
            std::memset(&hc, 0, sizeof hc);
            hc.struct_size = sizeof hc; hc.device = opt.device;
            CHN_CHECK(chn_hashset_create(&hc, &sets.set[bin]));
        }
        // two blocks: while the device minimises block i (and the host packs, sorts), a helper thread reads and unwraps block i + 1
        RawBlock blks[2];
        int cur = 0;
        auto fetch = [&in](RawBlock *b) { return in.next(*b, 1u << 20, 64u << 20); };
        bool have = fetch(&blks[0]);
        while (have) {
            RawBlock &blk = blks[cur];
            std::future<bool> following = std::async(std::launch::async, fetch, &blks[cur ^ 1]);
            lap(t_read);
            record_count += blk.recs.size();
            // a chromosome-sized record is handled as pieces of 2^26 bases overlapping by w-1 (same union-of-windows argument
            // as for the 4096-base chunks below), so any record length fits the stream
            std::vector<RecView> pieces;
            uint32_t piece = 1u << 26;
            if (const char *e = std::getenv("CHARON_INDEX_PIECE")) piece = std::max<uint32_t>(4096, (uint32_t)std::strtoul(e, nullptr, 10));  // test hook
            for (const RecView &rv : blk.recs) {
                if (rv.seq_len <= piece + opt.window_size) { pieces.push_back(rv); continue; }
                for (uint64_t st = 0; st + opt.window_size <= rv.seq_len; st += piece) {
                    RecView pv = rv;
                    pv.seq = rv.seq + st;
                    pv.seq_len = (uint32_t)std::min<uint64_t>(rv.seq_len - st, (uint64_t)piece + opt.window_size - 1);
                    pv.qual = nullptr; pv.qual_len = 0;
                    pieces.push_back(pv);
                }
            }
            size_t begin = 0;
            const size_t nrec = pieces.size();
            while (begin < nrec) {  // sub-batches that fit the stream
                uint64_t bases = 0;
                size_t endi = begin;
                // chunks overlap by w-1 bases and every record adds one partial chunk: keep 1/8 of the capacity in reserve
                while (endi < nrec && endi - begin < 60000 && bases + HostBatch::pad64(pieces[endi].seq_len) <= max_bases - max_bases / 8) { bases += HostBatch::pad64(pieces[endi].seq_len); ++endi; }
                if (endi == begin) throw std::runtime_error("internal error: a piece of " + fb.first + " does not fit the stream");
                HostBatch sub;
                sub.blk1.recs.assign(pieces.begin() + (long)begin, pieces.begin() + (long)endi);
                begin = endi;
                sub.pack(false, opt.threads, true);
                lap(t_pack);
                if (sub.keep.empty()) continue;
                // cut every record into chunks of 4096 bases overlapping by w-1: a chunk is created only where a whole window starts,
                // so the union of the chunks' minimisers is exactly the record's minimiser set
                std::vector<uint64_t> coff; std::vector<uint32_t> clen;
                for (size_t i = 0; i < sub.keep.size(); ++i) {
                    const uint64_t L = sub.len1[i], o = sub.off1[i];
                    const uint64_t nwin = L >= opt.window_size ? L - opt.window_size + 1 : 1;
                    const uint64_t nch = (nwin + chunk - 1) / chunk;
                    for (uint64_t c = 0; c < nch; ++c) {
                        const uint64_t st = c * chunk;
                        coff.push_back(o + st);
                        clen.push_back((uint32_t)std::min<uint64_t>(L - st, (uint64_t)chunk + opt.window_size - 1));
                    }
                }
                chn_batch bt;
                std::memset(&bt, 0, sizeof bt);
                bt.struct_size = sizeof bt; bt.n_reads = coff.size(); bt.n_bases = sub.n_bases; bt.bases2 = sub.bases.data();
                bt.nmask = sub.any_n ? sub.nmask.data() : nullptr; bt.seg1_offset = coff.data(); bt.seg1_length = clen.data();
                uint64_t nv = 0;
                if (chn_hashset *hs = sets.set[bin]) {
                    // the batch's minimisers go from the kernel's log into the set, device to device; only their number comes back
                    const int rc = chn_minimisers_into(stream, &bt, hs, &nv);
                    if (rc == CHN_OK) {
                        sets.appended[bin] += nv; since_unique += nv;
                        lap(t_min);
                        if (sets.held_with(hs) > sets.budget) sets.spill(bin, set, "the sets would hold more than the budget of " + std::to_string(sets.budget) + " bytes");
                        else if (since_unique > sets.compact_at) {
                            if (sets.unique(hs, distinct)) { since_unique = 0; lap(t_sort); }
                            else sets.spill(bin, set, "no room to sort its set within the budget of " + std::to_string(sets.budget) + " bytes");
                        }
                        if (!sets.set[bin]) lap(t_min);  // (the download of a spilled set)
                        continue;
                    }
                    if (rc != CHN_E_NOMEM && rc != CHN_E_CAPACITY) throw std::runtime_error(std::string("chn_minimisers_into failed: ") + chn_last_error());
                    // the set is as it was; this batch, too, goes the host's way
                    sets.spill(bin, set, rc == CHN_E_NOMEM ? "the device has no memory for its set" : "its set is full");
                }
                values.resize(sub.n_bases + (uint64_t)opt.window_size * coff.size());
                CHN_CHECK(chn_minimisers(stream, &bt, values.data(), values.size(), &nv));
                set.insert(set.end(), values.begin(), values.begin() + (long)nv);
                lap(t_min);
                if (set.size() > (1u << 26)) { sort_unique(set, opt.threads); lap(t_sort); }
            }
            have = following.get();  // (a parse error of the following block surfaces here)
            cur ^= 1;
        }
        lap(t_read);
        if (chn_hashset *hs = sets.set[bin]) {
            if (sets.unique(hs, distinct)) sets.held_done = sets.held_with(hs);
            else { sets.spill(bin, set, "no room to sort its set within the budget of " + std::to_string(sets.budget) + " bytes"); lap(t_min); }
        }
        if (!sets.set[bin]) { sort_unique(set, opt.threads); distinct = set.size(); }
        lap(t_sort);
        meta.records_per_bin[bin] += record_count;
        meta.hashes_per_bin[bin] += distinct;
        g_log.info("Added file " + fb.first + " with " + std::to_string(record_count) + " records and " + std::to_string(distinct) + " hashes to bin " + std::to_string(bin));
    }
    chn_stream_destroy(stream);
    chn_index_destroy(probe_index);

    // optimize_layout (:162-236)
    std::map<uint8_t, std::vector<uint8_t>> bucket_to_bins;
    if (!opt.optimize) {
        for (unsigned b = 0; b < meta.num_bins; ++b) bucket_to_bins[(uint8_t)b].push_back((uint8_t)b);
    } else {
        g_log.info("Optimize index bin layout");
        std::vector<std::pair<uint8_t, uint64_t>> sorted(meta.hashes_per_bin.begin(), meta.hashes_per_bin.end());
        std::stable_sort(sorted.begin(), sorted.end(), [](const std::pair<uint8_t, uint64_t> &l, const std::pair<uint8_t, uint64_t> &r) { return l.second < r.second; });
        const uint64_t max_num_hashes = sorted.back().second / 2;
        uint8_t next_bin = 0;
        std::map<std::string, uint8_t> last_bin;
        std::map<uint8_t, uint8_t> bin_to_bucket;
        std::map<uint8_t, uint64_t> new_hashes, new_records;
        for (const auto &pr : sorted) {
            const uint8_t bin = pr.first;
            const std::string &category = meta.bin_to_category.at(bin);
            uint8_t assigned = next_bin;
            auto it = last_bin.find(category);
            if (it != last_bin.end()) {
                if (new_hashes[it->second] + pr.second < max_num_hashes) assigned = it->second; else next_bin++;
            } else {
                next_bin++;
            }
            last_bin[category] = assigned;
            bin_to_bucket[bin] = assigned;
            bucket_to_bins[assigned].push_back(bin);
            new_hashes[assigned] += pr.second;
            new_records[assigned] += meta.records_per_bin.at(bin);
        }
        meta.hashes_per_bin = new_hashes; meta.records_per_bin = new_records;
        std::map<uint8_t, std::string> b2c;
        for (auto &fb : meta.filepath_to_bin) { const uint8_t bucket = bin_to_bucket[fb.second]; b2c[bucket] = meta.bin_to_category.at(fb.second); fb.second = bucket; }
        meta.bin_to_category = b2c;
        meta.num_bins = next_bin;
    }

    // build_index (:238-263)
    uint64_t max_hashes = 0;
    for (const auto &kv : meta.hashes_per_bin) max_hashes = std::max(max_hashes, kv.second);
    const uint64_t S = bin_size_in_bits(opt, max_hashes);
    // no reference produced a single minimiser: seqan3's IBF constructor rejects a bin size of 0 ("The size of a bin must be > 0"),
    // which ends the reference with an uncaught exception; fail as loudly here
    if (S == 0) throw std::runtime_error("no minimisers in any input file: the IBF would have a bin size of 0");
    g_log.info("Create new IBF with " + std::to_string(meta.num_bins) + " bins and " + std::to_string(S) + " bits");
    meta.bins = meta.num_bins; meta.bin_words = (meta.bins + 63) / 64; meta.technical_bins = meta.bin_words * 64;
    meta.bin_size = S; meta.hash_shift = (uint64_t)__builtin_clzll(S); meta.hash_funs = opt.num_hash;
    chn_index_desc d;
    std::memset(&d, 0, sizeof d);
    d.struct_size = sizeof d; d.device = opt.device; d.kmer_size = opt.kmer_size; d.window_size = opt.window_size; d.hash_funs = opt.num_hash;
    d.num_categories = (uint8_t)meta.categories.size(); d.host_index = meta.host_category_index(); d.minimiser_seed = 0x8F3F73B5CF1C9ADEULL;
    d.bins = meta.bins; d.technical_bins = meta.technical_bins; d.bin_size = S; d.hash_shift = meta.hash_shift; d.bin_words = meta.bin_words;
    for (uint64_t b = 0; b < meta.bins; ++b) d.bin_to_category[b] = meta.category_index(meta.bin_to_category.at((uint8_t)b));
    chn_index *index = nullptr;
    CHN_CHECK(chn_index_create(&d, &index));
    uint64_t bins_on_device = 0;
    for (const auto &kv : bucket_to_bins)
        for (uint8_t bin : kv.second) {
            if (chn_hashset *hs = sets.set[bin]) {
                bins_on_device += 1;
                CHN_CHECK(chn_index_emplace_set(index, hs, kv.first));
                chn_hashset_destroy(hs);
                sets.set[bin] = nullptr;
                continue;
            }
            CHN_CHECK(chn_index_emplace(index, hashes[bin].data(), hashes[bin].size(), kv.first));
            std::vector<uint64_t>().swap(hashes[bin]);
        }
    if (opt.gpu_sets) {
        uint64_t values_on_device = 0;
        for (uint64_t a : sets.appended) values_on_device += a;
        g_log.info("CHARON_GPU_INDEX_SETS=1: the minimiser sets of " + std::to_string(bins_on_device) + " of " + std::to_string(sets.appended.size()) +
                   " bins stayed on device " + std::to_string(opt.device) + " (" + std::to_string(values_on_device) + " values never crossed to the host)");
    }

    lap(t_emplace);
    // Index(...) compresses the IBF (include/index.hpp:43-50) and store_index writes it (include/store_index.hpp:12-17)
    const int nt_ef = std::max(1, (int)opt.threads);
    EliasFanoWriter ef;
    if (opt.gpu_ef) {
        // CHARON_GPU_INDEX_EF=1: the set bits are counted and the two arrays written on the device, slice of rows by slice of rows; the plain
        // index never comes to the host
        chn_ef_layout lay;
        CHN_CHECK(chn_index_ef_layout(index, &lay));
        ef.begin(lay.m_size, lay.ones);
        if (ef.wl != lay.wl || ef.high_bits != lay.high_bits || ef.high.size() != lay.n_high_words || ef.low.size() != lay.n_low_words + 1)
            throw std::runtime_error("internal error: chn_index_ef_layout and the writer disagree about the Elias-Fano layout");
        chn_ef_encode_job job;
        std::memset(&job, 0, sizeof job);
        job.struct_size = sizeof job; job.layout = &lay;
        if (const char *e = std::getenv("CHARON_INDEX_EF_SLICE")) job.slice_rows = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));  // test hook
        job.low = ef.low.data(); job.n_low_words = lay.n_low_words; job.high = ef.high.data(); job.n_high_words = lay.n_high_words;
        CHN_CHECK(chn_index_encode_ef(index, &job));
        ef.k = lay.ones;
        g_log.info("CHARON_GPU_INDEX_EF=1: the Elias-Fano arrays were encoded on device " + std::to_string(opt.device) + " (" + std::to_string(lay.ones) +
                   " set bits, kernels " + std::to_string(job.device_ms) + " ms)");
    } else {
        const uint64_t W = meta.bin_words, block_rows = std::max<uint64_t>(1, (256ULL << 20) / (8 * W));
        std::vector<uint64_t> block(block_rows * W);
        // both passes over the downloaded rows run on the -t threads: the second one cuts a block into one stretch per thread, counts the
        // set bits of each stretch, and every thread then writes its bits at their final places (a set bit's place in the Elias-Fano arrays
        // depends only on its position and on how many set bits precede it)
        uint64_t ones = 0;
        for (uint64_t r0 = 0; r0 < S; r0 += block_rows) {
            const uint64_t nr = std::min(block_rows, S - r0);
            CHN_CHECK(chn_index_download_rows(index, r0, nr, block.data()));
            uint64_t part = 0;
#pragma omp parallel for num_threads(nt_ef) reduction(+ : part) schedule(static)
            for (long i = 0; i < (long)(nr * W); ++i) part += (uint64_t)__builtin_popcountll(block[(size_t)i]);
            ones += part;
        }
        ef.begin(meta.technical_bins * S, ones);
        uint64_t before = 0;  // set bits in the blocks done
        for (uint64_t r0 = 0; r0 < S; r0 += block_rows) {
            const uint64_t nr = std::min(block_rows, S - r0), nwords = nr * W;
            CHN_CHECK(chn_index_download_rows(index, r0, nr, block.data()));
            before += ef_add_block(ef, block.data(), nwords, r0 * W * 64, before, nt_ef);
        }
        if (before != ones) throw std::runtime_error("internal error: the index changed between the two Elias-Fano passes");
        ef.k = ones;
    }
    chn_index_destroy(index);
    lap(t_ef);
    if (std::getenv("CHARON_TIMING"))
        std::fprintf(stderr, "charon index: timing (s): read %.3f  pack %.3f  minimisers (device + download) %.3f  sort+unique %.3f  layout+emplace %.3f  download + Elias-Fano %.3f\n",
                     t_read, t_pack, t_min, t_sort, t_emplace, t_ef);
    g_log.info("Saving index to file " + opt.prefix);
    BinWriter w(opt.prefix);
    w.pod<uint8_t>(meta.window_size); w.pod<uint8_t>(meta.kmer_size); w.pod<double>(meta.max_fpr);
    w.pod<uint8_t>(meta.num_bins);
    w.pod<uint64_t>(meta.categories.size());
    for (const auto &c : meta.categories) w.str(c);
    w.pod<uint64_t>(meta.filepath_to_bin.size());
    for (const auto &fb : meta.filepath_to_bin) { w.str(fb.first); w.pod<uint8_t>(fb.second); }
    w.pod<uint64_t>(meta.bin_to_category.size());
    for (const auto &kv : meta.bin_to_category) { w.pod<uint8_t>(kv.first); w.str(kv.second); }
    w.pod<uint32_t>(meta.num_files);
    w.pod<uint64_t>(meta.records_per_bin.size());
    for (const auto &kv : meta.records_per_bin) { w.pod<uint8_t>(kv.first); w.pod<uint64_t>(kv.second); }
    w.pod<uint64_t>(meta.hashes_per_bin.size());
    for (const auto &kv : meta.hashes_per_bin) { w.pod<uint8_t>(kv.first); w.pod<uint64_t>(kv.second); }
    w.pod<uint64_t>(meta.bins); w.pod<uint64_t>(meta.technical_bins); w.pod<uint64_t>(meta.bin_size);
    w.pod<uint64_t>(meta.hash_shift); w.pod<uint64_t>(meta.bin_words); w.pod<uint64_t>(meta.hash_funs);
    w.pod<uint64_t>(ef.size); w.pod<uint8_t>(ef.wl);
    w.int_vector(ef.wl ? ef.wl : 1, ef.ones * ef.wl, ef.low);
    w.int_vector(1, ef.high_bits, ef.high);
    // m_high_1_select, m_high_0_select (include/index.hpp:130: archive(ibf_) stores the whole sd_vector)
    for (int bit = 1; bit >= 0; --bit) {
        const std::string blk = selmcl::build(ef.high.data(), ef.high_bits, bit == 1, nt_ef);
        w.os.write(blk.data(), (std::streamsize)blk.size());
    }
    if (!w.os) throw std::runtime_error("writing " + opt.prefix + " failed");
    return 0;
}
