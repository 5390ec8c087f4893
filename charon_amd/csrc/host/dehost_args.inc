// dehost_args.inc -- `charon dehost` arguments and command-line parser (include/dehost_arguments.hpp, src/dehost_main.cpp:208-312)
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a
// stand-alone header.

// ---------------------------------------------------------------------------------------------------
// arguments (include/dehost_arguments.hpp:9-43)
// ---------------------------------------------------------------------------------------------------
struct DehostArguments {
    std::string read_file, read_file2, db, category_to_extract, prefix, dist = "kde", log_file = "charon.log";
    bool is_paired = false, run_extract = false;
    uint8_t chunk_size = 100;
    float lo_hi_threshold = 0.15f;
    uint16_t num_reads_to_fit = 5000;
    float min_quality = 15.0f;
    uint32_t min_length = 140;
    float min_compression = 0.0f;
    uint8_t confidence_threshold = 7;
    float confidence_probability_threshold = 0.0f;
    float host_unique_prop_lo_threshold = 0.05f;
    float min_proportion_difference = 0.04f;
    float min_prob_difference = 0.0f;
    uint8_t threads = 1, verbosity = 0;
    // not in the reference: GPU batching knobs (environment only, so the command line stays identical)
    uint64_t batch_reads = 65536, batch_bases = 1ULL << 30;
    int device = 0;
    // CHARON_DEVICES: one index replica (own copy of the index, own chn_stream, own driver thread) per entry; empty = the single device above
    std::vector<int> devices;
    bool devices_all = false;  // CHARON_DEVICES=all: every visible device (resolved once the HIP runtime is up)
    // CHARON_TEXT_BATCHES=1: reads go to the device as text (chn_text_submit): letters -> codes and the mean quality are formed there
    bool text_batches = false;
    uint8_t min_hits = 0;  // StatsModel::min_hits_ is uninitialised in the reference; CHARON_MIN_HITS overrides
    std::map<uint8_t, std::vector<std::string>> extract_category_to_file;  // include/dehost_arguments.hpp:20
    // `charon classify` (src/classify_main.cpp:24-119, include/classify_arguments.hpp): the same loop with ReadEntry::classify
    // (call_category) for every read and these defaults: dist beta, min_quality 10, min_compression 0.15, confidence 2,
    // min_proportion_diff 0; no --host_unique_prop_lo_threshold / --min_probability_diff options
    bool classify_mode = false;
    void set_classify_defaults() {
        classify_mode = true; dist = "beta"; min_quality = 10.0f; min_length = 140; min_compression = 0.15f; confidence_threshold = 2;
        min_proportion_difference = 0.0f;
    }
};

struct ParseError : std::runtime_error { using std::runtime_error::runtime_error; };

uint64_t parse_uint(const std::string &name, const std::string &v, uint64_t maxv) {
    if (v.empty() || v[0] == '-' || v[0] == '+') throw ParseError("--" + name + ": could not convert '" + v + "' to an unsigned integer");
    errno = 0;
    char *end = nullptr;
    unsigned long long x = std::strtoull(v.c_str(), &end, 10);
    if (errno || *end) throw ParseError("--" + name + ": could not convert '" + v + "'");
    if (x > maxv) throw ParseError("--" + name + ": value " + v + " out of range (max " + std::to_string(maxv) + ")");
    return x;
}
float parse_float(const std::string &name, const std::string &v) {
    errno = 0;
    char *end = nullptr;
    float x = std::strtof(v.c_str(), &end);
    if (v.empty() || errno || *end) throw ParseError("--" + name + ": could not convert '" + v + "' to a number");
    return x;
}

void print_classify_help() {
    std::cout << "Classify read file using index.\n"
                 "Usage: charon classify [OPTIONS] <fastaq> [<fastaq>]\n\n"
                 "Positionals:\n  <fastaq> FILE REQUIRED      Fasta/q file\n  <fastaq> FILE               Paired Fasta/q file\n\n"
                 "Options:\n"
                 "  -h,--help                   Print this help message and exit\n"
                 "  --db FILE REQUIRED          Prefix for the index.\n"
                 "  -e,--extract STRING         Reads from this category in the index will be extracted to file.\n"
                 "  -p,--prefix FILE            Prefix for the output files.\n"
                 "  --chunk_size INT=100        Read file is read in chunks of this size, to be processed in parallel within a chunk.\n"
                 "  --lo_hi_threshold FLOAT=0.15\n"
                 "  --num_reads_to_fit INT=5000 Number of reads to use to train each distribution in the model.\n"
                 "  -d,--dist STRING            Probability distribution to use for modelling.\n"
                 "  --min_quality INT=10        Minimum read quality to classify.\n"
                 "  --min_length INT=140        Minimum read length to classify.\n"
                 "  --min_compression FLOAT=0.15 Minimum read gzip compression ratio to classify.\n"
                 "  --confidence INT=2          Minimum difference between the top 2 unique hit counts.\n"
                 "  --min_proportion_diff FLOAT=0\n"
                 "  --log FILE                  File for log\n"
                 "  -t,--threads INT=1          Maximum number of threads to use.\n"
                 "  -v                          Verbosity of logging. Repeat for increased verbosity\n";
}

void print_dehost_help() {
    std::cout << "Dehost read file into host and other using index.\n"
                 "Usage: charon dehost [OPTIONS] <fastaq> [<fastaq>]\n\n"
                 "Positionals:\n  <fastaq> FILE REQUIRED      Fasta/q file\n  <fastaq> FILE               Paired Fasta/q file\n\n"
                 "Options:\n"
                 "  -h,--help                   Print this help message and exit\n"
                 "  --db FILE REQUIRED          Prefix for the index.\n"
                 "  -e,--extract STRING         Reads from this category in the index will be extracted to file.\n"
                 "  -p,--prefix FILE            Prefix for the output files.\n"
                 "  --chunk_size INT=100        Read file is read in chunks of this size, to be processed in parallel within a chunk.\n"
                 "  --lo_hi_threshold FLOAT=0.15\n"
                 "  --num_reads_to_fit INT=5000 Number of reads to use to train each distribution in the model.\n"
                 "  -d,--dist STRING            Probability distribution to use for modelling.\n"
                 "  --min_length INT=140        Minimum read length to classify.\n"
                 "  --min_quality INT=15        Minimum read quality to classify.\n"
                 "  --min_compression FLOAT=0   Minimum read gzip compression ratio to classify.\n"
                 "  --confidence INT=7          Minimum difference between the top 2 unique hit counts.\n"
                 "  --host_unique_prop_lo_threshold INT=0.05\n"
                 "  --min_proportion_diff FLOAT=0.04\n"
                 "  --min_probability_diff FLOAT=0\n"
                 "  --log FILE                  File for log\n"
                 "  -t,--threads INT=1          Maximum number of threads to use.\n"
                 "  -v                          Verbosity of logging. Repeat for increased verbosity\n";
}

// returns false if help was printed
bool parse_dehost(int argc, char **argv, DehostArguments &opt) {
    std::vector<std::string> pos;
    bool have_db = false;
    for (int i = 0; i < argc; ++i) {
        std::string a = argv[i];
        std::string val;
        bool has_val = false;
        if (a.size() > 2 && a[0] == '-' && a[1] == '-') {
            size_t eq = a.find('=');
            if (eq != std::string::npos) { val = a.substr(eq + 1); a = a.substr(0, eq); has_val = true; }
        } else if (a.size() > 2 && a[0] == '-' && a[1] != '-' && (a[1] == 't' || a[1] == 'e' || a[1] == 'p' || a[1] == 'd')) {
            val = a.substr(2); a = a.substr(0, 2); has_val = true;  // -t4
            if (!val.empty() && val[0] == '=') val = val.substr(1);
        }
        auto need = [&]() -> std::string {
            if (has_val) return val;
            if (i + 1 >= argc) throw ParseError(a + ": 1 required");
            return argv[++i];
        };
        if (a == "-h" || a == "--help") { if (opt.classify_mode) print_classify_help(); else print_dehost_help(); return false; }
        else if (a == "--db") { opt.db = need(); have_db = true; }
        else if (a == "-e" || a == "--extract") opt.category_to_extract = need();
        else if (a == "-p" || a == "--prefix") opt.prefix = need();
        else if (a == "--chunk_size") opt.chunk_size = (uint8_t)parse_uint("chunk_size", need(), 255);
        else if (a == "--lo_hi_threshold") opt.lo_hi_threshold = parse_float("lo_hi_threshold", need());
        else if (a == "--num_reads_to_fit") opt.num_reads_to_fit = (uint16_t)parse_uint("num_reads_to_fit", need(), 65535);
        else if (a == "-d" || a == "--dist") opt.dist = need();
        else if (a == "--min_length") opt.min_length = (uint32_t)parse_uint("min_length", need(), 4294967295ULL);
        else if (a == "--min_quality") opt.min_quality = parse_float("min_quality", need());
        else if (a == "--min_compression") opt.min_compression = parse_float("min_compression", need());
        else if (a == "--confidence") opt.confidence_threshold = (uint8_t)parse_uint("confidence", need(), 255);
        else if (a == "--host_unique_prop_lo_threshold" && !opt.classify_mode) opt.host_unique_prop_lo_threshold = parse_float("host_unique_prop_lo_threshold", need());
        else if (a == "--min_proportion_diff") opt.min_proportion_difference = parse_float("min_proportion_diff", need());
        else if (a == "--min_probability_diff" && !opt.classify_mode) opt.min_prob_difference = parse_float("min_probability_diff", need());
        else if (a == "--log") opt.log_file = need();
        else if (a == "-t" || a == "--threads") opt.threads = (uint8_t)parse_uint("threads", need(), 255);
        else if (a.size() >= 2 && a[0] == '-' && a.find_first_not_of('v', 1) == std::string::npos) opt.verbosity = (uint8_t)std::min<size_t>(255, opt.verbosity + a.size() - 1);
        else if (!a.empty() && a[0] == '-' && a.size() > 1) throw ParseError("The following argument was not expected: " + a);
        else pos.push_back(a);
    }
    if (pos.empty()) throw ParseError("<fastaq> is required");
    if (pos.size() > 2) throw ParseError("The following argument was not expected: " + pos[2]);
    if (!have_db) throw ParseError("--db is required");
    for (auto &p : pos) if (!is_file(p)) throw ParseError("<fastaq>: File does not exist: " + p);
    if (!path_exists(opt.db)) throw ParseError("--db: Path does not exist: " + opt.db);               // CLI::ExistingPath
    if (!opt.prefix.empty() && path_exists(opt.prefix)) throw ParseError("--prefix: Path already exists: " + opt.prefix);  // NonexistentPath
    opt.read_file = pos[0];
    if (pos.size() > 1) opt.read_file2 = pos[1];
    return true;
}

// CHARON_DEVICES: "all" or a comma list of device ordinals ("0,1,3"; a repeated ordinal is a second replica on that device).  Returns an
// error message, empty if the value is well formed.
std::string parse_device_list(const std::string &v, DehostArguments &opt) {
    opt.devices.clear();
    opt.devices_all = false;
    if (v == "all") { opt.devices_all = true; return ""; }
    size_t at = 0;
    for (;;) {
        const size_t comma = v.find(',', at);
        const std::string item = v.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
        if (item.empty()) return "empty entry in '" + v + "' (expected 'all' or a comma list of device ordinals such as 0,1,3)";
        if (item.size() > 9 || item.find_first_not_of("0123456789") != std::string::npos)
            return "'" + item + "' is not a device ordinal (expected 'all' or a comma list of non-negative integers such as 0,1,3)";
        if (opt.devices.size() == 64) return "more than 64 entries";
        opt.devices.push_back(std::atoi(item.c_str()));
        if (comma == std::string::npos) break;
        at = comma + 1;
    }
    return "";
}
