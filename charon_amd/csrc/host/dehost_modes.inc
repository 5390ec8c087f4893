// dehost_modes.inc -- which of the CHARON_GPU_* / CHARON_TEXT_BATCHES switches apply to this run's inputs, with the log line of each
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a stand-alone header.

struct RunModes {
    // CHARON_GPU_TEXT=1: no side, one (single-end input) or two (CHARON_GPU_TEXT_PAIRS=1 and a pair of files) stay in device memory
    int n_sides = 0;
    bool fasta_side = false;  // CHARON_GPU_TEXT_FASTA=1 took the input: the one side is a FASTA file
    // A device block is 64 MiB of text (a thousand members per chn_inflate_run: four wavefronts for each of the device's 256 CUs, and
    // some 13 000 reads of 5 kb per chn_text_split) instead of the 256 MB of a slab.
    // (CHARON_GPU_TEXT_BLOCK: test hook, a smaller block -- down to one BGZF member's 64 KiB)
    size_t resident_block_bytes = 0;
};

// why the device-resident loop cannot take `f` as BGZF FASTQ (or, `fasta`, as BGZF FASTA: by name, as BlockReader decides it); empty: it can
std::string not_resident_because(const std::string &f, bool fasta) {
    const std::string stem = f.substr(0, f.size() - std::min<size_t>(3, f.size()));
    if (!ends_with(f, ".gz")) return "not a .gz file";
    if (std::getenv("CHARON_NO_BGZF")) return "CHARON_NO_BGZF is set";
    bool named = false;
    if (fasta) { for (const char *x : {".fasta", ".fa", ".fna", ".ffn", ".faa", ".frn", ".fas"}) named = named || ends_with(stem, x); }
    else named = ends_with(stem, ".fastq") || ends_with(stem, ".fq");
    if (!named) return fasta ? "not FASTA" : "not FASTQ";
    if (!BgzfSource().open(f)) return "one deflate stream, not BGZF";
    return "";
}

// Settles the switches in the order their log lines have always come.  Sets the globals the reader and Result go by: g_gzip_emulator,
// g_pin_slabs, g_gpu_text_headroom, the device text pool's keep, and g_gpu_extract (cleared where it does not apply).
RunModes resolve_run_modes(const DehostArguments &opt) {
    RunModes modes;
    if (std::getenv("CHARON_ZLIB_ONLY")) g_gzip_emulator = false;
    else if (!gzip_emulator_self_check()) {
        g_gzip_emulator = false;
        g_log.warn(std::string("gzip size emulator disagrees with the linked zlib ") + zlibVersion() + "; using zlib for the compression column");
    }
    // CHARON_TEXT_BATCHES=1: slabs are page-locked from the first one on (the reader thread allocates them)
    g_pin_slabs = opt.text_batches || g_gpu_inflate;  // (CHARON_GPU_INFLATE=1 downloads straight into the slab)
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
    modes.resident_block_bytes = std::min<size_t>((size_t)std::min<uint64_t>(256ULL << 20, std::max<uint64_t>(1 << 20, opt.batch_bases)), (size_t)64 << 20);
    if (const char *e = std::getenv("CHARON_GPU_TEXT_BLOCK")) modes.resident_block_bytes = (size_t)std::min<unsigned long long>(modes.resident_block_bytes, std::max<unsigned long long>(65536, std::strtoull(e, nullptr, 10)));
    if (g_gpu_text) {
        bool two = false;
        if (g_gpu_text_pairs && !opt.is_paired)
            g_log.info("CHARON_GPU_TEXT_PAIRS=1 does not apply to " + opt.read_file + " (single-end input): CHARON_GPU_TEXT=1 alone decides");
        if (g_gpu_text_pairs && opt.is_paired) {
            std::string why = not_resident_because(opt.read_file, false), file = opt.read_file;
            if (why.empty()) { why = not_resident_because(opt.read_file2, false); file = opt.read_file2; }
            two = why.empty();
            if (!two) g_log.info("CHARON_GPU_TEXT_PAIRS=1 does not apply to " + file + " (" + why + "; both files must be BGZF FASTQ): the run goes on without it");
        }
        std::string why = two ? "" : opt.is_paired ? "paired input" : not_resident_because(opt.read_file, false);
        if (g_gpu_text_fasta) {
            const std::string fwhy = opt.is_paired ? "paired input" : not_resident_because(opt.read_file, true);
            modes.fasta_side = fwhy.empty();
            if (modes.fasta_side) why.clear();
            else g_log.info("CHARON_GPU_TEXT_FASTA=1 does not apply to " + opt.read_file + " (" + fwhy + "; single-end BGZF FASTA only): the run goes on as under CHARON_GPU_TEXT=1 alone");
        }
        if (why.empty()) {
            modes.n_sides = two ? 2 : 1;
            if (const char *e = std::getenv("CHARON_GPU_TEXT_HEADROOM")) g_gpu_text_headroom = (size_t)std::min<unsigned long long>(1ULL << 30, std::strtoull(e, nullptr, 10));
            // Device buffers: each side's reader fills one while two wait in its queue, the main thread holds one per side and up to two
            // batches in flight refer to one per side -- at most seven exist per side; of a pair's fourteen, eight free ones are kept.
            if (two || modes.fasta_side) g_dev_text_pool.keep = 8;
            g_log.info("CHARON_GPU_TEXT=1: BGZF text is inflated into the memory of device " + std::to_string(g_gpu_text_device) +
                       " and stays there (records split and packed on the device; headroom " + std::to_string(g_gpu_text_headroom) + " bytes)");
            if (modes.fasta_side) g_log.info("CHARON_GPU_TEXT_FASTA=1: FASTA records are found and unwrapped on the device (a second buffer per block holds the letters)");
            if (two) g_log.info("CHARON_GPU_TEXT_PAIRS=1: both files of the pair stay in device memory (two texts a batch; the ids of a pair are compared on the device)");
        } else {
            g_log.info("CHARON_GPU_TEXT=1 does not apply to " + opt.read_file + " (" + why + "; single-end BGZF FASTQ only): the run goes on without it");
        }
    }
    if (g_gpu_extract) {
        const char *why = opt.category_to_extract.empty() ? "does nothing without --extract"
                          : !modes.n_sides ? "does not apply (the input is not taken by the device-resident loop of CHARON_GPU_TEXT=1)"
                          : modes.fasta_side ? "does not apply (FASTA input: extract records are formed on the device for FASTQ only)" : nullptr;
        if (why) g_log.info(std::string("CHARON_GPU_EXTRACT=1 ") + why + ": the run goes on without it");
        else g_log.info("CHARON_GPU_EXTRACT=1: the records of the extract files are formed and compressed in the memory of device " + std::to_string(g_gpu_text_device));
        g_gpu_extract = why == nullptr;
    }
    return modes;
}
