// dehost.inc -- dehost_main (src/dehost_main.cpp:314-550): the driver over the stages in dehost_*.inc
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a stand-alone header.

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

// CHARON_TIMING=1: where the run's time went, stage by stage
void report_timing(const RunModes &modes, const DeviceSetup &setup, const MainThread &mt, const RowStage &rows, const ResidentLoop &resident, double t_entry) {
    timing_line("timing (main thread, s): wait-for-reader %.3f  pack %.3f  submit %.3f  wait-for-gpu %.3f  tallies->sizes %.3f  rows %.3f",
                mt.t_pop, mt.t_pack, mt.t_submit, mt.t_wait, rows.t_gz, rows.t_rows);
    timing_line("timing (reader thread, s): inflate %.3f  record splitting %.3f", g_reader_fill_s, g_reader_parse_s);
    if (g_gpu_inflate) timing_line("timing (reader thread, s): inside chn_inflate_run %.3f (part of inflate)", g_gpu_inflate_s);
    if (modes.n_sides)
        timing_line("timing (CHARON_GPU_TEXT=1): records split %llu  records fetched %llu  text bytes inflated %llu  text bytes fetched %llu  "
                    "seconds in inflate %.3f  seconds in split %.3f  seconds in fetch %.3f",
                    (unsigned long long)resident.dt_split_records, (unsigned long long)rows.dt_fetched_records, (unsigned long long)g_gpu_text_inflated,
                    (unsigned long long)rows.dt_fetched_bytes, g_gpu_inflate_s, resident.t_split, mt.t_fetch);
    if (modes.n_sides == 2)
        timing_line("timing (CHARON_GPU_TEXT_PAIRS=1): pairs checked %llu  id bytes of file 2 downloaded %llu  seconds in pair check %.3f",
                    (unsigned long long)resident.dp_pairs_checked, (unsigned long long)rows.dp_id2_bytes, resident.t_pair);
    if (g_gpu_deflate) timing_line("timing (main thread, s): inside chn_deflate_run %.3f (extract files)", g_gpu_deflate_s);
    if (g_gpu_extract)
        timing_line("timing (CHARON_GPU_EXTRACT=1): records formed on the device %llu  bytes appended from the host %llu  compressed bytes down %llu  "
                    "seconds in chn_extract calls %.3f", (unsigned long long)g_gpu_extract_records, (unsigned long long)g_gpu_extract_host_bytes,
                    (unsigned long long)g_gpu_extract_down, g_gpu_extract_s);
    timing_line("timing (start-up, s): index file read %.3f  device + index create %.3f  index decode, stream, models %.3f (of which reference self-check %.3f)  read loop %.3f",
                setup.t_meta - t_entry, setup.t_hip - setup.t_meta, setup.t_ready - setup.t_hip, setup.t_ready - setup.t_sc0, now() - setup.t_ready);
    timing_line("timing (index decode, s): select blocks checked %.3f  page-locked staging %.3f  slices staged %.3f  waited for the device %.3f  bin popcounts %.3f",
                setup.file.t_verify, setup.file.t_stage_alloc, setup.file.t_stage_fill, setup.file.t_device_wait, setup.file.t_popcounts);
}

// what every run says of its batches at the end, to the log
void report_counts(const DehostArguments &opt, const PackPlan &plan, const Replicas &replicas, const TextBatchCounts &text_counts, const RowStage &rows, bool timing) {
    for (size_t r = 0; r < replicas.size(); ++r) {
        const Replicas::Replica &rp = replicas.at(r);
        g_log.info("replica " + std::to_string(rp.index) + " (device " + std::to_string(rp.device) + "): " + std::to_string(rp.batches) + " batches, " +
                   std::to_string(rp.reads) + " reads");
        if (timing && replicas.dealing())
            timing_line("timing (replica %zu, device %d, s): submit %.3f  wait-for-gpu %.3f", rp.index, rp.device, rp.t_submit, rp.t_wait);
    }
    if (opt.text_batches)
        g_log.info("text batches: " + std::to_string(text_counts.slab.load()) + " sent as the block's slab, " + std::to_string(text_counts.copy.load()) +
                   " as a page-locked copy of letters and qualities");
    if (plan.gz_gpu_max) g_log.info("gzip column: " + std::to_string(rows.gz_on_device) + " reads sized from device deflate tallies (the rest on the host)");
    if (plan.gz_gpu_max) g_log.info("gzip column: " + std::to_string(rows.gz_long_on_device) + " reads beyond " + std::to_string(CHN_GZIP_MAX_LEN) + " letters sized by the device's long-read deflate pass");
}

int dehost_main(DehostArguments &opt) {
    const double t_entry = now();
    g_log.open(opt.log_file, opt.verbosity);
    g_reader_threads = reader_threads_for(opt.threads, looks_compressed(opt.read_file) || (!opt.read_file2.empty() && looks_compressed(opt.read_file2)));
    if (!ends_with(opt.db, ".idx")) opt.db += ".idx";                 // src/dehost_main.cpp:489-491
    if (!opt.read_file2.empty()) { opt.is_paired = true; opt.min_length = 80; }  // :493-496
    g_log.info(std::string(opt.classify_mode ? "Running charon classify\n\nCharon version: " : "Running charon dehost\n\nCharon version: ") + CHARON_VERSION);

    // WHAT IS STOPPED IN WHICH ORDER when this function is left -- by its normal return, by `return 1` before the loop, or by an exception
    // at any point.  Everything below is a local of this function, so it goes in the reverse order of the declarations, each only if
    // it exists by then:
    //   1. `replicas`: the replica threads are told to stop and joined (a thread with flights flying syncs its stream first).
    //   2. `writer`: the row writer's thread writes what is queued and is joined; then the flights in its queue, then `pool`'s, are freed.
    //   3. `result` (the extract files are closed).
    //   4. `setup`: the streams of replicas 1.., then their indexes; the select-block check is joined; the index file is let go.
    //      (Stream 0 and index 0: setup.destroy_first(), on the normal return alone.)
    //   5. warm_join: the thread that brings the HIP runtime up.
    //   6. side_reader_join1, side_reader_join0, reader_join: each reader's queue is aborted and its thread joined; then the readers.
    //   7. dev_text_pool_drain, slab_pool_drain: the device buffers and page-locked slabs left in the pools are released -- after
    //      everything that hands one back, while the HIP runtime is certainly still up.
    // An exception inside the read loop is caught there first: the host reader's queue is aborted, the replicas stopped, the reader joined.
    auto slab_pool_drain = scope_exit([] { std::lock_guard<std::mutex> lk(g_slab_pool.m); g_slab_pool.v.clear(); });
    auto dev_text_pool_drain = scope_exit([] { g_dev_text_pool.drain(); });
    const RunModes modes = resolve_run_modes(opt);
    // The readers start before the device is touched, so the first block is parsed while the HIP runtime initialises and the index is decoded.
    HostReader reader;
    SideReader side_reader[2];
    for (int k = 0; k < modes.n_sides; ++k) side_reader[k].start(k ? opt.read_file2 : opt.read_file, modes.resident_block_bytes, g_gpu_text_headroom);
    if (!modes.n_sides) reader.start(opt);
    auto reader_join = scope_exit([&reader] { reader.abort_and_join(); });
    auto side_reader_join0 = scope_exit([&side_reader] { side_reader[0].abort_and_join(); });
    auto side_reader_join1 = scope_exit([&side_reader] { side_reader[1].abort_and_join(); });
    // the HIP runtime takes 0.1-0.2 s to come up: let it do so while this thread reads the index file
    std::thread warm([]() { void *p = nullptr; if (chn_host_alloc(64, &p) == CHN_OK) chn_host_free(p); });
    auto warm_join = scope_exit([&warm] { if (warm.joinable()) warm.join(); });

    DeviceSetup setup(opt);
    if (!settle_outputs(opt, setup.meta)) return 1;
    setup.load(opt, warm, modes.n_sides != 0);

    std::ios::sync_with_stdio(false);
    Result result(setup.meta, opt, setup.stream[0], setup.model, std::cout);
    result.push_initial_model();
    g_log.info(std::string(opt.classify_mode ? "Classifying file " : "Dehosting file ") + opt.read_file + (opt.is_paired ? " and " + opt.read_file2 : ""));

    const PackPlan plan(opt);
    const bool timing = std::getenv("CHARON_TIMING") != nullptr;
    const size_t C = setup.meta.categories.size();
    FlightPool<Flight> pool;
    RowStage rows(opt, setup.meta, result, setup.stream[0]);
    TextBatchCounts text_counts;
    // (with as many -t threads as the process has CPUs the reader's, the packing and the formatting teams already take every core: a row writer
    //  beside them only adds contention -- -t 16 on a 16-CPU share: 1.67 instead of 1.89 M reads/s.  CHARON_ROW_WRITER=0 / 1 overrides.)
    bool use_row_writer = 2 * (int)opt.threads <= usable_cpus();
    if (const char *e = std::getenv("CHARON_ROW_WRITER")) use_row_writer = std::atoi(e) != 0;
    // (what the writer's thread may reach, and why this predicate makes that safe: row_writer.inc)
    Writer writer([&rows](Flight &f) { rows.finish_rows(f); }, [&pool](std::unique_ptr<Flight> &f) { pool.recycle(f); },
                  [&result, &opt, use_row_writer](const Flight &f) {
                      return use_row_writer && !opt.run_extract && result.models_final() && result.current_model_version() == f.version;
                  });
    Replicas replicas(setup.devices, setup.stream,
                      [&opt, &text_counts](chn_stream *st, Flight &f) { submit_flight(opt, text_counts, st, f); },
                      [&opt, C](chn_stream *st, Flight &f, double &acc_wait) { wait_flight(opt, C, st, f, acc_wait); },
                      [](chn_stream *st) { (void)chn_stream_sync(st); },
                      [&writer](std::unique_ptr<Flight> &f) { writer.hand_on(f); });
    MainThread mt{opt, plan, setup.stream[0], C, result, pool, rows, writer, replicas, text_counts};
    ResidentLoop resident(mt, modes, side_reader, reader);

    std::string failure;
    try {
        if (modes.n_sides) resident.run();
        run_host_loop(mt, reader.queue);
        if (!reader.queue.error.empty()) failure = reader.queue.error;
    } catch (std::exception &e) {
        failure = e.what();
        reader.queue.abort();  // the reader thread stops at its next block
        replicas.stop();
    }
    if (reader.t.joinable()) reader.t.join();
    if (!failure.empty()) { std::cout.flush(); throw std::runtime_error(failure); }
    result.complete();
    std::cout.flush();
    if (timing) report_timing(modes, setup, mt, rows, resident, t_entry);
    report_counts(opt, plan, replicas, text_counts, rows, timing);
    result.print_summary();
    // the process is about to exit: unmapping gigabytes of read file page by page is time nobody needs
    (void)reader.in1.release(); (void)reader.in2.release();
    const double t_tear = now();
    setup.destroy_first();
    if (timing) {
        const double wall = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
        std::fprintf(stderr, "charon: timing (tear-down, s): stream + index destroy %.3f; dehost_main %.3f in all, returning at wall clock %.3f\n", now() - t_tear, now() - t_entry, wall);
    }
    return 0;
}
