// dehost_loop.inc -- what the main thread of `charon dehost` holds while it reads, and the read loop over the host reader's blocks
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a stand-alone header.

typedef RowWriter<Flight> Writer;
typedef ReplicaSet<Flight, chn_stream *> Replicas;

// The ids of a pair differ after dropping their last characters (src/dehost_main.cpp:423-430): the two ids behind the rows printed so
// far, and the end the reference's uncaught exception gives.  The caller has drained whatever still had rows to print.
[[noreturn]] void pairs_do_not_match(const char *id1, size_t len1, const char *id2, size_t len2) {
    std::cout.flush();
    std::cout << std::string(id1, len1) << " " << std::string(id2, len2);
    std::cout.flush();
    std::fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n  what():  Your pairs don't match for read ids.\n");
    std::abort();
}

// The stages as the main thread's two read loops (this one and ResidentLoop) see them, and the main thread's own timers.
// Only the main thread touches this object.
struct MainThread {
    const DehostArguments &opt;
    const PackPlan &plan;
    chn_stream *const stream;  // stream 0
    const size_t C;            // categories
    Result &result;
    FlightPool<Flight> &pool;
    RowStage &rows;
    Writer &writer;
    Replicas &replicas;
    TextBatchCounts &text_counts;
    // CHARON_TIMING=1: wall seconds per phase of the main thread, to the log (where does the CLI's time go?)
    double t_pop = 0, t_pack = 0, t_submit = 0, t_wait = 0, t_fetch = 0;
    bool final_pushed = false;  // the final models are on stream 0

    // A flight on stream 0 from this thread -- every batch while the models train (they may change with every read added, so the caller
    // retires it before the next is submitted) and every batch of the device-resident loop: the models as they are now on the device,
    // the flight marked with their version, counted on replica 0.
    void submit_here(Flight &fl) {
        if (!final_pushed) { result.ensure_device_model(); final_pushed = result.models_final(); }
        fl.version = result.current_model_version();
        const double tk = now();
        submit_flight(opt, text_counts, stream, fl);
        t_submit += now() - tk;
        replicas.count(0, fl.reads());
    }
    void wait_here(Flight &fl) { wait_flight(opt, C, stream, fl, t_wait); }
    // the final models on every replica's stream (replica 0's may lag behind the last change in training), then the replica threads
    void start_replicas() {
        std::vector<uint32_t> version(replicas.size());
        result.ensure_device_model();
        version[0] = result.current_model_version();
        for (size_t r = 1; r < replicas.size(); ++r) version[r] = result.push_model_to_device(replicas.at(r).stream);
        replicas.start(version);
    }
};

// The read loop over the host reader's blocks, to the end of the input: every block cut into GPU batches that respect the stream's
// capacity; batch i + 1 is packed while the GPU works on batch i.
void run_host_loop(MainThread &mt, BlockQueue &queue) {
    const DehostArguments &opt = mt.opt;
    for (;;) {
        const double tp = now();
        std::shared_ptr<HostBatch> hbp = queue.pop();
        mt.t_pop += now() - tp;
        if (!hbp) break;
        HostBatch &hb = *hbp;
        const size_t nrec = hb.blk1.recs.size();
        if (opt.is_paired) {
            for (size_t i = 0; i < nrec; ++i) {  // pair ids must agree after dropping the last character (:423-430)
                const RecView &a = hb.blk1.recs[i], &b = hb.blk2.recs[i];
                const uint32_t la = a.id_len ? a.id_len - 1 : 0, lb = b.id_len ? b.id_len - 1 : 0;
                if (la != lb || std::memcmp(a.id, b.id, la) != 0) {
                    if (mt.replicas.dealing()) mt.replicas.drain();
                    mt.writer.drain();
                    pairs_do_not_match(a.id, la, b.id, lb);
                }
            }
        }
        size_t begin = 0;
        while (begin < nrec) {
            const size_t endi = cut_batch(opt, begin, nrec, [&](size_t i) {
                return HostBatch::pad64(hb.blk1.recs[i].seq_len) + (opt.is_paired ? HostBatch::pad64(hb.blk2.recs[i].seq_len) : 0);
            });
            if (mt.replicas.dealing()) mt.replicas.release_ready();
            std::unique_ptr<Flight> fl = mt.pool.take();
            fl->parent = hbp;
            fl->resident = false;
            HostBatch &sub = fl->sub;
            sub.bases.want_pinned = sub.nmask.want_pinned = true;  // three of these go round: uploads straight out of them
            sub.blk1.recs.assign(hb.blk1.recs.begin() + (long)begin, hb.blk1.recs.begin() + (long)endi);
            if (opt.is_paired) sub.blk2.recs.assign(hb.blk2.recs.begin() + (long)begin, hb.blk2.recs.begin() + (long)endi);
            begin = endi;
            const double tk = now();
            sub.pack(opt.is_paired, opt.threads, mt.plan.skip_compression, mt.plan.gz_gpu_max, mt.plan.gz_route_long, opt.text_batches,
                     (!opt.is_paired && !hb.blk1.map_begin) ? &hb.blk1.buf : nullptr);
            mt.t_pack += now() - tk;
            if (sub.keep.empty()) continue;
            if (mt.result.models_final()) {
                // (nothing is in flight on replica 0 when the models become final: every training batch is retired before the next)
                if (!mt.replicas.dealing()) mt.start_replicas();
                fl->version = mt.result.current_model_version();
                mt.replicas.deal(fl);
                mt.replicas.release_ready();
                continue;
            }
            mt.submit_here(*fl);
            mt.wait_here(*fl);
            mt.writer.hand_on(fl);
        }
    }
    if (mt.replicas.dealing()) mt.replicas.close();
    mt.writer.drain();
}
