// dehost_readers.inc -- the reader threads of `charon dehost`: the host reader (whole-record blocks) and the side readers of the
// device-resident loop (blocks of text in device memory)
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a stand-alone header.

// The host reader parses whole-record blocks while the previous batch is packed / compressed / classified / printed.  Its thread reaches
// this object and the options (read-only) and nothing else; the main thread reaches `queue`, and the rest only while no thread runs
// (resume_from before start; in1 / in2 after the join).
struct HostReader {
    BlockQueue queue;
    // the readers outlive the reader thread: records of a mapped file are views into the mapping until their rows are printed
    std::unique_ptr<BlockReader> in1, in2;
    // the device-resident loop was left: file k goes on at compressed offset resume_z[k] with resume_carry[k] in front
    bool resumed[2] = {false, false};
    size_t resume_z[2] = {0, 0};
    Slab resume_carry[2];
    std::thread t;

    void start(const DehostArguments &opt) { t = std::thread(&HostReader::body, this, std::cref(opt)); }
    // stop the reader and wait for it (nothing to do if it never ran, or has been joined)
    void abort_and_join() { if (t.joinable()) { queue.abort(); t.join(); } }

private:
    void body(const DehostArguments &opt) {
        try {
            in1.reset(new BlockReader(opt.read_file));
            if (opt.is_paired) in2.reset(new BlockReader(opt.read_file2));
            const size_t max_bytes = (size_t)std::min<uint64_t>(256ULL << 20, std::max<uint64_t>(1 << 20, opt.batch_bases));
            if (resumed[0]) in1->resume(resume_z[0], resume_carry[0]);
            if (resumed[1]) in2->resume(resume_z[1], resume_carry[1]);
            for (;;) {
                std::shared_ptr<HostBatch> hb(new HostBatch());
                // a batch may hold at most batch_bases padded bases: bound the record count by the byte budget as well
                if (!in1->next(hb->blk1, opt.batch_reads, max_bytes)) break;
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
    }
};

// CHARON_GPU_TEXT=1: while the run is device-resident, each of its files (one, or with CHARON_GPU_TEXT_PAIRS=1 the two of a pair) has a
// reader thread and a queue of its own, each with its own BlockReader, hence its own BgzfSource and inflate handle, which hand over
// blocks of text in device memory.  The host reader is then started only when the main thread leaves the mode.
struct SideReader {
    BlockQueue queue;
    std::thread t;

    void start(const std::string &file, size_t block_bytes, size_t headroom) { t = std::thread(&SideReader::body, this, file, block_bytes, headroom); }
    void abort_and_join() { if (t.joinable()) { queue.abort(); t.join(); } }

private:
    void body(std::string file, size_t block_bytes, size_t headroom) {
        try {
            BlockReader in(file);
            for (;;) {
                std::shared_ptr<HostBatch> hb(new HostBatch());
                hb->dtext = in.next_device(block_bytes, headroom);
                if (!hb->dtext) break;
                if (!queue.push(std::move(hb))) return;
            }
            queue.finish("");
        } catch (std::exception &e) {
            queue.finish(e.what());
        }
    }
};
