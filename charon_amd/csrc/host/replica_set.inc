// replica_set.inc -- CHARON_DEVICES: packed batches dealt round-robin to one thread per index replica, and back in input order
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order; behind run_util.inc and
// ordered_merge.inc); not a stand-alone header.

// Replica mode, once the models are final (before that every batch runs on replica 0, retired one by one: the models may change with
// every read).  The main thread reads, splits and packs as before and deals the packed batches round-robin, numbered in input order;
// each replica's thread submits them on its own stream and waits for them, and the ordered merge hands them back to `on_release` (the
// row writer's door) strictly in input order.  One replica (CHARON_DEVICES unset) is the same loop with N = 1.
//
// Who touches what.  A replica's thread: its Replica (under Replica::m where the main thread writes too: in, need, closing, stop), the
// flights it holds, and the two callables submit(stream, F &) and wait(stream, F &, seconds) -- which therefore must reach nothing but
// the flight, the stream and read-only options.  The main thread: everything else, `outstanding` and on_release included.
// F has version, seq and reads(); S is the stream handle.  Neither Result nor HIP is known here.
template <class F, class S>
class ReplicaSet {
public:
    typedef std::unique_ptr<F> Ptr;
    static const size_t kMaxOutstanding = 3;  // flights per replica between dealing and release (the writer holds two more)
    struct Replica {
        size_t index = 0;
        int device = 0;
        S stream = S();
        uint32_t model_version = 0;   // the models on its stream (every flight it submits must have been packed for them)
        std::mutex m;
        std::condition_variable cv;
        std::deque<Ptr> in;           // dealt, not yet submitted
        uint64_t need = 0;            // flights up to this sequence number are wanted back (need_set: any)
        bool need_set = false, closing = false, stop = false;
        size_t outstanding = 0;       // main thread: dealt and not yet released by the merge
        uint64_t batches = 0, reads = 0;
        double t_submit = 0, t_wait = 0;
        std::thread t;
    };

    // sync(stream): the stream is done with everything submitted on it (a replica thread that stops with flights still flying calls it
    // before they are freed)
    ReplicaSet(const std::vector<int> &devices, const std::vector<S> &streams, std::function<void(S, F &)> submit,
               std::function<void(S, F &, double &)> wait, std::function<void(S)> sync, std::function<void(Ptr &)> on_release)
        : submit_(std::move(submit)), wait_(std::move(wait)), sync_(std::move(sync)), on_release_(std::move(on_release)) {
        for (size_t r = 0; r < devices.size(); ++r) {
            reps_.emplace_back(new Replica());
            reps_[r]->index = r; reps_[r]->device = devices[r]; reps_[r]->stream = streams[r];
        }
    }
    ReplicaSet(const ReplicaSet &) = delete;
    ReplicaSet &operator=(const ReplicaSet &) = delete;
    ~ReplicaSet() { stop(); }

    size_t size() const { return reps_.size(); }
    const Replica &at(size_t r) const { return *reps_[r]; }
    bool dealing() const { return dealing_; }  // the replica threads run
    // a batch the main thread submitted itself on replica r's stream (training; the device-resident loop)
    void count(size_t r, size_t reads) { reps_[r]->batches += 1; reps_[r]->reads += reads; }

    // the replica threads; model_version[r]: the models the caller has put on replica r's stream
    void start(const std::vector<uint32_t> &model_version) {
        for (size_t r = 0; r < reps_.size(); ++r) reps_[r]->model_version = model_version[r];
        for (auto &rp : reps_) rp->t = std::thread(&ReplicaSet::body, this, std::ref(*rp));
        dealing_ = true;
    }
    void deal(Ptr &f) {
        const size_t n_rep = reps_.size();
        const uint64_t s = next_seq_++;
        Replica &rp = *reps_[(size_t)(s % n_rep)];
        while (rp.outstanding >= kMaxOutstanding) release_next();
        f->seq = s;
        rp.outstanding += 1;
        std::lock_guard<std::mutex> lk(rp.m);
        rp.in.push_back(std::move(f));
        // its earlier flights are wanted back: it waits for them while this one runs (submit i + 1, wait i)
        if (s >= n_rep && (!rp.need_set || rp.need < s - n_rep)) { rp.need = s - n_rep; rp.need_set = true; }
        rp.cv.notify_all();
    }
    // whatever has come back in order already, without waiting
    void release_ready() {
        Ptr f;
        while (merge_.try_take(f)) {
            reps_[(size_t)(f->seq % reps_.size())]->outstanding -= 1;
            on_release_(f);
        }
    }
    // every dealt flight back and on to its rows, in order
    void drain() {
        while (merge_.next_seq() < next_seq_) release_next();
    }
    // the end of the input: everything back, the threads told to finish and waited for
    void close() {
        drain();
        for (auto &rp : reps_) { std::lock_guard<std::mutex> lk(rp->m); rp->closing = true; rp->cv.notify_all(); }
        for (auto &rp : reps_) if (rp->t.joinable()) rp->t.join();
    }
    // a failure, or the run is left some other way: the threads stop where they are
    void stop() {
        for (auto &rp : reps_) { std::lock_guard<std::mutex> lk(rp->m); rp->stop = true; rp->cv.notify_all(); }
        for (auto &rp : reps_) if (rp->t.joinable()) rp->t.join();
    }

private:
    // the next flight in input order, back from its replica, on to its rows
    void release_next() {
        const uint64_t s = merge_.next_seq();
        Replica &owner = *reps_[(size_t)(s % reps_.size())];
        { std::lock_guard<std::mutex> lk(owner.m); if (!owner.need_set || owner.need < s) { owner.need = s; owner.need_set = true; } owner.cv.notify_all(); }
        Ptr f = merge_.take();
        owner.outstanding -= 1;
        on_release_(f);
    }
    void body(Replica &rp) {
        std::deque<Ptr> flying;  // submitted, oldest first
        try {
            for (;;) {
                Ptr f;
                {
                    std::unique_lock<std::mutex> lk(rp.m);
                    auto wait_oldest = [&rp, &flying] {
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
                    submit_(rp.stream, *f);
                    rp.t_submit += now() - tk;
                    rp.batches += 1; rp.reads += f->reads();
                    flying.push_back(std::move(f));
                    continue;
                }
                Ptr g = std::move(flying.front());
                flying.pop_front();
                wait_(rp.stream, *g, rp.t_wait);
                const uint64_t seq = g->seq;
                merge_.put(seq, std::move(g));
            }
        } catch (InputError &e) {
            merge_.fail(e.what());  // the input's fault, not the replica's: the message a run without replicas gives
        } catch (std::exception &e) {
            merge_.fail("replica " + std::to_string(rp.index) + " (device " + std::to_string(rp.device) + "): " + e.what());
        }
        if (!flying.empty()) sync_(rp.stream);  // the uploads out of these flights' buffers are over before they are freed
    }

    const std::function<void(S, F &)> submit_;
    const std::function<void(S, F &, double &)> wait_;
    const std::function<void(S)> sync_;
    const std::function<void(Ptr &)> on_release_;
    std::vector<std::unique_ptr<Replica>> reps_;
    OrderedMerge<Ptr> merge_;
    bool dealing_ = false;
    uint64_t next_seq_ = 0;
};
template <class F, class S>
const size_t ReplicaSet<F, S>::kMaxOutstanding;
