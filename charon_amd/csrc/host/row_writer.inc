// row_writer.inc -- the rows of a waited flight: written here, or by a thread of their own while the main thread packs the next batch
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a stand-alone header.

// The rows of a batch are formatted and written by a thread of their own once the models are final and nothing is extracted (every plain
// `charon dehost` run after its first read): the main thread packs and submits batch i + 1 meanwhile -- with the default -t 1 it used to
// alternate between packing (1.2 s of a 2.1 s loop on 4 M reads) and rows (0.8 s).  Batches go through in order; at most two wait.
//
// THE SHARED-STATE RULE.  The writer thread reaches the run's state only through `rows`, the callable it is given, and `recycle`.  In
// `charon dehost`, `rows` is RowStage::finish_rows, which on this thread takes the fast path alone: it reads the flight, appends through
// Result::bulk() and reads Result's getters (models_final, current_model_version).  Everything else of Result -- add_read, refresh,
// reclassify_raw, ensure_device_model, complete, the extract files -- is the main thread's, and may change what those getters return.
// So (1) a flight is handed over only when `may_hand_over` says so, which the caller makes imply "models final, the flight's version
// current, nothing to extract": from then on no call of the main thread moves the models; and (2) the main thread drains the writer before
// every path that can change Result: the inline branch of hand_on() below (the only way rows are written on the main thread), a pair-id
// failure, and the end of the read loop.  Both hold by structure: hand_on() is the one door to `rows`, and it drains first.
// Neither Result nor HIP is known here.
template <class F>
class RowWriter {
public:
    typedef std::unique_ptr<F> Ptr;
    static const size_t kMaxQueued = 2;

    // rows(F &): format and write the rows of a flight; recycle(Ptr &): the flight back to its pool; may_hand_over(const F &): the
    // caller's predicate, evaluated on the main thread
    RowWriter(std::function<void(F &)> rows, std::function<void(Ptr &)> recycle, std::function<bool(const F &)> may_hand_over)
        : rows_(std::move(rows)), recycle_(std::move(recycle)), may_hand_over_(std::move(may_hand_over)) {}
    RowWriter(const RowWriter &) = delete;
    RowWriter &operator=(const RowWriter &) = delete;
    // whatever way the run ends: the thread writes what is queued (unless it has failed: then it is gone already) and is waited for
    ~RowWriter() {
        { std::lock_guard<std::mutex> lk(m_); stop_ = true; cv_.notify_all(); }
        if (t_.joinable()) t_.join();
    }

    // everything handed over has been written (or has failed: throws the failure)
    void drain() {
        if (!t_.joinable()) return;
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [this] { return (q_.empty() && !busy_) || !error_.empty(); });
        if (!error_.empty()) throw std::runtime_error(error_);
    }
    // a waited flight on to its rows: the writer's queue, or here behind everything handed over before
    void hand_on(Ptr &f) {
        if (!may_hand_over_(*f)) {  // the reference's read-by-read state machine: here
            drain();
            rows_(*f);
            recycle_(f);
            return;
        }
        if (!t_.joinable()) t_ = std::thread(&RowWriter::body, this);
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [this] { return q_.size() < kMaxQueued || !error_.empty(); });
        if (!error_.empty()) throw std::runtime_error(error_);
        q_.push_back(std::move(f));
        cv_.notify_all();
    }

private:
    void body() {
        for (;;) {
            Ptr f;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [this] { return !q_.empty() || stop_; });
                if (q_.empty()) return;
                f = std::move(q_.front());
                q_.pop_front();
                busy_ = true;
                cv_.notify_all();
            }
            std::string err;
            try { rows_(*f); } catch (std::exception &e) { err = e.what(); }
            recycle_(f);
            std::lock_guard<std::mutex> lk(m_);
            busy_ = false;
            if (!err.empty() && error_.empty()) error_ = err;
            cv_.notify_all();
            if (!err.empty()) return;
        }
    }

    const std::function<void(F &)> rows_;
    const std::function<void(Ptr &)> recycle_;
    const std::function<bool(const F &)> may_hand_over_;
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<Ptr> q_;
    bool busy_ = false, stop_ = false;
    std::string error_;
    std::thread t_;
};
template <class F>
const size_t RowWriter<F>::kMaxQueued;
