// ordered_merge.inc -- release items completed out of order strictly by sequence number (CHARON_DEVICES: the batches of several index replicas
// go back to the row writer in input order, as the reference's ordered critical section does for its reads, src/dehost_main.cpp:374-375)
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a stand-alone header.

// Producers put(seq, item) in any order; the consumer takes item 0, 1, 2, ... in turn.  A producer that fails calls fail(): the consumer's next
// take() then throws instead of waiting for a sequence number that will never come.
template <class T>
class OrderedMerge {
    std::mutex m_;
    std::condition_variable cv_;
    std::map<uint64_t, T> done_;
    uint64_t next_ = 0;
    std::string error_;

public:
    void put(uint64_t seq, T item) {
        std::lock_guard<std::mutex> lk(m_);
        done_.emplace(seq, std::move(item));
        if (seq == next_) cv_.notify_all();
    }
    void fail(const std::string &msg) {
        std::lock_guard<std::mutex> lk(m_);
        if (error_.empty()) error_ = msg.empty() ? std::string("unknown failure") : msg;
        cv_.notify_all();
    }
    // the item of the next sequence number, waiting for it; throws once a producer has failed
    T take() {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return !error_.empty() || (!done_.empty() && done_.begin()->first == next_); });
        if (!error_.empty()) throw std::runtime_error(error_);
        T item = std::move(done_.begin()->second);
        done_.erase(done_.begin());
        ++next_;
        return item;
    }
    // the item of the next sequence number if it is there already
    bool try_take(T &out) {
        std::lock_guard<std::mutex> lk(m_);
        if (!error_.empty()) throw std::runtime_error(error_);
        if (done_.empty() || done_.begin()->first != next_) return false;
        out = std::move(done_.begin()->second);
        done_.erase(done_.begin());
        ++next_;
        return true;
    }
    uint64_t next_seq() {
        std::lock_guard<std::mutex> lk(m_);
        return next_;
    }
};

// hidden diagnostic `charon _ordered_merge T M seed`: T producer threads complete the sequence numbers 0..M-1, dealt round-robin from a seeded
// shuffle, with short random sleeps; the released order is printed one number per line (no GPU involved)
int ordered_merge_selftest(int threads, uint64_t m, uint64_t seed) {
    std::vector<uint64_t> order(m);
    for (uint64_t i = 0; i < m; ++i) order[i] = i;
    uint64_t x = seed * 0x9E3779B97F4A7C15ULL + 1;
    auto rnd = [](uint64_t &s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (uint64_t i = m; i > 1; --i) std::swap(order[i - 1], order[rnd(x) % i]);
    OrderedMerge<uint64_t> merge;
    std::vector<std::thread> producers;
    for (int t = 0; t < threads; ++t)
        producers.emplace_back([&, t]() {
            uint64_t s = (seed + 1) * 0xD1B54A32D192ED03ULL + (uint64_t)t + 1;
            for (uint64_t i = (uint64_t)t; i < m; i += (uint64_t)threads) {
                std::this_thread::sleep_for(std::chrono::microseconds(rnd(s) % 200));
                merge.put(order[i], order[i]);
            }
        });
    std::string out;
    for (uint64_t i = 0; i < m; ++i) out += std::to_string(merge.take()) + "\n";
    for (std::thread &p : producers) p.join();
    std::fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
