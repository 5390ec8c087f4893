// flight_pool.inc -- flight objects go round (their vectors keep their capacity: no fresh pages per batch)
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a stand-alone header.

// F::let_go() drops what a flight must not hold on to while it waits in the pool.  take() and recycle() may be called from any thread.
template <class F>
class FlightPool {
    std::mutex m_;
    std::vector<std::unique_ptr<F>> free_;

public:
    std::unique_ptr<F> take() {
        std::unique_ptr<F> f;
        {
            std::lock_guard<std::mutex> lk(m_);
            if (!free_.empty()) { f = std::move(free_.back()); free_.pop_back(); }
        }
        if (!f) f.reset(new F());
        return f;
    }
    void recycle(std::unique_ptr<F> &f) {
        f->let_go();
        std::lock_guard<std::mutex> lk(m_);
        free_.push_back(std::move(f));
    }
};
