// dehost_pipeline_check -- the thread machinery of `charon dehost` (host/flight_pool.inc, host/row_writer.inc, host/replica_set.inc over
// host/ordered_merge.inc) behind a main of its own, with a stub flight (a position in input order and a model version) and stub
// callables that sleep for a few pseudo-random microseconds, so that it can run under the thread sanitizer and under the address and
// undefined-behaviour sanitizers.  No GPU, no HIP, no Result, no OpenMP (libgomp gives the thread sanitizer false reports).
//
//   g++ -std=c++14 -O1 -g -Wall -pthread -fsanitize=thread -Icharon_amd/csrc/host tools/dehost_pipeline_check.cpp -o dehost_pipeline_check
//   ./dehost_pipeline_check
// and a second build with -fsanitize=address,undefined -fno-sanitize-recover=undefined in place of -fsanitize=thread.
//
// The main thread below does what run_host_loop (host/dehost_loop.inc) does with these pieces, and catches what dehost_main catches.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace {
#include "run_util.inc"
#include "ordered_merge.inc"
#include "flight_pool.inc"
#include "row_writer.inc"
#include "replica_set.inc"

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

std::atomic<long> g_made{0}, g_gone{0};  // constructions and destructions of stub flights

struct StubFlight {
    uint64_t seq = 0;
    uint32_t version = 0;
    uint64_t id = 0;           // position in input order
    std::vector<char> payload; // (its capacity must survive the pool)
    bool held = false;         // something let_go() has to drop
    StubFlight() { ++g_made; }
    ~StubFlight() { ++g_gone; }
    StubFlight(const StubFlight &) = delete;
    size_t reads() const { return 7; }
    void let_go() { held = false; }
};
typedef std::unique_ptr<StubFlight> Ptr;
typedef ReplicaSet<StubFlight, int> Set;  // the "stream" is the replica's number

void nap(uint64_t &s) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    std::this_thread::sleep_for(std::chrono::microseconds(s % 40));
}

enum Fault { NONE, SUBMIT, SUBMIT_INPUT, WAIT, ROWS };
struct Case {
    size_t n_rep = 1, n_flights = 0;
    Fault fault = NONE;
    uint64_t fault_at = 0;              // the flight (input position) at which the fault strikes
    uint64_t off_from = 0, off_to = 0;  // hand-over is switched off for flights [off_from, off_to): the models' version has moved
};
struct Outcome {
    std::vector<uint64_t> written;  // input positions in the order their rows were written
    int caught = 0;
    std::string error;
    uint64_t inline_rows = 0, writer_rows = 0, syncs = 0;
};

Outcome run_case(const Case &c) {
    Outcome out;
    const long made0 = g_made, gone0 = g_gone;
    {
        std::vector<int> devices, streams;
        for (size_t r = 0; r < c.n_rep; ++r) { devices.push_back(10 + (int)r); streams.push_back((int)r); }
        const std::thread::id main_id = std::this_thread::get_id();
        FlightPool<StubFlight> pool;
        uint32_t current_version = 1;  // main thread only (the predicate runs there)
        std::atomic<long> handed{0}, finished{0}, syncs{0};
        std::vector<std::atomic<int>> flying(c.n_rep), in_replica(c.n_rep);
        for (size_t r = 0; r < c.n_rep; ++r) { flying[r] = 0; in_replica[r] = 0; }
        uint64_t seed_rows = 0x9E3779B97F4A7C15ULL;
        // `out.written`, the row counts and seed_rows are plain data touched by whichever thread writes rows: the thread sanitizer
        // reports it if the main thread ever writes rows without having drained the writer
        RowWriter<StubFlight> writer(
            [&out, &c, &seed_rows, &finished, main_id](StubFlight &f) {
                nap(seed_rows);
                if (c.fault == ROWS && f.id == c.fault_at) { ++finished; throw std::runtime_error("rows failed"); }
                out.written.push_back(f.id);
                (std::this_thread::get_id() == main_id ? out.inline_rows : out.writer_rows) += 1;
                ++finished;
            },
            [&pool](Ptr &f) { pool.recycle(f); },
            [&current_version](const StubFlight &f) { return f.version == current_version; });
        Set replicas(
            devices, streams,
            [&c, &flying, &in_replica](int st, StubFlight &f) {
                uint64_t s = (f.id + 1) * 0xD1B54A32D192ED03ULL;
                nap(s);
                if (c.fault == SUBMIT && f.id == c.fault_at) throw std::runtime_error("submit failed");
                if (c.fault == SUBMIT_INPUT && f.id == c.fault_at) throw InputError("parse error: bad input");
                CHECK(++flying[(size_t)st] <= (int)Set::kMaxOutstanding);
                CHECK(++in_replica[(size_t)st] <= (int)Set::kMaxOutstanding);
            },
            [&c, &flying](int st, StubFlight &f, double &acc) {
                uint64_t s = (f.id + 3) * 0x9E3779B97F4A7C15ULL;
                const double t0 = now();
                nap(s);
                acc += now() - t0;
                --flying[(size_t)st];
                if (c.fault == WAIT && f.id == c.fault_at) throw std::runtime_error("wait failed");
            },
            [&syncs](int) { ++syncs; },
            [&writer, &handed, &finished, &in_replica, &c](Ptr &f) {
                --in_replica[(size_t)(f->seq % c.n_rep)];
                writer.hand_on(f);
                // two queued and the one being written
                CHECK(++handed - finished <= (long)RowWriter<StubFlight>::kMaxQueued + 1);
            });
        try {
            for (uint64_t i = 0; i < c.n_flights; ++i) {
                current_version = (i >= c.off_from && i < c.off_to) ? 2 : 1;  // (flights are packed for version 1 throughout)
                if (replicas.dealing()) replicas.release_ready();
                Ptr f = pool.take();
                f->id = i; f->version = 1; f->held = true;
                if (!replicas.dealing()) replicas.start(std::vector<uint32_t>(c.n_rep, 1));
                replicas.deal(f);
                for (size_t r = 0; r < c.n_rep; ++r) CHECK(replicas.at(r).outstanding <= Set::kMaxOutstanding);
                replicas.release_ready();
            }
            if (replicas.dealing()) replicas.close();
            writer.drain();
        } catch (std::exception &e) {
            out.caught += 1;
            out.error = e.what();
            replicas.stop();
        }
        out.syncs = (uint64_t)syncs;
        if (!out.caught) {
            uint64_t batches = 0;
            for (size_t r = 0; r < c.n_rep; ++r) { batches += replicas.at(r).batches; CHECK(replicas.at(r).reads == 7 * replicas.at(r).batches); }
            CHECK(batches == c.n_flights);
        }
    }  // replicas, writer and pool are gone: every thread is joined, every flight freed
    CHECK(g_made - made0 == g_gone - gone0);
    return out;
}

void check_order_and_bounds() {
    const size_t K = Set::kMaxOutstanding;
    for (size_t n_rep : {1, 2, 3, 8})
        for (size_t n : {(size_t)0, (size_t)1, K, K + 1, (size_t)300}) {
            Case c;
            c.n_rep = n_rep; c.n_flights = n;
            const Outcome o = run_case(c);
            CHECK(o.caught == 0);
            CHECK(o.written.size() == n);
            for (size_t i = 0; i < n; ++i) CHECK(o.written[i] == i);  // exactly once, in input order
            CHECK(o.inline_rows == 0);
        }
}

void check_hand_over_switch() {
    for (size_t n_rep : {1, 2, 3, 8}) {
        Case c;
        c.n_rep = n_rep; c.n_flights = 240; c.off_from = 80; c.off_to = 160;
        const Outcome o = run_case(c);
        CHECK(o.caught == 0 && o.written.size() == c.n_flights);
        for (size_t i = 0; i < c.n_flights; ++i) CHECK(o.written[i] == i);  // order holds across both switches
        // a flight is judged when it is released, up to n_rep * kMaxOutstanding flights behind the dealing: both paths were taken
        CHECK(o.inline_rows > 0 && o.writer_rows > 0 && o.inline_rows + o.writer_rows == c.n_flights);
    }
}

void check_failures() {
    const uint64_t n = 60;
    for (size_t n_rep : {1, 2, 3, 8})
        for (Fault fault : {SUBMIT, SUBMIT_INPUT, WAIT, ROWS})
            for (uint64_t at : {(uint64_t)0, n / 2, n - 1}) {
                Case c;
                c.n_rep = n_rep; c.n_flights = n; c.fault = fault; c.fault_at = at;
                const Outcome o = run_case(c);
                CHECK(o.caught == 1);  // once, on the main thread
                const std::string where = "replica " + std::to_string(at % n_rep) + " (device " + std::to_string(10 + at % n_rep) + "): ";
                const std::string want = fault == SUBMIT ? where + "submit failed" : fault == WAIT ? where + "wait failed"
                                         : fault == SUBMIT_INPUT ? "parse error: bad input" : "rows failed";
                if (o.error != want) { std::fprintf(stderr, "got \"%s\", want \"%s\"\n", o.error.c_str(), want.c_str()); std::exit(1); }
                // nothing behind the failure was written, and what was written is a prefix of the input in order
                CHECK(o.written.size() <= at);
                for (size_t i = 0; i < o.written.size(); ++i) CHECK(o.written[i] == i);
            }
}

void check_pool() {
    const long made0 = g_made;
    {
        FlightPool<StubFlight> pool;
        Ptr a = pool.take();
        StubFlight *pa = a.get();
        a->payload.resize(1 << 16);
        a->payload.clear();
        a->held = true;
        const size_t cap = a->payload.capacity();
        pool.recycle(a);
        CHECK(!a);
        Ptr b = pool.take();
        CHECK(b.get() == pa && b->payload.capacity() == cap && !b->held);  // the same object, its capacity kept, let_go() called
        Ptr d = pool.take();
        CHECK(d.get() != pa && g_made - made0 == 2);  // an empty pool makes a new one
        pool.recycle(b);
        pool.recycle(d);
    }
    CHECK(g_made == g_gone);
}

}  // namespace

int main() {
    (void)ordered_merge_selftest;  // (`charon _ordered_merge` runs that one)
    check_pool();
    check_order_and_bounds();
    check_hand_over_switch();
    check_failures();
    CHECK(g_made == g_gone);
    std::printf("flights made and freed: %ld\nok\n", (long)g_made);
    return 0;
}
