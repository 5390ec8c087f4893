// abi_helpers_check -- the helpers of csrc/parts/abi_device_call.inc that need no device, behind a main of their own so that they can
// run under the host sanitizers: grown_size (ensure_grow's arithmetic) against the expression it replaced, run_groups with stub
// callables (every group count from 1 to 5; a failing issue and a failing collect at the first, a middle and the last group), and
// CallTimer::report.  No HIP call is made: it runs on a machine without a GPU.
//
//   hipcc --offload-arch=gfx950 -std=c++14 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Icharon_amd/csrc tools/abi_helpers_check.hip -o abi_helpers_check && ./abi_helpers_check
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "charon_hip.h"
#include "parts/common.inc"
#include "parts/abi_device_call.inc"

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

// the capacity a grow-only buffer of `cap` bytes has after ensure(bytes)
static size_t after_ensure(size_t cap, size_t bytes) { return bytes <= cap ? cap : bytes; }

static void check_grown_size() {
    const size_t values[] = {0, 1, 15, 16, 17, 4095, 4096, 65280, (size_t)1 << 32, ((size_t)1 << 40) + 3};
    for (size_t cap : values)
        for (size_t need : values)
            for (size_t slack : {(size_t)0, (size_t)1, need / 4, (need > 64 ? need - 64 : 0) / 4}) {
                const size_t before = need + (cap < need ? slack : 0);  // the idiom as it stood at its twelve sites
                CHECK(after_ensure(cap, grown_size(cap, need, slack)) == after_ensure(cap, before));
                if (need > cap) CHECK(grown_size(cap, need, slack) == need + slack);
            }
    CHECK(grown_size(100, 100, 25) == 100 && grown_size(100, 101, 25) == 126 && grown_size(0, 0, 7) == 0);
}

struct StubPipe {
    int drains = 0;
    void drain() { ++drains; }
};
struct StubSet {
    bool busy = false;
    uint64_t first = 0, n = 0;
};

// `members` members in groups of `per`; issue number fail_issue / collect number fail_collect (from 0; -1: none) fails with -7
static void run_case(uint64_t members, uint64_t per, int fail_issue, int fail_collect) {
    StubPipe pipe;
    StubSet set[2];
    std::vector<std::string> log;
    int issues = 0, collects = 0;
    uint64_t handed = 0;
    const int rc = run_groups(pipe, set, members,
        [&](StubSet &st, uint64_t first, uint64_t &n) {
            CHECK(&st == &set[issues & 1] && !st.busy && first < members);  // the set whose turn it is, and it is free
            log.push_back("i" + std::to_string(issues));
            if (issues++ == fail_issue) return -7;
            n = std::min(per, members - first);
            st.first = first; st.n = n; st.busy = true;
            return CHN_OK;
        },
        [&](StubSet &st) {
            CHECK(&st == &set[collects & 1] && st.busy && st.first == handed);  // in order, each group once
            log.push_back("c" + std::to_string(collects));
            if (collects++ == fail_collect) return -7;
            st.busy = false;
            handed += st.n;
            return CHN_OK;
        });
    const int groups = (int)((members + per - 1) / per);
    const bool fails = (fail_issue >= 0 && fail_issue < groups) || (fail_collect >= 0 && fail_collect < groups);
    CHECK(rc == (fails ? -7 : CHN_OK));
    CHECK(pipe.drains == (fails ? 1 : 0));
    CHECK(!set[0].busy && !set[1].busy);
    if (!fails) {
        CHECK(handed == members && issues == groups && collects == groups);
        // i0 i1 c0 i2 c1 ... c(last): group g is collected right behind the issue of group g + 1
        for (int g = 0, at = 0; g < groups; ++g) {
            CHECK(log[at++] == "i" + std::to_string(g));
            if (g > 0) CHECK(log[at++] == "c" + std::to_string(g - 1));
            if (g + 1 == groups) CHECK(log[at++] == "c" + std::to_string(g) && at == (int)log.size());
        }
    } else {
        const std::string last = log.back();  // nothing is issued or collected behind the failure
        CHECK(last == (fail_issue >= 0 ? "i" + std::to_string(fail_issue) : "c" + std::to_string(fail_collect)));
    }
}

static void check_run_groups() {
    for (uint64_t groups = 1; groups <= 5; ++groups)
        for (uint64_t ragged : {0, 1}) {
            if (ragged && groups == 1) continue;
            const uint64_t per = 3, members = groups * per - ragged;
            run_case(members, per, -1, -1);
            for (int at : {0, (int)groups / 2, (int)groups - 1}) {
                run_case(members, per, at, -1);
                run_case(members, per, -1, at);
            }
        }
    StubPipe pipe;  // no member: nothing is issued, collected or drained
    StubSet set[2];
    CHECK(run_groups(pipe, set, 0, [](StubSet &, uint64_t, uint64_t &) { return -7; }, [](StubSet &) { return -7; }) == CHN_OK && pipe.drains == 0);
}

static void check_call_timer() {
    CallTimer t;
    double ms = -1;
    uint64_t calls = 99;
    t.report(&ms, &calls, 0);
    CHECK(ms == 0 && calls == 0);
    CHECK(t.begin(false, nullptr) == hipSuccess && t.end(false, nullptr) == hipSuccess && t.collect(false) == hipSuccess);  // not profiling: no event, no count
    CHECK(!t.ev[0] && !t.ev[1] && t.calls == 0);
    t.count_only();
    t.ms = 1.5; t.calls += 2;
    t.report(nullptr, nullptr, 0);
    t.report(&ms, nullptr, 0);
    CHECK(ms == 1.5);
    t.report(nullptr, &calls, 1);  // a reset hands out what it clears
    CHECK(calls == 3 && t.ms == 0 && t.calls == 0);
    t.report(&ms, &calls, 1);
    CHECK(ms == 0 && calls == 0);
    t.release();
}

int main() {
    check_grown_size();
    check_run_groups();
    check_call_timer();
    std::puts("abi_helpers_check: ok");
    return 0;
}
