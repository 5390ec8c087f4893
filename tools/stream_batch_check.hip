// stream_batch_check -- the host arithmetic of a batch's chain (csrc/parts/batch_plan.inc) behind a main of its own, so that it runs
// under the host sanitizers: the gzip column's plan against a brute-force restatement, the layout of a slot's result block, the dispatch
// on bin_words, the numbers of chn_stream_profile, waves_of and split_bound.  No HIP call is made: it runs on a machine without a GPU.
//
//   hipcc --offload-arch=gfx950 -std=c++14 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Icharon_amd/csrc tools/stream_batch_check.hip -o stream_batch_check && ./stream_batch_check
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "charon_hip.h"
#include "parts/common.inc"
#include "parts/lds_budget.hpp"
#include "parts/len_order.inc"
#include "parts/gzip_trees.inc"
#include "parts/gzip_walk.inc"
#include "parts/gzip_tally.inc"
#include "parts/gzip_size_dev.inc"
#include "parts/gzip_tally_long.inc"
#include "parts/batch_plan.inc"

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, g_case.c_str()); std::exit(1); } \
    } while (0)
static std::string g_case;

// ---- the gzip plan ----
static const size_t LDS_CU = (size_t)160 * 1024;
// a read's occupancy class by direct evaluation: wavefronts of its length that fit a CU's LDS, 16 at most; 0: not tallied
static uint32_t brute_class(uint64_t L, int bits, uint32_t bound) {
    if (L == 0 || L > bound) return 0;
    uint32_t w = 0;
    while (w < 16 && (size_t)(w + 1) * gzt_lds_bytes((uint32_t)L, bits) <= LDS_CU) ++w;
    return std::max(1u, w);
}
static uint32_t g_plans = 0;
static void plan_case(const char *name, const std::vector<uint32_t> &len1, const std::vector<uint32_t> &len2, int bits, uint32_t gzip_tallies, bool all_sizes) {
    g_case = std::string(name) + (bits == 4 ? ", 4-bit" : ", 2-bit") + (all_sizes ? ", all sizes" : "");
    const uint64_t n = len1.size();
    CHECK(len2.empty() || len2.size() == n);
    const uint32_t bound = std::min<uint32_t>(gzip_tallies, GZT_MAX_LEN), long_bound = gzip_tallies;  // as submit_gzip_column forms them
    auto len_of = [&](uint32_t i) { return (uint64_t)len1[i] + (len2.empty() ? 0 : len2[i]); };
    // the restatement: lists built with stable sorts
    std::vector<uint32_t> cls, lng, back;
    for (uint32_t i = 0; i < n; ++i) if (brute_class(len_of(i), bits, bound)) cls.push_back(i);
    std::stable_sort(cls.begin(), cls.end(), [&](uint32_t x, uint32_t y) { return brute_class(len_of(x), bits, bound) < brute_class(len_of(y), bits, bound); });
    if (all_sizes) {
        for (uint32_t i = 0; i < n; ++i) if (len_of(i) > GZT_MAX_LEN && len_of(i) <= long_bound && len_of(i) <= GZL_MAX_READ) lng.push_back(i);
        std::stable_sort(lng.begin(), lng.end(), [&](uint32_t x, uint32_t y) { return len_of(x) > len_of(y); });  // (stable: a tie goes to the lower read number)
        for (uint32_t i : cls) if (len_of(i) >= GZT_SYMBOL_LIMIT) back.push_back(i);
    }
    std::vector<uint32_t> index(7, 0xdeadbeefu);  // (what the slot's vector held before is none of the plan's)
    const GzPlan p = gz_plan(len1.data(), len2.empty() ? nullptr : len2.data(), n, bits, bound, long_bound, all_sizes, index);
    CHECK(p.long_at == cls.size() && p.rerun_at == cls.size() + lng.size() && index.size() == cls.size() + lng.size() + back.size());
    CHECK(std::equal(cls.begin(), cls.end(), index.begin()));
    CHECK(std::equal(lng.begin(), lng.end(), index.begin() + p.long_at));
    CHECK(std::equal(back.begin(), back.end(), index.begin() + p.rerun_at));
    CHECK(p.start[0] == 0 && p.start[1] == 0 && p.start[GZ_NCLS] == cls.size() && p.cmax[0] == 0);
    for (uint32_t c = 1; c < GZ_NCLS; ++c) {
        uint32_t count = 0, longest = 0;
        for (uint32_t i : cls) if (brute_class(len_of(i), bits, bound) == c) { ++count; longest = std::max(longest, (uint32_t)len_of(i)); }
        CHECK(p.start[c + 1] - p.start[c] == count && p.cmax[c] == longest);
        for (uint32_t j = p.start[c]; j < p.start[c + 1]; ++j) CHECK(index[j] < n && brute_class(len_of(index[j]), bits, bound) == c);
        if (count) CHECK(gzt_lds_bytes(longest, bits) <= LDS_CU);  // what the class's launch asks for fits a CU
    }
    ++g_plans;
}
static void check_gz_plan() {
    const uint32_t ALL = 0xFFFFFFFFu;  // gzip_tallies: no bound of the caller's
    const std::vector<uint32_t> none;
    for (int bits : {2, 4}) {
        // where the class changes: the last length of a class and the first of the next
        std::vector<uint32_t> edges, one_per_class;
        for (uint32_t L = 1; L < GZT_MAX_LEN; ++L)
            if (brute_class(L, bits, GZT_MAX_LEN) != brute_class(L + 1, bits, GZT_MAX_LEN)) { edges.push_back(L); edges.push_back(L + 1); one_per_class.push_back(L); }
        one_per_class.push_back(GZT_MAX_LEN);
        CHECK(!edges.empty() && brute_class(1, bits, GZT_MAX_LEN) == 16);
        for (bool all : {false, true}) {
            plan_case("no read", none, none, bits, ALL, all);
            plan_case("no read in any class", {0, 0, 1001, 70000, 0}, none, bits, 1000, all);
            plan_case("all reads in class 16", std::vector<uint32_t>(300, 150), none, bits, ALL, all);
            plan_case("one read per class", one_per_class, none, bits, ALL, all);
            std::vector<uint32_t> twice(edges);
            twice.insert(twice.end(), edges.rbegin(), edges.rend());
            plan_case("both sides of every class boundary", twice, none, bits, ALL, all);
            plan_case("bound and one more", {999, 1000, 1001, 1000, 1}, none, bits, 1000, all);
            plan_case("bound beyond the symbol limit", {GZT_SYMBOL_LIMIT - 1, GZT_SYMBOL_LIMIT, GZT_SYMBOL_LIMIT + 1, 20000, 20001, 5}, none, bits, 20000, all);
            plan_case("GZT_MAX_LEN and GZT_SYMBOL_LIMIT, one less and one more",
                      {GZT_MAX_LEN - 1, GZT_MAX_LEN, GZT_MAX_LEN + 1, GZT_SYMBOL_LIMIT - 1, GZT_SYMBOL_LIMIT, GZT_SYMBOL_LIMIT + 1, 150, GZT_SYMBOL_LIMIT, GZT_MAX_LEN + 1}, none, bits, ALL, all);
            plan_case("GZL_MAX_READ and one more", {GZL_MAX_READ, GZL_MAX_READ + 1, 150, GZL_MAX_READ - 1, GZL_MAX_READ}, none, bits, ALL, all);
            plan_case("long reads beyond the caller's bound", {100000, 100001, 99999, 61441, 150}, none, bits, 100000, all);
            plan_case("equal lengths in the long list", {70000, 90000, 70000, 150, 90000, 70000, 80000, 90000}, none, bits, ALL, all);
            plan_case("pairs", {150, 100, 0, 61000, 61440, 16000, 40000, 0}, {150, 0, 100, 440, 1, 383, 40000, 0}, bits, ALL, all);
            plan_case("pairs whose lengths sum beyond 2^32", {0xFFFFFFFFu, 0xFFFFFFFFu, 0x80000000u, 150, 0xFFF00000u}, {5, 0xFFFFFFFFu, 0x80000000u, 150, 0}, bits, ALL, all);
            std::vector<uint32_t> mixed;  // a few hundred reads of every kind, in no order
            uint64_t x = 88172645463325252ULL;
            for (int i = 0; i < 400; ++i) {
                x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                const uint32_t kind = (uint32_t)(x >> 60), r = (uint32_t)(x >> 20);
                mixed.push_back(kind < 8 ? r % 400 : kind < 12 ? r % 70000 : kind < 14 ? edges[r % edges.size()] : 61000 + r % 40000);
            }
            plan_case("mixed", mixed, none, bits, ALL, all);
            plan_case("mixed, bounded", mixed, none, bits, 30000, all);
        }
    }
}

// ---- ResLayout ----
static void check_res_layout() {
    for (uint64_t n : {1, 63, 64, 65})
        for (uint64_t C : {1, 2, 8}) {
            g_case = "ResLayout n = " + std::to_string(n) + ", C = " + std::to_string(C);
            const ResLayout L(n, C);
            // the columns in the order of launch_tail's downloads (the control words first, the double column next: it stays 8-byte aligned)
            const size_t at[] = {L.ctl, L.prob, L.nh, L.counts, L.unique, L.call, L.conf, L.flags, L.total};
            const size_t bytes[] = {CTL_WORDS * 8, n * C * 8, n * 4, n * C * 4, n * C * 4, n, n, n};
            CHECK(at[0] == 0);
            for (int i = 0; i < 8; ++i) CHECK(at[i + 1] == at[i] + bytes[i]);  // back to back: no overlap, no hole, total is the end
            CHECK(L.prob % 8 == 0 && L.nh % 4 == 0 && L.counts % 4 == 0 && L.unique % 4 == 0);
        }
}

// ---- by_words ----
static void check_by_words() {
    for (uint64_t W : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)4, (uint64_t)5, (uint64_t)255, ((uint64_t)1 << 32) + 1, ~(uint64_t)0}) {
        g_case = "by_words " + std::to_string(W);
        int reached[5] = {0, 0, 0, 0, 0};
        const int got = by_words(W, [&](auto w) { ++reached[decltype(w)::value]; return (int)decltype(w)::value; });
        const int want = W >= 1 && W <= 4 ? (int)W : 4;  // outside 1 .. 4: the instance for 4, as the switches' `default:` had it
        CHECK(got == want);
        for (int i = 0; i < 5; ++i) CHECK(reached[i] == (i == want ? 1 : 0));
        int calls = 0;
        by_words(W, [&](auto) { ++calls; });  // a callable that returns nothing
        CHECK(calls == 1);
    }
    int bits_seen = 0;
    gz_by_bits(4, [&](auto b) { bits_seen = decltype(b)::value; });
    CHECK(bits_seen == 4);
    gz_by_bits(2, [&](auto b) { bits_seen = decltype(b)::value; });
    CHECK(bits_seen == 2);
}

// ---- chn_stream_profile's numbers ----
static void check_profile_numbers() {
    g_case = "profile numbers";
    // as include/charon_hip.h documents them
    const int documented[][2] = {{PROF_PROBE, 0}, {PROF_COUNT, 1}, {PROF_MODEL, 2}, {PROF_CHAIN, 3}, {PROF_RERUNS, 4}, {PROF_FETCHES, 5}, {PROF_TEXT_UPLOAD, 6},
                                 {PROF_TEXT_PACK, 7}, {PROF_TEXT_SPLIT, 8}, {PROF_TEXT_FETCH, 9}, {PROF_PAIR_IDS, 11}, {PROF_GATED, 13}, {PROF_FASTA_SPLIT, 14}};
    int accepted = 0;
    for (const auto &d : documented) { CHECK(d[0] == d[1] && profile_which_ok(d[1])); ++accepted; }
    for (int which = -3; which <= 20; ++which) {
        bool is_documented = false;
        for (const auto &d : documented) is_documented |= d[1] == which;
        CHECK(profile_which_ok(which) == is_documented);
    }
    CHECK(accepted == 13 && !profile_which_ok(10) && !profile_which_ok(12) && !profile_which_ok(-1) && !profile_which_ok(15));
}

// ---- waves_of, split_bound ----
static void check_waves_and_split() {
    g_case = "waves_of";
    CHECK(waves_of(0) == 0 && waves_of(1) == 1 && waves_of(63) == 1 && waves_of(64) == 1 && waves_of(65) == 2 && waves_of(130) == 3);
    CHECK(waves_of(0xFFFFFF00ULL) == 0x3FFFFFCULL && waves_of(((uint64_t)1 << 32) + 1) == ((uint64_t)1 << 26) + 1);  // max_reads' limit, and past 32 bits
    for (uint64_t n = 1; n < 1000; ++n) CHECK((waves_of(n) - 1) * WAVE < n && n <= waves_of(n) * WAVE);
    g_case = "split_bound";
    CHECK(len_bucket_floor(LONG_BUCKET_DEFAULT) == 32768);
    for (uint32_t bucket : {64u, LONG_BUCKET_DEFAULT, 200u}) {
        const uint32_t fl = len_bucket_floor(bucket);
        const std::vector<uint32_t> lens = {fl, fl - 1, 0, fl + 1, 150, fl - 1, fl, 0xFFFFFFFFu};
        CHECK(split_bound(bucket, false, &lens, lens.size()) == 4);   // at the floor and above: long; one below: not
        CHECK(split_bound(bucket, true, &lens, lens.size()) == 0);    // pairs are never split
        CHECK(split_bound(256, false, &lens, lens.size()) == 0);      // nor is anything on a stream that never splits
        CHECK(split_bound(bucket, false, nullptr, lens.size()) == lens.size());  // a device batch: any of its reads may be long
        const std::vector<uint32_t> below(130, fl - 1), at(130, fl);
        CHECK(split_bound(bucket, false, &below, 130) == 0 && split_bound(bucket, false, &at, 130) == 130);
    }
    const std::vector<uint32_t> empty;
    CHECK(split_bound(LONG_BUCKET_DEFAULT, false, &empty, 0) == 0);
}

// ---- "window too large for LDS" ----
// submit_impl refuses a batch whose probe kernel would need more LDS than a CU has.  chn_index_desc.window_size is eight bits wide: over
// every index chn_index_create accepts (k 1 .. 27, window k .. 255, h 1 .. 5, W 1 .. 4; MODE_FUSED is W = 1 with at most 8 categories)
// the refusal is out of reach, which is why no GPU test provokes it.
static size_t check_window_refusal_unreachable() {
    g_case = "probe LDS over every accepted index";
    size_t most = 0;
    for (uint64_t seed : {(uint64_t)0x8F3F73B5CF1C9ADEULL, (uint64_t)0, ~(uint64_t)0})
        for (uint32_t k = 1; k <= 27; ++k)
            for (uint32_t w = k; w <= 255; ++w)
                for (uint32_t h = 1; h <= 5; ++h) {
                    const uint32_t wn = w - k + 1;
                    const bool pack = ring_pack_ok(k, wn, seed);
                    for (uint32_t W = 1; W <= 4; ++W) most = std::max(most, std::max(k1_lds_bytes(wn, 255, MODE_ROWS, h, W, 64 * W, pack), k1_lds_bytes(wn, 255, MODE_LIST, h, W, 64 * W, pack)));
                    for (uint32_t B = 1; B <= 8; ++B) most = std::max(most, k1_lds_bytes(wn, B, MODE_FUSED, h, 1, B, pack));
                }
    CHECK(most <= (size_t)160 * 1024);
    return most;
}

int main() {
    check_gz_plan();
    check_res_layout();
    check_by_words();
    check_profile_numbers();
    check_waves_and_split();
    const size_t most = check_window_refusal_unreachable();
    std::printf("stream_batch_check: %u gzip plans; the most LDS a probe wavefront of an accepted index takes: %zu bytes\nok\n", g_plans, most);
    return 0;
}
