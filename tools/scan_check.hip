// scan_check -- the wave, workgroup and one-workgroup array prefix sums of csrc/parts/scan.inc behind a main of its own, each compared
// exactly with a serial loop on the host: the array scan as the library's kernels instantiate it (256 threads; 32-bit sums, 64-bit sums
// of 32-bit values, a clamped load, in place, two fields of a struct in place, n read from the device), the block step at 64, 256 and
// 1024 threads.  Sizes are the smallest at which a lane, a wavefront's partial, a round of 1024 or the carry can go wrong.
// Needs a device.  One line per case; exits non-zero at the first mismatch, or at a HIP error after printing it (nothing is launched after).
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++14 -ffp-contract=off -Wall -Wno-unused-function -Iinclude -Icharon_amd/csrc \
//         tools/scan_check.hip -o scan_check && ./scan_check
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
#include "parts/scan.inc"

#define HIPOK(expr)                                                                                              \
    do {                                                                                                         \
        const hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) { std::printf("HIP error: %s: %s\n", #expr, hipGetErrorString(e_)); std::exit(2); } \
    } while (0)

static const uint32_t GUARD = 64;                 // elements behind the n scanned ones that must stay as they were
static const uint32_t MAX_N = 4097 + 8 + GUARD;   // (the device-side n cases reach a little past the largest size)
struct Pair { uint64_t a, b; uint32_t pad[4]; };  // two scanned fields among others, as WaveMeta has them

// ---- kernels: what the library's scan kernels do around array_scan / block_scan, and every thread's return value ----
template <class In, class T>
__global__ void __launch_bounds__(SCAN_THREADS) k_array(const In *in, T *out, const uint32_t *n_dev, uint32_t n_max, In clamp, T *total) {
    const uint32_t n = n_dev ? min(*n_dev, n_max) : n_max;
    total[threadIdx.x] = array_scan<SCAN_THREADS, T>(n, [&](uint32_t i) { const In v = in[i]; return v <= clamp ? v : (In)0; }, [&](uint32_t i, T at) { out[i] = at; });
}
__global__ void __launch_bounds__(SCAN_THREADS) k_fields(Pair *v, uint32_t n, uint64_t *total) {
    total[threadIdx.x] = array_scan<SCAN_THREADS, uint64_t>(n, [&](uint32_t i) { return v[i].a; }, [&](uint32_t i, uint64_t at) { v[i].a = at; });
    total[SCAN_THREADS + threadIdx.x] = array_scan<SCAN_THREADS, uint64_t>(n, [&](uint32_t i) { return v[i].b; }, [&](uint32_t i, uint64_t at) { v[i].b = at; });
}
template <uint32_t THREADS, class T>
__global__ void __launch_bounds__(THREADS) k_block(const T *in, T *prefix, T *total) {
    T all;
    prefix[threadIdx.x] = block_scan<THREADS, T>(in[threadIdx.x], all);
    total[threadIdx.x] = all;
}

// ---- host side ----
static void *d_in, *d_out, *d_total;
static uint32_t *d_n;
static uint32_t g_cases = 0;

static void ran() { HIPOK(hipGetLastError()); HIPOK(hipDeviceSynchronize()); }
static void verdict(const std::string &name, bool ok, const std::string &why) {
    std::printf("%-78s %s%s\n", name.c_str(), ok ? "ok" : "MISMATCH ", ok ? "" : why.c_str());
    if (!ok) std::exit(1);
    ++g_cases;
}
enum Values { ONES, MIX, ALL32 };
static const char *values_name(Values v) { return v == ONES ? "ones" : v == MIX ? "mix < 2^20" : "0xFFFFFFFF"; }
static uint64_t value_at(Values v, uint64_t seed, uint32_t i) { return v == ONES ? 1u : v == MIX ? mix64(seed + i) & 0xFFFFFu : 0xFFFFFFFFu; }

// n_dev < 0: the kernel gets no device-side n.  `over`: every seventh value is raised above the clamp (and counts 0).
template <class In, class T>
static void array_case(const char *kind, Values values, uint32_t n_max, long n_dev, bool over, bool in_place) {
    const In clamp = over ? (In)0xFFFFF : (In)~(In)0;
    const uint32_t n = n_dev < 0 ? n_max : (uint32_t)std::min<long>(n_dev, n_max), len = std::max(n, n_max) + GUARD;
    std::vector<In> in(len);
    for (uint32_t i = 0; i < len; ++i) in[i] = (In)value_at(values, 1000 + n_max, i) + (over && i % 7 == 3 ? (In)0x100000 : (In)0);
    std::vector<T> want(len), got(len), totals(SCAN_THREADS);
    T run = 0;
    for (uint32_t i = 0; i < len; ++i) {
        if (i < n) { want[i] = run; run += in[i] <= clamp ? in[i] : 0; }
        else if (in_place) want[i] = (T)in[i];
        else std::memset(&want[i], 0xA5, sizeof(T));
    }
    void *out = in_place ? d_in : d_out;
    HIPOK(hipMemcpy(d_in, in.data(), len * sizeof(In), hipMemcpyHostToDevice));
    if (!in_place) HIPOK(hipMemset(d_out, 0xA5, len * sizeof(T)));
    HIPOK(hipMemset(d_total, 0xA5, SCAN_THREADS * sizeof(T)));
    const uint32_t nd = n_dev < 0 ? 0 : (uint32_t)n_dev;
    HIPOK(hipMemcpy(d_n, &nd, 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL((k_array<In, T>), dim3(1), dim3(SCAN_THREADS), 0, 0, (const In *)d_in, (T *)out, n_dev < 0 ? (const uint32_t *)nullptr : d_n, n_max, clamp, (T *)d_total);
    ran();
    HIPOK(hipMemcpy(got.data(), out, len * sizeof(T), hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(totals.data(), d_total, SCAN_THREADS * sizeof(T), hipMemcpyDeviceToHost));
    std::string why;
    for (uint32_t i = 0; i < len && why.empty(); ++i)
        if (got[i] != want[i]) why = "at " + std::to_string(i) + ": " + std::to_string(got[i]) + ", not " + std::to_string(want[i]);
    for (uint32_t t = 0; t < SCAN_THREADS && why.empty(); ++t)
        if (totals[t] != run) why = "total of thread " + std::to_string(t) + ": " + std::to_string(totals[t]) + ", not " + std::to_string(run);
    verdict(std::string("array ") + kind + ", " + values_name(values) + ", n_max " + std::to_string(n_max) + (n_dev < 0 ? "" : ", device n " + std::to_string(n_dev)), why.empty(), why);
}

static void fields_case(uint32_t n) {
    const uint32_t len = n + GUARD;
    std::vector<Pair> v(len), got(len);
    for (uint32_t i = 0; i < len; ++i) { v[i].a = value_at(MIX, 77 + n, i); v[i].b = 0xFFFFFFFFu; for (uint32_t k = 0; k < 4; ++k) v[i].pad[k] = 0xC0FFEE00u + i + k; }
    std::vector<uint64_t> totals(2 * SCAN_THREADS);
    HIPOK(hipMemcpy(d_in, v.data(), len * sizeof(Pair), hipMemcpyHostToDevice));
    HIPOK(hipMemset(d_total, 0xA5, 2 * SCAN_THREADS * 8));
    hipLaunchKernelGGL(k_fields, dim3(1), dim3(SCAN_THREADS), 0, 0, (Pair *)d_in, n, (uint64_t *)d_total);
    ran();
    HIPOK(hipMemcpy(got.data(), d_in, len * sizeof(Pair), hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(totals.data(), d_total, 2 * SCAN_THREADS * 8, hipMemcpyDeviceToHost));
    uint64_t ra = 0, rb = 0;
    for (uint32_t i = 0; i < n; ++i) { const uint64_t a = v[i].a, b = v[i].b; v[i].a = ra; v[i].b = rb; ra += a; rb += b; }
    std::string why;
    for (uint32_t i = 0; i < len && why.empty(); ++i)
        if (std::memcmp(&got[i], &v[i], sizeof(Pair))) why = "at " + std::to_string(i);
    for (uint32_t t = 0; t < SCAN_THREADS && why.empty(); ++t)
        if (totals[t] != ra || totals[SCAN_THREADS + t] != rb) why = "totals of thread " + std::to_string(t);
    verdict("array two fields of a struct in place, n " + std::to_string(n), why.empty(), why);
}

template <uint32_t THREADS, class T>
static void block_case(Values values) {
    std::vector<T> in(THREADS), prefix(THREADS), totals(THREADS);
    for (uint32_t i = 0; i < THREADS; ++i) in[i] = (T)value_at(values, 5 + THREADS, i);
    HIPOK(hipMemcpy(d_in, in.data(), THREADS * sizeof(T), hipMemcpyHostToDevice));
    HIPOK(hipMemset(d_out, 0xA5, THREADS * sizeof(T)));
    HIPOK(hipMemset(d_total, 0xA5, THREADS * sizeof(T)));
    hipLaunchKernelGGL((k_block<THREADS, T>), dim3(1), dim3(THREADS), 0, 0, (const T *)d_in, (T *)d_out, (T *)d_total);
    ran();
    HIPOK(hipMemcpy(prefix.data(), d_out, THREADS * sizeof(T), hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(totals.data(), d_total, THREADS * sizeof(T), hipMemcpyDeviceToHost));
    T run = 0, all = 0;
    for (uint32_t i = 0; i < THREADS; ++i) all += in[i];
    std::string why;
    for (uint32_t i = 0; i < THREADS && why.empty(); ++i) {
        if (prefix[i] != run || totals[i] != all) why = "thread " + std::to_string(i) + ": prefix " + std::to_string(prefix[i]) + " total " + std::to_string(totals[i]) + ", not " + std::to_string(run) + " and " + std::to_string(all);
        run += in[i];
    }
    verdict("block step, " + std::to_string(THREADS) + " threads, " + std::to_string(8 * sizeof(T)) + "-bit, " + values_name(values), why.empty(), why);
}
template <uint32_t THREADS>
static void block_cases() {
    block_case<THREADS, uint32_t>(ONES); block_case<THREADS, uint32_t>(MIX);
    block_case<THREADS, uint64_t>(ONES); block_case<THREADS, uint64_t>(MIX); block_case<THREADS, uint64_t>(ALL32);
}

int main() {
    HIPOK(hipMalloc(&d_in, MAX_N * sizeof(Pair)));
    HIPOK(hipMalloc(&d_out, MAX_N * sizeof(uint64_t)));
    HIPOK(hipMalloc(&d_total, 2 * 1024 * sizeof(uint64_t)));
    HIPOK(hipMalloc((void **)&d_n, 4));
    block_cases<64>(); block_cases<256>(); block_cases<1024>();
    for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 255u, 256u, 257u, 1023u, 1024u, 1025u, 2048u, 3077u, 4097u}) {
        for (Values v : {ONES, MIX}) array_case<uint32_t, uint32_t>("32-bit", v, n, -1, false, false);                    // k_split_scan
        for (Values v : {ONES, MIX, ALL32}) array_case<uint32_t, uint64_t>("32-bit values, 64-bit sums", v, n, -1, false, false);  // k_ef_block_prefix
        array_case<uint32_t, uint64_t>("32-bit values clamped, 64-bit sums", MIX, n, -1, true, false);                    // k_deflate_scan
        for (Values v : {ONES, MIX, ALL32}) array_case<uint64_t, uint64_t>("64-bit in place", v, n, -1, false, true);      // k_scan_u64
        fields_case(n);                                                                                                    // k_scan_meta
    }
    for (uint32_t n_max : {1u, 1024u, 1025u, 3077u})  // k_split_scan's device-side n: below n_max, equal to it, above it
        for (long n_dev : {(long)n_max - 1, (long)n_max, (long)n_max + 5}) array_case<uint32_t, uint32_t>("32-bit", MIX, n_max, n_dev, false, false);
    HIPOK(hipFree(d_in)); HIPOK(hipFree(d_out)); HIPOK(hipFree(d_total)); HIPOK(hipFree(d_n));
    std::printf("scan_check: %u cases\nok\n", g_cases);
    return 0;
}
