// Checks the host arithmetic of charon_amd/csrc/parts/lds_budget.hpp (the ring-packing rule, the probe kernel's LDS size, the count
// kernel's budget) against independent restatements.  No GPU, no HIP:
//   g++ -std=c++14 -O1 -Icharon_amd/csrc/parts tools/lds_budget_check.cpp -o lds_budget_check && ./lds_budget_check
// Prints one line per fact and "ok"; exits 1 at the first mismatch.  (tests/test_lds_budget_cpu.py builds and runs it.)
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "lds_budget.hpp"

static void fail(const char *what, unsigned long long a, unsigned long long b, unsigned long long c) {
    std::fprintf(stderr, "FAILED: %s (%llu, %llu, %llu)\n", what, a, b, c);
    std::exit(1);
}

int main() {
    const uint64_t seed = 0x8F3F73B5CF1C9ADEULL;
    // 1. the rule, against 128-bit arithmetic: the largest value term, shifted up by the offset field with wn - 1 in it, fits 64 bits
    unsigned packed = 0, plane = 0, largest_k_packed_at_default_window = 0;
    for (uint32_t k = 1; k <= 27; ++k) {
        unsigned __int128 p5 = 1;
        for (uint32_t i = 0; i < k; ++i) p5 *= 5;
        const unsigned __int128 vmax = p5 - 1, smax = seed >> (64 - 2 * k), top = vmax > smax ? vmax : smax;
        for (uint32_t wn = 1; wn <= 300; ++wn) {
            uint32_t pb = 0;
            while (pb < 32 && (1u << pb) < wn) ++pb;  // smallest field that holds 0 .. wn - 1
            if (pb != ring_offset_bits(wn)) fail("offset bits", k, wn, pb);
            const bool fits = pb == 0 ? (top >> 64) == 0 : (((top << pb) | (wn - 1)) >> 64) == 0;
            if (fits != ring_pack_ok(k, wn, seed)) fail("ring_pack_ok", k, wn, fits);
            if (fits != (ring_value_bits(k, seed) + pb <= 64)) fail("bits + pb <= 64", k, wn, fits);
            (fits ? packed : plane) += 1;
            if (fits && wn == 23) largest_k_packed_at_default_window = k;
            // 2. the probe kernel's LDS shrinks by exactly the offset plane, in every mode
            const int modes[4] = {MODE_FUSED, MODE_ROWS, MODE_EMPLACE, MODE_LIST};
            for (int mode : modes)
                for (uint32_t B : {2u, 8u, 100u, 200u}) {
                    const uint32_t W = (B + 63) / 64, C = B < 8 ? B : 2;
                    const size_t a = k1_lds_bytes(wn, C, mode, 3, W, B, false), b = k1_lds_bytes(wn, C, mode, 3, W, B, true);
                    if (a - b != (size_t)wn * 64) fail("k1_lds_bytes difference", wn, a, b);
                }
        }
    }
    if (!packed || !plane) fail("both sides of the rule occur", packed, plane, 0);
    std::printf("rule: %u (k, wn) pairs packed, %u with the offset plane; at wn = 23 packed up to k = %u\n", packed, plane, largest_k_packed_at_default_window);
    if (largest_k_packed_at_default_window != 25) fail("wn = 23 packs up to k = 25", largest_k_packed_at_default_window, 0, 0);
    if (!ring_pack_ok(19, 23, seed) || ring_value_bits(19, seed) != 45 || ring_offset_bits(23) != 5) fail("default (19, 41)", ring_value_bits(19, seed), ring_offset_bits(23), 0);

    // 3. the 39g shape: k = 19, w = 41, h = 3, B = 100, C = 2, W = 2, 16-bit totals
    const size_t lds_plane = k1_lds_bytes(23, 2, MODE_ROWS, 3, 2, 100, false), lds_packed = k1_lds_bytes(23, 2, MODE_ROWS, 3, 2, 100, true);
    if (lds_plane != 22208 || lds_packed != 20736) fail("probe LDS at the default", lds_plane, lds_packed, 0);
    const size_t k2_64 = k2_lds_bytes(100, 2, 2, 64, true), k2_32 = k2_lds_bytes(100, 2, 2, 32, true);
    if (k2_64 != 14480) fail("count tables, 64 owners", k2_64, 0, 0);
    const auto up = [](size_t x) { return (x + LDS_GRANULE - 1) / LDS_GRANULE * LDS_GRANULE; };
    if (7 * up(lds_packed) + up(k2_64 + K2_LDS_STATIC) > CU_LDS_BYTES) fail("seven packed probe wavefronts + a 64-owner count workgroup fit a CU", 7 * up(lds_packed), up(k2_64 + K2_LDS_STATIC), CU_LDS_BYTES);
    if (8 * up(lds_packed) <= CU_LDS_BYTES) fail("seven packed probe wavefronts per CU, not eight", up(lds_packed), 0, 0);
    if (k2_group(100, 2, 2, true, k2_lds_budget(lds_packed)) != 64) fail("G at the default with packing", k2_group(100, 2, 2, true, k2_lds_budget(lds_packed)), k2_lds_budget(lds_packed), 0);
    // without packing, and with larger tables, the loop picks what the fixed 7 680 B picked
    if (k2_lds_budget(lds_plane) != 7680 || k2_group(100, 2, 2, true, k2_lds_budget(lds_plane)) != 32 || k2_32 > 7680) fail("G at the default without packing", k2_lds_budget(lds_plane), k2_32, 0);
    if (7 * up(lds_plane) + up(k2_32 + K2_LDS_STATIC) > CU_LDS_BYTES) fail("seven probe wavefronts with the plane + a 32-owner count workgroup fit a CU", up(lds_plane), up(k2_32 + K2_LDS_STATIC), 0);
    for (uint32_t wn = 1; wn <= 300; ++wn)
        for (uint32_t W = 1; W <= 4; ++W) {
            const size_t b = k2_lds_budget(k1_lds_bytes(wn, 2, MODE_ROWS, 3, W, 64 * W, ring_pack_ok(19, wn, seed)));
            if (b < K2_LDS_BUDGET_MIN || b > CU_LDS_BYTES) fail("budget range", wn, W, b);
            // what the budget promises: floor(160 KB / probe LDS) probe wavefronts and a count workgroup of that many bytes fit a CU (above the floor)
            const size_t p = up(k1_lds_bytes(wn, 2, MODE_ROWS, 3, W, 64 * W, ring_pack_ok(19, wn, seed)));
            if (b > K2_LDS_BUDGET_MIN && CU_LDS_BYTES / p * p + up(b + K2_LDS_STATIC) > CU_LDS_BYTES) fail("budget fits", wn, W, b);
        }
    std::printf("39g: probe LDS %zu -> %zu B, count tables %zu B (64 owners) within a budget of %zu B; without packing budget %zu B, 32 owners\n", lds_plane,
                lds_packed, k2_64, k2_lds_budget(lds_packed), k2_lds_budget(lds_plane));
    std::printf("ok\n");
    return 0;
}
