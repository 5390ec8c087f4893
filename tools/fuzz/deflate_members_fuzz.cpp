// Fuzzer of the deflate member compressor (charon_amd/csrc/parts/deflate_members.inc) on a CPU build under ASan / UBSan: the host policy
// of the very source k_deflate_members compiles.  Every member is inflated by zlib and compared with the piece, its CRC-32 with zlib's
// crc32, its size with the planned one and with the bound, and a BGZF member's header and trailer are checked field by field.
//   g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all -Icharon_amd/csrc tools/fuzz/deflate_members_fuzz.cpp -lz -o /tmp/deflate_members_fuzz
//   /tmp/deflate_members_fuzz [cases] [seed]
// Cases: FASTQ-like text, noise, runs, short periods, a far repeat (beyond 32 768), sparse alphabets; lengths 0 .. 65 280, small ones often.
// The piece lives in a buffer of exactly its length, the member's slot has exactly DFL_SLOT bytes (ASan watches both ends).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>
#include <zlib.h>

#include "parts/gzip_trees.inc"
#include "parts/inflate_members.inc"
#include "parts/deflate_members.inc"

static uint64_t g_x = 1;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }

int main(int argc, char **argv) {
    const long cases = argc > 1 ? std::atol(argv[1]) : 5000;
    g_x = (argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1) * 0x9E3779B97F4A7C15ULL + 1;
    DflShared *sh = new DflShared;
    uint32_t *tokens = new uint32_t[DFL_MAX_IN];
    long bad = 0, stored = 0;
    uint64_t in_total = 0, out_total = 0;
    for (long c = 0; c < cases; ++c) {
        const uint32_t pick = (uint32_t)(rnd() % 16);
        const size_t n = pick == 0 ? DFL_MAX_IN - rnd() % 3 : pick < 4 ? rnd() % (DFL_MAX_IN + 1) : pick < 8 ? rnd() % 300 : rnd() % 6000;
        std::vector<uint8_t> text(n);
        const unsigned kind = (unsigned)(rnd() % 7);
        const size_t period = 1 + rnd() % (rnd() % 2 ? 70 : 40000);
        const unsigned alphabet = 1 + (unsigned)(rnd() % 5);
        for (size_t i = 0; i < n; ++i)
            text[i] = kind == 0 ? (uint8_t)"ACGT\nF:@+"[rnd() % 9] : kind == 1 ? (uint8_t)rnd() : kind == 2 ? (uint8_t)('A' + (i / (1 + rnd() % 300)) % 3)
                    : kind == 3 ? (uint8_t)(40 + __builtin_ctzll(rnd() | (1ull << 23))) : kind == 4 ? (i >= period ? text[i - period] : (uint8_t)rnd())
                    : kind == 5 ? (uint8_t)('a' + rnd() % alphabet) : (i >= period && rnd() % 50 ? text[i - period] : (uint8_t)"ACGT"[rnd() % 4]);
        const uint32_t flags = (uint32_t)(rnd() % 2);
        uint8_t *in = new uint8_t[n ? n : 1], *slot = new uint8_t[DFL_SLOT];
        if (n) std::memcpy(in, text.data(), n);
        uint32_t crc = 0xDEADBEEFu;
        const uint32_t size = dfl_member_host(*sh, tokens, in, (uint32_t)n, flags, slot, &crc);
        const uint32_t head = flags ? DFL_BGZF_HEAD : 0, tail = flags ? DFL_BGZF_TAIL : 0;
        const char *why = nullptr;
        if (size > n + 5 + head + tail || size < head + tail + 2) why = "size outside the bound";
        else {
            std::vector<uint8_t> back(n + 1);
            z_stream zs;
            std::memset(&zs, 0, sizeof zs);
            inflateInit2(&zs, -15);
            zs.next_in = slot + head; zs.avail_in = size - head - tail;
            zs.next_out = back.data(); zs.avail_out = (uInt)back.size();
            const int rc = inflate(&zs, Z_FINISH);
            if (rc != Z_STREAM_END || zs.total_out != n || zs.avail_in != 0) why = "zlib's inflate does not accept the member as a whole";
            else if (n && std::memcmp(back.data(), text.data(), n) != 0) why = "the member inflates to other bytes";
            inflateEnd(&zs);
            const uint32_t want = (uint32_t)crc32(0L, text.data(), (uInt)n);
            if (!why && crc != want) why = "CRC-32 differs from zlib's";
            if (!why && flags) {
                const uint8_t h12[12] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0};
                uint32_t t[2];
                std::memcpy(t, slot + size - 8, 8);
                if (std::memcmp(slot, h12, 12) != 0 || slot[12] != 'B' || slot[13] != 'C' || slot[14] != 2 || slot[15] != 0) why = "bad BGZF header";
                else if ((uint32_t)(slot[16] | (slot[17] << 8)) != size - 1) why = "BSIZE is not the member's size - 1";
                else if (t[0] != want || t[1] != n) why = "bad trailer";
            }
            if (!why && (slot[head] & 6) == 0) ++stored;
        }
        if (why && ++bad < 10) std::printf("case %ld (kind %u, %zu bytes, flags %u, size %u): %s\n", c, kind, n, flags, size, why);
        in_total += n; out_total += size;
        delete[] in; delete[] slot;
    }
    std::printf("%ld cases, %ld stored, %llu bytes in, %llu out, %ld failures\n", cases, stored, (unsigned long long)in_total, (unsigned long long)out_total, bad);
    delete sh; delete[] tokens;
    return bad ? 1 : 0;
}
