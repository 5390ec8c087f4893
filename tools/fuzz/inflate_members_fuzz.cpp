// Fuzzer of the deflate member decoder (charon_amd/csrc/parts/inflate_members.inc) on a CPU build under ASan / UBSan: the host policy of
// the very source k_inflate_members compiles.  Every case is compared with zlib's inflate -- accept / reject and the bytes -- and, where
// zlib accepts, the decoder's CRC-32 (inf_crc32: 64 slices and the join, as on the device) with zlib's crc32 of the output.
//   g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all -Icharon_amd/csrc tools/fuzz/inflate_members_fuzz.cpp -lz -o /tmp/inflate_members_fuzz
//   /tmp/inflate_members_fuzz [cases] [seed]
// Cases: random texts (FASTQ-like, runs, noise) deflated at random levels / strategies with random flushes, then 0 - 3 byte mutations, a
// truncation or appended junk, and an expected size that is now and then off by one.  The output buffer is exactly out_length bytes long.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>
#include <zlib.h>

#include "parts/inflate_members.inc"

static uint64_t g_x = 1;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }

static std::vector<uint8_t> deflate_raw(const std::vector<uint8_t> &text) {
    z_stream zs;
    std::memset(&zs, 0, sizeof zs);
    const int levels[] = {0, 1, 4, 6, 9};
    const int strategies[] = {Z_DEFAULT_STRATEGY, Z_DEFAULT_STRATEGY, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, Z_FILTERED};
    deflateInit2(&zs, levels[rnd() % 5], Z_DEFLATED, -15, 1 + (int)(rnd() % 9), strategies[rnd() % 6]);
    std::vector<uint8_t> out(deflateBound(&zs, (uLong)text.size()) + 4096);
    zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
    size_t at = 0;
    while (at < text.size() && rnd() % 3 == 0) {  // a few flushes: empty stored blocks, new tables
        const size_t n = std::min<size_t>(text.size() - at, 1 + rnd() % 20000);
        zs.next_in = const_cast<uint8_t *>(text.data()) + at; zs.avail_in = (uInt)n;
        deflate(&zs, rnd() % 2 ? Z_SYNC_FLUSH : Z_FULL_FLUSH);
        at += n;
    }
    zs.next_in = const_cast<uint8_t *>(text.data()) + at; zs.avail_in = (uInt)(text.size() - at);
    deflate(&zs, Z_FINISH);
    out.resize(out.size() - zs.avail_out);
    deflateEnd(&zs);
    return out;
}

int main(int argc, char **argv) {
    const long cases = argc > 1 ? std::atol(argv[1]) : 20000;
    g_x = (argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1) * 0x9E3779B97F4A7C15ULL + 1;
    InfShared *sh = new InfShared;
    long accepted = 0, bad = 0, bad_crc = 0;
    for (long c = 0; c < cases; ++c) {
        const size_t n = rnd() % 8 == 0 ? rnd() % 65537 : rnd() % 6000;
        std::vector<uint8_t> text(n);
        const unsigned kind = (unsigned)(rnd() % 4);
        for (size_t i = 0; i < n; ++i)
            text[i] = kind == 0 ? (uint8_t)"ACGT\nF:@+"[rnd() % 9] : kind == 1 ? (uint8_t)rnd() : kind == 2 ? (uint8_t)('A' + (i / (1 + rnd() % 300)) % 3) : (uint8_t)(40 + __builtin_ctzll(rnd() | (1ull << 23)));
        std::vector<uint8_t> m = deflate_raw(text);
        for (unsigned k = (unsigned)(rnd() % 4); k > 0 && !m.empty(); --k) m[rnd() % 4 ? rnd() % m.size() : rnd() % std::min<size_t>(m.size(), 100)] ^= (uint8_t)(1 + rnd() % 255);
        if (rnd() % 8 == 0 && !m.empty()) m.resize(rnd() % m.size());
        if (rnd() % 8 == 0) for (unsigned k = 0; k < 3; ++k) m.push_back((uint8_t)rnd());
        uint32_t size = (uint32_t)n;
        if (rnd() % 16 == 0 && size < 65536) ++size; else if (rnd() % 16 == 0 && size) --size;
        // the yardstick
        std::vector<uint8_t> want((size_t)size + 1);
        z_stream zs;
        std::memset(&zs, 0, sizeof zs);
        inflateInit2(&zs, -15);
        zs.next_in = m.data(); zs.avail_in = (uInt)m.size();
        zs.next_out = want.data(); zs.avail_out = (uInt)want.size();
        const int rc = inflate(&zs, Z_FINISH);
        const bool ok = rc == Z_STREAM_END && zs.total_out == size;
        inflateEnd(&zs);
        // the decoder, into a buffer of exactly `size` bytes (ASan watches its end) from an input of exactly m.size() bytes
        uint8_t *in = new uint8_t[m.size() ? m.size() : 1], *out = new uint8_t[size ? size : 1];
        if (!m.empty()) std::memcpy(in, m.data(), m.size());
        uint32_t crc = 0xDEADBEEFu;
        const int st = inf_member_host(*sh, in, m.size(), out, size, &crc);
        if ((st == 0) != ok || (ok && size && std::memcmp(out, want.data(), size) != 0)) {
            if (++bad < 10) std::printf("case %ld: zlib %s (rc %d, %lu bytes), decoder status %d, expected size %u\n", c, ok ? "accepts" : "rejects", rc, zs.total_out, st, size);
        }
        if (ok && st == 0 && crc != (uint32_t)crc32(0L, want.data(), size)) {
            if (++bad_crc < 10) std::printf("case %ld: CRC-32 of %u bytes: decoder %08x, zlib %08lx\n", c, size, crc, crc32(0L, want.data(), size));
        }
        accepted += ok;
        delete[] in; delete[] out;
    }
    std::printf("%ld cases, %ld accepted by zlib, %ld disagreements, %ld CRC-32 disagreements among the accepted\n", cases, accepted, bad, bad_crc);
    delete sh;
    return bad || bad_crc ? 1 : 0;
}
