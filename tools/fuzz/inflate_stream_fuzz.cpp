// Fuzzer of the stream inflate (charon_amd/csrc/parts/inflate_stream.inc, abi_inflate_stream.inc) on a CPU build under ASan / UBSan: the host
// policy of the very decoder source k_inflate_chunks compiles, with the window hand-down, the symbol-to-byte rule and the counting rule of
// chn_inflate_stream_run_host.  Runs on the CPU only.
//   g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Icharon_amd/csrc tools/fuzz/inflate_stream_fuzz.cpp -lz -o /tmp/inflate_stream_fuzz
//   /tmp/inflate_stream_fuzz [cases] [seed]
// Cases: random texts deflated at random levels / strategies / memory levels with sync flushes (true, byte-aligned block starts), 0 - 2 byte
// mutations or a truncation; chunk starts drawn from the true starts and from random bit positions; a job that begins at the member's
// start or at a later true start with the true window, or a shorter one; out_bytes exact, generous or short.  Input and output live in
// buffers of exactly their size (ASan watches both ends).  Against zlib's inflate over the same input with the same window as dictionary:
//   * the counted bytes are a prefix of what zlib writes before it ends or fails, and every counted chunk's CRC-32 is zlib's crc32 of its bytes;
//   * an untouched stream cut at true starts only, with room and capacity enough, counts every chunk and all of the text;
//   * the counting rule holds between the arrays that come back.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>
#include <zlib.h>

#include "charon_hip.h"
static int fail(int rc, const std::string &) { return rc; }
#include "parts/inflate_members.inc"
#include "parts/inflate_stream.inc"
#include "parts/abi_inflate_stream.inc"

static uint64_t g_x = 1;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }

// raw deflate of `text`; starts: (data byte offset, text offset) of the stream's start and of every sync flush
static std::vector<uint8_t> deflate_raw(const std::vector<uint8_t> &text, std::vector<std::pair<size_t, size_t>> &starts) {
    z_stream zs;
    std::memset(&zs, 0, sizeof zs);
    const int levels[] = {0, 1, 4, 6, 9};
    const int strategies[] = {Z_DEFAULT_STRATEGY, Z_DEFAULT_STRATEGY, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, Z_FILTERED};
    deflateInit2(&zs, levels[rnd() % 5], Z_DEFLATED, -15, 1 + (int)(rnd() % 9), strategies[rnd() % 6]);
    std::vector<uint8_t> out(deflateBound(&zs, (uLong)text.size()) + 65536);
    zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
    starts.clear();
    starts.push_back({0, 0});
    size_t at = 0;
    const unsigned every = 1 + (unsigned)(rnd() % 4);
    while (at < text.size() && starts.size() < 40 && rnd() % every != 0 && zs.avail_out > 70000) {
        const size_t n = std::min<size_t>(text.size() - at, 1 + rnd() % 30000);
        zs.next_in = const_cast<uint8_t *>(text.data()) + at; zs.avail_in = (uInt)n;
        deflate(&zs, Z_SYNC_FLUSH);
        at += n;
        if (at < text.size()) starts.push_back({out.size() - zs.avail_out, at});
    }
    zs.next_in = const_cast<uint8_t *>(text.data()) + at; zs.avail_in = (uInt)(text.size() - at);
    deflate(&zs, Z_FINISH);
    out.resize(out.size() - zs.avail_out);
    deflateEnd(&zs);
    return out;
}

int main(int argc, char **argv) {
    const long cases = argc > 1 ? std::atol(argv[1]) : 5000;
    g_x = (argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1) * 0x9E3779B97F4A7C15ULL + 1;
    long bad = 0, clean_cases = 0, counted_chunks = 0, chunks = 0, with_window = 0, far = 0;
    unsigned long long bytes = 0;
    for (long c = 0; c < cases; ++c) {
        const size_t n = rnd() % 4 == 0 ? rnd() % 300000 : rnd() % 40000;
        std::vector<uint8_t> text(n);
        const unsigned kind = (unsigned)(rnd() % 4);
        const size_t period = 1 + rnd() % 300;
        for (size_t i = 0; i < n; ++i)
            text[i] = kind == 0 ? (uint8_t)"ACGT\nF:@+"[rnd() % 9] : kind == 1 ? (uint8_t)rnd() : kind == 2 ? (uint8_t)('A' + (i / period) % 3) : (i >= 200 && rnd() % 50) ? text[i - 200] : (uint8_t)(33 + rnd() % 60);
        std::vector<std::pair<size_t, size_t>> starts;
        std::vector<uint8_t> m = deflate_raw(text, starts);
        bool clean = true;
        for (unsigned k = (unsigned)(rnd() % 3) * (unsigned)(rnd() % 2); k > 0 && !m.empty(); --k) { m[rnd() % m.size()] ^= (uint8_t)(1 + rnd() % 255); clean = false; }
        if (rnd() % 10 == 0 && m.size() > 1) { m.resize(1 + rnd() % (m.size() - 1)); clean = false; }
        // where the job begins: a true start
        size_t s0 = rnd() % 3 == 0 ? rnd() % starts.size() : 0;
        while (s0 > 0 && starts[s0].first >= m.size()) --s0;
        const size_t d0 = starts[s0].first, t0 = starts[s0].second;
        size_t have = std::min<size_t>(t0, 32768);
        if (have && rnd() % 4 == 0) { have = rnd() % (have + 1); }
        const bool short_window = have < std::min<size_t>(t0, 32768);
        with_window += have > 0;
        // chunk starts: true starts behind s0 (each with probability 3/4) and a few random bit positions
        std::vector<uint64_t> begin;
        begin.push_back(0);
        bool all_true = true;
        for (size_t k = s0 + 1; k < starts.size(); ++k)
            if (starts[k].first < m.size() && rnd() % 4) begin.push_back((uint64_t)(starts[k].first - d0) * 8);
        const size_t in_bytes = m.size() - d0;
        for (unsigned k = (unsigned)(rnd() % 3) * (unsigned)(rnd() % 2); k > 0; --k) {
            const uint64_t b = 1 + rnd() % (8 * in_bytes - 1 ? 8 * in_bytes - 1 : 1);
            if (b < 8 * in_bytes) { begin.push_back(b); all_true = false; }
        }
        std::sort(begin.begin(), begin.end());
        begin.erase(std::unique(begin.begin(), begin.end()), begin.end());
        const size_t nc = begin.size();
        std::vector<uint64_t> target(nc);
        for (size_t k = 0; k < nc; ++k) target[k] = k + 1 < nc ? begin[k + 1] : 8 * (uint64_t)in_bytes;
        if (rnd() % 8 == 0) target[rnd() % nc] += rnd() % 4000;  // a target further on: the chunk overshoots its successor
        // the yardstick: everything zlib writes from there, with the window as its dictionary
        std::vector<uint8_t> want(n - t0 + 2000);  // (a mutated stream may write more than the text: zlib stops at the end of this buffer)
        size_t want_n;
        bool z_end;
        {
            z_stream zs;
            std::memset(&zs, 0, sizeof zs);
            inflateInit2(&zs, -15);
            if (have) inflateSetDictionary(&zs, text.data() + t0 - have, (uInt)have);
            zs.next_in = m.data() + d0; zs.avail_in = (uInt)in_bytes;
            zs.next_out = want.data(); zs.avail_out = (uInt)want.size();
            const int rc = inflate(&zs, Z_FINISH);
            want_n = zs.total_out;
            z_end = rc == Z_STREAM_END;
            inflateEnd(&zs);
        }
        // the job, in buffers of exactly their size
        const uint64_t out_bytes = rnd() % 4 == 0 ? rnd() % (want_n + 1) : rnd() % 2 || want_n == want.size() ? want_n : want_n + rnd() % 1000;
        const uint64_t cap = rnd() % 4 == 0 ? CHN_INFLATE_STREAM_MIN_SYMS : std::max<uint64_t>(CHN_INFLATE_STREAM_MIN_SYMS, n + 1);
        uint8_t *in = new uint8_t[in_bytes], *out = new uint8_t[out_bytes ? out_bytes : 1], *win = new uint8_t[have ? have : 1];
        std::memcpy(in, m.data() + d0, in_bytes);
        if (have) std::memcpy(win, text.data() + t0 - have, have);
        std::vector<uint64_t> end_bit(nc, ~0ull), out_length(nc, ~0ull);
        std::vector<uint32_t> status(nc, ~0u), crc(nc, ~0u);
        std::vector<uint8_t> fin(nc, 0xFF);
        uint64_t counted = ~0ull, used = ~0ull;
        chn_inflate_stream_job j;
        std::memset(&j, 0, sizeof j);
        j.struct_size = sizeof j; j.n_chunks = nc;
        j.in = in; j.in_bytes = in_bytes; j.begin_bit = begin.data(); j.target_bit = target.data();
        j.window = have ? win : nullptr; j.window_bytes = have; j.sym_capacity = cap;
        j.out = out; j.out_bytes = out_bytes;
        j.end_bit = end_bit.data(); j.out_length = out_length.data(); j.status = status.data(); j.final = fin.data(); j.crc32 = crc.data();
        j.n_counted = &counted; j.out_used = &used;
        const int rc = chn_inflate_stream_run_host(&j);
        std::string what;
        if (rc != CHN_OK) what = "the call failed";
        else if (counted < 1 || counted > nc) what = "n_counted out of range";
        else {
            uint64_t sum = 0;
            for (uint64_t k = 0; k < counted && what.empty(); ++k) {
                if (status[k] > 5 && status[k] != CHN_INFLATE_E_ROOM) what = "unknown status";
                else if (end_bit[k] < begin[k] || end_bit[k] > 8 * (uint64_t)in_bytes) what = "end_bit out of range";
                else if (k + 1 < counted && (status[k] != 0 || fin[k] != 0 || end_bit[k] != begin[k + 1])) what = "a chunk counted behind one that does not prove it";
                else if (k + 1 == counted && k + 1 < nc && status[k] == 0 && fin[k] == 0 && end_bit[k] == begin[k + 1]) what = "the chain ended where it goes on";
                else if (sum + out_length[k] > want_n) what = "more bytes than zlib wrote";
                else if (crc[k] != (uint32_t)crc32(0L, want.data() + sum, (uInt)out_length[k])) what = "CRC-32 differs from zlib's";
                sum += out_length[k];
                far += status[k] == 4 && out_length[k] == 0 && end_bit[k] == begin[k];
            }
            if (what.empty() && (sum != used || used > out_bytes)) what = "out_used is not the sum of out_length";
            if (what.empty() && used && std::memcmp(out, want.data(), used) != 0) what = "bytes differ from zlib's";
            if (what.empty() && clean && all_true && !short_window && z_end && out_bytes >= want_n && cap > n && target.back() == 8 * (uint64_t)in_bytes) {
                bool nudged = false;
                for (size_t k = 0; k + 1 < nc; ++k) nudged = nudged || target[k] != begin[k + 1];
                if (!nudged) {
                    ++clean_cases;
                    if (counted != nc || used != want_n || want_n != n - t0 || !fin[nc - 1] || status[nc - 1] != 0) what = "an untouched stream cut at true starts was not counted whole";
                }
            }
            counted_chunks += (long)counted; bytes += used;
        }
        chunks += (long)nc;
        if (!what.empty() && ++bad < 10)
            std::printf("case %ld: %s (chunks %zu, counted %llu, used %llu of zlib's %zu, window %zu, in %zu bytes, clean %d)\n", c, what.c_str(), nc, (unsigned long long)counted,
                        (unsigned long long)used, want_n, have, in_bytes, (int)clean);
        delete[] in; delete[] out; delete[] win;
    }
    std::printf("%ld cases (%ld with a window), %ld chunks, %ld counted, %llu bytes counted, %ld untouched streams counted whole, %ld distance-rule stops, %ld disagreements\n",
                cases, with_window, chunks, counted_chunks, bytes, clean_cases, far, bad);
    return bad ? 1 : 0;
}
