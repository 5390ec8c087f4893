// charon -- MI355X drop-in for `charon dehost` (rmcolq/charon).  C++14 host front end; every per-read
// computation of the hot path runs in libcharon_hip.so behind the C ABI of include/charon_hip.h.
//
// Mirrors (reference paths relative to the reference checkout):
//   * command line: src/main.cpp:49-65, src/dehost_main.cpp:208-312 (same flags, defaults and integer limits;
//     CLI11 itself is not reproduced)
//   * dehost_main / dehost_reads / dehost_paired_reads: src/dehost_main.cpp:314-550
//   * load_index: src/load_index.cpp:8-15, include/index.hpp:122-138 (cereal binary + sdsl::sd_vector, decoded
//     once to plain interleaved words and streamed into HBM)
//   * Result state machine + training: include/result.hpp, include/classify_stats.hpp:34-114,395-584
//   * TSV row: include/read_entry.hpp:322-337
// Host-side columns kept on the CPU as the survey prescribes: mean quality (src/dehost_main.cpp:355-360) and the
// gzip compression ratio (src/utils.cpp:114-124, zlib, computed in an OpenMP loop overlapping nothing yet).
// --extract writes <prefix>_<category>[_1|_2]<ext>.gz like src/dehost_main.cpp:515-536 / include/result.hpp:118-128 (plain gzip
// members; record layout as seqan3's sequence_file_output, which is recalled, not verified).
// `charon classify` (src/classify_main.cpp) shares the loop: call_category for every read, gamma / beta models (--dist), its own defaults.
// .bz2 input: this build's own block-parallel bzip2 decoder (bz2_stream.inc; libbz2 is not in the image).
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <climits>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <future>
#include <deque>
#include <mutex>
#include <thread>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <fcntl.h>
#include <sched.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <unordered_set>
#include <utility>
#include <vector>

#include <zlib.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif
#ifdef _OPENMP
#include <omp.h>
#include <parallel/algorithm>  // __gnu_parallel::sort (libstdc++ parallel mode, OpenMP): the index builder's minimiser sets
#endif

#include "charon_hip.h"
#include "gzip_size.hpp"
#include "../parts/radix_plan.hpp"  // what a chn_hashset_unique call takes in scratch: the index builder weighs it against its budget

#ifndef CHARON_VERSION
#define CHARON_VERSION "charon-mi355x 0.1.0 (reference behaviour: rmcolq/charon @ 2025-07-04)"
#endif

namespace {

// gzip column: bit-exact size emulator (host/gzip_size.hpp) unless CHARON_ZLIB_ONLY is set or the start-up cross-check against
// the linked zlib fails
bool g_gzip_emulator = true;

#include "log_util.inc"
#include "dehost_args.inc"
#include "sdsl_select.inc"
#include "index_file.inc"
#include "inflate_stream.inc"
#include "bz2_stream.inc"
#include "fastx_reader.inc"
#include "result.inc"
#include "run_util.inc"
#include "ordered_merge.inc"
#include "flight_pool.inc"
#include "row_writer.inc"
#include "replica_set.inc"
#include "host_batch.inc"
#include "dehost_modes.inc"
#include "dehost_readers.inc"
#include "dehost_setup.inc"
#include "dehost_flight.inc"
#include "dehost_rows.inc"
#include "dehost_loop.inc"
#include "dehost_resident.inc"
#include "dehost.inc"
#include "index_builder.inc"

}  // namespace

std::string g_inflate_stats;
// CHARON_GPU_INFLATE: 1 = BGZF members are inflated on the device, 0 or unset = on the reader's threads; anything else is an error.
// The device is CHARON_DEVICE, or the first entry of CHARON_DEVICES.
static bool parse_gpu_inflate_env(const DehostArguments *opt) {
    const char *e = std::getenv("CHARON_GPU_INFLATE");
    if (!e) return true;
    const std::string v(e);
    if (v != "0" && v != "1") { std::cerr << "charon: CHARON_GPU_INFLATE: '" << v << "' is neither 0 nor 1" << std::endl; return false; }
    g_gpu_inflate = v == "1";
    if (opt) g_gpu_inflate_device = opt->devices.empty() ? opt->device : opt->devices[0];
    else if (const char *d = std::getenv("CHARON_DEVICE")) g_gpu_inflate_device = std::atoi(d);
    return true;
}
// CHARON_GPU_INFLATE_STREAM: 1 (only together with CHARON_GPU_INFLATE=1) = the chunks of a one-stream .gz are inflated on the device
// (chn_inflate_stream_run), 0 or unset = on the reader's threads; anything else is an error.  Read behind CHARON_GPU_INFLATE: same device.
static bool parse_gpu_inflate_stream_env() {
    const char *e = std::getenv("CHARON_GPU_INFLATE_STREAM");
    if (!e) return true;
    const std::string v(e);
    if (v != "0" && v != "1") { std::cerr << "charon: CHARON_GPU_INFLATE_STREAM: '" << v << "' is neither 0 nor 1" << std::endl; return false; }
    if (v == "1" && !g_gpu_inflate) { std::cerr << "charon: CHARON_GPU_INFLATE_STREAM: takes effect only together with CHARON_GPU_INFLATE=1, which is not set" << std::endl; return false; }
    g_gpu_inflate_stream = v == "1";
    g_gpu_inflate_stream_device = g_gpu_inflate_device;
    return true;
}
// CHARON_GPU_DEFLATE: 1 = the extract files are compressed on the device as BGZF, 0 or unset = by zlib on the -t threads; anything else
// is an error.  The device is CHARON_DEVICE, or the first entry of CHARON_DEVICES.
static bool parse_gpu_deflate_env(const DehostArguments &opt) {
    const char *e = std::getenv("CHARON_GPU_DEFLATE");
    if (!e) return true;
    const std::string v(e);
    if (v != "0" && v != "1") { std::cerr << "charon: CHARON_GPU_DEFLATE: '" << v << "' is neither 0 nor 1" << std::endl; return false; }
    g_gpu_deflate = v == "1";
    g_gpu_deflate_device = opt.devices.empty() ? opt.device : opt.devices[0];
    return true;
}
int main(int argc, char **argv) {
    if (argc < 2) { std::cerr << "A subcommand is required\nRun with --help for more information.\n"; return 106; }
    const std::string sub = argv[1];
    if (sub == "-V" || sub == "--version") { std::cout << CHARON_VERSION << std::endl; return 0; }
    if (sub == "-h" || sub == "--help") {
        std::cout << "Charon: Dehost metagenomic reads\nUsage: charon [OPTIONS] SUBCOMMAND\n\nOptions:\n  -h,--help   Print this help message and exit\n  -V,--version   Show version\n\n"
                     "Subcommands:\n  index    Build an index (IBF) for a number of references split into a small number of bins.\n"
                     "  dehost   Dehost read file into host and other using index.\n"
                     "  classify Classify read file using index.\n";
        return 0;
    }
    if (sub == "_gzsize") {  // hidden diagnostic: per record, gzip size by the linked zlib and by the size emulator (no GPU involved)
        try {
            if (argc < 3) return 2;
            if (const char *t = std::getenv("CHARON_READER_THREADS")) g_reader_threads = std::max(1, std::atoi(t));
            BlockReader in(argv[2]);
            RawBlock blk;
            Deflater d;
            std::cout << "selfcheck\t" << (gzip_emulator_self_check() ? 1 : 0) << "\n";
            while (in.next(blk, 1000, 1u << 24))
                for (const RecView &r : blk.recs) {
                    if (r.seq_len == 0) continue;
                    d.load(r, nullptr);
                    const size_t n = r.seq_len;
                    const uint32_t e = d.sizer.size_padded(reinterpret_cast<const uint8_t *>(d.up.data()), n);
                    std::cout << std::string(r.id, r.id_len) << "\t" << d.zlib_size(n) << "\t" << e << "\n";
                }
            return 0;
        } catch (std::exception &e) { std::cerr << "charon: " << e.what() << std::endl; return 1; }
    }
    if (sub == "_bunzip2") {  // hidden diagnostic: decode a .bz2 with this build's decoder to stdout; block statistics on stderr
        try {
            if (argc < 3) return 2;
            if (const char *t = std::getenv("CHARON_READER_THREADS")) g_reader_threads = std::max(1, std::atoi(t));
            const size_t piece = argc > 3 ? (size_t)std::atol(argv[3]) : ((size_t)64 << 20);
            auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
            const double t0 = now();
            Bz2Source bz;
            bz.open(argv[2]);
            Slab buf;
            unsigned long long total = 0;
            const bool quiet = std::getenv("CHARON_BUNZIP2_QUIET") != nullptr;
            while (!bz.at_end()) {
                buf.clear();
                bz.fill(buf, piece);
                total += buf.size();
                if (!quiet && !buf.empty() && std::fwrite(buf.data(), 1, buf.size(), stdout) != buf.size()) return 1;
            }
            std::fflush(stdout);
            std::cerr << "bunzip2: " << total << " bytes, " << bz.blocks_counted() << " blocks counted, " << bz.blocks_wasted() << " discarded, " << (now() - t0) << " s\n";
            return 0;
        } catch (std::exception &e) { std::cerr << "charon: " << e.what() << std::endl; return 1; }
    }
    if (sub == "_inflate") {  // hidden diagnostic: inflate a .gz with this build's decoder and with zlib; sizes, checksums, rates
        try {
            if (argc < 3) return 2;
            if (const char *t = std::getenv("CHARON_READER_THREADS")) g_reader_threads = std::max(1, std::atoi(t));
            auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
            const size_t piece = argc > 3 ? (size_t)std::atol(argv[3]) : ((size_t)64 << 20);
            unsigned long long total = 0, sum = 1469598103934665603ULL;
            double t0 = now();
            {
                FastInflate fi(argv[2]);
                if (!fi.open()) { std::cerr << "charon: not a mappable gzip file\n"; return 1; }
                Slab buf;
                while (!fi.at_end()) {
                    buf.clear();
                    fi.fill(buf, piece);
                    total += buf.size();
                    sum += buf.empty() ? 0 : (unsigned char)buf[buf.size() / 2];  // (the decoder checks CRC32 / ISIZE itself)
                }
                g_inflate_stats = std::to_string(fi.parallel_rounds()) + " rounds, " + std::to_string(fi.chunks_accepted()) + " chunks counted, " + std::to_string(fi.chunks_discarded()) + " discarded";
            }
            const double t_own = now() - t0;
            std::cout << "parallel: " << g_inflate_stats << "; crc by " << (g_crc_clmul ? "pclmulqdq folding" : "zlib") << "\n";
            unsigned long long ztotal = 0, zsum = 1469598103934665603ULL;
            t0 = now();
            if (!std::getenv("CHARON_SKIP_ZLIB")) {
                gzFile f = gzopen(argv[2], "rb");
                if (!f) return 1;
                gzbuffer(f, 1 << 20);
                std::vector<char> buf(piece + 65536 + 400);
                // the same piece boundaries cannot be reproduced through gzread, so the checksum is over the whole data via one running crc
                unsigned long zc = crc32(0L, Z_NULL, 0);
                for (;;) {
                    const int n = gzread(f, buf.data(), (unsigned)std::min<size_t>(buf.size(), 1u << 30));
                    if (n <= 0) break;
                    ztotal += (unsigned long long)n;
                    zc += (unsigned char)buf[(size_t)n / 2];  // (gzread checks CRC32 / ISIZE itself)
                }
                gzclose(f);
                zsum = zc;
            }
            const double t_z = now() - t0;
            std::cout << "own: " << total << " bytes in " << t_own << " s (" << total / t_own / 1e9 << " GB/s)  zlib: " << ztotal << " bytes in " << t_z << " s ("
                      << ztotal / std::max(t_z, 1e-9) / 1e9 << " GB/s)\n";
            (void)sum; (void)zsum;
            return total == ztotal || std::getenv("CHARON_SKIP_ZLIB") ? 0 : 3;
        } catch (std::exception &e) { std::cerr << "charon: " << e.what() << std::endl; return 1; }
    }
    if (sub == "_find_blocks") {  // hidden diagnostic: _find_blocks <file> <chunk bytes> [first byte]: the reader's own block-start search
        try {                     // (FastInflate::find_block) over the raw file in ranges of that size; "from to found" in bits, "-" for none
            if (argc < 4) return 2;
            const long chunk = std::atol(argv[3]), first = argc > 4 ? std::atol(argv[4]) : 0;
            if (chunk < 1 || first < 0) return 2;
            FastInflate fi(argv[2]);
            if (!fi.open()) { std::cerr << "charon: not a mappable gzip file\n"; return 1; }
            fi.find_blocks_dump((size_t)chunk, (size_t)first, std::cout);
            return 0;
        } catch (std::exception &e) { std::cerr << "charon: " << e.what() << std::endl; return 1; }
    }
    if (sub == "_bgzf_crc") {  // hidden diagnostic: the CRC-32 pass of the reader's threads over the first members of a BGZF file (no GPU involved)
        try {                  // _bgzf_crc <file> <members> <-t value> [repetitions]: what CHARON_GPU_INFLATE=1 no longer does on the host
            if (argc < 5) return 2;
            g_reader_threads = reader_threads_for(std::max(1, std::atoi(argv[4])));
            const size_t want = (size_t)std::atol(argv[3]);
            const int reps = argc > 5 ? std::max(1, std::atoi(argv[5])) : 7;
            std::ifstream f(argv[2], std::ios::binary);
            std::vector<unsigned char> text;
            std::vector<std::pair<size_t, uint32_t>> ms;  // offset in text, size
            std::vector<uint32_t> crcs;
            std::vector<unsigned char> body;
            unsigned char head[18];
            while (ms.size() < want && f.read(reinterpret_cast<char *>(head), 18)) {
                if (head[0] != 0x1f || head[1] != 0x8b || head[3] != 4 || head[12] != 'B' || head[13] != 'C') { std::cerr << "charon: not a BGZF member\n"; return 1; }
                const size_t total = ((size_t)head[16] | ((size_t)head[17] << 8)) + 1;
                body.resize(total - 18);
                if (!f.read(reinterpret_cast<char *>(body.data()), (std::streamsize)body.size())) return 1;
                const unsigned char *tail = body.data() + body.size() - 8;
                const uint32_t crc = (uint32_t)tail[0] | ((uint32_t)tail[1] << 8) | ((uint32_t)tail[2] << 16) | ((uint32_t)tail[3] << 24);
                const uint32_t isize = (uint32_t)tail[4] | ((uint32_t)tail[5] << 8) | ((uint32_t)tail[6] << 16) | ((uint32_t)tail[7] << 24);
                if (isize == 0) continue;
                const size_t at = text.size();
                text.resize(at + isize);
                z_stream zs;
                std::memset(&zs, 0, sizeof zs);
                if (inflateInit2(&zs, -15) != Z_OK) return 1;
                zs.next_in = body.data(); zs.avail_in = (uInt)(body.size() - 8);
                zs.next_out = text.data() + at; zs.avail_out = isize;
                const int rc = inflate(&zs, Z_FINISH);
                inflateEnd(&zs);
                if (rc != Z_STREAM_END || zs.total_out != isize) { std::cerr << "charon: a member does not inflate\n"; return 1; }
                ms.emplace_back(at, isize); crcs.push_back(crc);
            }
            const int nt = std::max(1, std::min<int>(g_reader_threads, (int)ms.size()));
            std::vector<double> secs;
            bool bad = false;
            for (int r = 0; r <= reps; ++r) {  // the loop BgzfSource::fill ran behind chn_inflate_run; the first round warms up
                const double t0 = omp_get_wtime();
#pragma omp parallel for num_threads(nt) schedule(dynamic, 16) reduction(|| : bad)
                for (long i = 0; i < (long)ms.size(); ++i)
                    if (fast_crc32((uint32_t)crc32(0L, Z_NULL, 0), text.data() + ms[(size_t)i].first, ms[(size_t)i].second) != crcs[(size_t)i]) bad = true;
                if (r) secs.push_back(omp_get_wtime() - t0);
            }
            std::sort(secs.begin(), secs.end());
            std::cout << "bgzf_crc: " << ms.size() << " members, " << text.size() << " bytes, " << nt << " threads (" << (g_crc_clmul ? "pclmulqdq folding" : "zlib")
                      << "): min " << secs.front() * 1e3 << " ms  median " << secs[secs.size() / 2] * 1e3 << " ms  max " << secs.back() * 1e3 << " ms -> "
                      << text.size() / secs[secs.size() / 2] / 1e9 << " GB/s (median)" << (bad ? "  CRC MISMATCH" : "") << "\n";
            return bad ? 3 : 0;
        } catch (std::exception &e) { std::cerr << "charon: " << e.what() << std::endl; return 1; }
    }
    if (sub == "_gfmt") {  // hidden self-test: format_g6 against printf's %g on random values of every kind a row holds
        const unsigned long long n = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1000000ULL;
        unsigned long long x = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 1, bad = 0, fast = 0;
        auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
        char a[64], b[64];
        for (unsigned long long i = 0; i < n; ++i) {
            double v;
            const unsigned kind = (unsigned)(rnd() % 8);
            const double u = (double)(rnd() >> 11) / 9007199254740992.0;
            if (kind == 0) v = (double)(float)((double)(rnd() % 5000) / (double)(1 + rnd() % 5000));        // proportions: float(count) / float(n)
            else if (kind == 1) v = (double)((float)(rnd() % 100000) / (float)(1 + rnd() % 100000));
            else if (kind == 2) v = u;                                                                       // probabilities
            else if (kind == 3) v = std::pow(10.0, -12.0 * u) * (double)(rnd() % 10);
            else if (kind == 4) v = (double)(float)(40.0 * u);                                               // mean quality
            else if (kind == 5) v = (double)(rnd() % 2000000) / 2.0 * (rnd() & 1 ? 1.0 : 1e-3);              // exact ties and near-ties
            else if (kind == 6) v = ((double)(rnd() % 1000000) + 0.5) * std::pow(10.0, -(double)(rnd() % 10));
            else { uint64_t bits = rnd(); std::memcpy(&v, &bits, 8); }                                       // anything, NaN and infinities included
            if (rnd() % 16 == 0) v = -v;
            std::snprintf(a, sizeof a, "%g", v);
            const size_t len = format_g6(v, b);
            b[len] = 0;
            if (std::strcmp(a, b) != 0) { if (++bad < 10) std::cout << "mismatch: " << a << " vs " << b << "\n"; }
            const double av = v < 0 ? -v : v;
            if (av >= 1e-4 && av < 999999.0) ++fast;
        }
        std::cout << "format_g6: " << n << " values, " << fast << " in the fast range, " << bad << " mismatches\n";
        return bad ? 1 : 0;
    }
    if (sub == "_efcheck") {  // hidden diagnostic: Elias-Fano arrays written bit by bit in order (add) and by several threads at once (add_at)
        try {
            if (argc < 6) return 2;
            const uint64_t seed = std::strtoull(argv[2], nullptr, 10), nwords = std::strtoull(argv[3], nullptr, 10);
            const double density = std::atof(argv[4]);
            const int threads = std::max(1, std::atoi(argv[5]));
            std::vector<uint64_t> words(nwords);
            uint64_t x = seed * 0x9E3779B97F4A7C15ULL + 1, ones = 0;
            auto rnd = [&x]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
            for (uint64_t i = 0; i < nwords; ++i) {
                uint64_t w = 0;
                for (int b = 0; b < 64; ++b) if ((double)(rnd() >> 11) * (1.0 / 9007199254740992.0) < density) w |= 1ULL << b;
                words[i] = w; ones += (uint64_t)__builtin_popcountll(w);
            }
            EliasFanoWriter a, b;
            a.begin(nwords * 64, ones); b.begin(nwords * 64, ones);
            for (uint64_t i = 0; i < nwords; ++i) { uint64_t w = words[i]; while (w) { a.add(i * 64 + (uint64_t)__builtin_ctzll(w)); w &= w - 1; } }
            // the index builder's own routine, in two blocks so that `before` is exercised too
            const uint64_t half = nwords / 2;
            uint64_t got = ef_add_block(b, words.data(), half, 0, 0, threads);
            got += ef_add_block(b, words.data() + half, nwords - half, half * 64, got, threads);
            const bool same = a.low == b.low && a.high == b.high && a.k == ones && got == ones;
            std::cout << "ones " << ones << " wl " << (int)a.wl << " low words " << a.low.size() << " high words " << a.high.size() << " same " << (same ? 1 : 0) << "\n";
            return same ? 0 : 1;
        } catch (std::exception &e) { std::cerr << "charon: " << e.what() << std::endl; return 1; }
    }
    if (sub == "_selmcl") {  // hidden diagnostic: the two select_support_mcl blocks of a bit vector (u64 bit count + words), built or verified (no GPU involved)
        try {
            if (argc < 6) return 2;
            const std::string mode = argv[2];
            const int threads = std::max(1, std::atoi(argv[5]));
            auto slurp = [](const char *path) {
                std::ifstream f(path, std::ios::binary);
                if (!f) throw std::runtime_error(std::string("cannot open ") + path);
                return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            };
            const std::string bv = slurp(argv[3]);
            if (bv.size() < 8) return 2;
            uint64_t nbits = 0;
            std::memcpy(&nbits, bv.data(), 8);
            std::vector<uint64_t> words((nbits + 63) / 64 + 1, 0);
            if (bv.size() - 8 < (nbits + 63) / 64 * 8) return 2;
            std::memcpy(words.data(), bv.data() + 8, (nbits + 63) / 64 * 8);
            if (mode == "build") {
                std::ofstream o(argv[4], std::ios::binary);
                for (int bit = 1; bit >= 0; --bit) { const std::string b = selmcl::build(words.data(), nbits, bit == 1, threads); o.write(b.data(), (std::streamsize)b.size()); }
                return o ? 0 : 1;
            }
            const std::string blocks = slurp(argv[4]);
            selmcl::TailParser tp{blocks.data(), (uint64_t)blocks.size(), 0, 0};
            selmcl::verify(tp, words.data(), nbits, true, threads);
            selmcl::verify(tp, words.data(), nbits, false, threads);
            if (tp.off != tp.len) tp.fail(std::to_string(tp.len - tp.off) + " bytes follow m_high_0_select");
            std::cout << "select blocks agree with the bit vector\n";
            return 0;
        } catch (std::exception &e) { std::cerr << "charon: " << e.what() << std::endl; return 1; }
    }
    if (sub == "_ordered_merge") {  // hidden diagnostic: the ordered merge of CHARON_DEVICES under producer threads (no GPU involved)
        if (argc < 5) return 2;
        const int threads = std::atoi(argv[2]);
        if (threads < 1 || threads > 256) return 2;
        return ordered_merge_selftest(threads, std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10));
    }
    if (sub == "_records") {  // hidden diagnostic: dump what the block reader sees (no GPU involved unless CHARON_GPU_INFLATE=1)
        try {
            if (argc < 3) return 2;
            if (!parse_gpu_inflate_env(nullptr) || !parse_gpu_inflate_stream_env()) return 1;
            if (const char *t = std::getenv("CHARON_READER_THREADS")) g_reader_threads = std::max(1, std::atoi(t));
            BlockReader in(argv[2]);
            RawBlock blk;
            const size_t max_recs = argc > 3 ? (size_t)std::atol(argv[3]) : 1000, max_bytes = argc > 4 ? (size_t)std::atol(argv[4]) : (1u << 20);
            while (in.next(blk, max_recs, max_bytes))
                for (const RecView &r : blk.recs) {
                    unsigned long long h = 1469598103934665603ULL; long qs = 0;
                    for (uint32_t i = 0; i < r.seq_len; ++i) { h ^= (unsigned char)"ACGTN??"[std::min<unsigned>(g_codes.t[(unsigned char)r.seq[i]], 5)]; h *= 1099511628211ULL; }
                    for (uint32_t i = 0; i < r.qual_len; ++i) qs += r.qual[i] - 33;
                    std::cout << std::string(r.id, r.id_len) << "\t" << r.seq_len << "\t" << r.qual_len << "\t" << qs << "\t" << h << "\n";
                }
            if (std::getenv("CHARON_DIAG_SPLIT")) std::cerr << "split: " << g_split_pieces << " pieces, " << g_split_records << " records taken in parallel\n";
            return 0;
        } catch (std::exception &e) { std::cerr << "charon: " << e.what() << std::endl; return 1; }
    }
    if (sub == "index") {
        IndexArguments iopt;
        try {
            if (const char *e = std::getenv("CHARON_DEVICE")) iopt.device = std::atoi(e);
            if (!parse_index(argc - 2, argv + 2, iopt)) return 0;
        } catch (ParseError &e) {
            std::cerr << e.what() << "\nRun with --help for more information.\n";
            return 105;
        }
        if (const char *e = std::getenv("CHARON_GPU_INDEX_EF")) {
            // CHARON_GPU_INDEX_EF: 1 = the index's Elias-Fano arrays are encoded on the device (chn_index_encode_ef), 0 or unset = by the -t
            // threads from downloaded rows; anything else is an error.  Read by `charon index` alone.
            const std::string v(e);
            if (v != "0" && v != "1") { std::cerr << "charon: CHARON_GPU_INDEX_EF: '" << v << "' is neither 0 nor 1" << std::endl; return 1; }
            iopt.gpu_ef = v == "1";
        }
        if (const char *e = std::getenv("CHARON_GPU_INDEX_SETS")) {
            // CHARON_GPU_INDEX_SETS: 1 = every bin's minimisers stay in device memory, are sorted and made distinct there and emplaced in place
            // (chn_hashset), 0 or unset = they come to the host, are sorted by the -t threads and uploaded again; anything else is an
            // error.  Read by `charon index` alone.
            const std::string v(e);
            if (v != "0" && v != "1") { std::cerr << "charon: CHARON_GPU_INDEX_SETS: '" << v << "' is neither 0 nor 1" << std::endl; return 1; }
            iopt.gpu_sets = v == "1";
        }
        try {
            index_main(iopt);
            return 0;
        } catch (std::exception &e) {
            g_log.error(e.what());
            std::cerr << "charon: " << e.what() << std::endl;
            return 1;
        }
    }
    if (sub != "dehost" && sub != "classify") { std::cerr << "The following argument was not expected: " << sub << "\nRun with --help for more information.\n"; return 109; }
    DehostArguments opt;
    if (sub == "classify") opt.set_classify_defaults();
    try {
        if (const char *e = std::getenv("CHARON_BATCH_READS")) opt.batch_reads = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
        if (const char *e = std::getenv("CHARON_BATCH_BASES")) opt.batch_bases = std::max<uint64_t>(1 << 20, std::strtoull(e, nullptr, 10)) & ~63ULL;
        if (const char *e = std::getenv("CHARON_DEVICE")) opt.device = std::atoi(e);
        if (const char *e = std::getenv("CHARON_MIN_HITS")) opt.min_hits = (uint8_t)std::atoi(e);
        if (!parse_dehost(argc - 2, argv + 2, opt)) return 0;
    } catch (ParseError &e) {
        std::cerr << e.what() << "\nRun with --help for more information.\n";
        return 105;  // CLI11 parse errors exit non-zero through CLI11_PARSE (src/main.cpp:63)
    }
    if (const char *e = std::getenv("CHARON_DEVICES")) {
        // checked before the index file is opened and before any HIP call
        const std::string err = std::getenv("CHARON_DEVICE") ? std::string("cannot be set together with CHARON_DEVICE") : parse_device_list(e, opt);
        if (!err.empty()) { std::cerr << "charon: CHARON_DEVICES: " << err << std::endl; return 1; }
    }
    if (const char *e = std::getenv("CHARON_TEXT_BATCHES")) {
        // checked before the index file is opened and before any HIP call
        const std::string v(e);
        if (v != "0" && v != "1") { std::cerr << "charon: CHARON_TEXT_BATCHES: '" << v << "' is neither 0 nor 1" << std::endl; return 1; }
        opt.text_batches = v == "1";
    }
    if (!parse_gpu_inflate_env(&opt)) return 1;  // checked before the index file is opened and before any HIP call
    if (!parse_gpu_inflate_stream_env()) return 1;  // likewise
    if (!parse_gpu_deflate_env(opt)) return 1;   // likewise
    if (const char *e = std::getenv("CHARON_GPU_TEXT")) {
        // CHARON_GPU_TEXT: 1 = single-end BGZF FASTQ is inflated into device memory and stays there (split, packed and classified on the device of
        // CHARON_DEVICE, or the one entry of CHARON_DEVICES); 0 or unset = not.  Checked before the index file is opened and before any HIP call.
        const std::string v(e);
        if (v != "0" && v != "1") { std::cerr << "charon: CHARON_GPU_TEXT: '" << v << "' is neither 0 nor 1" << std::endl; return 1; }
        g_gpu_text = v == "1";
        g_gpu_text_device = opt.devices.empty() ? opt.device : opt.devices[0];
        if (g_gpu_text && opt.devices.size() > 1) {
            std::cerr << "charon: CHARON_GPU_TEXT: cannot be set together with a CHARON_DEVICES list of several entries (the text lives on one device)" << std::endl;
            return 1;
        }
    }
    if (const char *e = std::getenv("CHARON_GPU_TEXT_PAIRS")) {
        // CHARON_GPU_TEXT_PAIRS: 1 (only together with CHARON_GPU_TEXT=1) = paired BGZF FASTQ stays in device memory as well: two texts, the
        // ids of a pair compared on the device; 0 or unset = not.  Checked before the index file is opened and before any HIP call.
        const std::string v(e);
        if (v != "0" && v != "1") { std::cerr << "charon: CHARON_GPU_TEXT_PAIRS: '" << v << "' is neither 0 nor 1" << std::endl; return 1; }
        if (v == "1" && !g_gpu_text) { std::cerr << "charon: CHARON_GPU_TEXT_PAIRS: takes effect only together with CHARON_GPU_TEXT=1, which is not set" << std::endl; return 1; }
        g_gpu_text_pairs = v == "1";
    }
    if (const char *e = std::getenv("CHARON_GPU_TEXT_FASTA")) {
        // CHARON_GPU_TEXT_FASTA: 1 (only together with CHARON_GPU_TEXT=1) = single-end BGZF FASTA stays in device memory as well: records
        // found and unwrapped by chn_fasta_split; 0 or unset = not.  Checked before the index file is opened and before any HIP call.
        const std::string v(e);
        if (v != "0" && v != "1") { std::cerr << "charon: CHARON_GPU_TEXT_FASTA: '" << v << "' is neither 0 nor 1" << std::endl; return 1; }
        if (v == "1" && !g_gpu_text) { std::cerr << "charon: CHARON_GPU_TEXT_FASTA: takes effect only together with CHARON_GPU_TEXT=1, which is not set" << std::endl; return 1; }
        g_gpu_text_fasta = v == "1";
    }
    if (const char *e = std::getenv("CHARON_GPU_EXTRACT")) {
        // CHARON_GPU_EXTRACT: 1 (only together with CHARON_GPU_TEXT=1 and CHARON_GPU_DEFLATE=1) = under --extract the records of the reads the
        // device-resident loop calls are formed and compressed in device memory (chn_extract); 0 or unset = not.  Checked before the index
        // file is opened and before any HIP call.
        const std::string v(e);
        if (v != "0" && v != "1") { std::cerr << "charon: CHARON_GPU_EXTRACT: '" << v << "' is neither 0 nor 1" << std::endl; return 1; }
        if (v == "1" && !(g_gpu_text && g_gpu_deflate)) {
            std::cerr << "charon: CHARON_GPU_EXTRACT: takes effect only together with CHARON_GPU_TEXT=1 and CHARON_GPU_DEFLATE=1, which are not both set" << std::endl;
            return 1;
        }
        g_gpu_extract = v == "1";
    }
    try {
        dehost_main(opt);  // the reference's subcommand callback discards dehost_main's return value (src/dehost_main.cpp:311)
        return 0;
    } catch (std::exception &e) {
        g_log.error(e.what());
        std::cerr << "charon: " << e.what() << std::endl;
        return 1;
    }
}
