// gzip_size_dev.inc -- k_gzip_size: _tr_flush_block's arithmetic on the deflate tallies of k_gzip_tally, one lane per read
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.

// ------------------------------------------------------------------------------------------------
// The size of the gzip member zlib would write for a read = 18 bytes of header and trailer + the bits of ONE deflate block whose
// symbol frequencies k_gzip_tally counted: trees.c's Huffman trees and the stored / static / dynamic choice of _tr_flush_block,
// restated once for the device and the host in gzip_trees.inc (gztrees::flush_block_bits; zlib is the checker:
// tests/test_gpu_parity.py::test_gzip_sizes_on_the_device_equal_zlib).  The algorithm is a sequential heap walk per
// read with data-dependent control flow, so it runs one LANE per read with its arrays in private memory -- some 10 000 divergent
// instructions per read, a millisecond or two per batch beside the tally kernel's 20+, and it takes 1.7 us per read off the host
// (the whole of the main thread's sizing loop at -t 1) and 640 bytes per read off the download.
// ------------------------------------------------------------------------------------------------
struct GzSizeArgs {
    const uint16_t *tallies;  // [n][GZT_WORDS]
    const uint32_t *len1, *len2;
    uint32_t n_reads;
    uint32_t *sizes;          // [n]: gzip member size in bytes, 0 = not tallied on the device (size it on the host)
    const uint32_t *long_sizes;  // [n] or null: what k_gzip_long found for the reads the tallies hand back (CHN_GZIP_SIZES_ALL)
};

__global__ __launch_bounds__(WAVE) void k_gzip_size(const GzSizeArgs a) {
    using namespace gztrees;
    const uint32_t r = blockIdx.x * WAVE + threadIdx.x;
    if (r >= a.n_reads) return;
    const uint16_t *t = a.tallies + (size_t)r * GZT_WORDS;
    if (t[316] != 0) { a.sizes[r] = a.long_sizes ? a.long_sizes[r] : 0u; return; }
    const uint64_t stored_len = (uint64_t)a.len1[r] + (a.len2 ? a.len2[r] : 0u);
    Work w;
    uint64_t bits = 0;
    flush_block_bits(w, t, t + 286, stored_len, true, true, bits);
    a.sizes[r] = (uint32_t)(18 + (bits >> 3));
}
