// batch_plan.inc -- the host arithmetic of a batch's chain that makes no HIP call: wavefront counts, the dispatch on bin_words, the layout
// of a slot's result block, the numbers of chn_stream_profile, the SPLIT launch's bound and the gzip column's plan
// Part of the single translation unit charon_hip.hip (behind the kernels' files, whose constants it uses); tools/stream_batch_check.hip
// includes it behind common.inc, len_order.inc and the gzip kernels' files and runs it under the host sanitizers.

// wavefronts of an ordinary launch: one per 64 reads
static inline uint64_t waves_of(uint64_t n) { return (n + WAVE - 1) / WAVE; }

// f(integral_constant<int, W>), W = bin_words: the kernels' instance for an index of W words per row.  chn_index_create admits 1 .. 4
// only; any other value takes the instance for 4, as the hand-written switches did.
template <class F>
static auto by_words(uint64_t W, F f) -> decltype(f(std::integral_constant<int, 1>())) {
    switch (W) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        default: return f(std::integral_constant<int, 4>());
    }
}
// f(integral_constant<int, BITS>): the deflate kernels' form for a batch with N (4-bit codes) or without (2-bit codes: half the LDS, twice
// the wavefronts for long reads)
template <class F>
static void gz_by_bits(int bits, F f) {
    if (bits == 4) f(std::integral_constant<int, 4>());
    else f(std::integral_constant<int, 2>());
}

// layout of a slot's page-locked result block (the order launch_tail's downloads fill it in)
struct ResLayout {
    size_t ctl, prob, nh, counts, unique, call, conf, flags, total;
    ResLayout(uint64_t n, uint64_t C) {
        ctl = 0; prob = CTL_WORDS * 8; nh = prob + n * C * 8; counts = nh + n * 4; unique = counts + n * C * 4; call = unique + n * C * 4;
        conf = call + n; flags = conf + n; total = flags + n;
    }
};

// chn_stream_profile's `which`, by the numbers charon_hip.h documents (10 and 12 were never given out)
enum ProfileWhich {
    PROF_PROBE = 0, PROF_COUNT = 1, PROF_MODEL = 2, PROF_CHAIN = 3,  // a slot's four brackets, in this order in chn_stream::prof_ms / prof_n
    PROF_RERUNS = 4, PROF_FETCHES = 5, PROF_TEXT_UPLOAD = 6, PROF_TEXT_PACK = 7, PROF_TEXT_SPLIT = 8, PROF_TEXT_FETCH = 9, PROF_PAIR_IDS = 11,
    PROF_GATED = 13, PROF_FASTA_SPLIT = 14
};
static inline bool profile_which_ok(int which) { return which >= 0 && which <= 14 && which != 10 && which != 12; }

// Most reads the SPLIT launch can meet in a batch, as far as the host can tell: exact for a host batch (h_len1: its first segments'
// lengths), all n of them for a device batch (null; its segments may overlap: any number of its reads can be long).  0: no launch.
static uint32_t split_bound(uint32_t long_bucket, bool paired, const std::vector<uint32_t> *h_len1, uint64_t n) {
    if (paired || long_bucket >= 256) return 0;
    if (!h_len1) return (uint32_t)n;
    const uint32_t floor_len = len_bucket_floor(long_bucket);
    uint64_t c = 0;
    for (uint32_t L : *h_len1) c += L >= floor_len;
    return (uint32_t)c;
}

// ---- the gzip column's plan for a host batch ----
// Counting sort of the read numbers by OCCUPANCY class: class w holds the reads of which w wavefronts fit a CU's LDS (2.5 bytes per
// letter); reads short enough for 16 and more share class 16.  One k_gzip_tally launch per class in use, its LDS sized for the longest
// read of the class in this batch -- few launches with many reads each (512-letter classes left a long-read batch with some 90 launches
// of 30 reads on a 256-CU device).
// all_sizes (CHN_GZIP_SIZES_ALL): behind the class lists, the reads beyond GZT_MAX_LEN (longest first, equal lengths by read number),
// then the tallied reads long enough to reach a second deflate block (at least GZT_SYMBOL_LIMIT letters), in class-list order.
enum { GZ_NCLS = 17 };  // classes 1 .. 16 (0 unused)
struct GzPlan {
    uint32_t start[GZ_NCLS + 1];  // class c's reads are index[start[c] .. start[c + 1])
    uint32_t cmax[GZ_NCLS];       // its longest read
    size_t long_at, rerun_at;     // index[long_at .. rerun_at): beyond the tally kernel's reach; index[rerun_at ..): may be handed back
};
// len2: null for single reads.  bound: the longest read to tally (at most GZT_MAX_LEN); long_bound: the longest to size at all.
static GzPlan gz_plan(const uint32_t *len1, const uint32_t *len2, uint64_t n, int bits, uint32_t bound, uint32_t long_bound, bool all_sizes,
                      std::vector<uint32_t> &index) {
    const size_t lds_cu = (size_t)160 * 1024;
    GzPlan p;
    std::memset(&p, 0, sizeof p);
    auto len_of = [&](uint64_t i) { return (uint64_t)len1[i] + (len2 ? len2[i] : 0); };
    auto cls_of = [&](uint64_t i, uint32_t &L32) -> uint32_t {
        const uint64_t L = len_of(i);
        if (L == 0 || L > bound) return GZ_NCLS;
        L32 = (uint32_t)L;
        return (uint32_t)std::min<size_t>(16, std::max<size_t>(1, lds_cu / gzt_lds_bytes(L32, bits)));
    };
    for (uint64_t i = 0; i < n; ++i) { uint32_t L = 0; const uint32_t c = cls_of(i, L); if (c < GZ_NCLS) { ++p.start[c + 1]; p.cmax[c] = std::max(p.cmax[c], L); } }
    for (uint32_t c = 0; c < GZ_NCLS; ++c) p.start[c + 1] += p.start[c];
    index.resize(p.start[GZ_NCLS]);
    {
        uint32_t fill[GZ_NCLS];
        std::memcpy(fill, p.start, sizeof fill);
        for (uint64_t i = 0; i < n; ++i) { uint32_t L = 0; const uint32_t c = cls_of(i, L); if (c < GZ_NCLS) index[fill[c]++] = (uint32_t)i; }
    }
    p.long_at = p.rerun_at = index.size();
    if (all_sizes) {
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t L = len_of(i);
            if (L > GZT_MAX_LEN && L <= long_bound && L <= GZL_MAX_READ) index.push_back((uint32_t)i);
        }
        std::sort(index.begin() + p.long_at, index.end(), [&](uint32_t x, uint32_t y) {
            const uint64_t lx = len_of(x), ly = len_of(y);
            return lx != ly ? lx > ly : x < y;
        });
        p.rerun_at = index.size();
        for (size_t j = 0; j < p.long_at; ++j) {
            const uint32_t i = index[j];
            if (len_of(i) >= GZT_SYMBOL_LIMIT) index.push_back(i);
        }
    }
    return p;
}
