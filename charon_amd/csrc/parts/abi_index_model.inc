// abi_index_model.inc -- host objects (index, batch slot, the text calls' scratch, stream); chn_index_* entry points; chn_model_default
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.

// ------------------------------------------------------------------------------------------------
// host objects
// ------------------------------------------------------------------------------------------------
struct chn_index {
    chn_index_desc d;
    uint64_t *words = nullptr;
    uint64_t rows_local = 0;
    bool single_bin_categories = false;  // every category owns exactly one bin
    // chn_index_decode_ef: a stream of its own and two sets of device buffers (slice i's kernels run while slice i + 1 is copied in); kept from
    // slice to slice (five hipMalloc / hipFree pairs per slice otherwise, each hipFree a device-wide wait); released with the index or when its
    // first stream is made
    hipStream_t ef_stream = nullptr;
    hipEvent_t ef_copied = nullptr;
    void *ef_buf[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};  // high, low, block counts, block prefix
    size_t ef_cap[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    unsigned long long *ef_bad = nullptr;
    unsigned ef_turn = 0;
    void ef_release() {
        if (ef_stream) (void)hipStreamSynchronize(ef_stream);
        for (int k = 0; k < 2; ++k)
            for (int i = 0; i < 4; ++i) { if (ef_buf[k][i]) (void)hipFree(ef_buf[k][i]); ef_buf[k][i] = nullptr; ef_cap[k][i] = 0; }
        if (ef_bad) (void)hipFree(ef_bad);
        ef_bad = nullptr;
        if (ef_copied) (void)hipEventDestroy(ef_copied);
        ef_copied = nullptr;
        if (ef_stream) (void)hipStreamDestroy(ef_stream);
        ef_stream = nullptr;
    }
};

struct HostModel {  // deep copy of chn_model
    bool set = false;
    uint32_t C = 0;
    std::vector<std::vector<float>> pos, neg;
    float h_pos = 0.1f, h_neg = 0.001f, rate = 300.0f;
    float min_quality = 15.0f, min_compression = 0, cpt = 0, lo_thr = 0.05f, min_pd = 0.04f, min_prd = 0;
    uint32_t min_length = 140;
    int8_t conf_thr = 7;
    uint8_t min_hits = 0, paired = 0, host_index = 0;
    uint32_t dist = CHN_DIST_KDE;
    std::vector<float> dparams;  // [C][6] (gamma / beta), as K3Args::dparams
};

// Row-log scratch of one batch (general bin layouts): compact entries, escaped full rows, per-wavefront region table.
// Sized from an expected minimiser density (twice that of random sequence), not from the worst case of one emission per base:
// k_minimise_probe reports a wavefront that would overrun its region and chn_batch_wait then re-runs the batch on the
// stream's worst-case buffers (allocated only then).
struct LogBuf {
    DevBuf log, rows, meta, wcount;
    uint64_t log_cap = 0, esc_cap = 0;  // entries / rows
    uint32_t cap_num = 65536, esc_shift = 0;
    // n_waves: wavefront logs that can be in use at once (their rounding slack is part of the capacity); n_slots >= n_waves: entries of the
    // per-wavefront tables (every read of a device batch may turn out to be a long one with a wavefront of its own)
    int ensure(uint64_t sum_len, uint64_t n_waves, uint32_t W, uint32_t cap_num_, uint32_t esc_shift_, uint64_t n_slots = 0) {
        cap_num = cap_num_; esc_shift = esc_shift_;
        n_slots = std::max(n_slots, n_waves);
        const uint64_t lc = ((sum_len * cap_num) >> 16) + 128 * n_waves + 64, ec = (lc >> esc_shift) + 65 * n_waves + 64;
        int rc;
        if ((rc = log.ensure(lc * 4)) || (rc = rows.ensure(ec * W * 8)) || (rc = meta.ensure((n_slots + 1) * sizeof(WaveMeta))) || (rc = wcount.ensure(n_slots * 4))) return rc;
        log_cap = lc; esc_cap = ec;
        return CHN_OK;
    }
    void release() { log.release(); rows.release(); meta.release(); wcount.release(); log_cap = esc_cap = 0; }
};

// A profiling bracket: two timed events around a piece of a batch's work, and whether this batch recorded them.
struct EvBracket {
    hipEvent_t begin = nullptr, end = nullptr;
    bool used = false;
};

// Per-batch state.  Two slots let batch i+1 be submitted while batch i's count and model+call kernels (side stream) are still
// running: they then overlap the HBM-bound minimise+probe kernel of the next batch.
struct Slot {
    DevBuf d_num_hashes, d_counts, d_unique, d_prob, d_call, d_conf, d_flags;
    DevBuf d_ctl;                         // CTL_WORDS control words (len_order.inc): byte counter, log cursors, status
    DevBuf d_gzt, d_gzidx, d_gzsize, d_gzctr;                // deflate tallies of this batch (chn_batch.gzip_tallies); read indices by occupancy class; the launches' read counters
    std::vector<uint32_t> h_gzidx;
    bool want_gzt = false;
    // results of a host batch are downloaded IN STREAM, right behind the kernels that produce them and ahead of the next batch's
    // kernels on the same streams (a copy issued from chn_batch_wait would queue behind the next batch's work)
    PinBuf h_res, h_gzt, h_gzsize;
    bool staged = false, gz_staged = false;
    uint32_t gz_output = 0;
    hipEvent_t bases_up = nullptr, gz_done = nullptr;
    DevBuf d_gzlong;                      // CHN_GZIP_SIZES_ALL: k_gzip_long's sizes [max_reads], then its launches' read counters [64]
    hipEvent_t gzt_done = nullptr;        // ... the tally launches (tally stream) are done: the long-gzip stream forms the sizes behind them and its long-read launch
    DevBuf d_order;                       // length-class order of this batch (read by the count kernel on the side stream)
    LogBuf lb;                            // this batch's row log
    DevBuf d_len1, d_len2, d_mq, d_comp;  // staging of the small per-read arrays of host batches (read by k_model_call)
    DevBuf d_bases, d_nmask, d_off1, d_off2;  // staging of the large arrays: per slot, so batch i+1 uploads while batch i computes
    // text batches (abi_text_batch.inc; allocated with the first one): the uploaded text with 64 bytes of padding at both ends, the
    // byte offsets and quality lengths of its reads, k_text_pack's three words; page-locked staging of those words and of the
    // mean-quality column
    DevBuf d_text, d_tdesc, d_tctl;
    PinBuf h_text;
    std::vector<uint64_t> h_toff1, h_toff2;  // the segment layout chn_text_submit computed
    bool is_text = false;
    EvBracket t_text_upload, t_text_pack;  // profiling streams: the text's upload; k_text_pack + k_text_mq (made by the first text batch)
    uint32_t text_has_n = 0;
    uint64_t text_n_bases = 0;
    hipEvent_t uploaded = nullptr;
    const uint32_t *len1 = nullptr, *len2 = nullptr;
    const float *mq = nullptr, *comp = nullptr;
    uint64_t n_reads = 0;
    bool host_batch = false, model_ran = false, fused = false, list_mode = false;
    K1Args k1;                            // the launch arguments of this batch's minimise+probe kernel (re-run after a log overflow)
    std::vector<uint32_t> h_len1, h_len2;
    std::vector<float> h_mq, h_comp;
    // profiling streams: the probe kernel (both its launches), the count kernels, model + call, the whole chain from the probe
    // stream's first call of the batch to the last kernel on the side stream
    EvBracket t_probe, t_count, t_model, t_chain;
    hipEvent_t k1_done = nullptr, done = nullptr, split_done = nullptr;
    bool new_anchor = false;              // profiling streams: the stream's next time anchor was recorded behind this batch's probe kernel
    uint32_t split_bound = 0;            // most reads this batch's SPLIT launch (long reads over the lanes of a wavefront) can meet; 0: no such launch
};

// chn_text_split's scratch (abi_text_split.inc; allocated with the first call): tile counts and offsets, line starts, the descriptor
// columns, id positions, the ids back to back, the control words and their page-locked copy
struct TextSplitScratch {
    DevBuf d_tile, d_line, d_desc, d_idpos, d_ids, d_ctl;
    PinBuf h_ctl;
    CallTimer timer;  // profiling streams: around the kernels in front of the first wait
    void release() { d_tile.release(); d_line.release(); d_desc.release(); d_idpos.release(); d_ids.release(); d_ctl.release(); h_ctl.release(); timer.release(); }
};

// chn_text_fetch's staging (abi_text_fetch.inc; allocated with the first call): the range descriptors page-locked and on the device,
// the gathered bytes on the device and page-locked
struct TextFetchScratch {
    DevBuf d_desc, d_out;
    PinBuf h_desc, h_out;
    CallTimer timer;  // profiling streams: around the kernel
    void release() { d_desc.release(); d_out.release(); h_desc.release(); h_out.release(); timer.release(); }
};

// chn_text_pair_ids' staging (abi_text_pair.inc; allocated with the first call): the id descriptors of both files page-locked and on
// the device, the kernel's one word on the device and page-locked
struct TextPairScratch {
    DevBuf d_desc, d_first;
    PinBuf h_desc, h_first;
    CallTimer timer;  // profiling streams: around the kernel
    void release() { d_desc.release(); d_first.release(); h_desc.release(); h_first.release(); timer.release(); }
};

struct chn_stream {
    chn_index *idx = nullptr;
    chn_stream_cfg cfg;
    // The seven streams of a batch's chain (stream_roles, abi_stream_batch.inc, lists them with their priorities):
    hipStream_t q_probe[2] = {nullptr, nullptr};  // minimise+probe: [0] the even batches, the list-mode chains, chn_classify_counts, re-runs after a log overflow;
                                                  // [1] the odd batches: the next batch's wavefronts take the slots a draining grid frees
    hipStream_t q_side = nullptr;    // count + model+call (overlap the next batch's minimise+probe)
    hipStream_t q_copy = nullptr;    // host -> device uploads of host batches (truly asynchronous when the caller's memory is pinned), the ordering kernels, the text calls
    hipStream_t q_tally = nullptr;   // deflate tallies (latency-bound LDS work beside the HBM-bound probe kernel)
    hipStream_t q_split = nullptr;   // the SPLIT launch of k_minimise_probe (long reads), beside the ordinary launch
    hipStream_t q_gzlong = nullptr;  // k_gzip_long on the reads beyond CHN_GZIP_MAX_LEN (CHN_GZIP_SIZES_ALL), beside the tally launches (created with the first such batch)
    uint32_t long_bucket = 104;     // reads from this length class on are split over the lanes of a wavefront (256: never)
    DevBuf d_hist, d_model;
    DevBuf d_memo;                    // k_model_call memo table (cleared whenever the model changes)
    LogBuf big;                       // worst-case row log: re-runs after an overflow, dense row-sharded mode, chn_minimisers
    DevBuf d_list, d_cbase;           // row-sharded modes: minimiser value log, compact entry offsets (dense)
    uint64_t shard_entries = 0;
    bool shard_open = false;
    LogBuf shx;                       // sparse row-sharded mode: density-sized row log
    DevBuf d_shx_cnt;                 // [n_ranks][n_waves + 1] probe counts / offsets
    ShxArgs shx_args;
    int shx_stage = 0;                // 0 idle, 1 minimised, 2 counted, 3 queries written
    uint32_t cap_num = 65536, esc_shift = 0;  // sizing of the per-slot row logs (LogBuf)
    uint64_t overflow_reruns = 0;
    bool gzt_big_lds = false;         // k_gzip_tally's dynamic-LDS limit has been raised
    DevBuf d_gzscratch;               // k_gzip_tally's per-wavefront class arrays (shared by the launches of the stream, which run one after the other)
    DevBuf d_gzlscratch[2];           // k_gzip_long's per-wavefront epoch arrays: [0] its launches on the long-gzip stream, [1] the re-runs on the tally stream
    bool gzl_big_lds = false;         // k_gzip_long's dynamic-LDS limit has been raised
    uint32_t n_cus = 256;             // compute units of the device
    static const int N_SLOTS = 3;  // batches that may be in flight at once
    Slot slot[N_SLOTS];
    PinBuf h_block;    // the slots' result staging in one allocation (small streams)
    int head = 0;      // slot of the next submit
    int inflight = 0;  // batches submitted and not yet waited for (FIFO)
    uint64_t batch_seq = 0;  // whole-chain batches submitted so far: batch i's probe kernel runs on probe stream i & 1
    bool last_had_long = false;  // the batch waited for last had reads for the SPLIT launch: while that is so, every batch takes the first probe stream
    // The probe gate: a batch's ordinary launch waits in its queue (hipStreamWaitValue64) until *gate_signal has reached the value of the
    // gated batch before it, which that batch's grid writes when its last workgroup has started and a one-thread kernel behind the grid
    // writes again.  Every wait names a value whose writers this thread has already enqueued on this chn_stream.
    unsigned long long *gate_signal = nullptr;  // signal memory, zero at creation; null: no gate (no device support, CHN_STREAM_NO_PROBE_GATE)
    uint64_t gate_seq = 0;                      // value of the last gated batch whose writers are enqueued (0: none yet)
    uint64_t gated_batches = 0;                 // launches queued behind a gate wait (chn_stream_profile, which = 13)
    HostModel model;
    K3Args k3;
    // chn_classify_counts(_raw): inputs and outputs of k_model_call on the caller's counts.  A set of its own (allocated on first use,
    // max_reads rows): a batch slot's buffers may hold device-resident results the caller still reads
    struct CountsBufs { DevBuf num_hashes, counts, unique, len1, mq, comp, prob, call, conf, flags; } cc;
    // profiling
    double prof_ms[4] = {0, 0, 0, 0};
    uint64_t prof_n[4] = {0, 0, 0, 0};
    // prof_ms[0] is the time ATTRIBUTABLE to a batch's probe kernel: the part of its interval behind the end of the probe kernels
    // waited for before it (two probe grids overlap; bracket times would count the shared time twice).  A slot's events are
    // re-recorded by the third-next submit, so that end is kept as milliseconds behind an anchor event, and the anchor moves on
    // (prof_anchor[prof_cur ^ 1], recorded behind a batch's probe kernel, takes over when that batch is waited for) before a float
    // of milliseconds loses the 0.01 ms
    hipEvent_t prof_anchor[2] = {nullptr, nullptr};
    int prof_cur = 0;
    bool prof_anchor_pending = false, prof_have_end = false;
    double prof_prev_end = 0;  // ms behind prof_anchor[prof_cur]
    std::chrono::steady_clock::time_point prof_anchor_at;
    uint64_t last_bytes = 0, last_min = 0, last_fetches = 0;
    double text_ms[2] = {0, 0};  // text batches of a profiling stream: upload of the text, pack kernels
    uint64_t text_n = 0;
    TextSplitScratch tsp;
    TextSplitScratch fsp;  // chn_fasta_split's (abi_fasta_split.inc): tile summaries and sums in d_tile, header ranks in d_line
    TextFetchScratch txg;
    TextPairScratch tpi;
};

// What chn_text_split, chn_fasta_split, chn_text_fetch and chn_text_pair_ids do between their job check and their text check: a stream
// with three batches in flight has no idle copy stream to offer; the stream's device is selected and handed back.
static int stream_text_call(chn_stream *s, const char *who, int *device_out) {
    if (s->inflight >= chn_stream::N_SLOTS) return fail(CHN_E_INVALID, std::string(who) + ": three batches in flight on the stream: call chn_batch_wait first");
    const int device = s->idx->d.device;
    HIPCHK(hipSetDevice(device));
    *device_out = device;
    return CHN_OK;
}

// seconds on the steady clock: every host time point of the submit / wait diagnostics (CHN_DIAG_SUBMIT, CHN_DIAG_WAIT)
static double wall_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static uint64_t pow5(unsigned e) { uint64_t p = 1; while (e--) p *= 5; return p; }

extern "C" int chn_index_create(const chn_index_desc *desc, chn_index **out) {
    if (!desc || !out || desc->struct_size != sizeof(chn_index_desc)) return fail(CHN_E_INVALID, "chn_index_create: bad descriptor");
    const chn_index_desc &d = *desc;
    if (d.kmer_size < 1 || d.kmer_size > 27) return fail(CHN_E_INVALID, "kmer_size must be in 1..27 (5^k has to fit 64 bits)");
    if (d.window_size < d.kmer_size) return fail(CHN_E_INVALID, "window_size must be >= kmer_size");
    if (d.hash_funs < 1 || d.hash_funs > 5) return fail(CHN_E_INVALID, "hash_funs must be in 1..5");
    if (d.bins < 1 || d.bins > 255 || d.technical_bins != ((d.bins + 63) / 64) * 64 || d.bin_words != d.technical_bins / 64)
        return fail(CHN_E_INVALID, "IBF header inconsistent: technical_bins must be 64*ceil(bins/64), bin_words = technical_bins/64");
    if (d.bin_size == 0 || d.hash_shift != (uint64_t)__builtin_clzll(d.bin_size)) return fail(CHN_E_INVALID, "hash_shift must be countl_zero(bin_size)");
    if (d.num_categories < 1) return fail(CHN_E_INVALID, "num_categories must be >= 1");
    for (uint64_t b = 0; b < d.bins; ++b)
        if (d.bin_to_category[b] >= d.num_categories) return fail(CHN_E_INVALID, "bin_to_category entry out of range");
    chn_index *idx = new (std::nothrow) chn_index();
    if (!idx) return fail(CHN_E_NOMEM, "host allocation failed");
    idx->d = d;
    if (idx->d.row_begin == 0 && idx->d.row_end == 0) idx->d.row_end = d.bin_size;
    if (idx->d.row_end > d.bin_size || idx->d.row_begin >= idx->d.row_end) { delete idx; return fail(CHN_E_INVALID, "bad row shard"); }
    idx->rows_local = idx->d.row_end - idx->d.row_begin;
    std::vector<int> per_cat(d.num_categories, 0);
    for (uint64_t b = 0; b < d.bins; ++b) per_cat[d.bin_to_category[b]]++;
    idx->single_bin_categories = true;
    for (int c : per_cat) if (c != 1) idx->single_bin_categories = false;
    hipError_t e = hipSetDevice(d.device);
    // + 64 bytes: a probe fetches whole 16-byte blocks (LDS-DMA), the block of the last row may reach past the last word
    if (e == hipSuccess) e = hipMalloc((void **)&idx->words, idx->rows_local * d.bin_words * 8 + 64);
    if (e != hipSuccess) { delete idx; return fail(e == hipErrorOutOfMemory ? CHN_E_NOMEM : CHN_E_HIP, std::string("index allocation: ") + hipGetErrorString(e)); }
    e = hipMemset(idx->words, 0, idx->rows_local * d.bin_words * 8 + 64);
    if (e != hipSuccess) { (void)hipFree(idx->words); delete idx; return fail(CHN_E_HIP, std::string("index memset: ") + hipGetErrorString(e)); }
    *out = idx;
    return CHN_OK;
}

// Work queued on the index's own stream (Elias-Fano slices, a replica's copy) is waited for on the host before the words are read or
// written through the null stream: ef_stream is a blocking stream, but the ordering is stated here rather than left to the legacy
// null-stream semantics.
static int index_wait_queued(chn_index *idx) {
    if (idx->ef_stream) HIPCHK(hipStreamSynchronize(idx->ef_stream));
    return CHN_OK;
}

extern "C" int chn_index_upload_rows(chn_index *idx, uint64_t row_begin, uint64_t n_rows, const uint64_t *host_words) {
    if (!idx || !host_words) return fail(CHN_E_INVALID, "chn_index_upload_rows: null argument");
    if (row_begin < idx->d.row_begin || row_begin + n_rows > idx->d.row_end) return fail(CHN_E_INVALID, "rows outside this shard");
    HIPCHK(hipSetDevice(idx->d.device));
    if (const int rc = index_wait_queued(idx)) return rc;
    HIPCHK(hipMemcpy(idx->words + (row_begin - idx->d.row_begin) * idx->d.bin_words, host_words, n_rows * idx->d.bin_words * 8, hipMemcpyHostToDevice));
    return CHN_OK;
}
extern "C" int chn_index_download_rows(chn_index *idx, uint64_t row_begin, uint64_t n_rows, uint64_t *host_words) {
    if (!idx || !host_words) return fail(CHN_E_INVALID, "chn_index_download_rows: null argument");
    if (row_begin < idx->d.row_begin || row_begin + n_rows > idx->d.row_end) return fail(CHN_E_INVALID, "rows outside this shard");
    HIPCHK(hipSetDevice(idx->d.device));
    if (const int rc = index_wait_queued(idx)) return rc;
    HIPCHK(hipMemcpy(host_words, idx->words + (row_begin - idx->d.row_begin) * idx->d.bin_words, n_rows * idx->d.bin_words * 8, hipMemcpyDeviceToHost));
    return CHN_OK;
}
extern "C" int chn_index_decode_ef(chn_index *idx, uint64_t m_size, uint32_t wl, const uint64_t *high, uint64_t high_bit0, uint64_t n_high_words,
                                   uint64_t ones_before, const uint64_t *low, uint64_t low_elem0, uint64_t n_low_words, uint64_t *bad_bits) {
    if (!idx || !high || (wl && n_high_words && !low) || !bad_bits) return fail(CHN_E_INVALID, "chn_index_decode_ef: null argument");
    if ((high_bit0 & 63) || wl > 64 || low_elem0 > ones_before) return fail(CHN_E_INVALID, "chn_index_decode_ef: bad slice description");
    const chn_index_desc &d = idx->d;
    if (m_size != d.technical_bins * d.bin_size) return fail(CHN_E_INVALID, "chn_index_decode_ef: m_size != technical_bins * bin_size");
    if (n_high_words > (1ULL << 31)) return fail(CHN_E_INVALID, "chn_index_decode_ef: slice too large (at most 2^31 words)");
    HIPCHK(hipSetDevice(d.device));
    *bad_bits = 0;
    if (!idx->ef_bad) {
        if (n_high_words == 0) return index_wait_queued(idx);  // nothing was ever decoded (a replica's copy may be in flight)
        if (!idx->ef_stream) HIPCHK(hipStreamCreate(&idx->ef_stream));
        HIPCHK(hipEventCreateWithFlags(&idx->ef_copied, hipEventDisableTiming));
        HIPCHK(hipMalloc((void **)&idx->ef_bad, 8));
        HIPCHK(hipMemsetAsync(idx->ef_bad, 0, 8, idx->ef_stream));
    }
    hipStream_t st = idx->ef_stream;
    if (n_high_words == 0) {  // the last call: wait for the slices in flight, report what they found
        unsigned long long bad = 0;
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(&bad, idx->ef_bad, 8, hipMemcpyDeviceToHost));
        *bad_bits = bad;
        return CHN_OK;
    }
    // The slice's chain -- copy in, ones per block, their prefix, decode -- is queued on the index's own stream and runs while the caller
    // prepares the next slice; the call returns once its host buffers have been read (give it page-locked memory and that is all it waits for).
    const uint64_t n_blocks = (n_high_words + 255) / 256;
    const unsigned set = idx->ef_turn++ & 1u;
    const size_t want[4] = {(size_t)n_high_words * 8, (size_t)(n_low_words + 2) * 8, (size_t)n_blocks * 4, (size_t)n_blocks * 8};
    for (int i = 0; i < 4; ++i)
        if (want[i] > idx->ef_cap[set][i]) {
            HIPCHK(hipStreamSynchronize(st));  // (the buffer may be in use by the slice before the last)
            if (idx->ef_buf[set][i]) { (void)hipFree(idx->ef_buf[set][i]); idx->ef_buf[set][i] = nullptr; idx->ef_cap[set][i] = 0; }
            hipError_t e = hipMalloc(&idx->ef_buf[set][i], want[i] + want[i] / 8);
            if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CHN_E_NOMEM : CHN_E_HIP, std::string("chn_index_decode_ef: ") + hipGetErrorString(e));
            idx->ef_cap[set][i] = want[i] + want[i] / 8;
        }
    uint64_t *d_high = static_cast<uint64_t *>(idx->ef_buf[set][0]), *d_low = static_cast<uint64_t *>(idx->ef_buf[set][1]);
    uint32_t *d_counts = static_cast<uint32_t *>(idx->ef_buf[set][2]);
    uint64_t *d_prefix = static_cast<uint64_t *>(idx->ef_buf[set][3]);
    HIPCHK(hipMemcpyAsync(d_high, high, n_high_words * 8, hipMemcpyHostToDevice, st));
    if (n_low_words) HIPCHK(hipMemcpyAsync(d_low, low, n_low_words * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_low + n_low_words, 0, 16, st));  // the decode reads one word past an element that ends the slice
    HIPCHK(hipEventRecord(idx->ef_copied, st));
    hipLaunchKernelGGL(k_ef_block_counts, dim3((uint32_t)n_blocks), dim3(256), 0, st, d_high, n_high_words, d_counts);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_ef_block_prefix, dim3(1), dim3(SCAN_THREADS), 0, st, d_counts, n_blocks, d_prefix);
    HIPCHK(hipGetLastError());
    EfArgs a;
    a.high = d_high; a.low = d_low; a.n_high_words = n_high_words; a.high_bit0 = high_bit0; a.ones_before = ones_before; a.low_elem0 = low_elem0;
    a.m_size = m_size; a.row_begin = d.row_begin; a.row_end = d.row_end; a.words = idx->words; a.bad = idx->ef_bad; a.wl = wl;
    a.W = (uint32_t)d.bin_words; a.B = (uint32_t)d.bins; a.TB = (uint32_t)d.technical_bins;
    hipLaunchKernelGGL(k_ef_decode, dim3((uint32_t)n_blocks), dim3(256), 0, st, a, d_prefix);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventSynchronize(idx->ef_copied));
    return CHN_OK;
}

extern "C" int chn_index_bin_popcounts(chn_index *idx, uint64_t *out) {
    if (!idx || !out) return fail(CHN_E_INVALID, "chn_index_bin_popcounts: null argument");
    const chn_index_desc &d = idx->d;
    HIPCHK(hipSetDevice(d.device));
    if (const int rc = index_wait_queued(idx)) return rc;  // slices still being decoded, a replica's copy
    unsigned long long *d_out = nullptr;
    HIPCHK(hipMalloc((void **)&d_out, d.technical_bins * 8));
    HIPCHK(hipMemset(d_out, 0, d.technical_bins * 8));
    hipLaunchKernelGGL(k_bin_popcounts, dim3(4096), dim3(256), 0, 0, idx->words, idx->rows_local, (uint32_t)d.bin_words, d_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, d.technical_bins * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(CHN_E_HIP, std::string("chn_index_bin_popcounts: ") + hipGetErrorString(e));
    return CHN_OK;
}

extern "C" int chn_index_device_words(chn_index *idx, uint64_t **device_words, uint64_t *n_words) {
    if (!idx) return fail(CHN_E_INVALID, "null index");
    if (device_words) *device_words = idx->words;
    if (n_words) *n_words = idx->rows_local * idx->d.bin_words;
    return CHN_OK;
}
extern "C" int chn_index_get_desc(const chn_index *idx, chn_index_desc *out) {
    if (!idx || !out) return fail(CHN_E_INVALID, "null argument");
    *out = idx->d;
    return CHN_OK;
}
extern "C" int chn_device_count(int *count) {
    if (!count) return fail(CHN_E_INVALID, "chn_device_count: null argument");
    *count = 0;
    HIPCHK(hipGetDeviceCount(count));
    return CHN_OK;
}
// One hipMemcpyPeerAsync of the source's words (the zeroed 64-byte tail included) on the replica's own stream (ef_stream, which every call that
// reads or writes the words waits for).  Peer access is neither enabled nor required: the runtime stages a copy between devices without it.
extern "C" int chn_index_replicate(const chn_index *src, int32_t device, chn_index **out) {
    if (!src || !out) return fail(CHN_E_INVALID, "chn_index_replicate: null argument");
    *out = nullptr;
    int n_dev = 0;
    HIPCHK(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev)
        return fail(CHN_E_INVALID, "chn_index_replicate: device " + std::to_string(device) + " is not below the device count " + std::to_string(n_dev));
    chn_index *s = const_cast<chn_index *>(src);  // (only its queued work is waited for)
    HIPCHK(hipSetDevice(s->d.device));
    if (const int rc = index_wait_queued(s)) return rc;
    const size_t bytes = (size_t)(s->rows_local * s->d.bin_words * 8 + 64);
    HIPCHK(hipSetDevice(device));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if (bytes > free_b)
        return fail(CHN_E_NOMEM, "chn_index_replicate: device " + std::to_string(device) + " needs " + std::to_string(bytes) + " bytes for the index, " +
                                     std::to_string(free_b) + " bytes free");
    chn_index *idx = new (std::nothrow) chn_index();
    if (!idx) return fail(CHN_E_NOMEM, "host allocation failed");
    idx->d = s->d;
    idx->d.device = device;
    idx->rows_local = s->rows_local;
    idx->single_bin_categories = s->single_bin_categories;
    hipError_t e = hipMalloc((void **)&idx->words, bytes);
    if (e == hipSuccess) e = hipStreamCreate(&idx->ef_stream);
    if (e == hipSuccess) e = hipMemcpyPeerAsync(idx->words, device, s->words, s->d.device, bytes, idx->ef_stream);
    if (e != hipSuccess) {
        chn_index_destroy(idx);
        return fail(e == hipErrorOutOfMemory ? CHN_E_NOMEM : CHN_E_HIP, std::string("chn_index_replicate: ") + hipGetErrorString(e));
    }
    *out = idx;
    return CHN_OK;
}
extern "C" int chn_index_destroy(chn_index *idx) {
    if (!idx) return CHN_OK;
    (void)hipSetDevice(idx->d.device);
    idx->ef_release();
    if (idx->words) (void)hipFree(idx->words);
    delete idx;
    return CHN_OK;
}

// ---- model --------------------------------------------------------------------------------------
static std::vector<float> g_def_pos, g_def_neg;
static const float *g_def_pos_ptr[CHN_MAX_CATEGORIES], *g_def_neg_ptr[CHN_MAX_CATEGORIES];
static uint32_t g_def_n_pos[CHN_MAX_CATEGORIES], g_def_n_neg[CHN_MAX_CATEGORIES];
static std::once_flag g_def_once;

extern "C" int chn_model_default(chn_model *m, uint32_t num_categories, uint8_t host_index, int paired) {
    if (!m || num_categories < 1 || num_categories > CHN_MAX_CATEGORIES) return fail(CHN_E_INVALID, "chn_model_default: bad argument");
    // filled once, whatever host thread asks first (the tables are read-only afterwards)
    std::call_once(g_def_once, []() {
        for (double v : CHN_DEFAULT_POS) g_def_pos.push_back((float)v);
        for (double v : CHN_DEFAULT_NEG) g_def_neg.push_back((float)v);
        std::sort(g_def_pos.begin(), g_def_pos.end());  // KDEParams constructor sorts (include/classify_stats.hpp:214-218)
        std::sort(g_def_neg.begin(), g_def_neg.end());
        for (uint32_t c = 0; c < CHN_MAX_CATEGORIES; ++c) {
            g_def_pos_ptr[c] = g_def_pos.data(); g_def_neg_ptr[c] = g_def_neg.data();
            g_def_n_pos[c] = (uint32_t)g_def_pos.size(); g_def_n_neg[c] = (uint32_t)g_def_neg.size();
        }
    });
    std::memset(m, 0, sizeof(*m));
    m->struct_size = sizeof(chn_model);
    m->num_categories = num_categories;
    m->pos_data = g_def_pos_ptr; m->pos_n = g_def_n_pos; m->neg_data = g_def_neg_ptr; m->neg_n = g_def_n_neg;
    m->h_pos = 0.1f; m->h_neg = 0.001f; m->err_rate = 300.0f;
    m->min_quality = 15.0f; m->min_length = paired ? 80 : 140; m->min_compression = 0.0f;
    m->confidence_threshold = 7; m->min_hits = 0; m->paired = paired ? 1 : 0; m->host_index = host_index;
    m->confidence_probability_threshold = 0.0f; m->host_unique_prop_lo_threshold = 0.05f;
    m->min_proportion_difference = 0.04f; m->min_prob_difference = 0.0f;
    m->dist = CHN_DIST_KDE; m->pos_params = nullptr; m->neg_params = nullptr;
    return CHN_OK;
}

// stats::dgamma / stats::dbeta in float, as the reference calls them (include/classify_stats.hpp:377-381) [3P-recall]
static float host_dgamma(float x, float shape, float scale) {
    if (std::isnan(x) || std::isnan(shape) || std::isnan(scale) || shape < 0.0f || scale < 0.0f) return std::numeric_limits<float>::quiet_NaN();
    if (x < 0.0f) return 0.0f;
    if (x == 0.0f) return shape < 1.0f ? std::numeric_limits<float>::infinity() : (shape > 1.0f ? 0.0f : 1.0f / scale);
    if (std::isinf(x)) return 0.0f;
    return std::exp(-std::lgamma(shape) - shape * std::log(scale) + (shape - 1.0f) * std::log(x) - x / scale);
}
static float host_dbeta(float x, float a, float b) {
    const float inf = std::numeric_limits<float>::infinity();
    if (std::isnan(x) || std::isnan(a) || std::isnan(b) || a < 0.0f || b < 0.0f) return std::numeric_limits<float>::quiet_NaN();
    if (x < 0.0f || x > 1.0f) return 0.0f;
    if (a == 0.0f && b == 0.0f) return (x == 0.0f || x == 1.0f) ? inf : 0.0f;
    if (a == 0.0f || (std::isinf(b) && !std::isinf(a))) return x == 0.0f ? inf : 0.0f;
    if (b == 0.0f || (std::isinf(a) && !std::isinf(b))) return x == 1.0f ? inf : 0.0f;
    if (std::isinf(a) && std::isinf(b)) return x == 0.5f ? inf : 0.0f;
    if (x == 0.0f) return a < 1.0f ? inf : (a > 1.0f ? 0.0f : b);
    if (x == 1.0f) return b < 1.0f ? inf : (b > 1.0f ? 0.0f : a);
    return std::exp(-(std::lgamma(a) + std::lgamma(b) - std::lgamma(a + b)) + (a - 1.0f) * std::log(x) + (b - 1.0f) * std::log(1.0f - x));
}

// host restatement of the model + call used to re-evaluate reads the device flags as borderline
static float host_kde_prob(const std::vector<float> &data, float h, float x) {
    float total = 0.0f;
    for (float xi : data) {
        const float t = (x - xi) / h;
        total += (float)(std::exp(-std::pow((double)t, 2) / 2) / std::sqrt(2 * 3.141592653589793238463));
    }
    return total / (h * (float)data.size());
}
static void host_model_call(const HostModel &M, uint32_t nh, const uint32_t *cnts, const uint32_t *uq, float mq, float comp,
                            uint32_t length, double *prob, uint8_t *call_out, uint8_t *conf_out) {
    const uint32_t C = M.C;
    std::vector<float> props(C), uprops(C);
    for (uint32_t c = 0; c < C; ++c) {
        props[c] = (float)cnts[c] / (float)nh;
        uprops[c] = (float)uq[c] / (float)nh;
        const float x = uprops[c];
        float p_err;
        // statslib: NaN in -> quiet_NaN out (SURVEY App. A.6)
        if (std::isnan(x)) p_err = std::numeric_limits<float>::quiet_NaN(); else if (x < 0.0f) p_err = 0.0f; else p_err = std::exp(std::log(M.rate) - M.rate * x);
        float p_pos, p_neg;
        if (M.dist == CHN_DIST_GAMMA) {
            const float *q = M.dparams.data() + 6 * c;
            p_pos = host_dgamma(x - q[1], q[0], q[2]); p_neg = host_dgamma(x - q[4], q[3], q[5]);
        } else if (M.dist == CHN_DIST_BETA) {
            const float *q = M.dparams.data() + 6 * c;
            p_pos = host_dbeta(x, q[0], q[1]); p_neg = host_dbeta(x, q[3], q[4]);
        } else {
            p_pos = host_kde_prob(M.pos[c], M.h_pos, x);
            p_neg = host_kde_prob(M.neg[c], M.h_neg, x);
        }
        if (x == 1.0f) p_pos = 1.0f;
        const float total = p_err + p_pos + p_neg;
        prob[c] = (double)(p_pos / total);
    }
    uint8_t call = 255; uint32_t conf;
    if (!M.paired) {
        const uint32_t host = M.host_index, other = 1u - host;
        const double hu = uprops[host], ou = uprops[other], hp = prob[host], op = prob[other];
        uint32_t first = host, second = other;
        if (hu < ou) { first = other; second = host; }
        const uint32_t raw = uq[first] - uq[second];
        conf = raw > 255u ? 255u : raw;
        if (!((int)conf < (int)M.conf_thr) && !(mq < M.min_quality) && !(length < M.min_length) && !(comp < M.min_compression)) {
            const double dc = (double)conf;
            if (hu > ou && hu - ou > M.min_pd && hp > op && hp - op > M.min_prd && std::max(hp * dc, dc) >= M.cpt) call = (uint8_t)host;
            else if (hu < M.lo_thr && hu < ou && ou - hu > M.min_pd && hp < op && op - hp > M.min_prd && std::max(op * dc, dc) >= M.cpt) call = (uint8_t)other;
        }
    } else {
        uint32_t first = 0, second = 1;
        if (uq[second] > uq[first]) std::swap(first, second);
        for (uint32_t i = 2; i < C; ++i)
            if (uq[i] > uq[second]) { second = i; if (uq[second] > uq[first]) std::swap(first, second); }
        const uint32_t raw = uq[first] - uq[second];
        conf = raw > 255u ? 255u : raw;
        if (!(mq < M.min_quality) && !(length < M.min_length) && !(comp < M.min_compression)) {
            if (prob[second] == 0 && prob[first] > 0) call = (uint8_t)first;
            else if ((int)conf > (int)M.conf_thr && prob[first] > prob[second]) call = (uint8_t)first;
            if (cnts[second] > cnts[first] || cnts[first] - cnts[second] < M.min_hits) call = 255;
            if (props[second] > props[first] || props[first] - props[second] < M.min_pd) call = 255;
        }
    }
    *call_out = call; *conf_out = (uint8_t)conf;
}
