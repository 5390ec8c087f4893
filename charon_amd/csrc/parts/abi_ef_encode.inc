// abi_ef_encode.inc -- chn_ef_layout_of, chn_index_ef_layout, chn_index_encode_ef, chn_index_encode_ef_host: the index writer's
// Elias-Fano arrays (ef_encode.inc) from the plain index, slice of rows by slice of rows
// Part of the single translation unit charon_hip.hip (included in order, behind abi_index_model.inc); not a stand-alone source.
// The layout call and the host form build for the CPU alone as well (tools/fuzz/ef_encode_fuzz.cpp).

static const uint64_t EF_MAX_M_SIZE = 1ULL << 57;       // ones * wl and the high bit numbers stay far below 2^64
static const uint64_t EF_MAX_SLICE_WORDS = 1ULL << 31;  // as chn_index_decode_ef: block numbers fit a grid

static int ef_layout_fill(uint64_t m_size, uint64_t ones, chn_ef_layout *out, const std::string &W) {
    if (!out) return fail(CHN_E_INVALID, W + ": null layout");
    if (m_size == 0 || m_size > EF_MAX_M_SIZE) return fail(CHN_E_INVALID, W + ": m_size must be in 1 .. 2^57");
    if (ones > m_size) return fail(CHN_E_INVALID, W + ": more ones than m_size has bits");
    const EfLayoutRule r = ef_layout_rule(m_size, ones);
    out->struct_size = sizeof(chn_ef_layout); out->wl = r.wl; out->m_size = m_size; out->ones = ones;
    out->low_bits = r.low_bits; out->high_bits = r.high_bits; out->n_low_words = r.n_low_words; out->n_high_words = r.n_high_words;
    return CHN_OK;
}
extern "C" int chn_ef_layout_of(uint64_t m_size, uint64_t ones, chn_ef_layout *out) { return ef_layout_fill(m_size, ones, out, "chn_ef_layout_of"); }

static bool ef_whole_index(const chn_index_desc &d) { return d.row_begin == 0 && (d.row_end == 0 || d.row_end == d.bin_size); }

// What both forms of the encode ask of the descriptor and the job before anything runs or is written; *slice_rows is the rows per slice.
static int ef_encode_check(const chn_index_desc &d, const chn_ef_encode_job *j, uint64_t *slice_rows, const std::string &W) {
    if (!j) return fail(CHN_E_INVALID, W + ": null job");
    if (j->struct_size != sizeof(chn_ef_encode_job)) return fail(CHN_E_INVALID, W + ": bad struct_size");
    if (j->flags) return fail(CHN_E_INVALID, W + ": unknown flag");
    if (d.bin_words == 0 || d.technical_bins != 64 * d.bin_words || d.bin_size == 0 || d.bin_size > EF_MAX_M_SIZE / d.technical_bins)
        return fail(CHN_E_INVALID, W + ": bad index descriptor");
    if (!ef_whole_index(d)) return fail(CHN_E_INVALID, W + ": the index is a row shard: the Elias-Fano arrays are those of the whole index");
    const chn_ef_layout *l = j->layout;
    if (!l) return fail(CHN_E_INVALID, W + ": null layout");
    if (l->struct_size != sizeof(chn_ef_layout)) return fail(CHN_E_INVALID, W + ": bad struct_size of the layout");
    if (l->m_size != d.technical_bins * d.bin_size) return fail(CHN_E_INVALID, W + ": the layout's m_size != technical_bins * bin_size");
    chn_ef_layout want;
    if (const int rc = ef_layout_fill(l->m_size, l->ones, &want, W)) return rc;
    if (l->wl != want.wl || l->low_bits != want.low_bits || l->high_bits != want.high_bits || l->n_low_words != want.n_low_words || l->n_high_words != want.n_high_words)
        return fail(CHN_E_INVALID, W + ": the layout is not the one of its m_size and ones");
    if (j->n_low_words != l->n_low_words || j->n_high_words != l->n_high_words) return fail(CHN_E_INVALID, W + ": the arrays' sizes are not the layout's");
    if ((j->n_low_words && !j->low) || !j->high) return fail(CHN_E_INVALID, W + ": null array");
    uint64_t rows = j->slice_rows ? j->slice_rows : std::max<uint64_t>(1, (256ULL << 20) / (8 * d.bin_words));
    rows = std::min(rows, d.bin_size);
    if (rows > EF_MAX_SLICE_WORDS / d.bin_words) return fail(CHN_E_INVALID, W + ": slice too large (at most 2^31 words)");
    *slice_rows = rows;
    return CHN_OK;
}

// a slice's ranges, encoded at `low` / `high`, into the arrays of the whole index: neighbouring slices share the words at their seams
static void ef_merge_slice(const chn_ef_encode_job *j, const EfRange &r, const uint64_t *low, const uint64_t *high) {
    for (uint64_t i = 0; i < r.n_low; ++i) j->low[r.low_w0 + i] |= low[i];
    for (uint64_t i = 0; i < r.n_high; ++i) j->high[r.high_w0 + i] |= high[i];
}
static void ef_clear_arrays(const chn_ef_encode_job *j) {
    if (j->n_low_words) std::memset(j->low, 0, j->n_low_words * 8);
    std::memset(j->high, 0, j->n_high_words * 8);
}
static int ef_encode_close(chn_ef_encode_job *j, uint64_t written, uint64_t bad, double ms, const std::string &W) {
    j->ones_written = written; j->device_ms = ms;
    if (bad) return fail(CHN_E_INVALID, W + ": internal error: " + std::to_string(bad) + " words fell outside their slice's ranges");
    if (written != j->layout->ones) return fail(CHN_E_INVALID, W + ": " + std::to_string(written) + " set bits were written, the layout counts " + std::to_string(j->layout->ones));
    return CHN_OK;
}

extern "C" int chn_index_encode_ef_host(const chn_index_desc *desc, const uint64_t *host_words, chn_ef_encode_job *j) {
    const std::string W = "chn_index_encode_ef_host";
    if (!desc || desc->struct_size != sizeof(chn_index_desc)) return fail(CHN_E_INVALID, W + ": bad descriptor");
    if (!host_words) return fail(CHN_E_INVALID, W + ": null words");
    const chn_index_desc &d = *desc;
    uint64_t slice_rows = 0;
    if (const int rc = ef_encode_check(d, j, &slice_rows, W)) return rc;
    const uint64_t Wd = d.bin_words, S = d.bin_size;
    uint64_t total = 0;
    for (uint64_t i = 0; i < S * Wd; ++i) total += (uint64_t)__builtin_popcountll(host_words[i]);
    if (total != j->layout->ones) return fail(CHN_E_INVALID, W + ": the words hold " + std::to_string(total) + " set bits, the layout counts " + std::to_string(j->layout->ones));
    ef_clear_arrays(j);
    const uint32_t wl = j->layout->wl;
    uint64_t before = 0, bad = 0;
    std::vector<uint64_t> low, high;
    for (uint64_t r0 = 0; r0 < S; r0 += slice_rows) {
        const uint64_t nr = std::min(slice_rows, S - r0), n = nr * Wd;
        const uint64_t *words = host_words + r0 * Wd;
        uint64_t c = 0;
        for (uint64_t i = 0; i < n; ++i) c += (uint64_t)__builtin_popcountll(words[i]);
        if (!c) continue;
        const EfRange r = ef_slice_range(wl, r0 * Wd * 64, (r0 + nr) * Wd * 64, before, c);
        low.assign(r.n_low, 0); high.assign(r.n_high, 0);
        EfOut o;
        o.low = low.data(); o.high = high.data(); o.low_w0 = r.low_w0; o.n_low = r.n_low; o.high_w0 = r.high_w0; o.n_high = r.n_high;
        uint64_t k = before;
        for (uint64_t i = 0; i < n; ++i) {
            if (!words[i]) continue;
            bad += ef_encode_word(words[i], (r0 * Wd + i) * 64, k, wl, o, EfOrPlain());
            k += (uint64_t)__builtin_popcountll(words[i]);
        }
        ef_merge_slice(j, r, low.data(), high.data());
        before += c;
    }
    return ef_encode_close(j, before, bad, 0.0, W);
}

#ifdef __HIPCC__
// set bits of the whole index, counted on the device (k_bin_popcounts, summed over the technical bins)
static int ef_index_ones(chn_index *idx, uint64_t *ones) {
    std::vector<uint64_t> per_bin(idx->d.technical_bins, 0);
    if (const int rc = chn_index_bin_popcounts(idx, per_bin.data())) return rc;  // (waits for queued slices and a queued replica copy)
    *ones = 0;
    for (uint64_t c : per_bin) *ones += c;
    return CHN_OK;
}

extern "C" int chn_index_ef_layout(chn_index *idx, chn_ef_layout *out) {
    const std::string W = "chn_index_ef_layout";
    if (!idx || !out) return fail(CHN_E_INVALID, W + ": null argument");
    if (!ef_whole_index(idx->d)) return fail(CHN_E_INVALID, W + ": the index is a row shard: the Elias-Fano arrays are those of the whole index");
    uint64_t ones = 0;
    if (const int rc = ef_index_ones(idx, &ones)) return rc;
    return ef_layout_fill(idx->d.technical_bins * idx->d.bin_size, ones, out, W);
}

// The call's device scratch, page-locked staging and events: sized by the largest slice, released when the call returns.
struct EfEncodeScratch {
    DevBuf counts, prefix, out, bad;  // out: the slice's words of m_low, behind them its words of m_high (one clear, one download)
    PinBuf h_out;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~EfEncodeScratch() {
        counts.release(); prefix.release(); out.release(); bad.release(); h_out.release();
        events_destroy({&ev[0], &ev[1], &ev[2], &ev[3]});
    }
};

static int ef_encode_device(chn_index *idx, chn_ef_encode_job *j, uint64_t slice_rows, EfEncodeScratch &sc, const std::string &W) {
    const chn_index_desc &d = idx->d;
    const uint64_t Wd = d.bin_words, S = d.bin_size;
    const uint32_t wl = j->layout->wl;
    if (const int rc = events_create(W.c_str(), {}, {&sc.ev[0], &sc.ev[1], &sc.ev[2], &sc.ev[3]})) return rc;
    if (const int rc = sc.bad.ensure(8)) return rc;
    HIPCHK(hipMemsetAsync(sc.bad.p, 0, 8, 0));
    uint64_t before = 0;
    double ms = 0;
    for (uint64_t r0 = 0; r0 < S; r0 += slice_rows) {
        const uint64_t nr = std::min(slice_rows, S - r0), n = nr * Wd, n_blocks = (n + 255) / 256;
        const uint64_t *words = idx->words + r0 * Wd;
        int rc;
        if ((rc = sc.counts.ensure((n_blocks + 1) * 4)) || (rc = sc.prefix.ensure((n_blocks + 1) * 8))) return rc;
        // one more count, zero: the exclusive prefix of it is the slice's set bits
        HIPCHK(hipMemsetAsync(sc.counts.as<uint32_t>() + n_blocks, 0, 4, 0));
        HIPCHK(hipEventRecord(sc.ev[0], 0));
        hipLaunchKernelGGL(k_ef_block_counts, dim3((uint32_t)n_blocks), dim3(256), 0, 0, words, n, sc.counts.as<uint32_t>());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_ef_block_prefix, dim3(1), dim3(SCAN_THREADS), 0, 0, sc.counts.as<uint32_t>(), n_blocks + 1, sc.prefix.as<uint64_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(sc.ev[1], 0));
        uint64_t c = 0;
        HIPCHK(hipMemcpy(&c, sc.prefix.as<uint64_t>() + n_blocks, 8, hipMemcpyDeviceToHost));
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, sc.ev[0], sc.ev[1]));
        ms += t;
        if (!c) continue;
        if (c > j->layout->ones - before) return fail(CHN_E_INVALID, W + ": the index changed during the call");  // (the ranges below rest on the count)
        const EfRange r = ef_slice_range(wl, r0 * Wd * 64, (r0 + nr) * Wd * 64, before, c);
        if (r.low_w0 + r.n_low > j->n_low_words || r.high_w0 + r.n_high > j->n_high_words) return fail(CHN_E_INVALID, W + ": internal error: a slice's range leaves the arrays");
        const size_t out_bytes = (size_t)(r.n_low + r.n_high) * 8;
        if ((rc = sc.out.ensure_grow(out_bytes, out_bytes / 8)) || (rc = sc.h_out.ensure_grow(out_bytes, out_bytes / 8))) return rc;
        HIPCHK(hipMemsetAsync(sc.out.p, 0, out_bytes, 0));
        EfEncArgs a;
        a.words = words; a.n_words = n; a.pos0 = r0 * Wd * 64; a.ones_before = before; a.bad = sc.bad.as<unsigned long long>(); a.wl = wl;
        a.out.low = sc.out.as<uint64_t>(); a.out.high = sc.out.as<uint64_t>() + r.n_low;
        a.out.low_w0 = r.low_w0; a.out.n_low = r.n_low; a.out.high_w0 = r.high_w0; a.out.n_high = r.n_high;
        HIPCHK(hipEventRecord(sc.ev[2], 0));
        hipLaunchKernelGGL(k_ef_encode, dim3((uint32_t)n_blocks), dim3(256), 0, 0, a, sc.prefix.as<uint64_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(sc.ev[3], 0));
        HIPCHK(hipMemcpy(sc.h_out.p, sc.out.p, out_bytes, hipMemcpyDeviceToHost));
        HIPCHK(hipEventElapsedTime(&t, sc.ev[2], sc.ev[3]));
        ms += t;
        ef_merge_slice(j, r, sc.h_out.as<uint64_t>(), sc.h_out.as<uint64_t>() + r.n_low);
        before += c;
    }
    unsigned long long bad = 0;
    HIPCHK(hipMemcpy(&bad, sc.bad.p, 8, hipMemcpyDeviceToHost));
    return ef_encode_close(j, before, bad, ms, W);
}

extern "C" int chn_index_encode_ef(chn_index *idx, chn_ef_encode_job *j) {
    const std::string W = "chn_index_encode_ef";
    if (!idx) return fail(CHN_E_INVALID, W + ": null index");
    uint64_t slice_rows = 0;
    if (const int rc = ef_encode_check(idx->d, j, &slice_rows, W)) return rc;
    HIPCHK(hipSetDevice(idx->d.device));
    uint64_t total = 0;
    if (const int rc = ef_index_ones(idx, &total)) return rc;
    if (total != j->layout->ones) return fail(CHN_E_INVALID, W + ": the index holds " + std::to_string(total) + " set bits, the layout counts " + std::to_string(j->layout->ones));
    ef_clear_arrays(j);
    EfEncodeScratch sc;
    return ef_encode_device(idx, j, slice_rows, sc, W);
}
#endif
