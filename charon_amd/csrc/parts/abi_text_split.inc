// abi_text_split.inc -- chn_text_split / chn_text_split_host, and split_download: the tail it shares with chn_fasta_split
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.
//
// chn_text_split queues text_split.inc's kernels on the stream's copy stream and waits twice: once for the three output words (how
// many records, where they end, how many id bytes -- the sizes of everything that follows), once for the descriptors and the ids,
// which come down in one batch of copies.  The scratch is the stream's (chn_stream::tsp, grow-only): a word per 4 KiB tile of the
// text, and line starts, descriptors and id positions by the record bound min(max_records, bytes / 8).

// The tail the two split calls share, behind their first wait (n records, ids_bytes of ids): refuse ids that do not fit, put the ids
// back to back (k_split_ids), download the descriptor columns -- the quality offsets where the job has them -- and the ids, and wait
// once.  The job's out fields are the caller's to fill.
template <class J>
static int split_download(chn_stream *s, TextSplitScratch &x, J *j, uint64_t n, uint64_t ids_bytes, const uint64_t *id_off, const uint64_t *seq_off, const uint64_t *qual_off,
                          uint64_t *qual_offset, const uint32_t *id_len, const uint32_t *seq_len, const char *who, int (*ids_too_small)(const J *, uint64_t, const char *, std::string &)) {
    std::string why;
    if (j->ids && ids_bytes > j->ids_capacity) return fail(ids_too_small(j, ids_bytes, who, why), why);
    if (!n) return CHN_OK;
    if (j->ids && ids_bytes) {
        const int rc = x.d_ids.ensure_grow((size_t)ids_bytes, (size_t)(ids_bytes / 4));
        if (rc) return rc;
        hipLaunchKernelGGL(k_split_ids, dim3(std::min<uint32_t>((uint32_t)((n + 15) / 16), std::max<uint32_t>(1, s->n_cus) * 8)), dim3(256), 0, s->q_copy, j->text, id_off, id_len,
                           x.d_idpos.as<uint32_t>(), (uint32_t)n, x.d_ids.as<uint8_t>());
        HIPCHK(hipGetLastError());
    }
    hipError_t e = hipMemcpyAsync(j->id_offset, id_off, n * 8, hipMemcpyDeviceToHost, s->q_copy);
    if (e == hipSuccess) e = hipMemcpyAsync(j->seq_offset, seq_off, n * 8, hipMemcpyDeviceToHost, s->q_copy);
    if (e == hipSuccess && qual_off) e = hipMemcpyAsync(qual_offset, qual_off, n * 8, hipMemcpyDeviceToHost, s->q_copy);
    if (e == hipSuccess) e = hipMemcpyAsync(j->id_length, id_len, n * 4, hipMemcpyDeviceToHost, s->q_copy);
    if (e == hipSuccess) e = hipMemcpyAsync(j->seq_length, seq_len, n * 4, hipMemcpyDeviceToHost, s->q_copy);
    if (e == hipSuccess && j->ids && ids_bytes) e = hipMemcpyAsync(j->ids, x.d_ids.p, ids_bytes, hipMemcpyDeviceToHost, s->q_copy);
    const hipError_t w = hipStreamSynchronize(s->q_copy);  // nothing stays queued into the caller's arrays, whatever happened
    if (e == hipSuccess) e = w;
    if (e != hipSuccess) return fail(CHN_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return CHN_OK;
}

extern "C" int chn_text_split_host(chn_text_split_job *job) {
    std::string why;
    const int rc = tsp_host_job(job, why);
    return rc ? fail(rc, why) : CHN_OK;
}

extern "C" int chn_text_split(chn_stream *s, chn_text_split_job *j) {
    const char *who = "chn_text_split";
    if (!s) return fail(CHN_E_INVALID, "chn_text_split: null stream");
    std::string why;
    int rc = tsp_check_job(j, who, why);
    if (rc) return fail(rc, why);
    int device = 0;
    if ((rc = stream_text_call(s, who, &device)) || (rc = device_text_check(j->text, j->text_bytes, device, who))) return rc;
    const uint64_t start = j->start, end = j->text_bytes, bound64 = tsp_record_bound(j);
    if (bound64 == 0) {  // nothing to look at, or no room for a record
        j->n_records = 0; j->consumed = start; j->ids_bytes = 0;
        return CHN_OK;
    }
    const uint32_t bound = (uint32_t)bound64;  // <= 2^28
    const uint64_t tile0 = start / TSP_TILE;
    const uint32_t n_tiles = (uint32_t)((end + TSP_TILE - 1) / TSP_TILE - tile0);  // >= 1, <= 2^19
    const uint32_t cap = 4 * bound;                                                   // <= 2^30 line starts behind the first
    TextSplitScratch &x = s->tsp;
    // descriptors in one block: id_off[bound] seq_off[bound] qual_off[bound] (64-bit), id_len[bound] seq_len[bound] (32-bit)
    if ((rc = x.d_tile.ensure((size_t)n_tiles * 8)) || (rc = x.d_line.ensure(((size_t)cap + 1) * 4)) || (rc = x.d_desc.ensure((size_t)bound * 32)) ||
        (rc = x.d_idpos.ensure((size_t)bound * 4)) || (rc = x.d_ctl.ensure(TSP_CTL_WORDS * 4)) || (rc = x.h_ctl.ensure(TSP_CTL_WORDS * 4)))
        return rc;
    uint32_t *tile_count = x.d_tile.as<uint32_t>(), *tile_off = tile_count + n_tiles, *ctl = x.d_ctl.as<uint32_t>(), *line_start = x.d_line.as<uint32_t>();
    TspRecArgs a;
    a.text = j->text; a.line_start = line_start; a.ctl = ctl; a.bound = bound;
    a.id_off = x.d_desc.as<uint64_t>(); a.seq_off = a.id_off + bound; a.qual_off = a.seq_off + bound;
    a.id_len = reinterpret_cast<uint32_t *>(a.qual_off + bound); a.seq_len = a.id_len + bound;
    const uint32_t cus = std::max<uint32_t>(1, s->n_cus);
    const uint32_t tile_blocks = std::min<uint32_t>((n_tiles + 3) / 4, cus * 8), rec_blocks = std::min<uint32_t>((bound + 255) / 256, cus * 8);
    const bool prof = (s->cfg.flags & CHN_STREAM_PROFILE) != 0;
    HIPCHK(x.timer.begin(prof, s->q_copy));
    HIPCHK(hipMemsetAsync(ctl, 0, TSP_CTL_WORDS * 4, s->q_copy));
    HIPCHK(hipMemsetAsync(ctl + TSP_FIRST_BAD, 0xFF, 4, s->q_copy));
    hipLaunchKernelGGL(k_split_count, dim3(tile_blocks), dim3(256), 0, s->q_copy, j->text, start, end, tile0, n_tiles, tile_count);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(SCAN_THREADS), 0, s->q_copy, tile_count, tile_off, (const uint32_t *)nullptr, n_tiles, ctl + TSP_LINES);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_lines, dim3(tile_blocks), dim3(256), 0, s->q_copy, j->text, start, end, tile0, n_tiles, tile_off, line_start, cap);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_records, dim3(rec_blocks), dim3(256), 0, s->q_copy, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_close, dim3(1), dim3(64), 0, s->q_copy, line_start, ctl, bound);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(SCAN_THREADS), 0, s->q_copy, a.id_len, x.d_idpos.as<uint32_t>(), ctl + TSP_N, bound, ctl + TSP_IDS_BYTES);
    HIPCHK(hipGetLastError());
    HIPCHK(x.timer.end(prof, s->q_copy));
    HIPCHK(hipMemcpyAsync(x.h_ctl.p, ctl, TSP_CTL_WORDS * 4, hipMemcpyDeviceToHost, s->q_copy));
    HIPCHK(hipStreamSynchronize(s->q_copy));
    HIPCHK(x.timer.collect(prof));
    const uint32_t *h = x.h_ctl.as<uint32_t>();
    const uint64_t n = h[TSP_N], ids_bytes = h[TSP_IDS_BYTES];
    if ((rc = split_download(s, x, j, n, ids_bytes, a.id_off, a.seq_off, a.qual_off, j->qual_offset, a.id_len, a.seq_len, who, tsp_ids_too_small))) return rc;
    j->n_records = n; j->consumed = h[TSP_CONSUMED]; j->ids_bytes = ids_bytes;
    return CHN_OK;
}
