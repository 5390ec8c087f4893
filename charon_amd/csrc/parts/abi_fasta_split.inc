// abi_fasta_split.inc -- chn_fasta_split / chn_fasta_split_host
// Part of the single translation unit charon_hip.hip (included in order, behind abi_text_split.inc); not a stand-alone source.
//
// chn_fasta_split queues fasta_split.inc's kernels on the stream's copy stream and waits twice, as chn_text_split does: once for the
// four output words (how many records, where they end, how many id bytes, how many letters), once for the descriptors and the ids.
// The letters are in the caller's seq_text by the first wait.  The scratch is the stream's (chn_stream::fsp, grow-only): 52 bytes per
// 4 KiB tile of the text (the tile summaries, the resolved counts and their scans), and header positions, descriptors and id positions
// by the record bound min(max_records, bytes / 3).

extern "C" int chn_fasta_split_host(chn_fasta_split_job *job) {
    std::string why;
    const int rc = fsp_host_job(job, why);
    return rc ? fail(rc, why) : CHN_OK;
}

extern "C" int chn_fasta_split(chn_stream *s, chn_fasta_split_job *j) {
    const char *who = "chn_fasta_split";
    if (!s) return fail(CHN_E_INVALID, "chn_fasta_split: null stream");
    std::string why;
    int rc = fsp_check_job(j, who, why);
    if (rc) return fail(rc, why);
    int device = 0;
    if ((rc = stream_text_call(s, who, &device)) || (rc = device_text_check(j->text, j->text_bytes, device, who))) return rc;
    if (j->seq_capacity) {
        if ((reinterpret_cast<uintptr_t>(j->seq_text) & 15) || (j->seq_capacity & 15)) return fail(CHN_E_INVALID, "chn_fasta_split: seq_text must be 16-byte aligned and seq_capacity a multiple of 16");
        if (!device_memory_of(j->seq_text, j->seq_capacity, device, why)) return fail(CHN_E_INVALID, "chn_fasta_split: seq_text " + why);
    }
    const uint64_t start = j->start, end = j->text_bytes, bound64 = fsp_record_bound(j);
    if (bound64 == 0) {  // nothing to look at, or no room for a record
        j->n_records = 0; j->consumed = start; j->ids_bytes = 0; j->seq_bytes = 0;
        return CHN_OK;
    }
    const uint32_t bound = (uint32_t)bound64;  // < 2^30
    const uint32_t cap = bound + 1;            // header ranks kept: the candidates and the header behind the last of them
    const uint64_t tile0 = start / TSP_TILE;
    const uint32_t n_tiles = (uint32_t)((end + TSP_TILE - 1) / TSP_TILE - tile0);  // >= 1, <= 2^19
    TextSplitScratch &x = s->fsp;
    // per tile: the summary (FspTile), then seven words: state, headers, header feeds, kept bytes, and the exclusive sums of the last three
    // per record of the bound: hdr_pos, feed_pos, kept_before [cap]; id_off seq_off (64-bit), id_len seq_len (32-bit)
    if ((rc = x.d_tile.ensure((size_t)n_tiles * (sizeof(FspTile) + 28))) || (rc = x.d_line.ensure((size_t)cap * 12)) || (rc = x.d_desc.ensure((size_t)bound * 24)) ||
        (rc = x.d_idpos.ensure((size_t)bound * 4)) || (rc = x.d_ctl.ensure(FSP_CTL_WORDS * 4)) || (rc = x.h_ctl.ensure(FSP_CTL_WORDS * 4)))
        return rc;
    FspTile *tiles = x.d_tile.as<FspTile>();
    uint32_t *tile_state = reinterpret_cast<uint32_t *>(tiles + n_tiles), *tile_hdr = tile_state + n_tiles, *tile_feed = tile_hdr + n_tiles, *tile_kept = tile_feed + n_tiles;
    uint32_t *hdr_off = tile_kept + n_tiles, *feed_off = hdr_off + n_tiles, *kept_off = feed_off + n_tiles;
    uint32_t *ctl = x.d_ctl.as<uint32_t>();
    uint32_t *hdr_pos = x.d_line.as<uint32_t>(), *feed_pos = hdr_pos + cap, *kept_before = feed_pos + cap;
    FspRecArgs a;
    a.hdr_pos = hdr_pos; a.feed_pos = feed_pos; a.kept_before = kept_before; a.ctl = ctl;
    a.start = (uint32_t)start; a.bound = bound; a.eoi = (j->flags & CHN_FASTA_SPLIT_END_OF_INPUT) ? 1u : 0u;
    a.id_off = x.d_desc.as<uint64_t>(); a.seq_off = a.id_off + bound;
    a.id_len = reinterpret_cast<uint32_t *>(a.seq_off + bound); a.seq_len = a.id_len + bound;
    const uint32_t cus = std::max<uint32_t>(1, s->n_cus);
    const uint32_t tile_blocks = std::min<uint32_t>((n_tiles + 3) / 4, cus * 8), rec_blocks = std::min<uint32_t>((bound + 255) / 256, cus * 8);
    const bool prof = (s->cfg.flags & CHN_STREAM_PROFILE) != 0;
    HIPCHK(x.timer.begin(prof, s->q_copy));
    HIPCHK(hipMemsetAsync(ctl, 0, FSP_CTL_WORDS * 4, s->q_copy));
    HIPCHK(hipMemsetAsync(ctl + FSP_FIRST_BAD, 0xFF, 4, s->q_copy));
    hipLaunchKernelGGL(k_fasta_tiles, dim3(tile_blocks), dim3(256), 0, s->q_copy, j->text, start, end, tile0, n_tiles, tiles);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_fasta_resolve, dim3(1), dim3(256), 0, s->q_copy, tiles, n_tiles, tile_state, tile_hdr, tile_feed, tile_kept);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(SCAN_THREADS), 0, s->q_copy, tile_hdr, hdr_off, (const uint32_t *)nullptr, n_tiles, ctl + FSP_HDRS);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(SCAN_THREADS), 0, s->q_copy, tile_feed, feed_off, (const uint32_t *)nullptr, n_tiles, ctl + FSP_FEEDS);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(SCAN_THREADS), 0, s->q_copy, tile_kept, kept_off, (const uint32_t *)nullptr, n_tiles, ctl + FSP_KEPT);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_fasta_headers, dim3(tile_blocks), dim3(256), 0, s->q_copy, j->text, start, end, tile0, n_tiles, tile_state, hdr_off, feed_off, kept_off, ctl, hdr_pos,
                       feed_pos, kept_before, cap);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_fasta_records, dim3(rec_blocks), dim3(256), 0, s->q_copy, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_fasta_close, dim3(1), dim3(64), 0, s->q_copy, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_fasta_compact, dim3(tile_blocks), dim3(256), 0, s->q_copy, j->text, start, end, tile0, n_tiles, tile_state, kept_off, ctl, j->seq_text);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(SCAN_THREADS), 0, s->q_copy, a.id_len, x.d_idpos.as<uint32_t>(), ctl + FSP_N, bound, ctl + FSP_IDS_BYTES);
    HIPCHK(hipGetLastError());
    HIPCHK(x.timer.end(prof, s->q_copy));
    HIPCHK(hipMemcpyAsync(x.h_ctl.p, ctl, FSP_CTL_WORDS * 4, hipMemcpyDeviceToHost, s->q_copy));
    HIPCHK(hipStreamSynchronize(s->q_copy));
    HIPCHK(x.timer.collect(prof));
    const uint32_t *h = x.h_ctl.as<uint32_t>();
    const uint64_t n = h[FSP_N], ids_bytes = h[FSP_IDS_BYTES];
    if ((rc = split_download(s, x, j, n, ids_bytes, a.id_off, a.seq_off, nullptr, nullptr, a.id_len, a.seq_len, who, fsp_ids_too_small))) return rc;
    j->n_records = n; j->consumed = h[FSP_CONSUMED]; j->ids_bytes = ids_bytes; j->seq_bytes = h[FSP_SEQ_BYTES];
    return CHN_OK;
}
