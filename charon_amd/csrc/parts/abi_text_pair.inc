// abi_text_pair.inc -- chn_text_pair_ids / chn_text_pair_ids_host
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.
//
// chn_text_pair_ids checks the job, uploads the four descriptor columns in one copy (24 bytes per pair), runs k_pair_ids on the
// stream's copy stream and downloads its one word.  One wait.  The staging is the stream's (chn_stream::tpi, grow-only): 24 bytes per
// pair page-locked and on the device, and the word.

extern "C" int chn_text_pair_ids_host(chn_text_pair_job *job) {
    std::string why;
    const int rc = tpi_host_job(job, why);
    return rc ? fail(rc, why) : CHN_OK;
}

extern "C" int chn_text_pair_ids(chn_stream *s, chn_text_pair_job *j) {
    const char *who = "chn_text_pair_ids";
    if (!s) return fail(CHN_E_INVALID, "chn_text_pair_ids: null stream");
    std::string why;
    int rc = tpi_check_head(j, who, why);
    if (rc) return fail(rc, why);
    int device = 0;
    if ((rc = stream_text_call(s, who, &device)) || (rc = device_text_check(j->text1, j->text1_bytes, device, std::string(who) + ": text1")) ||
        (rc = device_text_check(j->text2, j->text2_bytes, device, std::string(who) + ": text2")))
        return rc;
    if ((rc = tpi_check_ranges(j, who, why))) return fail(rc, why);
    const uint64_t n = j->n_pairs;  // <= CHN_TEXT_PAIR_MAX_PAIRS: 24 n fits any size_t
    if (n == 0) {  // nothing to compare
        j->first_mismatch = 0;
        return CHN_OK;
    }
    TextPairScratch &x = s->tpi;
    const bool prof = (s->cfg.flags & CHN_STREAM_PROFILE) != 0;
    // descriptors in one block: off1[n] off2[n] (64-bit), len1[n] len2[n] (32-bit)
    if ((rc = x.h_desc.ensure((size_t)n * 24)) || (rc = x.d_desc.ensure((size_t)n * 24)) || (rc = x.d_first.ensure(16)) || (rc = x.h_first.ensure(16))) return rc;
    uint64_t *h_off1 = x.h_desc.as<uint64_t>(), *h_off2 = h_off1 + n;
    uint32_t *h_len1 = reinterpret_cast<uint32_t *>(h_off2 + n), *h_len2 = h_len1 + n;
    std::memcpy(h_off1, j->id1_offset, n * 8); std::memcpy(h_off2, j->id2_offset, n * 8);
    std::memcpy(h_len1, j->id1_length, n * 4); std::memcpy(h_len2, j->id2_length, n * 4);
    TpiArgs a;
    a.text1 = j->text1; a.text2 = j->text2;
    a.off1 = x.d_desc.as<uint64_t>(); a.off2 = a.off1 + n;
    a.len1 = reinterpret_cast<const uint32_t *>(a.off2 + n); a.len2 = a.len1 + n;
    a.n = n; a.first = x.d_first.as<unsigned long long>();
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)std::max<uint32_t>(1, s->n_cus) * 8);
    hipError_t e = hipMemcpyAsync(x.d_desc.p, x.h_desc.p, n * 24, hipMemcpyHostToDevice, s->q_copy);
    if (e == hipSuccess) e = hipMemsetAsync(x.d_first.p, 0xFF, 8, s->q_copy);
    if (e == hipSuccess) e = x.timer.begin(prof, s->q_copy);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_pair_ids, dim3(blocks), dim3(256), 0, s->q_copy, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = x.timer.end(prof, s->q_copy);
    if (e == hipSuccess) e = hipMemcpyAsync(x.h_first.p, x.d_first.p, 8, hipMemcpyDeviceToHost, s->q_copy);
    const hipError_t w = hipStreamSynchronize(s->q_copy);  // nothing stays queued, whatever happened
    if (e == hipSuccess) e = w;
    if (e != hipSuccess) return fail(CHN_E_HIP, std::string("chn_text_pair_ids: ") + hipGetErrorString(e));
    HIPCHK(x.timer.collect(prof));
    j->first_mismatch = std::min<uint64_t>(*x.h_first.as<uint64_t>(), n);
    return CHN_OK;
}
