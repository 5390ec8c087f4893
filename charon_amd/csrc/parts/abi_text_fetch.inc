// abi_text_fetch.inc -- chn_text_fetch / chn_text_fetch_host, and chn_device_copy
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.
//
// chn_text_fetch checks the job, computes the destination offsets (the exclusive scan of the lengths), uploads the descriptors in one
// copy, runs k_text_gather on the stream's copy stream into a device buffer and downloads the gathered bytes: straight into `out` where
// that is page-locked, else into page-locked staging from which they are copied out.  One wait.  The staging is the stream's
// (chn_stream::txg, grow-only): 20 bytes per range and the gathered bytes, on the device and page-locked.

extern "C" int chn_text_fetch_host(chn_text_fetch_job *job) {
    std::string why;
    const int rc = txg_host_job(job, why);
    return rc ? fail(rc, why) : CHN_OK;
}

extern "C" int chn_text_fetch(chn_stream *s, chn_text_fetch_job *j) {
    const char *who = "chn_text_fetch";
    if (!s) return fail(CHN_E_INVALID, "chn_text_fetch: null stream");
    std::string why;
    uint64_t total = 0;
    int rc = txg_check_job(j, who, why, total);
    if (rc) return fail(rc, why);
    int device = 0;
    if ((rc = stream_text_call(s, who, &device)) || (rc = device_text_check(j->text, j->text_bytes, device, who))) return rc;
    TextFetchScratch &x = s->txg;
    const bool prof = (s->cfg.flags & CHN_STREAM_PROFILE) != 0;
    if (total == 0) {  // nothing to move
        if (prof) x.timer.count_only();
        j->out_bytes = 0;
        return CHN_OK;
    }
    const uint64_t n = j->n_ranges;
    const bool direct = page_locked_host(j->out, total);
    // descriptors in one block: src_off[n] dst_off[n] (64-bit), len[n] (32-bit)
    if ((rc = x.h_desc.ensure((size_t)n * 20)) || (rc = x.d_desc.ensure((size_t)n * 20)) || (rc = x.d_out.ensure((size_t)((total + 15) & ~(uint64_t)15))) ||
        (!direct && (rc = x.h_out.ensure((size_t)total))))
        return rc;
    uint64_t *h_src = x.h_desc.as<uint64_t>(), *h_dst = h_src + n;
    uint32_t *h_len = reinterpret_cast<uint32_t *>(h_dst + n);
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; ++i) { h_src[i] = j->offset[i]; h_dst[i] = at; h_len[i] = j->length[i]; at += j->length[i]; }
    const uint64_t *d_src = x.d_desc.as<uint64_t>(), *d_dst = d_src + n;
    const uint32_t *d_len = reinterpret_cast<const uint32_t *>(d_dst + n);
    uint8_t *host_dst = direct ? j->out : x.h_out.as<uint8_t>();
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(n, (uint64_t)std::max<uint32_t>(1, s->n_cus) * 16);
    hipError_t e = hipMemcpyAsync(x.d_desc.p, x.h_desc.p, n * 20, hipMemcpyHostToDevice, s->q_copy);
    if (e == hipSuccess) e = x.timer.begin(prof, s->q_copy);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_text_gather, dim3(blocks), dim3(WAVE), 0, s->q_copy, j->text, d_src, d_dst, d_len, n, x.d_out.as<uint8_t>());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = x.timer.end(prof, s->q_copy);
    if (e == hipSuccess) e = hipMemcpyAsync(host_dst, x.d_out.p, total, hipMemcpyDeviceToHost, s->q_copy);
    const hipError_t w = hipStreamSynchronize(s->q_copy);  // nothing stays queued into the caller's memory, whatever happened
    if (e == hipSuccess) e = w;
    if (e != hipSuccess) return fail(CHN_E_HIP, std::string("chn_text_fetch: ") + hipGetErrorString(e));
    HIPCHK(x.timer.collect(prof));
    if (!direct) std::memcpy(j->out, x.h_out.p, total);
    j->out_bytes = total;
    return CHN_OK;
}

extern "C" int chn_device_copy(int device, void *dev_dst, const void *dev_src, uint64_t bytes) {
    if (!bytes) return CHN_OK;
    if (!dev_dst || !dev_src) return fail(CHN_E_INVALID, "chn_device_copy: null argument");
    HIPCHK(hipSetDevice(device));
    std::string why;
    if (!device_memory_of(dev_src, bytes, device, why)) return fail(CHN_E_INVALID, "chn_device_copy: the source " + why);
    if (!device_memory_of(dev_dst, bytes, device, why)) return fail(CHN_E_INVALID, "chn_device_copy: the destination " + why);
    const char *a = static_cast<const char *>(dev_src), *b = static_cast<const char *>(dev_dst);
    if (a < b + bytes && b < a + bytes) return fail(CHN_E_INVALID, "chn_device_copy: source and destination overlap");
    HIPCHK(hipMemcpy(dev_dst, dev_src, bytes, hipMemcpyDeviceToDevice));
    HIPCHK(hipStreamSynchronize(nullptr));  // a device-to-device hipMemcpy may return early: in place for work on any stream when the call returns
    return CHN_OK;
}
