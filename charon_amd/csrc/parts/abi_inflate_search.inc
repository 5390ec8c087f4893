// abi_inflate_search.inc -- chn_inflate_stream_search_host: block starts of one deflate stream (inflate_search.inc), on one CPU thread
// Part of the single translation unit charon_hip.hip (included in order, behind abi_inflate_stream.inc); not a stand-alone source.
// Builds for the CPU alone as well (tools/fuzz/inflate_search_fuzz.cpp).  The device form of the call is not built (DESIGN 7l).

static int inflate_search_check(const chn_inflate_search_job *j, const char *who) {
    const std::string W(who);
    if (!j) return fail(CHN_E_INVALID, W + ": null job");
    if (j->struct_size != sizeof(chn_inflate_search_job)) return fail(CHN_E_INVALID, W + ": bad struct_size");
    if (j->flags) return fail(CHN_E_INVALID, W + ": unknown flag");
    const uint64_t n = j->n_ranges;
    if (n > CHN_INFLATE_STREAM_MAX_CHUNKS) return fail(CHN_E_INVALID, W + ": n_ranges is above CHN_INFLATE_STREAM_MAX_CHUNKS");
    if (n == 0) return CHN_OK;
    if (!j->from_bit || !j->to_bit || !j->found_bit) return fail(CHN_E_INVALID, W + ": a range array is NULL");
    if (!j->in && j->in_bytes) return fail(CHN_E_INVALID, W + ": in is NULL");
    if (j->in_bytes > (~0ull >> 3)) return fail(CHN_E_INVALID, W + ": in_bytes is above 2^61");
    for (uint64_t i = 0; i < n; ++i) {
        const std::string M = W + ": range " + std::to_string(i);
        if (j->from_bit[i] > j->to_bit[i]) return fail(CHN_E_INVALID, M + " has its end in front of its begin");
        if (j->to_bit[i] > j->in_bytes * 8) return fail(CHN_E_INVALID, M + " ends beyond the end of in");
    }
    return CHN_OK;
}

extern "C" int chn_inflate_stream_search_host(const chn_inflate_search_job *j) {
    const char *who = "chn_inflate_stream_search_host";
    int rc = inflate_search_check(j, who);
    if (rc || j->n_ranges == 0) return rc;
    InfShared *sh = new (std::nothrow) InfShared;
    if (!sh) return fail(CHN_E_NOMEM, std::string(who) + ": no memory for the decoder's tables");
    for (uint64_t i = 0; i < j->n_ranges; ++i) j->found_bit[i] = infs_search_host(*sh, j->in, j->in_bytes, j->from_bit[i], j->to_bit[i]);
    delete sh;
    return CHN_OK;
}
