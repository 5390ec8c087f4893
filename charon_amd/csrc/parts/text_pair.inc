// text_pair.inc -- do the ids of the two mates of every pair agree?  k_pair_ids over two texts that lie in device memory
// (chn_text_pair_ids), and the same rule on the CPU (chn_text_pair_ids_host)
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.
//
// THE RULE is the front end's for paired input (host/dehost.inc, the reference's src/dehost_main.cpp:423-430): both ids lose their last
// byte -- the mate number of "name/1" and "name/2" -- and what is left must be equal:
//   la = id1_length ? id1_length - 1 : 0, lb likewise; the pair agrees if and only if la == lb and the first la bytes are equal.
// The dropped byte never counts; two empty ids agree, and so do an empty id and a one-byte id.  tpi_agree is that rule, written once
// as __host__ __device__ code over a text policy that hands out the 16 bytes at an offset as four little-endian dwords: on the
// device text_fetch16 (text_pack.inc: only aligned dwords that hold a wanted byte), on the CPU a byte loop over text of any alignment.
// Bytes of a piece behind `count` are unspecified in either policy and masked off by the rule.
//
// The device maps ONE LANE TO ONE PAIR.  An id is 20 - 70 bytes, two to five pieces, so a lane's loop is short and ends at the first
// piece that differs; several lanes per pair would add a cross-lane reduction and a broadcast of the descriptors to save at most
// four steps of a loop that waits on memory either way, and neighbouring pairs lie a whole record apart in the text, so neither
// mapping coalesces.  A long id simply loops (64-bit position: any uint32_t length).  The first disagreeing pair of the launch is the
// minimum over the wavefronts of their lowest disagreeing lane: one ballot and at most one atomicMin per wavefront and round, the
// pattern of k_split_records.  A looping grid; plain stores only, no LDS.

#ifndef __HIPCC__  // a CPU build of the checks and the host walk alone (tools/fuzz/text_pair_fuzz.cpp)
#ifndef __host__
#define __host__
#define __device__
#endif
#endif

// host text of any alignment: the `count` bytes at text + addr, nothing else is touched
struct TpiHostText {
    const uint8_t *text;
    __host__ __device__ void fetch16(uint64_t addr, uint32_t count, uint32_t w[4]) const {
        for (uint32_t k = 0; k < 4; ++k) w[k] = 0;
        for (uint32_t j = 0; j < count; ++j) w[j >> 2] |= (uint32_t)text[addr + j] << (8 * (j & 3));
    }
};

// the rule (above) for one pair: id a at ta[oa .. + ida), id b at tb[ob .. + idb)
template <class TextA, class TextB>
__host__ __device__ static inline bool tpi_agree(const TextA &ta, uint64_t oa, uint32_t ida, const TextB &tb, uint64_t ob, uint32_t idb) {
    const uint32_t la = ida ? ida - 1 : 0, lb = idb ? idb - 1 : 0;
    if (la != lb) return false;
    for (uint64_t p = 0; p < la; p += 16) {
        const uint32_t count = la - p < 16 ? (uint32_t)(la - p) : 16u;
        uint32_t x[4], y[4];
        ta.fetch16(oa + p, count, x);
        tb.fetch16(ob + p, count, y);
        uint32_t diff = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t nb = count > 4 * k ? (count - 4 * k < 4 ? count - 4 * k : 4u) : 0u;  // wanted bytes of dword k
            const uint32_t mask = nb == 4 ? ~0u : (1u << (8 * nb)) - 1u;
            diff |= (x[k] ^ y[k]) & mask;
        }
        if (diff) return false;
    }
    return true;
}

// The checks both calls make on a job before anything else, in two steps -- the job's own fields, which cost nothing, then every id
// range (chn_text_pair_ids looks at the stream and at the two pointers in between); `why` names the first that fails.  0 or a
// CHN_E_* code.
static int tpi_check_head(const chn_text_pair_job *j, const char *who, std::string &why) {
    const std::string W(who);
    if (!j) { why = W + ": null job"; return CHN_E_INVALID; }
    if (j->struct_size != sizeof(chn_text_pair_job)) { why = W + ": bad struct_size"; return CHN_E_INVALID; }
    if (j->flags) { why = W + ": unknown flag"; return CHN_E_INVALID; }
    if (j->n_pairs > CHN_TEXT_PAIR_MAX_PAIRS) {  // (before any array is walked or any size is formed from n_pairs)
        why = W + ": n_pairs " + std::to_string(j->n_pairs) + " is above CHN_TEXT_PAIR_MAX_PAIRS " + std::to_string(CHN_TEXT_PAIR_MAX_PAIRS);
        return CHN_E_INVALID;
    }
    if (j->n_pairs && (!j->id1_offset || !j->id1_length || !j->id2_offset || !j->id2_length)) { why = W + ": an id array is NULL"; return CHN_E_INVALID; }
    if (!j->text1 && j->text1_bytes) { why = W + ": text1 is NULL"; return CHN_E_INVALID; }
    if (!j->text2 && j->text2_bytes) { why = W + ": text2 is NULL"; return CHN_E_INVALID; }
    return CHN_OK;
}
static int tpi_check_ranges(const chn_text_pair_job *j, const char *who, std::string &why) {
    const std::string W(who);
    for (uint64_t i = 0; i < j->n_pairs; ++i)
        for (int m = 0; m < 2; ++m) {
            const uint64_t o = m ? j->id2_offset[i] : j->id1_offset[i], tb = m ? j->text2_bytes : j->text1_bytes;
            const uint32_t l = m ? j->id2_length[i] : j->id1_length[i];
            if (o > tb || l > tb - o) {
                why = W + ": id " + std::to_string(m + 1) + " of pair " + std::to_string(i) + " (offset " + std::to_string(o) + ", length " + std::to_string(l) +
                      ") ends behind text" + std::to_string(m + 1) + "_bytes " + std::to_string(tb);
                return CHN_E_INVALID;
            }
        }
    return CHN_OK;
}

// chn_text_pair_ids_host: one pair after another, up to the first that disagrees
static int tpi_host_job(chn_text_pair_job *j, std::string &why) {
    int rc = tpi_check_head(j, "chn_text_pair_ids_host", why);
    if (!rc) rc = tpi_check_ranges(j, "chn_text_pair_ids_host", why);
    if (rc) return rc;
    const TpiHostText a{j->text1}, b{j->text2};
    uint64_t i = 0;
    while (i < j->n_pairs && tpi_agree(a, j->id1_offset[i], j->id1_length[i], b, j->id2_offset[i], j->id2_length[i])) ++i;
    j->first_mismatch = i;
    return CHN_OK;
}

#ifdef __HIPCC__
// device text under the device text contract: aligned dwords that hold a wanted byte, shifted into place
struct TpiDevText {
    const uint8_t *text;
    __device__ __forceinline__ void fetch16(uint64_t addr, uint32_t count, uint32_t w[4]) const { text_fetch16(text, addr, count, w); }
};

struct TpiArgs {
    const uint8_t *text1, *text2;
    const uint64_t *off1, *off2;    // [n] id offsets, range-checked on the host
    const uint32_t *len1, *len2;    // [n] id lengths
    uint64_t n;
    unsigned long long *first;      // preset to all ones; lowered to the smallest disagreeing pair
};

__global__ void __launch_bounds__(256) k_pair_ids(const TpiArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    const TpiDevText t1{a.text1}, t2{a.text2};
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~(WAVE - 1)); i0 < a.n; i0 += stride) {  // (wave-uniform)
        const uint64_t i = i0 + lane_id();
        bool bad = false;
        if (i < a.n) bad = !tpi_agree(t1, a.off1[i], a.len1[i], t2, a.off2[i], a.len2[i]);
        const uint64_t m = __ballot(bad ? 1 : 0);
        if (m && lane_id() == 0) atomicMin(a.first, (unsigned long long)(i0 + (uint64_t)__ffsll((unsigned long long)m) - 1));
    }
}
#endif
