// k1_minimise_probe.inc -- k_minimise_probe: one lane per read (one wavefront per long read in its SPLIT launch), minimiser_hash + bulk_contains (the dominant kernel)
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.

// ------------------------------------------------------------------------------------------------
// k_minimise_probe
// ------------------------------------------------------------------------------------------------
// (MODE_FUSED, MODE_ROWS, MODE_EMPLACE, MODE_LIST and the defaults of the macros below: lds_budget.hpp, which sizes this kernel's LDS)
#ifndef CHN_LOG_BATCH
#define CHN_LOG_BATCH 4  // probe rounds per row-log store (1: a 256-byte dword store per round; 4: a 1 KiB dwordx4 store per four rounds)
#endif
#ifndef CHN_BASE_PIECES
#define CHN_BASE_PIECES 4  // 64-base chunks fetched per base prefetch (4 = 64 bytes per lane: half a line)
#endif  // LIST: log the minimiser values themselves (row-sharded mode)

#ifndef K1_COND_MAX_BINS
// MODE_FUSED indexes with at most this many bins are probed one row at a time (conditional probing).  At Charon's 21.5 % fill the first row
// of a 2-bin index is empty 62 % of the time (1.47 fetches per minimiser instead of 3: cfg2 27.3 -> 24.0 ms); with 8 bins it is empty 14 % of
// the time, 2.17 fetches remain, and the extra rounds cost more issue slots than the fetches saved (cfg5: 12.75 -> 14.25 ms, a kernel that
// issues for 55 % of its life: profiles/r03/sq_fused.txt).  0: never (DIAGNOSTICS: all h rows of every minimiser at once, as MODE_ROWS does).
#define K1_COND_MAX_BINS 4u
#endif
#ifndef FUSED_ROUNDS
#define FUSED_ROUNDS 2u        // MODE_FUSED: probe rounds in flight per wavefront (one row fetch per lane and round; LDS decides the wavefronts per CU)
#endif

struct WaveMeta { uint64_t base, esc_base; uint32_t cap, esc_cap, pad0, pad1; };  // a wavefront's log region / escaped-row region: start and capacity

struct K1Args {
    const uint64_t *words;   // IBF shard, word (row - row_begin) * W + b
    uint64_t *words_rw;      // MODE_EMPLACE
    uint64_t S, row_begin, row_end, seed, powk1;
    uint32_t shift, h, k, wn, n_reads, nseg, B, C;
    uint64_t b2c_packed;     // MODE_FUSED: category of bin b in byte b
    const uint32_t *bases, *nmask;
    const uint64_t *off1, *off2;
    const uint32_t *len1, *len2;
    const uint32_t *order;
    uint32_t *num_hashes, *counts, *unique;
    uint64_t *rows;          // MODE_ROWS: escaped full rows, row j of wavefront g at rows[(wave_meta[g].esc_base + j) * W];
                             // MODE_LIST: minimiser value of entry e of wavefront g at rows[wave_meta[g].base + e]
    uint32_t *rowlog;        // MODE_ROWS: compact entry (see encode_row) of every log entry; MODE_LIST: owner lane
    WaveMeta *wave_meta;     // per wavefront: start of its log region / of its escaped-row region
    uint32_t *wave_count;    // MODE_ROWS / MODE_LIST: entries written by wavefront g
    // Log regions.  `cursor` != nullptr: every wavefront claims its region when it starts (cursor[0] log entries, cursor[1]
    // escaped rows) -- no scan kernel before the launch, layout differs run to run (results do not).  nullptr: wave_meta was
    // filled by k_wave_caps + k_scan_meta (deterministic layout: the dense row-sharded mode needs the same entry order on
    // every rank).  A region holds cap = sum of the 64 read lengths * cap_num / 65536 + 64 entries (twice the density of random
    // sequence; cap_num = 65536 is the hard bound of one emission per base) and (cap >> esc_shift) + 64 escaped rows.  A
    // wavefront that would overrun either, or the buffers, raises status bit 0 and stops writing; the host then re-runs the
    // batch with worst-case regions (chn_batch_wait).
    unsigned long long *cursor;
    uint64_t log_capacity, esc_capacity;  // extent of rowlog / rows (in entries / rows)
    uint32_t cap_num, esc_shift;
    uint32_t *status;        // bit 0: log overflow; bit 1: a segment lies outside [0, n_bases) or is misaligned (it is treated as empty)
    uint64_t n_bases;        // extent of `bases` in bases
    uint32_t nt_probes;      // non-temporal row gathers (index much larger than the Infinity Cache)
    const uint8_t *read_bin; // MODE_EMPLACE: target bin of "read" (genome chunk) r
    uint32_t ablate;         // diagnostics only (CHN_ABLATE env): 1 = skip the gathers, 2 = skip hash+gathers
    uint32_t pack;           // the ring words carry their own offsets (ring_pack_ok(k, wn, seed), lds_budget.hpp): no offset plane in LDS.
                             // The WN_T > 0 instances are always packed: the host launches them only when the rule holds.
    uint32_t chain;          // MODE_ROWS, B <= 128: a row with 4..6 set bins is logged as two chained entries instead of escaping (rowlog_entry.hpp).
                             // Only the ordinary launch of a whole-index batch; its log then goes to k_count_wavelog with K2Args::chain set.
    // Long reads over the lanes of a wavefront (SPLIT launches, below).  n_long = *n_long_ptr reads -- the first n_long entries of
    // `order`, which lists the longest reads first -- are left out by the ordinary launch and taken one per wavefront by the SPLIT
    // launch, whose workgroup x loops over the reads x, x + gridDim.x, ...; its wavefront logs are numbered from wave_slot0.
    const unsigned long long *n_long_ptr;  // nullptr: no read is split
    uint32_t wave_slot0;
    unsigned long long *fetches;           // (may be null) += row fetches issued: h per minimiser, fewer with conditional probing
    // The probe gate (ordinary launch only; both pointers null: no gate).  Every workgroup counts itself in at *gate_started (a control
    // word of the slot, zeroed with the others); the one that finds all the others there -- the grid has no workgroup left to
    // dispatch -- raises *gate_signal, the stream's signal word, to gate_value, this batch's sequence number.  The next batch's launch
    // waits in its queue for exactly that (abi_stream_batch.inc).
    unsigned long long *gate_started, *gate_signal;
    unsigned long long gate_value;
};
// What a gated launch is followed by in its stream: whatever became of the grid, the signal reaches the batch's value.
// (The signal word is host memory behind the bus, which carries add, swap and compare-and-swap only: the attribute has the compiler
//  form the max from a compare-and-swap loop, not from an atomic the far side may never carry out.)
__global__ void k_gate_release(unsigned long long *signal, unsigned long long value) {
    if (threadIdx.x == 0 && blockIdx.x == 0) [[clang::atomic(remote_memory, fine_grained_memory)]] {
        (void)__hip_atomic_fetch_max(signal, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Does the first window (wn canonical k-mer values) of the sequence starting at base `o` hold its minimum more than once?
// Same rolling arithmetic as the kernel body.  A piece of a long read may start cold at `o` only if it does not (SURVEY H3).
__device__ bool first_window_tied(const K1Args &a, uint64_t o, uint32_t wn) {
    const uint64_t INV5 = 0xCCCCCCCCCCCCCCCDULL;
    const uint32_t k = a.k, w = wn + k - 1;
    uint64_t fwd = 0, rc = 0, best = ~0ULL;
    bool tie = false;
    auto digits = [&](uint64_t x, uint32_t &d, uint32_t &cd) {
        const uint32_t code = (a.bases[x >> 4] >> ((x & 15u) * 2u)) & 3u;
        const uint32_t nf = a.nmask ? (a.nmask[x >> 5] >> (x & 31u)) & 1u : 0u;
        d = nf ? 3u : code + (code == 3u);
        cd = nf ? 3u : (3u - code) + (code == 0u);
    };
    for (uint32_t i = 0; i < w; ++i) {
        uint32_t d_in, cd_in, d_out = 0, cd_out = 0;
        digits(o + i, d_in, cd_in);
        if (i >= k) digits(o + i - k, d_out, cd_out);
        fwd = (fwd - (uint64_t)d_out * a.powk1) * 5u + d_in;
        rc = (rc - cd_out) * INV5 + (uint64_t)cd_in * a.powk1;
        if (i + 1 >= k) {
            const uint64_t vf = fwd ^ a.seed, vr = rc ^ a.seed, v = vf < vr ? vf : vr;
            if (v < best) { best = v; tie = false; } else if (v == best) tie = true;
        }
    }
    return tie;
}

// (the compact row-log entry, its escape and its chain mode: rowlog_entry.hpp)
// regions are multiples of 64 entries: with 256-byte aligned buffers every probe round's store is two whole 128-byte lines
__host__ __device__ __forceinline__ uint64_t wave_log_cap(uint64_t sum_len, uint32_t cap_num) { return (((sum_len * cap_num) >> 16) + 64 + 63) & ~63ULL; }
__host__ __device__ __forceinline__ uint64_t wave_esc_cap(uint64_t cap, uint32_t esc_shift) { return (cap >> esc_shift) + 64; }
// returns the entry without the escape index (the caller adds (index + 1) << 2 for an escaped row)
template <int W>
__device__ __forceinline__ uint32_t encode_row(const uint64_t *acc, uint32_t B, uint32_t owner, bool &escaped) {
    uint32_t e[2];  // (unchained: the row-sharded kernels' logs; a row without a set bin gives owner << 26, which names nothing)
    rowlog_encode<W>(acc, B, owner, false, e, escaped);
    return e[0];
}

// LDS-DMA gather: every active lane's 16 bytes at `src` land at LDS byte address lds_dst (wave-uniform) + 16 * lane; no VGPR
// destination.  Written in asm so that hipcc does not know of the pending LDS write (it would guard every later ds_read of
// the probe buffer with s_waitcnt vmcnt(0)); completion is the caller's counted s_waitcnt vmcnt(N).  M0 carries the LDS
// base and is compiler-reserved: saved and restored inside the statement (cdna_hip_programming.md, inline-asm notes).
__device__ __forceinline__ void lds_dma_b128(const void *src, uint32_t lds_dst, bool nt) {
    unsigned keep;
    const uint32_t dst = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_dst);
    if (nt)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
}
// s_waitcnt takes an immediate: wait until at most n (wave-uniform) vector-memory operations of this wavefront are outstanding.
// A smaller immediate than asked for is always safe (it only waits for more).
__device__ __forceinline__ void wait_vmcnt(uint32_t n) {
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        case 9: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    }
}

// Sliding-window minimum without rescans.  Value indices are cut into blocks of wn; slot u of the per-lane LDS
// ring holds, for u <= t (t = offset of the newest value in its block), the raw values of the current block and,
// for u > t, the rightmost suffix minimum S[u] of the PREVIOUS block (value in `ring`, offset in `spos`).  The
// rightmost minimum of the window ending at offset t is then combine(S[t+1], running prefix minimum), and the
// suffix minima are produced in place by one backward pass at every block end (all lanes are at the same t).
//
// Packed ring (a.pack; always when WN_T > 0): there is no `spos` plane.  A slot holds (v << pb) | (wn - 1 - u), pb = bits(wn - 1), u the
// offset of the value in its block -- a raw value stored during the block and a suffix minimum read the same.  The top pb bits of v
// are constants of the launch (the seed's: the k-mer ranks are below 5^k and ring_pack_ok says they end below bit 64 - pb), so the shift
// loses nothing and they are put back when a word is unpacked.  The offset is complemented so that of two equal values the RIGHTMOST
// has the smaller word: the backward pass is a chain of unsigned 64-bit minima over the words and still yields the rightmost suffix
// minimum (the tie rule of SURVEY A.2), with no position select and no byte stores.
//
// Probe rounds are software-pipelined, two in flight: a round's h gathers are LDS-DMA loads into the wavefront's probe buffer
// and are only retired (AND + accumulate / row-log store) two rounds (~22 bases) later, behind a counted s_waitcnt vmcnt(N),
// so the HBM latency of the random gathers overlaps the hash rolling of the same wavefront.  Bases are fetched
// CHN_BASE_PIECES x 64 at a time (asm loads the kernel tracks itself), one chunk ahead of their use.
//
// SPLIT launches (long reads, src/dehost_main.cpp:346-350 caps a read's length only at uint32): ONE READ PER WAVEFRONT, cut into up
// to 64 pieces that start at multiples of 64 bases and overlap by w - 1 bases; lane j rolls piece j.  A piece other than the first
// starts "cold": its first window only sets the tracked minimum (mv, q) and emits nothing -- the emission rule (SURVEY A.2) depends
// on the past only through (mv, q), mv is always the window's minimum, and when that minimum occurs ONCE in the window its position
// is q whatever the history was.  So a piece whose first window holds its minimum once continues exactly where the sequential
// rule would be; the piece before it runs up to and including that window's last value.  A piece whose first window has a tie
// is not started: the piece before it simply runs on through it (a homopolymer read ends up as one lane's work, as before).  All
// lanes add to owner slot 0 (LDS counters or the owner field of the row-log entries); lane 0 writes the read's results.
__host__ __device__ constexpr uint32_t ring_pbits(uint32_t wn) {  // bits(wn - 1): width of a packed ring word's offset field
    uint32_t n = 0;
    for (uint32_t x = wn - 1; x; x >>= 1) ++n;
    return n;
}
template <int W, int MODE, int WN_T, bool SPLIT = false, bool COND_T = false>
__global__ __launch_bounds__(WAVE) void k_minimise_probe(const K1Args a) {
    extern __shared__ __align__(16) unsigned char smem[];
    // Probe gate: arrivals are counted (workgroups are dealt round-robin over the XCDs: the last index starting says nothing about the
    // others); max and not store, so the signal never moves backwards.  Done with before the first load the kernel counts itself.
    if (!SPLIT && a.gate_started && threadIdx.x == 0) {
        if (atomicAdd(a.gate_started, 1ULL) == (unsigned long long)gridDim.x - 1) [[clang::atomic(remote_memory, fine_grained_memory)]] {
            (void)__hip_atomic_fetch_max(a.gate_signal, a.gate_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    const uint32_t n_long = a.n_long_ptr ? (uint32_t)__builtin_nontemporal_load(a.n_long_ptr) : 0u;
    uint32_t item = blockIdx.x;
    if (SPLIT && item >= n_long) return;
    do {  // (one pass unless SPLIT)
    const uint32_t wslot = SPLIT ? a.wave_slot0 + item : item;  // this wavefront's log / region table entry
    const uint32_t wn = WN_T ? (uint32_t)WN_T : a.wn;
    // LDS carve-up (one wavefront per workgroup)
    constexpr uint32_t NBLK = (W == 1 || W == 2) ? 1u : 2u;  // 16-byte blocks fetched per probed row (W = 1: the block holding the word)
    // COND (MODE_FUSED with at most K1_COND_MAX_BINS bins): ONE hash function per round and lane (conditional probing, below): a round's landing
    // zone is 1 KiB, FUSED_ROUNDS of them are in flight, and the queue is longer because surviving entries come back into it
    constexpr bool COND = MODE == MODE_FUSED && COND_T;
    // (COND: at most 127 entries wait when a turn starts and a retired round adds at most 64 survivors: 191.  Not a power of two -- 64 more
    //  entries of 20 bytes would cost a wavefront per CU)
    constexpr uint32_t QC = COND ? QCAP + WAVE : QCAP;
    auto qwrap = [&](uint32_t x) -> uint32_t {  // position x (below 3 QC) in the queue ring
        if (!COND) return x & (QC - 1);
        x = x >= QC ? x - QC : x;
        return x >= QC ? x - QC : x;
    };
    const uint32_t pb_round = COND ? 1024u : (MODE == MODE_FUSED || MODE == MODE_ROWS) ? a.h * NBLK * 1024u : 0u;  // probe buffer of one round
    unsigned char *pbuf = smem;                                               // [rounds in flight][h][NBLK][64 lanes][16 B] LDS-DMA landing zone
    const uint32_t pbuf_lds = (uint32_t)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;  // its LDS byte address
    uint64_t *ring = reinterpret_cast<uint64_t *>(smem + (COND ? FUSED_ROUNDS : 2u) * pb_round);       // [wn][64] per-lane window store
    uint64_t *qv = ring + (size_t)wn * WAVE;                                  // [QC] queued minimiser values
    uint64_t *qa = qv + QC;                                                   // [QC] COND: AND of the rows fetched so far (entries that came back)
    uint32_t *qm = reinterpret_cast<uint32_t *>(qa + (COND ? QC : 0u));       // [QC] owner lane | next hash function << 6
    uint64_t *rbase = reinterpret_cast<uint64_t *>(qm + QC);                  // [64] EMPLACE bin
    uint32_t *cnt = reinterpret_cast<uint32_t *>(rbase + (MODE == MODE_EMPLACE ? WAVE : 0));  // MODE_FUSED [C][64]
    uint32_t *unq = cnt + (MODE == MODE_FUSED ? a.C * WAVE : 0);              // MODE_FUSED [C][64]
    // packed ring: the words carry their offsets (wave-uniform; a compile-time fact of the WN_T > 0 instances)
    const bool PK = WN_T ? true : a.pack != 0;
    constexpr uint32_t PB_T = ring_pbits(WN_T ? WN_T : 1);
    const uint32_t pbits = WN_T ? PB_T : ring_pbits(wn);  // bits(wn - 1)
    const uint32_t omask = (1u << pbits) - 1u;
    const uint64_t seed_top = pbits ? (a.seed >> (64u - pbits)) << (64u - pbits) : 0ULL;  // the bits of every value that the shift drops
    uint8_t *spos = reinterpret_cast<uint8_t *>(unq + (MODE == MODE_FUSED ? a.C * WAVE : 0));  // [wn][64] offset of S[u] (not packed)
    // MODE_ROWS: CHN_LOG_BATCH rounds of compact entries are staged here and leave as ONE store of 16 bytes per lane
    uint32_t *sbuf = reinterpret_cast<uint32_t *>(smem + (((size_t)(spos + (PK ? (size_t)0 : (size_t)wn * WAVE) - smem) + 15) & ~(size_t)15));

    const uint32_t lane = lane_id();
    const uint32_t g = SPLIT ? item : item * WAVE + lane;
    const bool valid = SPLIT ? true : (g < a.n_reads && g >= n_long);
    const uint32_t r = valid ? (a.order ? a.order[g] : g) : 0;
    const uint32_t own = SPLIT ? 0u : lane;  // owner slot of this lane's minimisers
    bool cold = false;                       // SPLIT: this lane's piece starts in the middle of the read

    if (MODE == MODE_FUSED)
        for (uint32_t c = 0; c < a.C; ++c) { cnt[c * WAVE + lane] = 0; unq[c * WAVE + lane] = 0; }
    if (MODE == MODE_EMPLACE) rbase[lane] = valid ? a.read_bin[r] : 0;
    __syncthreads();

    const uint32_t k = a.k;
    const uint64_t INV5 = 0xCCCCCCCCCCCCCCCDULL;  // 5^-1 mod 2^64 (exact division of the reverse strand)
    uint32_t my_emitted = 0;                      // == ReadEntry::num_hashes_ (include/read_entry.hpp:89)
    uint32_t qhead = 0, qcount = 0;               // wave-uniform queue state
    // Probe rounds: TWO in flight per wavefront.  A round's h gathers are LDS-DMA loads (global_load_lds_dwordx4: every lane's
    // 16-byte block lands in the wavefront's probe buffer, no VGPR destination), so hipcc has nothing to guard: round 1's
    // register gathers made it wait vmcnt(0) before every re-use of their destination registers and at every loop seam, which
    // drained whatever was in flight.  All waits are explicit and counted: before round r is retired the wavefront waits until
    // at most the DMAs of round r+1 are outstanding.
    uint32_t meta_s0 = 0, meta_s1 = 0;  // per slot: owner lane | per-read index << 6
    uint32_t sel_s0 = 0, sel_s1 = 0;    // per slot: bit i = the row of hash function i starts 8 bytes into its first 16-byte block
    uint32_t n_s0 = 0, n_s1 = 0;        // per slot: entries of the round (wave-uniform)
    uint32_t r_issued = 0, r_retired = 0;  // wave-uniform round counters; round r lives in slot r & 1
    uint32_t base_seq = 0;                 // r_issued when the outstanding base prefetch was issued
    bool base_ready = true;  // wave-uniform: no untracked (asm) base prefetch is outstanding
    uint32_t n_fetch = 0;    // row fetches issued by this wavefront (wave-uniform)
    uint32_t consumed = 0;   // MODE_ROWS / MODE_LIST: log entries of this wavefront so far (wave-uniform)
    uint32_t esc_n = 0;      // MODE_ROWS: escaped rows so far (wave-uniform)

    // segments of this lane's read, validated (a device batch is not checked by the host: a segment outside the base buffer
    // is treated as empty and reported through the status word)
    uint32_t seg_len0 = 0, seg_len1 = 0;
    uint64_t seg_off0 = 0, seg_off1 = 0;
    if (valid) {
        bool bad = false;
        {
            const uint32_t l = a.len1[r];
            const uint64_t o = a.off1[r];
            if ((o & 63u) || o > a.n_bases || l > a.n_bases - o) bad = true; else { seg_len0 = l; seg_off0 = o; }
        }
        if (a.nseg > 1) {
            const uint32_t l = a.len2[r];
            const uint64_t o = a.off2[r];
            if ((o & 63u) || o > a.n_bases || l > a.n_bases - o) bad = true; else { seg_len1 = l; seg_off1 = o; }
        }
        if (bad && a.status) atomicOr(a.status, 2u);
    }
    uint32_t read_len = seg_len0;  // SPLIT: the whole read (wave-uniform)
    if (SPLIT) {
        const uint32_t w = wn + a.k - 1, Lr = seg_len0;
        const uint64_t roff = seg_off0;
        // P pieces; piece j starts at base floor(j (Lr - w) / P) rounded down to a multiple of 64, so every piece has more than one
        // window and the pieces differ by at most 64 bases in length
        const uint32_t P = Lr > w + 64u ? min(64u, (Lr - w) >> 6) : 1u;
        const uint32_t start = lane < P ? (uint32_t)(((uint64_t)lane * (Lr - w)) / P) & ~63u : 0u;
        const bool tied = lane > 0 && lane < P && first_window_tied(a, roff + start, wn);
        const uint64_t alive = __ballot(lane < P && !tied) | 1ULL;
        seg_len0 = 0;
        if ((alive >> lane) & 1ULL) {
            const uint64_t above = lane == 63 ? 0ULL : alive >> (lane + 1);
            uint32_t end = Lr;
            if (above) {  // runs up to and including the first window of the next piece that starts
                const uint32_t nx = lane + 1 + (uint32_t)__ffsll((long long)above) - 1;
                end = ((uint32_t)(((uint64_t)nx * (Lr - w)) / P) & ~63u) + w;
            }
            seg_off0 = roff + start; seg_len0 = end - start; cold = lane > 0;
        }
    }
    // this wavefront's log region
    uint64_t wbase = 0, ebase = 0;
    uint32_t wcap = 0, ecap = 0;
    if (MODE == MODE_ROWS || MODE == MODE_LIST) {
        if (a.cursor) {
            uint64_t sum = (uint64_t)seg_len0 + seg_len1;
            for (int o = 32; o > 0; o >>= 1) sum += (uint64_t)__shfl_xor((long long)sum, o);
            if (SPLIT) sum = read_len;  // the pieces' emissions together are those of the read (their overlaps emit nothing twice)
            const uint64_t cap = wave_log_cap(sum, a.cap_num), ec = wave_esc_cap(cap, a.esc_shift);  // (MODE_LIST: the escaped rows of the later AND kernel)
            uint64_t b0 = 0, b1 = 0;
            if (lane == 0) {
                b0 = atomicAdd(a.cursor, (unsigned long long)cap);
                b1 = atomicAdd(a.cursor + 1, (unsigned long long)ec);
                a.wave_meta[wslot].base = b0;
                a.wave_meta[wslot].esc_base = b1;
            }
            wbase = (uint64_t)__shfl((long long)b0, 0);
            ebase = (uint64_t)__shfl((long long)b1, 0);
            // a region that does not fit the buffers is cut (to nothing if need be): the overflow bit then triggers the re-run
            const uint64_t room = wbase < a.log_capacity ? a.log_capacity - wbase : 0, eroom = ebase < a.esc_capacity ? a.esc_capacity - ebase : 0;
            wcap = (uint32_t)(cap < room ? cap : room);
            ecap = (uint32_t)(ec < eroom ? ec : eroom);
            if (wcap > 0xffffffc0u) wcap = 0xffffffc0u;
        } else {  // regions laid out by k_wave_caps + k_scan_meta: wave g + 1 starts where wave g ends
            wbase = a.wave_meta[wslot].base; ebase = a.wave_meta[wslot].esc_base;
            const uint64_t wend = wslot + 1 < gridDim.x ? a.wave_meta[wslot + 1].base : a.log_capacity;
            const uint64_t eend = wslot + 1 < gridDim.x ? a.wave_meta[wslot + 1].esc_base : a.esc_capacity;
            const uint64_t c = (wend < a.log_capacity ? wend : a.log_capacity), ce = (eend < a.esc_capacity ? eend : a.esc_capacity);
            wcap = (uint32_t)(c > wbase ? (c - wbase < 0xffffffc0ULL ? c - wbase : 0xffffffc0ULL) : 0);
            ecap = (uint32_t)(ce > ebase ? (ce - ebase < 0xffffffc0ULL ? ce - ebase : 0xffffffc0ULL) : 0);
        }
        if (ecap > ROWLOG_ESC_MAX) ecap = ROWLOG_ESC_MAX;
        if (lane == 0) { a.wave_meta[wslot].cap = wcap; a.wave_meta[wslot].esc_cap = ecap; }
    }
    bool overflow = false;   // wave-uniform
    const bool chain = MODE == MODE_ROWS && !SPLIT && a.chain != 0;  // rows with 4..6 set bins are chained, not escaped (wave-uniform)
    uint32_t staged = 0, flushed = 0;  // MODE_ROWS: kept entries waiting in sbuf / already stored (consumed = flushed + staged)

    // write the staged compact entries [0, count) to the row log at entry `first` (a multiple of 64; of CHN_LOG_BATCH x 64 unless a chained round forced an early flush): 16 bytes per lane
    auto log_flush = [&](uint32_t first, uint32_t count) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (uint32_t t4 = 0; t4 < CHN_LOG_BATCH * WAVE / 4; t4 += WAVE) {
            const uint32_t q4 = t4 + lane;  // uint4 index inside the batch
            if (q4 * 4 < count) {
                const uint4 v = reinterpret_cast<const uint4 *>(sbuf)[q4];
                *reinterpret_cast<uint4 *>(a.rowlog + wbase + first + q4 * 4) = v;
            }
        }
    };

    // Retire round r_retired (slot r_retired & 1): wait until only the DMAs of the rounds issued after it are outstanding, AND the
    // h rows, then count (MODE_FUSED, LDS) or append the round to the wavefront's row log (MODE_ROWS: 64 consecutive entries,
    // two whole 128-byte lines).  Called BEFORE the next round is issued, so the stores are older than every DMA that a
    // later counted wait leaves in flight.
    auto probe_retire = [&]() {
        const uint32_t slot = r_retired & 1u;
        const uint32_t newer = r_issued - r_retired - 1u;  // rounds issued after this one: 0 or 1
        wait_vmcnt((a.ablate & 3u) ? 0u : newer * a.h * NBLK);
        // what is now complete: everything issued before the first DMA of the newest round; a base prefetch is among that iff it
        // was issued before that round
        if (newer == 0u || base_seq < r_issued) base_ready = true;
        const uint32_t n = slot ? n_s1 : n_s0, meta = slot ? meta_s1 : meta_s0, sel = slot ? sel_s1 : sel_s0;
        const bool has = lane < n;
        uint64_t acc[W];
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = ~0ULL;
        const uint4 *pb4 = reinterpret_cast<const uint4 *>(pbuf + slot * pb_round);
#pragma unroll
        for (uint32_t i = 0; i < 5; ++i)
            if (i < a.h) {
                const uint4 v0 = pb4[(i * NBLK) * WAVE + lane];
                const uint64_t q0 = (uint64_t)v0.x | ((uint64_t)v0.y << 32), q1 = (uint64_t)v0.z | ((uint64_t)v0.w << 32);
                if (W == 1) {
                    acc[0] &= ((sel >> i) & 1u) ? q1 : q0;
                } else if (W == 2) {
                    acc[0] &= q0; acc[W > 1 ? 1 : 0] &= q1;
                } else {
                    const uint4 v1 = pb4[(i * NBLK + (NBLK - 1)) * WAVE + lane];
                    const uint64_t q2 = (uint64_t)v1.x | ((uint64_t)v1.y << 32), q3 = (uint64_t)v1.z | ((uint64_t)v1.w << 32);
                    if (W == 3) {
                        const bool odd = (sel >> i) & 1u;
                        acc[0] &= odd ? q1 : q0; acc[W > 1 ? 1 : 0] &= odd ? q2 : q1; acc[W > 2 ? 2 : 0] &= odd ? q3 : q2;
                    } else {
                        acc[0] &= q0; acc[W > 1 ? 1 : 0] &= q1; acc[W > 2 ? 2 : 0] &= q2; acc[W > 3 ? 3 : 0] &= q3;
                    }
                }
            }
        const uint32_t owner = meta & 63u;
        if (MODE == MODE_FUSED) {
            uint64_t m = has ? (acc[0] & ((a.B >= 64) ? ~0ULL : ((1ULL << a.B) - 1))) : 0;
            const bool single = __popcll(m) == 1;
            while (m) {
                const uint32_t b = (uint32_t)__ffsll((long long)m) - 1;
                m &= m - 1;
                const uint32_t c = (uint32_t)(a.b2c_packed >> (8 * b)) & 0xffu;
                atomicAdd(&cnt[c * WAVE + owner], 1u);
                if (single) atomicAdd(&unq[c * WAVE + owner], 1u);
            }
        } else if (MODE == MODE_ROWS) {
            bool esc = false;
            uint32_t ent[2] = {0u, 0u}, ne = 0;
            if (has) ne = rowlog_encode<W>(acc, a.B, owner, chain, ent, esc);
            uint32_t entry = ent[0];
            // A row without a set bin says nothing to the count kernel (it only counts in num_hashes, which this kernel keeps itself):
            // it gets no entry.  In a read set that mostly misses the index -- what dehosting sees -- that is most of the log.
            // Chain mode: a row with 4..6 set bins gets two entries, back to back: a lane's rank counts the lanes before it once more
            // for each of them that has two.
            const bool keep = ne != 0, two = ne == 2;
            const uint64_t km = __ballot(keep), tm = __ballot(two);
            const uint32_t nk = (uint32_t)__popcll(km) + (uint32_t)__popcll(tm);
            const uint32_t krank = __builtin_amdgcn_mbcnt_hi((uint32_t)(km >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)km, 0u)) +
                                   __builtin_amdgcn_mbcnt_hi((uint32_t)(tm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)tm, 0u));
            const bool fits = consumed + nk <= wcap;  // wave-uniform
            const uint64_t em = __ballot(esc);
            if (em) {  // escaped rows take the next free slots of the wavefront's escaped-row region
                const uint32_t ne = (uint32_t)__popcll(em);
                const uint32_t eslot = esc_n + __builtin_amdgcn_mbcnt_hi((uint32_t)(em >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)em, 0u));
                if (esc_n + ne > ecap) overflow = true;
                else if (esc && fits) {
#ifndef CHN_DIAG_NO_ESC_STORE  // DIAGNOSTICS BUILD ONLY: what do the scattered 8W-byte escaped-row stores cost?
                    uint64_t *dst = a.rows + (ebase + eslot) * W;
#pragma unroll
                    for (int w = 0; w < W; ++w) dst[w] = acc[w];
#endif
                    entry |= (eslot + 1) << 2;
                }
                esc_n += ne;
            }
#ifndef CHN_DIAG_NO_STORE  // DIAGNOSTICS BUILD ONLY: what do the row-log stores cost the probe pipeline?
            if (CHN_LOG_BATCH == 1) {
                if (keep && fits) a.rowlog[wbase + consumed + krank] = entry;
                if (two && fits) a.rowlog[wbase + consumed + krank + 1] = ent[1];
            } else {
                // kept entries are staged back to back; whenever CHN_LOG_BATCH x 64 of them are there they leave as one 1 KiB store
                // and the (at most 64) entries behind them move to the front
                if (staged + nk > (CHN_LOG_BATCH + 1) * WAVE) {
                    // (chain mode only, and rare: a round of up to 128 entries that the staging buffer cannot take beside what waits there --
                    //  the whole 256-byte pieces of that leave first)
                    const uint32_t whole = staged & ~(WAVE - 1u);
                    if (fits) log_flush(flushed, whole);
                    flushed += whole;
                    const uint32_t rem = staged - whole;
                    uint32_t t = 0;
                    if (lane < rem) t = sbuf[whole + lane];
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    if (lane < rem) sbuf[lane] = t;
                    staged = rem;
                }
                if (keep) sbuf[staged + krank] = entry;
                if (two) sbuf[staged + krank + 1] = ent[1];
                staged += nk;
                if (staged >= CHN_LOG_BATCH * WAVE) {
                    if (fits) log_flush(flushed, CHN_LOG_BATCH * WAVE);
                    flushed += CHN_LOG_BATCH * WAVE;
                    const uint32_t rem = staged - CHN_LOG_BATCH * WAVE;
                    uint32_t t = 0;
                    if (lane < rem) t = sbuf[CHN_LOG_BATCH * WAVE + lane];
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    if (lane < rem) sbuf[lane] = t;
                    staged = rem;
                }
            }
#endif
            if (!fits) overflow = true;
            consumed += nk;
        }
        r_retired += 1;
    };

    // Issue the next round: the first n_take queued minimisers, one per lane; h row hashes (hash_and_fit) and h * NBLK LDS-DMA
    // gathers into the round's slot of the probe buffer.
    auto probe_issue = [&](uint32_t n_take) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the queue writes (one wavefront per workgroup: LDS is in order)
        const bool has = lane < n_take;
        const uint32_t qslot = qwrap(qhead + lane);
        const uint64_t val = qv[qslot];
        const uint32_t meta = qm[qslot];
        const uint32_t slot = r_issued & 1u;
        uint32_t sel = 0;
        if (has) {
            const uint32_t dst_lds = pbuf_lds + slot * pb_round;  // LDS byte address of the round's slot
#pragma unroll
            for (uint32_t i = 0; i < 5; ++i)
                if (i < a.h) {
                    const uint64_t row = hash_and_fit_row(val, c_ibf_seeds[i], a.S, a.shift);
                    const uint64_t o = (row - a.row_begin) * (8u * W);  // byte offset of the row in this shard
                    if (W & 1) sel |= (uint32_t)((o >> 3) & 1u) << i;
                    const unsigned char *src = reinterpret_cast<const unsigned char *>(a.words) + (o & ~15ULL);
                    if (a.ablate & 3u) continue;
                    // Cache policy by index size (tools/gather_policy_bench.hip): from a table far larger than the 256 MiB Infinity
                    // Cache a probed line is never reused and `nt` gathers sustain 11 % more (54.3 vs 48.8 G/s at 39 GB); from a
                    // ~1 GiB table a quarter of the probes hit the Infinity Cache and the default policy wins (53.2 vs 49.8 G/s).
#pragma unroll
                    for (uint32_t j = 0; j < NBLK; ++j) lds_dma_b128(src + 16 * j, dst_lds + (i * NBLK + j) * 1024u, a.nt_probes != 0);
                }
        }
        if (slot) { meta_s1 = meta; sel_s1 = sel; n_s1 = n_take; } else { meta_s0 = meta; sel_s0 = sel; n_s0 = n_take; }
        n_fetch += n_take * a.h;
        r_issued += 1;
        qhead = qwrap(qhead + n_take);
        qcount -= n_take;
    };

    // ---- MODE_FUSED: conditional probing ----------------------------------------------------------------------------------------------
    // bulk_contains ANDs the h rows of a minimiser (src/dehost_main.cpp:368, SURVEY A.3).  With few bins most rows have no user bin set --
    // at 21.5 % fill a 2-bin row is empty 62 % of the time -- and once the running AND is zero the other rows cannot change that: AND with
    // zero is zero, the minimiser counts for nothing (bit-exact).  So a round fetches ONE row per lane: the row of hash function i of a
    // queue entry (value, owner, i, AND so far).  At retire, an entry whose AND & bin mask is zero is dropped; one with i + 1 < h goes back
    // into the queue for its next row; one that has seen all h rows is counted.  Every round is 64 useful fetches (1.47 per minimiser for
    // 2 bins instead of 3) and costs one LDS-DMA instruction; FUSED_ROUNDS rounds are in flight.
    uint64_t fv[FUSED_ROUNDS], fa[FUSED_ROUNDS];   // per slot: the lane's value and its AND so far
    uint32_t fm[FUSED_ROUNDS], fn[FUSED_ROUNDS];   // per slot: owner | i << 6 | (second half of the 16-byte block) << 31; entries of the round
#pragma unroll
    for (uint32_t sidx = 0; sidx < FUSED_ROUNDS; ++sidx) { fv[sidx] = 0; fa[sidx] = 0; fm[sidx] = 0; fn[sidx] = 0; }
    const uint64_t binmask = (a.B >= 64) ? ~0ULL : ((1ULL << a.B) - 1);
    auto cprobe_retire = [&]() {
        const uint32_t slot = r_retired % FUSED_ROUNDS;
        const uint32_t newer = r_issued - r_retired - 1u;  // rounds issued after this one, one DMA instruction each
        wait_vmcnt((a.ablate & 3u) ? 0u : newer);
        if (base_seq <= r_issued - newer) base_ready = true;  // a base prefetch older than the oldest round still in flight has landed
        uint64_t val = 0, acc = 0; uint32_t meta = 0, n = 0;
#pragma unroll
        for (uint32_t sidx = 0; sidx < FUSED_ROUNDS; ++sidx) if (slot == sidx) { val = fv[sidx]; acc = fa[sidx]; meta = fm[sidx]; n = fn[sidx]; }
        const uint4 v0 = reinterpret_cast<const uint4 *>(pbuf + slot * 1024u)[lane];
        const uint64_t q0 = (uint64_t)v0.x | ((uint64_t)v0.y << 32), q1 = (uint64_t)v0.z | ((uint64_t)v0.w << 32);
        acc &= (meta >> 31) ? q1 : q0;
        if (a.ablate & 3u) acc = 0;
        const uint32_t i = (meta >> 6) & 7u, owner = meta & 63u;
        uint64_t m = lane < n ? (acc & binmask) : 0;
        const bool again = m != 0 && i + 1 < a.h;
        const uint64_t am = __ballot(again);
        if (am) {  // survivors go back into the queue for their next row
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(am >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)am, 0u));
            if (again) {
                const uint32_t pos = qwrap(qhead + qcount + rank);
                qv[pos] = val; qa[pos] = acc; qm[pos] = owner | ((i + 1) << 6);
            }
            qcount += (uint32_t)__popcll(am);
        }
        if (!again) {  // all h rows seen: count (ReadEntry::get_counts with one bin per category, include/read_entry.hpp:92-138)
            const bool single = __popcll(m) == 1;
            while (m) {
                const uint32_t b = (uint32_t)__ffsll((long long)m) - 1;
                m &= m - 1;
                const uint32_t c = (uint32_t)(a.b2c_packed >> (8 * b)) & 0xffu;
                atomicAdd(&cnt[c * WAVE + owner], 1u);
                if (single) atomicAdd(&unq[c * WAVE + owner], 1u);
            }
        }
        r_retired += 1;
    };
    auto cprobe_issue = [&](uint32_t n_take) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the queue writes (one wavefront per workgroup: LDS is in order)
        const bool has = lane < n_take;
        const uint32_t qslot = qwrap(qhead + lane);
        const uint64_t val = qv[qslot];
        uint32_t meta = qm[qslot];
        const uint32_t i = (meta >> 6) & 7u;
        const uint64_t acc = i ? qa[qslot] : ~0ULL;  // a fresh minimiser has no AND yet
        const uint32_t slot = r_issued % FUSED_ROUNDS;
        if (has) {
            // (the seed by selects: an indexed read of the constant table would be a vector memory load the compiler waits for with vmcnt(0))
            const uint64_t seed = i == 0 ? c_ibf_seeds[0] : i == 1 ? c_ibf_seeds[1] : i == 2 ? c_ibf_seeds[2] : i == 3 ? c_ibf_seeds[3] : c_ibf_seeds[4];
            const uint64_t row = hash_and_fit_row(val, seed, a.S, a.shift);
            const uint64_t o = (row - a.row_begin) * 8u;  // W = 1
            meta |= (uint32_t)((o >> 3) & 1u) << 31;
            if (!(a.ablate & 3u)) lds_dma_b128(reinterpret_cast<const unsigned char *>(a.words) + (o & ~15ULL), pbuf_lds + slot * 1024u, a.nt_probes != 0);
        }
#pragma unroll
        for (uint32_t sidx = 0; sidx < FUSED_ROUNDS; ++sidx) if (slot == sidx) { fv[sidx] = val; fa[sidx] = acc; fm[sidx] = meta; fn[sidx] = n_take; }
        n_fetch += n_take;
        r_issued += 1;
        qhead = qwrap(qhead + n_take);
        qcount -= n_take;
    };

    // one probe turn: with two rounds in flight retire the older one (issued ~22 bases ago), then issue the next
    auto probe_turn = [&](uint32_t n_take) {
        if (COND) {
            // retire the oldest round when all slots are taken (its survivors join the queue), issue the next; as long as a full round is
            // queued -- survivors can make one -- go on
            for (;;) {
                if (r_issued - r_retired == FUSED_ROUNDS) cprobe_retire();
                cprobe_issue(n_take);
                if (qcount < WAVE) break;
                n_take = WAVE;
            }
            return;
        }
        if (MODE == MODE_FUSED || MODE == MODE_ROWS) {
            if (r_issued - r_retired == 2u) probe_retire();
            probe_issue(n_take);
            return;
        }
        // MODE_LIST (log the minimiser values) and MODE_EMPLACE (set their bits): nothing is gathered, no pipeline
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const bool has = lane < n_take;
        const uint32_t qslot = qwrap(qhead + lane);
        const uint64_t val = qv[qslot];
        const uint32_t meta = qm[qslot];
        if (MODE == MODE_EMPLACE) {
            if (has) {
                const uint32_t bin = (uint32_t)rbase[meta & 63u];
                for (uint32_t i = 0; i < a.h; ++i) {
                    uint64_t row = hash_and_fit_row(val, c_ibf_seeds[i], a.S, a.shift);
                    if (row >= a.row_begin && row < a.row_end)
                        atomicOr((unsigned long long *)&a.words_rw[(row - a.row_begin) * W + (bin >> 6)], 1ULL << (bin & 63));
                }
            }
        } else {
            const bool fits = consumed + n_take <= wcap;  // wave-uniform
            if (has && fits) {
                const uint64_t e = wbase + consumed + lane;
                a.rows[e] = val;
                a.rowlog[e] = (meta & 63u) << 26;
            }
            if (!fits) overflow = true;
            consumed += n_take;
        }
        qhead = qwrap(qhead + n_take);
        qcount -= n_take;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };

    // per-segment rolling state (hoisted so that the step body below can be one generic lambda)
    uint64_t fwd = 0, rc = 0, hist2 = 0, mv = 0, pv = 0;
    uint32_t histn = 0, q = 0, pq = 0;
    uint32_t t = 0, blk = 0;  // wave-uniform: offset of the newest value in its block, start index of that block
    uint32_t L = 0;
    bool has_nmask = false;

    // One base step.  STEADY: i >= k + wn and every lane is active (compile-time tag: the start-up, first-window, short-read
    // and activity checks disappear).  HASN: the batch carries an N mask.
    auto step = [&](auto STEADY, auto HASN, const uint32_t i, const uint32_t j, const uint32_t cur, const uint32_t ncur) {
        constexpr bool kSteady = decltype(STEADY)::value, kHasN = decltype(HASN)::value;
        const bool act = kSteady || i < L;
        bool emit = false;
#ifdef CHN_K1_FAKE_EMIT
        // DIAGNOSTICS BUILD ONLY (tools/build_diag.sh): no hashing, no window minimum -- a synthetic emission pattern at the
        // minimiser density of random sequence, so that the probe pipeline can be timed without the VALU work in front of it
        const bool have_value = false;
        if (act) {
            uint32_t hsh = (i * 0x9E3779B1u) ^ (lane * 0x85EBCA6Bu) ^ (wslot * 0xC2B2AE35u) ^ cur;
            hsh ^= hsh >> 15; hsh *= 0x2C1B3C6Du; hsh ^= hsh >> 12;
            emit = (hsh & 0xffffu) < 5833u;
            mv = mix64(((uint64_t)hsh << 32) | i);
        }
        if (false) {
            const uint32_t code = (cur >> (j * 2)) & 3u;
#else
        const bool have_value = kSteady || i + 1 >= k;  // wave-uniform
        if (act) {
            const uint32_t code = (cur >> (j * 2)) & 3u;
#endif
            const uint32_t nf = (kHasN && has_nmask) ? ((ncur >> (i & 31u)) & 1u) : 0u;
            // dna5 ranks A0 C1 G2 N3 T4; complement table [4,2,1,3,0]
            const uint32_t d_in = nf ? 3u : code + (code == 3u);
            const uint32_t cd_in = nf ? 3u : (3u - code) + (code == 0u);
            uint32_t d_out = 0, cd_out = 0;
            if (kSteady || i >= k) {
                const uint32_t oc = (uint32_t)(hist2 >> (2 * (k - 1))) & 3u;
                const uint32_t on = kHasN ? ((histn >> (k - 1)) & 1u) : 0u;
                d_out = on ? 3u : oc + (oc == 3u);
                cd_out = on ? 3u : (3u - oc) + (oc == 0u);
            }
            hist2 = (hist2 << 2) | code;
            if (kHasN) histn = (histn << 1) | nf;
            fwd = (fwd - (uint64_t)d_out * a.powk1) * 5u + d_in;
            rc = (rc - cd_out) * INV5 + (uint64_t)cd_in * a.powk1;
            if (have_value) {
                const uint32_t p = i + 1 - k;  // index of this canonical value (== blk + t)
                const uint64_t vf = fwd ^ a.seed, vr = rc ^ a.seed;
                const uint64_t v = vf < vr ? vf : vr;
                // running rightmost minimum of the current block's prefix [blk, p]
                if (t == 0 || v <= pv) { pv = v; pq = p; }
                if (!kSteady && p < wn) {  // first window: its rightmost minimum is the prefix minimum of block 0
                    mv = pv; q = pq;
                    emit = (p == wn - 1) && !cold;  // a cold piece's first window only sets (mv, q)
                } else if (q + wn == p) {  // tracked minimum left the window: rightmost minimum of the new one
                    mv = pv; q = pq;
                    if (t + 1 < wn) {
                        const uint64_t sw = ring[(t + 1) * WAVE + lane];
                        const uint64_t sv = PK ? (sw >> pbits) | seed_top : sw;
                        // (packed: the word holds wn - 1 - offset, the block before this one starts at blk - wn)
                        if (sv < pv) { mv = sv; q = PK ? blk - 1u - ((uint32_t)sw & omask) : blk - wn + spos[(t + 1) * WAVE + lane]; }
                    }
                    emit = true;
                } else if (v < mv) {
                    mv = v; q = p; emit = true;
                }
                ring[t * WAVE + lane] = PK ? (v << pbits) | (uint64_t)(wn - 1u - t) : v;
                // sequence shorter than one window: a single minimiser over all its values
                if (!kSteady && i + 1 == L && p + 1 < wn) emit = true;
            }
        }
        if (have_value) {
            if (t + 1 == wn) {
                // block end: turn the raw values of this block into rightmost suffix minima, in place
                uint64_t sv = ring[(wn - 1) * WAVE + lane];
                if (PK) {  // the words order by (value, rightmost first): a plain minimum chain
                    for (int u = (int)wn - 2; u >= 1; --u) {
                        const uint64_t x = ring[u * WAVE + lane];
                        sv = x < sv ? x : sv;
                        ring[u * WAVE + lane] = sv;
                    }
                } else {
                    uint32_t sp = wn - 1;
                    spos[(wn - 1) * WAVE + lane] = (uint8_t)sp;
#pragma unroll
                    for (int u = (int)wn - 2; u >= 1; --u) {
                        const uint64_t x = ring[u * WAVE + lane];
                        if (x < sv) { sv = x; sp = (uint32_t)u; }
                        ring[u * WAVE + lane] = sv;
                        spos[u * WAVE + lane] = (uint8_t)sp;
                    }
                }
                t = 0; blk += wn;
            } else {
                ++t;
            }
        }
        const uint64_t mask = __ballot(emit);
        if (mask) {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            if (emit) {
                const uint32_t pos = qwrap(qhead + qcount + rank);
                qv[pos] = mv;
                qm[pos] = own;
                ++my_emitted;
            }
            qcount += (uint32_t)__popcll(mask);
            if (qcount >= WAVE) probe_turn(WAVE);
        }
    };

    // The steady-state step again, hand-shaped for the hot path (no N mask in the batch, every lane past its first window, k <= 25):
    //  * digit * 5^(k-1) as one 32 x 32 -> 64 multiply-add plus a 24-bit multiply for the high word instead of two 64-bit
    //    multiply-adds, and x * 5 as a shift-add: 5 quarter-rate multiplies per base instead of 9;
    //  * the window update without divergent branches: the suffix minimum of the previous block is read every step (64 lanes
    //    expire at different times, so the wavefront took that path in 93 % of the steps anyway) and everything is selects;
    //  * at a block end (WN_T > 0) all raw values are read back first, the suffix minima are formed in registers and written out,
    //    instead of wn - 2 dependent LDS round trips.
    // Same arithmetic, same tie rule (SURVEY A.2): the parity tests cover both bodies.
    const uint32_t P_lo = (uint32_t)a.powk1, P_hi = (uint32_t)(a.powk1 >> 32);
    const bool fast_ok = P_hi < (1u << 22);  // wave-uniform: 4 * P_hi fits the 24-bit multiplier
    // (hipcc turns the plain C++ forms back into 64-bit multiply-adds, hence the two asm statements)
    auto mul_digit = [&](uint32_t d) -> uint64_t {  // d in 0..4
        uint32_t hi;
        asm("v_mul_u32_u24 %0, %1, %2" : "=v"(hi) : "v"(d), "s"(P_hi));
        return (uint64_t)d * P_lo + ((uint64_t)hi << 32);
    };
    auto times5 = [&](uint64_t x) -> uint64_t {
        uint64_t r;
        asm("v_lshl_add_u64 %0, %1, 2, %1" : "=v"(r) : "v"(x));
        return r;
    };
    auto step_fast = [&](const uint32_t i, const uint32_t j, const uint32_t cur) {
        // the previous block's suffix minimum at offset t + 1 (needed when the tracked minimum leaves the window)
        uint64_t sv = ~0ULL;
        uint32_t sq = 0;
        if (t + 1 < wn) {  // wave-uniform
            const uint64_t sw = ring[(t + 1) * WAVE + lane];
            sv = PK ? (sw >> pbits) | seed_top : sw;
            sq = PK ? blk - 1u - ((uint32_t)sw & omask) : blk - wn + spos[(t + 1) * WAVE + lane];
        }
        const uint32_t code = (cur >> (j * 2)) & 3u;
        const uint32_t oc = (uint32_t)(hist2 >> (2 * (k - 1))) & 3u;
        hist2 = (hist2 << 2) | code;
        // dna5 ranks A0 C1 G2 N3 T4; complement table [4,2,1,3,0]
        const uint32_t d_in = code + (code == 3u), cd_in = (3u - code) + (code == 0u);
        const uint32_t d_out = oc + (oc == 3u), cd_out = (3u - oc) + (oc == 0u);
        const uint64_t tf = fwd - mul_digit(d_out);
        fwd = times5(tf) + d_in;
        rc = (rc - cd_out) * INV5 + mul_digit(cd_in);
        const uint32_t p = i + 1 - k;  // index of this canonical value (== blk + t)
        const uint64_t vf = fwd ^ a.seed, vr = rc ^ a.seed;
        const uint64_t v = vf < vr ? vf : vr;
        const bool newpref = t == 0 || v <= pv;  // running rightmost minimum of the current block's prefix [blk, p]
        pv = newpref ? v : pv; pq = newpref ? p : pq;
        const bool expire = q + wn == p;         // the tracked minimum left the window: rightmost minimum of the new one
        const bool use_s = sv < pv;
        const uint64_t ev = use_s ? sv : pv;
        const uint32_t eq = use_s ? sq : pq;
        const bool less = v < mv;
        const bool emit = expire || less;
        mv = expire ? ev : (less ? v : mv);
        q = expire ? eq : (less ? p : q);
        ring[t * WAVE + lane] = PK ? (v << pbits) | (uint64_t)(wn - 1u - t) : v;
        if (t + 1 == wn) {
            // block end: turn the raw values of this block into rightmost suffix minima, in place
            if (WN_T > 1) {  // (always packed)
                uint64_t x[WN_T > 1 ? WN_T : 2];
#pragma unroll
                for (int u = 1; u < WN_T; ++u) x[u] = ring[u * WAVE + lane];
#pragma unroll
                for (int u = 1; u < WN_T; ++u) asm volatile("" : "+v"(x[u]));  // all reads issued and landed before the first store
                constexpr int LAST = WN_T > 1 ? WN_T - 1 : 1;
                uint64_t bsv = x[LAST];
#pragma unroll
                for (int u = WN_T - 2; u >= 1; --u) {
                    bsv = x[u] < bsv ? x[u] : bsv;
                    ring[u * WAVE + lane] = bsv;
                }
            } else if (PK) {
                uint64_t bsv = ring[(wn - 1) * WAVE + lane];
                for (int u = (int)wn - 2; u >= 1; --u) {
                    const uint64_t xx = ring[u * WAVE + lane];
                    bsv = xx < bsv ? xx : bsv;
                    ring[u * WAVE + lane] = bsv;
                }
            } else {
                uint64_t bsv = ring[(wn - 1) * WAVE + lane];
                uint32_t bsp = wn - 1;
                spos[(wn - 1) * WAVE + lane] = (uint8_t)bsp;
                for (int u = (int)wn - 2; u >= 1; --u) {
                    const uint64_t xx = ring[u * WAVE + lane];
                    if (xx < bsv) { bsv = xx; bsp = (uint32_t)u; }
                    ring[u * WAVE + lane] = bsv;
                    spos[u * WAVE + lane] = (uint8_t)bsp;
                }
            }
            t = 0; blk += wn;
        } else {
            ++t;
        }
        const uint64_t mask = __ballot(emit);
        if (mask) {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            if (emit) {
                const uint32_t pos = qwrap(qhead + qcount + rank);
                qv[pos] = mv;
                qm[pos] = own;
                ++my_emitted;
            }
            qcount += (uint32_t)__popcll(mask);
            if (qcount >= WAVE) probe_turn(WAVE);
        }
    };

    for (uint32_t s = 0; s < a.nseg; ++s) {
        L = s == 0 ? seg_len0 : seg_len1;
        const uint64_t off = s == 0 ? seg_off0 : seg_off1;
        const uint32_t maxL = wave_max_u32(L);
        const uint32_t minL = ~wave_max_u32(~L);  // lanes past the end of the batch have L = 0 and force the generic body
        const uint4 *bp = reinterpret_cast<const uint4 *>(a.bases + (off >> 4));   // 64 bases per uint4
        const uint2 *np = a.nmask ? reinterpret_cast<const uint2 *>(a.nmask + (off >> 5)) : nullptr;
        has_nmask = np != nullptr;
        fwd = 0; rc = 0; hist2 = 0; mv = 0; pv = 0; histn = 0; q = 0; pq = 0; t = 0; blk = 0;

        // Bases are prefetched one group of CHN_BASE_PIECES 64-base chunks ahead through asm loads (one dwordx4 per lane and chunk,
        // the pieces of a group issued back to back).  hipcc would guard their use with s_waitcnt vmcnt(0) at every group boundary
        // and thereby drain the probe round in flight; instead the kernel knows that any probe consume since the prefetch has
        // already waited for it (base_ready) and only waits when none happened.  Why groups: a lane walks its read 16 bytes at a
        // time, and between two chunks of the same 128-byte line the probe flood has turned the XCD's L2 over, so every chunk
        // load used to cost a full line fetch from HBM (PMC: 1 % L2 hits, 83 M extra requests per 1 M reads); a group fetches a
        // line's worth of chunks in one go (round 2 A/B: no base reads at all = +4 % gathers/s, so this is the ceiling of the gain).
        constexpr uint32_t NP = CHN_BASE_PIECES;
        const uint32_t nchunk = (maxL + 63) >> 6;
        u32x4_t wnext[NP];
        u32x2_t nnext[NP];
#pragma unroll
        for (uint32_t p = 0; p < NP; ++p) { wnext[p] = u32x4_t{0u, 0u, 0u, 0u}; nnext[p] = u32x2_t{0u, 0u}; }
        auto prefetch = [&](uint32_t grp) {
#ifndef CHN_DIAG_NO_BASE  // DIAGNOSTICS BUILD ONLY (with CHN_K1_FAKE_EMIT): no base reads at all
#pragma unroll
            for (uint32_t p = 0; p < NP; ++p) {
                const uint32_t c = grp * NP + p;
                if (c * 64 < L) { wnext[p] = asm_load_b128(bp + c); if (np) nnext[p] = asm_load_b64(np + c); }
            }
#endif
        };
        prefetch(0);
        base_ready = false; base_seq = r_issued;
        for (uint32_t c = 0; c < nchunk; ++c) {
            const uint32_t piece = c % NP;  // wave-uniform
            if (piece == 0) {
                if (!base_ready || (a.ablate & 4u)) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); base_ready = true; }  // bit 2: A/B diagnostic
            }
            uint4 wcur = make_uint4(0u, 0u, 0u, 0u);
            uint2 ncur2 = make_uint2(0u, 0u);
#pragma unroll
            for (uint32_t p = 0; p < NP; ++p) {
                asm volatile("" : "+v"(wnext[p]), "+v"(nnext[p]));  // the values are read only after the wait above
                if (piece == p) { wcur = make_uint4(wnext[p].x, wnext[p].y, wnext[p].z, wnext[p].w); ncur2 = make_uint2(nnext[p].x, nnext[p].y); }
            }
            // the last piece of the group has just been copied out: fetch the next group (one chunk = ~6 probe rounds ahead of its use)
            if (piece == NP - 1 && c + 1 < nchunk) { prefetch((c + 1) / NP); base_ready = false; base_seq = r_issued; }
            for (uint32_t dd = 0; dd < 4; ++dd) {
                const uint32_t cur = dd == 0 ? wcur.x : dd == 1 ? wcur.y : dd == 2 ? wcur.z : wcur.w;
                const uint32_t ncur = dd < 2 ? ncur2.x : ncur2.y;
                const uint32_t ibase = c * 64 + dd * 16;
                if (ibase >= maxL) break;
                const uint32_t jn = maxL - ibase < 16 ? maxL - ibase : 16;
                // Steady-state dword: every lane still has all 16 bases, and all of them lie past the warm-up and the first
                // window, so the specialised body drops the activity predicate and the start-up / short-read cases.
                const bool steady = ibase >= k + wn && ibase + 16 <= minL;
#if !defined(CHN_K1_FAKE_EMIT) && !defined(CHN_K1_NO_FAST_STEP)
                if (steady && !np && fast_ok) {
                    for (uint32_t j = 0; j < 16; ++j) step_fast(ibase + j, j, cur);
                } else
#endif
                if (steady && !np) {
                    for (uint32_t j = 0; j < 16; ++j) step(std::true_type(), std::false_type(), ibase + j, j, cur, ncur);
                } else if (steady) {
                    for (uint32_t j = 0; j < 16; ++j) step(std::true_type(), std::true_type(), ibase + j, j, cur, ncur);
                } else {
                    for (uint32_t j = 0; j < jn; ++j) step(std::false_type(), std::true_type(), ibase + j, j, cur, ncur);
                }
            }
        }
    }
    if (COND) {  // drain: what is queued goes out (in rounds of at most 64), what is in flight is retired and may queue survivors again
        while (qcount || r_retired < r_issued) {
            if (qcount && r_issued - r_retired < FUSED_ROUNDS) cprobe_issue(qcount < WAVE ? qcount : WAVE);
            else cprobe_retire();
        }
    } else {
        if (qcount) probe_turn(qcount);
        while (r_retired < r_issued) probe_retire();
    }
    if (MODE == MODE_ROWS && CHN_LOG_BATCH > 1 && !overflow && staged) log_flush(flushed, staged);  // the entries staged since the last full store

    __syncthreads();
    if ((MODE == MODE_ROWS || MODE == MODE_FUSED) && a.fetches && lane == 0 && n_fetch) atomicAdd(a.fetches, (unsigned long long)n_fetch);
    if ((MODE == MODE_ROWS || MODE == MODE_LIST) && lane == 0) {
        a.wave_count[wslot] = overflow ? 0u : consumed;  // an overflowed log is never read: the batch is re-run
        if (overflow) atomicOr(a.status, 1u);
    }
    if (SPLIT) {
        uint32_t tot_emitted = my_emitted;
        for (int o = 32; o > 0; o >>= 1) tot_emitted += (uint32_t)__shfl_xor((int)tot_emitted, o);
        my_emitted = tot_emitted;
    }
    if (valid && MODE != MODE_EMPLACE && (!SPLIT || lane == 0)) {
        a.num_hashes[r] = my_emitted;
        if (MODE == MODE_FUSED) {
            for (uint32_t c = 0; c < a.C; ++c) {
                a.counts[(size_t)r * a.C + c] = cnt[c * WAVE + lane];
                a.unique[(size_t)r * a.C + c] = unq[c * WAVE + lane];
            }
        }
    }
    if (SPLIT) __syncthreads();  // the next read of this workgroup re-uses the LDS
    item += gridDim.x;
    } while (SPLIT && item < n_long);
}
