/* charon_hip.h -- C ABI of libcharon_hip.so: the MI355X (gfx950) implementation of the per-read
 * classification path of `charon dehost`.
 *
 * The reference (rmcolq/charon) has no FFI/plugin interface; the seam this library replaces is the body
 * of the OpenMP loop in src/dehost_main.cpp:366-373 (single-end) / :456-468 (paired) plus the model
 * application and call that Result::classify_read performs on each entry (include/result.hpp:97-116 ->
 * include/read_entry.hpp:218-291).  Each entry point below cites the reference code it stands in for.
 * All paths are relative to the reference checkout.
 *
 * Conventions: every function returns 0 on success or a negative CHN_E_* code; chn_last_error() returns a
 * thread-local message owned by the library.  No C++ types, exceptions or torch types cross this boundary.
 * All sizes are 64-bit.  The library never writes to stdout/stderr.  A chn_stream is NOT thread-safe;
 * different streams may be driven from different host threads (a front end drives one index replica and its stream per thread).
 */
#ifndef CHARON_HIP_H
#define CHARON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHN_OK 0
#define CHN_E_INVALID (-1)   /* bad argument / unsupported parameter combination */
#define CHN_E_HIP (-2)       /* a HIP runtime call failed (message has the HIP error string) */
#define CHN_E_NOMEM (-3)     /* device or host allocation failed */
#define CHN_E_STATE (-4)     /* call sequence error (e.g. wait without submit) */
#define CHN_E_CAPACITY (-5)  /* batch exceeds the stream's configured capacity */

#define CHN_MAX_CATEGORIES 255
#define CHN_NO_CALL 255u

typedef struct chn_index chn_index;   /* immutable IBF resident in HBM */
typedef struct chn_stream chn_stream; /* one HIP stream + its device scratch */

/* ---- index ------------------------------------------------------------------------------------------
 * Replaces: Index (include/index.hpp:19-138) as far as the hot path reads it -- window_size()/kmer_size()
 * (:52-58), the IBF parameters and data (:26, seqan3::interleaved_bloom_filter<compressed>), the bin ->
 * category map (include/input_summary.hpp:20,39-45) and get_host_index() (include/index.hpp:72-80).
 * Device layout: plain interleaved 64-bit words, word (row * bin_words + b) holds technical bins
 * 64b..64b+63 of row `row` -- the same addressing seqan3 uses (bit index row * technical_bins + bin), with
 * the Elias-Fano (sdsl::sd_vector) compression undone once at load time. */
typedef struct chn_index_desc {
    uint32_t struct_size;      /* sizeof(chn_index_desc) */
    int32_t device;            /* HIP device ordinal */
    uint8_t kmer_size;         /* k  (1..27: 5^k must fit 64 bits, as in seqan3 for dna5) */
    uint8_t window_size;       /* w >= k */
    uint8_t hash_funs;         /* h in 1..5 */
    uint8_t num_categories;    /* C */
    uint8_t host_index;        /* InputSummary::host_category_index(); 255 if none */
    uint8_t reserved0[3];
    uint64_t minimiser_seed;   /* 0x8F3F73B5CF1C9ADE for seqan3::views::minimiser_hash defaults */
    uint64_t bins;             /* B  = InputSummary::num_bins */
    uint64_t technical_bins;   /* TB = 64 * ceil(B/64) */
    uint64_t bin_size;         /* S  = rows */
    uint64_t hash_shift;       /* countl_zero(S) */
    uint64_t bin_words;        /* W  = TB / 64 (1..4) */
    uint8_t bin_to_category[256]; /* category INDEX of each user bin */
    uint64_t row_begin;        /* shard: this object holds rows [row_begin, row_end); 0,0 = all rows */
    uint64_t row_end;
} chn_index_desc;

int chn_index_create(const chn_index_desc *desc, chn_index **out);
/* Copy `n_rows` rows (n_rows * bin_words words) starting at global row `row_begin` from HOST memory.
 * Replaces the archive(ibf_) step of Index::serialize (include/index.hpp:130) after EF decoding; the
 * loader streams row blocks so host RAM never holds the whole plain index. */
int chn_index_upload_rows(chn_index *idx, uint64_t row_begin, uint64_t n_rows, const uint64_t *host_words);
/* Elias-Fano (sdsl::sd_vector) decode ON THE DEVICE: the alternative to chn_index_upload_rows for the loader, replacing the
 * archive(ibf_) step of Index::serialize (include/index.hpp:130) for the compressed IBF the file really holds.
 * `high` is a slice of m_high starting at bit `high_bit0` (a multiple of 64) with `n_high_words` words; `ones_before` = number of
 * set bits of m_high before that slice (the caller keeps the running popcount); `low` holds the packed m_low elements starting
 * with element `low_elem0` <= ones_before, `n_low_words` words (the last partial word included).  Every one of the slice is turned
 * into its plain bit position ((zeros before it) << wl | low part) and set in the index words; positions outside this shard's
 * rows are skipped.
 * The slice's work is QUEUED: the call returns as soon as `high` and `low` have been read (page-locked memory: chn_host_alloc; the copy
 * of pageable memory is what it waits for otherwise), so the caller prepares the next slice while the device decodes this one.
 * A closing call with n_high_words == 0 waits for every slice in flight and sets *bad_bits to the number of positions >= m_size or in
 * technical bins >= bins that the slices met (must be 0 for a well-formed file); calls with a slice set *bad_bits to 0.
 * chn_index_bin_popcounts and chn_stream_create wait for the slices as well. */
int chn_index_decode_ef(chn_index *idx, uint64_t m_size, uint32_t wl, const uint64_t *high, uint64_t high_bit0, uint64_t n_high_words,
                        uint64_t ones_before, const uint64_t *low, uint64_t low_elem0, uint64_t n_low_words, uint64_t *bad_bits);
/* Elias-Fano (sdsl::sd_vector) ENCODE: the inverse of chn_index_decode_ef for the writer, replacing the compression of the IBF in
 * Index(...) (include/index.hpp:43-50) whose result archive(ibf_) stores (include/index.hpp:130, store_index.hpp:12-17).
 * The layout of a vector of m_size bits with `ones` set bits, with hi(x) = floor(log2 x) and hi(0) = 0: logm = hi(ones) + 1,
 * logn = hi(m_size) + 1, logm one less where the two are equal; wl = logn - logm >= 1; low_bits = ones * wl; high_bits = ones + 2^logm;
 * the word counts round up.  ones == 0 is legal (wl from logm = 1, no low words, two high bits).  The set bit of rank k at plain position
 * pos = row * technical_bins + bin puts its low wl bits at bit k * wl of m_low and sets bit (pos >> wl) + k of m_high.
 * chn_ef_layout_of is that rule alone and needs no GPU: CHN_E_INVALID for a null `out`, m_size == 0 or above 2^57, ones > m_size. */
typedef struct chn_ef_layout {
    uint32_t struct_size, wl;                 /* struct_size: set by the calls that fill the layout */
    uint64_t m_size, ones;
    uint64_t low_bits, high_bits;
    uint64_t n_low_words, n_high_words;
} chn_ef_layout;
int chn_ef_layout_of(uint64_t m_size, uint64_t ones, chn_ef_layout *out);
/* The layout of this index: its set bits are counted on the device, m_size = technical_bins * bin_size (include/index.hpp:43-50,130;
 * store_index.hpp:12-17).  Waits for queued Elias-Fano slices and a queued replica copy; a row shard is refused with CHN_E_INVALID. */
int chn_index_ef_layout(chn_index *idx, chn_ef_layout *out);
/* m_low and m_high of the whole index into HOST memory (include/index.hpp:43-50,130; store_index.hpp:12-17: the two int_vectors the file
 * holds).  Synchronous.  The call owns both arrays: every word of low[0, n_low_words) and high[0, n_high_words) is written, zeros included.
 * The index is worked through in slices of `slice_rows` rows (0: 256 MiB of rows): a slice's set bits are counted, the words of m_low and
 * m_high they can touch follow from the set bits in front of the slice and from its first and last position, device scratch of that size
 * is zeroed, k_ef_encode fills it, and the host ORs the downloaded ranges into the arrays (neighbouring slices share the words at their
 * seams).  The scratch is bounded by the slice, not by the index.
 * CHN_E_INVALID, nothing having been written: a null job, a wrong struct_size (job or layout), a non-zero flag, a null layout or array, a
 * layout that is not the one of this index's m_size and of its own `ones`, array sizes that are not the layout's, a slice of more than
 * 2^31 words, a row shard, set bits in the index that number other than layout->ones (counted before anything is written).
 * ones_written is the number of set bits encoded; device_ms the time of the kernels, from events, summed over the slices.
 * Waits for queued Elias-Fano slices and a queued replica copy.
 * chn_index_encode_ef_host is the same rule source on the calling thread over plain words in host memory (rows of `desc`, which must
 * describe a whole index): the same checks, the same slices and seams; device_ms is 0. */
typedef struct chn_ef_encode_job {
    uint32_t struct_size, flags;              /* flags: 0 */
    uint64_t slice_rows;                      /* 0: 256 MiB of rows */
    const chn_ef_layout *layout;
    uint64_t *low;  uint64_t n_low_words;     /* HOST; must equal the layout's */
    uint64_t *high; uint64_t n_high_words;    /* HOST */
    uint64_t ones_written;                    /* out */
    double device_ms;                         /* out */
} chn_ef_encode_job;
int chn_index_encode_ef(chn_index *idx, chn_ef_encode_job *job);
int chn_index_encode_ef_host(const chn_index_desc *desc, const uint64_t *host_words, chn_ef_encode_job *job);   /* one CPU thread; no GPU needed */
/* set bits per technical bin over the rows this object holds (loader self-check iv); out[technical_bins] */
int chn_index_bin_popcounts(chn_index *idx, uint64_t *out);
/* Device pointer to the shard's words (for on-device index fabrication and for download in tests). */
int chn_index_device_words(chn_index *idx, uint64_t **device_words, uint64_t *n_words);
int chn_index_download_rows(chn_index *idx, uint64_t row_begin, uint64_t n_rows, uint64_t *host_words);
int chn_index_get_desc(const chn_index *idx, chn_index_desc *out);
int chn_index_destroy(chn_index *idx);
/* An independent copy of `src` on HIP device `device` (the same device as src's or another one): same descriptor except `device`, a
 * row shard included.  The call waits on the host for src's queued Elias-Fano slices, checks that `device` is a valid ordinal
 * (CHN_E_INVALID otherwise) and that the words fit in its free memory (CHN_E_NOMEM, the message names the device, the bytes needed
 * and the bytes free), allocates the words and QUEUES one hipMemcpyPeerAsync on the replica's own stream; peer access is not
 * enabled and no device setting is changed.  Like chn_index_decode_ef it returns as soon as the copy is queued: the replica's
 * chn_stream_create, chn_index_bin_popcounts, chn_index_download_rows, chn_index_upload_rows, chn_index_emplace and
 * chn_index_destroy wait for it.  `src` must not be destroyed or written until one of those calls on the replica has returned.
 * No reference counterpart (the reference is single-process and runs one index): one index replica per device, each fed its own
 * batches of reads, is the "device list" part of SURVEY 8(b).3. */
int chn_index_replicate(const chn_index *src, int32_t device, chn_index **out);
/* Number of HIP devices visible to the process (hipGetDeviceCount). */
int chn_device_count(int *count);

/* ---- model --------------------------------------------------------------------------------------------
 * Replaces: StatsModel + Model + KDEParams as read by ReadEntry::apply_model / call_host / call_category
 * (include/classify_stats.hpp:210-254,370-389,395-519; include/read_entry.hpp:157-279).
 * `paired` selects the caller: 0 = call_host (single-end dehost), 1 = call_category (paired dehost and every
 * `charon classify` run, include/read_entry.hpp:281-285). */
typedef struct chn_model {
    uint32_t struct_size;
    uint32_t num_categories;
    /* per category c: KDE datasets IN THE ORDER THE REFERENCE ITERATES THEM (default tables sorted by the
     * KDEParams constructor :214-218; trained tables in insertion order :234-240) */
    const float *const *pos_data; /* [C] host pointers */
    const uint32_t *pos_n;        /* [C] */
    const float *const *neg_data;
    const uint32_t *neg_n;
    float h_pos;                  /* 0.1   (:270) */
    float h_neg;                  /* 0.001 (:271) */
    float err_rate;               /* 300: stats::dexp(x, 300) (:371) */
    /* thresholds (include/dehost_arguments.hpp:30-37) */
    float min_quality;
    uint32_t min_length;
    float min_compression;
    int8_t confidence_threshold;  /* already narrowed to int8 (include/classify_stats.hpp:404,497) */
    uint8_t min_hits;             /* StatsModel::min_hits_ -- never initialised in the reference; caller's choice */
    uint8_t paired;               /* 1: call_category (what paired dehost runs, src/dehost_main.cpp:470) */
    uint8_t host_index;
    float confidence_probability_threshold;
    float host_unique_prop_lo_threshold;
    float min_proportion_difference;
    float min_prob_difference;
    /* Parametric models (`charon classify`, `charon dehost --dist gamma|beta`; include/classify_stats.hpp:116-208,289-339,
     * 377-381).  dist == CHN_DIST_KDE: the KDE datasets above are used and the two pointers are ignored.  Otherwise per
     * category three floats for the pos and three for the neg distribution: gamma (shape, loc, scale) -- reference defaults
     * pos {25, 0, 0.02}, neg {10, 0, 0.005} (:265-266) -- or beta (alpha, beta, unused) -- defaults pos {6, 4}, neg {6, 40}
     * (:267-268); the KDE datasets may then be NULL / empty. */
    uint32_t dist;
    const float *pos_params;      /* [C][3] */
    const float *neg_params;      /* [C][3] */
} chn_model;
#define CHN_DIST_KDE 0u
#define CHN_DIST_GAMMA 1u
#define CHN_DIST_BETA 2u

/* Fill `m` with the reference defaults (default KDE tables of src/dehost_main.cpp:23-206, sorted; thresholds
 * of include/dehost_arguments.hpp).  Pointers refer to static storage inside the library. */
int chn_model_default(chn_model *m, uint32_t num_categories, uint8_t host_index, int paired);

/* ---- streams and batches --------------------------------------------------------------------------------
 * One batch = what the reference calls a chunk (src/dehost_main.cpp:335-339), but sized for the GPU
 * (>= 64k reads rather than <= 255). */
typedef struct chn_stream_cfg {
    uint32_t struct_size;
    uint32_t flags;             /* CHN_STREAM_* */
    uint64_t max_reads;         /* per batch */
    uint64_t max_bases;         /* per batch, sum of padded segment lengths */
} chn_stream_cfg;
#define CHN_STREAM_PROFILE 1u   /* bracket every kernel with HIP events (chn_stream_profile) */
#define CHN_STREAM_TINY_LOG 2u  /* testing only: start with a deliberately undersized row log so that every batch takes the
                                 * overflow -> worst-case re-run path of chn_batch_wait */
#define CHN_STREAM_NO_PROBE_GATE 4u /* testing only: never hold a batch's minimise+probe launch back until its predecessor has
                                     * dispatched its last workgroup (the probe gate); consecutive batches' probe kernels then share
                                     * the device from their first workgroup on, as they also do on a device without stream-wait-value
                                     * support */
/* A single-end read of 32 768 bases or more is rolled by the 64 lanes of one wavefront at once, in pieces that overlap by w - 1
 * bases (exact: a piece starts only where the window minimum is unique); shorter reads take one lane each.  Testing only:
 * CHN_STREAM_SPLIT_BUCKET(b) moves that limit to length class b (8 classes per octave: class = 8 (floor(log2 L) - 2) + the three
 * bits below L's leading one; 64 = 1 024 bases, the smallest accepted; 104 = the default; 255 = never split). */
#define CHN_STREAM_SPLIT_BUCKET(b) (((uint32_t)(b) & 0xffu) << 8)

int chn_stream_create(chn_index *idx, const chn_stream_cfg *cfg, chn_stream **out);
int chn_stream_destroy(chn_stream *s);
int chn_model_set(chn_stream *s, const chn_model *m);

/* Input batch.  Bases are 2-bit codes A0 C1 G2 T3, 4 per byte, least-significant bits first; base j of the
 * batch is bits [2*(j%16), +2) of little-endian dword j/16.  `nmask` (optional) has one bit per base in the
 * same order (bit j%32 of dword j/32): 1 = the base is N (any non-ACGT IUPAC letter, seqan3 dna5 rank 3);
 * its 2-bit code is then ignored.  Every segment must start at a multiple of 64 bases.
 * A read has one segment (single-end) or two (paired: mates are minimised separately and share one
 * accumulator, src/dehost_main.cpp:458-465).  mean_quality / compression are the host-side columns of
 * src/dehost_main.cpp:355-363 that gate the call (include/read_entry.hpp:242-252); NULL = 0.
 * If `on_device` is non-zero every pointer is a device pointer valid on the stream's device and no copy is
 * made (the caller keeps them alive until chn_batch_wait returns). */
typedef struct chn_batch {
    uint32_t struct_size;
    uint32_t on_device;
    uint64_t n_reads;
    uint64_t n_bases;            /* extent of `bases2`/`nmask` in bases (multiple of 64) */
    const uint32_t *bases2;
    const uint32_t *nmask;       /* may be NULL */
    const uint64_t *seg1_offset; /* [n] in bases */
    const uint32_t *seg1_length; /* [n] */
    const uint64_t *seg2_offset; /* [n] or NULL (single-end) */
    const uint32_t *seg2_length; /* [n] or NULL */
    const float *mean_quality;   /* [n] or NULL */
    const float *compression;    /* [n] or NULL */
    /* Deflate tallies for the `compression` column (get_compression_ratio, src/utils.cpp:114-124) ON THE DEVICE: non-zero = the
     * longest read (both mates together) to handle there, at most CHN_GZIP_MAX_LEN (any length with CHN_GZIP_SIZES_ALL).  For every read the library then runs zlib's
     * level-6 deflate_slow as a kernel and returns the literal/length and distance code frequencies of its deflate block
     * (chn_result.gzip_tallies) -- the caller turns them into the exact gzip size with _tr_flush_block's arithmetic (a few
     * microseconds per read; charon_amd/csrc/host/gzip_size.hpp).  With tallies requested `compression` is not known when the
     * call kernel runs: its `compression < min_compression` gate (include/read_entry.hpp:189-191,250-252) is left open and the
     * CALLER must apply it (call = CHN_NO_CALL where the ratio is below the threshold). */
    uint32_t gzip_tallies;
    /* What comes back for the reads tallied on the device: CHN_GZIP_TALLIES (0) the tallies; CHN_GZIP_SIZES the gzip member
     * SIZES (chn_result.gzip_sizes) -- _tr_flush_block's tree arithmetic then runs on the device too (k_gzip_size) and only
     * four bytes per read are downloaded; CHN_GZIP_BOTH both.
     * CHN_GZIP_SIZES_ALL: the SIZE of EVERY read of 1 .. gzip_tallies letters (both mates together), whatever its length and
     * however many deflate blocks zlib writes for it (host batches; a device-resident batch is refused with CHN_E_INVALID for now); gzip_tallies may exceed CHN_GZIP_MAX_LEN
     * there (CHN_GZIP_ANY_LEN: no bound).  Reads beyond CHN_GZIP_MAX_LEN, and reads the tallies hand back for a second deflate
     * block, run through a deflate pass with zlib's window slide and block flushes (k_gzip_long, one wavefront per read, longest
     * first on a stream of its own); a size of 0 then only means "longer than gzip_tallies" (or an empty read).  Tallies cannot
     * describe a read of several blocks: this mode returns sizes only.  Its scratch (some 256 KiB per wavefront the device holds
     * at once) is allocated with the first such batch; CHN_E_NOMEM if it does not fit. */
    uint32_t gzip_output;
} chn_batch;
#define CHN_GZIP_TALLIES 0u
#define CHN_GZIP_SIZES 1u
#define CHN_GZIP_BOTH 2u
#define CHN_GZIP_SIZES_ALL 3u
#define CHN_GZIP_ANY_LEN 0xFFFFFFFFu  /* chn_batch.gzip_tallies under CHN_GZIP_SIZES_ALL: no length bound */
#define CHN_GZIP_MAX_LEN 61440u  /* one wavefront holds the whole read in LDS; short reads run many wavefronts per CU, a 60 kb read one */
#define CHN_GZIP_TALLY_WORDS 320u /* per read: [0,286) literal/length code frequencies, [286,316) distance code frequencies,
                                   * [316] status: 0 = tallies valid, non-zero = not handled on the device (longer than asked for,
                                   * more than one deflate block): size this read on the host.
                                   * Long reads run few wavefronts per CU (one beyond 31 k letters): a caller with many idle host threads may prefer to keep
                                   * reads beyond ~16 k letters for itself (gzip_tallies = 16384) */

/* Per-read results (what a post-processed + classified ReadEntry holds, include/read_entry.hpp:23-32):
 * num_hashes_, counts_[C], unique_counts_[C], probabilities_[C], call_, confidence_score_.
 * proportions are not returned: they are float(count)/float(num_hashes) (:140-150), recomputed by the caller.
 * `flags` bit 0: a probability comparison that decides `call` was closer than 2e-6 relative (or a probability sits at the
 * float underflow edge of the `prob == 0` test of call_category), so the host should re-evaluate that read with its own
 * libm (the device exp() may differ from glibc in the last ulp; 2e-4 for gamma / beta models, whose densities the device forms from a
 * double log-density while the reference evaluates them in float: device-resident probabilities then agree to ~1e-5 only).
 * chn_batch_wait does that itself for host batches with host result buffers -- for gamma / beta it re-evaluates every read in float --;
 * with on_device results the flags are only reported and NOTHING is re-evaluated: a caller that needs the reference's `call` on
 * flagged reads runs chn_classify_counts on their counts (which leaves the device-resident results in place). */
typedef struct chn_result {
    uint32_t struct_size;
    uint32_t on_device;        /* 0: pointers below are host buffers to fill; 1: receive device pointers */
    uint32_t *num_hashes;      /* [n] */
    uint32_t *counts;          /* [n*C] */
    uint32_t *unique_counts;   /* [n*C] */
    double *probabilities;     /* [n*C] */
    uint8_t *call;             /* [n] (CHN_NO_CALL = unclassified) */
    uint8_t *confidence;       /* [n] */
    uint8_t *flags;            /* [n] */
    uint16_t *gzip_tallies;    /* [n][CHN_GZIP_TALLY_WORDS] when the batch asked for them (may be NULL otherwise) */
    uint32_t *gzip_sizes;      /* [n] bytes of the gzip member (get_compression_ratio's numerator) when the batch asked for sizes;
                                * 0 = not handled on the device (too long, more than one deflate block): size it on the host
                                * (CHN_GZIP_SIZES_ALL: 0 only for reads longer than gzip_tallies) */
} chn_result;

/* Up to THREE batches may be in flight per stream.  Two (submit, submit, wait, submit, wait, ...) let batch i's count and
 * model+call kernels run on a side HIP stream under batch i+1's minimise+probe kernel; they then usually finish only when
 * that kernel does, so a caller with HOST buffers keeps three in flight (submit i+2 before waiting for i): the upload of batch
 * i+2 then runs under the probe kernel of batch i+1.  chn_batch_wait returns the OLDEST batch in flight.  With on_device
 * results the returned pointers stay valid until the third-next submit.  Host results are downloaded in stream into
 * page-locked staging right behind the kernels that produce them; chn_batch_wait copies from there.
 * Scratch: the per-batch row log is sized for twice the minimiser density of random sequence (not for the worst case
 * of one minimiser per base); a batch that overruns it is detected on the device and re-run by chn_batch_wait on
 * worst-case buffers allocated at that point (CHN_E_NOMEM if they do not fit) -- results are identical either way.
 * A device batch (on_device != 0) whose segments are misaligned or reach beyond n_bases makes chn_batch_wait fail with
 * CHN_E_INVALID (such segments are never read). */
int chn_batch_submit(chn_stream *s, const chn_batch *b);   /* asynchronous */
int chn_batch_wait(chn_stream *s, chn_result *r);          /* blocks; fills / points `r` */
int chn_stream_sync(chn_stream *s);

/* ---- text batches: reads as they stand in the caller's input buffer ---------------------------------------
 * Replaces, together with chn_batch_submit, the whole per-read body of src/dehost_main.cpp:344-373 / :430-468 including the
 * mean-quality loop (:355-360): the caller hands over `record.sequence()` as one byte per base and the phred characters, as
 * (offset, length) pairs into ONE host buffer (e.g. the decoded FASTQ block itself -- ids and `+` lines may lie between the
 * stretches), and k_text_pack forms the packed batch in device memory: 2-bit codes, N mask, 64-base-aligned segments (read
 * i's mate 1 at `cur`, cur += pad64(len1), then mate 2; n_bases = max(cur, 64)) and the mean quality -- bit for bit what a host
 * packer that follows the chn_batch rules writes.
 * Letters: A a -> 0, C c -> 1, G g -> 2, T t U u -> 3; N R Y S W K M B D H V in either case -> N (mask bit set, code bits 0);
 * any other byte is ILLEGAL.  With CHN_TEXT_DNA5_RANKS the bytes are seqan3 dna5 ranks instead (what std::vector<seqan3::dna5>
 * holds): 0 A, 1 C, 2 G, 3 N, 4 T; a byte above 4 is illegal.
 * Mean quality of a read: int sum of (signed char)q - 33 over the quality bytes of both mates / their number, one float
 * division, 0.0f where there are none (and for a read without any letter).  A quality string may be longer than its sequence
 * (the reference's reader allows it); every byte of it counts.
 * Every descriptor is checked on the host: offset + length <= text_bytes, else CHN_E_INVALID and nothing is launched.
 * CHN_TEXT_ON_DEVICE: `text` is DEVICE memory on the stream's device under the device text contract -- 16-byte aligned, and the
 * allocation readable up to text_bytes rounded up to 16; every chn_device_malloc result whose size is rounded up to 16 qualifies
 * (e.g. the `out` of a chn_inflate_run with CHN_INFLATE_OUT_DEVICE).  Nothing is staged or uploaded: k_text_pack reads the caller's
 * buffer (only aligned dwords that hold a wanted byte).  The descriptor arrays stay HOST arrays and are checked as above; layout,
 * verdict, chain and results are those of the same bytes in host memory.  A pointer that is not device memory of that device
 * (page-locked or pageable host memory, another device) or is misaligned is CHN_E_INVALID before anything is launched, and the
 * stream stays usable.  The buffer may be reused as soon as the call returns.  Combines with CHN_TEXT_DNA5_RANKS.
 * TWO TEXTS (the two files of paired input, each inflated into a device buffer of its own): chn_text_batch2 is a chn_text_batch with
 * `text2` and `text2_bytes` appended, and the calls below take either -- struct_size says which.  With text2 != NULL mate 1 stays in
 * `text` and seq2_offset / qual2_offset are bytes into `text2`, a second device buffer under the same contract, checked in the same
 * way before anything is launched; every mate-2 stretch is range-checked against text2_bytes.  Layout, verdict, chain and results are
 * those of the same bytes in one text.  CHN_E_INVALID before any launch, the stream staying usable: text2 without
 * CHN_TEXT_ON_DEVICE, text2 without seq2_*, text2 that is not device memory of the stream's device or is misaligned, a mate-2 stretch
 * beyond text2_bytes.  text2 == NULL is a batch with one text (text2_bytes is not looked at).
 * struct_size: sizeof(chn_text_batch) (== offsetof(chn_text_batch2, text2)) means "no text2" and nothing behind gzip_output is read,
 * so a caller built before text2 existed keeps working; sizeof(chn_text_batch2) is the form with text2.  Any other value is
 * CHN_E_INVALID. */
#define CHN_TEXT_DNA5_RANKS 1u
#define CHN_TEXT_ON_DEVICE 2u
typedef struct chn_text_batch {
    uint32_t struct_size;
    uint32_t flags;               /* CHN_TEXT_DNA5_RANKS | CHN_TEXT_ON_DEVICE */
    uint64_t n_reads;
    const uint8_t *text;          /* HOST memory; page-locked memory (chn_host_alloc) is uploaded asynchronously (CHN_TEXT_ON_DEVICE: DEVICE) */
    uint64_t text_bytes;
    const uint64_t *seq1_offset;  /* [n] bytes into `text` */
    const uint32_t *seq1_length;  /* [n] */
    const uint64_t *qual1_offset; /* [n], or NULL together with qual1_length (FASTA: mean quality 0) */
    const uint32_t *qual1_length; /* [n]; may exceed seq1_length */
    const uint64_t *seq2_offset;  /* [n] or NULL together with seq2_length (single-end) */
    const uint32_t *seq2_length;
    const uint64_t *qual2_offset; /* [n] or NULL together with qual2_length; needs seq2_* */
    const uint32_t *qual2_length;
    const float *compression;     /* [n] or NULL, as chn_batch.compression */
    uint32_t gzip_tallies;        /* as chn_batch.gzip_tallies */
    uint32_t gzip_output;         /* as chn_batch.gzip_output */
} chn_text_batch;
/* the batch with a second text behind it (TWO TEXTS above): hand &t.batch to chn_text_submit / chn_text_pack with
 * t.batch.struct_size = sizeof(chn_text_batch2) */
typedef struct chn_text_batch2 {
    chn_text_batch batch;
    const uint8_t *text2;         /* NULL, or DEVICE memory that holds mate 2 (needs CHN_TEXT_ON_DEVICE and seq2_*) */
    uint64_t text2_bytes;
} chn_text_batch2;
typedef struct chn_text_result {
    uint32_t struct_size;
    uint32_t has_n;               /* out: 1 if any base of the batch is N */
    uint64_t n_bases;             /* out: extent of the packed batch (multiple of 64) */
    float *mean_quality;          /* [n] HOST buffer to fill, or NULL */
} chn_text_result;
/* chn_text_submit takes a slot exactly like chn_batch_submit (three batches in flight, text and packed batches freely mixed;
 * chn_batch_wait and chn_text_wait both return the OLDEST batch).  It lays the segments out, checks the capacity of the stream
 * (CHN_E_CAPACITY), uploads text and descriptors on the stream's copy stream, runs k_text_pack behind them and WAITS for that
 * kernel's verdict -- does the batch hold an N, does it hold an illegal byte -- before it queues the chain: the chain's kernels
 * are picked on the host by whether the batch has an N mask.  A batch without N then runs exactly the launches of
 * chn_batch_submit with nmask = NULL, so every result column equals that of the host-packed batch.  The wait covers one upload
 * and one streaming kernel while the device keeps working on the batches in flight.  Consequences:
 *   - `text` and the descriptor arrays may be reused as soon as chn_text_submit returns;
 *   - an illegal byte makes chn_text_submit ITSELF return CHN_E_INVALID (the message names the smallest read index that holds
 *     one and the number of such bytes); nothing is queued, no slot is taken and the stream stays usable.
 * The device text staging (per slot, text_bytes + padding, grow-only) is allocated with the first text batch (CHN_E_NOMEM if it
 * does not fit); a process that never submits text allocates nothing for it.  The mean quality is downloaded into page-locked
 * staging for the host re-evaluation of borderline reads that chn_batch_wait does.
 * chn_text_wait = chn_batch_wait + the text columns; CHN_E_STATE (nothing consumed) if the oldest batch is not a text batch.
 * chn_batch_wait on a text batch works and simply drops the text columns. */
int chn_text_submit(chn_stream *s, const chn_text_batch *t);
int chn_text_wait(chn_stream *s, chn_result *r, chn_text_result *t);
/* chn_text_pack: the packing alone, synchronous (what a caller uses who wants the packed form back, as chn_minimisers exists
 * for `charon index`): the packed form of `t` downloaded into host arrays (any of them NULL = skip): bases2
 * [n_bases / 16], nmask [n_bases / 32] (all zero exactly when *has_n == 0), seg1_offset / seg2_offset [n], mean_quality [n].
 * Size the arrays from the layout rule above (or call once with NULL arrays for *n_bases).  Fewer than three batches may be in
 * flight.  Errors as chn_text_submit. */
int chn_text_pack(chn_stream *s, const chn_text_batch *t, uint32_t *bases2, uint32_t *nmask, uint64_t *seg1_offset,
                  uint64_t *seg2_offset, float *mean_quality, uint64_t *n_bases, uint32_t *has_n);

/* ---- FASTQ records found in a text that lies in device memory (no reference counterpart: the reference parses through seqan3 on
 * the CPU) ---------------------------------------------------------------------------------------------------------------------
 * With chn_inflate_run's CHN_INFLATE_OUT_DEVICE in front and CHN_TEXT_ON_DEVICE behind, a caller goes from BGZF members to per-read
 * calls while the text never leaves device memory: compressed bytes go up; about 40 bytes of descriptors per read, the id bytes and
 * the results come back.
 * THE RECORD RULE -- exactly what the front end's parallel FASTQ splitter accepts, applied from `start` one record after another.
 * A record is taken if and only if
 *   - its first byte is '@';
 *   - four line feeds follow inside [start, text_bytes);
 *   - the sequence line, after dropping one trailing '\r', has length n >= 1 and does not begin with '+';
 *   - the third line begins with '+';
 *   - the fourth line, after dropping one trailing '\r', has length n;
 * and its id is what follows '@' up to the line end, minus one trailing '\r' (it may be empty).  n_records is the number of records
 * taken before the first place where the rule fails or before max_records is reached, `consumed` the offset behind the last taken
 * record (`start` if there is none).  A blank line, a wrapped record, an empty read, a last line without a line feed or anything
 * else ends the run; everything from `consumed` on is the caller's business (typically: carry it in front of the next piece of
 * text, or hand it to a sequential parser with its own error handling).  `start` must be a record boundary for the result to mean
 * anything; a caller that processes a file in pieces passes the offset of the tail the piece before left over.
 * Descriptors: record i has its id at text[id_offset[i] .. + id_length[i]), its sequence at seq_offset[i] with seq_length[i] bytes
 * and its quality string at qual_offset[i] with the same length -- what chn_text_batch takes as seq1_* / qual1_*.  With `ids` the id
 * bytes come back to back, id i at the sum of id_length[0 .. i); ids_bytes is their total whether or not `ids` is given.
 * DEVICE TEXT CONTRACT (as CHN_TEXT_ON_DEVICE): `text` is device memory of the stream's device, 16-byte aligned, the allocation
 * readable up to text_bytes rounded up to 16.  The descriptor arrays and `ids` are HOST memory.
 * chn_text_split is SYNCHRONOUS: it runs its kernels on the stream's copy stream (count the line feeds per 4 KiB tile, scan, rank the
 * line starts, one lane per candidate record, scan and gather the ids), waits for the three output words and then for the descriptors
 * and ids, which come down in one batch of copies.  Batches in flight on the stream are not disturbed, but there must be fewer than
 * three.  Its scratch is the stream's, grow-only: 8 bytes per 4 KiB of text, and 52 bytes per record of the bound
 * min(max_records, (text_bytes - start) / 8) -- size max_records to the records expected, not to the worst case.
 * chn_text_split_host runs the same rule source on the CPU over HOST text (any alignment) and gives the same outputs.
 * Errors: CHN_E_INVALID for a wrong struct_size, a flag, start > text_bytes, a NULL descriptor array with max_records > 0, text that
 * is not device memory of the stream's device or misaligned, three batches in flight; CHN_E_CAPACITY for text_bytes above
 * CHN_TEXT_SPLIT_MAX_BYTES and for ids_capacity below ids_bytes (the message names the bytes needed).  On an error no output is
 * defined and nothing stays queued. */
#define CHN_TEXT_SPLIT_MAX_BYTES (1ull << 31)
typedef struct chn_text_split_job {
    uint32_t struct_size, flags;                 /* flags: 0 */
    const uint8_t *text; uint64_t text_bytes;    /* DEVICE memory on the stream's device (chn_text_split_host: HOST) */
    uint64_t start;                              /* records are looked for from this byte on; it is a record boundary */
    uint64_t max_records;                        /* capacity of the arrays below */
    uint64_t *id_offset;  uint32_t *id_length;   /* [max_records] HOST out; offsets are bytes into `text` */
    uint64_t *seq_offset; uint32_t *seq_length;  /* the quality string has the sequence's length */
    uint64_t *qual_offset;
    uint8_t *ids; uint64_t ids_capacity;         /* HOST out or NULL: the id bytes back to back, id i at sum(id_length[0..i)) */
    uint64_t n_records, consumed, ids_bytes;     /* out */
} chn_text_split_job;
int chn_text_split(chn_stream *s, chn_text_split_job *job);   /* synchronous */
int chn_text_split_host(chn_text_split_job *job);             /* the same rule source on the CPU; no GPU needed */

/* ---- FASTA records found and unwrapped in a text that lies in device memory (no reference counterpart: the reference parses
 * through seqan3 on the CPU) -------------------------------------------------------------------------------------------------------
 * What chn_text_split is for FASTQ, for FASTA: with chn_inflate_run's CHN_INFLATE_OUT_DEVICE in front and CHN_TEXT_ON_DEVICE behind,
 * the text never leaves device memory.  A FASTA sequence is spread over many lines, so besides finding the records the call UNWRAPS
 * them: the letters of the taken records are written back to back into a second device buffer, `seq_text`, which is what the caller
 * then submits as the text of a CHN_TEXT_ON_DEVICE batch (seq_offset / seq_length as seq1_*, no quality arrays).
 * THE RECORD RULE -- exactly what the front end's BlockReader::parse_fasta produces from a record boundary on (and with it what
 * seqan3::sequence_file_input gives the reference for a FASTA file: lines starting with '>' or ';' are id lines, blanks and digits
 * inside sequence lines are skipped).  Lines end at '\n' inside [start, text_bytes).
 *   - A HEADER LINE is a line whose first byte is '>' or ';'.  Record i runs from header line i up to the next header line.
 *   - The id is what follows the first byte up to the line feed, minus one trailing '\r' (it may be empty).
 *   - The sequence is the bytes of the lines between the two header lines, in order, without '\n', '\r', ' ', '\t' and '0' .. '9'.
 *   - A record is taken if and only if its first byte begins a header line, the header's line feed lies in the text, the next header
 *     line begins inside the text, and the compacted sequence has length >= 1.
 * With CHN_FASTA_SPLIT_END_OF_INPUT the end of the text counts as a following header line, and as the line end of a last line that
 * has no line feed: the last record of a file is taken too (parse_fasta at the end of its file).
 * Records are taken from `start` one after another until the rule fails or max_records is reached.  An empty record, a text that does
 * not begin with a header (leading blank lines included) and a record with no header behind it end the run; everything from
 * `consumed` on is the caller's business, as with chn_text_split.  `consumed` is the offset of the first record not taken
 * (text_bytes if everything was taken under the flag, `start` if nothing was).
 * Descriptors: record i has its id at text[id_offset[i] .. + id_length[i]) and its letters at seq_text[seq_offset[i] .. +
 * seq_length[i]); seq_offset[0] = 0, seq_offset[i + 1] = seq_offset[i] + seq_length[i], seq_bytes is the total.  Ids come back as
 * from chn_text_split.
 * `text` follows the DEVICE TEXT CONTRACT above.  So does `seq_text`: device memory of the stream's device, 16-byte aligned,
 * seq_capacity a multiple of 16 and at least text_bytes - start rounded up to 16 (a smaller one is CHN_E_CAPACITY); it must not
 * overlap `text`.  Nothing at or behind seq_bytes rounded up to 16 is written.  The descriptor arrays and `ids` are HOST memory.
 * chn_fasta_split is SYNCHRONOUS and keeps chn_text_split's conventions: its kernels run on the stream's copy stream (a summary per
 * 4 KiB tile, a one-workgroup scan that resolves the line running into every tile, header ranks, one lane per candidate record, the
 * compaction of the letters through LDS into aligned 16-byte stores, id scan and gather), it waits for the four output words and then
 * for the descriptors and ids.  Batches in flight on the stream are not disturbed, but there must be fewer than three.  Its scratch is
 * the stream's, grow-only: 52 bytes per 4 KiB of text, and 40 bytes per record of the bound min(max_records, (text_bytes - start) / 3).
 * chn_fasta_split_host runs the same rule source sequentially on the CPU over HOST text and a HOST seq_text of any alignment.
 * Errors: CHN_E_INVALID for a wrong struct_size, an unknown flag, start > text_bytes, a NULL descriptor array with max_records > 0,
 * seq_text overlapping text, text or seq_text that is not device memory of the stream's device or misaligned, a seq_capacity that is
 * no multiple of 16 (device call), three batches in flight; CHN_E_CAPACITY for text_bytes above CHN_TEXT_SPLIT_MAX_BYTES, a
 * seq_capacity below text_bytes - start rounded up to 16, and ids_capacity below ids_bytes (the message names the bytes needed).  On an
 * error no output is defined and nothing stays queued. */
#define CHN_FASTA_SPLIT_END_OF_INPUT 1u
typedef struct chn_fasta_split_job {
    uint32_t struct_size, flags;                 /* flags: 0 or CHN_FASTA_SPLIT_END_OF_INPUT */
    const uint8_t *text; uint64_t text_bytes;    /* DEVICE memory on the stream's device (chn_fasta_split_host: HOST) */
    uint64_t start;                              /* records are looked for from this byte on; it is a record boundary */
    uint64_t max_records;                        /* capacity of the arrays below */
    uint64_t *id_offset;  uint32_t *id_length;   /* [max_records] HOST out; offsets are bytes into `text` */
    uint64_t *seq_offset; uint32_t *seq_length;  /* [max_records] HOST out; offsets are bytes into `seq_text` */
    uint8_t *seq_text; uint64_t seq_capacity;    /* DEVICE out (chn_fasta_split_host: HOST): the letters of the taken records back to back */
    uint8_t *ids; uint64_t ids_capacity;         /* HOST out or NULL: the id bytes back to back, id i at sum(id_length[0..i)) */
    uint64_t n_records, consumed, ids_bytes, seq_bytes;   /* out */
} chn_fasta_split_job;
int chn_fasta_split(chn_stream *s, chn_fasta_split_job *job);   /* synchronous */
int chn_fasta_split_host(chn_fasta_split_job *job);             /* the same rule source on the CPU; no GPU needed */

/* ---- byte ranges of a text that lies in device memory, fetched into host memory (no reference counterpart) ------------------------
 * What a caller of the chain above uses for the few records whose letters it needs on the host after all (a gzip ratio the device
 * left open, a record to be written out): range i is text[offset[i] .. + length[i]) and goes to out + sum(length[0 .. i)), so the
 * ranges come back to back in the order given.  Ranges may overlap, repeat and have length 0; out_bytes is the sum of the lengths.
 * `text` follows the DEVICE TEXT CONTRACT above and nothing beyond it is read; offset, length and out are HOST memory, `out` pageable
 * or page-locked (page-locked memory is downloaded into directly, pageable memory through page-locked staging of the stream's).
 * chn_text_fetch is SYNCHRONOUS: it uploads 20 bytes per range, runs k_text_gather on the stream's copy stream (one wavefront a range
 * at a time; whole 16-byte pieces of the destination are single aligned stores built from aligned loads) and waits once for the
 * bytes.  Batches in flight on the stream are not disturbed, but there must be fewer than three.  Its staging is the stream's,
 * grow-only: 20 bytes per range, and the gathered bytes on the device and (pageable `out`) page-locked.
 * chn_text_fetch_host applies the same copy rule on the CPU over HOST text (any alignment).
 * Errors, all before anything is queued: CHN_E_INVALID for a wrong struct_size, a flag, a NULL range array with n_ranges > 0, a range
 * with offset[i] + length[i] > text_bytes (the message names it), text that is not device memory of the stream's device or misaligned,
 * three batches in flight; CHN_E_CAPACITY for out_capacity below the sum of the lengths (the message names the bytes needed).  On an
 * error nothing has been written and the stream stays usable. */
typedef struct chn_text_fetch_job {
    uint32_t struct_size, flags;                 /* flags: 0 */
    const uint8_t *text; uint64_t text_bytes;    /* DEVICE, device text contract (chn_text_fetch_host: HOST) */
    uint64_t n_ranges;
    const uint64_t *offset; const uint32_t *length;  /* [n] HOST; ranges may overlap, repeat, have length 0 */
    uint8_t *out; uint64_t out_capacity;         /* HOST, pageable or page-locked: range i at sum(length[0..i)) */
    uint64_t out_bytes;                          /* out: sum of the lengths */
} chn_text_fetch_job;
int chn_text_fetch(chn_stream *s, chn_text_fetch_job *job);   /* synchronous */
int chn_text_fetch_host(chn_text_fetch_job *job);             /* same copy rule on the CPU, no GPU needed */

/* ---- do the ids of the mates of every pair agree?  Two texts that lie in device memory (replaces the id comparison of the
 * reference's paired loop, src/dehost_main.cpp:423-430, for a caller whose two files are device-resident) ------------------------------
 * What a caller of the chain above uses on paired input, so that the ids of file 2 need not come down (the output names a pair by the
 * id of mate 1): pair i has its ids at text1[id1_offset[i] .. + id1_length[i]) and text2[id2_offset[i] .. + id2_length[i]) -- what
 * chn_text_split gave for the two files.
 * THE RULE (the front end's): both ids lose their LAST byte, the mate number of "name/1" and "name/2": la = id1_length ? id1_length - 1
 * : 0, lb likewise; the pair agrees if and only if la == lb and the first la bytes are equal.  The dropped byte never counts; two
 * empty ids agree, and so do an empty id and a one-byte id.  first_mismatch is the smallest i whose ids disagree, n_pairs if there is
 * none.  An id may have any uint32_t length.
 * text1 and text2 follow the DEVICE TEXT CONTRACT above (they may be the same buffer) and nothing beyond it is read; the id arrays are
 * HOST memory.
 * chn_text_pair_ids is SYNCHRONOUS: it uploads 24 bytes per pair, runs k_pair_ids on the stream's copy stream (one lane per pair;
 * aligned dwords that hold a wanted byte, shifted into place; the lowest disagreeing lane of a ballot, one atomicMin per wavefront)
 * and waits once for the one word.  Batches in flight on the stream are not disturbed, but there must be fewer than three.  Its
 * staging is the stream's, grow-only: 24 bytes per pair page-locked and on the device.  n_pairs == 0 is a no-op: first_mismatch = 0.
 * chn_text_pair_ids_host applies the same rule source on the CPU over HOST texts (any alignment).
 * Errors, all before anything is queued: CHN_E_INVALID for a wrong struct_size, a flag, n_pairs above CHN_TEXT_PAIR_MAX_PAIRS (2^28,
 * the record bound of chn_text_split; no array is looked at), a NULL id array with n_pairs > 0, an id with
 * offset + length > text1_bytes / text2_bytes (the whole id, dropped byte included; the message names pair and file), a text that is
 * not device memory of the stream's device or misaligned, three batches in flight.  On an error first_mismatch is not defined and
 * the stream stays usable. */
#define CHN_TEXT_PAIR_MAX_PAIRS (1ull << 28)
typedef struct chn_text_pair_job {
    uint32_t struct_size, flags;                        /* flags: 0 */
    const uint8_t *text1; uint64_t text1_bytes;         /* DEVICE, device text contract (chn_text_pair_ids_host: HOST, any alignment) */
    const uint8_t *text2; uint64_t text2_bytes;
    uint64_t n_pairs;
    const uint64_t *id1_offset; const uint32_t *id1_length;   /* [n] HOST: what chn_text_split gave for file 1 */
    const uint64_t *id2_offset; const uint32_t *id2_length;   /* [n] HOST: ... for file 2 */
    uint64_t first_mismatch;                            /* out: smallest i whose ids disagree, n_pairs if none */
} chn_text_pair_job;
int chn_text_pair_ids(chn_stream *s, chn_text_pair_job *job);   /* synchronous */
int chn_text_pair_ids_host(chn_text_pair_job *job);             /* same rule source on the CPU, no GPU needed */

/* Model + call only (k_model_call) on per-read counts the caller already holds -- used for reads that the
 * Result state machine cached while the KDE models were still training (include/result.hpp:139-151,181-198)
 * and that must be classified with the models as they are later.  All pointers are HOST arrays; outputs as in
 * chn_result.  Replaces ReadEntry::dehost / ReadEntry::classify (include/read_entry.hpp:281-291).
 * The rows are re-evaluated on the host exactly as chn_batch_wait does for host batches: every flagged row, every
 * row with num_hashes == 0 and, for gamma / beta models, every row.  No batch may be in flight.  The call stages its
 * inputs and outputs in device buffers of the stream's own (allocated on first use, max_reads rows): device-resident
 * results of earlier batches stay valid, so a caller with on_device results may run it on the counts of flagged reads. */
int chn_classify_counts(chn_stream *s, uint64_t n_reads, const uint32_t *num_hashes, const uint32_t *counts,
                        const uint32_t *unique_counts, const uint32_t *lengths, const float *mean_quality,
                        const float *compression, double *probabilities, uint8_t *call, uint8_t *confidence);
/* The same launch without the host re-evaluation: probabilities, call, confidence and flags exactly as k_model_call
 * wrote them -- the values a device-resident batch returns for the same counts.  Same buffers and rules as
 * chn_classify_counts; `flags` [n_reads] as chn_result.flags. */
int chn_classify_counts_raw(chn_stream *s, uint64_t n_reads, const uint32_t *num_hashes, const uint32_t *counts,
                            const uint32_t *unique_counts, const uint32_t *lengths, const float *mean_quality,
                            const float *compression, double *probabilities, uint8_t *call, uint8_t *confidence,
                            uint8_t *flags);

/* ---- row-sharded ("hash-bin" sharded) mode, dense exchange (the checker of the sparse exchange below) -----------
 * For an index too large for one GPU: rank r creates a chn_index with row_begin/row_end = its slice and a stream on it.
 * Per batch, on EVERY rank and for the SAME batch:
 *   1. chn_shard_minimise   all reads are minimised (redundantly); returns E = number of minimisers of the batch
 *   2. chn_shard_probe      partial[e][i][w] = word w of row hash_i(minimiser e) if this rank owns the row, else 0
 *   3. the caller sums `partial` (E*h*W uint64) over ranks with ONE all-reduce (RCCL; sum == select because exactly
 *      one rank owns each row) -- the library itself has no RCCL dependency
 *   4. chn_shard_finish     AND over the h hash functions, counts, model+call; then chn_batch_wait as usual.
 * `dev_partial` is a device buffer of the caller (e.g. a torch tensor); it may be NULL when E = 0 (a batch without a
 * minimiser has no partial words).  One sharded batch, dense or sparse, at a time per stream.  No reference counterpart (the reference is
 * single-process); replaces the same loop body as chn_batch_submit. */
int chn_shard_minimise(chn_stream *s, const chn_batch *b, uint64_t *n_entries);
int chn_shard_probe(chn_stream *s, const chn_index *shard, uint64_t *dev_partial, uint64_t capacity_words);
int chn_shard_finish(chn_stream *s, const uint64_t *dev_partial);

/* ---- row-sharded mode, sparse exchange -----------------------------------------------------------------------
 * The faster way to use an index whose rows are spread over n_ranks GPUs (rank r holds rows [row_splits[r], row_splits[r+1])):
 * every rank classifies ITS OWN reads, asks the owners for the rows it needs and gets them back.  Per batch, on every rank:
 *   1. chn_shardx_minimise   (asynchronous) the rank's reads are minimised; nothing is probed yet
 *   2. chn_shardx_counts     (blocks) send_counts[r] = number of probes (minimiser x hash function) whose row rank r owns,
 *                            *n_probes = their sum
 *   3. chn_shardx_queries    (asynchronous) dev_queries[n_probes]: the owner-local row number of every probe, grouped by owner
 *                            rank in rank order
 *   4. the caller exchanges the groups (all-to-all, 4 bytes per probe; RCCL on torch tensors -- the library has no RCCL dependency)
 *   5. chn_shardx_serve      (asynchronous; on the OWNER) dev_rows_out[j][w] = word w of the shard's row dev_queries_in[j]
 *   6. the caller sends the rows back the way the queries came (second all-to-all, 8 * bin_words bytes per probe), so that
 *      dev_rows_back is laid out exactly like dev_queries
 *   7. chn_shardx_finish     (asynchronous) AND over the h hash functions, counts, model+call; then chn_batch_wait as usual.
 * The asynchronous calls run on the stream's HIP stream: call chn_stream_sync before handing a buffer to a collective that runs
 * on another stream.  The stream `s` may be created on any index object of the same IBF (its rows are not read by steps 1-4, 7);
 * one sharded batch at a time per stream (use two streams to overlap step 1 of the next batch with step 5 of this one).
 * No reference counterpart (the reference is single-process); replaces the same loop body as chn_batch_submit. */
int chn_shardx_minimise(chn_stream *s, const chn_batch *b);
int chn_shardx_counts(chn_stream *s, uint32_t n_ranks, const uint64_t *row_splits /* [n_ranks + 1] */, uint64_t *n_probes,
                      uint64_t *send_counts /* [n_ranks] */);
int chn_shardx_queries(chn_stream *s, uint32_t *dev_queries, uint64_t capacity);
int chn_shardx_serve(chn_stream *s, const chn_index *shard, const uint32_t *dev_queries_in, uint64_t n_in, uint64_t *dev_rows_out);
int chn_shardx_finish(chn_stream *s, const uint64_t *dev_rows_back);

/* ---- index construction (`charon index`, src/index_main.cpp:118-160,238-263) ------------------------------
 * chn_minimisers: all minimisers emitted for the segments of `b` (seqan3 minimiser_hash with the stream's k, w), with
 * repeats, in an unspecified but deterministic order, copied to host memory.  Replaces the per-record
 * `record.sequence() | hash_adaptor` of count_and_store_hashes (:142-148); segments may overlap in `bases2`, which is how
 * long reference sequences are cut into chunks overlapping by w-1 bases (the union over such chunks is exactly the set
 * of window minima of the whole sequence).
 * chn_index_emplace: ibf.emplace(value, bin) for every value (:252-255); values are host memory. */
int chn_minimisers(chn_stream *s, const chn_batch *b, uint64_t *host_values, uint64_t capacity, uint64_t *n_values);
int chn_index_emplace(chn_index *idx, const uint64_t *host_values, uint64_t n_values, uint32_t bin);

/* ---- minimiser sets in device memory (`charon index`, src/index_main.cpp:141-149,247-255) ----------------------------------
 * The reference collects the minimisers of a file in an std::unordered_set (:141-149) and re-inserts every one of them into the
 * bucket's bin (:247-255).  A chn_hashset is that set kept in HBM: 64-bit values in one device buffer, appended to device to device,
 * made distinct by a radix sort and a unique pass on the device, and read in place by the emplace.  Only counts cross to the host.
 * A set is used by ONE thread at a time; every call is synchronous.  Every call checks its arguments before its first HIP call
 * (CHN_E_INVALID: a null pointer, a wrong struct_size, a tile_keys that is neither 0 nor a multiple of 256 up to 65 536, a non-zero
 * `reserved`), and every refusal, a failed allocation included, leaves the set holding the values it held and the caller's memory as it was.
 * Memory rule: the set owns one buffer, bytes_held bytes of it; an append that does not fit allocates max(need, twice the size),
 * copies device to device and frees the old buffer.  chn_hashset_unique takes scratch of its own (a second key buffer of n values,
 * 1 KiB of counters per tile of 4 096 keys, 18 KiB of histograms), frees it before it returns, and leaves the set in a buffer of
 * exactly n_distinct values.  A failed hipMalloc is CHN_E_NOMEM and the set stays valid (chn_hashset_download still gives every value).
 * A set holds fewer than 2^32 values: an append beyond that is CHN_E_CAPACITY.
 *   chn_hashset_append     n values from HOST memory (tests, and callers whose values are on the host)
 *   chn_minimisers_into    the values chn_minimisers returns for the same batch, as a multiset, appended in device memory; nothing
 *                          comes down but *n_values.  The overflow and misalignment statuses of chn_minimisers; CHN_E_INVALID, before
 *                          anything runs, where the stream's index and the set are on different devices
 *   chn_hashset_unique     sorts ascending and drops repeats; *n_distinct = values left.  Idempotent; after later appends it gives the
 *                          distinct values of everything appended so far (the whole buffer is sorted again)
 *   chn_hashset_size       *n = values held (repeats included until the next unique call), *bytes_held = device bytes of the buffer
 *   chn_hashset_download   values [first, first + n) to HOST memory; CHN_E_INVALID, nothing written, where that is not inside the set
 *   chn_index_emplace_set  ibf.emplace(value, bin) for every value of the set (:252-255), read in place: chn_index_emplace without the
 *                          upload, with its waits and refusals (a bin out of range, row shards emplace the rows they hold);
 *                          CHN_E_INVALID where index and set are on different devices
 *   chn_device_memory      free and total bytes of a device (hipMemGetInfo): what a caller sizes a budget for its sets from */
typedef struct chn_hashset chn_hashset;
typedef struct chn_hashset_cfg {
    uint32_t struct_size;      /* sizeof(chn_hashset_cfg) */
    int32_t device;            /* HIP device ordinal */
    uint32_t tile_keys;        /* 0: 4 096.  Test hook: a smaller multiple of 256 lets a small array span many tiles and scan rounds */
    uint32_t reserved;         /* 0 */
} chn_hashset_cfg;
int chn_hashset_create(const chn_hashset_cfg *cfg, chn_hashset **out);
int chn_hashset_destroy(chn_hashset *set);
int chn_hashset_append(chn_hashset *set, const uint64_t *host_values, uint64_t n);
int chn_minimisers_into(chn_stream *s, const chn_batch *b, chn_hashset *set, uint64_t *n_values);
int chn_hashset_unique(chn_hashset *set, uint64_t *n_distinct);
int chn_hashset_size(const chn_hashset *set, uint64_t *n, uint64_t *bytes_held);
int chn_hashset_download(const chn_hashset *set, uint64_t first, uint64_t n, uint64_t *host_values);
int chn_index_emplace_set(chn_index *idx, const chn_hashset *set, uint32_t bin);
int chn_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);

/* Per-kernel device time accumulated since the last reset (CHN_STREAM_PROFILE streams only), added up as the batches are waited for.
 * which: 0 = minimise+probe kernel, 1 = count kernel, 2 = model+call kernel, 3 = whole batch chain;
 *   0 is the device time ATTRIBUTABLE to each batch's minimise+probe kernel (both its launches): the probe kernels of consecutive
 *   batches run on two streams and overlap (unless the batch waited for last held reads long enough to be split over a wavefront:
 *   then every batch takes the first of the two), so a batch counts from max(its kernel's start, the latest end of the probe kernels of the
 *   batches waited for before it) to its kernel's end.  With one batch in flight that is the kernel's own time from start to end; with
 *   several, the total is the time during which some probe kernel was running (the union of their intervals, never more than the wall
 *   time around them) and total / launches is what a batch adds to it.  *launches counts batches.  reset forgets the previous end.
 *   1, 2 and 3 are event-bracketed times of each batch on its own; 3 runs from the batch's turn on its probe stream to the end of its
 *   model+call kernel and so contains the time its launch waits at the probe gate (until the batch before it has dispatched its last
 *   workgroup: about one kernel length with three in flight) and the time its probe kernel shares the device with its neighbour's; the
 *   brackets of 0 start behind that wait;
 * 4 (any stream): *launches = number of batches chn_batch_wait re-ran on worst-case buffers after a row-log overflow;
 * 5 (any stream): *launches = row fetches the last waited batch's minimise+probe kernel issued (h per minimiser; fewer for an index of
 *   at most four bins, whose rows are fetched one at a time and only while the AND so far still has a bin set);
 * 6, 7 (text batches of a CHN_STREAM_PROFILE stream): the host -> device copy of the text / k_text_pack and the mean-quality division,
 *   timed with events on the copy stream; *launches = text batches packed (chn_text_submit and chn_text_pack; reset with which = 7);
 * 8 (CHN_STREAM_PROFILE streams): chn_text_split's kernels in front of its first wait (count, scan, line starts, records, id scan), timed with
 *   events on the copy stream; *launches = calls;
 * 9 (CHN_STREAM_PROFILE streams): chn_text_fetch's k_text_gather, timed with events on the copy stream; *launches = calls;
 * 11 (CHN_STREAM_PROFILE streams): chn_text_pair_ids' k_pair_ids, timed with events on the copy stream; *launches = calls that ran
 *   it (n_pairs > 0).  10 and 12 are not slots: they are refused with CHN_E_INVALID like every other value;
 * 13 (any stream): *launches = batches whose minimise+probe launch was queued behind a probe-gate wait, i.e. held in its queue until the
 *   batch before it had no workgroup left to dispatch (0 on a CHN_STREAM_NO_PROBE_GATE stream, on a device without stream-wait-value
 *   support, and for batches that take the first probe stream because of long reads).  *total_ms is no time here: 1 if the stream
 *   gates at all (the device can wait for a value in memory and the stream was not created with CHN_STREAM_NO_PROBE_GATE), else 0;
 * 14 (CHN_STREAM_PROFILE streams): chn_fasta_split's kernels in front of its first wait (tiles, resolve, scans, headers, records,
 *   compaction, id scan), timed with events on the copy stream; *launches = calls. */
int chn_stream_profile(chn_stream *s, int which, double *total_ms, uint64_t *launches, int reset);
/* Algorithmic bytes of the last batch by SURVEY 8(d): sum over reads of ceil(L/4) + M*h*W*8 + (8 + 8C). */
int chn_stream_last_batch_bytes(chn_stream *s, uint64_t *bytes, uint64_t *total_minimisers);

/* ---- raw deflate members on the device (BGZF input of the front end; no reference counterpart: the reference reads through
 * seqan3's bgzf stream on CPU threads) ------------------------------------------------------------------------------------------
 * A job names n_members independent raw deflate streams (RFC 1951, no zlib or gzip wrapper) inside `in` and where in `out` each one's
 * bytes go.  The expected size of every member is known beforehand (a BGZF member carries it in its trailer) and is at most
 * CHN_INFLATE_MAX_OUT.  k_inflate_members decodes one member per wavefront; what it accepts is what zlib's inflate accepts, bytes of a
 * member behind its final block are ignored.  The descriptors are checked before anything runs: in_offset[i] + in_length[i] <= in_bytes,
 * out_length[i] <= CHN_INFLATE_MAX_OUT, out_offset[i] + out_length[i] <= out_bytes, out_offset[i + 1] >= out_offset[i] + out_length[i];
 * a violation is CHN_E_INVALID, chn_last_error() names the member, and nothing has run.  A corrupt member is NOT an error of the call:
 * the call returns 0, status[i] != 0, and every other member is decoded; the bytes of a failed member's stretch of `out` are
 * unspecified, bytes outside the members' stretches are never written.  n_members == 0 is a no-op and out_length[i] == 0 is legal
 * (BGZF's end-of-file marker).  chn_inflate_run / chn_inflate_run_host leave the CRC-32 of a member to the caller; the _crc forms take
 * it on the way (below).
 * A chn_inflate owns its streams and staging buffers (grow-only); it is used by ONE thread at a time, different handles may be driven
 * from different threads.  chn_inflate_run is synchronous.
 * CHN_INFLATE_OUT_DEVICE (chn_inflate_run / chn_inflate_run_crc only; the _host forms refuse it with CHN_E_INVALID): `out` is DEVICE
 * memory on the handle's device; out_offset / out_length / out_bytes mean what they mean otherwise.  k_inflate_members writes every
 * member straight to out + out_offset[i], whatever its alignment, and never outside the member's stretch; no output is staged or
 * downloaded; statuses (and CRCs) come back as always.  The call stays synchronous: when it returns the bytes are in place for work
 * on any stream.  `out` is checked before anything is launched: memory that is not device memory of the handle's device (page-locked
 * or pageable host memory, another device) is CHN_E_INVALID and the message says which.  Any other flag bit is CHN_E_INVALID. */
#define CHN_INFLATE_MAX_OUT 65536u
#define CHN_INFLATE_OUT_DEVICE 1u
/* status[i]: 0 ok | 1 input exhausted | 2 bad block header (type 3, stored LEN/NLEN) | 3 bad code lengths
 * | 4 bad symbol or distance | 5 more output than out_length | 6 stream ended short of out_length */
typedef struct chn_inflate chn_inflate;
typedef struct chn_inflate_job {
    uint32_t struct_size, flags;              /* flags: 0 or CHN_INFLATE_OUT_DEVICE */
    uint64_t n_members;
    const uint8_t *in;  uint64_t in_bytes;    /* HOST; pageable (e.g. a mapped file) or page-locked */
    const uint64_t *in_offset; const uint32_t *in_length;    /* [n] raw deflate data of member i */
    uint8_t *out;  uint64_t out_bytes;        /* HOST (CHN_INFLATE_OUT_DEVICE: DEVICE) */
    const uint64_t *out_offset; const uint32_t *out_length;  /* [n] expected size, <= CHN_INFLATE_MAX_OUT */
    uint32_t *status;                         /* [n] out */
} chn_inflate_job;
int chn_inflate_create(int32_t device, chn_inflate **out);
int chn_inflate_run(chn_inflate *h, const chn_inflate_job *job);       /* synchronous */
int chn_inflate_run_host(const chn_inflate_job *job);                  /* same decoder source on the CPU, one thread; no GPU needed */
int chn_inflate_destroy(chn_inflate *h);
/* measurement aid: device time of the kernels of the handle's last chn_inflate_run / chn_inflate_run_crc, from events around them */
int chn_inflate_kernel_ms(chn_inflate *h, double *ms);
/* The same calls with the members' CRC-32 -- the gzip trailer's, zlib's crc32(0, data, out_length); 0 for a member of length 0 -- taken
 * by the decoder itself: on the device by the member's wavefront, from the decoded bytes while they are still in LDS.  With `expected`,
 * a member that decodes completely (status 0) but whose CRC-32 differs from expected[i] gets status CHN_INFLATE_E_CRC; a decode failure
 * keeps its status 1..6.  crc32[i] is defined where status[i] is 0 or CHN_INFLATE_E_CRC and unspecified elsewhere; the bytes of a member
 * with CHN_INFLATE_E_CRC are what its stream decodes to.  crc == NULL is chn_inflate_run / chn_inflate_run_host exactly, and so is a
 * chn_inflate_crc with both arrays NULL (nothing is taken).  A wrong struct_size or a non-zero `reserved` is CHN_E_INVALID before anything
 * runs; the job is checked as above. */
#define CHN_INFLATE_E_CRC 7u   /* status: decoded completely, but the CRC-32 differs from expected[i] */
typedef struct chn_inflate_crc {
    uint32_t struct_size, reserved;   /* reserved: 0 */
    const uint32_t *expected;         /* [n] HOST, or NULL: nothing is compared */
    uint32_t *crc32;                  /* [n] HOST out, or NULL */
} chn_inflate_crc;
int chn_inflate_run_crc(chn_inflate *h, const chn_inflate_job *job, const chn_inflate_crc *crc);   /* synchronous */
int chn_inflate_run_host_crc(const chn_inflate_job *job, const chn_inflate_crc *crc);

/* ---- chunks of ONE deflate stream on the device (the ordinary one-stream .gz of the front end; no reference counterpart: the
 * reference reads through seqan3's gz input stream on CPU threads, src/dehost_main.cpp:324) ---------------------------------------
 * A job names n_chunks bit positions inside raw deflate data `in` (RFC 1951, no gzip header; it need not reach the end of the stream):
 * begin_bit[i] is the position of the block header chunk i starts at, strictly increasing; chunk 0's is a true block start BY CONTRACT,
 * the others may be guesses.  k_inflate_chunks decodes all chunks side by side, one wavefront each, without the 32 KiB of output in
 * front of them (16-bit symbols; a match reaching in front of its chunk leaves markers that name window positions): chunk i decodes
 * whole blocks until it stands at a block boundary at or behind target_bit[i] (>= begin_bit[i]) or has decoded a final block.  Then the
 * windows are handed down the chunks in stream order (window[k + 1] = the last 32 768 bytes of window[k] followed by chunk k's bytes;
 * `window`, at most 32 768 bytes, is what lies in front of chunk 0, window_bytes == 0: a member starts here) and every chunk's symbols
 * become bytes and a CRC-32 (zlib's crc32(0, bytes of chunk i, out_length[i])).
 * Per chunk: end_bit[i] / out_length[i] = the last complete block boundary it reached and the bytes it produced up to there;
 * final[i] = 1 if that block had BFINAL; status[i] says why it stopped: 0 at its target or behind a final block | 1 input exhausted
 * | 2, 3, 4 as in chn_inflate_job | 5 sym_capacity exhausted inside a block | CHN_INFLATE_E_ROOM out_bytes exhausted.
 * THE COUNTING RULE (the front end's induction): chunk k is PROVEN if k == 0, or if chunk k - 1 is proven, status[k - 1] == 0,
 * final[k - 1] == 0 and end_bit[k - 1] == begin_bit[k] -- its predecessor came to stand exactly on its start.  *n_counted is the
 * number of proven chunks.  The bytes of proven chunk k -- through its last complete block, whatever its status -- lie in `out` back
 * to back at the running sum of out_length; *out_used is their total.  The outputs of unproven chunks and the bytes of `out` behind
 * *out_used are unspecified; nothing is ever written behind out_bytes.  A proven chunk whose bytes do not fit gets
 * CHN_INFLATE_E_ROOM and out_length 0 and ends the chain.
 * THE DISTANCE RULE: a match that reaches in front of the member's first byte is status 4 (zlib's "invalid distance too far back").
 * Chunk 0 notices it while decoding (the distance exceeds window_bytes + its bytes so far), a later chunk when a marker resolves to a
 * window position below 32 768 - (window_bytes + the bytes of the chunks before it); such a chunk reports out_length 0 and
 * end_bit == begin_bit and ends the chain.
 * A corrupt or falsely started chunk is never an error of the call.  CHN_E_INVALID, with chn_last_error() naming the chunk and nothing
 * having run or been written: a wrong struct_size, an unknown flag (CHN_INFLATE_OUT_DEVICE is the only one; the _host form refuses
 * it), n_chunks > CHN_INFLATE_STREAM_MAX_CHUNKS, begin_bit not increasing or at or beyond 8 * in_bytes, target_bit[i] < begin_bit[i],
 * window_bytes > 32768, sym_capacity < CHN_INFLATE_STREAM_MIN_SYMS, a NULL array but crc32.  n_chunks == 0 is a no-op.
 * sym_capacity is the number of symbols ONE chunk may produce (the device keeps n_chunks stretches of that many 16-bit symbols;
 * values above 2^30 are taken as 2^30).  `in` is host memory, pageable or page-locked; `out` is host memory, or with
 * CHN_INFLATE_OUT_DEVICE device memory of the handle's device (checked before anything is launched, as in chn_inflate_run).
 * chn_inflate_stream_run is synchronous and shares the handle (ONE thread at a time) with chn_inflate_run; chn_inflate_kernel_ms
 * afterwards reports the device time of this run's kernels.  chn_inflate_stream_run_host runs the same decoder source and the same
 * hand-down and byte rules on one CPU thread. */
#define CHN_INFLATE_STREAM_MAX_CHUNKS 4096u
#define CHN_INFLATE_STREAM_MIN_SYMS 131072u
#define CHN_INFLATE_E_ROOM 8u   /* status: a proven chunk whose bytes do not fit into out_bytes */
typedef struct chn_inflate_stream_job {
    uint32_t struct_size, flags;              /* flags: 0 or CHN_INFLATE_OUT_DEVICE */
    uint64_t n_chunks;
    const uint8_t *in;  uint64_t in_bytes;    /* HOST */
    const uint64_t *begin_bit; const uint64_t *target_bit;   /* [n] */
    const uint8_t *window;  uint64_t window_bytes;           /* HOST: the output in front of chunk 0, at most 32 768 bytes */
    uint64_t sym_capacity;
    uint8_t *out;  uint64_t out_bytes;        /* HOST (CHN_INFLATE_OUT_DEVICE: DEVICE) */
    uint64_t *end_bit; uint64_t *out_length;  /* [n] out */
    uint32_t *status;                         /* [n] out */
    uint8_t *final;                           /* [n] out */
    uint32_t *crc32;                          /* [n] out, or NULL */
    uint64_t *n_counted; uint64_t *out_used;  /* out */
} chn_inflate_stream_job;
int chn_inflate_stream_run(chn_inflate *h, const chn_inflate_stream_job *job);   /* synchronous */
int chn_inflate_stream_run_host(const chn_inflate_stream_job *job);              /* same decoder source on the CPU, one thread; no GPU needed */

/* ---- block starts of ONE deflate stream (the search in front of chn_inflate_stream_run; CPU form only; no reference counterpart: the
 * reference reads through seqan3's gz input stream on CPU threads, src/dehost_main.cpp:324) ---------------------------------------
 * A job names n_ranges ranges [from_bit[i], to_bit[i]) of bit positions inside `in` (positions count from bit 0 of `in`, LSB first);
 * the ranges need not be ordered or disjoint.  found_bit[i] is the FIRST position p of range i that passes all of R0 - R6, or
 * CHN_INFLATE_SEARCH_NONE:
 *   R0  (p >> 3) + 8 <= in_bytes, and with at = p + 17 also (at >> 3) + 9 <= in_bytes;
 *   R1  the 3 bits at p are BFINAL = 0, BTYPE = 2 (value 4), the HLIT field is <= 29 and the HDIST field is <= 29;
 *   R2  of the HCLEN + 4 three-bit code-length-code lengths at p + 17, 128 >> l summed over the non-zero lengths l is exactly 128;
 *   R3  the dynamic header parses by the rules of the library's decoder (zlib's: a complete code-length code, repeats in range, an
 *       end-of-block code present, literal/length and distance sets complete or a single 1-bit code, an empty distance set);
 *   R4  the block decodes symbol by symbol until end-of-block or until at least 32 768 output symbols have been produced: the count is
 *       checked before each literal/length code is read, a match counts as its length and may pass the limit, nothing read after the
 *       limit is reached can refute; every literal is text (9, 10, 13 or 32 .. 126), every code is valid, no more bits are consumed
 *       than `in` holds.  There is NO distance check: the window is unknown, any distance up to 32 768 is acceptable anywhere;
 *   R5  at least 32 symbols were produced;
 *   R6  if the block ended at end-of-block, the next three bits start a block header that parses, with any BFINAL: type 0 with
 *       LEN == ~NLEN behind the byte boundary, type 1 always, type 2 a dynamic header as under R3; type 3 refutes.
 * A found position is only a CANDIDATE: noise passes these tests now and then, and it is the counting rule of chn_inflate_stream_run
 * (a chunk in front of it comes to stand exactly on it) that proves or refutes it.
 * CHN_E_INVALID, with chn_last_error() naming the range and nothing having run or been written: a wrong struct_size, a non-zero flag,
 * n_ranges > CHN_INFLATE_STREAM_MAX_CHUNKS, a NULL array, from_bit[i] > to_bit[i], to_bit[i] > 8 * in_bytes.  n_ranges == 0 is a
 * no-op; an empty range reports CHN_INFLATE_SEARCH_NONE.
 * chn_inflate_stream_search_host runs on the calling thread, with the decoder source of chn_inflate_stream_run_host and an output side
 * that stores nothing.  There is no device form of the call yet: the job struct is laid out for one (a handle as first argument, as
 * chn_inflate_stream_run has it). */
#define CHN_INFLATE_SEARCH_NONE (~(uint64_t)0)
typedef struct chn_inflate_search_job {
    uint32_t struct_size, flags;              /* flags: 0 */
    uint64_t n_ranges;                        /* <= CHN_INFLATE_STREAM_MAX_CHUNKS */
    const uint8_t *in;  uint64_t in_bytes;    /* HOST */
    const uint64_t *from_bit; const uint64_t *to_bit;   /* [n] from <= to <= 8 * in_bytes */
    uint64_t *found_bit;                      /* [n] out: the position, or CHN_INFLATE_SEARCH_NONE */
} chn_inflate_search_job;
int chn_inflate_stream_search_host(const chn_inflate_search_job *job);              /* one CPU thread; no GPU needed */

/* ---- deflate on the device (the extract files of the front end; no reference counterpart: the reference writes through zlib's
 * gzFile on one CPU thread) -------------------------------------------------------------------------------------------------------
 * A job names n_members independent pieces of at most CHN_DEFLATE_MAX_IN bytes (bgzip's block size) inside `in`.  Every piece becomes
 * one raw deflate stream (RFC 1951) of a single block with BFINAL = 1 -- stored, static or dynamic, whichever zlib's own rule finds
 * smallest, so never more than in_length + 5 bytes -- and with CHN_DEFLATE_BGZF a complete BGZF block: the 18-byte gzip header with the
 * BC subfield and BSIZE, the deflate data, CRC-32 and ISIZE.  The members come out back to back in member order: member i at
 * out_offset[i] with out_length[i] bytes, out_offset[0] = 0, out_offset[i + 1] = out_offset[i] + out_length[i], *out_used = the end of
 * the last, so out[0 .. *out_used) can be written to a file as it stands.  in_length[i] == 0 is legal and yields the empty member:
 * under CHN_DEFLATE_BGZF the 28-byte end-of-file marker.  crc32 (optional) receives zlib's crc32(0, piece, in_length[i]).
 * The descriptors are checked before anything runs: struct_size, no unknown flag, in_offset[i] + in_length[i] <= in_bytes,
 * in_length[i] <= CHN_DEFLATE_MAX_IN, out_bytes >= chn_deflate_bound(n_members, sum of in_length, flags); a violation is CHN_E_INVALID,
 * chn_last_error() names the member, and nothing has run or been written.  n_members == 0 is a no-op (*out_used = 0).
 * k_deflate_members compresses one piece per wavefront; chn_deflate_run_host runs the same compressor source on the CPU and gives the
 * same bytes.  A chn_deflate owns its streams, staging and scratch (grow-only); ONE thread at a time per handle.  chn_deflate_run is
 * synchronous. */
#define CHN_DEFLATE_MAX_IN 65280u
#define CHN_DEFLATE_BGZF 1u
typedef struct chn_deflate chn_deflate;
typedef struct chn_deflate_job {
    uint32_t struct_size, flags;              /* flags: 0 or CHN_DEFLATE_BGZF */
    uint64_t n_members;
    const uint8_t *in;  uint64_t in_bytes;    /* HOST; pageable or page-locked */
    const uint64_t *in_offset; const uint32_t *in_length;    /* [n] piece i; the pieces may lie anywhere in `in` */
    uint8_t *out;  uint64_t out_bytes;        /* HOST; pageable or page-locked */
    uint64_t *out_offset; uint32_t *out_length;              /* [n] out */
    uint64_t *out_used;                       /* out */
    uint32_t *crc32;                          /* [n] out, or NULL */
} chn_deflate_job;
int chn_deflate_create(int32_t device, chn_deflate **out);
int chn_deflate_run(chn_deflate *h, const chn_deflate_job *job);       /* synchronous */
int chn_deflate_run_host(const chn_deflate_job *job);                  /* same compressor source on the CPU, one thread; no GPU needed */
int chn_deflate_destroy(chn_deflate *h);
/* bytes that `out` must have for n_members pieces of in_bytes_total bytes altogether */
int chn_deflate_bound(uint64_t n_members, uint64_t in_bytes_total, uint32_t flags, uint64_t *bytes);
/* measurement aid: device time of the kernels of the handle's last chn_deflate_run, from events around them */
int chn_deflate_kernel_ms(chn_deflate *h, double *ms);
/* testing and measurement aid: at most `members` (1 .. 1024, the default) members in one group of chn_deflate_run's pipeline */
int chn_deflate_group_members(chn_deflate *h, uint32_t members);

/* ---- the records of an --extract file formed and deflated on the device (no reference counterpart: the reference forms them on the
 * CPU and writes through zlib's gzFile) ------------------------------------------------------------------------------------------
 * What a caller of the device-resident chain (chn_inflate_run's CHN_INFLATE_OUT_DEVICE, chn_text_split, CHN_TEXT_ON_DEVICE) uses to
 * write reads out as BGZF FASTQ without bringing their letters down: a chn_extract stands for ONE output file.
 * THE RECORD RULE: record i is  '@' id '\n' SEQ '\n' '+' '\n' qual '\n'  with id = text[id_offset[i] .. + id_length[i]) and
 * qual = text[qual_offset[i] .. + qual_length[i]) as they stand and SEQ = text[seq_offset[i] .. + seq_length[i]) with every byte
 * through the front end's letter map: A C G T in either case become upper case, U / u become T, every other byte (the IUPAC letters;
 * a byte that is no letter cannot be in a read chn_text_submit accepted) becomes N.  It has id_length + seq_length + qual_length + 6
 * bytes; the records of a job follow one another in the order given.
 * THE FILE'S TEXT is everything appended to the handle, in order -- records formed on the device by chn_extract_append_records from
 * a device text, and host bytes the caller formed itself, uploaded by chn_extract_append_bytes.  It is cut into pieces of
 * CHN_DEFLATE_MAX_IN bytes at multiples of that size from the file's start, whatever the appends were.  Every append writes its bytes
 * behind the handle's pending tail in device memory, compresses every whole piece that is there then (k_deflate_members under
 * CHN_DEFLATE_BGZF, reading the pending buffer in place), brings the members down back to back into `out` (*out_used bytes, possibly
 * 0) and keeps the fewer than CHN_DEFLATE_MAX_IN bytes behind the last piece as the new tail.  chn_extract_finish compresses a
 * non-empty tail as one last, shorter member and leaves the handle empty, ready for another file; it writes NO end-of-file marker.
 * THE PIN: for any sequence of appends, the bytes the handle returned, chn_extract_finish's included, are those of chn_deflate_run_host
 * under CHN_DEFLATE_BGZF over the file's text cut at multiples of CHN_DEFLATE_MAX_IN.
 * chn_extract_bound gives the bytes `out` must have for an append of appended_bytes to the handle as it stands (appended_bytes is the
 * sum of the records' lengths, or n); with appended_bytes == 0, what chn_extract_finish needs.
 * `text` follows the DEVICE TEXT CONTRACT (device memory of the handle's device, 16-byte aligned, readable up to text_bytes rounded up
 * to 16) and nothing beyond it is read; the descriptor arrays, `bytes` and `out` are HOST memory, `out` pageable or page-locked.
 * Every call is SYNCHRONOUS: when it returns, nothing of it is queued and `text` is no longer needed.  A chn_extract owns its streams,
 * its staging and a grow-only device buffer of pending text; ONE thread at a time per handle, no chn_stream.  n_records == 0 and
 * n == 0 are no-ops (out_used = 0).
 * chn_extract_records_host applies the record rule on the CPU over HOST text of any alignment: the records of `job` (its out fields
 * are not looked at) back to back into text_out, *bytes their total; CHN_E_CAPACITY if capacity is below it.
 * Errors, all before anything is queued, the handle staying usable and nothing appended: CHN_E_INVALID for a wrong struct_size, a
 * flag, a NULL descriptor array with n_records > 0, an id, sequence or quality string that ends behind text_bytes (the message names
 * the record), text that is not device memory of the handle's device or misaligned; CHN_E_CAPACITY for out_capacity below
 * chn_extract_bound for this append (the message names the bytes needed).  After CHN_E_HIP the handle can only be destroyed. */
typedef struct chn_extract chn_extract;
typedef struct chn_extract_job {
    uint32_t struct_size, flags;                 /* flags: 0 */
    const uint8_t *text; uint64_t text_bytes;    /* DEVICE, device text contract (chn_extract_records_host: HOST) */
    uint64_t n_records;
    const uint64_t *id_offset;   const uint32_t *id_length;    /* [n] HOST: what chn_text_split gave */
    const uint64_t *seq_offset;  const uint32_t *seq_length;
    const uint64_t *qual_offset; const uint32_t *qual_length;
    uint8_t *out; uint64_t out_capacity;         /* HOST, pageable or page-locked: the BGZF members of the whole pieces */
    uint64_t out_used;                           /* out */
} chn_extract_job;
int chn_extract_create(int32_t device, chn_extract **out);
int chn_extract_destroy(chn_extract *h);
int chn_extract_bound(const chn_extract *h, uint64_t appended_bytes, uint64_t *out_bytes);
int chn_extract_append_records(chn_extract *h, chn_extract_job *job);     /* synchronous */
int chn_extract_append_bytes(chn_extract *h, const uint8_t *bytes, uint64_t n, uint8_t *out, uint64_t out_capacity, uint64_t *out_used);
int chn_extract_finish(chn_extract *h, uint8_t *out, uint64_t out_capacity, uint64_t *out_used);
int chn_extract_records_host(chn_extract_job *job, uint8_t *text_out, uint64_t capacity, uint64_t *bytes);
/* measurement aid: device time of the kernels of the handle's last call (k_extract_records and the compressor's), from events around them */
int chn_extract_kernel_ms(chn_extract *h, double *ms);

/* ---- synthetic workload fabrication on the device (bench / tests; no reference counterpart) ---------- */
/* Measurement aid: the rate this device sustains for NOTHING BUT the index's probe pattern -- independent uniformly random row
 * fetches of 8 * bin_words bytes from THIS index's words (one load per thread in flight, 32 wavefronts per CU, `nt` cache policy if
 * nt != 0) -- in row fetches per second.  bench.py reports k_minimise_probe's probe rate against it (roofline.gather_roof). */
int chn_index_gather_roof(chn_index *idx, int nt, double *fetches_per_s);
/* Random 2-bit genomes: n_genomes x genome_len bases (genome_len multiple of 64), counter-based PRNG. */
int chn_synth_genomes(int device, uint64_t seed, uint64_t n_genomes, uint64_t genome_len, uint32_t **dev_bases2);
/* Set every bit of user bins [0,B) of every row with probability `density` (background fill). */
int chn_synth_fill_index(chn_index *idx, uint64_t seed, double density);
/* Insert the minimisers of genome g into bin genome_bin[g] (IBF emplace, 3 rows each). */
int chn_synth_plant(chn_index *idx, const uint32_t *dev_bases2, uint64_t n_genomes, uint64_t genome_len,
                    const uint8_t *genome_bin /* host, [n_genomes] */);
/* Sample `n_reads` reads of `read_len` bases: read i comes from genome (hash % n_genomes) with probability
 * 1 - random_fraction (uniform start, i.i.d. substitutions at `sub_rate`), else is uniformly random.
 * Writes a packed batch into freshly allocated device buffers (segments padded to 64 bases). */
typedef struct chn_synth_reads_out {
    uint32_t *bases2;
    uint64_t *seg1_offset;
    uint32_t *seg1_length;
    float *mean_quality;
    float *compression;
    uint64_t n_bases;
} chn_synth_reads_out;
/* `first_read_id`: global index of read 0 of this batch; a read's content depends only on (seed, global index), so
 * the union of the batches of N ranks equals one batch of N times the size. */
int chn_synth_reads(int device, uint64_t seed, const uint32_t *dev_genomes, uint64_t n_genomes, uint64_t genome_len,
                    uint64_t first_read_id, uint64_t n_reads, uint32_t read_len_min, uint32_t read_len_max, double sub_rate,
                    double random_fraction, float mean_quality, chn_synth_reads_out *out);
/* Page-locked host memory.  Host batches whose arrays live in such memory are uploaded asynchronously on a copy stream,
 * so with batches in flight the upload of the next one overlaps the kernels of those before; pageable memory works too but
 * its copies are staged synchronously by the runtime. */
int chn_host_alloc(uint64_t bytes, void **ptr);
int chn_host_free(void *ptr);
int chn_device_malloc(int device, uint64_t bytes, void **ptr);
int chn_device_free(int device, void *ptr);
int chn_device_upload(int device, void *dev_dst, const void *host_src, uint64_t bytes);
int chn_device_download(int device, void *host_dst, const void *dev_src, uint64_t bytes);
/* bytes from one place in device memory to another on the SAME device (e.g. the unconsumed tail of one block of text in front of the
 * next).  Synchronous.  CHN_E_INVALID if either stretch is not device memory of `device`, or if the two overlap. */
int chn_device_copy(int device, void *dev_dst, const void *dev_src, uint64_t bytes);

const char *chn_last_error(void);
const char *chn_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CHARON_HIP_H */
