"""ctypes binding of libcharon_hip.so (C ABI: include/charon_hip.h).

There is no fallback path: if the library is missing this module raises at import, so a GPU test can
never silently pass on CPU code.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CHARON_HIP_LIB") or os.path.join(HERE, "libcharon_hip.so")  # the override is for A/B diagnostics builds
if not os.path.exists(LIB_PATH):
    raise ImportError("charon_amd: %s not built -- run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
_L = C.CDLL(LIB_PATH)

MINIMISER_SEED = 0x8F3F73B5CF1C9ADE
STREAM_PROFILE = 1
STREAM_TINY_LOG = 2
STREAM_NO_PROBE_GATE = 4
# chn_batch.gzip_output (include/charon_hip.h)
GZIP_TALLIES, GZIP_SIZES, GZIP_BOTH = 0, 1, 2
GZIP_SIZES_ALL = 3           # the gzip size of every read of 1 .. gzip_tallies letters, any length, any number of deflate blocks
GZIP_ANY_LEN = 0xFFFFFFFF    # gzip_tallies under GZIP_SIZES_ALL: no length bound


class IndexDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("kmer_size", C.c_uint8), ("window_size", C.c_uint8),
                ("hash_funs", C.c_uint8), ("num_categories", C.c_uint8), ("host_index", C.c_uint8), ("reserved0", C.c_uint8 * 3),
                ("minimiser_seed", C.c_uint64), ("bins", C.c_uint64), ("technical_bins", C.c_uint64), ("bin_size", C.c_uint64),
                ("hash_shift", C.c_uint64), ("bin_words", C.c_uint64), ("bin_to_category", C.c_uint8 * 256),
                ("row_begin", C.c_uint64), ("row_end", C.c_uint64)]


class Model(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("num_categories", C.c_uint32), ("pos_data", C.POINTER(C.POINTER(C.c_float))),
                ("pos_n", C.POINTER(C.c_uint32)), ("neg_data", C.POINTER(C.POINTER(C.c_float))), ("neg_n", C.POINTER(C.c_uint32)),
                ("h_pos", C.c_float), ("h_neg", C.c_float), ("err_rate", C.c_float), ("min_quality", C.c_float),
                ("min_length", C.c_uint32), ("min_compression", C.c_float), ("confidence_threshold", C.c_int8),
                ("min_hits", C.c_uint8), ("paired", C.c_uint8), ("host_index", C.c_uint8),
                ("confidence_probability_threshold", C.c_float), ("host_unique_prop_lo_threshold", C.c_float),
                ("min_proportion_difference", C.c_float), ("min_prob_difference", C.c_float),
                ("dist", C.c_uint32), ("pos_params", C.POINTER(C.c_float)), ("neg_params", C.POINTER(C.c_float))]


class StreamCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("max_reads", C.c_uint64), ("max_bases", C.c_uint64)]


class Batch(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("on_device", C.c_uint32), ("n_reads", C.c_uint64), ("n_bases", C.c_uint64),
                ("bases2", C.c_void_p), ("nmask", C.c_void_p), ("seg1_offset", C.c_void_p), ("seg1_length", C.c_void_p),
                ("seg2_offset", C.c_void_p), ("seg2_length", C.c_void_p), ("mean_quality", C.c_void_p),
                ("compression", C.c_void_p), ("gzip_tallies", C.c_uint32), ("gzip_output", C.c_uint32)]


class Result(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("on_device", C.c_uint32), ("num_hashes", C.c_void_p), ("counts", C.c_void_p),
                ("unique_counts", C.c_void_p), ("probabilities", C.c_void_p), ("call", C.c_void_p), ("confidence", C.c_void_p),
                ("flags", C.c_void_p), ("gzip_tallies", C.c_void_p), ("gzip_sizes", C.c_void_p)]


TEXT_DNA5_RANKS = 1          # chn_text_batch.flags: the text holds seqan3 dna5 ranks (0 A, 1 C, 2 G, 3 N, 4 T), not letters
TEXT_ON_DEVICE = 2           # chn_text_batch.flags: `text` is device memory (16-byte aligned, readable up to text_bytes rounded up to 16)
TEXT_SPLIT_MAX_BYTES = 1 << 31   # CHN_TEXT_SPLIT_MAX_BYTES
TEXT_PAIR_MAX_PAIRS = 1 << 28    # CHN_TEXT_PAIR_MAX_PAIRS


class TextBatch(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_reads", C.c_uint64), ("text", C.c_void_p),
                ("text_bytes", C.c_uint64), ("seq1_offset", C.c_void_p), ("seq1_length", C.c_void_p), ("qual1_offset", C.c_void_p),
                ("qual1_length", C.c_void_p), ("seq2_offset", C.c_void_p), ("seq2_length", C.c_void_p), ("qual2_offset", C.c_void_p),
                ("qual2_length", C.c_void_p), ("compression", C.c_void_p), ("gzip_tallies", C.c_uint32), ("gzip_output", C.c_uint32)]


class TextBatch2(C.Structure):
    """chn_text_batch2: a chn_text_batch with a second device text behind it (the fields of the batch are named as in TextBatch)"""
    _fields_ = TextBatch._fields_ + [("text2", C.c_void_p), ("text2_bytes", C.c_uint64)]


class TextSplitJob(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("text", C.c_void_p), ("text_bytes", C.c_uint64), ("start", C.c_uint64),
                ("max_records", C.c_uint64), ("id_offset", C.c_void_p), ("id_length", C.c_void_p), ("seq_offset", C.c_void_p),
                ("seq_length", C.c_void_p), ("qual_offset", C.c_void_p), ("ids", C.c_void_p), ("ids_capacity", C.c_uint64),
                ("n_records", C.c_uint64), ("consumed", C.c_uint64), ("ids_bytes", C.c_uint64)]


FASTA_SPLIT_END_OF_INPUT = 1     # CHN_FASTA_SPLIT_END_OF_INPUT


class FastaSplitJob(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("text", C.c_void_p), ("text_bytes", C.c_uint64), ("start", C.c_uint64),
                ("max_records", C.c_uint64), ("id_offset", C.c_void_p), ("id_length", C.c_void_p), ("seq_offset", C.c_void_p),
                ("seq_length", C.c_void_p), ("seq_text", C.c_void_p), ("seq_capacity", C.c_uint64), ("ids", C.c_void_p),
                ("ids_capacity", C.c_uint64), ("n_records", C.c_uint64), ("consumed", C.c_uint64), ("ids_bytes", C.c_uint64),
                ("seq_bytes", C.c_uint64)]


class TextFetchJob(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("text", C.c_void_p), ("text_bytes", C.c_uint64), ("n_ranges", C.c_uint64),
                ("offset", C.c_void_p), ("length", C.c_void_p), ("out", C.c_void_p), ("out_capacity", C.c_uint64), ("out_bytes", C.c_uint64)]


class TextPairJob(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("text1", C.c_void_p), ("text1_bytes", C.c_uint64), ("text2", C.c_void_p),
                ("text2_bytes", C.c_uint64), ("n_pairs", C.c_uint64), ("id1_offset", C.c_void_p), ("id1_length", C.c_void_p),
                ("id2_offset", C.c_void_p), ("id2_length", C.c_void_p), ("first_mismatch", C.c_uint64)]


class TextResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("has_n", C.c_uint32), ("n_bases", C.c_uint64), ("mean_quality", C.c_void_p)]


INFLATE_MAX_OUT = 65536      # CHN_INFLATE_MAX_OUT
# chn_inflate_job.status values
INFLATE_STATUS = {0: "ok", 1: "input exhausted", 2: "bad block header", 3: "bad code lengths", 4: "bad symbol or distance",
                  5: "more output than out_length", 6: "stream ended short of out_length", 7: "CRC-32 differs from the expected one"}
INFLATE_E_CRC = 7            # CHN_INFLATE_E_CRC
INFLATE_OUT_DEVICE = 1       # CHN_INFLATE_OUT_DEVICE: chn_inflate_job.out is device memory


class InflateJob(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_members", C.c_uint64), ("in_", C.c_void_p), ("in_bytes", C.c_uint64),
                ("in_offset", C.c_void_p), ("in_length", C.c_void_p), ("out", C.c_void_p), ("out_bytes", C.c_uint64),
                ("out_offset", C.c_void_p), ("out_length", C.c_void_p), ("status", C.c_void_p)]


class InflateCrc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("expected", C.c_void_p), ("crc32", C.c_void_p)]


INFLATE_STREAM_MAX_CHUNKS = 4096    # CHN_INFLATE_STREAM_MAX_CHUNKS
INFLATE_STREAM_MIN_SYMS = 131072    # CHN_INFLATE_STREAM_MIN_SYMS
INFLATE_E_ROOM = 8                  # CHN_INFLATE_E_ROOM


class InflateStreamJob(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_chunks", C.c_uint64), ("in_", C.c_void_p), ("in_bytes", C.c_uint64),
                ("begin_bit", C.c_void_p), ("target_bit", C.c_void_p), ("window", C.c_void_p), ("window_bytes", C.c_uint64),
                ("sym_capacity", C.c_uint64), ("out", C.c_void_p), ("out_bytes", C.c_uint64), ("end_bit", C.c_void_p),
                ("out_length", C.c_void_p), ("status", C.c_void_p), ("final", C.c_void_p), ("crc32", C.c_void_p),
                ("n_counted", C.c_void_p), ("out_used", C.c_void_p)]


INFLATE_SEARCH_NONE = 2 ** 64 - 1    # CHN_INFLATE_SEARCH_NONE


class InflateSearchJob(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_ranges", C.c_uint64), ("in_", C.c_void_p), ("in_bytes", C.c_uint64),
                ("from_bit", C.c_void_p), ("to_bit", C.c_void_p), ("found_bit", C.c_void_p)]


DEFLATE_MAX_IN = 65280       # CHN_DEFLATE_MAX_IN
DEFLATE_BGZF = 1             # CHN_DEFLATE_BGZF


class DeflateJob(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_members", C.c_uint64), ("in_", C.c_void_p), ("in_bytes", C.c_uint64),
                ("in_offset", C.c_void_p), ("in_length", C.c_void_p), ("out", C.c_void_p), ("out_bytes", C.c_uint64),
                ("out_offset", C.c_void_p), ("out_length", C.c_void_p), ("out_used", C.c_void_p), ("crc32", C.c_void_p)]


class ExtractJob(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("text", C.c_void_p), ("text_bytes", C.c_uint64), ("n_records", C.c_uint64),
                ("id_offset", C.c_void_p), ("id_length", C.c_void_p), ("seq_offset", C.c_void_p), ("seq_length", C.c_void_p),
                ("qual_offset", C.c_void_p), ("qual_length", C.c_void_p), ("out", C.c_void_p), ("out_capacity", C.c_uint64),
                ("out_used", C.c_uint64)]


class EfLayout(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("wl", C.c_uint32), ("m_size", C.c_uint64), ("ones", C.c_uint64), ("low_bits", C.c_uint64),
                ("high_bits", C.c_uint64), ("n_low_words", C.c_uint64), ("n_high_words", C.c_uint64)]


class EfEncodeJob(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("slice_rows", C.c_uint64), ("layout", C.POINTER(EfLayout)),
                ("low", C.c_void_p), ("n_low_words", C.c_uint64), ("high", C.c_void_p), ("n_high_words", C.c_uint64),
                ("ones_written", C.c_uint64), ("device_ms", C.c_double)]


class HashSetCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("tile_keys", C.c_uint32), ("reserved", C.c_uint32)]


class SynthReadsOut(C.Structure):
    _fields_ = [("bases2", C.c_void_p), ("seg1_offset", C.c_void_p), ("seg1_length", C.c_void_p), ("mean_quality", C.c_void_p),
                ("compression", C.c_void_p), ("n_bases", C.c_uint64)]


# every symbol include/charon_hip.h declares
EXPORTS = ["chn_index_create", "chn_index_upload_rows", "chn_index_device_words", "chn_index_download_rows",
           "chn_index_get_desc", "chn_index_destroy", "chn_model_default", "chn_stream_create", "chn_stream_destroy",
           "chn_model_set", "chn_batch_submit", "chn_batch_wait", "chn_stream_sync", "chn_classify_counts", "chn_classify_counts_raw", "chn_stream_profile",
           "chn_stream_last_batch_bytes", "chn_synth_genomes", "chn_synth_fill_index", "chn_synth_plant", "chn_synth_reads",
           "chn_device_free", "chn_device_download", "chn_device_malloc", "chn_device_upload", "chn_host_alloc", "chn_host_free", "chn_shard_minimise",
           "chn_shard_probe", "chn_shard_finish", "chn_shardx_minimise", "chn_shardx_counts", "chn_shardx_queries", "chn_shardx_serve", "chn_shardx_finish", "chn_minimisers", "chn_index_emplace", "chn_hashset_create", "chn_hashset_destroy", "chn_hashset_append", "chn_minimisers_into", "chn_hashset_unique", "chn_hashset_size", "chn_hashset_download", "chn_index_emplace_set", "chn_device_memory", "chn_index_decode_ef", "chn_ef_layout_of", "chn_index_ef_layout", "chn_index_encode_ef", "chn_index_encode_ef_host", "chn_index_bin_popcounts", "chn_index_replicate", "chn_device_count", "chn_index_gather_roof", "chn_text_submit", "chn_text_wait", "chn_text_pack", "chn_text_split", "chn_text_split_host", "chn_fasta_split", "chn_fasta_split_host", "chn_text_fetch", "chn_text_fetch_host", "chn_text_pair_ids", "chn_text_pair_ids_host", "chn_device_copy", "chn_inflate_create", "chn_inflate_run",
           "chn_inflate_run_host", "chn_inflate_destroy", "chn_inflate_kernel_ms", "chn_inflate_run_crc", "chn_inflate_run_host_crc", "chn_inflate_stream_run", "chn_inflate_stream_run_host", "chn_inflate_stream_search_host", "chn_deflate_create", "chn_deflate_run", "chn_deflate_run_host",
           "chn_deflate_destroy", "chn_deflate_bound", "chn_deflate_kernel_ms", "chn_deflate_group_members", "chn_extract_create", "chn_extract_destroy",
           "chn_extract_bound", "chn_extract_append_records", "chn_extract_append_bytes", "chn_extract_finish", "chn_extract_records_host",
           "chn_extract_kernel_ms", "chn_last_error", "chn_version"]

_L.chn_last_error.restype = C.c_char_p
_L.chn_version.restype = C.c_char_p
_L.chn_index_create.argtypes = [C.POINTER(IndexDesc), C.POINTER(C.c_void_p)]
_L.chn_index_upload_rows.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
_L.chn_index_download_rows.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
_L.chn_index_device_words.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
_L.chn_index_get_desc.argtypes = [C.c_void_p, C.POINTER(IndexDesc)]
_L.chn_index_destroy.argtypes = [C.c_void_p]
_L.chn_model_default.argtypes = [C.POINTER(Model), C.c_uint32, C.c_uint8, C.c_int]
_L.chn_stream_create.argtypes = [C.c_void_p, C.POINTER(StreamCfg), C.POINTER(C.c_void_p)]
_L.chn_stream_destroy.argtypes = [C.c_void_p]
_L.chn_model_set.argtypes = [C.c_void_p, C.POINTER(Model)]
_L.chn_batch_submit.argtypes = [C.c_void_p, C.POINTER(Batch)]
_L.chn_batch_wait.argtypes = [C.c_void_p, C.POINTER(Result)]
_L.chn_stream_sync.argtypes = [C.c_void_p]
_L.chn_classify_counts.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 9
_L.chn_classify_counts_raw.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 10
_L.chn_stream_profile.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
_L.chn_stream_last_batch_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
_L.chn_synth_genomes.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]
_L.chn_synth_fill_index.argtypes = [C.c_void_p, C.c_uint64, C.c_double]
_L.chn_index_gather_roof.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
_L.chn_synth_plant.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_char_p]
_L.chn_synth_reads.argtypes = [C.c_int, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                               C.c_double, C.c_double, C.c_float, C.POINTER(SynthReadsOut)]
_L.chn_device_free.argtypes = [C.c_int, C.c_void_p]
_L.chn_device_malloc.argtypes = [C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]
_L.chn_host_alloc.argtypes = [C.c_uint64, C.POINTER(C.c_void_p)]
_L.chn_host_free.argtypes = [C.c_void_p]
_L.chn_device_upload.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]
_L.chn_shard_minimise.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(C.c_uint64)]
_L.chn_shard_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
_L.chn_shard_finish.argtypes = [C.c_void_p, C.c_void_p]
_L.chn_shardx_minimise.argtypes = [C.c_void_p, C.POINTER(Batch)]
_L.chn_shardx_counts.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
_L.chn_shardx_queries.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
_L.chn_shardx_serve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
_L.chn_shardx_finish.argtypes = [C.c_void_p, C.c_void_p]
_L.chn_minimisers.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
_L.chn_index_emplace.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
_L.chn_hashset_create.argtypes = [C.POINTER(HashSetCfg), C.POINTER(C.c_void_p)]
_L.chn_hashset_destroy.argtypes = [C.c_void_p]
_L.chn_hashset_append.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
_L.chn_minimisers_into.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(C.c_uint64)]
_L.chn_hashset_unique.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
_L.chn_hashset_size.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
_L.chn_hashset_download.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
_L.chn_index_emplace_set.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
_L.chn_device_memory.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
_L.chn_index_decode_ef.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64,
                                   C.POINTER(C.c_uint64)]
_L.chn_ef_layout_of.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(EfLayout)]
_L.chn_index_ef_layout.argtypes = [C.c_void_p, C.POINTER(EfLayout)]
_L.chn_index_encode_ef.argtypes = [C.c_void_p, C.POINTER(EfEncodeJob)]
_L.chn_index_encode_ef_host.argtypes = [C.POINTER(IndexDesc), C.c_void_p, C.POINTER(EfEncodeJob)]
_L.chn_index_bin_popcounts.argtypes = [C.c_void_p, C.c_void_p]
_L.chn_index_replicate.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
_L.chn_device_count.argtypes = [C.POINTER(C.c_int)]
_L.chn_device_download.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]
_L.chn_text_submit.argtypes = [C.c_void_p, C.c_void_p]   # a chn_text_batch or a chn_text_batch2: struct_size says which
_L.chn_text_wait.argtypes = [C.c_void_p, C.POINTER(Result), C.POINTER(TextResult)]
_L.chn_text_pack.argtypes = [C.c_void_p, C.c_void_p] + [C.c_void_p] * 5 + [C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
_L.chn_text_split.argtypes = [C.c_void_p, C.POINTER(TextSplitJob)]
_L.chn_text_split_host.argtypes = [C.POINTER(TextSplitJob)]
_L.chn_fasta_split.argtypes = [C.c_void_p, C.POINTER(FastaSplitJob)]
_L.chn_fasta_split_host.argtypes = [C.POINTER(FastaSplitJob)]
_L.chn_text_fetch.argtypes = [C.c_void_p, C.POINTER(TextFetchJob)]
_L.chn_text_fetch_host.argtypes = [C.POINTER(TextFetchJob)]
_L.chn_text_pair_ids.argtypes = [C.c_void_p, C.POINTER(TextPairJob)]
_L.chn_text_pair_ids_host.argtypes = [C.POINTER(TextPairJob)]
_L.chn_device_copy.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]
_L.chn_inflate_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
_L.chn_inflate_run.argtypes = [C.c_void_p, C.POINTER(InflateJob)]
_L.chn_inflate_run_host.argtypes = [C.POINTER(InflateJob)]
_L.chn_inflate_destroy.argtypes = [C.c_void_p]
_L.chn_inflate_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
_L.chn_inflate_run_crc.argtypes = [C.c_void_p, C.POINTER(InflateJob), C.POINTER(InflateCrc)]
_L.chn_inflate_run_host_crc.argtypes = [C.POINTER(InflateJob), C.POINTER(InflateCrc)]
_L.chn_inflate_stream_run.argtypes = [C.c_void_p, C.POINTER(InflateStreamJob)]
_L.chn_inflate_stream_run_host.argtypes = [C.POINTER(InflateStreamJob)]
_L.chn_inflate_stream_search_host.argtypes = [C.POINTER(InflateSearchJob)]
_L.chn_deflate_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
_L.chn_deflate_run.argtypes = [C.c_void_p, C.POINTER(DeflateJob)]
_L.chn_deflate_run_host.argtypes = [C.POINTER(DeflateJob)]
_L.chn_deflate_destroy.argtypes = [C.c_void_p]
_L.chn_deflate_bound.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
_L.chn_deflate_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
_L.chn_deflate_group_members.argtypes = [C.c_void_p, C.c_uint32]
_L.chn_extract_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
_L.chn_extract_destroy.argtypes = [C.c_void_p]
_L.chn_extract_bound.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
_L.chn_extract_append_records.argtypes = [C.c_void_p, C.POINTER(ExtractJob)]
_L.chn_extract_append_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
_L.chn_extract_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
_L.chn_extract_records_host.argtypes = [C.POINTER(ExtractJob), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
_L.chn_extract_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]


E_INVALID, E_HIP, E_NOMEM, E_STATE, E_CAPACITY = -1, -2, -3, -4, -5  # CHN_E_*


class ChnError(RuntimeError):
    code = 0  # the CHN_E_* value


def _chk(rc):
    if rc != 0:
        e = ChnError("libcharon_hip error %d: %s" % (rc, _L.chn_last_error().decode()))
        e.code = rc
        raise e


def lib():
    return _L


def version():
    return _L.chn_version().decode()


def clz64(x):
    return 64 - int(x).bit_length()


def make_desc(bins, bin_size, bin_to_cat, num_categories, host_index, k=19, w=41, hash_funs=3, device=0,
              row_begin=0, row_end=0):
    d = IndexDesc()
    d.struct_size = C.sizeof(IndexDesc)
    d.device = device
    d.kmer_size, d.window_size, d.hash_funs = k, w, hash_funs
    d.num_categories, d.host_index = num_categories, host_index
    d.minimiser_seed = MINIMISER_SEED
    d.bins = bins
    d.bin_words = (bins + 63) // 64
    d.technical_bins = d.bin_words * 64
    d.bin_size = bin_size
    d.hash_shift = clz64(bin_size)
    for b in range(bins):
        d.bin_to_category[b] = int(bin_to_cat[b])
    d.row_begin, d.row_end = row_begin, row_end
    return d


class Index:
    def __init__(self, desc):
        self.desc = desc
        self.h = C.c_void_p()
        _chk(_L.chn_index_create(C.byref(desc), C.byref(self.h)))

    @property
    def device(self):
        return self.desc.device

    def upload(self, words, row_begin=0):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        n_rows = words.size // self.desc.bin_words
        _chk(_L.chn_index_upload_rows(self.h, row_begin, n_rows, words.ctypes.data))

    def download(self, row_begin=0, n_rows=None):
        n_rows = self.desc.bin_size if n_rows is None else n_rows
        out = np.zeros(n_rows * self.desc.bin_words, np.uint64)
        _chk(_L.chn_index_download_rows(self.h, row_begin, n_rows, out.ctypes.data))
        return out

    def device_words(self):
        p, n = C.c_void_p(), C.c_uint64()
        _chk(_L.chn_index_device_words(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def decode_ef(self, m_size, wl, high, high_bits, low, slice_words=1 << 20):
        """decode a whole sd_vector (numpy uint64 arrays `high` with `high_bits` valid bits, `low` packed wl-bit elements) on the
        device in slices of `slice_words` words of m_high; returns the number of ill-placed bits (0 for a well-formed vector)"""
        high = np.ascontiguousarray(high, np.uint64)
        low = np.ascontiguousarray(low, np.uint64)
        n_high = (high_bits + 63) // 64
        ones_before, bad_total = 0, 0
        for w0 in range(0, n_high, slice_words):
            hs = high[w0:min(n_high, w0 + slice_words)]
            ones = int(sum(bin(int(x)).count("1") for x in hs)) if hs.size < 4096 else int(np.unpackbits(hs.view(np.uint8)).sum())
            if ones == 0:
                continue
            elem0 = ones_before & ~63  # a multiple of 64 elements starts on a word boundary whatever wl is
            lw0 = elem0 * wl // 64
            lw1 = ((ones_before + ones) * wl + 63) // 64
            ls = low[lw0:min(low.size, lw1)]
            bad = C.c_uint64()
            _chk(_L.chn_index_decode_ef(self.h, m_size, wl, hs.ctypes.data, w0 * 64, hs.size, ones_before, ls.ctypes.data if ls.size else None,
                                        elem0, ls.size, C.byref(bad)))
            bad_total += bad.value
            ones_before += ones
        bad = C.c_uint64()  # the closing call: waits for the slices in flight and reports the ill-placed bits they met
        _chk(_L.chn_index_decode_ef(self.h, m_size, wl, high.ctypes.data if high.size else np.zeros(1, np.uint64).ctypes.data, 0, 0, 0, None, 0, 0, C.byref(bad)))
        return bad_total + bad.value

    def ef_layout(self):
        """chn_index_ef_layout: the sd_vector layout of this index (its set bits are counted on the device)"""
        lay = EfLayout()
        _chk(_L.chn_index_ef_layout(self.h, C.byref(lay)))
        return lay

    def encode_ef(self, slice_rows=0, layout=None):
        """chn_index_encode_ef: (layout, low, high, device_ms) -- m_low and m_high of the whole index as numpy uint64 arrays, encoded on
        the device in slices of `slice_rows` rows (0: 256 MiB of rows)"""
        lay = self.ef_layout() if layout is None else layout
        job, low, high = ef_encode_job(lay, slice_rows)
        _chk(_L.chn_index_encode_ef(self.h, C.byref(job)))
        return lay, low, high, job.device_ms

    def bin_popcounts(self):
        out = np.zeros(self.desc.technical_bins, np.uint64)
        _chk(_L.chn_index_bin_popcounts(self.h, out.ctypes.data))
        return out

    def replicate(self, device):
        """an independent copy of this index on `device` (chn_index_replicate: the copy is queued; this index must stay alive and
        unwritten until a call on the replica that waits for it -- bin_popcounts, download, ... -- has returned)"""
        h = C.c_void_p()
        _chk(_L.chn_index_replicate(self.h, device, C.byref(h)))
        rep = Index.__new__(Index)
        rep.desc = IndexDesc.from_buffer_copy(self.desc)
        rep.desc.device = device
        rep.h = h
        return rep

    def emplace(self, values, bin_index):
        values = np.ascontiguousarray(values, dtype=np.uint64)
        _chk(_L.chn_index_emplace(self.h, values.ctypes.data, values.size, bin_index))

    def emplace_set(self, hashset, bin_index):
        """chn_index_emplace_set: emplace every value of the device-resident set, read in place"""
        _chk(_L.chn_index_emplace_set(self.h, hashset.h, bin_index))

    def gather_roof(self, nt=True):
        """row fetches per second this device sustains for nothing but random probes of this index (measurement aid)"""
        r = C.c_double()
        _chk(_L.chn_index_gather_roof(self.h, 1 if nt else 0, C.byref(r)))
        return r.value

    def synth_fill(self, seed, density):
        _chk(_L.chn_synth_fill_index(self.h, seed, density))

    def synth_plant(self, dev_genomes, n_genomes, genome_len, genome_bin):
        _chk(_L.chn_synth_plant(self.h, dev_genomes, n_genomes, genome_len, bytes(bytearray(int(b) for b in genome_bin))))

    def destroy(self):
        if self.h:
            _L.chn_index_destroy(self.h)
            self.h = None


class HashSet:
    """chn_hashset: 64-bit values in device memory (tile_keys: test hook, 0 = default)"""

    def __init__(self, device=0, tile_keys=0):
        cfg = HashSetCfg(C.sizeof(HashSetCfg), device, tile_keys, 0)
        self.h = C.c_void_p()
        _chk(_L.chn_hashset_create(C.byref(cfg), C.byref(self.h)))

    def append(self, values):
        values = np.ascontiguousarray(values, dtype=np.uint64)
        _chk(_L.chn_hashset_append(self.h, values.ctypes.data if values.size else None, values.size))

    def unique(self):
        """sort ascending and drop repeats; returns the number of distinct values"""
        n = C.c_uint64()
        _chk(_L.chn_hashset_unique(self.h, C.byref(n)))
        return n.value

    def size(self):
        """(values held, device bytes held)"""
        n, b = C.c_uint64(), C.c_uint64()
        _chk(_L.chn_hashset_size(self.h, C.byref(n), C.byref(b)))
        return n.value, b.value

    def download(self, first=0, n=None):
        n = self.size()[0] - first if n is None else n
        out = np.zeros(max(n, 0), np.uint64)
        _chk(_L.chn_hashset_download(self.h, first, n, out.ctypes.data if out.size else None))
        return out

    def destroy(self):
        if self.h:
            _L.chn_hashset_destroy(self.h)
            self.h = None


def device_memory(device=0):
    """chn_device_memory: (free bytes, total bytes) of a device"""
    f, t = C.c_uint64(), C.c_uint64()
    _chk(_L.chn_device_memory(device, C.byref(f), C.byref(t)))
    return f.value, t.value


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)  # set bits of a byte


def ef_layout_of(m_size, ones):
    """chn_ef_layout_of: the sd_vector layout of m_size bits with `ones` set bits (the pure rule; no GPU)"""
    lay = EfLayout()
    _chk(_L.chn_ef_layout_of(m_size, ones, C.byref(lay)))
    return lay


def ef_encode_job(layout, slice_rows=0, low=None, high=None):
    """a chn_ef_encode_job for `layout` with arrays of the layout's sizes (filled with ones where this makes them: the call writes every word)"""
    low = np.full(layout.n_low_words, 2 ** 64 - 1, np.uint64) if low is None else low
    high = np.full(layout.n_high_words, 2 ** 64 - 1, np.uint64) if high is None else high
    job = EfEncodeJob()
    job.struct_size = C.sizeof(EfEncodeJob)
    job.slice_rows = slice_rows
    job.layout = C.pointer(layout)
    job.low, job.n_low_words = (low.ctypes.data if low.size else None), low.size
    job.high, job.n_high_words = (high.ctypes.data if high.size else None), high.size
    return job, low, high


def encode_ef_host(desc, words, slice_rows=0, layout=None):
    """chn_index_encode_ef_host: (layout, low, high, device_ms = 0) of the plain rows `words` of a whole index described by `desc`, on one
    CPU thread (no GPU), in the slices chn_index_encode_ef walks"""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    if words.size != desc.bin_size * desc.bin_words:
        raise ValueError("encode_ef_host: %d words, the index has %d" % (words.size, desc.bin_size * desc.bin_words))
    lay = ef_layout_of(desc.technical_bins * desc.bin_size, int(_POP8[words.view(np.uint8)].sum(dtype=np.uint64))) if layout is None else layout
    job, low, high = ef_encode_job(lay, slice_rows)
    _chk(_L.chn_index_encode_ef_host(C.byref(desc), words.ctypes.data, C.byref(job)))
    return lay, low, high, job.device_ms


DIST = {"kde": 0, "gamma": 1, "beta": 2}
# Model defaults of include/classify_stats.hpp:265-268: gamma (shape, loc, scale), beta (alpha, beta, -)
DIST_DEFAULTS = {"gamma": ((25.0, 0.0, 0.02), (10.0, 0.0, 0.005)), "beta": ((6.0, 4.0, 0.0), (6.0, 40.0, 0.0))}


def default_model(num_categories, host_index, paired=False, dist="kde", pos_params=None, neg_params=None, **overrides):
    """paired=True selects call_category (paired dehost, every classify run).  dist gamma / beta: per-category parameter triples
    (default: the reference's) instead of the KDE datasets."""
    m = Model()
    _chk(_L.chn_model_default(C.byref(m), num_categories, host_index, 1 if paired else 0))
    if dist != "kde":
        pp = np.ascontiguousarray(pos_params if pos_params is not None else [DIST_DEFAULTS[dist][0]] * num_categories, np.float32)
        nn = np.ascontiguousarray(neg_params if neg_params is not None else [DIST_DEFAULTS[dist][1]] * num_categories, np.float32)
        m._keep = (pp, nn)
        m.dist = DIST[dist]
        m.pos_params = pp.ctypes.data_as(C.POINTER(C.c_float))
        m.neg_params = nn.ctypes.data_as(C.POINTER(C.c_float))
    for k, v in overrides.items():
        setattr(m, k, v)
    return m


class Stream:
    def __init__(self, index, max_reads, max_bases, profile=False, tiny_log=False, split_bucket=0, probe_gate=True):
        """probe_gate=False (testing): CHN_STREAM_NO_PROBE_GATE, consecutive probe grids share the device from their first workgroup on.
        split_bucket (testing): length class from which single-end reads are cut over the 64 lanes of a wavefront
        (CHN_STREAM_SPLIT_BUCKET: 0 = default, 32 768 bases; 64 = 1 024 bases; 255 = never)"""
        self.index = index
        cfg = StreamCfg(C.sizeof(StreamCfg), (STREAM_PROFILE if profile else 0) | (STREAM_TINY_LOG if tiny_log else 0) | (0 if probe_gate else STREAM_NO_PROBE_GATE) |
                        ((split_bucket & 0xff) << 8),
                        max_reads, max_bases)
        self.h = C.c_void_p()
        _chk(_L.chn_stream_create(index.h, C.byref(cfg), C.byref(self.h)))
        self.C = index.desc.num_categories
        self._fifo = []  # (n_reads, keep-alive host arrays) of the batches in flight

    def set_model(self, model):
        _chk(_L.chn_model_set(self.h, C.byref(model)))

    def submit_host(self, packed, mean_quality=None, compression=None, gzip_tallies=0, gzip_output=0):
        """packed: dict from charon_amd.pack.pack_reads; gzip_tallies: longest read to tally on the device (0 = off);
        gzip_output: 0 tallies, 1 gzip member sizes (tree arithmetic on the device as well), 2 both,
        3 (GZIP_SIZES_ALL) the size of every read up to gzip_tallies letters, whatever its length (GZIP_ANY_LEN: no bound)"""
        b, keep, n = self._host_batch(packed, mean_quality, compression)
        b.gzip_tallies, b.gzip_output = gzip_tallies, gzip_output
        _chk(_L.chn_batch_submit(self.h, C.byref(b)))
        self._fifo.append((n, keep, gzip_tallies, gzip_output))

    def _host_batch(self, packed, mean_quality, compression):
        n = len(packed["seg1_length"])
        b = Batch()
        b.struct_size, b.on_device, b.n_reads, b.n_bases = C.sizeof(Batch), 0, n, packed["n_bases"]
        keep = []

        def ptr(a, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            keep.append(a)
            return a.ctypes.data

        b.bases2 = ptr(packed["bases2"], np.uint32)
        b.nmask = ptr(packed.get("nmask"), np.uint32)
        b.seg1_offset = ptr(packed["seg1_offset"], np.uint64)
        b.seg1_length = ptr(packed["seg1_length"], np.uint32)
        b.seg2_offset = ptr(packed.get("seg2_offset"), np.uint64)
        b.seg2_length = ptr(packed.get("seg2_length"), np.uint32)
        b.mean_quality = ptr(mean_quality, np.float32)
        b.compression = ptr(compression, np.float32)
        return b, keep, n

    def minimisers_host(self, packed):
        """all minimisers of the batch (with repeats) as a uint64 array"""
        b, keep, n = self._host_batch(packed, None, None)
        cap = int(packed["n_bases"])
        out = np.zeros(max(cap, 1), np.uint64)
        e = C.c_uint64()
        _chk(_L.chn_minimisers(self.h, C.byref(b), out.ctypes.data, cap, C.byref(e)))
        return out[:e.value]

    def minimisers_into(self, packed, hashset):
        """chn_minimisers_into: the batch's minimisers (with repeats) appended to the device-resident set; returns how many"""
        b, keep, n = self._host_batch(packed, None, None)
        e = C.c_uint64()
        _chk(_L.chn_minimisers_into(self.h, C.byref(b), hashset.h, C.byref(e)))
        return e.value

    # ---- row-sharded mode (see include/charon_hip.h) ----
    def shard_minimise_host(self, packed, mean_quality=None, compression=None):
        b, keep, n = self._host_batch(packed, mean_quality, compression)
        e = C.c_uint64()
        _chk(_L.chn_shard_minimise(self.h, C.byref(b), C.byref(e)))
        self._shard = (n, keep)
        return e.value

    def shard_minimise_device(self, n_reads, n_bases, bases2, seg1_offset, seg1_length, mean_quality=None, compression=None):
        b = Batch()
        b.struct_size, b.on_device, b.n_reads, b.n_bases = C.sizeof(Batch), 1, n_reads, n_bases
        b.bases2, b.seg1_offset, b.seg1_length, b.mean_quality, b.compression = bases2, seg1_offset, seg1_length, mean_quality, compression
        e = C.c_uint64()
        _chk(_L.chn_shard_minimise(self.h, C.byref(b), C.byref(e)))
        self._shard = (n_reads, None)
        return e.value

    def shard_probe(self, shard_index, dev_partial, capacity_words):
        _chk(_L.chn_shard_probe(self.h, shard_index.h, dev_partial, capacity_words))

    def shard_finish(self, dev_partial):
        _chk(_L.chn_shard_finish(self.h, dev_partial))
        self._fifo.append(self._shard)
        self._shard = None

    # ---- row-sharded mode, sparse exchange (see include/charon_hip.h) ----
    def shardx_minimise_host(self, packed, mean_quality=None, compression=None):
        b, keep, n = self._host_batch(packed, mean_quality, compression)
        _chk(_L.chn_shardx_minimise(self.h, C.byref(b)))
        self._shard = (n, keep)

    def shardx_minimise_device(self, n_reads, n_bases, bases2, seg1_offset, seg1_length, mean_quality=None, compression=None):
        b = Batch()
        b.struct_size, b.on_device, b.n_reads, b.n_bases = C.sizeof(Batch), 1, n_reads, n_bases
        b.bases2, b.seg1_offset, b.seg1_length, b.mean_quality, b.compression = bases2, seg1_offset, seg1_length, mean_quality, compression
        _chk(_L.chn_shardx_minimise(self.h, C.byref(b)))
        self._shard = (n_reads, None)

    def shardx_counts(self, row_splits):
        sp = np.ascontiguousarray(row_splits, dtype=np.uint64)
        n_ranks = sp.size - 1
        counts = np.zeros(n_ranks, np.uint64)
        total = C.c_uint64()
        _chk(_L.chn_shardx_counts(self.h, n_ranks, sp.ctypes.data, C.byref(total), counts.ctypes.data))
        return total.value, [int(x) for x in counts]

    def shardx_queries(self, dev_queries, capacity):
        _chk(_L.chn_shardx_queries(self.h, dev_queries, capacity))

    def shardx_serve(self, shard_index, dev_queries_in, n_in, dev_rows_out):
        _chk(_L.chn_shardx_serve(self.h, shard_index.h, dev_queries_in, n_in, dev_rows_out))

    def shardx_finish(self, dev_rows_back):
        _chk(_L.chn_shardx_finish(self.h, dev_rows_back))
        self._fifo.append(self._shard)
        self._shard = None

    def submit_device(self, n_reads, n_bases, bases2, seg1_offset, seg1_length, mean_quality=None, compression=None,
                      nmask=None, seg2_offset=None, seg2_length=None, gzip_tallies=0, gzip_output=0):
        b = Batch()
        b.struct_size, b.on_device, b.n_reads, b.n_bases = C.sizeof(Batch), 1, n_reads, n_bases
        b.bases2, b.nmask, b.seg1_offset, b.seg1_length = bases2, nmask, seg1_offset, seg1_length
        b.seg2_offset, b.seg2_length, b.mean_quality, b.compression = seg2_offset, seg2_length, mean_quality, compression
        b.gzip_tallies, b.gzip_output = gzip_tallies, gzip_output
        _chk(_L.chn_batch_submit(self.h, C.byref(b)))
        self._fifo.append((n_reads, None, gzip_tallies, gzip_output))

    # ---- text batches (see include/charon_hip.h) ----
    def _text_batch(self, tb, compression=None, gzip_tallies=0, gzip_output=0, text_device=None, text2_device=None):
        """tb: dict from charon_amd.pack.text_batch (text may be any uint8 array, e.g. a pinned_array).  text_device: (device pointer,
        text_bytes) of the same text in device memory -- CHN_TEXT_ON_DEVICE; tb["text"] is then not looked at.  text2_device: (device
        pointer, text2_bytes) of a second device text that holds mate 2: seq2_offset / qual2_offset are then bytes into it"""
        t = TextBatch() if text2_device is None else TextBatch2()
        n = len(tb["seq1_length"])
        t.struct_size, t.flags, t.n_reads = C.sizeof(t), tb.get("flags", 0) | (TEXT_ON_DEVICE if text_device is not None else 0), n
        keep = []

        def ptr(a, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            keep.append(a)
            return a.ctypes.data

        if text_device is not None:
            t.text, t.text_bytes = text_device
        else:
            text = tb["text"]
            t.text, t.text_bytes = ptr(text, np.uint8) if len(text) else None, tb.get("text_bytes", len(text))
        for k, dt in (("seq1_offset", np.uint64), ("seq1_length", np.uint32), ("qual1_offset", np.uint64), ("qual1_length", np.uint32),
                      ("seq2_offset", np.uint64), ("seq2_length", np.uint32), ("qual2_offset", np.uint64), ("qual2_length", np.uint32)):
            setattr(t, k, ptr(tb.get(k), dt))
        t.compression = ptr(compression, np.float32)
        t.gzip_tallies, t.gzip_output = gzip_tallies, gzip_output
        if text2_device is not None:
            t.text2, t.text2_bytes = text2_device
        return t, keep, n

    def submit_text(self, tb, compression=None, gzip_tallies=0, gzip_output=0, text_device=None, text2_device=None):
        """chn_text_submit: the text and the descriptor arrays may be reused as soon as this returns.  text_device, text2_device: see
        _text_batch"""
        t, keep, n = self._text_batch(tb, compression, gzip_tallies, gzip_output, text_device, text2_device)
        _chk(_L.chn_text_submit(self.h, C.byref(t)))
        self._fifo.append((n, None, gzip_tallies, gzip_output))

    def wait_text(self):
        """chn_text_wait: the dict of wait_host plus mean_quality, has_n, n_bases"""
        n = self._fifo[0][0]
        mq = np.zeros(n, np.float32)
        tr = TextResult(C.sizeof(TextResult), 0, 0, mq.ctypes.data)
        out = self.wait_host(tr)
        out["mean_quality"], out["has_n"], out["n_bases"] = mq, int(tr.has_n), int(tr.n_bases)
        return out

    def text_pack(self, tb, text_device=None, text2_device=None):
        """chn_text_pack: the packed form of a text batch as the dict pack.pack_reads returns (nmask always an array) plus
        mean_quality and has_n.  text_device, text2_device: see _text_batch"""
        t, keep, n = self._text_batch(tb, text_device=text_device, text2_device=text2_device)
        nb, hn = C.c_uint64(), C.c_uint32()
        _chk(_L.chn_text_pack(self.h, C.byref(t), None, None, None, None, None, C.byref(nb), C.byref(hn)))  # layout only: sizes the arrays
        paired = tb.get("seq2_offset") is not None
        out = dict(bases2=np.zeros(nb.value // 16, np.uint32), nmask=np.zeros(nb.value // 32, np.uint32), seg1_offset=np.zeros(n, np.uint64),
                   seg1_length=np.array(tb["seq1_length"], np.uint32), seg2_offset=np.zeros(n, np.uint64) if paired else None,
                   seg2_length=np.array(tb["seq2_length"], np.uint32) if paired else None, mean_quality=np.zeros(n, np.float32))
        _chk(_L.chn_text_pack(self.h, C.byref(t), out["bases2"].ctypes.data, out["nmask"].ctypes.data, out["seg1_offset"].ctypes.data,
                              out["seg2_offset"].ctypes.data if paired else None, out["mean_quality"].ctypes.data, C.byref(nb), C.byref(hn)))
        out["n_bases"], out["has_n"] = int(nb.value), int(hn.value)
        return out

    def text_split(self, dev_ptr, nbytes, start=0, max_records=None, want_ids=True, ids_capacity=None):
        """chn_text_split: the FASTQ records of device text [start, nbytes) -- see text_split_host for what comes back"""
        j, a = text_split_job(dev_ptr, nbytes, start, max_records, want_ids, ids_capacity)
        _chk(_L.chn_text_split(self.h, C.byref(j)))
        return _text_split_results(j, a)

    def fasta_split(self, dev_ptr, nbytes, seq_ptr, seq_capacity, start=0, max_records=None, want_ids=True, ids_capacity=None, end_of_input=False):
        """chn_fasta_split: the FASTA records of device text [start, nbytes), their letters unwrapped into the device buffer at seq_ptr
        -- see fasta_split_host for what comes back (seq_text stays on the device and is not part of it)"""
        j, a = fasta_split_job(dev_ptr, nbytes, seq_ptr, seq_capacity, start, max_records, want_ids, ids_capacity, end_of_input)
        _chk(_L.chn_fasta_split(self.h, C.byref(j)))
        return _fasta_split_results(j, a)

    def text_fetch(self, dev_ptr, nbytes, offsets, lengths, out=None, out_capacity=None):
        """chn_text_fetch: the byte ranges of device text [0, nbytes) back to back -- see text_fetch_host for what comes back"""
        j, keep = text_fetch_job(dev_ptr, nbytes, offsets, lengths, out, out_capacity)
        _chk(_L.chn_text_fetch(self.h, C.byref(j)))
        return keep[2][:int(j.out_bytes)]

    def pair_ids(self, dev1, nbytes1, dev2, nbytes2, id1_offset, id1_length, id2_offset, id2_length):
        """chn_text_pair_ids: the smallest pair whose ids in the two device texts disagree, the number of pairs if none does -- see
        pair_ids_host for the rule"""
        j, keep = text_pair_job(dev1, nbytes1, dev2, nbytes2, id1_offset, id1_length, id2_offset, id2_length)
        _chk(_L.chn_text_pair_ids(self.h, C.byref(j)))
        return int(j.first_mismatch)

    def wait_host(self, text_result=None):
        n, Cn = self._fifo[0][0], self.C
        out = dict(num_hashes=np.zeros(n, np.uint32), counts=np.zeros((n, Cn), np.uint32), unique=np.zeros((n, Cn), np.uint32),
                   probs=np.zeros((n, Cn), np.float64), call=np.zeros(n, np.uint8), conf=np.zeros(n, np.uint8),
                   flags=np.zeros(n, np.uint8))
        want_gz = len(self._fifo[0]) > 2 and self._fifo[0][2]
        gz_out = self._fifo[0][3] if len(self._fifo[0]) > 3 else 0
        if want_gz and gz_out in (GZIP_TALLIES, GZIP_BOTH):
            out["gzip_tallies"] = np.zeros((n, 320), np.uint16)
        if want_gz and gz_out != 0:
            out["gzip_sizes"] = np.zeros(n, np.uint32)
        r = Result(C.sizeof(Result), 0, out["num_hashes"].ctypes.data, out["counts"].ctypes.data, out["unique"].ctypes.data,
                   out["probs"].ctypes.data, out["call"].ctypes.data, out["conf"].ctypes.data, out["flags"].ctypes.data,
                   out["gzip_tallies"].ctypes.data if "gzip_tallies" in out else None,
                   out["gzip_sizes"].ctypes.data if "gzip_sizes" in out else None)
        self._waited(_L.chn_text_wait(self.h, C.byref(r), C.byref(text_result)) if text_result is not None else
                     _L.chn_batch_wait(self.h, C.byref(r)))
        return out

    def _waited(self, rc):
        """A wait that reports the batch's failure has still taken the batch off the stream (only a call-sequence error leaves it in
        flight): the next wait must size its arrays for the next batch."""
        if rc != E_STATE and self._fifo:
            self._fifo.pop(0)
        _chk(rc)

    def wait_device(self):
        r = Result()
        r.struct_size, r.on_device = C.sizeof(Result), 1
        self._waited(_L.chn_batch_wait(self.h, C.byref(r)))
        return r

    def sync(self):
        _chk(_L.chn_stream_sync(self.h))

    def _counts_args(self, num_hashes, counts, unique, lengths, mean_quality, compression):
        n, Cn = len(num_hashes), self.C
        a = [np.ascontiguousarray(x, dt) for x, dt in ((num_hashes, np.uint32), (counts, np.uint32), (unique, np.uint32),
                                                       (lengths, np.uint32), (mean_quality, np.float32), (compression, np.float32))]
        out = dict(probs=np.zeros((n, Cn), np.float64), call=np.zeros(n, np.uint8), conf=np.zeros(n, np.uint8))
        return n, a, out

    def classify_counts(self, num_hashes, counts, unique, lengths, mean_quality, compression):
        n, a, out = self._counts_args(num_hashes, counts, unique, lengths, mean_quality, compression)
        _chk(_L.chn_classify_counts(self.h, n, *[x.ctypes.data for x in a], out["probs"].ctypes.data, out["call"].ctypes.data,
                                    out["conf"].ctypes.data))
        return out

    def classify_counts_raw(self, num_hashes, counts, unique, lengths, mean_quality, compression):
        """k_model_call's own outputs on the given counts (no host re-evaluation): probs, call, conf, flags"""
        n, a, out = self._counts_args(num_hashes, counts, unique, lengths, mean_quality, compression)
        out["flags"] = np.zeros(n, np.uint8)
        _chk(_L.chn_classify_counts_raw(self.h, n, *[x.ctypes.data for x in a], out["probs"].ctypes.data, out["call"].ctypes.data,
                                        out["conf"].ctypes.data, out["flags"].ctypes.data))
        return out

    def profile(self, which, reset=False):
        ms, n = C.c_double(), C.c_uint64()
        _chk(_L.chn_stream_profile(self.h, which, C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, n.value

    def last_batch_bytes(self):
        b, m = C.c_uint64(), C.c_uint64()
        _chk(_L.chn_stream_last_batch_bytes(self.h, C.byref(b), C.byref(m)))
        return b.value, m.value

    def destroy(self):
        if self.h:
            _L.chn_stream_destroy(self.h)
            self.h = None


# ---- FASTQ records of a text (see include/charon_hip.h) ----
def text_split_job(text_ptr, nbytes, start=0, max_records=None, want_ids=True, ids_capacity=None):
    """the chn_text_split_job of the text at `text_ptr`.  max_records defaults to the most records the text can hold (one per 8
    bytes: callers with large texts pass what they expect), ids_capacity to the bytes behind `start`.  Returns (job, arrays)."""
    nbytes, start = int(nbytes), int(start)
    if max_records is None:
        max_records = max(nbytes - start, 0) // 8
    m = max(int(max_records), 1)
    a = dict(id_offset=np.zeros(m, np.uint64), id_length=np.zeros(m, np.uint32), seq_offset=np.zeros(m, np.uint64),
             seq_length=np.zeros(m, np.uint32), qual_offset=np.zeros(m, np.uint64), ids=None)
    j = TextSplitJob()
    j.struct_size, j.flags, j.text, j.text_bytes, j.start, j.max_records = C.sizeof(TextSplitJob), 0, text_ptr, nbytes, start, int(max_records)
    for k in ("id_offset", "id_length", "seq_offset", "seq_length", "qual_offset"):
        setattr(j, k, a[k].ctypes.data)
    if want_ids:
        cap = max(nbytes - start, 0) if ids_capacity is None else int(ids_capacity)
        a["ids"] = np.zeros(max(cap, 1), np.uint8)
        j.ids, j.ids_capacity = a["ids"].ctypes.data, cap
    return j, a


def _text_split_results(j, a):
    n = int(j.n_records)
    out = {k: a[k][:n].copy() for k in ("id_offset", "id_length", "seq_offset", "seq_length", "qual_offset")}
    out.update(n_records=n, consumed=int(j.consumed), ids_bytes=int(j.ids_bytes),
               ids=a["ids"][:int(j.ids_bytes)].tobytes() if a["ids"] is not None else None)
    return out


def text_split_host(data, start=0, max_records=None, want_ids=True, ids_capacity=None, nbytes=None):
    """chn_text_split_host: the rule the GPU runs, on the CPU, over `data` (bytes or a uint8 array).  Returns a dict: n_records,
    consumed, ids_bytes, the descriptor arrays id_offset / id_length / seq_offset / seq_length / qual_offset cut to n_records, and
    ids (the id bytes back to back, None without want_ids)."""
    buf = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
    nbytes = buf.size if nbytes is None else nbytes
    j, a = text_split_job(buf.ctypes.data if buf.size else None, nbytes, start, max_records, want_ids, ids_capacity)
    _chk(_L.chn_text_split_host(C.byref(j)))
    return _text_split_results(j, a)


# ---- FASTA records of a text (see include/charon_hip.h) ----
FASTA_KEYS = ("id_offset", "id_length", "seq_offset", "seq_length")


def fasta_split_job(text_ptr, nbytes, seq_ptr, seq_capacity, start=0, max_records=None, want_ids=True, ids_capacity=None, end_of_input=False):
    """the chn_fasta_split_job of the text at `text_ptr` with the letters going to `seq_ptr`.  max_records defaults to the most records
    the text can hold (one per 3 bytes: callers with large texts pass what they expect), ids_capacity to the bytes behind `start`.
    Returns (job, arrays)."""
    nbytes, start = int(nbytes), int(start)
    if max_records is None:
        max_records = max(nbytes - start, 0) // 3
    m = max(int(max_records), 1)
    a = dict(id_offset=np.zeros(m, np.uint64), id_length=np.zeros(m, np.uint32), seq_offset=np.zeros(m, np.uint64),
             seq_length=np.zeros(m, np.uint32), ids=None)
    j = FastaSplitJob()
    j.struct_size, j.flags, j.text, j.text_bytes = C.sizeof(FastaSplitJob), FASTA_SPLIT_END_OF_INPUT if end_of_input else 0, text_ptr, nbytes
    j.start, j.max_records, j.seq_text, j.seq_capacity = start, int(max_records), seq_ptr, int(seq_capacity)
    for k in FASTA_KEYS:
        setattr(j, k, a[k].ctypes.data)
    if want_ids:
        cap = max(nbytes - start, 0) if ids_capacity is None else int(ids_capacity)
        a["ids"] = np.zeros(max(cap, 1), np.uint8)
        j.ids, j.ids_capacity = a["ids"].ctypes.data, cap
    return j, a


def _fasta_split_results(j, a):
    n = int(j.n_records)
    out = {k: a[k][:n].copy() for k in FASTA_KEYS}
    out.update(n_records=n, consumed=int(j.consumed), ids_bytes=int(j.ids_bytes), seq_bytes=int(j.seq_bytes),
               ids=a["ids"][:int(j.ids_bytes)].tobytes() if a["ids"] is not None else None)
    return out


def fasta_split_host(data, start=0, max_records=None, want_ids=True, ids_capacity=None, nbytes=None, end_of_input=False, seq_capacity=None):
    """chn_fasta_split_host: the rule the GPU runs, on the CPU, over `data` (bytes or a uint8 array).  Returns a dict: n_records,
    consumed, ids_bytes, seq_bytes, the descriptor arrays id_offset / id_length / seq_offset / seq_length cut to n_records, ids (the id
    bytes back to back, None without want_ids), seq_text (the letters of the taken records back to back, as bytes) and seq_tail_untouched."""
    buf = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
    nbytes = buf.size if nbytes is None else nbytes
    if seq_capacity is None:
        seq_capacity = (max(nbytes - start, 0) + 15) & ~15
    seq = np.full(max(int(seq_capacity), 1), 0xA5, np.uint8)
    j, a = fasta_split_job(buf.ctypes.data if buf.size else None, nbytes, seq.ctypes.data, seq_capacity, start, max_records, want_ids, ids_capacity,
                           end_of_input)
    _chk(_L.chn_fasta_split_host(C.byref(j)))
    out = _fasta_split_results(j, a)
    out["seq_text"] = seq[:out["seq_bytes"]].tobytes()
    out["seq_tail_untouched"] = bool((seq[out["seq_bytes"]:] == 0xA5).all())  # the buffer was filled with 0xA5: nothing behind the letters is written
    return out


# ---- byte ranges of a text (see include/charon_hip.h) ----
def text_fetch_job(text_ptr, nbytes, offsets, lengths, out=None, out_capacity=None):
    """the chn_text_fetch_job of ranges (offsets[i], lengths[i]) of the text at `text_ptr`.  `out` is a uint8 array to fill (pageable
    or from pinned_array) and defaults to a fresh one of the bytes needed; out_capacity defaults to its size.  Returns (job, arrays
    to keep alive: offsets, lengths, out)."""
    off, ln = np.ascontiguousarray(offsets, np.uint64), np.ascontiguousarray(lengths, np.uint32)
    if off.shape != ln.shape or off.ndim != 1:
        raise ValueError("offsets and lengths must be one-dimensional and of one size")
    if out_capacity is None:
        out_capacity = int(ln.sum(dtype=np.uint64)) if out is None else out.size
    if out is None:
        out = np.zeros(max(int(out_capacity), 1), np.uint8)
    j = TextFetchJob()
    j.struct_size, j.flags, j.text, j.text_bytes, j.n_ranges = C.sizeof(TextFetchJob), 0, text_ptr, int(nbytes), off.size
    j.offset, j.length, j.out, j.out_capacity = off.ctypes.data, ln.ctypes.data, out.ctypes.data, int(out_capacity)
    return j, (off, ln, out)


def text_fetch_host(data, offsets, lengths, out=None, out_capacity=None, nbytes=None):
    """chn_text_fetch_host: the copy rule the GPU runs, on the CPU, over `data` (bytes or a uint8 array).  Returns the uint8 array of
    the ranges back to back (a view of `out` where that is given)."""
    buf = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
    nbytes = buf.size if nbytes is None else nbytes
    j, keep = text_fetch_job(buf.ctypes.data if buf.size else None, nbytes, offsets, lengths, out, out_capacity)
    _chk(_L.chn_text_fetch_host(C.byref(j)))
    return keep[2][:int(j.out_bytes)]


# ---- the ids of the two mates of every pair (see include/charon_hip.h) ----
def text_pair_job(text1_ptr, nbytes1, text2_ptr, nbytes2, id1_offset, id1_length, id2_offset, id2_length):
    """the chn_text_pair_job of pairs whose ids are (id1_offset[i], id1_length[i]) in the text at `text1_ptr` and (id2_offset[i],
    id2_length[i]) in the text at `text2_ptr`.  Returns (job, arrays to keep alive)."""
    keep = (np.ascontiguousarray(id1_offset, np.uint64), np.ascontiguousarray(id1_length, np.uint32),
            np.ascontiguousarray(id2_offset, np.uint64), np.ascontiguousarray(id2_length, np.uint32))
    if any(a.ndim != 1 or a.size != keep[0].size for a in keep):
        raise ValueError("the four id arrays must be one-dimensional and of one size")
    j = TextPairJob()
    j.struct_size, j.flags, j.n_pairs = C.sizeof(TextPairJob), 0, keep[0].size
    j.text1, j.text1_bytes, j.text2, j.text2_bytes = text1_ptr, int(nbytes1), text2_ptr, int(nbytes2)
    j.id1_offset, j.id1_length, j.id2_offset, j.id2_length = (a.ctypes.data for a in keep)
    j.first_mismatch = 0xDEADBEEF
    return j, keep


def pair_ids_host(data1, data2, id1_offset, id1_length, id2_offset, id2_length):
    """chn_text_pair_ids_host: the rule the GPU runs, on the CPU, over `data1` and `data2` (bytes or uint8 arrays): both ids of a pair
    lose their last byte, and what is left must be equal.  Returns the smallest pair that disagrees, the number of pairs if none."""
    bufs = [np.frombuffer(bytes(d), np.uint8) if isinstance(d, (bytes, bytearray)) else np.ascontiguousarray(d, np.uint8) for d in (data1, data2)]
    j, keep = text_pair_job(bufs[0].ctypes.data if bufs[0].size else None, bufs[0].size, bufs[1].ctypes.data if bufs[1].size else None, bufs[1].size,
                            id1_offset, id1_length, id2_offset, id2_length)
    _chk(_L.chn_text_pair_ids_host(C.byref(j)))
    return int(j.first_mismatch)


# ---- raw deflate members (see include/charon_hip.h) ----
def inflate_job(members, sizes, guard=0, out=None, out_device=None, out_offset=None):
    """the chn_inflate_job of `members` (raw deflate streams as bytes) with expected `sizes`: the members back to back in one input
    array, the outputs in order with `guard` untouched bytes (0xA5) behind each.  `out`: a uint8 array to decode into (e.g. a
    pinned_array) instead of a fresh one.  out_device: (device pointer, bytes) to decode into instead -- CHN_INFLATE_OUT_DEVICE; the
    caller fills and reads that memory, arrays["out"] is None.  out_offset: the members' places in `out`, where they are not to lie
    in order `guard` bytes apart.  Returns (job, arrays) -- `arrays` keeps the memory alive and names it."""
    n = len(members)
    in_length = np.array([len(m) for m in members], np.uint32)
    in_offset = np.zeros(n, np.uint64)
    if n:
        in_offset[1:] = np.cumsum(in_length[:-1], dtype=np.uint64)
    data = np.frombuffer(b"".join(members), np.uint8) if n and int(in_length.sum()) else np.zeros(0, np.uint8)
    out_length = np.array([int(x) for x in sizes], np.uint32)
    if out_offset is not None:
        out_offset = np.array([int(x) for x in out_offset], np.uint64)
        out_bytes = int(out_offset[-1]) + int(out_length[-1]) + guard if n else 0
    else:
        out_offset = np.zeros(n, np.uint64)
        if n:
            out_offset[1:] = np.cumsum(out_length[:-1].astype(np.uint64) + np.uint64(guard), dtype=np.uint64)
        out_bytes = int(out_length.astype(np.uint64).sum()) + guard * n
    if out_device is not None:
        out = None
        assert out_device[1] >= out_bytes
    else:
        if out is None:
            out = np.empty(max(out_bytes, 1), np.uint8)
        assert out.dtype == np.uint8 and out.size >= out_bytes
        out[:] = 0xA5
    status = np.full(max(n, 1), 0xFFFFFFFF, np.uint32)
    j = InflateJob()
    j.struct_size, j.flags, j.n_members = C.sizeof(InflateJob), INFLATE_OUT_DEVICE if out_device is not None else 0, n
    j.in_, j.in_bytes = (data.ctypes.data if data.size else None), data.size
    j.in_offset, j.in_length = in_offset.ctypes.data, in_length.ctypes.data
    j.out, j.out_bytes = (out_device[0] if out_device is not None else out.ctypes.data), out_bytes
    j.out_offset, j.out_length, j.status = out_offset.ctypes.data, out_length.ctypes.data, status.ctypes.data
    return j, dict(data=data, in_offset=in_offset, in_length=in_length, out=out, out_offset=out_offset, out_length=out_length,
                   status=status, guard=guard, n=n)


def _inflate_results(a):
    """(list of bytes -- None where the decode failed --, status array) of a finished job; the guard bytes must be untouched"""
    res, st = [], a["status"][:a["n"]].copy()
    for i in range(a["n"]):
        o, l = int(a["out_offset"][i]), int(a["out_length"][i])
        res.append(a["out"][o:o + l].tobytes() if st[i] in (0, INFLATE_E_CRC) else None)  # (a CRC mismatch still has its bytes)
        if a["guard"] and not (a["out"][o + l:o + l + a["guard"]] == 0xA5).all():
            raise ChnError("inflate: member %d wrote behind its out_length" % i)
    return res, st


def inflate_crc(n, expected=None, want_crc=False):
    """the chn_inflate_crc of a job of n members: `expected` (n CRC-32 values) is compared, want_crc asks for the CRCs.  Returns
    (struct, arrays) -- `arrays` keeps the memory alive; arrays["crc32"] is None unless want_crc."""
    c = InflateCrc()
    c.struct_size, c.reserved = C.sizeof(InflateCrc), 0
    exp = None
    if expected is not None:
        exp = np.array([int(x) & 0xFFFFFFFF for x in expected], np.uint32)
        assert exp.size == n
        exp = np.concatenate([exp, np.zeros(1, np.uint32)])  # (never empty)
        c.expected = exp.ctypes.data
    crc = np.full(max(n, 1), 0xFFFFFFFF, np.uint32) if want_crc else None
    if want_crc:
        c.crc32 = crc.ctypes.data
    return c, dict(expected=exp, crc32=crc)


def _inflate_crc_results(a, ca, want_crc):
    """_inflate_results, and the CRC array behind it if it was asked for"""
    res, st = _inflate_results(a)
    return (res, st, ca["crc32"][:a["n"]].copy()) if want_crc else (res, st)


def inflate_host(members, sizes, guard=0, expected=None, want_crc=False):
    """chn_inflate_run_host: the decoder the GPU runs, on the CPU.  Returns (list of bytes, or None where status != 0; status array).
    expected: the members' CRC-32 values to compare with (a difference is status INFLATE_E_CRC); want_crc: the CRC-32 array is
    returned as a third value (chn_inflate_run_host_crc: the 64 slices and the join the kernel runs, serially)."""
    j, a = inflate_job(members, sizes, guard)
    if expected is None and not want_crc:
        _chk(_L.chn_inflate_run_host(C.byref(j)))
        return _inflate_results(a)
    c, ca = inflate_crc(a["n"], expected, want_crc)
    _chk(_L.chn_inflate_run_host_crc(C.byref(j), C.byref(c)))
    return _inflate_crc_results(a, ca, want_crc)


# ---- chunks of one deflate stream (see include/charon_hip.h) ----
def inflate_stream_job(data, begin_bit, target_bit, window=b"", sym_capacity=INFLATE_STREAM_MIN_SYMS, out_bytes=0, guard=0, out=None,
                       out_device=None, want_crc=True):
    """the chn_inflate_stream_job of raw deflate `data` with chunks at begin_bit / target_bit and `window` in front of chunk 0.
    out_bytes is what the job may write, `guard` bytes (0xA5) lie behind it in the array; `out`: a uint8 array to use (e.g. a
    pinned_array); out_device: (device pointer, bytes) -- CHN_INFLATE_OUT_DEVICE, arrays["out"] is None.  Every output array starts
    as all ones.  Returns (job, arrays) -- `arrays` keeps the memory alive and names it."""
    n = len(begin_bit)
    assert len(target_bit) == n
    inp = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(0, np.uint8)
    win = np.frombuffer(bytes(window), np.uint8) if len(window) else np.zeros(0, np.uint8)
    begin = np.array([int(x) for x in begin_bit] + [0], np.uint64)
    target = np.array([int(x) for x in target_bit] + [0], np.uint64)
    if out_device is not None:
        out = None
        assert out_device[1] >= out_bytes
    else:
        if out is None:
            out = np.empty(max(out_bytes + guard, 1), np.uint8)
        assert out.dtype == np.uint8 and out.size >= out_bytes + guard
        out[:] = 0xA5
    a = dict(data=inp, window=win, begin_bit=begin, target_bit=target, out=out, out_bytes=out_bytes, guard=guard, n=n,
             end_bit=np.full(n + 1, 2 ** 64 - 1, np.uint64), out_length=np.full(n + 1, 2 ** 64 - 1, np.uint64),
             status=np.full(n + 1, 0xFFFFFFFF, np.uint32), final=np.full(n + 1, 0xFF, np.uint8),
             crc32=np.full(n + 1, 0xFFFFFFFF, np.uint32) if want_crc else None, counts=np.full(2, 2 ** 64 - 1, np.uint64))
    j = InflateStreamJob()
    j.struct_size, j.flags, j.n_chunks = C.sizeof(InflateStreamJob), INFLATE_OUT_DEVICE if out_device is not None else 0, n
    j.in_, j.in_bytes = (inp.ctypes.data if inp.size else None), inp.size
    j.begin_bit, j.target_bit = begin.ctypes.data, target.ctypes.data
    j.window, j.window_bytes = (win.ctypes.data if win.size else None), win.size
    j.sym_capacity = sym_capacity
    j.out, j.out_bytes = (out_device[0] if out_device is not None else out.ctypes.data), out_bytes
    j.end_bit, j.out_length, j.status, j.final = a["end_bit"].ctypes.data, a["out_length"].ctypes.data, a["status"].ctypes.data, a["final"].ctypes.data
    j.crc32 = a["crc32"].ctypes.data if want_crc else None
    j.n_counted, j.out_used = a["counts"].ctypes.data, a["counts"].ctypes.data + 8
    return j, a


def _inflate_stream_results(a):
    """dict of a finished stream job: n_counted, out_used, the per-chunk arrays cut to the COUNTED chunks, and `bytes` =
    out[:out_used] (None for device output); the guard bytes behind out_bytes must be untouched"""
    nc, used = int(a["counts"][0]), int(a["counts"][1])
    res = dict(n_counted=nc, out_used=used, end_bit=[int(x) for x in a["end_bit"][:nc]], out_length=[int(x) for x in a["out_length"][:nc]],
               status=[int(x) for x in a["status"][:nc]], final=[int(x) for x in a["final"][:nc]],
               crc32=[int(x) for x in a["crc32"][:nc]] if a["crc32"] is not None else None, bytes=None)
    if a["out"] is not None:
        ob = a["out_bytes"]
        if not (a["out"][ob:] == 0xA5).all():
            raise ChnError("inflate stream: a byte behind out_bytes was written")
        res["bytes"] = a["out"][:used].tobytes()
    return res


def inflate_stream_host(data, begin_bit, target_bit, **kw):
    """chn_inflate_stream_run_host: the chunk decoder, the window hand-down and the byte rules the GPU runs, on the CPU.
    Keywords as in inflate_stream_job.  Returns the dict of _inflate_stream_results."""
    j, a = inflate_stream_job(data, begin_bit, target_bit, **kw)
    _chk(_L.chn_inflate_stream_run_host(C.byref(j)))
    return _inflate_stream_results(a)


# ---- block starts of one deflate stream (see include/charon_hip.h) ----
def inflate_search_job(data, from_bit, to_bit):
    """the chn_inflate_search_job of the ranges [from_bit[i], to_bit[i]) of `data`.  found_bit starts as 0xA5 bytes.
    Returns (job, arrays) -- `arrays` keeps the memory alive and names it."""
    n = len(from_bit)
    assert len(to_bit) == n
    inp = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(0, np.uint8)
    a = dict(data=inp, n=n, from_bit=np.array([int(x) for x in from_bit] + [0], np.uint64),
             to_bit=np.array([int(x) for x in to_bit] + [0], np.uint64), found_bit=np.full(n + 1, 0xA5A5A5A5A5A5A5A5, np.uint64))
    j = InflateSearchJob()
    j.struct_size, j.flags, j.n_ranges = C.sizeof(InflateSearchJob), 0, n
    j.in_, j.in_bytes = (inp.ctypes.data if inp.size else None), inp.size
    j.from_bit, j.to_bit, j.found_bit = a["from_bit"].ctypes.data, a["to_bit"].ctypes.data, a["found_bit"].ctypes.data
    return j, a


def _inflate_search_results(a):
    """the found positions of a finished search job, None where there is none; the element behind the last must be untouched"""
    if int(a["found_bit"][a["n"]]) != 0xA5A5A5A5A5A5A5A5:
        raise ChnError("inflate search: an element behind found_bit[n_ranges - 1] was written")
    return [None if int(x) == INFLATE_SEARCH_NONE else int(x) for x in a["found_bit"][:a["n"]]]


def inflate_search_host(data, from_bit, to_bit):
    """chn_inflate_stream_search_host: the first position of every range [from_bit[i], to_bit[i]) where a dynamic block seems to
    start (rules R0 - R6 of the header), on the CPU.  Returns a list of positions, None for none."""
    j, a = inflate_search_job(data, from_bit, to_bit)
    _chk(_L.chn_inflate_stream_search_host(C.byref(j)))
    return _inflate_search_results(a)


class Inflater:
    """chn_inflate: raw deflate members decoded on the device, one wavefront a member.  One thread at a time per object."""

    def run_stream(self, data, begin_bit, target_bit, **kw):
        """chn_inflate_stream_run: chunks of one deflate stream decoded side by side on the device (see inflate_stream_host)"""
        j, a = inflate_stream_job(data, begin_bit, target_bit, **kw)
        _chk(_L.chn_inflate_stream_run(self.h, C.byref(j)))
        return _inflate_stream_results(a)

    def run_stream_job(self, job):
        """chn_inflate_stream_run on a prepared InflateStreamJob: no copies on the Python side, for measurements"""
        _chk(_L.chn_inflate_stream_run(self.h, C.byref(job)))

    def __init__(self, device=0):
        self.h = C.c_void_p()
        _chk(_L.chn_inflate_create(device, C.byref(self.h)))

    def run(self, members, sizes, guard=0, out=None, expected=None, want_crc=False, out_device=None, out_offset=None):
        """members: list of raw deflate streams (bytes); sizes: their expected inflated sizes (<= INFLATE_MAX_OUT).
        Returns (list of bytes, or None where status != 0; status array).  expected / want_crc as in inflate_host
        (chn_inflate_run_crc: the CRC-32 is taken on the device).  out_device=(device pointer, bytes): the members are written into
        that device memory (CHN_INFLATE_OUT_DEVICE) at out_offset (default: in order, `guard` bytes apart) and the first value
        returned is None -- the bytes are the caller's to download."""
        j, a = inflate_job(members, sizes, guard, out, out_device, out_offset)
        if expected is None and not want_crc:
            _chk(_L.chn_inflate_run(self.h, C.byref(j)))
            return _inflate_results(a) if out_device is None else (None, a["status"][:a["n"]].copy())
        c, ca = inflate_crc(a["n"], expected, want_crc)
        _chk(_L.chn_inflate_run_crc(self.h, C.byref(j), C.byref(c)))
        if out_device is not None:
            st = a["status"][:a["n"]].copy()
            return (None, st, ca["crc32"][:a["n"]].copy()) if want_crc else (None, st)
        return _inflate_crc_results(a, ca, want_crc)

    def run_job(self, job, crc=None):
        """chn_inflate_run (or chn_inflate_run_crc with an InflateCrc) on a prepared InflateJob (inflate_job): no copies on the
        Python side, for measurements"""
        if crc is None:
            _chk(_L.chn_inflate_run(self.h, C.byref(job)))
        else:
            _chk(_L.chn_inflate_run_crc(self.h, C.byref(job), C.byref(crc)))

    def kernel_ms(self):
        ms = C.c_double()
        _chk(_L.chn_inflate_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def destroy(self):
        if self.h:
            _L.chn_inflate_destroy(self.h)
            self.h = None


# ---- deflate on the device (see include/charon_hip.h) ----
def deflate_bound(n_members, in_bytes_total, flags=0):
    b = C.c_uint64()
    _chk(_L.chn_deflate_bound(n_members, in_bytes_total, flags, C.byref(b)))
    return b.value


def deflate_job(pieces, flags=0, data=None, out=None, slack=0):
    """the chn_deflate_job of `pieces`.  pieces: a list of bytes (laid back to back into one input array), or -- with `data`, a uint8
    array (e.g. a pinned_array) that holds them -- a list of (offset, length).  `out`: a uint8 array to compress into instead of a fresh
    one of chn_deflate_bound + slack bytes.  Returns (job, arrays) -- `arrays` keeps the memory alive and names it."""
    n = len(pieces)
    if data is None:
        in_length = np.array([len(m) for m in pieces], np.uint32)
        in_offset = np.zeros(n, np.uint64)
        if n:
            in_offset[1:] = np.cumsum(in_length[:-1], dtype=np.uint64)
        data = np.frombuffer(b"".join(pieces), np.uint8) if n and int(in_length.sum()) else np.zeros(0, np.uint8)
    else:
        in_offset = np.array([int(o) for o, _ in pieces], np.uint64)
        in_length = np.array([int(l) for _, l in pieces], np.uint32)
    in_offset = np.concatenate([in_offset, np.zeros(1, np.uint64)])  # (never empty)
    in_length = np.concatenate([in_length, np.zeros(1, np.uint32)])
    bound = deflate_bound(n, int(in_length.astype(np.uint64).sum()), flags & DEFLATE_BGZF)
    if out is None:
        out = np.empty(max(bound + slack, 1), np.uint8)
    assert out.dtype == np.uint8
    out[:] = 0xA5
    out_offset = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, np.uint64)
    out_length = np.full(n + 1, 0xFFFFFFFF, np.uint32)
    crc = np.full(n + 1, 0xFFFFFFFF, np.uint32)
    used = np.full(1, 0xFFFFFFFFFFFFFFFF, np.uint64)
    j = DeflateJob()
    j.struct_size, j.flags, j.n_members = C.sizeof(DeflateJob), flags, n
    j.in_, j.in_bytes = (data.ctypes.data if data.size else None), data.size
    j.in_offset, j.in_length = in_offset.ctypes.data, in_length.ctypes.data
    j.out, j.out_bytes = out.ctypes.data, out.size
    j.out_offset, j.out_length, j.out_used, j.crc32 = out_offset.ctypes.data, out_length.ctypes.data, used.ctypes.data, crc.ctypes.data
    return j, dict(data=data, in_offset=in_offset, in_length=in_length, out=out, out_offset=out_offset, out_length=out_length,
                   used=used, crc32=crc, bound=bound, n=n)


def _deflate_results(a):
    """a finished job as a dict: out (bytes, out[0 .. out_used)), offset, length, crc32 (arrays of n), used, bound"""
    n, used = a["n"], int(a["used"][0])
    return dict(out=a["out"][:used].tobytes(), offset=a["out_offset"][:n].copy(), length=a["out_length"][:n].copy(),
                crc32=a["crc32"][:n].copy(), used=used, bound=a["bound"])


def deflate_host(pieces, flags=0, data=None):
    """chn_deflate_run_host: the compressor the GPU runs, on the CPU -- the same bytes.  See _deflate_results for what is returned."""
    j, a = deflate_job(pieces, flags, data)
    _chk(_L.chn_deflate_run_host(C.byref(j)))
    return _deflate_results(a)


class Deflater:
    """chn_deflate: pieces of at most DEFLATE_MAX_IN bytes deflated on the device, one wavefront a piece, optionally framed as BGZF
    blocks.  One thread at a time per object."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        _chk(_L.chn_deflate_create(device, C.byref(self.h)))

    def run(self, pieces, flags=0, data=None, out=None):
        j, a = deflate_job(pieces, flags, data, out)
        _chk(_L.chn_deflate_run(self.h, C.byref(j)))
        return _deflate_results(a)

    def run_job(self, job):
        """chn_deflate_run on a prepared DeflateJob (deflate_job): no copies on the Python side, for measurements"""
        _chk(_L.chn_deflate_run(self.h, C.byref(job)))

    def group_members(self, members):
        """testing / measurement: at most `members` members in a group of the pipeline (1 .. 1024)"""
        _chk(_L.chn_deflate_group_members(self.h, members))

    def kernel_ms(self):
        ms = C.c_double()
        _chk(_L.chn_deflate_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def destroy(self):
        if self.h:
            _L.chn_deflate_destroy(self.h)
            self.h = None


# ---- the records of an --extract file formed and deflated on the device (see include/charon_hip.h) ----
def extract_job(text_ptr, nbytes, id_offset, id_length, seq_offset, seq_length, qual_offset, qual_length, out=None, out_capacity=None):
    """the chn_extract_job of records whose id, sequence and quality string are the given ranges of the text at `text_ptr`.  `out`:
    a uint8 array for the members (pageable or from pinned_array), out_capacity defaults to its size.  Returns (job, arrays to keep
    alive)."""
    keep = [np.ascontiguousarray(id_offset, np.uint64), np.ascontiguousarray(id_length, np.uint32),
            np.ascontiguousarray(seq_offset, np.uint64), np.ascontiguousarray(seq_length, np.uint32),
            np.ascontiguousarray(qual_offset, np.uint64), np.ascontiguousarray(qual_length, np.uint32)]
    if any(a.ndim != 1 or a.size != keep[0].size for a in keep):
        raise ValueError("the six descriptor arrays must be one-dimensional and of one size")
    j = ExtractJob()
    j.struct_size, j.flags, j.text, j.text_bytes, j.n_records = C.sizeof(ExtractJob), 0, text_ptr, int(nbytes), keep[0].size
    j.id_offset, j.id_length, j.seq_offset, j.seq_length, j.qual_offset, j.qual_length = (a.ctypes.data for a in keep)
    if out is not None:
        j.out, j.out_capacity = out.ctypes.data, out.size if out_capacity is None else int(out_capacity)
    else:
        j.out, j.out_capacity = None, int(out_capacity or 0)
    j.out_used = 0xDEADBEEF
    return j, keep + [out]


def extract_record_bytes(id_length, seq_length, qual_length):
    """the bytes the records of these lengths have altogether: id + sequence + quality string + 6 each"""
    return int(sum(int(np.asarray(a, np.uint64).sum(dtype=np.uint64)) for a in (id_length, seq_length, qual_length))) + 6 * len(id_length)


def extract_records_host(data, id_offset, id_length, seq_offset, seq_length, qual_offset, qual_length, nbytes=None, capacity=None):
    """chn_extract_records_host: the record rule the GPU runs, on the CPU, over `data` (bytes or a uint8 array).  Returns the records
    back to back as bytes."""
    buf = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
    nbytes = buf.size if nbytes is None else nbytes
    j, keep = extract_job(buf.ctypes.data if buf.size else None, nbytes, id_offset, id_length, seq_offset, seq_length, qual_offset, qual_length)
    cap = extract_record_bytes(keep[1], keep[3], keep[5]) if capacity is None else int(capacity)
    out = np.full(cap + 16, 0xA5, np.uint8)
    got = C.c_uint64(0xDEADBEEF)
    _chk(_L.chn_extract_records_host(C.byref(j), out.ctypes.data, cap, C.byref(got)))
    assert bytes(out[got.value:]) == b"\xa5" * (out.size - got.value), "chn_extract_records_host wrote behind the records"
    return out[:got.value].tobytes()


class Extractor:
    """chn_extract: ONE extract file.  Records formed out of a device text (append_records) and host bytes (append_bytes) make up the
    file's text; every call returns the BGZF members of the whole 65 280-byte pieces that became complete, finish() the last, shorter
    one (no end-of-file marker).  One thread at a time per object."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        _chk(_L.chn_extract_create(device, C.byref(self.h)))

    def bound(self, appended_bytes):
        """bytes `out` must have for an append of appended_bytes now; with 0, what finish() needs"""
        b = C.c_uint64()
        _chk(_L.chn_extract_bound(self.h, int(appended_bytes), C.byref(b)))
        return b.value

    def _out(self, need, out, guard):
        if out is None:
            out = np.empty(need + 2 * guard, np.uint8)
        out[:] = 0xA5
        return out

    def append_records(self, text_ptr, nbytes, id_offset, id_length, seq_offset, seq_length, qual_offset, qual_length, out=None, guard=16):
        """chn_extract_append_records.  `out`: a uint8 array of at least bound + 2 * guard bytes (e.g. a pinned_array); the members go
        to out[guard:], and the bytes around them must stay 0xA5.  Returns the members as bytes."""
        need = self.bound(extract_record_bytes(id_length, seq_length, qual_length))
        out = self._out(need, out, guard)
        j, keep = extract_job(text_ptr, nbytes, id_offset, id_length, seq_offset, seq_length, qual_offset, qual_length, out[guard:], need)
        _chk(_L.chn_extract_append_records(self.h, C.byref(j)))
        return self._taken(out, guard, int(j.out_used), need)

    def append_job(self, job):
        """chn_extract_append_records on a prepared ExtractJob (extract_job)"""
        _chk(_L.chn_extract_append_records(self.h, C.byref(job)))
        return int(job.out_used)

    def append_bytes(self, data, out=None, guard=16, capacity=None):
        buf = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
        need = self.bound(buf.size) if capacity is None else int(capacity)
        out = self._out(need, out, guard)
        used = C.c_uint64(0xDEADBEEF)
        _chk(_L.chn_extract_append_bytes(self.h, buf.ctypes.data if buf.size else None, buf.size, out[guard:].ctypes.data, need, C.byref(used)))
        return self._taken(out, guard, used.value, need)

    def finish(self, out=None, guard=16, capacity=None):
        need = self.bound(0) if capacity is None else int(capacity)
        out = self._out(need, out, guard)
        used = C.c_uint64(0xDEADBEEF)
        _chk(_L.chn_extract_finish(self.h, out[guard:].ctypes.data, need, C.byref(used)))
        return self._taken(out, guard, used.value, need)

    @staticmethod
    def _taken(out, guard, used, need):
        assert used <= need, "more bytes than chn_extract_bound gave"
        assert bytes(out[:guard]) == b"\xa5" * guard and bytes(out[guard + used:]) == b"\xa5" * (out.size - guard - used), \
            "bytes outside the returned members were written"
        return out[guard:guard + used].tobytes()

    def kernel_ms(self):
        ms = C.c_double()
        _chk(_L.chn_extract_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def destroy(self):
        if self.h:
            _L.chn_extract_destroy(self.h)
            self.h = None


def synth_genomes(device, seed, n_genomes, genome_len):
    p = C.c_void_p()
    _chk(_L.chn_synth_genomes(device, seed, n_genomes, genome_len, C.byref(p)))
    return p.value


def synth_reads(device, seed, dev_genomes, n_genomes, genome_len, n_reads, len_min, len_max, sub_rate=0.05,
                random_fraction=0.1, mean_quality=40.0, first_read_id=0):
    out = SynthReadsOut()
    _chk(_L.chn_synth_reads(device, seed, dev_genomes, n_genomes, genome_len, first_read_id, n_reads, len_min, len_max, sub_rate,
                            random_fraction, mean_quality, C.byref(out)))
    return out


def device_count():
    n = C.c_int()
    _chk(_L.chn_device_count(C.byref(n)))
    return n.value


def pinned_array(shape, dtype):
    """numpy array backed by page-locked host memory (chn_host_alloc); keep the returned array alive while in use.
    The memory is released with host_free(arr)."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape))
    p = C.c_void_p()
    _chk(_L.chn_host_alloc(max(n * dtype.itemsize, 16), C.byref(p)))
    buf = (C.c_char * (n * dtype.itemsize)).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)
    _PINNED[arr.ctypes.data] = p.value
    return arr


_PINNED = {}


def host_free(arr):
    p = _PINNED.pop(arr.ctypes.data, None)
    if p:
        _chk(_L.chn_host_free(p))


def device_malloc(device, nbytes):
    p = C.c_void_p()
    _chk(_L.chn_device_malloc(device, nbytes, C.byref(p)))
    return p.value


def device_upload(device, ptr, arr):
    arr = np.ascontiguousarray(arr)
    _chk(_L.chn_device_upload(device, ptr, arr.ctypes.data, arr.nbytes))


def device_free(device, ptr):
    if ptr:
        _chk(_L.chn_device_free(device, ptr))


def device_copy(device, dst_ptr, src_ptr, nbytes):
    """chn_device_copy: nbytes from src_ptr to dst_ptr, both device memory of `device`"""
    _chk(_L.chn_device_copy(device, dst_ptr, src_ptr, int(nbytes)))


def device_download(device, ptr, nbytes, dtype):
    out = np.zeros(nbytes // np.dtype(dtype).itemsize, dtype)
    _chk(_L.chn_device_download(device, out.ctypes.data, ptr, nbytes))
    return out
