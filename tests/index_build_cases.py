"""Case tables and builders of the index-build tests (tests/test_index_build_cases_cpu.py checks them without a GPU;
tests/test_gpu_index_build.py and tests/test_gpu_index_kw_cli.py run them): the (k, w) pairs the list form of the probe kernel is held
to the oracle at, the reads of those batches, the record `charon index` cuts into chunks and the cutting rule restated, and the value
arrays whose reference stays cheap however many values go to the device.  Plain module: no test in here."""
import numpy as np

from oracle import pyref
from tests import util
from tests.test_gpu_ring_pack import KW as RING_KW

U64 = np.uint64
MAX = 2 ** 64 - 1
CHUNK = 4096          # windows a chunk of `charon index` starts (host/index_builder.inc)

# test_gpu_ring_pack.KW: packed and unpacked window rings, wn = 1, the pb edge 34 / 35.  Then: a tiny k; k = w = 1; the default window at
# a small k; a wide window; w - k + 1 = 23 (the fixed-window instance's width) at a k other than 19; the widest window there is
KW_LIST = list(RING_KW) + [(4, 8), (1, 1), (11, 41), (15, 120), (5, 27), (19, 255)]
KW_CLI = [(27, 29), (21, 21), (15, 120), (11, 41)]


def kw_id(kw):
    return "k%d_w%d" % kw


def pack_ok(k, w):
    """ring_pack_ok of parts/lds_budget.hpp, restated: bits(max(5^k - 1, seed >> (64 - 2k))) + bits(wn - 1) <= 64"""
    wn = w - k + 1
    return max(5 ** k - 1, pyref.SEED >> (64 - 2 * k)).bit_length() + (wn - 1).bit_length() <= 64


# ---- the reads of the whole-batch and single-read tests -----------------------------------------------------------------------------
def edge_reads(k, w, seed=0):
    """the reads that go alone as well: lengths around k, w, the wavefront and one chunk; ties; N at the ends and across a window; all N;
    lower case and IUPAC letters"""
    r = util.rng(4000 + 300 * k + w + seed)
    g = util.random_seq(r, 6000)
    reads = [g[s:s + n] for s, n in zip(range(0, 1100, 100), (k - 1, k, w - 1, w, w + 1, 63, 64, 65, 128, 129, CHUNK + w - 1))]
    reads += [b"A" * 1000, b"T" * (w + 1), b"C" * w, b"AC" * 400, b"ACG" * 200 + b"T" * 77, b"ACGGTCA" * 60,   # homopolymers, periods 2, 3, 7
              g[:150] + b"AC" * 150 + g[150:250] + b"G" * 3 * w]                                            # ties that come and go
    reads += [b"N" + g[1000:1500], g[1500:2000] + b"N", g[2000:2100] + b"N" * (w + 2) + g[2100:2400],        # N first, last, across a window
              g[2400:2500] + b"N" + g[2500:2520] + b"NN" + g[2520:2900], b"N" * 300, b"ACGTN" * 60,
              g[3000:3600].lower(), g[3600:3900] + b"RYKMSWBDHV" + g[3900:4200].lower() + b"u" * 5 + g[4200:4300]]
    return reads


def batch_reads(k, w):
    """(all reads of the whole-batch test, how many of them are the edge reads in front): the edge reads, one 40 000-base read (the list
    modes never split a read) and 200 sampled reads"""
    edge = edge_reads(k, w)
    r = util.rng(5000 + 300 * k + w)
    g0, g1 = util.random_seq(r, 5000), util.random_seq(r, 5000)
    low = b"A" * 300 + g0[:200] + b"AC" * 150 + g1[:100] + b"ACG" * 90
    return edge + [util.random_seq(r, 40000)] + util.sample_reads(r, [g0, g1, low], 200, (1, 1500), sub_rate=0.02), len(edge)


BATCH_SIZES = (1, 63, 64, 65, None)   # a wavefront takes 64 reads; None: the full set


def oracle_minimisers(po, reads, k, w):
    """the oracle's minimisers of every read, in order of occurrence: a list of uint64 arrays"""
    return [po.minimisers(s.decode(), k, w).copy() for s in reads]


def sorted_concat(arrays):
    return np.sort(np.concatenate([np.zeros(0, U64)] + list(arrays)))


# ---- the record `charon index` cuts into chunks -------------------------------------------------------------------------------------
RECORD_BASES = 30000


def chunked_record():
    """30 000 bases with N runs laid across the chunk seams at 4 096 and 8 192 and inside the overlap behind them"""
    a = bytearray(util.random_seq(util.rng(77), RECORD_BASES))
    for s, n in ((4085, 16), (4096 + 20, 1), (8180, 120), (12288 - 1, 2), (16384 + 7, 30), (20000, 300)):
        a[s:s + n] = b"N" * n
    return bytes(a)


def chunks(L, w):
    """the builder's cutting rule: one chunk per started block of 4 096 windows, [c * 4096, min(L, c * 4096 + 4096 + w - 1));
    a record shorter than w has one window's worth of chunk"""
    nwin = L - w + 1 if L >= w else 1
    return [(c * CHUNK, min(L, c * CHUNK + CHUNK + w - 1) - c * CHUNK) for c in range((nwin + CHUNK - 1) // CHUNK)]


def chunked_batch(seq, w):
    """the record packed once, every chunk a read of its own (seg1_offset / seg1_length as the builder writes them)"""
    from charon_amd import pack
    p = pack.pack_reads([seq])
    cs = chunks(len(seq), w)
    p["seg1_offset"] = np.array([s for s, _ in cs], np.uint64)
    p["seg1_length"] = np.array([n for _, n in cs], np.uint32)
    return p, cs


# ---- values for the emplace tests ----------------------------------------------------------------------------------------------------
def emplace_values(r, n):
    """n values with 0, 2^64 - 1 and repeats among them"""
    v = r.integers(0, MAX, n, dtype=U64, endpoint=True)
    v[:4] = (0, MAX, 0, MAX)
    v[n // 2:n // 2 + n // 8] = v[:n // 8]
    return v


def emplace_bins(bins):
    """bin 0, 63, 64 and the last one, as far as the index has them"""
    return sorted({b for b in (0, 63, 64, bins - 1) if b < bins})


def shard_ranges(S):
    """row shards [begin, end): the first row, the last row, an inner range, and two adjacent ranges that make the whole index"""
    cut = S // 3 + 1
    return [(0, 1), (S - 1, S), (S // 5, S // 2 + 3), (0, cut), (cut, S)]


# ---- many values, few distinct: the reference emplaces np.unique of them ------------------------------------------------------------
POOL = 3000
FRESH = 5000
N_GRID = 65535 * 256 + FRESH     # the grid of k_emplace_values is clipped at 65 535 workgroups of 256: the fresh values are a second turn's
N_PIECE = 2 ** 26 + FRESH        # chn_index_emplace uploads 2^26 values at a time: the fresh values are the second piece


def pool_and_fresh(seed):
    """(pool of 3 000 values, 5 000 fresh values) -- disjoint (tests/test_index_build_cases_cpu.py asserts it): pool values have bit 63
    clear, fresh ones have it set"""
    r = util.rng(seed)
    pool = r.integers(0, 2 ** 63, POOL, dtype=U64)
    fresh = np.unique(r.integers(2 ** 63, MAX, 2 * FRESH, dtype=U64, endpoint=True))[:FRESH]
    r.shuffle(fresh)
    return pool, fresh


def draws_then_fresh(seed, n):
    """n values: the pool once, then draws from the pool, and the fresh values last.  Filled a block at a time, so that nothing but the
    array itself is large.  -> (values, np.unique(values) by construction)"""
    pool, fresh = pool_and_fresh(seed)
    r = util.rng(seed + 1)
    v = np.empty(n, U64)
    head = n - FRESH
    v[:POOL] = pool
    block = pool[r.integers(0, POOL, 1 << 20)]
    for at in range(POOL, head, block.size):
        m = min(block.size, head - at)
        v[at:at + m] = block[:m]
    v[head:] = fresh
    return v, np.unique(np.concatenate([pool, fresh]))


# ---- sizes of the sort tests ---------------------------------------------------------------------------------------------------------
N_HIST = 2048 * 4096 + 4099      # k_radix_hist walks 4 096 keys a workgroup and is clipped at 2 048 workgroups
TILE_SIZES = {65536: (65535, 65536, 65537, 3 * 65536 + 5),   # the largest legal tile: a wavefront walks 16 384 keys in 256 rounds
              768: (767, 768, 769, 5 * 768 + 3)}              # 192 keys a wavefront: no power of two
