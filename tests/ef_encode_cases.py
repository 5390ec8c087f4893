"""Cases of the Elias-Fano encode (chn_index_encode_ef, chn_index_encode_ef_host), shared by tests/test_ef_encode_cpu.py and
tests/test_gpu_ef_encode.py: the smallest shapes at which the rule, the slices' seams or the kernel's scan can go wrong.

A case is (name, bins, bin_size, maker, slices): maker(rng, bins, tb, bin_size) returns the ascending plain positions
pos = row * technical_bins + bin of the set bits; `slices` are the slice_rows values the case runs with.  Positions come from a generator
seeded by the case's name.  The expected arrays are oracle.pyref.ef_encode of the positions (the independent restatement of sdsl's sd_vector
layout), computed once per case and shared."""
import functools
import zlib

import numpy as np

from oracle import pyref


def _random(ones, all_bins=False):
    def make(rng, bins, tb, bin_size):
        rows = rng.integers(0, bin_size, ones * 2)
        cols = rng.integers(0, tb if all_bins else bins, ones * 2)
        return np.unique(rows.astype(np.int64) * tb + cols)[:ones]
    return make


def _all_real_bits(rng, bins, tb, bin_size):
    return (np.arange(bin_size, dtype=np.int64)[:, None] * tb + np.arange(bins, dtype=np.int64)[None, :]).ravel()


def _fixed(positions):
    return lambda rng, bins, tb, bin_size: np.array([p if p >= 0 else tb * bin_size + p for p in positions], np.int64)


def _in_rows(rows_and_counts):
    """`count` random bits in each of the given rows, nothing elsewhere"""
    def make(rng, bins, tb, bin_size):
        out = []
        for row, count in rows_and_counts:
            out.append(row * tb + np.sort(rng.choice(bins, count, replace=False)).astype(np.int64))
        return np.concatenate(out)
    return make


def _technical_only(rng, bins, tb, bin_size):
    """bits in the technical-only bins (>= bins) of a third of the rows, some real ones beside them"""
    rows = rng.integers(0, bin_size, 400)
    cols = np.where(rng.random(400) < 0.7, rng.integers(bins, tb, 400), rng.integers(0, bins, 400))
    return np.unique(rows.astype(np.int64) * tb + cols)


def _blocks_of_256(rng, bins, tb, bin_size):
    """one word a row: words 0..255 all ones, 256..511 all zeros, 512..767 all ones, 768..1023 zeros, then noise"""
    w = np.zeros(bin_size, np.uint64)
    w[0:256] = ~np.uint64(0)
    w[512:768] = ~np.uint64(0)
    w[1024:] = rng.integers(0, 2 ** 63, bin_size - 1024, dtype=np.uint64) & rng.integers(0, 2 ** 63, bin_size - 1024, dtype=np.uint64)
    return np.flatnonzero(np.unpackbits(w.view(np.uint8), bitorder="little")).astype(np.int64)


def _three_ways(given, bin_size):
    return (given, 1, bin_size)


CASES = [
    # the five shapes of test_device_elias_fano_decode, each with the given slice, with one row a slice and as one slice
    ("decode_100x5000", 100, 5000, _random(60000), _three_ways(64, 5000)),
    ("decode_8x70001", 8, 70001, _random(300000), _three_ways(1000, 70001)),
    ("decode_130x997_one", 130, 997, _random(1), _three_ways(1 << 20, 997)),
    ("decode_3x4096_full", 3, 4096, _all_real_bits, _three_ways(7, 4096)),
    ("decode_200x3001", 200, 3001, _random(150000), _three_ways(33, 3001)),
    ("empty", 5, 100, _fixed([]), (0, 7)),
    ("bit_at_0", 64, 50, _fixed([0]), (0, 1, 7)),
    ("bit_at_last", 64, 50, _fixed([-1]), (0, 1, 7)),
    ("full_64x64", 64, 64, _all_real_bits, (0, 1, 5)),            # logm == logn: the decrement applies
    ("ones_2j_minus_1", 64, 100, _random(255), (0, 9)),          # wl changes between 255 and 256 ones
    ("ones_2j", 64, 100, _random(256), (0, 9)),
    ("ones_2j_plus_1", 64, 100, _random(257), (0, 9)),
    ("straddle", 64, 1000, _random(100), (0, 1, 13)),             # wl = 9: low elements straddle words
    ("one_bin_2_20_rows", 1, 1 << 20, _fixed([5 * 64, (1 << 19) * 64, -64]), (0, 1 << 18)),   # wl = 25, long zero runs in m_high
    ("technical_only_bins", 3, 300, _technical_only, (0, 1, 11)),
    # slice boundaries (8 rows a slice) directly behind / in front of the one row that holds all of a slice's ones
    ("ones_at_slice_edges", 130, 40, _in_rows([(7, 90), (8, 120), (23, 64), (24, 1), (39, 130)]), (8, 0)),
    ("empty_slice_between", 100, 30, _in_rows([(r, 40) for r in range(0, 10)] + [(r, 55) for r in range(20, 30)]), (10, 0)),
    ("blocks_of_256", 64, 1500, _blocks_of_256, (0, 300, 256)),
]
CASE = {c[0]: c for c in CASES}
RUNS = [(c[0], s) for c in CASES for s in c[4]]


def to_words(value, bits):
    """python int (bit i = position i) -> numpy uint64 words"""
    return np.frombuffer(int(value).to_bytes(((bits + 63) // 64) * 8, "little"), np.uint64).copy()


@functools.lru_cache(maxsize=None)
def build(name):
    """the case's data: bins, bin_size, tb, universe, pos, words (plain rows), and the expected wl, low_bits, low, high_bits, high"""
    _, bins, bin_size, maker, _ = CASE[name]
    tb = (bins + 63) // 64 * 64
    universe = tb * bin_size
    pos = np.asarray(maker(np.random.default_rng(zlib.crc32(name.encode())), bins, tb, bin_size), np.int64)
    assert (np.diff(pos) > 0).all() and (pos.size == 0 or (pos[0] >= 0 and pos[-1] < universe))
    words = np.zeros(universe // 64, np.uint64)
    np.bitwise_or.at(words, pos >> 6, np.uint64(1) << (pos & 63).astype(np.uint64))
    wl, low_bits, low, high_bits, high = pyref.ef_encode([int(p) for p in pos], universe)
    d = dict(name=name, bins=bins, bin_size=bin_size, tb=tb, universe=universe, pos=pos, words=words, wl=wl, low_bits=low_bits,
             low=to_words(low, low_bits), high_bits=high_bits, high=to_words(high, high_bits))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def assert_is_expected(case, layout, low, high):
    """wl, the bit counts and both arrays, word for word, against oracle.pyref.ef_encode of the case's positions"""
    assert (layout.wl, layout.m_size, layout.ones) == (case["wl"], case["universe"], case["pos"].size)
    assert (layout.low_bits, layout.high_bits) == (case["low_bits"], case["high_bits"])
    assert (layout.n_low_words, layout.n_high_words) == (case["low"].size, case["high"].size)
    assert np.array_equal(low, case["low"]), np.flatnonzero(low != case["low"])[:8]
    assert np.array_equal(high, case["high"]), np.flatnonzero(high != case["high"])[:8]
