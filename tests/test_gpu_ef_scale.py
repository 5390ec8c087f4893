"""GPU tests of the Elias-Fano kernels where the small cases do not reach: slices of thousands of 256-word blocks (k_ef_block_prefix's
scan takes several rounds of 1024 counts and carries the sum in a register) through chn_index_encode_ef and chn_index_decode_ef; decode slices that begin in the middle of a word of
m_low at every wl the cases have; decodes of the whole vector into row shards; and vectors sdsl does not write (positions beyond m_size,
wl = 0).  Every comparison is word for word: with oracle.pyref.ef_encode for the small cases, with its numpy restatement ef_encode_np
(pinned to pyref in test_ef_encode_cpu.py) for the large ones, with the positions' own words for what a decode leaves."""
import functools

import numpy as np
import pytest

import charon_amd.api as api
from tests import ef_encode_cases as cases

pytestmark = pytest.mark.gpu


def desc_of(case, **kw):
    return api.make_desc(case["bins"], case["bin_size"], [0] * case["bins"], 1, 0, **kw)


@functools.lru_cache(maxsize=None)
def real_words(name):
    want, ill_placed = cases.real_words(cases.build(name))
    want.setflags(write=False)
    return want, ill_placed


def decoded(desc, case, slice_words, wl=None, high=None, high_bits=None, low=None):
    """(bad, rows, popcounts per technical bin) of a fresh index of `desc` after a decode of the case's arrays (or the given ones)"""
    g = api.Index(desc)
    try:
        bad = g.decode_ef(case["universe"], case["wl"] if wl is None else wl, case["high"] if high is None else high,
                          case["high_bits"] if high_bits is None else high_bits, case["low"] if low is None else low, slice_words=slice_words)
        lo = desc.row_begin
        n = (desc.row_end if desc.row_end else desc.bin_size) - lo
        return bad, g.download(lo, n), g.bin_popcounts()
    finally:
        g.destroy()


# ---- slices of many blocks ------------------------------------------------------------------------------------------------------------

def _slice_with_a_short_tail(bin_size):
    """three slices of more than 2048 blocks and a fourth of 100 to 102 words: a last grid of one block that is mostly past the end"""
    return (bin_size - 100) // 3


@pytest.mark.parametrize("slices", ["one", "1024_blocks", "1025_blocks", "short_tail"])
@pytest.mark.parametrize("name", list(cases.LARGE))
def test_encode_slices_of_many_blocks(name, slices):
    case = cases.build_large(name)
    slice_rows = {"one": 0, "1024_blocks": 1 << 18, "1025_blocks": cases.LARGE_SLICE_ROWS,
                  "short_tail": _slice_with_a_short_tail(case["bin_size"])}[slices]
    if slices == "short_tail":
        assert 0 < case["bin_size"] % slice_rows < 256 and slice_rows > 2048 * 256
    if slices == "1024_blocks":  # (the zero count the call appends is the 1025th: the slice's total comes out of the second round)
        assert slice_rows == cases.PREFIX_CHUNK * cases.BLOCK_WORDS
    g = api.Index(desc_of(case))
    try:
        g.upload(case["words"])
        lay, low, high, _ = g.encode_ef(slice_rows)
    finally:
        g.destroy()
    cases.assert_is_expected(case, lay, low, high)
    hlay, hlow, hhigh, _ = api.encode_ef_host(desc_of(case), case["words"], slice_rows)
    for f, _t in api.EfLayout._fields_:
        assert getattr(lay, f) == getattr(hlay, f), f
    assert np.array_equal(low, hlow) and np.array_equal(high, hhigh)


@pytest.mark.parametrize("slice_words", [1 << 20, 262144, 262145, 65536])
@pytest.mark.parametrize("name", list(cases.LARGE))
def test_decode_slices_of_many_blocks(name, slice_words):
    case = cases.build_large(name)
    if slice_words == 1 << 20:  # Index.decode_ef's default: the whole of m_high in one slice, every round of the prefix loop
        assert case["high"].size <= slice_words
    bad, rows, per_bin = decoded(desc_of(case), case, slice_words)
    assert bad == 0
    assert np.array_equal(rows, case["words"]), np.flatnonzero(rows != case["words"])[:8]
    assert np.array_equal(per_bin, case["per_bin"])


# ---- decode seams ---------------------------------------------------------------------------------------------------------------------

SEAM_NAMES = [c[0] for c in cases.CASES] + [cases.SEAM[0]]
MORE_THAN_2048_HIGH_WORDS = ("decode_8x70001", "decode_200x3001")  # a word a slice is for the others
SEAM_RUNS = [(n, s) for n in SEAM_NAMES for s in (1, 3, 255, 256, 257) if s > 1 or n not in MORE_THAN_2048_HIGH_WORDS]


@pytest.mark.parametrize("name,slice_words", SEAM_RUNS)
def test_decode_seams(name, slice_words):
    """the decode half of test_device_form, from the reference arrays, over slices that begin at any rank and any bit of m_low"""
    case = cases.build(name)
    assert (case["high"].size > 2048) == (name in MORE_THAN_2048_HIGH_WORDS)
    if name == cases.SEAM[0]:
        assert 64 % case["wl"] != 0 and case["pos"].size > 64 * 3 and case["high"].size > 200
    want, ill_placed = real_words(name)
    bad, rows, _ = decoded(desc_of(case), case, slice_words)
    assert bad == ill_placed
    assert np.array_equal(rows, want), np.flatnonzero(rows != want)[:8]
    if name != "technical_only_bins":
        assert bad == 0 and np.array_equal(want, case["words"])
    else:
        assert bad > 0


# ---- row shards -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("slice_words", [64, 1 << 20])
@pytest.mark.parametrize("name,a", [("decode_200x3001", 1237), (cases.SEAM[0], 33331), ("technical_only_bins", 101)])
def test_decode_into_row_shards(name, a, slice_words):
    """every shard is handed the whole vector and keeps its own rows; ill-placed bits are counted in front of the row filter (include/
    charon_hip.h: "the number of positions >= m_size or in technical bins >= bins that the slices met"), so every shard reports them all"""
    case = cases.build(name)
    want, ill_placed = real_words(name)
    tb, W, S = case["tb"], case["tb"] // 64, case["bin_size"]
    assert 1 < a < S
    real = case["pos"][case["pos"] % tb < case["bins"]]
    got = []
    for lo, hi in ((0, 1), (1, a), (a, S)):
        bad, rows, per_bin = decoded(desc_of(case, row_begin=lo, row_end=hi), case, slice_words)
        assert bad == ill_placed
        assert rows.size == (hi - lo) * W
        mine = real[(real // tb >= lo) & (real // tb < hi)]
        assert np.array_equal(per_bin, np.bincount(mine % tb, minlength=tb).astype(np.uint64)), (lo, hi)
        got.append(rows)
    got = np.concatenate(got)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert (ill_placed > 0) == (name == "technical_only_bins")


# ---- vectors sdsl does not write ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sliced", [False, True])
def test_positions_beyond_m_size_are_counted_not_written(sliced):
    case = cases.build(cases.SEAM[0])
    U, m = case["universe"], case["pos"].size
    beyond = np.array([2 * U - 1000, 2 * U - 77, 2 * U - 1], np.int64)
    wl, low_bits, low, high_bits, high = cases.ef_encode_np(np.concatenate([case["pos"], beyond]), 2 * U)
    slice_words = 1 << 20
    if sliced:  # a seam between the last one of a position in the index and the first of one beyond it: those three are a slice's all
        last_inside, first_beyond = (int(case["pos"][-1]) >> wl) + m - 1, (int(beyond[0]) >> wl) + m
        slice_words = first_beyond // 64
        assert last_inside < slice_words * 64 and slice_words < high.size <= 2 * slice_words and m % 64 != 0
    bad, rows, per_bin = decoded(desc_of(case), case, slice_words, wl=wl, high=high, high_bits=high_bits, low=low)
    assert bad == 3
    assert np.array_equal(rows, case["words"])
    assert int(per_bin.sum()) == m


@pytest.mark.parametrize("slice_words", [1 << 20, 7])
def test_wl_0_with_no_low_array(slice_words):
    """sdsl's rule gives wl >= 1; the call takes wl = 0 with a null `low`: the one of rank k at position p is bit p + k of m_high"""
    bins, bin_size = 64, 50
    U = bins * bin_size
    rng = np.random.default_rng(300)
    pos = np.sort(rng.choice(U, 300, replace=False)).astype(np.int64)
    bits = np.zeros(U + pos.size, np.uint8)
    bits[pos + np.arange(pos.size)] = 1
    high = np.zeros((bits.size + 63) // 64 * 8, np.uint8)
    high[:(bits.size + 7) // 8] = np.packbits(bits, bitorder="little")
    want = np.zeros(U // 64, np.uint64)
    np.bitwise_or.at(want, pos >> 6, np.uint64(1) << (pos & 63).astype(np.uint64))
    case = dict(universe=U)
    bad, rows, per_bin = decoded(api.make_desc(bins, bin_size, [0] * bins, 1, 0), case, slice_words, wl=0, high=high.view(np.uint64),
                                 high_bits=bits.size, low=np.zeros(0, np.uint64))
    assert bad == 0
    assert np.array_equal(rows, want)
    assert np.array_equal(per_bin, np.bincount(pos % bins, minlength=bins).astype(np.uint64))
