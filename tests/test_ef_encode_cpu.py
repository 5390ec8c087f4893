"""CPU tests of the Elias-Fano encode: chn_ef_layout_of (the layout rule) and chn_index_encode_ef_host (the rule source of
chn_index_encode_ef on one CPU thread, walking the same slices) against oracle.pyref.ef_encode; the jobs the call refuses."""
import ctypes as C

import numpy as np
import pytest

import charon_amd.api as api
from oracle import pyref
from tests import ef_encode_cases as cases


def desc_of(case, **kw):
    return api.make_desc(case["bins"], case["bin_size"], [0] * case["bins"], 1, 0, **kw)


@pytest.mark.parametrize("name,slice_rows", cases.RUNS)
def test_host_form_equals_the_reference_layout(name, slice_rows):
    case = cases.build(name)
    lay, low, high, ms = api.encode_ef_host(desc_of(case), case["words"], slice_rows)
    cases.assert_is_expected(case, lay, low, high)
    assert ms == 0
    if name == "straddle":  # (asserted from the layout: the case is there for elements that straddle two words)
        assert 64 % lay.wl != 0 and lay.ones > 64
    if name == "full_64x64":
        assert lay.wl == 1 and lay.high_bits == 4096 + (1 << 12)  # logm == logn == 13: logm is decremented


@pytest.mark.parametrize("name", [c[0] for c in cases.CASES] + [cases.SEAM[0]])
def test_numpy_reference_equals_pyref(name):
    """ef_encode_np is the reference of the large cases only as long as it is pyref.ef_encode on everything pyref can carry"""
    case = cases.build(name)
    wl, low_bits, low, high_bits, high = cases.ef_encode_np(case["pos"], case["universe"])
    assert (wl, low_bits, high_bits) == (case["wl"], case["low_bits"], case["high_bits"])
    assert low.dtype == np.uint64 and high.dtype == np.uint64
    assert np.array_equal(low, case["low"]) and np.array_equal(high, case["high"])
    if name == cases.SEAM[0]:
        assert 64 % wl != 0 and case["pos"].size > 64 * 3


@pytest.mark.parametrize("slice_rows", [0, cases.LARGE_SLICE_ROWS])
@pytest.mark.parametrize("name", list(cases.LARGE))
def test_host_form_on_slices_of_many_blocks(name, slice_rows):
    """thousands of 256-word blocks a slice, as one slice and at 1025 blocks a slice (the builder asserts the shapes' conditions)"""
    case = cases.build_large(name)
    lay, low, high, _ = api.encode_ef_host(desc_of(case), case["words"], slice_rows)
    cases.assert_is_expected(case, lay, low, high)
    assert cases.prefix_chunks(case["high"].size) >= cases.LARGE[name]["decode_rounds"]
    assert cases.prefix_chunks(case["words"].size) >= 3 and cases.prefix_chunks(cases.LARGE_SLICE_ROWS) == 2


class _Counted:
    """a position list of `n` entries that are never looked at: pyref.ef_encode takes wl and the bit counts from its length alone"""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter(())


def test_layout_rule_around_powers_of_two():
    around = sorted({max(1, (1 << p) + d) for p in range(0, 41) for d in (-1, 0, 1)})
    n = 0
    for m_size in around:
        for ones in [0] + around:
            if ones > m_size:
                continue
            wl, low_bits, _, high_bits, _ = pyref.ef_encode(_Counted(ones), m_size)
            lay = api.ef_layout_of(m_size, ones)
            assert (lay.struct_size, lay.wl, lay.m_size, lay.ones) == (C.sizeof(api.EfLayout), wl, m_size, ones), (m_size, ones)
            assert (lay.low_bits, lay.high_bits) == (low_bits, high_bits), (m_size, ones)
            assert (lay.n_low_words, lay.n_high_words) == ((low_bits + 63) // 64, (high_bits + 63) // 64)
            assert lay.wl >= 1
            n += 1
    assert n > 5000
    lay = api.ef_layout_of(6400, 0)  # no ones: logm = 1, no low words, two high bits
    assert (lay.wl, lay.n_low_words, lay.high_bits, lay.n_high_words) == (12, 0, 2, 1)
    with pytest.raises(api.ChnError) as e:
        api.ef_layout_of(100, 101)
    assert e.value.code == api.E_INVALID
    assert api.lib().chn_ef_layout_of(100, 5, None) == api.E_INVALID


def test_struct_sizes():
    assert C.sizeof(api.EfLayout) == 56
    assert C.sizeof(api.EfEncodeJob) == 72


def test_invalid_jobs_leave_the_arrays_alone():
    case = cases.build("straddle")
    d = desc_of(case)
    words = case["words"]
    L = api.lib()
    good = api.ef_layout_of(case["universe"], case["pos"].size)
    mark = 0x5A5A5A5A5A5A5A5A

    def refused(change=None, layout=good, desc=d, n_low=None, n_high=None, null_job=False):
        low = np.full(layout.n_low_words + 2 if n_low is None else n_low, mark, np.uint64)
        high = np.full(layout.n_high_words + 2 if n_high is None else n_high, mark, np.uint64)
        job, _, _ = api.ef_encode_job(layout, 0, low, high)
        if n_low is None:
            job.n_low_words = layout.n_low_words
        if n_high is None:
            job.n_high_words = layout.n_high_words
        if change:
            change(job)
        rc = L.chn_index_encode_ef_host(C.byref(desc), words.ctypes.data, None if null_job else C.byref(job))
        assert rc == api.E_INVALID, rc
        assert (low == mark).all() and (high == mark).all()
        return L.chn_last_error().decode()

    assert "null job" in refused(null_job=True)
    assert "struct_size" in refused(lambda j: setattr(j, "struct_size", j.struct_size - 8))
    assert "flag" in refused(lambda j: setattr(j, "flags", 1))
    assert "null layout" in refused(lambda j: setattr(j, "layout", C.POINTER(api.EfLayout)()))
    assert "sizes" in refused(n_low=good.n_low_words + 1)
    assert "sizes" in refused(n_low=good.n_low_words - 1)
    assert "sizes" in refused(n_high=good.n_high_words + 1)
    assert "sizes" in refused(n_high=good.n_high_words - 1)
    # a layout that is right in itself, for a count of ones that is not the words'
    for other in (case["pos"].size - 1, case["pos"].size + 1, 0):
        assert "set bits" in refused(layout=api.ef_layout_of(case["universe"], other))
    # a layout that is not the rule's: one field changed
    bent = api.EfLayout.from_buffer_copy(good)
    bent.wl += 1
    assert "layout" in refused(layout=bent)
    bent = api.EfLayout.from_buffer_copy(good)
    bent.struct_size = 48
    assert "struct_size" in refused(layout=bent)
    assert "m_size" in refused(layout=api.ef_layout_of(case["universe"] + 64, case["pos"].size))
    # a row shard has no Elias-Fano arrays of its own
    assert "row shard" in refused(desc=desc_of(case, row_begin=0, row_end=case["bin_size"] // 2))
    assert "row shard" in refused(desc=desc_of(case, row_begin=10, row_end=case["bin_size"]))
    # and the untouched job is fine: the call clears and writes every word, whatever was there
    low = np.full(good.n_low_words, mark, np.uint64)
    high = np.full(good.n_high_words, mark, np.uint64)
    job, _, _ = api.ef_encode_job(good, 0, low, high)
    assert L.chn_index_encode_ef_host(C.byref(d), words.ctypes.data, C.byref(job)) == 0
    cases.assert_is_expected(case, good, low, high)
    assert job.ones_written == good.ones
