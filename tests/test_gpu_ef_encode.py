"""GPU tests of chn_index_encode_ef (k_ef_encode): the shared cases through Index.encode_ef against oracle.pyref.ef_encode, back through
chn_index_decode_ef to the uploaded rows, and field by field against the host form; the calls' refusals and their wait for queued work."""
import ctypes as C

import numpy as np
import pytest

import charon_amd.api as api
from tests import ef_encode_cases as cases

pytestmark = pytest.mark.gpu


def desc_of(case, **kw):
    return api.make_desc(case["bins"], case["bin_size"], [0] * case["bins"], 1, 0, **kw)


def uploaded(case):
    g = api.Index(desc_of(case))
    g.upload(case["words"])
    return g


@pytest.mark.parametrize("name,slice_rows", cases.RUNS)
def test_device_form(name, slice_rows):
    case = cases.build(name)
    g = uploaded(case)
    try:
        lay = g.ef_layout()
        lay2, low, high, ms = g.encode_ef(slice_rows)
        # (1) the reference layout, word for word
        cases.assert_is_expected(case, lay, low, high)
        assert bytes(lay) == bytes(lay2)
        assert ms >= 0
        if name == "straddle":
            assert 64 % lay.wl != 0 and lay.ones > 64
        # (2) the host form, field by field
        hlay, hlow, hhigh, _ = api.encode_ef_host(desc_of(case), case["words"], slice_rows)
        for f, _t in api.EfLayout._fields_:
            assert getattr(lay, f) == getattr(hlay, f), f
        assert np.array_equal(low, hlow) and np.array_equal(high, hhigh)
    finally:
        g.destroy()
    # (3) the round trip through the loader's decode gives back the uploaded rows (bits in technical-only bins are what the decode
    # reports instead of setting: they are encoded as they stand and counted there)
    tb, bins = case["tb"], case["bins"]
    real = case["pos"][case["pos"] % tb < bins]
    want = np.zeros(case["universe"] // 64, np.uint64)
    np.bitwise_or.at(want, real >> 6, np.uint64(1) << (real & 63).astype(np.uint64))
    g2 = api.Index(desc_of(case))
    try:
        bad = g2.decode_ef(case["universe"], lay.wl, high, lay.high_bits, low, slice_words=1000)
        assert bad == case["pos"].size - real.size
        assert np.array_equal(g2.download(), want)
        if name != "technical_only_bins":
            assert bad == 0 and np.array_equal(want, case["words"])
    finally:
        g2.destroy()


def test_a_row_shard_is_refused():
    case = cases.build("straddle")
    half = case["bin_size"] // 2
    for kw in (dict(row_begin=0, row_end=half), dict(row_begin=half, row_end=case["bin_size"])):
        g = api.Index(desc_of(case, **kw))
        try:
            with pytest.raises(api.ChnError) as e:
                g.ef_layout()
            assert e.value.code == api.E_INVALID and "row shard" in str(e.value)
            lay = api.ef_layout_of(case["universe"], 0)
            job, low, high = api.ef_encode_job(lay)
            assert api.lib().chn_index_encode_ef(g.h, C.byref(job)) == api.E_INVALID
            assert "row shard" in api.lib().chn_last_error().decode()
            assert (high == np.uint64(2 ** 64 - 1)).all()
        finally:
            g.destroy()


def test_invalid_jobs_leave_the_arrays_alone():
    case = cases.build("ones_2j")
    g = uploaded(case)
    L = api.lib()
    mark = np.uint64(2 ** 64 - 1)
    try:
        good = g.ef_layout()
        for layout, change, word in ((good, lambda j: setattr(j, "flags", 2), "flag"),
                                     (good, lambda j: setattr(j, "struct_size", 64), "struct_size"),
                                     (good, lambda j: setattr(j, "n_high_words", j.n_high_words - 1), "sizes"),
                                     (good, lambda j: setattr(j, "n_low_words", j.n_low_words + 1), "sizes"),
                                     (good, lambda j: setattr(j, "layout", C.POINTER(api.EfLayout)()), "null layout"),
                                     (api.ef_layout_of(case["universe"], good.ones + 1), None, "set bits")):
            job, low, high = api.ef_encode_job(layout)
            if change:
                change(job)
            assert L.chn_index_encode_ef(g.h, C.byref(job)) == api.E_INVALID
            assert word in L.chn_last_error().decode()
            assert (low == mark).all() and (high == mark).all()
        assert L.chn_index_encode_ef(g.h, None) == api.E_INVALID
        assert L.chn_index_encode_ef(None, None) == api.E_INVALID
        assert L.chn_index_ef_layout(g.h, None) == api.E_INVALID
    finally:
        g.destroy()


def test_encode_right_behind_queued_decode_slices_sees_all_of_them():
    """chn_index_decode_ef queues a slice's work and returns; the layout call and the encode wait for what is queued"""
    case = cases.build("decode_100x5000")
    high, low, wl = case["high"], case["low"], case["wl"]
    L = api.lib()
    g = api.Index(desc_of(case))
    try:
        # the slices of Index.decode_ef without its closing call, which is the one that waits
        slice_words, ones_before = 257, 0
        pop = api._POP8
        for w0 in range(0, high.size, slice_words):
            hs = np.ascontiguousarray(high[w0:w0 + slice_words])
            ones = int(pop[hs.view(np.uint8)].sum())
            if ones == 0:
                continue
            elem0 = ones_before & ~63
            ls = np.ascontiguousarray(low[elem0 * wl // 64:((ones_before + ones) * wl + 63) // 64])
            bad = C.c_uint64()
            assert L.chn_index_decode_ef(g.h, case["universe"], wl, hs.ctypes.data, w0 * 64, hs.size, ones_before, ls.ctypes.data, elem0, ls.size,
                                         C.byref(bad)) == 0
            ones_before += ones
        lay, elow, ehigh, _ = g.encode_ef(100)
        cases.assert_is_expected(case, lay, elow, ehigh)
        assert np.array_equal(g.download(), case["words"])
    finally:
        g.destroy()
