"""The cases of tests/test_gpu_row_sharded.py, checked without a GPU: every case must reach, by the model of tests/sharded_cases.py
(the oracle's minimisers, row function and index words), the branch of the row-sharded chains it is there for.  These are
conditions on the inputs; the GPU tests run the same seeded bytes."""
import numpy as np
import pytest

from tests import sharded_cases as sc


def test_model_agrees_with_the_oracle_index(oracle_lib):
    """the model's pieces against the oracle's own lookups: minimiser counts against process_reads, ANDed rows against bulk_contains"""
    for name in ("w3", "paired12", "h5", "nruns"):
        c = sc.case(name)
        m = c.model()
        assert np.array_equal(np.bincount(m["read_of"], minlength=len(c.reads)), c.oracle()["num_hashes"])
        for e in range(0, len(m["values"]), max(1, len(m["values"]) // 200)):
            assert np.array_equal(m["anded"][e], c.oidx.bulk_contains(m["values"][e]))
        assert m["rows"].shape == (len(m["values"]), c.oidx.hash_funs) and m["rows"].min() >= 0 and m["rows"].max() < c.oidx.bin_size


@pytest.mark.parametrize("name,W,bins", [("w3", 3, 130), ("w4", 4, 200)])
def test_wide_rows_have_a_partial_last_word_in_use(oracle_lib, name, W, bins):
    c = sc.case(name)
    assert c.oidx.bin_words == W and c.oidx.bins == bins and bins & 63
    m = c.model()
    last = sc.mask_to_bins(m["anded"], bins)[:, -1]
    assert (last != 0).sum() >= 100
    # (the index holds nothing in the technical bins behind B: the mask of the last word is tested by the bins in front of it)
    assert not (m["anded"][:, -1] >> np.uint64(bins & 63)).any()
    assert len(c.reads) <= 400 and max(len(s) for s in c.reads) <= 2000


@pytest.mark.parametrize("name,W", [("esc1", 1), ("w3", 3)])
def test_escape_within_capacity(oracle_lib, name, W):
    c = sc.case(name)
    assert c.oidx.bin_words == W
    m = c.model()
    frac = m["n_escaped"] / len(m["values"])
    assert 0.02 <= frac <= 0.08, frac
    assert m["n_escaped"] >= 500
    for (n_min, n_esc), (cap, ecap) in zip(sc.group_counts(m, c.reads), sc.sparse_caps(c.oidx, c.reads)):
        assert n_esc >= 1
        assert n_esc <= ecap // 2, (n_esc, ecap)
        assert n_min <= cap  # (the minimiser log itself holds)


def test_escape_beyond_capacity(oracle_lib):
    c = sc.case("over")
    assert c.oidx is sc.case("esc1").oidx  # one stream can run both batches
    m = c.model()
    over = [n_esc > ecap for (n_min, n_esc), (cap, ecap) in zip(sc.group_counts(m, c.reads), sc.sparse_caps(c.oidx, c.reads))]
    assert any(over)
    assert all(n_min <= cap for (n_min, _), (cap, _) in zip(sc.group_counts(m, c.reads), sc.sparse_caps(c.oidx, c.reads)))


def test_region_sizes_restated(oracle_lib):
    """the two formulas at known values: 64 reads of 1 000 bases at (19, 41) -- cap_num 10 923 -- and the 128-bin threshold of esc_shift"""
    c = sc.case("esc1")
    assert sc.wave_log_cap(64000, 10923) == 10752 and sc.wave_esc_cap(10752, 3) == 1408 and sc.wave_esc_cap(10752, 1) == 5440
    reads = [b"A" * 1000] * 64 + [b"A" * 10]
    assert sc.sparse_caps(c.oidx, reads) == [(10752, 1408), (128, 80)]
    assert [sc.len_bucket(n) for n in (0, 7, 8, 15, 16, 1000, 32767, 32768, 40000)] == [0, 7, 8, 15, 16, 63, 103, 104, 105]
    assert sc.groups([b"A" * 5, b"A" * 600, b"A" * 5, b"A" * 601]) == [[1, 3, 0, 2]]


def test_sixteen_owner_split(oracle_lib):
    c = sc.case("w2")
    S = c.oidx.bin_size
    assert c.oidx.bin_words == 2 and len(c.reads) == 1 + 63 + 64 + 200
    sp = sc.owner_splits16(S, c.model()["rows"])
    assert len(sp) == 17 and sp[0] == 0 and sp[-1] == S and all(a <= b for a, b in zip(sp[:-1], sp[1:]))
    size = np.diff(sp)
    empty = [r for r in range(16) if size[r] == 0]
    assert empty == [0, 7, 8, 15]
    assert 1 in size and 17 in size
    m = c.model(sp)
    assert m["counts"][list(size).index(17)] >= 1 and m["counts"][list(size).index(1)] >= 1
    assert all(m["counts"][r] == 0 for r in empty)
    assert np.isin(m["rows"], sp[1:-1]).any()  # a probe row that equals a split exactly
    # every owner that holds rows is asked for some by the batch
    assert all(m["counts"][r] > 0 for r in range(16) if r not in empty)
    # the model's owner against the definition, independently of searchsorted
    rows, own = m["rows"].ravel(), m["owner"].ravel()
    assert all(sp[o] <= x < sp[o + 1] for x, o in zip(rows[::97], own[::97]))


def test_long_read_case(oracle_lib):
    c = sc.case("long")
    lens = [len(s) for s in c.reads]
    assert max(lens) == 40000 and sorted(lens)[-2] <= 2000
    i = lens.index(40000)
    assert len(c.model()["per_read"][i]) >= 2500
    first = sc.groups(c.reads)[0]
    assert first[0] == i and len(first) == 64 and all(lens[j] <= 2000 for j in first[1:])
    # hits the index it was sampled from
    assert c.oracle()["counts"][i, 0] > 1500


def test_no_minimiser_case(oracle_lib):
    c = sc.case("nomin")
    assert all(len(s) < c.oidx.k for s in c.reads) and any(len(s) == 0 for s in c.reads)
    assert len(c.model()["values"]) == 0 and c.model()["counts"] == [0]
    assert not c.oracle()["num_hashes"].any()


def test_tiny_log_case_fits(oracle_lib):
    """the batch a CHN_STREAM_TINY_LOG stream (cap_num 64, esc_shift 6) must hold: fewer minimisers than one region's 64 entries; the
    large batch of the same index overruns such a region in every group"""
    c = sc.case("w2_tiny")
    assert 0 < len(c.model()["values"]) < 64 and len(sc.groups(c.reads)) == 1
    big = sc.case("w2")
    for (n_min, _), g in zip(sc.group_counts(big.model(), big.reads), sc.groups(big.reads)):
        cap = sc.wave_log_cap(sum(len(big.reads[i]) for i in g), 64)
        if len(g) == 64:
            assert n_min > cap


def test_mode_list_inputs(oracle_lib):
    c = sc.case("paired12")
    assert c.mates is not None and c.oidx.ncat == 12 and len(c.reads) == len(c.mates) == 250
    c = sc.case("nruns")
    assert sum(b"N" in s for s in c.reads) >= 200
    for name, k, w in (("kw_15_15", 15, 15), ("kw_27_31", 27, 31), ("kw_5_200", 5, 200)):
        c = sc.case(name)
        assert (c.oidx.k, c.oidx.w) == (k, w) and len(c.model()["values"]) > 100
    for name, h in (("h1", 1), ("h5", 5)):
        c = sc.case(name)
        assert c.oidx.hash_funs == h and c.model()["rows"].shape[1] == h
        assert (c.oracle()["call"] != 255).any()
