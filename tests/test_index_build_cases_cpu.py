"""CPU tests of tests/index_build_cases.py: the cases of the GPU index-build tests say what their docstrings claim, and the rule by which
`charon index` cuts a record into chunks loses and invents no minimiser -- with the oracle alone, independently of any kernel.  That is
what makes the oracle's set of the whole record the reference of the chunked GPU calls."""
import numpy as np
import pytest

from tests import index_build_cases as cases
from tests import test_gpu_ring_pack as ring_pack

U64 = np.uint64


def test_kw_list_is_the_ring_pack_pairs_and_six_more():
    assert cases.KW_LIST[:len(ring_pack.KW)] == ring_pack.KW
    assert cases.KW_LIST[len(ring_pack.KW):] == [(4, 8), (1, 1), (11, 41), (15, 120), (5, 27), (19, 255)]
    assert len(cases.KW_LIST) == len(set(cases.KW_LIST)) == 14
    assert all(1 <= k <= 27 and k <= w <= 255 for k, w in cases.KW_LIST)
    assert set(cases.KW_CLI) <= set(cases.KW_LIST)


def test_kw_list_lies_on_both_sides_of_the_packing_rule():
    sides = {kw: cases.pack_ok(*kw) for kw in cases.KW_LIST}
    assert all(sides[kw] == ring_pack.pack_ok(*kw) for kw in cases.KW_LIST)   # the two restatements of ring_pack_ok agree
    assert [kw for kw in cases.KW_LIST if not sides[kw]] == [(27, 29), (26, 48), (25, 64)]
    assert sides[(19, 255)] and sides[(1, 1)] and sides[(27, 28)]
    wn = {kw: kw[1] - kw[0] + 1 for kw in cases.KW_LIST}
    assert [kw for kw in cases.KW_LIST if wn[kw] == 1] == [(21, 21), (1, 1)]
    assert [kw for kw in cases.KW_LIST if wn[kw] == 23] == [(19, 41), (26, 48), (5, 27)]   # the fixed-window width: at k = 19, unpacked, at a small k
    assert sides[(27, 29)] is False and {kw for kw in cases.KW_CLI if not sides[kw]} == {(27, 29)}


def test_the_cutting_rule_restated():
    assert cases.chunks(30000, 41) == [(c * 4096, 4096 + 40) for c in range(7)] + [(7 * 4096, 30000 - 7 * 4096)]
    assert cases.chunks(4096 + 40, 41) == [(0, 4136)]            # exactly 4 096 windows: one chunk
    assert cases.chunks(4096 + 41, 41) == [(0, 4136), (4096, 41)]  # one window more: a chunk of one window
    assert cases.chunks(40, 41) == [(0, 40)] and cases.chunks(18, 41) == [(0, 18)]   # shorter than w: the record as it is
    assert cases.chunks(8192, 1) == [(0, 4096), (4096, 4096)]
    for k, w in cases.KW_LIST:
        cs = cases.chunks(cases.RECORD_BASES, w)
        assert len(cs) == (cases.RECORD_BASES - w + 1 + 4095) // 4096 >= 7
        assert all(s % 64 == 0 and n >= w and s + n <= cases.RECORD_BASES for s, n in cs)   # a segment starts on a 64-base boundary
        assert all(b[0] - a[0] == 4096 and a[0] + a[1] - b[0] == w - 1 for a, b in zip(cs, cs[1:]))   # neighbours overlap by w - 1
        assert cs[-1][0] + cs[-1][1] == cases.RECORD_BASES


def test_the_record_has_n_runs_across_the_chunk_seams():
    rec = cases.chunked_record()
    assert len(rec) == cases.RECORD_BASES and set(rec) == set(b"ACGTN")
    for seam in (4096, 8192):
        assert rec[seam - 1:seam + 1] == b"NN"
    assert rec[4085:4101] == b"N" * 16 and rec[4084:4085] != b"N" and rec[4101:4102] != b"N"
    assert rec[8180:8300] == b"N" * 120 and rec[12287:12289] == b"NN"


@pytest.mark.parametrize("kw", cases.KW_LIST, ids=cases.kw_id)
def test_chunk_minimisers_unite_to_the_records(oracle_lib, kw):
    """the oracle's minimiser sets of the builder's chunks unite to the oracle's set of the whole record"""
    k, w = kw
    rec = cases.chunked_record()
    whole = np.unique(oracle_lib.minimisers(rec.decode(), k, w))
    parts = cases.oracle_minimisers(oracle_lib, [rec[s:s + n] for s, n in cases.chunks(len(rec), w)], k, w)
    assert whole.size > (100 if k >= 5 else 2)   # (k = 1 has three canonical values, k = 4 fewer than a hundred)
    np.testing.assert_array_equal(np.unique(np.concatenate(parts)), whole)
    assert sum(p.size for p in parts) >= whole.size


@pytest.mark.parametrize("kw", cases.KW_LIST, ids=cases.kw_id)
def test_every_pair_yields_minimisers_on_the_test_reads(oracle_lib, kw):
    k, w = kw
    reads, n_edge = cases.batch_reads(k, w)
    assert 20 <= n_edge <= 30 and len(reads) == n_edge + 201 and reads[:n_edge] == cases.edge_reads(k, w)
    assert [len(s) for s in reads[:11]] == [k - 1, k, w - 1, w, w + 1, 63, 64, 65, 128, 129, 4096 + w - 1]
    assert len(reads[n_edge]) == 40000
    mins = cases.oracle_minimisers(oracle_lib, reads, k, w)
    assert sum(m.size for m in mins) > 1000 and mins[n_edge].size > 100
    assert mins[0].size == 0 and mins[1].size == 1                      # k - 1 bases: nothing; k bases: one window
    assert all(m.size >= 1 for s, m in zip(reads, mins) if len(s) >= k and set(s) <= set(b"ACGT"))
    all_n = reads.index(b"N" * 300)
    assert all_n < n_edge
    # more than one wavefront, and the batch sizes of the GPU test are batches of these reads
    assert all(n is None or n < len(reads) for n in cases.BATCH_SIZES)


def test_emplace_cases():
    assert [cases.emplace_bins(b) for b in (1, 64, 65, 255)] == [[0], [0, 63], [0, 63, 64], [0, 63, 64, 254]]
    v = cases.emplace_values(np.random.default_rng(1), 4000)
    assert v.size == 4000 and 0 in v and cases.MAX in v and np.unique(v).size < v.size - 400
    for S in (20011, 65536):
        sh = cases.shard_ranges(S)
        assert sh[0] == (0, 1) and sh[1] == (S - 1, S) and 0 < sh[2][0] < sh[2][1] < S
        assert sh[3][0] == 0 and sh[3][1] == sh[4][0] and sh[4][1] == S


def test_fresh_values_are_not_in_the_pool():
    for seed in (31, 32):
        pool, fresh = cases.pool_and_fresh(seed)
        assert pool.size == cases.POOL and fresh.size == cases.FRESH == np.unique(fresh).size
        assert not np.isin(fresh, pool).any()
    assert cases.N_GRID == 65535 * 256 + 5000 and cases.N_PIECE == 2 ** 26 + 5000


def test_draws_then_fresh_is_what_it_says():
    v, uniq = cases.draws_then_fresh(31, cases.N_GRID)
    pool, fresh = cases.pool_and_fresh(31)
    assert v.size == cases.N_GRID and v.dtype == U64
    np.testing.assert_array_equal(v[-cases.FRESH:], fresh)           # the fresh values are the last ones: the second turn's
    np.testing.assert_array_equal(np.unique(v[:65535 * 256]), np.unique(pool))   # in front of them: the pool, all of it, and nothing else
    np.testing.assert_array_equal(uniq, np.unique(np.concatenate([pool, fresh])))
    assert uniq.size == np.unique(pool).size + cases.FRESH


def test_sort_sizes():
    assert cases.N_HIST == 2048 * 4096 + 4099 and (cases.N_HIST + 4095) // 4096 > 2048
    assert set(cases.TILE_SIZES) == {768, 65536}
    for t, ns in cases.TILE_SIZES.items():
        assert t % 256 == 0 and 256 <= t <= 65536 and ns[:3] == (t - 1, t, t + 1) and ns[3] > 3 * t
    assert (768 // 4) & (768 // 4 - 1) != 0 and 65536 // 4 // 64 == 256
