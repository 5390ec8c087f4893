"""GPU tests (-m gpu) of the calls `charon index` is made of, each against the CPU oracle or numpy, never against a second GPU call:
chn_minimisers / chn_minimisers_into (the list form of the probe kernel and k_compact_list) for every (k, w) of
index_build_cases.KW_LIST -- whole batches, single reads, the record cut into the builder's chunks, a buffer one value short;
chn_index_emplace / chn_index_emplace_set (k_emplace_values) against Index.new(...).emplace_many for 1 to 5 hash functions, 1 to 4 words
a row, row shards and a bin of about 2^27 rows; and sizes past every clipped grid and host piece: a second turn of k_emplace_values,
the second host piece of chn_index_emplace, the clipped grid of k_radix_hist, and the tiles 768 and 65 536 of the sort.
Every comparison is of integers and exact."""
import ctypes as C

import numpy as np
import pytest

from tests import index_build_cases as cases
from tests import util
from tests.test_gpu_hashset import contents

pytestmark = pytest.mark.gpu
U64 = np.uint64
MAX = cases.MAX
GUARD = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def api():
    import charon_amd.api as api
    return api


def probe_index(api, k, w):
    return api.Index(api.make_desc(1, 64, [0], 1, 255, k=k, w=w))


_REFERENCE = {}


def reference(po, kw):
    """(reads, edge reads among them, the oracle's minimisers of every read, the packed full batch) -- made once per pair, never changed"""
    if kw not in _REFERENCE:
        from charon_amd import pack
        reads, n_edge = cases.batch_reads(*kw)
        mins = cases.oracle_minimisers(po, reads, *kw)
        for m in mins:
            m.setflags(write=False)
        _REFERENCE[kw] = (reads, n_edge, mins, pack.pack_reads(reads))
    return _REFERENCE[kw]


class Probe:
    """a 1-bin index of (k, w) and a stream on it, as `charon index` has them"""

    def __init__(self, api, kw, max_reads, max_bases):
        self.st = None
        self.idx = probe_index(api, *kw)
        try:
            self.st = api.Stream(self.idx, max_reads, max_bases)
        except Exception:
            self.idx.destroy()
            raise

    def destroy(self):
        if self.st:
            self.st.destroy()
        self.idx.destroy()


# ---- 1. chn_minimisers / chn_minimisers_into against the oracle -----------------------------------------------------------------------
@pytest.mark.parametrize("kw", cases.KW_LIST, ids=cases.kw_id)
def test_minimisers_of_whole_batches(api, oracle_lib, kw):
    """batches of 1, 63, 64, 65 reads and of all of them: the sorted values are the sorted concatenation of the oracle's"""
    from charon_amd import pack
    reads, n_edge, mins, full = reference(oracle_lib, kw)
    p = Probe(api, kw, len(reads), full["n_bases"])
    try:
        for n in cases.BATCH_SIZES:
            batch = full if n is None else pack.pack_reads(reads[:n])
            want = cases.sorted_concat(mins[:n])
            got = p.st.minimisers_host(batch)
            assert got.size == want.size, (kw, n, got.size, want.size)
            np.testing.assert_array_equal(np.sort(got), want, err_msg=str((kw, n)))
        assert want.size > 1000
    finally:
        p.destroy()


@pytest.mark.parametrize("kw", cases.KW_LIST, ids=cases.kw_id)
def test_minimisers_of_single_reads(api, oracle_lib, kw):
    """every edge read as a batch of its own: an error is placed in a read"""
    from charon_amd import pack
    reads, n_edge, mins, full = reference(oracle_lib, kw)
    p = Probe(api, kw, 64, 8192)
    try:
        for i in range(n_edge):
            got = p.st.minimisers_host(pack.pack_reads([reads[i]]))
            np.testing.assert_array_equal(np.sort(got), np.sort(mins[i]), err_msg=str((kw, i, len(reads[i]), reads[i][:60])))
    finally:
        p.destroy()


@pytest.mark.parametrize("kw", cases.KW_LIST, ids=cases.kw_id)
def test_minimisers_of_the_chunked_record(api, oracle_lib, kw):
    """the record as the builder hands it over, every chunk a read of its own: the multiset is the oracle's of the chunks' substrings, its
    distinct values the oracle's set of the whole record -- through chn_minimisers and through chn_minimisers_into and unique()"""
    k, w = kw
    rec = cases.chunked_record()
    batch, cs = cases.chunked_batch(rec, w)
    want = cases.sorted_concat(cases.oracle_minimisers(oracle_lib, [rec[s:s + n] for s, n in cs], k, w))
    whole = np.unique(oracle_lib.minimisers(rec.decode(), k, w))
    p = Probe(api, kw, len(cs), batch["n_bases"])
    hs = api.HashSet()
    try:
        got = p.st.minimisers_host(batch)
        np.testing.assert_array_equal(np.sort(got), want)
        np.testing.assert_array_equal(np.unique(got), whole)
        assert p.st.minimisers_into(batch, hs) == want.size
        assert hs.size()[0] == want.size
        np.testing.assert_array_equal(np.sort(hs.download()), want)
        assert hs.unique() == whole.size
        np.testing.assert_array_equal(hs.download(), whole)
    finally:
        hs.destroy()
        p.destroy()


@pytest.mark.parametrize("kw", cases.KW_LIST, ids=cases.kw_id)
def test_minimisers_with_a_buffer_one_value_short(api, oracle_lib, kw):
    """capacity = total - 1: CHN_E_CAPACITY with the count reported, nothing written; the same batch then succeeds on the same stream"""
    reads, n_edge, mins, full = reference(oracle_lib, kw)
    want = cases.sorted_concat(mins)
    L = api.lib()
    p = Probe(api, kw, len(reads), full["n_bases"])
    try:
        b, keep, n = p.st._host_batch(full, None, None)
        buf = np.full(want.size + 4, GUARD, U64)
        e = C.c_uint64()
        assert L.chn_minimisers(p.st.h, C.byref(b), buf[2:].ctypes.data, want.size - 1, C.byref(e)) == api.E_CAPACITY
        assert e.value == want.size and (buf == GUARD).all()
        assert L.chn_minimisers(p.st.h, C.byref(b), None, 0, C.byref(e)) == api.E_CAPACITY and e.value == want.size
        assert L.chn_minimisers(p.st.h, C.byref(b), buf[2:].ctypes.data, want.size, C.byref(e)) == 0
        assert e.value == want.size and (buf[:2] == GUARD).all() and (buf[-2:] == GUARD).all()
        np.testing.assert_array_equal(np.sort(buf[2:-2]), want)
    finally:
        p.destroy()


# ---- 2. chn_index_emplace / chn_index_emplace_set against Index.new(...).emplace_many -------------------------------------------------
def oracle_index(po, bins, S, h):
    return po.Index.new(bins, S, [0] * bins, ["c"], nhash=h)


def desc_of(api, bins, S, h, rows=(0, 0)):
    return api.make_desc(bins, S, [0] * bins, 1, 255, hash_funs=h, row_begin=rows[0], row_end=rows[1])


@pytest.mark.parametrize("h", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("bins", [1, 64, 65, 255])
def test_emplace_against_the_oracle(api, oracle_lib, bins, h):
    """both calls, over random words uploaded first (earlier bits stay), and a set made unique: the words the oracle has"""
    for S in (20011, 65536):
        r = util.rng(1000 * bins + 10 * h + S % 7)
        o = oracle_index(oracle_lib, bins, S, h)
        a, b, d = (api.Index(desc_of(api, bins, S, h)) for _ in range(3))
        sets = []
        try:
            assert o.bin_words == (bins + 63) // 64 and o.hash_funs == h and o.words().size == S * o.bin_words
            before = r.integers(0, MAX, S * o.bin_words, dtype=U64, endpoint=True) & r.integers(0, MAX, S * o.bin_words, dtype=U64, endpoint=True)
            for g in (a, b, d):
                g.upload(before)
            for bin_index in cases.emplace_bins(bins):
                v = cases.emplace_values(r, 3000 + 17 * bin_index)
                o.emplace_many(v, bin_index)
                a.emplace(v, bin_index)
                for g, make_unique in ((b, False), (d, True)):
                    hs = api.HashSet()
                    sets.append(hs)
                    hs.append(v)
                    if make_unique:
                        assert hs.unique() == np.unique(v).size
                    g.emplace_set(hs, bin_index)
            assert o.words().any()
            want = before | o.words()
            assert (want != before).any()
            for name, g in (("emplace", a), ("emplace_set", b), ("emplace_set of a unique set", d)):
                assert np.array_equal(g.download(), want), (name, bins, h, S)
        finally:
            for hs in sets:
                hs.destroy()
            for g in (a, b, d):
                g.destroy()
            o.free()


@pytest.mark.parametrize("bins,h", [(1, 1), (65, 3), (255, 5)])
def test_emplace_into_row_shards(api, oracle_lib, bins, h):
    """the device rows of a shard are the same rows of the oracle's whole index; two adjacent shards side by side are the whole index"""
    for S in (20011, 65536):
        r = util.rng(77 + bins + S % 5)
        o = oracle_index(oracle_lib, bins, S, h)
        W = o.bin_words
        per_bin = [(bin_index, cases.emplace_values(r, 2500)) for bin_index in cases.emplace_bins(bins)]
        for bin_index, v in per_bin:
            o.emplace_many(v, bin_index)
        whole = o.words().reshape(S, W)
        got = {}
        try:
            for rows in cases.shard_ranges(S):
                for use_set in (False, True):
                    g = api.Index(desc_of(api, bins, S, h, rows))
                    sets = []
                    try:
                        for bin_index, v in per_bin:
                            if use_set:
                                hs = api.HashSet()
                                sets.append(hs)
                                hs.append(v)
                                g.emplace_set(hs, bin_index)
                            else:
                                g.emplace(v, bin_index)
                        got[rows] = g.download(rows[0], rows[1] - rows[0])
                        assert np.array_equal(got[rows].reshape(-1, W), whole[rows[0]:rows[1]]), (rows, use_set, bins, h, S)
                    finally:
                        for hs in sets:
                            hs.destroy()
                        g.destroy()
            sh = cases.shard_ranges(S)
            assert np.array_equal(np.concatenate([got[sh[3]], got[sh[4]]]), o.words())
            assert whole[sh[2][0]:sh[2][1]].any() and whole[:sh[3][1]].any() and whole[sh[4][0]:].any()
        finally:
            o.free()


def test_emplace_hits_the_first_and_the_last_row(api, oracle_lib):
    """values chosen (with the oracle's hash) to fall into row 0 and row S - 1: the one-row shards [0, 1) and [S - 1, S) hold their bits,
    and a value of neither leaves them empty"""
    S, h, bins = 20011, 3, 65
    L = oracle_lib.lib()
    r = util.rng(123)
    cand = r.integers(0, MAX, 60000, dtype=U64, endpoint=True)
    rows = np.array([[L.orc_hash_and_fit(int(x), j, S) for j in range(h)] for x in cand])
    first, last = cand[(rows == 0).any(axis=1)], cand[(rows == S - 1).any(axis=1)]
    other = cand[~((rows == 0) | (rows == S - 1)).any(axis=1)][:100]
    assert first.size and last.size
    for rng_, mine in (((0, 1), first), ((S - 1, S), last)):
        o = oracle_index(oracle_lib, bins, S, h)
        g = api.Index(desc_of(api, bins, S, h, rng_))
        try:
            g.emplace(other, 64)
            assert not g.download(rng_[0], 1).any()
            g.emplace(mine, 64)
            o.emplace_many(np.concatenate([other, mine]), 64)
            want = o.words().reshape(S, 2)[rng_[0]]
            assert want.any()
            assert np.array_equal(g.download(rng_[0], 1), want)
        finally:
            g.destroy()
            o.free()


def test_emplace_into_a_bin_of_about_2_to_the_27_rows(api, oracle_lib):
    """1 bin of 2^27 - 39 rows (the fastrange shift of a large bin; 1 GiB of rows on the device): both calls against the oracle, the rows
    compared a slice at a time"""
    S, h = 2 ** 27 - 39, 3
    r = util.rng(27)
    v = cases.emplace_values(r, 1 << 20)
    o = oracle_index(oracle_lib, 1, S, h)
    a = api.Index(desc_of(api, 1, S, h))
    hs = api.HashSet()
    try:
        o.emplace_many(v, 0)
        want = o.words()
        assert want.size == S
        a.emplace(v[:v.size // 2], 0)
        hs.append(v[v.size // 2:])
        a.emplace_set(hs, 0)
        step = 1 << 24
        ones = 0
        for row in range(0, S, step):
            n = min(step, S - row)
            got = a.download(row, n)
            assert np.array_equal(got, want[row:row + n]), row
            ones += int(np.count_nonzero(got))
        assert ones > 2 * np.unique(v).size   # (h rows a value, few collisions in 2^27 rows)
    finally:
        hs.destroy()
        a.destroy()
        o.free()


# ---- 3. past every clipped grid and host piece ------------------------------------------------------------------------------------------
BIG = dict(bins=70, S=2 ** 22 - 3, h=5, bin_index=67)


def big_reference(po, uniq):
    o = oracle_index(po, BIG["bins"], BIG["S"], BIG["h"])
    o.emplace_many(uniq, BIG["bin_index"])
    return o


def assert_big_index(g, o):
    S, step = BIG["S"], 1 << 20
    want = o.words().reshape(S, 2)
    assert np.count_nonzero(want) > 4 * (cases.POOL + cases.FRESH)
    for row in range(0, S, step):
        n = min(step, S - row)
        assert np.array_equal(g.download(row, n).reshape(n, 2), want[row:row + n]), row


@pytest.mark.parametrize("call", ["emplace", "emplace_set"])
def test_a_second_turn_of_the_emplace_kernel(api, oracle_lib, call):
    """65 535 * 256 + 5 000 values: the grid is clipped at 65 535 workgroups, the last 5 000 values -- which are nowhere else -- are set
    by threads on their second turn.  The set was appended to and not made unique."""
    v, uniq = cases.draws_then_fresh(31, cases.N_GRID)
    o = big_reference(oracle_lib, uniq)
    g = api.Index(desc_of(api, BIG["bins"], BIG["S"], BIG["h"]))
    hs = api.HashSet()
    try:
        if call == "emplace":
            g.emplace(v, BIG["bin_index"])
        else:
            hs.append(v[:1000])
            hs.append(v[1000:])
            assert hs.size()[0] == v.size
            g.emplace_set(hs, BIG["bin_index"])
        assert_big_index(g, o)
    finally:
        hs.destroy()
        g.destroy()
        o.free()


def test_the_second_host_piece_of_emplace(api, oracle_lib):
    """2^26 + 5 000 values: chn_index_emplace uploads 2^26 at a time, the 5 000 fresh values are the second piece"""
    v, uniq = cases.draws_then_fresh(32, cases.N_PIECE)
    o = big_reference(oracle_lib, uniq)
    g = api.Index(desc_of(api, BIG["bins"], BIG["S"], BIG["h"]))
    try:
        g.emplace(v, BIG["bin_index"])
        assert_big_index(g, o)
    finally:
        g.destroy()
        o.free()


def check_sort(api, keys, tile_keys, what):
    keys = np.asarray(keys, U64)
    want = np.unique(keys)
    hs = api.HashSet(0, tile_keys)
    try:
        hs.append(keys)
        assert hs.size()[0] == keys.size
        d = hs.unique()
        assert d == want.size, (what, d, want.size)
        n, held = hs.size()
        assert n == d
        if keys.size >= 2:
            assert held == 8 * want.size, what   # the memory rule: a buffer of exactly the distinct values
        np.testing.assert_array_equal(hs.download(), want, err_msg=str(what))
    finally:
        hs.destroy()


def test_sort_past_the_clipped_histogram_grid(api):
    """2 048 * 4 096 + 4 099 random values at the default tile: k_radix_hist is launched with its 2 048 workgroups and loops"""
    keys = util.rng(41).integers(0, MAX, cases.N_HIST, dtype=U64, endpoint=True)
    keys[-3:] = (0, MAX, keys[0])
    check_sort(api, keys, 0, "random")


@pytest.mark.parametrize("tile_keys", sorted(cases.TILE_SIZES))
def test_sort_sizes_at_the_tiles_768_and_65536(api, tile_keys):
    r = util.rng(tile_keys)
    for n in cases.TILE_SIZES[tile_keys]:
        check_sort(api, r.integers(0, MAX, n, dtype=U64, endpoint=True), tile_keys, ("random", n))
        check_sort(api, r.integers(0, 40, n, dtype=U64), tile_keys, ("forty values", n))


@pytest.mark.parametrize("tile_keys", sorted(cases.TILE_SIZES))
def test_sort_contents_at_the_tiles_768_and_65536(api, tile_keys):
    """the random, forty-values and runs-across-seams contents of tests/test_gpu_hashset.py, at 3 tiles + 5 keys"""
    r = util.rng(50 + tile_keys)
    c = contents(r, tile_keys)
    n = 3 * tile_keys + 5
    c["forty values"] = r.integers(0, 40, n, dtype=U64)
    for what in ("random", "forty values", "runs across seams"):
        assert c[what].size == n
        check_sort(api, c[what], tile_keys, what)
