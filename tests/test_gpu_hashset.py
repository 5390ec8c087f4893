"""GPU tests of the device-resident minimiser sets (chn_hashset): the radix sort and unique pass against numpy.unique at the default tile
and at the smallest one (tile_keys = 256, where a small array spans many tiles and more than one round of the one-workgroup scans),
over sizes around the wavefront, the workgroup and the tile and over contents that make the sort skip passes; chn_minimisers_into
against chn_minimisers; chn_index_emplace_set against chn_index_emplace.  The expected value is never the code under test."""
import ctypes as C

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu
TILES = (0, 256)          # chn_hashset_cfg.tile_keys: the default and the test hook's smallest
U64 = np.uint64
MAX = 2 ** 64 - 1


@pytest.fixture(scope="module")
def api():
    import charon_amd.api as api
    return api


def tile_of(tile_keys):
    return tile_keys or 4096


def sorted_unique(api, keys, tile_keys):
    """(count unique() returns, the set downloaded behind it, bytes held)"""
    hs = api.HashSet(0, tile_keys)
    try:
        hs.append(keys)
        assert hs.size()[0] == len(keys)
        d = hs.unique()
        n, held = hs.size()
        assert n == d
        return d, hs.download(), held
    finally:
        hs.destroy()


def check(api, keys, tile_keys, what):
    keys = np.asarray(keys, U64)
    want = np.unique(keys)
    d, got, held = sorted_unique(api, keys, tile_keys)
    assert d == want.size, (what, d, want.size)
    np.testing.assert_array_equal(got, want, err_msg=str(what))
    if len(keys) >= 2:
        assert held == 8 * want.size, what  # the memory rule: a buffer of exactly the distinct values


@pytest.mark.parametrize("tile_keys", TILES)
def test_sizes_around_wavefront_workgroup_and_tile(api, tile_keys):
    T = tile_of(tile_keys)
    r = util.rng(5)
    for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5):
        check(api, r.integers(0, MAX, n, dtype=U64, endpoint=True), tile_keys, ("random", n))
        check(api, r.integers(0, 40, n, dtype=U64), tile_keys, ("forty values", n))


def test_more_than_one_round_of_the_scans(api):
    """tile_keys = 256 and 1 025 * 256 + 7 keys: 1 026 tiles, so the per-digit scan of the tile counts and the unique pass's scan of the
    tile counts both take a second round of 1 024 values"""
    r = util.rng(6)
    n = 1025 * 256 + 7
    check(api, r.integers(0, MAX, n, dtype=U64, endpoint=True), 256, "random")
    check(api, r.integers(0, 5000, n, dtype=U64) << U64(13), 256, "5000 values, three passes")


def one_byte(r, n, js):
    """keys that differ in the bytes `js` only"""
    base = U64(int(r.integers(0, MAX, dtype=U64, endpoint=True)))
    keys = np.full(n, base, U64)
    for j in js:
        keys = (keys & ~(U64(0xFF) << U64(8 * j))) | (r.integers(0, 256, n, dtype=U64) << U64(8 * j))
    return keys


def contents(r, T):
    n = 3 * T + 5
    rnd = r.integers(0, MAX, n, dtype=U64, endpoint=True)
    out = {"random": rnd,
           "all equal": np.full(n, 0x0123456789ABCDEF, U64),
           "two alternating": np.where(np.arange(n) % 2 == 0, U64(0xFFFFFFFF00000001), U64(0x00000000FFFFFFFE)).astype(U64),
           "ascending": np.sort(rnd),
           "descending": np.sort(rnd)[::-1].copy(),
           "0 and 2^64 - 1": np.concatenate([rnd[:n - 4], np.array([0, MAX, MAX, 0], U64)]),
           # runs of T + 1 equal keys: sorted, every run lies across a tile seam (and the 7 single keys in front shift the runs off the seams)
           "runs across seams": np.concatenate([rnd[:7], np.repeat(rnd[7:10], T + 1)])[:n],
           "300 values": rnd[:300][r.integers(0, 300, n)]}
    for j in range(8):
        out["byte %d only" % j] = one_byte(r, n, (j,))  # one pass runs, seven are skipped
    out["bytes 0 and 5"] = one_byte(r, n, (0, 5))        # two passes: the sorted keys end in the set's own buffer
    out["bytes 0, 1 and 2"] = one_byte(r, n, (0, 1, 2))  # three passes: they end in the second buffer
    return out


@pytest.mark.parametrize("tile_keys", TILES)
def test_contents_at_a_multi_tile_size(api, tile_keys):
    r = util.rng(7)
    for what, keys in contents(r, tile_of(tile_keys)).items():
        check(api, keys, tile_keys, what)


@pytest.mark.parametrize("tile_keys", TILES)
def test_unique_twice_and_after_later_appends(api, tile_keys):
    T = tile_of(tile_keys)
    r = util.rng(8)
    a = r.integers(0, 3000, 2 * T + 3, dtype=U64) << U64(20)
    hs = api.HashSet(0, tile_keys)
    try:
        hs.append(a)
        d1 = hs.unique()
        first = hs.download()
        assert hs.unique() == d1
        np.testing.assert_array_equal(hs.download(), first)
        np.testing.assert_array_equal(first, np.unique(a))
        # values already present and new ones, in two appends
        b = np.concatenate([first[::3], r.integers(0, MAX, T + 9, dtype=U64, endpoint=True)])
        c = one_byte(r, 77, (1,))
        hs.append(b)
        hs.append(c)
        hs.append(np.zeros(0, U64))
        assert hs.size()[0] == d1 + b.size + c.size
        want = np.unique(np.concatenate([a, b, c]))
        assert hs.unique() == want.size
        np.testing.assert_array_equal(hs.download(), want)
        assert hs.unique() == want.size
    finally:
        hs.destroy()


def test_download_ranges_and_refusals(api):
    L = api.lib()
    r = util.rng(9)
    keys = np.unique(r.integers(0, MAX, 1000, dtype=U64, endpoint=True))
    n = keys.size
    hs = api.HashSet()
    try:
        hs.append(keys)
        assert hs.unique() == n
        np.testing.assert_array_equal(hs.download(0, 1), keys[:1])
        np.testing.assert_array_equal(hs.download(n - 1, 1), keys[n - 1:])
        np.testing.assert_array_equal(hs.download(n - 5), keys[n - 5:])
        np.testing.assert_array_equal(hs.download(17, 300), keys[17:317])
        assert hs.download(n, 0).size == 0 and hs.download(0, 0).size == 0
        guard = 0xA5A5A5A5A5A5A5A5
        buf = np.full(n + 4, guard, U64)
        for first, count in ((n, 1), (0, n + 1), (n + 1, 0), (1, n), (MAX, 2), (2, MAX)):
            assert L.chn_hashset_download(hs.h, first, count, buf[2:].ctypes.data) == api.E_INVALID, (first, count)
            assert (buf == guard).all(), (first, count)
        assert L.chn_hashset_download(hs.h, 0, 1, None) == api.E_INVALID
        # a whole download between the guard words
        assert L.chn_hashset_download(hs.h, 0, n, buf[2:].ctypes.data) == 0
        assert (buf[:2] == guard).all() and (buf[n + 2:] == guard).all()
        np.testing.assert_array_equal(buf[2:n + 2], keys)
        # null out pointers with a live set; the set is as it was
        assert L.chn_hashset_unique(hs.h, None) == api.E_INVALID
        assert L.chn_hashset_size(hs.h, None, None) == api.E_INVALID
        assert L.chn_hashset_append(hs.h, None, 3) == api.E_INVALID
        np.testing.assert_array_equal(hs.download(), keys)
    finally:
        hs.destroy()


# ---- chn_minimisers_into against chn_minimisers ----------------------------------------------------------------------------------------
def edge_reads(r):
    """the edge-read batch of the parity tests (ties, N, reads shorter than w) and one 40 000-base read"""
    g0, g1 = util.random_seq(r, 5000), util.random_seq(r, 5000)
    low = b"A" * 300 + g0[:200] + b"AC" * 150 + g1[:100] + b"ACG" * 90
    reads = [b"A" * 1000, b"AC" * 400, b"ACGT" * 100, b"ACG" * 200 + b"T" * 77, low, low[100:700], b"A" * 18, b"A" * 19, b"C" * 40,
             b"G" * 41, b"T" * 42, b"N" * 300, g0[:500].replace(b"A", b"N", 3), b"ACGTN" * 60,
             g0[100:160] + b"NNNN" + g0[164:900], b"A", b"ACGTACGTACGTACGTACG", g1[:63], g1[:64], g1[:65], g0[:128], g0[:129],
             (g0[:300] + b"RYKM" + g0[304:600]).lower(), g1[200:241], g1[200:240], util.random_seq(r, 40000)]
    return reads + util.sample_reads(r, [g0, g1, low], 200, (1, 1500), sub_rate=0.02)


def chunked(seq, w=41, chunk=4096):
    """one record as `charon index` cuts it: segments of 4 096 bases that overlap by w - 1"""
    from charon_amd import pack
    p = pack.pack_reads([seq])
    nwin = len(seq) - w + 1
    starts = np.arange(0, nwin, chunk, dtype=np.uint64)
    p["seg1_offset"] = starts
    p["seg1_length"] = np.minimum(len(seq) - starts, chunk + w - 1).astype(np.uint32)
    return p


def probe_index(api):
    return api.Index(api.make_desc(1, 64, [0], 1, 255))


def test_minimisers_into_equals_minimisers(api):
    from charon_amd import pack
    r = util.rng(10)
    b1 = pack.pack_reads(edge_reads(r))
    b2 = chunked(util.random_seq(r, 30000) + b"N" * 50 + util.random_seq(r, 9000))
    idx = probe_index(api)
    st = api.Stream(idx, 4096, max(b1["n_bases"], b2["n_bases"]))
    hs = api.HashSet()
    try:
        want1 = st.minimisers_host(b1).copy()
        want2 = st.minimisers_host(b2).copy()
        assert want1.size > 1000 and want2.size > 1000
        assert st.minimisers_into(b1, hs) == want1.size
        assert hs.size()[0] == want1.size
        np.testing.assert_array_equal(np.sort(hs.download()), np.sort(want1))
        # a second batch into the same set: the first one's values stay, through the growth of the buffer
        assert st.minimisers_into(b2, hs) == want2.size
        both = np.concatenate([want1, want2])
        np.testing.assert_array_equal(np.sort(hs.download()), np.sort(both))
        assert hs.unique() == np.unique(both).size
        np.testing.assert_array_equal(hs.download(), np.unique(both))
        # the existing call still gives what it gave
        np.testing.assert_array_equal(np.sort(st.minimisers_host(b1)), np.sort(want1))
        # a batch without a minimiser
        none = pack.pack_reads([b"ACGT", b"A" * 18])
        assert st.minimisers_host(none).size == 0
        assert st.minimisers_into(none, hs) == 0 and hs.size()[0] == np.unique(both).size
    finally:
        hs.destroy()
        st.destroy()
        idx.destroy()


def test_sets_and_devices(api):
    """an ordinal that is not a device; a set on another device than the stream or the index (where there is a second device)"""
    from charon_amd import pack
    L = api.lib()
    n = api.device_count()
    out = C.c_void_p()
    for dev in (n, -1):
        cfg = api.HashSetCfg(C.sizeof(api.HashSetCfg), dev, 0, 0)
        assert L.chn_hashset_create(C.byref(cfg), C.byref(out)) == api.E_INVALID and not out.value
    free, total = api.device_memory(0)
    assert 0 < free <= total
    if n >= 2:
        idx = probe_index(api)
        st = api.Stream(idx, 64, 4096)
        hs = api.HashSet(1)
        try:
            hs.append(np.arange(10, dtype=U64))
            with pytest.raises(api.ChnError) as e:
                st.minimisers_into(pack.pack_reads([util.random_seq(util.rng(3), 500)]), hs)
            assert e.value.code == api.E_INVALID and "device" in str(e.value)
            with pytest.raises(api.ChnError) as e:
                idx.emplace_set(hs, 0)
            assert e.value.code == api.E_INVALID
            np.testing.assert_array_equal(hs.download(), np.arange(10, dtype=U64))
            assert not idx.download().any()
        finally:
            hs.destroy()
            st.destroy()
            idx.destroy()


# ---- chn_index_emplace_set against chn_index_emplace ----------------------------------------------------------------------------------
@pytest.mark.parametrize("bins,h", [(3, 2), (3, 3), (70, 2), (70, 3)])
def test_emplace_set_equals_emplace(api, bins, h):
    r = util.rng(11 + bins + h)
    S = 20011
    values = [r.integers(0, MAX, n, dtype=U64, endpoint=True) for n in (5000, 1, 777)]
    where = [0, bins // 2, bins - 1]  # the last bin among them
    for rows in ((0, 0), (5000, 12345)):  # the whole index, and a row shard
        desc = api.make_desc(bins, S, [0] * bins, 1, 255, hash_funs=h, row_begin=rows[0], row_end=rows[1])
        a, b = api.Index(desc), api.Index(desc)
        row0, nrows = (rows[0], rows[1] - rows[0]) if rows[1] else (0, S)
        sets = []
        try:
            for v, bin_index in zip(values, where):
                a.emplace(v, bin_index)
                hs = api.HashSet()
                sets.append(hs)
                hs.append(v)
                b.emplace_set(hs, bin_index)
                np.testing.assert_array_equal(hs.download(), v)  # read in place, left as it was
            want = a.download(row0, nrows)
            assert want.any()
            np.testing.assert_array_equal(b.download(row0, nrows), want)
            # a set made distinct emplaces the same bits
            d = api.Index(desc)
            try:
                for hs, bin_index in zip(sets, where):
                    hs.append(hs.download())
                    hs.unique()
                    d.emplace_set(hs, bin_index)
                np.testing.assert_array_equal(d.download(row0, nrows), want)
            finally:
                d.destroy()
            # a bin out of range: refused, rows untouched; an empty set: nothing
            with pytest.raises(api.ChnError) as e:
                b.emplace_set(sets[0], bins)
            assert e.value.code == api.E_INVALID
            empty = api.HashSet()
            sets.append(empty)
            b.emplace_set(empty, 0)
            np.testing.assert_array_equal(b.download(row0, nrows), want)
        finally:
            for hs in sets:
                hs.destroy()
            a.destroy()
            b.destroy()
