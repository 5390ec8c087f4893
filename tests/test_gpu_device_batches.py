"""GPU tests (-m gpu) of device-resident batches (chn_batch.on_device = 1): the form of the ABI bench.py's headline figures and
INTEGRATION.md's recommended caller use -- paired, with an N mask, with the gzip column, into host buffers and into device pointers.

Yardsticks, none of which is the code under test: the CPU oracle (util.assert_parity: integer columns bit-exact, probabilities within
1e-6), the same reads sent as a HOST batch on the same stream (both forms run the same kernels: any difference is plumbing), zlib
(len of the level-6 gzip member of mate 1 + mate 2 as one string, N as `N`) for the sizes, and the host batch's tallies (pinned to
zlib by tests/test_gpu_cli.py::test_cli_gzip_column_from_device_tallies) for the tallies.

Device results are never re-evaluated on the host, so a row whose deciding comparison is a near tie may legitimately differ from the
oracle in `call`; such rows carry flags != 0.  The read sets of the tests with default thresholds are seeded so that the ORACLE's
probabilities put fewer than 5 % of the rows with minimisers near a tie (near_tie_fraction, asserted), and no more than that may be
flagged."""
import zlib

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

GZ_TALLIES, GZ_SIZES, GZ_BOTH, GZ_SIZES_ALL = 0, 1, 2, 3
COLUMNS = ("num_hashes", "counts", "unique", "probs", "call", "conf", "flags")


@pytest.fixture(scope="module")
def api():
    import charon_amd.api as api
    return api


# ---- the two indices and the read sets (no GPU involved: tools may import these) ----------------------------------------------
def make_genomes():
    r = util.rng(4100)
    return [util.random_seq(r, 3000) for _ in range(8)]


def build_indices(po, gs):
    """cfg5's shape -- 8 bins, 8 categories, one bin each (MODE_FUSED, W = 1) -- and a 70-bin, 2-category index (MODE_ROWS, W = 2):
    bins 0 .. 59 hold slices of the genomes (genomes 0 .. 3 are category 0, genomes 4 .. 7 category 1), bins 60 .. 69 ALL hold the
    first half of genome 0, so that the rows of its minimisers have more than three set bins (escaped rows)"""
    fused = util.build_oracle_index(po, [[g] for g in gs], list(range(8)), ["c%d" % i for i in range(7)] + ["host"])
    pool = b"".join(gs)
    many = [pool[i * 400:i * 400 + 440] for i in range(60)] + [gs[0][:1500]] * 10
    rows = util.build_oracle_index(po, [[m] for m in many], [0] * 30 + [1] * 30 + [0] * 10, ["human", "microbial"], bin_size=3001,
                                   fill_seed=8, fill=0.08)
    return fused, rows


def with_n_runs(r, gs, reads, at):
    """N runs across 16-, 32- and 64-base boundaries, a read of N only, an N as the last base of a segment (also at a 64-base end)"""
    reads = list(reads)
    for j, (start, run) in enumerate(((10, 12), (28, 9), (60, 10), (5, 130), (0, 70))):
        s = bytearray(util.mutate(r, gs[j][100:400], 0.03))
        s[start:start + run] = b"N" * run
        reads[at + j] = bytes(s)
    reads[at + 5] = b"N" * 97
    reads[at + 6] = util.mutate(r, gs[5][200:399], 0.03) + b"N"
    reads[at + 7] = gs[6][300:363] + b"N"
    reads[at + 8] = util.mutate(r, gs[7][:2499], 0.03) + b"N"
    reads[at + 9] = b"N" * 64
    return reads


def sample_pairs(r, gs, n, len1, len2, sub_rate=0.03, random_fraction=0.03):
    """mates as a sequencer makes them: both from one genome (a few pairs: random sequence), of unequal length"""
    m1, m2 = [], []
    for _ in range(n):
        l1, l2 = int(r.integers(len1[0], len1[1] + 1)), int(r.integers(len2[0], len2[1] + 1))
        if r.random() < random_fraction:
            m1.append(util.random_seq(r, l1))
            m2.append(util.random_seq(r, l2))
            continue
        g = gs[int(r.integers(0, len(gs)))]
        s1, s2 = int(r.integers(0, len(g) - l1)), int(r.integers(0, len(g) - l2))
        m1.append(util.mutate(r, g[s1:s1 + l1], sub_rate))
        m2.append(util.mutate(r, g[s2:s2 + l2], sub_rate))
    return m1, m2


def make_sets(gs):
    """name -> (reads, mates or None); n = 333 each (not a multiple of 64)"""
    r = util.rng(4101)
    pool = b"".join(gs)
    se = util.sample_reads(r, gs, 333, (0, 2500), sub_rate=0.04, random_fraction=0.03)
    se[0], se[1], se[2], se[3], se[4], se[5], se[332] = b"", gs[0][5:15], gs[1][7:37], gs[2][:19], gs[3][:40], gs[4][:41], b""
    m1, m2 = sample_pairs(r, gs, 333, (30, 400), (30, 700))
    m1[0], m2[0] = b"", util.mutate(r, gs[1][100:400], 0.02)
    m1[1], m2[1] = util.mutate(r, gs[2][100:400], 0.02), b""
    m1[2], m2[2] = b"", b""
    m1[3], m2[3] = util.mutate(r, pool[:20000], 0.03), util.mutate(r, pool[3000:23000], 0.03)   # l1 + l2 >= 32 768: 32-bit totals
    m1[4], m2[4] = gs[3][:12], util.mutate(r, gs[3][500:800], 0.02)                               # mate 1 shorter than k
    m1[332], m2[332] = util.mutate(r, gs[7][:150], 0.02), util.mutate(r, gs[7][400:550], 0.02)
    se_n = with_n_runs(r, gs, se, 10)
    p1, p2 = with_n_runs(r, gs, m1, 10), list(m2)
    for j in range(20, 30):   # N in mate 2 only; the clean mate 1 lies at another 64-base offset
        s = bytearray(p2[j] + gs[j % 8][:100])
        s[70:70 + 3 * (j - 19)] = b"N" * (3 * (j - 19))
        p2[j] = bytes(s)
    p2[30] = b"N" * 150
    p2[31] = p2[31][:-1] + b"N"
    full_n = [b"N" * len(s) for s in se_n]
    return dict(se=(se, None), pairs=(m1, m2), se_n=(se_n, None), pairs_n=(p1, p2), se_full_n=(full_n, None),
                pairs_full_n=([b"N" * len(s) for s in p1], [b"N" * len(s) for s in p2]))


def make_gzip_sets(gs):
    """reads of 1 .. 9 000 letters (a pair: both mates together): never more symbols than letters, so one deflate block is certain"""
    r = util.rng(4103)
    pool = b"".join(gs)

    def piece(L):
        s = int(r.integers(0, len(pool) - L + 1))
        return util.mutate(r, pool[s:s + L], 0.03)
    lens = [1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 257, 258, 259, 8999, 9000] + [int(x) for x in r.integers(1, 9000, 50)]
    se = [piece(L) for L in lens] + [b"A" * 1000, b"ACGT" * 500, gs[0][:700] * 3, b"AAC" * 700]
    se_n = list(se)
    for i in range(0, len(se_n), 3):
        s = bytearray(se_n[i])
        a, run = int(r.integers(0, len(s))), int(r.integers(1, 40))
        s[a:a + run] = b"N" * len(s[a:a + run])
        se_n[i] = bytes(s)
    se_n += [b"N" * 300, piece(500) + b"N", b"N"]
    l1 = [int(x) for x in r.integers(0, 4500, 60)]
    l2 = [int(x) for x in r.integers(0, 4500, 60)]
    m1, m2 = [piece(L) for L in l1], [piece(L) for L in l2]
    m1 += [b"", piece(777), b"", piece(4500), b"A"]
    m2 += [piece(555), b"", b"", piece(4500), b""]
    n2 = list(m2)
    for i in range(0, 60, 2):
        s = bytearray(n2[i])
        if len(s):
            a = int(r.integers(0, len(s)))
            s[a:a + 25] = b"N" * len(s[a:a + 25])
            n2[i] = bytes(s)
    n2[61] = b"N" * 100
    # against a bound of 2 000 letters: reads of 1 990 .. 2 010, pairs whose sum straddles it
    # (read 0 is one of those left out: the wavefront that skips a read must not come back to read 0 -- see k_gzip_tally)
    b_se = [b""] + [piece(L) for L in range(1990, 2011)] + [piece(1), piece(5000), piece(300)]
    b_m1 = [b""] + [piece(1000) for _ in range(21)] + [b"", piece(2001), piece(1500), piece(2000)]
    b_m2 = [b""] + [piece(L) for L in range(990, 1011)] + [piece(2000), b"", piece(1500), b""]
    return dict(se=(se, None), se_n=(se_n, None), pairs=(m1, m2), pairs_n2=(m1, n2), bound_se=(b_se, None), bound_pairs=(b_m1, b_m2))


def zsize(b):
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 8)
    return len(co.compress(b) + co.flush())


def near_tie_fraction(orc, paired, host=0, rel=1e-4):
    """share of the rows with minimisers whose deciding probabilities the ORACLE puts within `rel` of each other (or at the float
    underflow edge, which the call kernel also treats as borderline): the comparisons a last-ulp exp() difference could turn"""
    nh, uq, pr = orc["num_hashes"], orc["unique"].astype(np.int64), orc["probs"]
    rows = np.nonzero(nh > 0)[0]
    near = 0
    for i in rows:
        if paired:   # call_category: the two categories with the most unique hits, the first of equals
            order = sorted(range(uq.shape[1]), key=lambda c: (-uq[i, c], c))
            a, b = pr[i, order[0]], pr[i, order[1]]
            edge = min(a, b) < 1e-30
        else:
            a, b = pr[i, host], pr[i, 1 - host]
            edge = False
        near += bool(edge or abs(a - b) <= rel * max(abs(a), abs(b), 1e-300))
    return near / max(1, rows.size)


def oracle_run(oidx, reads, mates=None, thr=None):
    seqs, offs, split = util.concat(reads, mates)
    return oidx.process_reads(seqs, offs, mate_split=split, thr=thr)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(api, oracle_lib):
    gs = make_genomes()
    fused, rows = build_indices(oracle_lib, gs)
    w = dict(gs=gs, fused=fused, rows=rows, gf=util.gpu_index_from_oracle(api, fused), gr=util.gpu_index_from_oracle(api, rows),
             sets=make_sets(gs), gz=make_gzip_sets(gs), memo={})
    yield w
    w["gf"].destroy()
    w["gr"].destroy()
    fused.free()
    rows.free()


def oracle_of(world, index, name):
    """the oracle's results for a read set on an index: computed once, shared, never changed (callers take slices, which copy)"""
    key = (index, name)
    if key not in world["memo"]:
        reads, mates = world["sets"][name]
        world["memo"][key] = oracle_run(world[index], reads, mates)
    return world["memo"][key]


def rows_of(d, sel):
    return {k: v[sel] for k, v in d.items() if isinstance(v, np.ndarray)}


def model_for(api, gidx, paired, **kw):
    return api.default_model(gidx.desc.num_categories, 0 if paired else gidx.desc.host_index, paired=paired, **kw)


def packed_and_device(api, reads, mates=None):
    from charon_amd import pack
    p = pack.pack_reads(reads, mates)
    return p, util.to_device_batch(api, p, mq=40.0, comp=0.0)


def host_columns(n):
    return np.full(n, 40.0, np.float32), np.zeros(n, np.float32)


def wait_downloaded(api, st, n, gzip_output=None):
    return util.download_results(api, st.wait_device(), n, st.C, gzip_output=gzip_output)


def assert_flag_cap(out, orc, paired, host=0):
    """default thresholds: the oracle sees fewer than 5 % of the rows near a tie, and no more than 5 % may come back flagged"""
    assert near_tie_fraction(orc, paired, host) < 0.05
    with_min = out["num_hashes"] > 0
    assert out["flags"][with_min].sum() <= 0.05 * max(1, with_min.sum()), (int(out["flags"][with_min].sum()), int(with_min.sum()))


def assert_equals_host_batch(dev, host):
    """the same reads as a host batch into host buffers: integer columns of every row; probabilities BITWISE, call and confidence
    wherever chn_batch_wait did not re-evaluate the host batch's row with the host libm (flagged rows, rows without minimisers)"""
    for key in ("num_hashes", "counts", "unique", "conf", "flags"):
        assert np.array_equal(dev[key], host[key]), key
    kept = (host["flags"] == 0) & (host["num_hashes"] > 0)
    util.assert_same_results(rows_of(dev, kept), rows_of(host, kept))


def device_vs_oracle_and_host(api, world, index, name, subsets=()):
    """the read set as a device batch == the oracle == the host batch on the same stream; `subsets`: slices sent as batches of
    their own (n = 64, n = 1)"""
    reads, mates = world["sets"][name]
    paired = mates is not None
    gidx, orc = world["g" + index[0]], oracle_of(world, index, name)
    host = 0 if paired else gidx.desc.host_index
    p, db = packed_and_device(api, reads, mates)
    st = api.Stream(gidx, len(reads), p["n_bases"])
    st.set_model(model_for(api, gidx, paired))
    try:
        db.submit(st)
        dev = wait_downloaded(api, st, len(reads))
        util.assert_parity(dev, orc)
        assert_flag_cap(dev, orc, paired, host)
        st.submit_host(p, *host_columns(len(reads)))
        assert_equals_host_batch(dev, st.wait_host())
        for sl in subsets:
            sub = (reads[sl], mates[sl] if paired else None)
            ps, ds = packed_and_device(api, *sub)
            ds.submit(st)
            got = wait_downloaded(api, st, len(sub[0]))
            ds.free()
            util.assert_parity(got, rows_of(orc, sl))
            util.assert_same_results(got, rows_of(dev, sl), keys=COLUMNS)
    finally:
        st.destroy()
        db.free()
    return dev


# ---- 1. paired device batches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", ["fused", "rows"])
def test_paired_device_batches_equal_the_oracle(api, world, index):
    """cfg5's form: pairs (mates of unequal length, either or both empty, one pair of 40 000 bases) as a device batch, results as device
    pointers; n = 333, 64 and 1"""
    dev = device_vs_oracle_and_host(api, world, index, "pairs", subsets=(slice(3, 67), slice(7, 8)))
    assert (dev["call"] != 255).sum() > 100 and dev["num_hashes"][3] > 2500 and dev["num_hashes"][2] == 0


# ---- 2. N masks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,name", [("fused", "pairs_n"), ("rows", "pairs_n"), ("rows", "se_n")])
def test_device_batches_with_an_n_mask(api, world, index, name):
    """the N mask of a device batch is the caller's device pointer, for both mates; a batch full of N goes first on the same stream
    (device and host form), so that a stale mask would show"""
    reads, mates = world["sets"][name]
    paired = mates is not None
    gidx, orc = world["g" + index[0]], oracle_of(world, index, name)
    full = world["sets"]["pairs_full_n" if paired else "se_full_n"]
    n = len(reads)
    p, db = packed_and_device(api, reads, mates)
    pf, dbf = packed_and_device(api, *full)
    assert p["nmask"] is not None and pf["n_bases"] == p["n_bases"]
    st = api.Stream(gidx, n, p["n_bases"])
    st.set_model(model_for(api, gidx, paired))
    try:
        dbf.submit(st)
        orc_full = oracle_of(world, index, "pairs_full_n" if paired else "se_full_n")   # (N is a fifth letter: it has k-mers of its own)
        util.assert_parity(wait_downloaded(api, st, n), orc_full)
        db.submit(st)
        dev = wait_downloaded(api, st, n)
        util.assert_parity(dev, orc)
        assert_flag_cap(dev, orc, paired, 0 if paired else gidx.desc.host_index)
        st.submit_host(pf, *host_columns(n))
        util.assert_parity(st.wait_host(), orc_full)
        st.submit_host(p, *host_columns(n))
        assert_equals_host_batch(dev, st.wait_host())
        # a NULL mask means "no N": the batch is then what the packer wrote under the N, the 2-bit code of A
        as_a = ([s.replace(b"N", b"A") for s in reads], [s.replace(b"N", b"A") for s in mates] if paired else None)
        orc_a = oracle_run(world[index], *as_a)
        assert (orc_a["num_hashes"] != orc["num_hashes"]).sum() >= 5   # (the mask matters to what comes out)
        db.submit(st, nmask=None)
        util.assert_parity(wait_downloaded(api, st, n), orc_a)
    finally:
        st.destroy()
        db.free()
        dbf.free()


def test_single_end_device_batch_equals_the_oracle(api, world):
    """the clean single-end set (an empty read, one shorter than k, one of k .. w - 1 bases) on the row-log index: n = 333, 64 and 1"""
    dev = device_vs_oracle_and_host(api, world, "rows", "se", subsets=(slice(0, 64), slice(9, 10)))
    assert dev["num_hashes"][0] == 0 and dev["num_hashes"][1] == 0 and dev["num_hashes"][2] == 1


# ---- 3. the gzip column ---------------------------------------------------------------------------------------------------------
def gz_expect(reads, mates, bound):
    """(zlib's sizes, left out) from the letters and the lengths alone: an empty read and a read above the bound are not sized"""
    whole = [s + (mates[i] if mates is not None else b"") for i, s in enumerate(reads)]
    out = np.array([len(s) == 0 or len(s) > bound for s in whole])
    return np.array([0 if o else zsize(s) for s, o in zip(whole, out)], np.uint32), out


@pytest.mark.parametrize("name,bound", [("se", 9000), ("se_n", 9000), ("pairs", 9000), ("pairs_n2", 9000), ("bound_se", 2000),
                                        ("bound_pairs", 2000)])
def test_gzip_column_of_a_device_batch_equals_zlib(api, world, name, bound):
    """one k_gzip_tally launch without an index list, LDS sized by the caller's bound: the 2-bit kernel (no N), the 4-bit one (N),
    two mates as one string, N in mate 2 only; every mode, into device pointers and into host buffers"""
    reads, mates = world["gz"][name]
    paired = mates is not None
    n = len(reads)
    want, left = gz_expect(reads, mates, bound)
    if bound == 2000:
        # what the lengths say: of 1 990 .. 2 010 the ten above the bound, the empty read(s), the long one(s); thirteen reads remain
        assert left.sum() == (13 if paired else 12) and (~left).sum() == 13
    else:
        assert left.sum() == (1 if paired else 0)                               # only the pair of two empty mates
    gidx = world["gf"] if paired else world["gr"]
    p, db = packed_and_device(api, reads, mates)
    assert (p["nmask"] is not None) == name.endswith(("_n", "_n2"))
    st = api.Stream(gidx, n, p["n_bases"])
    st.set_model(model_for(api, gidx, paired))
    try:
        st.submit_host(p, *host_columns(n), gzip_tallies=bound, gzip_output=GZ_TALLIES)
        host_t = st.wait_host()["gzip_tallies"]
        assert np.array_equal(host_t[:, 316] != 0, left)
        for mode in (GZ_SIZES, GZ_BOTH, GZ_TALLIES):
            db.submit(st, gzip_tallies=bound, gzip_output=mode)
            dev = wait_downloaded(api, st, n, gzip_output=mode)
            db.submit(st, gzip_tallies=bound, gzip_output=mode)
            hst = st.wait_host()
            for out, where in ((dev, "device pointers"), (hst, "host buffers")):
                if mode != GZ_TALLIES:
                    bad = np.nonzero(out["gzip_sizes"] != want)[0]
                    assert bad.size == 0, (where, mode, bad[:10], out["gzip_sizes"][bad[:10]], want[bad[:10]])
                else:
                    assert "gzip_sizes" not in out
                if mode != GZ_SIZES or out is dev:   # (device results carry the status word in every mode)
                    t = out["gzip_tallies"]
                    assert np.array_equal(t[:, 316] != 0, left), (where, mode)
                    if mode != GZ_SIZES:
                        assert np.array_equal(t[~left, :317], host_t[~left, :317]), (where, mode)
                else:
                    assert "gzip_tallies" not in out
            util.assert_same_results(dev, hst, keys=COLUMNS)
        with pytest.raises(api.ChnError, match="host batches only"):
            db.submit(st, gzip_tallies=bound, gzip_output=GZ_SIZES_ALL)
        db.submit(st)   # the refusal left the stream as it was
        util.assert_same_results(wait_downloaded(api, st, n), dev, keys=COLUMNS[:3])
    finally:
        st.destroy()
        db.free()


def test_open_compression_gate_of_a_device_batch(api, world):
    """tallies requested: the ratios are still to come, so the call kernel leaves the compression gate to the caller -- with
    min_compression = 0.9 (which the batch's column of zeros fails) the calls are those of a model without that gate"""
    reads, _ = world["gz"]["se"]
    gidx, n = world["gr"], len(reads)
    p, db = packed_and_device(api, reads)
    st = api.Stream(gidx, n, p["n_bases"])
    try:
        st.set_model(model_for(api, gidx, False, min_compression=0.0))
        db.submit(st)
        plain = wait_downloaded(api, st, n)
        st.set_model(model_for(api, gidx, False, min_compression=0.9))
        db.submit(st)
        shut = wait_downloaded(api, st, n)
        db.submit(st, gzip_tallies=9000, gzip_output=GZ_TALLIES)
        dev = wait_downloaded(api, st, n, gzip_output=GZ_TALLIES)
        db.submit(st, gzip_tallies=9000, gzip_output=GZ_BOTH)
        hst = st.wait_host()
    finally:
        st.destroy()
        db.free()
    assert (plain["call"] != 255).sum() > 10 and (shut["call"] == 255).all()
    for out in (dev, hst):
        util.assert_same_results(out, plain, keys=COLUMNS)


# ---- 4. the four combinations of chn_batch.on_device and chn_result.on_device -----------------------------------------------------
@pytest.mark.parametrize("index,name", [("fused", "pairs_n"), ("rows", "se_n")])
def test_batch_and_result_residency_are_independent(api, world, index, name):
    reads, mates = world["sets"][name]
    paired = mates is not None
    gidx, orc = world["g" + index[0]], oracle_of(world, index, name)
    n = len(reads)
    p, db = packed_and_device(api, reads, mates)
    st = api.Stream(gidx, n, p["n_bases"])
    st.set_model(model_for(api, gidx, paired))
    try:
        # device batch -> host buffers: nothing staged, nothing re-evaluated -- the download of the same batch's device results
        db.submit(st)
        dd = wait_downloaded(api, st, n)
        db.submit(st)
        dh = st.wait_host()
        util.assert_same_results(dh, dd, keys=COLUMNS)
        # host batch -> device pointers: the call kernel's own outputs on its own counts
        st.submit_host(p, *host_columns(n))
        hd = wait_downloaded(api, st, n)
        util.assert_same_results(hd, dd, keys=COLUMNS)
        lengths = p["seg1_length"].astype(np.uint32) + (p["seg2_length"] if paired else 0)
        raw = st.classify_counts_raw(hd["num_hashes"], hd["counts"], hd["unique"], lengths, *host_columns(n))
        for key in ("probs", "call", "conf", "flags"):
            assert np.array_equal(raw[key], hd[key], equal_nan=(key == "probs")), key
        for out in (dh, hd):
            assert_flag_cap(out, orc, paired, 0 if paired else gidx.desc.host_index)
            util.assert_parity(rows_of(out, out["flags"] == 0), rows_of(orc, out["flags"] == 0))
    finally:
        st.destroy()
        db.free()


# ---- 5. flags of device results -------------------------------------------------------------------------------------------------
def test_flagged_rows_of_device_results_are_the_callers_to_reevaluate(api, world, oracle_lib):
    """confidence threshold 0 opens the gate for reads without a unique hit (both probabilities equal): with device results
    nothing is re-evaluated, the rows come back flagged, and chn_classify_counts on their counts gives the oracle's answer"""
    r = util.rng(4105)
    gs, gidx = world["gs"], world["gr"]
    reads = util.sample_reads(r, gs, 333, (150, 900), sub_rate=0.05, random_fraction=0.4)
    thr = oracle_lib.default_thresholds()
    thr.confidence_threshold = 0
    orc = oracle_run(world["rows"], reads, thr=thr)
    n = len(reads)
    p, db = packed_and_device(api, reads)
    st = api.Stream(gidx, n, p["n_bases"])
    st.set_model(model_for(api, gidx, False, confidence_threshold=0))
    try:
        db.submit(st)
        res = st.wait_device()
        dev = util.download_results(api, res, n, 2)
        f = dev["flags"] != 0
        assert f.sum() > 10
        util.assert_parity(rows_of(dev, ~f), rows_of(orc, ~f))
        for key in ("num_hashes", "counts", "unique", "conf"):
            assert np.array_equal(dev[key], orc[key]), key
        again = st.classify_counts(dev["num_hashes"][f], dev["counts"][f], dev["unique"][f], p["seg1_length"][f], *host_columns(int(f.sum())))
        fixed = rows_of(dev, f)
        fixed.update(again)
        util.assert_parity(fixed, rows_of(orc, f))
        # the later call worked on buffers of its own: the device-resident results are as they were
        util.assert_same_results(util.download_results(api, res, n, 2), dev, keys=COLUMNS)
    finally:
        st.destroy()
        db.free()


# ---- 6. pointer lifetime, three in flight ---------------------------------------------------------------------------------------
def test_three_device_batches_in_flight_and_pointer_lifetime(api, world):
    """three device batches with buffers of their own in flight come back oldest first, each as when run alone; a fourth submit is
    refused; result pointers stay valid until the third-next submit"""
    gidx = world["gr"]
    parts = [world["sets"]["se"][0][a:b] for a, b in ((0, 150), (150, 217), (217, 333))]
    batches = [packed_and_device(api, part) for part in parts]
    cap_bases = max(p["n_bases"] for p, _ in batches)
    st = api.Stream(gidx, 150, cap_bases)
    st.set_model(model_for(api, gidx, False))
    try:
        alone = []
        for (p, db), part in zip(batches, parts):
            db.submit(st)
            alone.append(wait_downloaded(api, st, len(part)))
        orc = oracle_of(world, "rows", "se")
        for a, sl in zip(alone, (slice(0, 150), slice(150, 217), slice(217, 333))):
            util.assert_parity(a, rows_of(orc, sl))
        for _, db in batches:
            db.submit(st)
        with pytest.raises(api.ChnError, match="in flight"):
            batches[0][1].submit(st)
        for a, part in zip(alone, parts):
            util.assert_same_results(wait_downloaded(api, st, len(part)), a, keys=COLUMNS)
        # A's pointers after two further submits and waits
        batches[0][1].submit(st)
        res_a = st.wait_device()
        for k in (1, 2):
            batches[k][1].submit(st)
            util.assert_same_results(wait_downloaded(api, st, len(parts[k])), alone[k], keys=COLUMNS)
        util.assert_same_results(util.download_results(api, res_a, len(parts[0]), 2), alone[0], keys=COLUMNS)
    finally:
        st.destroy()
        for _, db in batches:
            db.free()


# ---- 7. a bad second segment ----------------------------------------------------------------------------------------------------
def test_bad_second_segment_of_a_device_batch(api, world):
    """every seg1 is good; one seg2 is misaligned, or reaches beyond n_bases: never read, and chn_batch_wait fails -- without and
    with the deflate pass (k_gzip_tally checks its segments the same way).  The stream stays usable."""
    m1, m2 = (x[5:101] for x in world["sets"]["pairs"])
    n = len(m1)
    orc = rows_of(oracle_of(world, "fused", "pairs"), slice(5, 101))
    gidx = world["gf"]
    p, db = packed_and_device(api, m1, m2)
    st = api.Stream(gidx, n, p["n_bases"])
    st.set_model(model_for(api, gidx, True))
    spare = []
    try:
        for kind in ("misaligned", "beyond"):
            o2, l2 = p["seg2_offset"].copy(), p["seg2_length"].copy()
            if kind == "misaligned":
                o2[40] += 3
            else:
                l2[70] = p["n_bases"]   # from a good offset to far behind the buffer
            d_o2, d_l2 = util.to_device(api, o2), util.to_device(api, l2)
            spare += [d_o2, d_l2]
            for gz in (0, 3000):
                db.submit(st, gzip_tallies=gz, gzip_output=GZ_SIZES, seg2_offset=d_o2, seg2_length=d_l2)
                with pytest.raises(api.ChnError, match="misaligned or lies outside"):
                    st.wait_device()
            db.submit(st)   # the repaired batch
            util.assert_parity(wait_downloaded(api, st, n), orc)
    finally:
        st.destroy()
        db.free()
        for ptr in spare:
            api.device_free(0, ptr)


# ---- 8. the overflow re-run reads the caller's buffers again --------------------------------------------------------------------
@pytest.mark.parametrize("name,split_bucket", [("se", 64), ("pairs", 0)])
def test_row_log_overflow_rerun_of_a_device_batch(api, world, name, split_bucket):
    """CHN_STREAM_TINY_LOG: every batch overruns its row log and chn_batch_wait runs it again on worst-case buffers, from the caller's
    device buffers -- single-end with the SPLIT launch taking the reads of 1 024 bases and more, paired, two batches in flight"""
    reads, mates = world["sets"][name]
    paired = mates is not None
    gidx, orc = world["gr"], oracle_of(world, "rows", name)
    n = len(reads)
    assert paired or sum(len(s) >= 1024 for s in reads) >= 2
    p, db = packed_and_device(api, reads, mates)
    try:
        for tiny in (True, False):
            st = api.Stream(gidx, n, p["n_bases"], tiny_log=tiny, split_bucket=split_bucket)
            st.set_model(model_for(api, gidx, paired))
            db.submit(st)
            outs = [wait_downloaded(api, st, n)]
            db.submit(st)
            db.submit(st)
            outs += [wait_downloaded(api, st, n), st.wait_host()]
            reruns = st.profile(4)[1]
            st.destroy()
            for out in outs:
                util.assert_parity(out, orc)
            assert reruns == (3 if tiny else 0)
    finally:
        db.free()
