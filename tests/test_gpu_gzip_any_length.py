"""chn_batch.gzip_output = CHN_GZIP_SIZES_ALL: the device returns the exact gzip member size (zlib level 6, wbits 31, memLevel 8, as
gzip-hpp writes it: src/utils.cpp:114-124) for EVERY read of a host batch, whatever its length and however many deflate blocks zlib
writes for it -- zlib's window slide, block flushes, pairs (device-resident batches are refused).  Every size is compared with Python's
zlib."""
import zlib

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import charon_amd.api as api
    return api


@pytest.fixture(scope="module")
def gidx(api, oracle_lib):
    r = util.rng(5)
    gs = [util.random_seq(r, 4000), util.random_seq(r, 4000)]
    oidx = util.build_oracle_index(oracle_lib, [[g] for g in gs], [0, 1], ["host", "microbial"])
    g = util.gpu_index_from_oracle(api, oidx)
    yield g
    g.destroy()
    oidx.free()


def zsize(b):
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 8)
    return len(co.compress(b) + co.flush())


def forms(reads):
    """the batch as it is (4-bit codes when it holds an N) and without any N (the kernel's 2-bit form)"""
    yield reads
    yield [rd.replace(b"N", b"G") for rd in reads]


def gzip_host(api, g, reads, mates=None, bound=None, mode=3):
    from charon_amd import pack
    api_bound = api.GZIP_ANY_LEN if bound is None else bound
    p = pack.pack_reads(reads, mates)
    st = api.Stream(g, len(reads), p["n_bases"])
    st.set_model(api.default_model(2, 0))
    st.submit_host(p, np.full(len(reads), 40.0, np.float32), None, gzip_tallies=api_bound, gzip_output=mode)
    out = st.wait_host()
    st.destroy()
    assert "gzip_tallies" not in out or mode != 3
    return out


def sizes_host(api, g, reads, mates=None, bound=None, mode=3):
    return gzip_host(api, g, reads, mates, bound, mode)["gzip_sizes"]


def check(api, g, reads, mates=None):
    for rs in forms(reads):
        ms = None if mates is None else [m.replace(b"N", b"G") for m in mates] if rs is not reads else mates
        got = sizes_host(api, g, rs, ms)
        for i, rd in enumerate(rs):
            whole = rd + (ms[i] if ms is not None else b"")
            assert int(got[i]) == zsize(whole), (i, len(whole), whole[:30])


def test_mode_3_random_reads_across_the_window_slide(api, gidx):
    r = util.rng(11)
    lens = [61441, 65273, 65274, 65275, 65276, 65536, 98042, 200000, 1000000, 2000000]
    check(api, gidx, [util.random_seq(r, n) for n in lens])


def test_mode_3_low_entropy_and_n_rich_reads(api, gidx):
    r = util.rng(12)
    reads = [bytes(r.choice(list(b"ACGTN"), 150000, p=[0.2, 0.2, 0.2, 0.2, 0.2]).astype(np.uint8)),
             bytes(r.choice(list(b"ACGTN"), 90000, p=[0.05, 0.05, 0.05, 0.05, 0.8]).astype(np.uint8)),
             b"A" * 1000000, b"ACG" * 166667, b"TTAGGG" * 83334, b"N" * 70000,
             util.mutate(r, b"TTAGGG" * 50000, 0.01)]
    check(api, gidx, reads)


def test_mode_3_copies_at_the_window_edges(api, gidx):
    """internal copies at distances MAX_DIST - 1, MAX_DIST, MAX_DIST + 1 planted around the slide points; three-letter matches at
    distance 4 096 / 4 097 (TOO_FAR) beyond 64 k"""
    r = util.rng(13)
    reads = []
    for d in (32505, 32506, 32507):
        for slide in (65274, 65274 + 32768, 65274 + 2 * 32768):
            for shift in (-300, -5, 0, 3, 200):
                s = bytearray(util.random_seq(r, 200000))
                dst = slide + shift
                s[dst:dst + 400] = s[dst - d:dst - d + 400]
                reads.append(bytes(s))
    for d in (4096, 4097):
        s = bytearray(r.choice(list(b"ACG"), 120000).astype(np.uint8).tobytes())
        for at in (70000, 100000):
            s[at:at + 5] = b"ATTTC"
            s[at + d:at + d + 5] = b"GTTTA"
        reads.append(bytes(s))
    check(api, gidx, reads)


def test_mode_3_pairs_beyond_one_window(api, gidx):
    r = util.rng(14)
    m1 = [util.random_seq(r, 40000), util.random_seq(r, 35000), b"ACGT" * 20000, util.random_seq(r, 100)]
    m2 = [util.random_seq(r, 30000), m1[1][:34000], util.random_seq(r, 70000), b"N" * 64000]
    check(api, gidx, m1, m2)


def test_mode_3_prefixes_across_block_flushes(api, gidx):
    """reads of A/C/G/T/N reach zlib's 16 383 symbols per block only beyond some 90 000 letters (a symbol covers four letters and more:
    no read within the tally kernel's 61 440 letters needs a second block, so the tallies' status word cannot locate a flush there).
    Prefixes of one read at every 401st length across its first and second flush, each through mode 3 against zlib: the flush lands in
    either branch and at every distance from the end of the input."""
    r = util.rng(15)
    for src in (bytes(r.choice(list(b"ACGTN"), 260000).astype(np.uint8)), util.random_seq(r, 260000)):
        reads = [src[:L] for L in range(80000, 260000, 401)]
        got = sizes_host(api, gidx, reads)
        for i, rd in enumerate(reads):
            assert int(got[i]) == zsize(rd), (len(rd), i)


def test_mode_3_mixed_batch_keeps_the_short_sizes(api, gidx):
    r = util.rng(16)
    reads = [util.random_seq(r, 5000) for _ in range(300)]
    for i in range(0, 300, 50):
        reads.insert(i, util.random_seq(r, int(r.integers(61441, 400000))))
    s1 = sizes_host(api, gidx, reads, bound=61440, mode=api.GZIP_SIZES)
    s3 = sizes_host(api, gidx, reads)
    for i, rd in enumerate(reads):
        if len(rd) <= 61440:
            assert s1[i] == s3[i] and s1[i] != 0
        else:
            assert s1[i] == 0
        assert int(s3[i]) == zsize(rd), i


def test_mode_3_more_long_reads_than_wavefronts(api, gidx):
    """more reads beyond 61 440 letters than the device holds k_gzip_long wavefronts at once (three per CU without N)"""
    r = util.rng(17)
    pool = util.random_seq(r, 400000)
    reads = []
    for i in range(900):
        a = int(r.integers(0, 300000))
        rd = pool[a:a + 62000 + int(r.integers(0, 2000))]
        if i % 3 == 0:
            rd = rd[:31000] + rd[:31000]
        reads.append(rd)
    got = sizes_host(api, gidx, reads)
    for i, rd in enumerate(reads):
        assert int(got[i]) == zsize(rd), i


def test_mode_3_device_batch_is_refused(api, gidx):
    """device-resident batches do not take CHN_GZIP_SIZES_ALL yet: refused before anything is launched"""
    st = api.Stream(gidx, 4, 256)
    st.set_model(api.default_model(2, 0))
    d = api.device_malloc(0, 4096)
    api.device_upload(0, d, np.zeros(1024, np.uint32))
    with pytest.raises(api.ChnError, match="host batches only"):
        st.submit_device(4, 256, d, d, d, gzip_tallies=api.GZIP_ANY_LEN, gzip_output=api.GZIP_SIZES_ALL)
    st.destroy()
    api.device_free(0, d)


def test_mode_3_bound_below_a_reads_length_hands_it_back(api, gidx):
    r = util.rng(19)
    reads = [util.random_seq(r, n) for n in (5000, 80000, 150000, 99999, 100000, 100001)]
    got = sizes_host(api, gidx, reads, bound=100000)
    for i, rd in enumerate(reads):
        assert int(got[i]) == (zsize(rd) if len(rd) <= 100000 else 0), i


def test_both_kernels_size_the_reads_below_the_tally_bound_alike(api, gidx):
    """the seam between the two instances of the walk: reads of 45 000 .. 61 440 letters through k_gzip_tally (GZIP_BOTH, bound 61 440)
    and through mode 3.  Mode 3 is zlib's size for every read; where the tallies cover the read (status 0) the size formed from them
    is the same; a read the tally kernel hands back for a second deflate block (status not 0) has no size in GZIP_BOTH, and mode 3
    sizes it with k_gzip_long.  (DNA reads of this length rarely reach 16 383 symbols: no read has to be handed back here.)"""
    r = util.rng(21)
    reads = []
    for i, n in enumerate(np.linspace(45000, 61440, 40).astype(int).tolist()):
        if i % 4 == 2:  # N at 10 %
            rd = bytes(r.choice(list(b"ACGTN"), n, p=[0.225, 0.225, 0.225, 0.225, 0.1]).astype(np.uint8))
        else:
            rd = util.random_seq(r, n)
        if i % 4 == 3:  # an internal copy at distance 32 500
            s = bytearray(rd)
            dst = int(r.integers(32500, n - 400))
            s[dst:dst + 400] = s[dst - 32500:dst - 32100]
            rd = bytes(s)
        reads.append(rd)
    assert len(reads[-1]) == 61440 and any(b"N" in rd for rd in reads)
    for rs in forms(reads):
        both = gzip_host(api, gidx, rs, bound=61440, mode=api.GZIP_BOTH)
        s2, status = both["gzip_sizes"], both["gzip_tallies"][:, 316]
        s3 = sizes_host(api, gidx, rs)
        for i, rd in enumerate(rs):
            assert int(s3[i]) == zsize(rd), (i, len(rd))
            if status[i] == 0:
                assert int(s2[i]) == int(s3[i]), (i, len(rd))
            else:
                assert int(s2[i]) == 0, (i, len(rd))
