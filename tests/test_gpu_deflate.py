"""GPU tests (-m gpu) of k_deflate_members behind chn_deflate_run: the device's bytes are the host policy's bytes
(chn_deflate_run_host, which tests/test_deflate_cpu.py holds against zlib), whatever the job's size, grouping and memory."""
import zlib

import numpy as np
import pytest

from tests import deflate_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def deflater():
    import charon_amd.api as api
    h = api.Deflater(0)
    yield h
    h.destroy()


@pytest.fixture(scope="module")
def pool():
    """small pieces (64 .. 4 096 bytes of the fixtures and of noise, runs and an empty one among them) for the jobs of many members, and
    their host members -- computed once"""
    import charon_amd.api as api
    r = np.random.default_rng(77)
    texts = [f() for _, f in dc.fixtures()] + [dc._rand(40000, 9), b"I" * 40000]
    pieces = [b""]
    for k in range(160):
        t = texts[k % len(texts)]
        n = int(r.integers(64, 4097))
        at = int(r.integers(0, len(t) - n))
        pieces.append(t[at:at + n])
    host = {f: api.deflate_host(pieces, f) for f in (0, api.DEFLATE_BGZF)}
    members = {f: [h["out"][int(o):int(o) + int(l)] for o, l in zip(h["offset"], h["length"])] for f, h in host.items()}
    return pieces, members, {f: h["crc32"] for f, h in host.items()}


def same(dev, host):
    assert dev["used"] == host["used"] and dev["bound"] == host["bound"]
    assert (dev["offset"] == host["offset"]).all() and (dev["length"] == host["length"]).all()
    assert (dev["crc32"] == host["crc32"]).all()
    assert dev["out"] == host["out"]


@pytest.mark.parametrize("flags", [0, 1])
def test_shapes_are_the_host_s_bytes(deflater, flags):
    import charon_amd.api as api
    pieces = [p for _, p in dc.shapes()]
    same(deflater.run(pieces, flags), api.deflate_host(pieces, flags))
    data, where = dc.scattered(pieces)  # odd offsets, gaps, not in order
    same(deflater.run(where, flags, data=data), api.deflate_host(where, flags, data=data))


@pytest.mark.parametrize("name,text", dc.fixtures())
def test_fixtures_are_the_host_s_bytes(deflater, name, text):
    import charon_amd.api as api
    pieces = dc.pieces_of(text())
    for flags in (0, api.DEFLATE_BGZF):
        same(deflater.run(pieces, flags), api.deflate_host(pieces, flags))


def draw(pool, n, seed, flags):
    pieces, members, crc = pool
    pick = [int(x) for x in np.random.default_rng(seed).integers(0, len(pieces), n)]
    return [pieces[i] for i in pick], b"".join(members[flags][i] for i in pick), [int(crc[flags][i]) for i in pick]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 513])
def test_job_sizes_pageable_and_page_locked(deflater, pool, n):
    """513 members are more than the grid has workgroups: the cursor hands the last one to a wavefront that has finished another"""
    import charon_amd.api as api
    flags = api.DEFLATE_BGZF
    pieces, want, crc = draw(pool, n, 300 + n, flags)
    r = deflater.run(pieces, flags)  # pageable in and out
    assert r["out"] == want and [int(c) for c in r["crc32"]] == crc
    total = sum(map(len, pieces))
    pin_in, pin_out = api.pinned_array(max(total, 1), np.uint8), api.pinned_array(api.deflate_bound(n, total, flags) + 64, np.uint8)
    try:
        pin_in[:total] = np.frombuffer(b"".join(pieces), np.uint8)
        where, at = [], 0
        for p in pieces:
            where.append((at, len(p)))
            at += len(p)
        r = deflater.run(where, flags, data=pin_in, out=pin_out)  # page-locked: downloaded into directly
        assert r["out"] == want and [int(c) for c in r["crc32"]] == crc
        assert (pin_out[r["used"]:] == 0xA5).all()
    finally:
        api.host_free(pin_in)
        api.host_free(pin_out)


def test_three_groups_and_a_second_handle(pool):
    """groups of at most 200 members: 513 members are three, so both buffer sets are used again; then a fresh handle, and the first one
    again with a small job that must not see what the large one left behind"""
    import charon_amd.api as api
    a, b = api.Deflater(0), api.Deflater(0)
    try:
        a.group_members(200)
        for flags in (0, api.DEFLATE_BGZF):
            pieces, want, crc = draw(pool, 513, 900 + flags, flags)
            r = a.run(pieces, flags)
            assert r["out"] == want and [int(c) for c in r["crc32"]] == crc
            assert (np.diff(r["offset"].astype(np.int64)) == r["length"][:-1]).all() and int(r["offset"][0]) == 0
        pieces, want, crc = draw(pool, 70, 5, 0)
        assert b.run(pieces, 0)["out"] == want
        pieces, want, crc = draw(pool, 2, 6, api.DEFLATE_BGZF)
        assert a.run(pieces, api.DEFLATE_BGZF)["out"] == want
        assert a.kernel_ms() > 0
    finally:
        a.destroy()
        b.destroy()


def test_bgzf_job_inflated_on_the_device(deflater):
    """what one handle writes the other reads: every member back through k_inflate_members with its trailer's CRC-32 expected"""
    import charon_amd.api as api
    pieces = [p for _, p in dc.shapes()] + dc.pieces_of(dc.fastq_150b())
    r = deflater.run(pieces, api.DEFLATE_BGZF)
    blocks = dc.parse_bgzf(r["out"])
    assert [b[4] for b in blocks] == [len(p) for p in pieces]
    inf = api.Inflater(0)
    try:
        res, st, crc = inf.run([b[2] for b in blocks], [b[4] for b in blocks], guard=16, expected=[b[3] for b in blocks], want_crc=True)
    finally:
        inf.destroy()
    assert not st.any(), st
    assert res == pieces and [int(c) for c in crc] == [zlib.crc32(p) for p in pieces]


def test_descriptor_error_launches_nothing(deflater):
    import charon_amd.api as api
    big = np.zeros(70000, np.uint8)
    for where, member in (([(0, 100), (10, dc.MAX_IN + 1)], 1), ([(0, 100), (70001, 0)], 1), ([(69990, 11)], 0)):
        j, a = api.deflate_job(where, 0, data=big, out=np.empty(300000, np.uint8))
        with pytest.raises(api.ChnError, match="member %d" % member):
            deflater.run_job(j)
        assert (a["out"] == 0xA5).all() and int(a["out_length"][0]) == 0xFFFFFFFF
    j, a = api.deflate_job([b"ACGT" * 10], 1, out=np.empty(40 + 31 - 1, np.uint8))
    with pytest.raises(api.ChnError, match="chn_deflate_bound"):
        deflater.run_job(j)
    assert (a["out"] == 0xA5).all()
    j, a = api.deflate_job([b"ACGT" * 10], 1)
    j.struct_size -= 8
    with pytest.raises(api.ChnError, match="struct_size"):
        deflater.run_job(j)
    assert deflater.kernel_ms() == 0  # (the time of the last call's kernels: there were none)
    j, a = api.deflate_job([], 1)  # no member: a no-op
    deflater.run_job(j)
    assert int(a["used"][0]) == 0 and (a["out"] == 0xA5).all()
