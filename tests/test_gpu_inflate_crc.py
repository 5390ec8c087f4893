"""GPU tests (-m gpu) of the CRC-32 that k_inflate_members<true> takes from the decoded window (chn_inflate_run_crc) and of
CHARON_GPU_INFLATE=1 relying on it.  The yardstick is Python's zlib.crc32 of what Python's zlib inflates; the host form
(chn_inflate_run_host_crc) is compared value by value and status by status on top."""
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

from tests import inflate_cases as ic
from tests import util
from tests.test_gpu_cli import assert_same_tsv
from tests.test_gpu_inflate import crafted_bad_job, crafted_good, repeated_job, run_cli
from tests.test_inflate_crc_cpu import CORRUPT, crc_set

pytestmark = pytest.mark.gpu
G = os.path.join(util.ROOT, "tests", "golden")
IDX = os.path.join(G, "cfg1.idx")
FQ = os.path.join(G, "cfg1_reads.fastq.gz")


@pytest.fixture(scope="module")
def inflater():
    import charon_amd.api as api
    h = api.Inflater(0)
    yield h
    h.destroy()


@pytest.fixture(scope="module")
def host_crc():
    """the whole crc_set through the host form, once"""
    import charon_amd.api as api
    cs = crc_set()
    return api.inflate_host([c[1] for c in cs], [c[2] for c in cs], guard=64, want_crc=True)


def draw(n, seed):
    """n members drawn from the crc_set as tests/test_gpu_inflate.py draws from its good set; their bytes and CRCs by zlib"""
    cs = crc_set()
    r = util.rng(seed)
    pick = [int(x) for x in r.integers(0, len(cs), n)]
    return [cs[i][1] for i in pick], [cs[i][2] for i in pick], [cs[i][3] for i in pick], [cs[i][4] for i in pick]


@pytest.mark.parametrize("guard", [0, 1, 7, 64])
def test_every_length_against_zlib_and_the_host_form(inflater, host_crc, guard):
    """the guard shifts every destination in `out`; a pageable `out` goes through staging, the page-locked one is downloaded into
    directly where the members lie back to back (guard 0).  (On the device a group's outputs lie back to back whatever the guard: the
    misalignment classes of the window are the next test's.)"""
    import charon_amd.api as api
    cs = crc_set()
    ms, sizes = [c[1] for c in cs], [c[2] for c in cs]
    hres, hst, hcrc = host_crc
    pinned = api.pinned_array(sum(sizes) + guard * len(cs) + 16, np.uint8)
    try:
        for out in (None, pinned):
            res, st, crc = inflater.run(ms, sizes, guard=guard, out=out, want_crc=True)
            assert not st.any()
            for c, r, got in zip(cs, res, crc):
                assert r == c[3], c[0]
                assert int(got) == c[4], (c[0], hex(int(got)), hex(c[4]))
            assert (st == hst).all() and (crc == hcrc).all() and res == hres
            res, st = inflater.run(ms, sizes, guard=guard, out=out, expected=[c[4] for c in cs])
            assert not st.any() and res == hres
    finally:
        api.host_free(pinned)
    assert int(hcrc[0]) == 0 and sizes[0] == 0


def test_every_misalignment_of_the_window(inflater):
    """the window index is shifted by the destination's misalignment to 16 bytes, and on the device the outputs of a job lie back to
    back: fillers in front bring each of six members onto each of the 16 classes; the slices are cut by output position, so the CRC
    does not move"""
    import charon_amd.api as api
    by_name = {c[0]: c for c in crc_set()}
    job, at, seen = [], 0, set()
    for name in ("fastq_1", "random_17", "fastq_65", "random_4097", "fastq_65279", "random_65535"):
        for cls in range(16):
            delta = (cls - at) % 16
            for n in [4] * (delta // 4) + ([delta % 4] if delta % 4 else []):
                job.append(by_name["random_%d" % n])
                at += n
            assert at % 16 == cls
            seen.add((name, cls))
            job.append(by_name[name])
            at += by_name[name][2]
    assert len(seen) == 96
    ms, sizes = [c[1] for c in job], [c[2] for c in job]
    res, st, crc = inflater.run(ms, sizes, want_crc=True, expected=[c[4] for c in job])
    assert not st.any() and res == [c[3] for c in job] and [int(x) for x in crc] == [c[4] for c in job]
    hres, hst, hcrc = api.inflate_host(ms, sizes, want_crc=True)
    assert (hst == st).all() and (hcrc == crc).all()


def test_one_member_at_a_time(inflater):
    for name, m, s, data, want in crc_set():
        res, st, crc = inflater.run([m], [s], guard=3, want_crc=True)
        assert int(st[0]) == 0 and res[0] == data and int(crc[0]) == want, name


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_job_sizes(inflater, n):
    ms, sizes, want, crcs = draw(n, 200 + n)
    res, st, crc = inflater.run(ms, sizes, guard=5, expected=crcs, want_crc=True)
    assert not st.any() and res == want and [int(x) for x in crc] == crcs


def test_large_job_then_small_job_on_one_handle():
    """1 100 members: more than one group and more members than the grid has workgroups, so a workgroup decodes member after member
    with CRC tables built in between; then two members on the same handle, and a plain run"""
    import charon_amd.api as api
    cs = crc_set()
    big = [i for i, c in enumerate(cs) if c[2] >= 65279]
    r = util.rng(11)
    pick = [big[int(x)] if k % 4 else int(r.integers(0, len(cs))) for k, x in enumerate(r.integers(0, len(big), 1100))]
    ms, sizes, want, crcs = [cs[i][1] for i in pick], [cs[i][2] for i in pick], [cs[i][3] for i in pick], [cs[i][4] for i in pick]
    assert sum(sizes) > (40 << 20)
    h = api.Inflater(0)
    try:
        res, st, crc = h.run(ms, sizes, expected=crcs, want_crc=True)
        assert not st.any() and [int(x) for x in crc] == crcs
        assert res == want
        ms, sizes, want, crcs = draw(2, 12)
        res, st, crc = h.run(ms, sizes, guard=64, expected=crcs, want_crc=True)
        assert not st.any() and res == want and [int(x) for x in crc] == crcs
        res, st = h.run(ms, sizes, guard=64)
        assert not st.any() and res == want
        res, st, crc = h.run([], [], want_crc=True)
        assert res == [] and len(st) == 0 and len(crc) == 0
    finally:
        h.destroy()


def test_wrong_expected_is_status_7_exactly_there(inflater):
    import charon_amd.api as api
    ms, sizes, want, crcs = draw(130, 31)
    exp = list(crcs)
    for at in (0, 64, 129):
        exp[at] ^= 0x00010000
    res, st, crc = inflater.run(ms, sizes, guard=9, expected=exp, want_crc=True)
    assert [int(x) for x in st] == [7 if i in (0, 64, 129) else 0 for i in range(130)]
    assert res == want and [int(x) for x in crc] == crcs  # the bytes and the CRC that was found are still reported
    hres, hst, hcrc = api.inflate_host(ms, sizes, guard=9, expected=exp, want_crc=True)
    assert (hst == st).all() and (hcrc == crc).all() and hres == res


def test_rejected_members_keep_their_status_with_expected_present(inflater):
    import charon_amd.api as api
    _, bad, _ = ic.member_set()
    cs = crc_set()
    cases = [(m, s) for _, m, s in bad] + ic.sweep_cases()[:200]
    verdicts = [ic.yardstick(m, s) for m, s in cases]
    ms, sizes, exp, data = [], [], [], []
    for k, ((m, s), (ok, out)) in enumerate(zip(cases, verdicts)):  # each between good members
        g = cs[(7 * k) % len(cs)]
        ms += [g[1], m]; sizes += [g[2], s]; exp += [g[4], zlib.crc32(out) if ok else 0x12345678]; data += [g[3], out if ok else None]
    _, plain = api.inflate_host(ms, sizes, guard=64)
    res, st, crc = inflater.run(ms, sizes, guard=64, expected=exp, want_crc=True)
    assert (st == plain).all() and res == data
    assert [(int(x) == 0) for x in st] == [d is not None for d in data] and any(int(x) for x in st)
    assert all(int(c) == e for c, e, d in zip(crc, exp, data) if d is not None)
    _, st7 = inflater.run(ms, sizes, guard=64, expected=[e ^ 1 for e in exp])
    assert [int(x) for x in st7] == [7 if int(p) == 0 else int(p) for p in plain]


def test_crafted_and_foreign_members_through_the_crc_kernel(inflater):
    """tests/test_gpu_inflate.py's crafted and foreign members again, with the CRC-32 taken and compared on the device"""
    import charon_amd.api as api
    ms, sizes, names, want = crafted_good()
    crcs = [zlib.crc32(w) & 0xFFFFFFFF for w in want]
    assert crcs[-4:] == [c for _, _, _, c in ic.foreign_set()]  # the fixture's own
    res, st, crc = inflater.run(ms, sizes, guard=64, expected=crcs, want_crc=True)
    assert [n for n, x in zip(names, st) if int(x) != 0] == []
    for name, out, w, got, c in zip(names, res, want, crc, crcs):
        assert out == w and int(got) == c, name
    hres, hst, hcrc = api.inflate_host(ms, sizes, guard=64, expected=crcs, want_crc=True)
    assert (hst == st).all() and (hcrc == crc).all() and hres == res


def test_crafted_rejects_keep_their_status_with_expected_present(inflater):
    import charon_amd.api as api
    ms, sizes, expect = crafted_bad_job()
    exp = [zlib.crc32(e) & 0xFFFFFFFF if e is not None else 0x12345678 for e in expect]
    _, plain = api.inflate_host(ms, sizes, guard=64)
    res, st, crc = inflater.run(ms, sizes, guard=64, expected=exp, want_crc=True)
    assert (st == plain).all() and res == expect
    assert [(int(x) == 0) for x in st] == [e is not None for e in expect]
    assert all(int(c) == x for c, x, e in zip(crc, exp, expect) if e is not None)


def test_all_symbols_and_many_blocks_seventy_times(inflater):
    ms, sizes, want, crcs = repeated_job()
    res, st, crc = inflater.run(ms, sizes, expected=crcs, want_crc=True)
    assert not st.any() and res == want and [int(x) for x in crc] == crcs


def test_plain_run_is_what_it_was(inflater):
    """no CRC asked for: the plain kernel; results equal zlib's and the host decoder's on the member set, after CRC runs on the handle"""
    import charon_amd.api as api
    good, bad, trailing = ic.member_set()
    every = good + bad + trailing
    ms, sizes = [m for _, m, _ in every], [s for _, _, s in every]
    inflater.run(ms, sizes, guard=64, want_crc=True)
    res, st = inflater.run(ms, sizes, guard=64)
    hres, hst = api.inflate_host(ms, sizes, guard=64)
    assert (st == hst).all() and res == hres
    for (name, m, s), out, status in zip(every, res, st):
        ok, want = ic.yardstick(m, s)
        assert (int(status) == 0) == ok and out == want, name
    j, a = api.inflate_job(ms, sizes, guard=64)
    c, _ = api.inflate_crc(len(ms))  # both arrays NULL: decode only
    inflater.run_job(j, c)
    assert (a["status"][:len(ms)] == st).all()


# ---- the front end -------------------------------------------------------------------------------------------------------------------
def _second_member(f):
    at = f.index(b"\x1f\x8b\x08\x04", 100)
    return at, struct.unpack("<H", f[at + 16:at + 18])[0] + 1


def test_cli_only_the_device_crc_can_catch_these(tmp_path):
    data = gzip.decompress(open(FQ, "rb").read())
    # 1. stored blocks, one payload byte of the second member flipped: it still inflates to its full size, only the CRC differs
    stored = bytearray(ic.bgzf(data, level=0, block=20000))
    at, total = _second_member(bytes(stored))
    stored[at + 18 + 5 + 200] ^= 0x01
    member = bytes(stored[at + 18:at + total - 8])
    crc, isize = struct.unpack("<II", bytes(stored[at + total - 8:at + total]))
    ok, out = ic.yardstick(member, 20000)
    assert ok and isize == 20000 and len(out) == 20000 and zlib.crc32(out) != crc
    assert out != data[20000:40000] and sum(a != b for a, b in zip(out, data[20000:40000])) == 1
    # 2. level 6, one bit of the second member's stored CRC flipped
    flipped = bytearray(ic.bgzf(data, level=6, block=20000))
    at, total = _second_member(bytes(flipped))
    flipped[at + total - 8 + 2] ^= 0x04
    for name, content in (("payload", stored), ("trailer", flipped)):
        f = tmp_path / (name + ".fastq.gz")
        f.write_bytes(bytes(content))
        errs = []
        for env in ({}, {"CHARON_GPU_INFLATE": "1"}):
            rc, out, err = run_cli("dehost", ["--db", IDX, str(f)], str(tmp_path / (name + "".join(env.values()))), env)
            assert rc == 1 and CORRUPT in err, (name, env, rc, err)
            errs.append(err)
        assert errs[0] == errs[1], name


def test_cli_intact_files_and_the_log(tmp_path):
    data = gzip.decompress(open(FQ, "rb").read())
    b1 = tmp_path / "g_1.fastq.gz"
    b1.write_bytes(ic.bgzf(data, level=0, block=20000))
    b2 = tmp_path / "g_2.fastq.gz"
    b2.write_bytes(ic.bgzf(data, level=6, block=20000))
    for tag, files in (("single", [str(b1)]), ("paired", [str(b1), str(b2)])):
        outs = {}
        for name, env in (("off", {}), ("on", {"CHARON_GPU_INFLATE": "1"}), ("on_text", {"CHARON_GPU_INFLATE": "1", "CHARON_TEXT_BATCHES": "1"})):
            rc, out, err = run_cli("dehost", ["--db", IDX] + files, str(tmp_path / (tag + name)), env)
            assert rc == 0, err
            outs[name] = out
            log = open(tmp_path / (tag + name) / "charon.log").read()
            assert ("CHARON_GPU_INFLATE=1" in log) == name.startswith("on")
            if name.startswith("on"):
                line = [x for x in log.splitlines() if "CHARON_GPU_INFLATE=1" in x][0]
                assert "CRC-32 are checked on the device" in line, line
        assert outs["off"].count("\n") > 10
        assert outs["on"] == outs["off"] and outs["on_text"] == outs["off"], tag
        if tag == "single":
            assert_same_tsv(outs["on"], open(os.path.join(G, "cfg1_expected.tsv")).read())
