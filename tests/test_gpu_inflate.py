"""GPU tests (-m gpu) of k_inflate_members behind chn_inflate_run and of CHARON_GPU_INFLATE=1 in the front end.  The yardstick is
Python's zlib (tests/inflate_cases.py); the host decoder (chn_inflate_run_host) is compared status by status on top."""
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import inflate_cases as ic
from tests import util
from tests.test_gpu_cli import assert_same_tsv

pytestmark = pytest.mark.gpu
G = os.path.join(util.ROOT, "tests", "golden")
EXE = os.path.join(util.ROOT, "charon_amd", "bin", "charon")
IDX = os.path.join(G, "cfg1.idx")
FQ = os.path.join(G, "cfg1_reads.fastq.gz")
SWITCHES = ("CHARON_GPU_INFLATE", "CHARON_TEXT_BATCHES", "CHARON_NO_BGZF")


@pytest.fixture(scope="module")
def inflater():
    import charon_amd.api as api
    h = api.Inflater(0)
    yield h
    h.destroy()


@pytest.fixture(scope="module")
def good_set():
    good, _, trailing = ic.member_set()
    members = good + trailing
    return members, [ic.yardstick(m, s)[1] for _, m, s in members]


def draw(good_set, n, seed):
    """n members drawn from the good set, sizes mixed; their expected bytes"""
    members, want = good_set
    r = util.rng(seed)
    pick = [int(x) for x in r.integers(0, len(members), n)]
    return [members[i][1] for i in pick], [members[i][2] for i in pick], [want[i] for i in pick]


def test_member_set_in_one_job(inflater, good_set):
    import charon_amd.api as api
    members, want = good_set
    res, st = inflater.run([m for _, m, _ in members], [s for _, _, s in members], guard=64)
    assert [int(x) for x in st] == [0] * len(members)
    for (name, _, _), out, w in zip(members, res, want):
        assert out == w, name
    hres, hst = api.inflate_host([m for _, m, _ in members], [s for _, _, s in members], guard=64)
    assert (hst == st).all() and hres == res


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_job_sizes_pageable_and_page_locked(inflater, good_set, n):
    import charon_amd.api as api
    ms, sizes, want = draw(good_set, n, 100 + n)
    res, st = inflater.run(ms, sizes, guard=64)  # pageable out, gaps between the members: through staging
    assert not st.any() and res == want
    pinned = api.pinned_array(sum(sizes) + 16, np.uint8)
    try:
        res, st = inflater.run(ms, sizes, guard=0, out=pinned)  # page-locked, members back to back: downloaded into directly
        assert not st.any() and res == want
        assert (pinned[sum(sizes):] == 0xA5).all()
        res, st = inflater.run(ms, sizes, guard=16 if n > 1 else 0, out=api.pinned_array(sum(sizes) + 16 * n + 16, np.uint8))
        assert not st.any() and res == want  # page-locked with gaps
    finally:
        api.host_free(pinned)


def test_large_job_then_small_job_on_one_handle(good_set):
    """1 100 members: more than one group (over 32 MiB of output) and more members than the grid has workgroups; then a job of two
    on the same handle, which must not see what the large one left in the staging buffers"""
    import charon_amd.api as api
    h = api.Inflater(0)
    try:
        ms, sizes, want = draw(good_set, 1100, 7)
        assert sum(sizes) > (40 << 20)
        res, st = h.run(ms, sizes)
        assert not st.any() and res == want
        ms, sizes, want = draw(good_set, 2, 8)
        res, st = h.run(ms, sizes, guard=64)
        assert not st.any() and res == want
        res, st = h.run([], [])
        assert res == [] and len(st) == 0
    finally:
        h.destroy()


def test_rejected_members_and_mutations_between_good_ones(inflater, good_set):
    """the rejected members and the first 200 cases of the mutation sweep (every one of which the host decoder has been through in
    tests/test_inflate_cpu.py), each between good members: the status is non-zero exactly where zlib rejects, equal to the host
    decoder's, the neighbours are intact and no byte behind an out_length is written"""
    import charon_amd.api as api
    _, bad, _ = ic.member_set()
    members, want = good_set
    small = [i for i, (n, _, _) in enumerate(members) if n in ("fixed_one_byte", "empty", "run_of_a", "dynamic", "stored")]
    cases = [(m, s) for _, m, s in bad] + ic.sweep_cases()[:200]
    verdicts = [ic.yardstick(m, s) for m, s in cases]
    ms, sizes, expect = [], [], []
    for k, ((m, s), (ok, out)) in enumerate(zip(cases, verdicts)):
        g = small[k % len(small)]
        ms += [members[g][1], m]; sizes += [members[g][2], s]; expect += [want[g], out if ok else None]
    hres, hst = api.inflate_host(ms, sizes, guard=64)
    res, st = inflater.run(ms, sizes, guard=64)  # raises if a guard byte was touched
    assert [(int(x) == 0) for x in st] == [e is not None for e in expect]
    assert res == expect
    assert (st == hst).all() and res == hres


@functools.lru_cache(maxsize=None)
def crafted_good():
    """the crafted good set and the foreign set (streams zlib's deflate does not write): (members, sizes, names, zlib's bytes)"""
    good, _ = ic.crafted_set()
    every = good + [(n, m, s) for n, m, s, _ in ic.foreign_set()]
    return [m for _, m, _ in every], [s for _, _, s in every], [n for n, _, _ in every], [ic.yardstick(m, s)[1] for _, m, s in every]


@functools.lru_cache(maxsize=None)
def crafted_bad_job():
    """the crafted rejects and the first 300 cases of crafted_sweep() (every one of which the host decoder has been through in
    tests/test_inflate_cpu.py), each behind a small good member: (members, sizes, zlib's bytes -- None where zlib rejects)"""
    _, bad = ic.crafted_set()
    good, _, trailing = ic.member_set()
    small = [(m, s, ic.yardstick(m, s)[1]) for n, m, s in good if n in ("fixed_one_byte", "empty", "run_of_a", "dynamic", "stored")]
    cases = [(m, s) for _, m, s in bad] + ic.crafted_sweep()[:300]
    verdicts = [ic.yardstick(m, s) for _, m, s in bad] + ic.crafted_sweep_verdicts()[:300]
    ms, sizes, expect = [], [], []
    for k, ((m, s), (ok, out)) in enumerate(zip(cases, verdicts)):
        g = small[k % len(small)]
        ms += [g[0], m]; sizes += [g[1], s]; expect += [g[2], out if ok else None]
    assert sum(e is None for e in expect) >= 12 + 10 and sum(e is not None for e in expect[1::2]) >= 10
    return ms, sizes, expect


@functools.lru_cache(maxsize=None)
def repeated_job(copies=70):
    """all_symbols and many_blocks `copies` times each, in turn.  In front of copy k stand filler members (stored blocks of 0 .. 15
    bytes, empty members) that bring its input onto the offset k mod 16 of the caller's array and its output -- the members of a job
    lie back to back in device memory, and the window is shifted by the output's misalignment -- onto 7 k + 3 mod 16: every class of
    either occurs for both members.  (members, sizes, zlib's bytes, crcs)"""
    import zlib
    from tests import deflate_writer as dw
    good, _ = ic.crafted_set()
    big = [(m, s, ic.yardstick(m, s)[1]) for n, m, s in good if n in ("all_symbols", "many_blocks")]
    assert len(big) == 2
    r = util.rng(70)
    empty = (b"\x03\x00", 0, b"")

    def fillers(din, dout):
        for n_stored in (0, 1, 2):
            for n_empty in range(8):
                if (5 * n_stored + (dout if n_stored else 0) + 2 * n_empty) % 16 == din and (dout if n_stored else 0) == dout:
                    payload = [bytes(int(x) for x in r.integers(0, 256, dout if q == 0 else 0)) for q in range(n_stored)]
                    return [(dw.write([dw.stored(p)]), len(p), p) for p in payload] + [empty] * n_empty
        raise AssertionError((din, dout))

    job, at_in, at_out, seen_in, seen_out = [], 0, 0, set(), set()
    for k in range(copies):
        for which, b in enumerate(big):
            for f in fillers((k - at_in) % 16, (7 * k + 3 + which - at_out) % 16):
                job.append(f)
                at_in += len(f[0]); at_out += f[1]
            seen_in.add((which, at_in % 16)); seen_out.add((which, at_out % 16))
            job.append(b)
            at_in += len(b[0]); at_out += b[1]
    assert len(seen_in) == 32 and len(seen_out) == 32
    assert all(ic.yardstick(m, s) == (True, w) for m, s, w in job if s < 16)
    return [j[0] for j in job], [j[1] for j in job], [j[2] for j in job], [zlib.crc32(j[2]) & 0xFFFFFFFF for j in job]


def test_crafted_and_foreign_members_in_one_job(inflater):
    """the streams zlib's deflate never writes: every length and distance symbol out of tables of 14- and 15-bit codes, single-code
    and empty sets, repeat codes across HLIT, 200 table builds in one member, stored headers at every bit position, libdeflate's
    members -- status 0, zlib's bytes, and the host decoder's results status by status"""
    import charon_amd.api as api
    ms, sizes, names, want = crafted_good()
    res, st = inflater.run(ms, sizes, guard=64)
    assert [n for n, x in zip(names, st) if int(x) != 0] == []
    for name, out, w in zip(names, res, want):
        assert out == w, name
    hres, hst = api.inflate_host(ms, sizes, guard=64)
    assert (hst == st).all() and hres == res


def test_crafted_rejects_and_mutations_between_good_ones(inflater):
    """non-zero exactly where zlib rejects, the host decoder's status, the neighbours intact, no byte behind an out_length written"""
    import charon_amd.api as api
    ms, sizes, expect = crafted_bad_job()
    hres, hst = api.inflate_host(ms, sizes, guard=64)
    res, st = inflater.run(ms, sizes, guard=64)  # raises if a guard byte was touched
    assert [(int(x) == 0) for x in st] == [e is not None for e in expect]
    assert res == expect
    assert (st == hst).all() and res == hres


def test_all_symbols_and_many_blocks_seventy_times(inflater):
    """more members than one pass of a small grid, so a workgroup builds these tables over what the previous member left; see
    repeated_job for the offsets"""
    ms, sizes, want, _ = repeated_job()
    assert len(ms) > 140
    res, st = inflater.run(ms, sizes)
    assert not st.any() and res == want


def test_descriptor_error_runs_nothing(inflater, good_set):
    import ctypes
    import charon_amd.api as api
    ms, sizes, _ = draw(good_set, 3, 5)
    j, a = api.inflate_job(ms, sizes)
    a["out_length"][1] = 65537
    assert api.lib().chn_inflate_run(inflater.h, ctypes.byref(j)) == -1
    assert "member 1" in api.lib().chn_last_error().decode()
    assert (a["out"] == 0xA5).all() and (a["status"] == 0xFFFFFFFF).all()


# ---- the front end -------------------------------------------------------------------------------------------------------------------
def run_cli(sub, args, cwd, env_extra=None, log=True):
    os.makedirs(cwd, exist_ok=True)
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra or {})
    p = subprocess.run([EXE, sub] + args + (["--log", os.path.join(cwd, "charon.log")] if log else []), cwd=cwd, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def test_records_identical_with_and_without_the_switch(tmp_path):
    text = ic.fastq_text(80000, 3)
    text = text[:text.rindex(b"\n@") + 1]
    f = tmp_path / "r.fastq.gz"
    f.write_bytes(ic.bgzf(text, block=len(text) // 19))
    assert f.read_bytes().count(b"\x1f\x8b\x08\x04") >= 21  # 20 members and the end-of-file marker
    outs = []
    for env in ({}, {"CHARON_GPU_INFLATE": "1"}, {"CHARON_GPU_INFLATE": "0"}, {"CHARON_NO_BGZF": "1"}, {"CHARON_GPU_INFLATE": "1", "CHARON_NO_BGZF": "1"},
                {"CHARON_GPU_INFLATE": "1", "CHARON_READER_THREADS": "4"}):
        rc, out, err = run_cli("_records", [str(f), "100", "20000"], str(tmp_path), env, log=False)
        assert rc == 0, err
        outs.append(out)
    assert outs[0].count("\n") > 100 and all(o == outs[0] for o in outs)


def test_dehost_golden_bgzf_single_and_paired(tmp_path):
    data = gzip.decompress(open(FQ, "rb").read())
    b1 = tmp_path / "g_1.fastq.gz"
    b1.write_bytes(ic.bgzf(data, block=20000))
    b2 = tmp_path / "g_2.fastq.gz"
    b2.write_bytes(ic.bgzf(data, block=65280))
    for tag, files in (("single", [str(b1)]), ("paired", [str(b1), str(b2)])):
        outs = {}
        for name, env in (("off", {}), ("on", {"CHARON_GPU_INFLATE": "1"}), ("on_text", {"CHARON_GPU_INFLATE": "1", "CHARON_TEXT_BATCHES": "1"}),
                          ("on_t8", {"CHARON_GPU_INFLATE": "1", "CHARON_BATCH_READS": "37"})):
            rc, out, err = run_cli("dehost", ["--db", IDX, "-t", "8" if name == "on_t8" else "1"] + files, str(tmp_path / (tag + name)), env)
            assert rc == 0, err
            outs[name] = out
            said = "CHARON_GPU_INFLATE=1" in open(tmp_path / (tag + name) / "charon.log").read()
            assert said == (name != "off")
        assert outs["off"].count("\n") > 10
        assert outs["on"] == outs["off"] and outs["on_text"] == outs["off"] and outs["on_t8"] == outs["off"], tag
        if tag == "single":
            assert_same_tsv(outs["on"], open(os.path.join(G, "cfg1_expected.tsv")).read())


def test_corrupt_member_and_bad_value(tmp_path):
    data = gzip.decompress(open(FQ, "rb").read())
    good = ic.bgzf(data, block=20000)
    second = good.index(b"\x1f\x8b\x08\x04", 100)
    bad = bytearray(good)
    bad[second + 18 + 200] ^= 0x40  # a byte of the second member's deflate data
    f = tmp_path / "bad.fastq.gz"
    f.write_bytes(bytes(bad))
    errs = []
    for env in ({}, {"CHARON_GPU_INFLATE": "1"}):
        rc, out, err = run_cli("dehost", ["--db", IDX, str(f)], str(tmp_path / ("c" + "".join(env.values()))), env)
        assert rc == 1 and "a BGZF member is corrupt (inflate, size or CRC32 mismatch)" in err, (rc, err)
        errs.append(err)
    assert errs[0] == errs[1]
    (tmp_path / "junk.idx").write_bytes(b"not an index")
    for v in ("2", "", "yes"):
        rc, out, err = run_cli("dehost", ["--db", str(tmp_path / "junk.idx"), FQ], str(tmp_path / "v"), {"CHARON_GPU_INFLATE": v})
        assert rc == 1 and out == "" and "charon: CHARON_GPU_INFLATE: " in err and "junk.idx" not in err, (v, err)
