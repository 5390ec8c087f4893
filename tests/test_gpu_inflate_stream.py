"""chn_inflate_stream_run on the device -- k_inflate_chunks, k_inflate_windows, k_inflate_bytes -- over the cases of
tests/inflate_stream_cases.py: against zlib (bytes, CRCs) and, field by field, against the host form of the same decoder source."""
import ctypes

import numpy as np
import pytest

from tests import inflate_cases as ic
from tests import inflate_stream_cases as sc
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inflater():
    import charon_amd.api as api
    h = api.Inflater(0)
    yield h
    h.destroy()


def both(inflater, c, **more):
    import charon_amd.api as api
    dev = sc.run(inflater.run_stream, c, **more)
    sc.check(dev, c)
    sc.same(dev, sc.run(api.inflate_stream_host, c), c["name"])
    return dev


@pytest.mark.parametrize("flavour", [f[0] for f in sc.FLAVOURS])
def test_fastq_text_in_every_chunking_and_from_a_later_start(inflater, flavour):
    for c in sc.fastq_cases():
        if c["name"].startswith("fastq_%s_" % flavour):
            both(inflater, c)


def test_stored_blocks_lines_and_markers_that_live_long(inflater):
    for c in sc.stored_cases() + sc.lines_cases():
        both(inflater, c)


CRAFTED = sc.crafted_cases()


@pytest.mark.parametrize("case", CRAFTED, ids=[c["name"] for c in CRAFTED])
def test_crafted_stream(inflater, case):
    both(inflater, case, guard=256)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 600])
def test_many_small_chunks_pageable_and_page_locked(inflater, n):
    """600 chunks are more than the grid holds (two workgroups a CU): the cursor hands them out"""
    import charon_amd.api as api
    c = sc.many_chunks(n)
    both(inflater, c, guard=64)
    pinned = api.pinned_array(c["kw"]["out_bytes"] + 64, np.uint8)
    try:
        sc.check(sc.run(inflater.run_stream, c, guard=64, out=pinned), c)
    finally:
        api.host_free(pinned)


@pytest.mark.parametrize("name", ["fastq_l6_every", "ring_wrap", "no_room_for_chunk_1"])
def test_device_output_with_guard_bytes(inflater, name):
    import charon_amd.api as api
    c = [c for c in sc.fastq_cases() + CRAFTED if c["name"] == name][0]
    ob, front = c["kw"]["out_bytes"], 48 + 5  # (an odd start: the write-out's ragged ends)
    p = api.device_malloc(0, front + ob + 256)
    try:
        api.device_upload(0, p, np.full(front + ob + 256, 0xA5, np.uint8))
        res = sc.run(inflater.run_stream, c, out_device=(p + front, ob))
        assert res["bytes"] is None
        sc.check(res, c)
        got = api.device_download(0, p, front + ob + 256, np.uint8)
        assert got[front:front + res["out_used"]].tobytes() == c["text"]
        assert (got[:front] == 0xA5).all() and (got[front + ob:] == 0xA5).all()
        sc.same(res, sc.run(api.inflate_stream_host, c), name)
    finally:
        api.device_free(0, p)


def test_host_memory_as_device_output_is_refused_before_launch(inflater):
    import charon_amd.api as api
    c = sc.many_chunks(3)
    out = np.full(c["kw"]["out_bytes"], 0xA5, np.uint8)
    j, a = api.inflate_stream_job(c["data"], c["begin"], c["target"], out_bytes=out.size, out_device=(out.ctypes.data, out.size))
    assert api.lib().chn_inflate_stream_run(inflater.h, ctypes.byref(j)) == -1
    assert "not device memory" in api.lib().chn_last_error().decode()
    assert (out == 0xA5).all() and (a["status"] == 0xFFFFFFFF).all() and (a["counts"] == 2 ** 64 - 1).all()


def test_descriptor_error_runs_nothing(inflater):
    import charon_amd.api as api
    c = sc.many_chunks(4)
    j, a = api.inflate_stream_job(c["data"], c["begin"], c["target"], out_bytes=c["kw"]["out_bytes"], guard=16)
    a["target_bit"][2] = a["begin_bit"][2] - 1
    assert api.lib().chn_inflate_stream_run(inflater.h, ctypes.byref(j)) == -1
    msg = api.lib().chn_last_error().decode()
    assert "chn_inflate_stream_run:" in msg and "chunk 2" in msg
    assert (a["out"] == 0xA5).all() and (a["status"] == 0xFFFFFFFF).all() and (a["counts"] == 2 ** 64 - 1).all()
    res = inflater.run_stream(b"", [], [])
    assert res["n_counted"] == 0 and res["out_used"] == 0


def test_large_job_then_small_job_then_member_jobs_on_one_handle():
    """a large stream job, a small one, and member jobs (chn_inflate_run_crc) in between on the same handle: neither sees what the
    other left in the handle's buffers; the kernel time is that of the last run"""
    import zlib
    import charon_amd.api as api
    h = api.Inflater(0)
    try:
        big = [c for c in sc.fastq_cases() if c["name"] == "fastq_l6_every"][0]
        small = sc.many_chunks(2)
        good, _, _ = ic.member_set()
        ms, sizes = [m for _, m, _ in good], [s for _, _, s in good]
        want = [ic.yardstick(m, s)[1] for m, s in zip(ms, sizes)]
        sc.check(sc.run(h.run_stream, big), big)
        t_big = h.kernel_ms()
        res, st, crc = h.run(ms, sizes, guard=64, want_crc=True)
        assert not st.any() and res == want and [int(x) for x in crc] == [zlib.crc32(w) for w in want]
        sc.check(sc.run(h.run_stream, small, guard=64), small)
        t_small = h.kernel_ms()
        print("kernel ms: %.3f for %d bytes in %d chunks, %.3f for %d bytes in 2 chunks" % (t_big, len(big["text"]), len(big["begin"]), t_small,
                                                                                         len(small["text"])))
        assert t_big > 0 and t_small > 0
        res, st, crc = h.run(ms, sizes, guard=64, want_crc=True)
        assert not st.any() and res == want
        sc.check(sc.run(h.run_stream, big), big)
    finally:
        h.destroy()


# ---- the front end: CHARON_GPU_INFLATE_STREAM=1 ----------------------------------------------------------------------------------------
import gzip
import os
import subprocess

G = os.path.join(util.ROOT, "tests", "golden")
EXE = os.path.join(util.ROOT, "charon_amd", "bin", "charon")
IDX = os.path.join(G, "cfg1.idx")
FQ = os.path.join(G, "cfg1_reads.fastq.gz")
SWITCHES = ("CHARON_GPU_INFLATE", "CHARON_GPU_INFLATE_STREAM", "CHARON_GPU_INFLATE_ROUND", "CHARON_INFLATE_CHUNK", "CHARON_TEXT_BATCHES",
            "CHARON_NO_BGZF", "CHARON_SERIAL_INFLATE", "CHARON_ZLIB_INFLATE", "CHARON_GPU_TEXT")
ON = {"CHARON_GPU_INFLATE": "1", "CHARON_GPU_INFLATE_STREAM": "1"}
SAID = "CHARON_GPU_INFLATE_STREAM=1: the chunks of the one-stream .gz are inflated on device 0"
NOT = "CHARON_GPU_INFLATE_STREAM=1 does not apply: "


def run_cli(sub, args, cwd, env_extra=None, log=True):
    os.makedirs(cwd, exist_ok=True)
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra or {})
    p = subprocess.run([EXE, sub] + args + (["--log", os.path.join(cwd, "charon.log")] if log else []), cwd=cwd, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.fixture(scope="module")
def one_stream(tmp_path_factory):
    """the golden reads as ONE gzip member, and the text.  gzip.compress makes two deflate blocks of this text (its reads come from
    two short genomes: long matches, few symbols), which leaves a round nothing to cut; zlib's memLevel 2 ends a block every 256 symbols,
    so that chunks of a few KiB find starts.  (gzip.compress's file is test_plain_gzip_compress_falls_back's.)"""
    import zlib
    d = tmp_path_factory.mktemp("one_stream")
    text = gzip.decompress(open(FQ, "rb").read())
    f = d / "one.fastq.gz"
    c = zlib.compressobj(6, zlib.DEFLATED, 31, 2)
    f.write_bytes(c.compress(text) + c.flush())
    data = f.read_bytes()
    assert gzip.decompress(data) == text and data.count(b"\x1f\x8b\x08\x00") == 1
    return str(f), text


def device_rounds(err):
    """[(chunks with a start, chunks counted)] of the device rounds a run traced (CHARON_DIAG_INFLATE_ROUNDS)"""
    import re
    return [(int(a), int(b)) for a, b in re.findall(r"inflate round \(device\): \d+ chunks, (\d+) with a start, (\d+) counted", err)]


TRACE = {"CHARON_DIAG_INFLATE": "1", "CHARON_DIAG_INFLATE_ROUNDS": "1"}


def test_records_identical_with_the_switch_in_small_rounds(tmp_path, one_stream):
    """what the block reader sees, round by round: chunks of 2 and 4 KiB, rounds of 3 and 64 chunks, one reader thread and eight"""
    f, text = one_stream
    rc, want, err = run_cli("_records", [f, "100", "50000"], str(tmp_path), {}, log=False)
    assert rc == 0 and want.count("\n") == 200, err
    for chunk in ("2048", "4096"):
        for rnd in ("3", "64"):
            for threads in ("1", "8"):
                env = dict(ON, CHARON_INFLATE_CHUNK=chunk, CHARON_GPU_INFLATE_ROUND=rnd, CHARON_READER_THREADS=threads, **TRACE)
                rc, out, err = run_cli("_records", [f, "100", "50000"], str(tmp_path), env, log=False)
                assert rc == 0 and out == want, (chunk, rnd, threads, err)
                rounds = device_rounds(err)  # the rounds really ran on the device, and chunks behind the first were proven
                assert len(rounds) >= (2 if int(rnd) < 10 else 1) and sum(c for _, c in rounds) > len(rounds), (chunk, rnd, threads, err)
                assert all(s <= int(rnd) for s, _ in rounds)


def test_plain_gzip_compress_falls_back(tmp_path):
    """the golden reads through gzip.compress are two deflate blocks: fewer than two starts in any round, so the reader's own
    sequential decode runs, with the switch on as without it"""
    text = gzip.decompress(open(FQ, "rb").read())
    g = tmp_path / "two_blocks.fastq.gz"
    g.write_bytes(gzip.compress(text))
    rc, want, err = run_cli("_records", [str(g), "100", "50000"], str(tmp_path), {}, log=False)
    assert rc == 0 and want.count("\n") == 200, err
    rc, out, err = run_cli("_records", [str(g), "100", "50000"], str(tmp_path), dict(ON, CHARON_INFLATE_CHUNK="4096", **TRACE), log=False)
    assert rc == 0 and out == want and device_rounds(err) == [], err


def test_dehost_tsv_and_extract_files_identical(tmp_path, one_stream):
    f, text = one_stream
    outs = {}
    for name, env, t, extract in (("off", {}, "1", False), ("r3_t1", dict(ON, CHARON_INFLATE_CHUNK="4096", CHARON_GPU_INFLATE_ROUND="3"), "1", False),
                                  ("r64_t8", dict(ON, CHARON_INFLATE_CHUNK="2048", CHARON_GPU_INFLATE_ROUND="64"), "8", False),
                                  ("x_off", {}, "1", True), ("x_r3_t8", dict(ON, CHARON_INFLATE_CHUNK="4096", CHARON_GPU_INFLATE_ROUND="3"), "8", True),
                                  ("x_r64_t1", dict(ON, CHARON_INFLATE_CHUNK="3000", CHARON_GPU_INFLATE_ROUND="64"), "1", True)):
        cwd = str(tmp_path / name)
        args = ["--db", IDX, "-t", t] + (["--extract", "microbial", "-p", os.path.join(cwd, "out"), "--num_reads_to_fit", "20"] if extract else []) + [f]
        rc, out, err = run_cli("dehost", args, cwd, dict(env, **TRACE))
        assert rc == 0, (name, err)
        assert (len(device_rounds(err)) >= 1) == bool(env), (name, err)
        outs[name] = out
        assert (SAID in open(os.path.join(cwd, "charon.log")).read()) == bool(env), name
        if extract:
            outs[name + "_file"] = gzip.decompress(open(os.path.join(cwd, "out_microbial.fastq.gz"), "rb").read())
    assert outs["off"].count("\n") > 10 and outs["r3_t1"] == outs["off"] and outs["r64_t8"] == outs["off"]
    assert outs["x_r3_t8"] == outs["x_off"] and outs["x_r64_t1"] == outs["x_off"]
    assert len(outs["x_off_file"]) > 1000 and outs["x_r3_t8_file"] == outs["x_off_file"] and outs["x_r64_t1_file"] == outs["x_off_file"]
    from tests.test_gpu_cli import assert_same_tsv
    assert_same_tsv(outs["r3_t1"], open(os.path.join(G, "cfg1_expected.tsv")).read())


def test_two_members_and_a_file_smaller_than_two_chunks(tmp_path, one_stream):
    f, text = one_stream
    cut = text.index(b"\n@", len(text) // 2) + 1
    two = tmp_path / "two.fastq.gz"
    import zlib

    def member(t, level):
        c = zlib.compressobj(level, zlib.DEFLATED, 31, 2)
        return c.compress(t) + c.flush()
    two.write_bytes(member(text[:cut], 6) + member(text[cut:], 1))
    small = tmp_path / "small.fastq.gz"
    small.write_bytes(member(text[:text.index(b"\n@", 6000) + 1], 6))
    for g, env in ((two, dict(ON, CHARON_INFLATE_CHUNK="4096", CHARON_GPU_INFLATE_ROUND="3")), (two, dict(ON, CHARON_INFLATE_CHUNK="2048")),
                   (small, dict(ON, CHARON_INFLATE_CHUNK="4096")), (small, ON)):
        rc, want, err = run_cli("_records", [str(g), "100", "50000"], str(tmp_path), {}, log=False)
        assert rc == 0 and want.count("\n") > 2, err
        rc, out, err = run_cli("_records", [str(g), "100", "50000"], str(tmp_path), dict(env, **TRACE), log=False)
        assert rc == 0 and out == want, (g, env, err)
        assert (len(device_rounds(err)) >= 1) == (g == two), (g, env, err)  # (the small file: no round, the sequential decode)


def test_corrupt_and_truncated_files_fail_like_the_host_path(tmp_path, one_stream):
    f, text = one_stream
    good = open(f, "rb").read()
    for name, data in (("flip", good[:20000] + bytes([good[20000] ^ 0x10]) + good[20001:]), ("cut", good[:30000]), ("cut_trailer", good[:-4])):
        g = tmp_path / (name + ".fastq.gz")
        g.write_bytes(data)
        seen = []
        for env in ({"CHARON_INFLATE_CHUNK": "4096"}, dict(ON, CHARON_INFLATE_CHUNK="4096", CHARON_GPU_INFLATE_ROUND="3"),
                    dict(ON, CHARON_INFLATE_CHUNK="2048", CHARON_GPU_INFLATE_ROUND="64"))[:3 if name == "flip" else 2]:
            rc, out, err = run_cli("dehost", ["--db", IDX, "-t", "4", str(g)], str(tmp_path / (name + str(len(seen)))), env)
            assert rc == 1 and "gzip read error in " in err, (name, env, rc, err)
            seen.append(err)
        assert all(e == seen[0] for e in seen), (name, seen)


def test_where_the_switch_does_not_apply_and_bad_values(tmp_path, one_stream):
    import bz2
    f, text = one_stream
    (tmp_path / "b.fastq.gz").write_bytes(ic.bgzf(text, block=20000))
    (tmp_path / "z.fastq.bz2").write_bytes(bz2.compress(text))
    (tmp_path / "p.fastq").write_bytes(text)
    rc, want, err = run_cli("dehost", ["--db", IDX, f], str(tmp_path / "want"), {})
    assert rc == 0, err
    for name, g, env, why in (("bgzf", tmp_path / "b.fastq.gz", {}, "BGZF"), ("bz2", tmp_path / "z.fastq.bz2", {}, "bzip2"),
                              ("plain", tmp_path / "p.fastq", {}, "not compressed"), ("serial", f, {"CHARON_SERIAL_INFLATE": "1"}, "CHARON_SERIAL_INFLATE"),
                              ("zlib", f, {"CHARON_ZLIB_INFLATE": "1"}, "CHARON_ZLIB_INFLATE")):
        cwd = str(tmp_path / name)
        rc, out, err = run_cli("dehost", ["--db", IDX, str(g)], cwd, dict(ON, **env))
        assert rc == 0 and out == want, (name, err)
        log = open(os.path.join(cwd, "charon.log")).read()
        assert log.count(NOT) == 1 and why in log.split(NOT)[1].split("\n")[0] and SAID not in log, (name, log)
    (tmp_path / "junk.idx").write_bytes(b"not an index")
    for env in ({"CHARON_GPU_INFLATE": "1", "CHARON_GPU_INFLATE_STREAM": "2"}, {"CHARON_GPU_INFLATE": "1", "CHARON_GPU_INFLATE_STREAM": ""},
                {"CHARON_GPU_INFLATE_STREAM": "1"}, {"CHARON_GPU_INFLATE": "0", "CHARON_GPU_INFLATE_STREAM": "1"}):
        rc, out, err = run_cli("dehost", ["--db", str(tmp_path / "junk.idx"), f], str(tmp_path / "v"), env)
        assert rc == 1 and out == "" and "charon: CHARON_GPU_INFLATE_STREAM: " in err and "junk.idx" not in err, (env, err)
