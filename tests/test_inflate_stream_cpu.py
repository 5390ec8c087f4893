"""CPU tests of chn_inflate_stream_run_host -- the chunk decoder, the window hand-down and the symbol-to-byte rules that
k_inflate_chunks / k_inflate_windows / k_inflate_bytes run, on one host thread.  The yardstick for bytes is Python's zlib over the whole
stream and zlib.crc32 (tests/inflate_stream_cases.py), never the code under test."""
import ctypes
import os
import re
import subprocess

import pytest

from tests import inflate_cases as ic
from tests import inflate_stream_cases as sc
from tests import util

NAMES = ["chn_inflate_stream_run", "chn_inflate_stream_run_host"]


def _header():
    return open(os.path.join(util.ROOT, "include", "charon_hip.h")).read()


def test_job_layout_matches_header():
    import charon_amd.api as api
    body = re.search(r"typedef struct chn_inflate_stream_job \{(.*?)\} chn_inflate_stream_job;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ptr = "*" in decl
        base = re.match(r"(const\s+)?(\w+)", decl).group(2)
        for name in re.sub(r"^(const\s+)?\w+\s*", "", decl).split(","):
            fields.append((name.replace("*", "").strip(), "ptr" if ptr else base))
    want = [(n.rstrip("_"), "ptr" if t is ctypes.c_void_p else {ctypes.c_uint32: "uint32_t", ctypes.c_uint64: "uint64_t"}[t])
            for n, t in api.InflateStreamJob._fields_]
    assert fields == want
    assert [n for n, _ in fields] == ["struct_size", "flags", "n_chunks", "in", "in_bytes", "begin_bit", "target_bit", "window", "window_bytes",
                                     "sym_capacity", "out", "out_bytes", "end_bit", "out_length", "status", "final", "crc32", "n_counted",
                                     "out_used"]
    assert ctypes.sizeof(api.InflateStreamJob) == 144
    assert api.InflateStreamJob.n_chunks.offset == 8 and api.InflateStreamJob.out.offset == 72 and api.InflateStreamJob.out_used.offset == 136
    header = _header()
    assert api.INFLATE_STREAM_MAX_CHUNKS == 4096 and "#define CHN_INFLATE_STREAM_MAX_CHUNKS 4096u" in header
    assert api.INFLATE_STREAM_MIN_SYMS == 131072 and "#define CHN_INFLATE_STREAM_MIN_SYMS 131072u" in header
    assert api.INFLATE_E_ROOM == 8 and "#define CHN_INFLATE_E_ROOM 8u" in header
    assert ctypes.sizeof(api.InflateJob) == 88 and ctypes.sizeof(api.InflateCrc) == 24  # no existing struct changed


def test_names_declared_described_exported():
    import charon_amd.api as api
    header = _header()
    integration = open(os.path.join(util.ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in api.EXPORTS and getattr(api.lib(), name) is not None
        assert name in integration, name
    assert "src/dehost_main.cpp:324" in header


@pytest.mark.parametrize("flavour", [f[0] for f in sc.FLAVOURS])
def test_fastq_text_in_every_chunking_and_from_a_later_start(flavour):
    import charon_amd.api as api
    cases = [c for c in sc.fastq_cases() if c["name"].startswith("fastq_%s_" % flavour)]
    assert len(cases) == 9
    for c in cases:
        sc.check(sc.run(api.inflate_stream_host, c), c)
    # the short window is not enough for this text: the first chunk whose matches reach further says so (Z_RLE: all distances are 1)
    assert any(c["status"][-1] == 4 for c in cases if c["name"].endswith("w1000")) == (flavour != "rle")
    assert all(set(c["status"]) == {0} for c in cases if not c["name"].endswith("w1000"))


def test_stored_blocks_and_the_empty_block_alone():
    import charon_amd.api as api
    for c in sc.stored_cases():
        sc.check(sc.run(api.inflate_stream_host, c), c)


def test_markers_that_live_to_a_chunks_end():
    import charon_amd.api as api
    for c in sc.lines_cases():
        sc.check(sc.run(api.inflate_stream_host, c), c)


CRAFTED = sc.crafted_cases()


@pytest.mark.parametrize("case", CRAFTED, ids=[c["name"] for c in CRAFTED])
def test_crafted_stream(case):
    import charon_amd.api as api
    sc.check(sc.run(api.inflate_stream_host, case), case)


def test_the_crafted_set_holds_what_it_claims():
    names = [c["name"] for c in CRAFTED]
    assert len(set(names)) == len(names)
    for kind in sc.corrupt_kinds():
        for at in (0, 2):
            c = [c for c in CRAFTED if c["name"] == "corrupt_%s_in_chunk_%d" % (kind, at)][0]
            assert len(c["begin"]) == 4 and c["n_counted"] == at + 1 and c["status"][-1] in (1, 2, 3, 4) and c["lengths"][-1] > 0
    by = {c["name"]: c for c in CRAFTED}
    assert by["capacity_block_first"]["lengths"] == [0] and by["capacity_block_third"]["lengths"] == [1300]
    assert len(by["ring_wrap"]["text"]) > 40000 + 3 * 32768
    assert by["no_room_for_chunk_1"]["status"] == [0, sc.E_ROOM]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 600])
def test_many_small_chunks(n):
    import charon_amd.api as api
    c = sc.many_chunks(n)
    assert len(c["begin"]) == n
    sc.check(sc.run(api.inflate_stream_host, c), c)


def test_without_crc_array():
    import charon_amd.api as api
    c = sc.many_chunks(5)
    res = sc.run(api.inflate_stream_host, c, want_crc=False)
    assert res["crc32"] is None and res["bytes"] == c["text"] and res["n_counted"] == 5


def _job(**kw):
    import charon_amd.api as api
    c = sc.many_chunks(4)
    args = dict(window=c["window"], out_bytes=c["kw"]["out_bytes"], guard=16)
    args.update(kw)
    return api.inflate_stream_job(c["data"], c["begin"], c["target"], **args)


ERRORS = ["struct_size", "flag", "begin_not_increasing", "begin_equal", "begin_beyond", "target_before_begin", "window_too_long", "capacity",
          "too_many_chunks"]


@pytest.mark.parametrize("case", ERRORS)
def test_descriptor_errors_are_invalid_and_name_the_chunk(case):
    import charon_amd.api as api
    j, a = _job()
    chunk = None
    if case == "struct_size":
        j.struct_size -= 8
    elif case == "flag":
        j.flags = 2
    elif case == "begin_not_increasing":
        a["begin_bit"][2] = a["begin_bit"][1] - 1
        a["target_bit"][2] = a["begin_bit"][2]
        chunk = 2
    elif case == "begin_equal":
        a["begin_bit"][3] = a["begin_bit"][2]
        chunk = 3
    elif case == "begin_beyond":
        a["begin_bit"][3] = a["target_bit"][3] = 8 * j.in_bytes
        chunk = 3
    elif case == "target_before_begin":
        a["target_bit"][1] = a["begin_bit"][1] - 1
        chunk = 1
    elif case == "window_too_long":
        j.window_bytes = 32769
    elif case == "capacity":
        j.sym_capacity = 131071
    else:
        j.n_chunks = 4097
    rc = api.lib().chn_inflate_stream_run_host(ctypes.byref(j))
    assert rc == -1  # CHN_E_INVALID
    msg = api.lib().chn_last_error().decode()
    assert "chn_inflate_stream_run_host" in msg
    if chunk is not None:
        assert ("chunk %d" % chunk) in msg, msg
    # nothing ran, nothing was written
    assert (a["out"] == 0xA5).all() and (a["status"] == 0xFFFFFFFF).all() and (a["end_bit"] == 2 ** 64 - 1).all()
    assert (a["out_length"] == 2 ** 64 - 1).all() and (a["final"] == 0xFF).all() and (a["crc32"] == 0xFFFFFFFF).all()
    assert (a["counts"] == 2 ** 64 - 1).all()


def test_the_host_form_refuses_device_output_and_an_empty_job_is_a_no_op():
    import charon_amd.api as api
    j, a = _job()
    j.flags = api.INFLATE_OUT_DEVICE
    assert api.lib().chn_inflate_stream_run_host(ctypes.byref(j)) == -1
    res = api.inflate_stream_host(b"", [], [])
    assert res["n_counted"] == 0 and res["out_used"] == 0 and res["bytes"] == b""
    j, a = _job()
    j.n_chunks = 0
    assert api.lib().chn_inflate_stream_run_host(ctypes.byref(j)) == 0
    assert (a["out"] == 0xA5).all() and (a["status"] == 0xFFFFFFFF).all() and list(a["counts"]) == [0, 0]


def test_guard_bytes_behind_out_bytes_stay_untouched():
    import charon_amd.api as api
    c = sc.room_case()
    res = sc.run(api.inflate_stream_host, c, guard=4096)  # (raises if a byte behind out_bytes was written)
    sc.check(res, c)
    full = sc.zcase("exact_room", "fastq", 6, 0, 40000, lambda cuts: cuts[:3])
    full["kw"]["out_bytes"] = sum(full["lengths"])
    sc.check(sc.run(api.inflate_stream_host, full, guard=4096), full)


def test_switch_value_is_checked_and_off_is_todays_path(tmp_path):
    """CHARON_GPU_INFLATE_STREAM: anything but 0 / 1, or 1 without CHARON_GPU_INFLATE=1, ends the run with status 1 before a file is opened;
    0 is the path of the unset switch; `charon index` does not read it"""
    import gzip
    exe = os.path.join(util.ROOT, "charon_amd", "bin", "charon")
    text = ic.fastq_text(30000, 4)
    text = text[:text.rindex(b"\n@") + 1]
    f = tmp_path / "r.fastq.gz"
    f.write_bytes(gzip.compress(text))
    env = {k: v for k, v in os.environ.items() if k not in ("CHARON_GPU_INFLATE", "CHARON_GPU_INFLATE_STREAM", "CHARON_NO_BGZF")}
    runs = {}
    for v in (None, "0", "2", "", "1"):
        e = dict(env) if v is None else dict(env, CHARON_GPU_INFLATE_STREAM=v)
        runs[v] = subprocess.run([exe, "_records", str(f), "50", "10000"], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert runs[None].returncode == 0 and runs[None].stdout.count(b"\n") > 40
    assert runs["0"].returncode == 0 and runs["0"].stdout == runs[None].stdout
    for v in ("2", "", "1"):
        assert runs[v].returncode == 1 and runs[v].stdout == b"" and b"charon: CHARON_GPU_INFLATE_STREAM: " in runs[v].stderr
    assert b"CHARON_GPU_INFLATE=1" in runs["1"].stderr
    (tmp_path / "none.idx").write_bytes(b"not an index")
    for sub in ("dehost", "classify"):
        for e in (dict(env, CHARON_GPU_INFLATE="1", CHARON_GPU_INFLATE_STREAM="on"), dict(env, CHARON_GPU_INFLATE_STREAM="1")):
            p = subprocess.run([exe, sub, "--db", str(tmp_path / "none.idx"), str(f)], env=e, cwd=str(tmp_path), stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, timeout=120)
            assert p.returncode == 1 and b"charon: CHARON_GPU_INFLATE_STREAM: " in p.stderr and b"none.idx" not in p.stderr
    # `charon index` does not read it: a bad value changes nothing about what it says of a missing input
    said = [subprocess.run([exe, "index", str(tmp_path / "no_such_table.tsv")], env=e, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=120) for e in (dict(env), dict(env, CHARON_GPU_INFLATE_STREAM="bogus"))]
    assert said[0].returncode == said[1].returncode and said[0].stderr == said[1].stderr and b"CHARON_GPU_INFLATE_STREAM" not in said[1].stderr
