"""CPU tests of the CRC-32 behind chn_inflate_run_host_crc -- the 64 slices and the join k_inflate_members<true> runs, walked serially by the
host policy of the same source.  The yardstick is Python's zlib.crc32 of the bytes Python's zlib inflates (tests/inflate_cases.py), never
this code's own output."""
import ctypes
import functools
import gzip
import os
import random
import re
import struct
import subprocess
import zlib

import pytest

from tests import inflate_cases as ic
from tests import util

# where a slice is empty, one byte long, or where the 64 slices differ in length
LENGTHS = [0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 65279, 65280, 65535, 65536]
NAMES = ["chn_inflate_run_crc", "chn_inflate_run_host_crc"]
G = os.path.join(util.ROOT, "tests", "golden")
EXE = os.path.join(util.ROOT, "charon_amd", "bin", "charon")
CORRUPT = "a BGZF member is corrupt (inflate, size or CRC32 mismatch)"


@functools.lru_cache(maxsize=None)
def crc_set():
    """list of (name, member, size, bytes, zlib.crc32 of the bytes): FASTQ-like and random bytes of every length of LENGTHS, then the good
    and the trailing members of inflate_cases.member_set().  Shared with tests/test_gpu_inflate_crc.py; nobody changes it."""
    r = random.Random(606)
    noise = bytes(r.randrange(256) for _ in range(ic.MAX_OUT))
    out = []
    for n in LENGTHS:
        for kind, data in (("fastq", ic.fastq_text(n, 1000 + n)), ("random", noise[ic.MAX_OUT - n:])):
            out.append(("%s_%d" % (kind, n), ic.raw(data), n, data, zlib.crc32(data)))
    good, _, trailing = ic.member_set()
    for name, m, s in good + trailing:
        ok, data = ic.yardstick(m, s)
        assert ok
        out.append((name, m, s, data, zlib.crc32(data)))
    return out


def test_crc_of_every_length_in_one_job():
    import charon_amd.api as api
    cs = crc_set()
    res, st, crc = api.inflate_host([c[1] for c in cs], [c[2] for c in cs], guard=64, want_crc=True)
    assert not st.any()
    for (name, _, _, data, want), out, got in zip(cs, res, crc):
        assert out == data, name
        assert int(got) == want, (name, hex(int(got)), hex(want))
    assert int(crc[0]) == 0 and cs[0][2] == 0  # a member of length 0 has CRC 0


def test_crc_one_member_at_a_time():
    import charon_amd.api as api
    for name, m, s, data, want in crc_set():
        res, st, crc = api.inflate_host([m], [s], want_crc=True)
        assert int(st[0]) == 0 and res[0] == data and int(crc[0]) == want, name


def test_correct_expected_is_status_0_and_one_wrong_one_is_status_7_there_only():
    import charon_amd.api as api
    cs = crc_set()
    ms, sizes, want = [c[1] for c in cs], [c[2] for c in cs], [c[4] for c in cs]
    res, st = api.inflate_host(ms, sizes, guard=64, expected=want)
    assert not st.any() and res == [c[3] for c in cs]
    for at in (0, 7, len(cs) // 2, len(cs) - 1):
        exp = list(want)
        exp[at] ^= 1 << (at % 32)
        res, st, crc = api.inflate_host(ms, sizes, guard=64, expected=exp, want_crc=True)
        assert [int(x) for x in st] == [7 if i == at else 0 for i in range(len(cs))]
        assert res == [c[3] for c in cs]                # the bytes are what the stream decodes to
        assert [int(x) for x in crc] == want            # and the CRC that was found is reported
    assert api.INFLATE_E_CRC == 7 and "#define CHN_INFLATE_E_CRC 7u" in _header()


def test_rejected_members_keep_their_status_with_expected_present():
    import charon_amd.api as api
    _, bad, _ = ic.member_set()
    cases = [(m, s) for _, m, s in bad] + ic.sweep_cases()[:200]
    ms, sizes = [m for m, _ in cases], [s for _, s in cases]
    _, plain = api.inflate_host(ms, sizes, guard=64)
    verdicts = [ic.yardstick(m, s) for m, s in cases]
    exp = [zlib.crc32(out) if ok else 0x12345678 for ok, out in verdicts]
    res, st, crc = api.inflate_host(ms, sizes, guard=64, expected=exp, want_crc=True)
    assert (st == plain).all()
    assert all(int(x) != 0 for x in st[:len(bad)]) and 0 < sum(1 for x in st if x == 0) < len(cases)
    for (ok, out), r, s_, c, e in zip(verdicts, res, st, crc, exp):
        assert (int(s_) == 0) == ok
        if ok:
            assert r == out and int(c) == e
    # and with a wrong CRC everywhere: 7 exactly where the member decodes, the decode failures unchanged
    _, st7 = api.inflate_host(ms, sizes, guard=64, expected=[e ^ 0x80000000 for e in exp])
    assert [int(x) for x in st7] == [7 if int(p) == 0 else int(p) for p in plain]


def _job():
    import charon_amd.api as api
    cs = [c for c in crc_set() if c[0] in ("fastq_4097", "random_65", "dynamic", "empty")]
    assert len(cs) == 4
    j, a = api.inflate_job([c[1] for c in cs], [c[2] for c in cs], guard=8)
    return cs, j, a


def test_null_crc_and_two_null_arrays_are_the_plain_call():
    import charon_amd.api as api
    cs, j0, a0 = _job()
    assert api.lib().chn_inflate_run_host(ctypes.byref(j0)) == 0
    _, j1, a1 = _job()
    assert api.lib().chn_inflate_run_host_crc(ctypes.byref(j1), None) == 0
    _, j2, a2 = _job()
    c, _ = api.inflate_crc(len(cs))
    assert not c.expected and not c.crc32
    assert api.lib().chn_inflate_run_host_crc(ctypes.byref(j2), ctypes.byref(c)) == 0
    for a in (a1, a2):
        assert (a["status"] == a0["status"]).all() and (a["out"] == a0["out"]).all()
    assert not a0["status"].any()


@pytest.mark.parametrize("case", ["struct_size_small", "struct_size_large", "reserved"])
def test_bad_crc_struct_is_invalid_and_runs_nothing(case):
    import charon_amd.api as api
    cs, j, a = _job()
    c, ca = api.inflate_crc(len(cs), [x[4] for x in cs], True)
    if case == "struct_size_small":
        c.struct_size -= 8
    elif case == "struct_size_large":
        c.struct_size += 8
    else:
        c.reserved = 1
    assert api.lib().chn_inflate_run_host_crc(ctypes.byref(j), ctypes.byref(c)) == -1  # CHN_E_INVALID
    assert "chn_inflate_run_host_crc" in api.lib().chn_last_error().decode()
    assert (a["out"] == 0xA5).all() and (a["status"] == 0xFFFFFFFF).all() and (ca["crc32"] == 0xFFFFFFFF).all()
    # the job's own checks and their messages are those of the plain call
    cs, j, a = _job()
    c, ca = api.inflate_crc(len(cs), None, True)
    a["out_length"][1] = 65537
    assert api.lib().chn_inflate_run_host_crc(ctypes.byref(j), ctypes.byref(c)) == -1
    assert "member 1 has out_length above CHN_INFLATE_MAX_OUT" in api.lib().chn_last_error().decode()
    assert (a["status"] == 0xFFFFFFFF).all() and (ca["crc32"] == 0xFFFFFFFF).all()


def _header():
    return open(os.path.join(util.ROOT, "include", "charon_hip.h")).read()


def test_crc_struct_layout_matches_header():
    import charon_amd.api as api
    body = re.search(r"typedef struct chn_inflate_crc \{(.*?)\} chn_inflate_crc;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = re.match(r"(const\s+)?(\w+)", decl).group(2)
        for name in re.sub(r"^(const\s+)?\w+\s*", "", decl).split(","):
            fields.append((name.replace("*", "").strip(), "ptr" if "*" in decl else base))
    want = [(n, "ptr" if t is ctypes.c_void_p else {ctypes.c_uint32: "uint32_t"}[t]) for n, t in api.InflateCrc._fields_]
    assert fields == want == [("struct_size", "uint32_t"), ("reserved", "uint32_t"), ("expected", "ptr"), ("crc32", "ptr")]
    assert ctypes.sizeof(api.InflateCrc) == 24 and api.InflateCrc.expected.offset == 8 and api.InflateCrc.crc32.offset == 16
    assert ctypes.sizeof(api.InflateJob) == 88  # the job is the one it was


def test_names_declared_described_exported():
    import charon_amd.api as api
    header = _header()
    integration = open(os.path.join(util.ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in api.EXPORTS and getattr(api.lib(), name) is not None
        assert name in integration, name


def test_front_end_rejects_a_flipped_crc_bit_on_the_host_path(tmp_path):
    """the switch unset, a BGZF file whose second member has one bit flipped in its stored CRC: exit status 1 and the message the
    device path has to reproduce"""
    data = gzip.decompress(open(os.path.join(G, "cfg1_reads.fastq.gz"), "rb").read())
    good = ic.bgzf(data, block=20000)
    second = good.index(b"\x1f\x8b\x08\x04", 100)
    total = struct.unpack("<H", good[second + 16:second + 18])[0] + 1
    bad = bytearray(good)
    bad[second + total - 8 + 1] ^= 0x10  # the trailer: CRC32 (4 bytes), ISIZE (4 bytes)
    f = tmp_path / "bad_crc.fastq.gz"
    f.write_bytes(bytes(bad))
    env = {k: v for k, v in os.environ.items() if k not in ("CHARON_GPU_INFLATE", "CHARON_NO_BGZF", "CHARON_TEXT_BATCHES")}
    p = subprocess.run([EXE, "_records", str(f), "50", "100000"], env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 1 and CORRUPT in p.stderr.decode(), (p.returncode, p.stderr.decode())
    f.write_bytes(good)
    p = subprocess.run([EXE, "_records", str(f), "50", "100000"], env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stdout.count(b"\n") > 40, p.stderr.decode()
