"""CPU tests of the deflate member compressor through chn_deflate_run_host: the source k_deflate_members compiles, under its one-lane
policy -- the same bytes as the device's (tests/test_gpu_deflate.py compares them).  The yardsticks are Python's zlib and gzip and
the library's own decoder."""
import ctypes as C
import gzip
import struct
import zlib

import numpy as np
import pytest

import charon_amd.api as api
from tests import deflate_cases as dc


CHN_E_INVALID = -1


def check_members(pieces, r, flags):
    """everything a job's result must satisfy, member by member"""
    n, bgzf = len(pieces), bool(flags & api.DEFLATE_BGZF)
    at = 0
    for i, p in enumerate(pieces):
        o, l = int(r["offset"][i]), int(r["length"][i])
        assert o == at, (i, o, at)                                     # back to back, in member order
        at += l
        m = r["out"][o:o + l]
        assert int(r["crc32"][i]) == zlib.crc32(p)
        if bgzf:
            (blk,) = dc.parse_bgzf(m)
            assert blk[1] == l and blk[3] == zlib.crc32(p) and blk[4] == len(p)      # BSIZE, CRC-32, ISIZE
            m = blk[2]
        assert len(m) <= len(p) + 5                                    # the stored fallback
        assert dc.inflate_raw(m, len(p)) == p
        assert m[0] & 1 and (m[0] >> 1) & 3 != 3                       # one block, BFINAL set
    assert r["used"] == at and r["used"] <= r["bound"] == api.deflate_bound(n, sum(map(len, pieces)), flags)
    if bgzf and n:
        assert gzip.decompress(r["out"]) == b"".join(pieces)


@pytest.mark.parametrize("flags", [0, api.DEFLATE_BGZF])
def test_shapes_round_trip(flags):
    pieces = [p for _, p in dc.shapes()]
    r = api.deflate_host(pieces, flags)
    check_members(pieces, r, flags)


def test_bgzf_members_through_our_own_decoder():
    pieces = [p for _, p in dc.shapes()]
    r = api.deflate_host(pieces, api.DEFLATE_BGZF)
    blocks = dc.parse_bgzf(r["out"])
    assert len(blocks) == len(pieces)
    res, st, crc = api.inflate_host([b[2] for b in blocks], [b[4] for b in blocks], guard=8, expected=[b[3] for b in blocks], want_crc=True)
    assert (st == 0).all(), st
    assert res == pieces
    assert [int(c) for c in crc] == [zlib.crc32(p) for p in pieces]


def test_empty_member_is_the_bgzf_end_of_file_marker():
    r = api.deflate_host([b""], api.DEFLATE_BGZF)
    assert r["out"] == dc.BGZF_EOF and len(r["out"]) == 28
    r = api.deflate_host([b""], 0)
    assert dc.inflate_raw(r["out"], 0) == b""


def test_noise_leaves_as_a_stored_block():
    noise = dict(dc.shapes())["noise"]
    for flags in (0, api.DEFLATE_BGZF):
        r = api.deflate_host([noise], flags)
        assert int(r["length"][0]) <= len(noise) + 5 + 26
        assert (r["out"][18 if flags else 0] >> 1) & 3 == 0


def test_far_repeats_stay_inside_the_window():
    """a repeat 40 000 or 32 769 bytes back cannot be named (zlib's inflate in the round trip rejects a member that does); the one
    32 768 back can: the key of edge32768 is found again, that of edge32769 is sixteen literals"""
    s = dict(dc.shapes())
    size = {k: int(api.deflate_host([s[k]])["length"][0]) for k in ("far40000", "far32769", "edge32768", "edge32769")}
    assert size["far40000"] > 65280 and size["far32769"] > 65280       # noise whose only repeat is out of reach
    assert size["edge32768"] < size["edge32769"]


def test_scattered_pieces_at_odd_offsets():
    pieces = [p for _, p in dc.shapes()]
    data, where = dc.scattered(pieces)
    assert any(o % 2 for o, _ in where) and any(where[i + 1][0] != where[i][0] + where[i][1] for i in range(len(where) - 1))
    for flags in (0, api.DEFLATE_BGZF):
        r = api.deflate_host(where, flags, data=data)
        check_members(pieces, r, flags)
        assert r["out"] == api.deflate_host(pieces, flags)["out"]      # where a piece lies does not change its member


def test_zero_members_is_a_no_op():
    j, a = api.deflate_job([], api.DEFLATE_BGZF)
    assert api._L.chn_deflate_run_host(C.byref(j)) == 0
    assert int(a["used"][0]) == 0 and (a["out"] == 0xA5).all()


def _expect_invalid(j, a, member):
    rc = api._L.chn_deflate_run_host(C.byref(j))
    msg = api._L.chn_last_error().decode()
    assert rc == CHN_E_INVALID, (rc, msg)
    if member is not None:
        assert "member %d" % member in msg, msg
    assert (a["out"] == 0xA5).all()                                    # nothing was written
    return msg


def test_descriptor_errors():
    pieces = [b"ACGT" * 100, b"TTGA" * 50, b"N" * 30]
    # a length of 65 281
    big = np.zeros(70000, np.uint8)
    j, a = api.deflate_job([(0, 100), (10, dc.MAX_IN + 1), (5, 5)], 0, data=big, out=np.empty(300000, np.uint8))
    assert "CHN_DEFLATE_MAX_IN" in _expect_invalid(j, a, 1)
    # an offset beyond in_bytes
    j, a = api.deflate_job([(0, 100), (10, 10), (70001, 0)], 0, data=big, out=np.empty(300000, np.uint8))
    _expect_invalid(j, a, 2)
    j, a = api.deflate_job([(69990, 11), (10, 10)], 0, data=big, out=np.empty(300000, np.uint8))
    _expect_invalid(j, a, 0)
    # out_bytes one below the bound
    for flags in (0, api.DEFLATE_BGZF):
        bound = api.deflate_bound(3, sum(map(len, pieces)), flags)
        j, a = api.deflate_job(pieces, flags, out=np.empty(bound - 1, np.uint8))
        assert "chn_deflate_bound" in _expect_invalid(j, a, 2)
        j, a = api.deflate_job(pieces, flags, out=np.empty(bound, np.uint8))
        assert api._L.chn_deflate_run_host(C.byref(j)) == 0
    # a wrong struct_size, an unknown flag
    j, a = api.deflate_job(pieces, 0)
    j.struct_size += 8
    assert "struct_size" in _expect_invalid(j, a, None)
    j, a = api.deflate_job(pieces, 0)
    j.flags = 2
    assert "flag" in _expect_invalid(j, a, None)


@pytest.mark.parametrize("name,text", [(n, f) for n, f in dc.fixtures()])
def test_no_larger_than_zlib_level_1(name, text, capsys):
    """Effectiveness, against zlib and not against the code under test: the fixture's raw deflate total is at most zlib level 1's on the
    same pieces.  The ratio to level 6 (what the extract files are written with when the switch is off) is printed, not asserted."""
    pieces = dc.pieces_of(text())
    r = api.deflate_host(pieces, 0)
    check_members(pieces, r, 0)
    z1, z6 = dc.zlib_raw_total(pieces, 1), dc.zlib_raw_total(pieces, 6)
    with capsys.disabled():
        print("\n%s: %d pieces, %d bytes -> %d (zlib 1: %d, zlib 6: %d; %.3f of level 1, %.3f of level 6)"
              % (name, len(pieces), sum(map(len, pieces)), r["used"], z1, z6, r["used"] / z1, r["used"] / z6))
    assert r["used"] <= z1


def test_bgzf_framing_of_a_fixture():
    pieces = dc.pieces_of(dc.fastq_golden())
    r = api.deflate_host(pieces, api.DEFLATE_BGZF)
    check_members(pieces, r, api.DEFLATE_BGZF)
    sizes = [struct.unpack_from("<H", r["out"], int(o) + 16)[0] + 1 for o in r["offset"]]
    assert sizes == [int(x) for x in r["length"]]
