"""GPU tests (-m gpu) of what the device calls of the C ABI share (csrc/parts/abi_device_call.inc): the call timer behind
chn_stream_profile's slots 8, 9, 11 and 14, the group driver of chn_inflate_run and chn_deflate_run after a refused job, and the
path of a chn_extract append through more than one group.

Yardsticks, none of which is the code under test: chn_deflate_run_host (which tests/test_deflate_cpu.py holds against zlib) for
every deflated byte, zlib (tests/inflate_cases.py) for every inflated one, the sequential Python rule of tests/test_text_split_cpu.py
for the records."""
import ctypes

import numpy as np
import pytest

from tests import inflate_cases as ic
from tests import test_text_fetch_cpu as tfc
from tests import test_text_split_cpu as tsc
from tests.test_gpu_text_batch import api, world  # noqa: F401 (fixtures)
from tests.test_gpu_text_chain import DeviceText

pytestmark = pytest.mark.gpu

PIECE = 65280
TIMED_SLOTS = (8, 9, 11, 14)  # chn_text_split, chn_text_fetch, chn_text_pair_ids, chn_fasta_split


@pytest.fixture(scope="module")
def streams(api, world):
    """a profiling stream and one without CHN_STREAM_PROFILE"""
    prof, plain = api.Stream(world["gf"], 64, 1 << 16, profile=True), api.Stream(world["gf"], 64, 1 << 16)
    yield prof, plain
    prof.destroy()
    plain.destroy()


def test_text_split_profile_slot(api, streams):
    """slot 8: three 4 KiB tiles of text that hold a dozen four-line records"""
    prof, plain = streams
    text = tsc.join(tsc.records(12, 8, 400, 400))
    assert 2 * 4096 < len(text) <= 3 * 4096
    want = tsc.py_split(text)
    assert want["n_records"] == 12
    buf = DeviceText(api, len(text) + 16)
    try:
        n = buf.put(text)
        for which in TIMED_SLOTS:
            prof.profile(which, reset=True)
        others = [prof.profile(which) for which in TIMED_SLOTS[1:]]
        assert prof.profile(8) == (0.0, 0) and others == [(0.0, 0)] * 3
        for _ in range(2):
            tsc.assert_split_equal(prof.text_split(buf.ptr, n), want, "profiled")
        ms, calls = prof.profile(8)
        assert calls == 2 and 0.0 < ms < 1000.0
        assert prof.profile(8, reset=True) == (ms, calls)  # a reset hands out what it clears
        assert prof.profile(8) == (0.0, 0)
        assert [prof.profile(which) for which in TIMED_SLOTS[1:]] == others  # slots 9, 11 and 14 did not move
        tsc.assert_split_equal(plain.text_split(buf.ptr, n), want, "plain")
        assert plain.profile(8) == (0.0, 0)  # no CHN_STREAM_PROFILE: nothing is timed
    finally:
        buf.free()


def test_text_fetch_of_no_bytes_counts_a_call_without_a_time(api, streams):
    """every length 0: nothing runs; a profiling stream counts the call, and no time with it"""
    prof, plain = streams
    text = tfc.the_text()
    buf = DeviceText(api, len(text) + 16)
    try:
        n = buf.put(text)
        prof.profile(9, reset=True)
        assert prof.text_fetch(buf.ptr, n, (0, 17, n), (0, 0, 0)).size == 0
        assert prof.profile(9) == (0.0, 1)
        assert prof.text_fetch(buf.ptr, n, (3,), (40,)).tobytes() == text[3:43]  # a call that runs adds its time
        ms, calls = prof.profile(9, reset=True)
        assert calls == 2 and 0.0 < ms < 1000.0
        assert plain.text_fetch(buf.ptr, n, (0, 17), (0, 0)).size == 0
        assert plain.profile(9) == (0.0, 0)
    finally:
        buf.free()


def test_deflate_three_groups_behind_a_refused_job(api):
    """a job refused as a whole, then 5 pieces of 1, 65 280 and 17 bytes in groups of 2 on the same handle: three groups, both buffer
    sets used, the second one twice; the bytes are the host's"""
    r = np.random.default_rng(16)
    text = bytes(r.choice(np.frombuffer(b"ACGT", np.uint8), 2 * PIECE))
    pieces = [b"A", text[:PIECE], b"ACGTACGTACGTACGTA", text[PIECE:], b"T"]
    assert [len(p) for p in pieces] == [1, PIECE, 17, PIECE, 1]
    d = api.Deflater(0)
    try:
        d.group_members(2)
        for flags in (0, api.DEFLATE_BGZF):
            j, a = api.deflate_job([(0, 100), (70001, 0)], flags, data=np.zeros(70000, np.uint8), out=np.empty(300000, np.uint8))
            with pytest.raises(api.ChnError, match="member 1"):
                d.run_job(j)
            assert (a["out"] == 0xA5).all() and d.kernel_ms() == 0
            host, dev = api.deflate_host(pieces, flags), d.run(pieces, flags)
            assert dev["out"] == host["out"] and dev["used"] == host["used"]
            assert (dev["offset"] == host["offset"]).all() and (dev["length"] == host["length"]).all() and (dev["crc32"] == host["crc32"]).all()
            assert d.kernel_ms() > 0
    finally:
        d.destroy()


def test_inflate_three_groups_behind_a_refused_job(api):
    """a job refused as a whole, then members of the good set that inflate to more than 64 MiB on the same handle: groups close at
    32 MiB of output, so there are at least three"""
    good, _, trailing = ic.member_set()
    members = good + trailing
    pick = [int(x) for x in np.random.default_rng(17).integers(0, len(members), 1500)]
    ms, sizes = [members[i][1] for i in pick], [members[i][2] for i in pick]
    assert sum(sizes) > (64 << 20)
    want = {i: ic.yardstick(members[i][1], members[i][2])[1] for i in set(pick)}
    h = api.Inflater(0)
    try:
        j, a = api.inflate_job(ms[:3], sizes[:3])
        a["out_length"][1] = 65537
        assert api.lib().chn_inflate_run(h.h, ctypes.byref(j)) == -1 and "member 1" in api.lib().chn_last_error().decode()
        assert (a["out"] == 0xA5).all() and (a["status"] == 0xFFFFFFFF).all()
        res, st = h.run(ms, sizes)
        assert not st.any()
        assert all(got == want[i] for got, i in zip(res, pick))
    finally:
        h.destroy()


def test_extract_append_of_more_than_one_group(api):
    """one append of 1 025 pieces and a byte: a group holds 1 024 members, so the handle's second buffer set takes the last piece
    while the first group's members come down; the tail of one byte moves to the front behind it.  Every piece differs."""
    n = 1025 * PIECE + 1
    text = b"".join(b"line %07d of the append\n" % k * 2000 for k in range(n // 54000 + 1))[:n]  # (54 000 bytes between changes)
    pieces = [text[at:at + PIECE] for at in range(0, n, PIECE)]
    assert len(pieces) == 1026 and len(pieces[-1]) == 1 and len(set(pieces)) == 1026
    want = api.deflate_host(pieces, api.DEFLATE_BGZF)
    cut = int(want["offset"][1025])
    x = api.Extractor(0)
    try:
        assert x.append_bytes(text) == want["out"][:cut]
        assert x.kernel_ms() > 0
        assert x.bound(0) == 1 + 31
        assert x.finish() == want["out"][cut:]
    finally:
        x.destroy()
