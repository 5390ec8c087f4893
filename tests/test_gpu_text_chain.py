"""GPU tests (-m gpu) of the device-resident text chain: chn_inflate_run with CHN_INFLATE_OUT_DEVICE, chn_text_split, and
chn_text_submit / chn_text_pack with CHN_TEXT_ON_DEVICE -- BGZF members to per-read calls while the text stays in device memory.

Yardsticks, none of which is the new code: zlib and the host decoder for the inflated bytes, the sequential Python rule of
tests/test_text_split_cpu.py (and the CPU twin on top) for the records, the host-text path of the same batch for every result
column bitwise, the oracle for parity, zlib for the gzip sizes.  The shapes are the smallest at which the kernels can go wrong."""
import re
import struct
import zlib

import numpy as np
import pytest

from tests import inflate_cases as ic
from tests import test_text_split_cpu as tsc
from tests import util
from tests.test_gpu_parity import run_oracle
from tests.test_gpu_text_batch import api, awkward_batch, good_quals, random_quals, with_n, world, zsize  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu


class DeviceText:
    """a device buffer under the device text contract: 16-byte aligned, its size a multiple of 16"""

    def __init__(self, api, nbytes, fill=None):
        self.api, self.nbytes = api, (max(int(nbytes), 16) + 15) & ~15
        self.ptr = api.device_malloc(0, self.nbytes)
        if fill is not None:
            self.put(np.full(self.nbytes, fill, np.uint8))

    def put(self, data, pad=b"\n"):
        """upload `data`; the bytes up to the next multiple of 16 become `pad` (line feeds: a reader that does not mask them counts them)"""
        data = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else data
        n = (data.size + 15) & ~15
        assert n <= self.nbytes
        if n:
            self.api.device_upload(0, self.ptr, np.concatenate([data, np.full(n - data.size, ord(pad), np.uint8)]))
        return data.size

    def get(self, nbytes=None):
        return self.api.device_download(0, self.ptr, self.nbytes if nbytes is None else nbytes, np.uint8)

    def free(self):
        self.api.device_free(0, self.ptr)


@pytest.fixture(scope="module")
def inflater(api):
    h = api.Inflater(0)
    yield h
    h.destroy()


# ---- 1. inflate into device memory ---------------------------------------------------------------------------------------------------
def spread(sizes, gaps=(0, 1, 3, 15, 16, 17)):
    """out offsets with gaps[i % 6] bytes in front of member i: every gap, and with them every misalignment, occurs"""
    offs, at = [], 0
    for i, s in enumerate(sizes):
        at += gaps[i % len(gaps)]
        offs.append(at)
        at += s
    return offs, at + 32


def test_inflate_into_device_memory_member_set(api, inflater):
    good, bad, trailing = ic.member_set()
    members = good + bad + trailing + good[::-1]  # (the second run of good members meets other gaps and alignments)
    ms, sizes = [m for _, m, _ in members], [s for _, _, s in members]
    hres, hst, hcrc = api.inflate_host(ms, sizes, want_crc=True)
    assert (hst != 0).sum() == len(bad)
    offs, total = spread(sizes)
    assert len({o % 16 for o in offs}) >= 8
    stretch = np.zeros(total, bool)
    for o, s in zip(offs, sizes):
        stretch[o:o + s] = True
    buf = DeviceText(api, total)
    try:
        expected = [zlib.crc32(r) if r is not None else 0 for r in hres]
        for kw in (dict(), dict(want_crc=True), dict(expected=expected, want_crc=True)):
            buf.put(np.full(buf.nbytes, 0xA5, np.uint8))
            got = inflater.run(ms, sizes, out_device=(buf.ptr, buf.nbytes), out_offset=offs, **kw)
            assert got[0] is None and (got[1] == hst).all(), kw
            out = buf.get()
            for i, (o, s) in enumerate(zip(offs, sizes)):
                if hst[i] == 0:
                    assert out[o:o + s].tobytes() == hres[i], (kw, members[i][0])
            assert (out[:total][~stretch] == 0xA5).all() and (out[total:] == 0xA5).all(), kw  # no gap byte was written
            if kw:
                ok = hst == 0
                assert (got[2][ok] == hcrc[ok]).all(), kw
    finally:
        buf.free()


def test_inflate_into_device_memory_beyond_the_group_limit(api, inflater):
    """70 000 members -- more than one group of 65 536 -- of one byte each, three bytes apart, a longer member now and then"""
    good, _, _ = ic.member_set()
    d = {n: (m, s) for n, m, s in good}
    one, text = d["fixed_one_byte"], d["fixed"]
    want_text = ic.yardstick(*text)[1]
    n = 70000
    ms = [text[0] if i % 9973 == 5 else one[0] for i in range(n)]
    sizes = [text[1] if i % 9973 == 5 else one[1] for i in range(n)]
    offs, at = [], 0
    for s in sizes:
        offs.append(at)
        at += s + 2
    buf = DeviceText(api, at, fill=0xA5)
    try:
        _, st, crc = inflater.run(ms, sizes, out_device=(buf.ptr, buf.nbytes), out_offset=offs, want_crc=True)
        assert not st.any()
        out = buf.get()
        want = np.full(buf.nbytes, 0xA5, np.uint8)
        for i in range(n):
            if sizes[i] == 1:
                want[offs[i]] = ord("A")
            else:
                want[offs[i]:offs[i] + sizes[i]] = np.frombuffer(want_text, np.uint8)
        assert np.array_equal(out, want)
        assert crc[0] == zlib.crc32(b"A") and crc[5] == zlib.crc32(want_text) and crc[n - 1] == zlib.crc32(b"A")
    finally:
        buf.free()


def test_inflate_refuses_output_that_is_not_device_memory(api, inflater):
    import ctypes
    good, _, _ = ic.member_set()
    ms, sizes = [good[3][1], good[2][1]], [good[3][2], good[2][2]]
    want = [ic.yardstick(m, s)[1] for m, s in zip(ms, sizes)]
    pinned = api.pinned_array(sum(sizes) + 64, np.uint8)
    pageable = np.zeros(sum(sizes) + 64, np.uint8)
    buf = DeviceText(api, sum(sizes) + 64, fill=0xA5)
    try:
        for host, word in ((pinned, "page-locked"), (pageable, "not device memory")):
            j, a = api.inflate_job(ms, sizes, out=host)
            j.flags = api.INFLATE_OUT_DEVICE
            assert api.lib().chn_inflate_run(inflater.h, ctypes.byref(j)) == -1
            assert word in api.lib().chn_last_error().decode() and "out" in api.lib().chn_last_error().decode()
            assert (host == 0xA5).all() and (a["status"] == 0xFFFFFFFF).all()  # nothing ran
        j, a = api.inflate_job(ms, sizes, out_device=(buf.ptr, buf.nbytes))
        j.flags |= 2
        assert api.lib().chn_inflate_run(inflater.h, ctypes.byref(j)) == -1 and "unknown flag" in api.lib().chn_last_error().decode()
        assert (buf.get() == 0xA5).all()
        res, st = inflater.run(ms, sizes, guard=16)  # the handle works on
        assert not st.any() and res == want
        _, st = inflater.run(ms, sizes, out_device=(buf.ptr, buf.nbytes))
        assert not st.any() and buf.get(sum(sizes)).tobytes() == b"".join(want)
    finally:
        buf.free()
        api.host_free(pinned)


# ---- 2. records found on the device --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream(api, world):
    st = api.Stream(world["gf"], 4096, 1 << 22)
    st.set_model(api.default_model(2, world["gf"].desc.host_index))
    yield st
    st.destroy()


def placed_cases():
    """texts whose first record is sized so that a line feed, a \\r, an '@' or a record end falls on byte P of the buffer, P on either
    side of a 16-byte piece, a 1 KiB round and a 4 KiB tile; and texts whose `start` lies there, behind a record or behind line feeds"""
    rest = tsc.join(tsc.records(9, 31))
    rec = lambda id_bytes, eol=b"\n": b"@" + b"i" * id_bytes + eol + b"A" + eol + b"+" + eol + b"F" + eol
    cases = []
    for P in (15, 16, 1023, 1024, 4095, 4096):
        cases.append(("id_line_feed_at_%d" % P, rec(P - 1) + rest, 0, None))
        cases.append(("cr_at_%d" % P, rec(P - 1, b"\r\n") + rest, 0, None))
        cases.append(("at_sign_at_%d" % P, rec(P - 8) + rest, 0, None))
        cases.append(("record_end_at_%d" % P, rec(P - 7) + rest, 0, None))
        cases.append(("crlf_record_end_at_%d" % P, rec(P - 11, b"\r\n") + rest, 0, None))
        for S in (P, P + 1):
            cases.append(("start_%d_behind_a_record" % S, rec(S - 8) + rest, S, None))
            cases.append(("start_%d_behind_a_crlf_record" % S, rec(S - 12, b"\r\n") + rest, S, None))
            cases.append(("start_%d_behind_line_feeds" % S, b"\n" * S + rest, S, None))
            cases.append(("start_%d_inside_a_line" % S, b"\n" * S + rest[3:], S, None))
    for name, text, start, m in cases:  # the texts are what their names say
        P = int(re.search(r"\d+", name).group())
        if name.startswith(("id_line_feed", "cr_at")):
            assert text[P:P + 1] == (b"\n" if name.startswith("id") else b"\r"), name
        if name.startswith(("at_sign", "start")) and "inside" not in name:
            assert text[P:P + 1] == b"@" and text[P - 1:P] == b"\n", name
        if "record_end_at" in name:
            assert text[P:P + 2] == b"\n@", name
        if "inside" not in name:
            assert tsc.py_split(text, start)["n_records"] == (10 if start == 0 else 9), name
    return cases


def test_split_on_the_device_equals_the_host_twin_and_the_python_rule(api, stream):
    cases = tsc.all_cases() + placed_cases()
    buf = DeviceText(api, max(len(c[1]) for c in cases) + 16)
    try:
        for name, text, start, m in cases:
            n = buf.put(text)
            want = tsc.py_split(text, start, m)
            tsc.assert_split_equal(stream.text_split(buf.ptr, n, start=start, max_records=m), want, name)
            tsc.assert_split_equal(api.text_split_host(text, start=start, max_records=m), want, name)
        # without the ids: everything else alike
        name, text, start, m = cases[0]
        got = stream.text_split(buf.ptr, buf.put(text), want_ids=False)
        assert got["ids"] is None
        tsc.assert_split_equal(dict(got, ids=tsc.py_split(text)["ids"]), tsc.py_split(text), name)
    finally:
        buf.free()


def test_split_70000_short_records(api, stream):
    """records that span many tiles and wavefronts; a start in the middle, a record bound inside a wavefront, a failure far in"""
    recs = tsc.records(70000, 77, 1, 9)
    text = tsc.join(recs)
    assert len(text) > 300 * 4096
    buf = DeviceText(api, len(text) + 16)
    try:
        n = buf.put(text)
        want = tsc.py_split(text)
        assert want["n_records"] == 70000
        tsc.assert_split_equal(stream.text_split(buf.ptr, n), want, "all")
        mid = int(want["id_offset"][33333]) - 1
        tsc.assert_split_equal(stream.text_split(buf.ptr, n, start=mid), tsc.py_split(text, mid), "start")
        for m in (65, 4096, 69999):
            tsc.assert_split_equal(stream.text_split(buf.ptr, n, max_records=m), tsc.py_split(text, 0, m), m)
        broken = bytearray(text)
        broken[int(want["seq_offset"][50001])] = ord("+")
        n = buf.put(broken)
        got = stream.text_split(buf.ptr, n)
        assert got["n_records"] == 50001
        tsc.assert_split_equal(got, tsc.py_split(broken), "broken")
    finally:
        buf.free()


def test_split_refusals_leave_the_stream_usable(api, stream):
    import ctypes
    from charon_amd import pack
    L = api.lib()
    text = tsc.join(tsc.records(50, 3))
    want = tsc.py_split(text)
    buf = DeviceText(api, len(text) + 64)
    pinned = api.pinned_array(len(text) + 16, np.uint8)
    pageable = np.frombuffer(text + b"\n" * 16, np.uint8).copy()
    pinned[:len(text)] = np.frombuffer(text, np.uint8)
    try:
        n = buf.put(text)

        def call(ptr, **over):
            j, a = api.text_split_job(ptr, n)
            for k, v in over.items():
                setattr(j, k, v)
            return L.chn_text_split(stream.h, ctypes.byref(j)), L.chn_last_error().decode()

        for ptr, word in ((pinned.ctypes.data, "page-locked"), (pageable.ctypes.data, "not device memory"), (buf.ptr + 1, "16-byte aligned")):
            rc, err = call(ptr)
            assert rc == -1 and word in err, err
        for over, word in ((dict(struct_size=8), "struct_size"), (dict(flags=4), "flag"), (dict(start=n + 1), "start"), (dict(seq_offset=None), "NULL")):
            rc, err = call(buf.ptr, **over)
            assert rc == -1 and word in err, err
        rc, err = call(buf.ptr, text_bytes=api.TEXT_SPLIT_MAX_BYTES + 16)
        assert rc == -5 and "CHN_TEXT_SPLIT_MAX_BYTES" in err
        rc, err = call(buf.ptr, ids_capacity=want["ids_bytes"] - 1)
        assert rc == -5 and ("need %d bytes" % want["ids_bytes"]) in err, err
        # three batches in flight
        r = util.rng(5)
        reads = [util.random_seq(r, 200) for _ in range(8)]
        tb = pack.text_batch(reads, good_quals(r, reads), gap=b"\n")
        for _ in range(3):
            stream.submit_text(tb, np.zeros(len(reads), np.float32))
        rc, err = call(buf.ptr)
        assert rc == -1 and "three batches" in err
        first = stream.wait_text()
        tsc.assert_split_equal(stream.text_split(buf.ptr, n), want, "two in flight")  # batches in flight are not disturbed
        for _ in range(2):
            util.assert_same_results(stream.wait_text(), first)
    finally:
        buf.free()
        api.host_free(pinned)


# ---- 3. text batches from device text ------------------------------------------------------------------------------------------------
def assert_same_packed(a, b):
    assert (a["n_bases"], a["has_n"]) == (b["n_bases"], b["has_n"])
    for k in ("bases2", "nmask", "seg1_offset", "seg1_length", "seg2_offset", "seg2_length"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or np.array_equal(a[k], b[k])), k
    assert np.array_equal(a["mean_quality"].view(np.uint32), b["mean_quality"].view(np.uint32))


@pytest.mark.parametrize("paired", [False, True])
def test_text_batch_from_device_text(api, world, paired):
    from charon_amd import pack
    r = util.rng(41)
    seqs, quals = awkward_batch(r)
    mates = mquals = None
    if paired:
        mates = [s[::-1][:max(0, len(s) - 7)] for s in seqs]
        mates[3] = util.random_seq(r, 1000)
        mquals = [random_quals(r, len(m)) for m in mates]
        mquals[4] = random_quals(r, len(mates[4]) + 20)
    n = len(seqs)
    g, oidx = world["gf"], world["fused"]
    st = api.Stream(g, n, pack.pack_reads(seqs, mates)["n_bases"])
    st.set_model(api.default_model(2, 0 if paired else g.desc.host_index, paired=paired))
    pinned = None
    bufs = []
    try:
        comp = np.zeros(n, np.float32)
        for gap, ranks in ((b"\n", False), (b"\n+\n", False), (b"\x07" * 3, True)):
            tb = pack.text_batch(seqs, quals, mates, mquals, gap=gap, ranks=ranks)
            buf = DeviceText(api, tb["text"].size)
            bufs.append(buf)
            nbytes = buf.put(tb["text"], pad=b"X")  # (a letter that is illegal if it is ever packed)
            dev = (buf.ptr, nbytes)
            for _ in range(2):  # (twice: the slot's buffers are recycled)
                assert_same_packed(st.text_pack(tb, text_device=dev), st.text_pack(tb))
            st.submit_text(tb, comp)
            host = st.wait_text()
            st.submit_text(dict(tb, text=None), comp, text_device=dev)  # the descriptors alone: the host text is not looked at
            got = st.wait_text()
            util.assert_same_results(got, host)
            for k in ("flags", "has_n", "n_bases"):
                assert np.array_equal(got[k], host[k]), k
            assert np.array_equal(got["mean_quality"].view(np.uint32), host["mean_quality"].view(np.uint32))
            if not ranks:
                util.assert_parity(got, run_oracle(oidx, seqs, mates))
        # refusals: host memory with the flag, before any launch; the stream takes an ordinary batch afterwards
        tb = pack.text_batch(seqs, quals, mates, mquals, gap=b"\n")
        pinned = api.pinned_array(tb["text"].size + 16, np.uint8)
        pinned[:tb["text"].size] = tb["text"]
        pageable = np.concatenate([tb["text"], np.zeros(16, np.uint8)])
        for call in (st.submit_text, st.text_pack):
            for host_text, word in ((pinned, "page-locked"), (pageable, "not device memory")):
                with pytest.raises(api.ChnError, match="error -1:.*CHN_TEXT_ON_DEVICE.*" + word):
                    call(tb, text_device=(host_text.ctypes.data, tb["text"].size))
            with pytest.raises(api.ChnError, match="error -1:.*16-byte aligned"):
                call(tb, text_device=(bufs[0].ptr + 4, tb["text"].size))
        st.submit_text(tb, comp)
        util.assert_same_results(st.wait_text(), host)
    finally:
        st.destroy()
        for buf in bufs:
            buf.free()
        if pinned is not None:
            api.host_free(pinned)


# ---- 4. BGZF members to calls --------------------------------------------------------------------------------------------------------
def bgzf_members(data):
    """(deflate data, CRC-32, inflated size) of every member of a BGZF file"""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 14] == b"BC"
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", data, at + size - 8)
        out.append((data[at + 18:at + size - 8], crc, isize))
        at += size
    return out


def test_bgzf_members_to_calls(api, world, inflater):
    r = util.rng(91)
    gs = world["gs"]
    reads = with_n(r, util.sample_reads(r, gs, 1990, (30, 1500)))
    reads += [util.mutate(r, gs[i % 2][1000 * i:1000 * i + L], 0.03) for i, L in enumerate((40000, 33000, 32768, 32767, 20000, 9000, 30, 31, 5000, 17000))]
    order = r.permutation(len(reads))
    reads = [reads[i] for i in order]
    quals = good_quals(r, reads)
    ids = [b"read%d some text/%d" % (i, len(s)) if i % 11 else b"" for i, s in enumerate(reads)]
    text = b"".join(b"@" + i + b"\n" + s + b"\n+\n" + q + b"\n" for i, s, q in zip(ids, reads, quals))
    members = bgzf_members(ic.bgzf(text))
    assert len(members) > 40 and members[-1][2] == 0  # (the end-of-file marker is a member like any other)
    cum = np.concatenate([[0], np.cumsum([m[2] for m in members])])
    n = len(reads)
    from charon_amd import pack
    g = world["gf"]
    st = api.Stream(g, n, pack.pack_reads(reads)["n_bases"])
    st.set_model(api.default_model(2, g.desc.host_index))
    buf = DeviceText(api, len(text) + 16, fill=0xA5)
    gz = dict(gzip_tallies=61440, gzip_output=api.GZIP_SIZES)
    try:
        got_ids, got, host = [], [], []
        first, start, k = 0, 0, len(members) // 2
        for last in (k, len(members)):  # two jobs; the second starts with the members that hold the first one's tail
            part = members[first:last]
            nbytes = int(cum[last] - cum[first])
            _, status = inflater.run([m[0] for m in part], [m[2] for m in part], expected=[m[1] for m in part],
                                     out_device=(buf.ptr, buf.nbytes))
            assert not status.any()
            sp = st.text_split(buf.ptr, nbytes, start=start, max_records=n)
            assert sp["n_records"] > 0
            tsc.assert_split_equal(sp, tsc.py_split(text[cum[first]:cum[last]], start, n), last)
            at = 0
            for length in sp["id_length"]:
                got_ids.append(sp["ids"][at:at + int(length)])
                at += int(length)
            tb = dict(seq1_offset=sp["seq_offset"], seq1_length=sp["seq_length"], qual1_offset=sp["qual_offset"], qual1_length=sp["seq_length"])
            st.submit_text(tb, text_device=(buf.ptr, nbytes), **gz)
            got.append(st.wait_text())
            st.submit_text(dict(tb, text=np.frombuffer(text[cum[first]:cum[last]], np.uint8)), **gz)  # the host-text path, same descriptors
            host.append(st.wait_text())
            # the caller-side carry: where the tail begins, in the file's inflated bytes, and the member that holds that byte
            tail = int(cum[first]) + sp["consumed"]
            first = int(np.searchsorted(cum, tail, side="right")) - 1
            start = tail - int(cum[first])
        assert tail == len(text) and got_ids == ids
        assert len(got[0]["call"]) + len(got[1]["call"]) == n and min(len(x["call"]) for x in got) > 200
        for a, b in zip(got, host):
            util.assert_same_results(a, b)
            for key in ("flags", "gzip_sizes", "has_n", "n_bases"):
                assert np.array_equal(a[key], b[key]), key
            assert np.array_equal(a["mean_quality"].view(np.uint32), b["mean_quality"].view(np.uint32))
        both = {key: np.concatenate([got[0][key], got[1][key]]) for key in ("num_hashes", "counts", "unique", "conf", "call", "probs", "gzip_sizes")}
        util.assert_parity(both, run_oracle(world["fused"], reads))
        assert [int(x) for x in both["gzip_sizes"]] == [zsize(s) for s in reads]
        assert (both["call"] != 255).sum() > 300
    finally:
        st.destroy()
        buf.free()
