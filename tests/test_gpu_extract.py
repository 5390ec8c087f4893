"""GPU tests (-m gpu) of chn_extract: the records of an extract file formed out of a device text by k_extract_records, deflated in
place by k_deflate_members and returned as BGZF members.

Yardsticks, none of which is the new kernel or the new call: the record rule restated in Python (tests/extract_cases.py) and its
CPU twin chn_extract_records_host for the text, zlib for every member, and THE PIN -- the bytes a handle returns, finish included,
are chn_deflate_run_host's under CHN_DEFLATE_BGZF over the file's text cut at multiples of 65 280, whatever the appends were."""
import ctypes
import zlib

import numpy as np
import pytest

from tests import extract_cases as xc
from tests import inflate_cases as ic
from tests import util
from tests.test_gpu_text_batch import api, world  # noqa: F401 (fixtures)
from tests.test_gpu_text_chain import DeviceText, bgzf_members

pytestmark = pytest.mark.gpu

PIECE = 65280
E_INVALID, E_CAPACITY = -1, -5


def member_texts(data):
    """the inflated bytes of every member of `data`, each through zlib, its CRC-32 and ISIZE checked"""
    out = []
    for z, crc, isize in bgzf_members(data):
        t = zlib.decompress(z, -15)
        assert len(t) == isize and zlib.crc32(t) & 0xFFFFFFFF == crc
        out.append(t)
    return out


_PIN = {}


def pin(api, text):
    """chn_deflate_run_host over `text` cut at multiples of 65 280 (kept: several tests pin the same text)"""
    key = (len(text), zlib.crc32(text))
    if key not in _PIN:
        pieces = [text[at:at + PIECE] for at in range(0, len(text), PIECE)]
        _PIN[key] = api.deflate_host(pieces, api.DEFLATE_BGZF)["out"] if pieces else b""
    return _PIN[key]


class File:
    """one extract file: what was appended (`text`, records by the CPU twin) and what the handle returned (`got`)"""

    def __init__(self, api, out=None):
        self.api, self.x, self.text, self.got, self.out = api, api.Extractor(0), b"", b"", out

    def records(self, dev_ptr, nbytes, text, d):
        """append the records `d` of the device text at dev_ptr, whose bytes are `text`"""
        add = self.api.extract_records_host(text, *xc.args(d))
        if add:  # (a bound for no bytes is what finish needs)
            assert self.x.bound(len(add)) == ((len(self.text) % PIECE + len(add)) // PIECE) * (PIECE + 31)
        piece = self.x.append_records(dev_ptr, nbytes, *xc.args(d), out=self.out)
        self.text += add
        return self._took(piece)

    def bytes(self, data):
        piece = self.x.append_bytes(data, out=self.out)
        self.text += bytes(data)
        return self._took(piece)

    def _took(self, piece):
        self.got += piece
        assert len(self.got) == len(pin(self.api, self.text[:len(self.text) // PIECE * PIECE])), "an append returns exactly the whole pieces"
        return piece

    def finish(self):
        piece = self.x.finish(out=self.out)
        self.got += piece
        assert (piece == b"") == (len(self.text) % PIECE == 0)
        assert self.x.bound(0) == 0 and self.x.finish() == b""  # empty again
        assert self.got == pin(self.api, self.text), "the pin"
        texts = member_texts(self.got)
        assert b"".join(texts) == self.text
        assert all(len(t) == PIECE for t in texts[:-1]) and (not texts or 0 < len(texts[-1]) <= PIECE)
        return self.got

    def close(self):
        self.x.destroy()


@pytest.fixture(scope="module")
def outs(api):
    pinned = api.pinned_array(1 << 21, np.uint8)
    yield {"pageable": None, "page-locked": pinned}
    api.host_free(pinned)


def all_cases(api):
    cases = [(name, ) + getattr(xc, "case_" + name)() for name in ("lengths", "offsets", "letters")]
    cases += [("ragged%d" % k, t, d) for k, (t, d) in enumerate(xc.case_ragged_end())]
    text = xc.crlf_fastq()
    s = api.text_split_host(text, want_ids=False)
    d = {k: s[k] for k in ("id_offset", "id_length", "seq_offset", "seq_length", "qual_offset")}
    d["qual_length"] = s["seq_length"]
    cases.append(("crlf", text, d))
    cases.append(("no record", text, xc.EMPTY))
    return cases


@pytest.mark.parametrize("kind", ["pageable", "page-locked"])
def test_records_on_the_device_equal_the_host_twin_and_the_pin(api, outs, kind):
    cases = all_cases(api)
    buf = DeviceText(api, max(len(c[1]) for c in cases) + 48)
    f = File(api, outs[kind])
    try:
        for k, (name, text, d) in enumerate(cases):
            want = xc.py_records(text, d)
            for lead in ((0, 5) if k % 2 else (0, 11)):  # bytes in front: the first record's destination aligned and not
                # the text at the buffer's start or 16 / 32 bytes into it, 0xEE up to the next multiple of 16
                shift = 16 * ((k + lead) % 3)
                api.device_upload(0, buf.ptr + shift, np.frombuffer(text + b"\xEE" * (-len(text) % 16), np.uint8))
                before = len(f.text)
                f.bytes(b"x" * lead)
                f.records(buf.ptr + shift, len(text), text, d)
                assert f.text[before + lead:] == want, name
                f.finish()
                f.text, f.got = b"", b""
    finally:
        f.close()
        buf.free()


def record_of(b, total, id_len=None):
    """(id, seq, qual) of a record of exactly `total` bytes"""
    if id_len is None:
        id_len = total % 2 + (10 if total >= 18 else 0)
    n = (total - 6 - id_len) // 2
    assert id_len + 2 * n + 6 == total and n >= 0
    return b.make_id(id_len), b.make_seq(n), b.make_qual(n)


def test_tails_of_0_1_and_65279_bytes(api):
    """appends of records sized so that the tail behind the pieces is 0, 1 and 65 279 bytes, and what each returns"""
    sizes = (PIECE, PIECE + 1, PIECE - 2, 7, PIECE - 6, 2 * PIECE + 65279, 6)
    tails = (0, 1, 65279, 6, 0, 65279, 5)
    returned = (1, 1, 0, 1, 1, 2, 1)  # members
    b = xc.Builder(21)
    for k, total in enumerate(sizes):
        b.add(*record_of(b, total), k, 2 * k + 1, 17 - k)
    text, d = b.done()
    buf = DeviceText(api, len(text) + 16)
    f = File(api)
    try:
        n = buf.put(text, pad=b"\xEE")
        for k in range(len(sizes)):
            one = {key: v[k:k + 1] for key, v in d.items()}
            piece = f.records(buf.ptr, n, text, one)
            assert len(f.text) % PIECE == tails[k] and len(bgzf_members(piece)) == returned[k], k
            assert f.x.bound(0) == (tails[k] + 31 if tails[k] else 0)
        f.finish()
        # the same through append_bytes
        whole, f.text, f.got = f.text, b"", b""
        at = 0
        for total in sizes:
            f.bytes(whole[at:at + total])
            at += total
        assert f.finish() == pin(api, whole)
    finally:
        f.close()
        buf.free()


def test_a_record_across_a_piece_boundary_at_every_seam(api):
    """id 20, sequence 30, quality 30: the cut between two pieces in front of, inside and behind each of the record's fixed bytes"""
    b = xc.Builder(22)
    b.add(b.make_id(20), b.make_seq(30), b.make_qual(30), 3, 7, 13)
    text, d = b.done()
    seams = (1, 21, 22, 52, 53, 54, 55, 85)  # behind '@', id, LF, sequence, LF, '+', LF, quality
    cuts = sorted({c + e for c in seams for e in (-1, 0, 1)} - {0, 87} | {43})
    lead = np.random.RandomState(5).randint(0x21, 0x7F, PIECE).astype(np.uint8).tobytes()
    buf = DeviceText(api, len(text) + 16)
    f = File(api)
    try:
        n = buf.put(text, pad=b"\xEE")
        for cut in cuts:
            f.text, f.got = b"", b""
            f.bytes(lead[:PIECE - cut])
            piece = f.records(buf.ptr, n, text, d)
            assert len(bgzf_members(piece)) == 1 and len(f.text) % PIECE == 86 - cut, cut
            got = f.finish()
            assert b"".join(member_texts(got))[PIECE - cut:] == xc.py_records(text, d), cut
    finally:
        f.close()
        buf.free()


def test_one_read_of_70000_letters(api):
    """one record of 140 016 bytes: three pieces, every wavefront pass of the copy loops taken many times"""
    b = xc.Builder(23)
    b.add(b.make_id(10), b.make_seq(70000), b.make_qual(70000), 5, 9, 2)
    text, d = b.done()
    buf = DeviceText(api, len(text) + 16)
    f = File(api)
    try:
        n = buf.put(text, pad=b"\xEE")
        for lead in (0, 5):
            f.text, f.got = b"", b""
            f.bytes(b"y" * lead)
            piece = f.records(buf.ptr, n, text, d)
            assert len(bgzf_members(piece)) == 2
            assert len(member_texts(f.finish())) == 3
            assert f.text[lead:] == xc.py_records(text, d)
    finally:
        f.close()
        buf.free()


@pytest.fixture(scope="module")
def many(api):
    """5 000 records of 1 .. 300 letters: more than the looping grid has wavefronts; their text on the device"""
    b = xc.Builder(24)
    for k in range(5000):
        n = 1 + int(b.r.randint(0, 300))
        b.add(b.make_id(int(b.r.randint(0, 40))), b.make_seq(n), b.make_qual(n), int(b.r.randint(0, 18)), int(b.r.randint(0, 18)), int(b.r.randint(0, 18)))
    text, d = b.done()
    buf = DeviceText(api, len(text) + 16)
    n = buf.put(text, pad=b"\xEE")
    yield dict(text=text, d=d, buf=buf, n=n, want=xc.py_records(text, d))
    buf.free()


@pytest.mark.parametrize("step", [1, 37, 5000])
def test_5000_records_in_appends_of_1_37_and_all(api, many, step):
    f = File(api)
    try:
        d = many["d"]
        x, got = f.x, []
        for at in range(0, 5000, step):  # (straight through the handle: the pin of the whole file is checked once, at the end)
            got.append(x.append_records(many["buf"].ptr, many["n"], *[d[k][at:at + step] for k in xc.EMPTY], guard=0))
        f.text, f.got = many["want"], b"".join(got)
        assert len(f.got) == len(pin(api, f.text[:len(f.text) // PIECE * PIECE]))
        f.finish()
    finally:
        f.close()


def test_append_bytes_and_append_records_interleaved(api, many, outs):
    d, text = many["d"], many["text"]
    f = File(api, outs["page-locked"])
    try:
        at = 0
        for k, step in enumerate((3, 700, 1, 0, 1200, 95)):
            part = {key: v[at:at + step] for key, v in d.items()}
            if k % 2:
                f.bytes(xc.py_records(text, part))  # the host forms these itself
            else:
                f.records(many["buf"].ptr, many["n"], text, part)
            at += step
            f.bytes(b"")
        assert f.text == many["want"][:len(f.text)] and len(f.text) > 5 * PIECE
        f.finish()
    finally:
        f.close()


def test_finish_on_an_empty_handle_and_after_a_tail(api, outs):
    for kind in ("pageable", "page-locked"):
        f = File(api, outs[kind])
        try:
            assert f.finish() == b""
            f.bytes(b"@r\nACGT\n+\nIIII\n")
            got = f.finish()
            assert member_texts(got) == [b"@r\nACGT\n+\nIIII\n"]
            f.text, f.got = b"", b""
            f.bytes(b"z" * PIECE)
            assert f.finish() == pin(api, b"z" * PIECE)
        finally:
            f.close()


def test_refusals_leave_the_handle_usable(api):
    L = api.lib()
    text, d = xc.case_letters()
    buf = DeviceText(api, len(text) + 32)
    pinned = api.pinned_array(len(text) + 32, np.uint8)
    host_text = np.frombuffer(text, np.uint8).copy()
    f = File(api)
    try:
        n = buf.put(text, pad=b"\xEE")
        f.bytes(b"q" * (PIECE - 100))  # a tail, so that the job below completes a piece
        out = np.full(PIECE + 31 + 32, 0xA5, np.uint8)

        def refused(code, *words, text_ptr=buf.ptr, desc=d, edit=None, capacity=PIECE + 31):
            j, keep = api.extract_job(text_ptr, n, *xc.args(desc), out=out[16:], out_capacity=capacity)
            if edit:
                edit(j)
            rc = L.chn_extract_append_records(f.x.h, ctypes.byref(j))
            msg = L.chn_last_error().decode()
            assert rc == code, (rc, msg)
            for w in words:
                assert w in msg, msg
            assert (out == 0xA5).all() and f.x.bound(0) == PIECE - 100 + 31  # nothing written, nothing appended

        refused(E_INVALID, "struct_size", edit=lambda j: setattr(j, "struct_size", j.struct_size + 8))
        refused(E_INVALID, "flag", edit=lambda j: setattr(j, "flags", 2))
        for name in xc.EMPTY:
            refused(E_INVALID, "NULL", edit=lambda j: setattr(j, name, None))
        last = len(d["seq_offset"]) - 1
        for name, what in (("id", "id"), ("seq", "sequence"), ("qual", "quality string")):
            e = {k: v.copy() for k, v in d.items()}
            e[name + "_offset"][last] = n - int(e[name + "_length"][last]) + 1
            refused(E_INVALID, "record %d:" % last, what, "text_bytes %d" % n, desc=e)
        refused(E_INVALID, "not device memory", text_ptr=host_text.ctypes.data)
        refused(E_INVALID, "page-locked", text_ptr=pinned.ctypes.data)
        refused(E_INVALID, "16-byte aligned", text_ptr=buf.ptr + 1)
        need = f.x.bound(len(xc.py_records(text, d)))
        assert need == PIECE + 31
        refused(E_CAPACITY, "need %d bytes" % need, capacity=need - 1)
        # chn_extract_append_bytes and chn_extract_finish: the same capacity rule
        used = ctypes.c_uint64(5)
        data = np.full(200, ord("w"), np.uint8)
        assert L.chn_extract_append_bytes(f.x.h, data.ctypes.data, 200, out[16:].ctypes.data, need - 1, ctypes.byref(used)) == E_CAPACITY
        assert "need %d bytes" % need in L.chn_last_error().decode()
        assert L.chn_extract_finish(f.x.h, out[16:].ctypes.data, PIECE - 100 + 30, ctypes.byref(used)) == E_CAPACITY
        assert "need %d bytes" % (PIECE - 100 + 31) in L.chn_last_error().decode()
        assert used.value == 5 and (out == 0xA5).all() and f.x.bound(0) == PIECE - 100 + 31
        # and the handle goes on as if nothing had been asked of it
        f.records(buf.ptr, n, text, d)
        f.finish()
    finally:
        f.close()
        buf.free()
        api.host_free(pinned)


def test_the_pieces_together_bgzf_members_to_an_extract_file(api, world):
    """a BGZF file of 300 reads inflated into device memory, split there, every third record appended: the extract file inflates
    to exactly those records"""
    r = util.rng(31)
    b = xc.Builder(25)
    reads = [b.make_seq(1 + int(r.integers(0, 900)), xc.ACGT + b"NnRy") for _ in range(300)]
    recs = [(b"read%d extra/%d" % (i, i % 3), s, b.make_qual(len(s)).replace(b"@", b"A")) for i, s in enumerate(reads)]
    text = b"".join(b"@" + i + b"\n" + s + b"\n+\n" + q + b"\n" for i, s, q in recs)
    members = bgzf_members(ic.bgzf(text, block=700))
    st = api.Stream(world["gf"], 512, 1 << 20)
    inflater = api.Inflater(0)
    buf = DeviceText(api, len(text) + 16, fill=0xA5)
    f = File(api)
    try:
        _, status = inflater.run([m[0] for m in members], [m[2] for m in members], expected=[m[1] for m in members], out_device=(buf.ptr, buf.nbytes))
        assert not status.any()
        sp = st.text_split(buf.ptr, len(text), max_records=300, want_ids=False)
        assert sp["n_records"] == 300 and sp["consumed"] == len(text)
        d = {k: sp[k][::3] for k in ("id_offset", "id_length", "seq_offset", "seq_length", "qual_offset")}
        d["qual_length"] = d["seq_length"]
        f.records(buf.ptr, len(text), text, d)
        got = b"".join(member_texts(f.finish()))
        assert got == b"".join(b"@" + i + b"\n" + s.translate(xc.MAP) + b"\n+\n" + q + b"\n" for i, s, q in recs[::3])
    finally:
        f.close()
        inflater.destroy()
        st.destroy()
        buf.free()
