"""CPU tests of chn_extract_records_host: the record rule of the extract files ('@' id LF SEQ LF '+' LF qual LF, SEQ through the front
end's letter map) by the source k_extract_records compiles (charon_amd/csrc/parts/extract_records.inc), and the refusals of
chn_extract_append_records that need no device (the host call makes the same checks).

The yardstick is a Python restatement of the rule (tests/extract_cases.py: py_records); it never calls into the library.  The cases
are what tests/test_gpu_extract.py runs through the kernel as well."""
import ctypes

import numpy as np
import pytest

import charon_amd.api as api
from tests import extract_cases as xc

L = api.lib()


def host(text, d, **kw):
    return api.extract_records_host(text, *xc.args(d), **kw)


def test_letter_map_of_every_byte():
    """the 256 bytes as one sequence, at every position of a dword: letters by the front end's table, all else N"""
    for shift in range(4):
        seq = bytes(range(256)) * 2
        text = b"#" * shift + seq
        d = dict(id_offset=[0], id_length=[0], seq_offset=[shift], seq_length=[len(seq)], qual_offset=[shift], qual_length=[0])
        got = host(text, d)
        assert got == b"@\n" + seq.translate(xc.MAP) + b"\n+\n\n"
    assert bytes(range(256)).translate(xc.MAP).count(b"N") == 256 - 10  # only A C G T U and their lower case are not N


@pytest.mark.parametrize("case", ["lengths", "offsets", "letters"])
def test_rule_against_restatement(case):
    text, d = getattr(xc, "case_" + case)()
    assert host(text, d) == xc.py_records(text, d)


def test_lengths_case_has_every_length():
    text, d = xc.case_lengths()
    assert set(d["id_length"].tolist()) == set(xc.ID_LENGTHS) and set(d["seq_length"].tolist()) == set(xc.SEQ_LENGTHS)
    assert any(b" " in text[int(o):int(o) + int(l)] for o, l in zip(d["id_offset"], d["id_length"]))
    text, d = xc.case_offsets()
    assert len({(int(a) % 16, int(b) % 16, int(c) % 16) for a, b, c in zip(d["id_offset"], d["seq_offset"], d["qual_offset"])}) == 16 ** 3


def test_ranges_that_end_at_a_ragged_text_end():
    """text_bytes is no multiple of 16 and a range ends exactly there: no byte behind the text is looked at (the text is an array of
    exactly its size)"""
    for text, d in xc.case_ragged_end():
        arr = np.frombuffer(text, np.uint8).copy()
        assert host(arr, d) == xc.py_records(text, d)


def test_crlf_text():
    text = xc.crlf_fastq()
    s = api.text_split_host(text, want_ids=False)
    assert s["n_records"] == 40 and s["consumed"] == len(text)
    d = {k: s[k] for k in ("id_offset", "id_length", "seq_offset", "seq_length", "qual_offset")}
    d["qual_length"] = s["seq_length"]
    got = host(text, d)
    assert b"\r" not in got
    assert got == xc.py_records(text, d)
    # and that is what a plain parser makes of the text with the \r dropped
    lines = text.replace(b"\r\n", b"\n").split(b"\n")[:-1]
    want = b"".join(lines[i] + b"\n" + lines[i + 1].translate(xc.MAP) + b"\n+\n" + lines[i + 3] + b"\n" for i in range(0, len(lines), 4))
    assert got == want


def test_no_record():
    assert host(b"", xc.EMPTY) == b""
    assert host(b"@a\nA\n+\nI\n", xc.EMPTY) == b""


def test_empty_ranges():
    d = {k: np.zeros(3, a.dtype) for k, a in xc.EMPTY.items()}
    assert host(b"", d) == b"@\n\n+\n\n" * 3


def _job(text, d):
    buf = np.frombuffer(bytes(text), np.uint8)
    j, keep = api.extract_job(buf.ctypes.data if buf.size else None, buf.size, *xc.args(d))
    return j, (buf, keep)


def _refused(j, code, *words, capacity=1 << 20):
    out = np.full(capacity + 1, 0xA5, np.uint8)
    got = ctypes.c_uint64(77)
    rc = L.chn_extract_records_host(ctypes.byref(j), out.ctypes.data, capacity, ctypes.byref(got))
    msg = L.chn_last_error().decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, msg
    assert got.value == 77 and bytes(out) == b"\xa5" * out.size  # nothing written
    return msg


def test_refusals_that_need_no_device():
    text, d = xc.case_letters()
    E_INVALID, E_CAPACITY = -1, -5
    msg = None
    j, keep = _job(text, d)
    j.struct_size -= 8
    _refused(j, E_INVALID, "struct_size")
    j, keep = _job(text, d)
    j.flags = 1
    _refused(j, E_INVALID, "flag")
    for name in ("id_offset", "id_length", "seq_offset", "seq_length", "qual_offset", "qual_length"):
        j, keep = _job(text, d)
        setattr(j, name, None)
        _refused(j, E_INVALID, "NULL")
    n = len(d["id_offset"])
    for rec, name, what in ((0, "id", "id"), (n // 2, "seq", "sequence"), (n - 1, "qual", "quality string")):
        for kind in range(3):
            e = {k: v.copy() for k, v in d.items()}
            if kind == 0:    # one byte too far
                e[name + "_offset"][rec] = len(text) - int(e[name + "_length"][rec]) + 1
            elif kind == 1:  # the offset itself behind the text
                e[name + "_offset"][rec] = len(text) + 1
                e[name + "_length"][rec] = 0
            else:            # a sum that wraps
                e[name + "_offset"][rec] = 0xFFFFFFFFFFFFFFFE
                e[name + "_length"][rec] = 9
            j, keep = _job(text, e)
            msg = _refused(j, E_INVALID, "record %d:" % rec, what, "text_bytes %d" % len(text))
    j, keep = _job(text, d)
    need = len(xc.py_records(text, d))
    _refused(j, E_CAPACITY, "need %d bytes" % need, capacity=need - 1)
    # and the job as it stands is taken
    assert host(text, d) == xc.py_records(text, d)
    assert msg
