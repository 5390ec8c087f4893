"""CPU tests of chn_text_split_host: FASTQ records found by the rule source that chn_text_split's kernels compile
(charon_amd/csrc/parts/text_split.inc), and the host-side refusals of the calls that came with it.

The yardstick is py_split below: a sequential Python restatement of the record rule as include/charon_hip.h spells it out.  It never
calls into the library.  Every case compares every descriptor array, n_records, consumed, the ids and ids_bytes.  The case list
(all_cases) is what tests/test_gpu_text_chain.py runs through the kernels as well."""
import ctypes
import functools
import random

import numpy as np
import pytest

from tests import inflate_cases as ic

KEYS = ("id_offset", "id_length", "seq_offset", "seq_length", "qual_offset")


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------
def strip_cr(line):
    return line[:-1] if line.endswith(b"\r") else line


def py_record(t, p, end):
    """the record that starts at byte p of t[:end], as (descriptor, offset behind it), or None where the rule fails"""
    if p >= end or t[p:p + 1] != b"@":                        # its first byte is '@'
        return None
    feeds, q = [], p
    for _ in range(4):                                        # four line feeds follow inside [start, text_bytes)
        e = t.find(b"\n", q, end)
        if e < 0:
            return None
        feeds.append(e)
        q = e + 1
    seq = strip_cr(t[feeds[0] + 1:feeds[1]])                  # the sequence line, one trailing \r dropped: n >= 1, no '+' in front
    if len(seq) < 1 or seq.startswith(b"+"):
        return None
    if not t[feeds[1] + 1:feeds[2]].startswith(b"+"):         # the third line begins with '+'
        return None
    if len(strip_cr(t[feeds[2] + 1:feeds[3]])) != len(seq):   # the fourth line, one trailing \r dropped, has length n
        return None
    ident = strip_cr(t[p + 1:feeds[0]])                       # the id: behind '@' up to the line end, minus one trailing \r
    return (p + 1, len(ident), feeds[0] + 1, len(seq), feeds[2] + 1), feeds[3] + 1


def py_split(t, start=0, max_records=None, end=None):
    t = bytes(t)
    end = len(t) if end is None else end
    recs, p, ids = [], start, b""
    while max_records is None or len(recs) < max_records:
        got = py_record(t, p, end)
        if got is None:
            break
        recs.append(got[0])
        ids += t[got[0][0]:got[0][0] + got[0][1]]
        p = got[1]
    out = {k: np.array([r[i] for r in recs], np.uint64 if k.endswith("offset") else np.uint32) for i, k in enumerate(KEYS)}
    out.update(n_records=len(recs), consumed=p, ids=ids, ids_bytes=len(ids))
    return out


def assert_split_equal(got, want, what=""):
    assert (got["n_records"], got["consumed"], got["ids_bytes"]) == (want["n_records"], want["consumed"], want["ids_bytes"]), what
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
    assert got["ids"] == want["ids"], what


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def records(n, seed, lo=1, hi=40):
    """n records as lists of four lines (without their line ends)"""
    r = random.Random(seed)
    out = []
    for i in range(n):
        length = r.randint(lo, hi)
        out.append([b"@r%d/%d" % (i, length), bytes(r.choice(b"ACGTN") for _ in range(length)), b"+" if i % 3 else b"+r%d" % i,
                    bytes(r.choice(b"FFFF:,#@+") for _ in range(length))])
    return out


def join(recs, eol=b"\n"):
    return b"".join(line + (eol(i, k) if callable(eol) else eol) for i, rec in enumerate(recs) for k, line in enumerate(rec))


BAD_KINDS = ("blank_line", "wrapped", "empty_read", "plus_missing", "qual_short", "qual_long", "at_missing")


def damage(rec, kind):
    """record `rec` (four lines) damaged; a list of lines"""
    ident, seq, plus, qual = rec
    if kind == "blank_line":
        return [b"", ident, seq, plus, qual]
    if kind == "wrapped":
        seq = seq + b"ACGT"
        return [ident, seq[:len(seq) // 2], seq[len(seq) // 2:], plus, qual + b"FFFF"]
    if kind == "empty_read":
        return [ident, b"", plus, b""]
    if kind == "plus_missing":
        return [ident, seq, plus[1:], qual]
    if kind == "qual_short":
        return [ident, seq + b"A", plus, qual]
    if kind == "qual_long":
        return [ident, seq, plus, qual + b"F"]
    assert kind == "at_missing"
    return [ident[1:], seq, plus, qual]


def mutate_lines(r, lines):
    """one line-level mutation of a list of lines (each with its line end)"""
    lines = list(lines)
    i = r.randrange(len(lines))
    kind = r.randrange(12)
    if kind == 0:
        lines[i] = lines[i].rstrip(b"\r\n")                           # a line feed dropped: two lines become one
    elif kind == 1:
        at = r.randrange(len(lines[i]) + 1)
        lines[i] = lines[i][:at] + b"\n" + lines[i][at:]             # a line feed inserted
    elif kind == 2:
        lines.insert(i, lines[i])                                     # a line twice
    elif kind == 3:
        del lines[i]
    elif kind == 4:
        lines.insert(i, r.choice([b"\n", b"\r\n"]))                   # a blank line
    elif kind == 5:
        lines[i] = lines[i].rstrip(b"\r\n") + r.choice([b"\r\n", b"\r\r\n", b"\n"])
    elif kind == 6:
        lines[i] = r.choice([b"@", b"+", b"\r"]) + lines[i]
    elif kind == 7:
        lines[i] = lines[i][1:]                                       # the first byte dropped ('@', '+' or a letter)
    elif kind == 8:
        at = r.randrange(len(lines[i]) + 1)
        lines[i] = lines[i][:at] + r.choice([b"\r", b"@", b"+"]) + lines[i][at:]
    elif kind == 9 and lines[i].startswith(b"@"):
        lines[i] = b"@" + lines[i][len(lines[i].rstrip(b"\r\n")):]    # an empty id
    elif kind == 10:
        lines[i] = lines[i].replace(b"\r", b"")
    else:
        lines = lines[:i] + [lines[i][:r.randrange(len(lines[i]) + 1)]]  # the file cut inside line i
    return lines


@functools.lru_cache(maxsize=None)
def sweep_cases():
    """2 400 texts: a file of twelve short records, line ends mixed, with one to three line-level mutations"""
    r = random.Random(4242)
    out = []
    for c in range(2400):
        recs = records(12, 1000 + c % 7, 1, 24)
        lines = [line + (b"\r\n" if (c % 3 == 1 or (c % 3 == 2 and r.random() < 0.5)) else b"\n") for rec in recs for line in rec]
        for _ in range(r.randint(1, 3)):
            if lines:
                lines = mutate_lines(r, lines)
        out.append(b"".join(lines))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    """list of (name, text, start, max_records); max_records None: as many as the text can hold"""
    cases = []
    for n, seed in ((3000, 1), (65280, 2), (200000, 3)):  # (cut inside a record: the last one is not taken)
        cases.append(("fastq_text_%d" % n, ic.fastq_text(n, seed), 0, None))
    whole = ic.fastq_text(30000, 4)
    whole = whole[:whole.rindex(b"\n@") + 1]
    cases.append(("fastq_text_whole_records", whole, 0, None))
    recs = records(70, 5)
    plain = join(recs)
    count = len(recs)
    cases.append(("crlf", join(recs, b"\r\n"), 0, None))
    cases.append(("empty_id", join([[b"@"] + rec[1:] if i % 2 else rec for i, rec in enumerate(recs)]), 0, None))
    cases.append(("empty_id_crlf", join([[b"@"] + rec[1:] for rec in recs], b"\r\n"), 0, None))
    cases.append(("mixed_line_ends", join(recs, lambda i, k: b"\r\n" if (4 * i + k) % 2 else b"\n"), 0, None))
    cases.append(("mixed_line_ends_by_record", join(recs, lambda i, k: b"\r\n" if i % 2 else b"\n"), 0, None))
    for at in (10, 33):
        cases.append(("start_at_record_%d" % at, plain, len(join(recs[:at])), None))
    cases.append(("start_inside_a_record", plain, len(join(recs[:10])) + 3, None))
    cases.append(("start_at_the_end", plain, len(plain), None))
    for m in (count, count - 1, 0, 1, count + 5):
        cases.append(("max_records_%d" % m, plain, 0, m))
    for kind in BAD_KINDS:
        for at in (0, 1, 63, 64, 65, count - 1):
            lines = [rec if i != at else damage(rec, kind) for i, rec in enumerate(recs)]
            cases.append(("%s_at_%d" % (kind, at), join(lines), 0, None))
    cases.append(("last_line_without_line_feed", plain[:-1], 0, None))
    cases.append(("last_line_without_line_feed_crlf", join(recs, b"\r\n")[:-1], 0, None))
    tiny = b"@\nA\n+\nI\n" * 4
    for n in (0, 1, 15, 16, 17):
        cases.append(("text_bytes_%d" % n, tiny[:n], 0, None))
        cases.append(("text_bytes_%d_of_a_file" % n, plain[:n], 0, None))
    cases.append(("only_line_feeds", b"\n" * 5000, 0, None))
    cases.append(("only_line_feeds_few_records", b"\n" * 5000, 0, 2))
    cases.append(("no_line_feed_at_all", b"@" + b"A" * 4999, 0, None))
    cases += [("sweep_%d" % i, t, 0, None) for i, t in enumerate(sweep_cases())]
    return cases


def expected_bad_index(name):
    for kind in BAD_KINDS:
        if name.startswith(kind + "_at_"):
            return int(name[len(kind) + 4:])
    return None


@pytest.fixture(scope="module")
def api():
    import charon_amd.api as api
    return api


# ---- the tests -----------------------------------------------------------------------------------------------------------------------
def test_the_case_list_is_what_it_says():
    """properties of the cases that the yardstick alone shows: where the damaged records stop the run, that the sweep is a mix"""
    cases = all_cases()
    assert len(cases) > 2400 and len(sweep_cases()) >= 2000
    by_name = {c[0]: c for c in cases}
    for name, text, start, m in cases:
        at = expected_bad_index(name)
        if at is not None:
            assert py_split(text)["n_records"] == at, name
    assert py_split(by_name["crlf"][1])["n_records"] == 70 and py_split(by_name["mixed_line_ends"][1])["n_records"] == 70
    assert py_split(by_name["empty_id_crlf"][1])["ids_bytes"] == 0
    assert py_split(by_name["last_line_without_line_feed"][1])["n_records"] == 69
    assert py_split(by_name["only_line_feeds"][1])["n_records"] == 0
    assert py_split(by_name["text_bytes_16"][1])["n_records"] == 2 and py_split(by_name["text_bytes_17"][1])["consumed"] == 16
    assert py_split(by_name["start_inside_a_record"][1], by_name["start_inside_a_record"][2])["n_records"] == 0
    taken = [py_split(t)["n_records"] for t in sweep_cases()]
    assert len(set(taken)) >= 12 and taken.count(0) < len(taken) // 2


def test_host_split_equals_the_python_rule_on_every_case(api):
    for name, text, start, m in all_cases():
        want = py_split(text, start, m)
        assert_split_equal(api.text_split_host(text, start=start, max_records=m), want, name)
        # without the ids nothing else changes, and ids_bytes is still reported
        got = api.text_split_host(text, start=start, max_records=m, want_ids=False)
        assert got["ids"] is None
        assert_split_equal(dict(got, ids=want["ids"]), want, name)


def test_text_bytes_shorter_than_the_buffer(api):
    """text_bytes ends the text, not the buffer: what lies behind is never looked at"""
    text = join(records(20, 9))
    for cut in (0, 1, len(text) // 2, len(text) - 1):
        assert_split_equal(api.text_split_host(text, nbytes=cut), py_split(text, end=cut), cut)


def split_job(api, text, **over):
    buf = np.frombuffer(text, np.uint8)
    j, a = api.text_split_job(buf.ctypes.data, len(text))
    for k, v in over.items():
        setattr(j, k, v)
    return j, a, buf


def test_refusals_of_the_host_call(api):
    L = api.lib()
    text = join(records(5, 3))
    err = lambda: L.chn_last_error().decode()
    j, a, buf = split_job(api, text)
    assert L.chn_text_split_host(ctypes.byref(j)) == 0 and j.n_records == 5
    for over, what in ((dict(struct_size=ctypes.sizeof(api.TextSplitJob) - 8), "struct_size"), (dict(flags=1), "flag"), (dict(flags=0x80000000), "flag"),
                       (dict(start=len(text) + 1), "start"), (dict(id_offset=None), "NULL"), (dict(id_length=None), "NULL"),
                       (dict(seq_offset=None), "NULL"), (dict(seq_length=None), "NULL"), (dict(qual_offset=None), "NULL")):
        j, a, buf = split_job(api, text, **over)
        assert L.chn_text_split_host(ctypes.byref(j)) == -1 and what in err(), (over, err())
    # ... a NULL descriptor array is fine where there is no room for a record anyway
    j, a, buf = split_job(api, text, max_records=0, id_offset=None, seq_length=None)
    assert L.chn_text_split_host(ctypes.byref(j)) == 0 and (j.n_records, j.consumed) == (0, 0)
    # capacity: the text (checked before a byte of it is read), the ids
    j, a, buf = split_job(api, text, text_bytes=api.TEXT_SPLIT_MAX_BYTES + 1)
    assert L.chn_text_split_host(ctypes.byref(j)) == -5 and "CHN_TEXT_SPLIT_MAX_BYTES" in err()
    need = py_split(text)["ids_bytes"]
    j, a, buf = split_job(api, text, ids_capacity=need - 1)
    assert L.chn_text_split_host(ctypes.byref(j)) == -5 and ("need %d bytes" % need) in err(), err()
    j, a, buf = split_job(api, text, ids_capacity=need)
    assert L.chn_text_split_host(ctypes.byref(j)) == 0 and j.ids_bytes == need
    assert L.chn_text_split_host(None) == -1


def test_inflate_run_host_refuses_device_output(api):
    good, _, _ = ic.member_set()
    ms, sizes = [good[2][1]], [good[2][2]]
    for crc in (False, True):
        j, a = api.inflate_job(ms, sizes)
        j.flags = api.INFLATE_OUT_DEVICE
        if crc:
            c, ca = api.inflate_crc(1, want_crc=True)
            rc = api.lib().chn_inflate_run_host_crc(ctypes.byref(j), ctypes.byref(c))
        else:
            rc = api.lib().chn_inflate_run_host(ctypes.byref(j))
        assert rc == -1 and "CHN_INFLATE_OUT_DEVICE" in api.lib().chn_last_error().decode()
        assert (a["out"] == 0xA5).all() and (a["status"] == 0xFFFFFFFF).all()
        j.flags = 2  # any other bit: unknown
        assert api.lib().chn_inflate_run_host(ctypes.byref(j)) == -1 and "unknown flag" in api.lib().chn_last_error().decode()
    res, st = api.inflate_host(ms, sizes)
    assert not st.any() and res == [b"A"]
