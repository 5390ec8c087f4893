"""CPU tests of chn_fasta_split_host: FASTA records found and unwrapped by the rule source that chn_fasta_split's kernels compile
(charon_amd/csrc/parts/fasta_split.inc), and the refusals of the call that need no device.

The yardstick is py_fasta_split below: a sequential Python restatement of the record rule as include/charon_hip.h spells it out (which
is BlockReader::parse_fasta from a record boundary on).  It never calls into the library.  Every case compares every descriptor array,
n_records, consumed, the ids, ids_bytes, seq_bytes and the unwrapped letters.  The case list (all_cases) is what
tests/test_gpu_fasta_split.py runs through the kernels as well."""
import ctypes
import functools
import os
import random
import re

import numpy as np
import pytest

KEYS = ("id_offset", "id_length", "seq_offset", "seq_length")
DROPPED = b"\n\r \t0123456789"
HEADERS = (b">", b";")


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------
def strip_cr(line):
    return line[:-1] if line.endswith(b"\r") else line


def py_fasta_record(t, p, end, eoi):
    """the record that starts at byte p of t[:end] as (id offset, id length, letters, offset of the next record), or None where the
    rule fails"""
    if p >= end or t[p:p + 1] not in HEADERS:                # its first byte begins a header line
        return None
    feed = t.find(b"\n", p, end)                             # the header's line feed lies in the text
    if feed < 0:
        return None
    q = feed + 1
    while True:                                              # the next header line begins inside the text ...
        if q >= end:
            nxt = end if eoi else None                       # ... or the text ends and that counts
            break
        if t[q:q + 1] in HEADERS:
            nxt = q
            break
        e = t.find(b"\n", q, end)
        if e < 0:
            nxt = end if eoi else None
            break
        q = e + 1
    if nxt is None:
        return None
    letters = t[feed + 1:nxt].translate(None, DROPPED)       # the lines between, without line ends, blanks and digits
    if not letters:                                          # the compacted sequence has length >= 1
        return None
    ident = strip_cr(t[p + 1:feed])                          # the id: behind the first byte up to the line feed, minus one trailing \r
    return p + 1, len(ident), letters, nxt


def py_fasta_split(t, start=0, max_records=None, end=None, eoi=False):
    t = bytes(t)
    end = len(t) if end is None else end
    recs, p, ids, seq = [], start, b"", b""
    while max_records is None or len(recs) < max_records:
        got = py_fasta_record(t, p, end, eoi)
        if got is None:
            break
        recs.append((got[0], got[1], len(seq), len(got[2])))
        ids += t[got[0]:got[0] + got[1]]
        seq += got[2]
        p = got[3]
    out = {k: np.array([r[i] for r in recs], np.uint64 if k.endswith("offset") else np.uint32) for i, k in enumerate(KEYS)}
    out.update(n_records=len(recs), consumed=p, ids=ids, ids_bytes=len(ids), seq_text=seq, seq_bytes=len(seq))
    return out


def assert_fasta_equal(got, want, what=""):
    for k in ("n_records", "consumed", "ids_bytes", "seq_bytes"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
    assert got["ids"] == want["ids"], what
    assert got["seq_text"] == want["seq_text"], what


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def letters(r, n, alphabet=b"ACGTNacgtnRYKM"):
    return bytes(r.choice(alphabet) for _ in range(n))


def fasta_records(n, seed, width=70, lo=1, hi=200):
    """n records as lists of lines (without their line ends): a header line, then the sequence in lines of `width` letters"""
    r = random.Random(seed)
    out = []
    for i in range(n):
        s = letters(r, r.randint(lo, hi))
        out.append([(b";" if i % 5 == 3 else b">") + b"r%d some text/%d" % (i, len(s))] + [s[a:a + width] for a in range(0, len(s), width)])
    return out


def join(recs, eol=b"\n"):
    return b"".join(line + (eol(i, k) if callable(eol) else eol) for i, rec in enumerate(recs) for k, line in enumerate(rec))


def mutate_lines(r, lines):
    """one line-level mutation of a list of lines (each with its line end)"""
    lines = list(lines)
    i = r.randrange(len(lines))
    kind = r.randrange(13)
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
        lines.insert(i, r.choice([b"\n", b"\r\n", b" \n", b"12\n"]))  # a blank line, or one of dropped bytes only
    elif kind == 5:
        lines[i] = lines[i].rstrip(b"\r\n") + r.choice([b"\r\n", b"\r\r\n", b"\n"])
    elif kind == 6:
        lines[i] = r.choice([b">", b";", b"\r", b" ", b"7"]) + lines[i]
    elif kind == 7:
        lines[i] = lines[i][1:]                                       # the first byte dropped ('>' or a letter)
    elif kind == 8:
        at = r.randrange(len(lines[i]) + 1)
        lines[i] = lines[i][:at] + r.choice([b"\r", b">", b";", b" ", b"\t", b"5"]) + lines[i][at:]
    elif kind == 9 and lines[i][:1] in HEADERS:
        lines[i] = lines[i][:1] + lines[i][len(lines[i].rstrip(b"\r\n")):]   # an empty id
    elif kind == 10:
        lines[i] = lines[i].replace(b"\r", b"")
    elif kind == 11 and lines[i][:1] not in HEADERS:
        lines[i] = lines[i].translate(None, b"ACGTNacgtnRYKM")        # a sequence line emptied
    else:
        lines = lines[:i] + [lines[i][:r.randrange(len(lines[i]) + 1)]]  # the file cut inside line i
    return lines


@functools.lru_cache(maxsize=None)
def sweep_cases():
    """3 000 texts: a file of twelve short records in lines of 9 letters, line ends mixed, with one to three line-level mutations"""
    r = random.Random(777)
    out = []
    for c in range(3000):
        recs = fasta_records(12, 2000 + c % 7, 9, 1, 30)
        lines = [line + (b"\r\n" if (c % 3 == 1 or (c % 3 == 2 and r.random() < 0.5)) else b"\n") for rec in recs for line in rec]
        for _ in range(r.randint(1, 3)):
            if lines:
                lines = mutate_lines(r, lines)
        out.append(b"".join(lines))
    return out


EMPTY_AT = (0, 1, 63, 64, 65, 69)


@functools.lru_cache(maxsize=None)
def all_cases():
    """list of (name, text, start, max_records, end_of_input); max_records None: as many as the text can hold"""
    cases = []

    def both(name, text, start=0, m=None):
        cases.append((name, text, start, m, False))
        cases.append((name + "_eoi", text, start, m, True))

    recs = fasta_records(70, 5)
    count = len(recs)
    plain = join(recs)
    both("plain", plain)
    both("crlf", join(recs, b"\r\n"))
    both("mixed_line_ends", join(recs, lambda i, k: b"\r\n" if (3 * i + k) % 2 else b"\n"))
    both("mixed_line_ends_by_record", join(recs, lambda i, k: b"\r\n" if i % 2 else b"\n"))
    both("empty_id", join([[rec[0][:1]] + rec[1:] if i % 2 else rec for i, rec in enumerate(recs)]))
    both("empty_id_crlf", join([[rec[0][:1]] + rec[1:] for rec in recs], b"\r\n"))
    both("id_ends_in_cr", join([[rec[0] + b"\r"] + rec[1:] for rec in recs]))
    both("id_ends_in_two_cr", join([[rec[0] + b"\r"] + rec[1:] for rec in recs], b"\r\n"))
    both("id_is_one_cr", join([[rec[0][:1] + b"\r"] + rec[1:] for rec in recs]))
    both("semicolon_headers", join([[b";" + rec[0][1:]] + rec[1:] for rec in recs]))
    for width in (1, 60, 70, 10000):
        both("lines_of_%d" % width, join(fasta_records(6, 40 + width, width, 9990 if width == 10000 else 100, 20100 if width == 10000 else 400)))
    both("blank_lines_inside", join([rec[:2] + [b"", b"\r"] + rec[2:] + [b""] for rec in recs]))
    r = random.Random(8)
    dirty = lambda s: b"".join(bytes([c]) + r.choice([b"", b"", b" ", b"\t", b"7", b"10 "]) for c in s)
    both("blanks_tabs_digits", join([[rec[0]] + [r.choice([b"", b"  61 "]) + dirty(line) for line in rec[1:]] for rec in recs]))
    both("genbank_style", b">x\n        1 acgtacgtac gtacgtacgt\n       21 acgt\n>y\n 1 a\n")
    both("other_bytes_are_kept", b">x\nAC-GT*.\x00\xff@[\n>y\n~\n")
    for at in EMPTY_AT:
        both("empty_record_at_%d" % at, join([rec if i != at else rec[:1] for i, rec in enumerate(recs)]))
        both("record_of_dropped_bytes_at_%d" % at, join([rec if i != at else rec[:1] + [b" 12\t", b"\r"] for i, rec in enumerate(recs)]))
        for m in (at, at + 1):
            both("max_records_%d" % m, plain, 0, m)
    both("max_records_beyond", plain, 0, count + 5)
    both("leading_blank_line", b"\n" + plain)
    both("leading_blank_line_crlf", b"\r\n" + join(recs, b"\r\n"))
    both("no_header_in_front", plain[1:])
    both("letters_in_front", b"ACGT\n" + plain)
    both("no_header_at_all", b"ACGT\nACGT\n" * 300)
    both("only_headers", b">a\n;b\n>c\n" * 100)
    both("only_line_feeds", b"\n" * 5000)
    both("only_header_bytes", b">" * 5000)
    both("no_line_feed_at_all", b">" + b"A" * 4999)
    both("ends_inside_a_sequence_line", plain[:-3])
    both("ends_inside_a_sequence_line_crlf", join(recs, b"\r\n")[:-1])
    both("ends_inside_a_header_line", plain + b">last id")
    both("ends_with_a_header_byte", plain + b">")
    both("ends_with_a_header_line", plain + b">last id\n")
    both("ends_with_a_header_line_and_dropped_bytes", plain + b">last id\n 12\n")
    lens = np.cumsum([0] + [len(join([rec])) for rec in recs])
    for at in (10, 33):
        both("start_at_record_%d" % at, plain, int(lens[at]))
    both("start_inside_a_header", plain, int(lens[10]) + 3)
    both("start_inside_a_sequence", plain, int(lens[10]) + len(recs[10][0]) + 3)
    both("start_at_the_end", plain, len(plain))
    for s in range(18):
        both("start_%d" % s, b"\n" * s + plain, s)
        both("start_%d_after_letters" % s, (b"ACGT" * 5)[:s] + plain, s)
    tiny = b">\nA\n" * 8
    for n in (0, 1, 2, 3, 4, 15, 16, 17):
        both("text_bytes_%d" % n, tiny[:n])
        both("text_bytes_%d_of_a_file" % n, plain[:n])
    cases.extend(("sweep_%d" % i, t, 0, None, bool(i & 1)) for i, t in enumerate(sweep_cases()))
    return cases


@pytest.fixture(scope="module")
def api():
    import charon_amd.api as api
    return api


# ---- the tests -----------------------------------------------------------------------------------------------------------------------
def test_the_case_list_is_what_it_says():
    """properties of the cases that the yardstick alone shows"""
    cases = all_cases()
    assert len(cases) > 3000 and len(sweep_cases()) >= 3000
    d = {c[0]: c for c in cases}
    n = lambda name: py_fasta_split(d[name][1], d[name][2], d[name][3], eoi=d[name][4])
    assert n("plain")["n_records"] == 69 and n("plain_eoi")["n_records"] == 70 and n("plain_eoi")["consumed"] == len(d["plain"][1])
    for name in ("crlf", "mixed_line_ends", "empty_id", "id_ends_in_cr", "semicolon_headers", "blank_lines_inside", "blanks_tabs_digits"):
        assert n(name + "_eoi")["n_records"] == 70, name
        assert n(name + "_eoi")["seq_text"] == n("plain_eoi")["seq_text"], name
    assert n("empty_id_crlf_eoi")["ids_bytes"] == 0 and n("id_is_one_cr_eoi")["ids_bytes"] == 0
    assert n("id_ends_in_cr_eoi")["ids"] == n("plain_eoi")["ids"]
    assert n("id_ends_in_two_cr_eoi")["ids_bytes"] == n("plain_eoi")["ids_bytes"] + 70  # one \r is dropped, the other is the id's
    assert n("genbank_style_eoi")["seq_text"] == b"acgtacgtacgtacgtacgtacgta"
    assert n("other_bytes_are_kept_eoi")["seq_text"] == b"AC-GT*.\x00\xff@[~"
    assert max(n("lines_of_10000_eoi")["seq_length"]) > 10000  # (wrapped even at that width)
    for at in EMPTY_AT:
        assert n("empty_record_at_%d_eoi" % at)["n_records"] == at and n("record_of_dropped_bytes_at_%d" % at)["n_records"] == at
        assert n("max_records_%d" % at)["n_records"] == at
    for name in ("leading_blank_line", "no_header_in_front", "letters_in_front", "no_header_at_all", "only_headers", "only_line_feeds", "start_inside_a_header"):
        assert n(name + "_eoi")["n_records"] == 0 and n(name + "_eoi")["consumed"] == d[name][2], name
    assert n("ends_inside_a_sequence_line")["n_records"] == 69 and n("ends_inside_a_sequence_line_eoi")["n_records"] == 70
    assert n("ends_inside_a_header_line")["n_records"] == 70 and n("ends_inside_a_header_line_eoi")["n_records"] == 70
    assert n("ends_inside_a_header_line_eoi")["consumed"] == len(d["plain"][1])
    assert n("ends_with_a_header_line_eoi")["n_records"] == 70 and n("ends_with_a_header_line_and_dropped_bytes_eoi")["n_records"] == 70
    assert n("text_bytes_3_eoi")["n_records"] == 1 and n("text_bytes_3")["n_records"] == 0 and n("text_bytes_16")["n_records"] == 3
    for s in range(18):
        assert n("start_%d_eoi" % s)["n_records"] == 70 and n("start_%d_after_letters_eoi" % s)["n_records"] == 70
    taken = [py_fasta_split(t, eoi=e)["n_records"] for name, t, _, _, e in cases if name.startswith("sweep_")]
    assert len(set(taken)) >= 12 and taken.count(0) < len(taken) // 2


def test_host_split_equals_the_python_rule_on_every_case(api):
    for name, text, start, m, eoi in all_cases():
        want = py_fasta_split(text, start, m, eoi=eoi)
        got = api.fasta_split_host(text, start=start, max_records=m, end_of_input=eoi)
        assert_fasta_equal(got, want, name)
        assert got["seq_tail_untouched"], name
    # without the ids nothing else changes, and ids_bytes is still reported
    for name, text, start, m, eoi in all_cases()[:40]:
        want = py_fasta_split(text, start, m, eoi=eoi)
        got = api.fasta_split_host(text, start=start, max_records=m, end_of_input=eoi, want_ids=False)
        assert got["ids"] is None
        assert_fasta_equal(dict(got, ids=want["ids"]), want, name)


def test_text_bytes_shorter_than_the_buffer(api):
    """text_bytes ends the text, not the buffer: what lies behind is never looked at"""
    text = join(fasta_records(20, 9))
    for cut in (0, 1, len(text) // 2, len(text) - 1):
        for eoi in (False, True):
            assert_fasta_equal(api.fasta_split_host(text, nbytes=cut, end_of_input=eoi), py_fasta_split(text, end=cut, eoi=eoi), cut)


def split_job(api, text, seq, **over):
    buf = np.frombuffer(text, np.uint8)
    j, a = api.fasta_split_job(buf.ctypes.data, len(text), seq.ctypes.data, seq.size)
    for k, v in over.items():
        setattr(j, k, v)
    return j, a, buf


def test_refusals_of_the_host_call(api):
    L = api.lib()
    text = join(fasta_records(5, 3))
    need16 = (len(text) + 15) & ~15
    seq = np.zeros(need16, np.uint8)
    err = lambda: L.chn_last_error().decode()
    j, a, buf = split_job(api, text, seq)
    assert L.chn_fasta_split_host(ctypes.byref(j)) == 0 and j.n_records == 4
    j, a, buf = split_job(api, text, seq, flags=api.FASTA_SPLIT_END_OF_INPUT)
    assert L.chn_fasta_split_host(ctypes.byref(j)) == 0 and (j.n_records, j.consumed) == (5, len(text))
    for over, what in ((dict(struct_size=ctypes.sizeof(api.FastaSplitJob) - 8), "struct_size"), (dict(flags=2), "flag"), (dict(flags=0x80000001), "flag"),
                       (dict(start=len(text) + 1), "start"), (dict(id_offset=None), "NULL"), (dict(id_length=None), "NULL"),
                       (dict(seq_offset=None), "NULL"), (dict(seq_length=None), "NULL"), (dict(seq_text=None), "seq_text is NULL")):
        j, a, buf = split_job(api, text, seq, **over)
        assert L.chn_fasta_split_host(ctypes.byref(j)) == -1 and what in err(), (over, err())
    # ... a NULL descriptor array is fine where there is no room for a record anyway
    j, a, buf = split_job(api, text, seq, max_records=0, id_offset=None, seq_length=None)
    assert L.chn_fasta_split_host(ctypes.byref(j)) == 0 and (j.n_records, j.consumed, j.seq_bytes) == (0, 0, 0)
    # overlap: seq_text inside the text, the text inside seq_text, seq_text ending in the text's last piece
    both = np.zeros(4 * need16, np.uint8)
    both[:len(text)] = np.frombuffer(text, np.uint8)
    for at in (0, 16, need16 - 16):
        j, a = api.fasta_split_job(both.ctypes.data, len(text), both.ctypes.data + at, need16)
        assert L.chn_fasta_split_host(ctypes.byref(j)) == -1 and "overlap" in err(), at
    j, a = api.fasta_split_job(both.ctypes.data + 16, len(text) - 16, both.ctypes.data, 4 * need16)
    assert L.chn_fasta_split_host(ctypes.byref(j)) == -1 and "overlap" in err()
    j, a = api.fasta_split_job(both.ctypes.data, len(text), both.ctypes.data + need16, need16)  # side by side is fine
    assert L.chn_fasta_split_host(ctypes.byref(j)) == 0 and j.n_records == 4
    # capacity: the text (checked before a byte of it is read), the letters, the ids
    j, a, buf = split_job(api, text, seq, text_bytes=api.TEXT_SPLIT_MAX_BYTES + 1, seq_capacity=1 << 32)
    assert L.chn_fasta_split_host(ctypes.byref(j)) == -5 and "CHN_TEXT_SPLIT_MAX_BYTES" in err()
    j, a, buf = split_job(api, text, seq, seq_capacity=need16 - 16)
    assert L.chn_fasta_split_host(ctypes.byref(j)) == -5 and ("need %d bytes" % need16) in err(), err()
    j, a, buf = split_job(api, text, seq, start=32, seq_capacity=need16 - 32)  # the bytes behind `start` count
    assert L.chn_fasta_split_host(ctypes.byref(j)) == 0
    need = py_fasta_split(text)["ids_bytes"]
    j, a, buf = split_job(api, text, seq, ids_capacity=need - 1)
    assert L.chn_fasta_split_host(ctypes.byref(j)) == -5 and ("need %d bytes" % need) in err(), err()
    j, a, buf = split_job(api, text, seq, ids_capacity=need)
    assert L.chn_fasta_split_host(ctypes.byref(j)) == 0 and j.ids_bytes == need
    assert L.chn_fasta_split_host(None) == -1
    # chn_text_split's contract is untouched: any flag is refused there
    tj, ta = api.text_split_job(buf.ctypes.data, len(text))
    tj.flags = api.FASTA_SPLIT_END_OF_INPUT
    assert L.chn_text_split_host(ctypes.byref(tj)) == -1 and "flag" in err()


def test_both_symbols_are_declared_and_exported(api):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "charon_hip.h")).read()
    assert re.search(r"^int chn_fasta_split\(chn_stream \*s, chn_fasta_split_job \*job\);", header, re.M)
    assert re.search(r"^int chn_fasta_split_host\(chn_fasta_split_job \*job\);", header, re.M)
    assert "#define CHN_FASTA_SPLIT_END_OF_INPUT 1u" in header and "} chn_fasta_split_job;" in header
    for name in ("chn_fasta_split", "chn_fasta_split_host"):
        assert name in api.EXPORTS and hasattr(api.lib(), name)
    # the struct of the bindings is the header's: eighteen fields, no padding
    assert ctypes.sizeof(api.FastaSplitJob) == 2 * 4 + 16 * 8
