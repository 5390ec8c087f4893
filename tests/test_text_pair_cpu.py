"""CPU tests of chn_text_pair_ids_host: do the ids of the two mates of every pair agree, by the rule source that chn_text_pair_ids
runs on the device (charon_amd/csrc/parts/text_pair.inc), and the refusals of the call that need no device.

The yardstick is a Python restatement of the rule (py_agree); it never calls into the library.  The call returns the FIRST
disagreeing pair only, so every pair of a case is pinned by walking on behind each mismatch (mismatches_of): the list of all
disagreeing indices must equal the yardstick's.  The case list (all_cases) is what tests/test_gpu_text_pair.py runs through
k_pair_ids as well."""
import ctypes
import functools

import numpy as np
import pytest

ID_LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 255, 5000)
OFFSETS = tuple(range(18))
KINDS = ("dropped_byte_only", "first_byte", "last_compared_byte", "one_longer", "equal")


def py_agree(a, b):
    """the yardstick: both ids lose their last byte, what is left must be equal"""
    a, b = bytes(a), bytes(b)
    return a[:max(len(a) - 1, 0)] == b[:max(len(b) - 1, 0)]


def variant(r, a, kind):
    """the id of mate 2 for the id `a` of mate 1"""
    b = bytearray(a)
    flip = lambda i: b.__setitem__(i, b[i] ^ (1 << int(r.integers(0, 8))))
    if kind == "dropped_byte_only" and len(b) >= 1:
        flip(len(b) - 1)
    elif kind == "first_byte" and len(b) >= 2:
        flip(0)
    elif kind == "last_compared_byte" and len(b) >= 2:
        flip(len(b) - 2)
    elif kind == "one_longer":
        b.append(int(r.integers(0, 256)))
    return bytes(b)


class Side:
    """one text under construction: ids placed `o` bytes behind a multiple of 32, random bytes in between"""

    def __init__(self, r):
        self.r, self.parts, self.size, self.off, self.len = r, [], 0, [], []

    def add(self, id_bytes, o):
        fill = (-self.size) % 32 + o
        self.parts.append(self.r.integers(0, 256, fill, dtype=np.uint8).tobytes())
        self.size += fill
        self.off.append(self.size)
        self.len.append(len(id_bytes))
        self.parts.append(id_bytes)
        self.size += len(id_bytes)

    def text(self):
        return b"".join(self.parts)


def make_case(name, r, pairs, end_exact=False):
    """pairs: (id1, id2, o1, o2); the case as (name, text1, text2, off1, len1, off2, len2, expected list of disagreeing pairs)"""
    s1, s2 = Side(r), Side(r)
    for a, b, o1, o2 in pairs:
        s1.add(a, o1)
        s2.add(b, o2)
    for s in (s1, s2):
        if not end_exact:  # bytes behind the last id, to a size that is no multiple of 16
            s.parts.append(s.r.integers(0, 256, 16 + (1 if s.size % 16 == 0 else 0), dtype=np.uint8).tobytes())
            s.size += len(s.parts[-1])
    want = [i for i, (a, b, _, _) in enumerate(pairs) if not py_agree(a, b)]
    return (name, s1.text(), s2.text(), tuple(s1.off), tuple(s1.len), tuple(s2.off), tuple(s2.len), want)


@functools.lru_cache(maxsize=None)
def all_cases():
    r = np.random.default_rng(1331)
    rid = lambda n: r.integers(0, 256, n, dtype=np.uint8).tobytes()
    cases = []
    # every id length at every offset 0 .. 17 of either side, independently; the difference kinds take turns, so every kind meets
    # every length at some 65 offset combinations (and the short lengths, where a kind cannot apply, yield equal ids)
    k = 0
    for L in ID_LENGTHS:
        pairs = []
        for o1 in OFFSETS:
            for o2 in OFFSETS:
                a = rid(L)
                pairs.append((a, variant(r, a, KINDS[k % len(KINDS)]), o1, o2))
                k += 1
        cases.append(make_case("length_%d" % L, r, pairs))
    # every kind at every length, named, one pair per job
    for L in ID_LENGTHS:
        for kind in KINDS:
            a = rid(L)
            cases.append(make_case("%s_length_%d" % (kind, L), r, [(a, variant(r, a, kind), (L + 3) % 18, (L * 7 + 11) % 18)]))
    cases.append(make_case("empty_against_one_byte", r, [(b"", b"x", 3, 9), (b"y", b"", 0, 17), (b"", b"", 5, 5), (b"a", b"b", 7, 7), (b"ab", b"cb", 1, 2)]))
    cases.append(make_case("empty_against_two_bytes", r, [(b"", b"xy", 3, 9), (b"xy", b"", 4, 4)]))
    # where the first mismatch lies among 200 pairs of ids of 1 .. 80 bytes: around a wavefront's 64 lanes, first and last
    base = [(rid(int(n)), int(o1), int(o2)) for n, o1, o2 in zip(r.integers(1, 81, 200), r.integers(0, 18, 200), r.integers(0, 18, 200))]
    same = [(a, a[:-1] + b"2", o1, o2) for a, o1, o2 in base]
    cases.append(make_case("200_pairs_all_agree", r, same))
    for bad in ((0,), (1,), (63,), (64,), (65,), (199,), (70, 130), (130, 64, 199)):
        pairs = list(same)
        for i in bad:
            a = pairs[i][0] if len(pairs[i][0]) >= 2 else rid(9)
            pairs[i] = (a, variant(r, a, "last_compared_byte"), pairs[i][2], pairs[i][3])
        cases.append(make_case("200_pairs_mismatch_at_" + "_".join(map(str, bad)), r, pairs))
    cases.append(make_case("no_pairs", r, []))
    # ids that end at a text_bytes that is no multiple of 16 (the sizes: 32 j + o + L)
    for L in (1, 2, 5, 17, 33):
        for kind in ("dropped_byte_only", "last_compared_byte"):
            a = rid(L)
            cases.append(make_case("ends_at_text_bytes_%s_%d" % (kind, L), r, [(rid(20), rid(20), 0, 0), (a, variant(r, a, kind), 2, 6)], end_exact=True))
    return tuple(cases)


def mismatches_of(first_mismatch, off1, len1, off2, len2):
    """every disagreeing pair, from a call that names the first one only: first_mismatch(off1, len1, off2, len2) over the tail behind
    each mismatch"""
    out, at, n = [], 0, len(off1)
    while True:
        m = first_mismatch(off1[at:], len1[at:], off2[at:], len2[at:])
        assert 0 <= m <= n - at
        if m == n - at:
            return out
        out.append(at + m)
        at += m + 1


def test_the_cases_are_what_the_issue_lists():
    cases = all_cases()
    names = {c[0] for c in cases}
    assert len(names) == len(cases)
    assert {"length_%d" % L for L in (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 255, 5000)} <= names
    by_name = {c[0]: c for c in cases}
    for L in ID_LENGTHS:
        _, t1, t2, o1, l1, o2, l2, want = by_name["length_%d" % L]
        assert {(a % 32, b % 32) for a, b in zip(o1, o2)} == {(a, b) for a in range(18) for b in range(18)}
        assert set(l1) == {L} and set(l2) <= {L, L + 1}
    for L in (2, 5000):
        assert by_name["first_byte_length_%d" % L][7] == [0] and by_name["last_compared_byte_length_%d" % L][7] == [0]
        assert by_name["dropped_byte_only_length_%d" % L][7] == [] and by_name["one_longer_length_%d" % L][7] == [0]
    assert by_name["one_longer_length_0"][7] == [] and by_name["empty_against_one_byte"][7] == [4]
    assert by_name["empty_against_two_bytes"][7] == [0, 1]
    for bad in ("0", "1", "63", "64", "65", "199"):
        assert by_name["200_pairs_mismatch_at_" + bad][7] == [int(bad)]
    assert by_name["200_pairs_mismatch_at_70_130"][7] == [70, 130] and by_name["no_pairs"][3] == ()
    for name, t1, t2, o1, l1, o2, l2, want in cases:
        assert all(o + l <= len(t1) for o, l in zip(o1, l1)) and all(o + l <= len(t2) for o, l in zip(o2, l2)), name
        assert len(t1) % 16 and len(t2) % 16, name
        if name.startswith("ends_at_text_bytes"):
            assert o1[-1] + l1[-1] == len(t1) and o2[-1] + l2[-1] == len(t2), name
    assert py_agree(b"", b"") and py_agree(b"", b"x") and py_agree(b"ab/1", b"ab/2") and not py_agree(b"ab/1", b"ac/1") and not py_agree(b"ab", b"a")


@pytest.mark.parametrize("shift", [0, 1, 5])
def test_pair_ids_host_equals_the_python_rule(shift):
    """every case, with the texts at three alignments in host memory (the host call takes any)"""
    from charon_amd import api
    for name, t1, t2, o1, l1, o2, l2, want in all_cases():
        hold = [np.zeros(len(t) + 16, np.uint8) for t in (t1, t2)]
        views = []
        for h, t, sh in zip(hold, (t1, t2), (shift, 5 - shift)):
            h[sh:sh + len(t)] = np.frombuffer(t, np.uint8)
            views.append(h[sh:sh + len(t)])
        got = mismatches_of(lambda *ids: api.pair_ids_host(views[0], views[1], *ids), o1, l1, o2, l2)
        assert got == want, name
        assert api.pair_ids_host(views[0], views[1], o1, l1, o2, l2) == (want[0] if want else len(o1)), name


def test_pair_ids_host_on_one_text_and_no_pairs():
    from charon_amd import api
    t = b"@read7/1\nACGT\n@read7/2\nACGT\n@read8/1\n"
    assert api.pair_ids_host(t, t, (1, 1), (7, 7), (15, 29), (7, 7)) == 1  # read7/1 ~ read7/2, read7/1 !~ read8/1
    assert api.pair_ids_host(t, t, (), (), (), ()) == 0
    assert api.pair_ids_host(b"", b"", (), (), (), ()) == 0
    assert api.pair_ids_host(b"", b"", (0,), (0,), (0,), (0,)) == 1  # two empty ids agree


def test_pair_ids_host_refusals():
    """every refusal that needs no device: struct_size, a flag, a NULL id array, an id behind text1_bytes / text2_bytes"""
    from charon_amd import api
    L = api.lib()
    t1, t2 = np.frombuffer(b"0123456789" * 10, np.uint8), np.frombuffer(b"0123456789" * 7, np.uint8)

    def call(o1=(0, 10), l1=(5, 5), o2=(0, 10), l2=(5, 5), **over):
        j, keep = api.text_pair_job(t1.ctypes.data, t1.size, t2.ctypes.data, t2.size, o1, l1, o2, l2)
        for k, v in over.items():
            setattr(j, k, v)
        return L.chn_text_pair_ids_host(ctypes.byref(j)), L.chn_last_error().decode(), int(j.first_mismatch)

    rc, err, _ = call(struct_size=8)
    assert rc == -1 and "struct_size" in err
    rc, err, _ = call(flags=1)
    assert rc == -1 and "flag" in err
    for n in (api.TEXT_PAIR_MAX_PAIRS + 1, 2 ** 64 - 1):  # refused before any of the (two-element) arrays is walked
        rc, err, _ = call(n_pairs=n)
        assert rc == -1 and "CHN_TEXT_PAIR_MAX_PAIRS" in err, err
    for k in ("id1_offset", "id1_length", "id2_offset", "id2_length"):
        rc, err, _ = call(**{k: None})
        assert rc == -1 and "NULL" in err, k
    for k in ("text1", "text2"):
        rc, err, _ = call(**{k: None})
        assert rc == -1 and k + " is NULL" in err, k
    for kw, words in ((dict(o1=(0, 96)), ("id 1 of pair 1 ", "text1_bytes 100")), (dict(o2=(66, 0)), ("id 2 of pair 0 ", "text2_bytes 70")),
                      (dict(o1=(101, 0), l1=(0, 5)), ("id 1 of pair 0 ", "text1_bytes")), (dict(o2=(0, 2 ** 64 - 2)), ("id 2 of pair 1 ", "text2_bytes")),
                      (dict(l2=(5, 2 ** 32 - 1)), ("id 2 of pair 1 ", "text2_bytes")), (dict(o1=(0, 96), o2=(66, 0)), ("id 2 of pair 0 ",))):
        rc, err, _ = call(**kw)
        assert rc == -1 and all(w in err for w in words), err
    rc, err, first = call(o1=(0, 95), o2=(65, 0))  # ... and ids that end at the last byte are taken
    assert (rc, first) == (0, 0)
    rc, err, first = call()
    assert (rc, first) == (0, 2)
    rc, err, first = call(n_pairs=0, id1_offset=None, id1_length=None, id2_offset=None, id2_length=None)
    assert (rc, first) == (0, 0)
    with pytest.raises(api.ChnError, match="error -1:.*chn_text_pair_ids_host.*id 1 of pair 0"):
        api.pair_ids_host(t1, t2, (99,), (2,), (0,), (2,))


def test_struct_layouts_match_the_header():
    import os
    import re
    from charon_amd import api
    from tests import util
    # chn_text_batch2: the 112 bytes of chn_text_batch, then text2 (8) and text2_bytes (8)
    assert ctypes.sizeof(api.TextBatch) == 112 and ctypes.sizeof(api.TextBatch2) == 128
    assert api.TextBatch2.text2.offset == 112 and api.TextBatch2.text2_bytes.offset == 120
    for name, _ in api.TextBatch._fields_:
        assert getattr(api.TextBatch2, name).offset == getattr(api.TextBatch, name).offset, name
    # chn_text_pair_job: 2 x uint32 (8) + 2 x (pointer + uint64) (32) + n_pairs (8) + 4 pointers (32) + first_mismatch (8)
    assert ctypes.sizeof(api.TextPairJob) == 88 and api.TextPairJob.n_pairs.offset == 40 and api.TextPairJob.first_mismatch.offset == 80
    header = open(os.path.join(util.ROOT, "include", "charon_hip.h")).read()
    fields = lambda cname: re.findall(r"\*?\s*\b([a-z_0-9]+)[;,]", re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1),
                                                                            flags=re.S))
    assert fields("chn_text_pair_job") == [f[0] for f in api.TextPairJob._fields_]
    assert fields("chn_text_batch2") == ["batch", "text2", "text2_bytes"]


def test_pair_symbols_are_declared_and_exported():
    from charon_amd import api
    for name in ("chn_text_pair_ids", "chn_text_pair_ids_host"):
        assert name in api.EXPORTS and getattr(api.lib(), name) is not None
