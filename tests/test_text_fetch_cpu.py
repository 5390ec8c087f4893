"""CPU tests of chn_text_fetch_host: byte ranges of a text gathered back to back by the copy rule that chn_text_fetch runs on the
device (charon_amd/csrc/parts/text_gather.inc), and the refusals of the call that need no device.

The yardstick is Python slicing (py_fetch); it never calls into the library.  The case list (all_cases) is what
tests/test_gpu_text_fetch.py runs through k_text_gather as well."""
import ctypes
import functools

import numpy as np
import pytest

SRC_OFFSETS = tuple(range(18))
LENGTHS = (0, 1, 3, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097)


def py_fetch(text, offsets, lengths):
    """the yardstick: range i is text[offsets[i] : offsets[i] + lengths[i]], the ranges back to back"""
    text = bytes(text)
    return b"".join(text[int(o):int(o) + int(n)] for o, n in zip(offsets, lengths))


@functools.lru_cache(maxsize=None)
def the_text(nbytes=4097 + 17 + 5, seed=77):
    """random bytes; the size is no multiple of 16, so that a range which ends at text_bytes ends inside a 16-byte piece"""
    assert nbytes % 16 != 0
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def all_cases():
    """(name, text, offsets, lengths): every source offset 0 .. 17 crossed with every length of LENGTHS -- one job per range, and all
    of them in one job behind a first range of d = 0 .. 15 bytes, which gives every range every misalignment of the destination --,
    overlapping and repeated ranges, no range at all, ranges that end at text_bytes"""
    t = the_text()
    n = len(t)
    grid = [(o, l) for o in SRC_OFFSETS for l in LENGTHS]
    cases = [("offset_%d_length_%d" % (o, l), t, (o,), (l,)) for o, l in grid]
    for d in range(16):
        cases.append(("grid_behind_%d_bytes" % d, t, (5,) + tuple(o for o, _ in grid), (d,) + tuple(l for _, l in grid)))
    cases.append(("overlapping", t, (0, 10, 20, 5, 0, 100, 90), (100, 100, 100, 200, n, 33, 33)))
    cases.append(("repeated", t, (7, 7, 7, 300, 300, 7), (50, 50, 50, 1, 1, 50)))
    cases.append(("no_ranges", t, (), ()))
    cases.append(("only_empty_ranges", t, (0, 9, n), (0, 0, 0)))
    cases.append(("empty_text", b"", (0, 0), (0, 0)))
    for l in (1, 2, 15, 16, 17, 40, n):
        cases.append(("last_%d_bytes" % l, t, (n - l,), (l,)))
    cases.append(("ends_at_text_bytes_twice", t, (n - 21, 3, n - 1, n - 16), (21, 9, 1, 16)))
    short = t[:23]  # a text shorter than two pieces
    cases.append(("short_text", short, (0, 22, 1, 16, 7), (23, 1, 22, 7, 16)))
    return tuple(cases)


def test_the_cases_are_what_the_issue_lists():
    names = {c[0] for c in all_cases()}
    assert len(names) == len(all_cases())
    assert {"offset_%d_length_%d" % (o, l) for o in range(18) for l in (0, 1, 3, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097)} <= names
    assert len(the_text()) % 16 != 0 and {"overlapping", "repeated", "no_ranges", "last_17_bytes"} <= names
    for name, text, offs, lens in all_cases():
        assert all(o + l <= len(text) for o, l in zip(offs, lens)), name


@pytest.mark.parametrize("shift", [0, 1, 5])
def test_fetch_host_equals_slicing(shift):
    """every case, with the text at three alignments in host memory (the host call takes any) and `out` between guard bytes"""
    from charon_amd import api
    for name, text, offs, lens in all_cases():
        want = py_fetch(text, offs, lens)
        hold = np.zeros(len(text) + 16, np.uint8)
        hold[shift:shift + len(text)] = np.frombuffer(text, np.uint8)
        out = np.full(len(want) + 64, 0xA5, np.uint8)
        got = api.text_fetch_host(hold[shift:shift + len(text)], offs, lens, out=out[32:32 + len(want)])
        assert got.tobytes() == want, name
        assert (out[:32] == 0xA5).all() and (out[32 + len(want):] == 0xA5).all(), name


def test_fetch_host_out_bytes_and_spare_capacity():
    from charon_amd import api
    t = the_text()
    out = np.full(100, 0xA5, np.uint8)
    j, keep = api.text_fetch_job(np.frombuffer(t, np.uint8).ctypes.data, len(t), (3, 40), (10, 20), out=out)
    j.out_bytes = 12345
    assert api.lib().chn_text_fetch_host(ctypes.byref(j)) == 0
    assert j.out_bytes == 30 and out[:30].tobytes() == t[3:13] + t[40:60] and (out[30:] == 0xA5).all()


def test_fetch_host_refusals():
    """every refusal of the issue that needs no device: struct_size, a flag, a range behind text_bytes, too little room"""
    from charon_amd import api
    L = api.lib()
    t = np.frombuffer(the_text(), np.uint8)
    n = t.size

    def call(offs, lens, capacity=None, **over):
        out = np.full(256, 0xA5, np.uint8)
        j, keep = api.text_fetch_job(t.ctypes.data, n, offs, lens, out=out, out_capacity=capacity)
        for k, v in over.items():
            setattr(j, k, v)
        rc = L.chn_text_fetch_host(ctypes.byref(j))
        assert rc == 0 or (out == 0xA5).all()  # a refused job writes nothing
        return rc, L.chn_last_error().decode()

    rc, err = call((0,), (4,), struct_size=8)
    assert rc == -1 and "struct_size" in err
    rc, err = call((0,), (4,), flags=1)
    assert rc == -1 and "flag" in err
    for offs, lens, i in (((0, n - 3), (4, 4), 1), ((n + 1,), (0,), 0), ((2 ** 64 - 2, 0), (4, 1), 0), ((0, 0, n), (1, 1, 1), 2)):
        rc, err = call(offs, lens)
        assert rc == -1 and ("range %d " % i) in err and "text_bytes" in err, err
    rc, err = call((0, 50), (100, 100), capacity=199)
    assert rc == -5 and "need 200 bytes" in err, err
    rc, err = call((0,), (4,), offset=None)
    assert rc == -1 and "NULL" in err
    rc, err = call((0, n), (4, 0))  # ... and the same job shapes are taken when they are right
    assert rc == 0
    with pytest.raises(api.ChnError, match="error -5"):
        api.text_fetch_host(the_text(), (0,), (10,), out_capacity=9)


def test_fetch_symbols_are_declared_and_exported():
    from charon_amd import api
    for name in ("chn_text_fetch", "chn_text_fetch_host", "chn_device_copy"):
        assert name in api.EXPORTS and getattr(api.lib(), name) is not None
