"""GPU tests (-m gpu) of chn_text_fetch -- k_text_gather: byte ranges of a text in device memory gathered into host memory -- and
of chn_device_copy.

Yardsticks, none of which is the new kernel: Python slicing (tests/test_text_fetch_cpu.py) for the bytes, the CPU twin on top, the
oracle for the parity of the batches a stream classifies after a refusal, an undisturbed run of the same batches for the ones in
flight around a fetch.  The shapes are the smallest at which the kernel can go wrong: every source offset against every
misalignment of the destination, lengths around one, four and 256 pieces, one range beyond a wavefront's single pass of 64 pieces,
more ranges than the looping grid has wavefronts."""
import ctypes

import numpy as np
import pytest

from tests import test_text_fetch_cpu as tfc
from tests import util
from tests.test_gpu_parity import run_oracle
from tests.test_gpu_text_batch import api, good_quals, world  # noqa: F401 (fixtures)
from tests.test_gpu_text_chain import DeviceText

pytestmark = pytest.mark.gpu

GUARD = 48  # 0xA5 bytes on either side of `out`, more than a stray 16-byte store reaches; `out` itself starts at GUARD + shift


@pytest.fixture(scope="module")
def stream(api, world):
    st = api.Stream(world["gf"], 4096, 1 << 22, profile=True)
    st.set_model(api.default_model(2, world["gf"].desc.host_index))
    yield st
    st.destroy()


@pytest.fixture(scope="module")
def outs(api):
    """a pageable and a page-locked array to fetch into"""
    size = 1 << 22
    pinned = api.pinned_array(size, np.uint8)
    yield {"pageable": np.zeros(size, np.uint8), "page-locked": pinned}
    api.host_free(pinned)


def fetch_guarded(stream, hold, shift, dev, nbytes, offs, lens, want_len):
    """fetch into hold[GUARD + shift : + want_len], everything around it 0xA5; returns the bytes and whether the rest is untouched"""
    hold[:GUARD + shift + want_len + GUARD] = 0xA5
    out = hold[GUARD + shift:GUARD + shift + want_len]
    got = stream.text_fetch(dev, nbytes, offs, lens, out=out)
    around = (hold[:GUARD + shift] == 0xA5).all() and (hold[GUARD + shift + want_len:GUARD + shift + want_len + GUARD] == 0xA5).all()
    return got.tobytes(), bool(around)


@pytest.mark.parametrize("kind", ["pageable", "page-locked"])
def test_fetch_on_the_device_equals_slicing_and_the_host_twin(api, stream, outs, kind):
    cases = tfc.all_cases()
    buf = DeviceText(api, max(len(c[1]) for c in cases) + 16)
    try:
        uploaded = None
        for k, (name, text, offs, lens) in enumerate(cases):
            if text is not uploaded:
                n = buf.put(text, pad=b"\xEE")
                uploaded = text
            want = tfc.py_fetch(text, offs, lens)
            got, around = fetch_guarded(stream, outs[kind], k % 3, buf.ptr, n, offs, lens, len(want))
            assert got == want, name
            assert around, name
            assert api.text_fetch_host(text, offs, lens).tobytes() == got, name
    finally:
        buf.free()


def test_one_long_range(api, stream, outs):
    """70 000 bytes: 4 375 pieces, 69 passes of a wavefront; a source that is aligned, and one that is not"""
    text = np.random.default_rng(3).integers(0, 256, 70000 + 40, dtype=np.uint8).tobytes()
    buf = DeviceText(api, len(text) + 16)
    try:
        n = buf.put(text)
        for off in (0, 16, 13, 39):
            for lead in (0, 5):  # bytes of a first range in front: the long one's destination aligned and not
                offs, lens = (1, off), (lead, 70000)
                want = tfc.py_fetch(text, offs, lens)
                got, around = fetch_guarded(stream, outs["pageable"], 0, buf.ptr, n, offs, lens, len(want))
                assert got == want and around, (off, lead)
    finally:
        buf.free()


@pytest.mark.parametrize("count", (5000, 10000))
def test_many_short_ranges(api, stream, outs, count):
    """5 000 and 10 000 ranges of 1 .. 300 bytes: more than the looping grid has wavefronts (16 per compute unit, 4 096 on 256 of them)"""
    r = np.random.default_rng(4)
    text = r.integers(0, 256, 200003, dtype=np.uint8).tobytes()
    lens = r.integers(1, 301, count)
    offs = r.integers(0, len(text) - 300, count)
    offs[-1], lens[-1] = len(text) - 300, 300  # the last one ends at text_bytes
    buf = DeviceText(api, len(text) + 16)
    try:
        n = buf.put(text, pad=b"\xEE")
        want = tfc.py_fetch(text, offs, lens)
        for kind in ("pageable", "page-locked"):
            got, around = fetch_guarded(stream, outs[kind], 1, buf.ptr, n, offs, lens, len(want))
            assert got == want and around, kind
        assert api.text_fetch_host(text, offs, lens).tobytes() == want
    finally:
        buf.free()


def small_batch(api, world, seed=5):
    from charon_amd import pack
    r = util.rng(seed)
    reads = util.sample_reads(r, world["gs"], 24, (150, 400))
    return pack.text_batch(reads, good_quals(r, reads), gap=b"\n"), run_oracle(world["fused"], reads)


def test_refusals_leave_the_stream_usable(api, world, stream):
    L = api.lib()
    text = tfc.the_text()
    buf = DeviceText(api, len(text) + 64)
    pinned = api.pinned_array(len(text) + 16, np.uint8)
    pageable = np.frombuffer(text + b"\n" * 16, np.uint8).copy()
    pinned[:len(text)] = np.frombuffer(text, np.uint8)
    tb, oracle = small_batch(api, world)
    try:
        n = buf.put(text)

        def refused(ptr, offs=(3, 100), lens=(40, 40), capacity=None, **over):
            out = np.full(256, 0xA5, np.uint8)
            j, keep = api.text_fetch_job(ptr, n, offs, lens, out=out, out_capacity=capacity)
            for k, v in over.items():
                setattr(j, k, v)
            rc, err = L.chn_text_fetch(stream.h, ctypes.byref(j)), L.chn_last_error().decode()
            assert (out == 0xA5).all()  # nothing was written
            stream.submit_text(tb)      # ... and the stream classifies a batch as ever
            util.assert_parity(stream.wait_text(), oracle)
            return rc, err

        for ptr, word in ((pinned.ctypes.data, "page-locked"), (pageable.ctypes.data, "not device memory"), (buf.ptr + 1, "16-byte aligned")):
            rc, err = refused(ptr)
            assert rc == -1 and word in err, err
        for over, word in ((dict(struct_size=8), "struct_size"), (dict(flags=1), "flag")):
            rc, err = refused(buf.ptr, **over)
            assert rc == -1 and word in err, err
        rc, err = refused(buf.ptr, offs=(3, n - 39))
        assert rc == -1 and "range 1 " in err and "text_bytes" in err, err
        rc, err = refused(buf.ptr, capacity=79)
        assert rc == -5 and "need 80 bytes" in err, err
        assert stream.text_fetch(buf.ptr, n, (3, 100), (40, 40)).tobytes() == text[3:43] + text[100:140]
    finally:
        buf.free()
        api.host_free(pinned)


def test_fetch_between_batches_in_flight(api, world, stream):
    L = api.lib()
    text = tfc.the_text()
    buf = DeviceText(api, len(text) + 16)
    tbs = [small_batch(api, world, seed)[0] for seed in (6, 7)]
    try:
        n = buf.put(text)
        alone = []
        for tb in tbs:  # the run without the fetch
            stream.submit_text(tb)
            alone.append(stream.wait_text())
        for tb in tbs:
            stream.submit_text(tb)
        offs, lens = (1, 17, 4000), (4097, 33, 100)
        assert stream.text_fetch(buf.ptr, n, offs, lens).tobytes() == tfc.py_fetch(text, offs, lens)
        stream.submit_text(tbs[0])  # a third: now the call is refused, and nothing else changes
        j, keep = api.text_fetch_job(buf.ptr, n, offs, lens)
        assert L.chn_text_fetch(stream.h, ctypes.byref(j)) == -1 and "three batches" in L.chn_last_error().decode()
        for want in alone + alone[:1]:
            got = stream.wait_text()
            util.assert_same_results(got, want)
            for k in ("flags", "has_n", "n_bases"):
                assert np.array_equal(got[k], want[k]), k
            assert np.array_equal(got["mean_quality"].view(np.uint32), want["mean_quality"].view(np.uint32))
    finally:
        buf.free()


def test_profile_counts_the_calls(api, world, stream):
    text = tfc.the_text()
    buf = DeviceText(api, len(text) + 16)
    plain = api.Stream(world["gf"], 64, 1 << 16)
    try:
        n = buf.put(text)
        stream.profile(9, reset=True)
        assert stream.profile(9) == (0.0, 0)
        for k in range(5):
            stream.text_fetch(buf.ptr, n, (k, 100), (4000, 17))
        ms, calls = stream.profile(9, reset=True)
        assert calls == 5 and 0.0 < ms < 1000.0
        assert stream.profile(9) == (0.0, 0)
        plain.text_fetch(buf.ptr, n, (0,), (64,))  # a stream without CHN_STREAM_PROFILE times nothing
        assert plain.profile(9) == (0.0, 0)
        with pytest.raises(api.ChnError):
            stream.profile(10)
    finally:
        plain.destroy()
        buf.free()


def test_device_copy(api):
    data = np.random.default_rng(8).integers(0, 256, 5000, dtype=np.uint8)
    a, b = DeviceText(api, 5008), DeviceText(api, 5008, fill=0xA5)
    host = np.zeros(64, np.uint8)
    pinned = api.pinned_array(64, np.uint8)
    try:
        a.put(data)
        api.device_copy(0, b.ptr + 7, a.ptr + 3, 4990)  # any alignment
        got = b.get()
        assert np.array_equal(got[7:4997], data[3:4993]) and (got[:7] == 0xA5).all() and (got[4997:] == 0xA5).all()
        api.device_copy(0, b.ptr, a.ptr, 0)
        api.device_copy(0, a.ptr + 2500, a.ptr, 2500)  # two stretches of one allocation
        assert np.array_equal(a.get()[2500:5000], data[:2500])
        for dst, src, word in ((b.ptr, host.ctypes.data, "source"), (host.ctypes.data, a.ptr, "destination"), (b.ptr, pinned.ctypes.data, "page-locked"),
                               (a.ptr + 100, a.ptr, "overlap")):
            with pytest.raises(api.ChnError, match="error -1:.*chn_device_copy.*" + word):
                api.device_copy(0, dst, src, 64 if word != "overlap" else 200)
        assert np.array_equal(b.get()[7:4997], data[3:4993])
    finally:
        a.free()
        b.free()
        api.host_free(pinned)
