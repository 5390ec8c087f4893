"""GPU tests (-m gpu) of chn_fasta_split: FASTA records found and unwrapped in device memory.

Yardsticks, none of which is the kernels: the CPU twin chn_fasta_split_host (pinned to a sequential Python rule by
tests/test_fasta_split_cpu.py, whose whole case list runs here too) and that Python rule itself for the placed texts; the host-text
path of the same batch for every result column bitwise, and the oracle for parity.  The shapes are the smallest at which the kernels
can go wrong: features on either side of a 16-byte piece, a 1 KiB round, a 4 KiB tile and `start`; lines longer than a tile; texts of
more tiles than one round of the scans takes."""
import ctypes
import re

import numpy as np
import pytest

from tests import test_fasta_split_cpu as fsc
from tests import util
from tests.test_gpu_parity import run_oracle
from tests.test_gpu_text_batch import api, good_quals, world  # noqa: F401 (fixtures)
from tests.test_gpu_text_chain import DeviceText

pytestmark = pytest.mark.gpu

GUARD = 64


class GuardedSeq:
    """the device buffer the letters go to, between two stretches of GUARD bytes of 0xA5; everything is 0xA5 before every call"""

    def __init__(self, api, capacity):
        self.api, self.capacity = api, (int(capacity) + 15) & ~15
        self.buf = DeviceText(api, self.capacity + 2 * GUARD, fill=0xA5)
        self.ptr = self.buf.ptr + GUARD

    def check_and_reset(self, seq_bytes, capacity, what):
        """the letters; the guard in front, and everything from seq_bytes rounded up to 16 on, must still be 0xA5"""
        used = (seq_bytes + 15) & ~15
        got = self.buf.get(GUARD + max(used, capacity) + GUARD)
        assert (got[:GUARD] == 0xA5).all(), what
        assert (got[GUARD + used:] == 0xA5).all(), what
        if used:
            self.api.device_upload(0, self.ptr, np.full(used, 0xA5, np.uint8))
        return got[GUARD:GUARD + seq_bytes].tobytes()

    def free(self):
        self.buf.free()


def device_split(stream, text_buf, seq, text, start=0, m=None, eoi=False, what="", **kw):
    """chn_fasta_split of `text` with a seq_text of exactly the capacity the contract asks for; the dict of fasta_split_host"""
    n = text_buf.put(text)
    capacity = (n - start + 15) & ~15
    got = stream.fasta_split(text_buf.ptr, n, seq.ptr, capacity, start=start, max_records=m, end_of_input=eoi, **kw)
    got["seq_text"] = seq.check_and_reset(got["seq_bytes"], capacity, what)
    return got


@pytest.fixture(scope="module")
def stream(api, world):
    st = api.Stream(world["gf"], 4096, 1 << 22, profile=True)
    st.set_model(api.default_model(2, world["gf"].desc.host_index))
    yield st
    st.destroy()


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def placed_cases():
    """texts built so that a header's first byte (which is the end of the record before), its line feed, a '\\r' and a dropped digit fall
    on byte P of the buffer, P on either side of a 16-byte piece, a 1 KiB round and a 4 KiB tile; and texts whose `start` lies there"""
    rest = fsc.join(fsc.fasta_records(9, 31))
    cases = []

    def both(name, text, start=0):
        cases.append((name, text, start, None, False))
        cases.append((name + "_eoi", text, start, None, True))

    for P in (15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097):
        both("header_at_%d" % P, b">a\n" + b"A" * (P - 4) + b"\n" + rest)
        both("header_at_%d_crlf" % P, b">a\r\n" + b"A" * (P - 6) + b"\r\n" + rest)
        both("header_feed_at_%d" % P, b">" + b"i" * (P - 1) + b"\nACGT\n" + rest)
        both("header_cr_at_%d" % P, b">" + b"i" * (P - 1) + b"\r\nACGT\n" + rest)
        both("empty_id_feed_at_%d" % P, b">a\n" + b"A" * (P - 5) + b"\n>\nACGT\n" + rest)
        both("sequence_cr_at_%d" % P, b">a\n" + b"A" * (P - 3) + b"\r\nCC\n" + rest)
        both("digit_at_%d" % P, b">a\n" + b"A" * (P - 3) + b"7CC\n" + rest)
        both("digit_line_at_%d" % P, b">a\nAC\n" + b"\n" * (P - 6) + b"7\n" + rest)
        both("empty_record_ends_at_%d" % P, b">a\nA\n>b\n" + b" " * (P - 8) + b"\n" + rest)
        for S in (P, P + 1):
            for fill_name, fill in (("line_feeds", b"\n" * S), ("letters", (b"ACGT>;\r7" * (S // 8 + 1))[:S]), ("header", b">" + b"h" * (S - 1))):
                both("start_%d_behind_%s" % (S, fill_name), fill + rest, S)
                both("start_%d_behind_%s_empty_id_cr_digit" % (S, fill_name), fill + b">\r\n7A\r\n" + rest, S)
                both("start_%d_behind_%s_no_header" % (S, fill_name), fill + b"A" + rest, S)
    long_header = b">" + (b"id > with ; bytes 0123 that are\ta header's " * 300) + b"\r"
    assert len(long_header) > 2 * 4096 + 100
    both("header_longer_than_two_tiles", b">a\nAC\n" + long_header + b"\nACGT\nAC GT\n" + rest)
    both("header_longer_than_two_tiles_in_front", long_header + b"\nACGT\n" + rest)
    both("sequence_line_over_three_tiles", b">a\nAC\n>b\n" + b"ACGTN" * 2700 + b"\n" + rest)
    both("sequence_line_over_three_tiles_to_the_end", b">a\nAC\n>b\n" + b"ACGTN" * 2700)
    both("digits_over_three_tiles", b">a\nAC\n>b\nA" + b"0123456789 \t" * 1100 + b"C\n" + rest)
    for name, text, start, m, eoi in cases:  # the texts are what their names say
        number = re.search(r"\d+", name)
        P = int(number.group()) if number else 0
        if name.startswith("header_at"):
            assert text[P:P + 1] == b">" and text[P - 1:P] == b"\n", name
        if name.startswith(("header_feed", "empty_id_feed")):
            assert text[P:P + 1] == b"\n" and text[:1] == b">", name
        if name.startswith(("header_cr", "sequence_cr")):
            assert text[P:P + 2] == b"\r\n", name
        if name.startswith(("digit_at", "digit_line")):
            assert text[P:P + 1] == b"7", name
        if name.startswith("empty_record_ends_at"):
            assert text[P:P + 2] == b"\n>" and fsc.py_fasta_split(text, eoi=eoi)["n_records"] == 1, name
        elif name.startswith("start") and "no_header" in name:
            assert fsc.py_fasta_split(text, start, eoi=eoi)["n_records"] == 0, name
        elif not name.startswith(("header_longer", "sequence_line", "digits_over")):
            extra = 0 if name.startswith("start") and "empty_id" not in name else 2 if name.startswith("empty_id") else 1
            assert fsc.py_fasta_split(text, start, eoi=eoi)["n_records"] == 8 + extra + eoi, name
    return cases


def test_split_on_the_device_equals_the_host_twin_on_every_case(api, stream):
    cases = fsc.all_cases() + placed_cases()
    size = max(len(c[1]) for c in cases) + 16
    buf, seq = DeviceText(api, size), GuardedSeq(api, size)
    try:
        for name, text, start, m, eoi in cases:
            want = api.fasta_split_host(text, start=start, max_records=m, end_of_input=eoi)
            fsc.assert_fasta_equal(device_split(stream, buf, seq, text, start, m, eoi, name), want, name)
            if not name.startswith("sweep_"):  # (the CPU suite holds the twin to the Python rule on these already; here once more, directly)
                fsc.assert_fasta_equal(want, fsc.py_fasta_split(text, start, m, eoi=eoi), name)
        # without the ids: everything else alike
        name, text, start, m, eoi = cases[1]
        got = device_split(stream, buf, seq, text, start, m, eoi, name, want_ids=False)
        assert got["ids"] is None
        want = fsc.py_fasta_split(text, start, m, eoi=eoi)
        fsc.assert_fasta_equal(dict(got, ids=want["ids"]), want, name)
    finally:
        buf.free()
        seq.free()


@pytest.mark.parametrize("mib", [1.1, 4.3])
def test_split_texts_of_many_tiles(api, stream, mib):
    """1.1 MiB: more than 256 tiles, every wavefront of the grid loops; 4.3 MiB: more than 1024 tiles, the one-workgroup scans loop.
    A start in the middle, a record bound inside a wavefront, an empty record far in, sizes that are no multiple of 16"""
    n_recs = int(mib * (1 << 20) / 300)
    rng = np.random.default_rng(77)
    lens = rng.integers(1, 601, n_recs)
    lens[-1] += (5 - int(lens.sum())) % 16            # (the letters: 5 more than a multiple of 16)
    pool = np.frombuffer(b"ACGTNacgtn", np.uint8)[rng.integers(0, 10, int(lens.sum()))].tobytes()
    ends = np.cumsum(lens)
    recs = [[b">r%d" % i] + [pool[a:min(a + 60, int(e))] for a in range(int(e - n), int(e), 60)] for i, (e, n) in enumerate(zip(ends, lens))]
    text = fsc.join(recs) + b">tail"
    text += b"x" * ((7 - len(text)) % 16)
    assert len(text) > mib * (1 << 20) and len(text) % 16 == 7
    buf, seq = DeviceText(api, len(text) + 16), GuardedSeq(api, len(text) + 16)
    try:
        want = api.fasta_split_host(text)
        assert want["n_records"] == n_recs and want["seq_bytes"] % 16 == 5 and len(text) // 4096 > (256 if mib < 2 else 1024)
        fsc.assert_fasta_equal(device_split(stream, buf, seq, text, what="all"), want, "all")
        assert want["seq_text"] == b"".join(b"".join(rec[1:]) for rec in recs)
        mid = int(want["id_offset"][n_recs // 3]) - 1
        fsc.assert_fasta_equal(device_split(stream, buf, seq, text, mid, eoi=True, what="start"), api.fasta_split_host(text, start=mid, end_of_input=True), "start")
        for m in (65, n_recs - 1):
            fsc.assert_fasta_equal(device_split(stream, buf, seq, text, m=m, what=m), api.fasta_split_host(text, max_records=m), m)
        at = n_recs - 1001
        broken = fsc.join(recs[:at] + [recs[at][:1] + [b" 12 "]] + recs[at + 1:])
        got = device_split(stream, buf, seq, broken, what="broken")
        assert got["n_records"] == at
        fsc.assert_fasta_equal(got, api.fasta_split_host(broken), "broken")
    finally:
        buf.free()
        seq.free()


def test_profile_slot(api, stream, world):
    text = fsc.join(fsc.fasta_records(50, 3))
    buf, seq = DeviceText(api, len(text) + 16), GuardedSeq(api, len(text) + 16)
    plain = api.Stream(world["gf"], 64, 1 << 16)
    try:
        stream.profile(14, reset=True)
        assert stream.profile(14) == (0.0, 0)
        split_before = stream.profile(8)
        for _ in range(3):
            device_split(stream, buf, seq, text)
        ms, calls = stream.profile(14, reset=True)
        assert calls == 3 and 0.0 < ms < 1000.0
        assert stream.profile(14) == (0.0, 0) and stream.profile(8) == split_before  # chn_text_split's slot is its own
        n = buf.put(text)
        plain.fasta_split(buf.ptr, n, seq.ptr, (n + 15) & ~15)
        assert plain.profile(14) == (0.0, 0)  # no CHN_STREAM_PROFILE: nothing is timed
        seq.check_and_reset(len(text), (n + 15) & ~15, "plain")
        with pytest.raises(api.ChnError):
            stream.profile(15)
    finally:
        plain.destroy()
        buf.free()
        seq.free()


# ---- batches from the unwrapped letters ----------------------------------------------------------------------------------------------
def fasta_text(reads, width=70, eol=b"\n"):
    return b"".join(b">read%d/%d" % (i, len(s)) + eol + b"".join(s[a:a + width] + eol for a in range(0, len(s), width)) for i, s in enumerate(reads))


def test_text_batch_from_the_letters_and_a_split_between_batches_in_flight(api, world):
    """a batch submitted from seq_text (CHN_TEXT_ON_DEVICE) equals the host-text batch of the same letters bitwise and is in parity with
    the oracle; a split between two batches in flight leaves their results as they are"""
    from charon_amd import pack
    r = util.rng(57)
    gs = world["gs"]
    reads = util.sample_reads(r, gs, 300, (30, 1500)) + [util.mutate(r, gs[0][5000:5000 + L], 0.03) for L in (9000, 20000, 69, 70, 71, 140)]
    reads = [s if i % 7 else s[:len(s) // 2] + b"N" * 3 + s[len(s) // 2:] for i, s in enumerate(reads)]
    text = fasta_text(reads, eol=b"\r\n")
    n = len(reads)
    g = world["gf"]
    st = api.Stream(g, n, pack.pack_reads(reads)["n_bases"])
    st.set_model(api.default_model(2, g.desc.host_index, min_quality=0.0))  # (FASTA: the mean quality is 0)
    buf, seq = DeviceText(api, len(text) + 16), GuardedSeq(api, len(text) + 16)
    other = fsc.join(fsc.fasta_records(40, 12))
    obuf, oseq = DeviceText(api, len(other) + 16), GuardedSeq(api, len(other) + 16)
    try:
        nbytes = buf.put(text)
        sp = st.fasta_split(buf.ptr, nbytes, seq.ptr, (nbytes + 15) & ~15, end_of_input=True)
        assert sp["n_records"] == n and sp["consumed"] == len(text)
        assert [int(x) for x in sp["seq_length"]] == [len(s) for s in reads] and sp["seq_bytes"] % 16 != 0
        tb = dict(seq1_offset=sp["seq_offset"], seq1_length=sp["seq_length"])
        comp = np.zeros(n, np.float32)
        st.submit_text(tb, comp, text_device=(seq.ptr, sp["seq_bytes"]))
        got = st.wait_text()
        st.submit_text(dict(tb, text=np.frombuffer(b"".join(reads), np.uint8)), comp)  # the host-text path, same descriptors
        host = st.wait_text()
        util.assert_same_results(got, host)
        for k in ("flags", "has_n", "n_bases"):
            assert np.array_equal(got[k], host[k]), k
        assert not got["mean_quality"].any() and not host["mean_quality"].any()
        util.assert_parity(got, run_oracle(world["fused"], reads))
        assert (got["call"] != 255).sum() > 50
        # two batches in flight, a split of another text between them
        st.submit_text(tb, comp, text_device=(seq.ptr, sp["seq_bytes"]))
        mid = device_split(st, obuf, oseq, other, eoi=True, what="between")
        st.submit_text(tb, comp, text_device=(seq.ptr, sp["seq_bytes"]))
        fsc.assert_fasta_equal(device_split(st, obuf, oseq, other, eoi=True, what="behind"), mid, "behind")
        fsc.assert_fasta_equal(mid, fsc.py_fasta_split(other, eoi=True), "between")
        for _ in range(2):
            again = st.wait_text()
            util.assert_same_results(again, got)
            assert np.array_equal(again["flags"], got["flags"])
    finally:
        st.destroy()
        for b in (buf, seq, obuf, oseq):
            b.free()


def test_refusals_leave_the_stream_usable(api, stream):
    from charon_amd import pack
    L = api.lib()
    text = fsc.join(fsc.fasta_records(50, 3))
    want = fsc.py_fasta_split(text)
    need16 = (len(text) + 15) & ~15
    buf, seq = DeviceText(api, 4 * need16, fill=0xA5), GuardedSeq(api, need16)
    pinned = api.pinned_array(need16, np.uint8)
    pageable = np.frombuffer(text + b"\n" * 16, np.uint8).copy()
    pinned[:len(text)] = np.frombuffer(text, np.uint8)
    try:
        n = buf.put(text)

        def call(ptr, seq_ptr, capacity=need16, **over):
            j, a = api.fasta_split_job(ptr, n, seq_ptr, capacity)
            for k, v in over.items():
                setattr(j, k, v)
            return L.chn_fasta_split(stream.h, ctypes.byref(j)), L.chn_last_error().decode()

        def still_works(what):
            fsc.assert_fasta_equal(device_split(stream, buf, seq, text, what=what), want, what)
            r = util.rng(5)
            reads = [util.random_seq(r, 200) for _ in range(8)]
            stream.submit_text(pack.text_batch(reads, good_quals(r, reads), gap=b"\n"), np.zeros(len(reads), np.float32))
            return stream.wait_text()

        first = still_works("before")
        refusals = [
            # a host pointer: the text, the letters
            (pinned.ctypes.data, seq.ptr, {}, -1, "text is page-locked"), (pageable.ctypes.data, seq.ptr, {}, -1, "text is not device memory"),
            (buf.ptr, pinned.ctypes.data, {}, -1, "seq_text is page-locked"), (buf.ptr, pageable.ctypes.data & ~15, {}, -1, "seq_text is not device memory"),
            # a misaligned pointer, a capacity that is no multiple of 16
            (buf.ptr + 1, seq.ptr, {}, -1, "16-byte aligned"), (buf.ptr, seq.ptr + 8, {}, -1, "16-byte aligned"),
            (buf.ptr, seq.ptr, dict(seq_capacity=need16 + 8), -1, "multiple of 16"),
            # overlapping buffers: the letters in the text's own allocation, over its front, its last piece, the whole of it
            (buf.ptr, buf.ptr, {}, -1, "overlap"), (buf.ptr, buf.ptr + need16 - 16, {}, -1, "overlap"), (buf.ptr + 16, buf.ptr, dict(seq_capacity=3 * need16), -1, "overlap"),
            # a short capacity
            (buf.ptr, seq.ptr, dict(seq_capacity=need16 - 16), -5, "need %d bytes" % need16), (buf.ptr, seq.ptr, dict(seq_capacity=0), -5, "need %d bytes" % need16),
            # and what chn_text_split refuses too
            (buf.ptr, seq.ptr, dict(struct_size=8), -1, "struct_size"), (buf.ptr, seq.ptr, dict(flags=2), -1, "flag"), (buf.ptr, seq.ptr, dict(start=n + 1), -1, "start"),
            (buf.ptr, seq.ptr, dict(seq_offset=None), -1, "NULL"), (buf.ptr, seq.ptr, dict(text_bytes=api.TEXT_SPLIT_MAX_BYTES + 16, seq_capacity=1 << 32), -5, "CHN_TEXT_SPLIT_MAX_BYTES"),
            (buf.ptr, seq.ptr, dict(ids_capacity=want["ids_bytes"] - 1), -5, "need %d bytes" % want["ids_bytes"]),
        ]
        for i, (ptr, seq_ptr, over, code, word) in enumerate(refusals):
            rc, err = call(ptr, seq_ptr, **over)
            assert rc == code and word in err, (i, rc, err)
            if "ids" in word or "ids_capacity" in over:
                seq.check_and_reset(want["seq_bytes"], need16, "ids")  # (the letters were there before the ids turned out not to fit)
            if i % 4 == 3 or i == len(refusals) - 1:
                util.assert_same_results(still_works(word), first)
        assert (buf.get()[need16:] == 0xA5).all()  # no refused call wrote into the text's allocation
        # the letters side by side with the text in one allocation are fine
        j, a = api.fasta_split_job(buf.ptr, n, buf.ptr + need16, need16)
        assert L.chn_fasta_split(stream.h, ctypes.byref(j)) == 0 and j.n_records == want["n_records"]
        assert buf.get()[need16:need16 + want["seq_bytes"]].tobytes() == want["seq_text"]
        # three batches in flight
        r = util.rng(5)
        reads = [util.random_seq(r, 200) for _ in range(8)]
        tb = pack.text_batch(reads, good_quals(r, reads), gap=b"\n")
        for _ in range(3):
            stream.submit_text(tb, np.zeros(len(reads), np.float32))
        rc, err = call(buf.ptr, seq.ptr)
        assert rc == -1 and "three batches" in err
        seq.check_and_reset(0, need16, "three in flight")  # nothing ran
        got = stream.wait_text()
        fsc.assert_fasta_equal(device_split(stream, buf, seq, text, what="two in flight"), want, "two in flight")
        for _ in range(2):
            util.assert_same_results(stream.wait_text(), got)
        util.assert_same_results(got, first)
    finally:
        buf.free()
        seq.free()
        api.host_free(pinned)
