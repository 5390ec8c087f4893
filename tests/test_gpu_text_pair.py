"""GPU tests (-m gpu) of chn_text_pair_ids -- k_pair_ids: do the ids of the two mates of every pair agree, over two texts in device
memory -- and of text batches whose two mates lie in two device texts (chn_text_batch2).

Yardsticks, none of which is the new code: the Python rule of tests/test_text_pair_cpu.py (and the CPU twin on top) for the ids,
pack.pack_reads and numpy for the packed form, the one-text run of the same bytes for every result column bitwise, the oracle for
parity, an undisturbed run of the same batches for the ones in flight around a check.  The shapes are the smallest at which the
kernels can go wrong: every id length around one, two and 16 pieces at every offset of either side, mismatches around a
wavefront's 64 lanes, more pairs than one round of the looping grid's first workgroups, mates of every length around a lane's 16
bases and a segment's 64 at every misalignment in either text."""
import ctypes

import numpy as np
import pytest

from tests import test_text_pair_cpu as tpc
from tests import util
from tests.test_gpu_parity import run_oracle
from tests.test_gpu_text_batch import api, assert_packed_like_numpy, good_quals, random_quals, world  # noqa: F401 (fixtures)
from tests.test_gpu_text_chain import DeviceText, assert_same_packed

pytestmark = pytest.mark.gpu

MATE_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 150, 151, 5000)


@pytest.fixture(scope="module")
def stream(api, world):
    st = api.Stream(world["gf"], 4096, 1 << 22, profile=True)
    st.set_model(api.default_model(2, world["gf"].desc.host_index))
    yield st
    st.destroy()


class TwoTexts:
    """two device buffers under the device text contract; what lies behind a text up to the next multiple of 16 differs between them"""

    def __init__(self, api, nbytes):
        self.a, self.b = DeviceText(api, nbytes + 16), DeviceText(api, nbytes + 16)

    def put(self, t1, t2):
        return self.a.ptr, self.a.put(t1, pad=b"\xEE"), self.b.ptr, self.b.put(t2, pad=b"\x11")

    def free(self):
        self.a.free()
        self.b.free()


# ---- 1. the pair-id check ---------------------------------------------------------------------------------------------------------------
def test_pair_ids_on_the_device_equal_the_host_twin_and_the_python_rule(api, stream):
    cases = tpc.all_cases()
    bufs = TwoTexts(api, max(max(len(c[1]), len(c[2])) for c in cases))
    try:
        for name, t1, t2, o1, l1, o2, l2, want in cases:
            p1, n1, p2, n2 = bufs.put(t1, t2)
            got = tpc.mismatches_of(lambda *ids: stream.pair_ids(p1, n1, p2, n2, *ids), o1, l1, o2, l2)
            host = tpc.mismatches_of(lambda *ids: api.pair_ids_host(t1, t2, *ids), o1, l1, o2, l2)
            assert got == host == want, name
    finally:
        bufs.free()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_5000_pairs(api, stream, seed):
    """more pairs than the lanes of 16 workgroups; ids of 1 .. 80 bytes as they lie in two FASTQ files whose records differ in size"""
    r = np.random.default_rng(seed)
    n = 5000
    s1, s2 = tpc.Side(r), tpc.Side(r)
    ids = [r.integers(33, 127, int(L), dtype=np.uint8).tobytes() for L in r.integers(1, 81, n)]
    for a, o1, o2 in zip(ids, r.integers(0, 18, n), r.integers(0, 18, n)):
        s1.add(a, int(o1))
        s2.add(a[:-1] + b"2", int(o2))
    t1, t2 = bytearray(s1.text() + b"\n"), bytearray(s2.text() + b"\n\n\n")
    bufs = TwoTexts(api, max(len(t1), len(t2)))
    try:
        args = (s1.off, s1.len, s2.off, s2.len)
        p1, n1, p2, n2 = bufs.put(t1, t2)
        assert stream.pair_ids(p1, n1, p2, n2, *args) == n == api.pair_ids_host(t1, t2, *args)
        bad = int(r.integers(0, n))
        while s2.len[bad] < 2:
            bad = (bad + 1) % n
        t2[s2.off[bad] + int(r.integers(0, s2.len[bad] - 1))] ^= 0x04
        p1, n1, p2, n2 = bufs.put(t1, t2)
        assert stream.pair_ids(p1, n1, p2, n2, *args) == bad == api.pair_ids_host(t1, t2, *args)
        assert stream.pair_ids(p1, n1, p2, n2, *[a[bad + 1:] for a in args]) == n - bad - 1
    finally:
        bufs.free()


def test_one_very_long_id(api, stream):
    """an id of 70 001 bytes beside short ones: the lane simply loops"""
    r = np.random.default_rng(9)
    a = r.integers(0, 256, 70001, dtype=np.uint8).tobytes()
    t1 = b"abc/1" + a + b"x"
    bufs = TwoTexts(api, len(t1) + 8)
    try:
        for flip, want in ((None, 2), (3 + 69999, 1), (3 + 70000, 2), (3 + 40000, 1)):
            t2 = bytearray(b"xyzabc/2" + a)
            if flip is not None:
                t2[5 + flip] ^= 0x80
            p1, n1, p2, n2 = bufs.put(t1, bytes(t2))
            assert stream.pair_ids(p1, n1, p2, n2, (0, 5), (5, 70001), (3, 8), (5, 70001)) == want == api.pair_ids_host(t1, bytes(t2), (0, 5), (5, 70001), (3, 8), (5, 70001))
    finally:
        bufs.free()


def small_batch(api, world, seed=5):
    from charon_amd import pack
    r = util.rng(seed)
    reads = util.sample_reads(r, world["gs"], 24, (150, 400))
    return pack.text_batch(reads, good_quals(r, reads), gap=b"\n"), run_oracle(world["fused"], reads)


def test_pair_refusals_leave_the_stream_usable(api, world, stream):
    L = api.lib()
    _, t1, t2, o1, l1, o2, l2, want = next(c for c in tpc.all_cases() if c[0] == "200_pairs_mismatch_at_70_130")
    bufs = TwoTexts(api, max(len(t1), len(t2)))
    pinned = api.pinned_array(len(t1) + 16, np.uint8)
    pageable = np.frombuffer(t1 + b"\n" * 16, np.uint8).copy()
    pinned[:len(t1)] = np.frombuffer(t1, np.uint8)
    tb, oracle = small_batch(api, world)
    try:
        p1, n1, p2, n2 = bufs.put(t1, t2)

        def refused(a=p1, b=p2, o1=o1, l1=l1, o2=o2, l2=l2, **over):
            j, keep = api.text_pair_job(a, n1, b, n2, o1, l1, o2, l2)
            for k, v in over.items():
                setattr(j, k, v)
            rc, err = L.chn_text_pair_ids(stream.h, ctypes.byref(j)), L.chn_last_error().decode()
            stream.submit_text(tb)  # ... and the stream classifies a batch as ever
            util.assert_parity(stream.wait_text(), oracle)
            return rc, err

        for ptr, word in ((pinned.ctypes.data, "page-locked"), (pageable.ctypes.data, "not device memory"), (p1 + 1, "16-byte aligned")):
            rc, err = refused(a=ptr)
            assert rc == -1 and "text1" in err and word in err, err
        for ptr, word in ((pinned.ctypes.data, "page-locked"), (pageable.ctypes.data, "not device memory"), (p2 + 8, "16-byte aligned")):
            rc, err = refused(b=ptr)
            assert rc == -1 and "text2" in err and word in err, err
        for over, word in ((dict(struct_size=8), "struct_size"), (dict(flags=1), "flag"), (dict(id2_length=None), "NULL"),
                           (dict(n_pairs=api.TEXT_PAIR_MAX_PAIRS + 1), "CHN_TEXT_PAIR_MAX_PAIRS")):
            rc, err = refused(**over)
            assert rc == -1 and word in err, err
        rc, err = refused(o1=o1[:7] + (n1 - l1[7] + 1,) + o1[8:])
        assert rc == -1 and "id 1 of pair 7 " in err and "text1_bytes" in err, err
        rc, err = refused(l2=l2[:199] + (n2 + 1,))
        assert rc == -1 and "id 2 of pair 199 " in err and "text2_bytes" in err, err
        assert stream.pair_ids(p1, n1, p2, n2, o1, l1, o2, l2) == 70
    finally:
        bufs.free()
        api.host_free(pinned)


def test_pair_check_between_batches_in_flight(api, world, stream):
    L = api.lib()
    _, t1, t2, o1, l1, o2, l2, want = next(c for c in tpc.all_cases() if c[0] == "200_pairs_mismatch_at_65")
    bufs = TwoTexts(api, max(len(t1), len(t2)))
    tbs = [small_batch(api, world, seed)[0] for seed in (6, 7)]
    try:
        p1, n1, p2, n2 = bufs.put(t1, t2)
        alone = []
        for tb in tbs:  # the run without the check
            stream.submit_text(tb)
            alone.append(stream.wait_text())
        for tb in tbs:
            stream.submit_text(tb)
        assert stream.pair_ids(p1, n1, p2, n2, o1, l1, o2, l2) == 65
        stream.submit_text(tbs[0])  # a third: now the call is refused, and nothing else changes
        j, keep = api.text_pair_job(p1, n1, p2, n2, o1, l1, o2, l2)
        assert L.chn_text_pair_ids(stream.h, ctypes.byref(j)) == -1 and "three batches" in L.chn_last_error().decode()
        for want_res in alone + alone[:1]:
            got = stream.wait_text()
            util.assert_same_results(got, want_res)
            for k in ("flags", "has_n", "n_bases"):
                assert np.array_equal(got[k], want_res[k]), k
            assert np.array_equal(got["mean_quality"].view(np.uint32), want_res["mean_quality"].view(np.uint32))
    finally:
        bufs.free()


def test_pair_profile_slot(api, world, stream):
    _, t1, t2, o1, l1, o2, l2, want = next(c for c in tpc.all_cases() if c[0] == "200_pairs_all_agree")
    bufs = TwoTexts(api, max(len(t1), len(t2)))
    plain = api.Stream(world["gf"], 64, 1 << 16)
    try:
        p1, n1, p2, n2 = bufs.put(t1, t2)
        stream.profile(11, reset=True)
        assert stream.profile(11) == (0.0, 0)
        for k in range(5):
            assert stream.pair_ids(p1, n1, p2, n2, o1[k:], l1[k:], o2[k:], l2[k:]) == 200 - k
        assert stream.pair_ids(p1, n1, p2, n2, (), (), (), ()) == 0  # no pairs: no kernel, not counted
        ms, calls = stream.profile(11, reset=True)
        assert calls == 5 and 0.0 < ms < 1000.0
        assert stream.profile(11) == (0.0, 0)
        assert plain.pair_ids(p1, n1, p2, n2, o1, l1, o2, l2) == 200  # a stream without CHN_STREAM_PROFILE times nothing
        assert plain.profile(11) == (0.0, 0)
        for which in (10, 12):
            with pytest.raises(api.ChnError):
                stream.profile(which)
    finally:
        plain.destroy()
        bufs.free()


# ---- 2. text batches over two device texts ----------------------------------------------------------------------------------------------
def lay_out(strings_by_read, misalign):
    """the strings of every read (e.g. sequence and quality) one after another in one text, string k of read i starting
    misalign(i, k) bytes behind a multiple of 32, 'X' -- no nucleotide letter -- in between.  -> (text, offsets[k][i], lengths[k][i])"""
    parts, size = [], 0
    m = len(strings_by_read[0])
    offs, lens = [[] for _ in range(m)], [[] for _ in range(m)]
    for i, strings in enumerate(strings_by_read):
        for k, s in enumerate(strings):
            fill = (-size) % 32 + misalign(i, k)
            parts.append(b"X" * fill)
            size += fill
            offs[k].append(size)
            lens[k].append(len(s))
            parts.append(s)
            size += len(s)
    parts.append(b"X" * (5 if (size + 5) % 16 else 6))
    return b"".join(parts), [np.array(o, np.uint64) for o in offs], [np.array(n, np.uint32) for n in lens]


def two_text_batch(seqs, quals, mates, mquals):
    """the batch as two texts (mate 1 in the first, mate 2 in the second, every misalignment 0 .. 17 in each, independently) and the
    same bytes as one text -- text 1, then text 2 from the next multiple of 16 on -- with the offsets of mate 2 rebased"""
    t1, o1, l1 = lay_out(list(zip(seqs, quals)), lambda i, k: (i + 7 * k) % 18)
    t2, o2, l2 = lay_out(list(zip(mates, mquals)), lambda i, k: (5 * i + 11 * k + 3) % 18)
    two = dict(flags=0, text=None, seq1_offset=o1[0], seq1_length=l1[0], qual1_offset=o1[1], qual1_length=l1[1], seq2_offset=o2[0], seq2_length=l2[0],
               qual2_offset=o2[1], qual2_length=l2[1])
    base = (len(t1) + 15) & ~15
    one_text = t1 + b"X" * (base - len(t1)) + t2
    one = dict(two, seq2_offset=o2[0] + np.uint64(base), qual2_offset=o2[1] + np.uint64(base))
    return t1, t2, two, one_text, one


def mate_cross(r, world, n_in_mate2):
    """mates of every length of MATE_LENGTHS on either side (all but the read without any letter), sampled from the genomes;
    n_in_mate2: three letters to put into every third mate 2, or None"""
    seqs, mates = [], []
    for a in MATE_LENGTHS:
        for b in MATE_LENGTHS:
            if a or b:
                seqs.append(util.sample_reads(r, world["gs"], 1, a)[0] if a else b"")
                mates.append(util.sample_reads(r, world["gs"], 1, b)[0] if b else b"")
    if n_in_mate2:
        for i in range(0, len(mates), 3):
            if len(mates[i]) >= 15:
                m = bytearray(mates[i])
                at = int(r.integers(0, len(m) - 3))
                m[at:at + 3] = n_in_mate2
                mates[i] = bytes(m)
    quals, mquals = good_quals(r, seqs), good_quals(r, mates)
    i = next(k for k, (s, m) in enumerate(zip(seqs, mates)) if len(s) == 150 and len(m) == 64)
    mquals[i] = random_quals(r, 64 + 37, 33 + 25, 33 + 60)  # a quality string longer than its sequence, on mate 2
    return seqs, quals, mates, mquals


class TwoTextWorld:
    def __init__(self, api, world, seqs, quals, mates, mquals):
        from charon_amd import pack
        self.api = api
        self.t1, self.t2, self.two, self.one_text, self.one = two_text_batch(seqs, quals, mates, mquals)
        self.n = len(seqs)
        self.bufs = [DeviceText(api, len(t)) for t in (self.t1, self.t2, self.one_text)]
        self.dev = [(b.ptr, b.put(t, pad=b"X")) for b, t in zip(self.bufs, (self.t1, self.t2, self.one_text))]
        self.st = api.Stream(world["gf"], self.n, pack.pack_reads(seqs, mates)["n_bases"])
        self.st.set_model(api.default_model(2, 0, paired=True))

    def close(self):
        self.st.destroy()
        for b in self.bufs:
            b.free()


@pytest.mark.parametrize("n_in_mate2", [None, b"NnR"])
def test_two_text_batch_packs_like_one_text_and_numpy(api, world, n_in_mate2):
    r = util.rng(61)
    seqs, quals, mates, mquals = mate_cross(r, world, n_in_mate2)
    w = TwoTextWorld(api, world, seqs, quals, mates, mquals)
    try:
        assert {int(o) % 32 for o in w.two["seq1_offset"]} >= set(range(18)) and {int(o) % 32 for o in w.two["seq2_offset"]} >= set(range(18))
        assert {int(o) % 32 for o in w.two["qual2_offset"]} >= set(range(18))
        for _ in range(2):  # (twice: the slot's buffers are recycled)
            two = w.st.text_pack(w.two, text_device=w.dev[0], text2_device=w.dev[1])
            one = w.st.text_pack(w.one, text_device=w.dev[2])
            assert_same_packed(two, one)
            assert_packed_like_numpy(two, seqs, quals, mates, mquals)
            assert two["has_n"] == (1 if n_in_mate2 else 0)
    finally:
        w.close()


@pytest.mark.parametrize("n_in_mate2", [None, b"NNN"])
def test_two_text_batch_through_the_chain(api, world, n_in_mate2):
    r = util.rng(62)
    seqs, quals, mates, mquals = mate_cross(r, world, n_in_mate2)
    w = TwoTextWorld(api, world, seqs, quals, mates, mquals)
    try:
        comp = np.zeros(w.n, np.float32)
        w.st.submit_text(w.one, comp, text_device=w.dev[2])
        one = w.st.wait_text()
        w.st.submit_text(w.two, comp, text_device=w.dev[0], text2_device=w.dev[1])
        two = w.st.wait_text()
        util.assert_same_results(two, one)
        for k in ("flags", "has_n", "n_bases"):
            assert np.array_equal(two[k], one[k]), k
        assert np.array_equal(two["mean_quality"].view(np.uint32), one["mean_quality"].view(np.uint32))
        util.assert_parity(two, run_oracle(world["fused"], seqs, mates))
    finally:
        w.close()


def test_two_text_batch_refusals_and_the_shorter_struct(api, world):
    L = api.lib()
    r = util.rng(63)
    seqs = util.sample_reads(r, world["gs"], 40, (100, 300))
    mates = util.sample_reads(r, world["gs"], 40, (100, 300))
    quals, mquals = good_quals(r, seqs), good_quals(r, mates)
    w = TwoTextWorld(api, world, seqs, quals, mates, mquals)
    oracle = run_oracle(world["fused"], seqs, mates)
    comp = np.zeros(w.n, np.float32)
    n2 = w.dev[1][1]
    pinned = api.pinned_array(len(w.t2) + 16, np.uint8)
    pinned[:len(w.t2)] = np.frombuffer(w.t2, np.uint8)
    pageable = np.frombuffer(w.t2 + b"X" * 16, np.uint8).copy()
    bad_buf = DeviceText(api, len(w.t2))
    try:
        def works():
            w.st.submit_text(w.two, comp, text_device=w.dev[0], text2_device=w.dev[1])
            util.assert_parity(w.st.wait_text(), oracle)

        def refused(tb, word, code=-1, **kw):
            for call in (lambda: w.st.submit_text(tb, comp, **kw), lambda: w.st.text_pack(tb, **kw)):
                with pytest.raises(api.ChnError, match="error %d:.*%s" % (code, word)):
                    call()
            works()  # the stream is usable, with nothing of the refused batch in it

        works()
        host_tb = dict(w.two, text=np.frombuffer(w.one_text, np.uint8))
        refused(host_tb, "text2 needs CHN_TEXT_ON_DEVICE", text2_device=w.dev[1])
        single = {k: v for k, v in w.two.items() if not k.endswith(("2_offset", "2_length"))}
        refused(single, "text2 without seq2_", text_device=w.dev[0], text2_device=w.dev[1])
        refused(w.two, "text2.*page-locked", text_device=w.dev[0], text2_device=(pinned.ctypes.data, n2))
        refused(w.two, "text2.*not device memory", text_device=w.dev[0], text2_device=(pageable.ctypes.data, n2))
        refused(w.two, "text2.*16-byte aligned", text_device=w.dev[0], text2_device=(w.dev[1][0] + 4, n2))
        # a mate-2 stretch beyond text2_bytes: the last quality string ends at the text's last 5 or 6 filler bytes
        last = int(w.two["qual2_offset"][-1]) + int(w.two["qual2_length"][-1])
        refused(w.two, "read %d reaches beyond" % (w.n - 1), text_device=w.dev[0], text2_device=(w.dev[1][0], last - 1))
        # ... which is measured against text2_bytes, not text_bytes: text 2 is the longer one here or not, both orders pass when in range
        w.st.submit_text(w.two, comp, text_device=w.dev[0], text2_device=(w.dev[1][0], last))
        util.assert_parity(w.st.wait_text(), oracle)
        # an illegal byte in mate 2 only names the read
        t2 = bytearray(w.t2)
        t2[int(w.two["seq2_offset"][17]) + 40] = ord("!")
        bad_dev = (bad_buf.ptr, bad_buf.put(bytes(t2), pad=b"X"))
        refused(w.two, "illegal byte in the sequence of read 17 ", text_device=w.dev[0], text2_device=bad_dev)

        # today's shorter struct_size: no text2, nothing behind gzip_output is looked at -- the one-text batch runs as before
        t, keep, n = w.st._text_batch(w.one, comp, text_device=w.dev[2], text2_device=(0x10, 1 << 40))  # (a text2 that is not read)
        t.struct_size = ctypes.sizeof(api.TextBatch)
        assert L.chn_text_submit(w.st.h, ctypes.byref(t)) == 0, L.chn_last_error().decode()
        w.st._fifo.append((n, None, 0, 0))
        util.assert_parity(w.st.wait_text(), oracle)
        t.struct_size = ctypes.sizeof(api.TextBatch) + 8
        assert L.chn_text_submit(w.st.h, ctypes.byref(t)) == -1 and "struct_size" in L.chn_last_error().decode()
        works()
    finally:
        w.close()
        bad_buf.free()
        api.host_free(pinned)


# ---- 3. the pieces together: two BGZF files to calls, the texts staying in device memory -------------------------------------------------
def test_two_bgzf_files_to_calls(api, world):
    """what a paired caller of the device-resident chain does: the members of either file inflated into a device buffer of its own,
    the records found there (file 2 without its ids), the ids compared on the device, one batch over the two texts"""
    from charon_amd import pack
    from tests import inflate_cases as ic
    from tests.test_gpu_text_chain import bgzf_members
    r = util.rng(93)
    n = 300
    seqs = util.sample_reads(r, world["gs"], n, (80, 250))
    mates = util.sample_reads(r, world["gs"], n, (30, 400))
    quals, mquals = good_quals(r, seqs), good_quals(r, mates)
    names = [b"pair%d lane %d" % (i, i % 7) if i % 13 else b"" for i in range(n)]
    fastq = lambda mate, ss, qs: b"".join(b"@" + (i + b"/%d" % mate if i else b"") + b"\n" + s + b"\n+\n" + q + b"\n" for i, s, q in zip(names, ss, qs))
    texts = [fastq(1, seqs, quals), fastq(2, mates, mquals)]
    inflater = api.Inflater(0)
    bufs = [DeviceText(api, len(t) + 16, fill=0xA5) for t in texts]
    st = api.Stream(world["gf"], n, pack.pack_reads(seqs, mates)["n_bases"])
    st.set_model(api.default_model(2, 0, paired=True))
    try:
        def split(k, text, want_ids):
            members = bgzf_members(ic.bgzf(text))
            _, status = inflater.run([m[0] for m in members], [m[2] for m in members], expected=[m[1] for m in members], out_device=(bufs[k].ptr, bufs[k].nbytes))
            assert not status.any()
            sp = st.text_split(bufs[k].ptr, len(text), max_records=n + 1, want_ids=want_ids)
            assert sp["n_records"] == n and sp["consumed"] == len(text)
            return sp

        sp1, sp2 = split(0, texts[0], True), split(1, texts[1], False)
        assert sp2["ids"] is None  # the ids of file 2 stay on the device
        ids = (sp1["id_offset"], sp1["id_length"], sp2["id_offset"], sp2["id_length"])
        dev = [(b.ptr, len(t)) for b, t in zip(bufs, texts)]
        assert st.pair_ids(*dev[0], *dev[1], *ids) == n
        tb = dict(flags=0, text=None, seq1_offset=sp1["seq_offset"], seq1_length=sp1["seq_length"], qual1_offset=sp1["qual_offset"], qual1_length=sp1["seq_length"],
                  seq2_offset=sp2["seq_offset"], seq2_length=sp2["seq_length"], qual2_offset=sp2["qual_offset"], qual2_length=sp2["seq_length"])
        comp = np.zeros(n, np.float32)
        st.submit_text(tb, comp, text_device=dev[0], text2_device=dev[1])
        got = st.wait_text()
        # the host-text path over the two files back to back, the offsets of mate 2 rebased
        base = np.uint64(len(texts[0]))
        st.submit_text(dict(tb, text=np.frombuffer(texts[0] + texts[1], np.uint8), seq2_offset=sp2["seq_offset"] + base, qual2_offset=sp2["qual_offset"] + base), comp)
        host = st.wait_text()
        util.assert_same_results(got, host)
        for k in ("flags", "has_n", "n_bases"):
            assert np.array_equal(got[k], host[k]), k
        assert np.array_equal(got["mean_quality"].view(np.uint32), host["mean_quality"].view(np.uint32))
        util.assert_parity(got, run_oracle(world["fused"], seqs, mates))
        assert (got["call"] != 255).sum() > 50
        # a pair whose names differ: found on the device, index and all
        bad = bytearray(texts[1])
        bad[int(sp2["id_offset"][123]) + 2] ^= 0x01
        sp2 = split(1, bytes(bad), False)
        assert st.pair_ids(*dev[0], *dev[1], sp1["id_offset"], sp1["id_length"], sp2["id_offset"], sp2["id_length"]) == 123
    finally:
        st.destroy()
        inflater.destroy()
        for b in bufs:
            b.free()
