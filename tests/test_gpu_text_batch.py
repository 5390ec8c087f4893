"""GPU tests (-m gpu) of text batches: reads handed over as plain text (letters and phred characters at any byte offset of one
buffer), packed on the device by k_text_pack, then classified by the unchanged chain.

Yardsticks, none of which is the new kernel: pack.pack_reads (numpy) for the packed form, numpy for the mean quality
(np.float32(sum) / np.float32(count), compared BITWISE), the existing host-packed path (submit_host) for every result column
including the probabilities bitwise, the oracle for parity, zlib for the gzip sizes."""
import zlib

import numpy as np
import pytest

from tests import util
from tests.test_gpu_parity import run_oracle

pytestmark = pytest.mark.gpu

AMBIG = b"NRYSWKMBDHV"
LENGTHS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 5000, 32767, 32768, 200003]


@pytest.fixture(scope="module")
def api():
    import charon_amd.api as api
    return api


@pytest.fixture(scope="module")
def world(api, oracle_lib):
    """two genomes; a 2-bin index (W = 1, counters in LDS) and a 70-bin one (W = 2, row log)"""
    r = util.rng(77)
    glen = 300000
    gs = [util.random_seq(r, glen), util.random_seq(r, glen)]
    fused = util.build_oracle_index(oracle_lib, [[g] for g in gs], [0, 1], ["host", "microbial"])
    many = [gs[i % 2][(i // 2) * (glen // 35):(i // 2 + 1) * (glen // 35) + 40] for i in range(70)]
    rows = util.build_oracle_index(oracle_lib, [[m] for m in many], [i % 2 for i in range(70)], ["human", "microbial"], fill_seed=8, fill=0.08)
    gf, gr = util.gpu_index_from_oracle(api, fused), util.gpu_index_from_oracle(api, rows)
    yield dict(gs=gs, fused=fused, rows=rows, gf=gf, gr=gr)
    gf.destroy()
    gr.destroy()
    fused.free()
    rows.free()


def random_quals(r, n, lo=33, hi=126):
    return r.integers(lo, hi + 1, n).astype(np.uint8).tobytes()


def numpy_mq(quals, mquals=None):
    """mean quality as the reference forms it: int sum of (signed char)q - 33 over both mates / count, one float division"""
    n = len(quals)
    out = np.zeros(n, np.float32)
    for i in range(n):
        q = quals[i] + (mquals[i] if mquals is not None else b"")
        if len(q):
            s = int(np.frombuffer(q, np.int8).astype(np.int64).sum()) - 33 * len(q)
            out[i] = np.float32(s) / np.float32(len(q))
    return out


def assert_packed_like_numpy(out, seqs, quals=None, mates=None, mquals=None):
    from charon_amd import pack
    up = lambda rs: None if rs is None else [bytes(x) for x in rs]
    p = pack.pack_reads(up(seqs), up(mates))
    assert out["n_bases"] == p["n_bases"]
    np.testing.assert_array_equal(out["seg1_offset"], p["seg1_offset"])
    if mates is not None:
        np.testing.assert_array_equal(out["seg2_offset"], p["seg2_offset"])
    assert out["bases2"].size == p["n_bases"] // 16 and out["nmask"].size == p["n_bases"] // 32
    np.testing.assert_array_equal(out["bases2"], p["bases2"])
    if p["nmask"] is None:
        assert out["has_n"] == 0 and not out["nmask"].any()
    else:
        assert out["has_n"] == 1 and out["nmask"].any()
        np.testing.assert_array_equal(out["nmask"], p["nmask"])
    want = numpy_mq(quals, mquals) if quals is not None else np.zeros(len(seqs), np.float32)
    np.testing.assert_array_equal(out["mean_quality"].view(np.uint32), want.view(np.uint32))


def awkward_batch(r):
    """every length class, letter and N placement the packer must get right"""
    alphabet = np.frombuffer(b"ACGTacgtUu", np.uint8)
    seqs = [alphabet[r.integers(0, alphabet.size, L)].tobytes() for L in LENGTHS]
    seqs += [AMBIG, AMBIG.lower(), AMBIG + AMBIG.lower() + b"acgu"]               # each ambiguity letter in both cases
    for start, run in ((10, 12), (28, 9), (60, 10), (5, 130), (0, 70)):           # N runs across 16-, 32- and 64-base boundaries
        s = bytearray(util.random_seq(r, 300))
        s[start:start + run] = b"N" * run
        seqs.append(bytes(s))
    seqs.append(util.random_seq(r, 75) + b"N" * 25)                               # an N run that ends a read
    seqs.append(util.random_seq(r, 64 - 3) + b"nnn")                              # ... exactly at a chunk boundary
    seqs += [b"N", b"N" * 16, b"N" * 97, b"n" * 64]                               # reads of N only
    big = bytearray(util.random_seq(r, 40000))
    big[39990:] = b"N" * 10
    seqs.append(bytes(big))
    seqs += [util.random_seq(r, int(L)) for L in r.integers(1, 40, 24)]           # short reads: many start alignments
    quals = [random_quals(r, len(s)) for s in seqs]
    quals[0] = b"!"
    quals[1] = b"~" * 15
    quals[5] = random_quals(r, 32 + 9)                                            # longer than its sequence (the reader allows it)
    quals[13] = random_quals(r, 5000 + 37)
    quals[2] = bytes(range(33, 127))[:16]
    quals[10] = bytes(range(33, 127)) + bytes(range(126, 93, -1))                 # the whole range ! .. ~ (127 letters)
    assert len(quals[10]) == 127
    return seqs, quals


def test_packing_alone_equals_the_numpy_packer(api, world):
    from charon_amd import pack
    r = util.rng(11)
    seqs, quals = awkward_batch(r)
    n = len(seqs)
    cap_bases = pack.pack_reads(seqs, seqs)["n_bases"] + 1024
    st = api.Stream(world["gf"], 2 * n, cap_bases)
    residues = set()
    for gap in (b"", b"\n", b"\n+\n", b"@r\n" * 5):
        tb = pack.text_batch(seqs, quals, gap=gap)
        residues |= {int(o) % 16 for o in tb["seq1_offset"]} & {int(o) % 16 for o in tb["qual1_offset"]}
        # a batch full of N first, then the batch twice: the buffers are recycled and the padding must come out zero
        full_n = pack.text_batch([b"N" * len(s) for s in seqs], [b"~" * len(q) for q in quals], gap=gap)
        assert_packed_like_numpy(st.text_pack(full_n), [b"N" * len(s) for s in seqs], [b"~" * len(q) for q in quals])
        for _ in range(2):
            assert_packed_like_numpy(st.text_pack(tb), seqs, quals)
    assert residues == set(range(16)), residues
    # FASTA: no qualities, mean quality 0.0
    assert_packed_like_numpy(st.text_pack(pack.text_batch(seqs, gap=b">x\n")), seqs)
    # an ACGT-only batch: no N, the mask all zero
    clean = [util.random_seq(r, int(L)) for L in (1, 16, 63, 64, 65, 700, 40000)]
    out = st.text_pack(pack.text_batch(clean, [random_quals(r, len(s)) for s in clean], gap=b"\n"))
    assert out["has_n"] == 0
    # pairs with mates of unequal length (one of them empty, one without letters at all but with the other mate present)
    mates = [s[::-1][:max(0, len(s) - 7)] for s in seqs]
    mates[3] = util.random_seq(r, 1000)
    mquals = [random_quals(r, len(m)) for m in mates]
    mquals[4] = random_quals(r, len(mates[4]) + 20)
    for gap in (b"", b"\n+\n"):
        tb = pack.text_batch(seqs, quals, mates, mquals, gap=gap)
        for _ in range(2):
            assert_packed_like_numpy(st.text_pack(tb), seqs, quals, mates, mquals)
    # mate 1 without letters: the read lives in its second segment
    s1, m1 = [b"", b"ACGT"], [b"ACGTN" * 9, b""]
    q1, mq1 = [b"", b"IIII"], [random_quals(r, 45), b""]
    assert_packed_like_numpy(st.text_pack(pack.text_batch(s1, q1, m1, mq1, gap=b"\n")), s1, q1, m1, mq1)
    # the same through dna5 ranks
    for gap in (b"", b"\x07" * 3):
        assert_packed_like_numpy(st.text_pack(pack.text_batch(seqs, quals, gap=gap, ranks=True)), seqs, quals)
        assert_packed_like_numpy(st.text_pack(pack.text_batch(seqs, quals, mates, mquals, gap=gap, ranks=True)), seqs, quals, mates, mquals)
    st.destroy()


def zsize(b):
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 8)
    return len(co.compress(b) + co.flush())


def both_ways(api, gidx, oidx, seqs, quals, mates=None, mquals=None, paired_model=False, split_bucket=0, gzip=None, gap=b"\n"):
    """the batch as text and host-packed on one stream; every column equal, parity with the oracle"""
    from charon_amd import pack
    n = len(seqs)
    p = pack.pack_reads(seqs, mates)
    st = api.Stream(gidx, n, p["n_bases"], split_bucket=split_bucket)
    C = gidx.desc.num_categories
    st.set_model(api.default_model(C, 0 if paired_model else gidx.desc.host_index, paired=paired_model))
    comp = None if gzip else np.zeros(n, np.float32)
    gz = dict(gzip_tallies=gzip[0], gzip_output=gzip[1]) if gzip else {}
    st.submit_text(pack.text_batch(seqs, quals, mates, mquals, gap=gap), comp, **gz)
    txt = st.wait_text()
    mq = numpy_mq(quals, mquals) if quals is not None else np.zeros(n, np.float32)
    st.submit_host(p, mq, comp, **gz)
    host = st.wait_host()
    st.destroy()
    util.assert_same_results(txt, host)
    np.testing.assert_array_equal(txt["flags"], host["flags"])
    np.testing.assert_array_equal(txt["mean_quality"].view(np.uint32), mq.view(np.uint32))
    assert txt["n_bases"] == p["n_bases"] and txt["has_n"] == (0 if p["nmask"] is None else 1)
    if gzip:
        np.testing.assert_array_equal(txt["gzip_sizes"], host["gzip_sizes"])
    util.assert_parity(txt, run_oracle(oidx, seqs, mates))
    return txt


def good_quals(r, seqs):
    """qualities well above the model's min_quality, so that the oracle (run at a constant 40) gates the same way"""
    return [random_quals(r, len(s), 33 + 25, 33 + 60) for s in seqs]


def with_n(r, reads, every=3):
    out = []
    for i, s in enumerate(reads):
        if i % every == 0 and len(s) > 40:
            b = bytearray(s)
            at = int(r.integers(0, len(s) - 20))
            b[at:at + int(r.integers(1, 20))] = b"N" * 19
            s = bytes(b[:len(s)])
        out.append(s)
    return out


def test_end_to_end_acgt_only(api, world):
    r = util.rng(21)
    reads = util.sample_reads(r, world["gs"], 600, (30, 3000))
    out = both_ways(api, world["gf"], world["fused"], reads, good_quals(r, reads))
    assert out["has_n"] == 0 and (out["call"] != 255).sum() > 100


def test_end_to_end_with_n(api, world):
    r = util.rng(22)
    reads = with_n(r, util.sample_reads(r, world["gs"], 600, (30, 3000)))
    out = both_ways(api, world["gf"], world["fused"], reads, good_quals(r, reads), gap=b"\n+\n")
    assert out["has_n"] == 1
    # FASTA: mean quality 0 gates every call, on both paths alike
    from charon_amd import pack
    st = api.Stream(world["gf"], len(reads), pack.pack_reads(reads)["n_bases"])
    st.set_model(api.default_model(2, world["gf"].desc.host_index))
    st.submit_text(pack.text_batch(reads, gap=b">r\n"), np.zeros(len(reads), np.float32))
    txt = st.wait_text()
    st.submit_host(pack.pack_reads(reads), np.zeros(len(reads), np.float32), np.zeros(len(reads), np.float32))
    util.assert_same_results(txt, st.wait_host())
    assert not txt["mean_quality"].any()
    st.destroy()


def test_end_to_end_pairs_call_category(api, oracle_lib):
    r = util.rng(23)
    gs = [util.random_seq(r, 3000) for _ in range(8)]
    oidx = util.build_oracle_index(oracle_lib, [[g] for g in gs], list(range(8)), ["c%d" % i for i in range(7)] + ["host"])
    g = util.gpu_index_from_oracle(api, oidx)
    m1 = util.sample_reads(r, gs, 400, (100, 150), sub_rate=0.01)
    m2 = [util.mutate(r, gs[int(r.integers(0, 8))][500:500 + int(r.integers(60, 150))], 0.01) for _ in range(400)]
    m1[0], m2[0] = b"ACGT", b"A" * 150
    m1[1], m2[1] = b"", b"C" * 19
    m1[2], m2[2] = b"G" * 30, b""
    try:
        out = both_ways(api, g, oidx, m1, good_quals(r, m1), m2, good_quals(r, m2), paired_model=True)
        assert (out["call"] != 255).sum() > 50
        m1n = with_n(r, m1)
        assert both_ways(api, g, oidx, m1n, good_quals(r, m1n), m2, good_quals(r, m2), paired_model=True)["has_n"] == 1
    finally:
        g.destroy()
        oidx.free()


def test_end_to_end_multi_bin_row_log(api, world):
    r = util.rng(24)
    reads = with_n(r, util.sample_reads(r, world["gs"], 500, (50, 2500)), every=7)
    both_ways(api, world["gr"], world["rows"], reads, good_quals(r, reads))
    clean = util.sample_reads(r, world["gs"], 300, (50, 2500))
    assert both_ways(api, world["gr"], world["rows"], clean, good_quals(r, clean))["has_n"] == 0


def test_end_to_end_long_read_split_over_a_wavefront(api, world):
    r = util.rng(25)
    gs = world["gs"]
    reads = [util.mutate(r, gs[0][1000:201000], 0.05), util.mutate(r, gs[1][5:70005], 0.1)] + util.sample_reads(r, gs, 100, (100, 6000))
    for gidx, oidx in ((world["gf"], world["fused"]), (world["gr"], world["rows"])):
        both_ways(api, gidx, oidx, reads, good_quals(r, reads), split_bucket=64)
    both_ways(api, world["gf"], world["fused"], with_n(r, reads, every=1), good_quals(r, reads), split_bucket=64)


def test_end_to_end_gzip_sizes(api, world):
    r = util.rng(26)
    for reads in (util.sample_reads(r, world["gs"], 200, (20, 4000)), with_n(r, util.sample_reads(r, world["gs"], 200, (20, 4000)))):
        reads[5] = b"ACGT" * 500
        out = both_ways(api, world["gf"], world["fused"], reads, good_quals(r, reads), gzip=(61440, api.GZIP_SIZES))
        for i, rd in enumerate(reads):
            assert int(out["gzip_sizes"][i]) == zsize(rd), (i, len(rd))


def test_three_in_flight_text_and_packed_alternating(api, world):
    from charon_amd import pack
    r = util.rng(27)
    g = world["gf"]
    sets = [with_n(r, util.sample_reads(r, world["gs"], 300, (50, 2000))), util.sample_reads(r, world["gs"], 257, (50, 2000)),
            util.sample_reads(r, world["gs"], 300, (50, 2000)), with_n(r, util.sample_reads(r, world["gs"], 100, (50, 2000)))]
    quals = [good_quals(r, s) for s in sets]
    cap = max(pack.pack_reads(s)["n_bases"] for s in sets)
    st = api.Stream(g, 300, cap)
    st.set_model(api.default_model(2, g.desc.host_index))
    want = []
    for s, q in zip(sets, quals):  # one at a time, host-packed: the yardstick
        st.submit_host(pack.pack_reads(s), numpy_mq(q), np.zeros(len(s), np.float32))
        want.append(st.wait_host())

    def text(i):
        tb = pack.text_batch(sets[i], quals[i], gap=b"\n+\n")
        st.submit_text(tb, np.zeros(len(sets[i]), np.float32))
        for k in tb:  # the caller's buffers are free again: scribble over all of them
            if isinstance(tb[k], np.ndarray):
                tb[k][...] = 0x58 if k == "text" else 0

    def packed(i):
        st.submit_host(pack.pack_reads(sets[i]), numpy_mq(quals[i]), np.zeros(len(sets[i]), np.float32))

    text(0), packed(1), text(2)
    with pytest.raises(api.ChnError, match="three batches"):
        text(3)
    got0 = st.wait_text()
    text(3)
    with pytest.raises(api.ChnError, match="not a text batch"):  # the oldest is the packed one: nothing is consumed
        st.wait_text()
    got1 = st.wait_host()
    got2 = st.wait_host()  # plain chn_batch_wait on a text batch: works, without the text columns
    got3 = st.wait_text()
    for i, got in enumerate((got0, got1, got2, got3)):
        util.assert_same_results(got, want[i])
    assert got0["has_n"] == 1 and got3["has_n"] == 1 and "mean_quality" not in got2
    np.testing.assert_array_equal(got0["mean_quality"].view(np.uint32), numpy_mq(quals[0]).view(np.uint32))
    st.destroy()


def test_illegal_bytes_and_bad_descriptors_are_refused(api, world):
    from charon_amd import pack
    r = util.rng(28)
    g = world["gf"]
    reads = util.sample_reads(r, world["gs"], 130, (40, 900))
    quals = good_quals(r, reads)
    p = pack.pack_reads(reads)
    st = api.Stream(g, len(reads), p["n_bases"])
    st.set_model(api.default_model(2, g.desc.host_index))
    st.submit_host(p, numpy_mq(quals), np.zeros(len(reads), np.float32))
    want = st.wait_host()

    def good_batch_still_right():
        st.submit_text(pack.text_batch(reads, quals, gap=b"\n"), np.zeros(len(reads), np.float32))
        util.assert_same_results(st.wait_text(), want)

    last = len(reads) - 1
    for ranks, bad_bytes in ((False, [ord("X"), ord("-"), ord("*"), ord("\n"), 0x00, 0xC3]), (True, [5])):
        for byte in bad_bytes:
            for read, pos in ((last, -1), (0, 0)):
                tb = pack.text_batch(reads, quals, gap=b"\n", ranks=ranks)
                at = int(tb["seq1_offset"][read]) + (pos if pos >= 0 else int(tb["seq1_length"][read]) - 1)
                tb["text"][at] = byte
                for call in (st.submit_text, st.text_pack):
                    with pytest.raises(api.ChnError) as e:
                        call(tb)
                    assert "error -1:" in str(e.value) and ("read %d " % read) in str(e.value) and "1 illegal byte" in str(e.value), str(e.value)
                good_batch_still_right()
    # two illegal bytes: the smallest read index is named, the count is 2
    tb = pack.text_batch(reads, quals, gap=b"\n")
    tb["text"][int(tb["seq1_offset"][7])] = ord("!")
    tb["text"][int(tb["seq1_offset"][90]) + 3] = ord("@")
    with pytest.raises(api.ChnError, match=r"read 7 \(2 illegal"):
        st.submit_text(tb)
    good_batch_still_right()
    # a descriptor beyond text_bytes: refused on the host
    for key in ("seq1", "qual1"):
        tb = pack.text_batch(reads, quals, gap=b"\n")
        tb[key + "_length"][last] += 1  # the last string ends the buffer
        if key == "seq1":
            tb["qual1_offset"][last] = 0
            tb["seq1_offset"][last] = len(tb["text"]) - int(tb["seq1_length"][last]) + 1
        with pytest.raises(api.ChnError, match=r"error -1:.*beyond text_bytes"):
            st.submit_text(tb)
    tb = pack.text_batch(reads, quals, gap=b"\n")
    tb["seq1_offset"][3] = 2 ** 63
    with pytest.raises(api.ChnError, match=r"error -1:.*read 3 "):
        st.submit_text(tb)
    # qualities given without their lengths
    tb = pack.text_batch(reads, quals, gap=b"\n")
    del tb["qual1_length"]
    with pytest.raises(api.ChnError, match="error -1:.*qual1"):
        st.submit_text(tb)
    # more reads, or more bases, than the stream was created for
    with pytest.raises(api.ChnError, match="error -5:"):
        st.submit_text(pack.text_batch(reads + [b"ACGT"], quals + [b"IIII"]))
    with pytest.raises(api.ChnError, match="error -5:"):
        st.submit_text(pack.text_batch(reads[:-1] + [reads[-1] + b"A" * 4096], quals))
    good_batch_still_right()
    st.destroy()
