"""CPU tests of the text-batch interface (chn_text_submit / chn_text_wait / chn_text_pack): struct layouts against the header,
the numpy layout helper pack.text_batch, and the header's documentation of every new name.  No compute calls."""
import ctypes
import os
import re

import numpy as np

from tests import util

HEADER = os.path.join(util.ROOT, "include", "charon_hip.h")


def test_text_struct_layout_matches_header():
    import charon_amd.api as api
    # chn_text_batch: 2 x uint32 (8) + n_reads (8) + text (8) + text_bytes (8) + 8 descriptor pointers (64) + compression (8)
    # + 2 x uint32 (8) = 112, no padding (every 8-byte field sits at a multiple of 8)
    assert ctypes.sizeof(api.TextBatch) == 112
    assert api.TextBatch.text.offset == 16 and api.TextBatch.seq1_offset.offset == 32 and api.TextBatch.qual2_length.offset == 88
    assert api.TextBatch.compression.offset == 96 and api.TextBatch.gzip_output.offset == 108
    # chn_text_result: 2 x uint32 (8) + n_bases (8) + mean_quality (8)
    assert ctypes.sizeof(api.TextResult) == 24
    assert api.TextResult.n_bases.offset == 8 and api.TextResult.mean_quality.offset == 16
    # the feature arrives as new structs: the existing ones keep their sizes
    assert ctypes.sizeof(api.Batch) == 96 and ctypes.sizeof(api.Result) == 80
    # field order as declared in the header
    header = open(HEADER).read()
    for cname, cls in (("chn_text_batch", api.TextBatch), ("chn_text_result", api.TextResult)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = re.findall(r"\*?\s*\b([a-z_0-9]+);", body)
        assert declared == [f[0] for f in cls._fields_], (cname, declared)
    assert api.TEXT_DNA5_RANKS == int(re.search(r"#define CHN_TEXT_DNA5_RANKS (\d+)u", header).group(1))


def test_header_documents_every_new_name():
    import charon_amd.api as api
    header = open(HEADER).read()
    for name in ("chn_text_submit", "chn_text_wait", "chn_text_pack"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in api.EXPORTS and getattr(api.lib(), name) is not None
        assert len(re.findall(r"\b%s\b" % name, header)) >= 2, "%s is declared but not described" % name
    for word in ("CHN_TEXT_DNA5_RANKS", "chn_text_batch", "chn_text_result", "text_bytes", "qual1_offset", "seq2_offset", "qual2_length",
                 "has_n", "illegal", "may be reused as soon as chn_text_submit returns", "CHN_E_CAPACITY", "dna5 ranks"):
        assert word in header, word
    for method in ("submit_text", "wait_text", "text_pack"):
        assert callable(getattr(api.Stream, method))


def _slices(tb, key):
    text = tb["text"].tobytes()
    return [text[int(o):int(o) + int(l)] for o, l in zip(tb[key + "_offset"], tb[key + "_length"])]


def test_text_batch_layout_round_trip():
    from charon_amd import pack
    seqs = [b"ACGTNNACGT" * 7, b"", b"acgtRYacgt", b"T" * 64, b"G" * 65, b"u"]
    quals = [b"I" * 70, b"", b"!~5IIIIIII#", b"5" * 64, b"~" * 65, b"#"]  # (one quality string longer than its sequence)
    mates = [s[::-1] for s in seqs]
    mquals = [q[::-1] for q in quals]
    for gap in (b"", b"\n", b"@id 1\n", b"x" * 15, b"+" * 16, b"\n+\n" * 11):
        tb = pack.text_batch(seqs, quals, mates, mquals, gap=gap)
        assert tb["flags"] == 0 and tb["text"].dtype == np.uint8
        assert _slices(tb, "seq1") == seqs and _slices(tb, "qual1") == quals
        assert _slices(tb, "seq2") == mates and _slices(tb, "qual2") == mquals
        assert tb["seq1_offset"].dtype == np.uint64 and tb["seq1_length"].dtype == np.uint32
        assert int(tb["seq1_offset"][0]) == len(gap)
        assert len(tb["text"]) == sum(map(len, seqs + quals + mates + mquals)) + 4 * len(seqs) * len(gap)
        # every string is preceded by exactly the gap
        if gap:
            text = tb["text"].tobytes()
            for key in ("seq1", "qual1", "seq2", "qual2"):
                for o in tb[key + "_offset"]:
                    assert text[int(o) - len(gap):int(o)] == gap
    # all 16 start residues can be reached through the gap
    res = set()
    for g in range(16):
        tb = pack.text_batch([b"ACGT" * 4] * 5, gap=b"-" * g)
        res |= {int(o) % 16 for o in tb["seq1_offset"]}
    assert res == set(range(16))
    # FASTA (no qualities), single-end: only the sequence columns exist
    tb = pack.text_batch(seqs, gap=b">r\n")
    assert _slices(tb, "seq1") == seqs and "qual1_offset" not in tb and "seq2_offset" not in tb and "qual2_offset" not in tb
    # str input
    assert _slices(pack.text_batch(["ACGT", "NN"], ["IIII", "!!"]), "qual1") == [b"IIII", b"!!"]


def test_text_batch_ranks():
    from charon_amd import pack
    seqs = [b"ACGTUNacgtun", b"RYSWKMBDHVryswkmbdhv", b"AX-"]
    tb = pack.text_batch(seqs, [b"I" * len(s) for s in seqs], gap=b"\xff", ranks=True)
    assert tb["flags"] == 1
    got = _slices(tb, "seq1")
    assert got[0] == bytes([0, 1, 2, 4, 4, 3] * 2)
    assert got[1] == bytes([3] * 20)
    assert got[2] == bytes([0, 255, 255])  # not IUPAC: a rank the library must refuse
    assert _slices(tb, "qual1") == [b"I" * len(s) for s in seqs]  # qualities stay characters
    # the same layout rule as the packed batch: ranks -> codes agrees with pack_reads on the letters
    p = pack.pack_reads([seqs[0], seqs[1]])
    back = pack.unpack_reads(p["bases2"], p["seg1_offset"], p["seg1_length"], p["nmask"])
    rank_to_letter = {0: b"A", 1: b"C", 2: b"G", 3: b"N", 4: b"T"}
    assert [b"".join(rank_to_letter[x] for x in g) for g in got[:2]] == back


def test_bad_text_batches_value_is_rejected_up_front(tmp_path):
    """CHARON_TEXT_BATCHES: anything but unset / 0 / 1 ends the run with status 1 before the index file is opened and before any HIP call"""
    import subprocess
    exe = os.path.join(util.ROOT, "charon_amd", "bin", "charon")
    g = os.path.join(util.ROOT, "tests", "golden")
    (tmp_path / "junk.idx").write_bytes(b"not an index")
    for sub in ("dehost", "classify"):
        for v in ("2", "", "yes", "01", "-1"):
            env = dict(os.environ, CHARON_TEXT_BATCHES=v)
            p = subprocess.run([exe, sub, "--db", str(tmp_path / "junk.idx"), os.path.join(g, "cfg1_reads.fastq.gz"), "--log", str(tmp_path / "charon.log")],
                               cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            err = p.stderr.decode()
            assert p.returncode == 1 and p.stdout == b"" and "charon: CHARON_TEXT_BATCHES: " in err, (v, err)
            assert "junk.idx" not in err and "hip" not in err.lower(), err
