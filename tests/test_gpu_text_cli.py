"""GPU tests (-m gpu) of CHARON_TEXT_BATCHES=1 in the front end: reads go to the device as text (chn_text_submit), letters -> codes
and the mean-quality column are formed there.  The TSV must be byte-identical to the run without the switch, for every kind of
input the reader knows and every mode of the read loop."""
import bz2
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import util
from tests.test_gpu_cli import assert_same_tsv

pytestmark = pytest.mark.gpu
G = os.path.join(util.ROOT, "tests", "golden")
EXE = os.path.join(util.ROOT, "charon_amd", "bin", "charon")
IDX = os.path.join(G, "cfg1.idx")
FQ = os.path.join(G, "cfg1_reads.fastq.gz")


def run_cli(args, cwd, env_extra=None, sub="dehost"):
    os.makedirs(cwd, exist_ok=True)
    env = {k: v for k, v in os.environ.items() if k != "CHARON_TEXT_BATCHES"}
    env.update(env_extra or {})
    p = subprocess.run([EXE, sub] + args + ["--log", os.path.join(cwd, "charon.log")], cwd=cwd, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def both(tmp_path, args, env=None, sub="dehost", tag="x"):
    """the run without the switch and with it: same exit status 0, byte-identical TSV; returns the TSV"""
    rc0, out0, err0 = run_cli(args, str(tmp_path / (tag + "_packed")), env, sub)
    rc1, out1, err1 = run_cli(args, str(tmp_path / (tag + "_text")), dict(env or {}, CHARON_TEXT_BATCHES="1"), sub)
    assert rc0 == 0 and rc1 == 0, (err0, err1)
    assert out0.count("\n") > 10
    assert out1 == out0, (args, env)
    assert "CHARON_TEXT_BATCHES=1" in open(tmp_path / (tag + "_text") / "charon.log").read()
    return out0


def genomes():
    recs, name = {}, None
    for fn in ("my.fasta", "cfg1_host.fasta"):
        for line in open(os.path.join(G, fn)):
            line = line.strip()
            if line.startswith(">"):
                name = fn + line[1:].split()[0]
                recs[name] = ""
            elif name:
                recs[name] += line
    return [s.encode() for s in recs.values() if len(s) > 500]


def write_fastq(path, reads, r, tag="", wrap=0, eol="\n", lo=5, hi=41):
    with open(path, "w", newline="") as f:
        for i, s in enumerate(reads):
            q = "".join(chr(33 + int(x)) for x in r.integers(lo, hi, len(s)))
            s = s.decode()
            if wrap:
                s = eol.join(s[j:j + wrap] for j in range(0, len(s), wrap))
                q = eol.join(q[j:j + wrap] for j in range(0, len(q), wrap))
            f.write("@read%d some text%s%s%s%s+%s%s%s" % (i, tag, eol, s, eol, eol, q, eol))


def test_text_switch_golden_and_every_input_format(tmp_path):
    out = both(tmp_path, ["--db", IDX, FQ], tag="golden")
    assert_same_tsv(out, open(os.path.join(G, "cfg1_expected.tsv")).read())  # as test_cli_golden_cfg1 compares
    data = gzip.decompress(open(FQ, "rb").read())
    (tmp_path / "plain.fastq").write_bytes(data)
    subprocess.run([sys.executable, os.path.join(util.ROOT, "tools", "make_bgzf.py"), str(tmp_path / "plain.fastq"), str(tmp_path / "b.fastq.gz"), "6", "2"], check=True)
    (tmp_path / "z.fastq.bz2").write_bytes(bz2.compress(data))
    for i, (f, env) in enumerate(((str(tmp_path / "plain.fastq"), {}), (str(tmp_path / "plain.fastq"), {"CHARON_NO_MMAP": "1"}),
                                  (str(tmp_path / "b.fastq.gz"), {}), (str(tmp_path / "z.fastq.bz2"), {}), (FQ, {"CHARON_INFLATE_CHUNK": "2048"}))):
        for t in ("1", "8"):
            assert both(tmp_path, ["--db", IDX, "-t", t, f], env, tag="fmt%d_t%s" % (i, t)) == out, (f, env, t)
    # decoded-slab inputs go out as the slab itself, a mapped plain file through the page-locked copy
    import re
    for tag, slab in (("golden", True), ("fmt0_t1", False), ("fmt1_t1", True), ("fmt2_t8", True), ("fmt3_t1", True)):
        m = re.search(r"text batches: (\d+) sent as the block's slab, (\d+) as a page-locked copy", open(tmp_path / (tag + "_text") / "charon.log").read())
        assert m and (int(m.group(1)) > 0) == slab and (int(m.group(2)) > 0) == (not slab), (tag, m and m.groups())
    # small batches: many text batches in flight, blocks cut into several of them
    for f in (FQ, str(tmp_path / "plain.fastq")):
        assert both(tmp_path, ["--db", IDX, "-t", "4", f], {"CHARON_BATCH_READS": "37"}, tag="b37" + os.path.basename(f)) == out
    # two replicas on one device
    assert both(tmp_path, ["--db", IDX, "-t", "4", FQ], {"CHARON_DEVICES": "0,0", "CHARON_BATCH_READS": "50"}, tag="dev") == out


def test_text_switch_wrapped_crlf_fasta_pairs_and_awkward_reads(tmp_path):
    r = util.rng(31)
    gs = genomes()
    reads = util.sample_reads(r, gs, 400, (30, 900), sub_rate=0.03)
    # N-rich, lower-case and ambiguity letters; one read beyond 61 440 letters
    reads[3] = reads[3].lower()
    reads[4] = b"N" * 200
    reads[5] = reads[5][:50] + b"NNNNNRYKMnnnswbdhv" + reads[5][68:]
    reads[6] = reads[6][:17].lower() + reads[6][17:]
    reads[7] = b"ACGU" + reads[7].replace(b"T", b"U")[4:]
    big = (gs[0] * (70000 // len(gs[0]) + 1))[:70001]
    reads[8] = util.mutate(r, big, 0.05)
    for i in range(20, 60):
        b = bytearray(reads[i])
        for at in r.integers(0, len(b), max(1, len(b) // 10)):
            b[int(at)] = ord("N")
        reads[i] = bytes(b)
    write_fastq(tmp_path / "a.fastq", reads, r)
    write_fastq(tmp_path / "w.fastq", reads, r, wrap=60, eol="\r\n")
    with open(tmp_path / "a.fasta", "w") as f:
        for i, s in enumerate(reads):
            s = s.decode()
            f.write(">read%d x\n%s\n" % (i, "\n".join(s[j:j + 70] for j in range(0, len(s), 70))))
    (tmp_path / "a.fastq.gz").write_bytes(gzip.compress((tmp_path / "a.fastq").read_bytes(), 6))
    (tmp_path / "a.fasta.gz").write_bytes(gzip.compress((tmp_path / "a.fasta").read_bytes(), 6))
    for i, f in enumerate(("a.fastq", "a.fastq.gz", "w.fastq", "a.fasta", "a.fasta.gz")):
        for env in ({}, {"CHARON_NO_MMAP": "1"}, {"CHARON_BATCH_READS": "37"}):
            both(tmp_path, ["--db", IDX, "-t", "4", str(tmp_path / f)], env, tag="awk%d_%s" % (i, "_".join(env) or "d"))
    # pairs (call_category), plain and compressed
    m1 = util.sample_reads(r, gs, 300, (80, 250), sub_rate=0.02)
    m2 = util.sample_reads(r, gs, 300, (80, 250), sub_rate=0.02)
    m1[5] = m1[5][:60] + b"NNNRY" + m1[5][65:]
    m2[9] = m2[9].lower()
    write_fastq(tmp_path / "r_1.fastq", m1, r, tag="/1")
    write_fastq(tmp_path / "r_2.fastq", m2, r, tag="/2")
    for n in ("r_1", "r_2"):
        (tmp_path / (n + ".fastq.gz")).write_bytes(gzip.compress((tmp_path / (n + ".fastq")).read_bytes(), 6))
    for ext in (".fastq", ".fastq.gz"):
        for env in ({}, {"CHARON_BATCH_READS": "37"}):
            both(tmp_path, ["--db", IDX, "-t", "4", str(tmp_path / ("r_1" + ext)), str(tmp_path / ("r_2" + ext))], env, tag="pair" + ext + "_".join(env))
    # charon classify with a parametric model
    both(tmp_path, ["--db", IDX, "--dist", "gamma", str(tmp_path / "a.fastq.gz")], sub="classify", tag="cls")
    both(tmp_path, ["--db", IDX, "--dist", "gamma", str(tmp_path / "a.fastq")], {"CHARON_BATCH_READS": "64"}, sub="classify", tag="cls64")


def test_text_switch_extract_and_training(tmp_path):
    args = ["--db", IDX, "--extract", "microbial", "--num_reads_to_fit", "20", FQ]
    out = both(tmp_path, args, {"CHARON_BATCH_READS": "64"}, tag="ext")
    assert_same_tsv(out, open(os.path.join(G, "cfg1_expected_extract.tsv")).read())
    files = {}
    for d in ("ext_packed", "ext_text"):
        files[d] = {f: gzip.decompress((tmp_path / d / f).read_bytes()) for f in sorted(os.listdir(tmp_path / d)) if f.endswith(".gz")}
    assert files["ext_packed"] and files["ext_packed"] == files["ext_text"]
    assert any(len(v) > 0 for v in files["ext_text"].values())


def test_text_switch_illegal_letter_and_bad_value(tmp_path):
    r = util.rng(32)
    reads = util.sample_reads(r, genomes(), 200, (100, 400))
    reads[150] = reads[150][:30] + b"X" + reads[150][31:]
    write_fastq(tmp_path / "bad.fastq", reads, r)
    (tmp_path / "bad.fastq.gz").write_bytes(gzip.compress((tmp_path / "bad.fastq").read_bytes(), 6))
    for f in ("bad.fastq", "bad.fastq.gz"):
        for env in ({}, {"CHARON_BATCH_READS": "64"}, {"CHARON_DEVICES": "0,0", "CHARON_BATCH_READS": "64"}):
            rc0, out0, err0 = run_cli(["--db", IDX, str(tmp_path / f)], str(tmp_path / "bad0"), env)
            rc1, out1, err1 = run_cli(["--db", IDX, str(tmp_path / f)], str(tmp_path / "bad1"), dict(env, CHARON_TEXT_BATCHES="1"))
            assert rc0 == 1 and rc1 == rc0, (rc0, rc1, err1)
            assert "parse error: illegal character in a sequence" in err0
            assert err1 == err0, (err0, err1)
            # no row of the offending batch or of a later one
            assert "read150\t" not in out1 and "read199\t" not in out1
    # anything but unset / 0 / 1: exit status 1 before the index file is opened
    (tmp_path / "junk.idx").write_bytes(b"not an index")
    for v in ("2", "", "yes", "01"):
        rc, out, err = run_cli(["--db", str(tmp_path / "junk.idx"), FQ], str(tmp_path / "v"), {"CHARON_TEXT_BATCHES": v})
        assert rc == 1 and out == "" and "charon: CHARON_TEXT_BATCHES: " in err and "junk.idx" not in err, (v, err)
    rc, out, err = run_cli(["--db", IDX, FQ], str(tmp_path / "v0"), {"CHARON_TEXT_BATCHES": "0"})
    assert rc == 0 and "CHARON_TEXT_BATCHES=1" not in open(tmp_path / "v0" / "charon.log").read()
