#!/usr/bin/env python3
"""The front end's whole output under a fixed table of settings, one line per setting: sha256 of the exit status, stdout, every extract
file, the log without time stamps and stderr -- log and stderr with CHARON_TIMING=1, their floating-point numbers masked (the wording
and the integer counters of the `timing (` lines, which come through chn_stream_profile, are compared).  Two builds give the same
output if and only if their lines are equal: run it once per `charon` binary (each finds the libcharon_hip.so next to it) and diff.

The settings are those of profiles/r17/dehost_stages.txt section 1, on the golden index and inputs made from the golden reads with the
builders of the CLI tests: plain, -t 1 / -t 4, CHARON_ROW_WRITER, pairs, classify, --dist gamma, text batches, CHARON_GPU_INFLATE,
CHARON_GPU_TEXT alone and with _PAIRS / _FASTA / CHARON_GPU_EXTRACT / CHARON_GPU_DEFLATE, headroom, host gzip, inputs that make the
resident loop leave the mode, damaged records and members, CHARON_DEVICES=0,0, --extract, refused options.
usage: python tools/cli_output_hashes.py /path/to/charon_amd/bin/charon workdir > hashes.txt"""
import glob
import gzip
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import util  # noqa: E402
from tests.test_gpu_text_resident_cli import bgzf, fastq, golden_text, SWITCHES  # noqa: E402
from tests.test_gpu_text_pairs_cli import pair_records, sample_pairs, write_pair  # noqa: E402
from tests.test_gpu_text_fasta_cli import fasta, golden_reads  # noqa: E402
from tests.test_gpu_text_cli import genomes  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
IDX = os.path.join(G, "cfg1.idx")
FQ = os.path.join(G, "cfg1_reads.fastq.gz")
ALL_SWITCHES = set(SWITCHES) | {"CHARON_GPU_TEXT_PAIRS", "CHARON_GPU_TEXT_FASTA", "CHARON_GPU_EXTRACT", "CHARON_GPU_TEXT_BLOCK", "CHARON_DEVICES", "CHARON_ROW_WRITER",
                                "CHARON_BATCH_READS", "CHARON_BATCH_BASES", "CHARON_GZIP_ON_HOST", "CHARON_NO_BGZF", "CHARON_TIMING", "CHARON_HIP_LIB"}
NUMBER = re.compile(r"[-+]?\d+\.\d+(e[-+]?\d+)?")
STAMP = re.compile(r"^\[?\d{4}-\d\d-\d\d[ T]\d\d:\d\d:\d\d[^ ]*\]? ?")


def masked(text, names):
    """time stamps off, the names of the working directory and of the build's own directory out, every floating-point number masked
    (times, rates; the integer counters stay)"""
    for i, name in enumerate(names):
        text = text.replace(name, "<dir%d>" % i)
    return "\n".join(NUMBER.sub("#", STAMP.sub("", line)) for line in text.splitlines()).encode()


def run(exe, work, name, sub, args, env_extra):
    d = os.path.join(work, "run_" + name)
    os.makedirs(d, exist_ok=True)
    env = {k: v for k, v in os.environ.items() if k not in ALL_SWITCHES}
    env.update(env_extra, CHARON_TIMING="1")
    p = subprocess.run([exe, sub] + args + ["--log", os.path.join(d, "charon.log")], cwd=d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    names = (work, os.path.dirname(os.path.dirname(exe)))
    log = open(os.path.join(d, "charon.log")).read() if os.path.exists(os.path.join(d, "charon.log")) else ""
    files = sorted(f for f in glob.glob(os.path.join(d, "*")) if not f.endswith("charon.log"))
    parts = [("exit", str(p.returncode).encode()), ("stdout", p.stdout), ("log", masked(log, names)), ("stderr", masked(p.stderr.decode(errors="replace"), names))]
    for f in files:
        data = open(f, "rb").read()
        parts.append((os.path.basename(f), gzip.decompress(data) if f.endswith(".gz") and data[:2] == b"\x1f\x8b" else data))
        parts.append((os.path.basename(f) + " as written", data))
    if p.returncode < 0:
        raise SystemExit("%s: ended by signal %d" % (name, -p.returncode))
    print("%-40s exit %-3d stdout %7d bytes  extract files %d  %s" % (name, p.returncode, len(p.stdout), len(files),
                                                                     " ".join("%s:%s" % (k, hashlib.sha256(v).hexdigest()[:12]) for k, v in parts)), flush=True)


def main():
    exe, work = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    inp = os.path.join(work, "inputs")
    os.makedirs(inp, exist_ok=True)
    from pathlib import Path
    P = Path(inp)
    r = util.rng(1817)
    text = golden_text()
    (P / "g.fastq.gz").write_bytes(bgzf(text))
    (P / "s.fastq.gz").write_bytes(bgzf(text * 8, r, 300, 700))
    ids, seqs = golden_reads()
    (P / "g.fasta.gz").write_bytes(bgzf(fasta(seqs, ids=ids)))
    pairs = write_pair(P, "p", *pair_records(*sample_pairs(r, 300), r))
    recs1, recs2 = pair_records(*sample_pairs(r, 300), r)
    (P / "n_1.fastq.gz").write_bytes(gzip.compress(b"".join(recs1)))
    (P / "n_2.fastq.gz").write_bytes(gzip.compress(b"".join(recs2)))
    plain_pairs = [str(P / "n_1.fastq.gz"), str(P / "n_2.fastq.gz")]
    reads = util.sample_reads(r, genomes(), 300, (100, 400))
    recs = fastq(reads, r)
    s, q = recs[150].split(b"\n")[1], recs[150].split(b"\n")[3]
    wrapped = list(recs)
    wrapped[150] = b"@read150 some text\n" + s[:60] + b"\n" + s[60:] + b"\n+\n" + q[:60] + b"\n" + q[60:] + b"\n"
    (P / "w.fastq.gz").write_bytes(bgzf(b"".join(wrapped), r, 3000, 9000))
    damaged = list(recs)
    damaged[150] = b"X" + damaged[150][1:]
    (P / "d.fastq.gz").write_bytes(bgzf(b"".join(damaged), r, 3000, 9000))
    fa = [b">read%d some text\n" % i + x + b"\n" for i, x in enumerate(reads)]
    fa[150] = b">read150 some text\n"   # an empty record in the middle: the FASTA loop leaves the mode
    (P / "w.fasta.gz").write_bytes(bgzf(b"".join(fa), r, 3000, 9000))

    g, sfq, gfa = str(P / "g.fastq.gz"), str(P / "s.fastq.gz"), str(P / "g.fasta.gz")
    db = ["--db", IDX]
    T, TP, TF = {"CHARON_GPU_TEXT": "1"}, {"CHARON_GPU_TEXT": "1", "CHARON_GPU_TEXT_PAIRS": "1"}, {"CHARON_GPU_TEXT": "1", "CHARON_GPU_TEXT_FASTA": "1"}
    BLK = {"CHARON_GPU_TEXT_BLOCK": "65536"}
    SMALL = {"CHARON_BATCH_READS": "37", "CHARON_BATCH_BASES": str(1 << 20)}
    X = ["--extract", "all", "--num_reads_to_fit", "20"]
    MQ0 = ["--min_quality", "0"]  # (a FASTA read has mean quality 0)
    table = [
        ("plain", "dehost", db + [FQ], {}),
        ("plain_small", "dehost", db + ["-t", "4", FQ], {"CHARON_BATCH_READS": "37"}),
        ("plain_t1", "dehost", db + ["-t", "1", FQ], {}),
        ("row_writer_0", "dehost", db + [FQ], {"CHARON_ROW_WRITER": "0"}),
        ("row_writer_1", "dehost", db + [FQ], {"CHARON_ROW_WRITER": "1"}),
        ("paired", "dehost", db + plain_pairs, {}),
        ("classify", "classify", db + [FQ], {}),
        ("dehost_gamma", "dehost", db + ["--dist", "gamma", FQ], {}),
        ("text_batches", "dehost", db + [FQ], {"CHARON_TEXT_BATCHES": "1"}),
        ("text_batches_paired", "dehost", db + plain_pairs, {"CHARON_TEXT_BATCHES": "1"}),
        ("gpu_inflate", "dehost", db + ["-t", "4", sfq], dict(SMALL, CHARON_GPU_INFLATE="1")),
        ("resident", "dehost", db + ["-t", "4", sfq], dict(SMALL, **T)),
        ("resident_block", "dehost", db + ["-t", "4", sfq], dict(T, **BLK)),
        ("resident_host_gzip", "dehost", db + ["-t", "4", sfq], dict(SMALL, CHARON_GZIP_ON_HOST="1", **T)),
        ("resident_headroom30", "dehost", db + ["-t", "4", sfq], dict(SMALL, CHARON_GPU_TEXT_HEADROOM="30", **T)),
        ("resident_pairs", "dehost", db + ["-t", "4"] + pairs, dict(TP, **BLK)),
        ("resident_pairs_small", "dehost", db + ["-t", "4"] + pairs, dict(SMALL, **TP)),
        ("resident_pairs_not_bgzf", "dehost", db + plain_pairs, TP),
        ("resident_pairs_classify", "classify", db + pairs, TP),
        ("resident_fasta", "dehost", db + ["-t", "4"] + MQ0 + [gfa], dict(TF, **BLK)),
        ("resident_fasta_on_fastq", "dehost", db + ["-t", "4", sfq], dict(SMALL, **TF)),
        ("resident_leaves", "dehost", db + ["-t", "4", str(P / "w.fastq.gz")], dict(SMALL, **T)),
        ("resident_fasta_leaves", "dehost", db + ["-t", "4"] + MQ0 + [str(P / "w.fasta.gz")], dict(SMALL, **TF)),
        ("resident_damaged", "dehost", db + [str(P / "d.fastq.gz")], dict(T, CHARON_BATCH_READS="1")),
        ("host_damaged", "dehost", db + [str(P / "d.fastq.gz")], {"CHARON_BATCH_READS": "1"}),
        ("devices_0_0", "dehost", db + [FQ], {"CHARON_DEVICES": "0,0", "CHARON_BATCH_READS": "37"}),
        ("devices_0_0_text_batches", "dehost", db + [FQ], {"CHARON_DEVICES": "0,0", "CHARON_BATCH_READS": "37", "CHARON_TEXT_BATCHES": "1"}),
        ("devices_0_0_damaged", "dehost", db + [str(P / "d.fastq.gz")], {"CHARON_DEVICES": "0,0", "CHARON_BATCH_READS": "1"}),
        ("devices_0_0_resident", "dehost", db + [g], dict(T, CHARON_DEVICES="0,0")),
        ("devices_out_of_range", "dehost", db + [FQ], {"CHARON_DEVICES": "0,99"}),
        ("dist_unknown", "dehost", db + ["--dist", "weibull", FQ], {}),
        ("index_missing", "dehost", ["--db", os.path.join(G, "nope.idx"), FQ], {}),
        ("extract_single", "dehost", db + X + ["-p", "x", FQ], {}),
        ("extract_paired", "dehost", db + X + ["-p", "x"] + plain_pairs, {}),
        ("extract_deflate", "dehost", db + X + ["-p", "x", FQ], {"CHARON_GPU_DEFLATE": "1"}),
        ("classify_gamma_extract", "classify", db + ["-d", "gamma"] + X + ["-p", "x", FQ], {}),
        ("resident_extract", "dehost", db + X + ["-p", "x", "-t", "4", sfq], dict(T, CHARON_GPU_EXTRACT="1", CHARON_GPU_DEFLATE="1", **BLK)),
        ("resident_extract_pairs", "dehost", db + X + ["-p", "x", "-t", "4"] + pairs, dict(TP, CHARON_GPU_EXTRACT="1", CHARON_GPU_DEFLATE="1", **BLK)),
        ("resident_extract_host_records", "dehost", db + X + ["-p", "x", "-t", "4", sfq], dict(T, CHARON_GPU_DEFLATE="1", **BLK)),
        ("gpu_extract_without_extract", "dehost", db + ["-t", "4", sfq], dict(T, CHARON_GPU_EXTRACT="1", **BLK)),
        ("gpu_extract_not_resident", "dehost", db + X + ["-p", "x", FQ], {"CHARON_GPU_EXTRACT": "1"}),
        ("extract_unknown_category", "dehost", db + ["-e", "fungi", FQ], {}),
    ]
    for name, sub, args, env in table:
        run(exe, work, name, sub, args, env)
    print("done: %d settings" % len(table))


if __name__ == "__main__":
    main()
