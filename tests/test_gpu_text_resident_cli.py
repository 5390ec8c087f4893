"""GPU tests (-m gpu) of CHARON_GPU_TEXT=1 in the front end: single-end BGZF FASTQ is inflated into device memory and stays there --
records are found by chn_text_split, submitted with CHN_TEXT_ON_DEVICE, and the letters of the few reads the host still needs come
back through chn_text_fetch.  The TSV (and the extract files) must be byte-identical to the run without the switch."""
import gzip
import os
import re
import struct
import zlib

import numpy as np
import pytest

from tests import util
from tests.test_gpu_cli import assert_same_tsv
from tests.test_gpu_text_cli import genomes

pytestmark = pytest.mark.gpu
G = os.path.join(util.ROOT, "tests", "golden")
EXE = os.path.join(util.ROOT, "charon_amd", "bin", "charon")
IDX = os.path.join(G, "cfg1.idx")
FQ = os.path.join(G, "cfg1_reads.fastq.gz")
SWITCHES = ("CHARON_GPU_TEXT", "CHARON_GPU_TEXT_HEADROOM", "CHARON_GPU_INFLATE", "CHARON_GPU_DEFLATE", "CHARON_TEXT_BATCHES")
APPLIED = "CHARON_GPU_TEXT=1: "
LEFT = "CHARON_GPU_TEXT=1: leaving the device-resident path"


def run_cli(args, cwd, env_extra=None, sub="dehost"):
    import subprocess
    os.makedirs(cwd, exist_ok=True)
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra or {})
    p = subprocess.run([EXE, sub] + args + ["--log", os.path.join(cwd, "charon.log")], cwd=cwd, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def both(tmp_path, args, env=None, tag="x", rows=10):
    """the run without the switch and with it: exit status 0, byte-identical TSV and stderr, the switch's log line; returns the TSV"""
    rc0, out0, err0 = run_cli(args, str(tmp_path / (tag + "_unset")), env)
    rc1, out1, err1 = run_cli(args, str(tmp_path / (tag + "_resident")), dict(env or {}, CHARON_GPU_TEXT="1"))
    assert rc0 == 0 and rc1 == 0, (err0, err1)
    assert out0.count("\n") > rows
    assert out1 == out0, (args, env)
    assert no_timing(err1) == no_timing(err0)
    assert APPLIED in log_of(tmp_path, tag + "_resident")
    assert "CHARON_GPU_TEXT" not in log_of(tmp_path, tag + "_unset")
    return out0


def no_timing(err):
    return [line for line in err.splitlines() if not line.startswith("charon: timing")]


def log_of(tmp_path, d):
    return open(tmp_path / d / "charon.log").read()


def bgzf(data, r=None, lo=65280, hi=65280):
    """`data` as BGZF members of lo..hi bytes of text each, with the end-of-file marker"""
    out, at = [], 0
    while True:
        c = data[at:at + (lo if r is None else int(r.integers(lo, hi + 1)))]
        at += len(c)
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        z = co.compress(c) + co.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 12 + 6 + len(z) + 8 - 1) + z +
                   struct.pack("<II", zlib.crc32(c) & 0xFFFFFFFF, len(c)))
        if not c:
            return b"".join(out)


def fastq(reads, r, eol="\n", lo=5, hi=41):
    parts = []
    for i, s in enumerate(reads):
        q = (r.integers(lo, hi, len(s)) + 33).astype(np.uint8).tobytes()
        parts.append(b"@read%d some text" % i + eol.encode() + s + eol.encode() + b"+" + eol.encode() + q + eol.encode())
    return parts


def golden_text():
    return gzip.decompress(open(FQ, "rb").read())


def test_resident_golden(tmp_path):
    (tmp_path / "g.fastq.gz").write_bytes(bgzf(golden_text()))
    for t in ("1", "8"):
        out = both(tmp_path, ["--db", IDX, "-t", t, str(tmp_path / "g.fastq.gz")], tag="golden_t" + t)
        assert_same_tsv(out, open(os.path.join(G, "cfg1_expected.tsv")).read())
        assert LEFT not in log_of(tmp_path, "golden_t%s_resident" % t)


def test_resident_records_straddle_members_blocks_and_batches(tmp_path):
    # members of 300..700 bytes: nearly every record straddles one; batches of 37 reads do not line up with anything
    text = golden_text() * 8  # 3.2 MB: four blocks of 1 MiB below
    (tmp_path / "s.fastq.gz").write_bytes(bgzf(text, util.rng(5), 300, 700))
    ref = both(tmp_path, ["--db", IDX, "-t", "4", str(tmp_path / "s.fastq.gz")], {"CHARON_BATCH_READS": "37"}, tag="straddle")
    # blocks of 1 MiB (the block size follows CHARON_BATCH_BASES), so that blocks end inside records; a headroom below one record's
    # length, so that the tail of a block does not fit the gap and a fresh buffer takes tail and block
    for headroom in ("0", "30", str(1 << 20)):
        env = {"CHARON_BATCH_READS": "37", "CHARON_BATCH_BASES": str(1 << 20), "CHARON_GPU_TEXT_HEADROOM": headroom}
        assert both(tmp_path, ["--db", IDX, "-t", "4", str(tmp_path / "s.fastq.gz")], env, tag="straddle_h" + headroom) == ref
        assert LEFT not in log_of(tmp_path, "straddle_h%s_resident" % headroom)


def awkward_reads(r, n):
    gs = genomes()
    reads = util.sample_reads(r, gs, n, (30, 900), sub_rate=0.03)
    reads[3] = reads[3].lower()
    reads[4] = b"N" * 200
    reads[5] = reads[5][:50] + b"NNNNNRYKMnnnswbdhv" + reads[5][68:]
    reads[6] = reads[6][:17].lower() + reads[6][17:]
    reads[7] = b"ACGU" + reads[7].replace(b"T", b"U")[4:]
    reads[8] = util.mutate(r, (gs[0] * (200000 // len(gs[0]) + 1))[:200001], 0.05)  # beyond every device limit of the gzip column
    for i in range(9, 15):
        reads[i] = reads[i][:3 + i]  # shorter than k
    for i in range(20, 60):
        b = bytearray(reads[i])
        for at in r.integers(0, len(b), max(1, len(b) // 10)):
            b[int(at)] = ord("N")
        reads[i] = bytes(b)
    return reads


def test_resident_host_gzip_fallback_and_crlf(tmp_path):
    r = util.rng(41)
    reads = awkward_reads(r, 2000)
    (tmp_path / "a.fastq.gz").write_bytes(bgzf(b"".join(fastq(reads, r))))
    (tmp_path / "c.fastq.gz").write_bytes(bgzf(b"".join(fastq(reads[:400], r, eol="\r\n"))))
    for env in ({}, {"CHARON_GZIP_ON_HOST": "1"}, {"CHARON_BATCH_READS": "300"}):
        both(tmp_path, ["--db", IDX, "-t", "4", str(tmp_path / "a.fastq.gz")], dict(env, CHARON_TIMING="1"), tag="awk" + "_".join(env))
    # only reads the device leaves unsized come down through the fetch (the 200 kb read where the routing keeps it on the host, a read
    # of a second deflate block); with the whole gzip column on the host every read does
    m = re.search(r"records split (\d+)  records fetched (\d+)", log_of(tmp_path, "awk_resident"))
    assert m and int(m.group(1)) == 2000 and int(m.group(2)) < 100, m and m.groups()
    m = re.search(r"records split (\d+)  records fetched (\d+)", log_of(tmp_path, "awkCHARON_GZIP_ON_HOST_resident"))
    assert m and int(m.group(2)) == 2000, m and m.groups()
    both(tmp_path, ["--db", IDX, "-t", "4", str(tmp_path / "c.fastq.gz")], tag="crlf")
    assert LEFT not in log_of(tmp_path, "crlf_resident")


def test_resident_extract(tmp_path):
    (tmp_path / "g.fastq.gz").write_bytes(bgzf(golden_text()))
    args = ["--db", IDX, "--extract", "microbial", "--num_reads_to_fit", "20", str(tmp_path / "g.fastq.gz")]
    for tag, env in (("ext", {"CHARON_BATCH_READS": "64"}), ("extd", {"CHARON_BATCH_READS": "64", "CHARON_GPU_DEFLATE": "1"})):
        out = both(tmp_path, args, env, tag=tag)
        assert_same_tsv(out, open(os.path.join(G, "cfg1_expected_extract.tsv")).read())
        files = {}
        for d in (tag + "_unset", tag + "_resident"):
            files[d] = {f: gzip.decompress((tmp_path / d / f).read_bytes()) for f in sorted(os.listdir(tmp_path / d)) if f.endswith(".gz")}
        assert files[tag + "_unset"] and files[tag + "_unset"] == files[tag + "_resident"]
        assert any(len(v) > 0 for v in files[tag + "_resident"].values())


def test_resident_leaves_the_mode(tmp_path):
    r = util.rng(43)
    reads = util.sample_reads(r, genomes(), 300, (100, 400))
    recs = fastq(reads, r)
    # a wrapped record in the middle of the file
    s, q = recs[150].split(b"\n")[1], recs[150].split(b"\n")[3]
    wrapped = list(recs)
    wrapped[150] = b"@read150 some text\n" + s[:60] + b"\n" + s[60:] + b"\n+\n" + q[:60] + b"\n" + q[60:] + b"\n"
    (tmp_path / "w.fastq.gz").write_bytes(bgzf(b"".join(wrapped), r, 3000, 9000))
    # a last record without a line feed
    (tmp_path / "n.fastq.gz").write_bytes(bgzf(b"".join(recs)[:-1], r, 3000, 9000))
    for f in ("w", "n"):
        for env in ({}, {"CHARON_BATCH_READS": "37", "CHARON_BATCH_BASES": str(1 << 20)}):
            tag = f + "_".join(env)
            both(tmp_path, ["--db", IDX, "-t", "4", str(tmp_path / (f + ".fastq.gz"))], env, tag=tag)
            assert log_of(tmp_path, tag + "_resident").count(LEFT) == 1
    # A record damaged in the middle of the file: same exit status, same message, same rows.  (The reader drops the whole block that holds
    # the damage, so which rows a run prints before it fails follows from its blocks; blocks of one record make that the same everywhere.)
    damaged = list(recs)
    damaged[150] = b"X" + damaged[150][1:]
    (tmp_path / "d.fastq.gz").write_bytes(bgzf(b"".join(damaged), r, 3000, 9000))
    env = {"CHARON_BATCH_READS": "1"}
    rc0, out0, err0 = run_cli(["--db", IDX, str(tmp_path / "d.fastq.gz")], str(tmp_path / "d_unset"), env)
    rc1, out1, err1 = run_cli(["--db", IDX, str(tmp_path / "d.fastq.gz")], str(tmp_path / "d_resident"), dict(env, CHARON_GPU_TEXT="1"))
    assert rc0 != 0 and rc1 == rc0, (rc0, rc1, err1)
    assert "record does not start with '@'" in err0 and err1 == err0, (err0, err1)
    assert out1 == out0 and "read148\t" in out0 and "read150\t" not in out0
    assert log_of(tmp_path, "d_resident").count(LEFT) == 1


def test_resident_corrupt_member(tmp_path):
    z = bytearray(bgzf(golden_text(), util.rng(6), 20000, 30000))
    # a payload bit of the member in the middle of the file
    at, starts = 0, []
    while at < len(z):
        starts.append(at)
        at += struct.unpack_from("<H", z, at + 16)[0] + 1
    z[starts[len(starts) // 2] + 18 + 40] ^= 0x10
    (tmp_path / "bad.fastq.gz").write_bytes(bytes(z))
    for env in ({}, {"CHARON_GPU_TEXT": "1"}):
        rc, out, err = run_cli(["--db", IDX, str(tmp_path / "bad.fastq.gz")], str(tmp_path / ("bad" + "_".join(env))), env)
        assert rc == 1 and "a BGZF member is corrupt" in err, (env, rc, err)


def test_resident_does_not_apply(tmp_path):
    r = util.rng(44)
    gs = genomes()
    reads = util.sample_reads(r, gs, 200, (100, 400))
    text = b"".join(fastq(reads, r))
    (tmp_path / "p.fastq").write_bytes(text)
    (tmp_path / "one.fastq.gz").write_bytes(gzip.compress(text, 6))
    (tmp_path / "a.fasta.gz").write_bytes(bgzf(b"".join(b">read%d x\n%s\n" % (i, s) for i, s in enumerate(reads))))
    m1, m2 = util.sample_reads(r, gs, 100, (80, 250)), util.sample_reads(r, gs, 100, (80, 250))
    for n, m in (("r_1", m1), ("r_2", m2)):
        (tmp_path / (n + ".fastq.gz")).write_bytes(bgzf(b"".join(x.replace(b" some text", b"/" + n[-1:].encode()) for x in fastq(m, r))))
    (tmp_path / "b.fastq.gz").write_bytes(bgzf(text))
    cases = (["p.fastq"], ["one.fastq.gz"], ["a.fasta.gz"], ["r_1.fastq.gz", "r_2.fastq.gz"])
    for i, files in enumerate(cases):
        args = ["--db", IDX, "-t", "4"] + [str(tmp_path / f) for f in files]
        rc0, out0, err0 = run_cli(args, str(tmp_path / ("na%d_unset" % i)))
        rc1, out1, err1 = run_cli(args, str(tmp_path / ("na%d_on" % i)), {"CHARON_GPU_TEXT": "1"})
        assert rc0 == 0 and rc1 == 0 and out0.count("\n") > 10 and out1 == out0, (files, err1)
        log = log_of(tmp_path, "na%d_on" % i)
        assert "CHARON_GPU_TEXT=1 does not apply to " + str(tmp_path / files[0]) in log and APPLIED not in log, files
    # CHARON_NO_BGZF wins; 0 is unset
    ref = both(tmp_path, ["--db", IDX, str(tmp_path / "b.fastq.gz")], tag="b")
    for env in ({"CHARON_GPU_TEXT": "1", "CHARON_NO_BGZF": "1"}, {"CHARON_GPU_TEXT": "0"}):
        rc, out, err = run_cli(["--db", IDX, str(tmp_path / "b.fastq.gz")], str(tmp_path / "nb"), env)
        assert rc == 0 and out == ref and APPLIED not in log_of(tmp_path, "nb"), env


def test_resident_bad_values(tmp_path):
    (tmp_path / "g.fastq.gz").write_bytes(bgzf(golden_text()))
    (tmp_path / "junk.idx").write_bytes(b"not an index")
    # anything but unset / 0 / 1, and several replicas: exit status 1 before the index file is opened
    for env in [{"CHARON_GPU_TEXT": v} for v in ("2", "", "yes", "01")] + [{"CHARON_GPU_TEXT": "1", "CHARON_DEVICES": "0,0"}]:
        rc, out, err = run_cli(["--db", str(tmp_path / "junk.idx"), str(tmp_path / "g.fastq.gz")], str(tmp_path / "v"), env)
        assert rc == 1 and out == "" and "charon: CHARON_GPU_TEXT: " in err and "junk.idx" not in err, (env, err)
    # one entry is one device
    both(tmp_path, ["--db", IDX, str(tmp_path / "g.fastq.gz")], {"CHARON_DEVICES": "0"}, tag="one")


def test_resident_text_does_not_travel(tmp_path):
    """2 000 reads of 5 kb, A/C/G/T only: the device sizes every one of them and nothing is extracted, so no read's letters are needed
    on the host (rows and cached entries are made of the id and the result columns: make_entry copies letters under --extract only)."""
    r = util.rng(45)
    gs = genomes()
    reads = [util.mutate(r, (g * (5000 // len(g) + 1))[:5000], 0.05) for g in (gs[int(i)] for i in r.integers(0, len(gs), 2000))]
    (tmp_path / "t.fastq.gz").write_bytes(bgzf(b"".join(fastq(reads, r))))
    both(tmp_path, ["--db", IDX, "-t", "4", str(tmp_path / "t.fastq.gz")], {"CHARON_TIMING": "1"}, tag="travel")
    m = re.search(r"records split (\d+)  records fetched (\d+)  text bytes inflated (\d+)  text bytes fetched (\d+)  seconds in inflate [\d.]+  "
                  r"seconds in split [\d.]+  seconds in fetch [\d.]+", log_of(tmp_path, "travel_resident"))
    assert m, log_of(tmp_path, "travel_resident")
    split, fetched, inflated, fetched_bytes = (int(x) for x in m.groups())
    print("records split %d, fetched %d; text bytes inflated %d, fetched %d" % (split, fetched, inflated, fetched_bytes))
    assert split == 2000 and inflated > 2000 * 10000
    assert fetched_bytes * 20 <= inflated
