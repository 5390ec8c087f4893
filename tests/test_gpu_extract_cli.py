"""GPU tests (-m gpu) of CHARON_GPU_EXTRACT=1 in the front end: under --extract the device-resident loop forms the records of the
reads it calls in device memory and compresses them there (chn_extract); only BGZF members come down.

Every case runs the command line twice with CHARON_GPU_TEXT=1 CHARON_GPU_DEFLATE=1, once with CHARON_GPU_EXTRACT=1 added.  The
TSV, stderr without the timing lines and the extract files -- their compressed bytes, not only their text -- must be the same."""
import gzip
import os
import re

import pytest

from tests import util
from tests.test_gpu_cli import assert_same_tsv
from tests.test_gpu_text_cli import genomes
from tests.test_gpu_text_pairs_cli import pair_records, sample_pairs, write_pair
from tests.test_gpu_text_resident_cli import G, IDX, LEFT, awkward_reads, bgzf, fastq, golden_text, log_of, no_timing, run_cli

pytestmark = pytest.mark.gpu
BASE = {"CHARON_GPU_TEXT": "1", "CHARON_GPU_DEFLATE": "1", "CHARON_TIMING": "1"}
APPLIED = "CHARON_GPU_EXTRACT=1: the records of the extract files are formed"
LINE = re.compile(r"timing \(CHARON_GPU_EXTRACT=1\): records formed on the device (\d+)  bytes appended from the host (\d+)  compressed bytes down (\d+)  "
                  r"seconds in chn_extract calls [\d.]+")
TEXT_LINE = re.compile(r"records split (\d+)  records fetched (\d+)  text bytes inflated (\d+)  text bytes fetched (\d+)")


def extract_files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".gz")}


def records_in(files):
    return sum(gzip.decompress(v).count(b"\n") // 4 for v in files.values())


def both(tmp_path, args, env=None, tag="x", rows=10, sub="dehost", files=1):
    """the run without CHARON_GPU_EXTRACT and with it: the same TSV, stderr and extract files; returns (TSV, the files, the counters
    of the switch's timing line: records formed on the device, bytes appended from the host, compressed bytes down)"""
    e0 = dict(BASE, **(env or {}))
    rc0, out0, err0 = run_cli(args, str(tmp_path / (tag + "_off")), e0, sub=sub)
    rc1, out1, err1 = run_cli(args, str(tmp_path / (tag + "_on")), dict(e0, CHARON_GPU_EXTRACT="1"), sub=sub)
    assert rc0 == 0 and rc1 == 0, (err0, err1)
    assert out0.count("\n") > rows and out1 == out0, (args, env)
    assert no_timing(err1) == no_timing(err0)
    f0, f1 = extract_files(tmp_path / (tag + "_off")), extract_files(tmp_path / (tag + "_on"))
    assert len(f0) >= files and sorted(f0) == sorted(f1)
    for name in f0:
        assert f1[name] == f0[name], (name, len(f0[name]), len(f1[name]))  # the compressed bytes
        gzip.decompress(f1[name])
    log = log_of(tmp_path, tag + "_on")
    assert APPLIED in log and "CHARON_GPU_EXTRACT" not in log_of(tmp_path, tag + "_off")
    m = LINE.search(log)
    assert m, log
    down = sum(len(v) - 28 for v in f1.values())  # all but the end-of-file markers came down from the device
    assert int(m.group(3)) == down, (m.groups(), down)
    return out0, f1, tuple(int(x) for x in m.groups())


def test_golden_reads(tmp_path):
    (tmp_path / "g.fastq.gz").write_bytes(bgzf(golden_text()))
    for t in ("1", "8"):
        args = ["--db", IDX, "-t", t, "--extract", "microbial", "--num_reads_to_fit", "20", str(tmp_path / "g.fastq.gz")]
        out, files, (formed, from_host, down) = both(tmp_path, args, {"CHARON_BATCH_READS": "64"}, tag="golden_t" + t)
        assert_same_tsv(out, open(os.path.join(G, "cfg1_expected_extract.tsv")).read())
        assert formed > 0 and from_host > 0 and down > 0  # flights on either path
        assert LEFT not in log_of(tmp_path, "golden_t%s_on" % t)


@pytest.mark.parametrize("what", ["all", "microbial"])
def test_host_path_and_device_path_flights_straddling_everything(tmp_path, what):
    # members of 300..700 bytes, batches of 37 reads, blocks of 1 MiB: records straddle members, blocks and pieces of the extract files
    text = golden_text() * 8
    (tmp_path / "s.fastq.gz").write_bytes(bgzf(text, util.rng(5), 300, 700))
    env = {"CHARON_BATCH_READS": "37", "CHARON_BATCH_BASES": str(1 << 20)}
    args = ["--db", IDX, "-t", "4", "--extract", what, "--num_reads_to_fit", "20", str(tmp_path / "s.fastq.gz")]
    out, files, (formed, from_host, down) = both(tmp_path, args, env, tag="straddle", files=1 if what != "all" else 2)
    assert records_in(files) // 2 < formed < records_in(files) and from_host > 0
    total = sum(len(gzip.decompress(v)) for v in files.values())
    assert total > 3 * 65280 and from_host * 4 < total  # most of the files' text never was on the host


def test_a_run_too_short_for_final_models_stays_on_the_host_path(tmp_path):
    text = b"\n".join(golden_text().split(b"\n")[:4 * 60]) + b"\n"  # 60 reads against the default --num_reads_to_fit of 5 000
    (tmp_path / "few.fastq.gz").write_bytes(bgzf(text))
    out, files, (formed, from_host, down) = both(tmp_path, ["--db", IDX, "--extract", "all", str(tmp_path / "few.fastq.gz")], tag="few", files=2)
    assert formed == 0 and from_host == sum(len(gzip.decompress(v)) for v in files.values())


def test_awkward_reads_and_crlf(tmp_path):
    r = util.rng(41)
    reads = awkward_reads(r, 1200)  # N, IUPAC, lower case, U, a 200 kb read, reads shorter than k
    (tmp_path / "a.fastq.gz").write_bytes(bgzf(b"".join(fastq(reads, r))))
    (tmp_path / "c.fastq.gz").write_bytes(bgzf(b"".join(fastq(reads[:400], r, eol="\r\n"))))
    for f, env in (("a", {}), ("a", {"CHARON_BATCH_READS": "300"}), ("c", {"CHARON_BATCH_READS": "100"})):
        args = ["--db", IDX, "-t", "4", "--extract", "all", "--num_reads_to_fit", "20", str(tmp_path / (f + ".fastq.gz"))]
        out, files, (formed, from_host, down) = both(tmp_path, args, env, tag=f + "_".join(env), files=2)
        # (without a batch limit the whole file is one flight, submitted while the models train: the host path)
        assert 0 < formed < records_in(files) if env else formed == 0
        assert all(b"\r" not in gzip.decompress(v) for v in files.values())
        assert LEFT not in log_of(tmp_path, f + "_".join(env) + "_on")


def test_pairs(tmp_path):
    r = util.rng(55)
    reads, mates = sample_pairs(r, 3000)
    a, b = pair_records(reads, mates, r)
    f = write_pair(tmp_path, "e", a, b, r=r, lo=300, hi=700)  # file 2 is cut differently from file 1
    args = ["--db", IDX, "-t", "4", "--extract", "all", "--num_reads_to_fit", "20"] + f
    env = {"CHARON_GPU_TEXT_PAIRS": "1", "CHARON_BATCH_READS": "64"}
    out, files, (formed, from_host, down) = both(tmp_path, args, env, tag="pairs", rows=2990, files=4)
    assert records_in(files) // 2 < formed < records_in(files) and any(b"/2\n" in gzip.decompress(v) for v in files.values())
    # the ids of file 2: all of them come down without the switch; with it, only those of the flights on the host path -- the first K
    # pairs -- and none once the models are final
    pat = re.compile(r"timing \(CHARON_GPU_TEXT_PAIRS=1\): pairs checked (\d+)  id bytes of file 2 downloaded (\d+)")
    off, on = (pat.search(log_of(tmp_path, "pairs_" + d)) for d in ("off", "on"))
    assert off and on and int(off.group(1)) == int(on.group(1)) == 3000
    id2 = [len(x.split(b"\n")[0]) - 1 for x in b]
    assert int(off.group(2)) == sum(id2)
    prefix = {sum(id2[:k]): k for k in range(3001)}
    assert int(on.group(2)) in prefix and 0 < prefix[int(on.group(2))] <= 1024, (on.groups(), formed)


def test_a_wrapped_record_in_the_last_of_three_blocks(tmp_path):
    r = util.rng(43)
    reads = util.sample_reads(r, genomes(), 5200, (100, 400))
    recs = fastq(reads, r)
    s, q = recs[5000].split(b"\n")[1], recs[5000].split(b"\n")[3]
    recs[5000] = b"@read5000 some text\n" + s[:60] + b"\n" + s[60:] + b"\n+\n" + q[:60] + b"\n" + q[60:] + b"\n"
    text = b"".join(recs)
    assert 2 << 20 < text.index(recs[5000]) and len(text) < 3 << 20
    (tmp_path / "w.fastq.gz").write_bytes(bgzf(text, r, 3000, 9000))
    env = {"CHARON_BATCH_BASES": str(1 << 20), "CHARON_BATCH_READS": "200"}
    args = ["--db", IDX, "-t", "4", "--extract", "all", "--num_reads_to_fit", "20", str(tmp_path / "w.fastq.gz")]
    out, files, (formed, from_host, down) = both(tmp_path, args, env, tag="wrapped", rows=5190, files=2)
    assert log_of(tmp_path, "wrapped_on").count(LEFT) == 1
    # the host parser's records (199 reads of 100 .. 400 letters behind the wrapped one) go up as bytes
    assert records_in(files) // 2 < formed < records_in(files) and from_host > 100 * 200
    assert re.search(rb"@read5[01]\d\d some text\n", b"".join(gzip.decompress(v) for v in files.values()))  # (a read behind the wrapped one)


def test_classify(tmp_path):
    (tmp_path / "g.fastq.gz").write_bytes(bgzf(golden_text() * 2))
    args = ["--db", IDX, "--extract", "all", "--num_reads_to_fit", "20", str(tmp_path / "g.fastq.gz")]
    out, files, (formed, from_host, down) = both(tmp_path, args, {"CHARON_BATCH_READS": "64"}, sub="classify", tag="cls", files=2)
    assert formed > 0


def test_bad_values_and_missing_companions(tmp_path):
    (tmp_path / "g.fastq.gz").write_bytes(bgzf(golden_text()))
    (tmp_path / "junk.idx").write_bytes(b"not an index")
    full = {"CHARON_GPU_TEXT": "1", "CHARON_GPU_DEFLATE": "1"}
    envs = [dict(full, CHARON_GPU_EXTRACT=v) for v in ("2", "", "yes", "01")]
    envs += [{"CHARON_GPU_EXTRACT": "1"}, {"CHARON_GPU_EXTRACT": "1", "CHARON_GPU_TEXT": "1"}, {"CHARON_GPU_EXTRACT": "1", "CHARON_GPU_DEFLATE": "1"},
             {"CHARON_GPU_EXTRACT": "1", "CHARON_GPU_TEXT": "0", "CHARON_GPU_DEFLATE": "1"}]
    for env in envs:  # exit status 1 before the index file is opened
        rc, out, err = run_cli(["--db", str(tmp_path / "junk.idx"), "--extract", "all", str(tmp_path / "g.fastq.gz")], str(tmp_path / "v"), env)
        assert rc == 1 and out == "" and "charon: CHARON_GPU_EXTRACT: " in err and "junk.idx" not in err, (env, err)
    # 0 is unset; without --extract, and on input the resident loop does not take, one line says so and the run goes on as ever
    args = ["--db", IDX, "--num_reads_to_fit", "20"]
    rc, ref, _ = run_cli(args + [str(tmp_path / "g.fastq.gz")], str(tmp_path / "ref"), full)
    assert rc == 0 and ref.count("\n") > 10
    rc, out, _ = run_cli(args + [str(tmp_path / "g.fastq.gz")], str(tmp_path / "zero"), dict(full, CHARON_GPU_EXTRACT="0"))
    assert rc == 0 and out == ref and "CHARON_GPU_EXTRACT" not in log_of(tmp_path, "zero")
    rc, out, _ = run_cli(args + [str(tmp_path / "g.fastq.gz")], str(tmp_path / "noext"), dict(full, CHARON_GPU_EXTRACT="1"))
    assert rc == 0 and out == ref and log_of(tmp_path, "noext").count("CHARON_GPU_EXTRACT=1 does nothing without --extract") == 1
    (tmp_path / "p.fastq").write_bytes(golden_text())
    res = {}
    for tag, env in (("plain_off", full), ("plain_on", dict(full, CHARON_GPU_EXTRACT="1"))):
        rc, out, _ = run_cli(args + ["--extract", "all", str(tmp_path / "p.fastq")], str(tmp_path / tag), env)
        assert rc == 0
        res[tag] = (out, extract_files(tmp_path / tag))
    assert res["plain_on"] == res["plain_off"] and len(res["plain_on"][1]) == 2
    log = log_of(tmp_path, "plain_on")
    assert log.count("CHARON_GPU_EXTRACT=1 does not apply") == 1 and APPLIED not in log


def test_the_text_does_not_travel_under_extract(tmp_path):
    """2 000 clean reads of 5 kb with --extract all: without the switch sequence and quality of every read come down (and go up
    again to be compressed); with it only the letters of reads the device left unsized do"""
    r = util.rng(45)
    gs = genomes()
    reads = [util.mutate(r, (g * (5000 // len(g) + 1))[:5000], 0.05) for g in (gs[int(i)] for i in r.integers(0, len(gs), 2000))]
    (tmp_path / "t.fastq.gz").write_bytes(bgzf(b"".join(fastq(reads, r))))
    # batches of 16 reads and models of 10: a flight submitted while the models train takes the host path, and few do
    args = ["--db", IDX, "-t", "4", "--extract", "all", "--num_reads_to_fit", "10", str(tmp_path / "t.fastq.gz")]
    out, files, (formed, from_host, down) = both(tmp_path, args, {"CHARON_BATCH_READS": "16"}, tag="travel", rows=1990, files=2)
    got = {}
    for d in ("off", "on"):
        m = TEXT_LINE.search(log_of(tmp_path, "travel_" + d))
        assert m, d
        got[d] = tuple(int(x) for x in m.groups())
        print(d, "records split %d, fetched %d; text bytes inflated %d, fetched %d" % got[d])
    assert got["on"][0] == got["off"][0] == 2000 and got["on"][2] > 2000 * 10000
    assert got["on"][3] * 20 <= got["on"][2]
    assert not got["off"][3] * 20 <= got["off"][2]  # without the switch the text comes down: the feature does something
