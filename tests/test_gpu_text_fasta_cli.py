"""GPU tests (-m gpu) of CHARON_GPU_TEXT_FASTA=1 (with CHARON_GPU_TEXT=1) in the front end: single-end BGZF FASTA is inflated into
device memory and stays there -- records are found and unwrapped by chn_fasta_split, submitted from the buffer of letters with
CHN_TEXT_ON_DEVICE, and the letters of the few reads the host still needs come back through chn_text_fetch.  Every case runs the CLI
with the switches unset and with both set: TSV, extract files, exit status and error text must be byte-identical."""
import gzip
import os
import re
import subprocess

import pytest

from tests import util
from tests.test_gpu_text_cli import genomes
from tests.test_gpu_text_resident_cli import EXE, G, IDX, LEFT, SWITCHES, awkward_reads, bgzf, golden_text, log_of, no_timing, run_cli

pytestmark = pytest.mark.gpu
ON = {"CHARON_GPU_TEXT": "1", "CHARON_GPU_TEXT_FASTA": "1"}
APPLIED = "CHARON_GPU_TEXT_FASTA=1: FASTA records are found and unwrapped on the device"
NOT = "CHARON_GPU_TEXT_FASTA=1 does not apply to "
MQ0 = ["--min_quality", "0"]  # (a FASTA read has mean quality 0: without this every read is left unclassified)


def fasta(reads, width=70, eol=b"\n", ids=None):
    return b"".join((b">read%d some text" % i if ids is None else ids[i]) + eol + b"".join(s[a:a + width] + eol for a in range(0, len(s), width))
                    for i, s in enumerate(reads))


def golden_reads():
    lines = golden_text().split(b"\n")
    return [b">" + i[1:] for i in lines[0::4] if i], [s for s in lines[1::4] if s]


def extract_files(tmp_path, d):
    return {f: gzip.decompress((tmp_path / d / f).read_bytes()) for f in sorted(os.listdir(tmp_path / d)) if f.endswith(".gz")}


def both(tmp_path, args, env=None, tag="x", rows=10, left=0):
    """the run with the switches unset and with both set: exit status 0, byte-identical TSV, stderr and extract files, the switch's
    log line, and how often the mode was left; returns the TSV"""
    rc0, out0, err0 = run_cli(args, str(tmp_path / (tag + "_unset")), env)
    rc1, out1, err1 = run_cli(args, str(tmp_path / (tag + "_resident")), dict(env or {}, **ON))
    assert rc0 == 0 and rc1 == 0, (err0, err1)
    assert out0.count("\n") > rows
    assert out1 == out0, (args, env)
    assert no_timing(err1) == no_timing(err0)
    log = log_of(tmp_path, tag + "_resident")
    assert APPLIED in log and NOT not in log and "CHARON_GPU_TEXT=1 does not apply" not in log
    assert log.count(LEFT) == left, log
    assert "CHARON_GPU_TEXT" not in log_of(tmp_path, tag + "_unset")
    assert extract_files(tmp_path, tag + "_unset") == extract_files(tmp_path, tag + "_resident")
    return out0


def test_fasta_golden(tmp_path):
    ids, reads = golden_reads()
    assert len(reads) == len(ids) > 100
    (tmp_path / "g.fasta.gz").write_bytes(bgzf(fasta(reads, ids=ids)))
    outs = [both(tmp_path, ["--db", IDX, "-t", t] + MQ0 + [str(tmp_path / "g.fasta.gz")], tag="golden_t" + t) for t in ("1", "8")]
    assert outs[0] == outs[1] and outs[0].count("\n") > 100


def test_fasta_records_straddle_members_blocks_and_batches(tmp_path):
    # members of 300..700 bytes: nearly every line straddles one; batches of 37 reads do not line up with anything
    ids, reads = golden_reads()
    (tmp_path / "s.fa.gz").write_bytes(bgzf(fasta(reads * 8), util.rng(5), 300, 700))
    args = ["--db", IDX, "-t", "4"] + MQ0 + [str(tmp_path / "s.fa.gz")]
    ref = both(tmp_path, args, {"CHARON_BATCH_READS": "37"}, tag="straddle")
    # blocks of 1 MiB, so that blocks end inside records; a headroom below one record's length, so that the tail of a block does not fit
    # the gap and a fresh buffer takes tail and block (and the letters a buffer of that size outside the pool)
    for headroom in ("0", "30", str(1 << 20)):
        env = {"CHARON_BATCH_READS": "37", "CHARON_BATCH_BASES": str(1 << 20), "CHARON_GPU_TEXT_HEADROOM": headroom}
        assert both(tmp_path, args, env, tag="straddle_h" + headroom) == ref


def test_fasta_awkward_reads_crlf_and_gzip_on_the_host(tmp_path):
    r = util.rng(41)
    reads = awkward_reads(r, 2000)  # N, IUPAC, lower case, shorter than k, one read of 200 kb
    (tmp_path / "a.fasta.gz").write_bytes(bgzf(fasta(reads)))
    (tmp_path / "c.fna.gz").write_bytes(bgzf(fasta(reads[:400], eol=b"\r\n")))
    (tmp_path / "w.fasta.gz").write_bytes(bgzf(fasta(reads[:400], width=1 << 30)))  # every sequence on one line
    for env in ({}, {"CHARON_GZIP_ON_HOST": "1"}, {"CHARON_BATCH_READS": "300", "CHARON_BATCH_BASES": str(1 << 20)}):
        both(tmp_path, ["--db", IDX, "-t", "4"] + MQ0 + [str(tmp_path / "a.fasta.gz")], dict(env, CHARON_TIMING="1"), tag="awk" + "_".join(env))
    m = re.search(r"records split (\d+)  records fetched (\d+)", log_of(tmp_path, "awk_resident"))
    assert m and int(m.group(1)) == 2000 and int(m.group(2)) < 100, m and m.groups()
    m = re.search(r"records split (\d+)  records fetched (\d+)", log_of(tmp_path, "awkCHARON_GZIP_ON_HOST_resident"))
    assert m and int(m.group(2)) == 2000, m and m.groups()
    both(tmp_path, ["--db", IDX, "-t", "4"] + MQ0 + [str(tmp_path / "c.fna.gz")], tag="crlf")
    both(tmp_path, ["--db", IDX, "-t", "4"] + MQ0 + [str(tmp_path / "w.fasta.gz")], tag="one_line")


def test_fasta_extract(tmp_path):
    ids, reads = golden_reads()
    (tmp_path / "g.fasta.gz").write_bytes(bgzf(fasta(reads, ids=ids)))
    args = ["--db", IDX, "--extract", "microbial", "--num_reads_to_fit", "20"] + MQ0 + [str(tmp_path / "g.fasta.gz")]
    for tag, env in (("ext", {"CHARON_BATCH_READS": "64"}), ("extd", {"CHARON_BATCH_READS": "64", "CHARON_GPU_DEFLATE": "1"})):
        both(tmp_path, args, env, tag=tag)
        files = extract_files(tmp_path, tag + "_resident")
        assert files and any(len(v) > 0 for v in files.values())
    # CHARON_GPU_EXTRACT=1 keeps saying that it does not apply to FASTA, and the files are the host's
    env = {"CHARON_BATCH_READS": "64", "CHARON_GPU_DEFLATE": "1", "CHARON_GPU_EXTRACT": "1"}
    rc, out, err = run_cli(args, str(tmp_path / "extx"), dict(env, **ON))
    assert rc == 0 and extract_files(tmp_path, "extx") == extract_files(tmp_path, "extd_unset")
    log = log_of(tmp_path, "extx")
    assert log.count("CHARON_GPU_EXTRACT=1 does not apply") == 1 and APPLIED in log


SMALL = {"CHARON_BATCH_READS": "37", "CHARON_BATCH_BASES": str(1 << 20)}


def three_hundred_reads():
    r = util.rng(43)
    reads = util.sample_reads(r, genomes(), 300, (100, 400))
    return r, reads, [fasta([s], ids=[b">read%d some text" % i]) for i, s in enumerate(reads)]


def test_fasta_end_of_the_file(tmp_path):
    r, reads, recs = three_hundred_reads()
    text = b"".join(recs)
    args = lambda f: ["--db", IDX, "-t", "4"] + MQ0 + [str(tmp_path / f)]
    small = SMALL
    # a last record without a final line feed, and blank lines behind the last record: the end-of-input flag takes them
    (tmp_path / "n.fasta.gz").write_bytes(bgzf(text[:-1], r, 3000, 9000))
    (tmp_path / "b.fasta.gz").write_bytes(bgzf(text + b"\n\r\n\n", r, 3000, 9000))
    for f in ("n", "b"):
        for env in ({}, small):
            out = both(tmp_path, args(f + ".fasta.gz"), env, tag=f + "_".join(env))
            assert "read299\t" in out


def test_fasta_leaves_the_mode(tmp_path):
    r, reads, recs = three_hundred_reads()
    text = b"".join(recs)
    args = lambda f: ["--db", IDX, "-t", "4"] + MQ0 + [str(tmp_path / f)]
    small = SMALL
    # an empty record in the middle: the mode is left, the host parser warns as ever
    empty = list(recs)
    empty[150] = b">read150 some text\n"
    (tmp_path / "e.fasta.gz").write_bytes(bgzf(b"".join(empty), r, 3000, 9000))
    for env in ({}, small):
        out = both(tmp_path, args("e.fasta.gz"), env, tag="e" + "_".join(env), left=1)
        assert "read149\t" in out and "read151\t" in out
    # a file that does not start with '>': blank lines in front (the host parser skips them), text that is no record (it fails)
    (tmp_path / "l.fasta.gz").write_bytes(bgzf(b"\n\r\n" + text, r, 3000, 9000))
    both(tmp_path, args("l.fasta.gz"), tag="l", left=1)
    (tmp_path / "x.fasta.gz").write_bytes(bgzf(b"ACGT\n" + text, r, 3000, 9000))
    rc0, out0, err0 = run_cli(args("x.fasta.gz"), str(tmp_path / "x_unset"))
    rc1, out1, err1 = run_cli(args("x.fasta.gz"), str(tmp_path / "x_resident"), ON)
    assert rc0 != 0 and rc1 == rc0 and "record does not start with '>'" in err0 and err1 == err0 and out1 == out0, (err0, err1)
    assert log_of(tmp_path, "x_resident").count(LEFT) == 1


def test_fasta_record_longer_than_a_block(tmp_path):
    r, reads, recs = three_hundred_reads()
    args = lambda f: ["--db", IDX, "-t", "4"] + MQ0 + [str(tmp_path / f)]
    # A record longer than a block (CHARON_GPU_TEXT_BLOCK, the test hook: blocks of 128 KiB): the mode is left instead of growing the
    # buffer without bound, and the host parser takes the rest.  A record longer than the headroom but shorter than a block is carried.
    g = genomes()[0]
    long_reads = reads[:40] + [util.mutate(r, (g * (300000 // len(g) + 1))[:300000], 0.05)] + reads[40:80]
    (tmp_path / "c.fasta.gz").write_bytes(bgzf(fasta(long_reads)))
    out = both(tmp_path, args("c.fasta.gz"), {"CHARON_GPU_TEXT_BLOCK": str(128 << 10)}, tag="chromosome", left=1)
    assert "read40\t" in out and "read80\t" in out
    assert both(tmp_path, args("c.fasta.gz"), {"CHARON_GPU_TEXT_BLOCK": str(512 << 10), "CHARON_GPU_TEXT_HEADROOM": "1000"}, tag="carried") == out


def test_fasta_illegal_letter(tmp_path):
    r, reads, recs = three_hundred_reads()
    args = lambda f: ["--db", IDX, "-t", "4"] + MQ0 + [str(tmp_path / f)]
    # An illegal letter: same exit status, same message.  Which of the rows in front of the offending read are printed is no property of
    # the input on either path: a run that fails in a submit drops the rows of the batches then in flight (up to three on the host path's
    # replica pipeline, up to two in the resident loop), as tests/test_gpu_text_cli.py notes for FASTQ.  So: in the first read, where no
    # row stands in front, the TSV is byte-identical; in the middle, no row of the offending read or a later one is printed and one TSV
    # is the other's beginning.
    for tag, at in (("i0", 0), ("i150", 150)):
        bad = list(recs)
        bad[at] = bad[at][:40] + b"!" + bad[at][41:]
        (tmp_path / (tag + ".fasta.gz")).write_bytes(bgzf(b"".join(bad), r, 3000, 9000))
        env = {"CHARON_BATCH_READS": "1"}
        rc0, out0, err0 = run_cli(args(tag + ".fasta.gz"), str(tmp_path / (tag + "_unset")), env)
        rc1, out1, err1 = run_cli(args(tag + ".fasta.gz"), str(tmp_path / (tag + "_resident")), dict(env, **ON))
        assert rc0 != 0 and rc1 == rc0, (rc0, rc1, err1)
        assert "illegal character in a sequence" in err0 and err1 == err0, (err0, err1)
        if at == 0:
            assert out1 == out0 == ""
        for out in (out0, out1):
            assert "read%d\t" % at not in out and "read%d\t" % (at + 1) not in out and "read299\t" not in out
        assert out0.startswith(out1) or out1.startswith(out0)
        assert at == 0 or ("read140\t" in out0 and "read140\t" in out1)
        assert APPLIED in log_of(tmp_path, tag + "_resident") and LEFT not in log_of(tmp_path, tag + "_resident")


def test_fasta_switch_does_not_apply(tmp_path):
    r = util.rng(44)
    gs = genomes()
    reads = util.sample_reads(r, gs, 200, (100, 400))
    text = fasta(reads)
    from tests.test_gpu_text_resident_cli import fastq
    (tmp_path / "q.fastq.gz").write_bytes(bgzf(b"".join(fastq(reads, r))))
    (tmp_path / "p.fasta").write_bytes(text)
    (tmp_path / "one.fasta.gz").write_bytes(gzip.compress(text, 6))
    (tmp_path / "a.fasta.gz").write_bytes(bgzf(text))
    for n in ("r_1", "r_2"):
        (tmp_path / (n + ".fasta.gz")).write_bytes(bgzf(fasta(util.sample_reads(r, gs, 100, (80, 250)), ids=[b">read%d/%s" % (i, n[-1:].encode()) for i in range(100)])))
    cases = ((["q.fastq.gz"], "not FASTA", True), (["p.fasta"], "not a .gz file", False), (["one.fasta.gz"], "one deflate stream, not BGZF", False),
             (["r_1.fasta.gz", "r_2.fasta.gz"], "paired input", False))
    for i, (files, why, fastq_resident) in enumerate(cases):
        args = ["--db", IDX, "-t", "4"] + MQ0 + [str(tmp_path / f) for f in files]
        rc0, out0, err0 = run_cli(args, str(tmp_path / ("na%d_unset" % i)))
        rc1, out1, err1 = run_cli(args, str(tmp_path / ("na%d_on" % i)), ON)
        assert rc0 == 0 and rc1 == 0 and out0.count("\n") > 10 and out1 == out0, (files, err1)
        log = log_of(tmp_path, "na%d_on" % i)
        assert log.count(NOT + str(tmp_path / files[0]) + " (" + why) == 1 and APPLIED not in log, (files, log)
        # ... and the run goes on as under CHARON_GPU_TEXT=1 alone
        assert ("CHARON_GPU_TEXT=1: BGZF text is inflated" in log) == fastq_resident
        assert ("CHARON_GPU_TEXT=1 does not apply to " + str(tmp_path / files[0]) in log) == (not fastq_resident)
    # CHARON_GPU_TEXT=1 alone keeps its line for FASTA; CHARON_NO_BGZF wins; 0 is unset
    args = ["--db", IDX] + MQ0 + [str(tmp_path / "a.fasta.gz")]
    ref = both(tmp_path, args, tag="a")
    for env, lines in (({"CHARON_GPU_TEXT": "1"}, ["CHARON_GPU_TEXT=1 does not apply to " + str(tmp_path / "a.fasta.gz") + " (not FASTQ"]),
                       (dict(ON, CHARON_NO_BGZF="1"), [NOT + str(tmp_path / "a.fasta.gz") + " (CHARON_NO_BGZF is set", "CHARON_GPU_TEXT=1 does not apply to "]),
                       (dict(ON, CHARON_GPU_TEXT_FASTA="0"), ["CHARON_GPU_TEXT=1 does not apply to " + str(tmp_path / "a.fasta.gz") + " (not FASTQ"])):
        rc, out, err = run_cli(args, str(tmp_path / "nb"), env)
        log = log_of(tmp_path, "nb")
        assert rc == 0 and out == ref and APPLIED not in log and all(x in log for x in lines), (env, log)


def test_fasta_switch_bad_values_and_charon_index(tmp_path):
    (tmp_path / "g.fasta.gz").write_bytes(bgzf(fasta(golden_reads()[1][:50])))
    (tmp_path / "junk.idx").write_bytes(b"not an index")
    # anything but unset / 0 / 1, and 1 without CHARON_GPU_TEXT=1: exit status 1 before the index file is opened
    envs = [{"CHARON_GPU_TEXT": "1", "CHARON_GPU_TEXT_FASTA": v} for v in ("2", "", "yes", "01")]
    envs += [{"CHARON_GPU_TEXT_FASTA": "1"}, {"CHARON_GPU_TEXT": "0", "CHARON_GPU_TEXT_FASTA": "1"}]
    for sub in ("dehost", "classify"):
        for env in envs:
            rc, out, err = run_cli(["--db", str(tmp_path / "junk.idx"), str(tmp_path / "g.fasta.gz")], str(tmp_path / "v"), env, sub=sub)
            assert rc == 1 and out == "" and "charon: CHARON_GPU_TEXT_FASTA: " in err and "junk.idx" not in err, (env, err)
    # 0 without CHARON_GPU_TEXT is fine (the index is then opened and refused)
    rc, out, err = run_cli(["--db", str(tmp_path / "junk.idx"), str(tmp_path / "g.fasta.gz")], str(tmp_path / "v"), {"CHARON_GPU_TEXT_FASTA": "0"})
    assert rc == 1 and "CHARON_GPU_TEXT_FASTA" not in err
    # `charon index` does not read the variable
    tsv = tmp_path / "refs.tsv"
    tsv.write_text("%s\tmicrobial\n%s\thost\n" % (os.path.join(G, "my.fasta"), os.path.join(G, "cfg1_host.fasta")))
    built = []
    for name, env in (("i_unset", {}), ("i_two", {"CHARON_GPU_TEXT_FASTA": "2"})):
        os.makedirs(tmp_path / name)
        env_all = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env_all.update(env)
        p = subprocess.run([EXE, "index", "-p", str(tmp_path / name / "x"), "--log", str(tmp_path / name / "i.log"), str(tsv)], cwd=str(tmp_path / name), env=env_all,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()
        built.append(open(tmp_path / name / "x.idx", "rb").read())
    assert built[0] == built[1] and len(built[0]) > 1000


def test_fasta_text_does_not_travel(tmp_path):
    """2 000 reads of 5 kb, A/C/G/T only: the device sizes every one of them and nothing is extracted, so no read's letters are needed
    on the host.  This is what shows that the device-resident path ran: every record was split there, and at most a twentieth of the
    inflated text came back (the bound tests/test_gpu_text_resident_cli.py holds for FASTQ at these lengths)."""
    r = util.rng(45)
    gs = genomes()
    reads = [util.mutate(r, (g * (5000 // len(g) + 1))[:5000], 0.05) for g in (gs[int(i)] for i in r.integers(0, len(gs), 2000))]
    (tmp_path / "t.fasta.gz").write_bytes(bgzf(fasta(reads)))
    both(tmp_path, ["--db", IDX, "-t", "4"] + MQ0 + [str(tmp_path / "t.fasta.gz")], {"CHARON_TIMING": "1"}, tag="travel")
    m = re.search(r"records split (\d+)  records fetched (\d+)  text bytes inflated (\d+)  text bytes fetched (\d+)  seconds in inflate [\d.]+  "
                  r"seconds in split [\d.]+  seconds in fetch [\d.]+", log_of(tmp_path, "travel_resident"))
    assert m, log_of(tmp_path, "travel_resident")
    split, fetched, inflated, fetched_bytes = (int(x) for x in m.groups())
    print("records split %d, fetched %d; text bytes inflated %d, fetched %d" % (split, fetched, inflated, fetched_bytes))
    assert split == 2000 and inflated > 2000 * 5000
    assert fetched_bytes * 20 <= inflated
