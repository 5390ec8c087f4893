"""GPU tests (-m gpu) of CHARON_GPU_TEXT_PAIRS=1 (together with CHARON_GPU_TEXT=1) in the front end: both files of paired BGZF FASTQ
are inflated into device memory and stay there -- records found by chn_text_split per file, the ids of a pair compared by
chn_text_pair_ids, batches over two device texts, letters fetched only where the host still needs them.

Every case runs the CLI twice -- with both switches unset and with both set -- and compares TSV and stderr (without the lines that
start with `charon: timing`) byte for byte.  No case runs the CLI into the id-mismatch abort: that is tested at the ABI
(tests/test_gpu_text_pair.py), where a mismatch is a returned index."""
import gzip
import os
import re
import struct

import numpy as np
import pytest

from tests import util
from tests.test_gpu_text_cli import genomes
from tests.test_gpu_text_resident_cli import G, IDX, LEFT, APPLIED, bgzf, fastq, log_of, no_timing, run_cli

pytestmark = pytest.mark.gpu
ON = {"CHARON_GPU_TEXT": "1", "CHARON_GPU_TEXT_PAIRS": "1"}
PAIRS_APPLIED = "CHARON_GPU_TEXT_PAIRS=1: both files"
PAIRS_NOT = "CHARON_GPU_TEXT_PAIRS=1 does not apply to "


def pair_records(reads, mates, r, eol1="\n", eol2="\n"):
    """the records of the two files: ids read<i>/1 and read<i>/2"""
    a = [x.replace(b" some text", b"/1") for x in fastq(reads, r, eol=eol1)]
    b = [x.replace(b" some text", b"/2") for x in fastq(mates, r, eol=eol2)]
    return a, b


def write_pair(tmp_path, name, recs1, recs2, r=None, lo=65280, hi=65280):
    """<name>_1.fastq.gz and <name>_2.fastq.gz as BGZF (the members of the two files cut by draws of their own); returns the two paths"""
    out = []
    for k, recs in ((1, recs1), (2, recs2)):
        p = tmp_path / ("%s_%d.fastq.gz" % (name, k))
        p.write_bytes(bgzf(b"".join(recs) if isinstance(recs, list) else recs, r, lo, hi))
        out.append(str(p))
    return out


def both(tmp_path, args, env=None, tag="x", rows=10, sub="dehost", applied=True):
    """the run with the switches unset and with both set: exit status 0, byte-identical TSV and stderr; returns the TSV"""
    rc0, out0, err0 = run_cli(args, str(tmp_path / (tag + "_unset")), env, sub=sub)
    rc1, out1, err1 = run_cli(args, str(tmp_path / (tag + "_on")), dict(env or {}, **ON), sub=sub)
    assert rc0 == 0 and rc1 == 0, (err0, err1)
    assert out0.count("\n") > rows
    assert out1 == out0, (args, env)
    assert no_timing(err1) == no_timing(err0)
    log = log_of(tmp_path, tag + "_on")
    if applied:
        assert APPLIED in log and PAIRS_APPLIED in log and PAIRS_NOT not in log
    assert "CHARON_GPU_TEXT" not in log_of(tmp_path, tag + "_unset")
    return out0


def sample_pairs(r, n, lo=80, hi=250):
    gs = genomes()
    return util.sample_reads(r, gs, n, (lo, hi), sub_rate=0.03), util.sample_reads(r, gs, n, (lo, hi), sub_rate=0.03)


def test_pairs_golden_index(tmp_path):
    r = util.rng(51)
    f = write_pair(tmp_path, "g", *pair_records(*sample_pairs(r, 300), r))
    outs = []
    for t in ("1", "8"):
        outs.append(both(tmp_path, ["--db", IDX, "-t", t] + f, tag="t" + t, rows=290))
        assert LEFT not in log_of(tmp_path, "t%s_on" % t)
    assert outs[0] == outs[1] and "read299/1\t" in outs[0]


def test_pairs_straddle_members_blocks_and_batches(tmp_path):
    # members of 300..700 bytes, cut differently in the two files; batches of 37 pairs line up with nothing; blocks of 1 MiB end inside
    # records and at different records on the two sides (the mates' records differ in size)
    r = util.rng(52)
    f = write_pair(tmp_path, "s", *pair_records(*sample_pairs(r, 6000), r), r=r, lo=300, hi=700)
    assert all(os.path.getsize(p) > 300000 for p in f)
    ref = both(tmp_path, ["--db", IDX, "-t", "4"] + f, {"CHARON_BATCH_READS": "37"}, tag="straddle", rows=5990)
    for headroom in ("0", "30", str(1 << 20)):
        env = {"CHARON_BATCH_READS": "37", "CHARON_BATCH_BASES": str(1 << 20), "CHARON_GPU_TEXT_HEADROOM": headroom}
        assert both(tmp_path, ["--db", IDX, "-t", "4"] + f, env, tag="straddle_h" + headroom, rows=5990) == ref
        assert LEFT not in log_of(tmp_path, "straddle_h%s_on" % headroom)


def test_pairs_mate_2_three_times_as_long(tmp_path):
    # 50 b against 150 b: file 2 has three times the text, so its side takes blocks (1 MiB here) more often than the other
    r = util.rng(53)
    gs = genomes()
    reads, mates = util.sample_reads(r, gs, 12000, 50), util.sample_reads(r, gs, 12000, 150)
    f = write_pair(tmp_path, "u", *pair_records(reads, mates, r))
    env = {"CHARON_BATCH_BASES": str(1 << 20)}
    out = both(tmp_path, ["--db", IDX, "-t", "4", "--min_length", "80"] + f, env, tag="uneven", rows=11990)
    assert "read11999/1\t" in out and LEFT not in log_of(tmp_path, "uneven_on")


def awkward_pairs(r, n):
    reads, mates = sample_pairs(r, n, 60, 400)
    mates[3] = mates[3].lower()
    mates[4] = b"N" * 150
    reads[5] = reads[5][:30] + b"NNRYKMnnswbdhv" + reads[5][44:]
    mates[6] = mates[6][:17].lower() + mates[6][17:]
    reads[7] = b"ACGU" + reads[7].replace(b"T", b"U")[4:]
    for i in range(9, 15):
        mates[i] = mates[i][:3 + i]   # a mate shorter than k
        reads[i + 10] = reads[i + 10][:2 + i]
    for i in range(30, 60):
        b = bytearray(mates[i])
        for at in r.integers(0, len(b), max(1, len(b) // 10)):
            b[int(at)] = ord("N")
        mates[i] = bytes(b)
    return reads, mates


def test_pairs_awkward_reads_crlf_and_host_gzip(tmp_path):
    r = util.rng(54)
    reads, mates = awkward_pairs(r, 600)
    a, b = pair_records(reads, mates, r, eol2="\r\n")  # CRLF in file 2 only
    a[100] = b"@\n" + a[100].split(b"\n", 1)[1]         # a record with an empty id, in both files
    b[100] = b"@\r\n" + b[100].split(b"\r\n", 1)[1]
    f = write_pair(tmp_path, "a", a, b)
    for env in ({}, {"CHARON_GZIP_ON_HOST": "1"}, {"CHARON_BATCH_READS": "100"}):
        both(tmp_path, ["--db", IDX, "-t", "4"] + f, dict(env, CHARON_TIMING="1"), tag="awk" + "_".join(env), rows=590)
        assert LEFT not in log_of(tmp_path, "awk" + "_".join(env) + "_on")
    # with the whole gzip column on the host, every pair's letters come down through the fetch; routed as ever, next to none do
    m = re.search(r"records split (\d+)  records fetched (\d+)", log_of(tmp_path, "awkCHARON_GZIP_ON_HOST_on"))
    assert m and int(m.group(1)) == 1200 and int(m.group(2)) == 600, m and m.groups()
    m = re.search(r"records split (\d+)  records fetched (\d+)", log_of(tmp_path, "awk_on"))
    assert m and int(m.group(2)) < 30, m and m.groups()


def test_pairs_extract(tmp_path):
    r = util.rng(55)
    f = write_pair(tmp_path, "e", *pair_records(*sample_pairs(r, 400), r))
    args = ["--db", IDX, "--extract", "microbial", "--num_reads_to_fit", "20"] + f
    for tag, env in (("ext", {"CHARON_BATCH_READS": "64"}), ("extd", {"CHARON_BATCH_READS": "64", "CHARON_GPU_DEFLATE": "1"})):
        both(tmp_path, args, env, tag=tag, rows=390)
        files = {}
        for d in (tag + "_unset", tag + "_on"):
            files[d] = {x: gzip.decompress((tmp_path / d / x).read_bytes()) for x in sorted(os.listdir(tmp_path / d)) if x.endswith(".gz")}
        assert len(files[tag + "_unset"]) == 2 and files[tag + "_unset"] == files[tag + "_on"]  # the files of both mates, as text
        assert all(len(v) > 0 for v in files[tag + "_on"].values())
        assert any(b"/2\n" in v for v in files[tag + "_on"].values())


def test_pairs_one_file_shorter(tmp_path):
    r = util.rng(56)
    a, b = pair_records(*sample_pairs(r, 300), r)
    for tag, (x, y) in (("short2", (a, b[:-3])), ("short1", (a[:-3], b))):
        f = write_pair(tmp_path, tag, x, y, r=r, lo=3000, hi=9000)
        for env in ({}, {"CHARON_BATCH_READS": "37"}):
            out = both(tmp_path, ["--db", IDX, "-t", "4"] + f, env, tag=tag + "_".join(env), rows=290)
            assert "read296/1\t" in out and "read297/1\t" not in out
            assert LEFT not in log_of(tmp_path, tag + "_".join(env) + "_on")


def test_pairs_leave_the_mode(tmp_path):
    r = util.rng(57)
    a, b = pair_records(*sample_pairs(r, 300, 100, 400), r)
    # a wrapped record in the middle of file 2 only
    s, q = b[150].split(b"\n")[1], b[150].split(b"\n")[3]
    wrapped = list(b)
    wrapped[150] = b"@read150/2\n" + s[:60] + b"\n" + s[60:] + b"\n+\n" + q[:60] + b"\n" + q[60:] + b"\n"
    fw = write_pair(tmp_path, "w", a, wrapped, r=r, lo=3000, hi=9000)
    # a last line without a line feed in file 1 only
    fn = write_pair(tmp_path, "n", b"".join(a)[:-1], b, r=r, lo=3000, hi=9000)
    for name, f in (("w", fw), ("n", fn)):
        for env in ({}, {"CHARON_BATCH_READS": "37", "CHARON_BATCH_BASES": str(1 << 20)}):
            tag = name + "_".join(env)
            out = both(tmp_path, ["--db", IDX, "-t", "4"] + f, env, tag=tag, rows=290)
            assert "read299/1\t" in out
            assert log_of(tmp_path, tag + "_on").count(LEFT) == 1
    # the same two kinds of text further into files of several blocks (1 MiB here), so that pairs have been submitted when the mode is
    # left and either side's text comes down from behind its last PAIRED record: a wrapped record in a block that is not the last
    # (the split stops there, the next block's carry begins with it and yields no record), and one in the last block
    a, b = pair_records(*sample_pairs(r, 6000, 100, 400), r)
    env = {"CHARON_BATCH_READS": "37", "CHARON_BATCH_BASES": str(1 << 20)}
    for at in (2500, 5900):
        s, q = b[at].split(b"\n")[1], b[at].split(b"\n")[3]
        wrapped = list(b)
        wrapped[at] = b"@read%d/2\n" % at + s[:60] + b"\n" + s[60:] + b"\n+\n" + q[:60] + b"\n" + q[60:] + b"\n"
        f = write_pair(tmp_path, "late%d" % at, a, wrapped, r=r, lo=3000, hi=9000)
        assert len(b"".join(wrapped)) > (2 << 20) and len(b"".join(wrapped[:at])) > (1 << 20)  # three blocks; the record lies behind the first
        out = both(tmp_path, ["--db", IDX, "-t", "4"] + f, env, tag="late%d" % at, rows=5990)
        assert "read5999/1\t" in out and log_of(tmp_path, "late%d_on" % at).count(LEFT) == 1
    a, b = pair_records(*sample_pairs(r, 300, 100, 400), r)
    # A record damaged in the middle of file 2: same exit status, same message, same rows.  (The reader drops the whole block that holds
    # the damage, so which rows a run prints before it fails follows from its blocks; blocks of one record make that the same everywhere.)
    damaged = list(b)
    damaged[150] = b"X" + damaged[150][1:]
    fd = write_pair(tmp_path, "d", a, damaged, r=r, lo=3000, hi=9000)
    env = {"CHARON_BATCH_READS": "1"}
    rc0, out0, err0 = run_cli(["--db", IDX] + fd, str(tmp_path / "d_unset"), env)
    rc1, out1, err1 = run_cli(["--db", IDX] + fd, str(tmp_path / "d_on"), dict(env, **ON))
    assert rc0 != 0 and rc1 == rc0, (rc0, rc1, err1)
    assert "record does not start with '@'" in err0 and err1 == err0, (err0, err1)
    assert out1 == out0 and "read148/1\t" in out0 and "read150/1\t" not in out0
    assert log_of(tmp_path, "d_on").count(LEFT) == 1


def test_pairs_file_1_leaves_while_mates_are_at_hand(tmp_path):
    # Mates half as long as the reads, blocks of 1 MiB: a block of file 2 holds about twice the records of one of file 1, so when file
    # 1's side takes its last block -- a wrapped record near its end: the mode must be left -- the other side still holds mates that
    # are split and not yet paired.  They are paired with the records in front of the wrapped one and submitted before the mode is
    # left; either file then comes down from behind its last paired record.
    r = util.rng(60)
    gs = genomes()
    reads, mates = util.sample_reads(r, gs, 6000, (200, 400), sub_rate=0.03), util.sample_reads(r, gs, 6000, (80, 150), sub_rate=0.03)
    a, b = pair_records(reads, mates, r)
    s, q = a[5900].split(b"\n")[1], a[5900].split(b"\n")[3]
    a[5900] = b"@read5900/1\n" + s[:60] + b"\n" + s[60:] + b"\n+\n" + q[:60] + b"\n" + q[60:] + b"\n"
    # file 1: the wrapped record lies in its fourth block; file 2: two blocks, the second taken long before that
    assert len(b"".join(a[:5900])) > (3 << 20) + (1 << 18) and (2 << 20) - (1 << 18) > len(b"".join(b)) > (1 << 20) + (1 << 18)
    f = write_pair(tmp_path, "m", a, b, r=r, lo=3000, hi=9000)
    env = {"CHARON_BATCH_READS": "37", "CHARON_BATCH_BASES": str(1 << 20), "CHARON_TIMING": "1"}
    out = both(tmp_path, ["--db", IDX, "-t", "4"] + f, env, tag="m", rows=5990)
    log = log_of(tmp_path, "m_on")
    assert "read5999/1\t" in out and log.count(LEFT) == 1
    # submit, then leave: every pair in front of the wrapped record went through the id check on the device, those of file 1's last
    # block included (leaving at once would have handed them to the host parser unchecked)
    m = re.search(r"timing \(CHARON_GPU_TEXT_PAIRS=1\): pairs checked (\d+)  ", log)
    assert m and int(m.group(1)) == 5900, m and m.groups()


def test_pairs_corrupt_member_in_file_2(tmp_path):
    r = util.rng(58)
    a, b = pair_records(*sample_pairs(r, 600), r)
    f = write_pair(tmp_path, "bad", a, b, r=r, lo=20000, hi=30000)
    z = bytearray(open(f[1], "rb").read())
    at, starts = 0, []
    while at < len(z):
        starts.append(at)
        at += struct.unpack_from("<H", z, at + 16)[0] + 1
    z[starts[len(starts) // 2] + 18 + 40] ^= 0x10  # a payload bit of the member in the middle of file 2
    open(f[1], "wb").write(bytes(z))
    res = [run_cli(["--db", IDX] + f, str(tmp_path / ("bad" + "_".join(env))), env) for env in ({}, ON)]
    for rc, out, err in res:
        assert rc == 1 and "a BGZF member is corrupt" in err and f[1] in err, (rc, err)
    assert [x for x in res[0][2].splitlines() if x.startswith("charon: ")] == [x for x in res[1][2].splitlines() if x.startswith("charon: ")]


def test_pairs_classify(tmp_path):
    r = util.rng(59)
    f = write_pair(tmp_path, "c", *pair_records(*sample_pairs(r, 300), r))
    both(tmp_path, ["--db", IDX, "--dist", "gamma"] + f, sub="classify", tag="cls", rows=290)
    both(tmp_path, ["--db", IDX, "--dist", "gamma"] + f, {"CHARON_BATCH_READS": "64"}, sub="classify", tag="cls64", rows=290)


def test_pairs_switch_does_not_apply(tmp_path):
    r = util.rng(60)
    reads, mates = sample_pairs(r, 200)
    a, b = pair_records(reads, mates, r)
    f = write_pair(tmp_path, "p", a, b)
    # a single-end file: one line says so, and the single-end resident path runs as it does under CHARON_GPU_TEXT=1 alone
    out = both(tmp_path, ["--db", IDX, "-t", "4", f[0]], tag="single", rows=190, applied=False)
    log = log_of(tmp_path, "single_on")
    assert log.count(PAIRS_NOT + f[0] + " (single-end input") == 1 and APPLIED in log and PAIRS_APPLIED not in log
    rc, out1, _ = run_cli(["--db", IDX, "-t", "4", f[0]], str(tmp_path / "single_text"), {"CHARON_GPU_TEXT": "1"})
    assert rc == 0 and out1 == out
    # FASTA pairs, and a one-stream .gz as file 2: one line names the file and the reason, and the run goes on as under CHARON_GPU_TEXT=1
    fa = []
    for k, rs in ((1, reads), (2, mates)):
        p = tmp_path / ("fa_%d.fasta.gz" % k)
        p.write_bytes(bgzf(b"".join(b">read%d/%d\n%s\n" % (i, k, s) for i, s in enumerate(rs))))
        fa.append(str(p))
    one = str(tmp_path / "one_2.fastq.gz")
    open(one, "wb").write(gzip.compress(b"".join(b), 6))
    for tag, files, named, why in (("fasta", fa, fa[0], "not FASTQ"), ("onegz", [f[0], one], one, "one deflate stream, not BGZF")):
        both(tmp_path, ["--db", IDX, "-t", "4"] + files, tag=tag, rows=190, applied=False)
        log = log_of(tmp_path, tag + "_on")
        assert log.count(PAIRS_NOT + named + " (" + why) == 1 and PAIRS_APPLIED not in log and APPLIED not in log, log
        assert "CHARON_GPU_TEXT=1 does not apply to " + files[0] + " (paired input" in log
    # CHARON_NO_BGZF wins
    rc, out2, _ = run_cli(["--db", IDX, "-t", "4"] + f, str(tmp_path / "nobgzf"), dict(ON, CHARON_NO_BGZF="1"))
    ref = both(tmp_path, ["--db", IDX, "-t", "4"] + f, tag="ref", rows=190)
    assert rc == 0 and out2 == ref and PAIRS_NOT + f[0] + " (CHARON_NO_BGZF is set" in log_of(tmp_path, "nobgzf")


def test_pairs_switch_values(tmp_path):
    r = util.rng(61)
    f = write_pair(tmp_path, "v", *pair_records(*sample_pairs(r, 100), r))
    (tmp_path / "junk.idx").write_bytes(b"not an index")
    # anything but unset / 0 / 1, and 1 without CHARON_GPU_TEXT=1: exit status 1 before the index file is opened
    envs = [{"CHARON_GPU_TEXT": "1", "CHARON_GPU_TEXT_PAIRS": v} for v in ("2", "", "yes", "01")]
    envs += [{"CHARON_GPU_TEXT_PAIRS": "1"}, {"CHARON_GPU_TEXT": "0", "CHARON_GPU_TEXT_PAIRS": "1"}]
    for env in envs:
        rc, out, err = run_cli(["--db", str(tmp_path / "junk.idx")] + f, str(tmp_path / "v"), env)
        assert rc == 1 and out == "" and "charon: CHARON_GPU_TEXT_PAIRS: " in err and "junk.idx" not in err, (env, err)
    # 0 is unset, with or without CHARON_GPU_TEXT; CHARON_GPU_TEXT=1 alone on pairs still logs today's line and takes the host path
    ref = both(tmp_path, ["--db", IDX] + f, tag="ref", rows=90)
    for tag, env in (("zero", {"CHARON_GPU_TEXT_PAIRS": "0"}), ("zero_text", {"CHARON_GPU_TEXT": "1", "CHARON_GPU_TEXT_PAIRS": "0"}), ("text", {"CHARON_GPU_TEXT": "1"})):
        rc, out, err = run_cli(["--db", IDX] + f, str(tmp_path / tag), env)
        log = log_of(tmp_path, tag)
        assert rc == 0 and out == ref and APPLIED not in log and "CHARON_GPU_TEXT_PAIRS" not in log, (tag, err)
        assert ("CHARON_GPU_TEXT=1 does not apply to " + f[0] + " (paired input" in log) == (tag != "zero")


def test_pairs_text_and_ids_of_file_2_do_not_travel(tmp_path):
    """2 000 pairs of 2 x 150 b, A/C/G/T only, nothing extracted: the device sizes every pair (300 letters), so no letters are needed
    on the host, and the ids of file 2 are compared where they lie"""
    r = util.rng(62)
    gs = genomes()
    reads, mates = util.sample_reads(r, gs, 2000, 150, sub_rate=0.03), util.sample_reads(r, gs, 2000, 150, sub_rate=0.03)
    f = write_pair(tmp_path, "t", *pair_records(reads, mates, r))
    both(tmp_path, ["--db", IDX, "-t", "4"] + f, {"CHARON_TIMING": "1"}, tag="travel", rows=1990)
    log = log_of(tmp_path, "travel_on")
    m = re.search(r"timing \(CHARON_GPU_TEXT_PAIRS=1\): pairs checked (\d+)  id bytes of file 2 downloaded (\d+)  seconds in pair check [\d.]+", log)
    assert m, log
    checked, id2_bytes = int(m.group(1)), int(m.group(2))
    m = re.search(r"records split (\d+)  records fetched (\d+)  text bytes inflated (\d+)  text bytes fetched (\d+)  seconds in inflate [\d.]+  "
                  r"seconds in split [\d.]+  seconds in fetch [\d.]+", log)
    assert m, log
    split, fetched, inflated, fetched_bytes = (int(x) for x in m.groups())
    print("pairs checked %d, id bytes of file 2 %d; records split %d, fetched %d; text bytes inflated %d, fetched %d" %
          (checked, id2_bytes, split, fetched, inflated, fetched_bytes))
    assert checked == 2000 and id2_bytes == 0
    assert split == 4000 and inflated > 2 * 2000 * 300
    assert fetched_bytes * 20 <= inflated
