"""GPU tests (-m gpu) of CHARON_GPU_DEFLATE=1 in the front end: the extract files of `charon dehost` / `charon classify` are written as
BGZF members compressed on the device.  The run with the variable unset is the yardstick: same TSV, same extracted bytes."""
import glob
import gzip
import os
import subprocess

import pytest

from tests import deflate_cases as dc
from tests import util

pytestmark = pytest.mark.gpu
G = os.path.join(util.ROOT, "tests", "golden")
EXE = os.path.join(util.ROOT, "charon_amd", "bin", "charon")
IDX = os.path.join(G, "cfg1.idx")
FQ = os.path.join(G, "cfg1_reads.fastq.gz")
SWITCHES = ("CHARON_GPU_DEFLATE", "CHARON_GPU_INFLATE", "CHARON_TEXT_BATCHES", "CHARON_NO_BGZF", "CHARON_DEVICE", "CHARON_DEVICES")


def run_cli(sub, args, cwd, env_extra=None):
    os.makedirs(cwd, exist_ok=True)
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra or {})
    p = subprocess.run([EXE, sub] + args + ["--log", os.path.join(cwd, "charon.log")], cwd=cwd, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def extract_files(cwd):
    return {os.path.basename(f): open(f, "rb").read() for f in sorted(glob.glob(os.path.join(cwd, "*.gz")))}


def assert_bgzf_file(blob):
    """a chain of BGZF blocks with consistent BSIZE that ends with the end-of-file marker; no piece above 65 280 bytes"""
    assert blob.endswith(dc.BGZF_EOF)
    blocks = dc.parse_bgzf(blob)
    assert sum(b[1] for b in blocks) == len(blob) and blocks[-1][4] == 0
    assert all(0 < b[4] <= dc.MAX_IN for b in blocks[:-1])
    assert all(b[4] == dc.MAX_IN for b in blocks[:-2])  # only the member written at close is short
    return blocks


def test_golden_extract_single_end(tmp_path):
    args = ["--db", IDX, "--extract", "microbial", "--num_reads_to_fit", "20", FQ]
    rc, off, err = run_cli("dehost", args, str(tmp_path / "off"))
    assert rc == 0, err
    runs = {}
    for name, env in (("on", {"CHARON_GPU_DEFLATE": "1"}), ("zero", {"CHARON_GPU_DEFLATE": "0"}),
                      ("on_devices", {"CHARON_GPU_DEFLATE": "1", "CHARON_DEVICES": "0,0"}), ("on_timing", {"CHARON_GPU_DEFLATE": "1", "CHARON_TIMING": "1"})):
        rc, out, err = run_cli("dehost", args, str(tmp_path / name), env)
        assert rc == 0, err
        assert out == off, name                                           # the TSV, byte for byte
        said = "CHARON_GPU_DEFLATE=1" in open(tmp_path / name / "charon.log").read()
        assert said == (name != "zero")
        assert ("inside chn_deflate_run" in err) == (name == "on_timing")
        runs[name] = extract_files(str(tmp_path / name))
    want = extract_files(str(tmp_path / "off"))
    assert list(want) == ["charon_microbial.fastq.gz"] and len(gzip.decompress(want["charon_microbial.fastq.gz"])) > 2 * dc.MAX_IN
    assert runs["zero"] == want                                           # 0 is unset: the zlib path, bytes unchanged
    for name in ("on", "on_devices", "on_timing"):
        assert list(runs[name]) == list(want)
        blob = runs[name]["charon_microbial.fastq.gz"]
        assert gzip.decompress(blob) == gzip.decompress(want["charon_microbial.fastq.gz"])
        assert len(assert_bgzf_file(blob)) >= 4
        assert blob == runs["on"]["charon_microbial.fastq.gz"]
    # the file is input again, through the BGZF reader: members in parallel on the host, on the device, and as one plain gzip stream
    mine = str(tmp_path / "on" / "charon_microbial.fastq.gz")
    outs = []
    for name, env in (("r_host", {}), ("r_dev", {"CHARON_GPU_INFLATE": "1"}), ("r_plain", {"CHARON_NO_BGZF": "1"})):
        rc, out, err = run_cli("dehost", ["--db", IDX, mine], str(tmp_path / name), env)
        assert rc == 0, err
        outs.append(out)
    assert outs[0].count("\n") > 20 and outs[1] == outs[0] and outs[2] == outs[0]
    bad = bytearray(open(mine, "rb").read())
    bad[dc.parse_bgzf(bytes(bad))[1][0] + 18 + 200] ^= 0x40               # a byte of the second member's deflate data
    (tmp_path / "bad.fastq.gz").write_bytes(bytes(bad))
    rc, out, err = run_cli("dehost", ["--db", IDX, str(tmp_path / "bad.fastq.gz")], str(tmp_path / "bad"))
    assert rc == 1 and "a BGZF member is corrupt" in err, err             # (it was read as BGZF)


def test_paired_extract_and_an_empty_category(tmp_path, oracle_lib):
    """the paired fixture of tests/test_gpu_cli.py with --extract all: two files per category; then reads of one genome only, which
    leaves the other category's files without a record: the end-of-file marker alone"""
    r = util.rng(21)
    gs = [util.random_seq(r, 6000) for _ in range(3)]
    for i, g in enumerate(gs):
        with open(tmp_path / ("g%d.fa" % i), "w") as f:
            f.write(">g%d\n%s\n" % (i, g.decode()))
    oidx = oracle_lib.Index.from_fasta([(str(tmp_path / "g0.fa"), "human"), (str(tmp_path / "g1.fa"), "bacteria"),
                                        (str(tmp_path / "g2.fa"), "human")], ["bacteria", "human"])
    oidx.store(str(tmp_path / "p.idx"))
    oidx.free()
    for tag, genomes in (("mixed", gs), ("bacteria_only", [gs[1]])):
        m1 = util.sample_reads(r, genomes, 300, (100, 250), sub_rate=0.02)
        m2 = util.sample_reads(r, genomes, 300, (100, 250), sub_rate=0.02)
        files = []
        for name, mates, mate in (("%s_1.fastq" % tag, m1, "/1"), ("%s_2.fastq" % tag, m2, "/2")):
            with open(tmp_path / name, "w") as f:
                for i, s in enumerate(mates):
                    q = "".join(chr(33 + int(x)) for x in r.integers(5, 41, len(s)))
                    f.write("@read%d%s\n%s\n+\n%s\n" % (i, mate, s.decode(), q))
            files.append(str(tmp_path / name))
        args = ["--db", str(tmp_path / "p.idx"), "--extract", "all", "--num_reads_to_fit", "20"] + files
        rc, off, err = run_cli("dehost", args, str(tmp_path / (tag + "_off")))
        assert rc == 0, err
        rc, on, err = run_cli("dehost", args, str(tmp_path / (tag + "_on")), {"CHARON_GPU_DEFLATE": "1"})
        assert rc == 0, err
        assert on == off and off.count("\n") > 100
        want, got = extract_files(str(tmp_path / (tag + "_off"))), extract_files(str(tmp_path / (tag + "_on")))
        assert list(got) == list(want) and len(want) == 4
        for name in want:
            assert_bgzf_file(got[name])
            assert gzip.decompress(got[name]) == gzip.decompress(want[name]), name
        if tag == "mixed":
            assert all(len(gzip.decompress(v)) > 1000 for v in want.values())
        else:
            empty = [name for name, v in want.items() if gzip.decompress(v) == b""]
            assert len(empty) == 2 and all("human" in name for name in empty)
            assert all(got[name] == dc.BGZF_EOF for name in empty)


def test_bad_value_and_charon_index(tmp_path):
    (tmp_path / "junk.idx").write_bytes(b"not an index")
    for sub in ("dehost", "classify"):
        for v in ("2", "", "yes"):
            rc, out, err = run_cli(sub, ["--db", str(tmp_path / "junk.idx"), "--extract", "all", FQ], str(tmp_path / "v"), {"CHARON_GPU_DEFLATE": v})
            assert rc == 1 and out == "" and "charon: CHARON_GPU_DEFLATE: " in err and "junk.idx" not in err, (v, err)
    # `charon index` does not read the variable
    tsv = tmp_path / "refs.tsv"
    tsv.write_text("%s\tmicrobial\n%s\thost\n" % (os.path.join(G, "my.fasta"), os.path.join(G, "cfg1_host.fasta")))
    built = []
    for name, env in (("i_unset", {}), ("i_two", {"CHARON_GPU_DEFLATE": "2"})):
        os.makedirs(tmp_path / name)
        env_all = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env_all.update(env)
        p = subprocess.run([EXE, "index", "-p", str(tmp_path / name / "x"), "--log", str(tmp_path / name / "i.log"), str(tsv)], cwd=str(tmp_path / name), env=env_all,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()
        built.append(open(tmp_path / name / "x.idx", "rb").read())
    assert built[0] == built[1] and len(built[0]) > 1000
