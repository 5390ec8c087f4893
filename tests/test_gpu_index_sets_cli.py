"""GPU tests of CHARON_GPU_INDEX_SETS (`charon index` keeps every bin's minimisers in device memory, sorts and uniques them there and
emplaces them in place): the .idx is the same bytes with the switch, without it, at every thread count, piece size and compaction
threshold, together with CHARON_GPU_INDEX_EF, under --optimize, and however a budget splits the bins between the device and the host
path; the switch's log lines; dehost ignores it.  The expected bytes are those the unset run writes."""
import os
import re
import subprocess

import pytest

from tests import util

pytestmark = pytest.mark.gpu
EXE = os.path.join(util.ROOT, "charon_amd", "bin", "charon")
LOG_LINE = "CHARON_GPU_INDEX_SETS=1: the minimiser sets of"
SPILL_LINE = "take the host path"
OURS = ("CHARON_GPU_INDEX_SETS", "CHARON_INDEX_SETS_BUDGET", "CHARON_INDEX_SETS_COMPACT", "CHARON_GPU_INDEX_EF", "CHARON_INDEX_EF_SLICE", "CHARON_INDEX_PIECE",
        "CHARON_TIMING")


def clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in OURS}
    env.update(extra)
    return env


def index(tmp, tab, name, args=(), **env):
    log = tmp / (name + ".log")
    p = subprocess.run([EXE, "index"] + list(args) + ["-p", str(tmp / name), "--log", str(log), str(tab)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=clean_env(**env))
    return p, (open(log).read() if log.exists() else "")


def write_fasta(path, seqs, tag):
    with open(path, "w") as f:
        for j, s in enumerate(seqs):
            f.write(">%s_%d\n" % (tag, j))
            f.write("\n".join(s[k:k + 70] for k in range(0, len(s), 70)) + "\n")


SMALL = 1500  # bases of each of the first two files


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """six small FASTA files, the table, and the index built with the switch unset.  The first two bins are small; the third has 130 000
    records of 45 bases (three batches of the builder's loop, so a set is appended to and compacted inside the loop) and far more
    minimisers than both together; then a record long enough to be cut into pieces, and records barely longer than w."""
    tmp = tmp_path_factory.mktemp("index_sets")
    r = util.rng(72)
    many = util.random_seq(r, 45 * 130000).decode()
    shapes = [[util.random_seq(r, SMALL).decode()],
              [util.random_seq(r, SMALL // 2).decode() for _ in range(2)],
              [many[i:i + 45] for i in range(0, len(many), 45)],
              [util.random_seq(r, 30000).decode()] + [util.random_seq(r, 9000).decode() for _ in range(2)],
              [util.random_seq(r, 50).decode() for _ in range(2)],
              [util.random_seq(r, 5000).decode(), "ACGT" * 10, util.random_seq(r, 60).decode()]]
    files = []
    for i, seqs in enumerate(shapes):
        path = tmp / ("ref%d.fa" % i)
        write_fasta(path, seqs, "rec%d" % i)
        files.append(str(path))
    tab = tmp / "in.tab"
    with open(tab, "w") as f:
        for p, c in zip(files, ["microbial", "human", "microbial", "human", "microbial", "human"]):
            f.write("%s\t%s\n" % (p, c))
    p, log = index(tmp, tab, "unset")
    assert p.returncode == 0, p.stderr.decode()
    assert LOG_LINE not in log and SPILL_LINE not in log
    hashes = [int(h) for h in re.findall(r"records and (\d+) hashes to bin \d+", log)]
    assert len(hashes) == 6 and min(hashes) > 0
    return dict(tmp=tmp, tab=tab, seqs=[shapes[0][0], shapes[3][0]], r=r, hashes=hashes, want=open(tmp / "unset.idx", "rb").read())


@pytest.mark.parametrize("name,args,env", [("zero", (), dict(CHARON_GPU_INDEX_SETS="0")),
                                           ("one_t1", ("-t", "1"), dict(CHARON_GPU_INDEX_SETS="1")),
                                           ("one_t5", ("-t", "5"), dict(CHARON_GPU_INDEX_SETS="1")),
                                           ("compact", (), dict(CHARON_GPU_INDEX_SETS="1", CHARON_INDEX_SETS_COMPACT="1000")),
                                           ("piece", (), dict(CHARON_GPU_INDEX_SETS="1", CHARON_INDEX_PIECE="4096")),
                                           ("with_ef", (), dict(CHARON_GPU_INDEX_SETS="1", CHARON_GPU_INDEX_EF="1"))])
def test_same_bytes_with_and_without_the_switch(built, name, args, env):
    p, log = index(built["tmp"], built["tab"], name, args, **env)
    assert p.returncode == 0, p.stderr.decode()
    assert open(built["tmp"] / (name + ".idx"), "rb").read() == built["want"]
    on = env["CHARON_GPU_INDEX_SETS"] == "1"
    assert (LOG_LINE in log) == on and SPILL_LINE not in log
    if on:
        assert "the minimiser sets of 6 of 6 bins stayed on device 0" in log
        # the hash counts the log names come from the device's counts: the same figures
        assert [int(h) for h in re.findall(r"records and (\d+) hashes to bin \d+", log)] == built["hashes"]
        m = re.search(r"\((\d+) values never crossed to the host\)", log)
        assert m and int(m.group(1)) >= sum(built["hashes"])


def test_same_bytes_under_optimize(built):
    p, log = index(built["tmp"], built["tab"], "opt_unset", ("--optimize",))
    assert p.returncode == 0, p.stderr.decode()
    p1, log1 = index(built["tmp"], built["tab"], "opt_one", ("--optimize",), CHARON_GPU_INDEX_SETS="1", CHARON_TIMING="1")
    assert p1.returncode == 0, p1.stderr.decode()
    assert LOG_LINE in log1 and LOG_LINE not in log
    got = open(built["tmp"] / "opt_one.idx", "rb").read()
    assert got == open(built["tmp"] / "opt_unset.idx", "rb").read()
    # the timing line keeps its shape, whichever path ran
    line = [ln for ln in p1.stderr.decode().split("\n") if "charon index: timing (s):" in ln]
    assert len(line) == 1
    m = re.search(r"read [\d.]+  pack [\d.]+  minimisers \(device \+ download\) [\d.]+  sort\+unique ([\d.]+)  layout\+emplace [\d.]+  download \+ Elias-Fano [\d.]+$", line[0])
    assert m and float(m.group(1)) >= 0, line[0]


def test_a_budget_that_spills_at_the_first_bin(built):
    p, log = index(built["tmp"], built["tab"], "spill0", (), CHARON_GPU_INDEX_SETS="1", CHARON_INDEX_SETS_BUDGET="1")
    assert p.returncode == 0, p.stderr.decode()
    assert open(built["tmp"] / "spill0.idx", "rb").read() == built["want"]
    assert log.count(SPILL_LINE) == 1 and "CHARON_GPU_INDEX_SETS=1: bin 0 and the bins behind it take the host path" in log
    assert "the minimiser sets of 0 of 6 bins stayed on device 0 (0 values never crossed to the host)" in log


@pytest.mark.parametrize("compact", (None, "50000"))
def test_a_budget_that_spills_at_the_third_bin(built, compact):
    """The budget admits the first two bins whole and half of the third bin's distinct values.  A finished set holds 8 bytes per distinct
    value (the memory rule).  While one of the first two bins is filled and sorted, the sets hold at most 8 * (hashes of the bin in front)
    + 8 * values + the scratch of its unique call, 8 * values + 1 KiB of counters + 18 440 bytes of histograms, with at most one value
    per base: below 4 * hashes[2], as asserted.  The third bin's set cannot stay below the budget, because it ends with 8 * hashes[2]
    bytes: it comes down, at one of its appends or at a unique call, depending on the compaction threshold."""
    h = built["hashes"]
    assert 4 * h[2] > 8 * SMALL + 16 * SMALL + 1024 + 18440
    budget = 8 * (h[0] + h[1]) + 4 * h[2]
    env = dict(CHARON_GPU_INDEX_SETS="1", CHARON_INDEX_SETS_BUDGET=str(budget))
    if compact:
        env["CHARON_INDEX_SETS_COMPACT"] = compact
    name = "spill2_%s" % compact
    p, log = index(built["tmp"], built["tab"], name, (), **env)
    assert p.returncode == 0, p.stderr.decode()
    assert open(built["tmp"] / (name + ".idx"), "rb").read() == built["want"]
    assert log.count(SPILL_LINE) == 1 and "CHARON_GPU_INDEX_SETS=1: bin 2 and the bins behind it take the host path" in log
    assert "the minimiser sets of 2 of 6 bins stayed on device 0" in log
    assert [int(x) for x in re.findall(r"records and (\d+) hashes to bin \d+", log)] == h


def test_no_minimisers_is_the_same_error_either_way(built):
    tmp = built["tmp"]
    # (shorter than w and than k: a record of k to w - 1 bases still has one window, as in seqan3)
    write_fasta(tmp / "short.fa", ["ACGTACGTAC", "ACGT" * 4, "ACGTACGTACGTACGTAC"], "short")
    tab = tmp / "short.tab"
    tab.write_text("%s\tmicrobial\n" % (tmp / "short.fa"))
    p0, _ = index(tmp, tab, "short_unset")
    p1, log1 = index(tmp, tab, "short_one", (), CHARON_GPU_INDEX_SETS="1")
    assert p0.returncode == 1 and p1.returncode == 1
    assert "no minimisers in any input file" in p0.stderr.decode() and p1.stderr.decode() == p0.stderr.decode()
    assert not (tmp / "short_one.idx").exists()


def test_the_file_loads_and_dehost_does_not_read_the_switch(built):
    tmp = built["tmp"]
    p, _ = index(tmp, built["tab"], "for_dehost", CHARON_GPU_INDEX_SETS="1")
    assert p.returncode == 0, p.stderr.decode()
    reads = util.sample_reads(built["r"], [s.encode() for s in built["seqs"]], 60, (200, 900))
    with open(tmp / "q.fastq", "w") as f:
        for i, s in enumerate(reads):
            s = s.decode().upper()
            f.write("@q%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))

    def dehost(db, **env):
        q = subprocess.run([EXE, "dehost", "--db", str(tmp / db), str(tmp / "q.fastq"), "--log", str(tmp / "d.log")], cwd=str(tmp), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, env=clean_env(**env))
        assert q.returncode == 0, q.stderr.decode()
        return q.stdout
    want = dehost("unset.idx")
    assert want.count(b"\n") > 10  # (a row per classified read)
    assert dehost("for_dehost.idx") == want
    assert dehost("for_dehost.idx", CHARON_GPU_INDEX_SETS="2", CHARON_INDEX_SETS_BUDGET="x", CHARON_INDEX_SETS_COMPACT="x") == want
