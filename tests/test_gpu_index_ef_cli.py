"""GPU tests of CHARON_GPU_INDEX_EF (`charon index` encodes the Elias-Fano arrays on the device): the .idx is the same bytes with the
switch, without it and for every slice size and thread count; the switch's log line; its refusal of other values; dehost ignores it."""
import os
import subprocess

import pytest

from tests import util

pytestmark = pytest.mark.gpu
EXE = os.path.join(util.ROOT, "charon_amd", "bin", "charon")
LOG_LINE = "CHARON_GPU_INDEX_EF=1: the Elias-Fano arrays were encoded on device"


def clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("CHARON_GPU_INDEX_EF", "CHARON_INDEX_EF_SLICE")}
    env.update(extra)
    return env


def index(tmp, tab, name, args=(), **env):
    log = tmp / (name + ".log")
    p = subprocess.run([EXE, "index"] + list(args) + ["-p", str(tmp / name), "--log", str(log), str(tab)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=clean_env(**env))
    return p, (open(log).read() if log.exists() else "")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """a handful of small FASTA files, the table, and the index built with the switch unset"""
    tmp = tmp_path_factory.mktemp("index_ef")
    r = util.rng(71)
    files, seqs = [], []
    for i, (nrec, L) in enumerate(((1, 30000), (3, 9000), (2, 50), (1, 5000), (2, 60))):
        path = tmp / ("ref%d.fa" % i)
        with open(path, "w") as f:
            for j in range(nrec):
                s = util.random_seq(r, L).decode()
                seqs.append(s)
                f.write(">rec%d_%d\n" % (i, j))
                f.write("\n".join(s[k:k + 70] for k in range(0, len(s), 70)) + "\n")
        files.append(str(path))
    tab = tmp / "in.tab"
    with open(tab, "w") as f:
        for p, c in zip(files, ["microbial", "human", "microbial", "human", "microbial"]):
            f.write("%s\t%s\n" % (p, c))
    p, log = index(tmp, tab, "unset")
    assert p.returncode == 0, p.stderr.decode()
    assert LOG_LINE not in log
    return dict(tmp=tmp, tab=tab, seqs=seqs, r=r, want=open(tmp / "unset.idx", "rb").read())


@pytest.mark.parametrize("name,args,env", [("zero", (), dict(CHARON_GPU_INDEX_EF="0")),
                                           ("one", (), dict(CHARON_GPU_INDEX_EF="1")),
                                           ("slice37_t1", ("-t", "1"), dict(CHARON_GPU_INDEX_EF="1", CHARON_INDEX_EF_SLICE="37")),
                                           ("slice37_t5", ("-t", "5"), dict(CHARON_GPU_INDEX_EF="1", CHARON_INDEX_EF_SLICE="37"))])
def test_same_bytes_with_and_without_the_switch(built, name, args, env):
    p, log = index(built["tmp"], built["tab"], name, args, **env)
    assert p.returncode == 0, p.stderr.decode()
    assert open(built["tmp"] / (name + ".idx"), "rb").read() == built["want"]
    assert (LOG_LINE in log) == (env["CHARON_GPU_INDEX_EF"] == "1")


def test_same_bytes_under_optimize(built):
    p, log = index(built["tmp"], built["tab"], "opt_unset", ("--optimize",))
    assert p.returncode == 0, p.stderr.decode()
    p1, log1 = index(built["tmp"], built["tab"], "opt_one", ("--optimize",), CHARON_GPU_INDEX_EF="1", CHARON_TIMING="1")
    assert p1.returncode == 0, p1.stderr.decode()
    assert LOG_LINE in log1 and LOG_LINE not in log
    assert open(built["tmp"] / "opt_one.idx", "rb").read() == open(built["tmp"] / "opt_unset.idx", "rb").read()
    # the timing line keeps its shape: the last figure is the stage, whichever path ran
    line = [ln for ln in p1.stderr.decode().split("\n") if "charon index: timing (s):" in ln]
    assert len(line) == 1 and "download + Elias-Fano " in line[0] and float(line[0].rsplit(" ", 1)[1]) >= 0


def test_other_values_end_the_run_before_anything_is_read(built):
    tmp = built["tmp"]
    p, log = index(tmp, built["tab"], "two", CHARON_GPU_INDEX_EF="2")
    assert p.returncode == 1 and "CHARON_GPU_INDEX_EF" in p.stderr.decode() and "neither 0 nor 1" in p.stderr.decode()
    assert not (tmp / "two.idx").exists() and "Found " not in log


def test_the_file_loads_and_dehost_does_not_read_the_switch(built):
    tmp = built["tmp"]
    p, _ = index(tmp, built["tab"], "for_dehost", CHARON_GPU_INDEX_EF="1")
    assert p.returncode == 0, p.stderr.decode()
    reads = util.sample_reads(built["r"], [s.encode() for s in built["seqs"][:2]], 60, (200, 900))
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
    assert dehost("for_dehost.idx", CHARON_GPU_INDEX_EF="2", CHARON_INDEX_EF_SLICE="x") == want
