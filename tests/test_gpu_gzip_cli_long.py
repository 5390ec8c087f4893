"""GPU tests (-m gpu) of the `compression` column for long reads through `charon dehost` / `classify`: reads beyond 61 440 letters that
the default routing (or CHARON_GZIP_GPU_MAX above 61 440) hands to the device's long-read deflate pass must print exactly what the
host emulator and zlib itself print."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu
EXE = os.path.join(util.ROOT, "charon_amd", "bin", "charon")


def run_cli(args, cwd, env_extra=None, sub="dehost"):
    env = dict(os.environ)
    env.update(env_extra or {})
    p = subprocess.run([EXE, sub] + args + ["--log", os.path.join(cwd, "charon.log")], cwd=cwd, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def long_count(cwd):
    m = re.findall(r"gzip column: (\d+) reads beyond 61440 letters sized by the device's long-read deflate pass",
                   open(os.path.join(cwd, "charon.log")).read())
    assert m
    return int(m[-1])  # (the run just made)


@pytest.fixture(scope="module")
def long_fasta(tmp_path_factory, oracle_lib):
    """a nanopore-like FASTA: reads of 1 - 60 kb and 40 reads of 62 - 300 kb (random, N-rich, repeats, copies), plus an index"""
    tmp = tmp_path_factory.mktemp("gzlong")
    r = util.rng(77)
    gs = [util.random_seq(r, 400000), util.random_seq(r, 400000)]
    for i, g in enumerate(gs):
        with open(tmp / ("g%d.fa" % i), "w") as f:
            f.write(">g%d\n%s\n" % (i, g.decode()))
    oidx = oracle_lib.Index.from_fasta([(str(tmp / "g0.fa"), "human"), (str(tmp / "g1.fa"), "microbial")], ["microbial", "human"])
    oidx.store(str(tmp / "z.idx"))
    oidx.free()
    recs = []
    for i in range(300):
        L = int(np.exp(r.uniform(np.log(1000), np.log(60000))))
        g = gs[i & 1]
        a = int(r.integers(0, len(g) - L))
        recs.append(util.mutate(r, g[a:a + L], 0.05))
    for i in range(40):
        L = int(r.integers(62000, 300000))
        g = gs[i & 1]
        a = int(r.integers(0, len(g) - L))
        s = np.frombuffer(util.mutate(r, g[a:a + L], 0.05), np.uint8).copy()
        if i % 4 == 1:
            s[r.random(L) < 0.03] = ord("N")
        elif i % 4 == 2:
            s[L // 3:L // 3 + 20000] = np.frombuffer(b"TTAGGG" * 3333 + b"TT", np.uint8)
        elif i % 4 == 3:
            d = int(r.integers(32400, 32600))
            s[L - 5000:L - 4000] = s[L - 5000 - d:L - 4000 - d].copy()
        recs.insert(int(r.integers(1, len(recs))), bytes(s))
    with open(tmp / "z.fasta", "w") as f:
        for i, s in enumerate(recs):
            f.write(">z%d\n%s\n" % (i, s.decode()))
    return tmp, recs


def test_cli_long_reads_gzip_column_is_identical_in_every_mode(long_fasta):
    tmp, recs = long_fasta
    cwd = str(tmp)
    args = ["--db", str(tmp / "z.idx"), "--min_quality", "0", str(tmp / "z.fasta")]
    n_long = sum(1 for s in recs[1:] if len(s) > 61440)
    outs = {}
    for mode, env in (("default", {}), ("gpu300k", {"CHARON_GZIP_GPU_MAX": "300000"}), ("gpu61440", {"CHARON_GZIP_GPU_MAX": "61440"}),
                      ("host", {"CHARON_GZIP_ON_HOST": "1"}), ("zlib", {"CHARON_ZLIB_ONLY": "1"}), ("devices", {"CHARON_DEVICES": "0,0"})):
        rc, out, err = run_cli(args, cwd, env)
        assert rc == 0, err
        outs[mode] = out
        if mode == "default":  # -t 1 and one batch of 40 long reads: the routing gives them to the device
            assert long_count(cwd) == n_long
        elif mode == "gpu300k":
            assert long_count(cwd) == n_long
        elif mode == "gpu61440":
            assert long_count(cwd) == 0
    assert len(outs["zlib"].strip().split("\n")) == len(recs) - 1
    for mode, out in outs.items():
        assert out == outs["zlib"], mode


def test_cli_long_pairs_classify_gzip_column(long_fasta):
    tmp, recs = long_fasta
    cwd = str(tmp)
    longs = [s for s in recs if len(s) > 61440][:20]
    shorts = [s for s in recs if len(s) <= 61440][:20]
    m1, m2 = longs[:10] + shorts[:10], shorts[10:20] + longs[10:20]
    for name, mates, tag in (("p_1.fasta", m1, "/1"), ("p_2.fasta", m2, "/2")):
        with open(tmp / name, "w") as f:
            for i, s in enumerate(mates):
                f.write(">p%d%s\n%s\n" % (i, tag, s.decode()))
    pargs = ["--db", str(tmp / "z.idx"), "--min_quality", "0", str(tmp / "p_1.fasta"), str(tmp / "p_2.fasta")]
    a = run_cli(pargs, cwd, {"CHARON_GZIP_GPU_MAX": "700000"}, sub="classify")
    assert a[0] == 0, a[2]
    assert long_count(cwd) > 0
    b = run_cli(pargs, cwd, {"CHARON_ZLIB_ONLY": "1"}, sub="classify")
    c = run_cli(pargs, cwd, {}, sub="classify")
    assert b[0] == 0 and c[0] == 0
    assert a[1] == b[1] == c[1] and a[1].count("\n") == len(m1) - 1
