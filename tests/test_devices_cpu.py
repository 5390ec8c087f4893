"""CPU tests of CHARON_DEVICES (index replicas of `charon dehost` / `charon classify`): malformed values end the run before the
index file is opened and before any HIP call, and the ordered merge that hands the replicas' batches back releases them strictly in
input order (`charon _ordered_merge`, no GPU involved)."""
import os
import subprocess

import pytest

from tests import util

EXE = os.path.join(util.ROOT, "charon_amd", "bin", "charon")
G = os.path.join(util.ROOT, "tests", "golden")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(EXE):
        import __graft_entry__ as g
        g.build()


def run(args, cwd, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("CHARON_DEVICE", "CHARON_DEVICES")}
    env.update(env_extra)
    p = subprocess.run([EXE] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.mark.parametrize("env", [{"CHARON_DEVICES": ""}, {"CHARON_DEVICES": "0,,1"}, {"CHARON_DEVICES": "a"}, {"CHARON_DEVICES": "-1"},
                                 {"CHARON_DEVICES": "0,1x"}, {"CHARON_DEVICES": "0,"}, {"CHARON_DEVICES": ",".join(["0"] * 65)},
                                 {"CHARON_DEVICE": "0", "CHARON_DEVICES": "0"}])
@pytest.mark.parametrize("sub", ["dehost", "classify"])
def test_bad_devices_value_is_rejected_up_front(tmp_path, env, sub):
    args = [sub, "--db", os.path.join(G, "cfg1.idx"), os.path.join(G, "cfg1_reads.fastq.gz"), "--log", str(tmp_path / "charon.log")]
    rc, out, err = run(args, str(tmp_path), env)
    assert rc == 1, (rc, err)
    assert out == ""
    assert "charon: CHARON_DEVICES: " in err, err
    assert "hip" not in err.lower(), err


def test_bad_devices_value_checked_before_the_index_file(tmp_path):
    # the index file is not an index: the variable is still what the run fails on
    (tmp_path / "junk.idx").write_bytes(b"not an index")
    args = ["dehost", "--db", str(tmp_path / "junk.idx"), os.path.join(G, "cfg1_reads.fastq.gz"), "--log", str(tmp_path / "charon.log")]
    rc, out, err = run(args, str(tmp_path), {"CHARON_DEVICES": "0;1"})
    assert rc == 1 and out == "" and "charon: CHARON_DEVICES: " in err and "junk.idx" not in err, err


@pytest.mark.parametrize("threads,m,seed", [(1, 1, 0), (1, 50, 3), (2, 7, 1), (3, 100, 7), (4, 257, 11), (8, 33, 5), (16, 400, 2), (5, 0, 9)])
def test_ordered_merge_releases_in_order(threads, m, seed):
    p = subprocess.run([EXE, "_ordered_merge", str(threads), str(m), str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    got = [int(x) for x in p.stdout.decode().split()]
    assert got == list(range(m))
