"""GPU tests (-m gpu) of index replicas: chn_index_replicate through the C ABI, and `charon dehost` / `charon classify` with
CHARON_DEVICES, whose rows must be byte-identical to the run without it (one GPU: a repeated ordinal is a second replica on it)."""
import ctypes
import gzip
import os
import re

import numpy as np
import pytest

from tests import util
from tests.test_gpu_cli import EXE, G, assert_same_tsv, relocated_cfg1_index, run_cli

pytestmark = pytest.mark.gpu

SETTINGS = ("0", "0,0", "0,0,0")
SMALL = {"CHARON_BATCH_READS": "16", "CHARON_BATCH_BASES": "1048576"}


@pytest.fixture(scope="module")
def api():
    import charon_amd.api as api
    return api


def run_gpu(api, gidx, reads):
    from charon_amd import pack
    p = pack.pack_reads(reads)
    n = len(reads)
    st = api.Stream(gidx, n, p["n_bases"])
    st.set_model(api.default_model(gidx.desc.num_categories, gidx.desc.host_index))
    st.submit_host(p, np.full(n, 40.0, np.float32), np.zeros(n, np.float32))
    out = st.wait_host()
    st.destroy()
    return out


def test_replicate_same_device(api, oracle_lib, my_fasta):
    r = util.rng(42)
    host = util.random_seq(r, 10000)
    micro = [s.encode() for s in my_fasta.values()]
    oidx = util.build_oracle_index(oracle_lib, [micro, [host]], [0, 1], ["microbial", "host"])
    reads = util.sample_reads(r, micro[1:4] + [host], 1000, 1000, sub_rate=0.05, random_fraction=0.1)
    src = util.gpu_index_from_oracle(api, oidx)
    rows, pops = src.download(), src.bin_popcounts()
    want = run_gpu(api, src, reads)
    rep = None
    try:
        rep = src.replicate(src.device)
        got_pops = rep.bin_popcounts()  # waits for the copy: the source may go from here on
        src.destroy()
        np.testing.assert_array_equal(got_pops, pops)
        np.testing.assert_array_equal(rep.download(), rows)
        d = api.IndexDesc()
        api._chk(api.lib().chn_index_get_desc(rep.h, ctypes.byref(d)))
        assert d.device == src.desc.device and d.bin_size == src.desc.bin_size and bytes(d.bin_to_category) == bytes(src.desc.bin_to_category)
        got = run_gpu(api, rep, reads)
        util.assert_same_results(got, want)
        assert set(np.unique(got["call"])) >= {0, 1, 255}
        # a copy of the copy: ordered behind its own queued copy
        rep2 = rep.replicate(0)
        np.testing.assert_array_equal(rep2.download(), rows)
        rep2.destroy()
        # an ordinal that is not below the device count
        n = api.device_count()
        h = ctypes.c_void_p()
        assert api.lib().chn_index_replicate(rep.h, n, ctypes.byref(h)) == -1 and not h.value
        assert str(n) in api.lib().chn_last_error().decode()
        assert api.lib().chn_index_replicate(rep.h, -1, ctypes.byref(h)) == -1
    finally:
        src.destroy()
        if rep is not None:
            rep.destroy()
        oidx.free()


def replica_runs(args, cwd, env, sub="dehost"):
    """the unset run, then every CHARON_DEVICES setting; stdout of each must be byte-identical to the unset one"""
    rc, base, err = run_cli(args, cwd, env, sub=sub)
    assert rc == 0, err
    for dv in SETTINGS:
        rc, out, err = run_cli(args, cwd, dict(env, CHARON_DEVICES=dv), sub=sub)
        assert rc == 0, (dv, err)
        assert out == base, dv
    return base


def replica_log(cwd):
    """replica count and per-replica batch counts of the LAST run logged (the log file is appended to)"""
    log = open(os.path.join(cwd, "charon.log")).read()
    log = log[log.rfind("replicas: "):]
    m = re.search(r"replicas: (\d+) \(devices ([0-9,]+)\)", log)
    batches = [int(b) for b in re.findall(r"replica \d+ \(device \d+\): (\d+) batches", log)]
    return (int(m.group(1)) if m else None), batches


def test_cli_replicas_cfg1(tmp_path):
    fq = os.path.join(G, "cfg1_reads.fastq.gz")
    db = relocated_cfg1_index(tmp_path)
    for t in ("1", "4"):
        out = replica_runs(["--db", db, "-t", t, fq], str(tmp_path), SMALL)
        assert_same_tsv(out, open(os.path.join(G, "cfg1_expected.tsv")).read())
    # the last run was 0,0,0: three replicas, each with batches of its own
    n, batches = replica_log(str(tmp_path))
    assert n == 3 and len(batches) == 3 and min(batches) >= 1, batches
    # unset: one replica, on device 0
    rc, out, err = run_cli(["--db", db, fq], str(tmp_path), SMALL)
    assert rc == 0, err
    n, batches = replica_log(str(tmp_path))
    assert n == 1 and len(batches) == 1 and batches[0] >= 1
    rc, o, err = run_cli(["--db", db, fq], str(tmp_path), dict(SMALL, CHARON_DEVICES="all"))
    assert rc == 0 and o == out, err


def test_cli_replicas_paired_and_fasta(tmp_path, oracle_lib):
    r = util.rng(21)
    gs = [util.random_seq(r, 6000) for _ in range(3)]
    for i, g in enumerate(gs):
        with open(tmp_path / ("g%d.fa" % i), "w") as f:
            f.write(">g%d\n%s\n" % (i, g.decode()))
    oidx = oracle_lib.Index.from_fasta([(str(tmp_path / "g0.fa"), "human"), (str(tmp_path / "g1.fa"), "bacteria"),
                                        (str(tmp_path / "g2.fa"), "human")], ["bacteria", "human"])
    oidx.store(str(tmp_path / "p.idx"))
    oidx.free()
    m1 = util.sample_reads(r, gs, 300, (100, 250), sub_rate=0.02)
    m2 = util.sample_reads(r, gs, 300, (100, 250), sub_rate=0.02)
    m1[5] = m1[5][:60] + b"NNNRY" + m1[5][65:]
    for name, mates, tag in (("r_1.fastq", m1, "/1"), ("r_2.fastq", m2, "/2")):
        with open(tmp_path / name, "w") as f:
            for i, s in enumerate(mates):
                q = "".join(chr(33 + int(x)) for x in r.integers(5, 41, len(s)))
                f.write("@read%d%s\n%s\n+\n%s\n" % (i, tag, s.decode(), q))
    for name, mates, tag in (("r_1.fasta", m1, "/1"), ("r_2.fasta", m2, "/2")):
        with open(tmp_path / name, "w") as f:
            for i, s in enumerate(mates):
                f.write(">read%d%s\n%s\n" % (i, tag, s.decode()))
    db = str(tmp_path / "p.idx")
    out = replica_runs(["--db", db, str(tmp_path / "r_1.fastq"), str(tmp_path / "r_2.fastq")], str(tmp_path), SMALL)
    assert len(out.strip().split("\n")) > 250 and sum(1 for x in out.split("\n") if x.startswith("C\t")) > 20
    out = replica_runs(["--db", db, "-t", "4", str(tmp_path / "r_1.fasta"), str(tmp_path / "r_2.fasta")], str(tmp_path), SMALL)
    assert len(out.strip().split("\n")) > 250


def test_cli_replicas_extract(tmp_path):
    fq = os.path.join(G, "cfg1_reads.fastq.gz")
    base = None
    for dv in (None,) + SETTINGS:
        env = dict(SMALL) if dv is None else dict(SMALL, CHARON_DEVICES=dv)
        pre = str(tmp_path / ("x%s" % (dv or "unset").replace(",", "_")))
        rc, out, err = run_cli(["--db", os.path.join(G, "cfg1.idx"), "--extract", "microbial", "--num_reads_to_fit", "20", "-p", pre, fq],
                               str(tmp_path), env)
        assert rc == 0, (dv, err)
        assert_same_tsv(out, open(os.path.join(G, "cfg1_expected_extract.tsv")).read())
        ext = gzip.decompress(open(pre + "_microbial.fastq.gz", "rb").read())
        assert ext.count(b"\n@") > 20
        if base is None:
            base = (out, ext)
        else:
            assert out == base[0] and ext == base[1], dv


def test_cli_replicas_classify_gamma(tmp_path):
    fq = os.path.join(G, "cfg1_reads.fastq.gz")
    out = replica_runs(["--db", os.path.join(G, "cfg1.idx"), "--dist", "gamma", fq], str(tmp_path), SMALL, sub="classify")
    assert len(out.strip().split("\n")) == 199


def test_cli_replicas_long_reads(tmp_path, oracle_lib):
    r = util.rng(808)
    gs = [util.random_seq(r, 200000), util.random_seq(r, 200000)]
    oidx = util.build_oracle_index(oracle_lib, [[gs[0]], [gs[1]]], [0, 1], ["host", "microbial"])
    oidx.compress()
    oidx.store(str(tmp_path / "l.idx"))
    oidx.free()
    reads = [util.mutate(r, gs[0][100:70100], 0.05), util.mutate(r, gs[1][:150000], 0.08), gs[0][5000:10000], b"ACGT" * 20000,
             util.mutate(r, gs[1][1000:66300], 0.02), gs[0][:65274] + b"N" * 40]
    reads = reads + reads[::-1] + reads
    with open(tmp_path / "long.fastq", "w") as f:
        for i, s in enumerate(reads):
            f.write("@L%d\n%s\n+\n%s\n" % (i, s.decode(), "I" * len(s)))
    env = {"CHARON_BATCH_READS": "2", "CHARON_BATCH_BASES": str(1 << 20)}
    for t in ("1", "4"):
        out = replica_runs(["--db", str(tmp_path / "l.idx"), "-t", t, str(tmp_path / "long.fastq")], str(tmp_path), env)
        assert len(out.strip().split("\n")) == len(reads) - 1


def test_cli_device_ordinal_out_of_range(tmp_path, api):
    n = api.device_count()
    fq = os.path.join(G, "cfg1_reads.fastq.gz")
    for dv in (str(n), "0,%d" % n):
        rc, out, err = run_cli(["--db", os.path.join(G, "cfg1.idx"), fq], str(tmp_path), {"CHARON_DEVICES": dv})
        assert rc != 0 and out == "", err
        assert ("device %d" % n) in err and ("device count %d" % n) in err, err
