"""GPU tests (-m gpu) of `charon index -k K -w W`: for pairs away from the default geometry -- the unpacked window ring (27, 29), wn = 1
(21, 21), a wide window (15, 120), a small k (11, 41) -- the .idx holds the parameters, the category map and the words of the oracle's
sequential builder Index.from_fasta(..., k=K, w=W); the same bytes come from tiny pieces and from the device-resident sets with the
Elias-Fano encoder on the device; `charon dehost --db` on it writes the oracle's TSV.  And the option rules: -k 28, -k 0, -w below -k."""
import os
import subprocess

import numpy as np
import pytest

from tests import index_build_cases as cases
from tests import util
from tests.test_gpu_cli import assert_same_tsv

pytestmark = pytest.mark.gpu
EXE = os.path.join(util.ROOT, "charon_amd", "bin", "charon")
OURS = ("CHARON_GPU_INDEX_SETS", "CHARON_INDEX_SETS_BUDGET", "CHARON_INDEX_SETS_COMPACT", "CHARON_GPU_INDEX_EF", "CHARON_INDEX_EF_SLICE", "CHARON_INDEX_PIECE")
CATS = ["microbial", "human", "microbial", "human"]
TIMEOUT = 120


def run(args, cwd, **env):
    e = {k: v for k, v in os.environ.items() if k not in OURS}
    e.update(env)
    return subprocess.run([EXE] + [str(a) for a in args], cwd=str(cwd), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT)


def index(tmp, name, k, w, **env):
    return run(["index", "-k", k, "-w", w, "-p", tmp / name, "--log", tmp / (name + ".log"), tmp / "in.tab"], tmp, **env)


def write_references(tmp, k, w, r):
    """four files shaped like those of test_cli_index_builds_the_same_index_as_the_oracle: a 30 kb record (cut into chunks); records with
    an N run, a lower-case stretch and a repeat; records of w - 1, w and w + 1 bases; a record of k - 1 bases beside a plain one"""
    big = util.random_seq(r, 9000).decode()
    shapes = [[util.random_seq(r, 30000).decode()],
              [util.random_seq(r, 9000).decode(), big[:4000] + "N" * 30 + big[4030:6000].lower() + "AC" * 200 + big[6400:], util.random_seq(r, 9000).decode()],
              [util.random_seq(r, n).decode() for n in (w - 1, w, w + 1)],
              [util.random_seq(r, 5000).decode(), util.random_seq(r, k - 1).decode()]]
    files = []
    for i, seqs in enumerate(shapes):
        path = tmp / ("ref%d.fa" % i)
        with open(path, "w") as f:
            for j, s in enumerate(seqs):
                f.write(">rec%d_%d\n" % (i, j))
                f.write("\n".join(s[c:c + 70] for c in range(0, len(s), 70)) + "\n")
        files.append(str(path))
    with open(tmp / "in.tab", "w") as f:
        for p, c in zip(files, CATS):
            f.write("%s\t%s\n" % (p, c))
    return files, [shapes[0][0], shapes[1][0]]


@pytest.fixture(scope="module", params=cases.KW_CLI, ids=cases.kw_id)
def built(request, tmp_path_factory):
    k, w = request.param
    tmp = tmp_path_factory.mktemp("index_%d_%d" % (k, w))
    r = util.rng(600 + 31 * k + w)
    files, genomes = write_references(tmp, k, w, r)
    p = index(tmp, "built", k, w)
    assert p.returncode == 0, p.stderr.decode()
    return dict(tmp=tmp, k=k, w=w, r=r, files=files, genomes=genomes, data=open(tmp / "built.idx", "rb").read())


@pytest.fixture(scope="module")
def twin(built, oracle_lib):
    """the oracle's index of the same files (in the category order of the file the CLI wrote) and that file as the oracle loads it"""
    got = oracle_lib.Index.load(str(built["tmp"] / "built.idx"))
    want = oracle_lib.Index.from_fasta(list(zip(built["files"], CATS)), got.categories, k=built["k"], w=built["w"])
    yield got, want
    got.free()
    want.free()


def test_the_index_is_the_oracles(built, twin):
    got, want = twin
    assert (got.k, got.w) == (built["k"], built["w"]) == (want.k, want.w)
    assert sorted(got.categories) == ["human", "microbial"] and got.categories == want.categories
    assert (got.bins, got.bin_size, got.hash_funs) == (want.bins, want.bin_size, want.hash_funs) and got.bins == 4
    assert list(got.bin_to_cat) == list(want.bin_to_cat)
    assert want.words().any()
    assert np.array_equal(got.words(), want.words())


def test_the_same_bytes_from_tiny_pieces(built):
    p = index(built["tmp"], "pieces", built["k"], built["w"], CHARON_INDEX_PIECE="4096")
    assert p.returncode == 0, p.stderr.decode()
    assert open(built["tmp"] / "pieces.idx", "rb").read() == built["data"]


def test_the_same_bytes_from_device_sets_and_device_elias_fano(built):
    p = index(built["tmp"], "sets_ef", built["k"], built["w"], CHARON_GPU_INDEX_SETS="1", CHARON_GPU_INDEX_EF="1")
    assert p.returncode == 0, p.stderr.decode()
    assert open(built["tmp"] / "sets_ef.idx", "rb").read() == built["data"]
    assert "CHARON_GPU_INDEX_SETS=1: the minimiser sets of 4 of 4 bins stayed on device" in open(built["tmp"] / "sets_ef.log").read()


def test_dehost_on_it_writes_the_oracles_rows(built, twin):
    got, want = twin
    tmp = built["tmp"]
    reads = util.sample_reads(built["r"], [g.encode() for g in built["genomes"]], 60, (200, 900))
    with open(tmp / "q.fastq", "w") as f:
        for i, s in enumerate(reads):
            f.write("@q%d\n%s\n+\n%s\n" % (i, s.decode(), "I" * len(s)))
    p = run(["dehost", "--db", tmp / "built.idx", tmp / "q.fastq", "--log", tmp / "d.log"], tmp)
    assert p.returncode == 0, p.stderr.decode()
    out = p.stdout.decode()
    assert sum(1 for x in out.split("\n") if x.startswith("C\t")) > 10
    assert_same_tsv(out, want.dehost_files(str(tmp / "q.fastq")))


@pytest.mark.parametrize("args,rule", [(("-k", "28"), "K must be at most 27"), (("-k", "0"), "K must be a positive integer"),
                                       (("-k", "19", "-w", "18"), "W must be greater than K"), (("-k", "25", "-w", "24"), "W must be greater than K")])
def test_option_rules(tmp_path, args, rule):
    with open(tmp_path / "g.fa", "w") as f:
        f.write(">g\n%s\n" % util.random_seq(util.rng(9), 3000).decode())
    (tmp_path / "in.tab").write_text("%s\tmicrobial\n" % (tmp_path / "g.fa"))
    p = run(["index"] + list(args) + ["-p", tmp_path / "no", "--log", tmp_path / "no.log", tmp_path / "in.tab"], tmp_path)
    assert p.returncode != 0
    assert rule in p.stderr.decode(), p.stderr.decode()
    assert not (tmp_path / "no.idx").exists()
