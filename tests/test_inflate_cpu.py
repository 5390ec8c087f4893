"""CPU tests of the deflate member decoder behind chn_inflate_run_host -- the same decoder source k_inflate_members runs, on one host
thread.  The yardstick is Python's zlib (tests/inflate_cases.py): a member is accepted exactly where zlib's inflate accepts it, and
the bytes are zlib's."""
import ctypes
import os
import re

import pytest

from tests import inflate_cases as ic
from tests import util

NAMES = ["chn_inflate_create", "chn_inflate_run", "chn_inflate_run_host", "chn_inflate_destroy"]


def _header():
    return open(os.path.join(util.ROOT, "include", "charon_hip.h")).read()


def test_job_layout_matches_header():
    import charon_amd.api as api
    body = re.search(r"typedef struct chn_inflate_job \{(.*?)\} chn_inflate_job;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl
        ptr = "*" in decl
        base = re.match(r"(const\s+)?(\w+)", decl).group(2)
        for name in re.sub(r"^(const\s+)?\w+\s*", "", names).split(","):
            fields.append((name.replace("*", "").strip(), "ptr" if ptr else base))
    want = [(n.rstrip("_"), "ptr" if t is ctypes.c_void_p else {ctypes.c_uint32: "uint32_t", ctypes.c_uint64: "uint64_t"}[t])
            for n, t in api.InflateJob._fields_]
    assert fields == want
    assert [n for n, _ in fields] == ["struct_size", "flags", "n_members", "in", "in_bytes", "in_offset", "in_length", "out", "out_bytes",
                                     "out_offset", "out_length", "status"]
    assert ctypes.sizeof(api.InflateJob) == 88
    assert api.InflateJob.n_members.offset == 8 and api.InflateJob.out.offset == 48 and api.InflateJob.status.offset == 80
    assert api.INFLATE_MAX_OUT == 65536 and "#define CHN_INFLATE_MAX_OUT 65536u" in _header()


def test_names_declared_described_exported():
    import charon_amd.api as api
    header = _header()
    integration = open(os.path.join(util.ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in api.EXPORTS and getattr(api.lib(), name) is not None
        assert name in integration, name
    assert "one thread at a time" in header.lower().replace("\n * ", " ") or "ONE thread at a time" in header


def test_existing_struct_sizes_unchanged():
    import charon_amd.api as api
    sizes = {api.IndexDesc: 336, api.Model: 104, api.StreamCfg: 24, api.Batch: 96, api.Result: 80, api.TextBatch: 112, api.TextResult: 24,
             api.SynthReadsOut: 48}
    for t, n in sizes.items():
        assert ctypes.sizeof(t) == n, t


def test_member_set_is_what_it_claims():
    ic.check_member_set()


def test_member_set_on_the_host_decoder():
    import charon_amd.api as api
    good, bad, trailing = ic.member_set()
    every = good + bad + trailing
    res, st = api.inflate_host([m for _, m, _ in every], [s for _, _, s in every], guard=64)
    for (name, m, s), out, status in zip(every, res, st):
        ok, want = ic.yardstick(m, s)
        assert (status == 0) == ok, (name, int(status))
        if ok:
            assert out == want, name
    assert all(x == 0 for x in st[:len(good)]) and all(x != 0 for x in st[len(good):len(good) + len(bad)]) and st[-1] == 0
    # the status says what was wrong
    by_name = {n: int(x) for (n, _, _), x in zip(every, st)}
    assert by_name["block_type_3"] == 2 and by_name["stored_nlen"] == 2 and by_name["cut_in_half"] == 1
    assert by_name["one_too_small"] == 5 and by_name["one_too_large"] == 6 and by_name["match_first"] == 4
    assert by_name["hlit_31"] == 3 and by_name["oversubscribed"] == 3


@pytest.mark.parametrize("which", range(8))
def test_a_rejected_member_leaves_its_neighbours_intact(which):
    import charon_amd.api as api
    good, bad, _ = ic.member_set()
    small = [g for g in good if g[0] in ("fixed_one_byte", "empty", "run_of_a", "dynamic")]
    job = small[:2] + [bad[which]] + small[2:]
    res, st = api.inflate_host([m for _, m, _ in job], [s for _, _, s in job], guard=64)
    assert st[2] != 0 and res[2] is None
    for i in (0, 1, 3, 4):
        assert st[i] == 0 and res[i] == ic.yardstick(job[i][1], job[i][2])[1], job[i][0]


def test_mutation_sweep_agrees_with_zlib_on_every_case():
    import charon_amd.api as api
    cases, verdicts = ic.sweep_cases(), ic.sweep_verdicts()
    assert len(cases) == 5000
    res, st = api.inflate_host([m for m, _ in cases], [s for _, s in cases], guard=64)  # raises if a guard byte was touched
    wrong = [i for i, ((ok, _), status) in enumerate(zip(verdicts, st)) if (status == 0) != ok]
    assert not wrong, (len(wrong), wrong[:10], [int(st[i]) for i in wrong[:10]])
    assert all(out == want for out, (ok, want) in zip(res, verdicts) if ok)
    accepted = sum(1 for ok, _ in verdicts if ok)
    print("sweep: %d of %d cases accepted by zlib" % (accepted, len(cases)))
    assert 0 < accepted < len(cases)


def test_crafted_and_foreign_sets_are_what_they_claim():
    """by zlib and by the profiler of tests/deflate_writer.py, neither of which is the code under test"""
    ic.check_crafted_set()
    ic.check_foreign_set()
    ic.check_crafted_sweep()


# statuses of the named rejects, as they follow from inflate_members.inc: 3 (INF_E_LENGTHS) where the header or a code set is at
# fault, 4 (INF_E_SYMBOL) where a symbol or a distance is
CRAFTED_STATUS = {"one_dist_code_unused_bit": 4, "empty_dist_used": 4, "only_eob_unused_bit": 4, "first_is_16": 3, "repeat_overruns": 3,
                  "no_eob": 3, "incomplete_ll": 3, "oversub_ll": 3, "fixed_286": 4, "fixed_dist30": 4, "dist_11_of_10": 4, "hdist_31": 3}


def test_crafted_and_foreign_members_on_the_host_decoder():
    import zlib
    import charon_amd.api as api
    good, bad = ic.crafted_set()
    every = good + bad + [(n, m, s) for n, m, s, _ in ic.foreign_set()]
    ms, sizes = [m for _, m, _ in every], [s for _, _, s in every]
    verdicts = [ic.yardstick(m, s) for m, s in zip(ms, sizes)]
    res, st = api.inflate_host(ms, sizes, guard=64)
    for (name, _, _), (ok, want), out, status in zip(every, verdicts, res, st):
        assert (status == 0) == ok, (name, int(status))
        assert out == want, name
    assert [n for (n, _, _), (ok, _) in zip(every, verdicts) if not ok] == [n for n, _, _ in bad]
    assert {n: int(x) for (n, _, _), x in zip(every, st) if x != 0} == CRAFTED_STATUS
    cres, cst, crc = api.inflate_host(ms, sizes, guard=64, want_crc=True)
    assert (cst == st).all() and cres == res
    for (name, _, _), (ok, want), got in zip(every, verdicts, crc):
        if ok:
            assert int(got) == (zlib.crc32(want) & 0xFFFFFFFF), name
    for (name, _, _, want), got in zip(ic.foreign_set(), crc[len(good) + len(bad):]):
        assert int(got) == want, name  # the fixture's own CRC-32


def test_crafted_sweep_agrees_with_zlib_on_every_case():
    import charon_amd.api as api
    cases, verdicts = ic.crafted_sweep(), ic.crafted_sweep_verdicts()
    assert len(cases) == 3400
    res, st = api.inflate_host([m for m, _ in cases], [s for _, s in cases], guard=64)  # raises if a guard byte was touched
    wrong = [i for i, ((ok, _), status) in enumerate(zip(verdicts, st)) if (status == 0) != ok]
    assert not wrong, (len(wrong), wrong[:10], [int(st[i]) for i in wrong[:10]])
    assert all(out == want for out, (ok, want) in zip(res, verdicts) if ok)
    accepted = sum(1 for ok, _ in verdicts if ok)
    print("crafted sweep: %d of %d cases accepted by zlib" % (accepted, len(cases)))


def _job(n=3):
    import charon_amd.api as api
    good, _, _ = ic.member_set()
    pick = [g for g in good if g[0] in ("fixed_one_byte", "run_of_a", "dynamic")][:n]
    return api.inflate_job([m for _, m, _ in pick], [s for _, _, s in pick])


@pytest.mark.parametrize("case", ["in_beyond", "out_length_too_large", "out_beyond", "out_overlap"])
def test_descriptor_errors_are_invalid_and_name_the_member(case):
    import charon_amd.api as api
    j, a = _job()
    if case == "in_beyond":
        a["in_length"][1] += 1 + int(a["in_length"][2])
    elif case == "out_length_too_large":
        a["out_length"][1] = 65537
        j.out_bytes += 1 << 20
    elif case == "out_beyond":
        a["out_offset"][2] = j.out_bytes - 1
    else:
        a["out_offset"][2] = a["out_offset"][1] + a["out_length"][1] - 1
    before = a["out"].copy()
    rc = api.lib().chn_inflate_run_host(ctypes.byref(j))
    assert rc == -1  # CHN_E_INVALID
    msg = api.lib().chn_last_error().decode()
    assert ("member %d" % (1 if case in ("in_beyond", "out_length_too_large") else 2)) in msg, msg
    assert (a["out"] == before).all() and (a["status"] == 0xFFFFFFFF).all()  # nothing ran


def test_empty_job_and_bad_struct():
    import charon_amd.api as api
    res, st = api.inflate_host([], [])
    assert res == [] and len(st) == 0
    j, a = _job()
    j.struct_size -= 8
    assert api.lib().chn_inflate_run_host(ctypes.byref(j)) == -1
    j, a = _job()
    j.flags = 1
    assert api.lib().chn_inflate_run_host(ctypes.byref(j)) == -1


def test_switch_value_is_checked_and_off_is_todays_path(tmp_path):
    """CHARON_GPU_INFLATE: anything but 0 / 1 ends the run with status 1 before a file is opened; 0 is the path of the unset switch"""
    import subprocess
    exe = os.path.join(util.ROOT, "charon_amd", "bin", "charon")
    text = ic.fastq_text(30000, 4)
    text = text[:text.rindex(b"\n@") + 1]
    f = tmp_path / "r.fastq.gz"
    f.write_bytes(ic.bgzf(text, block=4000))
    env = {k: v for k, v in os.environ.items() if k not in ("CHARON_GPU_INFLATE", "CHARON_NO_BGZF")}
    runs = {}
    for v in (None, "0", "2", ""):
        e = dict(env) if v is None else dict(env, CHARON_GPU_INFLATE=v)
        runs[v] = subprocess.run([exe, "_records", str(f), "50", "10000"], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert runs[None].returncode == 0 and runs[None].stdout.count(b"\n") > 40
    assert runs["0"].returncode == 0 and runs["0"].stdout == runs[None].stdout
    for v in ("2", ""):
        assert runs[v].returncode == 1 and runs[v].stdout == b"" and b"charon: CHARON_GPU_INFLATE: " in runs[v].stderr
    (tmp_path / "none.idx").write_bytes(b"not an index")
    for sub in ("dehost", "classify"):
        p = subprocess.run([exe, sub, "--db", str(tmp_path / "none.idx"), str(f)], env=dict(env, CHARON_GPU_INFLATE="on"), cwd=str(tmp_path),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 1 and b"charon: CHARON_GPU_INFLATE: " in p.stderr and b"none.idx" not in p.stderr
