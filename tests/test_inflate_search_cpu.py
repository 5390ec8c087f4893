"""CPU tests of chn_inflate_stream_search_host -- the filter and the trial of parts/inflate_search.inc on one host thread -- against the
independent restatement of the rule in tests/inflate_search_cases.py, and of the front end's own search (FastInflate::find_block, through
`charon _find_blocks`) against the same call."""
import ctypes
import os
import re
import subprocess

import pytest

from tests import inflate_search_cases as sc
from tests import util

NAMES = ["chn_inflate_stream_search_host"]
EXE = os.path.join(util.ROOT, "charon_amd", "bin", "charon")


def _header():
    return open(os.path.join(util.ROOT, "include", "charon_hip.h")).read()


def test_job_layout_matches_header():
    import charon_amd.api as api
    body = re.search(r"typedef struct chn_inflate_search_job \{(.*?)\} chn_inflate_search_job;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ptr = "*" in decl
        base = re.match(r"(const\s+)?(\w+)", decl).group(2)
        for name in re.sub(r"^(const\s+)?\w+\s*", "", decl).split(","):
            fields.append((name.replace("*", "").strip(), "ptr" if ptr else base))
    want = [(n.rstrip("_"), "ptr" if t is ctypes.c_void_p else {ctypes.c_uint32: "uint32_t", ctypes.c_uint64: "uint64_t"}[t])
            for n, t in api.InflateSearchJob._fields_]
    assert fields == want
    assert [n for n, _ in fields] == ["struct_size", "flags", "n_ranges", "in", "in_bytes", "from_bit", "to_bit", "found_bit"]
    assert ctypes.sizeof(api.InflateSearchJob) == 56
    assert api.INFLATE_SEARCH_NONE == 2 ** 64 - 1 and "#define CHN_INFLATE_SEARCH_NONE (~(uint64_t)0)" in _header()
    assert ctypes.sizeof(api.InflateStreamJob) == 144  # no existing struct changed


def test_names_declared_described_exported():
    import charon_amd.api as api
    header = _header()
    integration = open(os.path.join(util.ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in api.EXPORTS and getattr(api.lib(), name) is not None
        assert name in integration, name
    for rule in ("R0", "R1", "R2", "R3", "R4", "R5", "R6"):
        assert re.search(r"\b%s\b" % rule, header), rule
    assert "CANDIDATE" in header and header.count("src/dehost_main.cpp:324") == 2


CRAFTED = sc.crafted_cases()


@pytest.mark.parametrize("case", CRAFTED, ids=[c["name"] for c in CRAFTED])
def test_crafted_stream(case):
    import charon_amd.api as api
    sc.check(sc.run(api.inflate_search_host, case), case)


def test_the_crafted_set_holds_what_it_claims():
    names = [c["name"] for c in sc.all_cases()]
    assert len(set(names)) == len(names)
    decoys = sc.decoy_cases()
    assert {c["why"] for c in decoys} >= {"r1", "r2", "repeat of nothing", "repeat past the end", "no end-of-block code", "over-subscribed",
                                           "incomplete", "not text", "fewer than 32 symbols", "block type 3", "LEN / NLEN", None}
    for c in decoys:
        sc.check_decoy(c)
    assert {c["name"] for c in sc.alignment_cases()} == {"align_%d" % k for k in range(8)}


LIMIT = list(sc.limit_cases())


@pytest.mark.parametrize("case", LIMIT, ids=[c["name"] for c in LIMIT])
def test_the_limit_of_32768_symbols(case):
    import charon_amd.api as api
    sc.check(sc.run(api.inflate_search_host, case), case)


def test_noise_walks_the_filters():
    import charon_amd.api as api
    census = sc.noise_census()
    for name, r1, r2, r3 in census:
        print("%s: %d positions pass R0 - R1, %d R2, %d R3" % (name, r1, r2, r3))
        assert r2 > 100 and r1 > 50 * r2  # the filters were exercised, on either side
    # noise alone has no survivor of R3 (inflate_search_cases.planted); the planted pieces are where R3 passes, one in every lane
    assert all(r3 >= 64 for name, _, _, r3 in census if name.startswith("planted"))
    for c in sc.noise_cases() + sc.planted_cases():
        assert len(c["ranges"]) in (1, 17, 97)
        sc.check(sc.run(api.inflate_search_host, c), c)


def test_zlib_streams_in_ranges_of_4_and_20_kib():
    import charon_amd.api as api
    for c in sc.real_cases():
        want = sc.expected(c)
        sc.check(sc.run(api.inflate_search_host, c), c)
        assert sum(1 for w in want if w is not None) >= 5, c["name"]  # these streams have blocks to find


def test_600_ranges_unordered_and_overlapping():
    import charon_amd.api as api
    c = sc.cursor_case()
    assert len(c["ranges"]) == 600 and sum(1 for t in c["true"] if t is not sc.ANY) >= 20
    sc.check(sc.run(api.inflate_search_host, c), c)


INVALID = ["struct_size", "flag", "too_many", "null_from", "null_to", "null_found", "null_in", "from_behind_to", "to_beyond_in"]


@pytest.mark.parametrize("name", INVALID)
def test_invalid_jobs_are_refused_and_nothing_is_written(name):
    import charon_amd.api as api
    jobs = {n: (j, a, says) for n, j, a, says in sc.invalid_jobs(api)}
    assert sorted(jobs) == sorted(INVALID)
    j, a, says = jobs[name]
    assert api.lib().chn_inflate_stream_search_host(ctypes.byref(j)) == -1  # CHN_E_INVALID
    msg = api.lib().chn_last_error().decode()
    assert "chn_inflate_stream_search_host" in msg and says in msg, msg
    assert (a["found_bit"] == 0xA5A5A5A5A5A5A5A5).all()


def test_empty_jobs_and_empty_ranges():
    import charon_amd.api as api
    assert api.inflate_search_host(b"", [], []) == []
    j, a = api.inflate_search_job(sc.noise(1)[:100], [0, 5], [800, 5])
    j.n_ranges = 0
    assert api.lib().chn_inflate_stream_search_host(ctypes.byref(j)) == 0 and (a["found_bit"] == 0xA5A5A5A5A5A5A5A5).all()
    assert api.inflate_search_host(sc.noise(1)[:100], [5, 800, 0], [5, 800, 0]) == [None, None, None]


# ---- the front end ---------------------------------------------------------------------------------------------------------------------
GZIP_HEADER = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3])


def _find_blocks(path, chunk, first):
    p = subprocess.run([EXE, "_find_blocks", str(path), str(chunk), str(first)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr
    rows = [line.split() for line in p.stdout.decode().splitlines()]
    return [(int(a), int(b), None if c == "-" else int(c)) for a, b, c in rows]


def _same_as_find_block(tmp_path, name, data, chunk):
    """`data` behind a gzip header as a file: FastInflate::find_block over ranges of `chunk` bytes from the header's end on, and the new
    call over the same bytes and ranges, position for position"""
    import charon_amd.api as api
    whole = GZIP_HEADER + bytes(data)
    f = tmp_path / (name + ".gz")
    f.write_bytes(whole)
    rows = _find_blocks(f, chunk, len(GZIP_HEADER))
    assert rows and rows[0][0] == 8 * len(GZIP_HEADER) and rows[-1][1] == 8 * len(whole)
    got = api.inflate_search_host(whole, [r[0] for r in rows], [r[1] for r in rows])
    assert got == [r[2] for r in rows], (name, chunk, [(r, g) for r, g in zip(rows, got) if r[2] != g][:5])
    return got


def test_find_block_of_the_front_end_agrees_on_zlib_streams(tmp_path):
    seen = set()
    for c in sc.real_cases():
        if c["data"] in seen:
            continue
        seen.add(c["data"])
        for chunk in (4096, 20480):
            got = _same_as_find_block(tmp_path, c["name"], c["data"], chunk)
            assert sum(1 for g in got if g is not None) >= 5


def test_find_block_of_the_front_end_at_the_limit(tmp_path):
    """find_block takes up to three literals out of one refill and looks at its limit only in front of the first of them, so it may
    read -- and be refuted by -- one or two literals behind symbol 32 768 where R4 reads nothing: it is the stricter of the two on
    limit_nontext_at_32768 (its literals come in threes from symbol 0: 32 766, 32 767, 32 768) and agrees on every other limit case.
    Both answers are candidates only; find_block is not changed here."""
    import charon_amd.api as api
    for c in sc.limit_cases():
        whole = GZIP_HEADER + c["data"]
        f = tmp_path / (c["name"] + ".gz")
        f.write_bytes(whole)
        (frm, to, at), = _find_blocks(f, 1 << 20, len(GZIP_HEADER))
        rule = api.inflate_search_host(whole, [frm], [to])[0]
        if c["name"] == "limit_nontext_at_32768":
            assert rule == 8 * len(GZIP_HEADER) + c["true"][0] and at is not None and at > rule
        else:
            assert at == rule, c["name"]


def test_find_block_of_the_front_end_agrees_on_the_decoys(tmp_path):
    cases = sc.decoy_cases() + sc.follower_cases() + sc.distance_set_cases() + sc.alignment_cases()
    cases += [c for c in sc.input_end_cases() if len(c["data"]) >= 8]  # (the front end takes no file of fewer than 18 bytes)
    for c in cases:
        for chunk in (16, 1 << 20):
            _same_as_find_block(tmp_path, c["name"], c["data"], chunk)
