"""GPU tests (-m gpu) of the two probe streams: consecutive batches' minimise+probe kernels go to two HIP streams alternately, so two probe
grids can be on the device at once, each with its own slot (control words, length order, row log, result arrays).

Yardsticks, none of which is the code under test: the CPU oracle (util.assert_parity) and the same batch run ALONE -- one in flight, on a
fresh stream -- compared in all seven result columns, bit for bit including the probabilities (util.assert_same_results).  What could go
wrong is plumbing: a result or a control word in the wrong slot, a kernel that starts before what it reads is there, a re-run or a
list-mode call that meets a neighbour's kernel.  Index and read-set builders are those of tests/test_gpu_device_batches.py."""
import time

import numpy as np
import pytest

from tests import util
from tests import test_gpu_device_batches as dbt

pytestmark = pytest.mark.gpu

COLUMNS = dbt.COLUMNS
# three distinct sets per index; the 8-bin index has its host category last, so it takes pairs (call_category)
SETS = {"fused": ("pairs", "pairs_n", "pairs_full_n"), "rows": ("se", "se_n", "se_full_n")}


@pytest.fixture(scope="module")
def api():
    import charon_amd.api as api
    return api


@pytest.fixture(scope="module")
def world(api, oracle_lib):
    gs = dbt.make_genomes()
    fused, rows = dbt.build_indices(oracle_lib, gs)
    # the 8-bin fused shape with the host category FIRST: single-end dehost (the only form whose long reads are split) can use it
    fused_se = util.build_oracle_index(oracle_lib, [[g] for g in gs], list(range(8)), ["host"] + ["c%d" % i for i in range(7)])
    assert fused_se.host_index == 0
    sets = dbt.make_sets(gs)
    sets["se_rev"] = (list(reversed(sets["se"][0])), None)
    w = dict(gs=gs, fused=fused, rows=rows, fused_se=fused_se, sets=sets, memo={}, gf=util.gpu_index_from_oracle(api, fused),
             gr=util.gpu_index_from_oracle(api, rows), gs_=util.gpu_index_from_oracle(api, fused_se))
    yield w
    for key in ("gf", "gr", "gs_"):
        w[key].destroy()
    for key in ("fused", "rows", "fused_se"):
        w[key].free()


GIDX = {"fused": "gf", "rows": "gr", "fused_se": "gs_"}


def make_stream(api, world, index, paired, names, **kw):
    gidx = world[GIDX[index]]
    packed = {}
    for name in names:
        reads, mates = world["sets"][name]
        packed[name] = dbt.packed_and_device(api, reads, mates)
    st = api.Stream(gidx, 333, max(p["n_bases"] for p, _ in packed.values()), **kw)
    st.set_model(dbt.model_for(api, gidx, paired))
    return st, packed


def submit(st, packed, name, host):
    p, db = packed[name]
    if host:
        st.submit_host(p, *dbt.host_columns(333))
    else:
        db.submit(st)


def wait(api, st, host):
    return st.wait_host() if host else dbt.wait_downloaded(api, st, 333)


def pipelined(api, st, packed, plan, depth=3):
    """plan: [(set name, host form)]; `depth` batches in flight; -> the results in order"""
    outs, k = [], 0
    while k < min(depth - 1, len(plan)):
        submit(st, packed, *plan[k])
        k += 1
    for i in range(len(plan)):
        if k < len(plan):
            submit(st, packed, *plan[k])
            k += 1
        outs.append(wait(api, st, plan[i][1]))
    return outs


def assert_oracle(out, orc, host):
    """a host batch's rows are all the oracle's; a device batch's results are never re-evaluated on the host, so its rows flagged as a
    near tie are the caller's to decide (tests/test_gpu_device_batches.py): every integer column, and parity where no flag is set"""
    if host:
        return util.assert_parity(out, orc)
    for key in ("num_hashes", "counts", "unique", "conf"):
        assert np.array_equal(out[key], orc[key]), key
    keep = out["flags"] == 0
    assert keep.sum() >= 0.95 * keep.size
    util.assert_parity(dbt.rows_of(out, keep), dbt.rows_of(orc, keep))


def free_all(st, packed):
    st.destroy()
    for _, db in packed.values():
        db.free()


# ---- 1. small, every form -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", ["fused", "rows"])
def test_six_batches_three_in_flight_equal_the_oracle_and_their_run_alone(api, world, index):
    """six batches from three distinct 333-read sets, host and device-resident batches alternately, three in flight: each equals the
    oracle and the same batch (same form) alone on a fresh stream"""
    names, paired = SETS[index], index == "fused"
    plan = [(names[i % 3], i % 2 == 0) for i in range(6)]   # each set comes by once in either form
    st, packed = make_stream(api, world, index, paired, names)
    try:
        alone = {}
        for name, host in plan:
            submit(st, packed, name, host)
            alone[(name, host)] = wait(api, st, host)
    finally:
        st.destroy()
    st = api.Stream(world[GIDX[index]], 333, max(p["n_bases"] for p, _ in packed.values()))
    st.set_model(dbt.model_for(api, world[GIDX[index]], paired))
    try:
        outs = pipelined(api, st, packed, plan)
    finally:
        free_all(st, packed)
    assert len(outs) == 6
    for (name, host), out in zip(plan, outs):
        util.assert_parity(out, dbt.oracle_of(world, index, name))
        util.assert_same_results(out, alone[(name, host)], keys=COLUMNS)
    # (the sets differ in what comes out: a result in the wrong slot would show)
    assert not np.array_equal(outs[0]["num_hashes"], outs[1]["num_hashes"]) and not np.array_equal(outs[1]["num_hashes"], outs[2]["num_hashes"])


# ---- 2. two grids on the device -----------------------------------------------------------------------------------------------
def test_two_probe_grids_coexist_and_profile_counts_no_time_twice(api, oracle_lib):
    """262 144 device-made 1 kb reads are 4 096 wavefronts, more than the device holds at once (seven per CU): with three in flight
    batch i + 1's grid is dispatched while batch i's drains.  Results equal the run-alone results; the first 4 096 reads of each set
    equal the oracle (index rows pulled back from the device).  chn_stream_profile(0) is the time attributable to each probe kernel:
    six launches whose total cannot exceed the host-clock time around them (both ends synchronised: the union of the device intervals
    lies inside the wall interval); one in flight: positive and within the whole chain's time."""
    from charon_amd import pack
    B, S, n, L, glen, head = 100, 1 << 20, 1 << 18, 1000, 1 << 16, 4096
    b2c = [b % 2 for b in range(B)]
    g = api.Index(api.make_desc(B, S, b2c, 2, 0))
    assert g.desc.bin_words == 2
    gen = api.synth_genomes(0, 43, B, glen)
    g.synth_fill(43, 0.1)
    g.synth_plant(gen, B, glen, list(range(B)))
    sets = [api.synth_reads(0, 42, gen, B, glen, n, L, L, 0.05, 0.1, 40.0, first_read_id=j * n) for j in range(3)]
    max_bases = max(int(rd.n_bases) for rd in sets)

    def sub(st, rd):
        st.submit_device(n, rd.n_bases, rd.bases2, rd.seg1_offset, rd.seg1_length, rd.mean_quality, rd.compression)

    def new_stream():
        st = api.Stream(g, n, max_bases, profile=True)
        st.set_model(api.default_model(2, 0))
        return st
    try:
        # alone, one in flight, on a profiling stream of its own
        st1 = new_stream()
        alone = []
        for rd in sets:
            sub(st1, rd)
            alone.append(util.download_results(api, st1.wait_device(), n, 2))
        k1_ms, k1_n = st1.profile(0)
        chain_ms, chain_n = st1.profile(3)
        st1.destroy()
        print("one in flight: probe %.3f ms over %d launches, whole chain %.3f ms" % (k1_ms, k1_n, chain_ms))
        assert k1_n == 3 and chain_n == 3 and 0 < k1_ms <= chain_ms
        # six batches, three in flight
        st = new_stream()
        st.sync()
        outs = []
        t0 = time.perf_counter()
        sub(st, sets[0])
        sub(st, sets[1])
        for i in range(6):
            if i + 2 < 6:
                sub(st, sets[(i + 2) % 3])
            res = st.wait_device()
            if i >= 3:  # (the first three are waited for without a download in between, so that the grids queue up as in a caller's loop)
                outs.append(util.download_results(api, res, n, 2))
        st.sync()
        wall_ms = (time.perf_counter() - t0) * 1e3
        p_ms, p_n = st.profile(0)
        print("three in flight: probe %.3f ms over %d launches, wall %.3f ms" % (p_ms, p_n, wall_ms))
        assert p_n == 6 and 0 < p_ms <= wall_ms
        assert st.profile(4)[1] == 0
        st.profile(0, reset=True)
        assert st.profile(0) == (0.0, 0)
        # every set once more, pipelined, for the first three results
        sub(st, sets[0])
        sub(st, sets[1])
        sub(st, sets[2])
        first = [util.download_results(api, st.wait_device(), n, 2) for _ in range(3)]
        st.destroy()
        for j in range(3):
            util.assert_same_results(outs[j], alone[j], keys=COLUMNS)
            util.assert_same_results(first[j], alone[j], keys=COLUMNS)
        assert not np.array_equal(alone[0]["num_hashes"], alone[1]["num_hashes"])
        # the oracle on the first reads of each set
        oidx = oracle_lib.Index.new(B, S, b2c, ["human", "microbial"])
        oidx.words()[:] = g.download()
        for j, rd in enumerate(sets):
            lens = api.device_download(0, rd.seg1_length, head * 4, np.uint32)
            offs = api.device_download(0, rd.seg1_offset, head * 8, np.uint64)
            nb = int(offs[-1]) + (L + 63) // 64 * 64
            reads = pack.unpack_reads(api.device_download(0, rd.bases2, nb // 4, np.uint32), offs, lens)
            cat, o, _ = util.concat(reads)
            orc = oidx.process_reads(cat, o, threads=8)
            got = dbt.rows_of(alone[j], slice(0, head))
            # device results are not re-evaluated on the host: rows flagged as a near tie are the caller's (tests/test_gpu_device_batches.py)
            for key in ("num_hashes", "counts", "unique", "conf"):
                assert np.array_equal(got[key], orc[key]), (j, key)
            keep = got["flags"] == 0
            assert keep.sum() >= 0.95 * head
            util.assert_parity(dbt.rows_of(got, keep), dbt.rows_of(orc, keep))
            assert (orc["call"] == 0).sum() > head // 8 and (orc["call"] == 1).sum() > head // 8
        oidx.free()
    finally:
        for rd in sets:
            util.free_synth_reads(api, rd)
        api.device_free(0, gen)
        g.destroy()


# ---- 3. the overflow re-run beside a running neighbour --------------------------------------------------------------------------
def test_overflow_reruns_with_three_in_flight(api, world):
    """CHN_STREAM_TINY_LOG on the row-log index (the fused path keeps no row log, so nothing of it can overflow): every batch overruns
    its log and chn_batch_wait runs it again on the stream's worst-case buffers while the two batches behind it are on the device"""
    names = ("se", "se_n", "se_rev")
    plan = [(names[i % 3], i % 2 == 0) for i in range(6)]
    st, packed = make_stream(api, world, "rows", False, names, tiny_log=True)
    try:
        outs = pipelined(api, st, packed, plan)
        reruns = st.profile(4)[1]
    finally:
        free_all(st, packed)
    orc_rev = {k: v[::-1] for k, v in dbt.oracle_of(world, "rows", "se").items() if isinstance(v, np.ndarray)}
    for (name, host), out in zip(plan, outs):
        util.assert_parity(out, orc_rev if name == "se_rev" else dbt.oracle_of(world, "rows", name))
    assert reruns == 6


# ---- 4. long reads --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", ["fused_se", "rows"])
def test_split_launches_with_three_in_flight(api, world, index):
    """split_bucket = 64: the reads of 1 024 bases and more take the SPLIT launch (its end awaited by the count kernel
    whichever probe stream the ordinary launch went to; the first batches alternate, those submitted after a batch with long reads has
    been waited for take the first stream); single-end, the only form that is split"""
    names = ("se", "se_n", "se_rev")
    for name in names:
        assert sum(len(s) >= 1024 for s in world["sets"][name][0]) >= 2
    plan = [(names[i % 3], i % 2 == 0) for i in range(6)]
    st, packed = make_stream(api, world, index, False, names, split_bucket=64)
    try:
        outs = pipelined(api, st, packed, plan)
        assert st.profile(4)[1] == 0
    finally:
        free_all(st, packed)

    def orc_of(name):
        key = (index, name)
        if key not in world["memo"]:
            world["memo"][key] = dbt.oracle_run(world[index], *world["sets"][name])
        return world["memo"][key]
    for (name, host), out in zip(plan, outs):
        assert_oracle(out, orc_of(name), host)


# ---- 5. hand-over to the list-mode calls ----------------------------------------------------------------------------------------
def test_list_mode_calls_between_batches(api, world, oracle_lib):
    """three batches, then chn_minimisers and the dense row-sharded chain at one rank (both on the first probe stream, with nothing in
    flight), then three more batches: all equal the oracle"""
    names = ("se", "se_n", "se_rev")
    plan = [(names[i % 3], i % 2 == 1) for i in range(3)]
    gidx = world["gr"]
    st, packed = make_stream(api, world, "rows", False, names)
    orc = dbt.oracle_of(world, "rows", "se")
    orc_rev = {k: v[::-1] for k, v in orc.items() if isinstance(v, np.ndarray)}
    partial = None
    try:
        before = pipelined(api, st, packed, plan)
        p, db = packed["se"]
        mins = st.minimisers_host(p)
        want = np.concatenate([np.asarray(oracle_lib.minimisers(s.decode()), np.uint64) for s in world["sets"]["se"][0] if len(s)] or [np.zeros(0, np.uint64)])
        e = st.shard_minimise_device(333, p["n_bases"], db.bases2, db.seg1_offset, db.seg1_length, db.mean_quality, db.compression)
        nwords = e * gidx.desc.hash_funs * gidx.desc.bin_words
        partial = api.device_malloc(0, max(nwords, 2) * 8)
        st.shard_probe(gidx, partial, nwords)
        st.shard_finish(partial)
        chain = dbt.wait_downloaded(api, st, 333)
        after = pipelined(api, st, packed, plan)
    finally:
        free_all(st, packed)
        if partial:
            api.device_free(0, partial)
    assert e == int(orc["num_hashes"].sum()) and np.array_equal(np.sort(mins), np.sort(want))
    util.assert_parity(chain, orc)
    for outs in (before, after):
        for (name, host), out in zip(plan, outs):
            util.assert_parity(out, orc_rev if name == "se_rev" else dbt.oracle_of(world, "rows", name))
    for a, b in zip(before, after):
        util.assert_same_results(a, b, keys=COLUMNS)


# ---- 6. more long reads than SPLIT workgroups -----------------------------------------------------------------------------------
def test_split_workgroups_loop_over_more_long_reads_than_the_device_holds(api, oracle_lib):
    """The SPLIT grid is at most 8 192 workgroups, so with more long reads than that its workgroups take a second read
    (item += gridDim.x), re-use their LDS and find their log slot anew.  11 264 device-made reads of 900 - 1 500 bases with
    split_bucket = 64 (long from 1 024 bases): over 8 192 long reads and some thousand short ones per batch, against the 100-bin W = 2
    row-log index, two sets alternately, three in flight.  Every read of every batch equals the oracle (index rows pulled back from the
    device); no batch is re-run."""
    from charon_amd import pack
    B, S, n, lo, hi, glen = 100, 1 << 20, 11264, 900, 1500, 1 << 16
    b2c = [b % 2 for b in range(B)]
    g = api.Index(api.make_desc(B, S, b2c, 2, 0))
    assert g.desc.bin_words == 2
    gen = api.synth_genomes(0, 43, B, glen)
    g.synth_fill(43, 0.1)
    g.synth_plant(gen, B, glen, list(range(B)))
    sets = [api.synth_reads(0, 44, gen, B, glen, n, lo, hi, 0.05, 0.1, 40.0, first_read_id=j * n) for j in range(2)]
    oidx = None
    try:
        st = api.Stream(g, n, max(int(rd.n_bases) for rd in sets), split_bucket=64)
        st.set_model(api.default_model(2, 0))
        outs = []
        for i in range(4 + 2):
            if i < 4:
                rd = sets[i % 2]
                st.submit_device(n, rd.n_bases, rd.bases2, rd.seg1_offset, rd.seg1_length, rd.mean_quality, rd.compression)
            if i >= 2:
                outs.append(util.download_results(api, st.wait_device(), n, 2))
        reruns = st.profile(4)[1]
        st.destroy()
        oidx = oracle_lib.Index.new(B, S, b2c, ["human", "microbial"])
        oidx.words()[:] = g.download()
        for j, rd in enumerate(sets):
            lens = api.device_download(0, rd.seg1_length, n * 4, np.uint32)
            offs = api.device_download(0, rd.seg1_offset, n * 8, np.uint64)
            n_long = int((lens >= 1024).sum())
            print("set %d: %d long reads, %d short" % (j, n_long, n - n_long))
            assert n_long > 8192 and n - n_long >= 64
            nb = int(offs[-1]) + (int(lens[-1]) + 63) // 64 * 64
            reads = pack.unpack_reads(api.device_download(0, rd.bases2, nb // 4, np.uint32), offs, lens)
            cat, o, _ = util.concat(reads)
            orc = oidx.process_reads(cat, o, threads=8)
            for out in outs[j::2]:
                assert_oracle(out, orc, False)
        assert not np.array_equal(outs[0]["num_hashes"], outs[1]["num_hashes"])
        assert reruns == 0
    finally:
        if oidx is not None:
            oidx.free()
        for rd in sets:
            util.free_synth_reads(api, rd)
        api.device_free(0, gen)
        g.destroy()
