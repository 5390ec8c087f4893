"""GPU tests (-m gpu) of the probe gate: a batch's minimise+probe launch waits in its queue until the batch before it has dispatched its
last workgroup (every workgroup counts itself in; the last arrival raises the stream's signal word to the batch's sequence number, and a
one-thread kernel behind the grid raises it again), then fills that grid's thinning last generation.

Yardsticks, none of which is the code under test: the CPU oracle (util.assert_parity) and the same batch run ALONE -- one in flight, on a
fresh stream -- compared in all seven result columns, bit for bit (util.assert_same_results).  No test looks at a clock: what can go
wrong here is a successor released too early (it would still compute the same: the gate orders nothing the results depend on), never
released (a hang), or released by the wrong stream's signal; and the paths that launch no gated grid must leave no successor waiting for a
value nobody writes.  chn_stream_profile(13) counts the launches queued behind a gate wait; its total_ms says whether the stream gates at
all (a device without stream-wait-value support runs the ungated schedule, and the lower bounds on the count are skipped there).  (Slot
13 and not 12: tests/test_gpu_text_pair.py pins that 12 is refused.)
Index and read-set builders are those of tests/test_gpu_device_batches.py and tests/test_gpu_probe_overlap.py."""
import numpy as np
import pytest

from tests import util
from tests import test_gpu_device_batches as dbt
from tests import test_gpu_probe_overlap as pot
from tests.test_gpu_probe_overlap import api, world  # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu

COLUMNS = dbt.COLUMNS
GATED = 13  # chn_stream_profile slot
NO_WAIT_VALUE = "the device reports no stream-wait-value support: the stream runs the ungated schedule"


def gates(st):
    return st.profile(GATED)[0] == 1.0


# ---- the 100-bin W = 2 row-log index of the coexistence test, device-made reads, the oracle on rows pulled back from the device ------
@pytest.fixture(scope="module")
def synth(api, oracle_lib):
    B, S, glen = 100, 1 << 20, 1 << 16
    b2c = [b % 2 for b in range(B)]
    g = api.Index(api.make_desc(B, S, b2c, 2, 0))
    assert g.desc.bin_words == 2
    gen = api.synth_genomes(0, 43, B, glen)
    g.synth_fill(43, 0.1)
    g.synth_plant(gen, B, glen, list(range(B)))
    oidx = oracle_lib.Index.new(B, S, b2c, ["human", "microbial"])
    oidx.words()[:] = g.download()
    yield dict(B=B, glen=glen, g=g, gen=gen, oidx=oidx)
    oidx.free()
    api.device_free(0, gen)
    g.destroy()


def oracle_head(api, synth, rd, head):
    """the oracle's results for the first `head` reads of a device-made set"""
    from charon_amd import pack
    lens = api.device_download(0, rd.seg1_length, head * 4, np.uint32)
    offs = api.device_download(0, rd.seg1_offset, head * 8, np.uint64)
    nb = int(offs[-1]) + (int(lens[-1]) + 63) // 64 * 64
    reads = pack.unpack_reads(api.device_download(0, rd.bases2, nb // 4, np.uint32), offs, lens)
    cat, o, _ = util.concat(reads)
    return synth["oidx"].process_reads(cat, o, threads=8)


def assert_device_rows(got, orc):
    """device results are not re-evaluated on the host: every integer column, and parity where no near-tie flag is set
    (tests/test_gpu_device_batches.py); -> rows flagged"""
    for key in ("num_hashes", "counts", "unique", "conf"):
        assert np.array_equal(got[key], orc[key]), key
    keep = got["flags"] == 0
    util.assert_parity(dbt.rows_of(got, keep), dbt.rows_of(orc, keep))
    return int((~keep).sum())


def sub_synth(st, rd, n):
    st.submit_device(n, rd.n_bases, rd.bases2, rd.seg1_offset, rd.seg1_length, rd.mean_quality, rd.compression)


def run_synth(api, st, sets, sizes, order, depth=3):
    """the sets in `order`, `depth` in flight -> their downloaded results in order"""
    outs, k = [], 0
    while k < min(depth - 1, len(order)):
        sub_synth(st, sets[order[k]], sizes[order[k]])
        k += 1
    for i in range(len(order)):
        if k < len(order):
            sub_synth(st, sets[order[k]], sizes[order[k]])
            k += 1
        outs.append(util.download_results(api, st.wait_device(), sizes[order[i]], 2))
    return outs


# ---- 1. grids of one and two workgroups -------------------------------------------------------------------------------------------
def test_grids_of_one_and_two_workgroups(api, synth):
    """batches of 1, 63, 64, 65 and 128 reads of 200 - 400 bases are grids of one and two workgroups: the first arrival is also the
    last, so "the last arrival publishes" goes wrong here first.  Ten batches, three in flight, sizes cycling: every read of every batch
    equals the oracle, and at least 7 of the launches were queued behind a gate wait"""
    sizes = (1, 63, 64, 65, 128)
    sets = [api.synth_reads(0, 45, synth["gen"], synth["B"], synth["glen"], n, 200, 400, 0.05, 0.1, 40.0, first_read_id=1000 * j) for j, n in enumerate(sizes)]
    try:
        orcs = [oracle_head(api, synth, rd, n) for rd, n in zip(sets, sizes)]
        st = api.Stream(synth["g"], 128, max(int(rd.n_bases) for rd in sets))
        st.set_model(api.default_model(2, 0))
        try:
            order = [i % 5 for i in range(10)]
            outs = run_synth(api, st, sets, sizes, order)
            gating, gated = gates(st), st.profile(GATED)[1]
            assert st.profile(4)[1] == 0
        finally:
            st.destroy()
        flagged = sum(assert_device_rows(out, orcs[j]) for j, out in zip(order, outs))
        assert flagged <= 0.05 * 2 * sum(sizes)
        assert not np.array_equal(outs[1]["num_hashes"], outs[2]["num_hashes"][:63])
        if not gating:
            pytest.skip(NO_WAIT_VALUE)
        assert gated >= 7
    finally:
        for rd in sets:
            util.free_synth_reads(api, rd)


# ---- 2. more workgroups than the device holds -------------------------------------------------------------------------------------
def test_more_workgroups_than_the_device_holds_gated_and_ungated(api, synth):
    """262 144 device-made 1 kb reads are 4 096 wavefronts and the device holds 1 792: the last workgroup is dispatched when most of the
    grid has already retired, and the successor moves in then.  Six batches, three in flight, on a gated stream and on a
    probe_gate=False stream: both bit-identical to the run alone, the first 4 096 reads of each set equal the oracle; at least 4
    gated launches on the one, none on the other"""
    n, L, head = 1 << 18, 1000, 4096
    sets = [api.synth_reads(0, 42, synth["gen"], synth["B"], synth["glen"], n, L, L, 0.05, 0.1, 40.0, first_read_id=j * n) for j in range(3)]
    sizes = (n, n, n)
    max_bases = max(int(rd.n_bases) for rd in sets)

    def new_stream(**kw):
        st = api.Stream(synth["g"], n, max_bases, **kw)
        st.set_model(api.default_model(2, 0))
        return st
    try:
        st = new_stream()
        try:
            alone = run_synth(api, st, sets, sizes, [0, 1, 2], depth=1)
        finally:
            st.destroy()
        order = [i % 3 for i in range(6)]
        runs = {}
        for gate in (True, False):
            st = new_stream(probe_gate=gate)
            try:
                outs = run_synth(api, st, sets, sizes, order)
                runs[gate] = (outs, gates(st), st.profile(GATED)[1], st.profile(4)[1])
            finally:
                st.destroy()
        for gate in (True, False):
            for j, out in zip(order, runs[gate][0]):
                util.assert_same_results(out, alone[j], keys=COLUMNS)
            assert runs[gate][3] == 0
        assert not np.array_equal(alone[0]["num_hashes"], alone[1]["num_hashes"])
        for j, rd in enumerate(sets):
            orc = oracle_head(api, synth, rd, head)
            assert assert_device_rows(dbt.rows_of(alone[j], slice(0, head)), orc) <= 0.05 * head
            assert (orc["call"] == 0).sum() > head // 8 and (orc["call"] == 1).sum() > head // 8
        assert runs[False][1] is False and runs[False][2] == 0
        if not runs[True][1]:
            pytest.skip(NO_WAIT_VALUE)
        assert runs[True][2] >= 4
    finally:
        for rd in sets:
            util.free_synth_reads(api, rd)


# ---- 3. forty small batches -------------------------------------------------------------------------------------------------------
def test_forty_small_batches(api, world):
    """the 333-read sets, host and device form alternately, three in flight: the sequence number runs well past any slot arithmetic"""
    names = pot.SETS["rows"]
    plan = [(names[i % 3], i % 2 == 0) for i in range(40)]
    st, packed = pot.make_stream(api, world, "rows", False, names)
    try:
        outs = pot.pipelined(api, st, packed, plan)
        gating, gated = gates(st), st.profile(GATED)[1]
        assert st.profile(4)[1] == 0
    finally:
        pot.free_all(st, packed)
    assert len(outs) == 40
    for (name, host), out in zip(plan, outs):
        util.assert_parity(out, dbt.oracle_of(world, "rows", name))
    if gating:
        assert gated == 39  # every launch but the first: nothing here has long reads


# ---- 4. hand-overs: the paths that publish nothing or run ungated -----------------------------------------------------------------
def test_hand_over_to_the_list_mode_calls(api, world, oracle_lib):
    """three batches, then chn_minimisers and the dense one-rank chain (first probe stream, no gate, no sequence number), then three
    batches: the first of them waits for the last value actually written"""
    names = ("se", "se_n", "se_rev")
    plan = [(names[i % 3], i % 2 == 1) for i in range(3)]
    gidx = world["gr"]
    st, packed = pot.make_stream(api, world, "rows", False, names)
    orc = dbt.oracle_of(world, "rows", "se")
    orc_rev = {k: v[::-1] for k, v in orc.items() if isinstance(v, np.ndarray)}
    partial = None
    try:
        before = pot.pipelined(api, st, packed, plan)
        gated_before = st.profile(GATED)[1]
        p, db = packed["se"]
        mins = st.minimisers_host(p)
        want = np.concatenate([np.asarray(oracle_lib.minimisers(s.decode()), np.uint64) for s in world["sets"]["se"][0] if len(s)] or [np.zeros(0, np.uint64)])
        e = st.shard_minimise_device(333, p["n_bases"], db.bases2, db.seg1_offset, db.seg1_length, db.mean_quality, db.compression)
        nwords = e * gidx.desc.hash_funs * gidx.desc.bin_words
        partial = api.device_malloc(0, max(nwords, 2) * 8)
        st.shard_probe(gidx, partial, nwords)
        st.shard_finish(partial)
        chain = dbt.wait_downloaded(api, st, 333)
        assert st.profile(GATED)[1] == gated_before  # the list-mode calls are not gated
        after = pot.pipelined(api, st, packed, plan)
        gating, gated = gates(st), st.profile(GATED)[1]
    finally:
        pot.free_all(st, packed)
        if partial:
            api.device_free(0, partial)
    assert e == int(orc["num_hashes"].sum()) and np.array_equal(np.sort(mins), np.sort(want))
    util.assert_parity(chain, orc)
    for outs in (before, after):
        for (name, host), out in zip(plan, outs):
            util.assert_parity(out, orc_rev if name == "se_rev" else dbt.oracle_of(world, "rows", name))
    for a, b in zip(before, after):
        util.assert_same_results(a, b, keys=COLUMNS)
    if gating:
        assert (gated_before, gated) == (2, 5)


def test_hand_over_to_the_overflow_rerun(api, world):
    """tiny_log=True: every batch is run again, synchronously and ungated, on a slot whose counter has counted already, while the two
    batches behind it are on the device or waiting at their gates"""
    names = ("se", "se_n", "se_rev")
    plan = [(names[i % 3], i % 2 == 0) for i in range(6)]
    st, packed = pot.make_stream(api, world, "rows", False, names, tiny_log=True)
    try:
        outs = pot.pipelined(api, st, packed, plan)
        reruns, gating, gated = st.profile(4)[1], gates(st), st.profile(GATED)[1]
    finally:
        pot.free_all(st, packed)
    orc_rev = {k: v[::-1] for k, v in dbt.oracle_of(world, "rows", "se").items() if isinstance(v, np.ndarray)}
    for (name, host), out in zip(plan, outs):
        util.assert_parity(out, orc_rev if name == "se_rev" else dbt.oracle_of(world, "rows", name))
    assert reruns == 6
    if gating:
        assert gated == 5


def test_hand_over_to_the_long_read_schedule(api, world):
    """split_bucket=64: the batches submitted before one with long reads has been waited for alternate behind their gates (the SPLIT
    launch itself is never gated); from then on every batch takes the first probe stream, ungated"""
    names = ("se", "se_n", "se_rev")
    plan = [(names[i % 3], i % 2 == 0) for i in range(6)]
    st, packed = pot.make_stream(api, world, "rows", False, names, split_bucket=64)
    try:
        outs = pot.pipelined(api, st, packed, plan)
        reruns, gating, gated = st.profile(4)[1], gates(st), st.profile(GATED)[1]
    finally:
        pot.free_all(st, packed)
    for (name, host), out in zip(plan, outs):
        key = ("rows", name)
        if key not in world["memo"]:
            world["memo"][key] = dbt.oracle_run(world["rows"], *world["sets"][name])
        pot.assert_oracle(out, world["memo"][key], host)
    assert reruns == 0
    if gating:
        assert gated == 2  # batches 1 and 2: three are submitted before the first wait


# ---- 5. two streams on one index --------------------------------------------------------------------------------------------------
def test_two_streams_on_one_index_do_not_release_each_other(api, world):
    """two chn_streams driven alternately from one thread, three in flight each, different sets at the same moment: each has its own
    signal word and sequence.  Results equal the run alone and the oracle"""
    names = pot.SETS["rows"]
    plans = ([(names[i % 3], i % 2 == 0) for i in range(6)], [(names[(i + 1) % 3], i % 2 == 1) for i in range(6)])
    st, packed = pot.make_stream(api, world, "rows", False, names)
    try:
        alone = {}
        for name in names:
            for host in (True, False):
                pot.submit(st, packed, name, host)
                alone[(name, host)] = pot.wait(api, st, host)
    finally:
        st.destroy()
    gidx, max_bases = world["gr"], max(p["n_bases"] for p, _ in packed.values())
    sts = []
    try:
        for _ in range(2):
            sts.append(api.Stream(gidx, 333, max_bases))
            sts[-1].set_model(dbt.model_for(api, gidx, False))
        outs = ([], [])
        for k in range(2):
            for s in range(2):
                pot.submit(sts[s], packed, *plans[s][k])
        for i in range(6):
            if i + 2 < 6:
                for s in range(2):
                    pot.submit(sts[s], packed, *plans[s][i + 2])
            for s in range(2):
                outs[s].append(pot.wait(api, sts[s], plans[s][i][1]))
        gating, gated = gates(sts[0]), [s.profile(GATED)[1] for s in sts]
    finally:
        for s in sts:
            s.destroy()
        for _, db in packed.values():
            db.free()
    for s in range(2):
        for (name, host), out in zip(plans[s], outs[s]):
            util.assert_same_results(out, alone[(name, host)], keys=COLUMNS)
            util.assert_parity(out, dbt.oracle_of(world, "rows", name))
    if gating:
        assert gated == [5, 5]
