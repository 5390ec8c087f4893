"""GPU tests (-m gpu) of what a submit leaves behind when it is refused between two of its stages (abi_stream_batch.inc: check, stage the
inputs, pick the probe stream, the gzip column, order the reads, fill the probe kernel's arguments, launch, hand over to the tail), and of
creating and destroying a stream under every flag that owns streams or events of its own.

A refusal must leave the stream as the next submit expects it: the slot not in flight, the head where it was, the profiling state
unspoilt, whatever was already queued for the refused batch harmless.  Yardsticks, none of which is the code under test: the CPU oracle
(util.assert_parity), the same batch alone on a fresh stream (util.assert_same_results, bit for bit in all seven columns) and zlib for
the gzip sizes.  Two indices: the toy 2-bin, 2-category index (MODE_FUSED) and the 70-bin W = 2 row-log index of
tests/test_gpu_device_batches.py (MODE_ROWS: the count kernel and the row log take part); 130 reads of 150 bases -- two full wavefronts
and a partial one.

Not here: "window too large for LDS".  chn_index_desc.window_size is eight bits wide, and no (k, window <= 255, h, W) gives the probe
kernel more LDS than a CU has (tools/stream_batch_check.hip walks them all: the most is 156 352 bytes), so no index that
chn_index_create accepts can reach that refusal."""
import numpy as np
import pytest

from tests import util
from tests import test_gpu_device_batches as dbt
from tests import test_gpu_probe_overlap as pot

pytestmark = pytest.mark.gpu

COLUMNS = dbt.COLUMNS
N, L = 130, 150
INDICES = ("toy", "rows")


@pytest.fixture(scope="module")
def api():
    import charon_amd.api as api
    return api


@pytest.fixture(scope="module")
def world(api, oracle_lib):
    """per index: the oracle index, its device twin, four distinct read sets (packed, and as device batches) and the oracle's results"""
    from charon_amd import pack
    r = util.rng(1806)
    toy_gs = [util.random_seq(r, 10000), util.random_seq(r, 10000)]
    toy = util.build_oracle_index(oracle_lib, [[g] for g in toy_gs], [0, 1], ["microbial", "host"])
    gs = dbt.make_genomes()
    fused, rows = dbt.build_indices(oracle_lib, gs)
    fused.free()
    w = {}
    for name, oidx, genomes in (("toy", toy, toy_gs), ("rows", rows, gs)):
        sets = []
        for _ in range(4):
            reads = util.sample_reads(r, genomes, N, L)
            p = pack.pack_reads(reads)
            sets.append(dict(reads=reads, packed=p, dev=util.to_device_batch(api, p, mq=40.0, comp=0.0), orc=dbt.oracle_run(oidx, reads),
                             zlib=np.array([dbt.zsize(s) for s in reads], np.uint32)))
        w[name] = dict(oidx=oidx, g=util.gpu_index_from_oracle(api, oidx), sets=sets, max_bases=max(s["packed"]["n_bases"] for s in sets))
    assert w["toy"]["g"].desc.bin_words == 1 and w["rows"]["g"].desc.bin_words == 2
    yield w
    for x in w.values():
        for s in x["sets"]:
            s["dev"].free()
        x["g"].destroy()
        x["oidx"].free()


def new_stream(api, x, **kw):
    st = api.Stream(x["g"], N, x["max_bases"], **kw)
    st.set_model(dbt.model_for(api, x["g"], False))
    return st


def submit_host(st, s, **kw):
    st.submit_host(s["packed"], np.full(N, 40.0, np.float32), None if kw.get("gzip_tallies") else np.zeros(N, np.float32), **kw)


def alone(api, x, s, **kw):
    """the set as a host batch, one in flight, on a fresh stream"""
    st = new_stream(api, x)
    try:
        submit_host(st, s, **kw)
        return st.wait_host()
    finally:
        st.destroy()


@pytest.mark.parametrize("index", INDICES)
def test_refused_gzip_column_leaves_the_slot_and_the_profile_clean(api, world, index):
    """gzip_output = 7 is refused in the gzip column, after the batch's uploads were queued on the copy stream and the chain's bracket
    was opened on the probe stream.  The same reads submitted validly then equal the oracle, the run on a fresh stream and zlib, and
    the profiling stream has counted one probe launch and one chain"""
    x = world[index]
    s = x["sets"][0]
    st = new_stream(api, x, profile=True)
    try:
        with pytest.raises(api.ChnError, match="unknown value"):
            submit_host(st, s, gzip_tallies=L, gzip_output=7)
        submit_host(st, s, gzip_tallies=L, gzip_output=api.GZIP_SIZES)
        out = st.wait_host()
        probe, chain = st.profile(0), st.profile(3)
    finally:
        st.destroy()
    fresh = alone(api, x, s, gzip_tallies=L, gzip_output=api.GZIP_SIZES)
    util.assert_parity(out, s["orc"])
    util.assert_same_results(out, fresh, keys=COLUMNS)
    assert np.array_equal(out["gzip_sizes"], fresh["gzip_sizes"]) and np.array_equal(out["gzip_sizes"], s["zlib"])
    assert probe[1] == 1 and chain[1] == 1 and 0 < probe[0] <= chain[0]


@pytest.mark.parametrize("index", INDICES)
def test_full_stream_refuses_the_fourth_and_takes_the_next(api, world, index):
    """three batches in flight: a fourth submit is refused before anything is queued; the three come back in order, each equal to its
    run alone; the next submit is accepted and equals its own"""
    x = world[index]
    sets = x["sets"]
    runs = [alone(api, x, s) for s in sets]
    st = new_stream(api, x)
    try:
        for s in sets[:3]:
            submit_host(st, s)
        with pytest.raises(api.ChnError, match="three batches already in flight"):
            submit_host(st, sets[3])
        got = [st.wait_host() for _ in range(3)]
        submit_host(st, sets[3])
        got.append(st.wait_host())
    finally:
        st.destroy()
    for out, run, s in zip(got, runs, sets):
        util.assert_same_results(out, run, keys=COLUMNS)
        util.assert_parity(out, s["orc"])
    assert not np.array_equal(got[0]["num_hashes"], got[1]["num_hashes"]) and not np.array_equal(got[1]["num_hashes"], got[2]["num_hashes"])


@pytest.mark.parametrize("index", INDICES)
def test_refused_device_gzip_sizes_then_a_valid_device_batch_on_the_same_slot(api, world, index):
    """CHN_GZIP_SIZES_ALL is for host batches: a device batch that asks for it is refused in the gzip column.  The slot is not taken:
    the same device batch with CHN_GZIP_SIZES follows on it and equals the oracle and zlib"""
    x = world[index]
    s = x["sets"][1]
    st = new_stream(api, x)
    try:
        with pytest.raises(api.ChnError, match="host batches only"):
            s["dev"].submit(st, gzip_tallies=L, gzip_output=api.GZIP_SIZES_ALL)
        s["dev"].submit(st, gzip_tallies=L, gzip_output=api.GZIP_SIZES)
        out = dbt.wait_downloaded(api, st, N, gzip_output=api.GZIP_SIZES)
        with pytest.raises(api.ChnError, match="no batch in flight"):
            st.wait_device()
    finally:
        st.destroy()
    pot.assert_oracle(out, s["orc"], False)
    assert np.array_equal(out["gzip_sizes"], s["zlib"])


@pytest.mark.parametrize("index", INDICES)
@pytest.mark.parametrize("flags", [dict(), dict(profile=True), dict(probe_gate=False), dict(tiny_log=True)], ids=["none", "profile", "no_probe_gate", "tiny_log"])
def test_create_and_destroy_under_every_flag(api, world, index, flags):
    """chn_stream_create / chn_stream_destroy once per flag that owns streams or events of its own (the walked stream list, the slots'
    event brackets, the profiling anchor, the gate's signal word, the tiny row log and its re-run), one batch through each, with a
    chn_stream_sync while it is in flight"""
    x = world[index]
    s = x["sets"][2]
    st = new_stream(api, x, **flags)
    try:
        submit_host(st, s)
        st.sync()
        out = st.wait_host()
        reruns = st.profile(4)[1]
        counted = st.profile(3)[1]
    finally:
        st.destroy()
    util.assert_parity(out, s["orc"])
    print("re-runs after a row-log overflow: %d" % reruns)
    assert counted == (1 if flags.get("profile") else 0)
    if not flags.get("tiny_log"):
        assert reruns == 0
