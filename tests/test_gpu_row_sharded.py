"""The two row-sharded chains on the GPU: chn_shard_* (dense: k_probe_partial, k_and_partial) and chn_shardx_*
(sparse: k_shx_count / _scan / _scatter / _serve / _and), on the cases of tests/sharded_cases.py -- W = 3 and 4, escaped rows within
and beyond a wavefront's region, 1 to 16 owners with empty ones, paired reads, N, other (k, w) and h, a read one lane rolls alone, and
the calls' state machine.  Every comparison is bit-exact against the oracle, the model built from it, and the whole-index path;
the probability column within util.assert_parity's 1e-6.  tests/test_sharded_cases_cpu.py shows that each case reaches its branch."""
import functools
import subprocess
import sys

import numpy as np
import pytest

from tests import sharded_cases as sc
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import charon_amd.api as api
    return api


_replica = {}


def replica(api, name):
    """the whole-index path's results of a case, computed once"""
    if name not in _replica:
        c = sc.case(name)
        _replica[name] = sc.run_replica(api, c.oidx, c.reads, c.mates)
    return _replica[name]


def concat_outs(outs):
    return {k: np.concatenate([o[k] for o in outs]) for k in ("num_hashes", "counts", "unique", "call", "conf", "probs")}


def both_chains(api, name, cuts, splits, rank_sizes):
    """a case through the dense chain (shards at `cuts`) and the sparse chain (owners at `splits`, ranks of `rank_sizes` reads): results
    against the oracle and the whole-index path, what is exchanged against the model"""
    c = sc.case(name)
    orc, rep = c.oracle(), replica(api, name)
    util.assert_parity(rep, orc)
    d = sc.run_dense(api, c.oidx, c.reads, c.mates, cuts)
    for out in d["outs"]:
        util.assert_parity(out, orc)
        util.assert_same_results(out, rep)
    sc.check_dense_exchange(c.model(), c.oidx, d)
    rr, rm = sc.split_ranks(c.reads, rank_sizes, c.mates)
    got = sc.run_sparse(api, c.oidx, rr, rm, splits)
    whole = concat_outs([g["out"] for g in got])
    util.assert_parity(whole, orc)
    util.assert_same_results(whole, rep)
    sc.check_sparse_exchange(c.po, c.oidx, rr, rm, splits, got)
    return c, d, got


def halves(c):
    n = len(c.reads)
    return [n // 2, n - n // 2]


def refused(api, code, fn, *args, match=None):
    with pytest.raises(api.ChnError, match=match) as e:
        fn(*args)
    assert e.value.code == code, (e.value.code, str(e.value))


@functools.lru_cache(None)
def cu_count():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked in a child process: torch brings a HIP runtime of its own, and the
    library's calls in this process fail once that one has opened the device"""
    code = "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"
    return int(subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True, timeout=120).stdout.split()[-1])


# ---- 1. k_shx_serve alone -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_serve_kernel_alone(api, W):
    """out[j] = row queries[j] of the shard, for one query up to one more than a full pass of the grid (2 x CUs workgroups x 256 threads x 4
    queries: the grid-stride loop's second pass), with the first and the last row and repeated rows among the queries; the 64 words in
    front of and behind the output stay as they were.  W = 4 takes the two 16-byte loads and stores, W = 3 the word-by-word path."""
    cus = cu_count()
    r = util.rng(900 + W)
    rows = 50021
    words = r.integers(0, 1 << 63, rows * W, dtype=np.uint64) * np.uint64(2) + r.integers(0, 2, rows * W, dtype=np.uint64)
    bins = 64 * W - 3
    sh = api.Index(api.make_desc(bins, rows, [i % 2 for i in range(bins)], 2, 0))
    sh.upload(words)
    st = api.Stream(sh, 1, 64)
    table = words.reshape(-1, W)
    G = 64
    try:
        for n in (1, 255, 256, 257, 2 * cus * 256 * 4 + 3):
            q = r.integers(0, rows, n, dtype=np.uint32)
            q[0] = 0
            if n > 1:
                q[-1] = rows - 1
                q[n // 2:n // 2 + 40] = q[1]  # repeats (one wavefront's worth of the same row)
            guard = r.integers(1, 1 << 62, 2 * G + n * W, dtype=np.uint64)
            d_q, d_o = util.to_device(api, q), util.to_device(api, guard)
            st.shardx_serve(sh, d_q, n, d_o + G * 8)
            st.sync()
            got = api.device_download(0, d_o, guard.nbytes, np.uint64)
            api.device_free(0, d_q)
            api.device_free(0, d_o)
            assert np.array_equal(got[:G], guard[:G]) and np.array_equal(got[-G:], guard[-G:]), n
            assert np.array_equal(got[G:-G].reshape(-1, W), table[q]), n
    finally:
        st.destroy()
        sh.destroy()


# ---- 2. + 3. both chains on wide rows and on rows that escape ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w3", "w4", "esc1"])
def test_wide_and_escaped_rows_through_both_chains(api, oracle_lib, name):
    """W = 3 (130 bins) and W = 4 (200 bins), both with a partial last word; W = 1 and W = 3 with 2 - 8 % of the ANDed rows holding more
    than three set bins (within every wavefront's escaped-row region).  Dense: four shards, one of 17 rows; sparse: three owners (one of
    17 rows), two ranks."""
    S = sc.case(name).oidx.bin_size
    c, d, got = both_chains(api, name, [0, S // 3, S // 3 + 17, 2 * S // 3, S], [0, 17, S // 3, S], halves(sc.case(name)))
    assert len(d["outs"]) == 4
    if name != "w4":
        assert c.model()["n_escaped"] >= 500
        assert c.oracle()["unique"].sum() > 0


def test_dense_chain_holds_a_batch_whose_rows_nearly_all_escape(api, oracle_lib):
    """the dense chain lays its regions out for the worst case (every row escaped): the batch that overruns the sparse chain's regions
    succeeds here"""
    c = sc.case("over")
    S = c.oidx.bin_size
    d = sc.run_dense(api, c.oidx, c.reads, None, [0, S // 2, S])
    for out in d["outs"]:
        util.assert_parity(out, c.oracle())
        util.assert_same_results(out, replica(api, "over"))
    sc.check_dense_exchange(c.model(), c.oidx, d)
    assert c.model()["n_escaped"] > len(c.model()["values"]) // 2


def one_rank(api, oidx, st, shards, splits, reads, mates=None):
    """one batch of one rank through the sparse chain on stream `st` -> (results, rank dict)"""
    rk = sc.sparse_batch(api, oidx, shards, splits, [dict(st=st, reads=reads, mates=mates)])[0]
    return st.wait_host(), rk


# ---- 4. escaped rows beyond a region's capacity: an error, and the stream goes on ------------------------------------------------------
def test_sparse_escape_overflow_is_reported_and_the_stream_recovers(api, oracle_lib):
    from charon_amd import pack
    over, fits = sc.case("over"), sc.case("esc1")
    oidx, S = over.oidx, over.oidx.bin_size
    splits = [0, S // 2, S]
    shards = sc.make_shards(api, oidx, splits)
    nb = max(pack.pack_reads(c.reads)["n_bases"] for c in (over, fits))
    st = sc.open_stream(api, shards[0], oidx, max(len(over.reads), len(fits.reads)), nb)
    try:
        sc.sparse_batch(api, oidx, shards, splits, [dict(st=st, reads=over.reads)])
        refused(api, api.E_CAPACITY, st.wait_host, match="row log overflow in the row-sharded chain")
        for _ in range(2):  # (the second run takes the slot the failed batch had, or the one after it)
            out, rk = one_rank(api, oidx, st, shards, splits, fits.reads)
            util.assert_parity(out, fits.oracle())
            util.assert_same_results(out, replica(api, "esc1"))
            assert rk["counts"] == fits.model(splits)["counts"]
    finally:
        st.destroy()
        for sh in shards:
            sh.destroy()


# ---- 5. owner counts -----------------------------------------------------------------------------------------------------------------
def test_one_owner_and_sixteen_owners_with_empty_ones(api, oracle_lib):
    """the sparse chain with a single owner and with 16 (the maximum), four of them without rows -- the first, the last and two adjacent
    ones -- one of a single row and one of 17 rows, a split on a probed row; four ranks of 1, 63, 64 and 200 reads"""
    c = sc.case("w2")
    S = c.oidx.bin_size
    rr, _ = sc.split_ranks(c.reads, [1, 63, 64, 200])
    sp16 = sc.owner_splits16(S, c.model()["rows"])
    for splits in ([0, S], sp16):
        got = sc.run_sparse(api, c.oidx, rr, None, splits)  # (an owner without rows has no shard object: make_shards)
        whole = concat_outs([g["out"] for g in got])
        util.assert_parity(whole, c.oracle())
        util.assert_same_results(whole, replica(api, "w2"))
        sc.check_sparse_exchange(c.po, c.oidx, rr, None, splits, got)
        for g in got:
            assert all(g["counts"][o] == 0 for o in range(len(splits) - 1) if splits[o] == splits[o + 1])
    assert sum(g["counts"][3] for g in got) >= 1 and sum(g["counts"][4] for g in got) >= 1  # the owners of 1 and of 17 rows


def test_bad_row_splits_are_refused_and_the_stream_stays_usable(api, oracle_lib):
    from charon_amd import pack
    c = sc.case("w2_few")
    S = c.oidx.bin_size
    shards = sc.make_shards(api, c.oidx, [0, S])
    p = pack.pack_reads(c.reads)
    st = sc.open_stream(api, shards[0], c.oidx, len(c.reads), p["n_bases"])
    try:
        st.shardx_minimise_host(p, *sc.columns(len(c.reads)))
        seventeen = [0] + [S * i // 17 for i in range(1, 17)] + [S]
        assert len(seventeen) == 18
        refused(api, api.E_INVALID, st.shardx_counts, seventeen, match="1..16 ranks")
        refused(api, api.E_INVALID, st.shardx_counts, [0, S // 2, S // 3, S], match="ascend")
        refused(api, api.E_INVALID, st.shardx_counts, [0, S // 2, S - 1], match="cover")
        refused(api, api.E_INVALID, st.shardx_counts, [1, S // 2, S], match="cover")
        # the batch is still open at the stage it was: the chain goes on from chn_shardx_counts
        n_probes, counts = st.shardx_counts([0, S])
        assert [n_probes] == counts == c.model()["counts"]
        dq = api.device_malloc(0, n_probes * 4)
        st.shardx_queries(dq, n_probes)
        d_rows = api.device_malloc(0, n_probes * c.oidx.bin_words * 8)
        st.shardx_serve(shards[0], dq, n_probes, d_rows)
        st.shardx_finish(d_rows)
        util.assert_parity(st.wait_host(), c.oracle())
        api.device_free(0, dq)
        api.device_free(0, d_rows)
    finally:
        st.destroy()
        shards[0].destroy()


# ---- 6. what MODE_LIST of the probe kernel is given -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["paired12", "nruns", "kw_15_15", "kw_27_31", "kw_5_200", "h1", "h5", "long"])
def test_list_mode_inputs_through_both_chains(api, oracle_lib, name):
    """paired reads on a 12-category index, runs of N, other (k, w), one and five hash functions, a read of 40 000 bases (never split in
    the list modes: one lane rolls it, and the count kernel runs with 32-bit totals): oracle parity through both chains, and
    chn_minimisers against the oracle's minimisers as a multiset (check_dense_exchange)"""
    c = sc.case(name)
    S = c.oidx.bin_size
    both_chains(api, name, [0, S // 3, S], [0, S // 3, S], halves(c))


# ---- 7. the calls' state machine ---------------------------------------------------------------------------------------------------------
def test_calls_out_of_order_are_state_errors(api, oracle_lib):
    from charon_amd import pack
    c = sc.case("w2_few")
    S, W = c.oidx.bin_size, c.oidx.bin_words
    splits = [0, S // 2, S]
    shards = sc.make_shards(api, c.oidx, splits)
    p = pack.pack_reads(c.reads)
    n = len(c.reads)
    st = sc.open_stream(api, shards[0], c.oidx, n, p["n_bases"])
    buf = api.device_malloc(0, 1 << 20)
    try:
        # nothing open
        refused(api, api.E_STATE, st.shardx_counts, splits)
        refused(api, api.E_STATE, st.shardx_queries, buf, 1 << 18)
        refused(api, api.E_STATE, st.shardx_finish, buf)
        refused(api, api.E_STATE, st.shard_probe, shards[0], buf, 1 << 17)
        refused(api, api.E_STATE, st.shard_finish, buf)
        st._fifo.append((n, None))
        refused(api, api.E_STATE, st.wait_host, match="no batch in flight")
        st._fifo.clear()
        # sparse batch open, stage 1: only chn_shardx_counts may follow
        st.shardx_minimise_host(p, *sc.columns(n))
        refused(api, api.E_STATE, st.shardx_minimise_host, p)
        refused(api, api.E_STATE, st.shard_minimise_host, p)
        refused(api, api.E_STATE, st.minimisers_host, p)
        refused(api, api.E_STATE, st.shardx_queries, buf, 1 << 18)
        refused(api, api.E_STATE, st.shardx_finish, buf)
        n_probes, counts = st.shardx_counts(splits)
        # stage 2: only chn_shardx_queries
        refused(api, api.E_STATE, st.shardx_counts, splits)
        refused(api, api.E_STATE, st.shardx_finish, buf)
        refused(api, api.E_STATE, st.shardx_minimise_host, p)
        refused(api, api.E_CAPACITY, st.shardx_queries, buf, n_probes - 1, match="query buffer too small")
        st.shardx_queries(buf, n_probes)
        # stage 3: only chn_shardx_finish (chn_shardx_serve belongs to the owner and has no stage)
        refused(api, api.E_STATE, st.shardx_queries, buf, n_probes)
        refused(api, api.E_STATE, st.shardx_counts, splits)
        refused(api, api.E_STATE, st.shard_minimise_host, p)
        d_rows = api.device_malloc(0, n_probes * W * 8)
        st.shardx_serve(shards[0], buf, counts[0], d_rows)
        st.shardx_serve(shards[1], buf + 4 * counts[0], counts[1], d_rows + 8 * W * counts[0])
        st.shardx_finish(d_rows)
        refused(api, api.E_STATE, st.shardx_finish, d_rows)
        refused(api, api.E_STATE, st.shardx_minimise_host, p)  # a batch in flight: the list modes run alone
        util.assert_parity(st.wait_host(), c.oracle())
        api.device_free(0, d_rows)
        # dense batch open
        E = st.shard_minimise_host(p, *sc.columns(n))
        assert E == len(c.model()["values"])
        refused(api, api.E_STATE, st.shard_minimise_host, p)
        refused(api, api.E_STATE, st.shardx_minimise_host, p)
        refused(api, api.E_STATE, st.shardx_counts, splits)
        nwords = E * c.oidx.hash_funs * W
        other = api.Index(api.make_desc(c.oidx.bins, S + 2, c.oidx.bin_to_cat, c.oidx.ncat, sc.host_index(c.oidx), row_begin=0, row_end=8))
        refused(api, api.E_INVALID, st.shard_probe, other, buf, nwords, match="does not belong")
        other.destroy()
        refused(api, api.E_CAPACITY, st.shard_probe, shards[0], buf, nwords - 1, match="partial buffer too small")
        bufs = [buf, api.device_malloc(0, nwords * 8)]
        for sh, b in zip(shards, bufs):
            st.shard_probe(sh, b, nwords)
        total = api.device_download(0, bufs[0], nwords * 8, np.uint64) + api.device_download(0, bufs[1], nwords * 8, np.uint64)
        api.device_upload(0, buf, total)
        st.shard_finish(buf)
        refused(api, api.E_STATE, st.shard_finish, buf)
        refused(api, api.E_STATE, st.shard_probe, shards[0], buf, nwords)
        util.assert_parity(st.wait_host(), c.oracle())
        api.device_free(0, bufs[1])
    finally:
        api.device_free(0, buf)
        st.destroy()
        for sh in shards:
            sh.destroy()


def test_minimiser_log_overflow_is_reported_by_counts_and_the_stream_goes_on(api, oracle_lib):
    """CHN_STREAM_TINY_LOG: regions of about 64 entries per wavefront -- the large batch overruns them, chn_shardx_counts says so and
    closes the batch; a batch that fits then runs on the same stream"""
    from charon_amd import pack
    big, tiny = sc.case("w2"), sc.case("w2_tiny")
    S = big.oidx.bin_size
    splits = [0, S // 2, S]
    shards = sc.make_shards(api, big.oidx, splits)
    p = pack.pack_reads(big.reads)
    st = sc.open_stream(api, shards[1], big.oidx, len(big.reads), p["n_bases"], tiny_log=True)
    try:
        st.shardx_minimise_host(p, *sc.columns(len(big.reads)))
        refused(api, api.E_CAPACITY, st.shardx_counts, splits, match="minimiser log overflow")
        refused(api, api.E_STATE, st.shardx_counts, splits)
        out, rk = one_rank(api, big.oidx, st, shards, splits, tiny.reads)
        util.assert_parity(out, tiny.oracle())
        assert rk["counts"] == tiny.model(splits)["counts"]
    finally:
        st.destroy()
        for sh in shards:
            sh.destroy()


def test_batch_without_a_minimiser_through_both_chains(api, oracle_lib):
    """every read shorter than k: E = 0 and n_probes = 0, the caller's buffers have no bytes (null pointers), nothing is served"""
    c = sc.case("nomin")
    S = c.oidx.bin_size
    d = sc.run_dense(api, c.oidx, c.reads, None, [0, S // 2, S])
    assert d["E"] == 0 and d["values"].size == 0
    for out in d["outs"]:
        util.assert_parity(out, c.oracle())
    got = sc.run_sparse(api, c.oidx, [c.reads], None, [0, S // 2, S])
    assert got[0]["n_probes"] == 0 and got[0]["counts"] == [0, 0]
    util.assert_parity(got[0]["out"], c.oracle())
    assert not got[0]["out"]["num_hashes"].any() and (got[0]["out"]["call"] == 255).all()


def test_batches_of_other_shapes_in_turn_on_one_stream(api, oracle_lib):
    """A (16 owners, 300 reads), B (one owner, 5 reads), A again on one stream: the per-owner count buffer and the log regions are
    reused at other shapes; both runs of A give the same results and the same send_counts"""
    from charon_amd import pack
    big, few = sc.case("w2"), sc.case("w2_few")
    oidx, S = big.oidx, big.oidx.bin_size
    A = big.reads[:300]
    sp16 = sc.owner_splits16(S, big.model()["rows"])
    sh16, sh1 = sc.make_shards(api, oidx, sp16), sc.make_shards(api, oidx, [0, S])
    st = sc.open_stream(api, sh1[0], oidx, 300, pack.pack_reads(A)["n_bases"])
    try:
        a1, rk1 = one_rank(api, oidx, st, sh16, sp16, A)
        b, rkb = one_rank(api, oidx, st, sh1, [0, S], few.reads)
        a2, rk2 = one_rank(api, oidx, st, sh16, sp16, A)
        util.assert_same_results(a1, a2)
        assert rk1["counts"] == rk2["counts"] == sc.expected(big.po, oidx, A, None, sp16)["counts"]
        assert np.array_equal(np.sort(rk1["q"]), np.sort(rk2["q"]))
        orc = big.oracle()
        util.assert_parity(a1, {k: orc[k][:300] for k in ("num_hashes", "counts", "unique", "call", "conf", "probs")})
        util.assert_parity(b, few.oracle())
        assert rkb["counts"] == few.model()["counts"]
    finally:
        st.destroy()
        for sh in sh16 + sh1:
            if sh is not None:
                sh.destroy()
