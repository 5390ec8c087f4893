"""GPU parity tests (-m gpu) of chained row-log entries (charon_amd/csrc/parts/rowlog_entry.hpp): with at most 128 bins the ordinary
launch of k_minimise_probe logs a row of 4..6 set bins as two consecutive entries instead of storing its full words in the escaped-row
region, and k_count_wavelog judges the two together.  Indexes dense enough that every probe round mixes rows of at most 3, of 4..6 and of
7 and more set bins, at bin counts that fill the last word or not, beside logs that stay unchained (more than 128 bins, the SPLIT launch,
the re-run after a log overflow).  Integer columns must equal the CPU oracle's; unless a case says otherwise no batch may have been
re-run -- the chained path is what ran."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

# How the dense indexes and their reads are made.  The log regions are sized by read length alone: per minimiser of random sequence two
# entries and, at up to 128 bins, a quarter of an escaped row (wave_log_cap, wave_esc_cap; more than 128 bins: one escaped row).  A row that
# the fill alone sets has Poisson(4.3) set bins: 1.45 entries and 0.15 rows of seven and more per minimiser.  What the bins' own genomes add
# to the fill counts: 100 minimisers per bin in 7 001 rows would raise 4.3 to 5.4 and put three rows in ten beyond six set bins, past the
# escaped-row region whatever the reads -- that is the re-run, which these cases are not about.  So the genomes are short (300 bases, some
# 25 minimisers, + 1 % of fill) and a read is random sequence with a mutated copy of one genome written into it: its hits have one set bin
# more, the rest of it sees the fill alone.


def _reads(r, gs, n, length):
    out = []
    for _ in range(n):
        L = int(length if np.isscalar(length) else r.integers(length[0], length[1] + 1))
        a = bytearray(util.random_seq(r, L))
        if r.random() < 0.7 and L > 0:
            g = util.mutate(r, gs[int(r.integers(0, len(gs)))], 0.02)[:L]
            at = int(r.integers(0, L - len(g) + 1))
            a[at:at + len(g)] = g
        out.append(bytes(a))
    return out


def _fill_for(B, per_row=4.3):
    """the fill at which the AND of three rows keeps about `per_row` of B bins (0.35 at 100 bins)"""
    return (per_row / B) ** (1.0 / 3.0)


@pytest.fixture(scope="module")
def api():
    import charon_amd.api as api
    return api


def _dense_index(oracle_lib, r, B, b2c, cats, fill=0.35, bin_size=7001):
    """B bins of one 300-base genome each under a heavy random fill: the AND of three rows keeps fill^3 of the bins (0.043 at 0.35: about
    4.3 set bins per row at 100 bins)"""
    gs = [util.random_seq(r, 300) for _ in range(B)]
    oidx = util.build_oracle_index(oracle_lib, [[g] for g in gs], b2c, cats, bin_size=bin_size, fill_seed=B, fill=fill)
    return gs, oidx


@pytest.fixture(scope="module")
def dense100(oracle_lib):
    r = util.rng(1409)
    gs, oidx = _dense_index(oracle_lib, r, 100, [i % 2 for i in range(100)], ["human", "microbial"])
    assert oidx.bin_words == 2
    yield gs, oidx
    oidx.free()


def _run(api, oidx, reads, mates=None, tiny_log=False, split_bucket=0):
    """-> (results, the oracle's results, batches re-run after a log overflow)"""
    from charon_amd import pack
    g = util.gpu_index_from_oracle(api, oidx)
    try:
        p = pack.pack_reads(reads, mates)
        n = len(reads)
        st = api.Stream(g, n, p["n_bases"], tiny_log=tiny_log, split_bucket=split_bucket)
        paired = mates is not None
        st.set_model(api.default_model(g.desc.num_categories, 0 if paired else g.desc.host_index, paired=paired))
        st.submit_host(p, np.full(n, 40.0, np.float32), np.zeros(n, np.float32))
        out = st.wait_host()
        reruns = st.profile(4)[1]
        st.destroy()
    finally:
        g.destroy()
    seqs, offs, split = util.concat(reads, mates)
    return out, oidx.process_reads(seqs, offs, mate_split=split, mq_const=40.0), reruns


def test_mixed_row_densities_at_100_bins(api, dense100):
    """about 4.3 set bins per row: every round holds single entries, chains and escaped rows, some 93 entries per round of 64 rows -- more
    than the staging buffer takes beside a nearly full store, so the early flush of whole 256-byte pieces runs routinely"""
    gs, oidx = dense100
    r = util.rng(1)
    reads = _reads(r, gs, 300, (100, 2000))
    out, orc, reruns = _run(api, oidx, reads)
    util.assert_parity(out, orc)
    assert reruns == 0
    assert out["unique"].sum() > 0


@pytest.mark.parametrize("B", [128, 64, 130])
def test_other_widths(api, oracle_lib, B):
    """128 bins: the last word is full, bin indices use all seven bits; 64 bins, two to a category: one word, still the row log; 130 bins:
    three words, no chain mode -- rows of more than three set bins escape as before.  The fill follows the bin count so that a row keeps
    about 4.3 set bins as at 100 bins (at 0.35, 128 bins would keep 5.5 and three rows in ten would have seven and more: beyond the
    escaped-row region whatever the reads)"""
    r = util.rng(B)
    if B == 64:
        b2c, cats = [i // 2 for i in range(B)], ["human"] + ["c%d" % i for i in range(1, 32)]
    else:
        b2c, cats = [i % 2 for i in range(B)], ["human", "microbial"]
    gs, oidx = _dense_index(oracle_lib, r, B, b2c, cats, fill=_fill_for(B))
    assert oidx.bin_words == (B + 63) // 64
    try:
        if B == 64:  # more than two categories: the paired caller (call_category); 16-bit totals do not apply to pairs
            m1 = _reads(r, gs, 300, (50, 1000))
            m2 = _reads(r, gs, 300, (50, 1000))
            out, orc, reruns = _run(api, oidx, m1, m2)
        else:
            out, orc, reruns = _run(api, oidx, _reads(r, gs, 300, (100, 2000)))
        util.assert_parity(out, orc)
        assert reruns == 0
    finally:
        oidx.free()


def test_lightly_filled_index_overflows_and_reruns_unchained(api, oracle_lib):
    """the index of test_row_log_overflow_reruns_on_worst_case_buffers with the tiny log: the first run overflows and the batch is re-run
    on worst-case regions, one entry per base -- without chains"""
    r = util.rng(55)
    gs = [util.random_seq(r, 3000) for _ in range(70)]
    oidx = util.build_oracle_index(oracle_lib, [[g] for g in gs], [i % 2 for i in range(70)], ["human", "microbial"], bin_size=9001, fill_seed=8, fill=0.10)
    try:
        reads = util.sample_reads(r, gs, 500, (50, 2500), sub_rate=0.03) + [b"A" * 900, b"", b"ACGT" * 200]
        out, orc, reruns = _run(api, oidx, reads, tiny_log=True)
        util.assert_parity(out, orc)
        assert reruns == 1
    finally:
        oidx.free()


def test_a_long_read_in_the_batch_stays_unchained(api, dense100):
    """lowered split limit (reads of 1 024 bases and more go one to a wavefront): the SPLIT launch and k_count_longlog keep unchained logs
    beside the chained logs of the ordinary launch"""
    gs, oidx = dense100
    r = util.rng(4)
    reads = _reads(r, gs, 200, (100, 900))
    reads.insert(77, _reads(r, gs, 1, 1100)[0])
    assert len(reads[77]) >= 1024 and max(len(s) for i, s in enumerate(reads) if i != 77) < 1024
    out, orc, reruns = _run(api, oidx, reads, split_bucket=64)
    util.assert_parity(out, orc)
    assert reruns == 0 and out["num_hashes"][77] > 80


def test_paired_reads(api, dense100):
    """2 x 150 bases, call_category: two segments per lane, 32-bit totals in the count kernel"""
    gs, oidx = dense100
    r = util.rng(5)
    m1 = _reads(r, gs, 300, 150)
    m2 = _reads(r, gs, 300, 150)
    out, orc, reruns = _run(api, oidx, m1, m2)
    util.assert_parity(out, orc)
    assert reruns == 0
