"""GPU parity tests (-m gpu) of the probe kernel's packed window ring and of the count kernel with all 64 owners in one sweep.

A ring slot of k_minimise_probe holds (value << pb) | (wn - 1 - offset), pb = bits(wn - 1), where the index's (k, window) leave the
room (charon_amd/csrc/parts/lds_budget.hpp: ring_pack_ok); otherwise the offsets stay in a byte plane of their own.  The complemented
offset decides which of two equal values a suffix minimum keeps, so the shapes here are the ones with ties: homopolymers, short-period
repeats, repeats that come and go, reads around one window, N runs across block ends, pieces of split reads that start cold -- in
row-log mode (B = 100, W = 2), with conditional probing (B = 2, W = 1), and for (k, w) on both sides of the packing rule.  Everything is
compared with the CPU oracle through tests/util.assert_parity (num_hashes, counts, unique counts, call; confidence and probabilities too)."""
import numpy as np
import pytest

from oracle import pyref
from tests import util
from tests.test_gpu_parity import run_oracle

pytestmark = pytest.mark.gpu

ROWS = 65537  # rows of every index here (2^16 .. 2^20 asked for; a non-power of two)


@pytest.fixture(scope="module")
def api():
    import charon_amd.api as api
    return api


def pack_ok(k, w):
    """the rule of lds_budget.hpp, restated: bits(max(5^k - 1, seed >> (64 - 2k))) + bits(wn - 1) <= 64"""
    wn = w - k + 1
    return max(5 ** k - 1, pyref.SEED >> (64 - 2 * k)).bit_length() + (wn - 1).bit_length() <= 64


def k2_owners(B, C, W, k=19, w=41, h=3):
    """owners per sweep the host picks for k_count_wavelog (16-bit totals), restated from lds_budget.hpp"""
    wn = w - k + 1
    probe = wn * 64 * 8 + 128 * 12 + (0 if pack_ok(k, w) else wn * 64) + 2 * h * (1 if W <= 2 else 2) * 1024
    probe = (probe + 15) // 16 * 16 + 5 * 64 * 4
    probe = (probe + 255) // 256 * 256
    budget = max(7680, 163840 - 163840 // probe * probe - 1024)
    G = 64
    while G > 8 and G * ((B + 1) // 2) * 4 + (G * C + (G * C & 1)) * 4 + G * W * 8 + G * C + 16 > budget:
        G //= 2
    return G


def run_gpu(api, g, reads, split_bucket=0):
    from charon_amd import pack
    p = pack.pack_reads(reads)
    n = len(reads)
    st = api.Stream(g, n, p["n_bases"], split_bucket=split_bucket)
    st.set_model(api.default_model(g.desc.num_categories, g.desc.host_index))
    st.submit_host(p, np.full(n, 40.0, np.float32), np.zeros(n, np.float32))
    out = st.wait_host()
    st.destroy()
    return out


def check(api, oidx, reads, split_bucket=0):
    assert 64 <= len(reads) <= 256
    g = util.gpu_index_from_oracle(api, oidx)
    try:
        out = run_gpu(api, g, reads, split_bucket)
        util.assert_parity(out, run_oracle(oidx, reads))
        return out
    finally:
        g.destroy()


def low_complexity(r):
    """sequence planted in the indexes so that the tie reads also hit"""
    return b"A" * 200 + util.random_seq(r, 150) + b"AC" * 120 + util.random_seq(r, 90) + b"ACGT" * 70 + b"ACGGTCA" * 50 + b"T" * 90


def build_pair(po, k, w, seed, rows_bins=100):
    """(genomes, row-log index of `rows_bins` bins in two categories, conditional-probing index of 2 bins) for (k, w)"""
    r = util.rng(seed)
    gs = [util.random_seq(r, 1500) for _ in range(rows_bins)]
    gs[0] = gs[0] + low_complexity(r)
    gs[1] = low_complexity(r) + gs[1]
    rows = util.build_oracle_index(po, [[g] for g in gs], [i % 2 for i in range(rows_bins)], ["human", "microbial"], k=k, w=w, bin_size=ROWS,
                                   fill_seed=seed + 1, fill=0.03)
    cond = util.build_oracle_index(po, [gs[0::2][:6], gs[1::2][:6]], [0, 1], ["host", "microbial"], k=k, w=w, bin_size=ROWS, fill_seed=seed + 2, fill=0.2)
    return gs, rows, cond


@pytest.fixture(scope="module")
def default_pair(oracle_lib):
    gs, rows, cond = build_pair(oracle_lib, 19, 41, 100)
    assert rows.bin_words == 2 and cond.bin_words == 1 and cond.bins == 2
    yield gs, rows, cond
    rows.free(); cond.free()


def tie_reads(r, gs, k, w):
    """reads whose windows tie, around one window long, and enough ordinary ones to fill more than one wavefront"""
    wn = w - k + 1
    reads = [c * n for c in (b"A", b"C", b"G", b"T") for n in (100, 999, 3000)]                     # homopolymers
    reads += [b"AC" * 50, b"GT" * 1500, b"ACGT" * 25, b"TGCA" * 750, b"ACGGTCA" * 15, b"ACGGTCA" * 428]  # periods 2, 4, 7
    reads += [(b"AG" * 2000)[:n] for n in (101, 2 * wn + k, 2 * wn + k - 1, 3 * wn + k + 1)]          # a period against the block length
    reads += [util.random_seq(r, 700) + b"AC" * 400 + util.random_seq(r, 900),                       # a repeat that starts and stops inside a read
              util.random_seq(r, wn + 3) + b"T" * (5 * wn + 1) + util.random_seq(r, 333) + b"CAG" * 130 + util.random_seq(r, 40),
              b"G" * 500 + util.random_seq(r, 1000), util.random_seq(r, 1000) + b"G" * 500,
              gs[0][-700:], gs[1][:800], gs[0][1400:1900]]
    reads += [util.random_seq(r, n) for n in (1, k - 1, k, k + 1, w - 2, w - 1)] + [b"A" * (k - 1), b"A" * k, b"AC" * ((w - 1) // 2)]  # shorter than one window
    reads += [util.random_seq(r, w), b"A" * w, (b"AC" * w)[:w], util.random_seq(r, w + 1), b"C" * (w + 1), util.random_seq(r, w + wn), b"T" * (w + wn - 1)]  # exactly k + wn - 1, and next to it
    reads += util.sample_reads(r, gs[:12], 150 - len(reads), (100, 3000), sub_rate=0.03)
    return reads


@pytest.mark.parametrize("mode", ["rows", "cond"])
def test_ties(api, default_pair, mode):
    """B = 100, W = 2 (row log) and B = 2, W = 1 (conditional probing) at the default (19, 41): the fixed-window instance, always packed"""
    gs, rows, cond = default_pair
    assert pack_ok(19, 41)
    reads = tie_reads(util.rng(5), gs, 19, 41)
    out = check(api, rows if mode == "rows" else cond, reads)
    assert out["num_hashes"][2] == 1 + (3000 - 41) // 23      # homopolymer: the first window, then one emission per expiry
    assert out["counts"].sum() > 0


# default; wn = 1; wn a power of two (16: pb = 4) and one more (17: pb = 5); the largest k that still packs at its window (63 + 1 bits);
# and without room: k = 27 with wn = 3, the default window of 23 at k = 26 (leaves the fixed-window instance), a wide window at large k
KW = [(19, 41), (21, 21), (19, 34), (19, 35), (27, 28), (27, 29), (26, 48), (25, 64)]


def test_kw_cases_lie_on_both_sides_of_the_rule():
    sides = {kw: pack_ok(*kw) for kw in KW}
    assert sides == {(19, 41): True, (21, 21): True, (19, 34): True, (19, 35): True, (27, 28): True, (27, 29): False, (26, 48): False, (25, 64): False}
    assert any(sides.values()) and not all(sides.values())
    assert (34 - 19).bit_length() == 4 and (35 - 19).bit_length() == 5                      # the pb edge
    assert (5 ** 27 - 1).bit_length() + 1 == 64                                             # k = 27, the largest k there is, packs a window of two values


@pytest.mark.parametrize("kw", KW)
def test_kw_pairs(api, oracle_lib, kw):
    k, w = kw
    r = util.rng(1000 + 31 * k + w)
    gs, rows, cond = build_pair(oracle_lib, k, w, 200 + 31 * k + w, rows_bins=10)
    reads = tie_reads(r, gs, k, w)[:128]
    assert rows.bin_words == 1
    for oidx in (rows, cond):
        check(api, oidx, reads)
    rows.free(); cond.free()


def n_reads(r, gs, k, w):
    """random and planted reads with N runs placed across the ends of the blocks of wn values (value p ends a block when p % wn == wn - 1;
    base i completes value i + 1 - k)"""
    wn = w - k + 1
    out = []
    for j, run in enumerate((1, 2, 5, wn - 1, wn, wn + 1, k, w, 3 * wn)):
        for src in (util.random_seq(r, 1200 + 37 * j), gs[j % 4][100:1300 + 11 * j]):
            a = bytearray(src)
            for m in (1, 3, 4, 9):
                end = k - 1 + m * wn + wn - 1            # base completing the last value of block m
                s = max(0, end - run // 2 + (j % 3) - 1)
                a[s:s + run] = b"N" * min(run, len(a) - s)
            out.append(bytes(a))
    out += [b"N" * 100, b"A" * 500 + b"N" + b"A" * 500, b"AC" * 100 + b"N" * wn + b"AC" * 300, b"ACGTN" * 200, util.random_seq(r, 130) + b"N" * 7]
    out += util.sample_reads(r, gs[:8], 96 - len(out), (100, 3000), sub_rate=0.02)
    return out


def test_n_runs_across_block_ends(api, oracle_lib, default_pair):
    gs, rows, cond = default_pair
    reads = n_reads(util.rng(6), gs, 19, 41)
    check(api, rows, reads)
    check(api, cond, reads)
    # the general instance, packed (wn = 50, pb = 6)
    assert pack_ok(11, 60)
    gs2, rows2, cond2 = build_pair(oracle_lib, 11, 60, 300, rows_bins=10)
    reads = n_reads(util.rng(7), gs2, 11, 60)
    check(api, rows2, reads)
    check(api, cond2, reads)
    rows2.free(); cond2.free()


def test_split_reads_start_cold_on_a_packed_ring(api, default_pair):
    """CHN_STREAM_SPLIT_BUCKET(64): reads of 1 024 bases and more are cut over the lanes of a wavefront; a piece starts cold unless its
    first window ties, in which case its predecessor runs on"""
    gs, rows, cond = default_pair
    r = util.rng(8)
    reads = tie_reads(r, gs, 19, 41)[:100]
    reads += [util.mutate(r, (gs[0] + gs[2] + gs[4])[:3000], 0.03), util.random_seq(r, 2999), util.random_seq(r, 1024), util.random_seq(r, 1023),
              util.random_seq(r, 1100) + b"A" * 900 + util.random_seq(r, 1000), (b"ACGTTGCA" * 40 + util.random_seq(r, 300)) * 4]
    for oidx in (rows, cond):
        out = check(api, oidx, reads, split_bucket=64)
        g = util.gpu_index_from_oracle(api, oidx)
        util.assert_same_results(out, run_gpu(api, g, reads, split_bucket=255))  # one lane per read
        g.destroy()


@pytest.mark.parametrize("bins", [100, 128])
def test_count_kernel_owner_groups(api, oracle_lib, bins):
    """128 reads (two wavefront logs) in which every owner slot hits another bin of each category, some rows with more than three set
    bins (escaped rows): B = 100 is counted with all 64 owners in one sweep, the tables of B = 128 no longer fit and it falls back to 32"""
    assert k2_owners(100, 2, 2) == 64 and k2_owners(128, 2, 2) == 32
    r = util.rng(900 + bins)
    gs = [util.random_seq(r, 900) for _ in range(bins)]
    shared = util.random_seq(r, 400)
    for b in (0, 1, 2, 3, 4, 5, 64, 65, bins - 2, bins - 1):
        gs[b] = gs[b] + shared                                       # rows of `shared` have ten set bins: escaped
    oidx = util.build_oracle_index(oracle_lib, [[g] for g in gs], [i % 2 for i in range(bins)], ["human", "microbial"], bin_size=ROWS,
                                   fill_seed=bins, fill=0.04)
    assert oidx.bin_words == (bins + 63) // 64
    reads = []
    for j in range(128):
        b0, b1 = 2 * ((j * 3) % (bins // 2)), 2 * ((j * 5 + 1) % (bins // 2)) + 1    # owner j: its own bin of category 0 and of category 1
        rd = util.mutate(r, gs[b0][50:50 + 300 + (j % 7) * 40], 0.01) + util.mutate(r, gs[b1][100:100 + 250 + (j % 5) * 60], 0.01)
        if j % 3 == 0:
            rd += shared[(j % 4) * 20:200 + (j % 9) * 20]
        reads.append(rd)
    out = check(api, oidx, reads)
    assert (out["counts"] > 0).all(axis=1).sum() >= 120 and out["unique"].sum() > 0
    oidx.free()
