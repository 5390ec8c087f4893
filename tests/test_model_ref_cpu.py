"""The vectorised float-exact restatement of Model::prob and the calls (oracle/pyref.py) that tests/test_gpu_model_call.py pins
k_model_call to: checked here against the C++ oracle, scipy.stats and itself.  No GPU."""
import os

import numpy as np
import pytest

from oracle import pyref
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_vectorised_model_prob_is_bit_equal_to_the_oracle(oracle_lib):
    tables = pyref.load_tables(os.path.join(ROOT, "charon_amd", "data", "default_kde.txt"))
    r = util.rng(101)
    x = np.concatenate([np.linspace(0, 1, 401, dtype=np.float32), r.uniform(0, 0.2, 300).astype(np.float32),
                        pyref.unique_props(np.arange(0, 151), 150),
                        np.float32([0.0, 1.0, 1e-45, 3e-41, 2.0 ** -127, 2.0 ** -126, 0.049999997, 0.05, 1.0000001])])
    got = pyref.kde_model_prob(x, np.sort(tables["pos"]), np.sort(tables["neg"]))
    want = np.array([oracle_lib.lib().orc_default_model_prob(float(v), 0) for v in x])
    assert len(np.unique(x)) > 800
    np.testing.assert_array_equal(got, want)
    # and the scalar restatement, one x at a time
    for v in x[::37]:
        assert got[list(x).index(v)] == pyref.model_prob(v, tables)[0]


@pytest.mark.parametrize("shape,scale", [(25.0, 0.02), (10.0, 0.005), (0.5, 0.3), (1.0, 0.1), (3.7, 0.0123)])
def test_dgamma_agrees_with_scipy(shape, scale):
    from scipy import stats
    xs = np.float32([1e-6, 1e-3, 0.01, 0.05, 0.1, 0.25, 0.5, 0.9, 1.0, 2.0])
    for x in xs:
        want = stats.gamma.pdf(float(x), shape, scale=scale)
        got = float(pyref.dgamma_mp(x, np.float32(shape), np.float32(scale)))
        if want == 0.0:  # below double range
            assert got < 1e-300
            continue
        # scipy takes the float64 parameters; the reference the float32 ones: evaluate scipy at those
        want = stats.gamma.pdf(float(x), float(np.float32(shape)), scale=float(np.float32(scale)))
        assert abs(got - want) <= 1e-12 * want, (x, got, want)
    # the boundary cases of the support
    assert pyref.dgamma(0.0, 0.5, 1.0) == np.inf and pyref.dgamma(0.0, 2.0, 1.0) == 0 and pyref.dgamma(0.0, 1.0, 0.25) == 4
    assert pyref.dgamma(-1e-7, 2.0, 1.0) == 0 and pyref.dgamma(np.inf, 2.0, 1.0) == 0
    assert np.isnan(pyref.dgamma(0.1, -1.0, 1.0)) and np.isnan(pyref.dgamma(0.1, 2.0, np.nan)) and np.isnan(pyref.dgamma(np.nan, 2, 1))


@pytest.mark.parametrize("a,b", [(6.0, 4.0), (6.0, 40.0), (0.5, 0.5), (1.0, 1.0), (2.5, 300.0), (123.4, 17.0)])
def test_dbeta_agrees_with_scipy(a, b):
    from scipy import stats
    for x in np.float32([1e-6, 1e-3, 0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.999]):
        want = stats.beta.pdf(float(x), float(np.float32(a)), float(np.float32(b)))
        got = float(pyref.dbeta_mp(x, np.float32(a), np.float32(b)))
        if want < 1e-290:
            assert got < 1e-280
            continue
        assert abs(got - want) <= 1e-12 * want, (x, got, want)
    assert pyref.dbeta(0.0, 0.5, 2.0) == np.inf and pyref.dbeta(1.0, 2.0, 0.5) == np.inf and pyref.dbeta(0.0, 1.0, 6.0) == 6
    assert pyref.dbeta(1.0, 6.0, 1.0) == 6 and pyref.dbeta(1.5, 2.0, 2.0) == 0 and pyref.dbeta(0.5, np.inf, np.inf) == np.inf
    assert pyref.dbeta(0.0, 0.0, 0.0) == np.inf and pyref.dbeta(0.3, 0.0, 0.0) == 0 and np.isnan(pyref.dbeta(0.3, -1.0, 2.0))


def test_float32_rounding_is_done_once():
    import mpmath as mp
    one = np.float32(1.0)
    assert pyref._round_f32(mp.mpf(1) + mp.mpf(2) ** -24) == one  # a tie rounds to even
    with mp.workprec(100):
        above_tie = mp.mpf(1) + mp.mpf(2) ** -24 + mp.mpf(2) ** -80
    assert pyref._round_f32(above_tie) == np.nextafter(one, np.float32(2))  # (through a double, 1 + 2^-24 would be a tie)
    assert pyref._round_f32(mp.mpf(2) ** -149 * mp.mpf("0.6")) == np.float32(2.0 ** -149)
    assert pyref._round_f32(mp.mpf(2) ** 200) == np.inf


@pytest.mark.parametrize("ncat", [3, 8])
def test_call_category_agrees_with_the_oracle(oracle_lib, ncat):
    """recomputed from the oracle's own counts and probabilities, as test_call_host_two_restatements_agree does for call_host"""
    r = util.rng(200 + ncat)
    gs = [util.random_seq(r, 3000) for _ in range(ncat)]
    oidx = util.build_oracle_index(oracle_lib, [[g] for g in gs], list(range(ncat)), ["c%d" % i for i in range(ncat)])
    m1 = util.sample_reads(r, gs, 300, (40, 200), sub_rate=0.03, random_fraction=0.2)
    m2 = util.sample_reads(r, gs, 300, (40, 200), sub_rate=0.03, random_fraction=0.2)
    m1[0], m2[0] = b"ACGT", b"A" * 30  # no minimiser: num_hashes 0
    seqs, offs, split = util.concat(m1, m2)
    for conf_thr, min_pd, min_hits in ((7, 0.04, 0), (255, 0.0, 0), (2, 0.0, 3)):
        thr = oracle_lib.default_thresholds(paired=True)
        thr.confidence_threshold, thr.min_proportion_difference, thr.min_hits = conf_thr, min_pd, min_hits
        o = oidx.process_reads(seqs, offs, mate_split=split, mq_const=30.0, thr=thr)
        seen = set()
        for i in range(len(m1)):
            call, conf = pyref.call_category(o["unique"][i], o["counts"][i], o["probs"][i], o["num_hashes"][i], 30.0,
                                             len(m1[i]) + len(m2[i]), o["compression"][i], conf_thr=conf_thr, min_pd=min_pd,
                                             min_hits=min_hits)
            assert (call, conf) == (int(o["call"][i]), int(o["conf"][i])), i
            seen.add(call)
        assert len(seen) >= 3
    oidx.free()


def test_unsorted_table_is_order_sensitive():
    """the order test of the GPU file proves something only if the data-order and the sorted-order float sums differ"""
    t = util.kde_tables()["trained"]
    assert not np.all(np.diff(t) >= 0)
    x = pyref.unique_props(np.arange(0, 301), 300)
    for h in (0.1, 0.001):
        a, b = pyref.kde_prob_vec(x, t, h), pyref.kde_prob_vec(x, np.sort(t), h)
        assert (a != b).sum() >= 10
