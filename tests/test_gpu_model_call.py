"""k_model_call itself, through chn_classify_counts_raw (no host re-evaluation), on counts tables built for the purpose, against
the float-exact restatement of oracle/pyref.py: KDE and parametric probabilities to the float ulp, the two calls exactly on the
device's own probabilities, the borderline-flag contract, the memo, the fixed-up chn_classify_counts, and the device-resident
results of waited batches surviving a counts-only call."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from oracle import pyref
from tests import util

pytestmark = pytest.mark.gpu

H28 = 1 << 28
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def api():
    import charon_amd.api as api
    return api


def counts_stream(api, ncat, max_reads):
    """a stream on a tiny index with the right category count: classify_counts never reads the index"""
    g = api.Index(api.make_desc(ncat, 64, list(range(ncat)), ncat, 0))
    return g, api.Stream(g, max_reads, 1 << 12)


def kde_model(api, pos, neg, h_pos=0.1, h_neg=0.001, paired=False, host=0, **kw):
    """a KDE model with per-category datasets (lists of float32 arrays, iterated in the order given)"""
    ncat = len(pos)
    m = api.default_model(ncat, host, paired=paired, **kw)
    keep = [np.ascontiguousarray(t if len(t) else np.zeros(1), np.float32) for t in list(pos) + list(neg)]
    fp = C.POINTER(C.c_float)
    pd = (fp * ncat)(*[k.ctypes.data_as(fp) for k in keep[:ncat]])
    nd = (fp * ncat)(*[k.ctypes.data_as(fp) for k in keep[ncat:]])
    pn = (C.c_uint32 * ncat)(*[len(t) for t in pos])
    nn = (C.c_uint32 * ncat)(*[len(t) for t in neg])
    m._keep_kde = (keep, pd, nd, pn, nn)
    m.pos_data, m.neg_data, m.pos_n, m.neg_n = pd, nd, pn, nn
    m.h_pos, m.h_neg = h_pos, h_neg
    return m


def default_tables():
    """the default datasets, sorted as the KDEParams constructor leaves them"""
    t = pyref.load_tables(os.path.join(ROOT, "charon_amd", "data", "default_kde.txt"))
    return np.sort(t["pos"]), np.sort(t["neg"])


def ulps(a, ref):
    """|a - ref| in float32 ulps of ref; NaN positions must agree (sign free); both at or below 2^-126 counts as 0 within 2^-126"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(ref)), np.flatnonzero(np.isnan(a) != np.isnan(ref))[:10]
    ok = ~np.isnan(ref)
    a, ref = a[ok], ref[ok]
    same = (a == ref)
    unit = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.where(same, 0.0, np.abs(a - ref) / unit)
    tiny = (np.abs(a) <= pyref.F32_MIN_NORMAL) & (np.abs(ref) <= pyref.F32_MIN_NORMAL) & (np.abs(a - ref) <= pyref.F32_MIN_NORMAL)
    d[tiny & ~same] = 0.0
    return d, same


def raw(st, nh, counts, unique, lengths=None, mq=None, comp=None):
    n = len(nh)
    lengths = np.full(n, 1000, np.uint32) if lengths is None else lengths
    mq = np.full(n, 40.0, np.float32) if mq is None else mq
    comp = np.full(n, 0.5, np.float32) if comp is None else comp
    return st.classify_counts_raw(nh, counts, unique, lengths, mq, comp)


def grid_rows(max_nh=300):
    """every (uq, nh) with 0 <= uq <= nh <= max_nh, uq > nh and nh = 0 rows, and num_hashes up to 2^28 + 5 (no memo there)"""
    nh, uq = [], []
    for n in range(0, max_nh + 1):
        nh += [n] * (n + 1)
        uq += list(range(n + 1))
    extra = [(1, 0), (7, 0), (5, 3), (max_nh + 1, max_nh), (2, 1), (H28 - 1, H28 - 1), (3, H28 - 1), (H28, H28), (12345, H28),
             (H28 + 5, H28 + 5), (H28 + 4, H28 + 5), (1, H28 + 5), (H28 + 6, H28 + 5), ((1 << 24) + 1, (1 << 24) + 3)]
    uq += [e[0] for e in extra]
    nh += [e[1] for e in extra]
    return np.array(uq, np.uint32), np.array(nh, np.uint32)


def ref_by_distinct_x(x, fn):
    """fn evaluated once per distinct float32 x (NaN included), mapped back"""
    flat = x.ravel()
    key = flat.view(np.uint32)
    u, inv = np.unique(key, return_inverse=True)
    return fn(u.view(np.float32))[inv].reshape(x.shape)


# ---- KDE --------------------------------------------------------------------------------------------------------------------
KDE_NAMES = ["n0", "n1", "n63_dup", "n64_inf", "n65_nan", "trained", "n4097", "default"]


def kde_setup():
    t = util.kde_tables()
    t["default"] = default_tables()[0]
    pos = [t[k] for k in KDE_NAMES]
    neg = [t[KDE_NAMES[(c + 3) % 8]] for c in range(8)]
    neg[KDE_NAMES.index("default")] = default_tables()[1]
    return pos, neg


@pytest.mark.parametrize("h_pos,h_neg", [(0.1, 0.001), (1e-4, 10.0), (1e-3, 0.1), (10.0, 1e-4)])
def test_kde_probabilities_to_the_ulp(api, h_pos, h_neg):
    pos, neg = kde_setup()
    uq, nh = grid_rows()
    n = len(nh)
    g, st = counts_stream(api, 8, n)
    st.set_model(kde_model(api, pos, neg, h_pos, h_neg))
    U = np.repeat(uq[:, None], 8, axis=1)
    out = raw(st, nh, U, U)
    x = pyref.unique_props(uq, nh)
    total_same = total = 0
    worst = 0.0
    for c in range(8):
        ref = ref_by_distinct_x(x, lambda xs: pyref.kde_model_prob(xs, pos[c], neg[c], h_pos, h_neg))
        d, same = ulps(out["probs"][:, c], ref)
        assert d.max(initial=0) <= 2, (KDE_NAMES[c], d.max(), np.argmax(d))
        worst = max(worst, d.max(initial=0))
        total_same += same.sum() + np.isnan(ref).sum()
        total += n
    print("KDE h=(%g, %g): bit-equal %.6f of %d cells, worst %.1f ulp" % (h_pos, h_neg, total_same / total, total, worst))
    assert total_same >= 0.999 * total
    # a sorted copy of the unsorted table gives other bits: the kernel really sums in data order
    c = KDE_NAMES.index("trained")
    srt = ref_by_distinct_x(x, lambda xs: pyref.kde_model_prob(xs, np.sort(pos[c]), neg[c], h_pos, h_neg))
    if h_pos < 1:
        assert (out["probs"][:, c] != srt[:]).sum() > 0
    st.destroy()
    g.destroy()


def test_kde_formula_against_exact_arithmetic(api):
    """the whole probability evaluated exactly (mpmath) from the same float32 t values (and the same float32 dexp argument): the
    kernel is within the float summation bound 2 n 2^-24 relative (n = the points of both datasets plus two) plus 4 ulps"""
    import mpmath as mp
    t = util.kde_tables()
    dpos, dneg = default_tables()
    pos = [t["n1"], t["n63_dup"], t["trained"], dpos]
    neg = [dneg, t["n1"], t["n63_dup"], t["n4097"][:1000]]
    h_pos, h_neg = np.float32(0.1), np.float32(0.01)
    r = util.rng(5)
    nh = r.integers(20, 300, 50).astype(np.uint32)
    uq = (r.random(50) * (nh + 1) * 0.4).astype(np.uint32)
    uq[0] = nh[0]  # x == 1
    g, st = counts_stream(api, 4, 64)
    st.set_model(kde_model(api, pos, neg, float(h_pos), float(h_neg)))
    U = np.repeat(uq[:, None], 4, axis=1)
    out = raw(st, nh, U, U)
    x = pyref.unique_props(uq, nh)
    rate = np.float32(300)

    def dens(xv, data, h):
        ts = ((xv - data) / h).astype(np.float64)
        return mp.fsum(mp.exp(-mp.mpf(v) ** 2 / 2) for v in ts) / mp.sqrt(2 * mp.pi) / (mp.mpf(float(h)) * len(data))
    with mp.workdps(30):
        for c in range(4):
            for i in range(len(x)):
                xv = x[i]
                p_pos = mp.mpf(1) if xv == 1 else dens(xv, pos[c], h_pos)
                p_neg = dens(xv, neg[c], h_neg)
                arg = np.float32(np.float32(math.log(300.0)) - rate * xv)
                exact = p_pos / (mp.exp(mp.mpf(float(arg))) + p_pos + p_neg)
                nn = len(pos[c]) + len(neg[c]) + 2
                tol = 2 * nn * 2.0 ** -24 * float(exact) + 4 * float(np.spacing(np.float32(exact)))
                assert abs(out["probs"][i, c] - float(exact)) <= tol, (c, float(xv), out["probs"][i, c], float(exact))
    st.destroy()
    g.destroy()


# ---- gamma / beta -----------------------------------------------------------------------------------------------------------
NAN = float("nan")
INF = float("inf")
GAMMA = [((25, 0, 0.02), (10, 0, 0.005)), ((8.3, 0.0, 0.031), (2.2, -0.001, 0.004)), ((0.5, 0.25, 0.1), (1.0, 0.25, 0.05)),
         ((3.0, 0.25, 0.02), (1.0, 0.5, 0.2)), ((-1.0, 0, 0.1), (2.0, 0, NAN)), ((0.7, -0.1, 0.3), (1.5, 0.0, 0.05))]
_AB = [0.0, 0.5, 1.0, 6.0, INF]
BETA = [((6, 4, 0), (6, 40, 0)), ((3.1, 9.7, 0), (1.3, 55.0, 0)), ((-1.0, 2.0, 0), (NAN, 2.0, 0))] + \
       [((a, b, 0), (b, a, 0)) for a in _AB for b in _AB]


@pytest.mark.parametrize("dist", ["gamma", "beta"])
def test_parametric_probabilities_to_the_ulp(api, dist):
    params = GAMMA if dist == "gamma" else BETA
    ncat = len(params)
    uq, nh = grid_rows(48)
    uq, nh = uq[:-6], nh[:-6]  # (the 2^28 rows add nothing here)
    g, st = counts_stream(api, ncat, len(nh))
    pp = [p[0] for p in params]
    nn = [p[1] for p in params]
    st.set_model(api.default_model(ncat, 0, paired=True, dist=dist, pos_params=pp, neg_params=nn))
    U = np.repeat(uq[:, None], ncat, axis=1)
    out = raw(st, nh, U, U)
    x = pyref.unique_props(uq, nh)
    same_n = total = 0
    worst = 0.0
    cache = {}
    for c in range(ncat):
        key = (tuple(pp[c]), tuple(nn[c]))

        def fn(xs):
            return pyref.dist_model_prob(xs, dist, np.float32(pp[c]), np.float32(nn[c]))
        if key not in cache:
            cache[key] = ref_by_distinct_x(x, fn)
        ref = cache[key]
        d, same = ulps(out["probs"][:, c], ref)
        assert d.max(initial=0) <= 4, (dist, params[c], d.max(), x[~np.isnan(ref)][np.argmax(d)])
        worst = max(worst, d.max(initial=0))
        same_n += same.sum() + np.isnan(ref).sum()
        total += len(nh)
    print("%s: bit-equal %.6f of %d cells, worst %.1f ulp" % (dist, same_n / total, total, worst))
    st.destroy()
    g.destroy()


# ---- the calls on the device's own probabilities ----------------------------------------------------------------------------
def random_rows(r, n, ncat, thr):
    """rows that hit the call logic's edges: gates at their thresholds and NaN, unique differences > 255, counts[first] <
    counts[second], ties among 2, 3 and all categories"""
    nh = r.integers(0, 1200, n).astype(np.uint32)
    uq = (r.random((n, ncat)) * (nh[:, None] + 1) * r.choice([0.05, 0.3, 1.0], (n, 1))).astype(np.uint32)
    kind = r.integers(0, 6, n)
    top = uq.max(axis=1)
    for i in np.flatnonzero(kind == 1):  # tie of two
        a, b = r.choice(ncat, 2, replace=False)
        uq[i, a] = uq[i, b] = top[i]
    for i in np.flatnonzero(kind == 2):  # tie of three (or all when C <= 3)
        idx = r.choice(ncat, min(3, ncat), replace=False)
        uq[i, idx] = top[i]
    uq[kind == 3] = top[kind == 3][:, None]  # all C tie
    dom = np.flatnonzero(kind == 5)  # one category far ahead: unique differences beyond 255
    nh[dom] = r.integers(300, 1200, dom.size)
    uq[dom] = (r.random((dom.size, ncat)) * 20).astype(np.uint32)
    uq[dom, r.integers(0, ncat, dom.size)] = nh[dom] - r.integers(0, 20, dom.size).astype(np.uint32)
    counts = uq + r.integers(0, 40, (n, ncat)).astype(np.uint32)
    for i in np.flatnonzero(kind == 4):  # counts[first] < counts[second] (first / second: the two largest unique counts)
        o = np.argsort(uq[i], kind="stable")
        counts[i, o[-1]] = uq[i, o[-1]]
        counts[i, o[-2]] = uq[i, o[-1]] + 1 + r.integers(0, 5)
    mq = r.choice(np.float32([thr["min_q"], np.nan, 40.0, thr["min_q"] - 1, np.nextafter(np.float32(thr["min_q"]), 0)]), n)
    length = r.choice(np.array([thr["min_len"], 0, 5000, thr["min_len"] - 1], np.uint32), n)
    comp = r.choice(np.float32([thr["min_comp"], np.nan, 0.5, thr["min_comp"] - 0.01]), n)
    return nh, counts, uq, length, mq, comp


@pytest.mark.parametrize("paired,ncat", [(False, 2), (True, 2), (True, 3), (True, 8), (True, 64), (True, 255)])
def test_calls_equal_the_reference_on_the_device_probabilities(api, paired, ncat):
    r = util.rng(300 + ncat + paired)
    thr = dict(min_q=15.0, min_len=140, min_comp=0.2)
    n = 3000 if ncat < 64 else 600
    g, st = counts_stream(api, ncat, n)
    settings = [dict(confidence_threshold=c, min_hits=h, min_proportion_difference=pd, min_prob_difference=prd,
                     confidence_probability_threshold=cpt)
                for c, h, pd, prd, cpt in ((7, 0, 0.04, 0.0, 0.0), (-1, 3, 0.0, 0.1, 5.0), (-128, 3, 0.01, 0.0, 0.0),
                                           (0, 0, 0.0, 0.0, 200.0), (127, 0, 0.04, 0.0, 0.0))]
    hosts = [0, 1] if not paired else [0]
    seen_conf255, seen_calls = False, set()
    for host in hosts:
        for s in settings:
            m = api.default_model(ncat, host, paired=paired, min_quality=thr["min_q"], min_length=thr["min_len"],
                                  min_compression=thr["min_comp"], **s)
            st.set_model(m)
            nh, counts, uq, length, mq, comp = random_rows(r, n, ncat, thr)
            out = st.classify_counts_raw(nh, counts, uq, length, mq, comp)
            up = pyref.unique_props(uq, nh[:, None])
            ct = s["confidence_threshold"]
            for i in range(n):
                if paired:
                    want = pyref.call_category(uq[i], counts[i], out["probs"][i], nh[i], mq[i], int(length[i]), comp[i], conf_thr=ct,
                                               min_q=thr["min_q"], min_len=thr["min_len"], min_comp=thr["min_comp"],
                                               min_pd=s["min_proportion_difference"], min_hits=s["min_hits"])
                else:
                    want = pyref.call_host(uq[i].tolist(), up[i], list(out["probs"][i]), host, mq[i], int(length[i]), comp[i],
                                           conf_thr=ct, min_q=thr["min_q"], min_len=thr["min_len"], min_comp=thr["min_comp"],
                                           min_pd=s["min_proportion_difference"], min_prd=s["min_prob_difference"],
                                           cpt=s["confidence_probability_threshold"])
                assert (int(out["call"][i]), int(out["conf"][i])) == want, (host, s, i, nh[i], uq[i][:8], counts[i][:8])
            seen_conf255 |= bool((out["conf"] == 255).any())
            seen_calls.update(np.unique(out["call"]).tolist())
    assert seen_conf255 and len(seen_calls) >= min(ncat, 3)
    st.destroy()
    g.destroy()


def top_two(uq):
    """call_category's first / second of every row (include/read_entry.hpp:160-168)"""
    first, second = [], []
    for u in uq:
        f, sc = (1, 0) if u[1] > u[0] else (0, 1)
        for i in range(2, len(u)):
            if u[i] > u[sc]:
                sc = i
                if u[sc] > u[f]:
                    f, sc = sc, f
        first.append(f)
        second.append(sc)
    return np.array(first), np.array(second)


# ---- the borderline flag ----------------------------------------------------------------------------------------------------
def f32_steps(v, ks=(-2, -1, 0, 1, 2)):
    base = np.float32(v)
    out = []
    for k in ks:
        w = base
        for _ in range(abs(k)):
            w = np.nextafter(w, np.float32(np.inf if k > 0 else -np.inf))
        out.append(float(w))
    return out


def host_rows(r, n):
    """realistic single-end rows: one category dominant, the other rare"""
    nh = r.integers(60, 400, n).astype(np.uint32)
    hi = (nh * r.uniform(0.1, 0.9, n)).astype(np.uint32)
    lo = (nh * r.uniform(0.0, 0.04, n)).astype(np.uint32)
    sw = r.random(n) < 0.5
    uq = np.stack([np.where(sw, hi, lo), np.where(sw, lo, hi)], axis=1).astype(np.uint32)
    return nh, uq


def test_borderline_flag_contract(api):
    pos, neg = default_tables()
    r = util.rng(77)
    n = 4000
    nh, uq = host_rows(r, n)
    uq[:40] = np.stack([(nh[:40] * r.uniform(0.05, 0.15, 40)).astype(np.uint32), (nh[:40] * 0.01).astype(np.uint32)], 1)
    lengths = np.full(n, 1000, np.uint32)
    mq = np.full(n, 40.0, np.float32)
    comp = np.full(n, 0.5, np.float32)
    x = pyref.unique_props(uq, nh[:, None])
    ref = np.stack([ref_by_distinct_x(x[:, c], lambda xs: pyref.kde_model_prob(xs, pos, neg)) for c in range(2)], 1)
    g, st = counts_stream(api, 2, n)

    def run(**kw):
        m = api.default_model(2, 0, **kw)
        st.set_model(m)
        out = st.classify_counts_raw(nh, uq, uq, lengths, mq, comp)
        want = np.array([pyref.call_host(uq[i].tolist(), x[i], list(ref[i]), 0, 40.0, 1000, 0.5, min_prd=kw.get("min_prob_difference", 0.0),
                                         cpt=kw.get("confidence_probability_threshold", 0.0))[0] for i in range(n)])
        unflagged = out["flags"] == 0
        bad = np.flatnonzero(unflagged & (out["call"] != want))
        assert bad.size == 0, (kw, bad[:5], out["call"][bad[:5]], want[bad[:5]])
        return out
    # a row whose hp - op decides: the host wins on the proportions, min_prob_difference put 0, +-1, +-2 float ulps from hp - op
    hu, ou = x[:, 0].astype(np.float64), x[:, 1].astype(np.float64)
    cand = np.flatnonzero((hu - ou > 0.04) & (ref[:, 0] > ref[:, 1]) & (ref[:, 0] - ref[:, 1] > 1e-3) & (uq[:, 0] - uq[:, 1] >= 7))
    assert cand.size
    row = cand[0]
    for thr in f32_steps(ref[row, 0] - ref[row, 1]):
        out = run(min_prob_difference=thr)
        assert out["flags"][row] == 1, thr
    # max(hp * conf, conf) -- conf, as hp <= 1 -- put next to the confidence probability threshold
    conf = int(uq[row, 0] - uq[row, 1])
    for thr in f32_steps(max(ref[row, 0] * min(conf, 255), min(conf, 255))):
        out = run(confidence_probability_threshold=thr)
        assert out["flags"][row] == 1, thr
    # the random table with the default thresholds: few rows flagged
    out = run()
    assert out["flags"].mean() < 0.01, out["flags"].mean()
    st.destroy()
    g.destroy()
    # call_category: probabilities near 1e-30 and exact zeros (a narrow positive dataset far from the proportions)
    g, st = counts_stream(api, 3, n)
    nh3 = r.integers(60, 400, n).astype(np.uint32)
    uq3 = (nh3[:, None] * r.uniform(0.0, 0.3, (n, 3))).astype(np.uint32)
    far = [np.float32([0.9]), np.float32([0.6]), pos]
    m = kde_model(api, far, [neg] * 3, h_pos=0.05, paired=True, confidence_threshold=-1, min_proportion_difference=0.0)
    st.set_model(m)
    out = st.classify_counts_raw(nh3, uq3, uq3, lengths, mq, comp)
    x3 = pyref.unique_props(uq3, nh3[:, None])
    ref3 = np.stack([ref_by_distinct_x(x3[:, c], lambda xs: pyref.kde_model_prob(xs, far[c], neg, 0.05)) for c in range(3)], 1)
    assert ((ref3 > 0) & (ref3 < 1e-25)).any() and (ref3 == 0).any()
    first, second = top_two(uq3)  # the two categories call_category compares
    rows = np.arange(n)
    tiny = (ref3[rows, first] < 1e-30) | (ref3[rows, second] < 1e-30)
    assert tiny.sum() > 100 and out["flags"][tiny].all()
    for i in np.flatnonzero(out["flags"] == 0):
        want = pyref.call_category(uq3[i], uq3[i], ref3[i], nh3[i], 40.0, 1000, 0.5, conf_thr=-1, min_pd=0.0)
        assert int(out["call"][i]) == want[0], i
    st.destroy()
    g.destroy()


# ---- the memo ---------------------------------------------------------------------------------------------------------------
def test_memo_hits_evictions_and_model_changes(api):
    pos, neg = default_tables()
    n = 500_000
    g, st = counts_stream(api, 8, n)
    st.set_model(kde_model(api, [pos] * 8, [neg] * 8))
    # one (c, uq, nh) in every lane of many wavefronts
    k = 64 * 2000
    same = np.full((k, 8), 17, np.uint32)
    out = raw(st, np.full(k, 101, np.uint32), same, same)
    want = pyref.kde_model_prob(pyref.unique_props([17], [101]), pos, neg)[0]
    assert (out["probs"] == out["probs"][0, 0]).all()
    assert ulps(out["probs"][:1, :1], np.full((1, 1), want))[0].max() <= 2
    # distinct keys (c, nh, uq) beyond the table's 2^21 slots; x = j / 16 exactly, so the reference is cheap
    i = np.arange(n)
    mm = (1 + i // 17).astype(np.uint32)
    j = (i[:, None] + 3 * np.arange(8)[None, :]) % 17
    nh = 16 * mm
    U = (j * mm[:, None]).astype(np.uint32)
    nh[-6:] = H28 + np.arange(6)  # beyond the memo's key range
    U[-6:] = (nh[-6:, None] // 16 * j[-6:]).astype(np.uint32)
    x = pyref.unique_props(U, nh[:, None])
    ref = ref_by_distinct_x(x, lambda xs: pyref.kde_model_prob(xs, pos, neg))
    a = raw(st, nh, U, U)
    b = raw(st, nh, U, U)
    assert np.array_equal(a["probs"].view(np.uint64), b["probs"].view(np.uint64))
    assert np.array_equal(a["probs"], ref)
    # another model and back, same counts: no stale entry survives set_model
    other = kde_model(api, [pos[::3]] * 8, [neg[::2]] * 8, h_pos=0.05, h_neg=0.01)
    small = slice(0, 20000)
    ref_o = ref_by_distinct_x(x[small], lambda xs: pyref.kde_model_prob(xs, pos[::3], neg[::2], 0.05, 0.01))
    for model, want in ((other, ref_o), (kde_model(api, [pos] * 8, [neg] * 8), ref[small]), (other, ref_o)):
        st.set_model(model)
        got = raw(st, nh[small], U[small], U[small])
        d, _ = ulps(got["probs"], want)
        assert d.max() <= 2
        assert (got["probs"] == want).mean() >= 0.999
    st.destroy()
    g.destroy()


# ---- chn_classify_counts (the fixed-up path) --------------------------------------------------------------------------------
def test_classify_counts_fixed_up_equals_the_reference(api):
    pos, neg = default_tables()
    r = util.rng(88)
    n = 5000
    nh, uq = host_rows(r, n)
    nh[:50] = 0
    uq[:25] = 0
    uq[10:20, 0] = 3
    uq[200:300, 1] = uq[200:300, 0]  # ties: hp == op, flagged
    g, st = counts_stream(api, 2, n)
    st.set_model(api.default_model(2, 0, confidence_threshold=0))
    lengths = np.full(n, 1000, np.uint32)
    mq = np.full(n, 40.0, np.float32)
    comp = np.full(n, 0.5, np.float32)
    rw = st.classify_counts_raw(nh, uq, uq, lengths, mq, comp)
    out = st.classify_counts(nh, uq, uq, lengths, mq, comp)
    x = pyref.unique_props(uq, nh[:, None])
    ref = np.stack([ref_by_distinct_x(x[:, c], lambda xs: pyref.kde_model_prob(xs, pos, neg)) for c in range(2)], 1)
    d, same = ulps(out["probs"], ref)
    assert d.max() <= 2
    fixed = (rw["flags"] == 1) | (nh == 0)
    assert fixed.sum() >= 100
    assert np.array_equal(out["probs"][fixed], ref[fixed], equal_nan=True)
    for i in range(n):
        want = pyref.call_host(uq[i].tolist(), x[i], list(ref[i]), 0, 40.0, 1000, 0.5, conf_thr=0)
        assert (int(out["call"][i]), int(out["conf"][i])) == want, i
    st.destroy()
    g.destroy()


# ---- slot 0 -----------------------------------------------------------------------------------------------------------------
def test_counts_only_calls_leave_device_resident_results_alone(api, oracle_lib):
    """chn_batch_wait with on_device results hands out the slot's buffers (valid until the third-next submit); a counts-only
    call in between must not write them -- it used to stage everything in slot 0's buffers"""
    from charon_amd import pack
    r = util.rng(99)
    gs = [util.random_seq(r, 8000), util.random_seq(r, 8000)]
    oidx = util.build_oracle_index(oracle_lib, [[x] for x in gs], [0, 1], ["host", "microbial"])
    gidx = util.gpu_index_from_oracle(api, oidx)
    batches = [util.sample_reads(r, gs, 300, (200, 900)) for _ in range(3)]
    packed = [pack.pack_reads(b) for b in batches]
    st = api.Stream(gidx, 300, max(p["n_bases"] for p in packed))
    st.set_model(api.default_model(2, 0))
    for p in packed:
        st.submit_host(p, np.full(300, 40.0, np.float32), np.zeros(300, np.float32))
    res = [st.wait_device() for _ in range(3)]
    before = [util.download_results(api, x, 300, 2) for x in res]
    nh = r.integers(1, 300, 300).astype(np.uint32)
    U = (nh[:, None] * r.random((300, 2))).astype(np.uint32)
    args = (nh, U + 1, U, np.full(300, 500, np.uint32), np.full(300, 30.0, np.float32), np.zeros(300, np.float32))
    st.classify_counts(*args)
    st.classify_counts_raw(*args)
    after = [util.download_results(api, x, 300, 2) for x in res]
    for b, a in zip(before, after):
        for key in b:
            assert a[key].tobytes() == b[key].tobytes(), key
    st.destroy()
    gidx.destroy()
    oidx.free()
