"""Weighted quantiles and histograms on the device (gjx_weighted_quantiles, gjx_weighted_histogram) against the restatement of the
definition in tests/test_quantiles_cpu.py (``ref_quantile``, ``ref_hist``: NumPy with exact integers) on the same float32 inputs:
the kernels on raw tensors, then the host surface (ParticleCollection / TrialCollections .quantile, .median, .credible_interval,
.histogram, .probabilities and ScanBootstrapFilter.posterior_quantiles).

Exact cases (equal weights, and log-weights in {0, -inf}: the weights are the integers 2^32 and 0 on both sides) are compared
bitwise.  General weights are bracketed in float64 true weights e64 = exp(float64(logw) - max):
    F_<(v) <= q + delta  and  F_<=(v) >= q - delta,   delta = K 2^-32 / sum e64 + 1e-5
(the first term: the quantisation of u in numerator and denominator, 2 x K 2^-33; the second: 3 x the float32 error of the hardware
exponential of (w - M) log2 e for |w - M| <= 23, about 3e-6), and a histogram's mass by |mass - ref| <= delta per entry.
Worst slack / delta over the general-weight cases on an MI355X: see DESIGN.md section 5."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import genjax_amd as genjax
from genjax_amd import C
from genjax_amd import _abi as A
from test_quantiles_cpu import ref_hist, ref_quantile

DYADIC = [0.0, 0.125, 0.25, 0.5, 0.75, 1.0]
LEVELS = [0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0]
KS = [1, 2, 63, 1024, 1025, 16 * 1024 + 5, 1 << 17, (1 << 17) + 1029]      # (the last: more than 128 tiles, two tiles per block)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _bits_equal(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _wq(rows, logw=None, q=(0.5,), n_segments=1, ws=None):
    from genjax_amd import kernels
    return kernels.weighted_quantiles(rows, logw, q, n_segments, ws)


def _wh(rows, logw=None, bins=64, span=(-3.0, 3.0), n_segments=1, ws=None):
    from genjax_amd import kernels
    return kernels.weighted_histogram(rows, logw, bins, span, n_segments, ws)


def _e64(logw, K):
    """float64 true weights exp(logw - max), 0 for a dead particle"""
    if logw is None:
        return np.ones(K)
    w = np.asarray(logw, np.float64)
    live = ~np.isnan(w) & (w > -np.inf)
    return np.where(live, np.exp(np.where(live, w, 0.0) - w[live].max()), 0.0)


def _check_stats(st, logw, K):
    e = _e64(logw, K)
    ref = np.array([0.0 if logw is None else np.nanmax(np.where(np.isnan(logw), -np.inf, logw)), e.sum(), (e * e).sum(), e.sum() ** 2 / (e * e).sum()])
    assert st[0] == np.float32(ref[0])
    np.testing.assert_allclose(st[1:].astype(np.float64), ref[1:], rtol=1e-4)


# ---- exact cases ----
def _exact_rows(rs, K, dead):
    """the nine kinds of row of the exact cases; ``dead``: the particles that the {0, -inf} weights remove"""
    n = rs.standard_normal(K).astype(np.float32)
    low4 = (np.float32(1.0).view(np.uint32) | rs.integers(0, 16, K).astype(np.uint32)).view(np.float32)
    signexp = ((rs.integers(0, 2, K).astype(np.uint32) << 31) | (rs.integers(1, 255, K).astype(np.uint32) << 23)).view(np.float32)
    pool = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3e-39, -3e-39, 1.1754944e-38, 1.0, -1.0, 2.5, -1e30, 1e30], np.float32)
    mix = pool[rs.integers(0, pool.size, K)]
    nan_live = n.copy()
    nan_live[rs.random(K) < 0.1] = np.nan
    on_dead = rs.standard_normal(K).astype(np.float32)
    on_dead[dead] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), int(dead.sum()))
    return np.stack([n, np.full(K, 3.25, np.float32), (rs.random(K) < 0.3).astype(np.float32), rs.integers(0, 5, K).astype(np.float32), low4,
                     signexp, mix, nan_live, on_dead])


_exact: dict = {}


def _exact_case(K):
    """(rows, logw in {0, -inf}) on the host and on the device, made once per K and never written to"""
    if K not in _exact:
        rs = np.random.default_rng(500 + K)
        dead = rs.random(K) < 0.4
        dead[rs.integers(0, K)] = False
        logw = np.where(dead, -np.inf, 0.0).astype(np.float32)
        rows = _exact_rows(rs, K, dead)
        _exact[K] = (rows, logw, _dev(rows), _dev(logw))
    return _exact[K]


@pytest.mark.parametrize("weights", ["equal", "zero_or_dead"])
@pytest.mark.parametrize("K", KS)
def test_exact_cases_are_bitwise_the_definition(K, weights):
    rows, logw, drows, dlogw = _exact_case(K)
    lw, dlw = (None, None) if weights == "equal" else (logw, dlogw)
    got = _wq(drows, dlw, DYADIC)
    assert got["q"].shape == (rows.shape[0], len(DYADIC)) and got["stats"].shape == (4,)
    h = _np(got["q"])
    for r in range(rows.shape[0]):
        ref = ref_quantile(rows[r], lw, DYADIC)
        assert (_bits(h[r]) == _bits(ref)).all(), (K, weights, r, h[r], ref)
    n_live = K if lw is None else int((logw == 0).sum())
    np.testing.assert_array_equal(_np(got["stats"]), np.array([0, n_live, n_live, n_live], np.float32))
    one = _wq(drows[2], dlw, 0.5)                          # a 1-d row, a scalar level
    assert one["q"].shape == (1, 1) and _bits_equal(one["q"][0], got["q"][2, 3:4])


# ---- general weights ----
def _general_weights(rs, K, kind):
    logw = (10.0 * rs.standard_normal(K)).astype(np.float32)
    if kind == "dominant":
        logw[rs.integers(0, K)] = logw.max() + 30.0
    elif kind == "half_dead":
        logw[rs.permutation(K)[:K // 2]] = -np.inf
        logw[rs.permutation(K)[:K // 16]] = np.nan
    return logw


def _bracket(x, logw, levels, got, K, what):
    """-> worst slack / delta; asserts the live-value property and the bracket"""
    e = _e64(logw, K)
    W = e.sum()
    delta = K * 2.0 ** -32 / W + 1e-5
    live = e > 0 if logw is not None else np.ones(K, bool)
    live_bits = set(_bits(x[live]).tolist())
    xs = x.astype(np.float64)
    worst = 0.0
    for q, v in zip(levels, got):
        assert int(_bits(v)[0]) in live_bits, (what, q, v)
        below, upto = e[xs < float(v)].sum() / W, e[xs <= float(v)].sum() / W
        slack = max(below - q, q - upto, 0.0)
        worst = max(worst, slack / delta)
        assert below <= q + delta and upto >= q - delta, (what, q, v, below, upto, delta)
    return worst


@pytest.mark.parametrize("kind", ["spread", "dominant", "half_dead"])
@pytest.mark.parametrize("K", [1025, 16 * 1024 + 5])
def test_general_weights_are_bracketed(K, kind):
    rs = np.random.default_rng(K + len(kind))
    logw = _general_weights(rs, K, kind)
    rows = np.stack([rs.standard_normal(K), (rs.random(K) < 0.3), rs.integers(0, 5, K), 1000.0 + 0.01 * rs.standard_normal(K)]).astype(np.float32)
    rows[0, ~np.isfinite(logw)] = np.nan                   # values of dead particles must not matter
    got = _wq(_dev(rows), _dev(logw), LEVELS)
    h = _np(got["q"])
    worst = max(_bracket(rows[r], logw, LEVELS, h[r], K, f"K={K} {kind} row {r}") for r in range(rows.shape[0]))
    print(f"[quantiles] K={K} {kind}: worst slack/delta {worst:.3g}")
    _check_stats(_np(got["stats"]), logw, K)


@pytest.mark.parametrize("K", [63, 1500])
def test_without_weight_there_is_no_estimate(K):
    rs = np.random.default_rng(K)
    rows = _dev(rs.standard_normal((3, K)).astype(np.float32))
    dead = np.full(K, -np.inf, np.float32)
    mixed = dead.copy()
    mixed[::3] = np.nan
    overflow = rs.standard_normal(K).astype(np.float32)
    overflow[K // 2] = np.inf                              # exp(w - inf) = 0 everywhere else, NaN there: u = 0 everywhere
    for lw in (dead, np.full(K, np.nan, np.float32), mixed, overflow):
        got = _wq(rows, _dev(lw), [0.0, 0.5, 1.0])
        np.testing.assert_array_equal(_np(got["stats"]), np.array([-np.inf, 0, 0, 0], np.float32))
        assert np.isnan(_np(got["q"])).all()
        hist = _wh(rows, _dev(lw), 8)
        np.testing.assert_array_equal(_np(hist["stats"]), np.array([-np.inf, 0, 0, 0], np.float32))
        assert np.isnan(_np(hist["mass"])).all() and hist["mass"].shape == (3, 10)


# ---- levels ----
def test_levels_one_to_the_cap_any_order():
    import torch
    from genjax_amd._lib import load
    K, cap = 1500, A.QUANTILES_MAX_LEVELS
    rs = np.random.default_rng(3)
    logw = _general_weights(rs, K, "spread")
    rows = np.stack([rs.standard_normal(K), rs.integers(0, 3, K)]).astype(np.float32)
    drows, dlogw = _dev(rows), _dev(logw)
    levels = [0.5, 0.01, 1.0, 0.5, 0.99, 0.0, 0.25, 0.25, 0.75, 0.3, 0.5000001, 0.1, 0.9, 0.6, 0.4, 0.5][:cap]
    assert len(levels) == cap and levels != sorted(levels)
    full = _wq(drows, dlogw, levels)
    assert full["q"].shape == (2, cap)
    single = {q: _wq(drows, dlogw, [q]) for q in set(levels)}
    for j, q in enumerate(levels):                         # a level's result does not depend on the other levels
        assert single[q]["q"].shape == (2, 1) and _bits_equal(full["q"][:, j], single[q]["q"][:, 0]), (j, q)
        assert _bits_equal(full["stats"], single[q]["stats"])
    assert _bits_equal(_wq(drows, dlogw, levels[:5])["q"], full["q"][:, :5])
    with pytest.raises(ValueError, match=str(cap)):
        _wq(drows, dlogw, levels + [0.5])
    # the library itself refuses, before any launch: the outputs keep their contents
    stats, out = torch.full((4,), 7.0, device="cuda"), torch.full((2, cap + 1), 7.0, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lv = (ctypes.c_float * (cap + 1))(*(levels + [0.5]))
    rc = load().gjx_weighted_quantiles(p(drows), K, 2, p(dlogw), K, 1, lv, cap + 1, p(stats), p(out), p(ws), ws.numel(), None)
    assert rc == A.EUNSUPPORTED and str(cap) in load().gjx_last_error().decode()
    torch.cuda.synchronize()
    assert float(stats.min()) == 7.0 and float(out.min()) == 7.0


# ---- rows ----
@pytest.mark.parametrize("n_rows", [1, 9, 17])
def test_any_number_of_rows(n_rows):
    K = 1500
    rs = np.random.default_rng(n_rows)
    logw = np.where(rs.random(K) < 0.3, -np.inf, 0.0).astype(np.float32)
    rows = (rs.standard_normal((n_rows, K)) * (1.0 + np.arange(n_rows))[:, None]).astype(np.float32)
    rows[1::2] = np.floor(rows[1::2])                      # every other row with ties
    drows, dlogw = _dev(rows), _dev(logw)
    got = _wq(drows, dlogw, DYADIC)
    assert got["q"].shape == (n_rows, len(DYADIC))
    h = _np(got["q"])
    for r in range(n_rows):
        assert (_bits(h[r]) == _bits(ref_quantile(rows[r], logw, DYADIC))).all(), r
    hist = _wh(drows, dlogw, 16, (-4.0, 4.0))
    assert hist["mass"].shape == (n_rows, 18) and hist["edges"].shape == (17,)
    hm = _np(hist["mass"])
    for r in range(n_rows):
        assert (_bits(hm[r]) == _bits(ref_hist(rows[r], logw, -4.0, 4.0, 16)[2])).all(), r


@pytest.mark.parametrize("K", [1025, 1500])
def test_strided_and_unaligned_views(K):
    """a slice of a wider matrix (row_stride > K), and a view that starts at column 1: its rows are not 16-byte aligned: the scalar load
    path.  Same values: bitwise the contiguous call."""
    import torch
    rs = np.random.default_rng(K)
    logw = _general_weights(rs, K, "half_dead")
    rows = rs.standard_normal((4, K)).astype(np.float32)
    rows[3] = np.round(rows[3])
    drows, dlogw = _dev(rows), _dev(logw)
    wide = torch.full((4, K + 9), float("nan"), device="cuda")
    wide[:, :K] = drows
    wide1 = torch.full((4, K + 9), float("nan"), device="cuda")
    wide1[:, 1:K + 1] = drows
    lw1 = torch.full((K + 3,), float("nan"), device="cuda")
    lw1[1:K + 1] = dlogw
    base, hbase = _wq(drows, dlogw, LEVELS), _wh(drows, dlogw, 32)
    for view, lw in ((wide[:, :K], dlogw), (wide1[:, 1:K + 1], dlogw), (wide1[:, 1:K + 1], lw1[1:K + 1])):
        assert not view.is_contiguous() and view.stride() == (K + 9, 1)
        got, hgot = _wq(view, lw, LEVELS), _wh(view, lw, 32)
        assert _bits_equal(got["q"], base["q"]) and _bits_equal(got["stats"], base["stats"])
        assert _bits_equal(hgot["mass"], hbase["mass"]) and _bits_equal(hgot["stats"], hbase["stats"])


# ---- segments ----
@pytest.mark.parametrize("S,K_seg", [(50, 50), (4, 1024)])
def test_segments_are_normalised_on_their_own(S, K_seg):
    """K = 2500 with 50 segments (boundaries inside tiles) and K = 4096 with 4: every segment's outputs are bitwise those of a call on
    its slice alone"""
    K = S * K_seg
    rs = np.random.default_rng(S)
    logw = (3.0 * rs.standard_normal(K)).astype(np.float32) + np.repeat(rs.standard_normal(S) * 30.0, K_seg).astype(np.float32)
    rows = np.stack([rs.standard_normal(K), rs.integers(0, 4, K), rs.random(K) < 0.5]).astype(np.float32)
    logw[K_seg + 3] = -np.inf
    rows[:, K_seg + 3] = np.nan
    logw[2 * K_seg:3 * K_seg] = -np.inf                    # a whole segment without weight
    drows, dlogw = _dev(rows), _dev(logw)
    got = _wq(drows, dlogw, LEVELS, n_segments=S)
    hist = _wh(drows, dlogw, 8, (-2.0, 4.0), n_segments=S)
    assert got["stats"].shape == (S, 4) and got["q"].shape == (S, 3, len(LEVELS)) and hist["mass"].shape == (S, 3, 10)
    for s in range(S):
        a, b = s * K_seg, (s + 1) * K_seg
        alone, halone = _wq(drows[:, a:b], dlogw[a:b], LEVELS), _wh(drows[:, a:b], dlogw[a:b], 8, (-2.0, 4.0))
        assert _bits_equal(got["q"][s], alone["q"]) and _bits_equal(got["stats"][s], alone["stats"]), s
        assert _bits_equal(hist["mass"][s], halone["mass"]) and _bits_equal(hist["stats"][s], halone["stats"]), s
    assert np.isnan(_np(got["q"][2])).all() and np.isnan(_np(hist["mass"][2])).all()
    h = _np(got["q"])
    worst = 0.0
    for s in (0, 1, S - 1):
        a, b = s * K_seg, (s + 1) * K_seg
        for r in range(3):
            worst = max(worst, _bracket(rows[r, a:b], logw[a:b], LEVELS, h[s, r], K_seg, f"segment {s} row {r}"))
    print(f"[quantiles] {S} segments of {K_seg}: worst slack/delta {worst:.3g}")
    with pytest.raises(ValueError, match="segments"):
        _wq(drows, dlogw, LEVELS, n_segments=7)


# ---- reproducibility ----
@pytest.mark.parametrize("shape", ["ties", "continuous"])
def test_bit_reproducible(shape):
    import torch
    from genjax_amd._lib import load
    K = 1 << 14
    rs = np.random.default_rng(11)
    logw = _dev(_general_weights(rs, K, "spread"))
    x = rs.random((3, K)) < 0.5 if shape == "ties" else rs.standard_normal((3, K))
    rows = _dev(x.astype(np.float32))
    first, hfirst = _wq(rows, logw, LEVELS), _wh(rows, logw, 64)
    for _ in range(2):
        again, hagain = _wq(rows, logw, LEVELS), _wh(rows, logw, 64)
        assert all(_bits_equal(again[k], first[k]) for k in first) and all(_bits_equal(hagain[k], hfirst[k]) for k in hfirst)
    need = load().gjx_weighted_quantiles_workspace_bytes(3, K, 1, len(LEVELS))
    big = torch.full((2 * need + 4096,), 255, dtype=torch.uint8, device="cuda")          # larger, and dirty: the call zeroes what it needs
    dirty = _wq(rows, logw, LEVELS, ws=big[1:])                                             # (and not 8-byte aligned)
    assert all(_bits_equal(dirty[k], first[k]) for k in first)
    hdirty = _wh(rows, logw, 64, ws=big)
    assert all(_bits_equal(hdirty[k], hfirst[k]) for k in hfirst)


# ---- histogram ----
def _hist_row(rs, K):
    x = (1.5 * rs.standard_normal(K)).astype(np.float32)
    x[:8] = np.array([-3.0, 3.0, np.nan, np.inf, -np.inf, -0.0, np.nextafter(np.float32(3.0), np.float32(0.0)), -3.0000002], np.float32)[:min(8, K)]
    return x


@pytest.mark.parametrize("n_bins", [1, 2, 64, 4096])
def test_histogram_entries(n_bins):
    K = 16 * 1024 + 5
    rs = np.random.default_rng(n_bins)
    rows = np.stack([_hist_row(rs, K), rs.integers(-4, 5, K).astype(np.float32)])
    drows = _dev(rows)
    tol_sum = (n_bins + 2) * 2.0 ** -24
    # equal weights, and weights in {0, -inf}: exact
    zero_dead = np.where(rs.random(K) < 0.3, -np.inf, 0.0).astype(np.float32)
    for lw in (None, zero_dead):
        got = _wh(drows, None if lw is None else _dev(lw), n_bins, (-3.0, 3.0))
        assert got["mass"].shape == (2, n_bins + 2) and got["edges"].shape == (n_bins + 1,)
        m = _np(got["mass"])
        for r in range(2):
            counts, U, ref = ref_hist(rows[r], lw, -3.0, 3.0, n_bins)
            assert (_bits(m[r]) == _bits(ref)).all(), (n_bins, r)
            assert counts[0] > 0 and counts[n_bins + 1] > 0                            # under; over and NaN
            assert abs(m[r].astype(np.float64).sum() - 1.0) <= tol_sum
    e = _np(got["edges"])
    assert e[0] == -3.0 and e[-1] == 3.0 and (np.diff(e) > 0).all()
    # general weights
    logw = _general_weights(rs, K, "half_dead")
    got = _wh(drows, _dev(logw), n_bins, (-3.0, 3.0))
    m = _np(got["mass"]).astype(np.float64)
    delta = K * 2.0 ** -32 / _e64(logw, K).sum() + 1e-5
    worst = 0.0
    for r in range(2):
        ref = ref_hist(rows[r], logw, -3.0, 3.0, n_bins)[2].astype(np.float64)
        worst = max(worst, np.abs(m[r] - ref).max() / delta)
        assert (np.abs(m[r] - ref) <= delta).all(), (n_bins, r)
        assert abs(m[r].sum() - 1.0) <= tol_sum
    print(f"[histogram] n_bins={n_bins}: worst |mass - ref|/delta {worst:.3g}")
    _check_stats(_np(got["stats"]), logw, K)
    if n_bins == 64:
        with pytest.raises(ValueError, match=str(A.HISTOGRAM_MAX_BINS)):
            _wh(drows, None, A.HISTOGRAM_MAX_BINS + 1, (-3.0, 3.0))


# ---- the host surface ----
def _beta_bernoulli():
    @genjax.gen
    def model():
        p = genjax.beta(2.0, 2.0) @ "p"
        v = genjax.flip(p) @ "v"
        return v
    return model


def _beta32_cdf(x):
    return 4.0 * x ** 3 - 3.0 * x ** 4


def test_readme_beta_bernoulli_median_and_interval():
    """README: p ~ Beta(2, 2), v ~ flip(p) observed True: the posterior is Beta(3, 2), F(x) = 4 x^3 - 3 x^4.  A weighted sample quantile
    v of level q has F(v) within the binomial spread at the measured ESS: |F(v) - q| <= 5 sqrt(q (1 - q) / ESS)."""
    from genjax_amd.inference import ImportanceK, Target
    K = 1 << 16
    pc = ImportanceK(Target(_beta_bernoulli(), (), C["v"].set(True)), k_particles=K).run_smc(genjax.key(314159))
    ess = float(pc.effective_sample_size())
    assert 0.5 * K < ess <= K
    med, ci = pc.median("p"), pc.credible_interval("p", 0.9)
    assert med.shape == () and ci.shape == (2,) and med.is_cuda
    for v, q in ((float(med), 0.5), (float(ci[0]), 0.05), (float(ci[1]), 0.95)):
        assert abs(_beta32_cdf(v) - q) <= 5.0 * np.sqrt(q * (1.0 - q) / ess), (q, v)
        try:
            from scipy import stats
        except ImportError:
            continue
        assert abs(stats.beta(3, 2).cdf(v) - q) <= 5.0 * np.sqrt(q * (1.0 - q) / ess), (q, v)
    assert _bits_equal(pc.quantile("p", [0.05, 0.5, 0.95]), pc.quantile("p", (0.05, 0.5, 0.95)))
    assert _bits_equal(pc.quantile("p", [0.5])[0], med) and pc.quantile("p", [0.5]).shape == (1,)
    tr = pc.get_particles()
    x, lw = _np(tr.choices[tr.prog.slot_of["p"]]), _np(pc.get_log_weights())
    _bracket(x, lw, [0.05, 0.5, 0.95], _np(pc.quantile("p", [0.05, 0.5, 0.95])), K, "beta-bernoulli")
    # the constrained site reports its value; its probabilities are all on it
    assert float(pc.median("v")) == 1.0 and _np(pc.credible_interval("v")).tolist() == [1.0, 1.0]
    assert _np(pc.probabilities("v")).tolist() == [0.0, 1.0]
    mass, edges = pc.histogram("p", 10, (0.0, 1.0))
    assert mass.shape == (12,) and edges.shape == (11,)
    m = _np(mass).astype(np.float64)
    assert m[0] == 0.0 and m[11] == 0.0 and abs(m.sum() - 1.0) <= 12 * 2.0 ** -24
    cdf = _beta32_cdf(np.linspace(0.0, 1.0, 11))
    assert (np.abs(m[1:11] - np.diff(cdf)) <= 5.0 * np.sqrt(0.25 / ess)).all()
    with pytest.raises(ValueError, match="neither a flip nor a categorical"):
        pc.probabilities("p")
    with pytest.raises(KeyError):
        pc.median("q")


def test_probabilities_of_a_flip_are_its_mean():
    from genjax_amd.inference import ImportanceK, Target

    @genjax.gen
    def model():
        p = genjax.beta(2.0, 2.0) @ "p"
        v = genjax.flip(p) @ "v"
        w = genjax.flip(p) @ "w"
        return v

    pc = ImportanceK(Target(model, (), C["w"].set(True)), k_particles=1 << 14).run_smc(genjax.key(7))
    pr = pc.probabilities("v")
    assert pr.shape == (2,)
    p1 = float(pc.mean("v"))
    assert 0.4 < p1 < 0.8                                  # (E[p | w] = 0.6)
    assert abs(float(pr[1]) - p1) <= 1e-5 and abs(float(pr[0]) - (1.0 - p1)) <= 1e-5
    assert float(pc.median("v")) == 1.0 and float(pc.quantile("v", 0.25)) == 0.0


def test_trials_have_a_leading_axis():
    from genjax_amd.inference import ImportanceK, Target

    @genjax.gen
    def model():
        p = genjax.beta(2.0, 2.0) @ "p"
        v = genjax.flip(p) @ "v"
        w = genjax.flip(p) @ "w"
        return v

    n, K = 50, 50
    tc = ImportanceK(Target(model, (), C["w"].set(True)), k_particles=K).run_smc_trials(genjax.key(314159), n)
    q3, q1, pr = tc.quantile("p", [0.1, 0.5, 0.9]), tc.quantile("p", 0.5), tc.probabilities("v")
    assert q3.shape == (n, 3) and q1.shape == (n,) and pr.shape == (n, 2) and tc.quantile("w", 0.5).shape == (n,)
    assert _bits_equal(q3[:, 1], q1) and (_np(tc.quantile("w", 0.5)) == 1.0).all()
    for t in range(n):
        pc = tc.trial(t)
        assert _bits_equal(q3[t], pc.quantile("p", [0.1, 0.5, 0.9])), t
        assert _bits_equal(pr[t], pc.probabilities("v")), t


DX = 2


def _lgssm_scan(T):
    """a 2-d linear-Gaussian state space as @gen + .scan (x_0 ~ N(0, q))"""
    from genjax_amd import workloads
    s = workloads.ssm_problem(dx=DX, T=12)
    Am = np.asarray(s["A"], np.float32)
    q, r = float(s["q"]), float(s["r"])

    @genjax.gen
    def step(x_prev, _):
        x = genjax.mv_normal_diag(Am @ x_prev, np.full(DX, q, np.float32)) @ "x"
        genjax.mv_normal_diag(x, np.full(DX, r, np.float32)) @ "y"
        return x, None

    return step.scan(n=T), np.zeros(DX, np.float32), np.asarray(s["y"], np.float32)[:T]


def test_filter_posterior_quantiles():
    from genjax_amd import kernels
    from genjax_amd.inference import BootstrapFilter
    K = 1 << 14
    scan, carry0, ys = _lgssm_scan(3)
    bf = BootstrapFilter(scan, K)
    out = bf.run(genjax.key(9), C["y"].set(ys), (carry0, None))
    x, lw = bf.latent(out, "x"), out["logw"]
    levels = [0.05, 0.5, 0.95]
    pq = bf.posterior_quantiles(out, "x", levels)
    assert pq.shape == (DX, 3) and _bits_equal(pq, kernels.weighted_quantiles(x, lw, levels)["q"])
    assert _bits_equal(bf.posterior_quantiles(out, "x", 0.5), pq[:, 1])
    hx, hw = _np(x), _np(lw)
    for d in range(DX):
        _bracket(hx[d], hw, levels, _np(pq[d]), K, f"filter x[{d}]")
    with pytest.raises(KeyError):
        bf.posterior_quantiles(out, "nope", 0.5)


def test_stacked_scan_name():
    """ImportanceK over scan(n=4): "x" names the stacked sequence (what Trace.get_choices stacks), ("x", t) one step"""
    from genjax_amd.inference import ImportanceK, Target
    T, K = 4, 1500
    scan, carry0, ys = _lgssm_scan(T)
    pc = ImportanceK(Target(scan, (carry0, None), C["y"].set(ys)), k_particles=K).run_smc(genjax.key(5))
    q = pc.quantile("x", [0.25, 0.75])
    med = pc.median("x")
    assert q.shape == (T, DX, 2) and med.shape == (T, DX)
    tr, lw = pc.get_particles(), _np(pc.get_log_weights())
    for t in range(T):
        assert _bits_equal(q[t], pc.quantile(("x", t), [0.25, 0.75])) and _bits_equal(med[t], pc.median(("x", t)))
        slot = tr.prog.slot_of[("x", t)]
        for d in range(DX):
            _bracket(_np(tr.choices[slot + d]), lw, [0.25, 0.75], _np(q[t, d]), K, f"scan step {t} x[{d}]")
    mass, edges = pc.histogram("x", 8, (-4.0, 4.0))
    assert mass.shape == (T, DX, 10) and edges.shape == (9,)
