"""Weighted posterior moments on the device (gjx_weighted_moments) against float64 NumPy on the same float32 inputs: the kernel on
raw tensors (sizes around a wave, a tile and several tiles; strided and unaligned views; dead particles; segments; covariance;
bit-reproducibility), then the host surface: ParticleCollection / TrialCollections .moments(), .mean, .variance, .covariance and
ScanBootstrapFilter.posterior_moments.

Tolerances (eps = 1e-4 is the project's figure for float32 sums of fast_exp weights against float64,
tests/test_gpu_adaptive_filter.py; range_r = max - min of row r over the live particles):
    |mean_r - mean64_r|    <= eps range_r + 2^-22 |mean64_r|
    |second_rs - ref_rs|   <= eps range_r range_s + (2^-20)^2 |mean64_r mean64_s|
    stats within rel 1e-4 of float64, stats[0] (the maximum) exact."""
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

EPS = 1e-4
KS = [1, 63, 1025, 1500, 1 << 14]


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _bits_equal(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same(a: dict, b: dict):
    assert a.keys() == b.keys()
    for k in a:
        assert _bits_equal(a[k], b[k]), k


class Ref:
    """float64 moments of float32 rows [n][K] under float32 log-weights (None: equal), dead (-inf / NaN weight) particles removed"""

    def __init__(self, rows, logw=None):
        x = np.asarray(rows, np.float64)
        if logw is None:
            live = np.ones(x.shape[1], bool)
            m, e = 0.0, np.ones(x.shape[1])
        else:
            w = np.asarray(logw, np.float64)
            live = np.isfinite(w)
            m = w[live].max()
            e = np.exp(w[live] - m)
        x = x[:, live]
        W = e.sum()
        self.stats = np.array([m, W, (e * e).sum(), W * W / (e * e).sum()])
        self.mean = (x * e).sum(axis=1) / W
        d = x - self.mean[:, None]
        self.cov = (d * e) @ d.T / W
        self.var = np.diag(self.cov).copy()
        self.range = x.max(axis=1) - x.min(axis=1)
        self.tol_mean = EPS * self.range + 2.0 ** -22 * np.abs(self.mean)
        self.tol_cov = EPS * np.outer(self.range, self.range) + 2.0 ** -40 * np.abs(np.outer(self.mean, self.mean))
        self.tol_var = np.diag(self.tol_cov).copy()


def _check(got: dict, ref: Ref, what=""):
    """got: numpy dict of one segment.  Prints the worst error / tolerance ratios, then asserts."""
    st = got["stats"].astype(np.float64)
    em = np.abs(got["mean"].astype(np.float64) - ref.mean)
    line = f"[moments] {what}: mean err/tol {np.max(em / np.maximum(ref.tol_mean, 1e-300)):.3g}"
    es = None
    if "var" in got:
        es, ts = np.abs(got["var"].astype(np.float64) - ref.var), ref.tol_var
    elif "cov" in got:
        es, ts = np.abs(got["cov"].astype(np.float64) - ref.cov), ref.tol_cov
    if es is not None:
        line += f", second err/tol {np.max(es / np.maximum(ts, 1e-300)):.3g}"
    line += f", stats rel {np.max(np.abs(st[1:] - ref.stats[1:]) / ref.stats[1:]):.3g}"
    print(line)
    assert st[0] == np.float32(ref.stats[0])
    np.testing.assert_allclose(st[1:], ref.stats[1:], rtol=1e-4)
    assert (em <= ref.tol_mean).all(), (what, em, ref.tol_mean)
    if es is not None:
        assert (es <= ts).all(), (what, es, ts)


def _wm(rows, logw=None, want="var", n_segments=1, ws=None):
    from genjax_amd import kernels
    return kernels.weighted_moments(rows, logw, want, n_segments, ws)


def _host(d: dict):
    return {k: _np(v) for k, v in d.items()}


def _weights(rs, K):
    return (2.0 * rs.standard_normal(K) - 37.0).astype(np.float32)


def _four_rows(rs, K, logw):
    """N(0,1); a large offset with a small spread (what an uncentred second moment loses); a row correlated with the weights; a constant"""
    return np.stack([rs.standard_normal(K), 1000.0 + 0.01 * rs.standard_normal(K), 0.5 * logw + 0.3 * rs.standard_normal(K),
                     np.full(K, 3.25)]).astype(np.float32)


_cases: dict = {}


def _case(K):
    """(rows, logw) on the host and on the device, made once per K and never written to"""
    if K not in _cases:
        rs = np.random.default_rng(1000 + K)
        logw = _weights(rs, K)
        rows = _four_rows(rs, K, logw)
        _cases[K] = (rows, logw, _dev(rows), _dev(logw))
    return _cases[K]


@pytest.mark.parametrize("K", KS)
def test_means_and_variances_against_float64(K):
    rows, logw, drows, dlogw = _case(K)
    got = _wm(drows, dlogw)
    assert got["stats"].shape == (4,) and got["mean"].shape == (4,) and got["var"].shape == (4,)
    _check(_host(got), Ref(rows, logw), f"K={K}")
    only = _wm(drows, dlogw, "mean")
    assert set(only) == {"stats", "mean"}
    assert _bits_equal(only["mean"], got["mean"]) and _bits_equal(only["stats"], got["stats"])
    one = _wm(drows[1], dlogw)                         # a 1-d row
    assert _bits_equal(one["mean"], got["mean"][1:2]) and _bits_equal(one["var"], got["var"][1:2])


@pytest.mark.parametrize("n_rows", [1, 3, 17])
def test_any_number_of_rows(n_rows):
    K = 1500
    rs = np.random.default_rng(n_rows)
    logw = _weights(rs, K)
    rows = (rs.standard_normal((n_rows, K)) * (1.0 + np.arange(n_rows))[:, None] + 10.0 * np.arange(n_rows)[:, None]).astype(np.float32)
    got = _wm(_dev(rows), _dev(logw))
    assert got["mean"].shape == (n_rows,) and got["var"].shape == (n_rows,)
    _check(_host(got), Ref(rows, logw), f"n_rows={n_rows}")


@pytest.mark.parametrize("K", [1025, 1500])
def test_strided_and_unaligned_views(K):
    """a slice of a wider matrix (row_stride > K), and a view that starts at column 1: its rows are not 16-byte aligned, and neither are
    the rows of an odd stride: the scalar load path.  Same values, same lanes: bitwise the contiguous call."""
    rows, logw, drows, dlogw = _case(K)
    import torch
    wide = torch.full((4, K + 9), float("nan"), device="cuda")
    wide[:, :K] = drows
    wide1 = torch.full((4, K + 9), float("nan"), device="cuda")
    wide1[:, 1:K + 1] = drows
    lw1 = torch.full((K + 3,), float("nan"), device="cuda")
    lw1[1:K + 1] = dlogw
    base = _wm(drows, dlogw)
    for view, lw in ((wide[:, :K], dlogw), (wide1[:, 1:K + 1], dlogw), (wide1[:, 1:K + 1], lw1[1:K + 1])):
        assert not view.is_contiguous() and view.stride() == (K + 9, 1)
        got = _wm(view, lw)
        _check(_host(got), Ref(rows, logw), f"view K={K}")
        _same(got, base)
        _same(_wm(view[:3], lw, "cov"), _wm(drows[:3].contiguous(), dlogw, "cov"))


@pytest.mark.parametrize("K", KS)
def test_equal_weights(K):
    rows, _, drows, _ = _case(K)
    got = _host(_wm(drows, None))
    x = rows.astype(np.float64)
    ref = Ref(rows, None)
    np.testing.assert_allclose(ref.mean, x.mean(axis=1), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(ref.var, x.var(axis=1), rtol=1e-12, atol=1e-300)
    np.testing.assert_array_equal(got["stats"], np.array([0, K, K, K], np.float32))
    _check(got, ref, f"equal weights K={K}")


def test_dead_particles_contribute_nothing():
    """weights -inf and NaN, with NaN and inf row values there: the results are those of the collection without these particles"""
    K = 1500
    rows, logw, _, _ = _case(K)
    rows, logw = rows.copy(), logw.copy()
    rs = np.random.default_rng(5)
    dead = rs.choice(K, 400, replace=False)
    dead = np.concatenate([dead, np.arange(1024, 1100)])          # a run across the head of the second tile
    logw[dead[::2]] = -np.inf
    logw[dead[1::2]] = np.nan
    rows[:, dead[::3]] = np.nan
    rows[:, dead[1::3]] = np.inf
    rows[:, dead[2::3]] = -np.inf
    got = _host(_wm(_dev(rows), _dev(logw)))
    assert all(np.isfinite(v).all() for v in got.values())
    live = np.isfinite(logw)
    assert live.sum() < K - 400
    ref = Ref(rows[:, live], logw[live])
    _check(got, ref, "dead particles")
    _check(_host(_wm(_dev(rows[:, live]), _dev(logw[live]))), ref, "the same collection, compacted")
    cov = _host(_wm(_dev(rows[:3]), _dev(logw), "cov"))
    assert np.isfinite(cov["cov"]).all()
    _check(cov, Ref(rows[:3, live], logw[live]), "dead particles, cov")


@pytest.mark.parametrize("K,at", [(1, 0), (63, 17), (1500, 1234), (1 << 14, 9000)])
def test_one_live_particle_is_exact(K, at):
    rows, logw, _, _ = _case(K)
    rows = rows.copy()
    lw = np.full(K, -np.inf, np.float32)
    lw[1::2] = np.nan
    lw[at] = logw[at]
    rows[:, np.arange(K) != at] = np.nan
    got = _host(_wm(_dev(rows), _dev(lw)))
    np.testing.assert_array_equal(got["mean"], rows[:, at])
    np.testing.assert_array_equal(got["var"], np.zeros(4, np.float32))
    np.testing.assert_array_equal(got["stats"], np.array([logw[at], 1, 1, 1], np.float32))
    cov = _host(_wm(_dev(rows), _dev(lw), "cov"))
    np.testing.assert_array_equal(cov["mean"], rows[:, at])
    np.testing.assert_array_equal(cov["cov"], np.zeros((4, 4), np.float32))


@pytest.mark.parametrize("K", [63, 1500])
def test_no_live_particle_is_no_estimate(K):
    rows, _, drows, _ = _case(K)
    lw = np.full(K, -np.inf, np.float32)
    lw[::3] = np.nan
    for want in ("var", "cov"):
        got = _host(_wm(drows, _dev(lw), want))
        np.testing.assert_array_equal(got["stats"], np.array([-np.inf, 0, 0, 0], np.float32))
        assert np.isnan(got["mean"]).all() and np.isnan(got[want]).all()


def _correlated(rs, K, dim=3):
    L = np.tril(rs.standard_normal((dim, dim))) + 2.0 * np.eye(dim)
    return (L @ rs.standard_normal((dim, K)) + np.array([5.0, -200.0, 0.01][:dim] + [1.0] * max(dim - 3, 0))[:, None]).astype(np.float32)


@pytest.mark.parametrize("K", [1500, 1 << 14])
def test_covariance(K):
    rs = np.random.default_rng(77 + K)
    logw = _weights(rs, K)
    rows = _correlated(rs, K)
    drows, dlogw = _dev(rows), _dev(logw)
    got = _wm(drows, dlogw, "cov")
    assert got["cov"].shape == (3, 3)
    ref = Ref(rows, logw)
    h = _host(got)
    _check(h, ref, f"cov K={K}")
    np.testing.assert_array_equal(h["cov"], h["cov"].T)                       # exactly symmetric
    var = _host(_wm(drows, dlogw, "var"))
    assert (np.abs(np.diag(h["cov"]).astype(np.float64) - var["var"]) <= ref.tol_var).all()
    assert (np.abs(h["mean"].astype(np.float64) - var["mean"]) <= ref.tol_mean).all()


def test_covariance_row_cap():
    import ctypes
    import torch
    from genjax_amd import kernels
    from genjax_amd._lib import load
    cap, K = A.MOMENTS_MAX_COV_ROWS, 1025
    rs = np.random.default_rng(16)
    logw = _weights(rs, K)
    rows = _correlated(rs, K, cap + 1)
    drows, dlogw = _dev(rows), _dev(logw)
    got = _wm(drows[:cap], dlogw, "cov")
    assert got["cov"].shape == (cap, cap)
    h = _host(got)
    _check(h, Ref(rows[:cap], logw), f"cov of {cap} rows")
    np.testing.assert_array_equal(h["cov"], h["cov"].T)
    with pytest.raises(ValueError, match=str(cap)):
        _wm(drows, dlogw, "cov")
    # the library itself refuses, before any launch: the outputs keep their contents
    stats, mean = torch.full((4,), 7.0, device="cuda"), torch.full((cap + 1,), 7.0, device="cuda")
    second, ws = torch.full((cap + 1, cap + 1), 7.0, device="cuda"), torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = load().gjx_weighted_moments(p(drows), K, cap + 1, p(dlogw), K, 1, A.MOMENTS_COV, p(stats), p(mean), p(second), p(ws), ws.numel(), None)
    assert rc == A.EUNSUPPORTED and str(cap) in load().gjx_last_error().decode()
    torch.cuda.synchronize()
    assert float(stats.min()) == 7.0 and float(mean.min()) == 7.0 and float(second.min()) == 7.0
    assert kernels.weighted_moments(drows, dlogw, "var")["var"].shape == (cap + 1,)      # means and variances take any n_rows


@pytest.mark.parametrize("S,K_seg", [(50, 50), (5, 1500)])
def test_segments_are_normalised_on_their_own(S, K_seg):
    """segment boundaries fall inside tiles of the whole; every segment's outputs are bitwise those of a call on its slice alone"""
    K = S * K_seg
    rs = np.random.default_rng(S)
    logw = _weights(rs, K) + np.repeat(rs.standard_normal(S) * 30.0, K_seg).astype(np.float32)      # very different scales
    rows = _four_rows(rs, K, logw)
    logw[K_seg + 3] = -np.inf
    rows[:, K_seg + 3] = np.nan
    drows, dlogw = _dev(rows), _dev(logw)
    for want in ("var", "cov"):
        got = _wm(drows, dlogw, want, n_segments=S)
        assert got["stats"].shape == (S, 4) and got["mean"].shape == (S, 4) and got[want].shape == ((S, 4) if want == "var" else (S, 4, 4))
        for s in range(S):
            a, b = s * K_seg, (s + 1) * K_seg
            alone = _wm(drows[:, a:b], dlogw[a:b], want)
            for k in got:
                assert _bits_equal(got[k][s], alone[k]), (want, s, k)
        h = _host(got)
        for s in (0, 1, S // 2, S - 1):
            a, b = s * K_seg, (s + 1) * K_seg
            _check({k: v[s] for k, v in h.items()}, Ref(rows[:, a:b], logw[a:b]), f"segment {s} of {S} x {K_seg}, {want}")
    with pytest.raises(ValueError, match="segments"):
        _wm(drows, dlogw, "var", n_segments=S + 1 if K % (S + 1) else 7)


@pytest.mark.parametrize("want", ["var", "cov"])
def test_bit_reproducible(want):
    import torch
    from genjax_amd._lib import load
    K = 1 << 14
    _, _, drows, dlogw = _case(K)
    first = _wm(drows, dlogw, want)
    _same(_wm(drows, dlogw, want), first)
    need = load().gjx_weighted_moments_workspace_bytes(4, K, 1, A.MOMENTS_COV if want == "cov" else A.MOMENTS_VAR)
    big = torch.full((4 * need + 4096,), 255, dtype=torch.uint8, device="cuda")          # larger, and full of NaN bit patterns
    _same(_wm(drows, dlogw, want, ws=big), first)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = _wm(drows, dlogw, want)
    s.synchronize()
    _same(other, first)
    segs = _wm(drows, dlogw, want, n_segments=8)
    _same(_wm(drows, dlogw, want, n_segments=8), segs)


# ---- the host surface ----
def _beta_bernoulli():
    @genjax.gen
    def model():
        p = genjax.beta(2.0, 2.0) @ "p"
        v = genjax.flip(p) @ "v"
        return v
    return model


def test_readme_beta_bernoulli_posterior_mean():
    """README: p ~ Beta(2, 2), v ~ flip(p) observed True: the posterior is Beta(3, 2), mean 0.6, variance 0.04"""
    from genjax_amd.inference import ImportanceK, Moments, Target
    K = 1 << 14
    pc = ImportanceK(Target(_beta_bernoulli(), (), C["v"].set(True)), k_particles=K).run_smc(genjax.key(314159))
    m = pc.moments()
    assert isinstance(m, Moments) and pc.moments() is m
    tr = pc.get_particles()
    slot = tr.prog.slot_of["p"]
    ref = Ref(_np(tr.choices[slot:slot + 1]), _np(pc.get_log_weights()))
    mean, var = pc.mean("p"), pc.variance("p")
    assert mean.shape == () and var.shape == () and mean.is_cuda
    _check(dict(stats=_np(m.stats), mean=_np(mean).reshape(1), var=_np(var).reshape(1)), ref, "beta-bernoulli")
    ess = float(m.ess)
    assert ess == pytest.approx(float(pc.effective_sample_size()), rel=1e-4) and 0.5 * K < ess <= K
    assert abs(float(mean) - 0.6) <= 5.0 * np.sqrt(0.04 / ess)
    assert abs(float(var) - 0.04) <= 0.01
    assert float(pc.mean("v")) == 1.0 and float(pc.variance("v")) == 0.0         # the constrained site
    with pytest.raises(KeyError):
        pc.mean("q")


def test_trials_have_a_leading_axis():
    from genjax_amd.inference import ImportanceK, Target
    n, K = 50, 50
    tc = ImportanceK(Target(_beta_bernoulli(), (), C["v"].set(True)), k_particles=K).run_smc_trials(genjax.key(314159), n)
    m = tc.moments()
    mean, var = m.mean("p"), m.variance("p")
    assert mean.shape == (n,) and var.shape == (n,) and m.ess.shape == (n,) and m.mean("v").shape == (n,)
    tr = tc.particles
    slot = tr.prog.slot_of["p"]
    x, lw = _np(tr.choices[slot]).reshape(n, K), _np(tc.get_log_weights())
    hm, hv, hs = _np(mean), _np(var), _np(m.stats)
    for t in range(n):
        _check(dict(stats=hs[t], mean=hm[t:t + 1], var=hv[t:t + 1]), Ref(x[t:t + 1], lw[t]), f"trial {t}")
    assert (_np(m.mean("v")) == 1.0).all() and (_np(m.variance("v")) == 0.0).all()
    assert abs(float(mean.mean()) - 0.6) <= 3 * 0.2 / np.sqrt(n * 20)


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


@pytest.mark.parametrize("tau", [None, 0.5])
def test_filter_posterior_moments(tau):
    """BootstrapFilter over a Scan: the moments of the last step's particles under out["logw"] (tau = 0.5: the carried weights)"""
    from genjax_amd import kernels
    from genjax_amd.inference import BootstrapFilter
    scan, carry0, ys = _lgssm_scan(3)
    bf = BootstrapFilter(scan, 1024) if tau is None else BootstrapFilter(scan, 1024, ess_threshold=tau)
    out = bf.run(genjax.key(9), C["y"].set(ys), (carry0, None))
    x, lw = bf.latent(out, "x"), out["logw"]
    assert x.shape == (DX, 1024)
    ref = Ref(_np(x), _np(lw))
    for cov in (False, True):
        want = "cov" if cov else "var"
        pm = bf.posterior_moments(out, "x", cov=cov)
        km = kernels.weighted_moments(x, lw, want)
        assert set(pm) == {"mean", want} and pm[want].shape == ((DX, DX) if cov else (DX,))
        assert _bits_equal(pm["mean"], km["mean"]) and _bits_equal(pm[want], km[want])
        _check({"stats": _np(km["stats"]), "mean": _np(pm["mean"]), want: _np(pm[want])}, ref, f"filter tau={tau} {want}")
    with pytest.raises(KeyError):
        bf.posterior_moments(out, "nope")


def test_stacked_scan_name_and_site_covariance():
    """ImportanceK over scan(n=4): "x" names the stacked sequence (what Trace.get_choices stacks), ("x", t) one step"""
    import torch
    from genjax_amd.inference import ImportanceK, Target
    T, K = 4, 1500
    scan, carry0, ys = _lgssm_scan(T)
    pc = ImportanceK(Target(scan, (carry0, None), C["y"].set(ys)), k_particles=K).run_smc(genjax.key(5))
    m = pc.moments()
    mean, var = m.mean("x"), m.variance("x")
    assert mean.shape == (T, DX) and var.shape == (T, DX)
    tr = pc.get_particles()
    lw = _np(pc.get_log_weights())
    stats = _np(m.stats)
    for t in range(T):
        assert torch.equal(mean[t], m.mean(("x", t))) and torch.equal(var[t], pc.variance(("x", t)))
        slot = tr.prog.slot_of[("x", t)]
        ref = Ref(_np(tr.choices[slot:slot + DX]), lw)
        _check(dict(stats=stats, mean=_np(mean[t]), var=_np(var[t])), ref, f"scan step {t}")
        cov = pc.covariance(("x", t))
        assert cov.shape == (DX, DX)
        _check(dict(stats=stats, mean=_np(mean[t]), cov=_np(cov)), ref, f"scan step {t} cov")
    # the chain's values as the trace stacks them: [K][T][DX]
    x = _np(tr.get_choices()["x"]).astype(np.float64)
    e = np.exp(lw.astype(np.float64) - lw.max())
    np.testing.assert_allclose(_np(mean), np.einsum("k,ktd->td", e, x) / e.sum(), rtol=1e-4, atol=1e-4)
