"""Descendant weights on the device (gjx_lineage_weights) against the restatement of the definition in tests/lineage_ref.py (a backward
np.add.at on exact integers, checked against lineage tracing in tests/test_lineage_cpu.py), then the smoothed moments and quantiles
of ScanHistory / ParticleHistory against float64 NumPy on the history's own tensors and against the existing smoothed_means (float64
torch over paths()): two independent formulations of one estimator.

Exact cases (equal weights, and log-weights in {0, -inf}: every u_i is 0 or 2^32 on both sides) are compared bitwise.  General
weights per entry: |w - ref| <= delta, delta = K 2^-32 / sum e64 + 1e-5, the bound tests/test_gpu_quantiles.py applies to a
histogram's mass (rint of every integer; 3 x the float32 error of the hardware exponential) — a descendant weight is such a mass.

Through the filters, with ref the float64 estimate under the float64 reference weights of the step:
    |mean - ref|  <= 3e-5 max|x_t| + tol_mean,      |var - ref| <= 3e-5 max|x_t - mean_t|^2 + tol_var
over the step's surviving particles, tol_mean and tol_var being those of tests/test_gpu_moments.py (``Ref``, imported: eps range +
2^-22 |mean|, eps range^2 + 2^-40 mean^2; they do not depend on K).  The 3e-5: the total variation sum_j |w - ref| < 1e-5 of the
weights (above); the float32 log of w and the moments call's own exponential, about 1e-5; the float32 store of w.  Quantiles: the
bracket of tests/test_gpu_quantiles.py under the reference weights with delta' = K 2^-32 + 2e-5 (the quantile call's own delta with
sum e >= 1 after its renormalisation, and the 1e-5 total variation of its input weights).
The out-of-range guard is not exercised on the device: a wrong guard would be a memory fault.  In k_l_step / l_scatter an ancestor
is used as an index in one place, the head's atomicAdd, behind ``(uint32_t)d < (uint32_t)K``.
Worst error / bound ratios on an MI355X: see DESIGN.md section 5."""
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
from lineage_ref import descendant_weights, ref_e64, ref_u, ref_w32

LEVELS = (0.05, 0.5, 0.95)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a: dict, b: dict):
    import torch
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k].contiguous(), b[k].contiguous()
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), k


def _lw(anc, logw=None, ws=None):
    from genjax_amd import kernels
    return kernels.lineage_weights(anc, logw, ws)


# ---- the kernel, bitwise ----
TABLES = ["sorted", "permutation", "random", "all_to_0", "all_to_last", "identity"]


def _table(rs, T, K, kind):
    n = T - 1
    if n == 0:
        return np.zeros((0, K), np.int32)
    if kind == "sorted":
        a = np.sort(rs.integers(0, K, (n, K)), axis=1)
    elif kind == "permutation":
        a = np.stack([rs.permutation(K) for _ in range(n)])
    elif kind == "random":
        a = rs.integers(0, K, (n, K))
    elif kind == "all_to_0":
        a = np.zeros((n, K))
    elif kind == "all_to_last":
        a = np.full((n, K), K - 1)
    else:
        a = np.tile(np.arange(K), (n, 1))
    return np.ascontiguousarray(a, np.int32).reshape(n, K)


def _check_exact(got, anc, logw, K, T, what):
    u = ref_u(logw, K)
    U = int(u.sum())
    W = descendant_weights(anc, u)
    w, surv = _np(got["w"]), _np(got["survivors"])
    assert w.shape == (T, K) and w.dtype == np.float32 and surv.shape == (T,) and surv.dtype == np.int32
    assert (_bits(w) == _bits(ref_w32(W, U))).all(), what
    assert (surv == (W > 0).sum(axis=1)).all(), (what, surv)
    assert int(_np(got["n_bad"])[0]) == 0
    n = U >> 32
    np.testing.assert_array_equal(_np(got["stats"]), np.array([0, n, n, n], np.float32) if U else np.array([-np.inf, 0, 0, 0], np.float32))


@pytest.mark.parametrize("T", [1, 2, 9])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 1023, 1025, 4113])
def test_exact_cases_are_bitwise_the_definition(K, T):
    rs = np.random.default_rng(1000 * K + T)
    dead = rs.random(K) < 0.3
    dead[rs.integers(0, K)] = False
    logw = np.where(dead, -np.inf, 0.0).astype(np.float32)
    dlogw = _dev(logw)
    for kind in TABLES:
        anc = _table(rs, T, K, kind)
        danc = _dev(anc)
        for lw, dlw in ((None, None), (logw, dlogw)):
            _check_exact(_lw(danc, dlw), anc, lw, K, T, (K, T, kind, lw is None))


@pytest.mark.parametrize("K", [65, 1025])
def test_strided_view_and_dirty_workspace(K):
    import torch
    from genjax_amd._lib import load
    T = 5
    rs = np.random.default_rng(K)
    anc = _table(rs, T, K, "sorted")
    logw = np.where(rs.random(K) < 0.3, -np.inf, 0.0).astype(np.float32)
    danc, dlogw = _dev(anc), _dev(logw)
    base = _lw(danc, dlogw)
    _check_exact(base, anc, logw, K, T, K)
    wide = torch.full((T - 1, K + 9), -7, dtype=torch.int32, device="cuda")      # (what lies between the rows is never read as a link)
    wide[:, 1:K + 1] = danc
    view = wide[:, 1:K + 1]
    assert not view.is_contiguous() and view.stride() == (K + 9, 1)
    _same(_lw(view, dlogw), base)
    need = load().gjx_lineage_weights_workspace_bytes(T, K)
    big = torch.full((2 * need + 4096,), 255, dtype=torch.uint8, device="cuda")   # larger, and dirty: the call zeroes what it uses
    _same(_lw(danc, dlogw, ws=big[1:]), base)                                     # (and not 8-byte aligned)
    _same(_lw(danc, dlogw, ws=big[:need]), base)


@pytest.mark.parametrize("K", [63, 1500])
def test_without_weight_there_is_no_estimate(K):
    rs = np.random.default_rng(K)
    T = 4
    anc = _dev(_table(rs, T, K, "sorted"))
    dead = np.full(K, -np.inf, np.float32)
    mixed = dead.copy()
    mixed[::3] = np.nan
    overflow = rs.standard_normal(K).astype(np.float32)
    overflow[K // 2] = np.inf                              # exp(w - inf) = 0 everywhere else, NaN there: u = 0 everywhere
    for lw in (dead, np.full(K, np.nan, np.float32), mixed, overflow):
        got = _lw(anc, _dev(lw))
        np.testing.assert_array_equal(_np(got["stats"]), np.array([-np.inf, 0, 0, 0], np.float32))
        assert np.isnan(_np(got["w"])).all() and got["w"].shape == (T, K)
        assert (_np(got["survivors"]) == 0).all() and int(_np(got["n_bad"])[0]) == 0


@pytest.mark.parametrize("kind", ["all_to_last", "sorted", "random"])
def test_bit_reproducible(kind):
    K, T = 4113, 9
    rs = np.random.default_rng(17)
    anc = _dev(_table(rs, T, K, kind))
    logw = (3.0 * rs.standard_normal(K)).astype(np.float32)
    logw[rs.random(K) < 0.2] = -np.inf
    dlogw = _dev(logw)
    first = _lw(anc, dlogw)
    for _ in range(2):
        _same(_lw(anc, dlogw), first)
    _same(_lw(anc, None), _lw(anc, None))


# ---- the kernel, general weights ----
@pytest.mark.parametrize("kind", ["sorted", "random"])
@pytest.mark.parametrize("K", [1025, 4113])
def test_general_weights_are_within_the_mass_bound(K, kind):
    T = 9
    rs = np.random.default_rng(K + len(kind))
    anc = _table(rs, T, K, kind)
    logw = (3.0 * rs.standard_normal(K)).astype(np.float32)
    logw[rs.random(K) < 0.2] = -np.inf
    logw[rs.permutation(K)[:5]] = np.nan
    got = _lw(_dev(anc), _dev(logw))
    w, surv = _np(got["w"]).astype(np.float64), _np(got["survivors"])
    e = ref_e64(logw, K)
    ref = descendant_weights(anc, e) / e.sum()
    delta = K * 2.0 ** -32 / e.sum() + 1e-5
    err = np.abs(w - ref).max()
    print(f"[lineage] K={K} {kind}: worst |w - ref|/delta {err / delta:.3g}, row sums off by {np.abs(w.sum(axis=1) - 1.0).max():.3g}")
    assert err <= delta, (K, kind, err, delta)
    assert (np.diff(surv) >= 0).all() and surv[T - 1] == int((ref_u(logw, K) > 0).sum())
    assert (surv == (_np(got["w"]) > 0).sum(axis=1)).all()
    assert (np.abs(w.sum(axis=1) - 1.0) <= K * 2.0 ** -24).all()
    assert int(_np(got["n_bad"])[0]) == 0
    st = _np(got["stats"]).astype(np.float64)
    live = np.isfinite(logw)
    assert st[0] == logw[live].max()
    np.testing.assert_allclose(st[1:], [e.sum(), (e * e).sum(), e.sum() ** 2 / (e * e).sum()], rtol=1e-4)


# ---- through the filters ----
DX, T_RUN, K_RUN = 4, 8, 1 << 12


def _problem():
    from genjax_amd import workloads
    return workloads.ssm_problem(dx=DX, T=T_RUN, r=2.0)


def _lgssm_scan(s):
    """the linear-Gaussian state space as @gen + .scan (x_0 ~ N(0, q)), as tests/test_gpu_scan_filter.py writes it"""
    Am = np.asarray(s["A"], np.float32)
    q, r = float(s["q"]), float(s["r"])

    @genjax.gen
    def step(x_prev, _):
        x = genjax.mv_normal_diag(Am @ x_prev, np.full(DX, q, np.float32)) @ "x"
        genjax.mv_normal_diag(x, np.full(DX, r, np.float32)) @ "y"
        return x, None

    return step.scan(n=T_RUN), np.zeros(DX, np.float32)


_runs: dict = {}


def _run(which):
    """-> (history, args of its per-name methods, rows(t) -> (float32 rows [DX][K] on the host, the step whose weights they stand under),
    ancestors i32[T-1][K] on the host); made once per kind and never written to"""
    if which in _runs:
        return _runs[which]
    import torch
    from genjax_amd import core
    from genjax_amd.inference import BootstrapFilter
    s = _problem()
    ys = np.asarray(s["y"], np.float32)
    if which == "hand_written":
        from genjax_amd.inference.pf import LinearGaussianSSM
        bf = BootstrapFilter(LinearGaussianSSM(s["A"], s["q"], s["r"]), K_RUN)
        h = bf.run(core.key(3), s["y"], keep_history=True)["history"]
        name = ()
        anc = _np(torch.stack(h.ancestors))
        rows = lambda t: (_np(h.states[t]), t)
    else:
        scan, carry0 = _lgssm_scan(s)
        kw = dict(plain={}, moved=dict(rejuvenate=dict(n_moves=2, scale=0.35)), adaptive=dict(ess_threshold=0.5))[which]
        bf = BootstrapFilter(scan, K_RUN, **kw)
        h = bf.run(genjax.key(3), C["y"].set(ys), (carry0, None), keep_history=True)["history"]
        name = ("x",)
        anc = _np(h.ancestors)
        assert h.moved == (which == "moved")

        def rows(t):
            if which == "moved" and t < T_RUN - 1:       # the moved carry in step t+1's INPUT rows at the child's index, as paths() defines it
                prog = h.programs[t + 1]
                r0 = [prog.slot_of[sx.addr] for sx in prog.site_list.sites if prog.modes.get(sx.addr) == A.MODE_INPUT][0]
                return _np(h.rows_all[t + 1, r0:r0 + DX]), t + 1
            return _np(h.step(t, "x")), t
    assert len(h) == T_RUN and anc.shape == (T_RUN - 1, K_RUN)
    _runs[which] = (h, name, rows, anc)
    return _runs[which]


def _bracket(x, wref, levels, got, live_bits, delta, what):
    """the bracket of tests/test_gpu_quantiles.py under given float64 weights (sum 1) -> worst slack / delta"""
    xs = x.astype(np.float64)
    worst = 0.0
    for q, v in zip(levels, got):
        assert int(_bits(v)[0]) in live_bits, (what, q, v)
        below, upto = wref[xs < float(v)].sum(), wref[xs <= float(v)].sum()
        worst = max(worst, max(below - q, q - upto, 0.0) / delta)
        assert below <= q + delta and upto >= q - delta, (what, q, v, below, upto, delta)
    return worst


@pytest.mark.parametrize("which", ["plain", "moved", "adaptive", "hand_written"])
def test_smoothed_estimates_of_a_filter_run(which):
    from test_gpu_moments import Ref                        # its tol_mean / tol_var are the moments call's own allowance
    h, name, rows, anc = _run(which)
    K, T = K_RUN, T_RUN
    logw = _np(h.logw)
    e = ref_e64(logw, K)
    wref = descendant_weights(anc, e) / e.sum()            # float64 [T][K]
    w = h.smoothing_weights()
    assert h.smoothing_weights() is w and w.shape == (T, K) and w.is_cuda          # computed once
    wh = _np(w)
    surv = _np(h.survivors())
    assert surv[T - 1] == int((ref_u(logw, K) > 0).sum()) and (np.diff(surv) >= 0).all() and surv[0] >= 1
    assert (surv == (wh > 0).sum(axis=1)).all()
    assert np.abs(wh.astype(np.float64) - wref).max() <= K * 2.0 ** -32 / e.sum() + 1e-5

    mom = h.smoothed_moments(*name)
    assert sorted(mom) == ["ess", "mean", "var"] and mom["mean"].shape == (T, DX) and mom["var"].shape == (T, DX) and mom["ess"].shape == (T,)
    cov = h.smoothed_moments(*name, cov=True)
    assert sorted(cov) == ["cov", "ess", "mean"] and cov["cov"].shape == (T, DX, DX)
    qs = h.smoothed_quantiles(*name, LEVELS)
    assert qs.shape == (T, DX, 3) and qs.is_cuda
    mean, var, ess, qh = _np(mom["mean"]), _np(mom["var"]), _np(mom["ess"]), _np(qs)
    old = _np(h.smoothed_means(*name)).astype(np.float64)  # the existing formulation: float64 torch over paths()
    assert np.isfinite(ess).all() and (ess <= surv).all()
    delta_q = K * 2.0 ** -32 + 2e-5
    worst = dict(mean=0.0, var=0.0, cross=0.0, quant=0.0)
    for t in range(T):
        x, tw = rows(t)
        wt = wref[tw]
        live = wt > 0
        with np.errstate(divide="ignore"):
            ref = Ref(x, np.log(wt))
        xl = x[:, live].astype(np.float64)
        b_mean = 3e-5 * np.abs(xl).max(axis=1) + ref.tol_mean
        b_var = 3e-5 * (np.abs(xl - ref.mean[:, None]) ** 2).max(axis=1) + ref.tol_var
        e_mean, e_var, e_cross = np.abs(mean[t] - ref.mean), np.abs(var[t] - ref.var), np.abs(old[t] - mean[t])
        worst["mean"] = max(worst["mean"], (e_mean / b_mean).max())
        worst["var"] = max(worst["var"], (e_var / b_var).max())
        worst["cross"] = max(worst["cross"], (e_cross / b_mean).max())
        assert (e_mean <= b_mean).all(), (which, t, e_mean, b_mean)
        assert (e_var <= b_var).all(), (which, t, e_var, b_var)
        assert (e_cross <= b_mean).all(), (which, t, e_cross, b_mean)
        assert (np.abs(np.diagonal(_np(cov["cov"][t])) - ref.var) <= b_var).all() and (_bits(_np(cov["mean"][t])) == _bits(mean[t])).all()
        if t in (0, T - 1):                                 # the per-step outputs are those of the moments call on that step alone
            import torch
            from genjax_amd import kernels
            one = kernels.weighted_moments(_dev(x), torch.log(w[tw]), "var")
            assert (_bits(_np(one["mean"])) == _bits(mean[t])).all() and (_bits(_np(one["var"])) == _bits(var[t])).all()
            assert _bits(_np(one["stats"][3:4]))[0] == _bits(ess[t:t + 1])[0]
        dev_live = wh[tw] > 0
        for d in range(DX):
            bits = set(_bits(x[d][dev_live]).tolist())
            worst["quant"] = max(worst["quant"], _bracket(x[d], wt, LEVELS, qh[t, d], bits, delta_q, f"{which} step {t} x[{d}]"))
    print(f"[lineage] {which}: worst error/bound: mean {worst['mean']:.3g}, var {worst['var']:.3g}, "
          f"mean vs smoothed_means {worst['cross']:.3g}, quantile slack/delta' {worst['quant']:.3g}; survivors {surv.tolist()}")


def test_a_name_the_history_cannot_serve_raises_like_paths():
    h, name, rows, anc = _run("moved")
    with pytest.raises(NotImplementedError, match="does not receive"):
        h.smoothed_moments("y")                             # (no step receives the observation as carry)
    with pytest.raises(KeyError):
        _run("plain")[0].smoothed_quantiles("nope")
