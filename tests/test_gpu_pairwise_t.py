"""gjx_pairwise_t_lse and gjx_pairwise_t_mean against the float64 restatement in tests/pairwise_t_ref.py, and the marginal backward
smoother and its pair moments under a Student-t transition (dof=) against the float64 recursion written with the same restatement.
Finite outputs are held to pairwise_t_ref.bound / mean_bound at C = C_T; NaN and -inf must match exactly.  The kernels plan as the
Gaussian calls: 4 components a chunk, 256 queries a block, 64 keys a staged tile, 194 keys = four tiles = two key splits."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pairwise_t_ref as T
from test_gpu_pairwise import _dev, _np

C_T_MEASURED = 0.375          # worst lse error / bound(C = 1) over test_matches_float64's grid on an MI355X: 0.360 (d = 1, nu = 30,
                              # n_q = 17, n_k = 1; both kernels), rounded up; the tests use 4 x it, as every pairwise test here
C_T = 4.0 * C_T_MEASURED


def _check(q, k, bias, p, nu, centre=None, v=None, what=""):
    """both calls on float32 inputs against the restatement on the same numbers -> {name: device output}"""
    from genjax_amd import kernels
    ref_lse, ref_mean = T.pairwise_t(q, k, bias, p, nu, v)
    one, allowed = T.bound(q, k, bias, p, nu, centre), T.bound(q, k, bias, p, nu, centre, C_T)
    m = kernels.pairwise_t_mean(_dev(q), _dev(k), _dev(v), _dev(bias), p, nu, _dev(centre))
    outs = {"lse": kernels.pairwise_t_lse(_dev(q), _dev(k), _dev(bias), p, nu, _dev(centre)), "mean's lse": m["lse"], "mean": m["mean"]}
    for name, out in outs.items():
        ref, b1, bc = (ref_mean, T.mean_bound(one, v, bias), T.mean_bound(allowed, v, bias)) if name == "mean" else (ref_lse, one, allowed)
        got, fin = _np(out).astype(np.float64), np.isfinite(ref)
        np.testing.assert_array_equal(got[~fin], ref[~fin], err_msg=f"{what} {name}")
        if fin.any():
            err = np.abs(got - ref)[fin]
            print(f"pairwise t {what}: {name} worst error / bound(C = 1) = {(err / np.maximum(b1[fin], 1e-300)).max():.3f}")
            assert (err <= bc[fin]).all(), (what, name)
    return outs


@pytest.mark.parametrize("nu", [0.5, 1.0, 3.0, 30.0])
@pytest.mark.parametrize("d", [1, 4, 5, 32])
def test_matches_float64(d, nu):
    rs = np.random.default_rng(100 * d + int(10 * nu))
    for n_q in (1, 17, 257):
        for n_k in (1, 63, 65, 194):
            q, k = rs.standard_normal((d, n_q)).astype(np.float32), rs.standard_normal((d, n_k)).astype(np.float32)
            v, lw = rs.standard_normal((17, n_k)).astype(np.float32), 1.5 * rs.standard_normal(n_k)
            b = (lw - np.logaddexp.reduce(lw)).astype(np.float32)                              # normalised log-weights
            for dv in (1, 17):
                _check(q, k, b, 0.75, nu, v=v[:dv], what=f"d={d} nu={nu} n_q={n_q} n_k={n_k} dv={dv}")


# kind -> the NaN the rule asks for: (queries with a NaN lse, value rows that are NaN for every query); None: every output
EDGES = {"view": (0, 0), "offset": (0, 0), "spread": (0, 0), "dead": (0, 0), "all dead": None, "nan query": (1, 0), "poisoned key": None,
         "inf bias": None, "inf value": (0, 1)}


@pytest.mark.parametrize("kind", EDGES)
def test_edges_views_and_reproducibility(kind):
    import torch
    from genjax_amd import kernels
    rs = np.random.default_rng(5)
    d, dv, n_q, n_k, p, nu = 5, 6, 300, 500, 0.75, 3.0
    Q, K, V = (rs.standard_normal((n, w)).astype(np.float32) for n, w in ((d, n_q + 6), (d, n_k + 3), (dv, n_k + 5)))
    q, k, v, b, centre = Q[:, 1:1 + n_q], K[:, 3:3 + n_k], V[:, 5:5 + n_k], rs.standard_normal(n_k).astype(np.float32), None
    if kind == "offset":                                    # both sets at 1e3 + N(0, 1): only the centred call can meet the centred bound
        Q += 1e3
        K += 1e3
        centre = k.astype(np.float64).mean(1).astype(np.float32)
    if kind == "spread":                                    # biases over 160, rising: every staged tile moves the running maximum
        b = np.linspace(-160.0, 0.0, n_k).astype(np.float32)
    if kind == "dead":                                      # 30 % dead keys (-inf or NaN), carrying NaN and inf coordinates and values
        dead = rs.random(n_k) < 0.3
        b[dead] = np.where(rs.random(int(dead.sum())) < 0.5, np.nan, -np.inf)
        k[:, dead] = np.where(rs.random((d, int(dead.sum()))) < 0.5, np.nan, np.inf)
        v[:, dead] = np.where(rs.random((dv, int(dead.sum()))) < 0.5, np.nan, -np.inf)
    if kind == "all dead":
        b[:] = -np.inf
    q[2, 41] = np.nan if kind == "nan query" else q[2, 41]
    k[1, 77] = np.inf if kind == "poisoned key" else k[1, 77]
    b[77] = np.inf if kind == "inf bias" else b[77]
    v[4, 77] = np.inf if kind == "inf value" else v[4, 77]
    outs = _check(q, k, b, p, nu, centre, v, what=kind)
    lse, mean = _np(outs["lse"]), _np(outs["mean"])
    if kind == "all dead":
        assert (lse == -np.inf).all() and np.isnan(mean).all()
    elif EDGES[kind] is None:
        assert np.isnan(lse).all() and np.isnan(mean).all()
    else:
        assert np.isnan(lse).sum() == EDGES[kind][0] and np.isnan(mean).all(1).sum() == EDGES[kind][1]
        assert np.isnan(mean).sum() == EDGES[kind][0] * dv + EDGES[kind][1] * n_q
    if kind == "view":                                      # rows at odd columns of wider tables (4-byte aligned only), and a second run
        args = _dev(Q)[:, 1:1 + n_q], _dev(K)[:, 3:3 + n_k]
        view = kernels.pairwise_t_mean(*args, _dev(V)[:, 5:5 + n_k], _dev(b), p, nu)
        again = kernels.pairwise_t_mean(_dev(q), _dev(k), _dev(v), _dev(b), p, nu)
        for other in (view, again):
            assert torch.equal(outs["mean"].view(torch.int32), other["mean"].view(torch.int32))
            assert torch.equal(outs["mean's lse"].view(torch.int32), other["lse"].view(torch.int32))
        for _ in range(2):
            assert torch.equal(outs["lse"].view(torch.int32), kernels.pairwise_t_lse(*args, _dev(b), p, nu).view(torch.int32))


@pytest.mark.parametrize("d", [1, 2])
def test_ffbs_weights_and_pair_moments_under_a_t_transition(d):
    from cross_moments_ref import CrossRef
    from genjax_amd import kernels
    rs = np.random.default_rng(20 + d)
    n_t, K, p, nu = 4, 300, 2.0, 3.0
    x = [rs.standard_normal((d, K)).astype(np.float32) for _ in range(n_t)]
    means, logw = [(0.9 * a).astype(np.float32) for a in x], [rs.standard_normal(K).astype(np.float32) for _ in range(n_t)]
    dev = lambda rows: [_dev(a) for a in rows]
    w = kernels.ffbs_weights(dev(x), dev(logw), dev(means), p, dof=nu)
    ref = T.ffbs_log_weights(x, logw, means, p, nu)
    norm = lambda lw: lw.astype(np.float64) - np.logaddexp.reduce(lw.astype(np.float64))
    cen = [None] + [(x[t] * np.exp(norm(logw[t]))).sum(1) for t in range(1, n_t)]             # the calls' centres
    per_call = max(max(T.bound(x[t + 1], means[t], None, p, nu, cen[t + 1], C_T).max(), T.bound(means[t], x[t + 1], None, p, nu, cen[t + 1], C_T).max())
                   for t in range(n_t - 1))
    worst = np.abs(np.log(_np(w).astype(np.float64)) - ref)[ref > np.log(2.0 ** -40)].max()
    print(f"ffbs t d={d}: worst log-weight error {worst:.3e}, allowed {2 * n_t * per_call:.3e}")
    assert worst <= 2 * n_t * per_call and np.abs(_np(w).astype(np.float64).sum(1) - 1.0).max() < 1e-5
    got = {n: _np(a).astype(np.float64) for n, a in kernels.ffbs_pair_moments(dev(x), dev(logw), dev(means), p, weights=w, dof=nu).items()}
    for t in range(1, n_t):
        lw = norm(logw[t - 1])
        s = lw[None, :] - 0.5 * (nu + d) * np.log1p(p * ((x[t].astype(np.float64)[:, :, None] - means[t - 1].astype(np.float64)[:, None, :]) ** 2).sum(0) / nu)
        cond = np.exp(s - np.logaddexp.reduce(s, axis=1)[:, None])                             # f64[K][K]: parent i given child j
        r = CrossRef(x[t], x[t - 1].astype(np.float64) @ cond.T, np.log(_np(w)[t]))            # float64 moments of (x_t, c) and their tolerances
        extra = T.mean_bound(T.bound(x[t], means[t - 1], lw, p, nu, cen[t], C_T), x[t - 1], lw).max() * np.abs(x[t]).max()
        errs = {"mean": np.abs(got["mean"][t - 1] - r.mean_a) / (r.tol_mean_a + extra),
                "mean_prev": np.abs(got["mean_prev"][t - 1] - r.mean_b) / (r.tol_mean_b + extra),
                "cross": np.abs(got["cross"][t - 1] - r.cross) / (r.tol_cross + extra)}
        print(f"ffbs t pair d={d} t={t}: worst error / allowed " + ", ".join(f"{n} {e.max():.3g}" for n, e in errs.items()))
        assert all((e <= 1.0).all() for e in errs.values()), (t, errs)
