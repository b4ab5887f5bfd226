"""gjx_pairwise_gauss_mean against the float64 restatement in tests/pairwise_mean_ref.py, and the FFBSm lag-one pair moments built on
it against float64 pair sums on the history's own tensors.  Finite outputs are held to pairwise_mean_ref.bound (the mean) and
pairwise_ref.bound (the lse); NaN and -inf must match exactly.  The kernel plans as gjx_pairwise_gauss_lse does: 16 queries make a
group and 16 value rows a block, 64 keys a staged tile, 256 queries a block, 194 keys are split over two blocks."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from genjax_amd import _abi as A
import pairwise_mean_ref as M
import pairwise_ref as R
from test_gpu_pairwise import _dev, _np

SHAPES = [(1, 1, 1, 1), (3, 3, 15, 3), (8, 16, 17, 17), (13, 17, 257, 63), (32, 32, 1, 65), (8, 8, 257, 194), (4, 1, 17, 194), (1, 32, 16, 65)]


def _check(q, k, v, bias, p, centre=None, what=""):
    """one call on float32 inputs against the restatement on the same numbers; returns the device outputs"""
    from genjax_amd import kernels
    out = kernels.pairwise_gauss_mean(_dev(q), _dev(k), _dev(v), _dev(bias), p, _dev(centre))
    ref_mean, ref_lse = M.pairwise_mean(q, k, v, bias, p)
    for name, got, ref, bnd, bnd1 in (("lse", _np(out["lse"]), ref_lse, R.bound(q, k, bias, p, centre), R.bound(q, k, bias, p, centre, 1.0)),
                                      ("mean", _np(out["mean"]), ref_mean, M.bound(q, k, v, bias, p, centre), None)):
        fin = np.isfinite(ref)
        np.testing.assert_array_equal(got[~fin], ref[~fin], err_msg=f"{what} {name}")
        if fin.any():
            err = np.abs(got.astype(np.float64) - ref)[fin]
            scale = (bnd if bnd1 is None else bnd1)[fin]
            print(f"pairwise mean {what}: {name} worst error / bound{'' if bnd1 is None else '(C = 1)'} = "
                  f"{(err / np.maximum(scale, 1e-300)).max():.3f}")
            assert (err <= bnd[fin]).all(), (what, name)
    return out


@pytest.mark.parametrize("kind", ["none", "weights", "dead"])
@pytest.mark.parametrize("d,dv,n_q,n_k", SHAPES)
def test_matches_float64(d, dv, n_q, n_k, kind):
    rs = np.random.default_rng(1000 * d + 100 * dv + 10 * n_q + n_k)
    q, k = rs.standard_normal((d, n_q)).astype(np.float32), rs.standard_normal((d, n_k)).astype(np.float32)
    v = rs.standard_normal((dv, n_k)).astype(np.float32)
    lw = 1.5 * rs.standard_normal(n_k)
    b = None if kind == "none" else (lw - np.logaddexp.reduce(lw)).astype(np.float32)      # normalised log-weights
    if kind == "dead":                                      # 30 % dead keys (-inf or NaN), carrying NaN and inf coordinates and values
        dead = rs.random(n_k) < 0.3
        b[dead] = np.where(rs.random(int(dead.sum())) < 0.5, np.nan, -np.inf)
        k[:, dead] = np.where(rs.random((d, int(dead.sum()))) < 0.5, np.nan, np.inf)
        v[:, dead] = np.where(rs.random((dv, int(dead.sum()))) < 0.5, np.nan, -np.inf)
    _check(q, k, v, b, 0.7, what=f"d={d} dv={dv} n_q={n_q} n_k={n_k} {kind}")


def test_a_maximum_that_moves_in_every_tile():
    """queries near the origin, keys on shells of decreasing radius: every staged tile of 64 keys raises the running maximum, so the
    accumulated O^T is rescaled by a factor far from 1 in every tile"""
    rs = np.random.default_rng(9)
    d, n_q, n_k = 4, 40, 647
    k = rs.standard_normal((d, n_k))
    k = (k / np.sqrt((k ** 2).sum(0)) * np.linspace(np.sqrt(320.0), 0.1, n_k)).astype(np.float32)
    q = (0.05 * rs.standard_normal((d, n_q))).astype(np.float32)
    s = -0.5 * ((q[:, :1].astype(np.float64) - k) ** 2).sum(0)
    assert s.max() - s.min() > 150 and (np.diff(s[:640].reshape(10, 64).max(1)) > 0).all()
    _check(q, k, rs.standard_normal((5, n_k)).astype(np.float32), None, 1.0, what="spread")


def test_nan_query_inf_value_all_dead_views_and_reproducibility():
    import torch
    from genjax_amd import kernels
    rs = np.random.default_rng(5)
    d, dv, n_q, n_k = 5, 6, 300, 500
    Q, K, V = (rs.standard_normal((n, w)).astype(np.float32) for n, w in ((d, n_q + 6), (d, n_k + 3), (dv, n_k + 5)))
    q, k, v, b = Q[:, 1:1 + n_q], K[:, 3:3 + n_k], V[:, 5:5 + n_k], rs.standard_normal(n_k).astype(np.float32)
    q[2, 41] = np.nan                                       # one bad query: its outputs alone are NaN
    v[4, 77] = np.inf                                       # one live key's value: its component alone, every query
    out = _check(q, k, v, b, 0.9, what="one NaN query, one inf value")
    mean, lse = _np(out["mean"]), _np(out["lse"])
    assert np.isnan(lse[41]) and np.isfinite(np.delete(lse, 41)).all()
    assert np.isnan(mean[:, 41]).all() and np.isnan(mean[4]).all() and np.isfinite(np.delete(np.delete(mean, 4, 0), 41, 1)).all()
    # rows that start at an odd column of a wider table (4-byte aligned only, stride > n), and a second call: the same bits
    view = kernels.pairwise_gauss_mean(_dev(Q)[:, 1:1 + n_q], _dev(K)[:, 3:3 + n_k], _dev(V)[:, 5:5 + n_k], _dev(b), 0.9)
    again = kernels.pairwise_gauss_mean(_dev(q), _dev(k), _dev(v), _dev(b), 0.9)
    for name in ("mean", "lse"):
        assert torch.equal(out[name].view(torch.int32), view[name].view(torch.int32)), name
        assert torch.equal(out[name].view(torch.int32), again[name].view(torch.int32)), name
    out = _check(q, k, v, np.full(n_k, -np.inf, np.float32), 0.9, what="all dead")
    assert np.isnan(_np(out["mean"])).all() and (np.delete(_np(out["lse"]), 41) == -np.inf).all()


def test_refusals():
    import torch
    from genjax_amd import _lib
    lib = _lib.load()
    x, ws = torch.zeros((33, 64), device="cuda"), torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    mean, lse = torch.empty((33, 64), device="cuda"), torch.empty(64, device="cuda")
    call = lambda d=4, dv=4, p=1.0, n=ws.numel(), v=x.data_ptr(), sv=64, l=lse.data_ptr(): lib.gjx_pairwise_gauss_mean(
        x.data_ptr(), 64, 64, x.data_ptr(), 64, 64, d, v, sv, dv, None, p, None, mean.data_ptr(), l, ws.data_ptr(), n, None)
    assert call(p=0.0) == A.EINVAL and call(p=float("nan")) == A.EINVAL and call(d=0) == A.EINVAL and call(dv=0) == A.EINVAL
    assert call(v=None) == A.EINVAL and call(sv=63) == A.EINVAL
    assert call(d=33) == A.EUNSUPPORTED and call(dv=33) == A.EUNSUPPORTED
    need = lib.gjx_pairwise_gauss_mean_workspace_bytes(64, 64, 4, 4)
    assert 0 < need <= ws.numel() and call(n=need - 1) == A.EWORKSPACE and call(n=need) == A.OK and call(l=None) == A.OK
    torch.cuda.synchronize()


@pytest.mark.parametrize("K,dx", [(300, 2), (512, 8)])
def test_ffbs_pair_moments_of_a_filter_history(K, dx):
    import torch
    from cross_moments_ref import CrossRef
    from genjax_amd import core, workloads
    from genjax_amd.inference.pf import BootstrapFilter, LinearGaussianSSM
    T = 5
    s = workloads.ssm_problem(dx=dx, T=T, r=1.0)
    ssm = LinearGaussianSSM(s["A"], s["q"], s["r"])
    h = BootstrapFilter(ssm, K).run(core.key(3), s["y"], keep_history=True)["history"]
    lineage_before = h.smoothed_pair_moments()
    got = {n: _np(x).astype(np.float64) for n, x in h.smoothed_pair_moments(method="ffbs").items()}
    marginal = _np(h.smoothed_moments(method="ffbs")["mean"]).astype(np.float64)
    w, p = _np(h.ffbs_weights()).astype(np.float64), 1.0 / s["q"] ** 2
    x = [_np(a) for a in h.states]
    means = [_np(torch.matmul(torch.from_numpy(ssm.A).cuda(), a)) for a in h.states]        # the float32 means the kernel saw
    for t in range(1, T):
        lw = _np(h.logw_steps[t - 1]).astype(np.float64)
        lw, lw_t = lw - np.logaddexp.reduce(lw), _np(h.logw_steps[t]).astype(np.float64)
        cen = (x[t] * np.exp(lw_t - np.logaddexp.reduce(lw_t))).sum(1)                      # the call's centre
        sc = lw[None, :] - 0.5 * p * ((x[t].astype(np.float64)[:, :, None] - means[t - 1].astype(np.float64)[:, None, :]) ** 2).sum(0)
        cond = np.exp(sc - np.logaddexp.reduce(sc, axis=1)[:, None])                        # f64[K][K]: parent i given child j
        pair = w[t][:, None] * cond                                                         # the pair weights; they sum to 1
        mean, prev = x[t] @ pair.sum(1), x[t - 1] @ pair.sum(0)
        cross = (x[t] - mean[:, None]) @ pair @ (x[t - 1] - prev[:, None]).T
        # what gjx_weighted_cross_moments is allowed on (x_t, c), plus the error of c itself times the size of what it multiplies
        with np.errstate(divide="ignore"):
            tol = CrossRef(x[t], x[t - 1].astype(np.float64) @ cond.T, np.log(w[t]).astype(np.float32))
        extra = M.bound(x[t], means[t - 1], x[t - 1], lw.astype(np.float32), p, cen).max() * np.abs(x[t]).max()
        errs = {"mean": np.abs(got["mean"][t - 1] - mean) / (tol.tol_mean_a + extra),
                "mean_prev": np.abs(got["mean_prev"][t - 1] - prev) / (tol.tol_mean_b + extra),
                "cross": np.abs(got["cross"][t - 1] - cross) / (tol.tol_cross + extra),
                "marginal": np.abs(got["mean_prev"][t - 1] - marginal[t - 1]) / (tol.tol_mean_b + extra)}
        print(f"ffbs pair K={K} dx={dx} t={t}: worst error / allowed " + ", ".join(f"{n} {e.max():.3g}" for n, e in errs.items()))
        assert all((e <= 1.0).all() for e in errs.values()), (t, errs)
    again = h.smoothed_pair_moments()                       # the default: untouched by the ffbs call
    assert all(torch.equal(again[n].view(torch.int32), lineage_before[n].view(torch.int32)) for n in lineage_before)
    with pytest.raises(ValueError):
        h.smoothed_pair_moments(method="paths")
    moved = BootstrapFilter(ssm, K, rejuvenate=dict(n_moves=1, scale=0.4)).run(core.key(3), s["y"], keep_history=True)["history"]
    with pytest.raises(NotImplementedError):
        moved.smoothed_pair_moments(method="ffbs")
