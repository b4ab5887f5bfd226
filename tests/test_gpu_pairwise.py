"""gjx_pairwise_gauss_lse against the float64 restatement in tests/pairwise_ref.py, and the marginal backward smoother on it against the
float64 recursion on the history's own tensors.  Finite outputs are held to pairwise_ref.bound; -inf and NaN must match exactly.
256 queries make a block, 64 keys a staged tile, 193 is the smallest n_k that is split over two blocks."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from genjax_amd import _abi as A
import pairwise_ref as R

SHAPES = [(1, 1, 1), (3, 15, 3), (4, 16, 16), (8, 17, 17), (13, 257, 63), (32, 1, 65), (8, 257, 194), (1, 17, 194), (32, 16, 194),
          (3, 257, 65), (13, 15, 17), (4, 1, 63)]


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def _check(q, k, bias, p, centre=None, what=""):
    """one call on float32 inputs against the restatement on the same numbers; returns the device output"""
    from genjax_amd import kernels
    out = kernels.pairwise_gauss_lse(_dev(q), _dev(k), _dev(bias), p, _dev(centre))
    got, ref = _np(out).astype(np.float64), R.pairwise_lse(q, k, bias, p)
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(got[~fin], ref[~fin])
    if fin.any():
        err = np.abs(got - ref)[fin]
        print(f"pairwise {what}: worst error / bound(C = 1) = {(err / R.bound(q, k, bias, p, centre, 1.0)[fin]).max():.3f}")
        assert (err <= R.bound(q, k, bias, p, centre)[fin]).all(), what
    return out


@pytest.mark.parametrize("kind", ["none", "weights", "dead", "nan"])
@pytest.mark.parametrize("d,n_q,n_k", SHAPES)
def test_matches_float64(d, n_q, n_k, kind):
    rs = np.random.default_rng(1000 * d + 10 * n_q + n_k)
    q, k = rs.standard_normal((d, n_q)).astype(np.float32), rs.standard_normal((d, n_k)).astype(np.float32)
    lw = 1.5 * rs.standard_normal(n_k)
    b = None if kind == "none" else (lw - np.logaddexp.reduce(lw)).astype(np.float32)      # normalised log-weights
    if kind in ("dead", "nan"):                             # 30 % dead keys, carrying NaN and inf coordinates
        dead = rs.random(n_k) < 0.3
        b[dead] = np.nan if kind == "nan" else -np.inf
        k[:, dead] = np.where(rs.random((d, int(dead.sum()))) < 0.5, np.nan, np.inf)
    _check(q, k, b, 0.7, what=f"d={d} n_q={n_q} n_k={n_k} {kind}")


def test_views_nan_query_all_dead_and_reproducibility():
    import torch
    from genjax_amd import kernels
    rs = np.random.default_rng(5)
    d, n_q, n_k = 5, 300, 500
    Q, K = rs.standard_normal((d, n_q + 6)).astype(np.float32), rs.standard_normal((d, n_k + 3)).astype(np.float32)
    q, k, b = Q[:, 1:1 + n_q], K[:, 3:3 + n_k], rs.standard_normal(n_k).astype(np.float32)
    q[2, 41] = np.nan                                       # one bad query: its output alone is NaN
    out = _check(q, k, b, 0.9, what="one NaN query")
    assert np.isnan(_np(out)[41]) and np.isfinite(np.delete(_np(out), 41)).all()
    # rows that start at an odd column of a wider table (4-byte aligned only, stride > n): the same bits, NaN included
    view = kernels.pairwise_gauss_lse(_dev(Q)[:, 1:1 + n_q], _dev(K)[:, 3:3 + n_k], _dev(b), 0.9)
    assert torch.equal(out.view(torch.int32), view.view(torch.int32))
    k[:, ::3] = np.inf                                      # every key dead, some with coordinates to match
    out = _check(q, k, np.full(n_k, -np.inf, np.float32), 0.9, what="all dead")
    assert (np.delete(_np(out), 41) == -np.inf).all()


def test_centre_decides_the_accuracy_on_offset_data():
    """Both sets sit at 1e3 + N(0, 1).  The score's three terms are then each about p d 1e6 and cancel to O(d): without a centre their
    float32 roundings (2^-24 p d 1e6, about 0.5) are the error, and the bound, stated in the centred norms of the call that was made,
    says so.  Only the centred call is held to the bound of centred data."""
    rs = np.random.default_rng(8)
    q, k = (1e3 + rs.standard_normal((8, 100))).astype(np.float32), (1e3 + rs.standard_normal((8, 200))).astype(np.float32)
    centre = k.astype(np.float64).mean(1).astype(np.float32)
    _check(q, k, None, 1.0, centre, what="offset 1e3, centred")
    assert R.bound(q, k, None, 1.0, centre).max() < 1e-3 < 0.1 < R.bound(q, k, None, 1.0).min()
    _check(q, k, None, 1.0, None, what="offset 1e3, no centre (its own, looser bound)")


def test_scores_spread_over_160_with_a_maximum_that_moves_in_every_tile():
    """queries near the origin, keys on shells of decreasing radius: every staged tile of 64 keys raises the running maximum"""
    rs = np.random.default_rng(9)
    d, n_q, n_k = 4, 40, 647
    k = rs.standard_normal((d, n_k))
    k = (k / np.sqrt((k ** 2).sum(0)) * np.linspace(np.sqrt(320.0), 0.1, n_k)).astype(np.float32)
    q = (0.05 * rs.standard_normal((d, n_q))).astype(np.float32)
    s = -0.5 * ((q[:, :1].astype(np.float64) - k) ** 2).sum(0)
    assert s.max() - s.min() > 150 and (np.diff(s[:640].reshape(10, 64).max(1)) > 0).all()
    _check(q, k, None, 1.0, what="spread")


def test_refusals():
    import torch
    from genjax_amd import _lib
    lib = _lib.load()
    x, ws, out = torch.zeros((33, 64), device="cuda"), torch.zeros(1 << 16, dtype=torch.uint8, device="cuda"), torch.empty(64, device="cuda")
    call = lambda d=4, p=1.0, n=ws.numel(), q=x.data_ptr(): lib.gjx_pairwise_gauss_lse(q, 64, 64, x.data_ptr(), 64, 64, d, None, p, None,
                                                                                     out.data_ptr(), ws.data_ptr(), n, None)
    assert call(p=0.0) == A.EINVAL and call(p=float("nan")) == A.EINVAL and call(d=0) == A.EINVAL and call(q=None) == A.EINVAL
    assert call(d=33) == A.EUNSUPPORTED and lib.gjx_pairwise_gauss_lse_workspace_bytes(64, 64, 33) == 0
    need = lib.gjx_pairwise_gauss_lse_workspace_bytes(64, 64, 4)
    assert 0 < need <= ws.numel() and call(n=need - 1) == A.EWORKSPACE and call(n=need) == A.OK
    torch.cuda.synchronize()


@pytest.mark.parametrize("K,dx", [(300, 2), (300, 8), (512, 2), (512, 8)])
def test_ffbs_weights_of_a_filter_history(K, dx):
    import torch
    from genjax_amd import core, kernels, workloads
    from genjax_amd.inference.pf import BootstrapFilter, LinearGaussianSSM
    T = 5
    s = workloads.ssm_problem(dx=dx, T=T, r=1.0)
    ssm = LinearGaussianSSM(s["A"], s["q"], s["r"])
    h = BootstrapFilter(ssm, K).run(core.key(3), s["y"], keep_history=True)["history"]
    lineage_before = h.smoothed_moments()
    w = h.ffbs_weights()
    assert w.shape == (T, K) and w.dtype == torch.float32
    states, logw, p = [_np(x).astype(np.float64) for x in h.states], [_np(l) for l in h.logw_steps], 1.0 / s["q"] ** 2
    means = [_np(torch.matmul(torch.from_numpy(ssm.A).cuda(), x)).astype(np.float64) for x in h.states]     # the float32 means the kernel saw
    ref = R.ffbs_log_weights(states, logw, means, p)
    per_call = 0.0          # the largest bound over both calls of every step, with the smoother's centre (the weighted mean of x_{t+1})
    for t in range(T - 1):
        cen = (states[t + 1] * np.exp(logw[t + 1] - np.logaddexp.reduce(logw[t + 1].astype(np.float64)))).sum(1)
        per_call = max(per_call, R.bound(states[t + 1], means[t], None, p, cen).max(), R.bound(means[t], states[t + 1], None, p, cen).max())
    worst = np.abs(np.log(_np(w).astype(np.float64)) - ref)[ref > np.log(2.0 ** -40)].max()
    print(f"ffbs K={K} dx={dx}: worst log-weight error {worst:.3e}, allowed {2 * T * per_call:.3e}")
    assert worst <= 2 * T * per_call
    assert np.abs(_np(w).astype(np.float64).sum(1) - 1.0).max() < 1e-5
    np.testing.assert_allclose(_np(w)[T - 1], np.exp(ref[T - 1]), rtol=1e-5, atol=0)          # the filter's own normalised weights
    m = h.smoothed_moments(method="ffbs")                   # the moments kernel under exactly these weights
    for t in range(T):
        one = kernels.weighted_moments(h.states[t], torch.log(w[t]), "var")
        assert torch.equal(m["mean"][t], one["mean"]) and torch.equal(m["var"][t], one["var"])
    assert h.smoothed_quantiles((0.5,), method="ffbs").shape == (T, dx, 1)
    again = h.smoothed_moments(method="lineage")            # the default: untouched, and still today's definition
    assert all(torch.equal(again[n], lineage_before[n]) for n in ("mean", "var", "ess"))
    assert torch.equal(again["mean"][0], kernels.weighted_moments(h.states[0], torch.log(h.smoothing_weights())[0], "var")["mean"])
    moved = BootstrapFilter(ssm, K, rejuvenate=dict(n_moves=1, scale=0.4)).run(core.key(3), s["y"], keep_history=True)["history"]
    with pytest.raises(NotImplementedError):
        moved.smoothed_moments(method="ffbs")
