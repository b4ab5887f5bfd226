"""gjx_pairwise_gauss_pick against the float64 cumulative windows of tests/pairwise_pick_ref.py, and backward simulation (FFBSi) built on
it along the kernel's own path.  Every pick must be acceptable (pairwise_pick_ref.acceptable), the lse within pairwise_ref.bound, and in
every case the reference alone must accept more than one key for at most 5 % of the queries.  64 keys make a staged tile and a chunk,
256 queries a block; 194 keys are two splits, 321 three."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pairwise_pick_ref as P
import pairwise_ref as R
from test_gpu_pairwise import _dev, _np

SEED = 20                                                   # chosen on the CPU: every case of the grid is sharp under it


def _case(d, n_q, n_k, kind, seed=SEED):
    """coordinates of norm about 1 (the bound grows with the norms) in wider tables, "full": bias and centre; uniforms in float32"""
    rs = np.random.default_rng(seed + 1000 * d + 10 * n_q + n_k)
    Q, K = (rs.standard_normal((d, n_q + 5)) / np.sqrt(d)).astype(np.float32), (rs.standard_normal((d, n_k + 3)) / np.sqrt(d)).astype(np.float32)
    lw, u, k = 1.5 * rs.standard_normal(n_k), rs.random(n_q).astype(np.float32), K[:, 3:3 + n_k]
    full = kind == "full"
    return Q[:, 1:1 + n_q], k, (lw - np.logaddexp.reduce(lw)).astype(np.float32) if full else None, 0.7, u, k.mean(1) if full else None, Q, K


def _check(q, k, bias, p, u, centre=None, what="", dq=None, dk=None):
    """one call against the rule; ``dq`` / ``dk``: device views to call with in place of copies.  Returns the picks."""
    from genjax_amd import kernels
    out = kernels.pairwise_gauss_pick(_dev(q) if dq is None else dq, _dev(k) if dk is None else dk, _dev(u), _dev(bias), p, _dev(centre))
    pick, lse, ref = _np(out["pick"]), _np(out["lse"]).astype(np.float64), R.pairwise_lse(q, k, bias, p)
    ok, n_acc, slack = P.acceptable(pick, q, k, bias, p, u, centre)
    print(f"pairwise pick {what}: worst slack / tol(C_SUM = 1) = {slack.max():.3f}, ambiguous {np.mean(n_acc > 1):.3f}")
    assert np.mean(n_acc > 1) <= 0.05, what                 # the reference alone: the rule pins one index for the others
    assert ok.all(), (what, np.flatnonzero(~ok)[:8], pick[~ok][:8])
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(lse[~fin], ref[~fin])
    assert (np.abs(lse - ref)[fin] <= R.bound(q, k, bias, p, centre)[fin]).all(), what
    return pick


@pytest.mark.parametrize("kind", ["plain", "full"])
@pytest.mark.parametrize("n_k", [1, 63, 64, 65, 194, 321])
@pytest.mark.parametrize("n_q", [1, 17, 257])
@pytest.mark.parametrize("d", [1, 4, 5, 32])
def test_picks_are_acceptable(d, n_q, n_k, kind):
    q, k, b, p, u, cen, Q, K = _case(d, n_q, n_k, kind)
    views = dict(dq=_dev(Q)[:, 1:1 + n_q], dk=_dev(K)[:, 3:3 + n_k]) if kind == "full" else {}      # row-strided, 4-byte aligned only
    _check(q, k, b, p, u, cen, f"d={d} n_q={n_q} n_k={n_k} {kind}", **views)


def test_placement_the_ends_of_the_range_and_stratified_uniforms():
    rs = np.random.default_rng(11)
    d, n_k, marks = 4, 194, [0, 63, 128, 193]               # first key, last key of a tile, first key of the second split, last key
    k, b = (0.5 * rs.standard_normal((d, n_k))).astype(np.float32), rs.standard_normal(n_k)
    b[marks] += 6.0                                         # each of the four carries a good share of the mass
    b = (b - np.logaddexp.reduce(b)).astype(np.float32)
    q = np.repeat((0.5 * rs.standard_normal((d, 1))).astype(np.float32), 8, 1)
    W = P.windows(q, k, b, 1.0)[0]
    u = np.array([(W[c] + W[c + 1]) / 2 for c in marks] + [0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24], np.float32)
    assert list(_check(q, k, b, 1.0, u, what="placement")[:7]) == marks + [0, n_k - 1, 0]
    b = np.full(n_k, np.log(1e-6 / (n_k - 1)), np.float32)  # one key carries all but 1e-6 of the mass
    b[100] = 0.0
    q, k, u = np.zeros((d, 64), np.float32), np.zeros((d, n_k), np.float32), ((np.arange(64) + 0.5) / 64).astype(np.float32)
    assert (_check(q, k, b, 1.0, u, what="one heavy key") == 100).all()
    q, k, b, p, _, cen, _, _ = _case(4, 1, 321, "full")     # 256 copies of one query: a cumulative out of key order would show
    pick = _check(np.repeat(q, 256, 1), k, b, p, ((np.arange(256) + 0.5) / 256).astype(np.float32), cen, "stratified")
    assert (np.diff(pick) >= 0).all() and len(set(pick)) > 32


def test_dead_and_poisoned_keys_nan_query_nan_u_and_reproducibility():
    import torch
    from genjax_amd import kernels
    rs = np.random.default_rng(12)
    d, n_q, n_k = 5, 300, 321
    q, k = (0.5 * rs.standard_normal((d, n_q))).astype(np.float32), (0.5 * rs.standard_normal((d, n_k))).astype(np.float32)
    b, u = rs.standard_normal(n_k).astype(np.float32), rs.random(n_q).astype(np.float32)
    dead = np.r_[0, 64:256, n_k - 1]                        # the ends, a whole tile (64 .. 127) and a whole split (128 .. 255)
    b[dead] = np.where(rs.random(len(dead)) < 0.5, np.nan, -np.inf)
    k[:, dead] = np.where(rs.random((d, len(dead))) < 0.5, np.nan, np.inf)
    u[:4] = 0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24
    q[2, 41], u[77] = np.nan, np.nan                        # one bad query, one bad uniform: -1 for these alone
    pick = _check(q, k, b, 0.9, u, what="dead tile and split")
    assert pick[0] == 1 and pick[1] == n_k - 2 and not np.isin(pick, dead).any()
    assert pick[41] == -1 and pick[77] == -1 and (np.delete(pick, [41, 77]) >= 0).all()
    ws = torch.empty(kernels.load().gjx_pairwise_gauss_pick_workspace_bytes(n_q, n_k, d), dtype=torch.uint8, device="cuda")
    two = [kernels.pairwise_gauss_pick(_dev(q), _dev(k), _dev(u), _dev(b), 0.9, ws=ws.fill_(0xFF)) for _ in range(2)]      # 0xFF, twice
    assert np.array_equal(_np(two[0]["pick"]), pick) and torch.equal(two[0]["pick"], two[1]["pick"])
    assert torch.equal(two[0]["lse"].view(torch.int32), two[1]["lse"].view(torch.int32))
    assert (_check(q, k, np.full(n_k, -np.inf, np.float32), 0.9, u, what="all dead") == -1).all()
    k[1, 300] = np.inf                                      # a poisoned live key: nobody picks, and the lse is NaN as the lse call's
    out = kernels.pairwise_gauss_pick(_dev(q), _dev(k), _dev(u), _dev(b), 0.9)
    assert np.isnan(P.windows(q, k, b, 0.9)).all() and (_np(out["pick"]) == -1).all() and np.isnan(_np(out["lse"])).all()


def test_backward_paths_of_a_history():
    import torch
    from genjax_amd import core
    from genjax_amd.inference.pf import LinearGaussianSSM, ParticleHistory
    rs = np.random.default_rng(13)
    T, K, n, key, th = 4, 300, 100, core.key(7), 0.3
    h = ParticleHistory()
    h.ssm = LinearGaussianSSM(np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]], np.float32), 0.5, 1.0)
    for t in range(T):
        lw = rs.standard_normal(K).astype(np.float32)
        lw[rs.integers(0, K, 5)] = -np.inf
        h.append(_dev(rs.standard_normal((2, K))), None, _dev(lw))
    paths, idx = _np(h.backward_paths(key, n)), _np(h.backward_indices)
    x, lw = [_np(a) for a in h.states], [_np(a).astype(np.float64) for a in h.logw_steps]
    assert paths.shape == (T, 2, n) and idx.min() >= 0 and idx.max() < K and np.isfinite(lw[T - 1][idx[T - 1]]).all()
    for t in range(T):
        np.testing.assert_array_equal(paths[t], x[t][:, idx[t]])
    for t in range(T - 2, -1, -1):                          # the kernel's own path: the query is the particle returned at t + 1
        bits = np.array([core.threefry2x32_py(key[0], key[1], t, j)[0] for j in range(n)], np.uint64)
        u = np.minimum(((bits >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24, 1.0 - 2.0 ** -24).astype(np.float32)
        cen = (x[t + 1] * np.exp(lw[t + 1] - np.logaddexp.reduce(lw[t + 1]))).sum(1)
        means = _np(torch.matmul(torch.from_numpy(h.ssm.A).cuda(), h.states[t]))            # the float32 means the kernel saw
        ok, n_acc, _ = P.acceptable(idx[t], x[t + 1][:, idx[t + 1]], means, (lw[t] - np.logaddexp.reduce(lw[t])).astype(np.float32), 4.0, u, cen)
        assert ok.all() and np.mean(n_acc > 1) <= 0.05, t
