"""gjx_pairwise_t_pick and gjx_pairwise_t_argmax against tests/pairwise_t_pickmax_ref.py (its rules, with the existing C_T and C_SUM), and
backward simulation and the particle Viterbi path under a Student-t transition (dof=) built on them.  The reference alone may accept
more than one key for at most 5 % of the queries POOLED over a case's shapes (at n_q = 1 or 17 one query is more than 5 % of a shape).
64 keys make a staged tile and a chunk, 256 queries a block; 194 keys are two splits, 321 three.  d = 32 with nu = 1 runs at n_k <= 65
only: beyond, the tolerance's factor (nu + d) / nu makes the reference itself ambiguous for 10 - 16 % of the queries."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pairwise_t_pickmax_ref as M
import pairwise_t_ref as T
from test_gpu_pairwise import _dev, _np
from test_gpu_pairwise_pick import _case


def _check(q, k, bias, p, nu, u, centre=None, what="", dq=None, dk=None, ws=None):
    """both calls against their rules; ``dq`` / ``dk``: device views to call with -> (pick, arg, ambiguous picks, ambiguous argmaxes)"""
    from genjax_amd import kernels
    dq, dk = _dev(q) if dq is None else dq, _dev(k) if dk is None else dk
    fill = lambda w: None if w is None else w.fill_(0xFF)
    pk = kernels.pairwise_t_pick(dq, dk, _dev(u), _dev(bias), p, nu, _dev(centre), ws=fill(ws and ws[0]))
    am = kernels.pairwise_t_argmax(dq, dk, _dev(bias), p, nu, _dev(centre), ws=fill(ws and ws[1]))
    pick, lse, arg, mx = _np(pk["pick"]), _np(pk["lse"]), _np(am["arg"]), _np(am["max"])
    ok, n_pick, slack = M.pick_acceptable(pick, q, k, bias, p, nu, u, centre)
    ref, E1 = T.pairwise_t(q, k, bias, p, nu)[0], T.bound(q, k, bias, p, nu, centre)
    fin = np.isfinite(ref)
    err = (np.abs(lse - ref)[fin] / E1[fin]).max(initial=0.0)
    ok_a, n_arg, slack_a, err_a = M.argmax_acceptable(arg, mx, q, k, bias, p, nu, centre)
    print(f"pairwise t {what}: pick slack / tol(C_SUM = 1) = {slack.max():.3f}, lse error / bound(C = 1) = {err:.3f}; "
          f"argmax slack / E(C = 1) = {slack_a:.3f}, max error / E(C = 1) = {err_a:.3f}")
    assert ok.all(), (what, "pick", np.flatnonzero(~ok)[:8], pick[~ok][:8])
    np.testing.assert_array_equal(lse[~fin], ref[~fin])
    assert (np.abs(lse - ref)[fin] <= T.bound(q, k, bias, p, nu, centre, M.C_T)[fin]).all(), (what, "lse")
    assert ok_a.all(), (what, "argmax", np.flatnonzero(~ok_a)[:8], arg[~ok_a][:8])
    assert np.array_equal(lse, _np(kernels.pairwise_t_lse(dq, dk, _dev(bias), p, nu, _dev(centre))), equal_nan=True), (what, "lse bits")
    return pick, arg, int((n_pick > 1).sum()), int((n_arg > 1).sum())


@pytest.mark.parametrize("kind", ["plain", "full"])
@pytest.mark.parametrize("d,nu", [(1, 1.0), (1, 30.0), (4, 1.0), (4, 30.0), (5, 1.0), (5, 30.0), (32, 1.0), (32, 30.0)])
def test_picks_and_argmaxes_are_acceptable(d, nu, kind):
    total = amb_pick = amb_arg = 0
    for n_q in (1, 17, 257):
        for n_k in (1, 63, 64, 65) + (() if (d, nu) == (32, 1.0) else (194, 321)):
            q, k, b, p, u, cen, Q, K = _case(d, n_q, n_k, kind)
            views = dict(dq=_dev(Q)[:, 1:1 + n_q], dk=_dev(K)[:, 3:3 + n_k]) if kind == "full" else {}      # row-strided views
            _, _, a_p, a_a = _check(q, k, b, p, nu, u, cen, f"d={d} nu={nu} n_q={n_q} n_k={n_k} {kind}", **views)
            total, amb_pick, amb_arg = total + n_q, amb_pick + a_p, amb_arg + a_a
    print(f"pairwise t d={d} nu={nu} {kind}: ambiguous picks {amb_pick / total:.3f}, argmaxes {amb_arg / total:.3f}")
    assert amb_pick <= 0.05 * total                         # the reference alone: it pins one key for the others
    # (d = 1 without a bias is the nearest of up to 321 points on a line: the float64 rule itself accepts two keys for 12 - 17 % of
    # the queries, so there the argmax is held to the rule but not to the cap, as test_gpu_pairwise_argmax.py leaves that case out)
    assert amb_arg <= 0.05 * total or (d, kind) == (1, "plain")


def test_exact_ties_go_to_the_smallest_index():
    from genjax_amd import kernels
    q, k, b, p, _, cen, _, _ = _case(5, 257, 194, "full")
    call = lambda k, b: _np(kernels.pairwise_t_argmax(_dev(q), _dev(k), _dev(b), p, 3.0, _dev(cen))["arg"])
    two = lambda a: np.concatenate([a, a], -1)              # the key set twice: the copy's values are the same bits 194 keys later
    arg = call(two(k), two(b))
    assert (arg >= 0).all() and (arg < 194).all()
    marks = [0, 63, 64, 128]                                # one key at the start, a tile's edge and the second split, with the largest bias
    k, b = k.copy(), b.copy()
    k[:, marks], b[marks] = k[:, :1], b.max() + 50.0
    assert (call(k, b) == 0).all()


def test_placement_the_ends_of_the_range_and_stratified_uniforms():
    rs = np.random.default_rng(11)
    d, n_k, nu, marks = 4, 194, 3.0, [0, 63, 128, 193]      # first key, last key of a tile, first key of the second split, last key
    k, b = (0.5 * rs.standard_normal((d, n_k))).astype(np.float32), rs.standard_normal(n_k)
    b[marks] += 6.0                                         # each of the four carries a good share of the mass
    b = (b - np.logaddexp.reduce(b)).astype(np.float32)
    q = np.repeat((0.5 * rs.standard_normal((d, 1))).astype(np.float32), 8, 1)
    s = M.scores(q, k, b, 1.0, nu)[0][0]
    W = np.r_[0.0, np.cumsum(np.exp(s - s.max())) / np.exp(s - s.max()).sum()]
    u = np.array([(W[c] + W[c + 1]) / 2 for c in marks] + [0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24], np.float32)
    assert list(_check(q, k, b, 1.0, nu, u, what="placement")[0][:7]) == marks + [0, n_k - 1, 0]
    q, k, b, p, _, cen, _, _ = _case(4, 1, 321, "full")     # 256 copies of one query: a cumulative out of key order would show
    pick = _check(np.repeat(q, 256, 1), k, b, p, nu, ((np.arange(256) + 0.5) / 256).astype(np.float32), cen, "stratified")[0]
    assert (np.diff(pick) >= 0).all() and len(set(pick)) > 32


@pytest.mark.parametrize("kind", ["dead", "all dead", "nan query", "nan u", "poisoned key", "inf bias"])
def test_edges_and_reproducibility(kind):
    import torch
    from genjax_amd import kernels
    rs = np.random.default_rng(12)
    d, n_q, n_k, p, nu = 5, 300, 321, 0.9, 3.0
    q, k = (0.5 * rs.standard_normal((d, n_q))).astype(np.float32), (0.5 * rs.standard_normal((d, n_k))).astype(np.float32)
    b, u = rs.standard_normal(n_k).astype(np.float32), rs.random(n_q).astype(np.float32)
    dead = np.r_[0, 64:256, n_k - 1]                        # the ends, a whole tile (64 .. 127) and a whole split (128 .. 255)
    b[dead] = np.where(rs.random(len(dead)) < 0.5, np.nan, -np.inf)
    k[:, dead] = np.where(rs.random((d, len(dead))) < 0.5, np.nan, np.inf)
    u[:4] = 0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24
    if kind == "all dead":
        b[:] = -np.inf
    q[2, 41] = np.nan if kind == "nan query" else q[2, 41]
    u[77] = np.nan if kind == "nan u" else u[77]
    k[1, 300] = np.inf if kind == "poisoned key" else k[1, 300]
    b[2] = np.inf if kind == "inf bias" else b[2]
    ws = [torch.empty(n(n_q, n_k, d), dtype=torch.uint8, device="cuda")
          for n in (kernels.load().gjx_pairwise_gauss_pick_workspace_bytes, kernels.load().gjx_pairwise_t_argmax_workspace_bytes)]
    one, two = (_check(q, k, b, p, nu, u, what=kind, ws=ws) for _ in range(2))             # workspace of 0xFF, twice
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    none = M.nothing(q, k, b)
    assert not np.isin(one[0], dead).any() and not np.isin(one[1], dead).any()
    assert np.array_equal(one[1] == -1, none) and np.array_equal(one[0] == -1, none | np.isnan(u))
    assert none.sum() == {"dead": 0, "nan u": 0, "nan query": 1}.get(kind, n_q)
    if kind == "dead":
        assert one[0][0] == 1 and one[0][1] == n_k - 2


def test_backward_paths_and_map_path_under_a_t_transition():
    from genjax_amd import core, kernels
    rs = np.random.default_rng(13)
    T_, K, n, d, p, nu, key = 4, 300, 100, 2, 4.0, 3.0, core.key(7)
    x, lw32 = ([rs.standard_normal(s).astype(np.float32) for _ in range(T_)] for s in ((d, K), K))
    for a in lw32:
        a[rs.integers(0, K, 5)] = -np.inf
    means, lw = [(0.9 * a).astype(np.float32) for a in x], [a.astype(np.float64) for a in lw32]
    dev = lambda rows: [_dev(a) for a in rows]
    res = kernels.ffbs_sample_paths(dev(x), dev(lw32), dev(means), p, key, n, dof=nu)
    paths, idx = _np(res["paths"]), _np(res["idx"])
    assert paths.shape == (T_, d, n) and idx.min() >= 0 and idx.max() < K and np.isfinite(lw[T_ - 1][idx[T_ - 1]]).all()
    for t in range(T_):
        np.testing.assert_array_equal(paths[t], x[t][:, idx[t]])
    for t in range(T_ - 2, -1, -1):                         # the kernel's own path: the query is the particle returned at t + 1
        bits = np.array([core.threefry2x32_py(key[0], key[1], t, j)[0] for j in range(n)], np.uint64)
        u = np.minimum(((bits >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24, 1.0 - 2.0 ** -24).astype(np.float32)
        cen = (x[t + 1] * np.exp(lw[t + 1] - np.logaddexp.reduce(lw[t + 1]))).sum(1)
        ok, n_acc, _ = M.pick_acceptable(idx[t], x[t + 1][:, idx[t + 1]], means[t], (lw[t] - np.logaddexp.reduce(lw[t])).astype(np.float32),
                                         p, nu, u, cen)
        assert ok.all() and np.mean(n_acc > 1) <= 0.05, t
    res = kernels.ffbs_map_path(dev(x), dev(lw32), dev(means), p, dof=nu)          # the same history, its weights as log-likelihoods
    idx, path = _np(res["idx"]), _np(res["path"])
    best, own, slack = M.viterbi(x, lw, means, np.zeros(K), p, nu, idx)
    print(f"t viterbi: optimum {best:.6f}, returned path {own:.6f}, log_joint {float(res['log_joint']):.6f}, slack {slack:.2e}")
    assert idx.min() >= 0 and idx.max() < K and np.isfinite(lw[T_ - 1][idx[T_ - 1]])
    assert own >= best - slack and abs(float(res["log_joint"]) - own) <= slack
    for t in range(T_):
        np.testing.assert_array_equal(path[t], x[t][:, idx[t]])
