"""gjx_pairwise_gauss_argmax (and _diag) against the direct form in float64 on the same float32 numbers, and the particle Viterbi path
built on it against a float64 dynamic programme.  With E_r the lse's score bound (pairwise_ref.bound; the diagonal call: the bound of
test_gpu_pairwise_diag.py) a result passes when arg[r] is a live key with s64[r, arg] >= max64[r] - 2 E_r and |max[r] - max64[r]| <= E_r;
in every case the reference alone may accept more than one key for at most 5 % of the queries.  64 keys make a staged tile, 256
queries a block; 194 keys are two splits, 321 three."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pairwise_ref as R
import test_gpu_pairwise_diag as D
from test_gpu_pairwise import _dev, _np
from test_gpu_pairwise_pick import _case


def _scores(q, k, bias, p):
    """s64[r][c], -inf for a dead key; ``p`` a number or the keys' precision matrix [d][n_k]"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    b, live = R._live(bias, k.shape[1])
    P = np.asarray(p, np.float64)[:, None, :] if np.ndim(p) else p
    with np.errstate(all="ignore"):
        s = b[None, :] - 0.5 * (P * (q[:, :, None] - k[:, None, :]) ** 2).sum(0)
    return np.where(live[None, :], s, -np.inf)


def _bound(q, k, bias, p, centre, **c):
    if np.ndim(p):
        return D.bound(q, k, bias, p, "keys", np.zeros(len(q)) if centre is None else centre, **c)
    return R.bound(q, k, bias, p, centre, **c)


def _check(q, k, bias, p, centre=None, what="", dq=None, dk=None):
    """one call against the rule; ``dq`` / ``dk``: device views to call with in place of copies.  Returns (arg, max)."""
    from genjax_amd import kernels
    out = kernels.pairwise_gauss_argmax(_dev(q) if dq is None else dq, _dev(k) if dk is None else dk, _dev(bias),
                                        _dev(p) if np.ndim(p) else p, _dev(centre))
    arg, mx, s, E = _np(out["arg"]), _np(out["max"]).astype(np.float64), _scores(q, k, bias, p), _bound(q, k, bias, p, centre)
    E1 = _bound(q, k, bias, p, centre, c=1.0)
    acc = s >= (s.max(1) - 2 * E)[:, None]
    got = s[np.arange(len(arg)), arg]
    print(f"pairwise argmax {what}: worst slack / E(C = 1) = {((s.max(1) - got) / E1).max():.3f}, "
          f"max error / E(C = 1) = {(np.abs(mx - s.max(1)) / E1).max():.3f}, ambiguous {np.mean(acc.sum(1) > 1):.3f}")
    assert np.mean(acc.sum(1) > 1) <= 0.05, what            # the reference alone: it pins one key for the others
    assert (arg >= 0).all() and acc[np.arange(len(arg)), arg].all(), (what, np.flatnonzero(~acc[np.arange(len(arg)), arg])[:8])
    assert (np.abs(mx - s.max(1)) <= E).all(), what
    return arg, mx


@pytest.mark.parametrize("d,kind", [(1, "full"), (4, "plain"), (4, "full"), (5, "plain"), (5, "full"), (32, "plain"), (32, "full")])
@pytest.mark.parametrize("n_k", [1, 63, 64, 65, 194, 321])
@pytest.mark.parametrize("n_q", [1, 17, 257])
def test_argmax_is_acceptable(d, n_q, n_k, kind):
    q, k, b, p, _, cen, Q, K = _case(d, n_q, n_k, kind)
    views = dict(dq=_dev(Q)[:, 1:1 + n_q], dk=_dev(K)[:, 3:3 + n_k]) if kind == "full" else {}      # row-strided, 4-byte aligned only
    _check(q, k, b, p, cen, f"d={d} n_q={n_q} n_k={n_k} {kind}", **views)


@pytest.mark.parametrize("n_k", [65, 321])
@pytest.mark.parametrize("n_q", [17, 257])
@pytest.mark.parametrize("d", [1, 5, 16])
def test_diagonal_precisions(d, n_q, n_k):
    q, k, b, p, _, cen, _, _ = _case(d, n_q, n_k, "full")
    prec = (10.0 ** np.random.default_rng(d + n_q + n_k).uniform(-1, 1, (d, n_k))).astype(np.float32)
    _check(q, k, b, prec, cen, f"diag d={d} n_q={n_q} n_k={n_k}")
    if (n_q, n_k) == (257, 321):                            # a constant table agrees with the scalar call inside the two bounds
        const = np.full((d, n_k), p, np.float32)
        (_, m_iso), (_, m_diag) = _check(q, k, b, p, cen, "iso"), _check(q, k, b, const, cen, "constant table")
        assert (np.abs(m_iso - m_diag) <= _bound(q, k, b, p, cen) + _bound(q, k, b, const, cen)).all()


@pytest.mark.parametrize("diag", [False, True])
def test_exact_ties_go_to_the_smallest_index(diag):
    q, k, b, p, _, cen, _, _ = _case(5, 257, 194, "full")
    from genjax_amd import kernels
    prec = (10.0 ** np.random.default_rng(3).uniform(-1, 1, k.shape)).astype(np.float32) if diag else None
    call = lambda k, b, P: _np(kernels.pairwise_gauss_argmax(_dev(q), _dev(k), _dev(b), _dev(P) if diag else p, _dev(cen))["arg"])
    two = lambda a: np.concatenate([a, a], -1)              # the key set twice: the copy's scores are the same bits 194 keys later
    arg = call(two(k), two(b), two(prec) if diag else None)
    assert (arg >= 0).all() and (arg < 194).all()
    marks = [0, 63, 64, 128]                                # one key at the start, a tile's edge and the second split, with the largest bias
    k, b = k.copy(), b.copy()
    k[:, marks], b[marks] = k[:, :1], b.max() + 50.0
    if diag:
        prec[:, marks] = prec[:, :1]
    assert (call(k, b, prec) == 0).all()


def test_dead_and_poisoned_keys_nan_query_inf_bias_and_reproducibility():
    import torch
    from genjax_amd import kernels
    rs = np.random.default_rng(12)
    d, n_q, n_k = 5, 300, 321
    q, k = (0.5 * rs.standard_normal((d, n_q))).astype(np.float32), (0.5 * rs.standard_normal((d, n_k))).astype(np.float32)
    b = rs.standard_normal(n_k).astype(np.float32)
    dead = np.r_[0, 64:256, n_k - 1]                        # the ends, a whole tile (64 .. 127) and a whole split (128 .. 255)
    b[dead] = np.where(rs.random(len(dead)) < 0.5, np.nan, -np.inf)
    k[:, dead] = np.where(rs.random((d, len(dead))) < 0.5, np.nan, np.inf)
    arg, mx = _check(q, k, b, 0.9, what="dead tile and split")
    assert not np.isin(arg, dead).any()
    ws = torch.empty(kernels.load().gjx_pairwise_gauss_argmax_workspace_bytes(n_q, n_k, d), dtype=torch.uint8, device="cuda")
    for P in (0.9, _dev(np.full((d, n_k), 0.9))):           # both kernels
        call = lambda q, k, b, **kw: kernels.pairwise_gauss_argmax(_dev(q), _dev(k), _dev(b), P, **kw)
        two = [call(q, k, b, ws=ws.fill_(0xFF)) for _ in range(2)]                    # 0xFF, twice
        assert torch.equal(two[0]["arg"], two[1]["arg"]) and torch.equal(two[0]["max"].view(torch.int32), two[1]["max"].view(torch.int32))
        assert not isinstance(P, float) or (np.array_equal(_np(two[0]["arg"]), arg) and np.array_equal(_np(two[0]["max"]), mx.astype(np.float32)))
        out = call(q, k, np.full(n_k, -np.inf, np.float32))                           # all dead
        assert (_np(out["arg"]) == -1).all() and (_np(out["max"]) == -np.inf).all()
        q2 = q.copy()
        q2[2, 41] = np.nan                                                            # one bad query: -1 / NaN for it alone
        out = call(q2, k, b)
        bad = np.arange(n_q) == 41
        assert np.array_equal(_np(out["arg"])[~bad], _np(two[0]["arg"])[~bad]) and _np(out["arg"])[41] == -1
        assert np.array_equal(np.isnan(_np(out["max"])), bad)
        k2, b2 = k.copy(), b.copy()
        k2[1, 300], b2[2] = np.inf, np.inf                                            # a poisoned live key; a +inf bias: everybody
        for out in (call(q, k2, b), call(q, k, b2)):
            assert (_np(out["arg"]) == -1).all() and np.isnan(_np(out["max"])).all()


def _viterbi_check(res, x, ll, means, prior, P):
    """the returned path against the float64 optimum over the same float32 inputs; ``P`` a number or the per-step list of tables"""
    T, K = len(x), x[0].shape[1]
    idx, path = _np(res["idx"]), _np(res["path"])
    delta, own, slack = prior + ll[0], prior[idx[0]] + ll[0][idx[0]], 0.0
    for t in range(1, T):
        p = P[t - 1] if isinstance(P, list) else P
        s = _scores(x[t], means[t - 1], np.zeros(K), p) + (0.5 * np.log(np.float64(p)).sum(0)[None, :] if np.ndim(p) else 0.0)
        cen = (x[t] * np.exp(ll[t] - np.logaddexp.reduce(ll[t]))).sum(1)
        slack += 2 * _bound(x[t], means[t - 1], delta, p, cen)[ll[t] > -np.inf].max()
        own += ll[t][idx[t]] + s[idx[t], idx[t - 1]]
        delta = ll[t] + (delta[None, :] + s).max(1)
    print(f"viterbi: optimum {delta.max():.6f}, returned path {own:.6f}, log_joint {float(res['log_joint']):.6f}, slack {slack:.2e}")
    assert idx.min() >= 0 and idx.max() < K and np.isfinite(ll[T - 1][idx[T - 1]])
    assert own >= delta.max() - slack and abs(float(res["log_joint"]) - own) <= slack
    for t in range(T):
        np.testing.assert_array_equal(path[t], x[t][:, idx[t]])


def test_map_path_of_a_history_and_per_step_precisions():
    import torch
    from genjax_amd import kernels
    from genjax_amd.inference.pf import LinearGaussianSSM, ParticleHistory
    rs = np.random.default_rng(13)
    T, K, th = 4, 300, 0.3
    h = ParticleHistory()
    h.ssm = LinearGaussianSSM(np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]], np.float32), 0.5, 1.0)
    for t in range(T):
        lw = rs.standard_normal(K).astype(np.float32)
        lw[rs.integers(0, K, 5)] = -np.inf
        h.append(_dev(rs.standard_normal((2, K))), None, _dev(lw))
    path = h.map_path()
    means_d = [torch.matmul(torch.from_numpy(h.ssm.A).cuda(), s) for s in h.states]       # the float32 means the kernel saw
    x, ll, means = [_np(a) for a in h.states], [_np(a).astype(np.float64) for a in h.logw_steps], [_np(a) for a in means_d]
    prior = _np((h.states[0] * h.states[0]).sum(0) * (-0.5 / (h.ssm.q0 * h.ssm.q0))).astype(np.float64)
    _viterbi_check(dict(idx=h.map_indices, path=path, log_joint=h.map_log_joint), x, ll, means, prior, 4.0)
    P = [np.stack([1.0 / (0.1 + x[t][0] ** 2), np.full(K, 2.0)]).astype(np.float32) for t in range(2)] + [np.tile(np.float32([[0.5], [2.0]]), K)]
    res = kernels.ffbs_map_path(h.states, h.logw_steps, means_d, [_dev(P[0]), _dev(P[1]), _dev(P[2][:, 0]), None])
    _viterbi_check(res, x, ll, means, np.zeros(K), P)
