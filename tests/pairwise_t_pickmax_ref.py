"""float64 NumPy restatement of gjx_pairwise_t_pick and gjx_pairwise_t_argmax (the direct |q - k|^2 form of pairwise_t_ref.pairwise_t)
and the rules the GPU tests hold them to, with E_r = pairwise_t_ref.bound(..., C_T)[r]:
  pick    pairwise_pick_ref.acceptable's rule on the t windows: a live key c is accepted for u_r iff
          P_r(c - 1) - tol_r <= u_r <= P_r(c) + tol_r,   tol_r = 2 E_r + C_SUM U log2(n_k + 1)
  argmax  arg[r] is a live key with s64[r, arg] >= max64[r] - 2 E_r, and |max[r] - max64[r]| <= E_r
C_T and C_SUM are the measured constants of the t lse and of the Gaussian pick: imported, not copied."""
import numpy as np

import pairwise_ref as R
import pairwise_t_ref as T
from pairwise_pick_ref import C_SUM, U
from test_gpu_pairwise_t import C_T


def scores(q, k, bias, p, nu):
    """-> s64[n_q][n_k] (-inf for a dead key), live bool[n_k]"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    b, live = R._live(bias, k.shape[1])
    with np.errstate(all="ignore"):
        s = b[None, :] - 0.5 * (nu + q.shape[0]) * np.log1p(p * ((q[:, :, None] - k[:, None, :]) ** 2).sum(0) / nu)
    return np.where(live[None, :], s, -np.inf), live


def nothing(q, k, bias, u=None):
    """-> bool[n_q]: no answer for the query (no live key, a poisoned live key or a +inf bias, a non-finite query, a NaN u): where the
    restated lse is not finite"""
    with np.errstate(all="ignore"):
        return ~np.isfinite(T.pairwise_t(q, k, bias, 1.0, 1.0)[0]) | (False if u is None else np.isnan(np.asarray(u, np.float64)))


def pick_acceptable(pick, q, k, bias, p, nu, u, centre=None, c_sum=C_SUM):
    """-> (ok bool[n_q], n_accepted int[n_q], slack f64[n_q] in units of tol(C_SUM = 1)), as pairwise_pick_ref.acceptable"""
    pick, none = np.asarray(pick), nothing(q, k, bias, u)
    u = np.clip(np.nan_to_num(np.asarray(u, np.float64)), 0.0, 1.0)
    s, live = scores(q, k, bias, p, nu)
    with np.errstate(all="ignore"):
        e = np.where(live[None, :], np.exp(s - s.max(1, keepdims=True)), 0.0)
        P = np.concatenate([np.zeros((len(u), 1)), np.cumsum(e, 1) / e.sum(1, keepdims=True)], 1)
    E = 2.0 * T.bound(q, k, bias, p, nu, centre, C_T)
    tol, tol1 = (E + c * U * np.log2(len(live) + 1.0) for c in (c_sum, 1.0))
    with np.errstate(invalid="ignore"):
        inside = live[None, :] & (P[:, :-1] - tol[:, None] <= u[:, None]) & (u[:, None] <= P[:, 1:] + tol[:, None]) & ~none[:, None]
        rows, c = np.arange(len(pick)), np.clip(pick, 0, len(live) - 1)
        out = np.maximum(np.maximum(P[rows, c] - u, u - P[rows, c + 1]), 0.0)
    ok = np.where(none, pick == -1, (pick >= 0) & inside[rows, c])
    return ok, inside.sum(1), np.where(none | (pick < 0), 0.0, out / tol1)


def argmax_acceptable(arg, mx, q, k, bias, p, nu, centre=None):
    """-> (ok bool[n_q], n_accepted int[n_q], worst (max64 - s64[arg]) / E(C = 1), worst |max - max64| / E(C = 1))"""
    arg, mx, none = np.asarray(arg), np.asarray(mx, np.float64), nothing(q, k, bias)
    (s, live), E, E1 = scores(q, k, bias, p, nu), T.bound(q, k, bias, p, nu, centre, C_T), T.bound(q, k, bias, p, nu, centre, 1.0)
    top, rows = s.max(1), np.arange(len(arg))
    with np.errstate(invalid="ignore"):
        acc = live[None, :] & (s >= (top - 2.0 * E)[:, None]) & ~none[:, None]
        got = s[rows, np.clip(arg, 0, len(live) - 1)]
        empty = ~live.any() & np.isfinite(np.asarray(q, np.float64)).all(0)     # nobody lives: -inf for a good query, NaN elsewhere
        ok = np.where(none, (arg == -1) & np.where(empty, mx == -np.inf, np.isnan(mx)),
                      (arg >= 0) & acc[rows, np.clip(arg, 0, len(live) - 1)] & (np.abs(mx - top) <= E))
        fin = ~none & (arg >= 0)
        slack, err = ((top - got) / E1)[fin], (np.abs(mx - top) / E1)[fin]
    return ok, acc.sum(1), slack.max(initial=0.0), err.max(initial=0.0)


def viterbi(x, ll, means, prior, p, nu, idx):
    """the float64 dynamic programme over the t transition without its constants -> (optimum, the log joint of the path ``idx``, the
    summed 2 E slack of the steps' calls)"""
    T_, K = len(x), x[0].shape[1]
    delta, own, slack = prior + ll[0], prior[idx[0]] + ll[0][idx[0]], 0.0
    for t in range(1, T_):
        s, _ = scores(x[t], means[t - 1], np.zeros(K), p, nu)
        cen = (x[t] * np.exp(ll[t] - np.logaddexp.reduce(ll[t]))).sum(1)
        slack += 2 * T.bound(x[t], means[t - 1], delta, p, nu, cen, C_T)[ll[t] > -np.inf].max()
        own += ll[t][idx[t]] + s[idx[t], idx[t - 1]]
        delta = ll[t] + (delta[None, :] + s).max(1)
    return delta.max(), own, slack
