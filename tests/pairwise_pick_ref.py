"""float64 NumPy restatement of gjx_pairwise_gauss_pick on top of pairwise_ref (the direct |q - k|^2 form) and the rule the GPU tests
hold a pick to.  The kernel draws by inverse CDF in key-index order, so the restatement knows nothing of tiles, chunks or splits:
P_r(c) is the normalised cumulative over keys 0 .. c (dead keys add 0), and a pick c is ACCEPTED for the uniform u_r iff key c is live and
    P_r(c - 1) - tol_r <= u_r <= P_r(c) + tol_r,     tol_r = 2 pairwise_ref.bound(...)[r] + C_SUM U log2(n_k + 1).
First term: a score error E moves every e_rc by a relative E, in the numerator and in the total.  Second term: the float32 sums of the
cumulative and of the total (chunks of 64 keys, then tiles, then splits: depth about log2 n_k).  C_SUM is the one measured constant, by
the convention of pairwise_ref.py: 4 x the worst |u_r - nearest edge of the picked key's window| / (tol_r with C_SUM = 1) seen on an
MI355X over the shape grid of tests/test_gpu_pairwise_pick.py.  u <= 0 and u >= 1 are the ends of the range, as the header says."""
import numpy as np

import pairwise_ref as R

U = R.U
C_SUM_MEASURED = 0.04         # worst slack / tol(C_SUM = 1) on an MI355X: 0.031 (d = 1, n_q = 257, n_k = 321, no bias), rounded up
C_SUM = 4.0 * C_SUM_MEASURED


def windows(q, k, bias, p, u=None):
    """-> P f64[n_q][n_k + 1], P[r][c + 1] = P_r(c), P[r][0] = 0; NaN rows where there is nothing to pick (no live key, a poisoned
    live key, a non-finite query, and with ``u`` a NaN u_r)"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    b, live = R._live(bias, k.shape[1])
    P = np.full((q.shape[1], k.shape[1] + 1), np.nan)
    if live.any():
        with np.errstate(invalid="ignore"):
            s = b[live][None, :] - 0.5 * p * ((q[:, :, None] - k[:, None, live]) ** 2).sum(0)
            e = np.zeros((q.shape[1], k.shape[1]))
            e[:, live] = np.exp(s - s.max(1, keepdims=True))
        P[:, 0] = 0.0
        P[:, 1:] = np.cumsum(e, 1) / e.sum(1, keepdims=True)
    P[~np.isfinite(q).all(0)] = np.nan
    if not np.isfinite(k[:, live]).all():                  # a poisoned live key: nobody picks
        P[:] = np.nan
    if u is not None:
        P[np.isnan(np.asarray(u, np.float64))] = np.nan
    return P


def tolerance(q, k, bias, p, centre=None, c_sum=C_SUM):
    return 2.0 * R.bound(q, k, bias, p, centre) + c_sum * U * np.log2(np.asarray(k).shape[1] + 1.0)


def acceptable(pick, q, k, bias, p, u, centre=None, c_sum=C_SUM):
    """-> (ok bool[n_q], n_accepted int[n_q]: how many keys the rule accepts for the query, slack f64[n_q]: the distance of u_r from the
    nearest edge of the pick's window in units of tol_r(C_SUM = 1), 0 inside)"""
    pick, u = np.asarray(pick), np.clip(np.asarray(u, np.float64), 0.0, 1.0)
    P, tol = windows(q, k, bias, p, u), tolerance(q, k, bias, p, centre, c_sum)
    _, live = R._live(bias, np.asarray(k).shape[1])
    none = np.isnan(P[:, 0])
    with np.errstate(invalid="ignore"):
        inside = live[None, :] & (P[:, :-1] - tol[:, None] <= u[:, None]) & (u[:, None] <= P[:, 1:] + tol[:, None])
    rows, c = np.arange(len(pick)), np.clip(pick, 0, P.shape[1] - 2)
    ok = np.where(none, pick == -1, (pick >= 0) & inside[rows, c])
    with np.errstate(invalid="ignore"):
        out = np.maximum(np.maximum(P[rows, c] - u, u - P[rows, c + 1]), 0.0)
    slack = np.where(none | (pick < 0), 0.0, out / tolerance(q, k, bias, p, centre, 1.0))
    return ok, inside.sum(1), slack
