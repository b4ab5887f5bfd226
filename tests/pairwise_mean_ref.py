"""float64 NumPy restatement of gjx_pairwise_gauss_mean (the direct |q - k|^2 form) on top of pairwise_ref's log-sum-exp, with the edge
rules of include/gjx.h, and the bound the GPU tests hold the mean to.  Per output (j, r), with E_r = pairwise_ref.bound(...)[r] the
error of a score and u = 2^-24, maximum over LIVE keys with a finite value:
    (2 E_r + u (n_k / 4 + 8)) max_c |v[j][c]|
2 E_r: a relative error E in every unnormalised weight moves a normalised mean by at most 2 E max|v| (numerator and denominator each
move by E).  u (n_k / 4 + 8): the worst case of the chained float32 accumulation of non-negative weights, four keys per matrix
instruction, plus the merge of the splits and the division.  Derived: no measured constant beyond pairwise_ref's own."""
import numpy as np

import pairwise_ref as R


def pairwise_mean(q, k, v, bias, p):
    """q f64[d][n_q], k f64[d][n_k], v f64[dv][n_k], bias [n_k] or None -> (mean f64[dv][n_q], lse f64[n_q])"""
    q, k, v = np.asarray(q, np.float64), np.asarray(k, np.float64), np.asarray(v, np.float64)
    b, live = R._live(bias, k.shape[1])
    mean = np.full((v.shape[0], q.shape[1]), np.nan)
    if live.any() and not np.isfinite(k[:, live]).all():            # a poisoned live key: NaN everywhere
        return mean, np.full(q.shape[1], np.nan)
    lse = R.pairwise_lse(q, k, bias, p)
    if live.any():
        with np.errstate(invalid="ignore"):
            s = b[live][None, :] - 0.5 * p * ((q[:, :, None] - k[:, None, live]) ** 2).sum(0)
            w = np.exp(s - lse[:, None])                             # (a NaN query: a NaN row)
            vl = v[:, live]
            mean = np.where(np.isfinite(vl), vl, 0.0) @ w.T
        mean[~np.isfinite(vl).all(1)] = np.nan                       # a live key's non-finite value: its component, every query
        mean[:, np.isnan(lse)] = np.nan
    return mean, lse


def bound(q, k, v, bias, p, centre=None):
    """-> f64[dv][n_q]"""
    v = np.asarray(v, np.float64)
    _, live = R._live(bias, v.shape[1])
    vmax = np.where(np.isfinite(v) & live[None, :], np.abs(v), 0.0).max(1)
    return (2.0 * R.bound(q, k, bias, p, centre) + R.U * (v.shape[1] / 4.0 + 8.0))[None, :] * vmax[:, None]
