"""float64 NumPy restatement of gjx_pairwise_t_lse and gjx_pairwise_t_mean (the direct |q - k|^2 form, not the kernel's expansion) with
the edge rules of include/gjx.h, the FFBSm recursion on it, and the bounds the GPU tests hold the kernels to.  Per lse output r (u =
2^-24, tildes: minus the call's centre, maximum over LIVE keys, a = (nu + d) / 2):
    C u [(d + 4) p (|q~_r|^2 + max_c |k~_c|^2) (nu + d) / nu  +  (nu + d)]  +  8 u (1 + log n_k)
First term: the kernel's x = p |q - k|^2 / nu carries the Gaussian calls' cancellation error over nu, and a log(1 + x) has slope at most
a in x.  Second: the rounding of 1 + x in front of the logarithm, times a.  Third: pairwise_ref's (bias, hardware exp and log).  The mean
is held to pairwise_mean_ref's form on that error.  C is the one measured constant (tests/test_gpu_pairwise_t.py)."""
import numpy as np

import pairwise_ref as R


def pairwise_t(q, k, bias, p, nu, v=None):
    """q f64[d][n_q], k f64[d][n_k], bias [n_k] or None, v f64[dv][n_k] or None -> (lse f64[n_q], mean f64[dv][n_q] or None)"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    v = None if v is None else np.asarray(v, np.float64)
    (d, n_q), (b, live) = q.shape, R._live(bias, k.shape[1])
    lse = np.full(n_q, -np.inf)
    mean = None if v is None else np.full((v.shape[0], n_q), np.nan)
    if live.any() and not (np.isfinite(k[:, live]).all() and (b[live] < np.inf).all()):      # a poisoned live key: NaN everywhere
        return np.full(n_q, np.nan), mean
    if live.any():
        with np.errstate(invalid="ignore"):
            s = b[live][None, :] - 0.5 * (nu + d) * np.log1p(p * ((q[:, :, None] - k[:, None, live]) ** 2).sum(0) / nu)
            m = s.max(1)
            lse = m + np.log(np.exp(s - m[:, None]).sum(1))
            if v is not None:
                vl = v[:, live]
                mean = np.where(np.isfinite(vl), vl, 0.0) @ np.exp(s - lse[:, None]).T
                mean[~np.isfinite(vl).all(1)] = np.nan                  # a live key's non-finite value: its component, every query
    bad = ~np.isfinite(q).all(0)                                        # a bad query: NaN for it alone
    lse[bad] = np.nan
    if v is not None:
        mean[:, bad] = np.nan
    return lse, mean


def bound(q, k, bias, p, nu, centre=None, c=1.0):
    """the lse's -> f64[n_q]"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    d = q.shape[0]
    cen = np.zeros((d, 1)) if centre is None else np.asarray(centre, np.float64).reshape(-1, 1)
    _, live = R._live(bias, k.shape[1])
    k2 = ((k[:, live] - cen) ** 2).sum(0).max() if live.any() else 0.0
    return c * R.U * ((d + R.C0) * p * (((q - cen) ** 2).sum(0) + k2) * (nu + d) / nu + (nu + d)) + R.C1 * R.U * (1.0 + np.log(k.shape[1]))


def mean_bound(lse_bound, v, bias):
    """the mean's, from the lse's (pairwise_mean_ref.bound's form) -> f64[dv][n_q]"""
    v = np.asarray(v, np.float64)
    _, live = R._live(bias, v.shape[1])
    vmax = np.where(np.isfinite(v) & live[None, :], np.abs(v), 0.0).max(1)
    return (2.0 * lse_bound + R.U * (v.shape[1] / 4.0 + 8.0))[None, :] * vmax[:, None]


def ffbs_log_weights(states, logw, means, p, nu):
    """pairwise_ref.ffbs_log_weights under the t transition -> log w_{t|T}, f64[T][K], every row normalised"""
    norm = lambda lw: lw - np.logaddexp.reduce(lw)
    T = len(states)
    out = [None] * T
    out[T - 1] = norm(np.asarray(logw[T - 1], np.float64))
    for t in range(T - 2, -1, -1):
        lw = norm(np.asarray(logw[t], np.float64))
        D = pairwise_t(states[t + 1], means[t], lw, p, nu)[0]
        out[t] = norm(lw + pairwise_t(means[t], states[t + 1], out[t + 1] - D, p, nu)[0])
    return np.stack(out)
