"""The definition of gjx_weighted_cross_moments (include/gjx.h), restated in float64 NumPy on the float32 inputs, for the tests:
particle i is the pair (rows_a[:, i], rows_b[:, index[i]]) under the self-normalised weight exp(logw_i); dead particles (weight -inf
or NaN) and live particles whose index is outside [0, K_b) are removed before anything is summed.

Tolerances are those of tests/test_gpu_moments.py (``Ref``, imported: the same arithmetic on the device): the means take tol_mean
(eps range + 2^-22 |mean|), the cross-moments  tol_cross = eps range_a (x) range_b + 2^-40 |mean_a (x) mean_b|,  eps = 1e-4 — the
covariance tolerance with the two ranges and the two means of the pair."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_moments import EPS, Ref


class CrossRef:
    def __init__(self, rows_a, rows_b, logw=None, index=None):
        a, b = np.atleast_2d(np.asarray(rows_a)), np.atleast_2d(np.asarray(rows_b))
        K, K_b = a.shape[1], b.shape[1]
        idx = np.arange(K) if index is None else np.asarray(index).astype(np.int64)
        live = np.ones(K, bool) if logw is None else np.isfinite(np.asarray(logw, np.float64))
        bad = live & ((idx < 0) | (idx >= K_b))
        keep = live & ~bad
        self.n_bad, self.keep = int(bad.sum()), keep
        self.a, self.b = a[:, keep], b[:, idx[keep]]
        n_a, n_b = a.shape[0], b.shape[0]
        if not keep.any():
            self.stats = np.array([-np.inf, 0.0, 0.0, 0.0])
            self.mean_a, self.mean_b, self.cross = np.full(n_a, np.nan), np.full(n_b, np.nan), np.full((n_a, n_b), np.nan)
            return
        lw = None if logw is None else np.asarray(logw)[keep]
        ra, rb = Ref(self.a, lw), Ref(self.b, lw)
        self.stats, self.mean_a, self.mean_b = ra.stats, ra.mean, rb.mean
        self.w = np.ones(int(keep.sum())) / keep.sum() if lw is None else np.exp(lw.astype(np.float64) - lw.astype(np.float64).max())
        self.w = self.w / self.w.sum()
        da = self.a.astype(np.float64) - ra.mean[:, None]
        db = self.b.astype(np.float64) - rb.mean[:, None]
        self.cross = (da * self.w) @ db.T
        self.range_a, self.range_b = ra.range, rb.range
        self.tol_mean_a, self.tol_mean_b = ra.tol_mean, rb.tol_mean
        self.tol_cross = EPS * np.outer(ra.range, rb.range) + 2.0 ** -40 * np.abs(np.outer(ra.mean, rb.mean))


def traced_pair_moments(x, anc, w_last):
    """the lag-one pair moments by following every last-step particle's lineage back: x f64[T][d][K] (step t's stored particles),
    anc i[T-1][K], w_last f64[K] (sum 1) -> (mean [T-1][d], mean_prev [T-1][d], cross [T-1][d][d]); entry t-1 is the pair
    (x_t, x_{t-1}) of the paths, each path weighted by its last particle"""
    T, d, K = x.shape
    idx = np.empty((T, K), np.int64)
    idx[T - 1] = np.arange(K)
    for t in range(T - 1, 0, -1):
        idx[t - 1] = anc[t - 1][idx[t]]
    mean, prev, cross = np.empty((T - 1, d)), np.empty((T - 1, d)), np.empty((T - 1, d, d))
    for t in range(1, T):
        xa, xb = x[t][:, idx[t]], x[t - 1][:, idx[t - 1]]
        mean[t - 1], prev[t - 1] = xa @ w_last, xb @ w_last
        cross[t - 1] = ((xa - mean[t - 1][:, None]) * w_last) @ (xb - prev[t - 1][:, None]).T
    return mean, prev, cross
