"""The definition of gjx_pareto_smooth (include/gjx.h) restated in NumPy: float32 log-weights in, a stable argsort of the keys,
everything else in float64, one rounding to float32 at the end.  Pareto smoothed importance sampling: Vehtari, Simpson, Gelman, Yao,
Gabry; the fit is Zhang & Stephens (2009) with the paper's priors."""
import math

import numpy as np


def tail_size(n: int) -> int:
    """M = min(floor(n / 5), ceil(3 sqrt(n))), the ceiling in integers: ceil(sqrt(9 n))"""
    return min(n // 5, math.isqrt(9 * n - 1) + 1) if n > 0 else 0


def keys(lw: np.ndarray) -> np.ndarray:
    """the order-preserving uint32 key of gjx_weighted_quantiles (-0.0 folded onto +0.0); 0, below every live key, for a dead
    particle (-inf, NaN)"""
    lw = np.ascontiguousarray(lw, np.float32)
    b = lw.view(np.uint32).copy()
    b[b == 0x80000000] = 0
    k = np.where(b & 0x80000000 != 0, b ^ np.uint32(0xFFFFFFFF), b ^ np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(lw) | (lw == -np.inf)] = 0
    return k


def order(lw: np.ndarray) -> np.ndarray:
    """ascending by (key, particle index)"""
    return np.argsort(keys(lw), kind="stable")


def gpd_fit(x: np.ndarray):
    """Zhang & Stephens' estimate of the generalised Pareto shape and scale of the ascending exceedances x (float64), with the
    weakly informative prior of the PSIS paper on k -> (k_hat, sigma_hat)"""
    M = x.size
    m = 30 + math.isqrt(M)
    xq = x[int(math.floor(M / 4 + 0.5)) - 1]
    j = np.arange(1, m + 1, dtype=np.float64)
    b = (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * xq) + 1.0 / x[-1]
    with np.errstate(all="ignore"):
        k = np.log1p(-b[:, None] * x[None, :]).mean(axis=1)
        L = M * (np.log(-b / k) - k - 1.0)
        fin = np.isfinite(L)
        w = np.where(fin, np.exp(L - (L[fin].max() if fin.any() else 0.0)), 0.0)
        w = w / w.sum()
        bh = float((w * b).sum())
        k0 = float(np.log1p(-bh * x).mean())
        return (M * k0 + 5.0) / (M + 10.0), -k0 / bh


def pareto_smooth_segment(lw: np.ndarray):
    """one segment -> (logw_out f32[n], fit f32[4] = {k_hat, sigma_hat, cutoff, M}, tail indices int64[M] ascending in the order)"""
    lw = np.ascontiguousarray(lw, np.float32)
    n = lw.size
    M = tail_size(n)
    o = order(lw)
    live = keys(lw) != 0
    tail = o[n - M:]
    cut = o[n - M - 1]                                     # (M <= n / 5 < n)
    c = lw[cut] if live[cut] else np.float32(np.nan)
    if c == 0:
        c = np.float32(0.0)                                # (-0.0 is reported as +0.0, as the key has it)
    out = lw.copy()
    none = np.array([np.nan, np.nan, c, M], np.float32)
    if M < 5 or int(live.sum()) <= M:
        return out, none, tail
    mx = np.float64(lw[o[-1]])
    ecut = np.exp(np.float64(c) - mx)
    x = np.exp(lw[tail].astype(np.float64) - mx) - ecut
    if not x[int(math.floor(M / 4 + 0.5)) - 1] > 0:
        return out, none, tail
    kh, sg = gpd_fit(x)
    p = (np.arange(M, dtype=np.float64) + 0.5) / M
    with np.errstate(all="ignore"):
        l1 = np.log1p(-p)
        q = -sg * l1 if kh == 0 else sg * np.expm1(-kh * l1) / kh
        v = np.log(q + ecut)
        v = np.where(v > 0, 0.0, v)
    out[tail] = (v + mx).astype(np.float32)
    return out, np.array([kh, sg, c, M]).astype(np.float32), tail


def pareto_smooth(lw: np.ndarray, n_segments: int = 1):
    """-> (logw_out f32[K], fit f32[S][4])"""
    lw = np.ascontiguousarray(lw, np.float32).reshape(n_segments, -1)
    res = [pareto_smooth_segment(r) for r in lw]
    return np.concatenate([r[0] for r in res]), np.stack([r[1] for r in res])


# ---- weight families of the tests ----
def pareto_weights(rs, K, k, offset=-1234.5):
    """exact Pareto ratios with shape k: lw = -k log u + offset"""
    return (-k * np.log(rs.random(K)) + offset).astype(np.float32)


def normal_ratio_weights(rs, K, s):
    """log of N(x; 0, 1) / N(x; 0, s) at x ~ N(0, s): the tail of the ratio is Pareto with k = 1 - s^2 for s < 1, bounded for s > 1"""
    x = s * rs.standard_normal(K)
    return (-0.5 * x * x + 0.5 * (x / s) ** 2 + math.log(s)).astype(np.float32)


def ulp_distance(a, b):
    """distance in float32 units in the last place between two float32 arrays (equal NaNs: 0; a NaN against a number: 2^31)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)

    def lin(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(lin(np.atleast_1d(a)) - lin(np.atleast_1d(b)))
    na, nb = np.isnan(np.atleast_1d(a)), np.isnan(np.atleast_1d(b))
    d[na & nb] = 0
    d[na ^ nb] = 1 << 31
    return d
