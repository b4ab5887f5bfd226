"""The definition of gjx_lineage_weights (include/gjx.h), restated in NumPy for the tests: the backward scatter-add of the last
step's weights through the ancestor table, on exact integers (uint64) or on float64 true weights, and the brute-force lineage tracing
it is checked against in tests/test_lineage_cpu.py."""
import numpy as np


def ref_u(logw, K):
    """the integer weights u_i = rint(exp(logw_i - M) 2^32) of gjx_weighted_quantiles (float64 exp) as uint64; dead (-inf, NaN): 0;
    logw None: 2^32 each"""
    if logw is None:
        return np.full(K, 1 << 32, np.uint64)
    return np.rint(ref_e64(logw, K) * 2.0 ** 32).astype(np.uint64)


def ref_e64(logw, K):
    """float64 true weights exp(logw - max), 0 for a dead particle (all 0 for a collection without weight)"""
    if logw is None:
        return np.ones(K)
    w = np.asarray(logw, np.float64)
    live = ~np.isnan(w) & (w > -np.inf)
    if not live.any() or np.isinf(w[live].max()):
        return np.zeros(K)
    return np.where(live, np.exp(np.where(live, w, 0.0) - w[live].max()), 0.0)


def descendant_weights(anc, last):
    """W[T][K] in the dtype of ``last`` (uint64: exact; float64): W[T-1] = last, W[t-1][a] = sum of W[t][i] over anc[t-1][i] = a"""
    anc = np.asarray(anc).reshape(-1, last.size)
    T = anc.shape[0] + 1
    W = np.zeros((T, last.size), last.dtype)
    W[T - 1] = last
    for t in range(T - 1, 0, -1):
        np.add.at(W[t - 1], anc[t - 1], W[t])
    return W


def descendant_weights_by_tracing(anc, last):
    """the same by following every last-step particle's lineage back: idx[t-1] = anc[t-1][idx[t]], W[t][idx[t]] += last"""
    anc = np.asarray(anc).reshape(-1, last.size)
    T = anc.shape[0] + 1
    W = np.zeros((T, last.size), last.dtype)
    idx = np.arange(last.size)
    for t in range(T - 1, -1, -1):
        np.add.at(W[t], idx, last)
        if t > 0:
            idx = anc[t - 1][idx]
    return W


def ref_w32(W, U):
    """what the library stores: the integer ratio rounded to double, then to float; NaN without weight"""
    if int(U) == 0:
        return np.full(W.shape, np.nan, np.float32)
    return np.float32(W.astype(np.float64) / np.float64(U))
