"""Weighted cross-moments of pairs of particles (gjx_weighted_cross_moments), host side: the C ABI's declarations (include/gjx.h <->
libgjx_hip.so <-> genjax_amd/_abi.py), the workspace query, every refusal that is decided before a launch, and the float64
restatement of the definition that the GPU tests compare with (tests/cross_moments_ref.py), itself checked against np.cov and against
explicitly traced paths.  No compute call is made here: the device pointers handed to the library are never dereferenced by a call
that refuses."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from genjax_amd import _abi as A
from cross_moments_ref import CrossRef, traced_pair_moments
from lineage_ref import descendant_weights

ROOT = os.path.dirname(HERE)
NEW = ("gjx_weighted_cross_moments_workspace_bytes", "gjx_weighted_cross_moments")
P = ctypes.c_void_p(0x1000)        # "some non-NULL pointer": a refusing call does not touch it


def _header():
    return open(os.path.join(ROOT, "include", "gjx.h")).read()


def _lib():
    from genjax_amd import _lib
    return _lib.load()


def _c(rows_a=P, stride_a=64, n_a=3, rows_b=P, stride_b=64, n_b=5, K_b=64, index=P, logw=P, K=64, stats=P, mean_a=P, mean_b=P, cross=P,
       n_bad=P, ws=P, ws_bytes=1 << 30):
    return _lib().gjx_weighted_cross_moments(rows_a, stride_a, n_a, rows_b, stride_b, n_b, K_b, index, logw, K, stats, mean_a, mean_b, cross,
                                             n_bad, ws, ws_bytes, None)


# ---- declarations ----
def test_header_declares_and_library_exports_the_calls():
    hdr, lib = _header(), _lib()
    assert re.search(r"\bsize_t\s+gjx_weighted_cross_moments_workspace_bytes\s*\(\s*int32_t\s+n_a\s*,\s*int32_t\s+n_b\s*,\s*int64_t\s+K\s*\)", hdr)
    assert re.search(r"\bint\s+gjx_weighted_cross_moments\s*\(", hdr)
    for name in NEW:
        assert name in A.PROTOTYPES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == A.PROTOTYPES[name][1]
    assert A.PROTOTYPES[NEW[0]] == (ctypes.c_size_t, [A.i32, A.i32, A.i64])
    assert A.PROTOTYPES[NEW[1]] == (ctypes.c_int, [A.vp, A.i64, A.i32, A.vp, A.i64, A.i32, A.i64, A.vp, A.vp, A.i64, A.vp, A.vp, A.vp, A.vp,
                                                   A.vp, A.vp, ctypes.c_size_t, A.vp])


def test_abi_version_is_unchanged():
    assert "#define GJX_ABI_VERSION 11" in _header() and A.ABI_VERSION == 11 and _lib().gjx_version() == 11


def test_workspace_is_the_partials_of_the_tiles():
    q = _lib().gjx_weighted_cross_moments_workspace_bytes
    for n_a, n_b in ((1, 1), (3, 5), (16, 16), (16, 1)):
        for K in (1, 1024, 1025, 4113, 1 << 20):
            assert q(n_a, n_b, K) == 4 * (3 + n_a + n_b + n_a * n_b) * ((K + 1023) // 1024), (n_a, n_b, K)
    for args in ((0, 1, 64), (1, 0, 64), (-1, 1, 64), (1, 1, 0), (1, 1, -64), (17, 1, 64), (1, 17, 64)):
        assert q(*args) == 0, args


# ---- refusals ----
def test_refusals_need_no_device():
    lib = _lib()
    for name in ("rows_a", "rows_b", "stats", "mean_a", "mean_b", "cross", "n_bad", "ws"):
        assert _c(**{name: None}) == A.EINVAL, name
        assert b"gjx_weighted_cross_moments" in lib.gjx_last_error()
    for kw in (dict(n_a=0), dict(n_b=0), dict(n_a=-1), dict(K=0), dict(K=-5), dict(K_b=0),
               dict(stride_a=63),                           # the rows of a would overlap
               dict(stride_b=63),                           # the rows of b would overlap
               dict(K_b=37, stride_b=37, index=None),       # the identity needs K_b >= K
               dict(K_b=1 << 31, stride_b=1 << 31)):        # an index is 32 bits
        assert _c(**kw) == A.EINVAL, kw
        assert b"gjx_weighted_cross_moments" in lib.gjx_last_error()
    for kw in (dict(n_a=17), dict(n_b=17), dict(n_a=17, n_b=40)):
        assert _c(**kw) == A.EUNSUPPORTED, kw
        msg = lib.gjx_last_error()
        assert b"gjx_weighted_cross_moments" in msg and b"16" in msg
    # what is NOT a refusal is decided next: the workspace
    need = lib.gjx_weighted_cross_moments_workspace_bytes(3, 5, 64)
    assert _c(ws_bytes=need - 1) == A.EWORKSPACE
    msg = lib.gjx_last_error()
    assert b"gjx_weighted_cross_moments" in msg and b"workspace" in msg
    assert _c(ws_bytes=0) == A.EWORKSPACE
    assert _c(index=None, ws_bytes=0) == A.EWORKSPACE       # (a NULL index is the identity ...)
    assert _c(logw=None, ws_bytes=0) == A.EWORKSPACE        # (... and NULL log-weights are equal weights)
    assert _c(K_b=37, stride_b=37, ws_bytes=0) == A.EWORKSPACE          # (with an index K_b is free)
    assert _c(K_b=100, stride_b=100, index=None, ws_bytes=0) == A.EWORKSPACE


def test_kernel_wrapper_refuses_before_it_reaches_the_library():
    import torch
    from genjax_amd import kernels
    f = kernels.weighted_cross_moments
    a, b = torch.zeros((3, 8)), torch.zeros((5, 8))
    with pytest.raises(ValueError, match="rows_a"):
        f(a.double(), b)
    with pytest.raises(ValueError, match="rows_b"):
        f(a, torch.zeros((2, 5, 8)))
    with pytest.raises(ValueError, match="column stride"):
        f(torch.zeros((8, 3)).t(), b)
    with pytest.raises(ValueError, match="16"):
        f(torch.zeros((17, 8)), b)
    with pytest.raises(ValueError, match="16"):
        f(a, torch.zeros((17, 8)))
    with pytest.raises(ValueError, match="logw"):
        f(a, b, torch.zeros(7))
    with pytest.raises(ValueError, match="index"):
        f(a, b, None, torch.zeros(8, dtype=torch.int64))
    with pytest.raises(ValueError, match="index"):
        f(a, b, None, torch.zeros(7, dtype=torch.int32))
    with pytest.raises(ValueError, match="index"):
        f(a, torch.zeros((5, 4)))                           # fewer parents than particles, and no index
    with pytest.raises(ValueError, match="no step"):
        kernels.weighted_cross_moments_steps([], torch.zeros((1, 8)))


def test_surfaces_have_the_methods():
    from genjax_amd.inference.pf import ParticleHistory
    from genjax_amd.inference.scan_filter import ScanHistory
    from genjax_amd.inference.smc import ParticleCollection
    assert callable(ParticleCollection.cross_covariance)
    for cls in (ScanHistory, ParticleHistory):
        assert callable(cls.smoothed_pair_moments) and callable(cls._smoothed_pair_moments)


# ---- the restatement ----
def _weights(rs, K):
    lw = (2.0 * rs.standard_normal(K) - 37.0).astype(np.float32)
    dead = rs.random(K) < 0.2
    dead[rs.integers(0, K)] = False
    lw[dead] = -np.inf
    lw[dead & (rs.random(K) < 0.3)] = np.nan
    return lw


@pytest.mark.parametrize("K,n_a,n_b", [(1, 1, 1), (65, 3, 5), (1025, 16, 1), (4113, 4, 4)])
def test_restatement_is_numpy_cov_of_the_stacked_problem(K, n_a, n_b):
    rs = np.random.default_rng(K + n_a)
    a = (rs.standard_normal((n_a, K)) + 100.0).astype(np.float32)
    b = (rs.standard_normal((n_b, 37)) * 3.0 - 5.0).astype(np.float32)
    idx = rs.integers(0, 37, K).astype(np.int32)
    a[0] += 0.5 * b[0, idx]                                 # something to find
    lw = _weights(rs, K)
    a[:, ~np.isfinite(lw)] = np.nan                         # dead particles: whatever values
    ref = CrossRef(a, b, lw, idx)
    live = np.isfinite(lw)
    assert ref.n_bad == 0 and (ref.keep == live).all()
    e = np.exp(lw[live].astype(np.float64) - lw[live].max())
    stacked = np.concatenate([a[:, live], b[:, idx[live]]]).astype(np.float64)
    full = np.cov(stacked, aweights=e, bias=True).reshape(n_a + n_b, n_a + n_b) if live.sum() > 1 else np.zeros((n_a + n_b,) * 2)
    np.testing.assert_allclose(ref.cross, full[:n_a, n_a:], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(ref.mean_a, np.average(stacked[:n_a], axis=1, weights=e), rtol=1e-12)
    np.testing.assert_allclose(ref.mean_b, np.average(stacked[n_a:], axis=1, weights=e), rtol=1e-12)
    np.testing.assert_allclose(ref.stats, [lw[live].max(), e.sum(), (e * e).sum(), e.sum() ** 2 / (e * e).sum()], rtol=1e-12)
    assert (ref.tol_cross > 0).all() and ref.tol_cross.shape == (n_a, n_b)
    # a live particle with an index outside the parents is removed and counted; a dead one is not counted
    bad = idx.copy()
    j, d = np.flatnonzero(live)[0], np.flatnonzero(~live)
    bad[j] = 37
    if d.size:
        bad[d[0]] = -1
    r2 = CrossRef(a, b, lw, bad)
    assert r2.n_bad == 1 and r2.keep.sum() == live.sum() - 1
    if live.sum() == 1:
        assert np.isnan(r2.cross).all() and r2.stats.tolist() == [-np.inf, 0, 0, 0]
    # the identity, and equal weights
    r3 = CrossRef(a[:, live], a[:, live])
    np.testing.assert_allclose(r3.cross, np.cov(a[:, live].astype(np.float64), bias=True).reshape(n_a, n_a) if live.sum() > 1 else 0.0,
                               rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("K,T", [(63, 2), (257, 5), (1025, 4)])
def test_restatement_over_an_ancestor_table_is_the_sum_over_traced_paths(K, T):
    """E[x_t x_{t-1}] of the paths = the restatement on (step t, step t-1 through ancestors[t-1]) under step t's descendant weights"""
    rs = np.random.default_rng(10 * K + T)
    d = 3
    x = rs.standard_normal((T, d, K)).astype(np.float32)
    for kind in ("sorted", "random"):
        anc = rs.integers(0, K, (T - 1, K)).astype(np.int32)
        if kind == "sorted":
            anc = np.sort(anc, axis=1)
        lw = _weights(rs, K)
        live = np.isfinite(lw)
        e = np.where(live, np.exp(np.where(live, lw, 0.0).astype(np.float64) - lw[live].max()), 0.0)
        W = descendant_weights(anc, e) / e.sum()
        mean, prev, cross = traced_pair_moments(x.astype(np.float64), anc, e / e.sum())
        for t in range(1, T):
            with np.errstate(divide="ignore"):
                ref = CrossRef(x[t], x[t - 1], np.log(W[t]), anc[t - 1])
            np.testing.assert_allclose(ref.mean_a, mean[t - 1], rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(ref.mean_b, prev[t - 1], rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(ref.cross, cross[t - 1], rtol=1e-9, atol=1e-12)
            # the parents' marginal is step t-1's own smoothing marginal: w[t-1][a] = sum of w[t] over the children of a
            np.testing.assert_allclose(ref.mean_b, x[t - 1].astype(np.float64) @ W[t - 1], rtol=1e-9, atol=1e-12)
