"""Descendant weights of a filter's history (gjx_lineage_weights), host side: the C ABI's declarations (include/gjx.h <->
libgjx_hip.so <-> genjax_amd/_abi.py), the workspace query, every refusal that is decided before a launch, and the restatement of
the definition that the GPU tests compare with (tests/lineage_ref.py: a backward np.add.at on uint64), itself checked against
brute-force lineage tracing.  No compute call is made here: the device pointers handed to the library are never dereferenced by a
call that refuses."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from genjax_amd import _abi as A
from lineage_ref import descendant_weights, descendant_weights_by_tracing, ref_e64, ref_u, ref_w32

ROOT = os.path.dirname(HERE)
NEW = ("gjx_lineage_weights_workspace_bytes", "gjx_lineage_weights")
P = ctypes.c_void_p(0x1000)        # "some non-NULL pointer": a refusing call does not touch it


def _header():
    return open(os.path.join(ROOT, "include", "gjx.h")).read()


def _lib():
    from genjax_amd import _lib
    return _lib.load()


def _l(anc=P, stride=64, T=3, K=64, logw=P, stats=P, w=P, survivors=P, n_bad=P, ws=P, ws_bytes=1 << 30):
    return _lib().gjx_lineage_weights(anc, stride, T, K, logw, stats, w, survivors, n_bad, ws, ws_bytes, None)


# ---- declarations ----
def test_header_declares_and_library_exports_the_calls():
    hdr, lib = _header(), _lib()
    assert re.search(r"\bsize_t\s+gjx_lineage_weights_workspace_bytes\s*\(\s*int32_t\s+T\s*,\s*int64_t\s+K\s*\)", hdr)
    assert re.search(r"\bint\s+gjx_lineage_weights\s*\(", hdr)
    for name in NEW:
        assert name in A.PROTOTYPES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == A.PROTOTYPES[name][1]
    assert A.PROTOTYPES["gjx_lineage_weights_workspace_bytes"] == (ctypes.c_size_t, [A.i32, A.i64])
    assert A.PROTOTYPES["gjx_lineage_weights"] == (ctypes.c_int, [A.vp, A.i64, A.i32, A.i64, A.vp, A.vp, A.vp, A.vp, A.vp, A.vp,
                                                                  ctypes.c_size_t, A.vp])


def test_abi_version_is_unchanged():
    assert "#define GJX_ABI_VERSION 11" in _header() and A.ABI_VERSION == 11 and _lib().gjx_version() == 11


def test_workspace_is_linear_in_K_and_independent_of_T():
    q = _lib().gjx_lineage_weights_workspace_bytes
    for K in (1, 63, 1024, 1025, 4113, 1 << 18, (1 << 20) + 1, (1 << 31) - 1):
        n = q(2, K)
        assert 0 < n <= 24 * K + 4096, (K, n)
        assert n >= 24 * K                                  # three u64[K]
        assert q(1, K) == n == q(9, K) == q(4096, K), K
    sizes = [q(4, K) for K in (1, 2, 63, 64, 1025, 1 << 14)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    # arguments the call refuses
    for args in ((0, 64), (-1, 64), (3, 0), (3, -64), (3, 1 << 31), (3, 1 << 40)):
        assert q(*args) == 0, args


# ---- refusals ----
def test_refusals_need_no_device():
    lib = _lib()
    assert _l(stats=None) == A.EINVAL
    assert _l(w=None) == A.EINVAL
    assert _l(survivors=None) == A.EINVAL
    assert _l(n_bad=None) == A.EINVAL
    assert _l(ws=None) == A.EINVAL
    assert _l(anc=None) == A.EINVAL                         # T = 3 needs its two rows of ancestors
    assert _l(anc=None, T=2) == A.EINVAL
    assert _l(T=0) == A.EINVAL
    assert _l(T=-2) == A.EINVAL
    assert _l(K=0) == A.EINVAL
    assert _l(K=-5) == A.EINVAL
    assert _l(stride=63) == A.EINVAL                        # steps would overlap
    assert _l(K=1 << 31, stride=1 << 31) == A.EINVAL
    assert _l(K=1 << 33, stride=1 << 33) == A.EINVAL
    assert b"gjx_lineage_weights" in lib.gjx_last_error()
    # what is NOT a refusal is decided next: the workspace
    need = lib.gjx_lineage_weights_workspace_bytes(3, 64)
    assert _l(ws_bytes=need - 1) == A.EWORKSPACE
    assert b"workspace" in lib.gjx_last_error()
    assert _l(ws_bytes=0) == A.EWORKSPACE
    assert _l(logw=None, ws_bytes=0) == A.EWORKSPACE        # (NULL log-weights are equal weights)
    assert _l(anc=None, T=1, ws_bytes=0) == A.EWORKSPACE    # (T = 1 has no ancestors ...)
    assert _l(anc=None, T=1, stride=0, ws_bytes=0) == A.EWORKSPACE      # (... and no stride to check)
    assert _l(K=(1 << 31) - 1, stride=(1 << 31) - 1, ws_bytes=1 << 30) == A.EWORKSPACE       # the largest K is taken: 48 GiB


def test_kernel_wrapper_refuses_before_it_reaches_the_library():
    import torch
    from genjax_amd import kernels
    with pytest.raises(ValueError, match="i32"):
        kernels.lineage_weights(torch.zeros((2, 8), dtype=torch.int64))
    with pytest.raises(ValueError, match="i32"):
        kernels.lineage_weights(torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="no particles"):
        kernels.lineage_weights(torch.zeros((2, 0), dtype=torch.int32))
    with pytest.raises(ValueError, match="column stride"):
        kernels.lineage_weights(torch.zeros((8, 3), dtype=torch.int32).t())
    with pytest.raises(ValueError, match="logw"):
        kernels.lineage_weights(torch.zeros((2, 8), dtype=torch.int32), torch.zeros(7))
    with pytest.raises(ValueError, match="logw"):
        kernels.lineage_weights(torch.zeros((2, 8), dtype=torch.int32), torch.zeros(8, dtype=torch.float64))


def test_histories_have_the_methods():
    from genjax_amd.inference.pf import ParticleHistory
    from genjax_amd.inference.scan_filter import ScanHistory
    for cls in (ScanHistory, ParticleHistory):
        for name in ("smoothing_weights", "survivors", "smoothed_moments", "smoothed_quantiles", "smoothed_means", "paths"):
            assert callable(getattr(cls, name)), (cls, name)


# ---- the restatement ----
def _ancestors(rs, T, K, kind):
    if T == 1:
        return np.zeros((0, K), np.int32)
    if kind == "sorted":
        return np.sort(rs.integers(0, K, (T - 1, K)), axis=1).astype(np.int32)
    if kind == "permutation":
        return np.stack([rs.permutation(K) for _ in range(T - 1)]).astype(np.int32).reshape(T - 1, K)
    return rs.integers(0, K, (T - 1, K)).astype(np.int32)


@pytest.mark.parametrize("K,T", [(1, 1), (1, 3), (63, 2), (1025, 5), (4113, 9)])
def test_restatement_is_lineage_tracing(K, T):
    rs = np.random.default_rng(100 * K + T)
    for kind in ("sorted", "permutation", "random"):
        anc = _ancestors(rs, T, K, kind)
        logw = (3.0 * rs.standard_normal(K)).astype(np.float32)
        dead = rs.random(K) < 0.2
        dead[rs.integers(0, K)] = False
        logw[dead] = -np.inf
        logw[dead & (rs.random(K) < 0.3)] = np.nan
        u = ref_u(logw, K)
        # (a live particle 22.2 or more below the maximum rounds to u = 0 as well: dead by its weight)
        assert u.dtype == np.uint64 and (u[dead] == 0).all() and (u[~dead] > 0).mean() > 0.99 and u.max() == 1 << 32
        U = int(u.sum())
        W = descendant_weights(anc, u)
        assert W.dtype == np.uint64 and W.shape == (T, K)
        np.testing.assert_array_equal(W, descendant_weights_by_tracing(anc, u))
        assert all(int(W[t].sum()) == U for t in range(T)), (K, T, kind)
        surv = (W > 0).sum(axis=1)
        assert surv[T - 1] == (u > 0).sum() and (np.diff(surv) >= 0).all()
        if kind == "permutation":
            assert (surv == surv[0]).all()                  # nobody shares a parent: nothing coalesces
        w = ref_w32(W, U)
        assert w.dtype == np.float32 and np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max() <= K * 2.0 ** -24
        # the float64 form of the same recursion, for general weights on the device
        e = ref_e64(logw, K)
        Wf = descendant_weights(anc, e)
        np.testing.assert_allclose(Wf / e.sum(), W.astype(np.float64) / U, rtol=0, atol=K * 2.0 ** -32 / e.sum())
    assert np.isnan(ref_w32(np.zeros((T, K), np.uint64), 0)).all()
    assert (ref_u(None, K) == 1 << 32).all() and (ref_u(np.full(K, -np.inf, np.float32), K) == 0).all()


def test_restatement_on_a_hand_computed_example():
    """4 particles, 3 steps; last weights 1, 1/2, 0, 1/4.  Parents of step 2: 0 0 1 3; of step 1: 2 2 2 0.
    W_2 = u;  W_1 = [u0 + u1, u2, 0, u3] = [1.5, 0, 0, 0.25];  W_0 = [0.25, 0, 1.5, 0]  (in units of 2^32)"""
    logw = np.log(np.array([1.0, 0.5, 1.0, 0.25])).astype(np.float32)
    logw[2] = -np.inf
    u = ref_u(logw, 4)
    anc = np.array([[2, 2, 2, 0], [0, 0, 1, 3]], np.int32)
    W = descendant_weights(anc, u)
    assert W[2].tolist() == u.tolist()
    assert W[1].tolist() == [u[0] + u[1], 0, 0, u[3]]
    assert W[0].tolist() == [u[3], 0, u[0] + u[1], 0]
    assert ((W > 0).sum(axis=1) == [2, 2, 3]).all()
