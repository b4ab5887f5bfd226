"""Pareto-smoothed importance weights (gjx_pareto_smooth), host side: the C ABI's declarations (include/gjx.h <-> libgjx_hip.so <->
genjax_amd/_abi.py), the workspace query, every refusal that is decided before a launch, and the restatement of the definition that
the GPU tests compare with (tests/psis_ref.py), checked on its own against weights whose tail shape is known.  No compute call is
made here: the device pointers handed to the library are never dereferenced by a call that refuses."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from genjax_amd import _abi as A
import psis_ref as R

ROOT = os.path.dirname(HERE)
NEW = ("gjx_pareto_smooth_workspace_bytes", "gjx_pareto_smooth")
P = ctypes.c_void_p(0x1000)        # "some non-NULL pointer": a refusing call does not touch it


def _header():
    return open(os.path.join(ROOT, "include", "gjx.h")).read()


def _lib():
    from genjax_amd import _lib
    return _lib.load()


def _p(logw=P, K=4096, S=1, out=P, fit=P, ws=P, ws_bytes=1 << 30):
    return _lib().gjx_pareto_smooth(logw, K, S, out, fit, ws, ws_bytes, None)


# ---- declarations ----
def test_header_declares_and_library_exports_the_calls():
    hdr, lib = _header(), _lib()
    assert re.search(r"\bsize_t\s+gjx_pareto_smooth_workspace_bytes\s*\(\s*int64_t\s+K\s*,\s*int64_t\s+n_segments\s*\)", hdr)
    assert re.search(r"\bint\s+gjx_pareto_smooth\s*\(\s*const\s+float\s*\*\s*logw\s*,\s*int64_t\s+K\s*,\s*int64_t\s+n_segments\s*,\s*float\s*\*\s*logw_out", hdr)
    for name in NEW:
        assert name in A.PROTOTYPES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == A.PROTOTYPES[name][1]
    assert A.PROTOTYPES["gjx_pareto_smooth_workspace_bytes"] == (ctypes.c_size_t, [A.i64, A.i64])
    assert A.PROTOTYPES["gjx_pareto_smooth"] == (ctypes.c_int, [A.vp, A.i64, A.i64, A.vp, A.vp, A.vp, ctypes.c_size_t, A.vp])


def test_abi_version_is_unchanged():
    assert "#define GJX_ABI_VERSION 11" in _header() and A.ABI_VERSION == 11 and _lib().gjx_version() == 11


def test_workspace_is_monotone_in_K_and_zero_for_refused_arguments():
    q = _lib().gjx_pareto_smooth_workspace_bytes
    sizes = [q(K, 1) for K in (1, 4, 24, 25, 50, 1000, 1024, 1025, 4113, (1 << 14) + 1, 1 << 20, 1 << 22)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
    # never particle-sized: the tail (M <= 6144), not the collection
    assert q(1 << 22, 1) < 1 << 18
    # S segments of n: S times the per-segment part of one segment of n
    one, many = q(1024, 1), q(50 * 1024, 50)
    assert one < many <= 50 * one
    for args in ((0, 1), (-8, 1), (64, 0), (64, -2), (64, 3), ((1 << 22) + 1, 1), (1 << 23, 1), (1 << 40, 1)):
        assert q(*args) == 0, args
    assert q(1 << 23, 2) > 0                               # the limit is on the segment, not on K


# ---- refusals ----
def test_refusals_need_no_device():
    lib = _lib()
    assert _p(logw=None) == A.EINVAL
    assert _p(out=None) == A.EINVAL
    assert _p(fit=None) == A.EINVAL
    assert _p(ws=None) == A.EINVAL
    assert _p(K=0) == A.EINVAL
    assert _p(K=-4096) == A.EINVAL
    assert _p(S=0) == A.EINVAL
    assert _p(S=-1) == A.EINVAL
    assert _p(S=3) == A.EINVAL                              # 3 does not divide 4096
    assert _p(K=1 << 23, out=None) == A.EINVAL              # a NULL pointer is a bad argument whatever the size
    assert b"gjx_pareto_smooth" in lib.gjx_last_error()
    assert _p(K=(1 << 22) + 1) == A.EUNSUPPORTED
    assert _p(K=1 << 23) == A.EUNSUPPORTED
    assert _p(K=3 << 22, S=2) == A.EUNSUPPORTED
    assert b"2^22" in lib.gjx_last_error()
    # what is NOT a refusal is decided next: the workspace
    need = lib.gjx_pareto_smooth_workspace_bytes(4096, 1)
    assert _p(ws_bytes=need - 1) == A.EWORKSPACE
    assert b"workspace" in lib.gjx_last_error()
    assert _p(ws_bytes=0) == A.EWORKSPACE
    assert _p(K=1 << 22, ws_bytes=0) == A.EWORKSPACE        # the largest segment is taken
    assert _p(K=1 << 23, S=2, ws_bytes=0) == A.EWORKSPACE
    assert _p(K=4096, S=4096, ws_bytes=0) == A.EWORKSPACE   # segments of one particle are a (trivial) call
    assert _p(logw=P, out=P, ws_bytes=0) == A.EWORKSPACE    # in place is allowed


def test_kernel_wrapper_refuses_before_it_reaches_the_library():
    import torch
    from genjax_amd import kernels
    with pytest.raises(ValueError, match="f32"):
        kernels.pareto_smooth(torch.zeros(64, dtype=torch.float64))
    with pytest.raises(ValueError, match="segments"):
        kernels.pareto_smooth(torch.zeros(0))
    with pytest.raises(ValueError, match="segments"):
        kernels.pareto_smooth(torch.zeros(64), 0)
    with pytest.raises(ValueError, match="segments"):
        kernels.pareto_smooth(torch.zeros(64), 3)
    with pytest.raises(ValueError, match="2\\^22"):
        kernels.pareto_smooth(torch.zeros(1).expand((1 << 22) + 1))
    for n in (1, 4, 5, 24, 25, 1024, 4113, 1 << 20, 1 << 22):
        assert kernels.pareto_tail(n) == R.tail_size(n) == min(n // 5, math.ceil(3 * math.sqrt(n)))
    assert kernels.pareto_tail(24) == 4 and kernels.pareto_tail(25) == 5 and kernels.pareto_tail(1 << 20) == 3072
    assert kernels.pareto_tail(1 << 22) == 6144


def test_collections_have_the_methods_and_the_threshold():
    from genjax_amd import inference
    from genjax_amd.inference.smc import ParticleCollection, TrialCollections
    for cls in (ParticleCollection, TrialCollections):
        for name in ("pareto_k", "pareto_smoothed"):
            assert callable(getattr(cls, name)), (cls, name)
    f = inference.pareto_k_threshold
    assert f(10 ** 10) == 0.7 and f(1 << 20) == 0.7 and f(2200) == 0.7
    assert f(1000) == pytest.approx(1 - 1 / 3) and f(100) == pytest.approx(0.5) and f(10) == pytest.approx(0.0)


# ---- the restatement alone is right ----
@pytest.mark.parametrize("k", [0.1, 0.3, 0.5, 0.7, 0.9])
def test_restatement_recovers_the_shape_of_exact_pareto_ratios(k):
    """K = 2^20, M = 3072: |k_hat - k| <= 0.1, about 3 standard errors (1 + k) / sqrt(M)"""
    lw = R.pareto_weights(np.random.default_rng(1), 1 << 20, k)
    out, fit, tail = R.pareto_smooth_segment(lw)
    print(f"k = {k}: k_hat {fit[0]:.4f}, sigma {fit[1]:.4g}, cutoff {fit[2]:.3f}")
    assert fit[3] == 3072 and tail.size == 3072
    assert abs(float(fit[0]) - k) <= 0.1
    assert fit[1] > 0 and fit[2] == np.sort(lw)[-3073]


def test_restatement_on_normal_ratios():
    """a standard normal target under an N(0, 0.6^2) proposal has Pareto ratios with k = 1 - 0.36; under N(0, 1.5^2) the ratio is
    bounded: k_hat < 0.  K = 2^16, M = 768: (1 + k) / sqrt(M) = 0.06 standard error, and the chi-square tail's slowly varying factor
    on top: within 0.2"""
    rs = np.random.default_rng(1)
    narrow = R.pareto_smooth_segment(R.normal_ratio_weights(rs, 1 << 16, 0.6))[1]
    wide = R.pareto_smooth_segment(R.normal_ratio_weights(rs, 1 << 16, 1.5))[1]
    print(f"N(0, 0.6): k_hat {narrow[0]:.4f}; N(0, 1.5): k_hat {wide[0]:.4f}")
    assert narrow[3] == 768 and abs(float(narrow[0]) - 0.64) <= 0.2
    assert wide[0] < 0


# ---- no estimate ----
def _is_copy_without_estimate(lw, M):
    out, fit, tail = R.pareto_smooth_segment(lw)
    assert out.view(np.uint32).tolist() == np.asarray(lw, np.float32).view(np.uint32).tolist()
    assert np.isnan(fit[0]) and np.isnan(fit[1]) and fit[3] == M and tail.size == M
    return fit


def test_no_estimate_cases():
    rs = np.random.default_rng(7)
    lw = rs.standard_normal(24).astype(np.float32)
    fit = _is_copy_without_estimate(lw, 4)                  # K = 24: M = 4 < 5
    assert fit[2] == np.sort(lw)[-5]
    assert R.pareto_smooth_segment(rs.standard_normal(25).astype(np.float32))[1][3] == 5      # ... and 25 is the smallest fit
    assert not np.isnan(R.pareto_smooth_segment(rs.standard_normal(25).astype(np.float32))[1][0])
    fit = _is_copy_without_estimate(np.full(1000, -3.25, np.float32), 95)      # equal weights: x_q = 0
    assert fit[2] == np.float32(-3.25)
    lw = rs.standard_normal(1000).astype(np.float32)
    lw[95:] = -np.inf                                       # 95 live particles = M: the particle below the tail is dead
    lw[200:300] = np.nan
    fit = _is_copy_without_estimate(lw, 95)
    assert np.isnan(fit[2])
    lw[95] = 0.5                                            # 96 live ones: an estimate
    out, fit, _ = R.pareto_smooth_segment(lw)
    assert not np.isnan(fit[0]) and fit[2] == lw[:96].min()
    _is_copy_without_estimate(np.full(64, -np.inf, np.float32), 12)
    _is_copy_without_estimate(np.zeros(3, np.float32), 0)
    assert R.pareto_smooth_segment(np.array([1.0, 3.0, 2.0], np.float32))[1][2] == 3.0      # M = 0: the "cutoff" is the largest


# ---- properties ----
def _families():
    rs = np.random.default_rng(11)
    yield "pareto", R.pareto_weights(rs, 4113, 0.6)
    yield "normal", R.normal_ratio_weights(rs, 4113, 0.6)
    yield "quarters", (np.round(4 * 3.0 * rs.standard_normal(4113)) / 4).astype(np.float32)
    lw = R.pareto_weights(rs, 4113, 0.4, 0.0)
    lw[rs.random(4113) < 0.5] = -np.inf
    lw[rs.random(4113) < 0.05] = np.nan
    yield "half dead", lw


@pytest.mark.parametrize("name,lw", list(_families()), ids=[n for n, _ in _families()])
def test_properties_of_the_restatement(name, lw):
    out, fit, tail = R.pareto_smooth_segment(lw)
    n, M = lw.size, int(fit[3])
    assert M == R.tail_size(n) == tail.size and not np.isnan(fit[0])
    o = np.argsort(R.keys(lw), kind="stable")
    assert (tail == o[n - M:]).all()                        # exactly the last M of the stable order
    rest = np.setdiff1d(np.arange(n), tail)
    assert (out[rest].view(np.uint32) == lw[rest].view(np.uint32)).all()       # bitwise unchanged, NaN and -inf included
    sm = out[tail]
    assert (np.diff(sm) >= 0).all()                         # monotone in the input order
    assert sm.max() <= np.nanmax(lw)                        # never above the raw maximum
    assert sm.min() >= fit[2]                               # ... nor below the cutoff
    if name == "quarters":                                  # ties run through the cutoff and through the quartile
        assert lw[tail[0]] == fit[2] and (lw == fit[2]).sum() > 2
        q = tail[int(math.floor(M / 4 + 0.5)) - 1]
        assert (lw[tail] == lw[q]).sum() > 2
        # among equal weights the later particle is the larger: the tail takes the tied particles with the largest indices
        tied = np.flatnonzero(lw == fit[2])
        in_tail = np.isin(tied, tail)
        assert in_tail.any() and not in_tail.all() and (np.diff(in_tail.astype(int)) >= 0).all()
