"""Weighted quantiles and histograms (gjx_weighted_quantiles, gjx_weighted_histogram), host side: the C ABI's declarations
(include/gjx.h <-> libgjx_hip.so <-> genjax_amd/_abi.py), the workspace queries, every refusal that is decided before a launch, and
the restatement of the definition that the GPU tests compare with (``ref_quantile``, ``ref_hist``: NumPy, exact integers), itself
checked against ``np.quantile(..., method="inverted_cdf")`` and a hand-computed example.  No compute call is made here: the device
pointers handed to the library are never dereferenced by a call that refuses."""
import ctypes
import math
import os
import re
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

from genjax_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gjx_weighted_quantiles_workspace_bytes", "gjx_weighted_quantiles", "gjx_weighted_histogram_workspace_bytes", "gjx_weighted_histogram")
P = ctypes.c_void_p(0x1000)        # "some non-NULL pointer": a refusing call does not touch it
KEY_NAN = 0xFFC00000               # the one key of every NaN: above +inf


# ---- the definition, restated (include/gjx.h) ----
def ref_weights(logw, K):
    """the integer weights u_i = rint(exp(logw_i - M) 2^32) (float64 exp; np.rint rounds to nearest even) as int64: their sums are
    exact integers below 2^63 for K < 2^30; dead: 0"""
    assert K < 1 << 30
    if logw is None:
        return np.full(K, 1 << 32, np.int64)
    w = np.asarray(logw, np.float64)
    live = ~np.isnan(w) & (w > -np.inf)
    if not live.any() or np.isinf(w[live].max()):
        return np.zeros(K, np.int64)
    e = np.where(live, np.exp(np.where(live, w, 0.0) - w[live].max()), 0.0)
    return np.rint(e * 2.0 ** 32).astype(np.int64)


def ref_keys(x):
    """order-preserving keys of float32 values: -0.0 folded onto +0.0, every NaN onto KEY_NAN, then bits ^ (sign ? ~0 : 1 << 31)"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    b = np.where(b == 0x80000000, 0, b)
    k = np.where(b & 0x80000000, b ^ 0xFFFFFFFF, b ^ 0x80000000)
    return np.where((b & 0x7FFFFFFF) > 0x7F800000, KEY_NAN, k)


def ref_value(key):
    key = int(key)
    bits = key ^ 0x80000000 if key & 0x80000000 else key ^ 0xFFFFFFFF
    return np.array([bits], np.uint32).view(np.float32)[0]


def ref_quantile(x, logw, q):
    """float32[len(q)]: for each level the smallest value v among the live particles with sum of u over {x_i <= v} >= t,
    t = max(1, ceil(q U)) in exact arithmetic (integers and a Fraction); NaN for a collection without weight"""
    x = np.asarray(x, np.float32)
    u = ref_weights(logw, x.size)
    U = int(u.sum())
    qs = np.atleast_1d(np.asarray(q, np.float32))
    if U == 0:
        return np.full(qs.size, np.nan, np.float32)
    keys = ref_keys(x)
    order = np.argsort(keys, kind="stable")
    run = np.cumsum(u[order])                      # exact: int64
    out = np.empty(qs.size, np.float32)
    for j, lv in enumerate(qs):
        t = min(max(1, math.ceil(Fraction(float(lv)) * U)), U)
        i = order[int(np.searchsorted(run, t, side="left"))]          # the first particle at which the running sum reaches t: a live one
        assert u[i] > 0
        out[j] = ref_value(keys[i])
    return out


def ref_bins(x, lo, hi, n_bins):
    """entry of every value: 0 below lo; n_bins + 1 at or above hi, for NaN and for b >= n_bins; else 1 + floor((x - lo) * scale),
    every operation rounded to float32 on its own"""
    x = np.asarray(x, np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    scale = np.float32(n_bins) / np.float32(hi - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        b = np.floor(((x - lo).astype(np.float32) * scale).astype(np.float32))
        inner = np.where(b < n_bins, 1 + np.nan_to_num(b, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64), n_bins + 1)
        return np.where(x < lo, 0, np.where(~(x < hi), n_bins + 1, inner))


def ref_hist(x, logw, lo, hi, n_bins):
    """(counts int64[n_bins + 2], U, mass float32[n_bins + 2] = the integer ratio rounded to double, then to float)"""
    x = np.asarray(x, np.float32)
    u = ref_weights(logw, x.size)
    counts = np.zeros(n_bins + 2, np.int64)
    np.add.at(counts, ref_bins(x, lo, hi, n_bins), u)
    U = int(u.sum())
    mass = np.array([int(c) / U for c in counts], np.float64).astype(np.float32) if U else np.full(n_bins + 2, np.nan, np.float32)
    return counts, U, mass


def test_restatement_equals_numpy_inverted_cdf_for_equal_weights():
    """(sizes at which q K is an integer for the dyadic levels only: next to an integer the float32 level decides, exactly here and
    up to a rounding of n q in NumPy)"""
    rs = np.random.default_rng(7)
    for K in (1, 2, 5, 64, 1001):
        for x in (rs.standard_normal(K), rs.integers(0, 3, K), np.full(K, 2.5)):
            x = np.asarray(x, np.float32)
            for q in (0.0, 0.1, 0.125, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.9, 1.0):
                q32 = float(np.float32(q))
                got = ref_quantile(x, None, [q32])[0]
                assert got == np.quantile(x, q32, method="inverted_cdf"), (K, q)
                assert got == ref_quantile(x, np.zeros(K, np.float32), [q32])[0]


def test_restatement_on_a_hand_computed_example():
    """values 3 1 2 5 4 0 with weights 1 1/2 1/4 1 1/2 1/4 (total 3.5): sorted, the running weights are
    0: 0.25, 1: 0.75, 2: 1.0, 3: 2.0, 4: 2.5, 5: 3.5"""
    x = np.array([3, 1, 2, 5, 4, 0], np.float32)
    logw = np.log(np.array([1, 0.5, 0.25, 1, 0.5, 0.25])).astype(np.float32) - 3.0
    u = ref_weights(logw, 6)
    assert u[0] == u[3] == 1 << 32 and abs(u[1] - (1 << 31)) < 256 and abs(u[2] - (1 << 30)) < 256
    levels = [0.0, 0.05, 0.1, 0.25, 0.5, 0.6, 0.75, 1.0]        # q * 3.5 = 0, .175, .35, .875, 1.75, 2.1, 2.625, 3.5
    np.testing.assert_array_equal(ref_quantile(x, logw, levels), np.array([0, 0, 1, 2, 3, 4, 5, 5], np.float32))
    # a dead particle is not there, whatever its value; an unordered list of levels is answered in its order
    logw2 = np.concatenate([logw, np.array([-np.inf, np.nan], np.float32)])
    x2 = np.concatenate([x, np.array([-7.0, np.nan], np.float32)])
    np.testing.assert_array_equal(ref_quantile(x2, logw2, [1.0, 0.0, 0.5]), np.array([5, 0, 3], np.float32))
    counts, U, mass = ref_hist(x2, logw2, 0.5, 4.5, 4)
    assert U == int(u.sum()) and list(counts) == [u[5], u[1], u[2], u[0], u[4], u[3]]
    np.testing.assert_allclose(mass, np.array([0.25, 0.5, 0.25, 1, 0.5, 1]) / 3.5, rtol=1e-6)
    assert np.isnan(ref_quantile(x, np.full(6, -np.inf, np.float32), [0.5])).all()


def test_restatement_orders_special_values():
    x = np.array([np.nan, np.inf, 1e-45, 0.0, -0.0, -1e-45, -np.inf, 1.0, -1.0, 2e-45], np.float32)
    k = ref_keys(x)
    assert k[3] == k[4] and k[0] == KEY_NAN and list(np.argsort(k, kind="stable")) == [6, 8, 5, 3, 4, 2, 9, 7, 1, 0]
    q = ref_quantile(x, None, [0.0, 0.5, 0.9, 1.0])
    assert q[0] == -np.inf and q[1].view(np.uint32) == 0 and q[2] == np.inf and q[3].view(np.uint32) == 0x7FC00000
    # (-1e-45 + 1 rounds to 1 in float32: the denormal below zero shares the bin of zero)
    np.testing.assert_array_equal(ref_bins(x, -1.0, 1.0, 4), [5, 5, 3, 3, 3, 3, 0, 5, 1, 3])


# ---- declarations ----
def _header():
    return open(os.path.join(ROOT, "include", "gjx.h")).read()


def _lib():
    from genjax_amd import _lib
    return _lib.load()


def _levels(*v):
    return (ctypes.c_float * len(v))(*v)


def _q(rows=P, stride=64, n_rows=2, logw=P, K=64, S=1, levels=(0.5,), n_levels=None, stats=P, out=P, ws=P, ws_bytes=1 << 30):
    lv = None if levels is None else _levels(*levels)
    return _lib().gjx_weighted_quantiles(rows, stride, n_rows, logw, K, S, lv, len(levels) if n_levels is None else n_levels, stats, out,
                                         ws, ws_bytes, None)


def _h(rows=P, stride=64, n_rows=2, logw=P, K=64, S=1, lo=0.0, hi=1.0, n_bins=8, stats=P, mass=P, ws=P, ws_bytes=1 << 30):
    return _lib().gjx_weighted_histogram(rows, stride, n_rows, logw, K, S, lo, hi, n_bins, stats, mass, ws, ws_bytes, None)


def test_header_declares_and_library_exports_the_calls():
    hdr, lib = _header(), _lib()
    assert re.search(r"\bsize_t\s+gjx_weighted_quantiles_workspace_bytes\s*\(", hdr)
    assert re.search(r"\bint\s+gjx_weighted_quantiles\s*\(", hdr)
    assert re.search(r"\bsize_t\s+gjx_weighted_histogram_workspace_bytes\s*\(", hdr)
    assert re.search(r"\bint\s+gjx_weighted_histogram\s*\(", hdr)
    for name in NEW:
        assert name in A.PROTOTYPES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == A.PROTOTYPES[name][1]
    assert A.PROTOTYPES["gjx_weighted_quantiles_workspace_bytes"] == (ctypes.c_size_t, [A.i32, A.i64, A.i64, A.i32])
    assert A.PROTOTYPES["gjx_weighted_histogram_workspace_bytes"] == (ctypes.c_size_t, [A.i32, A.i64, A.i64, A.i32])
    assert A.PROTOTYPES["gjx_weighted_quantiles"] == (ctypes.c_int, [A.vp, A.i64, A.i32, A.vp, A.i64, A.i64, A.vp, A.i32, A.vp, A.vp, A.vp,
                                                                     ctypes.c_size_t, A.vp])
    assert A.PROTOTYPES["gjx_weighted_histogram"] == (ctypes.c_int, [A.vp, A.i64, A.i32, A.vp, A.i64, A.i64, A.f32, A.f32, A.i32, A.vp, A.vp,
                                                                     A.vp, ctypes.c_size_t, A.vp])


def test_abi_version_is_unchanged():
    assert "#define GJX_ABI_VERSION 11" in _header() and A.ABI_VERSION == 11 and _lib().gjx_version() == 11


def test_caps_match_the_header():
    hdr = _header()
    m = re.search(r"#define\s+GJX_QUANTILES_MAX_LEVELS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == A.QUANTILES_MAX_LEVELS == 16
    m = re.search(r"#define\s+GJX_HISTOGRAM_MAX_BINS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == A.HISTOGRAM_MAX_BINS == 4096


def test_workspace_queries_are_positive_and_monotone():
    lib = _lib()
    Ks = [1, 63, 1024, 1025, 1500, 1 << 14, 1 << 20, (1 << 20) + 1]
    for q, sizes_of, cap in ((lib.gjx_weighted_quantiles_workspace_bytes, (1, 2, 3, 16), A.QUANTILES_MAX_LEVELS),
                             (lib.gjx_weighted_histogram_workspace_bytes, (1, 2, 64, 4096), A.HISTOGRAM_MAX_BINS)):
        for n_rows in (1, 3, 17):
            for n in sizes_of:
                sizes = [q(n_rows, K, 1, n) for K in Ks]
                assert sizes[0] > 0 and sizes == sorted(sizes), (n_rows, n, sizes)
        sizes = [q(n, 1 << 14, 1, 3) for n in range(1, 19)]
        assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes
        sizes = [q(3, 1 << 14, 1, n) for n in range(1, 17)]
        assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes
        assert q(3, 2500, 50, 3) > q(3, 2500, 1, 3) > 0                       # every segment has its own counters
        # arguments the call refuses
        for args in ((0, 64, 1, 3), (2, 0, 1, 3), (2, -64, 1, 3), (2, 64, 0, 3), (2, 64, 3, 3), (2, 64, 1, 0), (2, 64, 1, -1), (2, 64, 1, cap + 1)):
            assert q(*args) == 0, args
        assert q(2, 64, 1, cap) > 0


def test_quantile_refusals_need_no_device():
    lib = _lib()
    assert _q(rows=None) == A.EINVAL
    assert _q(stats=None) == A.EINVAL
    assert _q(out=None) == A.EINVAL
    assert _q(ws=None) == A.EINVAL
    assert _q(levels=None, n_levels=1) == A.EINVAL
    assert _q(K=0) == A.EINVAL
    assert _q(K=-5) == A.EINVAL
    assert _q(n_rows=0) == A.EINVAL
    assert _q(stride=63) == A.EINVAL                        # rows would overlap
    assert _q(S=0) == A.EINVAL
    assert _q(S=3) == A.EINVAL                              # 3 does not divide 64
    assert _q(n_levels=0) == A.EINVAL
    assert _q(n_levels=-1) == A.EINVAL
    for bad in (-0.25, 1.5, float("nan"), float("inf")):
        assert _q(levels=(0.5, bad, 0.25)) == A.EINVAL, bad
    assert b"gjx_weighted_quantiles" in lib.gjx_last_error()
    assert _q(logw=None, ws_bytes=0) == A.EWORKSPACE        # (NULL log-weights are equal weights, not a refusal)
    need = lib.gjx_weighted_quantiles_workspace_bytes(2, 64, 1, 3)
    assert _q(levels=(0.0, 0.5, 1.0), ws_bytes=need - 1) == A.EWORKSPACE
    assert b"workspace" in lib.gjx_last_error()


def test_histogram_refusals_need_no_device():
    lib = _lib()
    assert _h(rows=None) == A.EINVAL
    assert _h(stats=None) == A.EINVAL
    assert _h(mass=None) == A.EINVAL
    assert _h(ws=None) == A.EINVAL
    assert _h(K=0) == A.EINVAL
    assert _h(n_rows=0) == A.EINVAL
    assert _h(stride=63) == A.EINVAL
    assert _h(S=0) == A.EINVAL
    assert _h(S=3) == A.EINVAL
    assert _h(n_bins=0) == A.EINVAL
    assert _h(n_bins=-4) == A.EINVAL
    assert _h(lo=1.0, hi=1.0) == A.EINVAL
    assert _h(lo=2.0, hi=1.0) == A.EINVAL
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert _h(lo=bad) == A.EINVAL and _h(hi=bad) == A.EINVAL, bad
    assert b"gjx_weighted_histogram" in lib.gjx_last_error()
    need = lib.gjx_weighted_histogram_workspace_bytes(2, 64, 1, 8)
    assert _h(ws_bytes=need - 1) == A.EWORKSPACE
    assert b"workspace" in lib.gjx_last_error()


def test_over_the_caps_is_unsupported_and_says_the_cap():
    lib = _lib()
    cap = A.QUANTILES_MAX_LEVELS
    assert _q(levels=(0.5,) * cap, ws_bytes=0) == A.EWORKSPACE              # the cap itself is taken
    assert _q(levels=(0.5,) * (cap + 1)) == A.EUNSUPPORTED
    msg = lib.gjx_last_error().decode()
    assert str(cap) in msg and "GJX_QUANTILES_MAX_LEVELS" in msg, msg
    assert _q(levels=(0.5,) * (cap + 1), K=0) == A.EINVAL                   # a bad argument of such a call is still a bad argument
    cap = A.HISTOGRAM_MAX_BINS
    assert _h(n_bins=cap, ws_bytes=0) == A.EWORKSPACE
    assert _h(n_bins=cap + 1) == A.EUNSUPPORTED
    msg = lib.gjx_last_error().decode()
    assert str(cap) in msg and "GJX_HISTOGRAM_MAX_BINS" in msg, msg
    assert _h(n_bins=cap + 1, K=0) == A.EINVAL


def test_kernel_wrappers_refuse_before_they_reach_the_library():
    import torch
    from genjax_amd import kernels
    x = torch.zeros((3, 8))
    with pytest.raises(ValueError, match=r"at most %d\b" % A.QUANTILES_MAX_LEVELS):
        kernels.weighted_quantiles(x, None, [0.5] * (A.QUANTILES_MAX_LEVELS + 1))
    with pytest.raises(ValueError, match="levels"):
        kernels.weighted_quantiles(x, None, [0.5, 1.25])
    with pytest.raises(ValueError, match="levels"):
        kernels.weighted_quantiles(x, None, float("nan"))
    with pytest.raises(ValueError, match="no level"):
        kernels.weighted_quantiles(x, None, [])
    with pytest.raises(ValueError, match="column stride"):
        kernels.weighted_quantiles(torch.zeros((8, 6)).t(), None, 0.5)
    with pytest.raises(ValueError, match="segments"):
        kernels.weighted_quantiles(x, None, 0.5, n_segments=3)
    with pytest.raises(ValueError, match="logw"):
        kernels.weighted_quantiles(x, torch.zeros(7), 0.5)
    with pytest.raises(ValueError, match=r"at most %d\b" % A.HISTOGRAM_MAX_BINS):
        kernels.weighted_histogram(x, None, A.HISTOGRAM_MAX_BINS + 1, (0.0, 1.0))
    with pytest.raises(ValueError, match="bins"):
        kernels.weighted_histogram(x, None, 0, (0.0, 1.0))
    with pytest.raises(ValueError, match="range"):
        kernels.weighted_histogram(x, None, 8, (1.0, 1.0))
    with pytest.raises(ValueError, match="range"):
        kernels.weighted_histogram(x, None, 8, (0.0, float("inf")))
    with pytest.raises(ValueError, match="range"):
        kernels.weighted_histogram(x, None, 8)
    with pytest.raises(ValueError, match="column stride"):
        kernels.weighted_histogram(torch.zeros((8, 6)).t(), None, 8, (0.0, 1.0))
    with pytest.raises(ValueError, match="segments"):
        kernels.weighted_histogram(x, None, 8, (0.0, 1.0), n_segments=3)


def test_particle_collection_refuses_before_the_library():
    import torch
    from genjax_amd.gen import Trace
    from genjax_amd.inference import ParticleCollection
    from genjax_amd.program import SiteList
    sl = SiteList()
    sl.add("x", A.NORMAL, [0.0, 1.0])
    prog = SimpleNamespace(site_list=sl, slot_of={"x": 0}, rng_mode=A.RNG_FLAT)
    tr = Trace(None, (), prog, torch.zeros((1, 4)), torch.zeros(4), {}, True)
    pc = ParticleCollection(tr, torch.zeros(4))
    with pytest.raises(ValueError, match="neither a flip nor a categorical"):
        pc.probabilities("x")                               # a continuous site
    with pytest.raises(KeyError):
        pc.probabilities("nope")
    with pytest.raises(KeyError):
        pc.quantile("nope", 0.5)
    with pytest.raises(ValueError, match="levels"):
        pc.quantile("x", 1.5)
    with pytest.raises(ValueError, match="levels"):
        pc.quantile("x", [0.5] * (A.QUANTILES_MAX_LEVELS + 1))
    with pytest.raises(ValueError, match="mass"):
        pc.credible_interval("x", 1.5)
    with pytest.raises(ValueError, match="range"):
        pc.histogram("x", 8, (1.0, 0.0))
