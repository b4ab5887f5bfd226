"""Weighted posterior moments (gjx_weighted_moments), host side: the C ABI's declarations (include/gjx.h <-> libgjx_hip.so <->
genjax_amd/_abi.py), the workspace query and every refusal that is decided before a launch.  No compute call is made here: the
pointers handed to the library are never dereferenced by a call that refuses."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from genjax_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gjx_weighted_moments_workspace_bytes", "gjx_weighted_moments")
P = ctypes.c_void_p(0x1000)        # "some non-NULL pointer": a refusing call does not touch it


def _header():
    return open(os.path.join(ROOT, "include", "gjx.h")).read()


def _lib():
    from genjax_amd import _lib
    return _lib.load()


def _call(rows=P, stride=64, n_rows=2, logw=P, K=64, S=1, want=A.MOMENTS_VAR, stats=P, mean=P, second=P, ws=P, ws_bytes=1 << 30):
    return _lib().gjx_weighted_moments(rows, stride, n_rows, logw, K, S, want, stats, mean, second, ws, ws_bytes, None)


def test_header_declares_and_library_exports_the_moments_calls():
    hdr, lib = _header(), _lib()
    assert re.search(r"\bsize_t\s+gjx_weighted_moments_workspace_bytes\s*\(", hdr)
    assert re.search(r"\bint\s+gjx_weighted_moments\s*\(", hdr)
    for name in NEW:
        assert name in A.PROTOTYPES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == A.PROTOTYPES[name][1]
    assert A.PROTOTYPES["gjx_weighted_moments_workspace_bytes"] == (ctypes.c_size_t, [A.i32, A.i64, A.i64, A.i32])
    assert A.PROTOTYPES["gjx_weighted_moments"] == (ctypes.c_int, [A.vp, A.i64, A.i32, A.vp, A.i64, A.i64, A.i32, A.vp, A.vp, A.vp, A.vp,
                                                                   ctypes.c_size_t, A.vp])


def test_abi_version_is_unchanged():
    assert "#define GJX_ABI_VERSION 11" in _header() and A.ABI_VERSION == 11 and _lib().gjx_version() == 11


def test_constants_match_the_header():
    hdr = _header()
    for name, val in (("GJX_MOMENTS_MEAN", A.MOMENTS_MEAN), ("GJX_MOMENTS_VAR", A.MOMENTS_VAR), ("GJX_MOMENTS_COV", A.MOMENTS_COV)):
        m = re.search(name + r"\s*=\s*(\d+)", hdr)
        assert m and int(m.group(1)) == val, name
    m = re.search(r"#define\s+GJX_MOMENTS_MAX_COV_ROWS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == A.MOMENTS_MAX_COV_ROWS and A.MOMENTS_MAX_COV_ROWS >= 16


def test_workspace_query_is_positive_and_monotone():
    q = _lib().gjx_weighted_moments_workspace_bytes
    Ks = [1, 63, 1024, 1025, 1500, 1 << 14, 1 << 20, (1 << 20) + 1]
    for want in (A.MOMENTS_MEAN, A.MOMENTS_VAR, A.MOMENTS_COV):
        for n_rows in (1, 3, 16):
            sizes = [q(n_rows, K, 1, want) for K in Ks]
            assert sizes[0] > 0 and sizes == sorted(sizes), (want, n_rows, sizes)
            assert q(n_rows, 1025, 1, want) > q(n_rows, 1024, 1, want)          # one tile more
        sizes = [q(n, 1 << 14, 1, want) for n in range(1, 17)]
        assert all(b > a for a, b in zip(sizes, sizes[1:])), (want, sizes)
    assert q(17, 1 << 20, 1, A.MOMENTS_VAR) > q(16, 1 << 20, 1, A.MOMENTS_VAR) > 0       # means and variances: any n_rows
    # segments that do not fall on tile boundaries cost a tile each
    assert q(3, 2500, 50, A.MOMENTS_VAR) >= q(3, 2500, 1, A.MOMENTS_VAR) > 0
    # arguments the call refuses
    for args in ((0, 64, 1, 1), (2, 0, 1, 1), (2, 64, 0, 1), (2, 64, 3, 1), (2, 64, 1, 3), (2, 64, 1, -1), (17, 64, 1, A.MOMENTS_COV)):
        assert q(*args) == 0, args


def test_refusals_need_no_device():
    lib = _lib()
    assert _call(rows=None) == A.EINVAL
    assert _call(stats=None) == A.EINVAL
    assert _call(mean=None) == A.EINVAL
    assert _call(ws=None) == A.EINVAL
    assert _call(second=None, want=A.MOMENTS_VAR) == A.EINVAL
    assert _call(second=None, want=A.MOMENTS_COV) == A.EINVAL
    assert _call(K=0) == A.EINVAL
    assert _call(K=-5) == A.EINVAL
    assert _call(n_rows=0) == A.EINVAL
    assert _call(stride=63) == A.EINVAL                     # rows would overlap
    assert _call(S=0) == A.EINVAL
    assert _call(S=3) == A.EINVAL                           # 3 does not divide 64
    assert _call(want=3) == A.EINVAL
    assert _call(want=-1) == A.EINVAL
    assert b"gjx_weighted_moments" in lib.gjx_last_error()
    need = lib.gjx_weighted_moments_workspace_bytes(2, 64, 1, A.MOMENTS_VAR)
    assert _call(ws_bytes=need - 1) == A.EWORKSPACE
    assert b"workspace" in lib.gjx_last_error()


def test_covariance_over_the_cap_is_unsupported_and_says_the_cap():
    lib = _lib()
    cap = A.MOMENTS_MAX_COV_ROWS
    assert _call(n_rows=cap + 1, want=A.MOMENTS_COV) == A.EUNSUPPORTED
    msg = lib.gjx_last_error().decode()
    assert str(cap) in msg and "GJX_MOMENTS_MAX_COV_ROWS" in msg, msg
    # a bad argument of such a call is still a bad argument
    assert _call(n_rows=cap + 1, want=A.MOMENTS_COV, K=0) == A.EINVAL


def test_particle_collection_covariance_refuses_a_site_over_the_cap():
    import torch
    from genjax_amd.gen import Trace
    from genjax_amd.inference import ParticleCollection
    from genjax_amd.program import SiteList
    dim = A.MOMENTS_MAX_COV_ROWS + 1
    sl = SiteList()
    sl.add("x", A.MVNORMAL_DIAG, [np.zeros(dim, np.float32), np.ones(dim, np.float32)])
    assert sl["x"].dim == dim
    prog = SimpleNamespace(site_list=sl, slot_of={"x": 0}, rng_mode=A.RNG_FLAT)
    tr = Trace(None, (), prog, torch.zeros((dim, 4)), torch.zeros(4), {}, True)
    pc = ParticleCollection(tr, torch.zeros(4))
    with pytest.raises(ValueError, match=r"at most %d\b" % A.MOMENTS_MAX_COV_ROWS):
        pc.covariance("x")
    with pytest.raises(KeyError):
        pc.covariance("nope")


def test_kernel_wrapper_refuses_before_it_reaches_the_library():
    import torch
    from genjax_amd import kernels
    x = torch.zeros((A.MOMENTS_MAX_COV_ROWS + 1, 8))
    with pytest.raises(ValueError, match=r"at most %d\b" % A.MOMENTS_MAX_COV_ROWS):
        kernels.weighted_moments(x, None, "cov")
    with pytest.raises(ValueError, match="want"):
        kernels.weighted_moments(x, None, "skew")
    with pytest.raises(ValueError, match="column stride"):
        kernels.weighted_moments(torch.zeros((8, 6)).t(), None, "var")
    with pytest.raises(ValueError, match="segments"):
        kernels.weighted_moments(x, None, "var", n_segments=3)
