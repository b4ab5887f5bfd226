"""gjx_pairwise_gauss_mean, host side: the two declarations (include/gjx.h <-> libgjx_hip.so <-> genjax_amd/_abi.py), the shapes the
workspace call refuses, and the float64 restatement the GPU tests compare with (tests/pairwise_mean_ref.py) against plain loops."""
import ctypes
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from genjax_amd import _abi as A
from pairwise_mean_ref import pairwise_mean

C_TYPES = {"const float*": A.vp, "float*": A.vp, "void*": A.vp, "int64_t": A.i64, "int32_t": A.i32, "float": A.f32, "size_t": ctypes.c_size_t}


def test_header_library_and_abi_declare_the_calls():
    from genjax_amd import _lib
    hdr, lib = open(os.path.join(os.path.dirname(HERE), "include", "gjx.h")).read(), _lib.load()
    for name, ret in (("gjx_pairwise_gauss_mean_workspace_bytes", ("size_t", ctypes.c_size_t)), ("gjx_pairwise_gauss_mean", ("int", ctypes.c_int))):
        args = re.sub(r"/\*.*?\*/", "", re.search(rf"\b{ret[0]}\s+{name}\s*\(([^;]*)\);", hdr).group(1), flags=re.S).split(",")
        declared = [C_TYPES[a.strip().rsplit(" ", 1)[0]] for a in args]            # "const float* q" -> "const float*"
        assert A.PROTOTYPES[name] == (ret[1], declared), name
        assert getattr(lib, name).argtypes == declared and getattr(lib, name).restype == ret[1]
    need = lib.gjx_pairwise_gauss_mean_workspace_bytes
    assert need(64, 64, 8, 8) > 0 and need(64, 64, 33, 8) == 0 and need(64, 64, 8, 33) == 0 and need(64, 64, 8, 0) == 0


def test_restatement_is_the_double_loop():
    rs = np.random.default_rng(3)
    n_q, n_k, dv, d, p = 3, 4, 5, 2, 1.3
    q, k, v, b = rs.standard_normal((d, n_q)), rs.standard_normal((d, n_k)), rs.standard_normal((dv, n_k)), rs.standard_normal(n_k)
    mean, lse = pairwise_mean(q, k, v, b, p)
    for r in range(n_q):
        e = [np.exp(b[c] - 0.5 * p * sum((q[i, r] - k[i, c]) ** 2 for i in range(d))) for c in range(n_k)]
        np.testing.assert_allclose(lse[r], np.log(sum(e)), rtol=1e-13)
        for j in range(dv):
            np.testing.assert_allclose(mean[j, r], sum(e[c] * v[j, c] for c in range(n_k)) / sum(e), rtol=1e-12)


def test_values_equal_keys_and_a_huge_precision_return_the_nearest_key():
    rs = np.random.default_rng(4)
    q, k = rs.standard_normal((3, 20)), rs.standard_normal((3, 7))
    mean, _ = pairwise_mean(q, k, k, None, 1e6)
    nearest = ((q[:, :, None] - k[:, None, :]) ** 2).sum(0).argmin(1)
    np.testing.assert_allclose(mean, k[:, nearest], rtol=0, atol=1e-9)
