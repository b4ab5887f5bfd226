"""Pairwise Gaussian log-sum-exp (gjx_pairwise_gauss_lse), host side: the C ABI's declarations (include/gjx.h <-> libgjx_hip.so <->
genjax_amd/_abi.py) and the float64 restatement the GPU tests compare with (tests/pairwise_ref.py), whose FFBSm recursion is checked
here against the smoothing formula written out as plain sums."""
import ctypes
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from genjax_amd import _abi as A
from pairwise_ref import ffbs_log_weights

NEW = ("gjx_pairwise_gauss_lse_workspace_bytes", "gjx_pairwise_gauss_lse")


def test_header_library_and_abi_declare_the_calls():
    from genjax_amd import _lib
    hdr, lib = open(os.path.join(os.path.dirname(HERE), "include", "gjx.h")).read(), _lib.load()
    assert re.search(r"\bsize_t\s+gjx_pairwise_gauss_lse_workspace_bytes\s*\(\s*int64_t\s+n_q\s*,\s*int64_t\s+n_k\s*,\s*int32_t\s+d\s*\)", hdr)
    assert re.search(r"\bint\s+gjx_pairwise_gauss_lse\s*\(", hdr) and "#define GJX_PAIRWISE_MAX_DIM 32" in hdr
    assert "#define GJX_ABI_VERSION 11" in hdr and A.ABI_VERSION == 11 and lib.gjx_version() == 11 and A.PAIRWISE_MAX_DIM == 32
    for name in NEW:
        assert name in A.PROTOTYPES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == A.PROTOTYPES[name][1]
    assert A.PROTOTYPES[NEW[0]] == (ctypes.c_size_t, [A.i64, A.i64, A.i32])
    assert A.PROTOTYPES[NEW[1]] == (ctypes.c_int, [A.vp, A.i64, A.i64, A.vp, A.i64, A.i64, A.i32, A.vp, A.f32, A.vp, A.vp, A.vp,
                                                   ctypes.c_size_t, A.vp])


def test_restatement_recursion_is_the_ffbsm_formula():
    """K = 7, T = 3: w_{t|T}^i = w_t^i sum_j w_{t+1|T}^j f(x_{t+1}^j | x_t^i) / sum_l w_t^l f(x_{t+1}^j | x_t^l), with loops"""
    rs = np.random.default_rng(7)
    K, T, d, p = 7, 3, 2, 1.7
    Amat = 0.8 * rs.standard_normal((d, d))
    states = [rs.standard_normal((d, K)) for _ in range(T)]
    logw = [rs.standard_normal(K) for _ in range(T)]
    means = [Amat @ x for x in states]
    f = lambda t, j, i: np.exp(-0.5 * p * ((states[t + 1][:, j] - means[t][:, i]) ** 2).sum())
    w = [np.exp(l) / np.exp(l).sum() for l in logw]
    sm = [None] * T
    sm[T - 1] = w[T - 1]
    for t in (1, 0):
        sm[t] = np.array([w[t][i] * sum(sm[t + 1][j] * f(t, j, i) / sum(w[t][l] * f(t, j, l) for l in range(K)) for j in range(K))
                          for i in range(K)])
    got = np.exp(ffbs_log_weights(states, logw, means, p))
    np.testing.assert_allclose(got, np.stack(sm), rtol=1e-12, atol=0)
    np.testing.assert_allclose(got.sum(1), 1.0, rtol=1e-13)
