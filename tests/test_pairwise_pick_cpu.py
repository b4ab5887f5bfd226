"""gjx_pairwise_gauss_pick, host side: the two declarations (include/gjx.h <-> libgjx_hip.so <-> genjax_amd/_abi.py), the shapes the
workspace call refuses, the argument checks of the Python calls (no device is touched), and the rule of tests/pairwise_pick_ref.py on a
three-key example worked by hand."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from genjax_amd import _abi as A
import pairwise_pick_ref as P

C_TYPES = {"const float*": A.vp, "float*": A.vp, "int32_t*": A.vp, "void*": A.vp, "int64_t": A.i64, "int32_t": A.i32, "float": A.f32,
           "size_t": ctypes.c_size_t}


def test_header_library_and_abi_declare_the_calls():
    from genjax_amd import _lib
    hdr, lib = open(os.path.join(os.path.dirname(HERE), "include", "gjx.h")).read(), _lib.load()
    for name, ret in (("gjx_pairwise_gauss_pick_workspace_bytes", ("size_t", ctypes.c_size_t)), ("gjx_pairwise_gauss_pick", ("int", ctypes.c_int))):
        args = re.sub(r"/\*.*?\*/", "", re.search(rf"\b{ret[0]}\s+{name}\s*\(([^;]*)\);", hdr).group(1), flags=re.S).split(",")
        declared = [C_TYPES[a.strip().rsplit(" ", 1)[0]] for a in args]            # "const float* q" -> "const float*"
        assert A.PROTOTYPES[name] == (ret[1], declared), name
        assert getattr(lib, name).argtypes == declared and getattr(lib, name).restype == ret[1]
    need = lib.gjx_pairwise_gauss_pick_workspace_bytes
    assert need(64, 64, 8) > lib.gjx_pairwise_gauss_lse_workspace_bytes(64, 64, 8) > 0
    assert need(64, 64, 33) == 0 and need(0, 64, 8) == 0 and need(64, 0, 8) == 0 and need(64, 64, 0) == 0 and A.ABI_VERSION == 11


def test_bad_arguments_raise_before_any_device_work():
    from genjax_amd import kernels
    from genjax_amd.inference.pf import LinearGaussianSSM, ParticleHistory
    q, k, u, z = torch.zeros((3, 8)), torch.zeros((3, 5)), torch.zeros(8), torch.zeros
    for bad in (dict(u=z(7)), dict(u=z(8, dtype=torch.float64)), dict(u=z(16)[::2]), dict(k_rows=z((2, 5))), dict(precision=0.0),
                dict(bias=z(4)), dict(centre=z(2)), dict(q_rows=z((33, 8)), k_rows=z((33, 5))), dict(out=z(8)), dict(lse_out=z(7))):
        with pytest.raises(ValueError):
            kernels.pairwise_gauss_pick(**{**dict(q_rows=q, k_rows=k, u=u), **bad})
    h = ParticleHistory()
    h.append(q, None, z(8))
    ssm = LinearGaussianSSM(np.eye(3, dtype=np.float32), 1.0, 1.0)
    for call, err in ((lambda: kernels.ffbs_sample_paths([q], [None], [q], 1.0, (0, 1), 0), ValueError),
                      (lambda: kernels.ffbs_sample_paths([q], [None, None], [q], 1.0, (0, 1), 4), ValueError),
                      (lambda: h.backward_paths((0, 1)), ValueError),                                   # no model
                      (lambda: (setattr(h, "ssm", ssm), h.backward_paths((0, 1), 0)), ValueError),
                      (lambda: (setattr(h, "logw_steps", []), h.backward_paths((0, 1))), ValueError),   # no per-step weights
                      (lambda: (setattr(h, "_moved", True), h.backward_paths((0, 1))), NotImplementedError)):
        with pytest.raises(err):
            call()


def test_the_rule_on_three_keys_by_hand():
    """one query at 0 in one dimension, keys at 0, 0 (dead) and 2 sqrt(log 2) with p = 1/2: masses 1, 0, 1/2 -> P = 2/3, 2/3, 1"""
    q, k, b = np.zeros((1, 4)), np.array([[0.0, 0.0, 2.0 * np.sqrt(np.log(2.0))]]), np.array([0.0, -np.inf, 0.0])
    np.testing.assert_allclose(P.windows(q, k, b, 0.5)[0], [0.0, 2 / 3, 2 / 3, 1.0], rtol=1e-14)
    u = np.array([0.5, 0.7, 2 / 3, np.nan])
    assert np.isnan(P.windows(q, k, b, 0.5, u)[3]).all()
    for pick, want in (([0, 2, 0, -1], 1), ([0, 2, 2, -1], 1), ([2, 0, 1, 0], 0), ([1, 1, -1, 2], 0)):
        ok, n_acc, slack = P.acceptable(np.array(pick), q, k, b, 0.5, u)
        assert list(ok) == [bool(want)] * 4 and list(n_acc) == [1, 1, 2, 0], pick
    assert P.acceptable(np.array([2, 2, 2, -1]), q, k, b, 0.5, u)[2][0] == pytest.approx((2 / 3 - 0.5) / P.tolerance(q, k, b, 0.5, None, 1.0)[0])
