"""gjx_pairwise_t_pick / gjx_pairwise_t_argmax, host side: the declarations (include/gjx.h <-> libgjx_hip.so <-> genjax_amd/_abi.py), and
what the wrappers and the two ffbs_* functions refuse before any device work."""
import ctypes
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from genjax_amd import _abi as A
from genjax_amd import kernels
from test_pairwise_pick_cpu import C_TYPES


@pytest.mark.parametrize("name,ret", [("gjx_pairwise_t_pick", "int"), ("gjx_pairwise_t_argmax", "int"),
                                      ("gjx_pairwise_t_argmax_workspace_bytes", "size_t")])
def test_header_library_and_abi_declare_the_calls(name, ret):
    from genjax_amd import _lib
    hdr, lib = open(os.path.join(os.path.dirname(HERE), "include", "gjx.h")).read(), _lib.load()
    args = re.sub(r"/\*.*?\*/", "", re.search(rf"\b{ret}\s+{name}\s*\(([^;]*)\);", hdr).group(1), flags=re.S).split(",")
    declared = [C_TYPES[a.strip().rsplit(" ", 1)[0]] for a in args]                # "const float* q" -> "const float*"
    restype = ctypes.c_int if ret == "int" else ctypes.c_size_t
    assert A.PROTOTYPES[name] == (restype, declared), name
    assert getattr(lib, name).argtypes == declared and getattr(lib, name).restype == restype


X = lambda d, n: torch.zeros((d, n))
BAD = [dict(dof=None), dict(dof=0.0), dict(dof=-1.0), dict(dof=float("inf")), dict(dof=float("nan")), dict(precision=0.0),
       dict(precision=torch.ones(2, 8)), dict(precision=1e30, dof=1e-30), dict(k=X(3, 8)), dict(q=X(33, 8), k=X(33, 8))]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join(f"{n}={'tensor' if isinstance(x, torch.Tensor) else x}" for n, x in b.items()))
def test_wrappers_refuse_before_any_device_work(bad):
    a = dict(dict(q=X(2, 8), k=X(2, 8), precision=1.0, dof=3.0), **bad)              # CPU tensors: a call that got through would fail
    with pytest.raises(ValueError):
        kernels.pairwise_t_pick(a["q"], a["k"], torch.zeros(a["q"].shape[1]), None, a["precision"], a["dof"])
    with pytest.raises(ValueError):
        kernels.pairwise_t_argmax(a["q"], a["k"], None, a["precision"], a["dof"])


def test_pick_refuses_its_uniforms_and_ffbs_a_precision_list_with_dof():
    with pytest.raises(ValueError):
        kernels.pairwise_t_pick(X(2, 8), X(2, 8), torch.zeros(9), dof=3.0)
    states, lw, prec = [X(2, 8)] * 3, [None] * 3, [torch.ones(2)] * 3
    for p, dof in ((prec, 3.0), (1.0, 0.0), (1.0, float("nan")), (0.0, 3.0)):
        with pytest.raises(ValueError):
            kernels.ffbs_sample_paths(states, lw, states, p, (0, 1), 4, dof=dof)
        with pytest.raises(ValueError):
            kernels.ffbs_map_path(states, lw, states, p, dof=dof)
