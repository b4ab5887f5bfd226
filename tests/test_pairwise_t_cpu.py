"""gjx_pairwise_t_lse / gjx_pairwise_t_mean, host side: the two declarations (include/gjx.h <-> libgjx_hip.so <-> genjax_amd/_abi.py),
and what the wrappers refuse before any device work."""
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
from test_pairwise_mean_cpu import C_TYPES


def test_header_library_and_abi_declare_the_calls():
    from genjax_amd import _lib
    hdr, lib = open(os.path.join(os.path.dirname(HERE), "include", "gjx.h")).read(), _lib.load()
    for name in ("gjx_pairwise_t_lse", "gjx_pairwise_t_mean"):
        args = re.sub(r"/\*.*?\*/", "", re.search(rf"\bint\s+{name}\s*\(([^;]*)\);", hdr).group(1), flags=re.S).split(",")
        declared = [C_TYPES[a.strip().rsplit(" ", 1)[0]] for a in args]            # "const float* q" -> "const float*"
        assert A.PROTOTYPES[name] == (ctypes.c_int, declared), name
        assert getattr(lib, name).argtypes == declared and getattr(lib, name).restype == ctypes.c_int
        names = [a.split()[-1] for a in args]
        assert names[names.index("precision") + 1] == "dof", name


X = lambda d, n: torch.zeros((d, n))
BAD = [dict(dof=None), dict(dof=0.0), dict(dof=-1.0), dict(dof=float("inf")), dict(dof=float("nan")), dict(precision=0.0),
       dict(precision=float("inf")), dict(precision=1e30, dof=1e-30), dict(k=X(3, 8)), dict(q=X(33, 8), k=X(33, 8))]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join(f"{n}={'tensor' if isinstance(x, torch.Tensor) else x}" for n, x in b.items()))
def test_wrappers_refuse_before_any_device_work(bad):
    a = dict(dict(q=X(2, 8), k=X(2, 8), precision=1.0, dof=3.0), **bad)              # CPU tensors: a call that got through would fail
    with pytest.raises(ValueError):
        kernels.pairwise_t_lse(a["q"], a["k"], None, a["precision"], a["dof"])
    with pytest.raises(ValueError):
        kernels.pairwise_t_mean(a["q"], a["k"], X(2, a["k"].shape[1]), None, a["precision"], a["dof"])


def test_mean_refuses_its_values_and_ffbs_a_precision_list_with_dof():
    with pytest.raises(ValueError):
        kernels.pairwise_t_mean(X(2, 8), X(2, 8), X(33, 8), dof=3.0)
    with pytest.raises(ValueError):
        kernels.pairwise_t_mean(X(2, 8), X(2, 8), X(2, 9), dof=3.0)
    states, lw, prec = [X(2, 8)] * 3, [None] * 3, [torch.ones(2)] * 3
    for call in (kernels.ffbs_weights, kernels.ffbs_pair_moments):
        for p, dof in ((prec, 3.0), (1.0, 0.0), (1.0, float("nan")), (0.0, 3.0)):
            with pytest.raises(ValueError):
                call(states, lw, states, p, dof=dof)

