"""gjx_pairwise_gauss_mean_diag and gjx_pairwise_gauss_pick_diag without a GPU: the declarations, the workspace queries and the refusals
made before any device work."""
import os
import re

import pytest
import torch

from genjax_amd import _abi as A
from genjax_amd import _lib, kernels

HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gjx.h")).read()
F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("name", ["gjx_pairwise_gauss_mean_diag_workspace_bytes", "gjx_pairwise_gauss_mean_diag",
                                  "gjx_pairwise_gauss_pick_diag_workspace_bytes", "gjx_pairwise_gauss_pick_diag"])
def test_header_abi_and_library_agree(name):
    decl = re.search(r"^(?:size_t|int) " + name + r"\(([^;]*)\);", HDR, re.M)
    assert decl and len(decl.group(1).split(",")) == len(A.PROTOTYPES[name][1]) and hasattr(_lib.load(), name)


def test_workspace_queries():
    lib = _lib.load()
    mean, pick = lib.gjx_pairwise_gauss_mean_diag_workspace_bytes, lib.gjx_pairwise_gauss_pick_diag_workspace_bytes
    for n_q, n_k, d, dv in [(64, 64, 8, 8), (300, 5000, 16, 32), (1, 1, 1, 1)]:
        assert mean(n_q, n_k, d, dv) == lib.gjx_pairwise_gauss_mean_workspace_bytes(n_q, n_k, d, dv) > 0
        assert pick(n_q, n_k, d) == lib.gjx_pairwise_gauss_pick_workspace_bytes(n_q, n_k, d) > 0
    assert [mean(64, 64, 17, 8), mean(64, 64, 8, 33), mean(64, 64, 0, 8), mean(0, 64, 8, 8), mean(64, 0, 8, 8)] == [0] * 5
    assert [pick(64, 64, 17), pick(64, 64, 0), pick(0, 64, 8), pick(64, 0, 8)] == [0] * 4


@pytest.mark.parametrize("call", ["mean", "pick"])
@pytest.mark.parametrize("d,prec_shape,dtype,side", [(3, (3, 5), F32, "keys"), (3, (2, 7), F32, "keys"), (3, (3, 7, 1), F32, "keys"),
                                                     (3, (3, 7), F64, "keys"), (17, (17, 7), F32, "keys"), (3, (3, 7), F32, "queries"),
                                                     (3, (3, 5), F32, "queries"), (3, (3, 14), F32, "strided")])
def test_refuses_before_device_work(call, d, prec_shape, dtype, side):
    prec = torch.ones(prec_shape, dtype=dtype)
    if side == "strided":                                   # a view whose column stride is 2
        prec, side = prec[:, ::2], "keys"
    q, k = torch.zeros(d, 5), torch.zeros(d, 7)
    with pytest.raises(ValueError):                         # 5 queries, 7 keys, on the CPU: anything but a refusal would fail otherwise
        if call == "mean":
            kernels.pairwise_gauss_mean(q, k, torch.zeros(2, 7), None, prec, precision_of=side)
        else:
            kernels.pairwise_gauss_pick(q, k, torch.zeros(5), None, prec, precision_of=side)


@pytest.mark.parametrize("call", ["pair_moments", "sample_paths"])
@pytest.mark.parametrize("prec", [[torch.ones(2, 6)] * 2, [torch.ones(2, 5)] * 3, [torch.ones(3)] * 3, [torch.ones(2, 6, dtype=F64)] * 3,
                                  [1.0] * 3])
def test_ffbs_calls_refuse_before_device_work(call, prec):
    x = [torch.zeros(2, 6)] * 3
    with pytest.raises(ValueError):
        if call == "pair_moments":
            kernels.ffbs_pair_moments(x, [None] * 3, x, prec, weights=torch.ones(3, 6))
        else:
            kernels.ffbs_sample_paths(x, [None] * 3, x, prec, (0, 1), 4)
