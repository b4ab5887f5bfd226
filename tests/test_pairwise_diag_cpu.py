"""gjx_pairwise_gauss_lse_diag without a GPU: the declarations, the workspace query and the refusals made before any device work."""
import os
import re

import pytest
import torch

from genjax_amd import _abi as A
from genjax_amd import _lib, kernels

HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gjx.h")).read()
F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("name", ["gjx_pairwise_gauss_lse_diag_workspace_bytes", "gjx_pairwise_gauss_lse_diag"])
def test_header_abi_and_library_agree(name):
    decl = re.search(r"^(?:size_t|int) " + name + r"\(([^;]*)\);", HDR, re.M)
    assert decl and len(decl.group(1).split(",")) == len(A.PROTOTYPES[name][1]) and hasattr(_lib.load(), name)
    for macro, val in (("DIAG_MAX_DIM", A.PAIRWISE_DIAG_MAX_DIM), ("PREC_KEYS", A.PAIRWISE_PREC_KEYS), ("PREC_QUERIES", A.PAIRWISE_PREC_QUERIES)):
        assert f"#define GJX_PAIRWISE_{macro} {val}\n" in HDR


def test_workspace_query():
    need = _lib.load().gjx_pairwise_gauss_lse_diag_workspace_bytes
    assert need(64, 64, 8) == _lib.load().gjx_pairwise_gauss_lse_workspace_bytes(64, 64, 8) > 0
    assert [need(64, 64, 17), need(64, 64, 0), need(0, 64, 8), need(64, 0, 8)] == [0, 0, 0, 0]


@pytest.mark.parametrize("d,prec_shape,dtype,side", [(3, (3, 7), F64, "keys"), (3, (3, 5), F32, "keys"), (3, (3, 7), F32, "queries"),
                                                     (3, (2, 7), F32, "keys"), (3, (3, 7, 1), F32, "keys"), (17, (17, 7), F32, "keys"),
                                                     (3, (3, 7), F32, "both")])
def test_lse_refuses_before_device_work(d, prec_shape, dtype, side):
    with pytest.raises(ValueError):                         # 5 queries, 7 keys, on the CPU: anything but a refusal would fail otherwise
        kernels.pairwise_gauss_lse(torch.zeros(d, 5), torch.zeros(d, 7), None, torch.ones(prec_shape, dtype=dtype), precision_of=side)


@pytest.mark.parametrize("prec", [[torch.ones(2, 6)] * 2, [torch.ones(2, 5)] * 3, [torch.ones(3)] * 3, [torch.ones(2, 6, dtype=F64)] * 3,
                                  [1.0] * 3])
def test_ffbs_weights_refuses_before_device_work(prec):
    x = [torch.zeros(2, 6)] * 3
    with pytest.raises(ValueError):
        kernels.ffbs_weights(x, [None] * 3, x, prec)
