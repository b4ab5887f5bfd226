"""gjx_pairwise_gauss_argmax and gjx_pairwise_gauss_argmax_diag without a GPU: the declarations, the workspace queries and the refusals
made before any device work."""
import os
import re

import pytest
import torch

from genjax_amd import _abi as A
from genjax_amd import _lib, kernels

HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gjx.h")).read()
F32, F64, I32 = torch.float32, torch.float64, torch.int32


@pytest.mark.parametrize("name", ["gjx_pairwise_gauss_argmax_workspace_bytes", "gjx_pairwise_gauss_argmax",
                                  "gjx_pairwise_gauss_argmax_diag_workspace_bytes", "gjx_pairwise_gauss_argmax_diag"])
def test_header_abi_and_library_agree(name):
    decl = re.search(r"^(?:size_t|int) " + name + r"\(([^;]*)\);", HDR, re.M)
    assert decl and len(decl.group(1).split(",")) == len(A.PROTOTYPES[name][1]) and hasattr(_lib.load(), name)


def test_workspace_is_the_lse_workspace():
    lib = _lib.load()
    iso, diag = lib.gjx_pairwise_gauss_argmax_workspace_bytes, lib.gjx_pairwise_gauss_argmax_diag_workspace_bytes
    for n_q, n_k, d in [(64, 64, 8), (300, 5000, 16), (1, 1, 1), (1 << 14, 1 << 14, 8)]:
        assert iso(n_q, n_k, d) == diag(n_q, n_k, d) == lib.gjx_pairwise_gauss_lse_workspace_bytes(n_q, n_k, d) > 0
    assert iso(64, 64, 32) > 0 and [iso(64, 64, 33), iso(64, 64, 0), iso(0, 64, 8), iso(64, 0, 8), diag(64, 64, 17)] == [0] * 5


@pytest.mark.parametrize("kw", [
    dict(k=torch.zeros(4, 7)),                                                # queries have 3 components, keys 4
    dict(q=torch.zeros(33, 5), k=torch.zeros(33, 7)),                         # d > 32
    dict(q=torch.zeros(17, 5), k=torch.zeros(17, 7), precision=torch.ones(17, 7)),      # d > 16 with a precision matrix
    dict(precision=torch.ones(3, 5), precision_of="queries"),
    dict(precision=torch.ones(3, 5)),                                         # a matrix of the keys is f32[3][7]
    dict(precision=torch.ones(3, 7, dtype=F64)),
    dict(precision=0.0), dict(precision=-1.0), dict(precision=float("inf")), dict(precision=float("nan")),
    dict(bias=torch.zeros(5)),
    dict(out=torch.zeros(5, dtype=F32)), dict(out=torch.zeros(7, dtype=I32)),
    dict(max_out=torch.zeros(5, dtype=F64)), dict(max_out=torch.zeros(5, dtype=I32)),
])
def test_refuses_before_device_work(kw):
    args = dict(q=torch.zeros(3, 5), k=torch.zeros(3, 7))
    args.update(kw)
    with pytest.raises(ValueError):                         # 5 queries, 7 keys, on the CPU: anything but a refusal would fail otherwise
        kernels.pairwise_gauss_argmax(args.pop("q"), args.pop("k"), **args)


def test_map_path_refusals_before_device_work():
    from genjax_amd.inference.pf import ParticleHistory
    x, h = [torch.zeros(2, 6)] * 3, ParticleHistory()
    for prec, n in [([torch.ones(2, 6)] * 2, 3), ([torch.ones(2, 5)] * 3, 3), ([torch.ones(2, 6, dtype=F64)] * 3, 3), ([1.0] * 3, 3), (1.0, 2)]:
        with pytest.raises(ValueError):
            kernels.ffbs_map_path(x, [None] * n, x, prec)
    h.append(x[0], None)
    with pytest.raises(ValueError):                         # no model, no per-step weights
        h.map_path()
    h._moved = True
    with pytest.raises(NotImplementedError):
        h.map_path()
