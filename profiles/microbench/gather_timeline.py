"""Phase stamps of k_resample_gather<4> at the bench shape (mixture step, K = 2^20, 17 rows), per block, us from the first block's start.
For every capture: the absolute time of each stamp (min / median / max over the 1024 blocks, and the value of the LAST block: the one
whose tile total is published last, every block waits for it), then the intervals of the head in front of the row copy (median over
the blocks, last block).
usage: python profiles/microbench/gather_timeline.py [captures, default 1]"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from genjax_amd import _abi as A, kernels, workloads
from genjax_amd._lib import load

K = 1 << 20
prog, _ = workloads.gmm_program()
ws = kernels.workspace(A.OP_RUN, K, "cuda")
ws2 = kernels.workspace(A.OP_RESAMPLE, K, "cuda")
out = kernels.run_program(prog, (0, 1), K, ws=ws, want_weight=False, want_lse=False)
n_part = kernels.run_partials_count(prog, K, 0)
rows = torch.empty_like(out["choices"])
lse = torch.empty(4, device="cuda")


def go():
    kernels.run_program(prog, (0, 2), K, ws=ws, out=out, want_weight=False, want_lse=False)
    kernels.resample_gather(out["logw"], 0.37, out["choices"], partials=(ws, n_part), lse_out=lse, out=rows, ws=ws2, allow_fallback=False)


for _ in range(20):
    go()
tl = torch.zeros((1024, 8), dtype=torch.int64, device="cuda")
load().gjx_debug_timeline(C.c_void_p(tl.data_ptr()), tl.numel() * tl.element_size())
STAMPS = [(0, "start"), (1, "tile total published"), (2, "totals gathered"), (6, "window boundaries"), (7, "source tiles found"),
          (3, "tile range known"), (4, "ancestors known"), (5, "rows copied (end)")]
NAMES = dict(STAMPS)
for cap in range(int(sys.argv[1]) if len(sys.argv) > 1 else 1):
    tl.zero_()
    go()
    torch.cuda.synchronize()
    t = tl.cpu().numpy().astype(np.float64) * 0.01           # 100 MHz clock -> us
    t -= t[:, 0].min()
    last = int(np.argmax(t[:, 1]))
    print(f"capture {cap}: last block to publish is {last}")
    for j, n in STAMPS:
        print(f"{n:24s} min {t[:, j].min():7.2f}  median {np.median(t[:, j]):7.2f}  max {t[:, j].max():7.2f}  last block {t[last, j]:7.2f} us")
    for a, b in ((0, 1), (1, 2), (2, 6), (6, 7), (7, 3), (3, 4)):
        d = t[:, b] - t[:, a]
        print(f"  {NAMES[a]} -> {NAMES[b]}: median {np.median(d):6.2f}  last block {d[last]:6.2f} us")
