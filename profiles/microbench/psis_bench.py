"""Times gjx_pareto_smooth against what a user writes today: torch.topk(logw, M + 1, sorted=True) and the same fit and smoothing in
torch float64 on the device.  Two shapes: one segment of K = 2^20 (M = 3072) and 1024 segments of 1024 (M = 96 each); exact Pareto
ratios with k = 0.7.  The two sides alternate in one process; device events around N back-to-back calls, warmed up, REPS
repetitions, medians.  torch.topk alone is timed as well: it is the part of the torch side that finds the tail.
Usage: python profiles/microbench/psis_bench.py [out.txt]"""
import math
import statistics
import sys

import numpy as np
import torch

from genjax_amd import kernels

REPS, N = 7, 20


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n          # us per call


def torch_psis(lw, M):
    """lw f32[S][n] -> (smoothed f32[S][n], k_hat f64[S]): the definition of include/gjx.h in torch (ties at the cutoff fall as topk
    leaves them)"""
    top, idx = torch.topk(lw, M + 1, dim=1, sorted=True)
    top, idx = top.flip(1).double(), idx.flip(1)
    c, mx = top[:, :1], top[:, -1:]
    ecut = torch.exp(c - mx)
    x = torch.exp(top[:, 1:] - mx) - ecut
    m = 30 + math.isqrt(M)
    xq = x[:, (M + 2) // 4 - 1:(M + 2) // 4]
    j = torch.arange(1, m + 1, dtype=torch.float64, device=lw.device)
    b = (1.0 - torch.sqrt(m / (j - 0.5)))[None, :] / (3.0 * xq) + 1.0 / x[:, -1:]
    k = torch.log1p(-b[:, :, None] * x[:, None, :]).mean(2)
    L = M * (torch.log(-b / k) - k - 1.0)
    w = torch.softmax(torch.where(torch.isfinite(L), L, torch.full_like(L, -math.inf)), 1)
    bh = (w * b).sum(1, keepdim=True)
    k0 = torch.log1p(-bh * x).mean(1, keepdim=True)
    sigma, kh = -k0 / bh, (M * k0 + 5.0) / (M + 10.0)
    l1 = torch.log1p(-(torch.arange(M, dtype=torch.float64, device=lw.device) + 0.5) / M)[None, :]
    q = sigma * torch.expm1(-kh * l1) / kh
    v = torch.clamp(torch.log(q + ecut), max=0.0) + mx
    out = lw.clone()
    out.scatter_(1, idx[:, 1:], v.float())
    return out, kh[:, 0]


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    rs = np.random.default_rng(1)
    for S, n in ((1, 1 << 20), (1024, 1024)):
        K, M = S * n, kernels.pareto_tail(n)
        lw = torch.from_numpy((-0.7 * np.log(rs.random(K)) - 1234.5).astype(np.float32)).cuda()
        lw2 = lw.view(S, n)
        ws = torch.empty(kernels.load().gjx_pareto_smooth_workspace_bytes(K, S), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(lw)

        def ours():
            return kernels.pareto_smooth(lw, S, ws, dst)

        def topk():
            return torch.topk(lw2, M + 1, dim=1, sorted=True)

        def theirs():
            return torch_psis(lw2, M)

        a, (b_out, b_k) = ours(), theirs()
        torch.cuda.synchronize()
        dk = float((a["k"].reshape(-1).double() - b_k).abs().max())
        same = float((a["logw"] == b_out.reshape(-1)).float().mean())
        print(f"# {S} segment(s) of {n}, M = {M}: k_hat {float(a['k'].reshape(-1)[0]):.4f}; max |k_hat - torch's| = {dk:.3g}; "
              f"{100 * same:.3f} % of the outputs equal torch's bit for bit", file=out)
        for fn in (ours, topk, theirs):
            timed(fn, 5)
        t = {"gjx_pareto_smooth": [], "torch.topk alone": [], "torch.topk + fit in float64": []}
        for _ in range(REPS):
            t["gjx_pareto_smooth"].append(timed(ours, N))
            t["torch.topk alone"].append(timed(topk, N))
            t["torch.topk + fit in float64"].append(timed(theirs, N))
        for name, v in t.items():
            print(f"{name:30s} {statistics.median(v):9.1f} us  ({min(v):.1f} .. {max(v):.1f})", file=out)
        out.flush()


if __name__ == "__main__":
    main()
