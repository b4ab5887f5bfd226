"""Times gjx_weighted_cross_moments against what the library and torch offer for the same pair moments.
  1. K = 2^20, n_a = n_b = 8, a resampled (sorted) index, two weight sets: general weights, and a coalesced lineage (about 1 % of
     the weights non-zero, the rest -inf).  Compared, alternating in one process:
       cross     kernels.weighted_cross_moments(a, b, logw, index)                                   (outputs allocated per call)
       compose   kernels.gather_rows(b, index) into rows 8..15 of a [16][K] buffer whose rows 0..7 hold a (copied once, outside the
                 window), then kernels.weighted_moments(buffer, logw, "cov"): the library's own composition before this call
       torch     b.index_select(1, index), w = softmax(logw), means by matmul, einsum("ik,k,jk->ij") on the centred rows
     and the results compared with each other.
  2. smoothed_pair_moments("x") on the history of a T = 256, K = 2^18, dx = 8 run of the generic filter (the history of
     lineage_bench.py), with the lineage weights kept and with them cleared before every call.
Device events around N back-to-back calls, warmed up, REPS repetitions, medians.  Usage: python profiles/microbench/cross_moments_bench.py [out.txt]"""
import statistics
import sys

import numpy as np
import torch

import genjax_amd as genjax
from genjax_amd import C, kernels, workloads
from genjax_amd.inference import BootstrapFilter

REPS = 5


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n          # us per call


def history(dx, T, K):
    s = workloads.ssm_problem(dx=dx, T=T)
    Am, q, r = np.asarray(s["A"], np.float32), float(s["q"]), float(s["r"])

    @genjax.gen
    def step(x_prev, _):
        x = genjax.mv_normal_diag(Am @ x_prev, np.full(dx, q, np.float32)) @ "x"
        genjax.mv_normal_diag(x, np.full(dx, r, np.float32)) @ "y"
        return x, None

    bf = BootstrapFilter(step.scan(n=T), K)
    out = bf.run(genjax.key(3), C["y"].set(np.asarray(s["y"], np.float32)), (np.zeros(dx, np.float32), None), keep_history=True)
    return out["history"]


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    K, n = 1 << 20, 8
    g = torch.Generator(device="cuda").manual_seed(1)
    b = torch.randn((n, K), device="cuda", generator=g) + 3.0
    index = torch.sort(torch.randint(0, K, (K,), device="cuda", generator=g)).values.to(torch.int32)
    a = 0.9 * b[:, index.long()] + 0.3 * torch.randn((n, K), device="cuda", generator=g)
    general = 2.0 * torch.randn(K, device="cuda", generator=g) - 37.0
    coalesced = torch.where(torch.rand(K, device="cuda", generator=g) < 0.01, general, torch.full_like(general, float("-inf")))
    stacked = torch.empty((2 * n, K), device="cuda")
    stacked[:n] = a
    idx64 = index.long()
    ws = torch.empty(kernels.load().gjx_weighted_cross_moments_workspace_bytes(n, n, K), dtype=torch.uint8, device="cuda")

    for label, logw in (("general weights", general), (f"coalesced lineage ({int(torch.isfinite(coalesced).sum())} of {K} weights non-zero)", coalesced)):
        def cross():
            return kernels.weighted_cross_moments(a, b, logw, index, ws)["cross"]

        def compose():
            kernels.gather_rows(b, index, dst=stacked[n:])
            return kernels.weighted_moments(stacked, logw, "cov")["cov"][:n, n:]

        def torch_lines():
            bg = b.index_select(1, idx64)
            w = torch.softmax(logw, dim=0)
            ma, mb = a @ w, bg @ w
            return torch.einsum("ik,k,jk->ij", a - ma[:, None], w, bg - mb[:, None])

        fns = (("cross", cross), ("compose", compose), ("torch", torch_lines))
        res = {name: fn() for name, fn in fns}                  # (warms every shape up)
        torch.cuda.synchronize()
        scale = float(res["cross"].abs().max())
        print(f"# {label}; K = {K}, n_a = n_b = {n}, sorted index; max |cross| {scale:.3g}; max |cross - compose| "
              f"{float((res['cross'] - res['compose']).abs().max()):.3g}, max |cross - torch| {float((res['cross'] - res['torch']).abs().max()):.3g}", file=out)
        ts = {name: [] for name, _ in fns}
        for _ in range(REPS):
            for name, fn in fns:
                ts[name].append(timed(fn, 50))
        for name, _ in fns:
            print(f"{name:8s} {statistics.median(ts[name]):9.1f} us per call  ({min(ts[name]):.1f} .. {max(ts[name]):.1f})", file=out)
        print(f"# compose / cross {statistics.median(ts['compose']) / statistics.median(ts['cross']):.2f}, "
              f"torch / cross {statistics.median(ts['torch']) / statistics.median(ts['cross']):.2f}", file=out)
        out.flush()
    del a, b, stacked, index, idx64, general, coalesced, ws
    torch.cuda.empty_cache()

    # ---- 2. the history ----
    T, K, dx = 256, 1 << 18, 8
    h = history(dx, T, K)

    def kept():
        return h.smoothed_pair_moments("x")

    def cleared():
        h._lineage_out = h._lineage_logw = None               # the whole path: lineage weights, log, T - 1 calls
        return h.smoothed_pair_moments("x")

    kept()
    torch.cuda.synchronize()
    tk, tc = [], []
    for _ in range(REPS):
        tk.append(timed(kept, 3))
        tc.append(timed(cleared, 3))
    print(f"# smoothed_pair_moments('x'), K = {K}, T = {T}, dx = {dx}; survivors at t = T-1, T-9, T/2, 0: "
          f"{[int(h.survivors()[t]) for t in (T - 1, T - 9, T // 2, 0)]}", file=out)
    print(f"weights kept     {statistics.median(tk):9.0f} us  ({min(tk):.0f} .. {max(tk):.0f})  = {statistics.median(tk) / (T - 1):.2f} us per pair", file=out)
    print(f"weights cleared  {statistics.median(tc):9.0f} us  ({min(tc):.0f} .. {max(tc):.0f})", file=out)


if __name__ == "__main__":
    main()
