"""Times gjx_pairwise_gauss_pick and backward simulation (FFBSi) built on it.
  1. one call at d = 8 for n_q = n_k = 2^12, 2^14 (random particles, normalised random log-weights as bias, random uniforms) against
     gjx_pairwise_gauss_lse on the same inputs (the two alternate inside every repetition), and the share of picks that agree with
     torch's float32 inverse CDF  (torch.cumsum(torch.softmax(scores, 1), 1) >= u).argmax(1)  (a check of the workload, not a test).
  2. h.backward_paths(key) (K paths) on one T = 64, K = 2^14, dx = 8 history of the hand-written filter, and the number of distinct
     particles the paths visit at t = 1 against h.paths().
Device events around N back-to-back calls, warmed up, REPS repetitions, medians.  Usage: python profiles/microbench/pairwise_pick_bench.py [out.txt]"""
import statistics
import sys

import torch

from genjax_amd import core, kernels, workloads
from genjax_amd.inference.pf import BootstrapFilter, LinearGaussianSSM

REPS, D, P = 7, 8, 1.3


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n          # us per call


def med(ts):
    return f"{statistics.median(ts):9.1f} ({min(ts):.1f} .. {max(ts):.1f})"


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    g = torch.Generator(device="cuda").manual_seed(1)
    print(f"# gjx_pairwise_gauss_pick, d = {D}, n_q = n_k = n; {torch.cuda.get_device_name(0)}", file=out)
    print("        n  pick_us (min .. max)   lse_us (min .. max)  pick/lse  agree with torch", file=out)
    for lg in (12, 14):
        n = 1 << lg
        q, k = (torch.randn((D, n), device="cuda", generator=g) for _ in range(2))
        bias = torch.log_softmax(torch.randn(n, device="cuda", generator=g), 0)
        u = torch.rand(n, device="cuda", generator=g)
        lib = kernels.load()
        ws = torch.empty(lib.gjx_pairwise_gauss_pick_workspace_bytes(n, n, D), dtype=torch.uint8, device="cuda")
        ws_l = torch.empty(lib.gjx_pairwise_gauss_lse_workspace_bytes(n, n, D), dtype=torch.uint8, device="cuda")
        res, lse, res_l = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        pick = lambda: kernels.pairwise_gauss_pick(q, k, u, bias, P, None, ws, out=res, lse_out=lse)
        only = lambda: kernels.pairwise_gauss_lse(q, k, bias, P, None, ws_l, out=res_l)
        pick(), only()
        theirs = (torch.cumsum(torch.softmax(bias - 0.5 * P * torch.cdist(q.t(), k.t()) ** 2, 1), 1) >= u[:, None]).to(torch.int8).argmax(1)
        agree = float((theirs == pick()["pick"]).float().mean())
        del theirs
        torch.cuda.synchronize()
        tp, tl = [], []
        for _ in range(REPS):
            tp.append(timed(pick, 50))
            tl.append(timed(only, 50))
        print(f"{n:9d}  {med(tp)}  {med(tl)}  {statistics.median(tp) / statistics.median(tl):8.2f}  {agree:.5f}", file=out)
        out.flush()
        del q, k, bias, u, ws, ws_l, res, lse, res_l
        torch.cuda.empty_cache()

    T, K, dx = 64, 1 << 14, 8
    s = workloads.ssm_problem(dx=dx, T=T)
    h = BootstrapFilter(LinearGaussianSSM(s["A"], s["q"], s["r"]), K).run(core.key(3), s["y"], keep_history=True)["history"]
    back = lambda: h.backward_paths(core.key(5))
    back()
    torch.cuda.synchronize()
    tb = [timed(back, 1) for _ in range(REPS)]
    anc = torch.arange(K, dtype=torch.int32, device="cuda")
    for a in reversed(h.ancestors[1:]):
        anc = a[anc.long()]
    print(f"# backward simulation of K paths through a T = {T}, K = {K}, dx = {dx} history", file=out)
    print(f"backward_paths  {med(tb)} us   ({T - 1} pairwise_gauss_pick calls)", file=out)
    print(f"distinct particles at t = 1: backward_paths {int(h.backward_indices[1].unique().numel())}   paths() {int(anc.unique().numel())}", file=out)


if __name__ == "__main__":
    main()
