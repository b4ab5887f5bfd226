"""Times gjx_pairwise_gauss_mean and the FFBSm lag-one pair moments built on it.
  1. one call at d = dv = 8 for n_q = n_k = 2^12, 2^14 (random particles and values, normalised random log-weights as bias) against
     gjx_pairwise_gauss_lse on the same inputs (the two alternate inside every repetition) and against the torch line
     torch.softmax(bias - p / 2 * torch.cdist(q, k) ** 2, 1) @ v.t(); the largest difference of the two results.
  2. h.smoothed_pair_moments(method="ffbs") (the kept ffbs_weights() in place, as an EM step after smoothed_moments finds them) against
     method="lineage" (its kept weights likewise) on one T = 64, K = 2^14, dx = 8 history of the hand-written filter, and the effective
     sample size both report for the pair at t = 1.
Device events around N back-to-back calls, warmed up, REPS repetitions, medians.  Usage: python profiles/microbench/pairwise_mean_bench.py [out.txt]"""
import statistics
import sys

import torch

from genjax_amd import core, kernels, workloads
from genjax_amd.inference.pf import BootstrapFilter, LinearGaussianSSM

REPS, D, P = 5, 8, 1.3


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
    print(f"# gjx_pairwise_gauss_mean, d = dv = {D}, n_q = n_k = n; {torch.cuda.get_device_name(0)}", file=out)
    print("        n  mean_us (min .. max)   lse_us (min .. max)  mean/lse   torch_us (min .. max)  max|diff|", file=out)
    for lg in (12, 14):
        n = 1 << lg
        q, k, v = (torch.randn((D, n), device="cuda", generator=g) for _ in range(3))
        bias = torch.log_softmax(torch.randn(n, device="cuda", generator=g), 0)
        lib = kernels.load()
        ws = torch.empty(lib.gjx_pairwise_gauss_mean_workspace_bytes(n, n, D, D), dtype=torch.uint8, device="cuda")
        ws_l = torch.empty(lib.gjx_pairwise_gauss_lse_workspace_bytes(n, n, D), dtype=torch.uint8, device="cuda")
        res, lse, res_l = torch.empty((D, n), device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        mean = lambda: kernels.pairwise_gauss_mean(q, k, v, bias, P, None, ws, out=res, lse_out=lse)
        only = lambda: kernels.pairwise_gauss_lse(q, k, bias, P, None, ws_l, out=res_l)
        theirs = lambda: torch.softmax(bias - 0.5 * P * torch.cdist(q.t(), k.t()) ** 2, 1) @ v.t()
        mean(), only()
        diff = float((theirs().t() - mean()["mean"]).abs().max())
        torch.cuda.synchronize()
        tm, tl, tt = [], [], []
        for _ in range(REPS):
            tm.append(timed(mean, 50))
            tl.append(timed(only, 50))
            tt.append(timed(theirs, 10))
        print(f"{n:9d}  {med(tm)}  {med(tl)}  {statistics.median(tm) / statistics.median(tl):8.2f}  {med(tt)}  {diff:.2e}", file=out)
        out.flush()
        del q, k, v, bias, ws, ws_l, res, lse, res_l
        torch.cuda.empty_cache()

    T, K, dx = 64, 1 << 14, 8
    s = workloads.ssm_problem(dx=dx, T=T)
    h = BootstrapFilter(LinearGaussianSSM(s["A"], s["q"], s["r"]), K).run(core.key(3), s["y"], keep_history=True)["history"]
    ffbs, lineage = lambda: h.smoothed_pair_moments(method="ffbs"), lambda: h.smoothed_pair_moments()
    mf, ml = ffbs(), lineage()
    torch.cuda.synchronize()
    tf, tl = [timed(ffbs, 1) for _ in range(REPS)], [timed(lineage, 3) for _ in range(REPS)]
    print(f"# lag-one pair moments of a T = {T}, K = {K}, dx = {dx} history (smoothing weights of either kind already kept)", file=out)
    print(f"method='ffbs'     {med(tf)} us   ({T - 1} pairwise_gauss_mean calls, one weighted_cross_moments_steps)", file=out)
    print(f"method='lineage'  {med(tl)} us", file=out)
    print(f"ESS of the pair at t = 1: ffbs {float(mf['ess'][0]):.1f}   lineage {float(ml['ess'][0]):.1f}", file=out)
    print(f"largest |cross| difference of the two methods at t = T-1: {float((mf['cross'][-1] - ml['cross'][-1]).abs().max()):.3e}", file=out)


if __name__ == "__main__":
    main()
