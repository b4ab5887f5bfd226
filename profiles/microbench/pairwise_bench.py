"""Times gjx_pairwise_gauss_lse and the marginal backward smoother built on it.
  1. one call at d = 8 for n_q = n_k = 2^12, 2^14, 2^16 (random particles, normalised random log-weights as bias), against
     torch.logsumexp(bias - p / 2 * torch.cdist(q, k) ** 2, 1) wherever its n_q x n_k floats fit (2^16: 16 GiB for the distances
     alone, not run).  Pairs per second, and the share of the device's exponential rate (256 CUs x 16 v_exp_f32 lanes per clock at
     2.4 GHz) that one exponential per pair comes to.
  2. h.ffbs_weights() (caches cleared before every call) against h.smoothing_weights() (likewise) on one T = 64, K = 2^14, dx = 8
     history of the hand-written filter, and the effective sample size 1 / sum w^2 of both kinds of weights at t = 0, T/2, T-1.
Device events around N back-to-back calls, warmed up, REPS repetitions, medians.  Usage: python profiles/microbench/pairwise_bench.py [out.txt]"""
import statistics
import sys

import torch

from genjax_amd import core, kernels, workloads
from genjax_amd.inference.pf import BootstrapFilter, LinearGaussianSSM

REPS, D, P = 5, 8, 1.3
EXP_PER_S = 256 * 16 * 2.4e9


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n          # us per call


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    g = torch.Generator(device="cuda").manual_seed(1)
    print(f"# gjx_pairwise_gauss_lse, d = {D}, n_q = n_k = n; {torch.cuda.get_device_name(0)}", file=out)
    print("        n  kernel_us  (min .. max)   Gpairs/s  exp_rate_share   torch_us  (min .. max)  max|diff|", file=out)
    for lg in (12, 14, 16):
        n = 1 << lg
        q, k = torch.randn((D, n), device="cuda", generator=g), torch.randn((D, n), device="cuda", generator=g)
        bias = torch.log_softmax(torch.randn(n, device="cuda", generator=g), 0)
        ws = torch.empty(kernels.load().gjx_pairwise_gauss_lse_workspace_bytes(n, n, D), dtype=torch.uint8, device="cuda")
        res = torch.empty(n, device="cuda")
        ours = lambda: kernels.pairwise_gauss_lse(q, k, bias, P, None, ws, out=res)
        theirs = lambda: torch.logsumexp(bias - 0.5 * P * torch.cdist(q.t(), k.t()) ** 2, 1)
        reps = 20 if lg < 16 else 3
        ours()
        torch.cuda.synchronize()
        tk = [timed(ours, reps) for _ in range(REPS)]
        mk = statistics.median(tk)
        line = f"{n:9d}  {mk:9.1f}  ({min(tk):.1f} .. {max(tk):.1f})  {n * n / mk / 1e3:8.1f}  {n * n / (mk * 1e-6) / EXP_PER_S:14.2f}"
        if lg < 16:
            diff = float((theirs() - ours()).abs().max())
            tt = [timed(theirs, reps) for _ in range(REPS)]
            line += f"  {statistics.median(tt):9.1f}  ({min(tt):.1f} .. {max(tt):.1f})  {diff:.2e}"
        else:
            line += "  (torch: n x n floats do not fit)"
        print(line, file=out)
        out.flush()
        del q, k, bias, ws, res
        torch.cuda.empty_cache()

    T, K, dx = 64, 1 << 14, 8
    s = workloads.ssm_problem(dx=dx, T=T)
    h = BootstrapFilter(LinearGaussianSSM(s["A"], s["q"], s["r"]), K).run(core.key(3), s["y"], keep_history=True)["history"]

    def ffbs():
        h._ffbs_w = None
        return h.ffbs_weights()

    def lineage():
        h._lineage_out = None
        return h.smoothing_weights()

    wf, wl = ffbs(), lineage()
    torch.cuda.synchronize()
    tf, tl = [timed(ffbs, 1) for _ in range(REPS)], [timed(lineage, 3) for _ in range(REPS)]
    print(f"# smoothing weights of a T = {T}, K = {K}, dx = {dx} history (2 (T - 1) pairwise calls against T scatter launches)", file=out)
    print(f"ffbs_weights       {statistics.median(tf):10.0f} us  ({min(tf):.0f} .. {max(tf):.0f})", file=out)
    print(f"smoothing_weights  {statistics.median(tl):10.0f} us  ({min(tl):.0f} .. {max(tl):.0f})", file=out)
    ess = lambda w, t: float(1.0 / (w[t].double() ** 2).sum())
    surv = h.survivors().cpu().numpy()
    for t in (0, T // 2, T - 1):
        print(f"ESS at t = {t:2d}: ffbs {ess(wf, t):9.1f}   lineage {ess(wl, t):9.1f}   (survivors {int(surv[t])} of {K})", file=out)


if __name__ == "__main__":
    main()
