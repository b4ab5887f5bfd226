"""Times gjx_pairwise_gauss_argmax and the particle Viterbi path (ParticleHistory.map_path) built on it.
  1. one call at d = 8 for n_q = n_k = 2^12, 2^14 (random particles, normalised random log-weights as bias) against
     gjx_pairwise_gauss_lse on the same inputs (the two alternate inside every repetition), torch's
     (bias - 1/2 p cdist(q, k)^2).max(1) beside them, and the share of indices that agree with torch's (a check of the workload, not
     a test).
  2. h.map_path() on one T = 64, K = 2^14, dx = 8 history of the hand-written filter against the 63 bare calls.
Device events around N back-to-back calls, warmed up, REPS repetitions, medians.  Usage: python profiles/microbench/pairwise_argmax_bench.py [out.txt]"""
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
    print(f"# gjx_pairwise_gauss_argmax, d = {D}, n_q = n_k = n; {torch.cuda.get_device_name(0)}", file=out)
    print("        n  argmax_us (min .. max)   lse_us (min .. max)  argmax/lse  torch cdist+max_us  agree with torch", file=out)
    for lg in (12, 14):
        n = 1 << lg
        q, k = (torch.randn((D, n), device="cuda", generator=g) for _ in range(2))
        bias = torch.log_softmax(torch.randn(n, device="cuda", generator=g), 0)
        ws = torch.empty(kernels.load().gjx_pairwise_gauss_argmax_workspace_bytes(n, n, D), dtype=torch.uint8, device="cuda")
        arg, top, lse = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        ours = lambda: kernels.pairwise_gauss_argmax(q, k, bias, P, None, ws, out=arg, max_out=top)
        only = lambda: kernels.pairwise_gauss_lse(q, k, bias, P, None, ws, out=lse)
        theirs = lambda: (bias - 0.5 * P * torch.cdist(q.t(), k.t()) ** 2).max(1)
        ours(), only()
        agree = float((theirs()[1] == arg).float().mean())
        torch.cuda.synchronize()
        ta, tl, tt = [], [], []
        for _ in range(REPS):
            ta.append(timed(ours, 50))
            tl.append(timed(only, 50))
            tt.append(timed(theirs, 5))
        print(f"{n:9d}  {med(ta)}  {med(tl)}  {statistics.median(ta) / statistics.median(tl):10.2f}  {med(tt)}  {agree:.5f}", file=out)
        out.flush()
        del q, k, bias, ws, arg, top, lse
        torch.cuda.empty_cache()

    T, K, dx = 64, 1 << 14, 8
    s = workloads.ssm_problem(dx=dx, T=T)
    h = BootstrapFilter(LinearGaussianSSM(s["A"], s["q"], s["r"]), K).run(core.key(3), s["y"], keep_history=True)["history"]
    h.map_path()
    ws = torch.empty(kernels.load().gjx_pairwise_gauss_argmax_workspace_bytes(K, K, dx), dtype=torch.uint8, device="cuda")
    arg, top = torch.empty(K, dtype=torch.int32, device="cuda"), torch.empty(K, device="cuda")
    p = 1.0 / (s["q"] * s["q"])
    bare = lambda: [kernels.pairwise_gauss_argmax(h.states[t], h.states[t - 1], h.logw_steps[t - 1], p, None, ws, out=arg, max_out=top)
                    for t in range(1, T)]
    bare()
    torch.cuda.synchronize()
    tm, tb = [], []
    for _ in range(REPS):
        tm.append(timed(h.map_path, 1))
        tb.append(timed(bare, 1))
    print(f"# the most probable trajectory through a T = {T}, K = {K}, dx = {dx} history", file=out)
    print(f"map_path  {med(tm)} us   the {T - 1} bare pairwise_gauss_argmax calls  {med(tb)} us", file=out)
    print(f"log joint of the path {float(h.map_log_joint):.3f}, indices {int(h.map_indices.min())} .. {int(h.map_indices.max())}", file=out)


if __name__ == "__main__":
    main()
