"""Times gjx_pairwise_gauss_mean_diag against gjx_pairwise_gauss_mean and gjx_pairwise_gauss_pick_diag against gjx_pairwise_gauss_pick
at d = dv = 8, n_q = n_k = 2^12 and 2^14: random particles and values, normalised random log-weights as bias, precisions of the keys
log-uniform over 10^+-1 (the isotropic calls at their geometric mean 1), uniforms in (0, 1).  The four calls alternate in one process;
device events around N back-to-back calls, warmed up, REPS repetitions, medians with the range.
Usage: python profiles/microbench/pairwise_meanpick_diag_bench.py [out.txt]"""
import statistics
import sys

import torch

from genjax_amd import kernels
from pairwise_diag_bench import timed

REPS, N, D = 7, 50, 8


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    g = torch.Generator(device="cuda").manual_seed(1)
    rand = lambda *s: torch.rand(s, device="cuda", generator=g)
    randn = lambda *s: torch.randn(s, device="cuda", generator=g)
    print(f"# diag mean and pick against the isotropic calls, d = dv = {D}, n_q = n_k = n; {torch.cuda.get_device_name(0)}", file=out)
    print("        n  call            us  (min .. max)   ratio to the isotropic call", file=out)
    for lg in (12, 14):
        n = 1 << lg
        q, k, v, u = randn(D, n), randn(D, n), randn(D, n), rand(n)
        prec, bias = 10.0 ** (2.0 * rand(D, n) - 1.0), torch.log_softmax(randn(n), 0)
        lib = kernels.load()
        ws = torch.empty(max(lib.gjx_pairwise_gauss_mean_diag_workspace_bytes(n, n, D, D), lib.gjx_pairwise_gauss_pick_diag_workspace_bytes(n, n, D)),
                         dtype=torch.uint8, device="cuda")
        mean, lse, pick = torch.empty((D, n), device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        calls = {"mean": lambda: kernels.pairwise_gauss_mean(q, k, v, bias, 1.0, None, ws, mean, lse),
                 "mean diag": lambda: kernels.pairwise_gauss_mean(q, k, v, bias, prec, None, ws, mean, lse),
                 "pick": lambda: kernels.pairwise_gauss_pick(q, k, u, bias, 1.0, None, ws, pick, lse),
                 "pick diag": lambda: kernels.pairwise_gauss_pick(q, k, u, bias, prec, None, ws, pick, lse)}
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in calls}
        for _ in range(REPS):                   # the calls alternate
            for name, fn in calls.items():
                times[name].append(timed(fn, N))
        for name, t in times.items():
            iso = statistics.median(times[name.split()[0]])
            print(f"{n:9d}  {name:9s}  {statistics.median(t):8.1f}  ({min(t):.1f} .. {max(t):.1f})  {statistics.median(t) / iso:6.2f}", file=out)
        out.flush()


if __name__ == "__main__":
    main()
