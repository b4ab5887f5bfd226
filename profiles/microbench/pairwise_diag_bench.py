"""Times gjx_pairwise_gauss_lse_diag (both sides) against gjx_pairwise_gauss_lse at the same d = 8 and the same shapes, n_q = n_k =
2^12 and 2^14: random particles, normalised random log-weights as bias, precisions log-uniform over 10^+-1 (the isotropic call at
their geometric mean 1).  The three calls alternate in one process; device events around N back-to-back calls, warmed up, REPS
repetitions, medians with the range.  Usage: python profiles/microbench/pairwise_diag_bench.py [out.txt]"""
import statistics
import sys

import torch

from genjax_amd import kernels

REPS, N, D = 7, 50, 8


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
    print(f"# gjx_pairwise_gauss_lse_diag against gjx_pairwise_gauss_lse, d = {D}, n_q = n_k = n; {torch.cuda.get_device_name(0)}", file=out)
    print("        n  call       us  (min .. max)   ratio to the isotropic call", file=out)
    for lg in (12, 14):
        n = 1 << lg
        q, k = torch.randn((D, n), device="cuda", generator=g), torch.randn((D, n), device="cuda", generator=g)
        prec = 10.0 ** (2.0 * torch.rand((D, n), device="cuda", generator=g) - 1.0)
        bias = torch.log_softmax(torch.randn(n, device="cuda", generator=g), 0)
        ws = torch.empty(kernels.load().gjx_pairwise_gauss_lse_diag_workspace_bytes(n, n, D), dtype=torch.uint8, device="cuda")
        res = torch.empty(n, device="cuda")
        calls = {"isotropic": lambda: kernels.pairwise_gauss_lse(q, k, bias, 1.0, None, ws, out=res),
                 "keys": lambda: kernels.pairwise_gauss_lse(q, k, bias, prec, None, ws, out=res, precision_of="keys"),
                 "queries": lambda: kernels.pairwise_gauss_lse(q, k, bias, prec, None, ws, out=res, precision_of="queries")}
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in calls}
        for _ in range(REPS):                   # the calls alternate
            for name, fn in calls.items():
                times[name].append(timed(fn, N))
        iso = statistics.median(times["isotropic"])
        for name, t in times.items():
            print(f"{n:9d}  {name:9s}  {statistics.median(t):8.1f}  ({min(t):.1f} .. {max(t):.1f})  {statistics.median(t) / iso:6.2f}", file=out)
        out.flush()


if __name__ == "__main__":
    main()
