"""Times gjx_pairwise_t_lse and gjx_pairwise_t_mean (nu = 3) against gjx_pairwise_gauss_lse and gjx_pairwise_gauss_mean at the same d =
dv = 8 and the same shapes, n_q = n_k = 2^12 and 2^14: random particles, normalised random log-weights as bias, precision 1.  The four
calls alternate in one process; device events around N back-to-back calls, warmed up, REPS repetitions, medians with the range, and
the largest difference of each t result from float64 torch on the same numbers.
Usage: python profiles/microbench/pairwise_t_bench.py [out.txt]"""
import statistics
import sys

import torch

from genjax_amd import kernels

REPS, N, D, NU = 7, 50, 8, 3.0


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
    print(f"# gjx_pairwise_t_lse / _mean (nu = {NU}) against the Gaussian calls, d = dv = {D}, n_q = n_k = n; {torch.cuda.get_device_name(0)}",
          file=out)
    print("        n  call            us  (min .. max)   ratio to its Gaussian twin", file=out)
    for lg in (12, 14):
        n = 1 << lg
        q, k, v = (torch.randn((D, n), device="cuda", generator=g) for _ in range(3))
        bias = torch.log_softmax(torch.randn(n, device="cuda", generator=g), 0)
        ws = torch.empty(kernels.load().gjx_pairwise_gauss_mean_workspace_bytes(n, n, D, D), dtype=torch.uint8, device="cuda")
        res, mean = torch.empty(n, device="cuda"), torch.empty((D, n), device="cuda")
        calls = {"gauss lse": lambda: kernels.pairwise_gauss_lse(q, k, bias, 1.0, None, ws, out=res),
                 "t lse": lambda: kernels.pairwise_t_lse(q, k, bias, 1.0, NU, None, ws, out=res),
                 "gauss mean": lambda: kernels.pairwise_gauss_mean(q, k, v, bias, 1.0, None, ws, out=mean, lse_out=res),
                 "t mean": lambda: kernels.pairwise_t_mean(q, k, v, bias, 1.0, NU, None, ws, out=mean, lse_out=res)}
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in calls}
        for _ in range(REPS):                   # the calls alternate
            for name, fn in calls.items():
                times[name].append(timed(fn, N))
        for name, t in times.items():
            twin = statistics.median(times["gauss " + name.split()[1]])
            print(f"{n:9d}  {name:10s}  {statistics.median(t):8.1f}  ({min(t):.1f} .. {max(t):.1f})  {statistics.median(t) / twin:6.2f}", file=out)
        # what was timed is the t kernel: float64 torch on 1024 of the queries
        s = bias.double()[None, :] - 0.5 * (NU + D) * torch.log1p(torch.cdist(q[:, :1024].double().T, k.double().T) ** 2 / NU)
        got = kernels.pairwise_t_mean(q[:, :1024].contiguous(), k, v, bias, 1.0, NU)
        print(f"{n:9d}  largest difference from float64 torch: lse {float((got['lse'] - torch.logsumexp(s, 1)).abs().max()):.2e}, "
              f"mean {float((got['mean'] - (torch.softmax(s, 1) @ v.double().T).T).abs().max()):.2e}", file=out)
        out.flush()


if __name__ == "__main__":
    main()
