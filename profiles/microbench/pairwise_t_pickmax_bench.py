"""Times gjx_pairwise_t_pick and gjx_pairwise_t_argmax (nu = 3) at d = 8, n_q = n_k = 2^12 and 2^14: the pick against
gjx_pairwise_gauss_pick, the argmax against gjx_pairwise_gauss_argmax and against gjx_pairwise_t_lse (one logarithm and one exponential
per pair, where the product form of the argmax has neither).  Random particles, normalised random log-weights as bias, precision 1.
The five calls alternate in one process; device events around N back-to-back calls, warmed up, REPS repetitions, medians with the
range, and how many of 1024 queries' argmaxes agree with float64 torch on the same numbers.
Usage: python profiles/microbench/pairwise_t_pickmax_bench.py [out.txt]"""
import statistics
import sys

import torch

from genjax_amd import kernels

REPS, N, D, NU = 7, 50, 8, 3.0
AGAINST = {"t pick": ("gauss pick",), "t argmax": ("gauss argmax", "t lse")}


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
    print(f"# gjx_pairwise_t_pick / _argmax (nu = {NU}), d = {D}, n_q = n_k = n; {torch.cuda.get_device_name(0)}", file=out)
    print("        n  call                us  (min .. max)   ratios", file=out)
    for lg in (12, 14):
        n = 1 << lg
        q, k = (torch.randn((D, n), device="cuda", generator=g) for _ in range(2))
        bias, u = torch.log_softmax(torch.randn(n, device="cuda", generator=g), 0), torch.rand(n, device="cuda", generator=g)
        lib = kernels.load()
        ws = torch.empty(max(lib.gjx_pairwise_gauss_pick_workspace_bytes(n, n, D), lib.gjx_pairwise_t_argmax_workspace_bytes(n, n, D)),
                         dtype=torch.uint8, device="cuda")
        res, idx = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        calls = {"gauss pick": lambda: kernels.pairwise_gauss_pick(q, k, u, bias, 1.0, None, ws, out=idx, lse_out=res),
                 "t pick": lambda: kernels.pairwise_t_pick(q, k, u, bias, 1.0, NU, None, ws, out=idx, lse_out=res),
                 "gauss argmax": lambda: kernels.pairwise_gauss_argmax(q, k, bias, 1.0, None, ws, out=idx, max_out=res),
                 "t argmax": lambda: kernels.pairwise_t_argmax(q, k, bias, 1.0, NU, None, ws, out=idx, max_out=res),
                 "t lse": lambda: kernels.pairwise_t_lse(q, k, bias, 1.0, NU, None, ws, out=res)}
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in calls}
        for _ in range(REPS):                   # the calls alternate
            for name, fn in calls.items():
                times[name].append(timed(fn, N))
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            ratios = ", ".join(f"{med[name] / med[other]:.2f} x {other}" for other in AGAINST.get(name, ()))
            print(f"{n:9d}  {name:12s}  {med[name]:8.1f}  ({min(t):.1f} .. {max(t):.1f})  {ratios}", file=out)
        # what was timed is the t kernel: float64 torch on 1024 of the queries
        s = bias.double()[None, :] - 0.5 * (NU + D) * torch.log1p(torch.cdist(q[:, :1024].double().T, k.double().T) ** 2 / NU)
        got = kernels.pairwise_t_argmax(q[:, :1024].contiguous(), k, bias, 1.0, NU)
        print(f"{n:9d}  argmax equal to float64 torch's for {int((got['arg'] == s.argmax(1)).sum())} of 1024 queries, "
              f"largest difference of max {float((got['max'] - s.max(1).values).abs().max()):.2e}", file=out)
        out.flush()


if __name__ == "__main__":
    main()
