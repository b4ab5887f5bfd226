"""Times gjx_weighted_quantiles (3 levels) and gjx_weighted_histogram (64 bins) on 1 and 17 rows of 2^20 particles, for a continuous row
and for a 0/1 flip row (the worst case for the LDS atomics), against the torch lines a user writes without them (per row: sort,
softmax, cumsum, searchsorted; bincount with weights).  Device events around N back-to-back calls, warmed up, the library and torch
alternating, REPS repetitions, medians; once on one buffer and once rotating over COPIES copies of the rows (more bytes than the
last-level cache holds).  Usage: python profiles/microbench/quantiles_bench.py [out.txt]"""
import statistics
import sys

import numpy as np
import torch

from genjax_amd import kernels

K, LEVELS, BINS, SPAN = 1 << 20, (0.05, 0.5, 0.95), 64, (-4.0, 4.0)
N, N_TORCH, REPS, COPIES, PASSES = 100, 5, 5, 4, 4
PEAK = 8.0e12     # B/s


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n          # us per call


def torch_quantiles(rows, logw, q):
    w = torch.softmax(logw, 0)
    out = []
    for r in range(rows.shape[0]):
        xs, idx = torch.sort(rows[r])
        cw = torch.cumsum(w[idx].double(), 0)
        out.append(xs[torch.searchsorted(cw, q * cw[-1]).clamp(max=K - 1)])
    return torch.stack(out)


def torch_histogram(rows, logw):
    w = torch.softmax(logw, 0).double()
    out = []
    for r in range(rows.shape[0]):
        b = torch.floor((rows[r] - SPAN[0]) * (BINS / (SPAN[1] - SPAN[0]))).clamp(-1, BINS).long() + 1
        out.append(torch.bincount(b, weights=w, minlength=BINS + 2))
    return torch.stack(out)


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    g = torch.Generator(device="cuda").manual_seed(1)
    logw = 2.0 * torch.randn(K, device="cuda", generator=g) - 37.0
    q64 = torch.tensor(LEVELS, dtype=torch.float64, device="cuda")
    print(f"# K = {K}, levels {LEVELS}, {BINS} bins; us per call, median of {REPS} x {N} calls ({N_TORCH} for torch); "
          f"bytes = passes x (4 + 4 n_rows) K; roofline {PEAK / 1e12:.0f} TB/s", file=out)
    print("call        rows kind        us(1 buf)  us(rotating)  TB/s   of_peak  torch_us  ratio", file=out)
    for n_rows in (1, 17):
        for kind in ("continuous", "flip"):
            def make():
                x = torch.randn((n_rows, K), device="cuda", generator=g)
                return (x < 0.3).float() if kind == "flip" else x
            bufs = [make() for _ in range(COPIES)]
            for name, passes, lib, ref in (
                    ("quantiles", PASSES, lambda x, ws: kernels.weighted_quantiles(x, logw, LEVELS, 1, ws), lambda x: torch_quantiles(x, logw, q64)),
                    ("histogram", 1, lambda x, ws: kernels.weighted_histogram(x, logw, BINS, SPAN, 1, ws), lambda x: torch_histogram(x, logw))):
                need = 1 << 20
                ws = torch.empty(need, dtype=torch.uint8, device="cuda")
                for x in bufs:                                   # warm up every shape of the timed window
                    lib(x, ws)
                ref(bufs[0])
                torch.cuda.synchronize()
                one, rot, tor = [], [], []
                for _ in range(REPS):
                    one.append(timed(lambda i: lib(bufs[0], ws), N))
                    tor.append(timed(lambda i: ref(bufs[i % COPIES]), N_TORCH))
                    rot.append(timed(lambda i: lib(bufs[i % COPIES], ws), N))
                t1, tr, tt = statistics.median(one), statistics.median(rot), statistics.median(tor)
                nbytes = passes * (4 + 4 * n_rows) * K
                rate = nbytes / (tr * 1e-6)
                print(f"{name:11s} {n_rows:4d} {kind:11s} {t1:9.1f}  {tr:12.1f}  {rate / 1e12:5.2f}  {rate / PEAK:7.1%}  {tt:8.0f}  {tt / tr:5.0f}x"
                      f"   (spread {min(rot):.1f} .. {max(rot):.1f})", file=out)
                out.flush()
    # the results agree with the torch lines where both are defined (continuous row, the median)
    x = bufs[0][:1] if kind == "continuous" else torch.randn((1, K), device="cuda", generator=g)
    a, b = kernels.weighted_quantiles(x, logw, LEVELS)["q"][0], torch_quantiles(x, logw, q64)[0]
    print(f"# library {a.tolist()}  torch {b.tolist()}", file=out)


if __name__ == "__main__":
    main()
