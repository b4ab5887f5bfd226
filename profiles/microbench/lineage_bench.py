"""Times gjx_lineage_weights and the smoothed estimates built on it, on histories of real runs of the generic filter (linear-Gaussian
state space as @gen + .scan, K = 2^18).
  1. lineage: ancestors and last weights of a T = 256 run (the workload of BASELINE config 3).  One call = T launches; a call on the
     last n rows of the table runs exactly the first n + 1 launches of the full call, so time(n) over n gives the time per launch
     while every lane is alive (n small) and time(255) - time(255 - n) that of the last launches, where few lanes are alive.
     The 64-bit atomics a step issues are COUNTED on the host from the table (heads of runs of equal adjacent ancestors inside 64
     consecutive particles whose sum is not zero), not read from a counter.
  2. smoothed_moments("x") (lineage weights, log, T moments calls; caches cleared before every call) against smoothed_means("x")
     (T path gathers, a stack, a float64 softmax-multiply-sum) on one T = 64, dx = 4 history, alternating; peak extra memory of each.
Device events around N back-to-back calls, warmed up, REPS repetitions, medians.  Usage: python profiles/microbench/lineage_bench.py [out.txt]"""
import statistics
import sys

import numpy as np
import torch

import genjax_amd as genjax
from genjax_amd import C, kernels, workloads
from genjax_amd.inference import BootstrapFilter

K, REPS = 1 << 18, 5


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n          # us per call


def history(dx, T):
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


def atomics_of(anc_row, W_row):
    """64-bit atomics the launch issues: run heads (inside 64 consecutive particles) whose run carries weight"""
    a = anc_row.cpu().numpy().astype(np.int64)
    w = W_row.cpu().numpy() > 0
    lane = np.arange(a.size) % 64
    head = (lane == 0) | (a != np.roll(a, 1))
    run = np.cumsum(head) - 1
    return int((np.bincount(run, weights=w) > 0).sum())


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    # ---- 1. the library call ----
    T = 256
    h = history(8, T)
    anc, logw = h.ancestors.clone(), h.logw.clone()
    del h
    torch.cuda.empty_cache()
    ws = torch.empty(kernels.load().gjx_lineage_weights_workspace_bytes(T, K), dtype=torch.uint8, device="cuda")
    full = kernels.lineage_weights(anc, logw, ws)
    surv = full["survivors"].cpu().numpy()
    print(f"# gjx_lineage_weights, K = {K}, T = {T}; n_bad {int(full['n_bad'])}; survivors at t = T-1, T-2, T-9, T-33, T/2, 0: "
          f"{[int(surv[t]) for t in (T - 1, T - 2, T - 9, T - 33, T // 2, 0)]}", file=out)
    for t in (T - 1, T - 2, T - 9, T - 33, T // 2, 1):
        print(f"#   step {t}: {atomics_of(anc[t - 1], full['w'][t])} atomics (counted on the host) for {int(surv[t])} live lanes of {K}", file=out)
    ns = (1, 8, 32, 128, 223, 247, 255)
    for n in ns:                                               # warm up every shape
        kernels.lineage_weights(anc[T - 1 - n:], logw, ws)
    torch.cuda.synchronize()
    t_of = {n: [] for n in ns}
    for _ in range(REPS):
        for n in ns:
            t_of[n].append(timed(lambda: kernels.lineage_weights(anc[T - 1 - n:], logw, ws), 20))
    med = {n: statistics.median(v) for n, v in t_of.items()}
    print("rows_of_table  us_per_call  (min .. max)   us_per_launch", file=out)
    for n in ns:
        print(f"{n:13d}  {med[n]:11.1f}  ({min(t_of[n]):.1f} .. {max(t_of[n]):.1f})  {med[n] / (n + 1):8.2f}", file=out)
    print(f"# whole call {med[255]:.1f} us = {med[255] / T:.2f} us per step; first launches (all lanes alive): (t(32) - t(8)) / 24 = "
          f"{(med[32] - med[8]) / 24:.2f} us; last launches: (t(255) - t(223)) / 32 = {(med[255] - med[223]) / 32:.2f} us, "
          f"(t(255) - t(247)) / 8 = {(med[255] - med[247]) / 8:.2f} us", file=out)
    out.flush()
    del anc, logw, full, ws
    torch.cuda.empty_cache()

    # ---- 2. smoothed_moments against smoothed_means ----
    T, dx = 64, 4
    h = history(dx, T)

    def new():
        h._lineage_out = h._lineage_logw = None               # the whole path: lineage weights, log, T moments calls
        return h.smoothed_moments("x")

    def old():
        return h.smoothed_means("x")

    a, b = new()["mean"], old()
    torch.cuda.synchronize()
    print(f"# smoothed_moments vs smoothed_means, K = {K}, T = {T}, dx = {dx}: max |mean - smoothed_means| = {float((a - b).abs().max()):.3g} "
          f"(max |mean| {float(b.abs().max()):.3g})", file=out)
    peak = {}
    for name, fn in (("new", new), ("old", old)):
        h._lineage_out = h._lineage_logw = None               # (the kept weights of the call before are not "extra" of this one)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
    tn, to = [], []
    for _ in range(REPS):
        tn.append(timed(new, 3))
        to.append(timed(old, 3))
    print(f"smoothed_moments  {statistics.median(tn):9.0f} us  ({min(tn):.0f} .. {max(tn):.0f})  peak extra memory {peak['new'] / 2**20:.1f} MiB "
          f"(T K 4 = {T * K * 4 / 2**20:.0f} MiB for w, as much for its log)", file=out)
    print(f"smoothed_means    {statistics.median(to):9.0f} us  ({min(to):.0f} .. {max(to):.0f})  peak extra memory {peak['old'] / 2**20:.1f} MiB "
          f"(T dx K (4 + 8) = {T * dx * K * 12 / 2**20:.0f} MiB)", file=out)
    print(f"# ratio smoothed_means / smoothed_moments {statistics.median(to) / statistics.median(tn):.2f}", file=out)
    tq = [timed(lambda: h.smoothed_quantiles("x"), 3) for _ in range(REPS)]
    print(f"smoothed_quantiles (3 levels, weights cached) {statistics.median(tq):9.0f} us", file=out)


if __name__ == "__main__":
    main()
