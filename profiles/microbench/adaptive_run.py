"""adaptive resampling of the generic filter (ess_threshold) on the stochastic-volatility scan of the tests, K = 2^18, T = 256:
wall clock per step of every mode, or — MODE=<mode> — a few runs of ONE mode for rocprofv3 --kernel-trace --stats.
modes: tau1, tau05, tau0 (gjx_scan_filter_adaptive), two (two launches per step, resampling in front of every step), one (the one-launch form)"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import numpy as np, torch
import genjax_amd as genjax
from genjax_amd import C
from genjax_amd.inference import BootstrapFilter

fx = json.load(open(os.path.join(ROOT, "tests", "golden", "sv_pf_float64.json")))
phi, sigma, ys = fx["phi"], fx["sigma"], np.asarray(fx["y"], np.float32)
K, T = int(os.environ.get("KK", 1 << 18)), len(ys)


@genjax.gen
def step(x_prev, _):
    x = genjax.normal(phi * x_prev, sigma) @ "x"
    genjax.normal(0.0, genjax.exp(0.5 * x)) @ "y"
    return x, None


MODES = dict(tau1=1.0, tau05=0.5, tau0=0.0, two=None, one=None)


def run_mode(mode, n):
    os.environ.pop("GJX_SCAN_FILTER_TWO_LAUNCH", None)
    if mode == "two":
        os.environ["GJX_SCAN_FILTER_TWO_LAUNCH"] = "1"
    bf = BootstrapFilter(step.scan(n=T), K, ess_threshold=MODES[mode])
    o = bf.run(genjax.key(100), C["y"].set(ys), (0.0, None))
    torch.cuda.synchronize()
    ts = []
    for i in range(n):
        t0 = time.perf_counter()
        o = bf.run(genjax.key(100 + i), C["y"].set(ys), (0.0, None))
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / T * 1e6)
    share = float(o["resampled"][1:].float().mean()) if "resampled" in o else 1.0
    print(f"{mode:6s} K={K} T={T}: {np.median(ts):7.2f} us per step (median of {n}; min {min(ts):.2f}), form {o['info']['form_name']!r}, "
          f"{o['info']['launches']} launches, steps resampled {share:.3f}, log_ml {float(o['log_ml']):.4f}", flush=True)


if __name__ == "__main__":
    only = os.environ.get("MODE")
    for m in ([only] if only else list(MODES)):
        run_mode(m, 3 if only else 7)
