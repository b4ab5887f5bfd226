"""A plain `bench.py` run on the GPU: exactly the contract's line (no roofline, baselines or side file: those are --full's), and
--dump-outputs writes the last timed step's outputs, the same from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 1 << 16


def _plain(tmp_path, tag):
    side = tmp_path / (tag + "_side.json")
    dump = tmp_path / tag
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                          "--k-per-gpu", str(K), "--extra-file", str(side), "--dump-outputs", str(dump)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and out.stdout.strip().splitlines()[-1] == lines[0], out.stdout[-2000:]
    assert not side.exists()                      # the full record is --full's
    return json.loads(lines[0]), {n[:-4]: np.load(dump / n) for n in os.listdir(dump)}


def test_bench_plain_run_line_and_dumped_outputs(tmp_path):
    rec, a = _plain(tmp_path, "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec, k
    assert rec["metric"] == "particle_steps_per_sec" and rec["unit"] == "particle-steps/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "f32" and rec["steps"] == 5 and rec["warmup"] == 2 and rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(K * 1e3 / rec["ms_per_step"], rel=1e-9)
    for k in ("roofline", "cpu_baseline", "other_configs", "full_record", "log_ml_rel_err"):
        assert k not in rec, k
    assert sorted(a) == ["choices", "logw", "lse", "resampled", "score"]
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["choices"].shape == a["resampled"].shape == (17, K) and a["logw"].shape == a["score"].shape == (K,)
    assert np.isfinite(a["choices"]).all() and np.isfinite(a["resampled"]).all() and np.isfinite(a["lse"]).all()
    assert float(a["lse"][3]) == pytest.approx(rec["log_ml"], rel=1e-6)
    # every resampled particle is one of the step's particles
    cols = {c.tobytes() for c in np.ascontiguousarray(a["choices"].T)}
    assert all(c.tobytes() in cols for c in np.ascontiguousarray(a["resampled"].T))
    # same arguments, same inputs: the same outputs
    _, b = _plain(tmp_path, "b")
    assert sorted(b) == sorted(a)
    for k in ("choices", "score", "logw", "resampled"):
        assert np.array_equal(a[k], b[k]), k
    np.testing.assert_allclose(a["lse"], b["lse"], rtol=1e-6)
