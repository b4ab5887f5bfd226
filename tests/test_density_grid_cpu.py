"""tests/golden/density_grid.json.gz (mpmath, 50 digits: tests/golden/make_density_grid.py) against the CPU oracle, and a self-check of
the fixture.  This is what shows the fixture is right before any GPU sees it: the oracle evaluates densities in double and casts to
float32, so it has to land within 2 float32 ulps of the truth (+ 1e-6); its gradients are float32 code and get the device's
gradient tolerance (tests/test_gpu_density_grid.py)."""
import math
import re
import os

import numpy as np
import pytest

import helpers as H

GRID_KINDS = sorted(k for k in H.KIND if k not in H.VECTOR_KINDS)
GRAD_AT, GRAD_RT = 3e-3, 3e-3


@pytest.mark.parametrize("kind", GRID_KINDS)
def test_oracle_matches_density_grid(oracle, kind):
    rec = H.density_grid()[kind]
    prog, xs, ps, xi = H.density_grid_program(kind)
    ch = H.density_grid_choices(rec, prog, xs, ps)
    tr = H.density_grid_truth(rec)
    out = oracle.run_program(prog, (0, 1), ch.shape[1], choices=ch, want_site_scores=True)
    np.testing.assert_array_equal(out["choices"], ch)
    got = out["site_scores"][xi].astype(np.float64)
    want = tr["lp"]
    fin = np.isfinite(want)
    ulp = np.spacing(np.abs(np.where(fin, want, 1.0)).astype(np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ex = np.where(fin, np.abs(got - want) / (2.0 * ulp + 1e-6), np.where(got == want, 0.0, np.inf))
    ex = np.where(np.isnan(ex), np.inf, ex)
    bad = np.nonzero(ex > 1.0)[0]
    print(f"density_grid oracle {kind}: value excess {ex.max():.3g}")
    assert bad.size == 0, H.density_grid_rows(rec, bad, got)
    _, g = oracle.score_grad(prog, ch)
    for name, slot in [("x", xs)] + [(f"p{j}", s) for j, s in enumerate(ps)]:
        t, k = tr["grads"][name]
        ex = H.density_grid_excess(g[slot], t, k, GRAD_AT, GRAD_RT)
        print(f"density_grid oracle {kind}: d/d{name} excess {ex.max():.3g}")
        bad = np.nonzero(ex > 1.0)[0]
        assert bad.size == 0, (name, H.density_grid_rows(rec, bad, g[slot]), t[bad])


def test_density_grid_fixture():
    grid = H.density_grid()
    # every kind elem_logpdf switches on (its non-default cases), minus the vector kinds that keep their own tables
    src = open(os.path.join(os.path.dirname(__file__), "..", "genjax_amd", "csrc", "gjx_device.h")).read()
    body = src[src.index("GJX_DEV float elem_logpdf("):src.index("// ---- samplers")]
    cases = {c.lower() for c in re.findall(r"case GJX_([A-Z0-9_]+):", body)}
    names = {k.replace("mv_normal", "mvnormal").replace("double_sided", "doublesided") for k in grid}
    assert names == cases, names ^ cases
    assert set(grid) == set(H.KIND) - set(H.VECTOR_KINDS)
    f32_exact = lambda a: all(float(np.float32(v)) == v for v in a)
    for kind, rec in grid.items():
        n = len(rec["x"])
        assert 40 <= n <= 150 or kind in ("flip", "bernoulli_logits", "geometric"), (kind, n)     # (binary outcomes: 2 rows per parameter)
        assert len(rec["p"]) == H.NPAR[kind] == len(rec["params"])
        assert f32_exact(rec["x"]) and all(f32_exact(c) for c in rec["p"]), kind
        cols = [rec["lp"], rec["neg_inf"], rec["dx"], rec["k_lp"], rec["k_dx"]] + rec["dp"] + rec["k_dp"] + rec["p"]
        assert all(len(c) == n for c in cols), kind
        for c in [rec["k_lp"], rec["k_dx"]] + rec["k_dp"]:
            assert all(math.isfinite(v) and v >= 0.0 for v in c), kind
        assert all((lp is None) == bool(ni) for lp, ni in zip(rec["lp"], rec["neg_inf"])), kind
        assert all(lp is None or math.isfinite(lp) for lp in rec["lp"]), kind
        if rec["discrete"]:
            assert all(v is None for v in rec["dx"]), kind
