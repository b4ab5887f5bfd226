"""elem_logpdf and dlogpdf (genjax_amd/csrc/gjx_device.h) against tests/golden/density_grid.json.gz — mpmath at 50 digits, held to the
CPU oracle by tests/test_density_grid_cpu.py — on the site interpreter and on the generated kernel: the big-shape deviance forms on
both sides of their thresholds, the far tails, the support edges.  One launch per kind, one grid row per particle (K is whatever
the grid has: the ragged last wave is part of the test)."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

GRID_KINDS = sorted(k for k in H.KIND if k not in H.VECTOR_KINDS)
VAL_AT, VAL_RT = 1e-4, 1e-4          # test_logpdf_table_gpu's tolerance
GRAD_AT, GRAD_RT = 3e-3, 3e-3        # test_zoo3_gradient_parity's tolerance


@pytest.fixture(scope="module")
def K_():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from genjax_amd import kernels
    return kernels


@pytest.mark.parametrize("engine", ["interp", "gen"])
@pytest.mark.parametrize("kind", GRID_KINDS)
def test_density_grid(K_, kind, engine, monkeypatch):
    """values: |site score - truth| <= 1e-4 + 1e-4 |truth| + 2 kappa, -inf exactly where the truth is, no NaN, carriers untouched.
    gradients (gjx_score_grad, every site selected but a discrete x): d/dx and d/d(parameter) within 3e-3 + 3e-3 |truth| + 2 kappa
    wherever the truth is finite.  The parameter gradients of the discrete kinds (poisson, geometric, negative_binomial, flip,
    bernoulli_logits) arrive in their carriers' rows and are checked like the others."""
    import torch
    monkeypatch.setenv("GJX_ENGINE", engine)
    rec = H.density_grid()[kind]
    prog, xs, ps, xi = H.density_grid_program(kind)
    assert K_.program_engine(prog) == (4 if engine == "gen" else 0)
    ch = H.density_grid_choices(rec, prog, xs, ps)
    tr = H.density_grid_truth(rec)
    n = ch.shape[1]
    dev = torch.as_tensor(ch).cuda()
    out = K_.run_program(prog, (0, 1), n, choices=dev.clone(), want_site_scores=True)
    got = out["site_scores"][xi].cpu().numpy()
    np.testing.assert_array_equal(out["choices"].cpu().numpy(), ch)
    ex = H.density_grid_excess(got, tr["lp"], tr["k_lp"], VAL_AT, VAL_RT)
    bad = np.nonzero(ex > 1.0)[0]
    fails = [("value", H.density_grid_rows(rec, bad, got), tr["lp"][bad])] if bad.size else []
    _, g = K_.score_grad(prog, dev)
    g = g.cpu().numpy()
    worst = 0.0
    for name, slot in [("x", xs)] + [(f"p{j}", s) for j, s in enumerate(ps)]:
        t, k = tr["grads"][name]
        exg = H.density_grid_excess(g[slot], t, k, GRAD_AT, GRAD_RT)
        worst = max(worst, float(exg.max()))
        bad = np.nonzero(exg > 1.0)[0]
        if bad.size:
            fails.append((name, H.density_grid_rows(rec, bad, g[slot]), t[bad]))
    print(f"density_grid {kind} {engine}: value excess {ex.max():.3g} gradient excess {worst:.3g}")      # |error| / tolerance, before asserting
    assert not fails, fails
