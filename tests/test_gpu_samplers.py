"""elem_sample (genjax_amd/csrc/gjx_device.h) against exact CDFs, on the site interpreter and on the generated kernel, in both RNG layouts:
tests/golden/sampler_grid.json.gz (tests/golden/make_sampler_grid.py) holds, per kind, 6 to 12 parameter rows — ordinary points, both
sides of every branch threshold, the float32 extremes — and per row the exact CDF at about 260 edges.  One launch per kind, 2^20 draws
per row (particle i carries row i // 2^20); per edge |empirical - exact| <= 6 sqrt(F (1 - F) / M) + 1 / M, no draw outside the support or
the 1e-6 / M guard quantiles, every draw's own site score finite (helpers.sampler_grid_check; tests/test_samplers_cpu.py asks the same
of the CPU oracle).  The draws come back to the host and are counted there in float64 (a sort per row: about a second per kind)."""
import numpy as np
import pytest

import helpers as H
from genjax_amd import _abi as A

pytestmark = pytest.mark.gpu

GRID_KINDS = sorted(k for k in H.KIND if k not in H.VECTOR_KINDS)
RNGS = {"flat": A.RNG_FLAT, "jax32": A.RNG_JAX32}
ENGINE_CODE = {"interp": 0, "gen": 4}


@pytest.fixture(scope="module")
def K_():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from genjax_amd import kernels
    return kernels


def _run(K_, prog, n, choices=None):
    import torch
    dev = None if choices is None else torch.as_tensor(choices).cuda()
    out = K_.run_program(prog, (7, 11), n, choices=dev, want_site_scores=True)
    return out["choices"].cpu().numpy(), out["site_scores"].cpu().numpy()


@pytest.mark.parametrize("rng", sorted(RNGS))
@pytest.mark.parametrize("engine", ["interp", "gen"])
@pytest.mark.parametrize("kind", GRID_KINDS)
def test_sampler_grid(K_, kind, engine, rng, monkeypatch):
    monkeypatch.setenv("GJX_ENGINE", engine)
    rec = H.sampler_grid()[kind]
    prog, ch, xs, xi = H.sampler_grid_program(kind, RNGS[rng])
    assert K_.program_engine(prog) == ENGINE_CODE[engine]
    got, ss = _run(K_, prog, ch.shape[1], ch)
    np.testing.assert_array_equal(got[:xi], ch[:xi])          # the carriers came through untouched
    worst, z, bad = H.sampler_grid_check(got[xs], rec)
    print(f"sampler_grid {kind} {engine} {rng}: excess {worst:.3g} worst z {z:.2f}")      # |deviation| / bound, before asserting
    nf = np.nonzero(~np.isfinite(ss[xi]))[0]
    assert not bad, bad
    assert nf.size == 0, (nf.size, [(int(i), float(got[xs][i]), float(ss[xi][i]), tuple(float(c[i]) for c in ch[:xi])) for i in nf[:5]])


# ---- vector and categorical kinds: constant parameters, one site each ------------------------------------------------------------------
M = H.sampler_grid()["M"]


@pytest.mark.parametrize("rng", sorted(RNGS))
@pytest.mark.parametrize("alpha", H.DIRICHLET_ALPHAS, ids=lambda a: "-".join(str(t) for t in a))
def test_dirichlet_components(K_, alpha, rng, monkeypatch):
    """each component against beta(alpha_i, alpha_0 - alpha_i), rows sum to 1 within 1e-5, no component exactly 0 or 1, scores finite
    (the site interpreter: the emitter of generated kernels does not take dirichlet sites)"""
    monkeypatch.setenv("GJX_ENGINE", "interp")
    prog = H.one_vector_site(A.DIRICHLET, [np.asarray(alpha, np.float32)], dim=len(alpha), rng=RNGS[rng])
    assert K_.program_engine(prog) == 0
    got, ss = _run(K_, prog, M)
    worst, z, bad = H.dirichlet_check(got[:len(alpha)], alpha)
    print(f"sampler_grid dirichlet{alpha} interp {rng}: excess {worst:.3g} worst z {z:.2f}")
    assert not bad, bad
    assert np.isfinite(ss[0]).all()


@pytest.mark.parametrize("rng", sorted(RNGS))
@pytest.mark.parametrize("engine", ["interp", "gen"])
def test_mv_normal_diag_components(K_, engine, rng, monkeypatch):
    monkeypatch.setenv("GJX_ENGINE", engine)
    prog = H.one_vector_site(A.MVNORMAL_DIAG, [np.asarray(H.MVN_LOC, np.float32), np.asarray(H.MVN_SCALE, np.float32)], dim=5, rng=RNGS[rng])
    assert K_.program_engine(prog) == ENGINE_CODE[engine]
    got, ss = _run(K_, prog, M)
    worst, z, bad = H.mvn_check(got[:5])
    print(f"sampler_grid mv_normal_diag[5] {engine} {rng}: excess {worst:.3g} worst z {z:.2f}")
    assert not bad, bad
    assert np.isfinite(ss[0]).all()


# (the emitter of generated kernels takes categorical sites of up to 64 categories: 257 is the site interpreter's alone)
@pytest.mark.parametrize("rng", sorted(RNGS))
@pytest.mark.parametrize("probs", [False, True], ids=["logits", "probs"])
@pytest.mark.parametrize("n,engine", [(3, "interp"), (3, "gen"), (64, "interp"), (64, "gen"), (257, "interp")])
def test_categorical_frequencies(K_, n, probs, engine, rng, monkeypatch):
    monkeypatch.setenv("GJX_ENGINE", engine)
    par, p = H.categorical_case(n, probs)
    prog = H.one_vector_site(A.CATEGORICAL_PROBS if probs else A.CATEGORICAL_LOGITS, [par], rng=RNGS[rng])
    assert K_.program_engine(prog) == ENGINE_CODE[engine]
    got, ss = _run(K_, prog, M)
    worst, bad = H.categorical_check(got[0], p)
    print(f"sampler_grid categorical[{n}] {'probs' if probs else 'logits'} {engine} {rng}: excess {worst:.3g}")
    assert not bad, bad
    assert np.isfinite(ss[0]).all()
