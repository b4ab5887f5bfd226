"""The samplers of the CPU oracle (oracle/gjx_oracle.c, the restatement of elem_sample in genjax_amd/csrc/gjx_device.h) against exact
CDFs: tests/golden/sampler_grid.json.gz (tests/golden/make_sampler_grid.py) holds, per kind, 6 to 12 parameter rows — ordinary points,
both sides of every branch threshold, the float32 extremes — and per row the exact CDF at about 260 edges.  2^20 draws per row, one
program run per kind and RNG layout; per edge |empirical - exact| <= 6 sqrt(F (1 - F) / M) + 1 / M (helpers.sampler_grid_check), no draw
outside the support or the 1e-6 / M guard quantiles, and every draw's own site score finite.  tests/test_gpu_samplers.py asks the same
of the device."""
import numpy as np
import pytest

import helpers as H
from genjax_amd import _abi as A
from oracle import cpu as O

GRID_KINDS = sorted(k for k in H.KIND if k not in H.VECTOR_KINDS)
RNGS = {"flat": A.RNG_FLAT, "jax32": A.RNG_JAX32}


@pytest.mark.parametrize("rng", sorted(RNGS))
@pytest.mark.parametrize("kind", GRID_KINDS)
def test_sampler_grid(kind, rng):
    rec = H.sampler_grid()[kind]
    prog, ch, xs, xi = H.sampler_grid_program(kind, RNGS[rng])
    out = O.run_program(prog, (7, 11), ch.shape[1], choices=ch, want_site_scores=True)
    worst, z, bad = H.sampler_grid_check(out["choices"][xs], rec)
    print(f"sampler_grid {kind} oracle {rng}: excess {worst:.3g} worst z {z:.2f}")      # |deviation| / bound, before asserting
    ss = out["site_scores"][xi]
    nf = np.nonzero(~np.isfinite(ss))[0]
    assert not bad, bad
    assert nf.size == 0, (nf.size, [(int(i), float(out["choices"][xs][i]), float(ss[i]), tuple(float(c[i]) for c in ch[:xi])) for i in nf[:5]])


# ---- vector and categorical kinds: constant parameters, one site each ------------------------------------------------------------------
M = H.sampler_grid()["M"]


@pytest.mark.parametrize("rng", sorted(RNGS))
@pytest.mark.parametrize("alpha", H.DIRICHLET_ALPHAS, ids=lambda a: "-".join(str(t) for t in a))
def test_dirichlet_components(alpha, rng):
    """each component against beta(alpha_i, alpha_0 - alpha_i), rows sum to 1 within 1e-5, no component exactly 0 or 1, scores finite"""
    prog = H.one_vector_site(A.DIRICHLET, [np.asarray(alpha, np.float32)], dim=len(alpha), rng=RNGS[rng])
    out = O.run_program(prog, (7, 11), M, want_site_scores=True)
    worst, z, bad = H.dirichlet_check(out["choices"][:len(alpha)], alpha)
    print(f"sampler_grid dirichlet{alpha} oracle {rng}: excess {worst:.3g} worst z {z:.2f}")
    assert not bad, bad
    assert np.isfinite(out["site_scores"][0]).all()


@pytest.mark.parametrize("rng", sorted(RNGS))
def test_mv_normal_diag_components(rng):
    prog = H.one_vector_site(A.MVNORMAL_DIAG, [np.asarray(H.MVN_LOC, np.float32), np.asarray(H.MVN_SCALE, np.float32)], dim=5, rng=RNGS[rng])
    out = O.run_program(prog, (7, 11), M, want_site_scores=True)
    worst, z, bad = H.mvn_check(out["choices"][:5])
    print(f"sampler_grid mv_normal_diag[5] oracle {rng}: excess {worst:.3g} worst z {z:.2f}")
    assert not bad, bad
    assert np.isfinite(out["site_scores"][0]).all()


@pytest.mark.parametrize("rng", sorted(RNGS))
@pytest.mark.parametrize("probs", [False, True], ids=["logits", "probs"])
@pytest.mark.parametrize("n", [3, 64, 257])
def test_categorical_frequencies(n, probs, rng):
    par, p = H.categorical_case(n, probs)
    prog = H.one_vector_site(A.CATEGORICAL_PROBS if probs else A.CATEGORICAL_LOGITS, [par], rng=RNGS[rng])
    out = O.run_program(prog, (7, 11), M, want_site_scores=True)
    worst, bad = H.categorical_check(out["choices"][0], p)
    print(f"sampler_grid categorical[{n}] {'probs' if probs else 'logits'} oracle {rng}: excess {worst:.3g}")
    assert not bad, bad
    assert np.isfinite(out["site_scores"][0]).all()
