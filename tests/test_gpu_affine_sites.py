"""Affine likelihoods on the matrix cores against float64, shape branch by shape branch (tests/affine_sites_ref.py holds the cases, the
float64 restatement and the bounds; tests/test_affine_sites_cpu.py checks the cases themselves: shapes, paths, conditioning, and that
the data tells a misplaced row, coefficient, bias entry or observation from the right one).

  propagate (emit_mfma_site): the likelihood's site score, the total score and the weight of every particle against the restatement
      at the float32 choices the run returned; K = 256 and 512 (the matrix-core flavour), one case also at K = 300 (scalar flavour)
      and under both RNG layouts.
  HMC (hmc_emit_mfma_site with and without the fold; k_hmc_logreg, k_hmc_logreg_mfma, k_hmc_logreg_mfma2), on every engine a case
      runs on — fused, generated with and without the matrix-core flavour, interpreter:
      the score one move returns against the restatement at the choices it returns, and the device's GRADIENT at the start state,
      recovered from two one-step moves with the same key (affine_sites_ref.recover_gradient), against the analytic float64 gradient.
  Beside both: agreement with the CPU oracle within the tolerances of the neighbouring tests (test_gpu_codegen.py, test_gpu_hmcgen.py).
No tolerance is a flat number (module docstring of affine_sites_ref.py); no particle and no chain is excluded; the worst
|error| / bound of every comparison is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import affine_sites_ref as R                              # noqa: E402
from genjax_amd import _abi as A                          # noqa: E402

PROP, GEN, FUSED = R.prop_cases(), R.gen_cases(), R.fused_cases()
KNOBS = ("GJX_HMC_ENGINE", "GJX_HMC_GEN_NO_FOLD", "GJX_HMC_GEN_NO_MFMA", "GJX_HMC_MFMA", "GJX_HMC_NO_MFMA2", "GJX_HMC_NO_BIN", "GJX_GEN_NO_MFMA",
         "GJX_ENGINE", "GJX_GEN_PPT", "GJX_GEN_MFMA_DEBUG", "GJX_FORCE_GENERIC")
KEY, OFFSET = (4, 1), 5
SCORE_EPS, SCORE_L = 2.0 ** -6, 2            # the move whose returned score is checked


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def K_():
    from genjax_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def oracle():
    from oracle import cpu
    return cpu


def _check(what, ratios):
    print(f"{what}: worst |error| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, (what, ratios)


@pytest.mark.parametrize("which", list(PROP))
def test_propagate_sites_on_the_matrix_cores_against_float64(K_, oracle, which, monkeypatch):
    case = PROP[which]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    both = which == R.PROP_BOTH_RNG
    for rng in ((A.RNG_FLAT, A.RNG_JAX32) if both else (A.RNG_FLAT,)):
        prog = case.program(rng)
        j = [s.addr for s in prog.site_list.sites].index("y")
        assert all(t in K_.program_source(prog, 1 | 256) for t in case.text)
        for K in R.PROP_KS + ((R.PROP_SCALAR_K,) if both else ()):
            out = K_.run_program(prog, (0, 5), K, want_site_scores=True)
            assert out["_engine"] == 4
            ch = _np(out["choices"])
            ref = R.prop_reference(case, prog, ch)
            _check(f"{which} rng {rng} K {K}", dict(site=R.worst_ratio(_np(out["site_scores"])[j], ref["site"][j], ref["site_bound"][j]),
                                                    score=R.worst_ratio(_np(out["score"]), ref["score"], ref["score_bound"]),
                                                    weight=R.worst_ratio(_np(out["weight"]), ref["weight"], ref["weight_bound"])))
            ora = oracle.run_program(prog, (0, 5), K, want_site_scores=True)
            np.testing.assert_allclose(ch, ora["choices"], rtol=2e-4, atol=5e-5)
            for k in ("weight", "score", "site_scores"):
                np.testing.assert_allclose(_np(out[k]), ora[k], rtol=2e-4, atol=2e-2, err_msg=f"{which} {k}")


def _engines(K_, case, prog, monkeypatch):
    """(label, environment) of every engine the case runs on; the generated kernel without its matrix-core flavour only where that is
    another kernel"""
    def env(engine, extra=()):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("GJX_HMC_ENGINE", engine)
        for k, v in list(case.env.items()) + list(extra):
            monkeypatch.setenv(k, v)

    out = []
    if case.family == "fused":
        env("fused")
        assert K_.hmc_engine(prog) == case.engine
        out.append(("fused", lambda: env("fused")))
    env("gen")
    assert K_.hmc_engine(prog) == 4
    src = K_.program_hmc_source(prog)
    if case.family == "gen":
        assert src.count("on the matrix cores") == case.expect["n_mfma"] and all(t in src for t in case.text)
    out.append(("gen", lambda: env("gen")))
    if "on the matrix cores" in src:
        out.append(("gen without the matrix cores", lambda: env("gen", [("GJX_HMC_GEN_NO_MFMA", "1")])))
    env("interp")
    assert K_.hmc_engine(prog) == 0
    out.append(("interp", lambda: env("interp")))
    return out


def _hmc_case(K_, oracle, case, monkeypatch, chains):
    import torch
    prog = case.program()
    rows = R.selected_slots(prog, case.selected)
    q_all = R.start_state(case, prog, max(chains), 7)
    ref_all = R.hmc_reference(case, prog, q_all)               # once per case: the chain counts share the columns
    engines = _engines(K_, case, prog, monkeypatch)
    for n in chains:
        q0 = np.ascontiguousarray(q_all[:, :n])
        ora = oracle.hmc(prog, KEY, q0, SCORE_EPS, SCORE_L, False, False, offset=OFFSET)
        for label, setenv in engines:
            setenv()
            move = lambda eps, L: K_.hmc(prog, KEY, torch.as_tensor(q0).cuda(), eps, L, False, False, offset=OFFSET)     # noqa: E731
            g = move(SCORE_EPS, SCORE_L)
            ch = _np(g["choices"])
            vals = R.values_of(prog, ch)
            ratios = dict(score=R.worst_ratio(_np(g["score"]), case.ref.site_scores(vals).sum(0), case.ref.score_bounds(vals)[1]))
            q1a, q1b = _np(move(R.EPS1, 1)["choices"])[rows], _np(move(R.EPS2, 1)["choices"])[rows]
            grad, bound = ref_all["grad"][:, :n], ref_all["grad_bound"][:, :n] + R.recovery_rounding(q1a, q1b, ref_all["grad"][:, :n])
            ratios["gradient"] = R.worst_ratio(R.recover_gradient(q0[rows], q1a, q1b), grad, bound)
            _check(f"{case.name} {label} n {n}", ratios)
            # the existing practice beside it: the move agrees with the oracle's (test_gpu_hmcgen.py's tolerances)
            np.testing.assert_allclose(ch, ora["choices"], rtol=3e-3, atol=3e-3, err_msg=f"{case.name} {label}")
            np.testing.assert_allclose(_np(g["score"]), ora["score"], rtol=1e-3, atol=6e-3, err_msg=f"{case.name} {label}")
            mag = 5e-6 * np.maximum(np.abs(ora["score"]), np.abs(ora["score"] - ora["alpha"]))
            assert (np.abs(_np(g["alpha"]) - ora["alpha"]) <= 6e-3 + 6e-3 * np.abs(ora["alpha"]) + mag).all(), f"{case.name} {label} alpha"
            assert (_np(g["accepted"]) == 1).all()


@pytest.mark.parametrize("which", list(GEN))
def test_generated_hmc_sites_on_the_matrix_cores_against_float64(K_, oracle, which, monkeypatch):
    _hmc_case(K_, oracle, GEN[which], monkeypatch, R.GEN_CHAINS)


@pytest.mark.parametrize("which", list(FUSED))
def test_hand_written_logistic_kernels_against_float64(K_, oracle, which, monkeypatch):
    _hmc_case(K_, oracle, FUSED[which], monkeypatch, (17, 300))
