"""The expression node ops on the device, op by op against float64 at their edges: ties, kinks, poles, overflow and guarded
branches (tests/expr_ops_ref.py holds the programs, the grids and the float64 restatement; tests/test_expr_ops_cpu.py runs the same
grids on the CPU oracle and the host evaluator and checks that the restatement is well conditioned at EVERY grid point).

Eight programs — unary ops; binary ops, compare and select; integer powers; guards; linear layers with gaps; the special functions
erf, erfc, lgamma, expm1; log-sum-exp; the reductions — each on the generated
kernels (asserted: engine 4) and on the site interpreter.  K = 4099 columns for scores, 384 for gradients and HMC.  Tolerances are the
harness's (helpers.py): scores rtol 2e-4 / atol 2e-4; gradients rtol 2e-3 / atol 2e-3 against central differences of the restatement
with the decisions frozen at the base point (the analytic gradient at ties, kinks and guard boundaries under include/gjx.h's rules);
one HMC move (eps 2e-3, L 8) rtol 3e-3 / atol 3e-3 between the engines.  Where the reference is +-inf or NaN the device returns the
same infinity or NaN.  No grid point is excluded."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import helpers as H                       # noqa: E402
import expr_ops_ref as R                  # noqa: E402
import genjax_amd as genjax               # noqa: E402
from genjax_amd import C                  # noqa: E402
from genjax_amd import _abi as A          # noqa: E402
from expr_ops_ref import (REFRESH_CS, REFRESH_YS, fd_gradient, packed, same_nonfinite, selected_rows,      # noqa: E402
                               special_plate, special_scan, structural_plate, structural_scan, switching_filter)

K, N_GRAD, RT, AT = H.GRID_K, H.GRID_N_GRAD, H.GRID_RT, H.GRID_AT


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def K_():
    from genjax_amd import kernels
    return kernels


def _worst(got, want, rt, at):
    with np.errstate(invalid="ignore"):
        r = np.abs(got - want) / (at + rt * np.abs(want))
    r = r[np.isfinite(want)]
    return float(r.max()) if r.size else 0.0


@pytest.mark.parametrize("which", list(R.SPECS))
def test_scores_on_the_generated_kernel_and_the_interpreter(K_, which, monkeypatch):
    import torch
    spec = R.SPECS[which]
    prog = packed(spec, which)
    assert spec["ops"] <= R.block_ops(prog)
    vals = spec["grid"](K)
    want = H.float32_range(H.well_conditioned(spec, vals, edges=True))             # [n_sites][K], every point kept
    assert want.shape == (prog.n_sites, K)
    tot = H.float32_range(want.sum(0))
    ch = torch.as_tensor(H.grid_rows(prog, spec, vals)).cuda()
    for eng in (None, "interp"):
        if eng is None:
            monkeypatch.delenv("GJX_ENGINE", raising=False)
            assert K_.program_engine(prog) == 4, "the emitter must take the program"
        else:
            monkeypatch.setenv("GJX_ENGINE", eng)
            assert K_.program_engine(prog) == 0
        g = K_.run_program(prog, (3, 7), K, choices=ch.clone(), want_site_scores=True)
        ss, sc = _np(g["site_scores"]).astype(np.float64), _np(g["score"]).astype(np.float64)
        for (addr, _), got, ref in zip(spec["sites"], ss, want):
            print(f"{which} {eng or 'gen'} {addr}: max |score error| / (atol + rtol |ref|) = {_worst(got, ref, RT, AT):.2e}")
        for (addr, _), got, ref in zip(spec["sites"], ss, want):
            fin = same_nonfinite(got, ref, f"{which} {eng} {addr}")
            np.testing.assert_allclose(got[fin], ref[fin], rtol=RT, atol=AT, err_msg=f"{which} {eng} {addr}")
        fin = same_nonfinite(sc, tot, f"{which} {eng} total")
        np.testing.assert_allclose(sc[fin], tot[fin], rtol=RT, atol=AT, err_msg=f"{which} {eng}")


@pytest.mark.parametrize("which", list(R.SPECS))
def test_gradients_and_one_hmc_move(K_, which, monkeypatch):
    """gjx_score_grad against the float64 gradient (finite everywhere: a guarded pole contributes nothing); then one HMC move on the
    generated HMC kernel and on the interpreter: the same, finite trajectory"""
    import torch
    spec = R.SPECS[which]
    prog = packed(spec, which, grad=True)
    ch = H.grid_rows(prog, spec, spec["grad_grid"](N_GRAD))
    rows = selected_rows(spec, prog, which)
    fd, total = fd_gradient(spec, prog, ch, rows)
    sg, gg = K_.score_grad(prog, torch.as_tensor(ch).cuda())
    sg, gg = _np(sg).astype(np.float64), _np(gg).astype(np.float64)
    fin = same_nonfinite(sg, H.float32_range(total), f"{which} score")
    assert fin.sum() >= N_GRAD // 8
    np.testing.assert_allclose(sg[fin], total[fin], rtol=RT, atol=AT, err_msg=which)
    by_site = {}
    for a, _, d in spec["latents"]:
        rs_ = [prog.slot_of[a] + e for e in range(d) if prog.slot_of[a] + e in fd]
        if rs_:
            by_site[a] = max(_worst(gg[r], fd[r], 2e-3, 2e-3) for r in rs_)
            print(f"{which} {a}: max |gradient error| / (atol + rtol |ref|) = {by_site[a]:.2e}, max |ref| = {max(np.abs(fd[r]).max() for r in rs_):.3g}")
    for r in rows:
        assert np.isfinite(gg[r]).all(), (which, r)
        np.testing.assert_allclose(gg[r], fd[r], rtol=2e-3, atol=2e-3, err_msg=f"{which} row {r}")
    if which in R.EXACT_ZERO:             # tanh / sigmoid / erf far out: exactly 0 where float64 rounds to 0; a closed guard over a pole
        for r, cols in R.EXACT_ZERO[which](prog, ch):
            assert (np.abs(gg[r][cols]) <= 1e-37).all(), (r, gg[r][cols])
    moved = {}
    for eng in ("gen", "interp"):
        monkeypatch.setenv("GJX_HMC_ENGINE", eng)
        assert K_.hmc_engine(prog) == (4 if eng == "gen" else 0), eng
        g = K_.hmc(prog, (2, 9), torch.as_tensor(ch).cuda(), 2e-3, 8, False, False, offset=5)
        moved[eng] = _np(g["choices"])[rows]
        assert np.isfinite(moved[eng]).all(), eng
        assert np.abs(moved[eng] - ch[rows]).max() > 1e-3
    print(f"{which}: max |gen - interp| / (atol + rtol |interp|) after one move = {_worst(moved['gen'], moved['interp'], 3e-3, 3e-3):.2e}")
    np.testing.assert_allclose(moved["gen"], moved["interp"], rtol=3e-3, atol=3e-3)


def _plate_on_both_engines(K_, monkeypatch, prog, rows, scores, what):
    import torch
    want = H.float32_range(scores(rows.astype(np.float64)))
    for eng in (None, "interp"):
        if eng is None:
            monkeypatch.delenv("GJX_ENGINE", raising=False)
            assert K_.program_engine(prog) == 4
        else:
            monkeypatch.setenv("GJX_ENGINE", eng)
            assert K_.program_engine(prog) == 0
        g = K_.run_program(prog, (4, 5), K, choices=torch.as_tensor(rows).cuda(), want_site_scores=True)
        ss = _np(g["site_scores"]).astype(np.float64)
        print(f"{what} {eng or 'gen'}: max |site score error| / (atol + rtol |ref|) = {_worst(ss, want, RT, AT):.2e}")
        fin = same_nonfinite(ss, want, f"{what} {eng}")
        np.testing.assert_allclose(ss[fin], want[fin], rtol=RT, atol=AT, err_msg=str(eng))


def test_a_plate_with_a_guard_a_power_and_a_gapped_linear_form(K_, monkeypatch):
    """16 instances of a vmapped kernel, ONE plate site: the leaf readers and the table strides that only plates use; the unnamed row
    between the linear form's rows holds inf and NaN"""
    prog, rows, scores = structural_plate(K)
    assert prog.c_sites[prog.n_sites - 1].plate_n == 16 and prog.c_sites[prog.n_sites - 1].p[0].op == A.P_EXPR
    _plate_on_both_engines(K_, monkeypatch, prog, rows, scores, "plate")


def test_a_plate_whose_mean_is_lgamma_and_whose_scale_is_erfc(K_, monkeypatch):
    """16 instances, ONE plate site y ~ normal(lgamma(x0 a + b), erfc(x1 c + d)) with per-instance covariates and per-column observations:
    lgamma towards the pole at 0, between the negative poles and up to 14.5, erfc from 2 down to 0.14 (expr_ops_ref.special_plate)"""
    prog, rows, scores = special_plate(K)
    body = prog.c_sites[prog.n_sites - 1]
    assert prog.n_sites == 5 and body.plate_n == 16 and body.p[0].op == A.P_EXPR and body.p[1].op == A.P_EXPR
    assert {A.E_LGAMMA, A.E_ERFC} <= R.block_ops(prog)
    _plate_on_both_engines(K_, monkeypatch, prog, rows, scores, "special plate")


def test_a_rolled_scan_with_a_guard_a_power_and_a_gapped_linear_form(K_, monkeypatch):
    """64 steps of the same body: generated == interpreter, and the scores of the device's own draws == the float64 restatement"""
    _scan_on_both_engines(K_, monkeypatch, *structural_scan(), "scan")


def test_a_rolled_scan_with_a_log_sum_exp_an_expm1_scale_and_a_guarded_lgamma(K_, monkeypatch):
    """64 steps whose body holds a 3-operand log-sum-exp, an expm1 scale and a where-guarded lgamma (expr_ops_ref.special_scan)"""
    prog, restate = special_scan()
    assert prog.n_sites == 3 * R.T_SCAN and {A.E_LSEN, A.E_EXPM1, A.E_LGAMMA, A.E_WHERE} <= R.block_ops(prog)
    _scan_on_both_engines(K_, monkeypatch, prog, restate, "special scan")


def _scan_on_both_engines(K_, monkeypatch, prog, restate, what):
    monkeypatch.delenv("GJX_ENGINE", raising=False)
    assert K_.program_engine(prog) == 4
    out = {}
    for eng in ("gen", "interp"):
        monkeypatch.setenv("GJX_ENGINE", eng)
        assert K_.program_engine(prog) == (4 if eng == "gen" else 0)
        g = K_.run_program(prog, (8, 9), K)
        out[eng] = {k: _np(g[k]).astype(np.float64) for k in ("choices", "score", "logw")}
    for k in ("choices", "score", "logw"):
        np.testing.assert_allclose(out["gen"][k], out["interp"][k], rtol=RT, atol=AT, err_msg=k)
    for eng in ("gen", "interp"):
        lik, prior = restate(prog, out[eng]["choices"])
        print(f"{what} {eng}: max |score error| / (atol + rtol |ref|) = {_worst(out[eng]['score'], lik + prior, RT, AT):.2e}")
        np.testing.assert_allclose(out[eng]["logw"], lik, rtol=RT, atol=AT, err_msg=eng)
        np.testing.assert_allclose(out[eng]["score"], lik + prior, rtol=RT, atol=AT, err_msg=eng)


def test_new_data_that_changes_the_nodes_rebuilds_the_filter_programs(K_):
    """one ScanBootstrapFilter, run on cs = [1, 1, 1, 1] and then on [1, -1, 1, -1] (steps 1 and 3 turn exp(x^2) into tanh(x^2)): the second
    run equals, bit for bit, a FRESH filter's run on the second arguments — no kernel generated for the first survives"""
    con = C["y"].set(REFRESH_YS)
    key = genjax.key(11)
    flt = switching_filter()
    first = flt.run(key, con, (np.float32(0.1), REFRESH_CS[0]))
    first = {k: _np(first[k]).copy() for k in ("logw", "choices")} | {"log_ml": float(first["log_ml"])}
    second = flt.run(key, con, (np.float32(0.1), REFRESH_CS[1]))
    fresh = switching_filter().run(key, con, (np.float32(0.1), REFRESH_CS[1]))
    last = second["programs"][-1]                  # (the rows of its INPUT sites are workspace: "its INPUT rows unused")
    own = sorted(cs.slot + e for cs in (last.c_sites[j] for j in range(last.n_sites)) if cs.mode != A.MODE_INPUT and cs.slot >= 0 for e in range(cs.dim))
    assert own
    for k in ("logw", "choices"):
        pick = (lambda x: x[own]) if k == "choices" else (lambda x: x)
        assert np.array_equal(pick(_np(second[k])), pick(_np(fresh[k]))), k
        assert not np.array_equal(pick(_np(second[k])), pick(first[k])), k
    assert float(second["log_ml"]) == float(fresh["log_ml"]) and float(second["log_ml"]) != first["log_ml"]
