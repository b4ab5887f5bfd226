"""The CPU twin of tests/test_gpu_affine_sites.py (tests/affine_sites_ref.py holds the cases, the float64 restatement and the
bounds): every case has the shape and alignment it is named for and takes the path it claims (asserted on the emitted HIP source and
on the engine the launcher picks — nothing here needs a device); the float32 oracle (oracle.cpu.run_program, score_grad, hmc) meets
the bounds against the restatement; the bounds are never looser than the tolerances of the neighbouring tests; the one measured
constant C_ELEM is re-measured; and the data can tell: every misplacement an indexing bug would make moves the float64 result by
more than ten bounds on at least half the columns."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import affine_sites_ref as R                              # noqa: E402
from genjax_amd import _abi as A                          # noqa: E402
from genjax_amd.program import PackedProgram, Param, SiteList     # noqa: E402

PROP, GEN, FUSED = R.prop_cases(), R.gen_cases(), R.fused_cases()
HMC = {**GEN, **FUSED}
N_CHAINS = R.GEN_CHAINS[-1]


@pytest.fixture(scope="module")
def K_():
    from genjax_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def oracle():
    from oracle import cpu
    return cpu


def _setenv(monkeypatch, case, engine):
    for k in ("GJX_HMC_ENGINE", "GJX_HMC_GEN_NO_FOLD", "GJX_HMC_GEN_NO_MFMA", "GJX_HMC_MFMA", "GJX_HMC_NO_MFMA2", "GJX_HMC_NO_BIN", "GJX_GEN_NO_MFMA"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GJX_HMC_ENGINE", engine)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


# ---- shapes and paths -------------------------------------------------------------------------------------------------------------
def test_the_case_table_covers_what_it_is_meant_to():
    tb = lambda cs: {c.expect["tb"] for c in cs.values()}                                   # noqa: E731
    n_of = lambda cs: {c.expect["sites"][0][2] for c in cs.values()}                        # noqa: E731
    assert tb(PROP) == {1, 2, 4} and tb(GEN) == {1, 2, 4} and n_of(PROP) == n_of(GEN) == {16, 32, 48, 64}
    assert {c.expect["sites"][0][1] for c in PROP.values()} == {64, 80, 96, 65, 79, 200}
    assert {c.expect["sites"][0][1] for c in GEN.values()} == {48, 64, 96}
    assert {c.expect.get("ragged") for c in PROP.values()} >= {1, 15}
    assert any(c.expect["tb"] == 1 and "ragged" not in c.expect for c in PROP.values())       # TB = 1 on an aligned dim
    assert {c.expect["sites"][0][3] for c in PROP.values()} == {"scalar", "aligned", "misaligned"}     # (misaligned: the relocated case)
    assert {c.expect["sites"][0][4] for c in PROP.values()} == {"aligned", "misaligned"}
    assert {c.expect["sites"][0][3] for c in GEN.values()} == {"scalar", "aligned", "misaligned"}
    assert {c.expect["sites"][0][4] for c in GEN.values()} == {"aligned", "misaligned"}
    assert {c.expect["folded"] for c in GEN.values()} == {True, False}
    assert {(P, N) for P, N in ((c.expect["sites"][0][2], c.expect["sites"][0][1]) for c in FUSED.values())} >= (
        {(16, N) for N in (1, 15, 16, 17, 33, 64, 1000, 1024)} | {(P, None) for P in ()})
    assert {c.expect["sites"][0][2] for c in FUSED.values()} == {2, 4, 8, 16, 32}
    for P in (2, 4, 8, 32):
        assert len({c.expect["sites"][0][1] for c in FUSED.values() if c.expect["sites"][0][2] == P}) >= 2


@pytest.mark.parametrize("which", list(PROP))
def test_propagate_cases_have_their_shape_and_go_to_the_matrix_cores(K_, which, monkeypatch):
    case = PROP[which]
    monkeypatch.delenv("GJX_GEN_NO_MFMA", raising=False)
    monkeypatch.delenv("GJX_GEN_MFMA_DEBUG", raising=False)
    case.check_shape()
    prog = case.program()
    (_, dim, n, bias, obs_al), = case.expect["sites"]
    src = K_.program_source(prog, 1 | 256)
    assert all(t in src for t in case.text) and "__builtin_amdgcn_mfma_f32_16x16x4f32" in src, which
    assert f"n0_ += {16 * case.expect['tb']})" in src                                        # row tiles per trip
    assert f"s4_ < {n // 16};" in src                                                        # M / 4 b128 reads of a row of X
    y = prog.c_sites[[s.addr for s in prog.site_list.sites].index("y")]
    b128 = f"bias_[0] = *(const v4f_*)&TAB({y.p[0].off} + n0_ + 4 * q_)"
    clamped = f"bias_[0][r_] = TAB({y.p[0].off} + (row_ < {dim} ? row_ : {dim - 1}))"
    y128 = f"y_[0] = *(const v4f_*)&TAB({y.obs_off} + n0_ + 4 * q_)"
    yclamped = f"y_[0][r_] = TAB({y.obs_off} + (row_ < {dim} ? row_ : {dim - 1}))"
    whole = dim % 16 == 0 and obs_al == "aligned"
    assert (y128 in src) == whole and (yclamped in src) == (not whole), which
    if bias == "scalar":
        assert b128 not in src and clamped not in src and f"const float b0_ = TAB({y.p[0].off})" in src
    else:
        whole = dim % 16 == 0 and bias == "aligned"
        assert (b128 in src) == whole and (clamped in src) == (not whole), which
    assert (f"part_[g_] += row_ < {dim} ? e_ : 0.0f;" in src) == (dim % 16 != 0)
    for k in range(1, 4):                                                                    # constants of length dim: read by row
        q = y.p[k]
        if k < len(prog.site_list["y"].params) and q.len == dim:
            assert f"TAB({q.off} + row_ % {dim})" in src, (which, k)
    assert "on the matrix cores" not in K_.program_source(prog, 1)                           # what a K that is no multiple of 256 runs


@pytest.mark.parametrize("which", list(GEN))
def test_generated_hmc_cases_have_their_shape_and_go_to_the_matrix_cores(K_, which, monkeypatch):
    case = GEN[which]
    _setenv(monkeypatch, case, "gen")
    case.check_shape()
    prog = case.program()
    assert K_.hmc_engine(prog) == 4
    src = K_.program_hmc_source(prog)
    assert src.count("on the matrix cores") == case.expect["n_mfma"] and all(t in src for t in case.text), which
    assert "mfma_f32_16x16x4f32" in src
    (_, dim, n, bias, obs_al) = case.expect["sites"][0]
    y = prog.c_sites[[s.addr for s in prog.site_list.sites].index("y")]
    folded = case.expect["folded"]
    assert ("folded in the prologue" in src) == folded
    b128 = f"s_[t_] = *(const v4f_*)&TAB({y.p[0].off} + n0_ + 16 * t_ + 4 * q_);"
    unal = f"s_[t_][r_] = TAB({y.p[0].off} + n0_ + 16 * t_ + 4 * q_ + r_);"
    scal = f"const float b0_ = TAB({y.p[0].off}); s_[t_]"
    want = None if folded else {"scalar": scal, "aligned": b128, "misaligned": unal}[bias]
    for t in (b128, unal, scal):
        assert (t in src) == (t == want), (which, t)
    y128 = f"const v4f_ y4_ = *(const v4f_*)&TAB({y.obs_off} + n0_ + 16 * t_ + 4 * q_);"
    assert (y128 in src) == (not folded and obs_al == "aligned"), which
    any_in = which != "normal_64x16_inputs_not_selected"
    assert ("xc_[t_][b_] = " in src) == any_in and ("__shfl(gacc_[0]" in src) == any_in
    sel_slots = set(R.selected_slots(prog, case.selected)) if any_in else set()
    for e in range(n):                                                                       # the 16-lane exchange, input by input
        t = f"__shfl(gacc_[0][{e // 16}][{e % 4}], c16_ + {16 * ((e % 16) // 4)}, 64);"
        assert (t in src) == (y.p[0].slot + e in sel_slots), (which, e)
    monkeypatch.setenv("GJX_HMC_GEN_NO_MFMA", "1")
    assert "on the matrix cores" not in K_.program_hmc_source(prog)
    monkeypatch.setenv("GJX_HMC_ENGINE", "interp")
    assert K_.hmc_engine(prog) == 0


@pytest.mark.parametrize("which", list(FUSED))
def test_logistic_cases_have_their_shape_and_their_engine(K_, which, monkeypatch):
    case = FUSED[which]
    _setenv(monkeypatch, case, "fused")
    prog = R.fused_shape(case)
    assert K_.hmc_engine(prog) == case.engine and case.engine in (2, 3)
    y = case.obs["y"]
    assert (((y == 0) | (y == 1)).all()) == ("y03" not in which)
    monkeypatch.setenv("GJX_HMC_ENGINE", "gen")
    assert K_.hmc_engine(prog) == 4


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(HMC))
def test_the_analytic_float64_gradient_is_the_derivative_of_the_float64_score(which):
    case = HMC[which]
    prog = case.program()
    q0 = R.start_state(case, prog, 8, 5).astype(np.float64)
    g = R.stack_selected(prog, case.selected, case.ref.gradient(R.values_of(prog, q0)))
    rows = R.selected_slots(prog, case.selected)
    for r, row in enumerate(rows):
        h = 1e-6 * (1.0 + np.abs(q0[row]))
        qp, qm = q0.copy(), q0.copy()
        qp[row] += h
        qm[row] -= h
        fd = (case.ref.site_scores(R.values_of(prog, qp)).sum(0) - case.ref.site_scores(R.values_of(prog, qm)).sum(0)) / (2 * h)
        np.testing.assert_allclose(g[r], fd, rtol=1e-5, atol=1e-5 * (1.0 + np.abs(g).max()), err_msg=f"{which} slot {row}")


# ---- the oracle against the restatement, within the bounds ---------------------------------------------------------------------------
def _condition(what, bound, ref, rt, at):
    """the bound is never looser than the tolerance in force in the neighbouring tests, for every column"""
    tol = rt * np.abs(ref) + at
    fin = np.isfinite(ref)
    assert (np.broadcast_to(bound, ref.shape)[fin] <= tol[fin]).all(), (what, float((np.broadcast_to(bound, ref.shape)[fin] / tol[fin]).max()))


@pytest.mark.parametrize("which", list(PROP))
def test_the_oracle_scores_propagate_cases_within_the_bounds(oracle, which):
    case = PROP[which]
    prog = case.program()
    for K in R.PROP_KS[-1:]:
        o = oracle.run_program(prog, (0, 5), K, want_site_scores=True)
        ref = R.prop_reference(case, prog, o["choices"])
        j = [s.addr for s in prog.site_list.sites].index("y")
        rs = [R.worst_ratio(o["site_scores"][j], ref["site"][j], ref["site_bound"][j]), R.worst_ratio(o["score"], ref["score"], ref["score_bound"]),
              R.worst_ratio(o["weight"], ref["weight"], ref["weight_bound"])]
        print(f"{which} K={K}: oracle worst |error| / bound: site {rs[0]:.3f} score {rs[1]:.3f} weight {rs[2]:.3f}")
        assert max(rs) <= 1.0, (which, rs)
        for k in ("score", "weight"):
            _condition(f"{which} {k}", ref[k + "_bound"], ref[k], R.SCORE_RT, R.SCORE_AT)
        _condition(f"{which} site", ref["site_bound"][j], ref["site"][j], R.SCORE_RT, R.SCORE_AT)


@pytest.mark.parametrize("which", list(HMC))
def test_the_oracle_scores_and_differentiates_hmc_cases_within_the_bounds(oracle, which):
    case = HMC[which]
    prog = case.program()
    q0 = R.start_state(case, prog, N_CHAINS, 7)
    ref = R.hmc_reference(case, prog, q0)
    score, grad = oracle.score_grad(prog, q0)
    rows = R.selected_slots(prog, case.selected)
    rs = [R.worst_ratio(score, ref["score"], ref["score_bound"]), R.worst_ratio(grad[rows], ref["grad"], ref["grad_bound"])]
    # the recovery of the gradient from two one-step moves, on the oracle's own float32 leapfrog
    q1 = [oracle.hmc(prog, (4, 1), q0, e, 1, False, False, offset=5)["choices"] for e in (R.EPS1, R.EPS2)]
    rec = R.recover_gradient(q0[rows], q1[0][rows], q1[1][rows])
    full = ref["grad_bound"] + R.recovery_rounding(q1[0][rows], q1[1][rows], ref["grad"])
    rs.append(R.worst_ratio(rec, ref["grad"], full))
    print(f"{which}: oracle worst |error| / bound: score {rs[0]:.3f} gradient {rs[1]:.3f} recovered gradient {rs[2]:.3f}")
    assert max(rs) <= 1.0, (which, rs)
    _condition(f"{which} score", ref["score_bound"], ref["score"], R.SCORE_RT, R.SCORE_AT)
    _condition(f"{which} gradient", ref["grad_bound"] + R.recovery_rounding_worst(q0[rows].astype(np.float64), ref["grad"]), ref["grad"], R.GRAD_RT, R.GRAD_AT)


# ---- C_ELEM ---------------------------------------------------------------------------------------------------------------------------
def _element_error(oracle, case, prog, vals):
    """the oracle's element log-density against float64 at the SAME float32 logits, in units of u (1 + |l|): every element of every
    affine site of the case as one column of a carrier program  p_k ~ uniform, x ~ KIND(xf_k(p_k))"""
    worst = 0.0
    for s in case.ref.affine_sites():
        n = next(iter(vals.values())).shape[1]
        _, raws, _ = case.ref.elements(s, vals)
        raws = [np.broadcast_to(r, (s["dim"], n)).astype(np.float32).ravel() for r in raws]
        x = np.broadcast_to(s["obs"][:, None], (s["dim"], n)).astype(np.float32).ravel()
        sl = SiteList()
        for k in range(len(raws)):
            sl.add(f"p{k}", A.UNIFORM, [-1e37, 1e37])
        sl.add("x", s["kind"], [Param.value(f"p{k}", xf=q["xf"]) for k, q in enumerate(s["pars"])])
        carrier = PackedProgram(sl, {a: A.MODE_OBS_SLOT for a in [f"p{k}" for k in range(len(raws))] + ["x"]})
        ch = np.stack(raws + [x])
        got = oracle.run_program(carrier, (1, 2), ch.shape[1], choices=ch, want_site_scores=True)["site_scores"][len(raws)].astype(np.float64)
        want = R.logpdf(s["kind"], x.astype(np.float64), [R._xf(q["xf"], r.astype(np.float64))[0] for q, r in zip(s["pars"], raws)])
        fin = np.isfinite(want)
        assert (got[~fin] == want[~fin]).all()
        worst = max(worst, float((np.abs(got - want)[fin] / (R.U * (1.0 + np.abs(want[fin])))).max()))
    return worst


def test_c_elem_is_four_times_the_oracles_measured_element_error(oracle):
    worst = {}
    for name, case in PROP.items():
        prog = case.program()
        vals = R.values_of(prog, oracle.run_program(prog, (0, 5), 256)["choices"])
        worst[name] = _element_error(oracle, case, prog, vals)
    for name, case in HMC.items():
        prog = case.program()
        worst[name] = _element_error(oracle, case, prog, R.values_of(prog, R.start_state(case, prog, 64, 7)))
    top = max(worst, key=worst.get)
    print(f"oracle element error, units of u (1 + |l|): worst {worst[top]:.2f} ({top}); recorded {R.C_ELEM_MEASURED}")
    assert worst[top] <= R.C_ELEM_MEASURED and worst[top] >= 0.25 * R.C_ELEM_MEASURED, worst       # the record is the measurement, not a guess
    assert R.C_ELEM == 4.0 * R.C_ELEM_MEASURED


# ---- discrimination -------------------------------------------------------------------------------------------------------------------
def _moves(which, case, vals, what):
    base_s, base_g = case.ref.site_scores(vals).sum(0), None
    bound_s = case.ref.score_bounds(vals)[1]
    if case.selected:
        base_g = np.concatenate([case.ref.gradient(vals)[a] for a in case.selected], 0)
        bound_g = np.concatenate([case.ref.gradient_bounds(vals)[a] for a in case.selected], 0)
        bound_g = bound_g + R.recovery_rounding_worst(np.concatenate([vals[a] for a in case.selected], 0), base_g)
    bad = R.misplacements(case.ref)
    assert {"last row dropped", "last row counted twice"} <= set(bad) and len(bad) >= what, (which, sorted(bad))
    for name, ref in bad.items():
        with np.errstate(invalid="ignore"):
            moved = np.abs(ref.site_scores(vals).sum(0) - base_s) > 10.0 * bound_s
            if base_g is not None:
                g = np.concatenate([ref.gradient(vals)[a] for a in case.selected], 0)
                moved = moved | (np.abs(g - base_g) > 10.0 * bound_g).any(0)
        assert moved.mean() >= 0.5, (which, name, float(moved.mean()))


@pytest.mark.parametrize("which", list(PROP))
def test_misplaced_inputs_move_propagate_scores_by_more_than_ten_bounds(oracle, which):
    case = PROP[which]
    prog = case.program()
    vals = R.values_of(prog, oracle.run_program(prog, (0, 5), 256)["choices"])
    _moves(which, case, vals, 4 if case.expect["sites"][0][3] == "scalar" else 6)


@pytest.mark.parametrize("which", list(HMC))
def test_misplaced_inputs_move_hmc_scores_or_gradients_by_more_than_ten_bounds(which):
    case = HMC[which]
    prog = case.program()
    N = case.expect["sites"][0][1]
    P, vector = case.expect["sites"][0][2], case.ref.affine_sites()[0]["pars"][0]["values"].size > 1
    _moves(which, case, R.values_of(prog, R.start_state(case, prog, 64, 7)), (2 if N == 1 else 3) + (P > 2) + (2 if vector and N > 1 else 0))
