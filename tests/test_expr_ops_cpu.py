"""The CPU twins of tests/test_gpu_expr_ops.py: the same programs and grids (tests/expr_ops_ref.py) on the CPU oracle and on the host
evaluator expr.evaluate, against the same float64 restatement; the conditioning of that restatement on every grid; the packed forms
the fixes of this area pin (integer powers without log, linear forms that read no unnamed row) and the filter's refresh key.
Tolerances are those of the harness (helpers.py): scores rtol 2e-4 / atol 2e-4, gradients rtol 2e-3 / atol 2e-3."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import helpers as H                       # noqa: E402
import expr_ops_ref as R                  # noqa: E402
import genjax_amd as genjax               # noqa: E402
from genjax_amd import C                  # noqa: E402
from genjax_amd import _abi as A          # noqa: E402
from genjax_amd import expr as E          # noqa: E402
from genjax_amd.program import PackedProgram      # noqa: E402

from expr_ops_ref import REFRESH_CS, REFRESH_YS, fd_gradient, packed, same_nonfinite, selected_rows, switching_filter      # noqa: E402

K, N_GRAD, RT, AT = H.GRID_K, H.GRID_N_GRAD, H.GRID_RT, H.GRID_AT


@pytest.mark.parametrize("which", list(R.SPECS))
def test_the_reference_is_well_conditioned_on_every_grid_and_the_programs_hold_the_ops(which):
    spec = R.SPECS[which]
    want = H.well_conditioned(spec, spec["grid"](K), edges=True)            # every one of the K columns, none excluded
    assert want.shape == (len(spec["sites"]), K)
    prog = packed(spec, which)
    assert spec["ops"] <= R.block_ops(prog), sorted(spec["ops"] - R.block_ops(prog))
    g = spec["grad_grid"](N_GRAD)
    s = np.stack(spec["scores"]({k: x.astype(np.float64) for k, x in g.items()}))
    sel = [i for i, (a, _) in enumerate(spec["sites"]) if a not in R.UNSELECTED.get(which, ())]
    assert np.isfinite(s[sel]).all()                                        # the gradient grids hold kinks and boundaries, no infinities


def test_every_one_of_the_25_ops_is_in_some_program():
    ops = set()
    for which, spec in R.SPECS.items():
        ops |= R.block_ops(packed(spec, which))
    assert ops >= set(range(25)), sorted(set(range(25)) - ops)


@pytest.mark.parametrize("which", list(R.SPECS))
def test_the_oracle_scores_the_grids_like_float64(which):
    from oracle import cpu
    spec = R.SPECS[which]
    prog = packed(spec, which)
    vals = spec["grid"](K)
    want = H.float32_range(H.well_conditioned(spec, vals, edges=True))
    o = cpu.run_program(prog, (3, 7), K, choices=H.grid_rows(prog, spec, vals), want_site_scores=True)
    fin = same_nonfinite(o["site_scores"], want, which)
    np.testing.assert_allclose(o["site_scores"][fin], want[fin], rtol=RT, atol=AT)
    tot = H.float32_range(want.sum(0))
    fin = same_nonfinite(o["score"], tot, which)
    np.testing.assert_allclose(o["score"][fin], tot[fin], rtol=RT, atol=AT)


@pytest.mark.parametrize("which", list(R.SPECS))
def test_the_oracle_differentiates_the_grids_like_float64(which):
    from oracle import cpu
    spec = R.SPECS[which]
    prog = packed(spec, which, grad=True)
    ch = H.grid_rows(prog, spec, spec["grad_grid"](N_GRAD))
    rows = selected_rows(spec, prog, which)
    fd, total = fd_gradient(spec, prog, ch, rows)
    sc, g = cpu.score_grad(prog, ch)
    fin = same_nonfinite(sc, H.float32_range(total), which)
    assert fin.sum() >= N_GRAD // 8
    np.testing.assert_allclose(sc[fin], total[fin], rtol=RT, atol=AT, err_msg=which)
    for r in rows:
        assert np.isfinite(g[r]).all(), (which, r)
        np.testing.assert_allclose(g[r], fd[r], rtol=2e-3, atol=2e-3, err_msg=f"{which} row {r}")
    if which == "unary":
        for r, cols in R.exact_zero_gradients(prog, ch):
            assert (np.abs(g[r][cols]) <= 1e-37).all(), (r, g[r][cols])


@pytest.mark.parametrize("which", list(R.SPECS))
def test_the_host_evaluator_gives_the_values_of_the_restatement(which):
    spec = R.SPECS[which]
    sl, _ = spec["model"].site_list(())
    v = {k: x.astype(np.float64) for k, x in spec["grid"](K).items()}
    want = spec["values"](v)
    n_checked = 0
    for name, place, _, _ in spec["opsites"]:
        p = sl[name].params[0 if place == "mean" else 1]
        if p.op != A.P_EXPR:
            continue                                 # (a ** 0, a ** 1 on a plain value: closed forms, no expression)
        got = H.float32_range(np.broadcast_to(E.evaluate(p.outs, lambda a, e: v[a][e])[0], (K,)))
        fin = same_nonfinite(got, want[name], name)
        np.testing.assert_allclose(got[fin], np.broadcast_to(want[name], (K,))[fin], rtol=1e-6, atol=1e-30, err_msg=name)
        n_checked += 1
    assert n_checked >= len(spec["opsites"]) - 3


# ---- the packed forms ------------------------------------------------------------------------------------------------------------
def _nodes(prog, addr, k=0):
    j = [s.addr for s in prog.device_site_list.sites].index(addr)
    cp = prog.c_sites[j].p[k]
    assert cp.op == A.P_EXPR
    return prog.tab[cp.off:cp.off + A.EXPR_NODE_FLOATS * cp.n].reshape(-1, A.EXPR_NODE_FLOATS).astype(int)


def test_integer_powers_are_squares_and_products():
    """a ** k for an integer k: SQUARE, MUL and RECIP only (no LOG, no EXP), at most 2 log2|k| + 1 of them; k = 0.5 and a non-integer k
    keep their forms; the values on a negative base are those of float64"""
    spec = R.SPECS["powers"]
    prog = packed(spec, "powers")
    for k in R.POWERS:
        if k in (0, 1):
            continue
        nd = _nodes(prog, f"z_pow_{k}") if k > 1 else _nodes(prog, f"a_pow_{k}", 1)
        ops = nd[:, 0].tolist()
        assert set(ops) <= {A.E_VALUE, A.E_SQUARE, A.E_MUL, A.E_RECIP}, (k, ops)
        assert len([o for o in ops if o != A.E_VALUE]) - (k < 0 and k % 2 != 0) <= 2 * int(np.log2(abs(k))) + 1, (k, ops)

    @genjax.gen
    def model():
        a = genjax.normal(0.0, 1.0) @ "a"
        genjax.normal(a ** 4, 1.0) @ "p4"
        genjax.normal(a ** -2, 1.0) @ "m2"
        genjax.normal(a ** 2.5, 1.0) @ "frac"
        genjax.normal(a ** 0.5, 1.0) @ "half"
        return a ** 4
    sl, ret = model.site_list(())
    leaf = lambda a_, e_: np.array([-2.0, 3.0])                    # noqa: E731
    np.testing.assert_array_equal(E.evaluate(sl["p4"].params[0].outs, leaf)[0], [16.0, 81.0])
    np.testing.assert_allclose(E.evaluate(sl["m2"].params[0].outs, leaf)[0], [0.25, 1.0 / 9.0])
    frac = E.evaluate(sl["frac"].params[0].outs, leaf)[0]
    assert np.isnan(frac[0]) and frac[1] == pytest.approx(3.0 ** 2.5)             # a non-integer power of a negative base: NaN (jnp.power)
    assert sl["half"].params[0].outs[0][0] == "sqrt"


def test_a_linear_form_reads_only_the_rows_it_names():
    """exp(a * a) + 2 a + 3 c over the slots of a, b, c: no LINV node spans b's row; the oracle's value and gradient with b = inf and
    b = NaN are those of float64"""
    from oracle import cpu

    @genjax.gen
    def model():
        a = genjax.normal(0.0, 1.0) @ "a"
        genjax.normal(0.0, 1.0) @ "b"
        c = genjax.normal(0.0, 1.0) @ "c"
        genjax.normal(genjax.exp(a * a) + 2.0 * a + 3.0 * c, 1.0) @ "y"
    sl, _ = model.site_list(())
    prog = PackedProgram(sl, {s.addr: A.MODE_OBS_SLOT for s in sl.sites}, {}, selected=("a", "c"))
    nd = _nodes(prog, "y")
    named = {prog.slot_of["a"], prog.slot_of["c"]}
    read = set()
    for op, a, b, c, _, _ in nd:
        if op == A.E_VALUE:
            read.add(a)
        if op == A.E_LINV:
            read |= set(range(b, b + c))
            assert (prog.tab[a + 1:a + 1 + c] != 0.0).all()                       # no zero weight: nothing is bridged
    assert read == named
    ch = np.array([[0.5, 0.5, -0.3], [np.inf, np.nan, 1.0], [0.25, 0.25, 0.7], [1.0, 1.0, 1.0]], np.float32)
    o = cpu.run_program(prog, (0, 1), 3, choices=ch, want_site_scores=True)
    a64, c64 = ch[0].astype(np.float64), ch[2].astype(np.float64)
    np.testing.assert_allclose(o["site_scores"][3], H.nlp(1.0, np.exp(a64 * a64) + 2 * a64 + 3 * c64, 1.0), rtol=2e-5, atol=2e-5)
    _, g = cpu.score_grad(prog, ch)
    assert np.isfinite(g[[0, 2]]).all() and (g[1] == 0).all()


# ---- the filter's refresh key ----------------------------------------------------------------------------------------------------
def test_the_refresh_key_sees_data_that_became_nodes():
    flt = switching_filter()
    con = C["y"].set(REFRESH_YS)
    pa = flt.step_programs(con, (np.float32(0.1), REFRESH_CS[0]))
    pb = flt.step_programs(con, (np.float32(0.1), REFRESH_CS[1]))
    differ = []
    for a, b in zip(pa, pb):
        assert a.sites_bytes() == b.sites_bytes() and a.tab.size == b.tab.size and a.n_slots == b.n_slots      # what the guard used to compare
        differ.append(a.structure_bytes() != b.structure_bytes())
    assert differ == [False, True, False, True]
    from genjax_amd.inference.scan_filter import same_structure
    assert not same_structure(pb, pa) and same_structure(pa, flt.step_programs(con, (np.float32(0.1), REFRESH_CS[0])))      # the filter's own guard
    assert A.E_EXP in R.block_ops(pa[1]) and A.E_TANH in R.block_ops(pb[1]) and A.E_EXP not in R.block_ops(pb[1])
    # data that changes constants only (the observations) keeps the key: the cheap refresh path survives
    pc = flt.step_programs(C["y"].set(REFRESH_YS[::-1].copy()), (np.float32(0.1), REFRESH_CS[0]))
    assert all(a.structure_bytes() == c.structure_bytes() for a, c in zip(pa, pc))
    assert any((a.tab != c.tab).any() for a, c in zip(pa, pc)) and same_structure(pc, pa)


# ---- the structural cases on the oracle ------------------------------------------------------------------------------------------
def test_the_plate_and_the_scan_on_the_oracle():
    """the programs of the two structural GPU tests: one plate site / 64 steps, no unnamed row read, the oracle's scores those of float64"""
    from oracle import cpu
    prog, rows, scores = R.structural_plate(257)
    assert prog.n_sites == 5 and prog.c_sites[4].plate_n == R.N_PLATE and prog.c_sites[4].p[0].op == A.P_EXPR
    want = H.float32_range(scores(rows.astype(np.float64)))
    o = cpu.run_program(prog, (4, 5), 257, choices=rows, want_site_scores=True)
    fin = same_nonfinite(o["site_scores"], want, "plate")
    np.testing.assert_allclose(o["site_scores"][fin], want[fin], rtol=RT, atol=AT)
    prog, restate = R.structural_scan()
    assert prog.n_sites == 4 * R.T_SCAN
    o = cpu.run_program(prog, (8, 9), 257)
    lik, prior = restate(prog, o["choices"].astype(np.float64))
    np.testing.assert_allclose(o["logw"], lik, rtol=RT, atol=AT)
    np.testing.assert_allclose(o["score"], lik + prior, rtol=RT, atol=AT)
