"""The CPU twins of tests/test_gpu_expr_ops.py: the same programs and grids (tests/expr_ops_ref.py) on the CPU oracle and on the host
evaluator expr.evaluate, against the same float64 restatement; the conditioning of that restatement on every grid; the packed forms
the fixes of this area pin (integer powers without log, linear forms that read no unnamed row, log-sum-exp chunks and folds, the
NumPy / scipy spellings of the reductions and special functions), the oracle's refusal of unknown ops and the filter's refresh key.
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

from genjax_amd.program import Param, SiteList                # noqa: E402

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


def test_every_node_op_is_in_some_program():
    ops = set()
    for which, spec in R.SPECS.items():
        ops |= R.block_ops(packed(spec, which))
    assert A.E_OP_MAX == 30 and ops >= set(range(A.E_OP_MAX)), sorted(set(range(A.E_OP_MAX)) - ops)


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
    if which in R.EXACT_ZERO:
        for r, cols in R.EXACT_ZERO[which](prog, ch):
            assert (np.abs(g[r][cols]) <= 1e-37).all(), (r, g[r][cols])


@pytest.mark.parametrize("which", list(R.SPECS))
def test_the_host_evaluator_gives_the_values_of_the_restatement(which):
    spec = R.SPECS[which]
    sl, _ = spec["model"].site_list(())
    v = {k: x.astype(np.float64) for k, x in spec["grid"](K).items()}
    want = spec["values"](v)
    n_checked, closed = 0, set()
    for name, place, _, _ in spec["opsites"]:
        p = sl[name].params[0 if place == "mean" else 1]
        if p.op != A.P_EXPR:
            closed.add(name)                         # (a ** 0, a ** 1 on a plain value: closed forms, no expression)
            continue
        got = H.float32_range(np.broadcast_to(E.evaluate(p.outs, lambda a, e: v[a][e])[0], (K,)))
        fin = same_nonfinite(got, want[name], name)
        np.testing.assert_allclose(got[fin], np.broadcast_to(want[name], (K,))[fin], rtol=1e-6, atol=1e-30, err_msg=name)
        n_checked += 1
    assert n_checked >= len(spec["opsites"]) - 3 if which not in R.CLOSED_FORMS else closed == R.CLOSED_FORMS[which]


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


# ---- the newer ops: the oracle's own pieces, the packed forms of log-sum-exp and of the reductions, the NumPy / scipy spellings -----
def test_the_oracle_refuses_a_node_op_it_does_not_know():
    """an op code past GJX_E_OP_MAX (and a log-sum-exp over 65 operands) is an error in Python from every entry point — it used to be
    scored as a reciprocal; RECIP itself is still the reciprocal"""
    from oracle import cpu
    sl = SiteList()
    sl.add("a", A.NORMAL, [0.0, 1.0])
    sl.add("y", A.NORMAL, [Param.expr([E.unary("recip", E.unary("tanh", E.value("a", 0)))]), 1.0])
    prog = PackedProgram(sl, {"a": A.MODE_OBS_SLOT, "y": A.MODE_OBS_SLOT}, {}, selected=("a",))
    ch = np.array([[0.5, -2.0], [0.25, 0.25]], np.float32)
    o = cpu.run_program(prog, (0, 1), 2, choices=ch, want_site_scores=True)
    np.testing.assert_allclose(o["site_scores"][1], H.nlp(0.25, 1.0 / np.tanh(ch[0].astype(np.float64)), 1.0), rtol=2e-6)
    nd = _nodes(prog, "y")
    cp = prog.c_sites[1].p[0]
    at = cp.off + A.EXPR_NODE_FLOATS * int(np.nonzero(nd[:, 0] == A.E_RECIP)[0][0])
    for bad in (A.E_OP_MAX, A.E_OP_MAX + 7, -1):
        prog.tab[at] = bad
        for call in (lambda: cpu.run_program(prog, (0, 1), 2, choices=ch), lambda: cpu.score_grad(prog, ch), lambda: cpu.hmc(prog, (0, 1), ch, 1e-3, 2)):
            with pytest.raises(ValueError, match="refused"):
                call()
    prog.tab[at] = A.E_RECIP
    cpu.score_grad(prog, ch)


def test_the_oracle_s_digamma_is_scipy_s_on_both_sides_of_zero():
    """d/da of normal(lgamma(a), 1) at y = lgamma(a) + 1 is digamma(a): the oracle's recurrence, series and reflection against
    scipy.special.digamma from 1e-3 to 1e6 and between the negative poles down to -60"""
    import scipy.special as sp
    from oracle import cpu
    sl = SiteList()
    sl.add("a", A.UNIFORM, [-1e37, 1e37])
    sl.add("y", A.NORMAL, [Param.expr([E.unary("lgamma", E.value("a", 0))]), 1.0])
    prog = PackedProgram(sl, {"a": A.MODE_OBS_SLOT, "y": A.MODE_OBS_SLOT}, {}, selected=("a",))
    rs = np.random.default_rng(5)
    a = np.concatenate([np.geomspace(1e-3, 1e6, 300), [0.5, 1.0, 1.4616321, 2.0, 9.99, 10.0], -(rs.integers(0, 60, 600) + rs.uniform(0.02, 0.98, 600))]).astype(np.float32)
    a64 = a.astype(np.float64)
    y = (sp.gammaln(a64) + 1.0).astype(np.float32)
    _, g = cpu.score_grad(prog, np.stack([a, y]))
    want = (y.astype(np.float64) - np.float32(sp.gammaln(a64)).astype(np.float64)) * sp.digamma(a64)
    np.testing.assert_allclose(g[0], want, rtol=1e-5, atol=1e-6)
    assert (a < -5).sum() > 400


def _lse_model(n_operands):
    @genjax.gen
    def model():
        x = [genjax.mv_normal_diag(np.zeros(32, np.float32), np.ones(32, np.float32)) @ f"x{j}" for j in range(3)]
        el = [x[j // 32][j % 32] for j in range(n_operands)]
        genjax.normal(genjax.logsumexp(el), 1.0) @ "y"
    sl, _ = model.site_list(())
    return PackedProgram(sl, {s.addr: A.MODE_OBS_SLOT for s in sl.sites})


def test_the_packed_forms_of_log_sum_exp():
    """93 operands are exactly GJX_EXPR_MAX_NODES nodes and 94 are too many; 65 operands are a 64-operand node, a one-operand node and a
    node over both; an lse of lse's is ONE node over the leaves and its constant operands fold into one"""
    nd = _nodes(_lse_model(93), "y")
    assert len(nd) == A.EXPR_MAX_NODES == 96 and (nd[:93, 0] == A.E_VALUE).all()
    assert [tuple(r[[0, 2, 3]]) for r in nd[93:]] == [(A.E_LSEN, 0, 64), (A.E_LSEN, 64, 29), (A.E_LSEN, 93, 2)]
    with pytest.raises(E.ExprTooLarge):
        _lse_model(94)
    nd = _nodes(_lse_model(65), "y")
    assert [tuple(r[[0, 2, 3]]) for r in nd[nd[:, 0] == A.E_LSEN]] == [(A.E_LSEN, 0, 64), (A.E_LSEN, 64, 1), (A.E_LSEN, 65, 2)]
    spec = R.SPECS["lse"]
    prog = packed(spec, "lse")
    for k in R.LSE_ARITIES:
        ops = _nodes(prog, f"lse_{k}")[:, 0]
        assert (ops == A.E_LSEN).sum() == (1 if k <= 64 else 3) and (ops == A.E_VALUE).sum() == k
    nd = _nodes(prog, "lse_nested")
    lse_rows = nd[nd[:, 0] == A.E_LSEN]
    assert len(lse_rows) == 1 and lse_rows[0][3] == 4                        # b, c * c, c and ONE constant: log(e^0.5 + e^1.5)
    consts = [float(prog.tab[r[1]]) for r in nd if r[0] == A.E_CONST]
    assert consts == [pytest.approx(np.logaddexp(0.5, 1.5), rel=1e-7)]
    sl, _ = spec["model"].site_list(())
    assert sl["logaddexp"].params[0].outs[0][0] == "lse" and len(sl["logaddexp"].params[0].outs[0][1]) == 2


def _packs_alike(body_a, body_b):
    def pack_of(body):
        @genjax.gen
        def model():
            v = genjax.mv_normal_diag(np.zeros(6, np.float32), np.ones(6, np.float32)) @ "v"
            a = genjax.normal(0.0, 1.0) @ "a"
            for i, f in enumerate(body(v, a)):
                genjax.normal(f, 1.0) @ f"y{i}"
        sl, _ = model.site_list(())
        return PackedProgram(sl, {s.addr: A.MODE_OBS_SLOT for s in sl.sites})
    pa, pb = pack_of(body_a), pack_of(body_b)
    assert pa.n_sites == pb.n_sites and pa.n_sites > 2
    assert pa.structure_bytes() == pb.structure_bytes() and pa.sites_bytes() == pb.sites_bytes() and pa.tab.tobytes() == pb.tab.tobytes()
    return pa


def test_every_numpy_and_scipy_spelling_packs_like_the_method():
    import scipy.special as sp
    for gen_of in (lambda v: v, genjax.tanh):                                    # the plain latent vector (closed forms) and a general one
        p = _packs_alike(lambda v, a: (lambda g: [g.sum(), g.sum(), g.mean(), g.prod(), g.max(), g.max(), g.min(), g.min(), g.cumsum()[3], g.sum()])(gen_of(v)),
                         lambda v, a: (lambda g: [np.sum(g), np.add.reduce(g), np.mean(g), np.prod(g), np.max(g), np.amax(g), np.min(g), np.amin(g),
                                                  np.cumsum(g)[3], np.sum(g, axis=0)])(gen_of(v)))
        assert (gen_of is genjax.tanh) == (A.E_LINN in R.block_ops(p))
    p = _packs_alike(lambda v, a: [genjax.erf(a * a), genjax.erfc(a * a), genjax.lgamma(a * a), genjax.sigmoid(a * a), genjax.expm1(a * a),
                                   genjax.logsumexp([a * a, a]), genjax.logsumexp(v)],
                     lambda v, a: [sp.erf(a * a), sp.erfc(a * a), sp.gammaln(a * a), sp.expit(a * a), np.expm1(a * a), np.logaddexp(a * a, a),
                                   genjax.logsumexp([v[j] for j in range(6)])])
    assert {A.E_ERF, A.E_ERFC, A.E_LGAMMA, A.E_EXPM1, A.E_LSEN, A.E_SIGMOID} <= R.block_ops(p)


def test_the_host_evaluator_on_torch_tensors_agrees_with_its_numpy_path_for_the_newer_ops():
    import torch
    rs = np.random.default_rng(9)
    x = np.concatenate([rs.uniform(-3.0, 3.0, 200), [0.0, 1e-20, -1e-20, 5.0, -5.0, 30.0, -30.0]])
    xg = np.concatenate([rs.uniform(0.05, 12.0, 100), -(rs.integers(0, 6, 107) + rs.uniform(0.1, 0.9, 107))])
    for op, arg in (("erf", x), ("erfc", x), ("expm1", x), ("lgamma", xg)):
        n = E.unary(op, E.value("a", 0))
        got = E.evaluate([n], lambda a, e: torch.as_tensor(arg, dtype=torch.float64), xp=torch)[0].numpy()
        np.testing.assert_allclose(got, E.evaluate([n], lambda a, e: arg)[0], rtol=1e-12, atol=1e-300, err_msg=op)
    rows = rs.uniform(-3.0, 3.0, (5, 64))
    rows[:, 0], rows[1:, 1], rows[0, 2] = -np.inf, -np.inf, np.inf
    n = E.lse([E.value("r", j) for j in range(5)])
    got = E.evaluate([n], lambda a, e: torch.as_tensor(rows[e]), xp=torch)[0].numpy()
    want = E.evaluate([n], lambda a, e: rows[e])[0]
    assert got[0] == want[0] == -np.inf and got[2] == want[2] == np.inf
    np.testing.assert_allclose(got[3:], want[3:], rtol=1e-12)


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


def test_the_plate_and_the_scan_of_the_newer_ops_on_the_oracle():
    """the programs of the two structural GPU tests of the newer ops: ONE plate site of 16 instances whose mean is lgamma and whose scale
    is erfc, 64 rolled steps with a log-sum-exp, an expm1 scale and a guarded lgamma; the float64 restatement of the plate is well
    conditioned in every column and the oracle's scores are its"""
    from oracle import cpu
    prog, rows, scores = R.special_plate(K)
    body = prog.c_sites[4]
    assert prog.n_sites == 5 and body.plate_n == R.N_PLATE and body.p[0].op == A.P_EXPR and body.p[1].op == A.P_EXPR
    assert {A.E_LGAMMA, A.E_ERFC} <= R.block_ops(prog)
    r64 = rows.astype(np.float64)
    want, moved = scores(r64), scores(r64 * (1.0 + 2e-6))
    assert np.isfinite(want).all() and (np.abs(moved - want) < 0.5 * (AT + RT * np.abs(want))).all()
    arg_g = r64[0] * 2.0 + r64[1]
    assert arg_g.min() < -10.0 and (np.abs(r64[0][r64[1] == 0]).min() < 1e-11) and arg_g.max() > 14.0 and r64[3].min() < -5.9
    o = cpu.run_program(prog, (4, 5), K, choices=rows, want_site_scores=True)
    np.testing.assert_allclose(o["site_scores"], want, rtol=RT, atol=AT)
    prog, restate = R.special_scan()
    assert prog.n_sites == 3 * R.T_SCAN and {A.E_LSEN, A.E_EXPM1, A.E_LGAMMA, A.E_WHERE} <= R.block_ops(prog)
    o = cpu.run_program(prog, (8, 9), 257)
    lik, prior = restate(prog, o["choices"].astype(np.float64))
    np.testing.assert_allclose(o["logw"], lik, rtol=RT, atol=AT)
    np.testing.assert_allclose(o["score"], lik + prior, rtol=RT, atol=AT)
