"""What a ``@gen`` body may compute between two sites — CPU tests of the tracer's surface: reductions (sum / mean / prod / max / min /
cumsum), erf / erfc / lgamma / expm1, logsumexp (one GJX_E_LSEN device node per 64 operands), ``abs``, ``**`` with symbolic operands,
and NumPy / scipy.special calls on symbolic values (``__array_ufunc__`` / ``__array_function__``).  The closed parameter forms must
survive (``np.exp(site)`` is GJX_XF_EXP, ``x.sum()`` is GJX_P_AFFINE), and arrays on the LEFT of an operator must give what they gave
while the operators merely deferred to the reflected methods.  The reference for values is float64 scipy.special.
(The device engines are held to the same reference in tests/test_gpu_tracer_surface.py.)"""
import dataclasses
import os
import sys

import numpy as np
import pytest
import scipy.special as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import genjax_amd as genjax               # noqa: E402
from genjax_amd import _abi as A          # noqa: E402
from genjax_amd import expr as E          # noqa: E402
from genjax_amd.program import PackedProgram      # noqa: E402

DIM = 4
W = np.random.default_rng(0).standard_normal((3, DIM))
LW = np.linspace(-1.0, 1.0, DIM)


def _model(body):
    """a, b scalar latents, x a DIM-vector; the body's value is the mean of y"""
    @genjax.gen
    def model():
        a = genjax.normal(0.0, 1.0) @ "a"
        b = genjax.normal(0.5, 1.0) @ "b"
        x = genjax.mv_normal_diag(np.zeros(DIM, np.float32), np.ones(DIM, np.float32)) @ "x"
        genjax.normal(body(a, b, x), 1.0) @ "y"
    return model


def _param(body):
    sl, _ = _model(body).site_list(())
    return sl["y"].params[0]


def _block(body, dim=DIM):
    """int [n][6] node list of the mean of y, packed"""
    sl, _ = _model(body).site_list(())
    prog = PackedProgram(sl, {}, {})
    cp = prog.c_sites[prog.n_sites - 1].p[0]
    assert cp.op == A.P_EXPR
    return prog.tab[cp.off:cp.off + A.EXPR_NODE_FLOATS * cp.n].reshape(-1, A.EXPR_NODE_FLOATS).astype(int)


def _same(p, q):
    dp, dq = dataclasses.asdict(p), dataclasses.asdict(q)
    assert dp.keys() == dq.keys()
    for k in dp:
        if isinstance(dp[k], np.ndarray) or isinstance(dq[k], np.ndarray):
            assert dp[k] is not None and dq[k] is not None and np.array_equal(dp[k], dq[k]), k
        else:
            assert dp[k] == dq[k], k


BODIES = {
    "exp(x).sum()": lambda a, b, x: genjax.exp(x).sum(),
    "abs(x)": lambda a, b, x: abs(x)[0],
    "np.exp(x)": lambda a, b, x: np.sum(np.exp(x)),
    "np.sum(x * x)": lambda a, b, x: np.sum(x * x),
    "erf": lambda a, b, x: genjax.erf(a * b),
    "erfc": lambda a, b, x: genjax.erfc(a * b),
    "lgamma": lambda a, b, x: genjax.lgamma(a * a + 1.0),
    "expm1": lambda a, b, x: genjax.expm1(a * b),
    "logsumexp": lambda a, b, x: genjax.logsumexp(x * x),
    "np.tanh(W @ x)": lambda a, b, x: np.tanh(W @ x)[1],
    "scipy.special.erf(a)": lambda a, b, x: sp.erf(a),
    "lgamma(exp(a))": lambda a, b, x: genjax.lgamma(genjax.exp(a)),
    "logsumexp(lw + b * x)": lambda a, b, x: genjax.logsumexp(LW + b * x),
    "2.0 ** a": lambda a, b, x: 2.0 ** a,
    "a ** b": lambda a, b, x: a ** b,
}


@pytest.mark.parametrize("which", list(BODIES))
def test_bodies_a_user_writes_on_day_one_trace_and_pack(which):
    sl, _ = _model(BODIES[which]).site_list(())
    prog = PackedProgram(sl, {}, {})
    assert prog.n_sites == 4 and sl["y"].params[0].op in (A.P_EXPR, A.P_AFFINE, A.P_VALUE)


def test_public_names_and_plain_numbers():
    public = sys.modules["genjax_amd.gen"].__all__
    for name in ("erf", "erfc", "lgamma", "expm1", "logsumexp", "abs"):
        assert callable(getattr(genjax, name)) and name in public
    v = np.array([-1.5, 0.25, 2.0])
    np.testing.assert_allclose(genjax.erf(v), sp.erf(v), rtol=1e-15)
    np.testing.assert_allclose(genjax.erfc(v), sp.erfc(v), rtol=1e-15)
    np.testing.assert_allclose(genjax.lgamma(v), sp.gammaln(v), rtol=1e-14)
    np.testing.assert_allclose(genjax.expm1(v), np.expm1(v), rtol=1e-15)
    np.testing.assert_allclose(genjax.abs(v), np.abs(v))
    assert float(genjax.logsumexp(v)) == pytest.approx(float(sp.logsumexp(v)), rel=1e-15)
    np.testing.assert_allclose(genjax.logsumexp(np.stack([v, 2 * v]), axis=-1), sp.logsumexp(np.stack([v, 2 * v]), axis=-1), rtol=1e-15)


def test_numpy_calls_keep_the_closed_forms():
    p, q = _param(lambda a, b, x: np.exp(a)), _param(lambda a, b, x: genjax.exp(a))
    _same(p, q)
    assert p.op == A.P_VALUE and p.xf == A.XF_EXP
    _same(_param(lambda a, b, x: sp.expit(a)), _param(lambda a, b, x: genjax.sigmoid(a)))
    for body in (lambda a, b, x: x.sum(), lambda a, b, x: np.sum(x), lambda a, b, x: np.add.reduce(x), lambda a, b, x: np.sum(x, axis=-1)):
        p = _param(body)
        assert p.op == A.P_AFFINE and np.array_equal(p.matrix, np.ones((1, DIM), np.float32)) and not p.values.any()
    p = _param(lambda a, b, x: x.mean())
    assert p.op == A.P_AFFINE and np.array_equal(p.matrix, np.full((1, DIM), 0.25, np.float32))
    p = _param(lambda a, b, x: np.cumsum(2.0 * x + 1.0)[2])
    assert p.op == A.P_AFFINE and np.array_equal(p.matrix.ravel()[:3], [2.0, 2.0, 2.0]) and p.values.tolist() == [3.0]
    assert _param(lambda a, b, x: 2.0 ** a).xf == A.XF_EXP               # exp(a ln 2): a scaled value under GJX_XF_EXP


def test_a_sum_of_expressions_is_one_linear_node_over_its_operands():
    nodes = _block(lambda a, b, x: genjax.exp(x).sum())
    last = nodes[-1]
    assert last[0] == A.E_LINN and last[3] == DIM and (nodes[last[2]:last[2] + DIM, 0] == A.E_EXP).all()
    assert (nodes[:, 0] == A.E_EXP).sum() == DIM and len(nodes) == 2 * DIM + 1
    # mean and cumsum of an expression: one linear node per output; prod / max / min: chains of the binary ops
    nodes = _block(lambda a, b, x: (x * x).prod())
    assert (nodes[:, 0] == A.E_SQUARE).sum() + (nodes[:, 0] == A.E_MUL).sum() == 2 * DIM - 1 and nodes[-1][0] == A.E_MUL
    nodes = _block(lambda a, b, x: np.max(x) - x.min())
    assert (nodes[:, 0] == A.E_MAX).sum() == DIM - 1 and (nodes[:, 0] == A.E_MIN).sum() == DIM - 1


def test_logsumexp_is_one_device_node():
    lw = np.linspace(-1.0, 1.0, 8)

    @genjax.gen
    def model():
        b = genjax.normal(0.5, 1.0) @ "b"
        x = genjax.mv_normal_diag(np.zeros(8, np.float32), np.ones(8, np.float32)) @ "x"
        genjax.normal(genjax.logsumexp(lw + b * x), 1.0) @ "y"

    sl, _ = model.site_list(())
    prog = PackedProgram(sl, {}, {})
    cp = prog.c_sites[2].p[0]
    nodes = prog.tab[cp.off:cp.off + A.EXPR_NODE_FLOATS * cp.n].reshape(-1, A.EXPR_NODE_FLOATS).astype(int)
    lse = [i for i in range(len(nodes)) if nodes[i][0] == A.E_LSEN]
    assert lse == [len(nodes) - 1]
    op, a_, b_, c_, da, db = nodes[-1]
    assert c_ == 8 and b_ >= 0 and b_ + c_ <= len(nodes) - 1 and da == 0 and db == 0
    # the operands are the 8 rows lw_i + b x_i, at consecutive indices, each one linear node over its product
    ops = nodes[b_:b_ + 8]
    assert (ops[:, 0] == A.E_LINN).all() and (ops[:, 3] == 1).all()
    np.testing.assert_allclose([prog.tab[o[1]] for o in ops], lw.astype(np.float32))
    assert all(nodes[o[2]][0] == A.E_MUL for o in ops)
    # an lse of lse's is one node; constants fold; one operand is itself
    n = [E.value("x", i) for i in range(4)]
    assert E.lse([E.lse(n[:2]), E.lse(n[2:])]) == ("lse", tuple(n))
    assert E.lse([n[0]]) == n[0] and E.lse([E.const(1.0), E.const(2.0)])[1] == pytest.approx(float(sp.logsumexp([1.0, 2.0])), rel=1e-15)
    assert E.lse([n[0], E.const(-np.inf)]) == n[0] and E.lse([n[0], E.const(1.0), E.const(2.0)])[1][1][1] == pytest.approx(float(sp.logsumexp([1.0, 2.0])), rel=1e-15)
    assert E.count_nodes([E.lse(n)]) == 5 and E.sources([E.lse(n)]) == ["x"]


@pytest.mark.parametrize("n", [70, 100])
def test_more_than_64_operands_are_chunked_or_refused(n):
    """every operand costs at least one node, every chunk of 64 one LSEN, several chunks one more"""
    @genjax.gen
    def model():
        x = genjax.mv_normal_diag(np.zeros(n, np.float32), np.ones(n, np.float32)) @ "x"
        genjax.normal(genjax.logsumexp(x), 1.0) @ "y"

    sl, _ = model.site_list(())
    chunks = -(-n // 64)
    need = n + chunks + (1 if chunks > 1 else 0)
    if need > A.EXPR_MAX_NODES:
        with pytest.raises(E.ExprTooLarge):
            PackedProgram(sl, {}, {})
        return
    prog = PackedProgram(sl, {}, {})
    cp = prog.c_sites[1].p[0]
    nodes = prog.tab[cp.off:cp.off + A.EXPR_NODE_FLOATS * cp.n].reshape(-1, A.EXPR_NODE_FLOATS).astype(int)
    assert len(nodes) == need <= A.EXPR_MAX_NODES
    lse = nodes[nodes[:, 0] == A.E_LSEN]
    assert lse[:, 3].tolist() == [64, n - 64, 2]
    top = nodes[-1]
    assert (nodes[top[2]:top[2] + 2, 0] == A.E_LSEN).all()                      # the chunks' results, consecutive
    covered = sorted(s for l_ in lse[:-1] for s in nodes[l_[2]:l_[2] + l_[3], 1].tolist())
    assert covered == list(range(n)) and all((nodes[l_[2]:l_[2] + l_[3], 0] == A.E_VALUE).all() for l_ in lse[:-1])


LGAMMA_POINTS = np.concatenate([0.23 + 0.197 * np.arange(40), [-k - f for k in range(6) for f in (0.3, 0.45, 0.6, 0.75)]])
POINTS = {"erf": np.linspace(-3.0, 3.0, 64), "erfc": np.linspace(-3.0, 3.0, 64), "expm1": np.linspace(-3.0, 3.0, 64), "lgamma": LGAMMA_POINTS}
SCIPY = {"erf": sp.erf, "erfc": sp.erfc, "expm1": sp.expm1, "lgamma": sp.gammaln}


@pytest.mark.parametrize("op", list(POINTS))
def test_evaluate_against_scipy_special(op):
    v = POINTS[op]
    assert v.size == 64
    got, = E.evaluate([E.unary(op, E.value("a", 0))], lambda addr, e: v)
    np.testing.assert_allclose(got, SCIPY[op](v), rtol=1e-12, atol=0)
    assert E.unary(op, E.const(v[3])) == E.const(float(SCIPY[op](v[3]))) or E.unary(op, E.const(v[3]))[1] == pytest.approx(float(SCIPY[op](v[3])), rel=1e-12)


def test_evaluate_logsumexp_against_scipy():
    rows = np.random.default_rng(3).uniform(-30.0, 30.0, (62, 5))
    rows = np.concatenate([rows, np.full((1, 5), -np.inf), [[-3.0, 700.0, 1.0, -np.inf, 0.5]]])
    got, = E.evaluate([E.lse([E.value("x", i) for i in range(5)])], lambda addr, e: rows[:, e])
    want = sp.logsumexp(rows, axis=1)
    assert got.shape == (64,) and got[62] == -np.inf and not np.isnan(got).any()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


def test_a_return_value_through_the_torch_path():
    import torch

    @genjax.gen
    def model():
        a = genjax.normal(0.0, 1.0) @ "a"
        x = genjax.mv_normal_diag(np.zeros(DIM, np.float32), np.ones(DIM, np.float32)) @ "x"
        return genjax.erf(a) + x.max()

    _, ret = model.site_list(())
    rs = np.random.default_rng(5)
    a, x = rs.standard_normal(33), rs.standard_normal((DIM, 33))
    leaf = lambda addr, e: torch.as_tensor(a if addr == "a" else x[e], dtype=torch.float32)       # noqa: E731
    got, = E.evaluate(ret.elems, leaf, xp=torch)
    assert isinstance(got, torch.Tensor) and got.device.type == "cpu"
    np.testing.assert_allclose(got.numpy(), sp.erf(a) + x.max(axis=0), rtol=1e-6)
    # every new op, and logsumexp, on tensors
    for op in POINTS:
        got, = E.evaluate([E.unary(op, E.value("a", 0))], lambda addr, e: torch.as_tensor(POINTS[op]), xp=torch)
        np.testing.assert_allclose(got.numpy(), SCIPY[op](POINTS[op]), rtol=1e-6, atol=1e-12)
    got, = E.evaluate([E.lse([E.value("x", i) for i in range(DIM)] + [E.const(0.5)])], lambda addr, e: torch.as_tensor(x[e]), xp=torch)
    np.testing.assert_allclose(got.numpy(), sp.logsumexp(np.concatenate([x, np.full((1, 33), 0.5)]), axis=0), rtol=1e-12)


@pytest.mark.parametrize("body", [
    lambda a, b, x: x.sum(keepdims=True), lambda a, b, x: np.sum(x, keepdims=True), lambda a, b, x: x.sum(axis=1), lambda a, b, x: np.max(x, axis=1),
    lambda a, b, x: np.add.accumulate(x), lambda a, b, x: np.arctan(a), lambda a, b, x: genjax.logsumexp(x, axis=1),
    lambda a, b, x: np.multiply.reduce(x), lambda a, b, x: np.linalg.norm(x)],
    # names, not str(): a lambda's repr holds its address, which differs from run to run
    ids=["method_sum_keepdims", "np_sum_keepdims", "method_sum_axis1", "np_max_axis1", "add_accumulate", "arctan", "logsumexp_axis1",
         "multiply_reduce", "linalg_norm"])
def test_what_is_not_supported_says_so(body):
    with pytest.raises(genjax.NotSupportedInModelBody):
        _model(body).site_list(())


def test_the_message_names_the_ufunc():
    with pytest.raises(genjax.NotSupportedInModelBody, match="arctan"):
        _model(lambda a, b, x: np.arctan(a)).site_list(())
    with pytest.raises(genjax.NotSupportedInModelBody, match="add.accumulate"):
        _model(lambda a, b, x: np.add.accumulate(x)).site_list(())


def test_an_array_on_the_left_gives_what_the_reflected_operator_gives():
    W3 = np.random.default_rng(1).standard_normal((3, DIM))
    pairs = [
        (lambda a, b, x: np.float32(2) * a, lambda a, b, x: a * 2),
        (lambda a, b, x: (np.ones(DIM) - x)[1], lambda a, b, x: (-(x - 1))[1]),
        (lambda a, b, x: (W3 @ x)[2], lambda a, b, x: x.__rmatmul__(W3)[2]),
        (lambda a, b, x: (np.arange(DIM) + x)[3], lambda a, b, x: x.__radd__(np.arange(DIM))[3]),
        (lambda a, b, x: (np.full(DIM, 3.0) / x)[0], lambda a, b, x: x.__rtruediv__(np.full(DIM, 3.0))[0]),
        (lambda a, b, x: np.multiply(np.arange(1.0, DIM + 1), x)[2], lambda a, b, x: (x * np.arange(1.0, DIM + 1))[2]),
        (lambda a, b, x: np.where(np.float64(0.5) > a, a, b * b), lambda a, b, x: genjax.where(a < 0.5, a, b * b)),
    ]
    for left, right in pairs:
        _same(_param(left), _param(right))
    # whole vectors: the same Param for the 4-vector mean of a vector site
    @genjax.gen
    def m1():
        x = genjax.mv_normal_diag(np.zeros(DIM, np.float32), np.ones(DIM, np.float32)) @ "x"
        genjax.mv_normal_diag(np.ones(DIM) - x, np.ones(DIM, np.float32)) @ "y"
        genjax.mv_normal_diag(W3 @ x, np.ones(3, np.float32)) @ "z"

    @genjax.gen
    def m2():
        x = genjax.mv_normal_diag(np.zeros(DIM, np.float32), np.ones(DIM, np.float32)) @ "x"
        genjax.mv_normal_diag(-(x - 1), np.ones(DIM, np.float32)) @ "y"
        genjax.mv_normal_diag(x.__rmatmul__(W3), np.ones(3, np.float32)) @ "z"

    s1, s2 = m1.site_list(())[0], m2.site_list(())[0]
    for addr in ("y", "z"):
        _same(s1[addr].params[0], s2[addr].params[0])
