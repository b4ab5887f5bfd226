"""The tracer's new surface on the device: erf / erfc / lgamma / expm1 nodes, the n-ary log-sum-exp node (GJX_E_LSEN) and the
reductions, on the generated kernels (nodes emitted inline; reverse sweep emitted inline for HMC) and on the site interpreter.

The reference is a float64 restatement of every model written here with NumPy and scipy.special — the CPU oracle does not know the
new node ops, so no program of this file is handed to it.  Inputs are host-made grids supplied as the values of constrained sites
(no sampler is involved), K = 4099 columns (neither a multiple of the wave nor of the block); NO grid point is excluded: the grids
are chosen so that the reference itself is well conditioned, which `_well_conditioned` asserts (the float64 scores under inputs
scaled by 1 + 2e-6 — a few float32 ulps — move by less than half the tolerance at every point).
Tolerances: scores rtol 2e-4 / atol 2e-4, gradients rtol 2e-3 / atol 2e-3 against central differences (step 1e-5) of the float64
restatement, one HMC move (eps 2e-3, L 8) rtol 3e-3 / atol 3e-3 between the engines — what tests/test_gpu_expr.py uses."""
import math
import os
import sys

import numpy as np
import pytest
import scipy.special as sp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import genjax_amd as genjax               # noqa: E402
from genjax_amd import C                  # noqa: E402
from genjax_amd import _abi as A          # noqa: E402
from genjax_amd.program import PackedProgram      # noqa: E402
from helpers import GRID_AT as AT, GRID_K as K, GRID_N_GRAD as N_GRAD, GRID_RT as RT      # noqa: E402
from helpers import float32_range as _float32_range, grid_offsets as _offsets, grid_rows as _rows, nlp, well_conditioned as _well_conditioned      # noqa: E402


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def K_():
    from genjax_amd import kernels
    return kernels


# ---- the models: (the @gen function, its sites in order with their dims, the float64 restatement of the per-site scores, a grid) ----
UNARY = {"erf": (genjax.erf, sp.erf), "erfc": (genjax.erfc, sp.erfc), "lgamma": (genjax.lgamma, sp.gammaln), "expm1": (genjax.expm1, sp.expm1)}


def _unary_model(name):
    f = UNARY[name][0]

    @genjax.gen
    def model():
        a = genjax.normal(0.0, 2.0) @ "a"
        genjax.normal(f(a), 1.0) @ "y"
    return model


def _unary_arguments(name, n):
    if name != "lgamma":
        return np.linspace(-3.0, 3.0, n)
    # [0.2, 8] and negative non-integers at least 0.2 (and a little more: the float32 rounding of the grid) away from an integer
    pos = np.linspace(0.2, 8.0, n - n // 2)
    u = np.linspace(0.0, 1.0, n // 2, endpoint=False)
    neg = -(np.floor(u * 5.0) + 0.21 + 0.58 * ((u * 5.0) % 1.0))
    return np.concatenate([pos, neg])


def _unary_spec(name):
    ref = UNARY[name][1]

    def grid(n):
        a = _unary_arguments(name, n).astype(np.float32)
        return {"a": a[None], "y": (ref(a.astype(np.float64)) + _offsets(n)).astype(np.float32)[None]}

    def scores(v):
        return [nlp(v["a"][0], 0.0, 2.0), nlp(v["y"][0], ref(v["a"][0]), 1.0)]
    return dict(model=_unary_model(name), sites=[("a", 1), ("y", 1)], grid=grid, scores=scores, obs={"y": 0.7}, grad_grid=grid)


LW = np.linspace(-1.0, 1.0, 8)


@genjax.gen
def lse_model():
    a = genjax.normal(0.0, 1.0) @ "a"
    b = genjax.normal(1.0, 1.0) @ "b"
    x = genjax.mv_normal_diag(np.zeros(8, np.float32), np.ones(8, np.float32)) @ "x"
    genjax.normal(genjax.logsumexp(LW + b * x), 1.0) @ "y"
    genjax.normal(np.logaddexp(a, b), 1.0) @ "z"            # (the two-operand form, through the NumPy ufunc)


def _lse_grid(n, x_max=14.0, extreme=True):
    rs = np.random.default_rng(11)
    a = rs.uniform(-3.0, 3.0, n)
    b = rs.uniform(0.5, 2.0, n)
    x = rs.uniform(-x_max, x_max, (8, n))            # |lw + b x| <= 1 + 2 * 14 < 30
    x[:, 1] = x[0, 1]                                # a column of equal operands, and one dominated by a single operand
    x[:, 2] = -x_max
    x[3, 2] = x_max
    a, b, x = a.astype(np.float32), b.astype(np.float32), x.astype(np.float32)
    if extreme:                                      # every operand at -1e30: the result is -1e30, not NaN; the scores of x and of y
        b[0] = 1.0
        x[:, 0] = -1e30                              # are then beyond float32 (-inf on the device, see _float32_range); z's is ordinary
    m = sp.logsumexp(LW[:, None] + b.astype(np.float64) * x.astype(np.float64), axis=0)
    y = (m + _offsets(n)).astype(np.float32)
    if extreme:
        y[0] = 0.3
    z = (np.logaddexp(a.astype(np.float64), b.astype(np.float64)) + _offsets(n)[::-1]).astype(np.float32)
    return {"a": a[None], "b": b[None], "x": x, "y": y[None], "z": z[None]}


def _lse_scores(v):
    m = sp.logsumexp(LW[:, None] + v["b"][0] * v["x"], axis=0)
    return [nlp(v["a"][0], 0.0, 1.0), nlp(v["b"][0], 1.0, 1.0), nlp(v["x"], 0.0, 1.0).sum(0), nlp(v["y"][0], m, 1.0),
            nlp(v["z"][0], np.logaddexp(v["a"][0], v["b"][0]), 1.0)]


@genjax.gen
def reduce_model():
    x = genjax.mv_normal_diag(np.zeros(4, np.float32), np.ones(4, np.float32)) @ "x"
    genjax.normal(x.max(), genjax.exp(x).sum()) @ "y"
    genjax.normal(0.5, (x * x).prod()) @ "z"


def _reduce_grid(n):
    rs = np.random.default_rng(12)
    x = (rs.uniform(0.6, 1.6, (4, n)) * rs.choice([-1.0, 1.0], (4, n))).astype(np.float32)       # away from 0: the product is a scale
    x64 = x.astype(np.float64)
    y = x64.max(0) + np.exp(x64).sum(0) * _offsets(n)
    z = 0.5 + (x64 * x64).prod(0) * _offsets(n)[::-1]
    return {"x": x, "y": y.astype(np.float32)[None], "z": z.astype(np.float32)[None]}


def _reduce_scores(v):
    x = v["x"]
    return [nlp(x, 0.0, 1.0).sum(0), nlp(v["y"][0], x.max(0), np.exp(x).sum(0)), nlp(v["z"][0], 0.5, (x * x).prod(0))]


SPECS = {name: _unary_spec(name) for name in UNARY}
SPECS["logsumexp"] = dict(model=lse_model, sites=[("a", 1), ("b", 1), ("x", 8), ("y", 1), ("z", 1)], grid=_lse_grid, scores=_lse_scores,
                          obs={"y": 0.3, "z": 0.9}, grad_grid=lambda n: _lse_grid(n, x_max=3.0, extreme=False))
SPECS["reductions"] = dict(model=reduce_model, sites=[("x", 4), ("y", 1), ("z", 1)], grid=_reduce_grid, scores=_reduce_scores,
                           obs={"y": 2.0, "z": 0.8}, grad_grid=_reduce_grid)


@pytest.mark.parametrize("which", list(SPECS))
def test_scores_on_the_generated_kernel_and_the_interpreter(K_, which, monkeypatch):
    import torch
    spec = SPECS[which]
    sl, _ = spec["model"].site_list(())
    assert [s.addr for s in sl.sites] == [a for a, _ in spec["sites"]]
    prog = PackedProgram(sl, {s.addr: A.MODE_OBS_SLOT for s in sl.sites})
    assert any(prog.c_sites[j].p[k].op == A.P_EXPR for j in range(prog.n_sites) for k in range(A.MAX_PARAMS))
    vals = spec["grid"](K)
    want = _well_conditioned(spec, vals)                     # [n_sites][K], every point kept
    assert want.shape == (prog.n_sites, K)
    ch = torch.as_tensor(_rows(prog, spec, vals)).cuda()
    for eng in (None, "interp"):
        if eng is None:
            monkeypatch.delenv("GJX_ENGINE", raising=False)
            assert K_.program_engine(prog) == 4, "the emitter must take the new node ops"
        else:
            monkeypatch.setenv("GJX_ENGINE", eng)
            assert K_.program_engine(prog) == 0
        g = K_.run_program(prog, (3, 7), K, choices=ch.clone(), want_site_scores=True)
        ss, sc = _np(g["site_scores"]).astype(np.float64), _np(g["score"]).astype(np.float64)
        with np.errstate(invalid="ignore"):
            w32 = _float32_range(want)
            print(f"{which} {eng or 'gen'}: max |site score error| / (atol + rtol |ref|) = {np.nanmax(np.abs(ss - w32) / (AT + RT * np.abs(w32))):.2e}")
        assert not np.isnan(ss).any() and not np.isnan(sc).any()
        np.testing.assert_allclose(ss, _float32_range(want), rtol=RT, atol=AT, err_msg=f"{which} {eng}")
        np.testing.assert_allclose(sc, _float32_range(want.sum(0)), rtol=RT, atol=AT, err_msg=f"{which} {eng}")


@pytest.mark.parametrize("which", list(SPECS))
def test_gradients_and_one_hmc_move(K_, which, monkeypatch):
    """gjx_score_grad (the interpreter's reverse sweep) against central differences of the float64 restatement; then one HMC move on
    the generated HMC kernel (reverse sweep emitted inline) and on the interpreter: the same trajectory"""
    import torch
    spec = SPECS[which]
    sl, _ = spec["model"].site_list(())
    obs = {a: np.float32(v) for a, v in spec["obs"].items()}
    sel = tuple(a for a, _ in spec["sites"] if a not in obs)
    modes = {a: (A.MODE_OBS_TAB if a in obs else A.MODE_OBS_SLOT) for a, _ in spec["sites"]}
    prog = PackedProgram(sl, modes, obs, selected=sel)
    vals = {k: v for k, v in spec["grad_grid"](N_GRAD).items() if k not in obs}
    if which == "lgamma":
        assert (vals["a"] < 0).sum() > 100                    # negative arguments: the reflected digamma
    ch = _rows(prog, spec, vals)

    def total(rows):
        v = {a: rows[prog.slot_of[a]:prog.slot_of[a] + d] for a, d in spec["sites"] if a not in obs}
        v.update({a: np.full((1, rows.shape[1]), float(x)) for a, x in obs.items()})
        return np.sum(spec["scores"](v), axis=0)

    c64 = ch.astype(np.float64)
    fd = np.zeros_like(c64)
    h = 1e-5
    for r in range(c64.shape[0]):
        up, dn = c64.copy(), c64.copy()
        up[r] += h
        dn[r] -= h
        fd[r] = (total(up) - total(dn)) / (2 * h)
    sg, gg = K_.score_grad(prog, torch.as_tensor(ch).cuda())
    print(f"{which}: max |gradient error| / (atol + rtol |ref|) = {(np.abs(_np(gg) - fd) / (2e-3 + 2e-3 * np.abs(fd))).max():.2e}, max |ref| = {np.abs(fd).max():.3g}")
    np.testing.assert_allclose(_np(sg), total(c64), rtol=RT, atol=AT)
    np.testing.assert_allclose(_np(gg), fd, rtol=2e-3, atol=2e-3)
    moved = {}
    for eng in ("gen", "interp"):
        monkeypatch.setenv("GJX_HMC_ENGINE", eng)
        assert K_.hmc_engine(prog) == (4 if eng == "gen" else 0), eng
        g = K_.hmc(prog, (2, 9), torch.as_tensor(ch).cuda(), 2e-3, 8, False, False, offset=5)
        moved[eng] = _np(g["choices"])
        assert np.isfinite(moved[eng]).all() and np.abs(moved[eng] - ch).max() > 1e-3
    np.testing.assert_allclose(moved["gen"], moved["interp"], rtol=3e-3, atol=3e-3)


T_SCAN = 64


def _lse_scan():
    @genjax.gen
    def step(x_prev, _):
        x = genjax.normal(genjax.logsumexp([0.9 * x_prev, -0.5 * x_prev]) - 0.6, 0.5) @ "x"
        genjax.normal(x, genjax.expm1(0.5 + 0.1 * x * x)) @ "y"
        return x, None
    return step.scan(n=T_SCAN)


def test_a_scan_with_the_new_ops_is_rolled(K_, monkeypatch):
    """a periodic Scan whose transition mean is a log-sum-exp of two expressions of the carry and whose observation scale is an expm1:
    the propagate emitter rolls it (the LSEN node has no table entries: nothing strides); generated == interpreter, and the scores
    of the device's own draws == the float64 restatement"""
    rs = np.random.default_rng(2)
    ys = rs.standard_normal(T_SCAN).astype(np.float32)
    prog, _, _ = _lse_scan().pack((np.float32(0.1), None), C["y"].set(ys), True, rng_mode=A.RNG_FLAT)
    assert prog.n_sites == 2 * T_SCAN
    monkeypatch.delenv("GJX_ENGINE", raising=False)
    assert K_.program_engine(prog) == 4, "a periodic Scan with LSEN / EXPM1 nodes must roll onto a generated kernel"
    out = {}
    for eng in ("gen", "interp"):
        monkeypatch.setenv("GJX_ENGINE", eng)
        assert K_.program_engine(prog) == (4 if eng == "gen" else 0)
        g = K_.run_program(prog, (8, 9), K)
        out[eng] = {k: _np(g[k]).astype(np.float64) for k in ("choices", "score", "logw")}
    for k in ("choices", "score", "logw"):
        np.testing.assert_allclose(out["gen"][k], out["interp"][k], rtol=RT, atol=AT, err_msg=k)
    for eng in ("gen", "interp"):
        x = np.stack([out[eng]["choices"][prog.slot_of[("x", t)]] for t in range(T_SCAN)])
        prev = np.concatenate([np.full((1, K), np.float64(np.float32(0.1))), x[:-1]])
        prior = nlp(x, np.logaddexp(0.9 * prev, -0.5 * prev) - 0.6, 0.5).sum(0)
        lik = nlp(ys[:, None].astype(np.float64), x, np.expm1(0.5 + 0.1 * x * x)).sum(0)
        np.testing.assert_allclose(out[eng]["logw"], lik, rtol=RT, atol=AT, err_msg=eng)
        np.testing.assert_allclose(out[eng]["score"], lik + prior, rtol=RT, atol=AT, err_msg=eng)


def test_a_plate_whose_mean_is_an_erf(K_, monkeypatch):
    """y_i ~ normal(erf(w . x_i), 1) vmapped over 16 observations: ONE plate site, on a generated kernel, against float64"""
    import torch
    rs = np.random.default_rng(4)
    X = rs.standard_normal((16, 3)).astype(np.float32)
    Y = rs.standard_normal(16).astype(np.float32)

    @genjax.gen
    def kern(x_row, w):
        return genjax.normal(genjax.erf(genjax.dot(w, x_row)), 1.0) @ "y"

    @genjax.gen
    def model():
        w = genjax.normal(np.zeros(3, np.float32), 1.0) @ "w"
        kern.vmap(in_axes=(0, None))(X, w) @ "obs"

    prog, _, _ = model.pack((), C["obs", "y"].set(Y), False, per_particle=("w",), rng_mode=A.RNG_FLAT)
    assert prog.n_sites == 2 and prog.c_sites[1].plate_n == 16 and prog.c_sites[1].p[0].op == A.P_EXPR          # (no IrregularPlate: not unrolled)
    w = np.random.default_rng(5).uniform(-1.5, 1.5, (3, K)).astype(np.float32)
    w64 = w.astype(np.float64)

    def scores(w_, s=1.0):
        return np.stack([nlp(w_, 0.0, 1.0).sum(0), nlp(Y[:, None].astype(np.float64) * s, sp.erf(X.astype(np.float64) @ w_), 1.0).sum(0)])
    want = scores(w64)
    assert (np.abs(scores(w64 * (1 + 2e-6), 1 + 2e-6) - want) < 0.5 * (AT + RT * np.abs(want))).all()
    ch = np.zeros((prog.n_slots, K), np.float32)
    ch[prog.slot_of["w"]:prog.slot_of["w"] + 3] = w
    for eng in (None, "interp"):
        if eng is None:
            monkeypatch.delenv("GJX_ENGINE", raising=False)
            assert K_.program_engine(prog) == 4
        else:
            monkeypatch.setenv("GJX_ENGINE", eng)
        g = K_.run_program(prog, (4, 5), K, choices=torch.as_tensor(ch).cuda(), want_site_scores=True)
        np.testing.assert_allclose(_np(g["site_scores"]), want, rtol=RT, atol=AT, err_msg=str(eng))
        np.testing.assert_allclose(_np(g["score"]), want.sum(0), rtol=RT, atol=AT, err_msg=str(eng))


def test_the_erf_model_through_the_api(K_):
    """Target / ImportanceK end to end: the log-ML estimate against a 1-D numerical integration"""
    from genjax_amd.inference import ImportanceK, Target
    y = 0.3
    est = float(ImportanceK(Target(SPECS["erf"]["model"], (), C["y"].set(y)), k_particles=1 << 16).log_marginal_likelihood_estimate(genjax.key(5)))
    g = np.linspace(-16.0, 16.0, 4001)
    exact = math.log(np.exp(nlp(g, 0.0, 2.0) + nlp(y, sp.erf(g), 1.0)).sum() * (g[1] - g[0]))
    assert est == pytest.approx(exact, abs=0.02)
