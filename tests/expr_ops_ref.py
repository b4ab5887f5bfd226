"""The expression node ops (include/gjx.h GJX_E_CONST .. GJX_E_LSEN) at their edges — the 25 older ones in programs 1 to 5, erf, erfc,
lgamma, expm1, log-sum-exp and the reductions in programs 6 to 8: the programs, their grids and a
float64 NumPy / scipy.special restatement, shared by tests/test_gpu_expr_ops.py (generated kernels, site interpreter) and tests/test_expr_ops_cpu.py
(the CPU oracle, expr.evaluate).

A program is a list of scalar latents a ~ normal(0, sd) (or one 64-vector) and a list of OP SITES, one per op and edge family:
    "mean"   y ~ normal(f(latents), 1)    where |f| stays below about 30 (the score moves with the ABSOLUTE error of f)
    "scale"  y ~ normal(0, f(latents))    where f is positive and spans decades (the score moves with log f: the RELATIVE error)
Every site is constrained per column, so no sampler is involved.  The reference `ref(v, d)` of an op site is float64 NumPy; `v` holds
the values, `d` the values that DECIDE (comparisons, selections, the sign of abs): d = v everywhere except under finite differences,
where d stays at the base point — central differences of that function are the analytic gradient under the rule of include/gjx.h
(MAX / MIN to a at a tie, abs'(0) = 0, no gradient through GT, WHERE to the selected branch only, nothing from a zero adjoint).
A value beyond float32's range is compared as the infinity the device must return (helpers.float32_range).

Domain (include/gjx.h): float32's normal range.  Two edges are therefore placed with care, and neither is dropped after the fact:
  * sin / cos: the grid stops at |x| = 50.  The conditioning check moves the inputs by 2e-6 RELATIVE, which at |x| = 1e4 moves the
    argument by 0.02 — the reference itself is then not conditioned at the tolerance; multiples of pi / 2 (rounded to float32) are in.
  * log1p at -1 + 2^-20: relative to the argument this point is ill conditioned (1 + x moves by twice its size), so the node is
    reached as log1p(u - 1) with u = 2^-20 — the node's argument is exactly -1 + 2^-20 and the reference is conditioned in u.
"""
import numpy as np

import genjax_amd as genjax
from genjax_amd import _abi as A
from genjax_amd.program import PackedProgram
from helpers import float32_range, grid_offsets, nlp

F32 = np.float32
C1M3 = float(F32(1e-3))               # the guard constant as the device holds it


def _e(a):
    """a latent as a GENERAL expression (max(a, a) folds to the VALUE leaf): transforms of it are nodes, not the closed GJX_XF_* forms"""
    return genjax.maximum(a, a)


def _fill(edges, dense_lo, dense_hi, n, log=False, both_signs=False, seed=0):
    """edges first, then a dense part filling up to n columns (shuffled deterministically so that no block sees one regime only)"""
    edges = np.asarray(edges, np.float64)
    m = n - len(edges)
    assert m > 0
    dense = np.geomspace(dense_lo, dense_hi, m) if log else np.linspace(dense_lo, dense_hi, m)
    if both_signs:
        dense = dense * np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
    x = np.concatenate([edges, dense])
    return x[np.random.default_rng(seed).permutation(n)].astype(F32)


def _ulp_up(x):
    return np.nextafter(F32(x), F32(np.inf))


POW2 = lambda ks: np.concatenate([[2.0 ** -k, -2.0 ** -k] for k in ks])        # noqa: E731


class Spec(dict):
    """dict(model, sites, grid, grad_grid, scores, values, latents, opsites, ops): what the harness of helpers.py expects, built
    from the latents [(addr, sd) | (addr, sd, dim)] and the op sites [(name, place, build(L) -> Sym, ref(v, d) -> float64[n])]"""

    def __init__(self, latents, opsites, grid, grad_grid, ops):
        latents = [(t + (1,))[:3] for t in latents]

        @genjax.gen
        def model():
            L = {}
            for addr, sd, dim in latents:
                L[addr] = (genjax.normal(0.0, sd) if dim == 1 else genjax.mv_normal_diag(np.zeros(dim, F32), np.full(dim, sd, F32))) @ addr
            for name, place, build, _ in opsites:
                f = build(L)
                (genjax.normal(f, 1.0) if place == "mean" else genjax.normal(0.0, f)) @ name

        def values(v, d=None):
            """float64 value of every op site's expression, as the device can hold it"""
            d = v if d is None else d
            with np.errstate(all="ignore"):
                return {name: float32_range(np.asarray(ref(v, d), np.float64)) for name, _, _, ref in opsites}

        def scores(v, d=None):
            f = values(v, d)
            with np.errstate(all="ignore"):
                out = [nlp(v[a], 0.0, sd).sum(0) for a, sd, _ in latents]
                out += [nlp(v[name][0], f[name], 1.0) if place == "mean" else nlp(v[name][0], 0.0, f[name]) for name, place, _, _ in opsites]
            return out

        def finish(lat32, n):
            """the observations: a mean site's sits within 1.5 sd of f (of 0 where f is not finite); a scale site's at f * offset where
            1e-30 <= f <= 1e30 (else at 0: the quotient y / f would leave float32's normal range)"""
            v = {a: np.atleast_2d(x).astype(np.float64) for a, x in lat32.items()}
            f = values(v)
            off = grid_offsets(n)
            out = {a: np.atleast_2d(x).astype(F32) for a, x in lat32.items()}
            for i, (name, place, _, _) in enumerate(opsites):
                fi = np.broadcast_to(f[name], (n,))
                o = np.roll(off, 7 * i)
                if place == "mean":
                    y = np.where(np.isfinite(fi), fi, 0.0) + o
                else:
                    with np.errstate(invalid="ignore"):
                        y = np.where((fi >= 1e-30) & (fi <= 1e30), fi * o, 0.0)
                out[name] = y.astype(F32)[None]
            return out

        super().__init__(model=model, sites=[(a, dim) for a, _, dim in latents] + [(name, 1) for name, _, _, _ in opsites],
                         grid=lambda n: finish(grid(n), n), grad_grid=lambda n: finish(grad_grid(n), n), scores=scores, values=values,
                         latents=latents, opsites=opsites, ops=set(ops))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. unary ops
# ---------------------------------------------------------------------------------------------------------------------------------
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


BIG = [10.0, 20.0, 50.0, 90.0, 200.0]
HALF_PI = [float(F32(k * np.pi / 2)) for k in range(-8, 9)]
UN_LAT = [("xem", 100.0), ("xes", 100.0), ("xl", 1e20), ("xqs", 1e20), ("xqm", 1000.0), ("xsq", 10.0), ("xss", 1e20), ("xt", 100.0),
          ("xa", 10.0), ("xsc", 100.0), ("xp", 10.0), ("xu", 10.0), ("xrs", 1e20), ("sr", 10.0), ("xrm", 1e20), ("xth", 1e20), ("xsg", 1e20)]


SAT = BIG + [-b for b in BIG]          # tanh / sigmoid / softplus far out: the float64 derivative rounds to 0 from about 20 on


def _signed(g):
    """the sign row of the reciprocal's argument (unselected): 1 / x times it is a positive scale on either side of 0"""
    g["sr"] = np.sign(g["xrs"]).astype(F32)
    return g


def _un_grid(n):
    return _signed(dict(
        xem=_fill([-100.0, -88.0, -87.4, 0.0], -100.0, 3.0, n, seed=1),                                   # exp as a mean: underflows to 0
        xes=_fill([89.0, 88.0, 87.0, -69.0], -69.0, 88.0, n, seed=2),                                      # as a scale: to 1e38; 89: +inf
        xl=_fill(np.concatenate([[0.0, 1.0], 1.0 + POW2(range(4, 21))]), 1e-30, 1e30, n, log=True, seed=3),   # log: the cluster at 1, log 0
        xqs=_fill([1e-30, 1e30, 1.0], 1e-30, 1e30, n, log=True, seed=4),                                   # sqrt as a scale
        xqm=_fill([0.0, 1e-30, 1e-12], 0.0, 900.0, n, seed=5),                                             # sqrt as a mean, 0 included
        xsq=_fill([0.0, 1e-19, -1e-19, 1e-10, -1e-10], -5.0, 5.0, n, seed=6),                              # square as a mean, down to 1e-19
        xss=_fill([2e19, -2e19, 1e19, -1e19, 1e-15], 1e-15, 1e19, n, log=True, both_signs=True, seed=7),   # as a scale: to 1e38; 2e19: +inf
        xt=_fill(np.concatenate([POW2(range(4, 21)), BIG, [-b for b in BIG], [0.0]]), -8.0, 8.0, n, seed=8),   # tanh / sigmoid / softplus
        xa=_fill([0.0, -0.0, 1e-30, -1e-30], -5.0, 5.0, n, seed=9),                                        # abs / neg
        xsc=_fill(HALF_PI + [0.0, 50.0, -50.0], -50.0, 50.0, n, seed=10),                                  # sin / cos
        xp=_fill(np.concatenate([POW2(range(3, 25)), [-1.0 + 2.0 ** -k for k in range(1, 6)]]), -0.9, 5.0, n, seed=11),   # log1p: across 2^-6
        xu=_fill([2.0 ** -20, 2.0 ** -10, 1.0], 0.01, 3.0, n, seed=12),                                    # log1p(u - 1): argument -1 + 2^-20
        xrs=_fill([1e-30, -1e-30, 1e30, -1e30, 1.0, -1.0], 1e-30, 1e30, n, log=True, both_signs=True, seed=13),   # recip as a scale: +-(1e-30 .. 1e30)
        xth=_fill(SAT + [0.0], -8.0, 8.0, n, seed=15), xsg=_fill(SAT + [0.0], -8.0, 8.0, n, seed=16),      # tanh / sigmoid ALONE on a latent
        xrm=_fill([0.0, -0.0, 1e30, -1e30, 1.0 / 16, -1.0 / 16], 1.0 / 16, 1e30, n, log=True, both_signs=True, seed=14)))   # as a mean; +-0: +-inf


def _un_grad_grid(n):
    u = lambda lo, hi, s, edges=(): _fill(list(edges), lo, hi, n, seed=100 + s)          # noqa: E731
    return _signed(dict(xem=u(-3.0, 2.0, 1), xes=u(-2.0, 2.0, 2), xl=u(0.3, 6.0, 3), xqs=u(0.3, 6.0, 4), xqm=u(0.3, 9.0, 5), xsq=u(-3.0, 3.0, 6, [0.0]),
                xss=u(0.5, 2.5, 7), xt=u(-6.0, 6.0, 8, [0.0] + SAT), xa=u(-3.0, 3.0, 9, [0.0, -0.0]),
                xsc=u(-6.0, 6.0, 10, HALF_PI[4:13]), xp=u(-0.7, 4.0, 11, [0.0, 2.0 ** -6, -2.0 ** -6, 2.0 ** -7]), xu=u(0.3, 3.0, 12),
                xrs=_fill([], 0.4, 3.0, n, both_signs=True, seed=113), xrm=_fill([], 0.3, 4.0, n, both_signs=True, seed=114),
                xth=u(-6.0, 6.0, 15, [0.0] + SAT), xsg=u(-6.0, 6.0, 16, [0.0] + SAT)))


UN_SITES = [
    ("exp_m", "mean", lambda L: genjax.exp(_e(L["xem"])), lambda v, d: np.exp(v["xem"][0])),
    ("exp_s", "scale", lambda L: genjax.exp(_e(L["xes"])), lambda v, d: np.exp(v["xes"][0])),
    ("log_m", "mean", lambda L: genjax.log(L["xl"]), lambda v, d: np.log(v["xl"][0])),
    ("sqrt_s", "scale", lambda L: genjax.sqrt(L["xqs"]), lambda v, d: np.sqrt(v["xqs"][0])),
    ("sqrt_m", "mean", lambda L: genjax.sqrt(L["xqm"]), lambda v, d: np.sqrt(v["xqm"][0])),
    ("square_m", "mean", lambda L: genjax.square(L["xsq"]), lambda v, d: v["xsq"][0] ** 2),
    ("square_s", "scale", lambda L: genjax.square(L["xss"]), lambda v, d: v["xss"][0] ** 2),
    ("tanh", "mean", lambda L: genjax.tanh(L["xt"]), lambda v, d: np.tanh(v["xt"][0])),
    ("sigmoid", "mean", lambda L: genjax.sigmoid(_e(L["xt"])), lambda v, d: _sigmoid(v["xt"][0])),
    ("softplus", "mean", lambda L: genjax.softplus(_e(L["xt"])), lambda v, d: np.logaddexp(0.0, v["xt"][0])),
    ("abs", "mean", lambda L: genjax.abs(L["xa"]), lambda v, d: np.sign(d["xa"][0]) * v["xa"][0]),
    ("neg", "mean", lambda L: -genjax.abs(L["xa"]), lambda v, d: -np.sign(d["xa"][0]) * v["xa"][0]),
    ("sin", "mean", lambda L: genjax.sin(L["xsc"]), lambda v, d: np.sin(v["xsc"][0])),
    ("cos", "mean", lambda L: genjax.cos(L["xsc"]), lambda v, d: np.cos(v["xsc"][0])),
    ("log1p", "mean", lambda L: genjax.log1p(L["xp"]), lambda v, d: np.log1p(v["xp"][0])),
    ("log1p_shift", "mean", lambda L: genjax.log1p(L["xu"] - 1.0), lambda v, d: np.log(v["xu"][0])),
    ("recip_s", "scale", lambda L: (_e(L["xrs"]) ** -1) * L["sr"], lambda v, d: 1.0 / v["xrs"][0] * v["sr"][0]),      # (a wrong sign: a negative scale, NaN)
    ("tanh_only", "mean", lambda L: genjax.tanh(L["xth"]), lambda v, d: np.tanh(v["xth"][0])),
    ("sigmoid_only", "mean", lambda L: genjax.sigmoid(_e(L["xsg"])), lambda v, d: _sigmoid(v["xsg"][0])),
    ("recip_m", "mean", lambda L: _e(L["xrm"]) ** -1, lambda v, d: 1.0 / v["xrm"][0]),
    ("recip_sign", "mean", lambda L: genjax.tanh(_e(L["xrm"]) ** -1), lambda v, d: np.tanh(1.0 / v["xrm"][0])),      # the SIGN of 1 / +-0
]
UN_OPS = [A.E_VALUE, A.E_NEG, A.E_EXP, A.E_LOG, A.E_SQRT, A.E_SQUARE, A.E_TANH, A.E_SIGMOID, A.E_SOFTPLUS, A.E_ABS, A.E_SIN, A.E_COS,
          A.E_LOG1P, A.E_RECIP, A.E_LINV]


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. binary ops, compare and select
# ---------------------------------------------------------------------------------------------------------------------------------
BIN_LAT = [("a", 10.0), ("b", 10.0), ("p", 1e20), ("q", 1e20), ("sq", 10.0), ("n", 10.0), ("m", 1e20), ("c", 10.0)]


def _bin_grid(n, edges=True):
    rs = np.random.default_rng(21)
    a = (rs.uniform(0.3, 3.0, n) * rs.choice([-1.0, 1.0], n)).astype(F32)
    b = (rs.uniform(0.3, 3.0, n) * rs.choice([-1.0, 1.0], n)).astype(F32)
    b[0:40] = a[0:40]                                            # exact ties
    b[40:60] = _ulp_up(a[40:60])                                 # operands one ulp apart, either way
    a[60:80] = _ulp_up(b[60:80])
    a[80:84], b[80:84] = [0.0, -0.0, 0.0, -0.0], [0.0, 0.0, -0.0, -0.0]        # +-0 against +-0 (they tie)
    a[84:88], b[84:88] = [0.0, -0.0, 0.0, -0.0], [1.5, 1.5, -1.5, -1.5]
    # MUL / DIV over the decades: p * q and p / q stay within 1e-30 .. 1e30 in the dense part
    lp = rs.uniform(-15.0, 15.0, n)
    lq = rs.uniform(-15.0, 15.0, n)
    p, q = (10.0 ** lp).astype(F32), (10.0 ** lq * rs.choice([-1.0, 1.0], n)).astype(F32)        # q of either sign: +-(1e-15 .. 1e15)
    # DIV as a mean: numerator n, denominator m = +-(1/8 .. 1e30)
    nn = (rs.uniform(0.3, 3.0, n) * rs.choice([-1.0, 1.0], n)).astype(F32)
    m = (10.0 ** rs.uniform(-0.9, 30.0, n) * rs.choice([-1.0, 1.0], n)).astype(F32)
    c = rs.choice([0.0, 1.0, -2.0, 0.5], n).astype(F32)
    if edges:
        p[0:3], q[0:3] = [1e19, 1e19, 2e19], [1e19, 2e19, 2e19]                  # 1e38, 2e38, and 4e38: +inf
        p[3:5], q[3:5] = [1e-15, 1e15], [1e-15, 1e15]
        p[5:9], q[5:9] = [1.0, 1.0, 1.0, 1.0], [1e-30, -1e-30, 1e30, -1e30]      # the denominators' ends, either sign
        nn[0:6], m[0:6] = [1.0, 1.0, -1.0, -1.0, 0.0, -0.0], [0.0, -0.0, 0.0, -0.0, 0.0, 0.0]       # x / +-0 = +-inf; 0 / 0 = NaN
        m[6:8] = [1e30, -1e30]
        c[0:4] = [0.0, -0.0, 1.0, -1.0]                                        # the condition of a WHERE: +0.0 and -0.0 are both false
    return dict(a=a, b=b, p=p, q=q, sq=np.sign(q).astype(F32), n=nn, m=m, c=c)


def _bin_grad_grid(n):
    g = _bin_grid(n, edges=False)
    rs = np.random.default_rng(22)
    g["p"], g["q"] = rs.uniform(0.5, 2.0, n).astype(F32), (rs.uniform(0.5, 2.0, n) * rs.choice([-1.0, 1.0], n)).astype(F32)
    g["sq"] = np.sign(g["q"]).astype(F32)
    g["m"] = (rs.uniform(0.4, 3.0, n) * rs.choice([-1.0, 1.0], n)).astype(F32)
    g["c"][0:4] = [0.0, -0.0, 1.0, -1.0]
    return g


def _sel(cond, x, y):
    return np.where(cond, x, y)


BIN_SITES = [
    ("add", "mean", lambda L: genjax.square(L["a"]) + genjax.square(L["b"]), lambda v, d: v["a"][0] ** 2 + v["b"][0] ** 2),
    ("sub", "mean", lambda L: genjax.square(L["a"]) - genjax.square(L["b"]), lambda v, d: v["a"][0] ** 2 - v["b"][0] ** 2),
    ("mul_m", "mean", lambda L: L["a"] * L["b"], lambda v, d: v["a"][0] * v["b"][0]),
    # (q has either sign; the sign row sq = sign(q), unselected, makes the scale positive: a wrong sign of the result is NaN)
    ("mul_s", "scale", lambda L: (L["p"] * L["q"]) * L["sq"], lambda v, d: v["p"][0] * v["q"][0] * v["sq"][0]),
    ("div_s", "scale", lambda L: (L["p"] / L["q"]) * L["sq"], lambda v, d: v["p"][0] / v["q"][0] * v["sq"][0]),
    ("div_m", "mean", lambda L: L["n"] / L["m"], lambda v, d: v["n"][0] / v["m"][0]),
    ("div_sign", "mean", lambda L: genjax.tanh(L["n"] / L["m"]), lambda v, d: np.tanh(v["n"][0] / v["m"][0])),
    ("max", "mean", lambda L: genjax.maximum(L["a"], L["b"]), lambda v, d: _sel(d["a"][0] >= d["b"][0], v["a"][0], v["b"][0])),
    ("min", "mean", lambda L: genjax.minimum(L["a"], L["b"]), lambda v, d: _sel(d["a"][0] <= d["b"][0], v["a"][0], v["b"][0])),
    ("relu", "mean", lambda L: genjax.maximum(L["a"], 0.0), lambda v, d: _sel(d["a"][0] >= 0.0, v["a"][0], 0.0)),
    ("gt", "mean", lambda L: (L["a"] > L["b"]) * 1.0 + (L["a"] >= L["b"]) * 2.0 + (L["a"] < L["b"]) * 4.0,
     lambda v, d: (d["a"][0] > d["b"][0]) * 1.0 + (d["a"][0] >= d["b"][0]) * 2.0 + (d["a"][0] < d["b"][0]) * 4.0),
    ("where_cmp", "mean", lambda L: genjax.where(L["a"] > L["b"], genjax.tanh(L["a"]), genjax.square(L["b"])),
     lambda v, d: _sel(d["a"][0] > d["b"][0], np.tanh(v["a"][0]), v["b"][0] ** 2)),
    ("where_val", "mean", lambda L: genjax.where(L["c"], L["a"] * L["b"], genjax.sin(L["a"])),
     lambda v, d: _sel(d["c"][0] != 0.0, v["a"][0] * v["b"][0], np.sin(v["a"][0]))),
]
BIN_OPS = [A.E_CONST, A.E_VALUE, A.E_ADD, A.E_SUB, A.E_MUL, A.E_DIV, A.E_MAX, A.E_MIN, A.E_GT, A.E_WHERE]


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. integer powers: a ** k on bases of either sign.  |a ** 16| reaches 4e7, so on a the power is a SCALE (made positive by the sign
#    row s = sign(a) for odd k: a wrong sign of the power is a negative scale, NaN); base 0 and the sign itself on z in [-1, 1] as a mean
# ---------------------------------------------------------------------------------------------------------------------------------
POWERS = (0, 1, 2, 3, 4, 5, 7, 8, -1, -2, -3, 16)
POW_LAT = [("a", 10.0), ("s", 10.0), ("z", 10.0)]


def _pow_grid(n, lo=0.3, hi=3.0):
    a = _fill([lo, -lo, hi, -hi, 1.0, -1.0], lo, hi, n, both_signs=True, seed=31)
    return dict(a=a, s=np.sign(a).astype(F32), z=_fill([0.0, -0.0, 1.0, -1.0], -1.0, 1.0, n, seed=32))


def _pow_site_a(k):
    odd = k % 2 != 0
    return (f"a_pow_{k}", "scale", (lambda L: (L["a"] ** k) * L["s"]) if odd else (lambda L: L["a"] ** k),
            (lambda v, d: v["a"][0] ** k * v["s"][0]) if odd else (lambda v, d: v["a"][0] ** k + 0.0 * v["a"][0]))


def _pow_site_z(k):
    return (f"z_pow_{k}", "mean", lambda L: L["z"] ** k, lambda v, d: v["z"][0] ** k + 0.0 * v["z"][0])


POW_SITES = [_pow_site_a(k) for k in POWERS] + [_pow_site_z(k) for k in POWERS if k >= 0]
POW_OPS = [A.E_VALUE, A.E_SQUARE, A.E_MUL, A.E_RECIP]


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. guards: the unselected branch of a WHERE holds inf or NaN, in the value and under the gradient (the zero-adjoint rule)
# ---------------------------------------------------------------------------------------------------------------------------------
GUARD_LAT = [("x", 10.0), ("w", 100.0), ("c", 10.0)]


def _guard_grid(n, boundary=False):
    edges = [0.0, -0.0] * 8 + ([C1M3, -C1M3] * 4 if boundary else [])
    x = _fill(edges, 0.05, 9.0, n, both_signs=True, seed=41)
    rs = np.random.default_rng(42)
    c = rs.choice([0.0, 1.0, -0.0], n).astype(F32)
    w = np.where(c != 0, rs.uniform(-1.0, 1.0, n), rs.choice([89.0, 200.0, 1.0], n)).astype(F32)      # exp(w) = inf where c is false
    return dict(x=x, w=w, c=c)


def _guarded(cond, f, v, other):
    with np.errstate(all="ignore"):
        return np.where(cond, f(np.where(cond, v, 1.0)), other)


GUARD_SITES = [
    ("sqrt_pos", "mean", lambda L: genjax.where(L["x"] > 0, genjax.sqrt(L["x"]), 0.0), lambda v, d: _guarded(d["x"][0] > 0, np.sqrt, v["x"][0], 0.0)),
    ("log_pos", "mean", lambda L: genjax.where(L["x"] > 0, genjax.log(L["x"]), -1.0), lambda v, d: _guarded(d["x"][0] > 0, np.log, v["x"][0], -1.0)),
    ("recip_far", "mean", lambda L: genjax.where(genjax.abs(L["x"]) > 1e-3, 1.0 / L["x"], 0.0),
     lambda v, d: _guarded(np.abs(d["x"][0]) > C1M3, lambda t: 1.0 / t, v["x"][0], 0.0)),
    ("log1p_div", "mean", lambda L: genjax.where(L["x"] > 0, genjax.log1p(L["x"]) / L["x"], 1.0),
     lambda v, d: _guarded(d["x"][0] > 0, lambda t: np.log1p(t) / t, v["x"][0], 1.0)),
    ("relu_sqrt", "mean", lambda L: genjax.sqrt(genjax.maximum(L["x"], 0.0) + 1.0) * genjax.maximum(L["x"], 0.0),
     lambda v, d: (lambda r: np.sqrt(r + 1.0) * r)(_sel(d["x"][0] >= 0, v["x"][0], 0.0))),
    ("mul_inf", "mean", lambda L: genjax.where(L["c"], L["x"] * genjax.exp(_e(L["w"])), L["x"]),
     lambda v, d: _sel(d["c"][0] != 0.0, v["x"][0] * np.exp(np.where(d["c"][0] != 0.0, v["w"][0], 0.0)), v["x"][0])),
]
GUARD_OPS = [A.E_WHERE, A.E_GT, A.E_SQRT, A.E_LOG, A.E_ABS, A.E_DIV, A.E_LOG1P, A.E_MUL, A.E_EXP, A.E_MAX]


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. linear layers: LINV and LINN over 1, 2, 63 and 64 operands; a linear form over slots with a gap of one and of two unnamed slots
#    between them, with inf and NaN in the gap rows (include/gjx.h: LINV reads exactly the rows it names).  The 64 rows are two
#    32-vectors in consecutive slots (the generated kernels expand a choice of at most 32 elements): ONE LINV run spans both
# ---------------------------------------------------------------------------------------------------------------------------------
LIN_LAT = [("x", 1.0, 32), ("x2", 1.0, 32), ("a", 10.0), ("g1", 10.0), ("b", 10.0), ("g2", 10.0), ("g3", 10.0), ("c", 10.0)]
_rs = np.random.default_rng(51)
LIN_W = {k: _rs.uniform(-0.3, 0.3, k) for k in (1, 2, 63, 64)}
LIN_W[1] = np.array([0.7])
LINN_F = [("exp", np.exp, genjax.exp), ("square", np.square, genjax.square), ("tanh", np.tanh, genjax.tanh), ("sigmoid", _sigmoid, genjax.sigmoid),
          ("softplus", lambda t: np.logaddexp(0.0, t), genjax.softplus), ("abs", np.abs, genjax.abs), ("sin", np.sin, genjax.sin), ("cos", np.cos, genjax.cos),
          ("log1p", np.log1p, genjax.log1p), ("sqrt", np.sqrt, genjax.sqrt), ("log", np.log, genjax.log), ("recip", lambda t: 1.0 / t, lambda t: t ** -1),
          ("neg", lambda t: -t, lambda t: -t)]
# (LINN ranges over NODES: 64 operands in a block of at most 96 nodes are 13 unary ops of 5 leaves — 5 + 64 + 1 nodes)
LINN_TERMS = [(j, f64, fg) for _, f64, fg in LINN_F for j in range(5)]


def _linn_build(k):
    def build(L):
        xs = [_e(L["x"][j]) for j in range(5)]
        acc = None
        for (j, _, fg), w in zip(LINN_TERMS[:k], LIN_W[k]):
            t = float(w) * fg(xs[j])
            acc = t if acc is None else acc + t
        return acc + 0.25
    return build


def _linn_ref(k):
    return lambda v, d: 0.25 + sum(float(w) * f64(v["x"][j]) for (j, f64, _), w in zip(LINN_TERMS[:k], LIN_W[k]))


def _lin_grid(n, gaps=True):
    rs = np.random.default_rng(52)
    x = rs.uniform(-2.0, 2.0, (64, n))
    x[:5] = rs.uniform(0.3, 2.0, (5, n))            # the leaves of the LINN operands: every unary op is defined there
    out = dict(x=x[:32].astype(F32), x2=x[32:].astype(F32))
    for k in ("a", "b", "c", "g1", "g2", "g3"):
        out[k] = rs.uniform(-1.5, 1.5, n).astype(F32)
    if gaps:                                        # the rows BETWEEN the named ones: nothing may read them
        out["g1"][0::4] = np.inf
        out["g1"][1::4] = np.nan
        out["g2"][2::4] = -np.inf
        out["g3"][0::3] = np.nan
    return out


def _linv_build(k):
    if k <= 32:
        return lambda L: genjax.tanh(LIN_W[k] @ L["x"][:k])
    return lambda L: genjax.tanh(LIN_W[k][:32] @ L["x"] + LIN_W[k][32:] @ L["x2"][:k - 32])


LIN_SITES = [(f"linv_{k}", "mean", _linv_build(k),
              (lambda k: lambda v, d: np.tanh(LIN_W[k] @ np.concatenate([v["x"], v["x2"]])[:k]))(k)) for k in (1, 2, 63, 64)]
LIN_SITES += [(f"linn_{k}", "mean", _linn_build(k), _linn_ref(k)) for k in (1, 2, 63, 64)]
LIN_SITES += [
    ("gap_1", "mean", lambda L: genjax.tanh(L["a"] * L["a"]) + 2.0 * L["a"] + 3.0 * L["b"], lambda v, d: np.tanh(v["a"][0] ** 2) + 2.0 * v["a"][0] + 3.0 * v["b"][0]),
    ("gap_2", "mean", lambda L: genjax.tanh(L["b"] * L["b"]) - 2.0 * L["b"] + 0.5 * L["c"], lambda v, d: np.tanh(v["b"][0] ** 2) - 2.0 * v["b"][0] + 0.5 * v["c"][0]),
    ("gap_12", "mean", lambda L: genjax.sin(L["a"]) + 1.5 * L["a"] - 1.25 * L["b"] + 2.0 * L["c"] + 0.5,
     lambda v, d: np.sin(v["a"][0]) + 1.5 * v["a"][0] - 1.25 * v["b"][0] + 2.0 * v["c"][0] + 0.5),
]
LIN_OPS = [A.E_LINV, A.E_LINN, A.E_VALUE]


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the special functions: erf, erfc, lgamma, expm1 as general nodes, each as a mean (absolute error) and as a scale (relative error).
#    The float64 side is scipy.special / np.expm1.  Two lgamma edges are REACHED EXACTLY, none is masked:
#      * close approaches to the poles: lgamma(u - k), k = 0 .. 4, over a latent u that is a multiple of 2^-20 (2^-m, 4 <= m <= 20, among
#        them): u - k is exact in float32 and the reference is conditioned in u (a relative move of -k + 2^-20 itself would move the
#        distance to the pole by twice its size)
#      * the poles -1 .. -4 and a negative beyond 2^23 (every float32 there is an integer): u = 0 in some columns — 0 stays 0 under the
#        conditioning check's relative move, a pole written as a latent -1 would leave the pole.  The far one sits in the unselected
#        branch's place of a WHERE decided by u > 0
# ---------------------------------------------------------------------------------------------------------------------------------
import scipy.special as _sp           # noqa: E402

TINY32, MAX32 = float(np.finfo(F32).tiny), float(np.finfo(F32).max)


def _last_f32(ok, lo, hi):
    """the largest float32 x in [lo, hi] with ok(float64(x)) (ok holds at lo, fails at hi, changes once), by bisection on float64"""
    lo, hi = float(F32(lo)), float(F32(hi))
    assert ok(lo) and not ok(hi)
    while float(F32(0.5 * (lo + hi))) not in (lo, hi):
        mid = float(F32(0.5 * (lo + hi)))
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


ERFC_LAST = _last_f32(lambda t: _sp.erfc(t) >= TINY32, 9.0, 9.5)                  # about 9.1945: beyond it erfc(x) is no normal float32
EXPM1_OVER = float(np.log(MAX32))                                                # 88.7228: expm1 overflows
LGAMMA_OVER = _last_f32(lambda t: _sp.gammaln(t) <= MAX32, 1e36, 1e37)           # about 4.085e36: x log x overflows
FAR_NEG = 2.0 ** 24
SP_SHIFTS = (0, 1, 2, 3, 4)
SP_LAT = [("xfm", 1e20), ("xfs", 10.0), ("xcm", 1e20), ("xcs", 10.0), ("xem", 1e20), ("xes", 100.0), ("xgm", 10.0), ("u", 10.0), ("xgg", 1e20),
          ("xgs", 1e20)]
_NEAR = [-k + s * 0.05 for k in (0, 1, 2) for s in (-1, 1)] + [-k + s * 0.2 for k in range(3, 11) for s in (-1, 1)]       # -k +- delta


def _neg_between_poles(n, rs, margin):
    """n negatives -k - frac, k = 0 .. 10, frac in [margin, 1 - margin]: no closer to a pole than margin"""
    return -(rs.integers(0, 11, n) + rs.uniform(margin, 1.0 - margin, n))


def _dyadic(n, rs, lo_exp, edges=()):
    """n multiples of 2^-20 in [2^lo_exp, 1/2], log-uniform, after the edges"""
    j = np.floor(2.0 ** rs.uniform(lo_exp + 20, 19, n - len(edges)))
    x = np.concatenate([np.asarray(edges, np.float64), j * 2.0 ** -20])
    return x[rs.permutation(n)].astype(F32)


def _sp_grid(n):
    rs = np.random.default_rng(71)
    tiny = POW2(range(1, 100, 3))                                                # +-2^-k down to 1.6e-30
    far = [s * t for t in (3.9, 4.0, 5.0, 10.0, 1e10, 1e30) for s in (1.0, -1.0)]
    pos_g = _fill([1e-12, 0.5, 1.0, 2.0, 1.4616321, 14.0] + [0.5 * k for k in range(3, 28)], 1e-12, 14.0, n - n // 3, log=True, seed=77)
    neg_g = np.concatenate([_NEAR, _neg_between_poles(n // 3 - len(_NEAR), rs, 0.2)]).astype(F32)
    return dict(
        xfm=_fill(np.concatenate([[0.0, -0.0], tiny, far]), -4.0, 4.0, n, seed=72),                         # erf as a mean
        xfs=_fill([1e-30, 20.0, 1.0], 1e-30, 20.0, n, log=True, seed=73),                                    # as a scale: relative accuracy near 0
        xcm=_fill([0.0, 1e30, -1e30, 30.0, -30.0, 1e10, -1e10], -30.0, 30.0, n, seed=74),                   # erfc as a mean: 0 or 2 far out
        xcs=_fill([ERFC_LAST, -6.0, 0.0, 9.0], -6.0, ERFC_LAST, n, seed=75),                                 # as a scale: down to float32's smallest normal
        xem=_fill(np.concatenate([[0.0], tiny, [-17.0, -88.0, -104.0, -200.0, -1e30, 3.4]]), -20.0, 3.4, n, seed=76),      # expm1 as a mean
        xes=_fill([1e-30, 69.0, 88.7, 88.8, 1.0], 1e-30, 69.0, n, log=True, seed=78),                        # as a scale; 88.8: +inf
        xgm=np.concatenate([pos_g, neg_g])[rs.permutation(n)].astype(F32),                                   # lgamma as a mean, either side of 0
        u=_dyadic(n, rs, -20, [0.0] * 6 + [2.0 ** -m for m in range(4, 21)]),                                # lgamma(u - k): exact approaches, and the poles
        xgg=_fill([0.0, -0.0, -1.0, -2.0, -1e7] * 3, 0.05, 9.0, n, both_signs=True, seed=79),                # the guarded lgamma
        xgs=np.concatenate([_fill([3.0, 1e28, 0.99 * LGAMMA_OVER, 1.01 * LGAMMA_OVER], 3.0, 1e28, n - n // 2, log=True, seed=80),
                            _fill([1e-37, 0.5], 1e-37, 0.5, n // 2, log=True, seed=81)])[rs.permutation(n)].astype(F32))       # lgamma as a scale


def _sp_grad_grid(n):
    rs = np.random.default_rng(82)
    sat = [s * t for t in (5.0, 10.0, 30.0, 100.0) for s in (1.0, -1.0)]
    n_neg = n // 2                                                               # (at least a third of the lgamma columns: the reflection)
    return dict(
        xfm=_fill(np.concatenate([[0.0], POW2(range(4, 21, 4)), sat]), -3.0, 3.0, n, seed=83),
        xfs=_fill([], 0.01, 4.0, n, log=True, seed=84),
        xcm=_fill([0.0, 6.0, -6.0, 30.0, -30.0], -4.0, 4.0, n, seed=85),
        xcs=_fill([9.0, -3.0], -3.0, 9.0, n, seed=86),
        xem=_fill(np.concatenate([[0.0], POW2(range(4, 21, 4)), [-17.0, -20.0]]), -5.0, 3.0, n, seed=87),
        xes=_fill([], 0.01, 30.0, n, log=True, seed=88),
        xgm=np.concatenate([_fill([0.5, 1.0, 2.0, 1.4616321], 0.05, 14.0, n - n_neg, log=True, seed=89),
                            _neg_between_poles(n_neg, rs, 0.1)])[rs.permutation(n)].astype(F32),
        u=_dyadic(n, rs, -4),
        xgg=_fill([0.0, -0.0, -1.0, -2.0] * 3, 0.05, 9.0, n, both_signs=True, seed=90),
        xgs=np.concatenate([_fill([], 3.0, 50.0, n - n // 2, log=True, seed=91), _fill([], 0.01, 0.5, n // 2, log=True, seed=92)])[rs.permutation(n)].astype(F32))


def _lgamma_shift_site(k):
    return (f"lgamma_u_{k}", "mean", lambda L: genjax.lgamma(L["u"] - float(k)), lambda v, d: _sp.gammaln(v["u"][0] - float(k)))


SP_SITES = [
    ("erf_m", "mean", lambda L: genjax.erf(_e(L["xfm"])), lambda v, d: _sp.erf(v["xfm"][0])),
    ("erf_s", "scale", lambda L: genjax.erf(_e(L["xfs"])), lambda v, d: _sp.erf(v["xfs"][0])),
    ("erfc_m", "mean", lambda L: genjax.erfc(_e(L["xcm"])), lambda v, d: _sp.erfc(v["xcm"][0])),
    ("erfc_s", "scale", lambda L: genjax.erfc(_e(L["xcs"])), lambda v, d: _sp.erfc(v["xcs"][0])),       # (1 - erf: 0 from x = 4 on, a scale of 0)
    ("expm1_m", "mean", lambda L: genjax.expm1(_e(L["xem"])), lambda v, d: np.expm1(v["xem"][0])),
    ("expm1_s", "scale", lambda L: genjax.expm1(_e(L["xes"])), lambda v, d: np.expm1(v["xes"][0])),     # (exp(x) - 1: 0 below 6e-8, a scale of 0)
    ("lgamma_m", "mean", lambda L: genjax.lgamma(_e(L["xgm"])), lambda v, d: _sp.gammaln(v["xgm"][0])),
] + [_lgamma_shift_site(k) for k in SP_SHIFTS] + [
    ("lgamma_far", "mean", lambda L: genjax.where(L["u"] > 0, genjax.lgamma(L["u"] + 3.0), genjax.lgamma(L["u"] - FAR_NEG)),
     lambda v, d: _sel(d["u"][0] > 0, _sp.gammaln(v["u"][0] + 3.0), _sp.gammaln(np.where(d["u"][0] > 0, -0.5, v["u"][0] - FAR_NEG)))),
    ("lgamma_pos", "mean", lambda L: genjax.where(L["xgg"] > 0, genjax.lgamma(L["xgg"]), 0.0),
     lambda v, d: _guarded(d["xgg"][0] > 0, _sp.gammaln, v["xgg"][0], 0.0)),
    ("lgamma_s", "scale", lambda L: genjax.lgamma(_e(L["xgs"])), lambda v, d: _sp.gammaln(v["xgs"][0])),
]
SP_OPS = [A.E_ERF, A.E_ERFC, A.E_LGAMMA, A.E_EXPM1, A.E_WHERE, A.E_GT, A.E_LINV]


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. log-sum-exp: genjax.logsumexp over 2, 3, 63, 64, 65 and 93 elements of vector latents (93 operands pack into exactly 96 nodes; 65
#    lower to a 64-operand node, a one-operand node and a node over both), np.logaddexp, lists of general expressions, a nested and a
#    constant-carrying one.  The operand patterns sit in the first columns of the grid: all equal; ties at the maximum; one operand
#    ahead by more than 104 nats (the others underflow); all at -1e30; all -inf; some -inf; and one operand overflowed to +inf
#    (exp(a * a) at a = 10: the result is +inf, include/gjx.h).  The float64 side is scipy.special.logsumexp.
# ---------------------------------------------------------------------------------------------------------------------------------
LSE_ARITIES = (2, 3, 63, 64, 65, 93)
LSE_LAT = [("x", 1e20, 32), ("x2", 1e20, 32), ("x3", 1e20, 32), ("a", 10.0), ("b", 10.0), ("c", 10.0), ("w", 10.0, 3)]
LSE_AHEAD = (0, 1, 2, 62, 63, 64, 92)         # where the operand far ahead sits: in and across the 64-operand chunks


def _lse_rows(v):
    return np.concatenate([v["x"], v["x2"], v["x3"]])


def _lse64(rows):
    with np.errstate(all="ignore"):
        return _sp.logsumexp(np.asarray(rows, np.float64), axis=0)


def _lse_grid(n, edges=True):
    rs = np.random.default_rng(101)
    x = rs.uniform(-3.0, 3.0, (96, n))
    a, b, c = (rs.uniform(-1.5, 1.5, n) for _ in range(3))
    w = rs.uniform(0.05, 3.0, (3, n))
    pat = np.arange(n) % 7
    head = np.arange(n) < (28 * 7 if edges else 12 * 3)
    for i in np.nonzero(head)[0]:
        k = i // 7 if edges else i // 3
        p_ = pat[i] if edges else i % 3
        if p_ == 0:                                        # all equal
            x[:, i] = rs.uniform(-20.0, 20.0)
        elif p_ == 1:                                      # ties at the maximum: two or three positions
            top = rs.uniform(0.0, 4.0)
            x[:, i] = top - rs.uniform(0.5, 5.0, 96)
            x[rs.choice(96, 2 + k % 2, replace=False), i] = top
            x[[0, 1, 2][:2 + k % 2], i] = top              # (and among the first operands, for the small arities)
        elif p_ == 2:                                      # one operand ahead by more than 104 nats
            x[:, i] = -50.0 - rs.uniform(0.0, 3.0, 96)
            x[LSE_AHEAD[k % len(LSE_AHEAD)], i] = 60.0
        elif p_ == 3:
            x[:, i] = -1e30
        elif p_ == 4:
            x[:, i] = -np.inf
            w[:, i] = 0.0                                  # log 0 three times: every operand of the list is -inf too
        elif p_ == 5:                                      # some -inf, the first operand among them
            x[rs.random(96) < 0.5, i] = -np.inf
            x[0, i], x[1, i] = -np.inf, rs.uniform(-3.0, 3.0)
            w[k % 3, i] = 0.0
        else:
            a[i] = 10.0 if k % 2 == 0 else -10.0           # exp(a * a) = exp(100): +inf in float32
    return dict(x=x[:32].astype(F32), x2=x[32:64].astype(F32), x3=x[64:].astype(F32), a=a.astype(F32), b=b.astype(F32), c=c.astype(F32),
                w=w.astype(F32))


def _lse_arity_site(k):
    def build(L):
        el = [L["x"][j] for j in range(32)] + [L["x2"][j] for j in range(32)] + [L["x3"][j] for j in range(32)]
        return genjax.logsumexp(el[:k])
    return (f"lse_{k}", "mean", build, lambda v, d: _lse64(_lse_rows(v)[:k]))


LSE_SITES = [_lse_arity_site(k) for k in LSE_ARITIES] + [
    ("logaddexp", "mean", lambda L: np.logaddexp(L["a"], L["b"]), lambda v, d: np.logaddexp(v["a"][0], v["b"][0])),
    ("lse_list", "mean", lambda L: genjax.logsumexp([2.0 * L["a"], L["b"] * L["b"], genjax.tanh(L["c"])]),
     lambda v, d: _lse64([2.0 * v["a"][0], v["b"][0] ** 2, np.tanh(v["c"][0])])),
    ("lse_log", "mean", lambda L: genjax.logsumexp(genjax.log(_e(L["w"]))), lambda v, d: np.log(v["w"].sum(0))),
    ("lse_scale", "scale", lambda L: genjax.exp(genjax.logsumexp([20.0 * L["b"], 20.0 * L["c"], L["a"] * L["c"]])),
     lambda v, d: np.exp(_lse64([20.0 * v["b"][0], 20.0 * v["c"][0], v["a"][0] * v["c"][0]]))),
    ("lse_nested", "mean", lambda L: genjax.logsumexp([genjax.logsumexp([L["b"], L["c"] * L["c"]]), np.logaddexp(L["c"], 0.5), 1.5]),
     lambda v, d: _lse64([v["b"][0], v["c"][0] ** 2, v["c"][0], np.full_like(v["c"][0], 0.5), np.full_like(v["c"][0], 1.5)])),
    ("lse_inf", "mean", lambda L: genjax.logsumexp([genjax.exp(L["a"] * L["a"]), L["b"]]),
     lambda v, d: _lse64([np.exp(v["a"][0] ** 2), v["b"][0]])),
]
LSE_OPS = [A.E_LSEN, A.E_VALUE, A.E_EXP, A.E_LOG, A.E_MUL]


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. reductions: sum, mean, cumsum, prod, max, min over a plain latent vector (sums: the closed affine forms) and over a general
#    expression vector (sums: LINN; prod / max / min: folds of MUL / MAX / MIN), at lengths 1, 2 and 30.  The first columns hold: a sum
#    that cancels to a few ulps of its largest term (every partial sum exact in float32); a product with one zero, with two, with sign
#    changes, one that overflows and one that underflows; max / min with ties at two and three positions (the gradient goes to the
#    EARLIEST index: the fold and MAX's rule), 0.0 against -0.0, and +-inf elements
# ---------------------------------------------------------------------------------------------------------------------------------
RED_LENS = (1, 2, 30)
RED_LAT = [("r", 100.0, 32), ("p", 1e10, 8), ("m", 10.0, 4)]


def _red_grid(n, edges=True):
    rs = np.random.default_rng(111)
    r = rs.uniform(0.2, 1.5, (32, n)) * rs.choice([-1.0, 1.0], (32, n))
    p = rs.uniform(0.7, 1.3, (8, n)) * rs.choice([-1.0, 1.0], (8, n))
    m = rs.uniform(-2.0, 2.0, (4, n))
    for i in range(8):                                     # cancellation: 8192 - 8192 + k / 1024, nothing else
        r[:, i] = 0.0
        r[0, i], r[1, i] = 8192.0, -8192.0 + (i + 1) / 1024.0
    for i in range(8, 16):
        p[i % 8, i] = 0.0                                  # one zero: the gradient goes to that element only
    for i in range(16, 24):
        p[[i % 8, (i + 3) % 8], i] = 0.0                   # two zeros: the gradient is all zero
    for i in range(24, 48):                                # ties at two and at three positions; +0 against -0
        j = rs.choice(4, 2 + i % 2, replace=False)
        m[j, i] = m[:, i].max() + 0.25 if i % 4 < 2 else m[:, i].min() - 0.25
    m[:, 48], m[:, 49], m[:, 50], m[:, 51] = [0.0, -0.0, -1.0, -0.0], [-0.0, 0.0, -1.0, -2.0], [0.0, -0.0, 1.0, 0.0], [-0.0, 0.0, 0.5, 1.0]
    if edges:
        p[2:, 52], p[2:, 53] = 1e8, -1e8                   # six factors of 1e8 (the first two stay of order 1): 1e48, +-inf by the signs
        p[2:, 54] = 1e8 * np.array([1, -1, 1, 1, 1, 1.0])
        p[2:, 55], p[2:, 56] = 1e-9, -1e-9                 # 1e-54: 0
        m[:, 57], m[:, 58], m[:, 59] = [0.3, np.inf, -1.0, 0.1], [0.3, -np.inf, -1.0, 0.1], [np.inf, -np.inf, np.inf, 0.0]
    return dict(r=r.astype(F32), p=p.astype(F32), m=m.astype(F32))


def _gen(x):
    return genjax.tanh(x)            # the general expression vector the reductions range over


def _first(d, v, pick):
    """the element of v at the EARLIEST index where d attains its maximum (pick = np.argmax) or minimum (np.argmin)"""
    return np.take_along_axis(v, pick(d, axis=0)[None], 0)[0]


def _red_sites():
    out = []
    for k in RED_LENS:
        sl = (lambda k: lambda L: L["r"][:k])(k)
        out += [
            (f"sum_v_{k}", "mean", (lambda sl: lambda L: sl(L).sum())(sl), (lambda k: lambda v, d: v["r"][:k].sum(0))(k)),
            (f"mean_v_{k}", "mean", (lambda sl: lambda L: np.mean(sl(L)))(sl), (lambda k: lambda v, d: v["r"][:k].mean(0))(k)),
            (f"sum_g_{k}", "mean", (lambda sl: lambda L: _gen(sl(L)).sum())(sl), (lambda k: lambda v, d: np.tanh(v["r"][:k]).sum(0))(k)),
            (f"mean_g_{k}", "mean", (lambda sl: lambda L: _gen(sl(L)).mean())(sl), (lambda k: lambda v, d: np.tanh(v["r"][:k]).mean(0))(k)),
        ]
        for at in sorted({k // 2, k - 1}):
            out += [
                (f"cumsum_v_{k}_{at}", "mean", (lambda sl, at: lambda L: sl(L).cumsum()[at])(sl, at),
                 (lambda k, at: lambda v, d: v["r"][:at + 1].sum(0))(k, at)),
                (f"cumsum_g_{k}_{at}", "mean", (lambda sl, at: lambda L: np.cumsum(_gen(sl(L)))[at])(sl, at),
                 (lambda k, at: lambda v, d: np.tanh(v["r"][:at + 1]).sum(0))(k, at)),
            ]
    out += [
        ("prod_v", "mean", lambda L: L["p"].prod(), lambda v, d: v["p"].prod(0)),
        ("prod_g", "mean", lambda L: (1.5 * _gen(L["p"])).prod(), lambda v, d: (1.5 * np.tanh(v["p"])).prod(0)),
        ("prod_2", "mean", lambda L: L["p"][:2].prod(), lambda v, d: v["p"][:2].prod(0)),
        ("max_v", "mean", lambda L: L["m"].max(), lambda v, d: _first(d["m"], v["m"], np.argmax)),
        ("min_v", "mean", lambda L: L["m"].min(), lambda v, d: _first(d["m"], v["m"], np.argmin)),
        ("max_g", "mean", lambda L: np.max(_gen(L["m"])), lambda v, d: _first(np.tanh(d["m"]), np.tanh(v["m"]), np.argmax)),
        ("min_g", "mean", lambda L: np.amin(_gen(L["m"])), lambda v, d: _first(np.tanh(d["m"]), np.tanh(v["m"]), np.argmin)),
        ("max_1", "mean", lambda L: genjax.square(L["m"][:1].max()), lambda v, d: v["m"][0] ** 2),
    ]
    return out


RED_SITES = _red_sites()
# the sums over the PLAIN latent vector are closed affine forms (GJX_P_AFFINE / GJX_P_VALUE), not expression blocks: exactly these
CLOSED_FORMS = {"reduce": {s[0] for s in RED_SITES if s[0].startswith(("sum_v_", "mean_v_", "cumsum_v_"))}}
RED_OPS = [A.E_LINN, A.E_MUL, A.E_MAX, A.E_MIN, A.E_TANH, A.E_VALUE]


def _grad_of(grid, **kw):
    return lambda n: grid(n, **kw)


SPECS = {
    "unary": Spec(UN_LAT, UN_SITES, _un_grid, _un_grad_grid, UN_OPS),
    "binary": Spec(BIN_LAT, BIN_SITES, _bin_grid, _bin_grad_grid, BIN_OPS),
    "powers": Spec(POW_LAT, POW_SITES, _pow_grid, _pow_grid, POW_OPS),
    "guards": Spec(GUARD_LAT, GUARD_SITES, _guard_grid, _grad_of(_guard_grid, boundary=True), GUARD_OPS),
    "linear": Spec(LIN_LAT, LIN_SITES, _lin_grid, _grad_of(_lin_grid, gaps=True), LIN_OPS),
    "special": Spec(SP_LAT, SP_SITES, _sp_grid, _sp_grad_grid, SP_OPS),
    "lse": Spec(LSE_LAT, LSE_SITES, _lse_grid, _grad_of(_lse_grid, edges=False), LSE_OPS),
    "reduce": Spec(RED_LAT, RED_SITES, _red_grid, _grad_of(_red_grid, edges=False), RED_OPS),
}
# the latents whose rows hold inf / NaN on purpose (unnamed gap rows): their own sites' scores are then NaN in the reference too; they
# are not selected for gradients and HMC
UNSELECTED = {"linear": ("g1", "g2", "g3"), "powers": ("s",), "guards": ("c",), "binary": ("c", "sq"), "unary": ("sr",)}


def block_ops(prog):
    """the node ops of every expression block of a packed program"""
    ops = set()
    for j in range(prog.n_sites):
        for k in range(A.MAX_PARAMS):
            cp = prog.c_sites[j].p[k]
            if cp.op == A.P_EXPR:
                ops |= set(prog.tab[cp.off:cp.off + A.EXPR_NODE_FLOATS * cp.n].reshape(-1, A.EXPR_NODE_FLOATS)[:, 0].astype(int).tolist())
    return ops


# ---------------------------------------------------------------------------------------------------------------------------------
# the harness both test files use
# ---------------------------------------------------------------------------------------------------------------------------------
def same_nonfinite(got, want, what=""):
    """where the reference is +-inf or NaN the result is the SAME infinity or NaN; -> the mask of the finite reference points"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert (np.isnan(got) == np.isnan(want)).all(), f"{what}: NaN at {np.nonzero(np.isnan(got) != np.isnan(want))}"
    inf = np.isinf(want)
    assert (got[inf] == want[inf]).all(), f"{what}: the reference's infinities are not reproduced"
    return np.isfinite(want)


def packed(spec, which, grad=False):
    sl, _ = spec["model"].site_list(())
    assert [s.addr for s in sl.sites] == [a for a, _ in spec["sites"]]
    modes = {s.addr: A.MODE_OBS_SLOT for s in sl.sites}
    if not grad:
        return PackedProgram(sl, modes)
    sel = tuple(a for a, _, _ in spec["latents"] if a not in UNSELECTED.get(which, ()))
    return PackedProgram(sl, modes, {}, selected=sel)


def fd_gradient(spec, prog, ch, rows):
    """central differences (step 1e-5) of the float64 total with the decisions frozen at the base point: the analytic gradient
    under the rules of include/gjx.h at ties, kinks and guard boundaries, the ordinary derivative elsewhere"""
    c64 = ch.astype(np.float64)

    def vals(r):
        return {a: r[prog.slot_of[a]:prog.slot_of[a] + d] for a, d in spec["sites"]}
    base = vals(c64)

    def total(v):
        """(the rows that hold inf / NaN on purpose belong to unselected sites: their own, constant terms are left out of the sum)"""
        s = np.stack(spec["scores"](v, base))
        keep = np.isfinite(np.stack(spec["scores"](base))).all(axis=1)
        return s[keep].sum(0)
    fd = {}
    h = 1e-5
    for r in rows:
        up, dn = c64.copy(), c64.copy()
        up[r] += h
        dn[r] -= h
        with np.errstate(all="ignore"):
            fd[r] = (total(vals(up)) - total(vals(dn))) / (2 * h)
    with np.errstate(all="ignore"):
        return fd, np.stack(spec["scores"](base)).sum(0)           # (the total of EVERY site: NaN / -inf in the columns whose unnamed rows hold them)


def exact_zero_gradients(prog, ch):
    """the unary program's tanh-only and sigmoid-only latents (prior scale 1e20: the prior's own gradient is below 1e-37): -> [(row,
    columns)] where the float64 gradient of the site through the op is EXACTLY 0 — the derivative rounds to 0 far out (tanh from
    |x| = 20, sigmoid from x = 50) — and the device's must be too"""
    out = []
    for lat, site, f in (("xth", "tanh_only", np.tanh), ("xsg", "sigmoid_only", _sigmoid)):
        x, y = ch[prog.slot_of[lat]].astype(np.float64), ch[prog.slot_of[site]].astype(np.float64)
        df = 1.0 - f(x) ** 2 if site == "tanh_only" else f(x) * (1.0 - f(x))
        cols = np.nonzero((y - f(x)) * df == 0.0)[0]
        assert len(cols) >= (8 if site == "tanh_only" else 3), (site, len(cols))
        out.append((prog.slot_of[lat], cols))
    return out


def exact_zero_gradients_special(prog, ch):
    """the special program's erf latent far out (|x| >= 30: float64's exp(-x^2) is 0) and the guarded lgamma's latent where the guard is
    closed (a <= 0, the poles 0, -1 and -2 among them: digamma there is +-inf or NaN and meets a zero adjoint); both priors have scale 1e20"""
    x, y = ch[prog.slot_of["xfm"]].astype(np.float64), ch[prog.slot_of["erf_m"]].astype(np.float64)
    far = np.nonzero((y - _sp.erf(x)) * np.exp(-x * x) == 0.0)[0]
    closed = np.nonzero(ch[prog.slot_of["xgg"]] <= 0)[0]
    assert len(far) >= 4 and len(closed) >= 12 and {0.0, -1.0, -2.0} <= set(ch[prog.slot_of["xgg"]][closed].tolist())
    return [(prog.slot_of["xfm"], far), (prog.slot_of["xgg"], closed)]


EXACT_ZERO = {"unary": exact_zero_gradients, "special": exact_zero_gradients_special}


def selected_rows(spec, prog, which):
    return [prog.slot_of[a] + e for a, _, d in spec["latents"] if a not in UNSELECTED.get(which, ()) for e in range(d)]


# ---------------------------------------------------------------------------------------------------------------------------------
# structural cases: the same body — a guard, an integer power, a linear form over rows with an unnamed row between them — as ONE plate
# of 16 instances and as a rolled Scan of 64 steps
# ---------------------------------------------------------------------------------------------------------------------------------
N_PLATE, T_SCAN = 16, 64


def structural_plate(n):
    """-> (program, rows f32[n_slots][n], scores(rows64) -> float64[n_sites][n]).  Latents a, g, c, b in consecutive rows; the kernel's
    mean reads a, c and b — g, the row between a and c, holds inf and NaN in some columns and nothing but its own site may read it"""
    from genjax_amd import C
    rs = np.random.default_rng(61)
    X = rs.uniform(0.5, 1.5, (N_PLATE, 2)).astype(F32) * rs.choice([-1.0, 1.0], (N_PLATE, 2)).astype(F32)
    Y = rs.standard_normal(N_PLATE).astype(F32)

    @genjax.gen
    def kern(x_row, a, b, c):
        m = genjax.where(a > 0, genjax.sqrt(a), 0.0) + 0.1 * b ** 3 + genjax.tanh(a * b) + x_row[0] * a + x_row[1] * c
        return genjax.normal(m, 1.0) @ "y"

    @genjax.gen
    def model():
        a = genjax.normal(0.0, 1.0) @ "a"
        genjax.normal(0.0, 1.0) @ "g"
        c = genjax.normal(0.0, 1.0) @ "c"
        b = genjax.normal(0.0, 1.0) @ "b"
        kern.vmap(in_axes=(0, None, None, None))(X, a, b, c) @ "obs"

    prog, _, _ = model.pack((), C["obs", "y"].set(Y), False, per_particle=("a", "g", "c", "b"), rng_mode=A.RNG_FLAT)
    assert [prog.slot_of[k] for k in "agcb"] == [0, 1, 2, 3]
    rows = rs.uniform(-1.5, 1.5, (prog.n_slots, n)).astype(F32)
    rows[0, :8] = [0.0, -0.0, 0.0, -0.0, 1.0, 1.0, -1.0, -1.0]            # the guard's boundary
    rows[1, 0::4], rows[1, 1::4], rows[1, 2::4] = np.inf, np.nan, -np.inf

    def scores(r):
        a, g, c, b = r[0], r[1], r[2], r[3]
        X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
        with np.errstate(all="ignore"):
            m = np.where(a > 0, np.sqrt(np.where(a > 0, a, 1.0)), 0.0) + 0.1 * b ** 3 + np.tanh(a * b) + X64[:, :1] * a + X64[:, 1:] * c
            return np.stack([nlp(a, 0.0, 1.0), nlp(g, 0.0, 1.0), nlp(c, 0.0, 1.0), nlp(b, 0.0, 1.0), nlp(Y64[:, None], m, 1.0).sum(0)])
    return prog, rows, scores


def structural_scan():
    """-> (program, restate(prog, choices64) -> (likelihood, prior) float64[K]).  Step: x, g, z in consecutive rows; the next step's mean
    reads x and z of the step before (a linear form with g's row between them), a guard and a cube of x"""
    from genjax_amd import C
    ys = np.random.default_rng(62).standard_normal(T_SCAN).astype(F32)

    def mean(xp, zp, where, sqrt, tanh):
        return 0.5 * where(xp > 0, sqrt(xp), 0.0) - 0.02 * xp ** 3 + tanh(xp * zp) + 0.3 * xp - 0.4 * zp

    @genjax.gen
    def step(carry, _):
        xp, zp = carry
        x = genjax.normal(mean(xp, zp, genjax.where, genjax.sqrt, genjax.tanh), 0.5) @ "x"
        genjax.normal(0.0, 1.0) @ "g"
        z = genjax.normal(0.5 * zp, 0.5) @ "z"
        genjax.normal(x + z, 1.0) @ "y"
        return (x, z), None

    prog, _, _ = step.scan(n=T_SCAN).pack(((np.float32(0.4), np.float32(-0.2)), None), C["y"].set(ys), True, rng_mode=A.RNG_FLAT)

    def restate(prog, ch):
        x, g, z = (np.stack([ch[prog.slot_of[(k, t)]] for t in range(T_SCAN)]) for k in "xgz")
        xp = np.concatenate([np.full((1, x.shape[1]), np.float64(F32(0.4))), x[:-1]])
        zp = np.concatenate([np.full((1, x.shape[1]), np.float64(F32(-0.2))), z[:-1]])
        with np.errstate(all="ignore"):
            m = mean(xp, zp, np.where, lambda t: np.sqrt(np.where(t > 0, t, 1.0)), np.tanh)
        prior = (nlp(x, m, 0.5) + nlp(g, 0.0, 1.0) + nlp(z, 0.5 * zp, 0.5)).sum(0)
        return nlp(ys[:, None].astype(np.float64), x + z, 1.0).sum(0), prior
    return prog, restate


def special_plate(n):
    """-> (program, rows f32[n_slots][n], scores(rows64) -> float64[n_sites][n]).  16 instances, ONE plate site y ~ normal(lgamma(x0 a + b),
    erfc(x1 c + d)): the instance's covariates are data (per-instance table rows), a, b, c, d latent, the observations per column (rows).
    lgamma's argument runs to the edges of the special program's mean site: down to 1e-12 towards the pole at 0, between the negative
    poles to -10.8, up to 14.5.  erfc's runs from -6 (where it is 2) to 1.05 only: the site's mean is a float32 of size 1 to 30, known
    to 1e-7 at best, so a scale much below 0.1 would turn that error into more than the tolerance — the float64 restatement itself
    is not conditioned there (erfc as a scale down to 1.2e-38 is the special program's erfc_s, whose mean is exactly 0)"""
    rs = np.random.default_rng(63)
    X = np.stack([rs.uniform(0.5, 2.0, N_PLATE), rs.uniform(0.25, 0.95, N_PLATE)], 1).astype(F32)

    @genjax.gen
    def kern(x_row, a, b, c, d):
        return genjax.normal(genjax.lgamma(x_row[0] * a + b), genjax.erfc(x_row[1] * c + d)) @ "y"

    @genjax.gen
    def model():
        a = genjax.normal(0.0, 10.0) @ "a"
        b = genjax.normal(0.0, 10.0) @ "b"
        c = genjax.normal(0.0, 10.0) @ "c"
        d = genjax.normal(0.0, 10.0) @ "d"
        kern.vmap(in_axes=(0, None, None, None, None))(X, a, b, c, d) @ "obs"

    sl, _ = model.site_list(())
    ys = tuple(s.addr for s in sl.sites[4:])
    from genjax_amd.core import ChoiceMap
    prog, _, _ = model.pack((), ChoiceMap.empty(), False, per_particle=("a", "b", "c", "d") + ys, rng_mode=A.RNG_FLAT)
    y0 = prog.slot_of[ys[0]]
    assert [prog.slot_of[k] for k in "abcd"] == [0, 1, 2, 3] and [prog.slot_of[k] for k in ys] == list(range(y0, y0 + N_PLATE))
    rows = np.zeros((prog.n_slots, n), np.float32)
    rows[0], rows[1] = rs.uniform(1.0, 4.0, n), rs.uniform(0.0, 0.5, n)                 # lgamma's argument: 0.5 .. 8.5
    rows[2], rows[3] = rs.uniform(-3.0, 1.0, n), rs.uniform(-0.1, 0.1, n)              # erfc's: -3 .. 1.05
    q = n // 4
    rows[2, :2 * q] = rs.uniform(-3.0, 0.0, 2 * q)                                      # (a mean of size 30 wants a scale of order 1)
    rows[0, 3 * q::2] = rs.uniform(4.0, 7.0, len(rows[0, 3 * q::2]))                    # up to 14.5, with erfc's argument below 0
    rows[2, 3 * q::2] = rs.uniform(-3.0, 0.0, len(rows[0, 3 * q::2]))
    rows[0, :q], rows[1, :q] = 10.0 ** rs.uniform(-12.0, -1.0, q), 0.0                  # towards the pole at 0: down to 5e-13
    rows[0, q:2 * q] = 0.0                                                              # between the negative poles, for EVERY instance
    rows[1, q:2 * q] = -(rs.integers(0, 11, q) + rs.uniform(0.2, 0.8, q))
    rows[2, 2 * q:3 * q], rows[3, 2 * q:3 * q] = 0.0, rs.uniform(-6.0, -3.0, q)         # erfc where it is 2 less a few ulps
    r64 = rows.astype(np.float64)
    X64 = X.astype(np.float64)
    m, sg = _sp.gammaln(X64[:, :1] * r64[0] + r64[1]), _sp.erfc(X64[:, 1:] * r64[2] + r64[3])
    rows[y0:] = m + sg * np.stack([np.roll(grid_offsets(n), 5 * i) for i in range(N_PLATE)])

    def scores(r):
        a, b, c, d = r[0], r[1], r[2], r[3]
        with np.errstate(all="ignore"):
            m, sg = _sp.gammaln(X64[:, :1] * a + b), _sp.erfc(X64[:, 1:] * c + d)
            return np.stack([nlp(a, 0.0, 10.0), nlp(b, 0.0, 10.0), nlp(c, 0.0, 10.0), nlp(d, 0.0, 10.0), nlp(r[y0:], m, sg).sum(0)])
    return prog, rows, scores


def special_scan():
    """-> (program, restate(prog, choices64) -> (likelihood, prior) float64[K]).  64 rolled steps; the body holds a 3-operand log-sum-exp (the
    mean of x), an expm1 scale and a where-guarded lgamma (the mean of z).  The chain contracts (|x| stays below about 10 over 64 steps of
    4099 particles) and is continuous with bounded slopes — the guard opens at 1, where lgamma is 0: the two engines draw the same
    chain only up to the last bit of each step, and a slope like digamma's 1 / x at a guard opened at 0 turns that bit into 1e-3"""
    from genjax_amd import C
    ys = np.random.default_rng(64).standard_normal(T_SCAN).astype(F32)

    @genjax.gen
    def step(carry, _):
        xp, zp = carry
        x = genjax.normal(0.3 * genjax.logsumexp([xp, zp, -xp]), genjax.expm1(0.25 + 0.05 * genjax.square(zp))) @ "x"
        z = genjax.normal(genjax.where(xp > 1, 0.2 * genjax.lgamma(xp), 0.0), 0.5) @ "z"
        genjax.normal(x + z, 1.0) @ "y"
        return (x, z), None

    prog, _, _ = step.scan(n=T_SCAN).pack(((np.float32(0.4), np.float32(-0.2)), None), C["y"].set(ys), True, rng_mode=A.RNG_FLAT)

    def restate(prog, ch):
        x, z = (np.stack([ch[prog.slot_of[(k, t)]] for t in range(T_SCAN)]) for k in "xz")
        xp = np.concatenate([np.full((1, x.shape[1]), np.float64(F32(0.4))), x[:-1]])
        zp = np.concatenate([np.full((1, x.shape[1]), np.float64(F32(-0.2))), z[:-1]])
        with np.errstate(all="ignore"):
            mx, sx = 0.3 * _lse64([xp, zp, -xp]), np.expm1(0.25 + 0.05 * zp ** 2)
            mz = np.where(xp > 1, 0.2 * _sp.gammaln(np.where(xp > 1, xp, 1.0)), 0.0)
        prior = (nlp(x, mx, sx) + nlp(z, mz, 0.5)).sum(0)
        return nlp(ys[:, None].astype(np.float64), x + z, 1.0).sum(0), prior
    return prog, restate


# ---------------------------------------------------------------------------------------------------------------------------------
# the filter whose scanned DATA decides a node op
# ---------------------------------------------------------------------------------------------------------------------------------
def switching_filter(K_particles=1027):
    """x_t ~ normal(0.5 x_{t-1}, 0.3), y_t ~ normal(where(c_t > 0, exp(x_t^2), tanh(x_t^2)), 1): the scanned argument c_t is data, and the
    Python-level where() folds it into the step's node list"""
    from genjax_amd.inference.scan_filter import ScanBootstrapFilter

    @genjax.gen
    def step(x_prev, c_t):
        x = genjax.normal(0.5 * x_prev, 0.3) @ "x"
        genjax.normal(genjax.where(c_t > 0, genjax.exp(x * x), genjax.tanh(x * x)), 1.0) @ "y"
        return x, None
    return ScanBootstrapFilter(step.scan(n=4), K_particles)


REFRESH_YS = np.array([0.4, 1.2, 0.8, 1.1], np.float32)
REFRESH_CS = (np.array([1, 1, 1, 1], np.float32), np.array([1, -1, 1, -1], np.float32))
