"""The 25 older expression node ops (include/gjx.h GJX_E_CONST .. GJX_E_LINN) at their edges: the programs, their grids and a
float64 NumPy restatement, shared by tests/test_gpu_expr_ops.py (generated kernels, site interpreter) and tests/test_expr_ops_cpu.py
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


def _grad_of(grid, **kw):
    return lambda n: grid(n, **kw)


SPECS = {
    "unary": Spec(UN_LAT, UN_SITES, _un_grid, _un_grad_grid, UN_OPS),
    "binary": Spec(BIN_LAT, BIN_SITES, _bin_grid, _bin_grad_grid, BIN_OPS),
    "powers": Spec(POW_LAT, POW_SITES, _pow_grid, _pow_grid, POW_OPS),
    "guards": Spec(GUARD_LAT, GUARD_SITES, _guard_grid, _grad_of(_guard_grid, boundary=True), GUARD_OPS),
    "linear": Spec(LIN_LAT, LIN_SITES, _lin_grid, _grad_of(_lin_grid, gaps=True), LIN_OPS),
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
