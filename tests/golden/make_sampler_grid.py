"""Generates tests/golden/sampler_grid.json.gz (run by hand: python tests/golden/make_sampler_grid.py; no test imports this file).
The fixture is JSON, committed gzip-compressed (helpers.sampler_grid() reads it).

The truth behind tests/test_samplers_cpu.py and tests/test_gpu_samplers.py: for every SCALAR kind that elem_sample
(genjax_amd/csrc/gjx_device.h) switches on, 6 to 12 parameter rows — an ordinary point, both sides of every branch threshold of
the sampler (gamma shape 1, Poisson rate 10, von Mises concentration 1e-6), the float32 extremes (large rates and
concentrations, far and narrow truncation windows, tiny shapes) and, for the location/scale kinds, loc 1e4 with scale 1e-3 —
and per row the exact CDF at a fixed set of edges.  Parameters are rounded to float32 FIRST; the truth is taken at the rounded
values (TFP's parameter conventions, as in make_density_grid.py).

scipy's float64 CDFs are the truth where they keep their digits (about 1e-13; the bound they feed is never below 1e-6); mpmath at
50 digits where they do not: the truncated normal and Cauchy (differences of two nearly equal tail values).  The von Mises has
no closed form: its CDF is the integral of exp(k (cos t - 1)) by Gauss-Legendre on short pieces, held to mp.quad.  cross_check()
prints the stored values against mpmath at a sample of edges of every kind that has a closed form in mpmath.

Edge levels: 1e-4, 1e-3, 1e-2, j / 256 (j = 1 .. 255), 1 - 1e-2, 1 - 1e-3, 1 - 1e-4.  A continuous kind's edge is the level's
quantile rounded to float32, and F is the exact CDF AT the rounded edge; a discrete kind's edges are the integer quantiles,
deduplicated.  An edge is kept when
  * 0 < F < 1;
  * (continuous) it is float32-resolvable: the exact mass between its float32 neighbours is under a quarter of the bound the test
    applies there, 6 sqrt(F (1 - F) / M) + 1 / M, M = 2^20 draws per row;
  * it lies strictly inside (1.17549435e-38, inf) for the positive kinds and inside (1.17549435e-38, 1 - 2^-24) for the
    unit-interval kinds: the samplers clamp into those ranges, and an atom at a clamp value then never crosses an edge.
A candidate row whose exact distribution puts more than 1e-9 of its mass outside float32's finite range is not a row (printed).

Per kind: params (names), discrete, rows; per row:
  p        the parameters (float32 values)
  lv, e    kept edges: index into `levels` and the edge (the shortest decimal that reads back as the same float32)
  dF       F(e) - levels[lv], 3 digits (continuous: the quantile's rounding to float32, below 1e-7; F is exact to 1e-11 or better)
           discrete kinds store F itself ("F", 12 digits)
  x_lo, x_hi   guard quantiles at 1e-6 / M and 1 - 1e-6 / M, rounded outwards to float32 (the support's bound where it is bounded);
           null = unbounded on that side in float32
  lo, hi   the support (null = the real line on that side); lo_open / hi_open
  wrap     (von Mises) judge the difference to this loc wrapped into (-pi, pi]
"""
import gzip
import json
import math
import os
import sys

import mpmath as mp
import numpy as np
import scipy.special as sp
import scipy.stats as st

mp.mp.dps = 50
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
M = 1 << 20
TINY = 1.17549435e-38
F32_MAX = float(np.finfo(F).max)
ONE_M = 1.0 - 2.0 ** -24
LEVELS = [1e-4, 1e-3, 1e-2] + [j / 256.0 for j in range(1, 256)] + [1.0 - 1e-2, 1.0 - 1e-3, 1.0 - 1e-4]
Q_GUARD = 1e-6 / M
INF = float("inf")


def f32(v):
    return float(F(v))


def up32(v):
    return float(np.nextafter(F(v), F(np.inf)))


def dn32(v):
    return float(np.nextafter(F(v), F(-np.inf)))


def bound(Fv):
    return 6.0 * np.sqrt(Fv * (1.0 - Fv) / M) + 1.0 / M


class Dist:
    """cdf(x), sf(x) on float64 arrays, ppf(q), isf(q); support [lo, hi]"""

    def __init__(self, cdf, ppf, lo=-INF, hi=INF, sf=None, isf=None, discrete=False, lo_open=True, hi_open=True):
        self.cdf, self.ppf, self.lo, self.hi, self.discrete = cdf, ppf, lo, hi, discrete
        self.sf = sf or (lambda x: 1.0 - cdf(x))
        self.isf = isf or (lambda q: ppf(1.0 - q))
        self.lo_open, self.hi_open = lo_open, hi_open


def frozen(d, lo=-INF, hi=INF, discrete=False, **kw):
    return Dist(d.cdf, d.ppf, lo, hi, sf=d.sf, isf=d.isf, discrete=discrete, **kw)


def sg(l):
    return 1.0 / (1.0 + math.exp(-l))


# ---- mpmath truths: truncated normal / Cauchy, von Mises ---------------------------------------------------------------------------
def mp_Q(z):        # upper tail of the standard normal
    return mp.erfc(z / mp.sqrt(2)) / 2


class MpDist(Dist):
    """a distribution given by an mpmath CDF on [lo, hi]; edges by bisection in x on the exact CDF"""

    def __init__(self, cdf_mp, lo, hi, sf_mp=None):
        self.cdf_mp, self.sf_mp = cdf_mp, sf_mp or (lambda x: 1 - cdf_mp(x))
        Dist.__init__(self, lambda x: np.array([float(cdf_mp(mp.mpf(float(t)))) for t in np.atleast_1d(x)]), self._ppf, lo, hi,
                      sf=lambda x: np.array([float(self.sf_mp(mp.mpf(float(t)))) for t in np.atleast_1d(x)]), isf=self._isf,
                      lo_open=False, hi_open=False)

    def _solve(self, f, q, increasing):
        a, b = mp.mpf(self.lo), mp.mpf(self.hi)
        for _ in range(90):
            m = (a + b) / 2
            if (f(m) < q) == increasing:
                a = m
            else:
                b = m
        return float((a + b) / 2)

    def _ppf(self, q):
        return np.array([self._solve(self.cdf_mp, mp.mpf(float(t)), True) for t in np.atleast_1d(q)])

    def _isf(self, q):
        return np.array([self._solve(self.sf_mp, mp.mpf(float(t)), False) for t in np.atleast_1d(q)])


def truncated_normal(mu, sd, lo, hi):
    mu_, sd_, lo_, hi_ = (mp.mpf(t) for t in (mu, sd, lo, hi))
    zl, zh = (lo_ - mu_) / sd_, (hi_ - mu_) / sd_
    upper = zl + zh > 0
    mass = mp_Q(zl) - mp_Q(zh) if upper else mp_Q(-zh) - mp_Q(-zl)

    def cdf(x):
        z = (x - mu_) / sd_
        return ((mp_Q(zl) - mp_Q(z)) if upper else (mp_Q(-z) - mp_Q(-zl))) / mass

    def sf(x):
        z = (x - mu_) / sd_
        return ((mp_Q(z) - mp_Q(zh)) if upper else (mp_Q(-zh) - mp_Q(-z))) / mass
    return MpDist(cdf, lo, hi, sf)


def truncated_cauchy(mu, b, lo, hi):
    mu_, b_, lo_, hi_ = (mp.mpf(t) for t in (mu, b, lo, hi))
    al, ah = mp.atan((lo_ - mu_) / b_), mp.atan((hi_ - mu_) / b_)
    return MpDist(lambda x: (mp.atan((x - mu_) / b_) - al) / (ah - al), lo, hi, lambda x: (ah - mp.atan((x - mu_) / b_)) / (ah - al))


class VonMises(Dist):
    """the difference to loc on [-pi, pi] (symmetric: only [0, pi] is integrated).  No closed form: S(t) = P(d > t), t >= 0, is the
    integral of exp(k (cos s - 1)) over [t, pi] over the one over [0, pi], each summed piece by piece (64-point Gauss-Legendre in
    float64 on pieces no wider than half a standard deviation or pi / 64: the integrand is entire, the rule's error is far below
    1e-15 of a piece).  check() holds it to mp.quad at 30 digits."""
    GX, GW = np.polynomial.legendre.leggauss(64)

    def __init__(self, k):
        self.k = float(k)
        self.lo, self.hi, self.discrete, self.lo_open, self.hi_open = -math.pi, math.pi, False, False, False
        sd = 1.0 / math.sqrt(self.k) if self.k > 1.0 else math.pi
        cuts = np.concatenate([np.linspace(0.0, math.pi, 65), sd * np.arange(0.0, 60.0, 0.5)])
        self.cuts = np.unique(cuts[cuts <= math.pi])
        self.half = self._tail(0.0)

    def _piece(self, a, b):
        s = 0.5 * (b - a) * self.GX + 0.5 * (a + b)
        return 0.5 * (b - a) * float(np.dot(self.GW, np.exp(self.k * (np.cos(s) - 1.0))))

    def _tail(self, t):            # integral over [t, pi], smallest pieces first
        pts = np.concatenate([[t], self.cuts[self.cuts > t]])
        return math.fsum(self._piece(pts[i], pts[i + 1]) for i in range(len(pts) - 2, -1, -1))

    def _sf_pos(self, t):          # P(d > t), 0 <= t <= pi
        return self._tail(float(t)) / (2.0 * self.half)

    def cdf_small(self, x):        # P(d <= x) for x < 0 without 1 - (1 - small)
        return self._sf_pos(-float(x))

    def sf(self, x):
        return np.array([self._sf_pos(t) if t >= 0 else 1.0 - self._sf_pos(-t) for t in np.atleast_1d(x)])

    def cdf(self, x):
        return np.array([1.0 - self._sf_pos(t) if t >= 0 else self._sf_pos(-t) for t in np.atleast_1d(x)])

    def pdf(self, x):
        return math.exp(self.k * (math.cos(x) - 1.0)) / (2.0 * self.half)

    def guard(self, q):            # the exact upper q-quantile, by bisection on the tail integral
        a, b = 0.0, math.pi
        for _ in range(60):
            m = 0.5 * (a + b)
            if self._sf_pos(m) > q:
                a = m
            else:
                b = m
        return b

    def isf(self, q):              # edges only have to be NEAR the levels: scipy's float64 quantile; F is then exact AT the edge
        q = np.atleast_1d(np.asarray(q, np.float64))
        return math.pi * (1.0 - 2.0 * q) if self.k == 0 else st.vonmises(self.k).isf(q)

    def ppf(self, q):
        return -self.isf(q)

    def check(self, t):            # -> (this, mp.quad at 30 digits) for P(d > t)
        with mp.workdps(30):
            k = mp.mpf(self.k)
            g = lambda s: mp.exp(k * (mp.cos(s) - 1))
            sd = float(1 / mp.sqrt(k)) if self.k > 1 else math.pi
            pts = lambda a: [a] + [c for c in (sd * j for j in (1, 2, 4, 6, 8, 12, 20, 40)) if a < c < math.pi] + [mp.pi]
            return self._sf_pos(t), float(mp.quad(g, pts(mp.mpf(t))) / (2 * mp.quad(g, pts(mp.mpf(0)))))


# ---- the kinds -------------------------------------------------------------------------------------------------------------------
def geometric(p):
    l1 = math.log1p(-p) if p < 1.0 else -INF

    def cdf(k):
        return -np.expm1((np.floor(np.asarray(k, np.float64)) + 1.0) * l1)

    def sf(k):
        return np.exp((np.floor(np.asarray(k, np.float64)) + 1.0) * l1)

    def ppf(q):
        return np.maximum(np.ceil(np.log1p(-np.asarray(q, np.float64)) / l1 - 1e-12) - 1.0, 0.0)

    def isf(q):
        return np.maximum(np.ceil(np.log(np.asarray(q, np.float64)) / l1 - 1e-12) - 1.0, 0.0)
    return Dist(cdf, ppf, 0.0, INF, sf=sf, isf=isf, discrete=True, lo_open=False)


def bernoulli(p):
    return Dist(lambda x: np.where(np.asarray(x) >= 1.0, 1.0, 1.0 - p), lambda q: np.where(np.asarray(q) <= 1.0 - p, 0.0, 1.0), 0.0, 1.0,
                sf=lambda x: np.where(np.asarray(x) >= 1.0, 0.0, p), isf=lambda q: np.where(np.asarray(q) < p, 1.0, 0.0), discrete=True,
                lo_open=False, hi_open=False)


def transformed(base, fwd, inv, lo, hi, increasing=True, **kw):
    """x = fwd(y), y ~ base"""
    if increasing:
        return Dist(lambda x: base.cdf(inv(x)), lambda q: fwd(base.ppf(q)), lo, hi, sf=lambda x: base.sf(inv(x)), isf=lambda q: fwd(base.isf(q)), **kw)
    return Dist(lambda x: base.sf(inv(x)), lambda q: fwd(base.isf(q)), lo, hi, sf=lambda x: base.cdf(inv(x)), isf=lambda q: fwd(base.ppf(q)), **kw)


def folded(base, loc, scale):
    """loc + scale |y|, y ~ base symmetric about 0"""
    return Dist(lambda x: 1.0 - 2.0 * base.sf((np.asarray(x) - loc) / scale), lambda q: loc + scale * base.isf(0.5 * (1.0 - np.asarray(q))), loc, INF,
                sf=lambda x: 2.0 * base.sf((np.asarray(x) - loc) / scale), isf=lambda q: loc + scale * base.isf(0.5 * np.asarray(q)), lo_open=False)


def two_sided(base, loc, scale):
    """loc + scale s y, s = +-1, y ~ base >= 0"""
    def cdf(x):
        z = (np.asarray(x, np.float64) - loc) / scale
        return np.where(z < 0, 0.5 * base.sf(-z), 1.0 - 0.5 * base.sf(z))

    def sf(x):
        z = (np.asarray(x, np.float64) - loc) / scale
        return np.where(z < 0, 1.0 - 0.5 * base.sf(-z), 0.5 * base.sf(z))

    def ppf(q):
        q = np.asarray(q, np.float64)
        return np.where(q < 0.5, loc - scale * base.isf(np.minimum(2.0 * q, 1.0)), loc + scale * base.isf(np.minimum(2.0 * (1.0 - q), 1.0)))

    def isf(q):
        q = np.asarray(q, np.float64)
        return np.where(q < 0.5, loc + scale * base.isf(np.minimum(2.0 * q, 1.0)), loc - scale * base.isf(np.minimum(2.0 * (1.0 - q), 1.0)))
    return Dist(cdf, ppf, sf=sf, isf=isf)


def kumaraswamy(a, b):
    def cdf(x):
        return -np.expm1(b * np.log1p(-np.asarray(x, np.float64) ** a))

    def sf(x):
        return np.exp(b * np.log1p(-np.asarray(x, np.float64) ** a))

    def ppf(q):
        return (-np.expm1(np.log1p(-np.asarray(q, np.float64)) / b)) ** (1.0 / a)

    def isf(q):
        return (-np.expm1(np.log(np.asarray(q, np.float64)) / b)) ** (1.0 / a)
    return Dist(cdf, ppf, 0.0, 1.0, sf=sf, isf=isf)


def dist(kind, p):
    if kind in ("normal", "mv_normal_diag"):
        return frozen(st.norm(p[0], p[1]))
    if kind == "flip":
        return bernoulli(p[0])
    if kind == "bernoulli_logits":
        return bernoulli(sg(p[0]))
    if kind == "beta":
        return frozen(st.beta(p[0], p[1]), 0.0, 1.0)
    if kind == "uniform":
        return frozen(st.uniform(p[0], p[1] - p[0]), p[0], p[1], lo_open=False, hi_open=False)
    if kind == "exponential":
        return frozen(st.expon(scale=1.0 / p[0]), 0.0, INF, lo_open=False)
    if kind == "half_normal":
        return frozen(st.halfnorm(scale=p[0]), 0.0, INF, lo_open=False)
    if kind == "laplace":
        return frozen(st.laplace(p[0], p[1]))
    if kind == "log_normal":
        return frozen(st.lognorm(p[1], scale=math.exp(p[0])), 0.0, INF)
    if kind == "cauchy":
        return frozen(st.cauchy(p[0], p[1]))
    if kind == "gamma":
        return frozen(st.gamma(p[0], scale=1.0 / p[1]), 0.0, INF)
    if kind == "student_t":
        return frozen(st.t(p[0], p[1], p[2]))
    if kind == "half_student_t":
        return folded(st.t(p[0]), p[1], p[2])
    if kind == "truncated_normal":
        return truncated_normal(*p)
    if kind == "truncated_cauchy":
        return truncated_cauchy(*p)
    if kind == "poisson":
        return frozen(st.poisson(p[0]), 0.0, INF, discrete=True, lo_open=False)
    if kind == "geometric":
        return geometric(p[0])
    if kind == "gumbel":
        return frozen(st.gumbel_r(p[0], p[1]))
    if kind == "half_cauchy":
        return frozen(st.halfcauchy(p[0], p[1]), p[0], INF, lo_open=False)
    if kind == "inverse_gamma":
        return frozen(st.invgamma(p[0], scale=p[1]), 0.0, INF)
    if kind == "weibull":
        return frozen(st.weibull_min(p[0], scale=p[1]), 0.0, INF, lo_open=False)
    if kind == "logit_normal":
        return transformed(st.norm(p[0], p[1]), sp.expit, sp.logit, 0.0, 1.0)
    if kind == "chi2":
        return frozen(st.chi2(p[0]), 0.0, INF)
    if kind == "chi":
        return frozen(st.chi(p[0]), 0.0, INF)
    if kind == "exp_gamma":
        return transformed(st.gamma(p[0], scale=1.0 / p[1]), np.log, np.exp, -INF, INF)
    if kind == "exp_inverse_gamma":
        return transformed(st.invgamma(p[0], scale=p[1]), np.log, np.exp, -INF, INF)
    if kind == "kumaraswamy":
        return kumaraswamy(p[0], p[1])
    if kind == "moyal":
        return frozen(st.moyal(p[0], p[1]))
    if kind == "double_sided_maxwell":
        return two_sided(st.maxwell(), p[0], p[1])
    if kind == "inverse_gaussian":
        return frozen(st.invgauss(p[0] / p[1], scale=p[1]), 0.0, INF)
    if kind == "negative_binomial":
        return frozen(st.nbinom(p[0], sg(-p[1])), 0.0, INF, discrete=True, lo_open=False)
    if kind == "von_mises":
        return VonMises(p[1])
    raise KeyError(kind)


PARAMS = dict(
    normal=("loc", "scale"), mv_normal_diag=("loc", "scale"), flip=("p",), bernoulli_logits=("logits",), beta=("a", "b"),
    uniform=("low", "high"), exponential=("rate",), half_normal=("scale",), laplace=("loc", "scale"), log_normal=("loc", "scale"),
    cauchy=("loc", "scale"), gamma=("concentration", "rate"), student_t=("df", "loc", "scale"), half_student_t=("df", "loc", "scale"),
    truncated_normal=("loc", "scale", "low", "high"), truncated_cauchy=("loc", "scale", "low", "high"), poisson=("rate",),
    geometric=("p",), gumbel=("loc", "scale"), half_cauchy=("loc", "scale"), inverse_gamma=("concentration", "scale"),
    weibull=("concentration", "scale"), logit_normal=("loc", "scale"), chi2=("df",), chi=("df",), exp_gamma=("concentration", "rate"),
    exp_inverse_gamma=("concentration", "scale"), kumaraswamy=("a", "b"), moyal=("loc", "scale"), double_sided_maxwell=("loc", "scale"),
    inverse_gaussian=("loc", "concentration"), negative_binomial=("total_count", "logits"), von_mises=("loc", "concentration"))
POSITIVE = ("gamma", "exponential", "half_normal", "log_normal", "inverse_gamma", "weibull", "chi2", "chi", "inverse_gaussian")
UNIT = ("beta", "kumaraswamy", "logit_normal")
SHAPES = (0.01, 0.1, 0.99, 1.0, 1.01, 7.9, 8.0, 1e3, 1e5, 1e6)      # the gamma family (Marsaglia-Tsang: the boost below 1; the densities: 8)


def rows():
    R = {}
    ls = [(0.5, 2.0), (0.0, 1.0), (1e4, 1e-3), (-3.0, 1e-6), (0.0, 1e6), (1e6, 3.0)]
    for k in ("normal", "mv_normal_diag", "laplace", "cauchy", "gumbel", "moyal", "double_sided_maxwell"):
        R[k] = ls
    R["half_cauchy"] = ls
    R["log_normal"] = [(0.2, 0.4), (0.0, 1.0), (9.0, 1e-3), (-10.0, 1e-3), (0.0, 10.0), (3.0, 2.5)]
    R["logit_normal"] = [(0.1, 0.6), (0.0, 1.0), (-5.0, 3.0), (8.0, 0.5), (0.0, 1e-3), (0.0, 10.0)]
    R["uniform"] = [(-1.0, 3.0), (0.0, 1.0), (1e4, 1e4 + 1.0), (-1e6, 1e6), (0.0, 1e-6), (-2.0, -2.0 + 1e-6)]
    R["exponential"] = [(1.5,), (1.0,), (1e-6,), (1e6,), (1e-3,), (30.0,)]
    R["half_normal"] = [(1.0,), (0.8,), (1e-6,), (1e6,), (1e-3,), (30.0,)]
    R["gamma"] = [(2.5, 1.5), (0.6, 2.0)] + [(a, 1.0) for a in SHAPES]
    R["chi2"] = [(5.0,)] + [(2.0 * a,) for a in SHAPES]
    R["chi"] = [(3.0,)] + [(2.0 * a,) for a in SHAPES]
    R["inverse_gamma"] = [(3.0, 2.0)] + [(a, 2.0) for a in SHAPES]
    R["exp_gamma"] = [(2.5, 1.5)] + [(a, 1.5) for a in SHAPES]
    R["exp_inverse_gamma"] = [(3.0, 2.0)] + [(a, 2.0) for a in SHAPES]
    R["beta"] = [(2.0, 3.5), (0.01, 0.01), (0.1, 0.1), (0.5, 0.5), (0.99, 1.01), (1.0, 1.0), (7.9, 8.0), (1e3, 1e3), (1e5, 3.0), (1e6, 1e6), (0.1, 1e3)]
    R["student_t"] = [(4.0, 0.5, 1.5), (0.5, 0.0, 1.0), (1.0, 0.0, 1.0), (1.98, 0.0, 1.0), (2.0, 0.0, 1.0), (2.02, 0.0, 1.0), (16.0, 0.0, 1.0),
                      (1e3, 0.0, 1.0), (1e6, 0.0, 1.0), (4.0, 1e4, 1e-3), (0.05, 0.0, 1.0), (0.2, 0.0, 1.0)]
    R["half_student_t"] = [(5.0, 0.5, 1.5), (0.5, 0.0, 1.0), (1.0, 0.0, 1.0), (1.98, 0.0, 1.0), (2.0, 0.0, 1.0), (2.02, 0.0, 1.0), (16.0, 0.0, 1.0),
                           (1e3, 0.0, 1.0), (1e6, 0.0, 1.0), (4.0, 1e4, 1e-3), (0.2, 0.0, 1.0)]
    R["poisson"] = [(3.5,), (1e-3,), (0.5,), (9.99,), (10.0,), (30.0,), (1e3,), (1e5,), (1e6,), (1e7,)]
    R["negative_binomial"] = [(4.5, 0.3), (0.05, 0.0), (4.5, 8.0), (0.5, 12.0), (200.0, -3.0), (1.0, 2.0)]
    R["von_mises"] = [(0.7, 2.5), (0.0, 0.0), (0.0, 1e-7), (0.0, 9e-7), (0.0, 1e-6), (0.0, 1e-3), (-0.4, 0.3), (0.0, 50.0), (0.0, 300.0), (0.0, 1e3),
                      (0.0, 1e4), (0.0, 1e5), (0.7, 1e6)]
    wins = [(-1.0, 1.0), (-1e-3, 1e-3), (2.5, 6.0), (-6.0, -2.5), (-10.0, -8.0), (8.0, 10.0), (38.0, 40.0), (-40.0, -38.0), (5.0, 5.001), (-8.0, 0.5), (-12.0, 12.0)]
    R["truncated_normal"] = [(0.0, 1.0, lo, hi) for (lo, hi) in wins] + [(1e4, 1e-3, 1e4 + 2e-3, 1e4 + 8e-3)]
    R["truncated_cauchy"] = [(0.2, 1.5, -2.0, 3.0)] + [(0.0, 1.0, lo, hi) for (lo, hi) in
                                                       ((-1e-3, 1e-3), (250.0, 600.0), (-600.0, -250.0), (1e6, 1.25e6), (-1.25e6, -1e6), (5.0, 5.001), (-1e4, 0.5), (-1e8, 1e8))] + \
        [(1e4, 1e-3, 1e4 - 1.0, 1e4 + 1.0)]
    R["geometric"] = [(0.3,), (1e-6,), (1e-3,), (0.999,), (0.5,), (1.0,)]
    R["weibull"] = [(1.5, 2.0), (0.1, 1.0), (0.99, 1.0), (1.0, 1.0), (50.0, 1.0), (1.5, 1e-6), (0.02, 1.0)]
    R["kumaraswamy"] = [(2.0, 3.0), (0.05, 0.05), (50.0, 0.1), (1.0, 1.0), (0.5, 0.5), (0.1, 30.0)]
    R["inverse_gaussian"] = [(1.5, 4.0), (100.0, 0.01), (0.01, 100.0), (1e4, 1.0), (1.0, 1.0), (1e-3, 1e-6)]
    R["flip"] = [(0.3,), (0.0,), (1e-9,), (1.0,), (0.5,), (1.0 - 2.0 ** -24,)]
    R["bernoulli_logits"] = [(0.7,), (40.0,), (-40.0,), (0.0,), (-3.0,), (17.0,)]
    return R


def small_cdf(kind, d, x):
    """P(X <= x) where it is tiny, without 1 - (1 - small)"""
    if isinstance(d, VonMises) and x < 0:
        return d.cdf_small(x)
    return float(np.atleast_1d(d.cdf(x))[0])


def outside_float32(kind, d):
    """mass of the exact distribution outside float32's finite range"""
    m = 0.0
    if d.hi > F32_MAX:
        m += float(np.atleast_1d(d.sf(F32_MAX))[0])
    if d.lo < -F32_MAX:
        m += float(np.atleast_1d(d.cdf(-F32_MAX))[0])
    return m


def outward(v, sign):
    """v rounded to float32 away from the bulk; None when float32 has no finite value there"""
    if not math.isfinite(v) or abs(v) > F32_MAX:
        return None
    w = f32(v)
    if sign < 0 and w > v:
        w = dn32(w)
    if sign > 0 and w < v:
        w = up32(w)
    return w if abs(w) <= F32_MAX else None


def make_row(kind, p):
    p = tuple(f32(t) for t in p)
    d = dist(kind, p)
    if outside_float32(kind, d) > 1e-9:
        print("   not a row (mass outside float32):", kind, p, outside_float32(kind, d))
        return None
    wrap = kind == "von_mises"
    lv = np.asarray(LEVELS)
    row = dict(p=list(p))
    if d.discrete:
        e = np.unique(np.asarray(d.ppf(lv), np.float64))
        e = e[np.isfinite(e) & (e < 2.0 ** 24)]
        Fv = np.asarray(d.cdf(e), np.float64)
        keep = (Fv > 0.0) & (Fv < 1.0)
        row["e"] = [float(t) for t in e[keep]]
        row["F"] = [float("%.12g" % t) for t in Fv[keep]]
    else:
        q = np.where(lv < 0.5, lv, 1.0 - lv)
        raw = np.where(lv < 0.5, d.ppf(q), d.isf(q))
        idx, es, dFs = [], [], []
        for j, r in enumerate(raw):
            if not math.isfinite(r) or abs(r) > F32_MAX:
                continue
            e = f32(r)
            step = lambda v, fn: fn(v) if not wrap else v + (fn(abs(p[0]) + abs(v)) - (abs(p[0]) + abs(v)))     # (the draw is loc +- angle: loc's float32 step)
            eu, ed = step(e, up32), step(e, dn32)
            if not (d.lo < ed and eu < d.hi):
                continue
            if kind in POSITIVE and not e > TINY:
                continue
            if kind in UNIT and not (TINY < e < ONE_M):
                continue
            lower = lv[j] < 0.5
            f = (lambda x: small_cdf(kind, d, x)) if lower else (lambda x: float(np.atleast_1d(d.sf(x))[0]))
            Fe = f(e)
            between = d.pdf(e) * (eu - ed) if wrap else abs(f(eu) - f(ed))
            Fv = Fe if lower else 1.0 - Fe
            if not (0.0 < Fv < 1.0):
                continue
            if between >= 0.25 * bound(Fv):
                continue
            dF = (Fe - lv[j]) if lower else ((1.0 - lv[j]) - Fe)
            idx.append(j)
            es.append(float(str(F(e))))
            dFs.append(float("%.3g" % dF))
            assert F(es[-1]) == F(e)
        row.update(lv=idx, e=es, dF=dFs)
    # guards
    if wrap:
        hi_q = d.guard(Q_GUARD) if p[1] >= 1.0 else math.pi
        lo_q = -hi_q
    else:
        lo_q = float(np.atleast_1d(d.ppf(Q_GUARD))[0])
        hi_q = float(np.atleast_1d(d.isf(Q_GUARD))[0])
    lo_g = d.lo if math.isfinite(d.lo) else lo_q
    hi_g = d.hi if math.isfinite(d.hi) else hi_q
    if d.discrete:
        lo_g, hi_g = math.floor(lo_g), math.ceil(hi_g)
    row["x_lo"] = outward(lo_g, -1)
    row["x_hi"] = outward(hi_g, +1)
    row["lo"] = d.lo if math.isfinite(d.lo) else None
    row["hi"] = d.hi if math.isfinite(d.hi) else None
    row["lo_open"], row["hi_open"] = int(d.lo_open), int(d.hi_open)
    if wrap:
        row["wrap"] = p[0]
        row["x_lo"], row["x_hi"] = (-4.0, 4.0) if p[1] < 1.0 else (lo_q * (1 + 1e-6), hi_q * (1 + 1e-6))
        row["lo"], row["hi"] = -4.0, 4.0          # (the wrapped difference: always inside)
    return row


# ---- scipy against mpmath at a sample of edges (printed) --------------------------------------------------------------------------
def mp_cdf(kind, p, x):
    a = [mp.mpf(t) for t in p]
    x = mp.mpf(x)
    gP = lambda s, z: mp.gammainc(s, 0, z, regularized=True)
    N = lambda z: mp.erfc(-z / mp.sqrt(2)) / 2
    if kind in ("normal", "mv_normal_diag"):
        return N((x - a[0]) / a[1])
    if kind == "gamma":
        return gP(a[0], a[1] * x)
    if kind == "chi2":
        return gP(a[0] / 2, x / 2)
    if kind == "chi":
        return gP(a[0] / 2, x * x / 2)
    if kind == "inverse_gamma":
        return 1 - gP(a[0], a[1] / x)
    if kind == "exp_gamma":
        return gP(a[0], a[1] * mp.exp(x))
    if kind == "exp_inverse_gamma":
        return 1 - gP(a[0], a[1] * mp.exp(-x))
    if kind == "poisson":
        return mp.gammainc(mp.floor(x) + 1, a[0], mp.inf, regularized=True)
    if kind == "beta":
        return mp.betainc(a[0], a[1], 0, x, regularized=True)
    if kind == "negative_binomial":
        return mp.betainc(a[0], mp.floor(x) + 1, 0, 1 / (1 + mp.exp(a[1])), regularized=True)
    if kind == "student_t":
        z = (x - a[1]) / a[2]
        t = mp.betainc(a[0] / 2, mp.mpf(1) / 2, 0, a[0] / (a[0] + z * z), regularized=True) / 2
        return t if z < 0 else 1 - t
    if kind == "inverse_gaussian":
        mu, lam = a
        s = mp.sqrt(lam / x)
        return N(s * (x / mu - 1)) + mp.exp(2 * lam / mu + mp.log(N(-s * (x / mu + 1))))
    if kind == "weibull":
        return -mp.expm1(-(x / a[1]) ** a[0])
    if kind == "log_normal":
        return N((mp.log(x) - a[0]) / a[1])
    if kind == "cauchy":
        return mp.atan((x - a[0]) / a[1]) / mp.pi + mp.mpf(1) / 2
    if kind == "moyal":
        return mp.erfc(mp.exp(-(x - a[0]) / a[1] / 2) / mp.sqrt(2))
    if kind == "gumbel":
        return mp.exp(-mp.exp(-(x - a[0]) / a[1]))
    return None


def cross_check(out):
    worst = {}
    for row in out.get("von_mises", {}).get("rows", []):
        d = VonMises(row["p"][1])
        for t in (0.0, 0.5, 1.0, 3.0, 5.0):
            x = min(t / math.sqrt(max(d.k, 1.0)), 3.0)
            got, want = d.check(x)
            worst["von_mises"] = max(worst.get("von_mises", 0.0), abs(got - want) / bound(want))
    for kind, rec in out.items():
        for row in rec["rows"]:
            if mp_cdf(kind, row["p"], 1.0) is None:
                break
            Fs = row["F"] if rec["discrete"] else [LEVELS[j] + t for j, t in zip(row["lv"], row["dF"])]
            for i in range(0, len(Fs), 37):
                big = max(abs(t) for t in row["p"])
                if (big > 1e3 and kind in ("beta", "negative_binomial", "student_t")) or (big > 1e5 and i % 2):
                    continue       # (mpmath's hypergeometric series at such shapes take minutes: the gamma family alone goes on, every other sample)
                e = float(F(row["e"][i]))
                try:
                    t = mp_cdf(kind, row["p"], e)
                except (mp.libmp.NoConvergence, ValueError):
                    continue
                worst[kind] = max(worst.get(kind, 0.0), abs(float(t - mp.mpf(Fs[i]))) / bound(Fs[i]))
    print("cross-check, worst |stored F - mpmath| / bound per kind:", {k: float("%.3g" % v) for k, v in worst.items()})
    return {k: v for k, v in worst.items() if v > 1e-3}


def main():
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    R = rows()
    path = os.path.join(HERE, "sampler_grid.json.gz")
    out = {}
    if only and os.path.exists(path):
        out = json.load(gzip.open(path, "rt"))
        out.pop("levels", None), out.pop("M", None)
    for kind in R:
        if only and kind not in only:
            continue
        rs = [r for r in (make_row(kind, p) for p in R[kind]) if r is not None]
        out[kind] = dict(params=list(PARAMS[kind]), discrete=int(dist(kind, [f32(t) for t in R[kind][0]]).discrete), rows=rs)
        print(kind, len(rs), "rows,", sum(len(r["e"]) for r in rs), "edges", flush=True)
    out = dict(levels=LEVELS, M=M, **{k: out[k] for k in R if k in out})
    with open(path, "wb") as f, gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=f, mtime=0) as z:      # (mtime 0: same bytes every run)
        z.write(json.dumps(out, separators=(",", ":")).encode())
    print(os.path.getsize(path), "bytes", flush=True)
    assert os.path.getsize(path) < 400_000
    if "--no-check" not in sys.argv:
        bad = cross_check({k: out[k] for k in R if k in out})
        assert not bad, bad


if __name__ == "__main__":
    main()
