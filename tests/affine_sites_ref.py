"""Affine likelihoods `X v + b` on v_mfma_f32_16x16x4_f32, shape branch by shape branch: the case table, a float64 restatement of
every model and the error bounds, shared by tests/test_affine_sites_cpu.py (the CPU oracle, the paths through the emitted source, the
conditioning of the cases) and tests/test_gpu_affine_sites.py (the generated propagate kernel `emit_mfma_site`, the generated HMC
kernel `hmc_emit_mfma_site`, the hand-written k_hmc_logreg / k_hmc_logreg_mfma / k_hmc_logreg_mfma2).

A case is a SiteList with its observations (`Case.program()` packs it), the facts about its packed form that it is named for
(`Case.check_shape`: dim, p[0].n, p[0].len, p[0].off & 3, obs_off & 3, row tiles per trip) and the text its emitted kernel must hold.
Design of the data: rows of X have distinct norms (growing with the row), the bias is +-(1 + i / dim) with alternating sign, the
observations differ from row to row — a misplaced row, coefficient, bias entry or observation moves the result by far more than
the bound (test_affine_sites_cpu.py applies such misplacements to the restatement and asserts that).

What the packer cannot produce (PackedProgram.push aligns every table entry of 64 floats or more to 16 bytes):
  * a propagate site on the matrix cores has dim >= 64, so its observations and its vector bias are ALWAYS 16-byte aligned: the
    clamped per-row reads of `emit_mfma_site` are reached through ragged dims (65, 79, 200) only, never through `obs_off & 3` or
    `q.off & 3` — for a packed program; the two alignment terms are the guard of the b128 read for programs that reach the C
    interface from elsewhere, and one case (`relocated`) is such a program: a packed one whose observations and bias are copied to
    misaligned offsets at the end of the table, the site record pointed there;
  * in the generated HMC kernel the misaligned bias and observation reads are reached at dim = 48 (below 64 floats nothing is
    aligned): a small observed site of odd length in front shifts the offsets.
Kinds: the matrix-core flavour wants the AFFINE form in the FIRST parameter.  cauchy(loc, scale) has two parameters, so the third
and fourth constants come from student_t(df = X v + b, loc_i, scale_i) — second and third — and truncated_cauchy(loc = X v + b,
scale_i, low_i, high_i) — all four.

Bounds (none is a flat number; u = 2^-24, everything from the float64 reference, per column k):
  contraction   c_ik = 2 (n + 1) u (|b_i| + sum_j |X_ij| |v_jk|)     (2: the accumulation order inside the matrix instruction is not specified)
  element       e_ik = |l'(a_ik)| c_ik + C_ELEM u (1 + |l_ik|)       (l' by one-sided differences of the restatement: the larger side at a kink)
  site          sum_i e_ik + dim u sum_i |l_ik|
  a site without an affine form: the element term alone, plus |dl/dp| |p| C_ELEM u (1 + 2 |raw|) for a parameter p = exp(raw) or
  softplus(raw) of a value (the relative error of the transform: v_exp_f32 is evaluated as exp2 of a rounded product)
  total         sum of the sites' bounds + n_sites u sum |site scores|
  gradient      for a row term t_i (d l_i / d pre_i, or d l_i / d raw of a value parameter) entering slot j with weight X_ij (or 1):
                sum_i |X_ij| (|dt_i / dpre| c_ik + C_ELEM u (1 + |t_i|)) + (dim + 1) u sum_i |X_ij t_i|, the priors' own terms likewise,
                4 u sum |contributions| for adding them up, and the rounding of the recovery from two moves (recover_gradient):
                2 / (e1 - e2) (u |q1(e1)| / e1 + u |q1(e2)| / e2 + 2 u (P_MAX + e1 |g| / 2)),  P_MAX = 6 for standard-normal momenta.
C_ELEM is the one measured constant: the float32 oracle's worst element error against float64 at the same float32 logits over all
cases is C_ELEM_MEASURED in units of u (1 + |l|) (test_affine_sites_cpu.py measures it and asserts it is not above this record); the
device's v_exp_f32 / v_log_f32 / v_rcp_f32 are 1 ulp where libm is half an ulp and a density composes a few of them: C_ELEM = 4 x that.
Every bound is asserted (CPU test) to be no larger than the tolerance in force in the neighbouring tests: 2e-4 |ref| + 2e-2 for
scores, 2e-3 |ref| + 2e-3 for gradients — so these tests are never weaker than those.  For the 1000- and 1024-row logistic models
this needs gradients without cancellation (the backward sum's bound grows with sum |X_ij l'_i|): their rows carry the sign of their
observation, X_i = (2 y_i - 1) |X_i|, so that every row pulls the same way for every chain.
"""
import functools

import numpy as np
from scipy import special as sp

from genjax_amd import _abi as A
from genjax_amd.program import PackedProgram, Param, SiteList

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
C_ELEM_MEASURED = 2.5         # worst element error of the float32 oracle, units of u (1 + |l|): measured 2.31 (normal with an exp(ls) scale), rounded up
C_ELEM_FACTOR = 4.0
C_ELEM = C_ELEM_FACTOR * C_ELEM_MEASURED
P_MAX = 6.0                   # |momentum| of a standard-normal draw: 6 sigma
EPS1, EPS2 = 0.5, 0.25        # the two step sizes of the gradient recovery: exact in float32, and so are their halves
SCORE_RT, SCORE_AT = 2e-4, 2e-2          # test_gpu_codegen.py: the tolerance on the sums of a big affine site today
GRAD_RT, GRAD_AT = 2e-3, 2e-3            # helpers.py: the gradient tolerance of the float64 grid harness
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
MILD, WILD = 0.2, 3.0         # start states: mild chains, and every fourth chain scaled by 3 (saturated logits)


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def _sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def _xf(xf, raw):
    """-> (p, dp / draw)"""
    if xf == A.XF_NONE:
        return raw, np.ones_like(raw)
    if xf == A.XF_EXP:
        return np.exp(raw), np.exp(raw)
    if xf == A.XF_SOFTPLUS:
        return np.logaddexp(0.0, raw), _sigmoid(raw)
    raise ValueError(xf)


def logpdf(kind, x, p, grads=False):
    """float64 log-density of one element; with ``grads`` also (dl/dx, [dl/dp_k]) for the kinds an HMC case holds"""
    with np.errstate(all="ignore"):
        if kind in (A.NORMAL, A.MVNORMAL_DIAG):
            z = (x - p[0]) / p[1]
            l = -0.5 * z * z - np.log(p[1]) - HALF_LOG_2PI + 0.0 * x
            g = (-z / p[1], [z / p[1] + 0.0 * x, (z * z - 1.0) / p[1]])
        elif kind == A.BERNOULLI_LOGITS:       # -softplus(-a) y - softplus(a) (1 - y) for any y
            l = x * p[0] - np.logaddexp(0.0, p[0])
            g = (None, [x - _sigmoid(p[0])])
        elif kind == A.POISSON:
            l = np.where(x == 0.0, 0.0, x * np.log(p[0])) - p[0] - sp.gammaln(x + 1.0)
            l = np.where((x < 0.0) | (x != np.floor(x)), -np.inf, l)
            g = (None, [x / p[0] - 1.0])
        elif kind == A.HALF_NORMAL:
            z = x / p[0]
            l, g = np.where(x < 0.0, -np.inf, 0.5 * np.log(2.0 / np.pi) - np.log(p[0]) - 0.5 * z * z), None
        elif kind == A.LAPLACE:
            l, g = -np.abs(x - p[0]) / p[1] - np.log(2.0 * p[1]), None
        elif kind == A.CAUCHY:
            z = (x - p[0]) / p[1]
            l, g = -np.log(np.pi * p[1]) - np.log1p(z * z), None
        elif kind == A.STUDENT_T:              # p = df, loc, scale
            y = (x - p[1]) / p[2]
            l = (-0.5 * (p[0] + 1.0) * np.log1p(y * y / p[0]) - np.log(p[2]) - 0.5 * np.log(p[0] * np.pi)
                 + sp.gammaln(0.5 * (p[0] + 1.0)) - sp.gammaln(0.5 * p[0]))
            g = None
        elif kind == A.TRUNCATED_CAUCHY:       # p = loc, scale, low, high
            z = (x - p[0]) / p[1]
            l = -np.log(p[1]) - np.log1p(z * z) - np.log(np.arctan((p[3] - p[0]) / p[1]) - np.arctan((p[2] - p[0]) / p[1]))
            l, g = np.where((x < p[2]) | (x > p[3]), -np.inf, l), None
        else:
            raise ValueError(kind)
    return (l, g) if grads else l


class Ref:
    """the model of a SiteList in float64: the host-side description (matrices, biases, constants, observations) restated, nothing
    read from the packed table.  `vals`: {address: float64[dim][columns]} of the sites that are not observed from the table."""

    def __init__(self, sl, obs, selected=()):
        self.sites, self.selected = [], tuple(selected)
        for s in sl.sites:
            pars = [dict(op=p.op, xf=p.xf, src=p.src, length=p.length, values=None if p.values is None else np.asarray(p.values, F64).ravel(),
                         X=None if p.matrix is None else np.asarray(p.matrix, F64)) for p in s.params]
            y = np.broadcast_to(np.asarray(obs[s.addr], F32).astype(F64).ravel(), (s.dim,)).copy() if s.addr in obs else None
            self.sites.append(dict(addr=s.addr, kind=s.kind, dim=s.dim, pars=pars, obs=y))
        # an affine form over n values reads n consecutive rows of choices[][] from its source's first: with more than 32 inputs these
        # are the rows of several sites (a generated kernel keeps latent sites of at most 32 elements)
        latent = [s for s in sl.sites if s.addr not in obs]
        for s in self.sites:
            for q in s["pars"]:
                if q["op"] == A.P_AFFINE:
                    j, q["srcs"] = [t.addr for t in latent].index(q["src"]), []
                    while sum(d for _, d in q["srcs"]) < q["X"].shape[1]:
                        q["srcs"].append((latent[j].addr, latent[j].dim))
                        j += 1
                    assert sum(d for _, d in q["srcs"]) == q["X"].shape[1]

    def affine_sites(self):
        return [s for s in self.sites if s["pars"][0]["op"] == A.P_AFFINE]

    def copy(self):
        import copy
        return copy.deepcopy(self)

    @staticmethod
    def _raw(par, vals):
        if par["op"] == A.P_CONST:
            return par["values"][:, None]
        if par["op"] == A.P_VALUE:
            assert par["length"] == 1
            return vals[par["src"]][:1]
        if par["op"] == A.P_AFFINE:
            return par["X"] @ Ref._inputs(par, vals) + (par["values"] if par["values"].size > 1 else np.full(par["X"].shape[0], par["values"][0]))[:, None]
        raise ValueError(par["op"])

    @staticmethod
    def _inputs(par, vals):
        return np.concatenate([vals[a] for a, _ in par["srcs"]], 0)

    def _x(self, s, vals):
        return s["obs"][:, None] if s["obs"] is not None else vals[s["addr"]]

    def elements(self, s, vals, pre=None):
        """-> (l [dim][cols], raws, (dl/dx, [dl/draw_k]) or None); ``pre``: the affine parameter's contraction given instead of computed"""
        raws = [self._raw(q, vals) for q in s["pars"]]
        if pre is not None:
            raws[0] = pre
        pd = [_xf(q["xf"], r) for q, r in zip(s["pars"], raws)]
        l, g = logpdf(s["kind"], self._x(s, vals), [p for p, _ in pd], grads=True)
        if g is not None:
            g = (g[0], [gk * d for gk, (_, d) in zip(g[1], pd)])
        return l, raws, g

    def site_scores(self, vals):
        """float64[n_sites][cols]"""
        n = next(iter(vals.values())).shape[1]
        return np.stack([np.broadcast_to(self.elements(s, vals)[0], (s["dim"], n)).sum(0) for s in self.sites])

    def gradient(self, vals):
        """{selected address: d score / d value, float64[dim][cols]} — analytic"""
        n = next(iter(vals.values())).shape[1]
        g = {a: np.zeros((vals[a].shape[0], n)) for a in self.selected}
        for s in self.sites:
            _, _, d = self.elements(s, vals)
            assert d is not None, s["kind"]
            if s["obs"] is None and s["addr"] in g:
                g[s["addr"]] += np.broadcast_to(d[0], (s["dim"], n))
            for q, dk in zip(s["pars"], d[1]):
                if q["op"] == A.P_CONST:
                    continue
                dk = np.broadcast_to(dk, (s["dim"], n))
                if q["op"] == A.P_AFFINE:
                    for (a, d), lo in zip(q["srcs"], np.cumsum([0] + [d for _, d in q["srcs"]])):
                        if a in g:
                            g[a] += q["X"][:, lo:lo + d].T @ dk
                elif q["src"] in g:
                    g[q["src"]] += dk.sum(0, keepdims=True)
        return g

    # ---- bounds -------------------------------------------------------------------------------------------------------------
    def _contraction(self, s, vals):
        """c_ik of the affine first parameter (0 for a site without one), and the float64 contraction"""
        q = s["pars"][0]
        if q["op"] != A.P_AFFINE:
            return None, None
        b = q["values"] if q["values"].size > 1 else np.full(q["X"].shape[0], q["values"][0])
        c = 2.0 * (q["X"].shape[1] + 1) * U * (np.abs(b)[:, None] + np.abs(q["X"]) @ np.abs(self._inputs(q, vals)))
        return c, self._raw(q, vals)

    def _d_dpre(self, s, vals, pre, f):
        """|d f / d pre| by one-sided differences (the larger side: at a kink of the density the steeper slope)"""
        h = 2.0 ** -20 * (1.0 + np.abs(pre))
        with np.errstate(all="ignore"):
            f0, fp, fm = f(pre), f(pre + h), f(pre - h)
            d = np.maximum(np.abs(fp - f0), np.abs(f0 - fm)) / h
        return np.where(np.isfinite(d), d, 0.0)

    def _param_terms(self, s, vals, l):
        """a parameter given as a TRANSFORM of a value (exp(log_tau)): C_ELEM u (1 + 2 |raw|) relative, through |dl/dp| |p|"""
        out = 0.0
        if any(q["op"] == A.P_VALUE and q["xf"] != A.XF_NONE for q in s["pars"]):
            _, raws, d = self.elements(s, vals)
            for q, r, dk in zip(s["pars"], raws, d[1]):
                if q["op"] == A.P_VALUE and q["xf"] != A.XF_NONE:     # dk = dl/draw = dl/dp p for exp; for softplus |dl/dp| p >= |dk| is not needed here
                    out = out + np.abs(dk) * C_ELEM * U * (1.0 + 2.0 * np.abs(r))
        return out

    def score_bounds(self, vals):
        """-> (site bounds float64[n_sites][cols], bound of the total [cols])"""
        n = next(iter(vals.values())).shape[1]
        out, mags = [], []
        for s in self.sites:
            l = np.broadcast_to(self.elements(s, vals)[0], (s["dim"], n))
            lf = np.where(np.isfinite(l), l, 0.0)
            e = C_ELEM * U * (1.0 + np.abs(lf)) + self._param_terms(s, vals, l)
            c, pre = self._contraction(s, vals)
            if c is not None:
                e = e + self._d_dpre(s, vals, pre, lambda t, s=s: self.elements(s, vals, pre=t)[0]) * c
            out.append(np.broadcast_to(e, (s["dim"], n)).sum(0) + s["dim"] * U * np.abs(lf).sum(0))
            mags.append(np.abs(lf.sum(0)))
        out = np.stack(out)
        return out, out.sum(0) + len(self.sites) * U * np.sum(mags, 0)

    def gradient_bounds(self, vals):
        """{selected address: bound of the device's gradient, float64[dim][cols]} — without the recovery's rounding"""
        n = next(iter(vals.values())).shape[1]
        b = {a: np.zeros((vals[a].shape[0], n)) for a in self.selected}
        mag = {a: np.zeros((vals[a].shape[0], n)) for a in self.selected}
        for s in self.sites:
            _, raws, d = self.elements(s, vals)
            c, pre = self._contraction(s, vals)
            rel = 1.0
            for q, r in zip(s["pars"], raws):
                if q["op"] == A.P_VALUE and q["xf"] != A.XF_NONE:
                    rel = rel + 2.0 * np.abs(r)
            terms = []
            if s["obs"] is None and s["addr"] in b:
                terms.append((s["addr"], None, 0))
            for k, q in enumerate(s["pars"]):
                if q["op"] == A.P_AFFINE:
                    for (a, dd), lo in zip(q["srcs"], np.cumsum([0] + [dd for _, dd in q["srcs"]])):
                        if a in b:
                            terms.append((a, dict(q, X=q["X"][:, lo:lo + dd]), k + 1))
                elif q["op"] != A.P_CONST and q["src"] in b:
                    terms.append((q["src"], q, k + 1))
            for addr, q, which in terms:
                pick = (lambda dd, which=which: dd[0] if which == 0 else dd[1][which - 1])
                t = np.broadcast_to(pick(d), (s["dim"], n))
                e = C_ELEM * U * (1.0 + np.abs(t)) * rel
                if c is not None:
                    e = e + self._d_dpre(s, vals, pre, lambda x, s=s, pick=pick: np.broadcast_to(pick(self.elements(s, vals, pre=x)[2]), (s["dim"], n))) * c
                if q is not None and q["op"] == A.P_AFFINE:
                    aX = np.abs(q["X"])
                    b[addr] += aX.T @ e + (s["dim"] + 1) * U * (aX.T @ np.abs(t))
                    mag[addr] += np.abs(q["X"].T @ t)
                elif q is not None:
                    b[addr] += e.sum(0, keepdims=True) + (s["dim"] + 1) * U * np.abs(t).sum(0, keepdims=True)
                    mag[addr] += np.abs(t.sum(0, keepdims=True))
                else:
                    b[addr] += e
                    mag[addr] += np.abs(t)
        return {a: b[a] + 4.0 * U * mag[a] for a in b}


def recover_gradient(q0, q1a, q1b):
    """the device's gradient at q0 from two moves of ONE leapfrog step with the same key (same momenta p): q1(e) = q0 + e (p + e g / 2),
    d(e) = (q1(e) - q0) / e = p + e g / 2, so g = 2 (d(e1) - d(e2)) / (e1 - e2).  float64 arithmetic on the float32 results."""
    q0, q1a, q1b = (np.asarray(t, F64) for t in (q0, q1a, q1b))
    return 2.0 * ((q1a - q0) / EPS1 - (q1b - q0) / EPS2) / (EPS1 - EPS2)


def recovery_rounding(q1a, q1b, g):
    """what the float32 roundings of the leapfrog step (p + e/2 g, then q0 + e p) leave in recover_gradient"""
    return 2.0 / (EPS1 - EPS2) * (U * np.abs(q1a) / EPS1 + U * np.abs(q1b) / EPS2 + 2.0 * U * (P_MAX + EPS1 * np.abs(g) / 2.0))


def recovery_rounding_worst(q0, g):
    """the same before any move is made: |q1(e)| <= |q0| + e (P_MAX + e |g| / 2)"""
    q1 = lambda e: np.abs(q0) + e * (P_MAX + e * np.abs(g) / 2.0)      # noqa: E731
    return recovery_rounding(q1(EPS1), q1(EPS2), g)


def prop_reference(case, prog, choices):
    """float64 at the float32 choices a propagate run returned -> dict(site, site_bound [n_sites][K]; score, weight and their bounds [K]):
    the weight of a run whose latents are sampled from the prior is the sum of the observed sites' scores"""
    vals = values_of(prog, choices)
    ss = case.ref.site_scores(vals)
    sb, tb = case.ref.score_bounds(vals)
    ob = np.array([s.addr in case.obs for s in prog.site_list.sites])
    return dict(site=ss, site_bound=sb, score=ss.sum(0), score_bound=tb, weight=ss[ob].sum(0),
                weight_bound=sb[ob].sum(0) + ob.sum() * U * np.abs(ss[ob]).sum(0))


def hmc_reference(case, prog, q0):
    """float64 at a float32 chain state -> dict(score, score_bound [n]; grad, grad_bound [selected scalars][n], rows in the order of
    case.selected) — grad_bound without the recovery's rounding"""
    vals = values_of(prog, q0)
    ss = case.ref.site_scores(vals)
    _, tb = case.ref.score_bounds(vals)
    return dict(score=ss.sum(0), score_bound=tb, grad=stack_selected(prog, case.selected, case.ref.gradient(vals)),
                grad_bound=stack_selected(prog, case.selected, case.ref.gradient_bounds(vals)))


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the finite references; where the reference is +-inf the device must return the same infinity"""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    inf = np.isinf(want)
    assert (got[inf] == want[inf]).all() and not np.isnan(want).any() and not np.isnan(got).any()
    r = np.abs(got - want)[~inf] / np.broadcast_to(bound, want.shape)[~inf]
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------
def design(dim, n, seed, positive=False):
    """[dim][n] float32: entries of size 1 / sqrt(n) (an order-one contraction), row i scaled by 0.6 + 0.8 i / dim (distinct norms)"""
    z = np.random.default_rng(seed).standard_normal((dim, n))
    z = np.abs(z) if positive else z
    return (z * ((0.6 + 0.8 * np.arange(dim) / dim) / np.sqrt(n))[:, None]).astype(F32)


def bias_vector(dim):
    i = np.arange(dim)
    return (np.where(i % 2 == 0, 1.0, -1.0) * (1.0 + i / dim)).astype(F32)


def binary(dim, seed):
    return (np.random.default_rng(seed).random(dim) < 0.5).astype(F32)


def spread(dim, seed, width=1.5):
    """observations that differ from row to row: a fixed pattern of width `width` plus noise"""
    return (width * np.sin(1.0 + 0.7 * np.arange(dim)) + 0.3 * np.random.default_rng(seed).standard_normal(dim)).astype(F32)


def start_state(case, prog, n, seed):
    """float32[n_slots][n]: mild chains (scale 0.2); in every fourth chain, chain 0 included, the inputs of the affine forms are scaled
    by 3 instead, so that logits saturate.  The log-scale latents (log_tau, ls) stay mild in every chain: at exp(-9) the gradient is
    1e8 times a difference of order-one terms, and no bound that float32 can meet stays under 2e-3 |ref| + 2e-3 there."""
    q = np.random.default_rng(seed).standard_normal((prog.n_slots, n)) * MILD
    for a, d in sorted({t for s in case.ref.affine_sites() for t in s["pars"][0]["srcs"]}):
        q[prog.slot_of[a]:prog.slot_of[a] + d, ::4] *= WILD / MILD
    return q.astype(F32)


def values_of(prog, ch):
    """{address: float64 rows} of a choices array"""
    ch = np.asarray(ch, F64)
    return {s.addr: ch[prog.slot_of[s.addr]:prog.slot_of[s.addr] + s.dim] for s in prog.site_list.sites if prog.slot_of[s.addr] >= 0}


def selected_slots(prog, selected):
    return np.concatenate([np.arange(prog.slot_of[a], prog.slot_of[a] + prog.site_list[a].dim) for a in selected])


def stack_selected(prog, selected, d):
    return np.concatenate([d[a] for a in selected], 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
class Case:
    """name, family ("prop" | "gen" | "fused"), the site list with its observations, and what the packed program must look like:
    expect = dict(site, dim, n, bias = "scalar" | "aligned" | "misaligned", obs = "aligned" | "misaligned", tb, ...)"""

    def __init__(self, name, family, sl, obs, expect, selected=(), env=None, sampled=(), engine=None, text=(), relocate=False):
        self.name, self.family, self.sl, self.obs, self.expect, self.selected = name, family, sl, obs, expect, tuple(selected)
        self.relocate = relocate
        self.env, self.sampled, self.engine, self.text = dict(env or {}), tuple(sampled), engine, tuple(text)
        self.ref = Ref(sl, obs, selected)

    @functools.lru_cache(maxsize=None)
    def program(self, rng=A.RNG_FLAT):
        modes = {s.addr: (A.MODE_OBS_TAB if s.addr in self.obs else A.MODE_OBS_SLOT) for s in self.sl.sites if s.addr not in self.sampled}
        prog = PackedProgram(self.sl, modes, self.obs, selected=self.selected, rng_mode=rng)
        if self.relocate:
            # what the packer never produces, as a program built against the C interface may hold it: the observations and the vector
            # bias of "y" copied to the end of the table at offsets that are 1 and 2 mod 4, the site record pointed there
            j = [s.addr for s in prog.site_list.sites].index("y")
            cs, dim = prog.c_sites[j], prog.site_list["y"].dim
            y, b = prog.tab[cs.obs_off:cs.obs_off + dim].copy(), prog.tab[cs.p[0].off:cs.p[0].off + dim].copy()
            base = (prog.tab.size + 3) & ~3
            cs.obs_off, cs.p[0].off = base + 1, base + 1 + dim + (1 + (4 - (1 + dim) % 4)) % 4 + 1
            prog.obs_off["y"] = cs.obs_off
            tab = np.zeros(cs.p[0].off + dim, F32)
            tab[:prog.tab.size] = prog.tab
            tab[cs.obs_off:cs.obs_off + dim], tab[cs.p[0].off:cs.p[0].off + dim] = y, b
            prog.tab = tab
        return prog

    def check_shape(self):
        """the packed program has the shape and the alignment the case is named for"""
        prog, e = self.program(), self.expect
        for site, dim, n, bias, obs_al in e["sites"]:
            j = [s.addr for s in prog.site_list.sites].index(site)
            cs = prog.c_sites[j]
            q = cs.p[0]
            assert (cs.dim, q.op, q.n, q.moff & 3) == (dim, A.P_AFFINE, n, 0), (self.name, cs.dim, q.op, q.n, q.moff)
            assert q.len == (1 if bias == "scalar" else dim), (self.name, q.len)
            if bias != "scalar":
                assert ((q.off & 3) == 0) == (bias == "aligned"), (self.name, "bias offset", q.off)
            assert ((cs.obs_off & 3) == 0) == (obs_al == "aligned"), (self.name, "obs_off", cs.obs_off)
            assert cs.mode == A.MODE_OBS_TAB and cs.slot < 0
        if "tb" in e:
            dim = e["sites"][0][1]
            tb = 4 if dim % 64 == 0 else (2 if dim % 32 == 0 else 1)
            assert tb == e["tb"], (self.name, tb)
        if "ragged" in e:
            assert e["sites"][0][1] % 16 == e["ragged"], self.name


def _pad(sl, obs, k, observed):
    """a small site of odd length in front: its constants (and, observed, its value) shift every later table offset by an odd count"""
    sl.add("pad", A.NORMAL, [Param.const(np.linspace(-0.3, 0.3, k).astype(F32)), Param.const(np.full(k, 1.5, F32))], dim=k)
    if observed:
        obs["pad"] = np.linspace(0.2, 0.4, k).astype(F32)


def _latents(sl, name, n, make):
    """n latent values as sites of at most 32 elements in consecutive rows (name, name1): what an affine form over n > 32 inputs reads"""
    out = []
    for k, lo in enumerate(range(0, n, 32)):
        m = min(32, n - lo)
        kind, params = make(m)
        sl.add(name + (str(k) if k else ""), kind, params, dim=m)
        out.append(name + (str(k) if k else ""))
    return tuple(out)


def _saturate(X, rows30, rows100):
    """scale rows so that their logits reach about +-30 and +-100"""
    X = X.copy()
    for rows, to in ((rows30, 30.0), (rows100, 100.0)):
        for i in rows:
            X[i] *= F32(to / 1.2)
    return X


def _prop_case(name, kind, dim, n, bias, seed, pad=0, saturated=False, y03=False, sd=1.0, relocate=False):
    sl, obs = SiteList(), {}
    if pad:
        _pad(sl, obs, pad, False)
    positive = kind in (A.POISSON, A.STUDENT_T)
    lat = _latents(sl, "beta", n, (lambda m: (A.HALF_NORMAL, [Param.const(sd)])) if positive else (lambda m: (A.NORMAL, [Param.const(0.0), Param.const(sd)])))
    X = design(dim, n, seed, positive)
    if saturated:
        X = _saturate(X, (1, dim // 2, dim - 1) if kind == A.NORMAL else (1, dim // 2), (4, dim - 3))
    bv = bias_vector(dim)
    if positive:
        bv = np.abs(bv) + F32(0.5)
    b = bv if bias == "vector" else F32(0.7)
    i = np.arange(dim)
    rs = np.random.default_rng(seed + 100)
    per_row = (0.6 + 0.9 * ((7 * i) % dim) / dim).astype(F32)       # a second parameter of length dim: distinct per row
    aff = Param.affine(X, "beta", bias=b)
    if kind == A.NORMAL:
        params, y = [aff, Param.const(F32(2.0) if saturated else (per_row if bias == "vector" else F32(0.7)))], spread(dim, seed + 1)
    elif kind == A.BERNOULLI_LOGITS:
        params, y = [aff], binary(dim, seed + 1)
        if y03:
            y[dim // 3] = F32(0.3)
    elif kind == A.POISSON:
        params, y = [aff], rs.poisson(2.0 + (i % 5), dim).astype(F32)        # (values from 7 on take the large-count form of the density)
    elif kind == A.LAPLACE:
        X[3], X[dim - 6] = 0.0, 0.0                                          # rows whose location IS their bias: observed exactly there
        aff = Param.affine(X, "beta", bias=b)
        y = spread(dim, seed + 1)
        y[3], y[dim - 6] = np.broadcast_to(b, (dim,))[3], np.broadcast_to(b, (dim,))[dim - 6]
        params = [aff, Param.const(per_row)]
    elif kind == A.CAUCHY:
        params, y = [aff, Param.const(per_row)], spread(dim, seed + 1, 3.0)
    elif kind == A.STUDENT_T:      # df = X beta + b > 0; location and scale per row: the second and third constants
        params, y = [aff, Param.const((0.5 * bias_vector(dim)).astype(F32)), Param.const(per_row)], spread(dim, seed + 1, 5.0)      # (in the tails: there the density feels df)
    elif kind == A.TRUNCATED_CAUCHY:   # scale, low, high per row: second, third and fourth constants; every observation inside its window
        y = spread(dim, seed + 1, 2.0)
        params = [aff, Param.const(per_row), Param.const((y - 1.0 - per_row).astype(F32)), Param.const((y + 0.5 + 2.0 * per_row).astype(F32))]
    else:
        raise ValueError(kind)
    sl.add("y", kind, params, dim=dim)
    obs["y"] = y
    al = "misaligned" if relocate else "aligned"
    expect = dict(sites=[("y", dim, n, "scalar" if bias == "scalar" else al, al)], tb=4 if dim % 64 == 0 else (2 if dim % 32 == 0 else 1))
    if dim % 16:
        expect["ragged"] = dim % 16
    text = [f"kind {kind}, {dim} rows x {n} coefficients on the matrix cores"]
    return Case(name, "prop", sl, obs, expect, sampled=lat + (("pad",) if pad else ()), text=text, relocate=relocate)


@functools.lru_cache(maxsize=None)
def prop_cases():
    N, B, Po, L, Ca, St, TC = A.NORMAL, A.BERNOULLI_LOGITS, A.POISSON, A.LAPLACE, A.CAUCHY, A.STUDENT_T, A.TRUNCATED_CAUCHY
    cs = [
        _prop_case("normal_64x16_scalar_bias", N, 64, 16, "scalar", 11),                        # TB 4, scalar scale
        _prop_case("normal_96x32_vector_bias_row_scale", N, 96, 32, "vector", 12, pad=5),        # TB 2, b128 bias, scale of length dim
        _prop_case("bernoulli_80x48_vector_bias", B, 80, 48, "vector", 13),                      # TB 1 on an aligned dim, 3 b128 reads per row
        _prop_case("bernoulli_80x48_vector_bias_relocated", B, 80, 48, "vector", 13, relocate=True),   # aligned dim, misaligned bias and observations
        _prop_case("bernoulli_65x64_vector_bias_y03", B, 65, 64, "vector", 14, pad=3, y03=True),  # ragged 1: clamped bias and observation reads
        _prop_case("poisson_79x16_scalar_bias", Po, 79, 16, "scalar", 15),                       # ragged 15
        _prop_case("laplace_200x32_vector_bias", L, 200, 32, "vector", 16),                      # 13 tiles, ragged 8, kink at the location
        _prop_case("cauchy_64x48_scalar_bias", Ca, 64, 48, "scalar", 17),
        _prop_case("student_t_96x64_vector_bias", St, 96, 64, "vector", 18, pad=7),              # 4 b128 reads per row; second and third constants
        _prop_case("truncated_cauchy_80x16_vector_bias", TC, 80, 16, "vector", 19),              # second, third and fourth constants
        _prop_case("normal_64x32_saturated", N, 64, 32, "vector", 20, saturated=True),
        _prop_case("bernoulli_64x16_saturated", B, 64, 16, "scalar", 21, saturated=True),
        _prop_case("bernoulli_79x32_saturated_y03", B, 79, 32, "vector", 22, saturated=True, y03=True),
    ]
    return {c.name: c for c in cs}


PROP_KS = (256, 512)                    # the matrix-core flavour: whole blocks of four waves
PROP_SCALAR_K = 300                     # not a multiple of 256: the scalar flavour of the same program
PROP_BOTH_RNG = "normal_64x16_scalar_bias"


def _gen_case(name, what, dim, n, bias, seed, pad=0, pad_observed=False, y03=False, env=None, select=None):
    """what: "bernoulli" | "poisson_softplus" | "normal_exp_ls" | "unselected" | "two_sites" """
    sl, obs = SiteList(), {}
    if pad:
        _pad(sl, obs, pad, pad_observed)
    X = design(dim, n, seed)
    b = bias_vector(dim) if bias != "scalar" else F32(0.7)
    sel, sites = ["w"], []
    bias_kind = "scalar" if bias == "scalar" else bias
    if what in ("normal_exp_ls", "unselected"):
        sl.add("ls", A.NORMAL, [-0.3, 0.4])
        sel = ["ls", "w"]
    lat = _latents(sl, "w", n, lambda m: (A.MVNORMAL_DIAG, [Param.const(np.zeros(m, F32)), Param.const(np.full(m, 0.8, F32))]))
    # (the register form of the generated HMC kernel — the one with a matrix-core flavour — holds at most 48 selected values:
    # with 64 inputs `select` names the 32-element chunks that move, the others are values of the chain the move leaves alone)
    sel = sel[:-1] + [a for k, a in enumerate(lat) if select is None or k in select]
    if what == "bernoulli":
        y = binary(dim, seed + 1)
        if y03:
            y[dim // 3] = F32(0.3)
        sl.add("y", A.BERNOULLI_LOGITS, [Param.affine(X, "w", bias=b)], dim=dim)
    elif what == "poisson_softplus":
        y = np.random.default_rng(seed + 1).poisson(1.0 + (np.arange(dim) % 4), dim).astype(F32)
        sl.add("y", A.POISSON, [Param.affine(X, "w", bias=b, xf=A.XF_SOFTPLUS)], dim=dim)
    elif what == "normal_exp_ls":
        y = spread(dim, seed + 1)
        sl.add("y", A.NORMAL, [Param.affine(X, "w", bias=b), Param.value("ls", xf=A.XF_EXP)], dim=dim)
    elif what == "unselected":        # the affine's inputs are values of the chain that the move leaves alone: no backward contraction
        y = spread(dim, seed + 1)
        sl.add("y", A.NORMAL, [Param.affine(X, "w", bias=b), Param.value("ls", xf=A.XF_EXP)], dim=dim)
        sel = ["ls"]
    elif what == "two_sites":         # two likelihoods over ONE stored copy of X (PackedProgram shares the matrix)
        y = binary(dim, seed + 1)
        sl.add("y", A.BERNOULLI_LOGITS, [Param.affine(X, "w", bias=b)], dim=dim)
        sl.add("y2", A.NORMAL, [Param.affine(X, "w", bias=F32(-0.4)), Param.const(F32(0.8))], dim=dim)
        obs["y2"] = spread(dim, seed + 2)
    else:
        raise ValueError(what)
    obs["y"] = y
    obs_al = "misaligned" if (pad_observed and dim < 64) else "aligned"
    sites.append(("y", dim, n, bias_kind, obs_al))
    if what == "two_sites":
        sites.append(("y2", dim, n, "scalar", "aligned"))
    tb = 4 if dim % 64 == 0 else (2 if dim % 32 == 0 else 1)
    env = dict(env or {})
    folded = what == "bernoulli" and not y03 and "GJX_HMC_GEN_NO_FOLD" not in env
    line = f"{dim} rows x {n} inputs on the matrix cores, {tb} row tiles per trip"
    text = [line + ("; rows and bias carry the observation's sign" if folded else "\n")]
    return Case(name, "gen", sl, obs, dict(sites=sites, tb=tb, folded=folded, n_mfma=len(sites)), selected=sel, env=env, engine=4, text=text)


@functools.lru_cache(maxsize=None)
def gen_cases():
    nf = {"GJX_HMC_GEN_NO_FOLD": "1"}
    cs = [
        _gen_case("bernoulli_48x16_scalar_bias_folded", "bernoulli", 48, 16, "scalar", 31),                       # TB 1, NB 1
        _gen_case("bernoulli_64x48_vector_bias_folded", "bernoulli", 64, 48, "aligned", 32),                      # TB 4, NB 3, folded bias vector
        _gen_case("bernoulli_48x32_misaligned_bias_folded", "bernoulli", 48, 32, "misaligned", 33, pad=3),        # the fold reads a misaligned bias
        _gen_case("bernoulli_48x32_misaligned_bias_no_fold", "bernoulli", 48, 32, "misaligned", 33, pad=3, env=nf),   # the unaligned bias read
        _gen_case("bernoulli_64x48_vector_bias_no_fold", "bernoulli", 64, 48, "aligned", 32, env=nf),             # b128 bias, y128 observations
        _gen_case("bernoulli_96x64_vector_bias_y03", "bernoulli", 96, 64, "aligned", 34, y03=True, select=(1,)),   # TB 2, NB 4, fold off by the data; inputs 32..63 move
        _gen_case("bernoulli_48x16_scalar_bias_y03_misaligned_obs", "bernoulli", 48, 16, "scalar", 35, pad=3, pad_observed=True, y03=True),
        _gen_case("poisson_48x32_softplus", "poisson_softplus", 48, 32, "scalar", 36),                            # a transform on the contraction
        _gen_case("normal_96x16_exp_ls_vector_bias", "normal_exp_ls", 96, 16, "aligned", 37),                     # a second value parameter
        _gen_case("normal_48x64_exp_ls_misaligned", "normal_exp_ls", 48, 64, "misaligned", 38, pad=5, pad_observed=True, select=(0,)),   # n = 64, inputs 0..31 move
        _gen_case("normal_64x16_inputs_not_selected", "unselected", 64, 16, "scalar", 39),
        _gen_case("two_sites_64x32_shared_matrix", "two_sites", 64, 32, "aligned", 40),
    ]
    return {c.name: c for c in cs}


GEN_CHAINS = (1, 17, 300)


def logreg_case(P, N, bias="none", mean="scalar", y03=False, env=None, seed=0):
    """workloads.logreg_program's shape with the options it does not have: a scalar or vector bias, a vector prior mean, an
    observation that is not 0 / 1:  log_tau ~ N(0, 1);  beta ~ N(mu, exp(log_tau));  y ~ bernoulli(logits = X beta + b)"""
    name = f"logreg_P{P}_N{N}_bias_{bias}_mean_{mean}" + ("_y03" if y03 else "") + ("".join("_" + k[4:].lower() + v for k, v in (env or {}).items()))
    y = binary(N, 50 + seed + N + P)
    X = design(N, P, 60 + seed + N + P)
    if N >= 1000:      # no cancellation in the backward sum (module docstring)
        X = (np.abs(X) * (2.0 * y - 1.0)[:, None]).astype(F32)
    if y03:
        y[N // 3] = F32(0.3)
    sl = SiteList()
    sl.add("log_tau", A.NORMAL, [0.0, 1.0])
    mu = Param.const(0.0) if mean == "scalar" else Param.const((0.5 * bias_vector(P)).astype(F32))
    sl.add("beta", A.NORMAL, [mu, Param.value("log_tau", xf=A.XF_EXP)], dim=P)
    aff = Param.affine(X, "beta") if bias == "none" else Param.affine(X, "beta", bias=F32(0.7) if bias == "scalar" else bias_vector(N))
    sl.add("y", A.BERNOULLI_LOGITS, [aff], dim=N)
    env = dict(env or {})
    engine = 3 if (P == 16 and env.get("GJX_HMC_MFMA") != "0") else 2
    expect = dict(sites=[("y", N, P, "scalar" if bias != "vector" else ("aligned" if N >= 64 else None), "aligned" if N >= 64 else None)],
                  mu_len=1 if mean == "scalar" else P)
    return Case(name, "fused", sl, {"y": y}, expect, selected=("log_tau", "beta"), env=env, engine=engine)


@functools.lru_cache(maxsize=None)
def fused_cases():
    cs = [
        logreg_case(16, 1), logreg_case(16, 15, "scalar"), logreg_case(16, 16, "vector"), logreg_case(16, 17, "vector", "vector"),
        logreg_case(16, 33, "none", y03=True), logreg_case(16, 64, "scalar", y03=True), logreg_case(16, 1000, "vector", "vector"),
        logreg_case(16, 1024),                                   # the two-group kernel, its NP = 1024 specialisation
        logreg_case(16, 1024, "vector"),                         # Npad = 1024 with a bias: NOT the zero-bias specialisation
        logreg_case(16, 1024, "scalar", "vector", y03=True),     # BIN = false
        logreg_case(16, 1024, env={"GJX_HMC_NO_MFMA2": "1"}),    # k_hmc_logreg_mfma<BIN, NP = 1024>
        logreg_case(16, 33, "vector", "vector", env={"GJX_HMC_MFMA": "0"}),      # P = 16 on the vector kernel
        logreg_case(16, 1000, "scalar", env={"GJX_HMC_MFMA": "0"}),
        logreg_case(2, 17, "vector", "vector"), logreg_case(2, 64),
        logreg_case(4, 15, "scalar"), logreg_case(4, 33, "vector", y03=True),
        logreg_case(8, 16, "none", "vector"), logreg_case(8, 1000, "vector"),
        logreg_case(32, 17, "vector", "vector"), logreg_case(32, 64, "scalar", y03=True),
    ]
    return {c.name: c for c in cs}


def fused_shape(case):
    """the packed logistic program has the fields match_logreg reads: bias length, prior-mean length, row and input counts"""
    prog = case.program()
    (_, N, P, bias, _), = case.expect["sites"]
    y, beta = prog.c_sites[2], prog.c_sites[1]
    assert (y.dim, y.p[0].n, beta.dim, beta.p[0].len) == (N, P, P, case.expect["mu_len"]), case.name
    assert y.p[0].len == (N if "bias_vector" in case.name else 1) and prog.n_slots == 1 + P
    return prog


# ---------------------------------------------------------------------------------------------------------------------------------
# the misplacements an indexing bug would make, applied to the restatement (test_affine_sites_cpu.py: each must move the result by
# more than 10 x the bound on at least half the columns)
# ---------------------------------------------------------------------------------------------------------------------------------
def misplacements(ref):
    """-> {name: Ref with the first affine site's inputs misplaced}; a misplacement that is the identity for this case is left out"""
    out = {}
    s0 = ref.affine_sites()[0]
    j = [s["addr"] for s in ref.sites].index(s0["addr"])
    X, b, y = s0["pars"][0]["X"], s0["pars"][0]["values"], s0["obs"]
    dim, n = X.shape

    def variant(name, X2=None, b2=None, y2=None, same=False):
        if same:
            return
        r = ref.copy()
        s = r.sites[j]
        if X2 is not None:
            s["pars"][0]["X"] = X2
        if b2 is not None:
            s["pars"][0]["values"] = b2
        if y2 is not None:
            s["obs"] = y2
        out[name] = r

    zero_last = X.copy()
    zero_last[-1] = 0.0
    # a dropped row adds nothing: its X row, bias and the density itself vanish — restated as a model of dim - 1 rows
    r = ref.copy()
    s = r.sites[j]
    s["dim"] = dim - 1
    s["pars"][0]["X"] = X[:-1]
    if b.size > 1:
        s["pars"][0]["values"] = b[:-1]
    s["obs"] = y[:-1]
    for q in s["pars"][1:]:
        if q["op"] == A.P_CONST and q["values"].size == dim:
            q["values"] = q["values"][:-1]
    out["last row dropped"] = r
    r = ref.copy()
    s = r.sites[j]
    s["dim"] = dim + 1
    s["pars"][0]["X"] = np.concatenate([X, X[-1:]])
    if b.size > 1:
        s["pars"][0]["values"] = np.concatenate([b, b[-1:]])
    s["obs"] = np.concatenate([y, y[-1:]])
    for q in s["pars"][1:]:
        if q["op"] == A.P_CONST and q["values"].size == dim:
            q["values"] = np.concatenate([q["values"], q["values"][-1:]])
    out["last row counted twice"] = r
    for step, label in ((4, "j and j + 4"), (n // 4, "j and j + n / 4")):
        if step >= 1 and 1 + step < n:
            Xs = X.copy()
            Xs[:, [1, 1 + step]] = Xs[:, [1 + step, 1]]
            variant(f"coefficients {label} swapped", X2=Xs, same=(label == "j and j + n / 4" and n // 4 == 4))
    if b.size > 1:
        variant("bias shifted by one row", b2=np.roll(b, 1))
        variant("bias[0] for every row", b2=np.full(dim, b[0]))
    if dim > 1:
        variant("observations shifted by one", y2=np.roll(y, 1), same=bool((np.roll(y, 1) == y).all()))
    for jj, s in enumerate(ref.sites):
        q = s["pars"][0]
        if s["kind"] == A.NORMAL and s["obs"] is None and q["op"] == A.P_CONST and q["values"].size > 1 and s["addr"] in ref.selected:
            r = ref.copy()
            r.sites[jj]["pars"][0]["values"] = np.full(1, 0.0)
            out["scalar prior mean for the vector one"] = r
    return out
