"""Program builders shared by the CPU and GPU tests."""
import functools
import gzip
import json
import os

import numpy as np

from genjax_amd import _abi as A
from genjax_amd.program import PackedProgram, Param, SiteList
from genjax_amd import workloads as W

KIND = dict(normal=A.NORMAL, flip=A.FLIP, bernoulli_logits=A.BERNOULLI_LOGITS, beta=A.BETA, uniform=A.UNIFORM,
            exponential=A.EXPONENTIAL, half_normal=A.HALF_NORMAL, laplace=A.LAPLACE, log_normal=A.LOG_NORMAL,
            cauchy=A.CAUCHY, gamma=A.GAMMA, mv_normal_diag=A.MVNORMAL_DIAG, student_t=A.STUDENT_T,
            truncated_normal=A.TRUNCATED_NORMAL, poisson=A.POISSON, geometric=A.GEOMETRIC, dirichlet=A.DIRICHLET, gumbel=A.GUMBEL,
            half_cauchy=A.HALF_CAUCHY, inverse_gamma=A.INVERSE_GAMMA, weibull=A.WEIBULL, logit_normal=A.LOGIT_NORMAL, chi2=A.CHI2,
            chi=A.CHI, exp_gamma=A.EXP_GAMMA, exp_inverse_gamma=A.EXP_INVERSE_GAMMA, half_student_t=A.HALF_STUDENT_T, kumaraswamy=A.KUMARASWAMY,
            moyal=A.MOYAL, truncated_cauchy=A.TRUNCATED_CAUCHY, double_sided_maxwell=A.DOUBLESIDED_MAXWELL, inverse_gaussian=A.INVERSE_GAUSSIAN,
            negative_binomial=A.NEGATIVE_BINOMIAL, von_mises=A.VON_MISES)
NPAR = dict(normal=2, flip=1, bernoulli_logits=1, beta=2, uniform=2, exponential=1, half_normal=1, laplace=2,
            log_normal=2, cauchy=2, gamma=2, mv_normal_diag=2, student_t=3, truncated_normal=4, poisson=1, geometric=1,
            dirichlet=1, gumbel=2, half_cauchy=2, inverse_gamma=2, weibull=2, logit_normal=2, chi2=1,
            chi=1, exp_gamma=2, exp_inverse_gamma=2, half_student_t=3, kumaraswamy=2, moyal=2, truncated_cauchy=4, double_sided_maxwell=2,
            inverse_gaussian=2, negative_binomial=2, von_mises=2)


def one_site(kind: str, a, b=None, obs=None, rng=A.RNG_FLAT, c=None, d=None):
    sl = SiteList()
    params = [a, b, c, d][: NPAR[kind]]
    sl.add("v", KIND[kind], params)
    if obs is None:
        return PackedProgram(sl, rng_mode=rng)
    return PackedProgram(sl, {"v": A.MODE_OBS_TAB}, {"v": obs}, rng_mode=rng)


VECTOR_KINDS = ("dirichlet",)          # (with the categoricals: their own tables, not tests/golden/density_grid.json.gz)


@functools.lru_cache(maxsize=None)
def density_grid():
    """tests/golden/density_grid.json.gz (tests/golden/make_density_grid.py): {kind: record of arrays}, read once and left unchanged"""
    with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "density_grid.json.gz"), "rt") as f:
        return json.load(f)


def density_grid_program(kind: str):
    """One row of density_grid() per particle: a carrier site p_i ~ uniform(-1e37, 1e37) per parameter (its own
    gradient is 0, so its gradient row holds d/d(parameter) alone) and x ~ KIND(p0, ...), every site MODE_OBS_SLOT.  Selected for
    gradients: every site but a discrete x.  -> (program, slot of x, slots of the parameters, index of x's site)"""
    n = NPAR[kind]
    sl = SiteList()
    for j in range(n):
        sl.add(f"p{j}", A.UNIFORM, [-1e37, 1e37])
    sl.add("x", KIND[kind], [Param.value(f"p{j}") for j in range(n)])
    addrs = [f"p{j}" for j in range(n)] + ["x"]
    sel = tuple(a for a in addrs if a != "x" or KIND[kind] not in A.NO_GRADIENT_KINDS)
    prog = PackedProgram(sl, {a: A.MODE_OBS_SLOT for a in addrs}, selected=sel)
    return prog, prog.slot_of["x"], [prog.slot_of[f"p{j}"] for j in range(n)], n


def density_grid_choices(rec, prog, x_slot, p_slots):
    """the rows of one kind's record as particles: choices[slot][row]"""
    ch = np.zeros((max(prog.n_slots, 1), len(rec["x"])), np.float32)
    ch[x_slot] = np.asarray(rec["x"], np.float64)
    for j, s in enumerate(p_slots):
        ch[s] = np.asarray(rec["p"][j], np.float64)
    return ch


def density_grid_truth(rec):
    """-> dict(lp [rows] (-inf outside the support), k_lp, grads {name: (truth with NaN where not asserted, kappa)}); "x" first, then
    "p0".. in parameter order"""
    f = lambda a: np.array([np.nan if v is None else v for v in a], np.float64)
    lp = np.where(np.asarray(rec["neg_inf"], bool), -np.inf, f(rec["lp"]))
    grads = {"x": (f(rec["dx"]), f(rec["k_dx"]))}
    for j in range(len(rec["p"])):
        grads[f"p{j}"] = (f(rec["dp"][j]), f(rec["k_dp"][j]))
    return dict(lp=lp, k_lp=f(rec["k_lp"]), grads=grads)


def density_grid_excess(got, want, kappa, at, rt):
    """|got - want| / (at + rt |want| + 2 kappa) per row: the float tolerance plus the conditioning term (a kernel that forms (x - mu) / sd
    or b x - a with one or two roundings answers for inputs a float32 step away; 2 = one step in each of two inputs).  Rows where
    `want` is -inf must be -inf exactly (excess 0 or inf); rows where `want` is NaN are not asserted (excess 0); a NaN in `got`
    anywhere else is inf."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.abs(got - want) / (at + rt * np.abs(want) + 2.0 * np.asarray(kappa, np.float64))
    r = np.where(np.isneginf(want), np.where(np.isneginf(got), 0.0, np.inf), r)
    r = np.where(np.isnan(want), 0.0, r)
    return np.where(np.isnan(r), np.inf, r)


def density_grid_rows(rec, rows, got=None):
    """readable list of rows (for assertion messages): x, parameters[, what the code gave]"""
    return [(i, rec["x"][i], tuple(c[i] for c in rec["p"])) + (() if got is None else (float(got[i]),)) for i in rows]


def gmm(D=16, C=8, rng=A.RNG_FLAT, seed=0):
    return W.gmm_program(D, C, rng, seed)


def flip_flip(trivial: bool, rng=A.RNG_FLAT):
    """tests/inference/test_smc.py:32-87 of the reference."""
    sl = SiteList()
    sl.add("x", A.FLIP, [0.5])
    sl.add("y", A.FLIP, [0.7] if trivial else [Param.gather(np.array([0.3, 0.9], np.float32), "x")])
    return PackedProgram(sl, {"y": A.MODE_OBS_TAB}, {"y": 1.0}, rng_mode=rng)


def beta_bernoulli(obs: bool, rng=A.RNG_FLAT):
    """README.md:89-102 of the reference."""
    sl = SiteList()
    sl.add("p", A.BETA, [2.0, 2.0])
    sl.add("v", A.FLIP, [Param.value("p")])
    return PackedProgram(sl, {"v": A.MODE_OBS_TAB}, {"v": float(obs)}, rng_mode=rng)


def zoo(rng=A.RNG_FLAT, observed=()):
    """One site of every distribution kind, chained through every parameter-expression form."""
    sl = SiteList()
    sl.add("n0", A.NORMAL, [0.5, 2.0])
    sl.add("f0", A.FLIP, [0.3])
    sl.add("c0", A.CATEGORICAL_PROBS, [np.array([0.2, 0.5, 0.3], np.float32)])
    sl.add("n1", A.NORMAL, [Param.gather(np.array([-1.0, 0.0, 4.0], np.float32), "c0"), Param.value("n0", xf=A.XF_EXP)])
    sl.add("b0", A.BETA, [2.0, 3.5])
    sl.add("f1", A.FLIP, [Param.value("b0")])
    sl.add("u0", A.UNIFORM, [-1.0, 3.0])
    sl.add("bl", A.BERNOULLI_LOGITS, [Param.affine(np.array([[0.7]], np.float32), "u0", bias=-0.2)])
    sl.add("mv", A.MVNORMAL_DIAG, [np.array([0.0, 1.0, 2.0], np.float32), np.array([1.0, 0.5, 2.0], np.float32)], dim=3)
    sl.add("mv2", A.MVNORMAL_DIAG, [Param.affine(np.array([[1, 0, 1], [0, 2, 0]], np.float32), "mv", bias=[0.1, -0.1]),
                                    Param.const([0.7])], dim=2)
    sl.add("e0", A.EXPONENTIAL, [1.5])
    sl.add("h0", A.HALF_NORMAL, [Param.value("e0", xf=A.XF_SOFTPLUS)])
    sl.add("l0", A.LAPLACE, [Param.value("h0"), 0.8])
    sl.add("ln", A.LOG_NORMAL, [0.2, 0.4])
    sl.add("ca", A.CAUCHY, [Param.value("ln"), 2.0])
    sl.add("g0", A.GAMMA, [2.5, 1.5])
    sl.add("g1", A.GAMMA, [0.6, 2.0])
    sl.add("cl", A.CATEGORICAL_LOGITS, [Param.affine(np.array([[1.0], [0.0], [-1.0], [0.5]], np.float32), "n0")])
    sl.add("n2", A.NORMAL, [Param.value("ca", xf=A.XF_SIGMOID), 0.3])
    obs_vals = dict(n2=0.4, mv2=[0.3, 1.9], f1=1.0, l0=0.9)
    modes = {a: A.MODE_OBS_TAB for a in observed}
    return PackedProgram(sl, modes, {a: obs_vals[a] for a in observed}, rng_mode=rng)


def logreg(N=64, P=4, rng=A.RNG_FLAT, seed=0):
    return W.logreg_program(N, P, rng, seed)


def zoo2(rng=A.RNG_FLAT, observed=()):
    """The wider distribution set, one site per kind, chained through parameter forms."""
    sl = SiteList()
    sl.add("t0", A.STUDENT_T, [4.0, 0.5, 1.5])
    sl.add("tn", A.TRUNCATED_NORMAL, [Param.value("t0", xf=A.XF_SIGMOID), 0.8, -0.5, 2.0])
    sl.add("po", A.POISSON, [3.5])
    sl.add("pl", A.POISSON, [Param.value("tn", xf=A.XF_EXP)])
    sl.add("pb", A.POISSON, [40.0])                                    # transformed-rejection branch
    sl.add("ge", A.GEOMETRIC, [0.3])
    sl.add("di", A.DIRICHLET, [np.array([0.8, 2.0, 3.0], np.float32)], dim=3)
    sl.add("gu", A.GUMBEL, [Param.value("di", length=1, elem=1), 0.7])
    sl.add("hc", A.HALF_CAUCHY, [0.0, Param.value("gu", xf=A.XF_SOFTPLUS)])
    sl.add("ig", A.INVERSE_GAMMA, [3.0, 2.0])
    sl.add("we", A.WEIBULL, [1.5, Param.value("ig")])
    sl.add("lo", A.LOGIT_NORMAL, [Param.affine(np.array([[0.1]], np.float32), "po"), 0.6])
    sl.add("c2", A.CHI2, [5.0])
    sl.add("t1", A.STUDENT_T, [3.0, Param.value("lo"), Param.value("c2", xf=A.XF_SOFTPLUS)])
    sl.add("tr", A.TRUNCATED_NORMAL, [0.0, 1.0, 2.5, 6.0])            # far upper tail
    sl.add("n9", A.NORMAL, [Param.value("t1", xf=A.XF_SIGMOID), 0.3])
    obs_vals = dict(n9=0.4, di=[0.2, 0.3, 0.5], po=2.0, tn=0.7)
    modes = {a: A.MODE_OBS_TAB for a in observed}
    return PackedProgram(sl, modes, {a: obs_vals[a] for a in observed}, rng_mode=rng)


def zoo3(rng=A.RNG_FLAT, observed=()):
    """Nine more of the reference's TFP wrappers (round 6: chi, exp_gamma, exp_inverse_gamma, half_student_t, kumaraswamy, moyal,
    truncated_cauchy, double_sided_maxwell, inverse_gaussian), one site per kind plus chained copies through parameter forms."""
    sl = SiteList()
    sl.add("ch", A.CHI, [3.0])
    sl.add("eg", A.EXP_GAMMA, [2.5, 1.5])
    sl.add("ei", A.EXP_INVERSE_GAMMA, [3.0, 2.0])
    sl.add("hs", A.HALF_STUDENT_T, [5.0, 0.5, 1.5])
    sl.add("ku", A.KUMARASWAMY, [2.0, 3.0])
    sl.add("mo", A.MOYAL, [0.3, 0.8])
    sl.add("tc", A.TRUNCATED_CAUCHY, [0.2, 1.5, -2.0, 3.0])
    sl.add("dm", A.DOUBLESIDED_MAXWELL, [0.4, 0.7])
    sl.add("ig", A.INVERSE_GAUSSIAN, [1.5, 4.0])
    # chained: parameters that are values of earlier choices (under transforms that keep them in their domains)
    sl.add("ch2", A.CHI, [Param.value("ig", xf=A.XF_SOFTPLUS)])
    sl.add("eg2", A.EXP_GAMMA, [Param.value("ch"), Param.value("eg", xf=A.XF_EXP)])
    sl.add("ei2", A.EXP_INVERSE_GAMMA, [9.5, Param.value("ku", xf=A.XF_EXP)])                 # (concentration >= 8: the big-shape branch)
    sl.add("hs2", A.HALF_STUDENT_T, [Param.value("ch", xf=A.XF_SOFTPLUS), Param.value("mo"), Param.value("ig")])
    sl.add("ku2", A.KUMARASWAMY, [Param.value("ch"), Param.value("hs")])
    sl.add("mo2", A.MOYAL, [Param.value("dm"), Param.value("ku", xf=A.XF_SOFTPLUS)])
    sl.add("tc2", A.TRUNCATED_CAUCHY, [Param.value("mo", xf=A.XF_SIGMOID), Param.value("ch"), -1.0, 4.0])
    sl.add("dm2", A.DOUBLESIDED_MAXWELL, [Param.value("tc"), Param.value("ku", xf=A.XF_EXP)])
    sl.add("ig2", A.INVERSE_GAUSSIAN, [Param.value("ch"), Param.value("eg", xf=A.XF_EXP)])
    sl.add("nb", A.NEGATIVE_BINOMIAL, [4.5, 0.3])
    sl.add("vm", A.VON_MISES, [0.7, 2.5])
    sl.add("vs", A.VON_MISES, [-0.4, 0.3])                                                     # (small concentration: nearly uniform)
    sl.add("vb", A.VON_MISES, [Param.value("mo", xf=A.XF_SIGMOID), Param.value("ch", xf=A.XF_EXP)])   # (concentration up to exp(3))
    sl.add("nb2", A.NEGATIVE_BINOMIAL, [Param.value("ch"), Param.value("vm")])
    sl.add("n9", A.NORMAL, [Param.value("ig2", xf=A.XF_SIGMOID), 0.3])
    obs_vals = dict(n9=0.4, ku=0.35, mo=0.9, ig=1.1)
    modes = {a: A.MODE_OBS_TAB for a in observed}
    return PackedProgram(sl, modes, {a: obs_vals[a] for a in observed}, rng_mode=rng)


def shape_hierarchy(rng=A.RNG_FLAT):
    """a model whose SHAPE parameters are latent (gradients through them need digamma): log-normal hyper-parameters
    feeding gamma / beta concentrations, student-t / chi2 degrees of freedom and the inverse-gamma concentration"""
    from genjax_amd.program import PackedProgram, Param, SiteList
    sl = SiteList()
    sl.add("la", A.NORMAL, [0.3, 0.25])
    sl.add("lb", A.NORMAL, [0.1, 0.25])
    a, b = Param.value("la", xf=A.XF_EXP), Param.value("lb", xf=A.XF_EXP)
    sl.add("g", A.GAMMA, [a, b])
    sl.add("be", A.BETA, [a, b])
    sl.add("t", A.STUDENT_T, [Param.value("la", xf=A.XF_SOFTPLUS), 0.2, b])
    sl.add("ig", A.INVERSE_GAMMA, [a, 1.5])
    sl.add("c2", A.CHI2, [Param.value("lb", xf=A.XF_SOFTPLUS)])
    return sl


def scan_chain(T, rng=A.RNG_FLAT, carry=True, observe=False, sigma=0.1, r=0.5, seed=0, scan_id=0):
    """A Scan of T steps laid out as the host tracer does (gen.py ScanCombinator): step t holds x_t ~ N(x_{t-1}, sigma)
    (x_{-1} = 0; independent N(0, 1) draws without `carry`) and, with `observe`, y_t ~ N(x_t, r) constrained to data;
    every site of step t carries the tag GJX_SCAN_TAG(scan_id, t)."""
    rs = np.random.default_rng(seed)
    sl = SiteList()
    modes, obs = {}, {}
    ys = rs.standard_normal(T).astype(np.float32)
    for t in range(T):
        loc = Param.value(("x", t - 1)) if (carry and t > 0) else Param.const(0.0)
        sx = sl.add(("x", t), A.NORMAL, [loc, Param.const(sigma if carry else 1.0)])
        sx.scan = (scan_id << 20) | (t + 1)
        if observe:
            sy = sl.add(("y", t), A.NORMAL, [Param.value(("x", t)), Param.const(r)])
            sy.scan = (scan_id << 20) | (t + 1)
            modes[("y", t)] = A.MODE_OBS_TAB
            obs[("y", t)] = ys[t]
    return PackedProgram(sl, modes, obs, rng_mode=rng), ys


# ---------------------------------------------------------------------------------------------
# random general expressions (GJX_P_EXPR): shared by the CPU tests of the oracle and the GPU differential tests
# ---------------------------------------------------------------------------------------------
def random_expr_outs(rs, cont, dim, dom="real", depth=3, newer=False):
    """`dim` output nodes (genjax_amd/expr.py) of a random elementwise expression over the elements of the earlier continuous sites
    ``cont`` = [(addr, dim), ...] and constants.  Magnitudes stay bounded (every branch passes through tanh / sigmoid / sin or a
    bounded rational form before it is combined), the final value lands in the domain the parameter needs: "real", "pos", "prob".
    ``newer`` (off: every draw is what it was): a third of the inner nodes are erf, expm1 of a bounded subtree, lgamma(1.5 + sigmoid(.))
    or a log-sum-exp of two or three subtrees."""
    from genjax_amd import expr as E

    def leaf():
        if rs.random() < 0.25 or not cont:
            return E.const(float(rs.standard_normal() * 0.7))
        a, d = cont[int(rs.integers(len(cont)))]
        return E.value(a, int(rs.integers(d)))

    def bounded(n):          # any node -> (-1, 1)-ish, WELL CONDITIONED: no periodic or exploding function of an unbounded argument
        r = rs.random()      # (sin(exp(a)) amplifies the last bit of the device's v_exp_f32 into an O(1) difference: not a parity question)
        if r < 0.4:
            return E.unary("tanh", n)
        if r < 0.6:
            return E.unary("sin", E.lin(0.0, [(E.unary("tanh", n), 2.0)]))
        if r < 0.8:
            return E.lin(-1.0, [(E.unary("sigmoid", n), 2.0)])
        return E.binary("div", n, E.lin(1.0, [(E.unary("square", n), 1.0)]))      # x / (1 + x^2)

    def tree(d):
        if d == 0:
            return bounded(leaf())
        if newer and rs.random() < 0.35:
            r = rs.random()
            if r < 0.25:
                return E.unary("erf", tree(d - 1))
            if r < 0.5:
                return E.unary("expm1", bounded(tree(d - 1)))
            if r < 0.75:
                return E.unary("lgamma", E.lin(1.5, [(E.unary("sigmoid", tree(d - 1)), 1.0)]))
            return E.lse([tree(d - 1) for _ in range(int(rs.integers(2, 4)))])
        r = rs.random()
        a = tree(d - 1)
        if r < 0.18:
            return E.add(a, tree(d - 1))
        if r < 0.3:
            return E.sub(a, tree(d - 1))
        if r < 0.5:
            return E.binary("mul", a, tree(d - 1))
        if r < 0.58:
            return E.binary("max" if rs.random() < 0.5 else "min", a, tree(d - 1))
        if r < 0.66:
            return E.where(E.binary("gt", a, tree(d - 1)), tree(d - 1), a)
        if r < 0.74:          # a small linear layer over several sub-expressions
            k = int(rs.integers(2, 4))
            return bounded(E.lin(float(rs.standard_normal() * 0.3), [(tree(d - 1), float(rs.standard_normal() * 0.8)) for _ in range(k)]))
        if r < 0.8:
            return E.unary("abs", a)
        if r < 0.86:
            return E.unary("log1p", E.unary("square", a))
        if r < 0.92:
            return E.unary("sqrt", E.lin(0.5, [(E.unary("square", a), 1.0)]))
        return bounded(E.unary("exp", bounded(a)))

    outs = []
    for _ in range(dim):
        n = tree(int(rs.integers(1, depth + 1)))
        if dom == "pos":
            n = E.lin(0.25, [(E.unary("softplus", n), 1.0)]) if rs.random() < 0.5 else E.unary("exp", E.lin(0.0, [(bounded(n), 0.8)]))
        elif dom == "prob":
            n = E.lin(0.02, [(E.unary("sigmoid", n), 0.96)])
        outs.append(n)
    return outs


def bnn_model(N=64, DI=16, DH=8, seed=0, first_is_one=False):
    """a small Bayesian network classifier, the canonical model of general expressions inside a vmapped kernel: latent weights outside
    the plate (one site per hidden unit's row, one for the output layer), the observations vmapped over the data —
    y_n ~ bernoulli(logits = w2 . tanh(W1 x_n)).  -> (model, X, Y, float64 log-likelihood function of (W1 [DH][DI][K], w2 [DH][K]))"""
    import genjax_amd as genjax
    rs = np.random.default_rng(seed)
    X = rs.standard_normal((N, DI)).astype(np.float32)
    if first_is_one:
        X[3, 0] = 1.0          # (a covariate that constant-folds differently in ONE instance: the plate is irregular and stays unrolled)
    Y = (rs.random(N) < 0.5).astype(np.float32)

    @genjax.gen
    def kern(x_row, W1, w2):
        h = genjax.tanh(genjax.array([genjax.dot(W1[j], x_row) for j in range(DH)]))
        return genjax.bernoulli(logits=genjax.dot(w2, h)) @ "y"

    @genjax.gen
    def bnn():
        W1 = [genjax.normal(np.zeros(DI, np.float32), 0.5) @ f"W1_{j}" for j in range(DH)]
        w2 = genjax.normal(np.zeros(DH, np.float32), 1.0) @ "w2"
        kern.vmap(in_axes=(0, None, None))(X, W1, w2) @ "obs"

    def loglik(W1, w2):
        h = np.tanh(np.einsum("jik,ni->njk", W1, X.astype(np.float64)))
        lg = np.einsum("jk,njk->nk", w2, h)
        return (Y[:, None] * -np.logaddexp(0, -lg) + (1 - Y[:, None]) * -np.logaddexp(0, lg)).sum(0)

    return bnn, X, Y, loglik


# ---------------------------------------------------------------------------------------------
# the sampler grid (tests/golden/make_sampler_grid.py): exact CDFs at fixed edges, shared by tests/test_samplers_cpu.py and
# tests/test_gpu_samplers.py
# ---------------------------------------------------------------------------------------------
SAMPLER_Z = 6.0      # a normal deviate of 2e-9 per edge: over ~260 edges x ~300 rows x 6 variants (oracle and two engines, two RNG layouts) < 1e-3


@functools.lru_cache(maxsize=None)
def sampler_grid():
    """tests/golden/sampler_grid.json.gz: {"levels", "M", kind: record}, read once and left unchanged"""
    with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_grid.json.gz"), "rt") as f:
        return json.load(f)


def sampler_grid_program(kind: str, rng, rows=None):
    """Particle i carries grid row i // M: a carrier site p_j ~ uniform(-1e37, 1e37) per parameter, MODE_OBS_SLOT (its value comes in with
    the choices), and x ~ KIND(p_0, ...) left to be SAMPLED.  -> (program, choices [n_slots, rows * M], slot of x, index of x's site)"""
    g = sampler_grid()
    rec, M = g[kind], g["M"]
    rws = rec["rows"] if rows is None else [rec["rows"][i] for i in rows]
    n = NPAR[kind]
    sl = SiteList()
    for j in range(n):
        sl.add(f"p{j}", A.UNIFORM, [-1e37, 1e37])
    sl.add("x", KIND[kind], [Param.value(f"p{j}") for j in range(n)])
    prog = PackedProgram(sl, {f"p{j}": A.MODE_OBS_SLOT for j in range(n)}, rng_mode=rng)
    ch = np.zeros((max(prog.n_slots, 1), len(rws) * M), np.float32)
    for j in range(n):
        ch[prog.slot_of[f"p{j}"]] = np.repeat(np.asarray([r["p"][j] for r in rws], np.float32), M)
    return prog, ch, prog.slot_of["x"], n


def sampler_edges(g, rec, row):
    """-> (edges as float64 values of float32 numbers, exact F there)"""
    e = np.asarray(row["e"], np.float32).astype(np.float64)
    if rec["discrete"]:
        return e, np.asarray(row["F"], np.float64)
    return e, np.asarray(g["levels"], np.float64)[row["lv"]] + np.asarray(row["dF"], np.float64)


def sampler_edge_bound(F, M, z=SAMPLER_Z):
    return z * np.sqrt(F * (1.0 - F) / M) + 1.0 / M


def sampler_row_check(x, g, rec, row, integer=None):
    """one row's draws x (any float array, judged in float64) -> (excess, text): excess = the largest |empirical - exact| / bound over
    the row's edges, inf when a draw is not finite, outside the support, outside the guard quantiles or (discrete) no integer;
    text says which.  Also -> the largest z-score, |empirical - exact - (+-1/M)| / sqrt(F (1 - F) / M), for the write-down."""
    M = g["M"]
    x = np.asarray(x, np.float64)
    assert x.shape == (M,), x.shape
    if not np.isfinite(x).all():
        return np.inf, 0.0, f"{int((~np.isfinite(x)).sum())} draws are not finite"
    if "wrap" in row:
        x = x - row["wrap"]
        x = x - 2.0 * np.pi * np.round(x / (2.0 * np.pi))
    xs = np.sort(x)
    lo, hi = row["lo"], row["hi"]
    if lo is not None and (xs[0] < lo or (row["lo_open"] and xs[0] <= lo)):
        return np.inf, 0.0, f"{int((xs <= lo).sum())} draws at or below the support's lower edge {lo} (smallest {xs[0]!r})"
    if hi is not None and (xs[-1] > hi or (row["hi_open"] and xs[-1] >= hi)):
        return np.inf, 0.0, f"{int((xs >= hi).sum())} draws at or above the support's upper edge {hi} (largest {xs[-1]!r})"
    if row["x_lo"] is not None and xs[0] < row["x_lo"]:
        return np.inf, 0.0, f"smallest draw {xs[0]!r} below the 1e-6/M quantile {row['x_lo']!r}"
    if row["x_hi"] is not None and xs[-1] > row["x_hi"]:
        return np.inf, 0.0, f"largest draw {xs[-1]!r} above the 1 - 1e-6/M quantile {row['x_hi']!r}"
    if (rec["discrete"] if integer is None else integer) and (xs != np.floor(xs)).any():
        return np.inf, 0.0, "non-integer draws of a discrete kind"
    e, F = sampler_edges(g, rec, row)
    if e.size == 0:
        return 0.0, 0.0, "no edge"
    emp = np.searchsorted(xs, e, side="right") / M          # mean(x <= e_j)
    dev = np.abs(emp - F)
    ex = dev / sampler_edge_bound(F, M)
    zs = np.maximum(dev - 1.0 / M, 0.0) / np.sqrt(F * (1.0 - F) / M)
    j = int(np.argmax(ex))
    return float(ex[j]), float(zs.max()), f"edge {e[j]!r}: empirical {emp[j]:.6g}, exact {F[j]:.6g}, z {zs[j]:.2f} (largest |deviation| {dev.max():.3g})"


def sampler_grid_check(x, rec, rows=None):
    """x: [rows * M] draws of one kind's program (sampler_grid_program) -> (worst excess, worst z, [(row index, parameters, text)] of the
    rows whose excess is over 1).  Works in float64."""
    g = sampler_grid()
    M = g["M"]
    idx = list(range(len(rec["rows"]))) if rows is None else list(rows)
    x = np.asarray(x).reshape(len(idx), M)
    worst, worst_z, bad = 0.0, 0.0, []
    for k, i in enumerate(idx):
        ex, z, text = sampler_row_check(x[k], g, rec, rec["rows"][i])
        worst, worst_z = max(worst, ex), max(worst_z, z)
        if ex > 1.0:
            bad.append((i, tuple(rec["rows"][i]["p"]), text))
    return worst, worst_z, bad


def one_vector_site(kind_code: int, params, dim=None, rng=A.RNG_FLAT):
    """one sampled site "v" of a vector or categorical kind with constant parameters"""
    sl = SiteList()
    sl.add("v", kind_code, params, **({} if dim is None else {"dim": dim}))
    return PackedProgram(sl, rng_mode=rng)


def sampler_row_from_dist(dist, unit=False):
    """a grid row made on the spot from a frozen scipy distribution (the components of the vector kinds: beta marginals of a
    dirichlet, normal components), by make_sampler_grid.py's rules: the levels' quantiles rounded to float32, F exact AT the rounded
    edge, kept when 0 < F < 1, float32-resolvable (the mass between the edge's float32 neighbours under a quarter of its bound) and,
    for a unit-interval kind, strictly inside (1.17549435e-38, 1 - 2^-24).  -> (record, row) for sampler_row_check"""
    g = sampler_grid()
    M, lv = g["M"], np.asarray(g["levels"], np.float64)
    with np.errstate(all="ignore"):
        e = np.where(lv < 0.5, dist.ppf(lv), dist.isf(1.0 - lv)).astype(np.float32)
        up, dn = np.nextafter(e, np.float32(np.inf)).astype(np.float64), np.nextafter(e, np.float32(-np.inf)).astype(np.float64)
        e = e.astype(np.float64)
        F = dist.cdf(e)
        keep = np.isfinite(e) & (F > 0.0) & (F < 1.0) & (dist.cdf(up) - dist.cdf(dn) < 0.25 * sampler_edge_bound(F, M))
    if unit:
        keep &= (e > 1.17549435e-38) & (e < 1.0 - 2.0 ** -24)
    rec = dict(discrete=1)          # (F stored whole, as the discrete kinds do)
    q = 1e-6 / M
    row = dict(e=[float(t) for t in e[keep]], F=[float(t) for t in F[keep]], lo=0.0 if unit else None, hi=1.0 if unit else None,
               lo_open=1, hi_open=1, x_lo=None if unit else float(np.float32(dist.ppf(q)) - np.float32(abs(dist.ppf(q))) * 2.0 ** -22),
               x_hi=None if unit else float(np.float32(dist.isf(q)) + np.float32(abs(dist.isf(q))) * 2.0 ** -22))
    return rec, row


def sampler_component_check(x, dist, unit=False):
    """-> (excess, z, text) of one component's M draws against `dist` (sampler_row_check; integer test off)"""
    rec, row = sampler_row_from_dist(dist, unit)
    return sampler_row_check(x, sampler_grid(), rec, row, integer=False)


DIRICHLET_ALPHAS = ([0.8, 2.0, 3.0], [0.05, 0.05, 0.05], [50.0, 1.0, 0.2])
MVN_LOC = [0.0, 1e4, -2.0, 0.5, 3e2]
MVN_SCALE = [1.0, 1e-3, 1e-6, 2.5, 30.0]


def dirichlet_check(x, alpha):
    """x [dim, M] draws of dirichlet(alpha): each component against beta(alpha_i, alpha_0 - alpha_i), rows sum to 1 within 1e-5, no
    component exactly 0 or 1 (sampler_row_check's open support).  -> (worst excess, worst z, [failures])"""
    import scipy.stats as st
    x = np.asarray(x, np.float64)
    a = np.asarray(np.asarray(alpha, np.float32), np.float64)
    worst, wz, bad = 0.0, 0.0, []
    s = np.abs(x.sum(0) - 1.0).max()
    if not s <= 1e-5:
        bad.append(("sum", float(s)))
    for i in range(len(a)):
        ex, z, text = sampler_component_check(x[i], st.beta(a[i], a.sum() - a[i]), unit=True)
        worst, wz = max(worst, ex), max(wz, z)
        if ex > 1.0:
            bad.append((i, text))
    return worst, wz, bad


def mvn_check(x, loc=MVN_LOC, scale=MVN_SCALE):
    import scipy.stats as st
    x = np.asarray(x, np.float64)
    worst, wz, bad = 0.0, 0.0, []
    for i in range(len(loc)):
        ex, z, text = sampler_component_check(x[i], st.norm(float(np.float32(loc[i])), float(np.float32(scale[i]))))
        worst, wz = max(worst, ex), max(wz, z)
        if ex > 1.0:
            bad.append((i, text))
    return worst, wz, bad


def categorical_case(n, probs: bool):
    """-> (float32 parameter vector, exact float64 probabilities): n categories, a logit spread of 60 (n > 3), category 1 impossible
    (a -inf logit / a 0 probability)"""
    rs = np.random.default_rng(n)
    lg = (rs.random(n) * 6.0 - 3.0).astype(np.float32)
    lg[0] = 3.0
    if n > 3:
        lg[n - 1] = -57.0          # (with 3 categories, one of them impossible, a spread of 60 would leave a single outcome)
    if probs:
        par = np.exp(lg.astype(np.float64))
        par[1] = 0.0
        par = (par / par.sum() * 0.5).astype(np.float32)          # (unnormalised on purpose: the kernel normalises)
        p = par.astype(np.float64)
    else:
        lg[1] = -np.inf
        par = lg
        with np.errstate(all="ignore"):
            p = np.exp(lg.astype(np.float64) - 3.0)
    return par, p / p.sum()


def categorical_check(v, p):
    """v: M category draws -> (worst excess, [failures]): per category |count / M - p| <= 6 sqrt(p (1 - p) / M) + 1 / M; a category of
    probability 0 has count exactly 0; every draw an integer in range"""
    M = sampler_grid()["M"]
    v = np.asarray(v, np.float64)
    assert v.shape == (M,)
    if not (np.isfinite(v).all() and (v == np.floor(v)).all() and v.min() >= 0 and v.max() < len(p)):
        return np.inf, ["draws outside 0 .. n - 1"]
    cnt = np.bincount(v.astype(np.int64), minlength=len(p))
    ex = np.abs(cnt / M - p) / sampler_edge_bound(p, M)
    bad = [(int(c), int(cnt[c]), float(p[c])) for c in np.nonzero(ex > 1.0)[0]]
    bad += [(int(c), int(cnt[c]), 0.0) for c in np.nonzero((p == 0.0) & (cnt > 0))[0]]
    return float(ex.max()), bad


# ---- the float64 grid harness of the expression tests (tests/test_gpu_tracer_surface.py, tests/test_gpu_expr_ops.py, tests/test_expr_ops_cpu.py):
# host-made grids supplied as the values of constrained sites (no sampler), a float64 NumPy restatement of the per-site scores
GRID_K = 4099                 # columns for scores: neither a multiple of the wave nor of the block
GRID_N_GRAD = 384             # columns for gradients and HMC
GRID_RT, GRID_AT = 2e-4, 2e-4           # scores; gradients rtol / atol 2e-3, engine against engine after one HMC move 3e-3
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def nlp(x, mu, sig):
    """float64 log-density of normal(mu, sig) at x"""
    x, mu, sig = np.asarray(x, np.float64), np.asarray(mu, np.float64), np.asarray(sig, np.float64)
    return -0.5 * ((x - mu) / sig) ** 2 - np.log(sig) - HALF_LOG_2PI


def grid_offsets(n, width=1.5):
    """where an observation sits relative to its mean: a fixed pattern within +- width standard deviations"""
    return width * np.sin(1.0 + 0.7 * np.arange(n))


def well_conditioned(spec, vals32, edges=False):
    """the float64 reference under inputs a few float32 ulps away moves by less than half the tolerance, at EVERY grid point.
    ``edges``: the grid holds points whose reference is +-inf or NaN (an overflow, a pole, 0 / 0): there the reference under the
    moved inputs must be the SAME infinity (or NaN); every other point is held to the bound as before"""
    v = {k: x.astype(np.float64) for k, x in vals32.items()}
    with np.errstate(all="ignore"):
        s0 = np.stack(spec["scores"](v))
        s1 = np.stack(spec["scores"]({k: x * (1.0 + 2e-6) for k, x in v.items()}))
    if not edges:
        assert not np.isnan(s0).any() and not np.isinf(s0).any()
    for p, q in ((s0, s1), (s0.sum(0), s1.sum(0))):
        fin = np.isfinite(p)
        assert (np.isnan(p) == np.isnan(q)).all() and (p[np.isinf(p)] == q[np.isinf(p)]).all()
        p, q = p[fin], q[fin]
        assert (np.abs(q - p) < 0.5 * (GRID_AT + GRID_RT * np.abs(p))).all(), float((np.abs(q - p) / (GRID_AT + GRID_RT * np.abs(p))).max())
    return s0


def float32_range(want):
    """a float64 score beyond the largest float32 is what the device can only return as -inf (the density of a value 1e30 standard
    deviations out): the reference is compared as that infinity, every other value as it is"""
    with np.errstate(invalid="ignore"):
        big = np.abs(want) > float(np.finfo(np.float32).max)
    return np.where(big, np.copysign(np.inf, want), want)


def grid_rows(prog, spec, vals):
    ch = np.zeros((prog.n_slots, next(iter(vals.values())).shape[1]), np.float32)
    for addr, d in spec["sites"]:
        if addr in vals and prog.slot_of.get(addr, -1) >= 0:
            ch[prog.slot_of[addr]:prog.slot_of[addr] + d] = vals[addr]
    return ch
