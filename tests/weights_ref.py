"""Float64 restatement of the weight calls of include/gjx.h under its rule for non-finite weights ("Non-finite weights", above the
log-sum-exp section): gjx_logsumexp / gjx_lse_combine / gjx_trials_lse_pick's record, gjx_ess, the fixed-point weights of
gjx_weight_cumsum and the resamplers.  Plain NumPy on the float32 arrays the device receives; no project import beyond constants.
Also the weight families, the poison patterns and the launch geometry of gjx_logsumexp that tests/test_weights_cpu.py and
tests/test_gpu_weights.py share."""
import math

import numpy as np

SCALE = 1 << 30                 # the fixed point of gjx_weight_cumsum: q_i = trunc(w_i 2^30)
U = 2.0 ** -24                  # float32 unit roundoff

# gjx_logsumexp's launch (gjx_run.hip): ceil(K / 1024) blocks of 256 threads, at most 2048 blocks; a thread strides by the grid
LSE_BLOCK, LSE_PER_BLOCK, LSE_GRID_CAP = 256, 1024, 2048

# The constant of bound_lse, per call: 4 x the worst error / bound_lse(C = 1) measured on an MI355X over every size, family and
# poison pattern of tests/test_gpu_weights.py ("Non-finite weights").
C_LSE = {"logsumexp": 4 * 0.65, "lse_combine": 4 * 0.58, "trials": 4 * 0.23}

# relative error allowed to ONE float32 weight exp(x - max) against float64: the subtraction, the product with log2 e and the constant
# itself are three roundings of an exponent of at most 31 bits in magnitude (beyond that the weight is below 2^-30 and its fixed point
# is 0 either way), 3 * 31 * 2^-24 in base 2, times ln 2; v_exp_f32 (or libm's expf) adds one ulp
REL_LOG = 3 * 31 * U * math.log(2.0) + 2 * U


def live(x):
    """a weight of -inf or NaN is dead (x > -inf is False for a NaN)"""
    return np.asarray(x, np.float64) > -np.inf


def lse_grid(K):
    """(stride, per_thread) of gjx_logsumexp: thread t of the grid takes entries t, t + stride, ...; the longest thread takes per_thread"""
    nblocks = min(max(1, -(-K // LSE_PER_BLOCK)), LSE_GRID_CAP)
    stride = nblocks * LSE_BLOCK
    return stride, -(-K // stride)


def lse_record(x, K_total=None):
    """{max, sum exp(x - max), lse, lse - log K_total} over the live entries, float64.  No live entry: {-inf, 0, -inf, -inf}.  A live +inf:
    max = lse = lse - log K_total = +inf and entry 1 is NaN here (unspecified: nobody asserts it)."""
    x = np.asarray(x, np.float64).reshape(-1)
    K_total = x.size if K_total is None else K_total
    xl = x[live(x)]
    if xl.size == 0:
        return np.array([-np.inf, 0.0, -np.inf, -np.inf])
    m = xl.max()
    if m == np.inf:
        return np.array([np.inf, np.nan, np.inf, np.inf])
    s = math.fsum(np.exp(xl - m))
    l = m + math.log(s)
    return np.array([m, s, l, l - math.log(K_total)])


def lse_combine(pairs, K_total):
    """the record of G {max, sumexp} pairs; a pair whose maximum is -inf (or NaN) is an empty rank whatever its sum holds"""
    p = np.asarray(pairs, np.float64).reshape(-1, 2)
    p = p[live(p[:, 0])]
    if p.shape[0] == 0:
        return np.array([-np.inf, 0.0, -np.inf, -np.inf])
    m = p[:, 0].max()
    if m == np.inf:
        return np.array([np.inf, np.nan, np.inf, np.inf])
    s = math.fsum(p[:, 1] * np.exp(p[:, 0] - m))
    l = m + math.log(s)
    return np.array([m, s, l, l - math.log(K_total)])


def ess(x):
    """{max, sum e, sum e^2, (sum e)^2 / sum e^2}, e_i = exp(x_i - max) over the live entries; a dead collection: {-inf, 0, 0, 0}"""
    x = np.asarray(x, np.float64).reshape(-1)
    xl = x[live(x)]
    if xl.size == 0:
        return np.array([-np.inf, 0.0, 0.0, 0.0])
    m = xl.max()
    e = np.exp(xl - m)
    s1, s2 = math.fsum(e), math.fsum(e * e)
    return np.array([m, s1, s2, s1 * s1 / s2])


def weights64(x, is_log, mx=None):
    """float64 weights before normalisation: exp(x - mx) for log-weights (mx: their live maximum unless given), x itself for linear
    ones; dead entries (log: -inf or NaN; linear: <= 0 or NaN) are exactly 0"""
    x = np.asarray(x, np.float64).reshape(-1)
    if not is_log:
        return np.where(x > 0.0, x, 0.0)
    lv = live(x)
    if not lv.any():
        return np.zeros(x.size)
    mx = x[lv].max() if mx is None else float(mx)
    w = np.zeros(x.size)
    w[lv] = np.exp(x[lv] - mx)
    return w


def fixed_point(x, is_log, mx=None):
    """uint64[K]: trunc(w_i 2^30) with w from float64 exp (weights64)"""
    return np.floor(weights64(x, is_log, mx) * SCALE).astype(np.uint64)


def offspring_bound(x, N, is_log=True):
    """float64[K]: the largest |count_i - N w_i| a systematic resampler on the fixed-point weights q may show against the float64
    normalised weights w_i = e_i / sum e (e = weights64).

    Write eps_i = 2^30 e_i, E = sum eps, L = the number of live particles, d = the relative error of one weight (0 for linear weights,
    which arrive exact; REL_LOG for log-weights, whose exp is taken in float32).  Truncation loses less than one unit of 2^-30 per live
    particle, so  eps_i (1 - d) - 1 < q_i <= eps_i (1 + d)  and  E (1 - d) - L < Q = sum q <= E (1 + d).  Hence
        q_i / Q - w_i <= w_i ((1 + d) / (1 - d - L / E) - 1) = w_i (2 d + L / E) / (1 - d - L / E)
        w_i - q_i / Q <= w_i (1 - (1 - d) / (1 + d)) + 1 / (E (1 + d)) <= 2 d w_i + 1 / E.
    The comb puts slot j at p_j = (j + u) Q / N and gives it to the particle whose integer interval [c_{i-1}, c_i) holds floor(p_j):
    the slots are Q / N apart, so particle i gets floor or ceil of N q_i / Q, strictly within 1; p_j is two double roundings of a
    number below Q, an error below Q 2^-52, that is N 2^-52 slots.  Together
        |count_i - N w_i| < 1 + N 2^-52 + N max(w_i (2 d + L / E) / (1 - d - L / E), 2 d w_i + 1 / E).
    With log-weights the maximum has e = 1, so E >= 2^30 and the slack is small at every size tested."""
    e = weights64(x, is_log)
    E = float(e.sum()) * SCALE
    L = int((e > 0).sum())
    d = REL_LOG if is_log else 0.0
    assert L > 0 and d + L / E < 1.0, "offspring_bound: no live particle, or weights too small for the fixed point"
    w = e / e.sum()
    slack = np.maximum(w * (2 * d + L / E) / (1.0 - d - L / E), 2 * d * w + 1.0 / E)
    return 1.0 + N * 2.0 ** -52 + N * slack


def bound_lse(x, per_thread, C, K_total=None):
    """float64[4]: error bounds for the device's float32 record {max, sumexp, lse, lse - log K_total} of the log-weights x, whose threads
    each stream `per_thread` entries into a running (max, sum).  Entry 0 is exact (bound 0).  For the sum, in units of U = 2^-24:
      * every live term exp(x_i - m): the subtraction and the product with log2 e perturb the exponent by 2 U |x_i - m| log2 e, the
        v_exp_f32 result by one ulp (2 U): relative (2 + 2 |x_i - m|) U, weighted by the term's share p_i = e_i / S of the sum;
      * a thread rescales its running sum once per entry (one more v_exp_f32 on an exponent y <= 0 whose share of the total is at most
        y e^-y <= 1 / e, and one multiply) and adds once per entry: 5 U per entry, per_thread entries;
      * the tree above the threads: six DPP adds, the four waves of a block (a v_exp_f32, a multiply and an add each), and the same
        again in the finishing block, whose threads take up to eight partials: 40 roundings.
    lse = m + log S adds the relative error of S, one ulp of the logarithm (2 U |log S|) and the rounding of the sum (U |lse|); entry 3
    one more subtraction against a float32 log K_total.  C scales the whole bound (C_LSE: measured, times four)."""
    x = np.asarray(x, np.float64).reshape(-1)
    K_total = x.size if K_total is None else K_total
    xl = x[live(x)]
    if xl.size == 0 or xl.max() == np.inf:
        return np.zeros(4)
    m = xl.max()
    e = np.exp(xl - m)
    S = math.fsum(e)
    terms = math.fsum(e / S * (2.0 + 2.0 * (m - xl)))
    rel_s = U * (terms + 5.0 * per_thread + 40.0)
    l = m + math.log(S)
    b_l = rel_s + 2 * U * abs(math.log(S)) + U * abs(l)
    b_3 = b_l + U * (abs(l) + 2 * math.log(K_total))
    return C * np.array([0.0, rel_s * S, b_l, b_3])


def bound_combine(pairs, C, K_total):
    """bound_lse for gjx_lse_combine: a live pair contributes y_g exp(x_g - m) (one more multiply than a plain term: 3 + 2 |x_g - m|
    units of U on its share of the sum); the finishing block's threads take up to ceil(G / 256) pairs, then the same tree"""
    p = np.asarray(pairs, np.float64).reshape(-1, 2)
    G = p.shape[0]
    p = p[live(p[:, 0])]
    if p.shape[0] == 0 or p[:, 0].max() == np.inf:
        return np.zeros(4)
    m = p[:, 0].max()
    t = p[:, 1] * np.exp(p[:, 0] - m)
    S = math.fsum(t)
    rel_s = U * (math.fsum(t / S * (3.0 + 2.0 * (m - p[:, 0]))) + -(-G // 256) + 20.0)
    l = m + math.log(S)
    b_l = rel_s + 2 * U * abs(math.log(S)) + U * abs(l)
    return C * np.array([0.0, rel_s * S, b_l, b_l + U * (abs(l) + 2 * math.log(K_total))])


def project_bar(ref):
    """the suite's standing bar for a log-sum-exp against float64 (tests/test_gpu_parity.py): rtol 2e-6 + atol 2e-6"""
    return 2e-6 + 2e-6 * np.abs(ref)


def lse_tolerance(x, per_thread, C, K_total=None):
    """bound_lse, or the project's bar where that is tighter"""
    ref = lse_record(x, K_total)
    b = bound_lse(x, per_thread, C, K_total)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(ref), np.minimum(b, project_bar(ref)), 0.0)


# ---- shared cases ------------------------------------------------------------------------------------------------------------
# 513: the smallest K at which a thread of gjx_logsumexp's first kernel takes three entries (one block of 256 threads up to K = 1024)
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 513, 1023, 1024, 1025, 4097]


def families(K, seed=0):
    """name -> float32[K] log-weights, every one with at least one live entry"""
    rs = np.random.default_rng(1000 + 7 * K + seed)
    z = rs.standard_normal(K)
    f = {"normal3": 3.0 * z, "normal20": 20.0 * z, "equal": np.full(K, -1.25)}
    for name, at in (("one_first", 0), ("one_last", K - 1), ("one_wave", 64), ("one_block", 256)):
        x = np.full(K, -np.inf)
        x[min(at, K - 1)] = 0.75
        f[name] = x
    f["ramp_up"] = 0.37 * np.arange(K) - 11.0            # every entry moves a thread's running maximum
    f["ramp_down"] = -0.37 * np.arange(K) + 5.0          # none after the first does
    for name, top in (("huge_pos", 3.0e38), ("huge_neg", -3.0e38)):
        x = np.full(K, top - 100.0)                      # (100 is below half an ulp at 3e38: in float32 the rest EQUALS the maximum)
        x[K // 2] = top
        f[name] = x
        y = np.full(K, np.float32(top) * np.float32(1.0 - 2.0 ** -20) if top > 0 else np.float32(-3.3e38))   # representably below
        y[K // 2] = top
        f[name + "_gap"] = y
    f["spread"] = -60.0 * rs.random(K)                   # beyond ln 2^30 = 20.8: most q_i are 0
    f["spread"][K // 3] = 0.0
    x = 3.0 * z.copy()
    x[rs.random(K) < 0.3] = -np.inf
    x[(K * 2) // 3] = 1.0
    f["dead30"] = x
    return {k: v.astype(np.float32) for k, v in f.items()}


def poisons(K):
    """name -> (index array, values): entries to overwrite.  `first` / `later`: a thread's first entry only / a later entry only
    (index >= the grid's stride) under gjx_logsumexp's launch; `block`: one whole block of 256 entries."""
    stride, _ = lse_grid(K)
    nan = np.float32(np.nan)
    idx = np.arange(K)
    p = {}
    first = idx[(idx < stride) & (idx % 5 == 1)]
    if first.size:
        p["first"] = (first, nan)
    later = idx[(idx >= stride) & (idx % 3 == 0)]
    if later.size:
        p["later"] = (later, nan)
    p["at0"] = (idx[:1], nan)
    p["last"] = (idx[-1:], nan)
    b0 = 256 if K > 256 else 0
    p["block"] = (idx[b0:b0 + 256], nan)
    mixed = idx[idx % 3 == 2]
    if mixed.size:
        p["mixed"] = (mixed, np.where(mixed % 2 == 0, nan, np.float32(-np.inf)).astype(np.float32))
    p["half_half"] = (idx, np.where(idx % 2 == 0, np.float32(-np.inf), nan).astype(np.float32))     # everything dead, two ways
    p["all_nan"] = (idx, nan)
    return p


def poisoned(x, poison):
    """(x with the pattern applied, the same with -inf in place of every NaN)"""
    i, v = poison
    y = x.copy()
    y[i] = v
    return y, np.where(np.isnan(y), np.float32(-np.inf), y).astype(np.float32)
