"""The weight calls every collection and filter goes through — gjx_logsumexp, gjx_lse_combine, gjx_trials_lse_pick, gjx_categorical_pick,
gjx_ess, gjx_weight_cumsum (modes 0 and 1), gjx_resample_indices, gjx_resample_gather — against the float64 restatement in
tests/weights_ref.py and under the rule of include/gjx.h, "Non-finite weights": a call on weights that hold NaN gives, bit for bit, what
it gives with -inf in their place; no live particle: {-inf, 0, -inf, -inf}, the first index, identity ancestors and status 2; a live
+inf makes the three log-sum-exp records +inf.

Sizes: wave (64), block (256) and launch (1024 per block of gjx_logsumexp) boundaries, and 513, the smallest K at which a thread of
gjx_logsumexp's first kernel takes three entries: its grid is ceil(K / 1024) blocks of 256 threads, so one block strides by 256 up to
K = 1024 (the cap of 2048 blocks is reached only beyond K = 2^21 and is not exercised here).  A "later" NaN sits at an index at or
beyond that stride: it reaches a thread whose running maximum is already finite.

Finite log-sum-exp entries are held to weights_ref.lse_tolerance (bound_lse with the measured constant, or the suite's standing
rtol 2e-6 + atol 2e-6 where that is tighter); integers — prefix sums, totals, ancestors, picks, children — are exact.  In mode 1 the
device takes exp(x - max) with v_exp_f32 where the oracle calls libm's expf, so the fixed-point weights themselves are compared with
float64 (one unit of truncation + weights_ref.REL_LOG) and the ancestors with the oracle's comb on the device's own prefix sums; with
linear weights (mode 0) the prefix sums equal the oracle's bit for bit.

Host layer (the last two tests): a ParticleCollection over a model that scores NaN for a known third of its particles.  Under the rule
is every collection whose record is taken from its log-weights; the collection exactly as run_smc returns it finishes its record from
the producing kernel's block partials, which are not ("Open end"), and is pinned as such."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import genjax_amd as genjax
from genjax_amd import _abi as A
import weights_ref as R

RNGS = [A.RNG_FLAT, A.RNG_JAX32]
DEAD = np.array([-np.inf, 0.0, -np.inf, -np.inf], np.float32)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=np.float32):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _cases(x, K):
    """(name, poisoned, substituted) for the clean family and every pattern"""
    yield "clean", x, x
    for pname, poison in R.poisons(K).items():
        y, z = R.poisoned(x, poison)
        yield pname, y, z


def _check_record(got, ref, tol, unit, call, what):
    """got float32[4] against the float64 record: entry 0 exact, a dead record exact, +inf by rule 3 (entry 1 not asserted), the
    rest within tol; `unit` = the bound at C = 1, for the measured constant"""
    got = got.astype(np.float64)
    assert got[0] == np.float32(ref[0]), (what, got, ref)
    if ref[0] == -np.inf:
        np.testing.assert_array_equal(got, DEAD, err_msg=what)
        return 0.0
    if ref[0] == np.inf:
        assert got[2] == np.inf and got[3] == np.inf, (what, got)
        return 0.0
    err = np.abs(got - ref)[1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.where(err > 0, err / unit[1:], 0.0).max())
    assert (err <= tol[1:]).all(), f"{call} {what}: got {got}, float64 {ref}, error {err}, allowed {tol[1:]}, error / bound(C = 1) {ratio:.3f}"
    return ratio


@pytest.mark.parametrize("K", R.SIZES)
def test_logsumexp(K):
    from genjax_amd import kernels
    ws = kernels.workspace(A.OP_LSE, K)
    _, per_thread = R.lse_grid(K)
    Kt = 3 * K + 1                                              # K_total != K
    worst = 0.0
    for fam, x in R.families(K).items():
        for pname, y, z in _cases(x, K):
            got, sub = _np(kernels.logsumexp(_dev(y), Kt, ws=ws)), _np(kernels.logsumexp(_dev(z), Kt, ws=ws))
            np.testing.assert_array_equal(_bits(got), _bits(sub), err_msg=f"K={K} {fam} {pname}: NaN and -inf differ")
            worst = max(worst, _check_record(got, R.lse_record(y, Kt), R.lse_tolerance(y, per_thread, R.C_LSE["logsumexp"], Kt),
                                             R.bound_lse(y, per_thread, 1.0, Kt), "logsumexp", f"K={K} {fam} {pname}"))
        # a live +inf: at a thread's first entry, at its last, and beside NaN and -inf
        for at in sorted({0, K // 2, K - 1}):
            y = x.copy(); y[at] = np.inf
            if K > 2:
                y[(at + 1) % K] = np.nan
                y[(at + 2) % K] = -np.inf
            got = _np(kernels.logsumexp(_dev(y), Kt, ws=ws))
            assert got[0] == np.inf and got[2] == np.inf and got[3] == np.inf, (K, fam, at, got)
    print(f"logsumexp K={K}: worst error / bound(C = 1) {worst:.3f}")


@pytest.mark.parametrize("G", [1, 2, 3, 8, 64])
def test_lse_combine(G):
    from genjax_amd import kernels
    rs = np.random.default_rng(G)
    garbage = [np.nan, np.inf, 7.0, -1.0, -np.inf]
    worst = 0.0
    for K in (257, 4097):
        Kt = 2 * K + 3
        for fam, x in R.families(K).items():
            edges = np.linspace(0, K, G + 1).astype(int)
            pairs = np.zeros((G, 2), np.float32)
            for g in range(G):
                rec = R.lse_record(x[edges[g]:edges[g + 1]])
                pairs[g] = rec[:2]
                if rec[0] == -np.inf:                           # an empty rank: its sum holds anything
                    pairs[g, 1] = garbage[g % len(garbage)]
            for empty in ((), tuple(rs.choice(G, size=max(1, G // 3), replace=False)), tuple(range(G))):
                p = pairs.copy()
                for i, g in enumerate(empty):
                    p[g] = (-np.inf, garbage[i % len(garbage)])
                got = _np(kernels.lse_combine(_dev(p.reshape(-1)), Kt))
                ref = R.lse_combine(p, Kt)
                tol = np.minimum(R.bound_combine(p, R.C_LSE["lse_combine"], Kt), R.project_bar(ref)) if np.isfinite(ref[0]) else np.zeros(4)
                worst = max(worst, _check_record(got, ref, tol, R.bound_combine(p, 1.0, Kt), "lse_combine", f"G={G} K={K} {fam} empty={empty}"))
                # a maximum of NaN is an empty rank too, bit for bit
                pn = p.copy(); pn[np.isneginf(pn[:, 0]), 0] = np.nan
                np.testing.assert_array_equal(_bits(_np(kernels.lse_combine(_dev(pn.reshape(-1)), Kt))), _bits(got))
            p = pairs.copy(); p[G // 2] = (np.inf, 1.0)         # a rank that saw +inf
            got = _np(kernels.lse_combine(_dev(p.reshape(-1)), Kt))
            assert got[0] == np.inf and got[2] == np.inf and got[3] == np.inf, (G, K, fam, got)
    print(f"lse_combine G={G}: worst error / bound(C = 1) {worst:.3f}")


def _trial_rows(n, K, start="first"):
    """n trials of K log-weights: families in turn, every third trial poisoned (by every pattern in turn, beginning with `start` where
    this K has it), a clean one beside it, and a wholly dead trial (a NaN / -inf mix) at index 1; with n = 2 trial 1 is the clean one
    in the first variant and the dead one in every other"""
    fam = list(R.families(K).items())
    poi = R.poisons(K)
    names = list(poi)
    s0 = names.index(start) if start in names else 0
    y = np.zeros((n, K), np.float32)
    for t in range(n):
        x = fam[t % len(fam)][1]
        y[t] = R.poisoned(x, poi[names[(s0 + t // 3) % len(names)]])[0] if t % 3 == 0 else x
    dead = [1] if n > 2 or (n == 2 and start != "first") else []
    for t in dead:
        y[t] = np.nan
        y[t, ::2] = -np.inf
    return y


@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("n,K", [(1, 1), (3, 257), (50, 50), (2, 4097)])
def test_trials_lse_pick(oracle, rng, n, K):
    from genjax_amd import kernels
    off, key = 12_345, (3, 9)
    per_thread = -(-K // 256)
    worst = 0.0

    def record(got, y_t, what):
        return _check_record(got, R.lse_record(y_t), R.lse_tolerance(y_t, per_thread, R.C_LSE["trials"]), R.bound_lse(y_t, per_thread, 1.0),
                             "trials", what)

    # the poisoned trial(s) start at another pattern in every variant: K = 4097 (17 entries per thread) and K = 257 see a NaN at a
    # thread's first entry, at a later entry ("later"; at K = 257 the only one is the last index), as a whole block and mixed with -inf
    variants = [_trial_rows(n, K, start) for start in ("first", "later", "last", "block", "mixed")]
    if (n, K) == (1, 1):
        variants = [variants[0], np.full((1, 1), 0.3, np.float32), np.full((1, 1), -np.inf, np.float32)]      # (_trial_rows(1, 1) is NaN)
    for v, y in enumerate(variants):
        z = np.where(np.isnan(y), np.float32(-np.inf), y)
        lse, pick = kernels.trials_lse_pick(_dev(y.reshape(-1)), n, K, key, rng, offset=off)
        lse_z, pick_z = kernels.trials_lse_pick(_dev(z.reshape(-1)), n, K, key, rng, offset=off)
        lse, pick = _np(lse), _np(pick)
        np.testing.assert_array_equal(_bits(lse), _bits(_np(lse_z)))
        np.testing.assert_array_equal(pick, _np(pick_z))
        for t in range(n):
            worst = max(worst, record(lse[t], y[t], f"n={n} K={K} variant {v} trial {t}"))
            if not R.live(y[t]).any():
                assert pick[t] == off + t * K                   # a dead trial: its first particle
                continue
            assert R.live(y[t])[pick[t] - off - t * K], f"variant {v} trial {t}: a dead particle was picked"
            assert pick[t] == oracle.categorical_pick(y[t], lse[t], key, rng, offset=off + t * K)[1], f"n={n} K={K} variant {v} trial {t}"
            if v == 0 or n <= 3:
                one = kernels.categorical_pick(_dev(y[t]), _dev(lse[t]), key, rng, offset=off + t * K)
                assert int(one[1]) == pick[t]
    # a trial with a live +inf beside clean ones (records only: +inf is not supported by the pick)
    y = _trial_rows(n, K).copy()
    y[n - 1, K // 2] = np.inf
    lse, _ = kernels.trials_lse_pick(_dev(y.reshape(-1)), n, K, None, rng)
    lse = _np(lse)
    assert lse[n - 1, 0] == np.inf and lse[n - 1, 2] == np.inf and lse[n - 1, 3] == np.inf
    for t in range(n - 1):
        worst = max(worst, record(lse[t], y[t], f"n={n} K={K} trial {t} beside +inf"))
    print(f"trials n={n} K={K}: worst error / bound(C = 1) {worst:.3f}")


@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("K", [1, 65, 257, 1025, 4097])
def test_categorical_pick(oracle, rng, K):
    from genjax_amd import kernels
    off = 777
    ws, wl = kernels.workspace(A.OP_PICK, K), kernels.workspace(A.OP_LSE, K)
    for fam, x in R.families(K).items():                        # every family: the maxima at +-3e38 and one live particle at a wave
        for pname, y, z in _cases(x, K):                        # or block boundary are where logw - lse and the merges of pairs can slip
            yd, zd = _dev(y), _dev(z)
            l4 = kernels.logsumexp(yd, ws=wl)
            for key in ((5, 6), (9, 10)):
                got = _np(kernels.categorical_pick(yd, l4, key, rng, off, ws=ws))
                sub = _np(kernels.categorical_pick(zd, l4, key, rng, off, ws=ws))
                np.testing.assert_array_equal(got, sub, err_msg=f"K={K} {fam} {pname}")
                assert int(got[1]) == oracle.categorical_pick(y, _np(l4), key, rng, off)[1], f"K={K} {fam} {pname} {key}"
                if R.live(y).any():
                    assert R.live(y)[int(got[1]) - off], f"K={K} {fam} {pname}: a dead particle was picked"
                else:
                    assert int(got[1]) == off                    # a dead collection: its first particle
    if K == 65:                                                  # a NaN particle is never picked, 64 keys
        x = R.families(K)["normal3"].copy()
        x[[0, 7, 31, 63, 64]] = np.nan
        x[[1, 33]] = 40.0 + x[[1, 33]]                           # (and the heavy ones sit next to NaN)
        x[2] = np.nan
        xd = _dev(x)
        l4 = kernels.logsumexp(xd, ws=wl)
        for k in range(64):
            idx = int(_np(kernels.categorical_pick(xd, l4, (k, 99), rng, off, ws=ws))[1]) - off
            assert 0 <= idx < K and not np.isnan(x[idx])


@pytest.mark.parametrize("K", R.SIZES)
def test_ess(K):
    from genjax_amd import kernels
    ws = kernels.workspace(A.OP_RESAMPLE, K)
    for fam, x in R.families(K).items():
        for pname, y, z in _cases(x, K):
            got, sub = _np(kernels.ess(_dev(y), ws=ws)), _np(kernels.ess(_dev(z), ws=ws))
            np.testing.assert_array_equal(_bits(got), _bits(sub), err_msg=f"K={K} {fam} {pname}")
            ref = R.ess(y)
            assert got[0] == np.float32(ref[0])
            if ref[0] == -np.inf:
                np.testing.assert_array_equal(got, np.array([-np.inf, 0, 0, 0], np.float32))
            else:
                np.testing.assert_allclose(got[1:], ref[1:], rtol=1e-4, err_msg=f"K={K} {fam} {pname}")


def _linear(y):
    """float32 linear weights exp(y - max) of log-weights y: NaN stays NaN, -inf becomes 0 or (every other one) a negative weight"""
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.float32(R.lse_record(y)[0])
        a = np.exp(y - m, dtype=np.float32) if np.isfinite(m) else np.where(np.isnan(y), np.float32(np.nan), np.float32(0.0))
    neg = np.flatnonzero(np.isneginf(y))[::2]
    a[neg] = -0.5
    return a.astype(np.float32)


@pytest.mark.parametrize("K", R.SIZES)
def test_cumsum_and_resamplers(oracle, K):
    import torch
    from genjax_amd import kernels
    ws, wl = kernels.workspace(A.OP_RESAMPLE, K), kernels.workspace(A.OP_LSE, K)
    rows = np.random.default_rng(K).standard_normal((3, K)).astype(np.float32)
    rd = _dev(rows)
    u = 0.37
    Ns = sorted({K, max(1, K // 3), 2 * K + 1})
    worst_rel = 0.0
    for fam, x in R.families(K).items():
        for pname, y, z in _cases(x, K):
            for is_log in (True, False):
                what = f"K={K} {fam} {pname} log={is_log}"
                ay, az = (y, z) if is_log else (_linear(y), np.where(np.isnan(_linear(y)), np.float32(-np.inf), _linear(y)))
                yd, zd = _dev(ay), _dev(az)
                l4 = kernels.logsumexp(yd, ws=wl) if is_log else None
                cum, bt = kernels.weight_cumsum(yd, is_log, l4, ws=ws)
                cum_z, bt_z = kernels.weight_cumsum(zd, is_log, l4, ws=ws)
                assert torch.equal(cum, cum_z) and torch.equal(bt, bt_z), what
                cum_n = _np(cum).view(np.uint64)
                assert _np(bt).tolist() == [0, int(cum_n[-1])]
                lv = R.weights64(ay, is_log) > 0
                q = np.diff(np.concatenate([[0], cum_n.astype(np.int64)]))
                assert (q[~lv] == 0).all(), what
                if is_log:
                    q64 = R.fixed_point(ay, True, float(_np(l4)[0]) if lv.any() else None).astype(np.float64)
                    if (q64 > 0).any():                         # (measured: how much of the derived REL_LOG the device uses)
                        worst_rel = max(worst_rel, float(((np.abs(q - q64) - 1.0)[q64 > 0] / q64[q64 > 0]).max()) / R.REL_LOG)
                    assert (np.abs(q - q64) <= 1.0 + R.REL_LOG * q64).all(), what
                else:
                    cum_o, tot_o = oracle.weight_cumsum(ay)
                    np.testing.assert_array_equal(cum_n, cum_o, err_msg=what)
                    np.testing.assert_array_equal(q, R.fixed_point(ay, False).astype(np.int64), err_msg=what)
                for N in Ns:
                    anc = _np(kernels.resample_indices(yd, u, N, is_log, l4, ws=ws))
                    anc_z = _np(kernels.resample_indices(zd, u, N, is_log, l4, ws=ws))
                    np.testing.assert_array_equal(anc, anc_z, err_msg=what)
                    status = kernels.workspace_status(ws, raise_on_error=False)
                    if not lv.any():                            # nothing to resample from: identity ancestors, status bit 1
                        np.testing.assert_array_equal(anc, np.arange(N) % K, err_msg=what)
                        assert status == 2, what
                        continue
                    assert status == 0, what
                    np.testing.assert_array_equal(anc, oracle.resample_systematic(cum_n, u, N), err_msg=what)
                    counts = np.bincount(anc, minlength=K)
                    assert counts[~lv].sum() == 0, f"{what}: a dead particle has offspring"
                    w = R.weights64(ay, is_log)
                    assert (np.abs(counts - N * w / w.sum()) < R.offspring_bound(ay, N, is_log)).all(), f"{what} N={N}"
                a1, a2 = (torch.empty(K, dtype=torch.int32, device="cuda") for _ in range(2))
                ch = kernels.resample_gather(yd, u, rd, is_log, l4, anc=a1, ws=ws, allow_fallback=False)
                ch_z = kernels.resample_gather(zd, u, rd, is_log, l4, anc=a2, ws=ws, allow_fallback=False)
                assert torch.equal(ch, ch_z) and torch.equal(a1, a2), what
                status = kernels.workspace_status(ws, raise_on_error=False)
                if not lv.any():
                    assert torch.equal(ch, rd) and status == 2, what
                else:
                    want = oracle.resample_systematic(cum_n, u, K)
                    np.testing.assert_array_equal(_np(a1), want, err_msg=what)
                    np.testing.assert_array_equal(_np(ch), rows[:, want], err_msg=what)
                    assert status == 0, what
    print(f"weight_cumsum K={K}: worst (|q - q64| - 1) / q64 = {worst_rel:.3f} x REL_LOG")


# ---- the host layer: a model that scores NaN for a known subset of its particles --------------------------------------------------
CUT, Y_OBS, K_HOST = 0.4, 0.7, 1500          # (1500: six blocks of the resampler, two of gjx_logsumexp's first kernel, no multiple of 256)


@genjax.gen
def holed_model():
    """the likelihood mean is a * (ok / ok), ok = where(a > CUT, 0, 1): 0 / 0 = NaN exactly for the particles with a > CUT, a elsewhere"""
    a = genjax.normal(0.0, 1.0) @ "a"
    ok = genjax.where(a > CUT, 0.0, 1.0)
    genjax.normal(a * (ok / ok), 1.0) @ "y"


def _holed_collection():
    """ImportanceK on holed_model with y observed: about a third of the particles score NaN.
    -> (the collection as run_smc leaves it, a float32[K], dead bool[K])"""
    from genjax_amd import C
    from genjax_amd.inference import ImportanceK, Target
    pc = ImportanceK(Target(holed_model, (), C["y"].set(Y_OBS)), k_particles=K_HOST).run_smc(genjax.key(11))
    a = _np(pc.get_particles().get_choices()["a"]).astype(np.float32).reshape(-1)
    dead = a > np.float32(CUT)
    logw = _np(pc.get_log_weights())
    assert 0.2 * K_HOST < dead.sum() < 0.5 * K_HOST
    np.testing.assert_array_equal(np.isnan(logw), dead, err_msg="the model scores NaN exactly where a > CUT")
    a64 = a.astype(np.float64)[~dead]
    np.testing.assert_allclose(logw[~dead], -0.5 * (Y_OBS - a64) ** 2 - 0.5 * np.log(2 * np.pi), rtol=1e-5, atol=1e-5)
    return pc, a, dead


def test_collection_with_nan_scores(oracle):
    """ParticleCollection over the model's NaN log-weights, its record taken from the log-weights (no producer's partials: what
    ``pareto_smoothed``, ``TrialCollections.trial`` and every collection built from weights alone hold): the log-ML estimate, the
    effective sample size, ``sample_particle`` and ``inference.resample`` agree with the float64 reference on the live subset."""
    from genjax_amd import kernels
    from genjax_amd.inference import ParticleCollection, pf, resample
    run, a, dead = _holed_collection()
    pc = ParticleCollection(run.get_particles(), run.get_log_weights(), True, None, run.offset, run.K_total)
    logw = _np(pc.get_log_weights())
    live_only = logw[~dead]
    K = K_HOST
    _, per_thread = R.lse_grid(K)
    rec = _np(pc.lse())
    ref = R.lse_record(logw)
    np.testing.assert_array_equal(ref, R.lse_record(np.concatenate([live_only, np.full(int(dead.sum()), -np.inf)])))   # (the live subset alone)
    _check_record(rec, ref, R.lse_tolerance(logw, per_thread, R.C_LSE["logsumexp"]), R.bound_lse(logw, per_thread, 1.0), "logsumexp", "host")
    lml = float(pc.get_log_marginal_likelihood_estimate())
    assert lml == rec[3] and abs(lml - (ref[2] - np.log(K))) <= R.lse_tolerance(logw, per_thread, R.C_LSE["logsumexp"])[3]
    np.testing.assert_allclose(float(pc.effective_sample_size()), R.ess(live_only)[3], rtol=1e-4)
    rng = pc.get_particles().prog.rng_mode
    for k in range(16):                                          # sample_particle: the oracle's pick, never a dead particle
        key = genjax.key(100 + k)
        want = oracle.categorical_pick(logw, rec, (int(key[0]), int(key[1])), rng, 0)[1]
        assert not dead[want]
        got = _np(pc.sample_particle(key).get_choices()["a"]).reshape(-1)
        assert got.shape == (1,) and got[0] == a[want], (k, got, a[want])
    rows = run.get_particles().choices
    key = genjax.key(7)
    out, anc = resample(rows, pc.get_log_weights(), key, collection=pc, check=True)
    anc = _np(anc)
    assert not dead[anc].any(), "a particle with a NaN weight has offspring"
    cum, _ = kernels.weight_cumsum(pc.get_log_weights(), True, pc.lse())
    np.testing.assert_array_equal(anc, oracle.resample_systematic(_np(cum).view(np.uint64), pf._unit_from_key(key), K))
    np.testing.assert_array_equal(_np(out), _np(rows)[:, anc])
    w = R.weights64(logw, True)
    assert (np.abs(np.bincount(anc, minlength=K) - K * w / w.sum()) < R.offspring_bound(logw, K)).all()
    out3, anc3 = resample(rows, pc.get_log_weights(), key, collection=pc, n_out=K // 3, check=True)       # (the two-launch form)
    np.testing.assert_array_equal(_np(anc3), oracle.resample_systematic(_np(cum).view(np.uint64), pf._unit_from_key(key), K // 3))
    np.testing.assert_array_equal(_np(out3), _np(rows)[:, _np(anc3)])


def test_collection_record_from_run_partials_is_the_open_end():
    """The open end of DESIGN.md 6c, pinned so that it cannot change unnoticed: the collection exactly as ``run_smc`` returns it
    finishes its record from the block {max, sumexp} pairs the producing kernel left, and those sums are not under the rule.  What
    holds there: the effective sample size (gjx_ess on the log-weights) is the reference's; the record's maximum is the live maximum;
    its log-sum-exp entries are the reference's or NaN — never another finite number —; and the same weights in a collection of their
    own (the test above) are under the rule."""
    run, a, dead = _holed_collection()
    logw = _np(run.get_log_weights())
    np.testing.assert_allclose(float(run.effective_sample_size()), R.ess(logw)[3], rtol=1e-4)
    assert run.lse_partials() is not None, "run_smc without a proposal leaves its record to the block partials"
    rec = _np(run.lse())
    ref = R.lse_record(logw)
    _, per_thread = R.lse_grid(K_HOST)
    tol = R.lse_tolerance(logw, per_thread, R.C_LSE["logsumexp"])
    print(f"record from run partials {rec}, float64 on the live subset {ref}")
    assert rec[0] == np.float32(ref[0])
    for j in (1, 2, 3):
        assert np.isnan(rec[j]) or abs(rec[j] - ref[j]) <= tol[j], (j, rec, ref)
