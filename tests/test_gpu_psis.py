"""gjx_pareto_smooth on the device against its NumPy restatement (tests/psis_ref.py): the tail is exactly the last M particles of the
stable order, everything outside it is copied bit for bit, cutoff and tail size are exact, and the smoothed values, k-hat and sigma
are within 2 float32 ulps of the restatement's float32 rounding — both sides evaluate the same float64 formulas and differ by the
order of their sums and last-place libm errors, which the profile likelihood amplifies by at most M ~ 6e3: about 1e-12 relative
against a float32 half-ulp of 3e-8.  A larger gap would mean float32 arithmetic in the fit."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import genjax_amd as genjax
from genjax_amd import C
import psis_ref as R

SIZES = [25, 50, 1000, 1024, 1025, 4113, (1 << 14) + 1]      # 25: M = 5, the smallest fit; one tile, one block, a partial last tile
ULPS = 2


def _pareto(rs, n):
    return R.pareto_weights(rs, n, 0.7)


def _normal(rs, n):
    return R.normal_ratio_weights(rs, n, 0.6)


def _quantised(rs, n):
    """log-weights rounded to quarters: ties run through the cutoff and through the quartile"""
    return (np.round(4 * 3.0 * rs.standard_normal(n)) / 4).astype(np.float32)


def _half_dead(rs, n):
    lw = R.pareto_weights(rs, n, 0.4, 0.0)
    lw[rs.random(n) < 0.5] = -np.inf
    lw[rs.random(n) < 0.05] = np.nan
    return lw


def _dominated(rs, n):
    lw = R.normal_ratio_weights(rs, n, 0.8)
    lw[rs.integers(0, n)] += 50.0
    return lw


def _high(rs, n):
    return R.pareto_weights(rs, n, 0.5, 3.0e4)


def _low(rs, n):
    return R.pareto_weights(rs, n, 0.5, -3.0e4)


FAMILIES = {"pareto": _pareto, "normal": _normal, "quantised": _quantised, "half_dead": _half_dead, "dominated": _dominated,
            "offset_high": _high, "offset_low": _low}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _call(lw, S=1, in_place=False):
    import torch
    from genjax_amd import kernels
    t = torch.from_numpy(np.ascontiguousarray(lw, np.float32)).cuda()
    res = kernels.pareto_smooth(t, S, out=t if in_place else None)
    if in_place:
        assert res["logw"].data_ptr() == t.data_ptr()
    out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}
    if not in_place:
        assert (_bits(t.cpu().numpy()) == _bits(lw)).all()      # the input is left alone
    return out


def _check(lw, S=1, in_place=False, what=""):
    """-> (worst ulp distance of the smoothed values, of k-hat, of sigma)"""
    got = _call(lw, S, in_place)
    ref_out, ref_fit = R.pareto_smooth(lw, S)
    n = lw.size // S
    M = R.tail_size(n)
    assert got["tail"] == M and (ref_fit[:, 3] == M).all()
    k, sigma, cutoff = (np.atleast_1d(got[name]) for name in ("k", "sigma", "cutoff"))
    assert k.shape == sigma.shape == cutoff.shape == (S,) and got["logw"].shape == (lw.size,)
    nan = np.isnan(ref_fit[:, 2])                            # (a dead particle just below the tail)
    assert (np.isnan(cutoff) == nan).all() and (_bits(cutoff[~nan]) == _bits(ref_fit[~nan, 2])).all(), what
    worst = [0, 0, 0]
    for s in range(S):
        seg, o, r = lw[s * n:(s + 1) * n], got["logw"][s * n:(s + 1) * n], ref_out[s * n:(s + 1) * n]
        tail = R.order(seg)[n - M:]
        rest = np.ones(n, bool)
        rest[tail] = False
        assert (_bits(o)[rest] == _bits(seg)[rest]).all(), (what, s)        # outside the tail: the input, bit for bit
        if np.isnan(ref_fit[s, 0]):                          # no estimate: a copy, NaN k-hat and sigma
            assert (_bits(o) == _bits(seg)).all() and np.isnan(k[s]) and np.isnan(sigma[s]), (what, s)
            continue
        d = R.ulp_distance(o[tail], r[tail])
        dk, ds = int(R.ulp_distance(k[s], ref_fit[s, 0])[0]), int(R.ulp_distance(sigma[s], ref_fit[s, 1])[0])
        worst = [max(worst[0], int(d.max())), max(worst[1], dk), max(worst[2], ds)]
        assert d.max() <= ULPS and dk <= ULPS and ds <= ULPS, (what, s, int(d.max()), dk, ds, float(k[s]), float(ref_fit[s, 0]))
        assert o[tail].max() <= np.nanmax(seg) and (np.diff(o[tail]) >= 0).all()
    print(f"psis ulp distance [{what}] n = {n}, S = {S}: smoothed {worst[0]}, k {worst[1]}, sigma {worst[2]}")
    return worst


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_against_the_restatement(family, n):
    rs = np.random.default_rng(1000 * n + len(family))
    _check(FAMILIES[family](rs, n), what=family)


def test_a_million_particles():
    lw = R.pareto_weights(np.random.default_rng(1), 1 << 20, 0.7)
    got = _call(lw)
    assert got["tail"] == 3072 and abs(float(got["k"]) - 0.7) <= 0.1
    _check(lw, what="pareto 2^20")


@pytest.mark.parametrize("S,n", [(50, 50), (3, 1025), (8, 1000)])
def test_segments_are_calls_on_each_segment(S, n):
    rs = np.random.default_rng(S * n)
    lw = np.concatenate([FAMILIES[name](rs, n) for name, _ in zip(list(FAMILIES) * S, range(S))])
    _check(lw, S, what="segments")
    whole = _call(lw, S)
    for s in range(S):
        one = _call(lw[s * n:(s + 1) * n])
        assert (_bits(one["logw"]) == _bits(whole["logw"][s * n:(s + 1) * n])).all()
        for name in ("k", "sigma", "cutoff"):
            assert _bits(one[name]) == _bits(whole[name][s]), (s, name)


@pytest.mark.parametrize("family,n", [("pareto", 4113), ("quantised", 1025), ("half_dead", (1 << 14) + 1)])
def test_in_place(family, n):
    lw = FAMILIES[family](np.random.default_rng(n), n)
    _check(lw, in_place=True, what=family + " in place")
    a, b = _call(lw), _call(lw, in_place=True)
    assert all((_bits(a[name]) == _bits(b[name])).all() for name in ("logw", "k", "sigma", "cutoff"))


@pytest.mark.parametrize("n", [4113, 1 << 20])
def test_two_calls_agree_bitwise(n):
    lw = _quantised(np.random.default_rng(n), n) if n < 1 << 20 else R.normal_ratio_weights(np.random.default_rng(n), n, 0.6)
    a, b = _call(lw), _call(lw)
    assert not np.isnan(a["k"])
    assert all((_bits(a[name]) == _bits(b[name])).all() for name in ("logw", "k", "sigma", "cutoff"))


def test_no_estimate_is_a_copy():
    rs = np.random.default_rng(3)
    dead = rs.standard_normal(1000).astype(np.float32)
    dead[95:] = -np.inf                                      # 95 live particles = M
    dead[500:600] = np.nan
    for what, lw, M in (("K = 24", rs.standard_normal(24).astype(np.float32), 4), ("equal", np.full(1000, -3.25, np.float32), 95),
                        ("live <= M", dead, 95), ("all dead", np.full(64, -np.inf, np.float32), 12),
                        ("K = 3", np.array([1.0, 3.0, 2.0], np.float32), 0), ("K = 1", np.array([0.5], np.float32), 0)):
        got = _call(lw)
        assert (_bits(got["logw"]) == _bits(lw)).all() and np.isnan(got["k"]) and np.isnan(got["sigma"]) and got["tail"] == M, what
        _check(lw, what=what)
    assert _call(np.array([1.0, 3.0, 2.0], np.float32))["cutoff"] == 3.0


# ---- through the API ----
def _beta_bernoulli():
    @genjax.gen
    def model():
        p = genjax.beta(2.0, 2.0) @ "p"
        v = genjax.flip(p) @ "v"
        return v
    return model


def test_collection_methods_on_the_readme_model():
    import torch
    from genjax_amd import kernels
    from genjax_amd.inference import ImportanceK, ParticleCollection, Target, pareto_k_threshold
    K = 1 << 14
    pc = ImportanceK(Target(_beta_bernoulli(), (), C["v"].set(True)), k_particles=K).run_smc(genjax.key(314159))
    direct = kernels.pareto_smooth(pc.log_weights)
    kh = pc.pareto_k()
    assert kh.dim() == 0 and kh.is_cuda and _bits(kh.cpu().numpy()) == _bits(direct["k"].cpu().numpy())
    assert float(kh) < pareto_k_threshold(K)                 # weights p <= 1: a bounded tail
    sm = pc.pareto_smoothed()
    assert isinstance(sm, ParticleCollection) and sm.particles is pc.particles and len(sm) == K
    assert sm.offset == pc.offset and sm.K_total == pc.K_total
    assert torch.equal(sm.log_weights, direct["logw"]) and sm.log_weights.data_ptr() == pc._pareto()["logw"].data_ptr()
    ref_out, ref_fit = R.pareto_smooth(pc.log_weights.cpu().numpy())
    assert int(R.ulp_distance(kh.cpu().numpy(), ref_fit[0, 0])[0]) <= ULPS
    mean, ess, lml = float(sm.mean("p")), float(sm.effective_sample_size()), float(sm.get_log_marginal_likelihood_estimate())
    assert np.isfinite([mean, ess, lml]).all()
    assert abs(mean - 0.6) < 0.02 and 0.5 * K < ess <= K and abs(lml - np.log(0.5)) < 0.02      # the posterior is Beta(3, 2), p(v) = 1/2
    assert abs(lml - float(pc.get_log_marginal_likelihood_estimate())) < 1e-3
    assert np.isfinite(float(sm.quantile("p", 0.5)))
    shard = ParticleCollection(pc.particles, pc.log_weights, K_total=2 * K)
    with pytest.raises(NotImplementedError):
        shard.pareto_k()
    with pytest.raises(NotImplementedError):
        shard.pareto_smoothed()


def test_trial_collections_are_their_trials():
    import torch
    from genjax_amd.inference import ImportanceK, Target, TrialCollections
    n, K = 6, 1000
    tc = ImportanceK(Target(_beta_bernoulli(), (), C["v"].set(True)), k_particles=K).run_smc_trials(genjax.key(314159), n)
    kh, sm = tc.pareto_k(), tc.pareto_smoothed()
    assert kh.shape == (n,) and isinstance(sm, TrialCollections) and sm.particles is tc.particles and (sm.n_trials, sm.K) == (n, K)
    for t in range(n):
        one = tc.trial(t)
        assert _bits(one.pareto_k().cpu().numpy()) == _bits(kh[t].cpu().numpy())
        assert torch.equal(one.pareto_smoothed().log_weights, sm.get_log_weights()[t])
    assert torch.isfinite(sm.moments().mean("p")).all() and torch.isfinite(sm.get_log_marginal_likelihood_estimates()).all()
    one = ImportanceK(Target(_beta_bernoulli(), (), C["v"].set(True)), k_particles=K).run_smc_trials(genjax.key(2), 1)
    assert one.pareto_k().shape == (1,)
