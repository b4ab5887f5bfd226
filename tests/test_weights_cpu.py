"""tests/weights_ref.py against NumPy on finite inputs and against its own rule by construction, and the CPU oracle held to the rule
of include/gjx.h, "Non-finite weights": a log-weight of -inf or NaN is dead wherever it sits, a collection without a live particle
gives {-inf, 0, -inf, -inf}, the first index and zero totals, a live +inf makes the log-sum-exp +inf."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from genjax_amd import _abi as A
import weights_ref as R

KS = [1, 2, 65, 257, 513, 1025]
DEAD = np.array([-np.inf, 0.0, -np.inf, -np.inf])


def _positions(K):
    return sorted({0, K // 2, K - 1})


def test_reference_against_numpy_on_finite_inputs():
    for K in R.SIZES:
        for name, x in R.families(K).items():
            if not np.isfinite(x).all():
                continue
            x64 = x.astype(np.float64)
            want = np.logaddexp.reduce(x64)
            rec = R.lse_record(x, 3 * K + 1)
            assert rec[0] == x64.max()
            assert abs(rec[2] - want) <= 1e-12 * max(1.0, abs(want)), (K, name)
            assert abs(rec[3] - (want - np.log(3 * K + 1))) <= 1e-12 * max(1.0, abs(want))
            assert abs(rec[1] - np.exp(x64 - x64.max()).sum()) <= 1e-12 * rec[1]
            e = np.exp(x64 - x64.max())
            assert abs(R.ess(x)[3] - e.sum() ** 2 / (e * e).sum()) <= 1e-9 * K
            # two halves combined == the whole
            if K > 1:
                a, b = R.lse_record(x[: K // 2]), R.lse_record(x[K // 2:])
                both = R.lse_combine([a[0], a[1], b[0], b[1]], K)
                assert abs(both[2] - rec[2]) <= 1e-12 * max(1.0, abs(want))


def test_reference_against_scipy():
    import scipy.special as sp
    for K in (1, 65, 1025):
        for name, x in R.families(K).items():
            want = sp.logsumexp(x.astype(np.float64))          # (-inf entries are fine for scipy; the families hold no NaN)
            assert abs(R.lse_record(x)[2] - want) <= 1e-12 * max(1.0, abs(want)), (K, name)


def test_reference_dead_rule_by_construction():
    for K in (1, 2, 65, 257):
        fam = R.families(K)
        for name in ("normal3", "ramp_up", "dead30", "huge_neg_gap"):
            x = fam[name]
            for pos in range(K):                                # a NaN walked through every position
                y = x.copy(); y[pos] = np.nan
                z = x.copy(); z[pos] = -np.inf
                np.testing.assert_array_equal(R.lse_record(y, 2 * K), R.lse_record(z, 2 * K))
                np.testing.assert_array_equal(R.ess(y), R.ess(z))
                np.testing.assert_array_equal(R.fixed_point(y, True), R.fixed_point(z, True))
                assert R.fixed_point(y, True)[pos] == 0
        np.testing.assert_array_equal(R.lse_record(np.full(K, np.nan, np.float32)), DEAD)
        np.testing.assert_array_equal(R.ess(np.full(K, np.nan, np.float32)), [-np.inf, 0, 0, 0])
    # linear weights: <= 0 or NaN is dead
    np.testing.assert_array_equal(R.fixed_point(np.array([0.5, -1.0, np.nan, 0.0, 2.0], np.float32), False), [1 << 29, 0, 0, 0, 1 << 31])
    # +inf: the maximum is the result; an empty rank is empty whatever its sum holds
    rec = R.lse_record(np.array([0.0, np.inf, np.nan], np.float32), 7)
    assert rec[0] == rec[2] == rec[3] == np.inf
    np.testing.assert_array_equal(R.lse_combine([-np.inf, np.nan, 1.0, 2.0, -np.inf, np.inf], 5), R.lse_combine([1.0, 2.0], 5))
    np.testing.assert_array_equal(R.lse_combine([-np.inf, 3.0, -np.inf, np.nan], 5), DEAD)


@pytest.mark.parametrize("K", KS)
def test_oracle_logsumexp_under_the_rule(oracle, K):
    for name, x in R.families(K).items():
        want = R.lse_record(x, 2 * K)
        got = oracle.logsumexp(x, 2 * K)
        assert got[0] == np.float32(want[0])
        np.testing.assert_allclose(got[1:], want[1:], rtol=2e-7, atol=1e-6, err_msg=f"{K} {name}")
        for pos in _positions(K):
            y = x.copy(); y[pos] = np.nan
            z = x.copy(); z[pos] = -np.inf
            np.testing.assert_array_equal(oracle.logsumexp(y, 2 * K), oracle.logsumexp(z, 2 * K), err_msg=f"{K} {name} NaN at {pos}")
        for pname, poison in R.poisons(K).items():
            y, z = R.poisoned(x, poison)
            got = oracle.logsumexp(y, 2 * K)
            np.testing.assert_array_equal(got, oracle.logsumexp(z, 2 * K), err_msg=f"{K} {name} {pname}")
            if not R.live(y).any():
                np.testing.assert_array_equal(got, DEAD)
        y = x.copy(); y[K // 2] = np.inf
        if K > 1:
            y[0] = np.nan
        got = oracle.logsumexp(y, 2 * K)
        assert got[0] == got[2] == got[3] == np.inf, (K, name, got)


@pytest.mark.parametrize("rng", [A.RNG_FLAT, A.RNG_JAX32])
@pytest.mark.parametrize("K", KS)
def test_oracle_pick_under_the_rule(oracle, K, rng):
    off = 4321
    for name, x in R.families(K).items():
        for pos in _positions(K):
            y = x.copy(); y[pos] = np.nan
            z = x.copy(); z[pos] = -np.inf
            ly, lz = oracle.logsumexp(y), oracle.logsumexp(z)
            for key in ((3, 9), (11, 5)):
                py, pz = oracle.categorical_pick(y, ly, key, rng, off), oracle.categorical_pick(z, lz, key, rng, off)
                assert py[1] == pz[1] and (py[0] == pz[0] or K == 1), (K, name, pos)
                if R.live(y).any():
                    assert R.live(y)[py[1] - off], f"{K} {name}: a dead particle was picked"
                else:
                    assert py[1] == off                           # no live particle: the first index of the collection
    dead = np.full(K, np.nan, np.float32)
    assert oracle.categorical_pick(dead, oracle.logsumexp(dead), (1, 2), rng, off)[1] == off


@pytest.mark.parametrize("K", KS)
def test_oracle_cumsum_and_resampler_under_the_rule_and_offspring_bound(oracle, K):
    for name, x in R.families(K).items():
        cases = [("clean", x, x)]
        for pos in _positions(K):
            y = x.copy(); y[pos] = np.nan
            z = x.copy(); z[pos] = -np.inf
            cases.append((f"NaN at {pos}", y, z))
        cases += [(p, *R.poisoned(x, v)) for p, v in R.poisons(K).items()]
        for what, y, z in cases:
            for is_log in (True, False):
                if is_log:
                    ly, lz = oracle.logsumexp(y), oracle.logsumexp(z)
                    (cy, ty), (cz, tz) = oracle.weight_cumsum(y, True, ly), oracle.weight_cumsum(z, True, lz)
                    ay, az = y, z
                else:                                             # linear weights exp(x - max): NaN stays NaN, -inf becomes 0
                    with np.errstate(invalid="ignore", over="ignore"):
                        m = np.float32(R.lse_record(y)[0])
                        ay = np.exp(y - m, dtype=np.float32) if np.isfinite(m) else np.where(np.isnan(y), np.float32(np.nan), np.float32(0))
                        az = np.where(np.isnan(ay), np.float32(0.0), ay)
                    (cy, ty), (cz, tz) = oracle.weight_cumsum(ay), oracle.weight_cumsum(az)
                np.testing.assert_array_equal(cy, cz, err_msg=f"{K} {name} {what} log={is_log}")
                assert ty == tz
                lv = R.weights64(ay, is_log) > 0
                q = np.diff(np.concatenate([[0], cy.astype(np.int64)]))
                assert (q[~lv] == 0).all()
                if not lv.any():
                    assert ty == 0
                    continue
                # the oracle's fixed point against the float64 one: one unit of truncation and the relative error of a float32 exp
                q64 = R.fixed_point(ay, is_log).astype(np.float64)
                assert (np.abs(q - q64) <= 1.0 + (R.REL_LOG if is_log else 0.0) * q64).all(), f"{K} {name} {what} log={is_log}"
                for N in sorted({K, max(1, K // 3), 2 * K + 1}):
                    anc = oracle.resample_systematic(cy, 0.37, N)
                    np.testing.assert_array_equal(anc, oracle.resample_systematic(cz, 0.37, N))
                    counts = np.bincount(anc, minlength=K)
                    assert counts[~lv].sum() == 0, f"{K} {name} {what}: a dead particle has offspring"
                    w = R.weights64(ay, is_log)
                    assert (np.abs(counts - N * w / w.sum()) < R.offspring_bound(ay, N, is_log)).all(), f"{K} {name} {what} N={N} log={is_log}"
