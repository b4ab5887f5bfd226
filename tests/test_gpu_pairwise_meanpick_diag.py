"""gjx_pairwise_gauss_mean_diag and gjx_pairwise_gauss_pick_diag (pairwise_gauss_mean / pairwise_gauss_pick with a precision matrix of
the keys) against the direct form bias[c] - 1/2 sum_i prec[i][c] (q - k)^2 in float64 on the same float32 numbers, and ffbs_pair_moments /
ffbs_sample_paths with per-particle precisions against the full K x K tables.  Data recipe, lse reference and score bound E_r are
test_gpu_pairwise_diag's (its C = 0.32).  Mean: (2 E_r + u (n_k / 4 + 8)) max_c |v[j][c]|, the rule of pairwise_mean_ref.py.  Pick: the
rule of pairwise_pick_ref.py over the diag cumulative, tol_r = 2 E_r + C_SUM u log2(n_k + 1).  NaN, -inf and -1 must match exactly.
Measured on an MI355X over the grid, the views and the edge cases, worst / allowed with the constant at 1: mean 0.008, lse 0.074 (d = 3,
n_q = n_k = 1), pick slack 0.000 (every pick inside its exact window): neither constant (0.32, C_SUM = 0.16) is exceeded."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pairwise_pick_ref as Pk
import pairwise_ref as R
import test_gpu_pairwise_diag as D
from test_gpu_pairwise_diag import dev

SHAPES = [(1, 1), (17, 65), (257, 194)]
DIMS = [1, 3, 8, 16]
CALLS = pytest.mark.parametrize("call", ["mean", "pick"])
SEED = 2                      # of the uniforms, chosen on the CPU: 22 of the grid's 1100 queries have a second acceptable key (28 is typical)


def case(d, n_q, n_k, dv=1):
    """test_gpu_pairwise_diag.case, with values and uniforms; in the large shape 0, 1, NaN and a value just inside either end are among
    them (at the ends the rule accepts every leading or trailing key of mass below tol: they are most of the ambiguous queries)"""
    q, k, b, prec, cen = D.case(d, n_q, n_k, "keys")
    rs = np.random.default_rng(SEED + 1000 * d + 10 * n_q + n_k)
    v, u = rs.standard_normal((dv, n_k)).astype(np.float32), rs.random(n_q).astype(np.float32)
    if n_q >= 100:
        u[:5] = 0.0, 1.0, np.nan, 1e-30, 1.0 - 2.0 ** -24
    return q, k, b, prec, cen, v, u


def weights(q, k, bias, prec):
    """-> (e f64[n_q][n_k] = exp(score - lse), 0 at dead keys, NaN rows where nothing can be normalised; lse f64[n_q]: D.ref's rules)"""
    lse = D.ref(q, k, bias, prec, "keys")
    b, live = R._live(bias, k.shape[1])
    e = np.zeros((q.shape[1], k.shape[1]))
    with np.errstate(all="ignore"):
        d2 = (prec.astype(np.float64)[:, None, live] * (q.astype(np.float64)[:, :, None] - k.astype(np.float64)[:, None, live]) ** 2).sum(0)
        e[:, live] = np.exp(b[live][None, :] - 0.5 * d2 - lse[:, None])
    e[~np.isfinite(lse)] = np.nan
    return e, lse


def check_mean(q, k, v, bias, prec, centre, what, call=None):
    from genjax_amd import kernels
    out = call() if call else kernels.pairwise_gauss_mean(dev(q), dev(k), dev(v), dev(bias), dev(prec), dev(centre))
    e, lse = weights(q, k, bias, prec)
    live = R._live(bias, k.shape[1])[1][None, :]
    with np.errstate(invalid="ignore"):
        vz = np.where(np.isfinite(v) & live, v, 0.0).astype(np.float64)
        want = vz @ e.T
    want[(~np.isfinite(v) & live).any(1)] = np.nan                               # a live key's non-finite value: its row
    allowed = lambda c: (2.0 * D.bound(q, k, bias, prec, "keys", centre, c) + R.U * (k.shape[1] / 4.0 + 8.0))[None, :] * np.abs(vz).max(1)[:, None]
    for name, got, ref, tol, tol1 in (("mean", out["mean"], want, allowed(D.C), allowed(1.0)),
                                      ("lse", out["lse"], lse, D.bound(q, k, bias, prec, "keys", centre), D.bound(q, k, bias, prec, "keys", centre, 1.0))):
        got, fin = got.cpu().numpy().astype(np.float64), np.isfinite(ref)
        np.testing.assert_array_equal(got[~fin], ref[~fin])
        if fin.any():
            err = np.abs(got - ref)
            print(f"pairwise diag {name} {what}: worst error / allowed(C = 1) = {(err[fin] / np.maximum(tol1[fin], 1e-300)).max():.3f}")
            assert (err[fin] <= tol[fin]).all(), (what, name)
    return out


def accept(pick, q, k, bias, prec, u, centre, c_sum=Pk.C_SUM):
    """pairwise_pick_ref.acceptable over the diag cumulative -> (ok, keys the rule accepts per query, slack in units of tol(C_SUM = 1))"""
    e, _ = weights(q, k, bias, prec)
    P = np.concatenate([np.zeros((len(u), 1)), np.cumsum(e, 1) / e.sum(1, keepdims=True)], 1)
    P[np.isnan(u)] = np.nan
    tol = lambda c: 2.0 * D.bound(q, k, bias, prec, "keys", centre) + c * Pk.U * np.log2(k.shape[1] + 1.0)
    uc, none, live = np.clip(u.astype(np.float64), 0.0, 1.0), np.isnan(P[:, -1]), R._live(bias, k.shape[1])[1]
    with np.errstate(invalid="ignore"):
        inside = live[None, :] & (P[:, :-1] - tol(c_sum)[:, None] <= uc[:, None]) & (uc[:, None] <= P[:, 1:] + tol(c_sum)[:, None])
        rows, c = np.arange(len(u)), np.clip(pick, 0, k.shape[1] - 1)
        out = np.maximum(np.maximum(P[rows, c] - uc, uc - P[rows, c + 1]), 0.0)
    ok = np.where(none, pick == -1, (pick >= 0) & inside[rows, c])
    return ok, inside.sum(1), np.where(none | (pick < 0), 0.0, out / tol(1.0))


def check_pick(q, k, bias, prec, u, centre, what, call=None):
    from genjax_amd import kernels
    out = call() if call else kernels.pairwise_gauss_pick(dev(q), dev(k), dev(u), dev(bias), dev(prec), dev(centre))
    pick, lse, ref = out["pick"].cpu().numpy(), out["lse"].cpu().numpy().astype(np.float64), D.ref(q, k, bias, prec, "keys")
    ok, _, slack = accept(pick, q, k, bias, prec, u, centre)
    print(f"pairwise diag pick {what}: worst slack / tol(C_SUM = 1) = {slack.max():.3f}")
    assert ok.all(), (what, np.flatnonzero(~ok)[:8], pick[~ok][:8])
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(lse[~fin], ref[~fin])
    assert (np.abs(lse[fin] - ref[fin]) <= D.bound(q, k, bias, prec, "keys", centre)[fin]).all(), what
    return out


def test_the_tolerance_pins_one_key():
    """float64 alone: over the whole grid the rule accepts a second key for at most 2 % of the queries"""
    n_acc = []
    for d in DIMS:
        for n_q, n_k in SHAPES:
            q, k, b, prec, cen, _, u = case(d, n_q, n_k)
            n_acc.append(accept(np.zeros(n_q, np.int64), q, k, b, prec, u, cen)[1])
    n_acc = np.concatenate(n_acc)
    print(f"pairwise diag pick: {np.mean(n_acc > 1):.4f} of {len(n_acc)} queries have a second acceptable key")
    assert np.mean(n_acc > 1) <= 0.02


@pytest.mark.parametrize("dv", [1, 17])
@pytest.mark.parametrize("n_q,n_k", SHAPES)
@pytest.mark.parametrize("d", DIMS)
def test_mean_matches_float64(d, n_q, n_k, dv):
    q, k, b, prec, cen, v, _ = case(d, n_q, n_k, dv)
    check_mean(q, k, v, b, prec, cen, f"d={d} n_q={n_q} n_k={n_k} dv={dv}")


@pytest.mark.parametrize("n_q,n_k", SHAPES)
@pytest.mark.parametrize("d", DIMS)
def test_picks_are_acceptable(d, n_q, n_k):
    q, k, b, prec, cen, _, u = case(d, n_q, n_k)
    check_pick(q, k, b, prec, u, cen, f"d={d} n_q={n_q} n_k={n_k}")


@CALLS
def test_odd_offset_row_strided_views_and_reproducibility(call):
    import torch
    from genjax_amd import kernels
    q, k, b, prec, cen, v, u = case(5, 257, 194, 17)
    wide = lambda a, off: torch.nn.functional.pad(dev(a), (off, 4 - off), value=float("nan"))[:, off:off + a.shape[1]]
    lib, F = kernels.load(), torch.full
    if call == "mean":
        run = lambda ws=None: kernels.pairwise_gauss_mean(wide(q, 1), wide(k, 3), wide(v, 1), dev(b), wide(prec, 3), dev(cen), ws)
        out, n = check_mean(q, k, v, b, prec, cen, "views", run), lib.gjx_pairwise_gauss_mean_diag_workspace_bytes(257, 194, 5, 17)
    else:
        run = lambda ws=None: kernels.pairwise_gauss_pick(wide(q, 1), wide(k, 3), dev(u), dev(b), wide(prec, 3), dev(cen), ws)
        out, n = check_pick(q, k, b, prec, u, cen, "views", run), lib.gjx_pairwise_gauss_pick_diag_workspace_bytes(257, 194, 5)
    again = run(F((n,), 0xFF, dtype=torch.uint8, device="cuda"))
    assert all(torch.equal(out[name].view(torch.int32), again[name].view(torch.int32)) for name in out)


@CALLS
@pytest.mark.parametrize("edge", ["dead", "all dead", "k inf", "q nan", "v inf", 0.0, np.inf, np.nan])
def test_edges(call, edge):
    """the outputs that are NaN, -inf or -1 are the definition's, exactly; a float is a precision entry of a live key"""
    q, k, b, prec, cen, v, u = case(3, 40, 130, 3)
    dead, live = ~(b > -np.inf), int(np.flatnonzero(b > -np.inf)[70])          # (live: a live key of the second tile)
    run = (lambda w: check_mean(q, k, v, b, prec, cen, w)) if call == "mean" else (lambda w: check_pick(q, k, b, prec, u, cen, w))
    before = run("before")
    if edge == "dead":                                       # dead keys hold NaN coordinates, precisions and values: the same bits
        k[:, dead], prec[:, dead], v[:, dead] = np.nan, np.nan, np.nan
    elif edge == "all dead":                                 # mean NaN, lse -inf, pick -1
        b[:] = -np.inf
    elif edge == "k inf":                                    # a poisoned live key: NaN / -1 everywhere
        k[1, live] = np.inf
    elif edge == "q nan":                                    # NaN / -1 for that query alone
        q[2, 7] = np.nan
    elif edge == "v inf":                                    # NaN for that value row (the pick has no values: nothing changes)
        v[1, live] = np.inf
    else:                                                    # a poisoned live key
        prec[1, live] = edge
    after = run(str(edge))
    same = all(np.array_equal(after[n].cpu().numpy(), before[n].cpu().numpy(), equal_nan=True) for n in before)
    assert same == (edge == "dead" or (edge == "v inf" and call == "pick"))


@CALLS
def test_constant_precision_agrees_with_the_isotropic_call(call):
    from genjax_amd import kernels
    import pairwise_mean_ref as M
    q, k, b, prec, cen, v, u = case(8, 257, 194, 17)
    prec[:] = 0.7
    if call == "mean":
        iso = kernels.pairwise_gauss_mean(dev(q), dev(k), dev(v), dev(b), 0.7, dev(cen))["mean"].cpu().numpy().astype(np.float64)
        diag = check_mean(q, k, v, b, prec, cen, "constant")["mean"].cpu().numpy()
        both = M.bound(q, k, v, b, 0.7, cen) + (2.0 * D.bound(q, k, b, prec, "keys", cen) + R.U * (194 / 4.0 + 8.0))[None, :] * np.abs(v).max(1)[:, None]
        assert (np.abs(diag - iso) <= both).all()
    else:                                                    # the isotropic pick under the diag rule widened by the isotropic tolerance
        iso = kernels.pairwise_gauss_pick(dev(q), dev(k), dev(u), dev(b), 0.7, dev(cen))["pick"].cpu().numpy()
        check_pick(q, k, b, prec, u, cen, "constant")
        extra = (Pk.tolerance(q, k, b, 0.7, cen) / (Pk.U * np.log2(195.0))).max()
        assert accept(iso, q, k, b, prec, u, cen, Pk.C_SUM + extra)[0].all()


def model(T=4, K=300, d=2):
    """test_gpu_pairwise_diag's x_{t+1} ~ N(0.9 x_t, diag(0.1 + x_t0^2, 1/2)); the third step's precision is a constant f32[d]"""
    rs = np.random.default_rng(11)
    x, P, lw = [rs.standard_normal((d, K)).astype(np.float32)], [], []
    for t in range(T):
        P.append(np.stack([1.0 / (0.1 + x[t][0] ** 2), np.full(K, 2.0)]).astype(np.float32) if t != 2 else np.tile(np.float32([[0.5], [2.0]]), K))
        lw.append(rs.standard_normal(K).astype(np.float32))
        x.append((0.9 * x[t] + rs.standard_normal((d, K)) / np.sqrt(P[t])).astype(np.float32))
    m = [np.float32(0.9) * x[t] for t in range(T)]
    bias = [(a.astype(np.float64) - np.logaddexp.reduce(a.astype(np.float64)) + 0.5 * np.log(p.astype(np.float64)).sum(0)).astype(np.float32)
            for a, p in zip(lw, P)]                          # the normalised weight and the parent's normaliser: what the calls get
    cen = [(a * np.exp(w.astype(np.float64) - np.logaddexp.reduce(w.astype(np.float64)))).sum(1) for a, w in zip(x, lw)]
    return x[:T], P, lw, m, bias, cen, ([dev(a) for a in x[:T]], [dev(a) for a in lw], [dev(a) for a in m], [dev(P[0]), dev(P[1]), dev(P[2][:, 0]), None])


def test_ffbs_pair_moments_with_state_dependent_precision():
    from cross_moments_ref import CrossRef
    from genjax_amd import kernels
    x, P, lw, m, bias, cen, args = model()
    got = {n: a.cpu().numpy().astype(np.float64) for n, a in kernels.ffbs_pair_moments(*args).items()}
    w = kernels.ffbs_weights(*args).cpu().numpy().astype(np.float64)           # (held to float64 by test_gpu_pairwise_diag)
    for t in range(1, len(x)):
        cond = weights(x[t], m[t - 1], bias[t - 1], P[t - 1])[0]                # f64[K][K]: parent i given child j
        pair = w[t][:, None] * cond
        mean, prev = x[t] @ pair.sum(1), x[t - 1] @ pair.sum(0)
        cross = (x[t] - mean[:, None]) @ pair @ (x[t - 1] - prev[:, None]).T
        # what gjx_weighted_cross_moments is allowed on (x_t, c), plus the error of c itself times the size of what it multiplies
        with np.errstate(divide="ignore"):
            tol = CrossRef(x[t], x[t - 1].astype(np.float64) @ cond.T, np.log(w[t]).astype(np.float32))
        extra = ((2.0 * D.bound(x[t], m[t - 1], bias[t - 1], P[t - 1], "keys", cen[t]).max() + R.U * (300 / 4.0 + 8.0))
                 * np.abs(x[t - 1]).max() * np.abs(x[t]).max())
        errs = {"mean": np.abs(got["mean"][t - 1] - mean) / (tol.tol_mean_a + extra),
                "mean_prev": np.abs(got["mean_prev"][t - 1] - prev) / (tol.tol_mean_b + extra),
                "cross": np.abs(got["cross"][t - 1] - cross) / (tol.tol_cross + extra)}
        print(f"ffbs diag pair t={t}: worst error / allowed " + ", ".join(f"{n} {e.max():.3g}" for n, e in errs.items()))
        assert all((e <= 1.0).all() for e in errs.values()), (t, errs)


def test_ffbs_sample_paths_with_state_dependent_precision():
    from genjax_amd import core, kernels
    x, P, lw, m, bias, cen, args = model()
    key, n = core.key(7), 100
    out = kernels.ffbs_sample_paths(*args, key, n)
    idx, paths = out["idx"].cpu().numpy(), out["paths"].cpu().numpy()
    assert idx.min() >= 0 and idx.max() < 300
    for t in range(len(x)):
        np.testing.assert_array_equal(paths[t], x[t][:, idx[t]])
    for t in range(len(x) - 2, -1, -1):                      # the kernel's own path: the query is the particle returned at t + 1
        bits = np.array([core.threefry2x32_py(key[0], key[1], t, j)[0] for j in range(n)], np.uint64)
        u = np.minimum(((bits >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24, 1.0 - 2.0 ** -24).astype(np.float32)
        ok, n_acc, _ = accept(idx[t], paths[t + 1], m[t], bias[t], P[t], u, cen[t + 1])
        assert ok.all() and np.mean(n_acc > 1) <= 0.05, t
