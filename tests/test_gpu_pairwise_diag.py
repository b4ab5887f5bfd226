"""gjx_pairwise_gauss_lse_diag (pairwise_gauss_lse with a precision matrix) against the direct form in float64 on the same float32
numbers, and ffbs_weights with per-particle precisions against the float64 recursion over the full K x K tables.  Finite outputs are
held to  E_r = C 2^-24 (2 d + 4) max_c sum_j P_j (q~_rj^2 + k~_cj^2) + 8 2^-24 (1 + log n_k)  (tildes: minus the call's centre, maximum
over live keys: pairwise_ref.bound with the 2 d features the kernel multiplies); -inf and NaN must match exactly."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pairwise_ref as R

C_MEASURED = 0.08             # worst error / bound(C = 1) on an MI355X over the shape grid and the views: 0.074 (keys side, d = 3,
C = 4.0 * C_MEASURED          # n_q = n_k = 1), rounded up; the queries side's worst is 0.063 (d = 1, n_q = 257, n_k = 194)
SIDES = pytest.mark.parametrize("side", ["keys", "queries"])


def ref(q, k, bias, prec, side):
    """the definition in float64, its edge rules included; q [d][n_q], k [d][n_k], prec [d][n_k] (side keys) or [d][n_q] -> [n_q]"""
    q, k, prec = (np.asarray(x, np.float64) for x in (q, k, prec))
    b, live = R._live(bias, k.shape[1])
    out = np.full(q.shape[1], -np.inf)
    with np.errstate(all="ignore"):
        if live.any():
            P = prec[:, None, live] if side == "keys" else prec[:, :, None]
            s = b[live][None, :] - 0.5 * (P * (q[:, :, None] - k[:, None, live]) ** 2).sum(0)
            out = s.max(1) + np.log(np.exp(s - s.max(1)[:, None]).sum(1))
        p_ok = (prec > 0) & (prec < np.inf)
    bad_k = not np.isfinite(k[:, live]).all() or (side == "keys" and not p_ok[:, live].all())     # a live key's: every output
    bad_q = ~np.isfinite(q).all(0) | (False if side == "keys" else ~p_ok.all(0))                  # a query's: its own
    return np.where(bad_q | bad_k, np.nan, out)


def bound(q, k, bias, prec, side, centre, c=C):
    q, k, prec, cen = (np.asarray(x, np.float64) for x in (q, k, prec, np.reshape(centre, (-1, 1))))
    _, live = R._live(bias, k.shape[1])
    P = prec[:, None, live] if side == "keys" else prec[:, :, None]
    with np.errstate(all="ignore"):
        t = (P * (((q - cen) ** 2)[:, :, None] + ((k[:, live] - cen) ** 2)[:, None, :])).sum(0).max(1, initial=0.0)
    return c * R.U * (2 * q.shape[0] + R.C0) * t + R.C1 * R.U * (1.0 + np.log(k.shape[1]))


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def check(q, k, bias, prec, side, centre, what, call=None):
    """one call (`call`, or the plain one on contiguous copies) against the definition; returns the device output"""
    from genjax_amd import kernels
    out = call() if call else kernels.pairwise_gauss_lse(dev(q), dev(k), dev(bias), dev(prec), dev(centre), precision_of=side)
    got, want = out.cpu().numpy().astype(np.float64), ref(q, k, bias, prec, side)
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[~fin], want[~fin])
    if fin.any():
        err = np.abs(got - want)[fin]
        print(f"pairwise diag {what} {side}: worst error / bound(C = 1) = {(err / bound(q, k, bias, prec, side, centre, 1.0)[fin]).max():.3f}")
        assert (err <= bound(q, k, bias, prec, side, centre)[fin]).all(), what
    return out


def case(d, n_q, n_k, side):
    """data at 1e3 + N(0, 1) with its centre, precisions log-uniform over 10^+-2, normalised log-weights, a quarter of the keys dead"""
    rs = np.random.default_rng(1000 * d + 10 * n_q + n_k)
    q, k = (1e3 + rs.standard_normal((d, n_q))).astype(np.float32), (1e3 + rs.standard_normal((d, n_k))).astype(np.float32)
    prec = (10.0 ** rs.uniform(-2, 2, (d, n_k if side == "keys" else n_q))).astype(np.float32)
    lw = 1.5 * rs.standard_normal(n_k)
    b = (lw - np.logaddexp.reduce(lw)).astype(np.float32)
    b[1:][rs.random(n_k - 1) < 0.25] = -np.inf
    return q, k, b, prec, k.astype(np.float64).mean(1).astype(np.float32)


@SIDES
@pytest.mark.parametrize("n_q,n_k", [(1, 1), (17, 65), (257, 194)])
@pytest.mark.parametrize("d", [1, 2, 3, 8, 16])
def test_matches_float64(d, n_q, n_k, side):
    q, k, b, prec, cen = case(d, n_q, n_k, side)
    check(q, k, b, prec, side, cen, f"d={d} n_q={n_q} n_k={n_k}")


@SIDES
def test_odd_offset_row_strided_views_and_reproducibility(side):
    import torch
    from genjax_amd import kernels
    q, k, b, prec, cen = case(5, 257, 194, side)
    wide = lambda a, off: torch.nn.functional.pad(dev(a), (off, 4 - off), value=float("nan"))[:, off:off + a.shape[1]]
    args = (wide(q, 1), wide(k, 3), dev(b), wide(prec, 1), dev(cen))
    out = check(q, k, b, prec, side, cen, "views", lambda: kernels.pairwise_gauss_lse(*args, precision_of=side))
    ws = torch.full((kernels.load().gjx_pairwise_gauss_lse_diag_workspace_bytes(257, 194, 5),), 0xFF, dtype=torch.uint8, device="cuda")
    again = kernels.pairwise_gauss_lse(*args, ws=ws, precision_of=side)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))


@SIDES
@pytest.mark.parametrize("edge", ["dead", "all dead", "k inf", "q nan", 0.0, np.inf, np.nan])
def test_edges(side, edge):
    """the outputs that are NaN or -inf are the definition's (ref), exactly; a float is a precision entry, a live key's or a query's"""
    q, k, b, prec, cen = case(3, 40, 130, side)
    dead, live = ~(b > -np.inf), int(np.flatnonzero(b > -np.inf)[70])          # (live: a live key of the second tile)
    before = check(q, k, b, prec, side, cen, "before").cpu().numpy()
    if edge == "dead":                                       # dead keys hold NaN coordinates and NaN precisions: the same bits
        k[:, dead] = np.nan
        if side == "keys":
            prec[:, dead] = np.nan
    elif edge == "all dead":                                 # -inf
        b[:] = -np.inf
    elif edge == "k inf":                                    # a live key with a non-finite coordinate: NaN everywhere
        k[1, live] = np.inf
    elif edge == "q nan":                                    # NaN for that query alone
        q[2, 7] = np.nan
    else:                                                    # keys: NaN everywhere; queries: NaN for that query alone
        prec[1, live if side == "keys" else 7] = edge
    got = check(q, k, b, prec, side, cen, str(edge)).cpu().numpy()
    assert np.array_equal(got, before) == (edge == "dead")


@SIDES
def test_constant_precision_agrees_with_the_isotropic_call(side):
    from genjax_amd import kernels
    q, k, b, prec, cen = case(8, 257, 194, side)
    prec[:] = 0.7
    iso = kernels.pairwise_gauss_lse(dev(q), dev(k), dev(b), 0.7, dev(cen)).cpu().numpy().astype(np.float64)
    diag = check(q, k, b, prec, side, cen, "constant").cpu().numpy()
    assert (np.abs(diag - iso) <= R.bound(q, k, b, 0.7, cen) + bound(q, k, b, prec, side, cen)).all()


def test_ffbs_weights_with_state_dependent_precision():
    """x_{t+1} ~ N(0.9 x_t, diag(0.1 + x_t0^2, 1/2)); the third step's precision is a constant anisotropic f32[d], the last is not read"""
    from genjax_amd import kernels
    rs, T, K, d = np.random.default_rng(11), 4, 300, 2
    x, P, lw = [rs.standard_normal((d, K)).astype(np.float32)], [], []
    for t in range(T):
        P.append(np.stack([1.0 / (0.1 + x[t][0] ** 2), np.full(K, 2.0)]).astype(np.float32) if t != 2 else np.tile(np.float32([[0.5], [2.0]]), K))
        lw.append(rs.standard_normal(K).astype(np.float32))
        x.append((0.9 * x[t] + rs.standard_normal((d, K)) / np.sqrt(P[t])).astype(np.float32))
    m = [np.float32(0.9) * x[t] for t in range(T)]
    w = kernels.ffbs_weights([dev(a) for a in x[:T]], [dev(a) for a in lw], [dev(a) for a in m],
                             [dev(P[0]), dev(P[1]), dev(P[2][:, 0]), None]).cpu().numpy().astype(np.float64)
    norm = lambda a: a.astype(np.float64) - np.logaddexp.reduce(a.astype(np.float64))
    want, per_call = [None] * (T - 1) + [norm(lw[T - 1])], 0.0
    for t in range(T - 2, -1, -1):
        Pt, ln = P[t].astype(np.float64), 0.5 * np.log(P[t].astype(np.float64)).sum(0)
        S = ln[:, None] - 0.5 * (Pt[:, :, None] * (x[t + 1].astype(np.float64)[:, None, :] - m[t].astype(np.float64)[:, :, None]) ** 2).sum(0)
        D = np.logaddexp.reduce(norm(lw[t])[:, None] + S, 0)                            # S[i][j] = log f(x_{t+1}^j | x_t^i)
        want[t] = norm(norm(lw[t]) + np.logaddexp.reduce(want[t + 1][None, :] - D[None, :] + S, 1))
        cen = (x[t + 1] * np.exp(norm(lw[t + 1]))).sum(1)                               # the smoother's centre
        per_call = max(per_call, bound(x[t + 1], m[t], None, P[t], "keys", cen).max(), bound(m[t], x[t + 1], None, P[t], "queries", cen).max())
    want = np.stack(want)
    worst = np.abs(np.log(w) - want)[want > np.log(2.0 ** -40)].max()
    print(f"ffbs diag: worst log-weight error {worst:.3e}, allowed {2 * T * per_call:.3e}")
    assert worst <= 2 * T * per_call and np.abs(w.sum(1) - 1.0).max() < 1e-5
