"""Weighted cross-moments of pairs of particles on the device (gjx_weighted_cross_moments) against the float64 restatement of the
definition in tests/cross_moments_ref.py (checked against np.cov and traced paths in tests/test_cross_moments_cpu.py), then the
host surface: ParticleCollection.cross_covariance and smoothed_pair_moments of ScanHistory / ParticleHistory.

Tolerances are those of tests/test_gpu_moments.py, whose arithmetic the kernels share (eps = 1e-4; ranges over the live pairs):
    |mean - mean64|   <= eps range + 2^-22 |mean64|                                         (tol_mean, each side)
    |cross_rs - ref|  <= eps range_a,r range_b,s + 2^-40 |mean64_a,r mean64_b,s|            (tol_cross)
    stats within rel 1e-4 of float64, stats[0] (the maximum) exact.
Through the filters the bounds are those of tests/test_gpu_lineage.py (the 3e-5 is derived in its docstring: the total variation of
the descendant weights, the float32 log and exponential, the float32 store), over the surviving pairs of the step:
    |mean - ref| <= 3e-5 max|x| + tol_mean,      |cross_rs - ref| <= 3e-5 max|a_r - mean_a,r| max|b_s - mean_b,s| + tol_cross.
A pair of a recorded run is (x_t, x_{t-1}) as ``paths()`` gives them to a trajectory, so the comparison with float64 sums over
``h.paths()`` holds for every kind of run, and the two marginals of a pair are ``smoothed_moments`` at t and t-1.
The guard for a LIVE out-of-range index is not exercised on the device: a wrong guard would be a memory fault.  In k_cross_tiles an
index is compared once, ``(uint32_t)idx < (uint32_t)K_b`` right after the indices are loaded and in front of tile_head_t<true>, which
makes the particle dead; the gather reads rows_b[idx] only where e > 0 and that compare passed.  An out-of-range index on DEAD
particles is exercised: it must change nothing, and count nothing.
Worst error / bound ratios on an MI355X: see DESIGN.md section 5."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import genjax_amd as genjax
from genjax_amd import C
from genjax_amd import _abi as A
from cross_moments_ref import CrossRef
from lineage_ref import descendant_weights, ref_e64

KS = [1, 63, 64, 65, 1023, 1025, 4113]
SHAPES = [(1, 1), (3, 5), (16, 16), (16, 1)]
KINDS = [None, "sorted", "permutation", "random", "all_to_0"]


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _same(a: dict, b: dict):
    import torch
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k].contiguous(), b[k].contiguous()
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), k


def _xm(rows_a, rows_b, logw=None, index=None, ws=None):
    from genjax_amd import kernels
    return kernels.weighted_cross_moments(rows_a, rows_b, logw, index, ws)


def _host(d: dict):
    return {k: _np(v) for k, v in d.items()}


def _check(got: dict, ref: CrossRef, what=""):
    """got: numpy dict of one call.  Prints the worst error / tolerance ratios, then asserts."""
    st = got["stats"].astype(np.float64)
    ea, eb = np.abs(got["mean_a"] - ref.mean_a), np.abs(got["mean_b"] - ref.mean_b)
    ec = np.abs(got["cross"] - ref.cross)
    ratio = lambda e, t: np.max(e / np.maximum(t, 1e-300))
    print(f"[cross] {what}: mean_a err/tol {ratio(ea, ref.tol_mean_a):.3g}, mean_b {ratio(eb, ref.tol_mean_b):.3g}, "
          f"cross {ratio(ec, ref.tol_cross):.3g}, stats rel {np.max(np.abs(st[1:] - ref.stats[1:]) / ref.stats[1:]):.3g}")
    assert int(got["n_bad"][0]) == ref.n_bad
    assert st[0] == np.float32(ref.stats[0])
    np.testing.assert_allclose(st[1:], ref.stats[1:], rtol=1e-4)
    assert (ea <= ref.tol_mean_a).all(), (what, ea, ref.tol_mean_a)
    assert (eb <= ref.tol_mean_b).all(), (what, eb, ref.tol_mean_b)
    assert (ec <= ref.tol_cross).all(), (what, ec, ref.tol_cross)


def _weights(rs, K):
    return (2.0 * rs.standard_normal(K) - 37.0).astype(np.float32)


def _index(rs, K, K_b, kind):
    if kind is None:
        return None
    if kind == "sorted":
        a = np.sort(rs.integers(0, K_b, K))
    elif kind == "permutation":
        a = rs.permutation(K_b)[:K] if K_b >= K else rs.integers(0, K_b, K)
    elif kind == "random":
        a = rs.integers(0, K_b, K)
    else:
        a = np.zeros(K)
    return np.ascontiguousarray(a, np.int32)


def _rows(rs, n, K, logw=None):
    """N(0, r + 1) about offsets that alternate in sign and grow; row 1 (if any) has a large offset and a small spread — what an
    uncentred second moment loses; the last row follows the weights when they are given"""
    x = rs.standard_normal((n, K)) * (1.0 + np.arange(n))[:, None] + (10.0 * np.arange(n) * (-1.0) ** np.arange(n))[:, None]
    if n > 1:
        x[1] = 1000.0 + 0.01 * rs.standard_normal(K)
    if logw is not None and n > 2:
        x[n - 1] = 0.5 * logw + 0.3 * rs.standard_normal(K)
    return x.astype(np.float32)


_cases: dict = {}


def _case(K, n_a, n_b, K_b=None):
    """host (a, b, logw) with a correlated through every kind of index, and their device copies; made once and never written to"""
    key = (K, n_a, n_b, K_b)
    if key not in _cases:
        rs = np.random.default_rng(1000 * K + 16 * n_a + n_b)
        Kb = K if K_b is None else K_b
        logw = _weights(rs, K)
        b = _rows(rs, n_b, Kb)
        a = _rows(rs, n_a, K, logw)
        idx = {kind: _index(rs, K, Kb, kind) for kind in KINDS if not (kind is None and Kb < K)}
        _cases[key] = (a, b, logw, idx, _dev(a), _dev(b), _dev(logw), {k: _dev(v) for k, v in idx.items()})
    return _cases[key]


# ---- the kernel against float64 ----
@pytest.mark.parametrize("n_a,n_b", SHAPES)
@pytest.mark.parametrize("K", KS)
def test_against_float64(K, n_a, n_b):
    a, b, logw, idx, da, db, dlogw, didx = _case(K, n_a, n_b)
    for kind in KINDS:
        got = _xm(da, db, dlogw, didx[kind])
        assert got["stats"].shape == (4,) and got["mean_a"].shape == (n_a,) and got["mean_b"].shape == (n_b,)
        assert got["cross"].shape == (n_a, n_b) and got["n_bad"].shape == (1,) and got["n_bad"].dtype.is_floating_point is False
        _check(_host(got), CrossRef(a, b, logw, idx[kind]), f"K={K} {n_a}x{n_b} {kind}")
    eq = _xm(da, db, None, didx["sorted"])
    _check(_host(eq), CrossRef(a, b, None, idx["sorted"]), f"K={K} {n_a}x{n_b} equal weights")
    np.testing.assert_array_equal(_np(eq["stats"]), np.array([0, K, K, K], np.float32))


@pytest.mark.parametrize("K", [65, 4113])
def test_fewer_parents_than_particles(K):
    """K_b = 37 != K: every index kind but the identity, which the wrapper refuses"""
    a, b, logw, idx, da, db, dlogw, didx = _case(K, 3, 5, 37)
    assert b.shape == (5, 37)
    for kind in KINDS[1:]:
        _check(_host(_xm(da, db, dlogw, didx[kind])), CrossRef(a, b, logw, idx[kind]), f"K={K} K_b=37 {kind}")
    with pytest.raises(ValueError, match="index"):
        _xm(da, db, dlogw, None)
    more = _dev(np.concatenate([a, a[:, :9]], axis=1))      # K_b > K without an index: the first K parents
    _same(_xm(da, more, dlogw), _xm(da, da, dlogw))


@pytest.mark.parametrize("K", [1025, 1500])
def test_strided_and_unaligned_views_and_a_dirty_workspace(K):
    """slices of wider matrices (row stride > K) that start at column 1: rows, index and weights that are not 16-byte aligned take
    the scalar load path.  Same values, same lanes: bitwise the contiguous call.  The workspace needs no initialisation."""
    import torch
    from genjax_amd._lib import load
    a, b, logw, idx, da, db, dlogw, didx = _case(K, 3, 5)
    wa = torch.full((3, K + 9), float("nan"), device="cuda")
    wa[:, 1:K + 1] = da
    wb = torch.full((5, K + 13), float("nan"), device="cuda")
    wb[:, 1:K + 1] = db
    lw1 = torch.full((K + 3,), float("nan"), device="cuda")
    lw1[1:K + 1] = dlogw
    need = load().gjx_weighted_cross_moments_workspace_bytes(3, 5, K)
    big = torch.full((2 * need + 4096,), 255, dtype=torch.uint8, device="cuda")          # larger, and full of NaN bit patterns
    for kind in (None, "sorted", "random"):
        base = _xm(da, db, dlogw, didx[kind])
        i1 = None
        if kind is not None:
            i1 = torch.full((K + 3,), -7, dtype=torch.int32, device="cuda")              # (what lies around it is never read as an index)
            i1[1:K + 1] = didx[kind]
            i1 = i1[1:K + 1]
        va, vb = wa[:, 1:K + 1], wb[:, 1:K + 1]
        assert not va.is_contiguous() and va.stride() == (K + 9, 1) and vb.stride() == (K + 13, 1)
        for got in (_xm(va, db, dlogw, didx[kind]), _xm(da, vb, dlogw, didx[kind]), _xm(va, vb, lw1[1:K + 1], i1)):
            _same(got, base)
        _same(_xm(da, db, dlogw, didx[kind], ws=big), base)
        _same(_xm(da, db, dlogw, didx[kind], ws=big[:need]), base)
    _check(_host(_xm(wa[:, 1:K + 1], wb[:, 1:K + 1], lw1[1:K + 1], i1)), CrossRef(a, b, logw, idx["random"]), f"views K={K}")


def test_dead_particles_contribute_nothing():
    """weights -inf and NaN, with NaN and inf values in a there and indices that lead to NaN and inf parents: the results are those of
    the collection without these particles.  An index of -1 or K_b on DEAD particles gives bitwise the output of the same call with
    index 0 there, and n_bad == 0 (the compare that guards a live particle is not exercised: module docstring)."""
    K, n_a, n_b = 1500, 3, 5
    a, b, logw, idx, *_ = _case(K, n_a, n_b)
    a, logw = a.copy(), logw.copy()
    rs = np.random.default_rng(5)
    dead = rs.choice(K, 400, replace=False)
    dead = np.unique(np.concatenate([dead, np.arange(1024, 1100)]))        # with a run across the head of the second tile
    logw[dead[::2]] = -np.inf
    logw[dead[1::2]] = np.nan
    a[:, dead[::3]] = np.nan
    a[:, dead[1::3]] = np.inf
    a[:, dead[2::3]] = -np.inf
    K_b = K + 3                                                            # three parents no live particle has: NaN, inf, -inf
    b = np.concatenate([b, np.full((n_b, 1), np.nan), np.full((n_b, 1), np.inf), np.full((n_b, 1), -np.inf)], axis=1).astype(np.float32)
    index = idx["random"].copy()
    index[dead] = K + np.arange(dead.size) % 3
    live = np.isfinite(logw)
    assert live.sum() == K - dead.size
    da, db, dlogw = _dev(a), _dev(b), _dev(logw)
    got = _xm(da, db, dlogw, _dev(index))
    h = _host(got)
    assert all(np.isfinite(v).all() for v in h.values())
    ref = CrossRef(a, b, logw, index)
    _check(h, ref, "dead particles")
    _check(_host(_xm(_dev(a[:, live]), db, _dev(logw[live]), _dev(index[live]))), ref, "the same collection, compacted")
    outside, zero = index.copy(), index.copy()
    outside[dead[::2]] = -1
    outside[dead[1::2]] = K_b
    zero[dead] = 0
    g_out, g_zero = _xm(da, db, dlogw, _dev(outside)), _xm(da, db, dlogw, _dev(zero))
    _same(g_out, g_zero)
    _same(g_out, got)
    assert int(g_out["n_bad"][0]) == 0
    # without an index: NaN and inf parents AT the dead particles
    b2 = _case(K, n_a, n_b)[1].copy()
    b2[:, dead[::2]] = np.nan
    b2[:, dead[1::2]] = np.inf
    h2 = _host(_xm(da, _dev(b2), dlogw))
    assert all(np.isfinite(v).all() for v in h2.values())
    _check(h2, CrossRef(a, b2, logw), "dead particles, identity")


@pytest.mark.parametrize("K,at", [(1, 0), (63, 17), (1500, 1234), (4113, 4100)])
def test_one_live_pair_is_exact(K, at):
    a, b, logw, idx, *_ = _case(K, 3, 5)
    a, b = a.copy(), b.copy()
    lw = np.full(K, -np.inf, np.float32)
    lw[1::2] = np.nan
    lw[at] = logw[at]
    index = idx["random"]
    a[:, np.arange(K) != at] = np.nan
    b[:, np.arange(K) != index[at]] = np.nan
    for di in (_dev(index), None):
        got = _host(_xm(_dev(a), _dev(b) if di is not None else _dev(np.roll(b, at - index[at], axis=1)), _dev(lw), di))
        np.testing.assert_array_equal(got["mean_a"], a[:, at])
        np.testing.assert_array_equal(got["mean_b"], b[:, index[at]])
        np.testing.assert_array_equal(got["cross"], np.zeros((3, 5), np.float32))
        np.testing.assert_array_equal(got["stats"], np.array([logw[at], 1, 1, 1], np.float32))
        assert int(got["n_bad"][0]) == 0


@pytest.mark.parametrize("K", [63, 1500])
def test_no_live_particle_is_no_estimate(K):
    a, b, logw, idx, da, db, dlogw, didx = _case(K, 3, 5) if K == 1500 else _case(K, 16, 16)
    lw = np.full(K, -np.inf, np.float32)
    lw[::3] = np.nan
    for di in (didx["sorted"], None):
        got = _host(_xm(da, db, _dev(lw), di))
        np.testing.assert_array_equal(got["stats"], np.array([-np.inf, 0, 0, 0], np.float32))
        assert np.isnan(got["mean_a"]).all() and np.isnan(got["mean_b"]).all() and np.isnan(got["cross"]).all()
        assert int(got["n_bad"][0]) == 0


@pytest.mark.parametrize("kind", [None, "sorted", "random"])
def test_bit_reproducible(kind):
    import torch
    from genjax_amd._lib import load
    K = 4113
    a, b, logw, idx, da, db, dlogw, didx = _case(K, 16, 16)
    first = _xm(da, db, dlogw, didx[kind])
    need = load().gjx_weighted_cross_moments_workspace_bytes(16, 16, K)
    w1 = torch.full((need,), 255, dtype=torch.uint8, device="cuda")
    w2 = torch.full((3 * need + 64,), 0x3f, dtype=torch.uint8, device="cuda")
    _same(_xm(da, db, dlogw, didx[kind], ws=w1), first)
    _same(_xm(da, db, dlogw, didx[kind], ws=w2), first)
    _same(_xm(da, db, dlogw, didx[kind], ws=w1), _xm(da, db, dlogw, didx[kind], ws=w2))


# ---- consistency with the existing calls ----
@pytest.mark.parametrize("K,n", [(1025, 3), (4113, 16)])
def test_agrees_with_weighted_moments(K, n):
    """rows_b is rows_a and no index: the covariance of gjx_weighted_moments within its tolerance; the stats bitwise"""
    import torch
    from genjax_amd import kernels
    from test_gpu_moments import Ref
    a, b, logw, idx, da, db, dlogw, didx = _case(K, n, n)
    got = _xm(da, da, dlogw)
    cov = kernels.weighted_moments(da, dlogw, "cov")
    ref = Ref(a, logw)
    ec = np.abs(_np(got["cross"]).astype(np.float64) - _np(cov["cov"]))
    em = np.abs(_np(got["mean_a"]).astype(np.float64) - _np(cov["mean"]))
    print(f"[cross] vs weighted_moments K={K} n={n}: cross err/tol {np.max(ec / ref.tol_cov):.3g}, mean {np.max(em / ref.tol_mean):.3g}")
    assert (ec <= ref.tol_cov).all() and (em <= ref.tol_mean).all()
    assert (np.abs(_np(got["mean_b"]).astype(np.float64) - _np(cov["mean"])) <= ref.tol_mean).all()
    for index in (None, didx["random"]):                    # the weights alone decide the stats
        st = _xm(da, db, dlogw, index)["stats"]
        assert torch.equal(st.view(torch.int32), cov["stats"].view(torch.int32))
    eq = _xm(da, db, None, didx["sorted"])["stats"]
    assert torch.equal(eq.view(torch.int32), kernels.weighted_moments(da, None, "cov")["stats"].view(torch.int32))


def test_steps_variant_is_bitwise_the_single_call():
    import torch
    from genjax_amd import kernels
    K = 1500
    a, b, logw, idx, da, db, dlogw, didx = _case(K, 3, 5)
    rs = np.random.default_rng(3)
    lw = torch.stack([dlogw, _dev(_weights(rs, K)), torch.zeros(K, device="cuda")])
    wide = torch.full((5, K + 9), float("nan"), device="cuda")
    wide[:, 1:K + 1] = db
    steps = [(da, db, didx["sorted"], 0), (da, wide[:, 1:K + 1], didx["random"], 2), (da, db, None, 1), (da, db, didx["all_to_0"], 1)]
    got = kernels.weighted_cross_moments_steps(steps, lw)
    assert got["stats"].shape == (4, 4) and got["mean_a"].shape == (4, 3) and got["mean_b"].shape == (4, 5)
    assert got["cross"].shape == (4, 3, 5) and got["n_bad"].shape == (4,)
    for t, (ra, rb, index, tw) in enumerate(steps):
        one = _xm(ra, rb, lw[tw], index)
        _same({k: v[t].reshape(one[k].shape) for k, v in got.items()}, one)


# ---- the host surface ----
DXM = 2


def test_cross_covariance_of_two_sites():
    """ImportanceK over a 3-step linear-Gaussian scan: Cov[x_1, x_0] between two sites of one trace, against float64 on the trace"""
    from genjax_amd import workloads
    from genjax_amd.inference import ImportanceK, Target
    from test_gpu_moments import Ref
    s = workloads.ssm_problem(dx=DXM, T=12)
    Am, q, r = np.asarray(s["A"], np.float32), float(s["q"]), float(s["r"])

    @genjax.gen
    def step(x_prev, _):
        x = genjax.mv_normal_diag(Am @ x_prev, np.full(DXM, q, np.float32)) @ "x"
        genjax.mv_normal_diag(x, np.full(DXM, r, np.float32)) @ "y"
        return x, None

    T, K = 3, 1500
    ys = np.asarray(s["y"], np.float32)[:T]
    pc = ImportanceK(Target(step.scan(n=T), (np.zeros(DXM, np.float32), None), C["y"].set(ys)), k_particles=K).run_smc(genjax.key(5))
    tr = pc.get_particles()
    lw = _np(pc.get_log_weights())
    rows = lambda t: _np(tr.choices[tr.prog.slot_of[("x", t)]:tr.prog.slot_of[("x", t)] + DXM])
    for ta, tb in ((1, 0), (2, 1), (0, 2)):
        got = pc.cross_covariance(("x", ta), ("x", tb))
        assert got.shape == (DXM, DXM) and got.is_cuda
        ref = CrossRef(rows(ta), rows(tb), lw)
        err = np.abs(_np(got) - ref.cross)
        print(f"[cross] pc.cross_covariance x_{ta} x_{tb}: err/tol {np.max(err / ref.tol_cross):.3g}")
        assert (err <= ref.tol_cross).all()
    assert np.abs(CrossRef(rows(1), rows(0), lw).cross).max() > 10 * CrossRef(rows(1), rows(0), lw).tol_cross.max()     # something to find
    same = np.abs(_np(pc.cross_covariance(("x", 1), ("x", 1))).astype(np.float64) - _np(pc.covariance(("x", 1))))
    assert (same <= Ref(rows(1), lw).tol_cov).all()
    with pytest.raises(KeyError):
        pc.cross_covariance(("x", 1), "nope")


# ---- through the filters (the runs of tests/test_gpu_lineage.py) ----
DX, T_RUN, K_RUN = 4, 8, 1 << 12


def _problem():
    from genjax_amd import workloads
    return workloads.ssm_problem(dx=DX, T=T_RUN, r=2.0)


def _lgssm_scan(s):
    """the linear-Gaussian state space as @gen + .scan (x_0 ~ N(0, q)), as tests/test_gpu_scan_filter.py writes it"""
    Am = np.asarray(s["A"], np.float32)
    q, r = float(s["q"]), float(s["r"])

    @genjax.gen
    def step(x_prev, _):
        x = genjax.mv_normal_diag(Am @ x_prev, np.full(DX, q, np.float32)) @ "x"
        genjax.mv_normal_diag(x, np.full(DX, r, np.float32)) @ "y"
        return x, None

    return step.scan(n=T_RUN), np.zeros(DX, np.float32)


_runs: dict = {}


def _run(which):
    """-> (history, args of its per-name methods, rows(t) -> (float32 rows [DX][K] on the host, the step whose weights they stand under),
    ancestors i32[T-1][K] on the host); made once per kind and never written to"""
    if which in _runs:
        return _runs[which]
    import torch
    from genjax_amd import core
    from genjax_amd.inference import BootstrapFilter
    s = _problem()
    ys = np.asarray(s["y"], np.float32)
    if which == "hand_written":
        from genjax_amd.inference.pf import LinearGaussianSSM
        bf = BootstrapFilter(LinearGaussianSSM(s["A"], s["q"], s["r"]), K_RUN)
        h = bf.run(core.key(3), s["y"], keep_history=True)["history"]
        name = ()
        anc = _np(torch.stack(h.ancestors))
        rows = lambda t: (_np(h.states[t]), t)
    else:
        scan, carry0 = _lgssm_scan(s)
        kw = dict(plain={}, moved=dict(rejuvenate=dict(n_moves=2, scale=0.35)), adaptive=dict(ess_threshold=0.5))[which]
        bf = BootstrapFilter(scan, K_RUN, **kw)
        h = bf.run(genjax.key(3), C["y"].set(ys), (carry0, None), keep_history=True)["history"]
        name = ("x",)
        anc = _np(h.ancestors)
        assert h.moved == (which == "moved")

        def rows(t):
            if which == "moved" and t < T_RUN - 1:       # the moved carry in step t+1's INPUT rows at the child's index, as paths() defines it
                prog = h.programs[t + 1]
                r0 = [prog.slot_of[sx.addr] for sx in prog.site_list.sites if prog.modes.get(sx.addr) == A.MODE_INPUT][0]
                return _np(h.rows_all[t + 1, r0:r0 + DX]), t + 1
            return _np(h.step(t, "x")), t
    assert len(h) == T_RUN and anc.shape == (T_RUN - 1, K_RUN)
    _runs[which] = (h, name, rows, anc)
    return _runs[which]


@pytest.mark.parametrize("which", ["plain", "moved", "adaptive", "hand_written"])
def test_smoothed_pair_moments_of_a_filter_run(which):
    import torch
    h, name, rows, anc = _run(which)
    K, T = K_RUN, T_RUN
    logw = _np(h.logw)
    e = ref_e64(logw, K)
    wref = descendant_weights(anc, e) / e.sum()            # float64 [T][K]
    pm = h.smoothed_pair_moments(*name)
    assert sorted(pm) == ["cross", "ess", "mean", "mean_prev"]
    assert pm["mean"].shape == (T - 1, DX) and pm["mean_prev"].shape == (T - 1, DX) and pm["cross"].shape == (T - 1, DX, DX)
    assert pm["ess"].shape == (T - 1,) and pm["cross"].is_cuda
    mean, prev, cross, ess = (_np(pm[k]).astype(np.float64) for k in ("mean", "mean_prev", "cross", "ess"))
    sm = _np(h.smoothed_moments(*name)["mean"]).astype(np.float64)
    P = _np(h.paths(*name)).astype(np.float64)             # [T][DX][K]: the trajectories
    wl = _np(torch.softmax(h.logw.double(), dim=0))
    surv = _np(h.survivors())
    assert np.isfinite(ess).all() and (ess >= 1.0).all() and (ess <= surv[T - 1]).all()
    worst = dict(mean=0.0, prev=0.0, cross=0.0, p_mean=0.0, p_prev=0.0, p_cross=0.0, sm=0.0, sm_prev=0.0)
    for t in range(1, T):
        (xa, ta), (xb, tb) = rows(t), rows(t - 1)
        assert tb in (ta, ta - 1)
        with np.errstate(divide="ignore"):
            ref = CrossRef(xa, xb, np.log(wref[ta]), None if tb == ta else anc[tb])
        assert ref.n_bad == 0
        al, bl = ref.a.astype(np.float64), ref.b.astype(np.float64)                  # the surviving pairs
        b_mean = 3e-5 * np.abs(al).max(axis=1) + ref.tol_mean_a
        b_prev = 3e-5 * np.abs(bl).max(axis=1) + ref.tol_mean_b
        b_cross = 3e-5 * np.outer(np.abs(al - ref.mean_a[:, None]).max(axis=1), np.abs(bl - ref.mean_b[:, None]).max(axis=1)) + ref.tol_cross
        # float64 over the paths under softmax(logw)
        pa, pb = P[t] @ wl, P[t - 1] @ wl
        pc = ((P[t] - pa[:, None]) * wl) @ (P[t - 1] - pb[:, None]).T
        errs = dict(mean=(np.abs(mean[t - 1] - ref.mean_a), b_mean), prev=(np.abs(prev[t - 1] - ref.mean_b), b_prev),
                    cross=(np.abs(cross[t - 1] - ref.cross), b_cross),
                    p_mean=(np.abs(mean[t - 1] - pa), b_mean), p_prev=(np.abs(prev[t - 1] - pb), b_prev), p_cross=(np.abs(cross[t - 1] - pc), b_cross),
                    sm=(np.abs(mean[t - 1] - sm[t]), b_mean), sm_prev=(np.abs(prev[t - 1] - sm[t - 1]), b_prev))
        for k, (err, bound) in errs.items():
            worst[k] = max(worst[k], float((err / bound).max()))
        for k, (err, bound) in errs.items():
            assert (err <= bound).all(), (which, t, k, err, bound)
    print(f"[cross] {which}: worst error/bound vs the reference: mean {worst['mean']:.3g}, mean_prev {worst['prev']:.3g}, cross {worst['cross']:.3g}; "
          f"vs paths(): {worst['p_mean']:.3g}, {worst['p_prev']:.3g}, {worst['p_cross']:.3g}; "
          f"vs smoothed_moments: mean {worst['sm']:.3g}, mean_prev {worst['sm_prev']:.3g}; survivors {surv.tolist()}")
    assert np.abs(cross).max() > 0.01                       # the dynamics correlate a state with its parent: something to find


def test_a_name_the_history_cannot_serve_raises_like_smoothed_moments():
    h = _run("moved")[0]
    with pytest.raises(NotImplementedError, match="does not receive"):
        h.smoothed_pair_moments("y")                        # (no step receives the observation as carry)
    with pytest.raises(KeyError):
        _run("plain")[0].smoothed_pair_moments("nope")


class _Record:
    """the least a record supplies to LineageSmoothing"""

    def __init__(self, x, anc, logw):
        self.x, self.anc, self.logw = x, anc, logw

    def _ancestor_table(self):
        return self.anc

    def _smoothing_rows(self, t, name):
        return self.x[t], t


def test_one_step_is_empty_and_more_than_16_components_are_refused():
    import torch
    from genjax_amd.inference.smoothing import LineageSmoothing

    class Rec(_Record, LineageSmoothing):
        pass

    K = 65
    one = Rec(torch.randn((1, 3, K), device="cuda"), torch.zeros((0, K), dtype=torch.int32, device="cuda"), torch.zeros(K, device="cuda"))
    pm = one._smoothed_pair_moments(None)
    assert pm["mean"].shape == (0, 3) and pm["mean_prev"].shape == (0, 3) and pm["cross"].shape == (0, 3, 3) and pm["ess"].shape == (0,)
    wide = Rec(torch.randn((2, 17, K), device="cuda"), torch.zeros((1, K), dtype=torch.int32, device="cuda"), torch.zeros(K, device="cuda"))
    with pytest.raises(ValueError, match="16"):
        wide._smoothed_pair_moments(None)
    two = Rec(torch.randn((2, 16, K), device="cuda"), torch.arange(K, dtype=torch.int32, device="cuda").reshape(1, K), torch.zeros(K, device="cuda"))
    pm = two._smoothed_pair_moments(None)
    assert pm["cross"].shape == (1, 16, 16)
    ref = CrossRef(_np(two.x[1]), _np(two.x[0]))
    assert (np.abs(_np(pm["cross"][0]) - ref.cross) <= ref.tol_cross).all()
