"""Adaptive resampling in the generic particle filter: ``BootstrapFilter(kernel.scan(n=T), K, ess_threshold=tau)`` ->
gjx_scan_filter_adaptive.  The weights are carried over the steps and the collection is resampled in front of a step only when its
effective sample size has fallen under tau K; the decision is taken on the device.  Checked against
  * the filter that resamples in front of every step (``ess_threshold=None``, two launches per step): tau = 1 is that filter,
  * the ORACLE (oracle/gjx_oracle.c on the very step programs the device ran) step by step, with the oracle's own tile-scaled
    resampler on the accumulated weights where the device resampled and the un-gathered carry where it did not,
  * float64 NumPy: ESS, log-sum-exp records, the decision, and the Kalman log-likelihood.
The model is a linear-Gaussian state space written as @gen + .scan on workloads.ssm_problem(dx=2, T=12), x_0 ~ N(0, q)."""
import ctypes
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

DX, T_FULL = 2, 12


def _np(t):
    return t.detach().cpu().numpy()


def _problem():
    from genjax_amd import workloads
    return workloads.ssm_problem(dx=DX, T=T_FULL)


def _lgssm_scan(s, T):
    Am = np.asarray(s["A"], np.float32)
    q, r = float(s["q"]), float(s["r"])

    @genjax.gen
    def step(x_prev, _):
        x = genjax.mv_normal_diag(Am @ x_prev, np.full(DX, q, np.float32)) @ "x"
        genjax.mv_normal_diag(x, np.full(DX, r, np.float32)) @ "y"
        return x, None

    return step.scan(n=T), np.zeros(DX, np.float32)


def _sv_with_parameter(T):
    """stochastic volatility with a LATENT persistence in front of the Scan: it is drawn by step 0 and travels with the particle"""
    @genjax.gen
    def step(carry, _):
        x_prev, phi = carry
        x = genjax.normal(phi * x_prev, 0.3) @ "x"
        genjax.normal(0.0, genjax.exp(0.5 * x)) @ "y"
        return (x, phi), None

    @genjax.gen
    def model():
        phi = genjax.uniform(0.8, 0.99) @ "phi"
        step.scan(n=T)((0.0, phi), None) @ "chain"

    return model


def _step_keys(key, T):
    """the filter's key discipline (inference/pf.py): k_t = fold_in(k_{t-1}, t); (k_prop, k_res) = split(k_t); u = uniform(k_res)"""
    from genjax_amd.core import fold_in, split
    from genjax_amd.inference.pf import _unit_from_key
    ks, us, k = [], [], key
    for t in range(T):
        k = fold_in(k, t)
        kp, kr = split(k)
        ks.append(kp)
        us.append(_unit_from_key(kr))
    return ks, us


def _lse64(w):
    w = np.asarray(w, np.float64)
    m = w.max()
    return float(m + np.log(np.exp(w - m).sum()))


def _ess64(w):
    w = np.asarray(w, np.float64)
    e = np.exp(w - w.max())
    return float(e.sum() ** 2 / (e * e).sum())


def _check_ancestors(dev_anc, logw_prev, u):
    """the filter's ancestors against the oracle's tile-scaled resampler and the standalone device resampler on the same (here:
    ACCUMULATED) log-weights, bit for bit; the oracle is handed the device's quantised weights (the one float operation of the
    scheme, an exp2, is held to libm elsewhere: tests/test_gpu_tiled.py), everything behind them is integer work"""
    import torch
    from genjax_amd import kernels
    from oracle import cpu
    lw = np.ascontiguousarray(logw_prev, np.float32)
    anc_s, q, e = kernels.resample_indices_tiled(torch.as_tensor(lw).cuda(), u, lw.size, want_q=True)
    anc_o, _, e_o, dead = cpu.resample_systematic_tiled(lw, u, lw.size, q=_np(q).view(np.uint32))
    assert not dead
    np.testing.assert_array_equal(_np(e), e_o)
    np.testing.assert_array_equal(dev_anc, anc_o)
    np.testing.assert_array_equal(dev_anc, _np(anc_s))


def _prefix_runs(tau, K, key):
    """runs T' = 1 .. T of the SAME filter (it is deterministic: a prefix run ends where the longer run passes): the state behind
    every step.  -> list of dicts"""
    from genjax_amd.inference import BootstrapFilter
    s = _problem()
    ys = np.asarray(s["y"], np.float32)
    outs = []
    for Tp in range(1, T_FULL + 1):
        scan, carry0 = _lgssm_scan(s, Tp)
        bf = BootstrapFilter(scan, K, ess_threshold=tau)
        o = bf.run(key, C["y"].set(ys[:Tp]), (carry0, None), keep_ancestors=True)
        assert o["info"]["form"] == A.FILTER_FORM_TWO_LAUNCH
        outs.append(dict(x=_np(bf.latent(o, "x")).copy(), logw=_np(o["logw"]).copy(), anc=_np(o["ancestors"]).copy(), prog=o["programs"][-1],
                         lse=_np(o["lse_steps"]).copy(), ess=_np(o["ess"]).copy(), resampled=_np(o["resampled"]).copy(), log_ml=float(o["log_ml"]),
                         incs=_np(o["increments"]).copy()))
    for a, b in zip(outs[:-1], outs[1:]):                     # a prefix run IS the head of the longer run
        n = len(a["ess"])
        np.testing.assert_array_equal(a["ess"], b["ess"][:n])
        np.testing.assert_array_equal(a["resampled"], b["resampled"][:n])
        np.testing.assert_array_equal(a["lse"], b["lse"][:n])
        np.testing.assert_array_equal(a["anc"][: n - 1], b["anc"][: n - 1])
    return outs


@pytest.mark.parametrize("K", [1500, 1 << 14])
def test_threshold_one_is_the_filter_that_resamples_in_front_of_every_step(K, monkeypatch):
    """tau = 1: ancestors of every step, choices and log-weights equal the untouched path bit for bit (K = 1500: a partial tile and a
    partial wave); the LSE records to rel 3e-6 (float summation order, the tolerance of the existing record assertion)"""
    from genjax_amd.inference import BootstrapFilter
    T = 6
    s = _problem()
    ys = np.asarray(s["y"], np.float32)[:T]
    scan, carry0 = _lgssm_scan(s, T)
    monkeypatch.setenv("GJX_SCAN_FILTER_TWO_LAUNCH", "1")
    bf0, bf1 = BootstrapFilter(scan, K), BootstrapFilter(scan, K, ess_threshold=1.0)
    ref = bf0.run(genjax.key(9), C["y"].set(ys), (carry0, None), keep_ancestors=True)
    assert ref["info"]["form"] == A.FILTER_FORM_TWO_LAUNCH and "ess" not in ref
    o = bf1.run(genjax.key(9), C["y"].set(ys), (carry0, None), keep_ancestors=True)
    assert o["info"]["form"] == A.FILTER_FORM_TWO_LAUNCH
    np.testing.assert_array_equal(_np(o["ancestors"]), _np(ref["ancestors"]))
    np.testing.assert_array_equal(_np(bf1.latent(o, "x")), _np(bf0.latent(ref, "x")))      # (the choices; the step's INPUT rows are never written)
    np.testing.assert_array_equal(_np(o["logw"]), _np(ref["logw"]))
    np.testing.assert_allclose(_np(o["lse_steps"]), _np(ref["lse_steps"]), rtol=3e-6)
    res = _np(o["resampled"])
    assert res.dtype == np.bool_ and res.shape == (T,) and not res[0] and res[1:].all()
    assert _np(o["ess"]).shape == (T,) and (_np(o["ess"]) > 1.0).all() and (_np(o["ess"]) <= K * (1 + 1e-5)).all()
    assert len(np.unique(_np(o["ancestors"])[2])) < K                               # (resampling did something)


def test_threshold_zero_is_importance_sampling_along_the_scan():
    """tau = 0: no resampling at all — identity ancestors, the particles == the oracle on the step program fed the UN-gathered carry,
    W_T == the sum of the oracle's step weights, and log-ML = lse(W_T) - log K == the sum of the increments"""
    from oracle import cpu
    K, T = 4096, T_FULL
    key = genjax.key(21)
    keys, _ = _step_keys(key, T)
    outs = _prefix_runs(0.0, K, key)
    last = outs[-1]
    assert last["anc"].shape == (T - 1, K) and (last["anc"] == np.arange(K, dtype=np.int32)[None, :]).all()
    assert last["resampled"].shape == (T,) and not last["resampled"].any()
    W = np.zeros(K, np.float64)
    for t in range(T):
        cur, prog = outs[t], outs[t]["prog"]
        ch_in = np.zeros((prog.n_slots, K), np.float32)
        if t > 0:
            ch_in[:DX] = outs[t - 1]["x"]                                           # the carry as it is: nothing was gathered
        ora = cpu.run_program(prog, keys[t], K, choices=ch_in)
        sl = prog.slot_of[("x", t)]
        np.testing.assert_allclose(cur["x"], ora["choices"][sl:sl + DX], rtol=2e-4, atol=5e-5)
        W += ora["weight"].astype(np.float64)
        np.testing.assert_allclose(cur["logw"], W, rtol=0, atol=2e-4 * (t + 1))
    want = _lse64(last["logw"]) - np.log(K)
    assert last["log_ml"] == pytest.approx(want, rel=3e-6)
    assert float(last["incs"].astype(np.float64).sum()) == pytest.approx(want, rel=3e-6)
    assert float(last["lse"][:, 3].astype(np.float64).sum()) == pytest.approx(want, rel=3e-6)


def test_threshold_half_takes_the_right_decision_and_both_branches():
    """tau = 0.5, step by step.  ESS: the device's figure against float64 on the device's own W_t within rel 1e-4 — the one inexact
    operation is e = v_exp_f32((W - max) log2 e): the float32 product carries a rounding of 2^-24 relative, i.e. up to
    29 * 2^-24 * ln 2 = 1.2e-6 relative in e for |W - max| <= 20 (v_exp_f32 itself is good to 1 ulp, 6e-8), terms under e^-20 cannot
    move a ratio of sums whose largest term is 1, and float32 summation of K = 4096 such terms adds a few 1e-7: 1e-4 is about two
    orders above all of it.  The decision must be the float64 one (steps within 2e-4 of the threshold excluded: at most one); a
    resampled step's ancestors are the standalone tile-scaled resampler's on W_t, a skipped step's the identity; the next weights
    are (0 or W_t) + the oracle's weight on the gathered carry; the record's increment is lse(W_t) - c_t."""
    from oracle import cpu
    K, T, tau = 4096, T_FULL, 0.5
    key = genjax.key(21)
    keys, us = _step_keys(key, T)
    outs = _prefix_runs(tau, K, key)
    last = outs[-1]
    excluded = 0
    assert not last["resampled"][0]
    for t in range(T):
        cur, prog = outs[t], outs[t]["prog"]
        W_t = cur["logw"]
        ess64 = _ess64(W_t)
        print(f"step {t}: ESS device {last['ess'][t]:.3f} float64 {ess64:.3f} ({ess64 / K:.4f} K), resampled in front: {bool(last['resampled'][t])}")
        assert float(last["ess"][t]) == pytest.approx(ess64, rel=1e-4)
        # this step's particles and weights from the state behind step t - 1
        ch_in = np.zeros((prog.n_slots, K), np.float32)
        carried = np.zeros(K, np.float64)
        if t > 0:
            prev = outs[t - 1]
            anc = last["anc"][t - 1]
            if last["resampled"][t]:
                _check_ancestors(anc, prev["logw"], us[t])
            else:
                np.testing.assert_array_equal(anc, np.arange(K, dtype=np.int32))
                carried = prev["logw"].astype(np.float64)
            ch_in[:DX] = prev["x"][:, anc]
        ora = cpu.run_program(prog, keys[t], K, choices=ch_in)
        sl = prog.slot_of[("x", t)]
        np.testing.assert_allclose(cur["x"], ora["choices"][sl:sl + DX], rtol=2e-4, atol=5e-5)
        np.testing.assert_allclose(W_t, carried + ora["weight"], rtol=2e-4, atol=2e-4)
        # the record: lse(W_t) - c_t, c_t = log K at step 0 and behind a resampling, lse(W_{t-1}) behind a skip
        c_t = np.log(K) if (t == 0 or last["resampled"][t]) else _lse64(outs[t - 1]["logw"])
        assert float(last["lse"][t, 2]) == pytest.approx(_lse64(W_t), rel=3e-6)
        assert float(last["lse"][t, 3]) == pytest.approx(_lse64(W_t) - c_t, rel=3e-6)
        # the decision for the next step
        if t + 1 < T:
            if abs(ess64 / K - tau) < 2e-4:
                excluded += 1
            else:
                assert bool(last["resampled"][t + 1]) == (ess64 < tau * K), (t, ess64)
    assert excluded <= 1
    n_res = int(last["resampled"][1:].sum())
    assert n_res >= 2 and (T - 1 - n_res) >= 2, last["resampled"]
    assert last["log_ml"] == pytest.approx(float(last["lse"][:, 3].astype(np.float64).sum()), rel=3e-6)


def test_adaptive_filter_is_unbiased_against_the_kalman_log_likelihood(monkeypatch):
    """16 seeds at tau = 0.5 against 16 seeds of the untouched filter: the adaptive mean within 4 standard errors (measured on the
    untouched path) of the float64 Kalman value"""
    from genjax_amd.inference import BootstrapFilter
    from oracle import closed_form as cf
    K, T, n = 4096, T_FULL, 16
    s = _problem()
    ys = np.asarray(s["y"], np.float32)
    scan, carry0 = _lgssm_scan(s, T)
    exact, _, _ = cf.kalman_log_lik(s["A"], s["y"], s["q"], s["r"], q0=float(s["q"]))
    ad = BootstrapFilter(scan, K, ess_threshold=0.5)
    est = np.array([float(ad.run(genjax.key(300 + i), C["y"].set(ys), (carry0, None))["log_ml"]) for i in range(n)])
    monkeypatch.setenv("GJX_SCAN_FILTER_TWO_LAUNCH", "1")
    plain = BootstrapFilter(scan, K)
    ref = np.array([float(plain.run(genjax.key(300 + i), C["y"].set(ys), (carry0, None))["log_ml"]) for i in range(n)])
    std_none = ref.std(ddof=1)
    print(f"log-ML over {n} seeds: adaptive {est.mean():.4f} +- {est.std(ddof=1):.4f}, every step {ref.mean():.4f} +- {std_none:.4f}, Kalman {exact:.4f}")
    assert abs(est.mean() - exact) <= 4.0 * std_none / np.sqrt(n)


def test_history_of_an_adaptive_run_follows_identity_rows_too():
    """keep_history at tau = 0.5: ScanHistory.paths("x") reproduces each step's stored particles when followed through the
    ancestors — a skipped step's row is the identity — and the recorded run is the ordinary run"""
    import torch
    from genjax_amd.inference import BootstrapFilter
    K, T = 4096, T_FULL
    s = _problem()
    ys = np.asarray(s["y"], np.float32)
    scan, carry0 = _lgssm_scan(s, T)
    bf = BootstrapFilter(scan, K, ess_threshold=0.5)
    plain = bf.run(genjax.key(21), C["y"].set(ys), (carry0, None), keep_ancestors=True)
    out = bf.run(genjax.key(21), C["y"].set(ys), (carry0, None), keep_history=True)
    h = out["history"]
    assert len(h) == T and h.ancestors.shape == (T - 1, K)
    assert torch.equal(out["ancestors"], plain["ancestors"]) and torch.equal(out["logw"], plain["logw"])
    assert torch.equal(out["resampled"], plain["resampled"]) and torch.equal(out["ess"], plain["ess"])
    assert torch.equal(h.step(T - 1, "x"), bf.latent(plain, "x"))
    res = _np(out["resampled"])
    ident = torch.arange(K, device="cuda", dtype=torch.int32)
    for t in range(1, T):
        assert torch.equal(h.ancestors[t - 1], ident) == (not res[t])
    assert 0 < res[1:].sum() < T - 1
    paths = h.paths("x")
    assert paths.shape == (T, DX, K)
    cur = torch.arange(K, device="cuda")
    for t in range(T - 1, -1, -1):
        assert torch.equal(paths[t], h.step(t, "x")[:, cur])
        if t > 0:
            cur = h.ancestors[t - 1][cur].long()
    m = h.smoothed_means("x")
    assert m.shape == (T, DX) and bool(torch.isfinite(m).all())


def test_carried_statics_run_under_both_extremes(monkeypatch):
    """a model with one latent in front of the Scan (GJX_FILTER_ABSOLUTE_INPUTS): tau = 1 equals the untouched two-launch path bit for
    bit; tau = 0 gives identity ancestors, a parameter row that never moves, and a finite log-ML"""
    from genjax_amd.inference import BootstrapFilter
    K, T = 4096, 5
    ys = (np.random.default_rng(3).standard_normal(T) * 1.2).astype(np.float32)
    key = genjax.key(31)
    run = lambda bf: bf.run(key, C["chain", "y"].set(ys), (), keep_ancestors=True)
    monkeypatch.setenv("GJX_SCAN_FILTER_TWO_LAUNCH", "1")
    bf0 = BootstrapFilter(_sv_with_parameter(T), K)
    ref = run(bf0)
    assert ref["info"]["form"] == A.FILTER_FORM_TWO_LAUNCH
    bf1 = BootstrapFilter(_sv_with_parameter(T), K, ess_threshold=1.0)
    o = run(bf1)
    np.testing.assert_array_equal(_np(o["ancestors"]), _np(ref["ancestors"]))
    np.testing.assert_array_equal(_np(o["logw"]), _np(ref["logw"]))
    for name in ("phi", ("chain", "x")):
        np.testing.assert_array_equal(_np(bf1.latent(o, name)), _np(bf0.latent(ref, name)))
    np.testing.assert_allclose(_np(o["lse_steps"]), _np(ref["lse_steps"]), rtol=3e-6)
    bfz = BootstrapFilter(_sv_with_parameter(T), K, ess_threshold=0.0)
    z = run(bfz)
    assert (_np(z["ancestors"]) == np.arange(K, dtype=np.int32)[None, :]).all() and not _np(z["resampled"]).any()
    assert np.isfinite(float(z["log_ml"]))
    bfz1 = BootstrapFilter(_sv_with_parameter(1), K, ess_threshold=0.0)
    z1 = bfz1.run(key, C["chain", "y"].set(ys[:1]), ())
    np.testing.assert_array_equal(_np(bfz.latent(z, "phi")), _np(bfz1.latent(z1, "phi")))       # the parameter a particle drew at step 0
    assert float(z["log_ml"]) == pytest.approx(_lse64(_np(z["logw"])) - np.log(K), rel=3e-6)


@pytest.mark.parametrize("K", [1, 63, 1500, 1 << 14])
def test_effective_sample_size_of_log_weights(K):
    """gjx_ess / kernels.ess / ParticleCollection.effective_sample_size(): against float64 within rel 1e-4 (the derivation in the
    tau = 0.5 test; the weights here span 12 nats); equal weights give exactly K, one live particle exactly 1, none 0"""
    import torch
    from genjax_amd import kernels
    from genjax_amd.inference import ParticleCollection
    rs = np.random.default_rng(K)
    lw = (rs.standard_normal(K) * 2.0 - 37.0).astype(np.float32)
    out = _np(kernels.ess(torch.as_tensor(lw).cuda()))
    e = np.exp(lw.astype(np.float64) - lw.max())
    assert out[0] == lw.max()
    assert out[1] == pytest.approx(e.sum(), rel=1e-4) and out[2] == pytest.approx((e * e).sum(), rel=1e-4)
    assert out[3] == pytest.approx(_ess64(lw), rel=1e-4)
    pc = ParticleCollection(None, torch.as_tensor(lw).cuda())
    v = pc.effective_sample_size()
    assert v.dim() == 0 and v.is_cuda and float(v) == out[3]
    assert float(kernels.ess(torch.full((K,), -3.25, dtype=torch.float32, device="cuda"))[3]) == float(K)
    one = torch.full((K,), -float("inf"), dtype=torch.float32, device="cuda")
    assert _np(kernels.ess(one)).tolist() == [-np.inf, 0.0, 0.0, 0.0]
    one[K // 2] = 5.5
    assert _np(kernels.ess(one)).tolist() == [5.5, 1.0, 1.0, 1.0]
    if K > 1:
        one[0] = float("nan")                                                       # a NaN weight is a dead particle
        assert float(kernels.ess(one)[3]) == 1.0


def test_the_c_calls_refuse_what_they_do_not_run():
    """GJX_EUNSUPPORTED: the rejuvenation move, the HMC move, multinomial resampling; GJX_EINVAL: a threshold outside [0, 1] or NaN,
    NULL fields, NULL options — all decided before anything is launched"""
    import torch
    from genjax_amd import _lib
    from genjax_amd.inference.scan_filter import ScanBootstrapFilter, _bind_device
    lib = _lib.load()
    K, T = 1024, 3
    s = _problem()
    scan, carry0 = _lgssm_scan(s, T)
    progs = ScanBootstrapFilter(scan, K).step_programs(C["y"].set(np.asarray(s["y"], np.float32)[:T]), (carry0, None))
    dev = torch.device("cuda", torch.cuda.current_device())
    tabs = _bind_device(progs, dev)
    cps = (A.GjxProgram * T)()
    for t, p in enumerate(progs):
        cps[t] = p.c_program(tabs[0].device)
    f32 = torch.float32
    n_rows = max(p.n_slots for p in progs)
    rows = torch.zeros((2, n_rows, K), dtype=f32, device=dev)
    rows_all = torch.zeros((T, n_rows, K), dtype=f32, device=dev)
    logw, acc, ess = (torch.zeros(K, dtype=f32, device=dev) for _ in range(3))
    anc, res = torch.zeros((T, K), dtype=torch.int32, device=dev), torch.zeros(T, dtype=torch.int32, device=dev)
    lse = torch.zeros((T, 4), dtype=f32, device=dev)
    ws = torch.zeros(lib.gjx_workspace_bytes(A.OP_RUN, K) + lib.gjx_workspace_bytes(A.OP_RESAMPLE, K), dtype=torch.uint8, device=dev)
    p_ = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(opts, adapt, history=False):
        a = ctypes.byref(adapt) if adapt is not None else None
        o = ctypes.byref(opts) if opts is not None else None
        if history:
            return lib.gjx_scan_filter_adaptive_history(ctypes.cast(cps, ctypes.c_void_p), T, 0, 1, K, p_(rows_all), n_rows, p_(logw), p_(anc), p_(lse), p_(ws),
                                                        ws.numel(), None, o, None, a)
        return lib.gjx_scan_filter_adaptive(ctypes.cast(cps, ctypes.c_void_p), T, 0, 1, K, p_(rows[0]), p_(rows[1]), p_(logw), p_(anc), None, p_(lse), p_(ws),
                                            ws.numel(), None, o, None, a)

    good = lambda tau=0.5: A.GjxAdaptiveOpts(tau, 0, acc.data_ptr(), ess.data_ptr(), res.data_ptr())
    for history in (False, True):
        for field, value in (("n_moves", 2), ("flags", A.FILTER_MULTINOMIAL), ("hmc_targets", ctypes.cast(cps, ctypes.c_void_p))):
            o = A.GjxFilterOpts()
            setattr(o, field, value)
            assert call(o, good(), history) == A.EUNSUPPORTED, field
            assert b"adaptive" in lib.gjx_last_error()
        for tau in (-0.01, 1.01, float("nan"), float("inf")):
            assert call(None, good(tau), history) == A.EINVAL, tau
        for field in ("logw_acc", "ess_steps", "resampled"):
            a = good()
            setattr(a, field, None)
            assert call(None, a, history) == A.EINVAL, field
        assert call(None, None, history) == A.EINVAL
        assert call(A.GjxFilterOpts(), good(), history) == A.OK                      # (and the good call runs)
    torch.cuda.synchronize()
    assert lib.gjx_ess(None, K, p_(lse), p_(ws), ws.numel(), None) == A.EINVAL
    assert lib.gjx_ess(p_(logw), 0, p_(lse), p_(ws), ws.numel(), None) == A.EINVAL
    assert lib.gjx_ess(p_(logw), K, p_(lse), p_(ws), 64, None) == A.EWORKSPACE
