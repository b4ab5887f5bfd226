"""The in-tile search of the resample+gather kernels with several slots per lane (rank_in_tiles_sorted, csrc/gjx_tile.h: slot 0 of a
lane is searched 4-ary and anchors a window of kRankWalk entries in which the slots behind it are counted off; a slot past the window
or in another tile is searched 4-ary and anchors the next window) and k_resample_gather's window boundaries from two sums (the full
prefix of the tile totals only on the fallback branch): ancestors == the oracle's weight_cumsum + resample_systematic, children ==
rows[:, ancestors], for equality.

The oracle's fixed point is exact for PLAIN weights (q = trunc(w 2^30); its log form goes through libm's expf, the device's through
v_exp_f32), so the weight patterns are handed to both sides as float32 weights, dead particles as 0.  The tile-scaled plain-launch form
takes the same patterns as log-weights (dead: -inf) and is compared with resample_indices_tiled, as test_gpu_tiled.py does.

Every case runs with the slots per lane the launcher picks at that size (one: no walk) and with four slots per lane (the form the bench's
K = 2^20 runs; GJX_RESAMPLE_ITEMS, an existing knob of the launcher)."""
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from genjax_amd import _abi as A       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the walk's window (entries read from the anchor slot's rank, from an even index: the reads are 16 bytes wide)
W = int(re.search(r"constexpr int kRankWalk = (\d+);", open(os.path.join(ROOT, "genjax_amd", "csrc", "gjx_tile.h")).read()).group(1))
TILE = 1024
SIZES = [4, 1000, 1024, 2052, 3 * 1024, 9 * 1024]
US = [0.0, 0.5, 1.0 - 2.0 ** -24]


@pytest.fixture(scope="module")
def K_():
    from genjax_amd import kernels
    return kernels


def _np(t):
    return t.detach().cpu().numpy()


def _runs(K, rs, heavy):
    """live particles separated by runs of exactly W - 3 .. W + 2 dead ones (the window starts at an even index, so a slot W - 2 or
    W - 1 entries above the anchor is the last one inside it, depending on the parity of the anchor's rank; the longer runs end past
    it), a run of exactly W dead ones at the start and at the end of every tile; heavy: one particle takes three quarters of the
    slots, so the others own one or two slots each and most lanes cross a run, some of them two"""
    w = np.zeros(K, np.float64)
    p, j = 0, 0
    lens = [W - 1, W, W + 1, W - 3, W - 2, W + 2]
    while p < K:
        w[p] = 0.5 + rs.random()
        p += 1 + max(0, lens[j % len(lens)])
        j += 1
    for t0 in range(0, K, TILE):
        t1 = min(t0 + TILE, K)
        if t1 - t0 > 2 * W + 2:
            w[t0:t0 + W] = 0.0
            w[t0 + W] = 1.0
            w[t1 - W:t1] = 0.0
            w[t1 - W - 1] = 1.0
    if heavy:
        w[K - 1] = 3.0 * w[:K - 1].sum()
    return w


def _pattern(name, K):
    rs = np.random.default_rng(K * 31 + len(name))
    if name == "lognormal":
        return np.exp(rs.standard_normal(K))
    if name == "runs":
        return _runs(K, rs, False)
    if name == "runs_heavy":
        return _runs(K, rs, True)
    if name.startswith("giant"):                              # one particle owns more than 1024 slots (most of them where K is smaller)
        w = np.exp(rs.standard_normal(K))
        at = {"giant_first_in_tile": (K // 2) // TILE * TILE, "giant_last_in_tile": min(K - 1, ((K // 2) // TILE + 1) * TILE - 1),
              "giant_last": K - 1}[name]
        w[at] = 0.0
        w[at] = 1.5 * w.sum()                                 # 60 % of the slots: 1231 of 2052
        return w
    if name == "dead_tile":                                   # a whole dead tile in the middle: the slots of one lane straddle two source tiles
        w = np.exp(rs.standard_normal(K))
        if K >= 3 * TILE:
            w[TILE:2 * TILE] = 0.0
        else:
            w[K // 3:2 * K // 3] = 0.0
        return w
    if name == "equal":
        return np.full(K, 0.25)
    if name == "dead":
        return np.zeros(K)
    assert name == "collapsed_tile0"                          # every block but the first searches outside its window: the full prefix
    w = np.zeros(K)
    w[min(5, K - 1)] = 1.0
    return w


PATTERNS = ["lognormal", "runs", "runs_heavy", "giant_first_in_tile", "giant_last_in_tile", "giant_last", "dead_tile", "equal", "dead",
            "collapsed_tile0"]


@pytest.mark.parametrize("K", SIZES)
@pytest.mark.parametrize("name", PATTERNS)
def test_resample_gather_against_oracle(K_, oracle, monkeypatch, K, name):
    import torch
    w = _pattern(name, K)
    w = (w / max(w.max(), 1e-300)).astype(np.float32)
    rows = np.random.default_rng(K).standard_normal((3, K)).astype(np.float32)
    wd, rd = torch.as_tensor(w).cuda(), torch.as_tensor(rows).cuda()
    ws = K_.workspace(A.OP_RESAMPLE, K)
    cum_o, tot = oracle.weight_cumsum(w)
    if name == "giant_first_in_tile" and K > 2 * TILE:
        assert np.bincount(oracle.resample_systematic(cum_o, 0.5, K), minlength=K).max() > TILE
    for items in (None, "4"):
        if items:
            monkeypatch.setenv("GJX_RESAMPLE_ITEMS", items)
        for u in US:
            anc = torch.full((K,), -7, dtype=torch.int32, device="cuda")
            ch = K_.resample_gather(wd, u, rd, is_log=False, anc=anc, ws=ws, allow_fallback=False)
            if name == "dead":
                assert tot == 0
                np.testing.assert_array_equal(_np(anc), np.arange(K))
                assert torch.equal(ch, rd) and K_.workspace_status(ws, raise_on_error=False) == 2
                continue
            want = oracle.resample_systematic(cum_o, u, K)
            np.testing.assert_array_equal(_np(anc), want, err_msg=f"{name} K={K} u={u} items={items}")
            np.testing.assert_array_equal(_np(ch), rows[:, want])
        assert K_.workspace_status(ws, raise_on_error=False) == 0


@pytest.mark.parametrize("K", SIZES)
@pytest.mark.parametrize("name", PATTERNS)
def test_plain_launch_tiled_form_against_three_launch_resampler(K_, K, name):
    """the same patterns through gjx_resample_gather_tiled (tiled_search_tile: window path and re-scan rounds walk too) against
    gjx_resample_indices_tiled, itself oracle-exact (test_gpu_tiled.py)"""
    import torch
    w = _pattern(name, K)
    with np.errstate(divide="ignore"):
        lw = np.log(w / max(w.max(), 1e-300)).astype(np.float32)
    rows = np.random.default_rng(K + 1).standard_normal((3, K)).astype(np.float32)
    lwd, rd = torch.as_tensor(lw).cuda(), torch.as_tensor(rows).cuda()
    ws = K_.workspace(A.OP_RESAMPLE, K)
    for u in US:
        anc = torch.full((K,), -7, dtype=torch.int32, device="cuda")
        ch = K_.resample_gather_tiled(lwd, u, rd, anc=anc, ws=ws)
        if name == "dead":
            np.testing.assert_array_equal(_np(anc), np.arange(K))
            assert torch.equal(ch, rd) and K_.workspace_status(ws, raise_on_error=False) == 2
            continue
        want = _np(K_.resample_indices_tiled(lwd, u, K))
        np.testing.assert_array_equal(_np(anc), want, err_msg=f"{name} K={K} u={u}")
        np.testing.assert_array_equal(_np(ch), rows[:, want])
    assert K_.workspace_status(ws, raise_on_error=False) == 0
