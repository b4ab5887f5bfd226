"""The head of gjx_resample_gather (everything in front of the row copy) at the smallest shapes at which each of its pieces can go
wrong.  Every call is made twice: with FOUR slots per lane (GJX_RESAMPLE_ITEMS = 4, an existing knob of the launcher:
k_resample_gather<4>, 1024-particle tiles, the form the bench's K = 2^20 runs) and with the slots per lane the launcher picks at
these sizes (one: k_resample_gather<1>, 256-particle tiles, 4 .. 40 blocks).

The sizes are chosen for the four-slot form: one block with both neighbour tiles missing (1024), one neighbour (2048), three tiles,
the nine-boundary window exactly filled and just exceeded (9 and 10 tiles), a part tile (4096 + 4: one lane of the fifth block has
particles, the others take load_tile's part-tile form).  In the one-slot form the same sizes are 4 .. 40 whole tiles and a part tile
of 4 particles.  The three input forms (linear weights, log-weights with a finished LSE record, log-weights with the producing
kernel's block partials); weights that put the fixed-point sums at their edges (all equal: 2^30 per particle; with four slots per
lane 2^32 per lane and 2^40 per tile, with one 2^30 and 2^38), that send a block's slots out of the window (one live particle, a
strong drift) and a dead collection; comb offsets at both ends; two calls back to back on one workspace (epoch and tag of the
rendezvous); and block partials in numbers that take every path of the maximum's reduction (block_ref_max_only: a lane's second to
fourth pair, a ragged count, the loop's second trip).

Everything is compared bit for bit: ancestors with the oracle's systematic resampler on the device's fixed-point prefix sums
(gjx_weight_cumsum, the same input form), rows with gather_rows, and the LSE record of the partials form with the one
gjx_weight_cumsum finishes from the same partials (block_ref_max itself).  For the mixture kernel's partials the record is also
compared with the one run_program(want_lse=True) returns: the maximum exactly, the sums to 2e-6 — run_program's own finish reduces
the pairs in another order than block_ref_max, so the two records never were equal to the bit (test_consumer_side_lse_finish holds
them to the same 2e-6)."""
import numpy as np
import pytest

import helpers as H
from genjax_amd import _abi as A

pytestmark = pytest.mark.gpu

SIZES = [1024, 2048, 3072, 9 * 1024, 10 * 1024, 4096 + 4]
US = [0.0, 0.5, 1.0 - 2.0 ** -23]
KINDS = ["normal", "equal", "one_first", "one_middle", "one_last", "drift", "dead"]
ITEMS = ["4", None]      # slots per lane: four (forced), the launcher's choice (one at these sizes)


@pytest.fixture(scope="module")
def K_():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from genjax_amd import kernels
    return kernels


def _np(t):
    return t.detach().cpu().numpy()


def _slots(monkeypatch, items):
    if items:
        monkeypatch.setenv("GJX_RESAMPLE_ITEMS", items)
    else:
        monkeypatch.delenv("GJX_RESAMPLE_ITEMS", raising=False)


def _log_weights(kind, K, rs):
    nt = (K + 1023) // 1024
    if kind == "normal":
        return rs.standard_normal(K).astype(np.float32)
    if kind == "equal":
        return np.zeros(K, np.float32)
    if kind.startswith("one_"):
        lw = np.full(K, -np.inf, np.float32)
        tile = {"one_first": 0, "one_middle": nt // 2, "one_last": nt - 1}[kind]
        lw[min(tile * 1024 + 517, K - 1)] = 0.25
        return lw
    if kind == "drift":
        # e^{-70} .. 1 along the collection: fixed-point weights are zero below 0.70 K, so the first blocks draw from tiles far ahead
        return (70.0 * (np.arange(K, dtype=np.float64) / K - 1.0)).astype(np.float32)
    assert kind == "dead"
    return np.full(K, -np.inf, np.float32)


def _pairs_buffer(m, se, spare=0):
    """{max, sumexp} pairs as a producing kernel leaves them (256 bytes of header in front); `spare` more pairs behind them that no
    reader may take up (their maximum is 1e30)"""
    import torch
    n = len(m)
    pairs = np.full((n + spare, 2), 1e30, np.float32)
    pairs[:n, 0] = m
    pairs[:n, 1] = se
    ws = torch.zeros(256 + 8 * (n + spare), dtype=torch.uint8, device="cuda")
    ws[256:].view(torch.float32).view(-1, 2).copy_(torch.as_tensor(pairs))
    return ws, n


def _pairs(lw):
    """{max, sumexp} of every 1024 log-weights"""
    K = lw.size
    nt = (K + 1023) // 1024
    pad = np.full(nt * 1024, -np.inf, np.float32)
    pad[:K] = lw
    t = pad.reshape(nt, 1024)
    m = t.max(axis=1)
    with np.errstate(invalid="ignore"):
        se = np.where(np.isfinite(m), np.exp(t - np.where(np.isfinite(m), m, 0.0)[:, None]).sum(axis=1), 0.0).astype(np.float32)
    return _pairs_buffer(m, se)


def _check(K_, oracle, monkeypatch, x, form, u, rows, ws, anc, dead, what):
    """one call of resample_gather per entry of ITEMS in input form `form` (a dict of keyword arguments) against the oracle; -> the LSE
    records"""
    import torch
    K = x.numel()
    if dead:
        want = np.arange(K, dtype=np.int32)
    else:
        cum, _ = K_.weight_cumsum(x, **form)
        want = oracle.resample_systematic(_np(cum).view(np.uint64), u, K)
    children = K_.gather_rows(rows, torch.as_tensor(want).cuda())
    recs = []
    for items in ITEMS:
        _slots(monkeypatch, items)
        lse_out = torch.full((4,), np.nan, device="cuda") if "partials" in form else None
        anc.fill_(-7)
        ch = K_.resample_gather(x, u, rows, anc=anc, ws=ws, lse_out=lse_out, allow_fallback=False, **form)
        if dead:
            assert K_.workspace_status(ws, raise_on_error=False) == 2, (what, items)            # kStatusZeroTotal, nothing else
        np.testing.assert_array_equal(_np(anc), want, err_msg=f"{what} items={items}")
        assert torch.equal(ch, children), (what, items)
        recs.append(lse_out)
    return recs


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", SIZES)
def test_head_against_oracle(K_, oracle, monkeypatch, K, kind):
    import torch
    rs = np.random.default_rng(K + len(kind))
    lw = _log_weights(kind, K, rs)
    dead = kind == "dead"
    lwd = torch.as_tensor(lw).cuda()
    with np.errstate(invalid="ignore"):
        wd = torch.as_tensor(np.zeros(K, np.float32) if dead else np.exp(lw - lw.max()).astype(np.float32)).cuda()
    lse = K_.logsumexp(lwd, K)
    pws, n = _pairs(lw)
    forms = [(wd, dict(is_log=False)), (lwd, dict(is_log=True, lse=lse)), (lwd, dict(partials=(pws, n)))]
    ws = K_.workspace(A.OP_RESAMPLE, K)
    anc = torch.empty(K, dtype=torch.int32, device="cuda")
    if kind == "drift" and K >= 3072:       # the construction does what it is for: block 0 draws from tiles >= 2
        cum, _ = K_.weight_cumsum(lwd, True, lse)
        assert oracle.resample_systematic(_np(cum).view(np.uint64), 0.0, K)[:1024].min() >= 2048
    ref = torch.full((4,), np.nan, device="cuda")
    K_.weight_cumsum(lwd, partials=(pws, n), lse_out=ref)
    for nrows in (1, 17):
        rows = torch.as_tensor(rs.standard_normal((nrows, K)).astype(np.float32)).cuda()
        for x, form in forms:
            for u in US:
                what = f"K={K} {kind} rows={nrows} u={u} {sorted(form)}"
                for rec in _check(K_, oracle, monkeypatch, x, form, u, rows, ws, anc, dead, what):
                    if rec is not None:
                        np.testing.assert_array_equal(_np(rec).view(np.uint32), _np(ref).view(np.uint32), err_msg=what)
    if not dead:
        assert K_.workspace_status(ws) == 0


@pytest.mark.parametrize("K", SIZES)
def test_head_on_mixture_partials(K_, oracle, monkeypatch, K):
    """the partials form fed by the mixture kernel at that K: ancestors, rows, and the LSE record against run_program's own (the
    maximum exactly, the sums to the 2e-6 the two reduction orders differ by: see the module's docstring)"""
    import torch
    prog, _ = H.gmm()
    full = K_.run_program(prog, (5, K), K)
    rws = K_.workspace(A.OP_RUN, K)
    part = K_.run_program(prog, (5, K), K, want_lse=False, ws=rws)
    n = K_.run_partials_count(prog, K)
    ws = K_.workspace(A.OP_RESAMPLE, K)
    anc = torch.empty(K, dtype=torch.int32, device="cuda")
    ref = torch.full((4,), np.nan, device="cuda")
    K_.weight_cumsum(part["logw"], partials=(rws, n), lse_out=ref)
    for rows in (part["choices"][:1].contiguous(), part["choices"]):
        for u in US:
            what = f"K={K} rows={rows.shape[0]} u={u}"
            for rec in _check(K_, oracle, monkeypatch, part["logw"], dict(partials=(rws, n)), u, rows, ws, anc, False, what):
                np.testing.assert_array_equal(_np(rec).view(np.uint32), _np(ref).view(np.uint32), err_msg=what)
                assert float(rec[0]) == float(full["lse"][0]), what
                np.testing.assert_allclose(_np(rec), _np(full["lse"]), rtol=2e-6, atol=2e-6, err_msg=what)
    assert K_.workspace_status(ws) == 0


@pytest.mark.parametrize("items", ITEMS)
@pytest.mark.parametrize("K", [1024, 3072, 10 * 1024, 4096 + 4])
def test_two_calls_on_one_workspace(K_, oracle, monkeypatch, K, items):
    """two calls back to back on one workspace, nothing between them, == two oracle runs: the second call's rendezvous must not
    take the first call's granules for its own (epoch, tag), in each input form"""
    import torch
    rs = np.random.default_rng(K)
    lw = [rs.standard_normal(K).astype(np.float32), (3.0 * rs.standard_normal(K)).astype(np.float32)]
    rows = torch.as_tensor(rs.standard_normal((17, K)).astype(np.float32)).cuda()
    ws = K_.workspace(A.OP_RESAMPLE, K)
    for form_of in (lambda x: (torch.exp(x - x.max()), dict(is_log=False)),
                    lambda x: (x, dict(is_log=True, lse=K_.logsumexp(x, K))),
                    lambda x: (x, dict(partials=_pairs(_np(x))))):
        _slots(monkeypatch, None)
        ins = [form_of(torch.as_tensor(l).cuda()) for l in lw]
        ancs = [torch.empty(K, dtype=torch.int32, device="cuda") for _ in ins]
        recs = [torch.full((4,), np.nan, device="cuda") if "partials" in f else None for _, f in ins]
        torch.cuda.synchronize()
        _slots(monkeypatch, items)
        outs = [K_.resample_gather(x, u, rows, anc=a, ws=ws, lse_out=r, allow_fallback=False, **f)
                for (x, f), a, r, u in zip(ins, ancs, recs, (0.5, 0.0))]
        for (x, f), a, r, u, ch in zip(ins, ancs, recs, (0.5, 0.0), outs):
            cum, _ = K_.weight_cumsum(x, **f)
            want = oracle.resample_systematic(_np(cum).view(np.uint64), u, K)
            np.testing.assert_array_equal(_np(a), want, err_msg=f"K={K} {sorted(f)} u={u}")
            assert torch.equal(ch, K_.gather_rows(rows, torch.as_tensor(want).cuda()))
            if r is not None:
                ref = torch.full((4,), np.nan, device="cuda")
                K_.weight_cumsum(x, lse_out=ref, **f)
                np.testing.assert_array_equal(_np(r).view(np.uint32), _np(ref).view(np.uint32))
    assert K_.workspace_status(ws) == 0


@pytest.mark.parametrize("n", [257, 1000, 1025, 4096])
def test_maximum_of_many_partials(K_, oracle, monkeypatch, n):
    """block_ref_max_only keeps four pairs of a lane in flight and loops over 1024 pairs a trip; the sizes above never give a lane a
    second pair.  Synthetic pairs (a producer with 256-particle blocks leaves up to 4096): the maximum sits in the LAST pair (n = 257:
    a lane's second pair; 1000: a fourth pair under the ragged tail guard; 1025: the loop's second trip; 4096: its last), in the
    middle one and in the first, and dominates the log-weights, so a reduction that misses it shows in the record and in the
    ancestors.  The pairs behind the n-th hold 1e30: a reader past the count shows too.  Record == gjx_weight_cumsum's from the same
    pairs (block_ref_max), bit for bit."""
    import torch
    K, top = 2048, 8.0
    rs = np.random.default_rng(n)
    lw = np.minimum(rs.standard_normal(K), 6.0).astype(np.float32)
    lwd = torch.as_tensor(lw).cuda()
    rows = torch.as_tensor(rs.standard_normal((3, K)).astype(np.float32)).cuda()
    ws = K_.workspace(A.OP_RESAMPLE, K)
    anc = torch.empty(K, dtype=torch.int32, device="cuda")
    for at in (n - 1, n // 2, 0):
        m = rs.uniform(-3.0, 3.0, n).astype(np.float32)
        m[at] = top
        se = rs.uniform(1.0, 1024.0, n).astype(np.float32)
        form = dict(partials=_pairs_buffer(m, se, spare=8))
        ref = torch.full((4,), np.nan, device="cuda")
        K_.weight_cumsum(lwd, lse_out=ref, **form)
        what = f"n={n} at={at}"
        for rec in _check(K_, oracle, monkeypatch, lwd, form, 0.5, rows, ws, anc, False, what):
            assert float(rec[0]) == top, what
            np.testing.assert_array_equal(_np(rec).view(np.uint32), _np(ref).view(np.uint32), err_msg=what)
    assert K_.workspace_status(ws) == 0
