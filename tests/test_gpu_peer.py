"""Sharded collections over peer-mapped windows (csrc/gjx_peer.hip, gjx_pfilter.inl): G processes share the one GPU of
the test box, map each other's windows through hipIpc and run the sharded kernels concurrently — the same code path as G
GPUs over xGMI, with the device's own memory in place of the fabric.  Results must equal the unsharded kernels bit for
bit (streams are indexed by the global particle index; every integer of the resampling comes from the same granules)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return int(sk.getsockname()[1])


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(dx, T):
    import sys
    sys.path.insert(0, ROOT)
    from genjax_amd import workloads
    return workloads.ssm_problem(dx=dx, T=T)


def _filter_worker(rank, world, port, K_total, T, dx, rng, q, move=None, device_per_rank=False):
    try:
        import sys
        import torch
        import torch.distributed as dist
        sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          HSA_ENABLE_IPC_MODE_LEGACY="0")
        from genjax_amd import distributed as D
        from genjax_amd import kernels
        from genjax_amd.inference.pf import LinearGaussianSSM
        D.init_from_env("gloo")
        torch.cuda.set_device(rank if device_per_rank else 0)       # device_per_rank: one GPU per rank, windows mapped over xGMI
        s = _problem(dx, T)
        ssm = LinearGaussianSSM(s["A"], s["q"], s["r"])
        ys = torch.as_tensor(np.asarray(s["y"], np.float32)).cuda()
        ctx = kernels.PeerContext(K_total // world, dx, "cuda")
        outs = []
        for rep in range(3):                      # consecutive runs alternate the flag regions of the context
            o = ctx.ssm_filter(ssm.c_struct("cuda"), (0, 5 + rep), rng, ys, want_ancestors=True, move=move)
            torch.cuda.synchronize()
            outs.append((o["x"].cpu().numpy().copy(), o["logw"].cpu().numpy().copy(), o["lse_steps"].cpu().numpy().copy(),
                         o["ancestors"].cpu().numpy().copy(), int(o["accepted_total"][0]) if move else 0))
        st = ctx.status()
        q.put((rank, outs, st, ctx.ranks_on_device))
        ctx.close()
        if dist.is_initialized():
            dist.destroy_process_group()
    except BaseException:
        import traceback
        q.put((rank, "error", traceback.format_exc(), None))
        raise


@pytest.mark.parametrize("world,K_total,dx", [(1, 1 << 15, 8), (2, 1 << 15, 8), (4, 1 << 15, 4), (2, 1 << 17, 8),
                                              (4, 1 << 21, 8)])     # the last: config 4's shard (2^19 particles per rank, d_x = 8)
def test_peer_filter_equals_unsharded(world, K_total, dx):
    """gjx_ssm_filter_peer on `world` ranks (processes sharing the GPU) == gjx_ssm_filter_scheme(tile-scaled) on one rank:
    particles, log-weights and ancestors bit for bit, the LSE records to summation order."""
    import torch
    import torch.multiprocessing as mp
    from genjax_amd import _abi as A
    from genjax_amd import kernels
    from genjax_amd.inference.pf import LinearGaussianSSM
    T = 12
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_filter_worker, args=(r, world, port, K_total, T, dx, A.RNG_FLAT, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for r in res:
        assert r[1] != "error", r[2]
    res.sort(key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    s = _problem(dx, T)
    ssm = LinearGaussianSSM(s["A"], s["q"], s["r"])
    ys = torch.as_tensor(np.asarray(s["y"], np.float32)).cuda()
    for rep in range(3):
        ref = kernels.ssm_filter(ssm.c_struct("cuda"), (0, 5 + rep), A.RNG_FLAT, ys, K_total, weights=A.WEIGHTS_TILE_SCALED)
        torch.cuda.synchronize()
        x = np.concatenate([r[1][rep][0] for r in res], axis=1)
        lw = np.concatenate([r[1][rep][1] for r in res])
        anc = np.concatenate([r[1][rep][3] for r in res])
        np.testing.assert_array_equal(x, ref["x"].cpu().numpy())
        np.testing.assert_array_equal(lw, ref["logw"].cpu().numpy())
        np.testing.assert_array_equal(anc, ref["ancestors"].cpu().numpy())
        for r in res:                             # every rank holds the global records
            np.testing.assert_allclose(r[1][rep][2][:, 2:], ref["lse_steps"].cpu().numpy()[:, 2:], rtol=2e-6, atol=2e-6)
    assert all(r[2] == 0 for r in res), [r[2] for r in res]       # no rendezvous timed out, no dead step
    assert all(r[3] == world for r in res)                         # the ranks noticed that they share one device


@pytest.mark.parametrize("world,K_total,dx", [(1, 1 << 15, 8), (2, 1 << 15, 8), (4, 1 << 16, 4)])
def test_peer_move_filter_equals_unsharded(world, K_total, dx):
    """the sharded filter WITH resample-move rejuvenation (gjx_ssm_filter_peer_move: the parent means of the Metropolis
    target are pulled through the peer windows like the states) == gjx_ssm_filter_move on one rank: particles, weights
    and the number of accepted moves, bit for bit."""
    import torch
    import torch.multiprocessing as mp
    from genjax_amd import _abi as A
    from genjax_amd import kernels
    from genjax_amd.inference.pf import LinearGaussianSSM
    T, move = 12, (2, 0.4)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_filter_worker, args=(r, world, port, K_total, T, dx, A.RNG_FLAT, q, move)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for r in res:
        assert r[1] != "error", r[2]
    res.sort(key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    s = _problem(dx, T)
    ssm = LinearGaussianSSM(s["A"], s["q"], s["r"])
    ys = torch.as_tensor(np.asarray(s["y"], np.float32)).cuda()
    for rep in range(3):
        ref = kernels.ssm_filter_move(ssm.c_struct("cuda"), (0, 5 + rep), A.RNG_FLAT, ys, K_total, move[0], move[1])
        torch.cuda.synchronize()
        assert ref is not None
        np.testing.assert_array_equal(np.concatenate([r[1][rep][0] for r in res], axis=1), ref["x"].cpu().numpy())
        np.testing.assert_array_equal(np.concatenate([r[1][rep][1] for r in res]), ref["logw"].cpu().numpy())
        assert sum(r[1][rep][4] for r in res) == int(ref["accepted_total"][0]) > 0
        for r in res:
            np.testing.assert_allclose(r[1][rep][2][:, 2:], ref["lse_steps"].cpu().numpy()[:, 2:], rtol=2e-6, atol=2e-6)
    assert all(r[2] == 0 for r in res), [r[2] for r in res]


def _scan_filter_worker(rank, world, port, K_total, T, dx, q, env):
    try:
        import sys
        import torch
        import torch.distributed as dist
        sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          HSA_ENABLE_IPC_MODE_LEGACY="0", **env)
        import genjax_amd as genjax
        from genjax_amd import C, distributed as D, kernels, workloads
        from genjax_amd.inference import BootstrapFilter
        D.init_from_env("gloo")
        torch.cuda.set_device(0)
        scan, carry0, s = workloads.lgssm_scan(dx, T)
        ys = np.asarray(s["y"], np.float32)
        bf = BootstrapFilter(scan, K_total // world, resampler=env.get("GJX_TEST_RESAMPLER", "systematic"))
        rows = max(p.n_slots for p in bf.step_programs(C["y"].set(ys), (carry0, None)))
        ctx = kernels.PeerContext(K_total // world, rows, "cuda")
        outs = []
        for rep in range(2):                      # consecutive runs alternate the flag regions of the context
            o = bf.run_peer(ctx, genjax.key(5 + rep), C["y"].set(ys), (carry0, None), want_ancestors=True)
            torch.cuda.synchronize()
            outs.append((bf.latent(o, "x").cpu().numpy().copy(), o["logw"].cpu().numpy().copy(), o["lse_steps"].cpu().numpy().copy(),
                         o["ancestors"].cpu().numpy().copy(), o["info"]))
        st = ctx.status()
        q.put((rank, outs, st, ctx.ranks_on_device))
        ctx.close()
        if dist.is_initialized():
            dist.destroy_process_group()
    except BaseException:
        import traceback
        q.put((rank, "error", traceback.format_exc(), None))
        raise


def _run_scan_filter_ranks(world, K_total, T, dx, env):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_scan_filter_worker, args=(r, world, port, K_total, T, dx, q, env)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for r in res:
        assert r[1] != "error", r[2]
    res.sort(key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("world,K_total,dx,verify,resampler", [(1, 1 << 14, 8, 0, "systematic"), (2, 1 << 15, 8, 1, "systematic"), (4, 1 << 16, 4, 1, "systematic"),
                                                               (8, 1 << 19, 8, 1, "systematic"), (1, 1 << 14, 8, 0, "multinomial"),
                                                               (2, 1 << 15, 8, 1, "multinomial"), (4, 1 << 17, 4, 1, "multinomial"), (8, 1 << 19, 8, 0, "multinomial")])
def test_generic_filter_sharded_over_peer_windows_equals_unsharded(world, K_total, dx, verify, resampler):
    """gjx_scan_filter_peer — the filter kernel GENERATED for config 3's model written as @gen + .scan, on `world` ranks (processes
    sharing the GPU, windows mapped through hipIpc) — == gjx_scan_filter on one rank: states, log-weights and ancestors bit for bit, the
    global LSE records to summation order; with GJX_PEER_VERIFY=1 every pulled carry row is checked against its owner's word and every
    re-scanned tile against its granule, and no status bit may be raised.  resampler="multinomial" (gjx_scan_filter_peer_opts, SURVEY.md
    §8(e): sorted uniforms over the whole sharded collection): the spacing sums of every tile travel with its granule"""
    import genjax_amd as genjax
    from genjax_amd import C, workloads
    from genjax_amd import _abi as A
    from genjax_amd.inference import BootstrapFilter
    T = 10
    res = _run_scan_filter_ranks(world, K_total, T, dx, dict(GJX_PEER_VERIFY=str(verify), GJX_TEST_RESAMPLER=resampler))
    scan, carry0, s = workloads.lgssm_scan(dx, T)
    ys = np.asarray(s["y"], np.float32)
    bf = BootstrapFilter(scan, K_total, resampler=resampler)
    for rep in range(2):
        ref = bf.run(genjax.key(5 + rep), C["y"].set(ys), (carry0, None))
        x = np.concatenate([r[1][rep][0] for r in res], axis=1)
        lw = np.concatenate([r[1][rep][1] for r in res])
        anc = np.concatenate([r[1][rep][3] for r in res])
        np.testing.assert_array_equal(x, bf.latent(ref, "x").cpu().numpy())
        np.testing.assert_array_equal(lw, ref["logw"].cpu().numpy())
        np.testing.assert_array_equal(anc, ref["ancestors"].cpu().numpy())
        for r in res:                             # every rank holds the global records
            np.testing.assert_allclose(r[1][rep][2][:, 2:], ref["lse_steps"].cpu().numpy()[:, 2:], rtol=2e-6, atol=2e-6)
            assert r[1][rep][4]["form"] == A.FILTER_FORM_WIDE and r[1][rep][4]["launches"] == 2
    assert all(r[2] == 0 for r in res), [r[2] for r in res]       # no time-out, no dead step, no verify mismatch
    assert all(r[3] == world for r in res)


def test_generic_filter_verify_mode_detects_a_rank_that_publishes_wrong_check_words():
    """GJX_PEER_VERIFY_FAULT=<rank>: that rank's check words are wrong on purpose — every rank that pulls one of its carry rows must
    raise GJX_STATUS_VERIFY_MISMATCH (the detector of the generated filter kernel is itself tested)"""
    res = _run_scan_filter_ranks(2, 1 << 15, 8, 8, dict(GJX_PEER_VERIFY="1", GJX_PEER_VERIFY_FAULT="1"))
    assert any(r[2] & 4 for r in res), [r[2] for r in res]


def _weights(shape, K, seed=11):
    rs = np.random.default_rng(seed)
    lw = (rs.standard_normal(K) * (5.0 if shape == "wide" else 1.0)).astype(np.float32)
    if shape == "first":
        lw[K // 7:] -= 60.0                      # nearly all the mass on the first rank: every rank pulls from it
    if shape == "dead_tiles":
        lw[2048:9000] = -np.inf                  # whole tiles without weight, a rank boundary inside the stretch
        lw[K - 3000:] = -300.0                   # tiles that are shifted out entirely
    if shape == "spiky":
        lw[:] = -40.0
        lw[rs.integers(0, K, 40)] = rs.standard_normal(40).astype(np.float32) * 3.0   # a few particles with many children
    return lw


def _resample_worker(rank, world, port, K_total, R, shape, q):
    try:
        import sys
        import torch
        import torch.distributed as dist
        sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          HSA_ENABLE_IPC_MODE_LEGACY="0")
        from genjax_amd import distributed as D
        from genjax_amd import kernels
        D.init_from_env("gloo")
        torch.cuda.set_device(0)
        K = K_total // world
        ctx = kernels.PeerContext(K, R, "cuda")
        rows = np.random.default_rng(3).standard_normal((R, K_total)).astype(np.float32)
        outs = []
        for call in range(4):                    # consecutive calls alternate the buffers and the exchange words
            p = call & 1
            lw = _weights(shape, K_total, seed=11 + call)
            sl = slice(rank * K, (rank + 1) * K)
            ctx.logw[p].copy_(torch.as_tensor(lw[sl]))
            ctx.rows[p].copy_(torch.as_tensor(rows[:, sl] + call))
            # the producer's per-block {max, sumexp} pairs, as gjx_run_program leaves them at workspace + 256
            t = torch.as_tensor(lw[sl]).cuda().view(-1, 256)
            m = t.max(dim=1).values
            se = torch.where(torch.isfinite(m), torch.exp(t - torch.where(torch.isfinite(m), m, torch.zeros_like(m))[:, None]).sum(dim=1), torch.zeros_like(m))
            ws = torch.zeros(256 + 8 * m.numel(), dtype=torch.uint8, device="cuda")
            ws[256:].view(torch.float32).view(-1, 2).copy_(torch.stack([m, se], dim=1))
            anc = torch.empty(K, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            if dist.is_initialized():
                dist.barrier()      # the ranks launch together (each spent a different time making its inputs)
            out, rec = ctx.resample_gather(p, 0.37 + 0.1 * call, partials=(ws, m.numel()), anc=anc)
            torch.cuda.synchronize()
            outs.append((out.cpu().numpy(), anc.cpu().numpy(), rec.cpu().numpy()))
        q.put((rank, outs, ctx.status(), None))
        ctx.close()
        if dist.is_initialized():
            dist.destroy_process_group()
    except BaseException:
        import traceback
        q.put((rank, "error", traceback.format_exc(), None))
        raise


@pytest.mark.parametrize("world,shape", [(1, "mild"), (1, "first"), (1, "spiky"), (2, "mild"), (2, "wide"), (4, "first"), (4, "dead_tiles"), (2, "spiky")])
def test_peer_resample_gather_equals_unsharded(world, shape):
    """gjx_peer_resample_gather on `world` ranks == gjx_resample_indices_tiled + gjx_gather_rows on the whole collection:
    ancestors and children bit for bit (children crossing rank boundaries in both directions, dead and shifted-out tiles,
    many-offspring particles), global LSE record on every rank."""
    import torch
    import torch.multiprocessing as mp
    from genjax_amd import kernels
    K_total, R = 1 << 15, 5
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_resample_worker, args=(r, world, port, K_total, R, shape, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for r in res:
        assert r[1] != "error", r[2]
    res.sort(key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    rows = np.random.default_rng(3).standard_normal((R, K_total)).astype(np.float32)
    crossing = 0
    K = K_total // world
    for call in range(4):
        lw = _weights(shape, K_total, seed=11 + call)
        lw_d = torch.as_tensor(lw).cuda()
        anc = kernels.resample_indices_tiled(lw_d, 0.37 + 0.1 * call)
        want = kernels.gather_rows(torch.as_tensor(rows + call).cuda(), anc).cpu().numpy()
        got_anc = np.concatenate([r[1][call][1] for r in res])
        np.testing.assert_array_equal(got_anc, anc.cpu().numpy())
        np.testing.assert_array_equal(np.concatenate([r[1][call][0] for r in res], axis=1), want)
        lse = float(torch.logsumexp(lw_d.double(), dim=0))
        for r in res:
            np.testing.assert_allclose(r[1][call][2][2], lse, rtol=3e-6)
        crossing += int((got_anc // K != np.arange(K_total) // K).sum())
    assert all(r[2] in (0,) for r in res), [r[2] for r in res]
    if world > 1:
        assert crossing > 0                     # children did cross rank boundaries


_TRACE_SCRIPT = r'''
import sys
sys.path.insert(0, %(root)r)
import numpy as np, torch
from genjax_amd import core, workloads
from genjax_amd.inference.pf import BootstrapFilter, LinearGaussianSSM
T = int(sys.argv[1])
s = workloads.ssm_problem(T=T)
bf = BootstrapFilter(LinearGaussianSSM(s["A"], s["q"], s["r"]), 1 << 15, weights="tile_scaled")
ys = torch.as_tensor(np.asarray(s["y"], np.float32)).cuda()
for rep in range(3):
    out = bf._run_peer(core.key(3 + rep), ys, torch.device("cuda", 0), 1, True)     # the sharded path, one rank
print("LOGML", float(out["log_ml"]))
bf.close()
'''


def _hip_api_counts(tmp, T):
    import csv
    import glob
    import subprocess
    import sys
    d = os.path.join(tmp, "trace_T%d" % T)
    script = os.path.join(tmp, "run_T%d.py" % T)
    with open(script, "w") as f:
        f.write(_TRACE_SCRIPT % dict(root=ROOT))
    env = dict(os.environ, TMPDIR=tmp, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(["rocprofv3", "--hip-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, script, str(T)],
                       cwd=tmp, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "LOGML" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    files = glob.glob(os.path.join(d, "**", "*hip_api_stats.csv"), recursive=True)
    assert files, os.listdir(d)
    counts = {}
    for row in csv.DictReader(open(files[0])):
        counts[row["Name"]] = counts.get(row["Name"], 0) + int(row["Calls"])
    return counts


def test_sharded_filter_host_calls_do_not_depend_on_T(tmp_path):
    """Zero host involvement inside the T loop of the sharded filter, shown with a HIP-API trace (rocprofv3 --hip-trace):
    the number of kernel launches, synchronisations, copies and allocations of a process that runs the sharded filter
    three times is THE SAME for T = 8 and T = 128 steps."""
    import shutil
    if shutil.which("rocprofv3") is None:
        pytest.skip("rocprofv3 not on PATH")
    a = _hip_api_counts(str(tmp_path), 8)
    b = _hip_api_counts(str(tmp_path), 128)
    watched = [n for n in set(a) | set(b) if any(k in n for k in ("Synchronize", "Memcpy", "Memset", "Launch", "Malloc", "Free", "EventQuery", "StreamWait"))]
    assert any("Launch" in n for n in watched) and any("Synchronize" in n for n in watched), sorted(a)
    # (the step keys and comb offsets go up front as kernel ARGUMENTS, 120 eight-byte words per launch: two more launches per run
    # from 121 steps on — in front of the T loop, not inside it)
    runs, chunks = 3, lambda T: 2 * ((T + 119) // 120)
    b["hipLaunchKernel"] = b.get("hipLaunchKernel", 0) - runs * (chunks(128) - chunks(8))
    diff = {n: (a.get(n, 0), b.get(n, 0)) for n in watched if a.get(n, 0) != b.get(n, 0)}
    assert not diff, diff
    launches = sum(v for n, v in b.items() if "LaunchKernel" in n)
    assert launches < 200, launches               # 3 runs x 2 launches + torch's own fills / copies, not 3 x 128 x anything
