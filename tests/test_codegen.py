"""Per-program generated kernels (csrc/gjx_codegen.hip): emission and hipRTC compilation need no GPU (hipRTC
cross-compiles for gfx950), so they are checked here; execution and parity are in the -m gpu tests, where every program
outside the mixture shape runs on its generated kernel by default."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _programs():
    from genjax_amd import _abi as A
    from genjax_amd import workloads
    from genjax_amd.program import PackedProgram, Param, SiteList
    out = {}
    out["gmm"] = workloads.gmm_program(D=16, C=8)[0]
    out["gmm_jax32"] = workloads.gmm_program(D=4, C=3, rng=A.RNG_JAX32)[0]
    out["logreg"] = workloads.logreg_program(N=64, P=4)[0]
    sl = SiteList()
    sl.add("p", A.BETA, [np.float32(2.0), np.float32(2.0)])
    sl.add("v", A.FLIP, [Param.value("p", 1)])
    out["beta_bernoulli"] = PackedProgram(sl, {"v": A.MODE_OBS_TAB}, {"v": np.float32(1.0)})
    return out


def test_emitter_covers_the_workloads_and_compiles(tmp_path, monkeypatch):
    from genjax_amd import kernels
    monkeypatch.setenv("GJX_JIT_CACHE", str(tmp_path))
    for name, prog in _programs().items():
        for ppt in (1, 2):
            src = kernels.program_source(prog, ppt)
            assert 'extern "C" __global__' in src and "gjx_gen(GenArgs a)" in src, name
            assert src.count("---- site") == prog.n_sites
            kernels.program_precompile(prog, ppt)                 # hipRTC, gfx950, no GPU needed
    assert len([f for f in os.listdir(tmp_path) if f.endswith(".hsaco")]) == 2 * len(_programs())
    # the structure, not the table values, keys the cache: new observations reuse the code object
    from genjax_amd import workloads
    p2 = workloads.gmm_program(D=16, C=8, seed=3)[0]
    kernels.program_precompile(p2, 2)
    assert len([f for f in os.listdir(tmp_path) if f.endswith(".hsaco")]) == 2 * len(_programs())


def test_constants_are_hoisted_into_the_prologue():
    """log-softmax / running CDF of constant logits and log / reciprocal of table scales are computed once per block"""
    from genjax_amd import kernels
    src = kernels.program_source(_programs()["gmm"], 2)
    body = src[src.index("for (int64_t tix"):]
    assert "running CDF" in src and "#define TSRC(i) TAB(i)" in src and "fast_log(TSRC(" in src and "fast_rcp(TSRC(" in src
    assert "fast_log(" not in body and "fast_rcp(" not in body        # nothing transcendental per particle but the samplers


def test_uncovered_programs_report_unsupported():
    from genjax_amd import _abi as A
    from genjax_amd import kernels
    from genjax_amd._lib import GjxError
    from genjax_amd.program import PackedProgram, SiteList
    sl = SiteList()
    sl.add("w", A.DIRICHLET, [np.ones(3, np.float32)], dim=3)
    prog = PackedProgram(sl, {}, {})
    with pytest.raises(GjxError, match="coverage"):
        kernels.program_source(prog, 1)


RUN_CODES = {1, 2, 4, 257, 513, 514, 1537, 1538, 2561, 2562}
FILTER_CODES = {t | f for t in (1, 2, 4, 8, 16) for f in (0, 256, 512, 256 | 512, 1024, 256 | 1024)}


def _dirichlet_program():
    from genjax_amd import _abi as A
    from genjax_amd.program import PackedProgram, SiteList
    sl = SiteList()
    sl.add("w", A.DIRICHLET, [np.ones(3, np.float32)], dim=3)
    return PackedProgram(sl, {}, {})


@pytest.mark.parametrize("export,valid,top,message", [("program_precompile", RUN_CODES, 8192, "ppt must be"),
                                                      ("program_filter_precompile", FILTER_CODES, 4096, "tiles_per_block must be")])
def test_variant_codes_are_validated_by_one_decoder(export, valid, top, message):
    """A valid code reaches the emitter (which refuses a Dirichlet site before anything is compiled: "coverage"), every other
    code is EINVAL.  The filter set holds sharded + multinomial (| 256 | 1024): the kernel gjx_scan_filter_peer launches."""
    from genjax_amd import kernels
    from genjax_amd._lib import GjxError
    prog, call = _dirichlet_program(), getattr(kernels, export)
    assert len(valid) == (10 if export == "program_precompile" else 30)
    for code in list(range(top)) + [-1, 1 << 20]:
        with pytest.raises(GjxError) as err:
            call(prog, code)
        assert ("coverage" if code in valid else message) in str(err.value), (code, str(err.value))
        assert (message in str(err.value)) == (code not in valid), (code, str(err.value))


def test_emitter_knobs_are_part_of_a_kernels_identity(tmp_path, monkeypatch):
    """An environment variable the emitters read, flipped inside one process, gives the other kernel: not the one compiled before.

    GJX_GEN_ROLL=1 with and without GJX_GEN_NO_ROLL: a short Scan as one loop over its steps, or unrolled.  The sources differ, and
    program_precompile under both settings leaves two code objects (with a key that misses the variable the second call is answered
    from the in-memory cache, and one file appears).

    GJX_GEN_NO_MFMA, on the program with a big affine site at code 257, cannot show this through the source: the variable is read by
    has_mfma_site only, which decides the code a launcher PICKS — at a given code the emitted text is the same with and without it
    (one file on disk, named by the hash of that text).  It is folded into the key all the same: two entries in memory."""
    import helpers as H
    from genjax_amd import kernels, workloads
    monkeypatch.setenv("GJX_JIT_CACHE", str(tmp_path))
    hsaco = lambda: [f for f in os.listdir(tmp_path) if f.endswith(".hsaco")]
    prog = H.scan_chain(7, carry=True, observe=False, sigma=0.3, r=0.7)[0]
    monkeypatch.setenv("GJX_GEN_ROLL", "1")
    monkeypatch.delenv("GJX_GEN_NO_ROLL", raising=False)
    rolled = kernels.program_source(prog, 1)
    assert "for (int t_ = 1; t_ < 7; ++t_)" in rolled
    kernels.program_precompile(prog, 1)
    monkeypatch.setenv("GJX_GEN_NO_ROLL", "1")
    unrolled = kernels.program_source(prog, 1)
    assert unrolled != rolled and "for (int t_ = 1;" not in unrolled
    kernels.program_precompile(prog, 1)
    assert len(hsaco()) == 2
    monkeypatch.delenv("GJX_GEN_ROLL")
    monkeypatch.delenv("GJX_GEN_NO_ROLL")

    prog = workloads.logreg_importance_program()[0]
    monkeypatch.delenv("GJX_GEN_NO_MFMA", raising=False)
    src = kernels.program_source(prog, 257)
    kernels.program_precompile(prog, 257)
    n0 = kernels.jit_stats()["structures"]
    monkeypatch.setenv("GJX_GEN_NO_MFMA", "1")
    assert kernels.program_source(prog, 257) == src
    kernels.program_precompile(prog, 257)
    assert kernels.jit_stats()["structures"] == n0 + 1 and len(hsaco()) == 3
