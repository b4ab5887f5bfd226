"""Adaptive resampling (ess_threshold) of the generic particle filter, host side: the C ABI's declarations (include/gjx.h <->
libgjx_hip.so <-> genjax_amd/_abi.py) and the constructor's refusals.  No compute call is made here."""
import ctypes
import os
import re

import numpy as np
import pytest

import genjax_amd as genjax
from genjax_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gjx_scan_filter_adaptive", "gjx_scan_filter_adaptive_history", "gjx_ess")


def _header():
    return open(os.path.join(ROOT, "include", "gjx.h")).read()


def test_header_declares_and_library_exports_the_adaptive_calls():
    hdr = _header()
    from genjax_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in A.PROTOTYPES and hasattr(lib, name), name
    assert "#define GJX_ABI_VERSION 11" in hdr and A.ABI_VERSION == 11 and lib.gjx_version() == 11
    # the adaptive calls take the arguments of the calls they extend, and the options behind them
    for plain, adaptive in (("gjx_scan_filter", "gjx_scan_filter_adaptive"), ("gjx_scan_filter_history", "gjx_scan_filter_adaptive_history")):
        assert A.PROTOTYPES[adaptive][0] is A.PROTOTYPES[plain][0]
        assert A.PROTOTYPES[adaptive][1] == A.PROTOTYPES[plain][1] + [A.vp]
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % adaptive, hdr)
        assert m and re.search(r"const\s+gjx_adaptive_opts\s*\*\s*adapt\s*$", m.group(1).strip())
    assert A.PROTOTYPES["gjx_ess"] == (ctypes.c_int, [A.vp, A.i64, A.vp, A.vp, ctypes.c_size_t, A.vp])


def test_adaptive_opts_layout_matches_the_header():
    hdr = _header()
    m = re.search(r"typedef struct gjx_adaptive_opts \{(.*?)\} gjx_adaptive_opts;", hdr, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    c_types = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "float*": ctypes.c_void_p, "int32_t*": ctypes.c_void_p}
    off, declared = 0, []
    for f in fields:
        ty, name = f.rsplit(None, 1)
        ty = ty.replace(" ", "")
        if name.startswith("*"):
            ty, name = ty + "*", name[1:]
        ct = c_types[ty]
        al = ctypes.alignment(ct)
        off = (off + al - 1) // al * al
        declared.append((name, off, ctypes.sizeof(ct)))
        off += ctypes.sizeof(ct)
    assert [d[0] for d in declared] == ["ess_threshold", "reserved", "logw_acc", "ess_steps", "resampled"]
    assert [n for n, _ in A.GjxAdaptiveOpts._fields_] == [d[0] for d in declared]
    for name, o, size in declared:
        fld = getattr(A.GjxAdaptiveOpts, name)
        assert (fld.offset, fld.size) == (o, size), name
    assert ctypes.sizeof(A.GjxAdaptiveOpts) == 32 == (off + 7) // 8 * 8
    assert [getattr(A.GjxAdaptiveOpts, n).offset for n in ("ess_threshold", "reserved", "logw_acc", "ess_steps", "resampled")] == [0, 4, 8, 16, 24]


def test_filter_opts_keep_their_size():
    assert ctypes.sizeof(A.GjxFilterOpts) == 88


def _scan(T=3):
    @genjax.gen
    def step(x_prev, _):
        x = genjax.mv_normal_diag(np.eye(2, dtype=np.float32) @ x_prev, np.full(2, 0.5, np.float32)) @ "x"
        genjax.mv_normal_diag(x, np.full(2, 1.0, np.float32)) @ "y"
        return x, None

    return step.scan(n=T)


def test_constructor_takes_the_threshold_and_refuses_what_cannot_run_with_it():
    from genjax_amd.inference import BootstrapFilter, LinearGaussianSSM
    from genjax_amd.inference.scan_filter import ScanBootstrapFilter
    scan = _scan()
    bf = BootstrapFilter(scan, 1024, ess_threshold=0.5)
    assert isinstance(bf, ScanBootstrapFilter) and bf.ess_threshold == 0.5
    assert BootstrapFilter(scan, 1024).ess_threshold is None
    assert ScanBootstrapFilter(scan, 1024, ess_threshold=0).ess_threshold == 0.0 and ScanBootstrapFilter(scan, 1024, ess_threshold=1).ess_threshold == 1.0
    with pytest.raises(ValueError, match="rejuvenate"):
        BootstrapFilter(scan, 1024, ess_threshold=0.5, rejuvenate=dict(n_moves=1, scale=0.5))
    with pytest.raises(ValueError, match="moves"):
        BootstrapFilter(scan, 1024, ess_threshold=0.5, moves=[genjax.HMC(genjax.S["x"], 0.1, 3)])
    with pytest.raises(ValueError, match="systematic"):
        BootstrapFilter(scan, 1024, ess_threshold=0.5, resampler="multinomial")
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            BootstrapFilter(scan, 1024, ess_threshold=bad)
    ssm = LinearGaussianSSM(np.eye(2, dtype=np.float32), 0.5, 1.0)
    with pytest.raises(ValueError, match=r"@gen.*scan"):
        BootstrapFilter(ssm, 1024, ess_threshold=0.5)
    assert BootstrapFilter(ssm, 1024).K == 1024                                  # (the hand-written filter as before)
    with pytest.raises(NotImplementedError, match="ess_threshold"):
        bf.run_peer(type("Ctx", (), dict(K=1024))(), genjax.key(0), genjax.C["y"].set(np.zeros((3, 2), np.float32)), (np.zeros(2, np.float32), None))
