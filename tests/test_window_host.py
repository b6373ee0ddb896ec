"""Long-clip sampling, host side (CPU, no GPU): the window plan against an independent exact
computation (tests/_window_cases.py), its errors, the C-ABI additions, the new signatures and the
entry point's options."""
import inspect
import json
import os
import re
import subprocess
import sys
import textwrap

import pytest
import torch

from conftest import DROPIN, ROOT

import _window_cases as cases
from vdiff import _lib

WINDOW_SYMBOLS = ("vd_window_gather", "vd_window_blend")


def _plan(*a, **kw):
    from vdiff.schedulers import WindowPlan
    return WindowPlan(*a, **kw)


# ------------------------------------------------------------------ 1. plan structure
@pytest.mark.parametrize("blend", cases.BLENDS)
@pytest.mark.parametrize("L,T,S", cases.PLANS)
def test_plan_structure(L, T, S, blend):
    p = _plan(L, T, S, blend)
    st = cases.starts(L, T, S)
    W = cases.n_windows(L, T, S)
    assert (p.length, p.window, p.stride, p.blend, p.num_windows) == (L, T, S, blend, W)
    assert p.starts.dtype == torch.int32 and p.starts.tolist() == st
    assert len(set(st)) == W and st == sorted(st) and st[0] == 0 and st[-1] == L - T
    assert p.KMAX == 8 == _lib.WINDOW_KMAX
    assert p.cover_win.dtype == torch.int32 and tuple(p.cover_win.shape) == (L, 8)
    assert p.cover_wgt.dtype == torch.float32 and tuple(p.cover_wgt.shape) == (L, 8)
    assert p.weights64.dtype == torch.float64 and tuple(p.weights64.shape) == (L, 8)
    assert torch.equal(p.cover_wgt, p.weights64.float())
    want_cover, want_w = cases.cover(L, T, S), cases.weights(L, T, S, blend)
    assert p.max_coverage == cases.max_coverage(L, T, S)
    for l in range(L):
        K = len(want_cover[l])
        assert K >= 1, l  # every frame is covered
        assert p.cover_win[l, :K].tolist() == want_cover[l]  # ascending by construction
        assert (p.cover_win[l, K:] == -1).all() and (p.weights64[l, K:] == 0).all()
        got = p.weights64[l, :K].tolist()
        # one correctly rounded fp64 division of two small integers: the exact quotient rounded
        assert got == [float(f) for f in want_w[l]], (l, got, want_w[l])
        assert abs(sum(got) - 1.0) <= 4 * 2.0 ** -53 * K
        if K == 1:
            assert got == [1.0] and float(p.cover_wgt[l, 0]) == 1.0
    assert p.frame_index.dtype == torch.int64
    assert p.frame_index.tolist() == [s + f for s in st for f in range(T)]


def test_plan_examples_of_the_specification():
    assert _plan(11, 4, 3).starts.tolist() == [0, 3, 6, 7]
    p = _plan(9, 4, 2)
    assert p.starts.tolist() == [0, 2, 4, 5]
    assert p.cover_win[5, :4].tolist() == [1, 2, 3, -1] and p.max_coverage == 3
    assert p.weights64[5, :3].tolist() == [0.25, 0.5, 0.25]  # triangle: g = 1, 2, 1
    assert _plan(4, 4, 4).num_windows == 1 and _plan(4, 4).stride == 2
    u = _plan(10, 4, 2, "uniform")
    used = u.cover_wgt[u.cover_win >= 0]
    assert set(used.tolist()) == {0.5, 1.0}
    assert _plan(40, 16).stride == 8 and _plan(40, 16).num_windows == 4


def test_tables_are_cached_per_device():
    p = _plan(10, 4, 2)
    a, b = p._tables("cpu"), p._tables(torch.device("cpu"))
    assert all(x is y for x, y in zip(a, b)) and len(a) == 3
    assert [t.dtype for t in a] == [torch.int32, torch.int32, torch.float32]
    assert all(t.is_contiguous() for t in a)


# ------------------------------------------------------------------ 2. errors
def test_plan_value_errors():
    for args in ((3, 4), (10, 4, 0), (10, 4, 5), (10, 4, -1), (10, 0), (10, -2, 1)):
        with pytest.raises(ValueError):
            _plan(*args)
    with pytest.raises(ValueError):
        _plan(10, 4, 2, "cosine")
    with pytest.raises(ValueError, match="stride 1"):
        _plan(40, 16, 1)  # coverage 16 > 8
    assert _plan(40, 16, 2).max_coverage == 8


# ------------------------------------------------------------------ 3. C ABI
def test_symbols_declared_and_exported():
    import ctypes
    src = open(os.path.join(ROOT, "include", "vdiff.h")).read()
    assert re.search(r"#define\s+VD_WINDOW_KMAX\s+8\b", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(vd_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in WINDOW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name


def test_bad_arguments_fail_without_a_gpu():
    lib = _lib.load()
    rc = lib.vd_window_gather(None, None, None, None, 1, 3, 10, 4, 4, 64, 0, None)
    assert rc == 1 and b"null" in lib.vd_last_error()
    rc = lib.vd_window_blend(None, None, None, None, None, 8, 1, 3, 10, 4, 4, 64, 0, None)
    assert rc == 1 and b"null" in lib.vd_last_error()
    # refused before anything is launched: the pointers are never followed
    p = 4096
    for B, C, L, T, W, HW in ((0, 3, 10, 4, 4, 64), (1, 0, 10, 4, 4, 64), (1, 3, 0, 4, 4, 64),
                              (1, 3, 10, 0, 4, 64), (1, 3, 10, 4, 0, 64), (1, 3, 10, 4, 4, 0),
                              (1, 3, 10, 4, 4, -8)):
        assert lib.vd_window_gather(p, p, None, p, B, C, L, T, W, HW, 0, None) == 1
        assert b"empty" in lib.vd_last_error()
        assert lib.vd_window_blend(p, p, p, p, p, 8, B, C, L, T, W, HW, 0, None) == 1
        assert b"empty" in lib.vd_last_error()
    assert lib.vd_window_gather(p, p, None, p, 1, 3, 3, 4, 1, 64, 0, None) == 1
    assert b"longer" in lib.vd_last_error()
    assert lib.vd_window_blend(p, p, p, p, p, 8, 1, 3, 3, 4, 1, 64, 0, None) == 1
    assert b"longer" in lib.vd_last_error()
    for kmax in (0, 9, -1):
        assert lib.vd_window_blend(p, p, p, p, p, kmax, 1, 3, 10, 4, 4, 64, 0, None) == 1
        assert b"kmax" in lib.vd_last_error()
    # the 32-bit index parts: B * W * C and L * HW below 2^31
    assert lib.vd_window_gather(p, p, None, p, 1 << 20, 3, 10, 4, 1 << 10, 64, 0, None) == 1
    assert b"too large" in lib.vd_last_error()
    assert lib.vd_window_blend(p, p, p, p, p, 8, 1, 3, 1 << 16, 4, 4, 1 << 15, 0, None) == 1
    assert b"too large" in lib.vd_last_error()


# ------------------------------------------------------------------ signatures
def test_signatures_and_defaults():
    from vdiff import engine, ops
    from vdiff.schedulers import WindowPlan
    ps = inspect.signature(WindowPlan.__init__).parameters
    assert list(ps)[1:] == ["length", "window", "stride", "blend"]
    assert ps["stride"].default is None and ps["blend"].default == "triangle"
    ps = inspect.signature(engine.sample_long).parameters
    assert list(ps) == ["model", "sampler", "cond", "audio", "shape", "window", "stride", "blend",
                        "window_batch", "generator", "callback", "guidance_scale",
                        "guidance_rescale"]
    assert [ps[n].default for n in list(ps)[6:]] == [None, "triangle", None, None, None, 1.0, 0.0]
    assert list(inspect.signature(ops.window_gather).parameters) == ["x", "plan", "out", "dup"]
    assert list(inspect.signature(ops.window_blend).parameters) == ["win", "plan", "out"]
    assert issubclass(engine.LongDDIMGraph, engine.DDIMGraph)
    assert issubclass(engine.LongDPMGraph, engine.DPMGraph)
    # what the long-clip graphs keep from their parents
    for cls, base in ((engine.LongDDIMGraph, engine.DDIMGraph),
                      (engine.LongDPMGraph, engine.DPMGraph)):
        for name in ("capture", "node_types", "step"):
            assert getattr(cls, name) is getattr(base, name), (cls.__name__, name)


def test_sample_long_refuses_other_samplers_and_shapes():
    from vdiff.engine import sample_long
    from vdiff.schedulers import DDIMSampler, LinearNoiseSchedulerV2
    sch = LinearNoiseSchedulerV2(500, 0.00005, 0.015)
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(TypeError):
        sample_long(None, sch, x, None, (1, 3, 8, 8, 8), window=4)
    s = DDIMSampler(sch, steps=3)
    with pytest.raises(ValueError):
        sample_long(None, s, x, None, (1, 3, 8, 8), window=4)  # not a 5-d shape
    with pytest.raises(ValueError):
        sample_long(None, s, x, None, (1, 3, 3, 8, 8), window=4)  # L < T
    with pytest.raises(ValueError):
        sample_long(None, s, x, None, (1, 3, 8, 8, 8), window=4, window_batch=0)


# ------------------------------------------------------------------ entry point options
def _dropin(code):
    src = f"import sys; sys.path.insert(0, {DROPIN!r}); sys.path.insert(1, {ROOT!r})\n"
    out = subprocess.run([sys.executable, "-c", src + textwrap.dedent(code)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.strip().splitlines()[-1]


def test_entry_point_options():
    out = _dropin("""
        import json, test
        a = test.parse([])
        b = test.parse(["--dims", "3", "--frames", "4", "--clip-frames", "10", "--window-stride",
                        "2", "--window-blend", "uniform", "--window-batch", "2", "--sampler",
                        "dpm++"])
        c = test.parse(["--dims", "3", "--frames", "4", "--clip-frames", "4"])
        refused = []
        for argv in (["--dims", "3", "--frames", "4", "--clip-frames", "10"],
                     ["--dims", "3", "--frames", "4", "--clip-frames", "10", "--sampler",
                      "ddpm-v2"],
                     ["--dims", "2", "--clip-frames", "10", "--sampler", "ddim"],
                     ["--dims", "3", "--frames", "4", "--clip-frames", "3", "--sampler", "ddim"]):
            try:
                test.parse(argv)
                refused.append(None)
            except SystemExit as e:
                refused.append(str(e.code))
        print(json.dumps({
            "default": [a.clip_frames, a.window_stride, a.window_blend, a.window_batch],
            "set": [b.clip_frames, b.window_stride, b.window_blend, b.window_batch],
            "equal": [c.clip_frames, c.sampler], "refused": refused}))
    """)
    d = json.loads(out)
    assert d["default"] == [None, None, "triangle", None]
    assert d["set"] == [10, 2, "uniform", 2]
    assert d["equal"] == [4, "ddpm-v2"]  # a clip of one window: every sampler as before
    assert all(m and "frames" in m for m in d["refused"])
    assert all("--sampler ddim or dpm++" in m for m in d["refused"][:3])
