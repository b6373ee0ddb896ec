"""Dynamic thresholding, host side (CPU, no GPU): the rank rule, the C-ABI additions, the
samplers' and the entry point's new options, and the bounds of the GPU tests checked against an
fp32 emulation of the thresholded step on the GPU tests' own inputs (tests/_thr_cases.py)."""
import ctypes
import math
import os
import re
import subprocess
import sys
import textwrap

import pytest
import torch

from conftest import DROPIN, ROOT

import _cfg_cases as cfg
import _dpm_cases as dpm
import _thr_cases as cases
from _bounds import assert_elementwise
from vdiff import _lib

THR_SYMBOLS = ("vd_x0_quantile_workspace_size", "vd_x0_abs_quantile", "vd_ddim_step_thr",
               "vd_dpm_step_thr")


# ------------------------------------------------------------------ the rank rule
@pytest.mark.parametrize("p", [0.5, 0.9, 0.995, 1.0])
@pytest.mark.parametrize("P", [1, 2, 105, 768])
def test_rank_is_torch_quantile_higher(P, p):
    from vdiff import ops
    g = torch.Generator().manual_seed(P)
    a = torch.randn((3, P), generator=g, dtype=torch.float64).abs()
    k = ops.quantile_rank(p, P)
    assert k == cases.rank(p, P) == min(P - 1, math.ceil(p * (P - 1)))
    want = torch.quantile(a, p, dim=1, interpolation="higher")
    assert torch.equal(cases.order_stat(a, k), want)


def test_rank_rejects_p_outside_the_half_open_interval():
    from vdiff import ops
    for p in (0.0, -0.1, 1.0000001, float("nan")):
        with pytest.raises(ValueError):
            ops.quantile_rank(p, 100)
    assert ops.quantile_rank(1e-300, 100) == 1 and ops.quantile_rank(1.0, 100) == 99


# ------------------------------------------------------------------ the C-ABI
def test_symbols_declared_exported_and_struct_mirrored():
    src = open(os.path.join(ROOT, "include", "vdiff.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(vd_[a-z0-9_]+)\s*\(", code))
    for name in THR_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
    assert "vd_x0_source" in code
    # 8 pointers, int64 n_steps, int32 rule / prediction, float w / rescale
    assert ctypes.sizeof(_lib.X0Source) == 8 * 8 + 8 + 4 * 4 == 88
    assert [n for n, _ in _lib.X0Source._fields_] == re.findall(
        r"(\w+);", code[code.index("enum vd_x0_rule"):code.index("} vd_x0_source")].split("{")[-1])
    assert (_lib.X0_IDENTITY, _lib.X0_DDIM, _lib.X0_DPM) == (0, 1, 2)


def test_invalid_calls_fail_without_a_gpu():
    lib = _lib.load()
    src = _lib.X0Source()
    rc = lib.vd_x0_abs_quantile(None, 0, 1.0, 2.0, 1, 8, 0, None, None, 0, None)
    assert rc == 1 and b"null" in lib.vd_last_error()
    buf = (ctypes.c_float * 64)()
    ws = (ctypes.c_uint32 * 1024)()
    addr, wsa = ctypes.addressof(buf), ctypes.addressof(ws)
    src.x = addr
    n = lib.vd_x0_quantile_workspace_size(1, 8)
    for rank, floor, cap, P, nbytes, word in ((8, 1.0, 2.0, 8, n, b"rank"),
                                              (-1, 1.0, 2.0, 8, n, b"rank"),
                                              (0, 2.0, 1.0, 8, n, b"cap"),
                                              (0, 1.0, float("nan"), 8, n, b"cap"),
                                              (0, 1.0, 2.0, 8, n - 1, b"workspace"),
                                              (0, 1.0, 2.0, 1 << 32, 1 << 40, b"shape")):
        rc = lib.vd_x0_abs_quantile(src, rank, floor, cap, 1, P, 0, addr, wsa, nbytes, None)
        assert rc == 1 and word in lib.vd_last_error(), (rank, floor, cap, P, lib.vd_last_error())
    src.rule = 7
    rc = lib.vd_x0_abs_quantile(src, 0, 1.0, 2.0, 1, 8, 0, addr, wsa, n, None)
    assert rc == 1 and b"rule" in lib.vd_last_error()
    src.rule = _lib.X0_DDIM
    rc = lib.vd_x0_abs_quantile(src, 0, 1.0, 2.0, 1, 8, 0, addr, wsa, n, None)
    assert rc == 1 and b"DDIM" in lib.vd_last_error()
    rc = lib.vd_ddim_step_thr(None, None, None, None, None, None, None, None, None, None, 2.0,
                              0.0, None, 0.0, 0, None, 0, 0, 0, None)
    assert rc == 1 and b"null" in lib.vd_last_error()
    rc = lib.vd_dpm_step_thr(None, None, None, None, None, None, None, 0, None, 2.0, 0.0, None,
                             None, 0, 0, 0, None)
    assert rc == 1 and b"null" in lib.vd_last_error()


def test_workspace_size_is_rows_plus_state():
    lib = _lib.load()
    assert lib.vd_x0_quantile_workspace_size(0, 8) == 0
    for B, P in cases.SELECT_SHAPES + [(1, 1), (1, 3 * 32 * 128 * 128)]:
        nb = cfg.partials(P)[0]
        assert lib.vd_x0_quantile_workspace_size(B, P) == B * (nb * 256 + 4) * 4, (B, P)


# ------------------------------------------------------------------ constructors
def _samplers():
    from vdiff.schedulers import DDIMSampler, DPMSolverSampler
    sch = dpm.v2_scheduler()
    return sch, ((DDIMSampler, dict(steps=6)), (DPMSolverSampler, dict(steps=6)))


def test_constructor_validation_and_exclusivity():
    sch, kinds = _samplers()
    for cls, kw in kinds:
        s = cls(sch, dynamic_threshold=0.995, **kw)
        assert s.thresh == (0.995, math.inf) and s.clip_x0 is False
        s = cls(sch, dynamic_threshold=1.0, threshold_max=2, **kw)
        assert s.thresh == (1.0, 2.0)
        for bad in (dict(dynamic_threshold=0.0), dict(dynamic_threshold=1.5),
                    dict(dynamic_threshold=-0.5), dict(dynamic_threshold=float("nan")),
                    dict(dynamic_threshold=0.9, threshold_max=0.5),
                    dict(dynamic_threshold=0.9, threshold_max=float("nan")),
                    dict(threshold_max=2.0),
                    dict(dynamic_threshold=0.9, clip_x0=True)):
            with pytest.raises(ValueError):
                cls(sch, **kw, **bad)
        with pytest.raises(TypeError):  # keyword-only
            cls(sch, 6, *([0.0, False, "eps"] if cls.__name__ == "DDIMSampler"
                          else [2, "logsnr", False]), 0.995)


def test_option_off_leaves_the_sampler_as_it_was():
    sch, kinds = _samplers()
    for cls, kw in kinds:
        off, on = cls(sch, **kw), cls(sch, dynamic_threshold=0.995, threshold_max=3.0, **kw)
        assert off.thresh is None
        assert set(vars(on)) == set(vars(off))
        for name, v in vars(off).items():
            if name == "thresh":
                continue
            w = getattr(on, name)
            assert torch.equal(v, w) if torch.is_tensor(v) else v == w, name
    from vdiff.schedulers import _thresh_kw
    assert _thresh_kw(off) == {} and _thresh_kw(on) == {"thresh": (0.995, 3.0)}


def test_ops_raise_on_cpu_tensors_and_bad_options():
    from vdiff import ops
    s = cases.dpm_sampler()
    x = torch.randn(2, 64)
    t, tp = torch.tensor([10, 0]), torch.tensor([0, -1])
    acp = cases.acp_table()
    idx = torch.zeros(1, dtype=torch.int64)
    thr = (0.995, math.inf)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.abs_quantile(x, 0.5)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ddim_step(x, x, t, tp, acp, thresh=thr)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ddim_step_cfg(x, x, x, t, tp, acp, 7.5, thresh=thr)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.dpm_step(x, x, x.clone(), s.coef, idx, thresh=thr)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.dpm_step_cfg(x, x, x, x.clone(), s.coef, idx, 7.5, thresh=thr)
    calls = (lambda **kw: ops.ddim_step(x, x, t, tp, acp, **kw),
             lambda **kw: ops.ddim_step_cfg(x, x, x, t, tp, acp, 7.5, **kw),
             lambda **kw: ops.dpm_step(x, x, x.clone(), s.coef, idx, **kw),
             lambda **kw: ops.dpm_step_cfg(x, x, x, x.clone(), s.coef, idx, 7.5, **kw))
    for call in calls:
        for bad in (dict(thresh=(0.0, 2.0)), dict(thresh=(1.1, 2.0)), dict(thresh=(0.9, 0.5)),
                    dict(thresh=0.9), dict(thresh=thr, clip=True)):
            with pytest.raises(ValueError):
                call(**bad)
    with pytest.raises(ValueError):
        ops.abs_quantile(x, 0.0)


# ------------------------------------------------------------------ the entry point
def _dropin(code, ok=True):
    src = f"import sys; sys.path.insert(0, {DROPIN!r}); sys.path.insert(1, {ROOT!r})\n"
    out = subprocess.run([sys.executable, "-c", src + textwrap.dedent(code)],
                         capture_output=True, text=True, timeout=600)
    assert (out.returncode == 0) == ok, out.stderr[-3000:]
    return out


def test_entry_point_flags():
    out = _dropin("""
        import json, test
        a = test.parse([])
        b = test.parse(["--sampler", "ddim", "--dynamic-threshold", "0.995"])
        c = test.parse(["--sampler", "dpm++", "--dynamic-threshold", "0.9", "--threshold-max",
                        "2.5", "--dims", "3", "--frames", "4", "--clip-frames", "8"])
        print(json.dumps([[a.dynamic_threshold, a.threshold_max],
                          [b.dynamic_threshold, b.threshold_max],
                          [c.dynamic_threshold, c.threshold_max, c.clip_frames]]))
    """)
    import json
    assert json.loads(out.stdout.strip().splitlines()[-1]) == [[None, None], [0.995, None],
                                                               [0.9, 2.5, 8]]


@pytest.mark.parametrize("argv", [["--dynamic-threshold", "0.995"],
                                  ["--sampler", "ddpm-v2", "--dynamic-threshold", "0.995"],
                                  ["--sampler", "ddim", "--dynamic-threshold", "1.5"],
                                  ["--sampler", "ddim", "--threshold-max", "2"],
                                  ["--sampler", "ddim", "--dynamic-threshold", "0.9",
                                   "--threshold-max", "0.5"]])
def test_entry_point_refuses(argv):
    """ancestral DDPM (the default sampler) has no x0 clamp to replace: an argparse error (exit
    status 2 and a usage message), as for the other bad values."""
    out = _dropin(f"import test; test.parse({argv!r})", ok=False)
    assert out.returncode == 2 and "usage:" in out.stderr and "error:" in out.stderr, out.stderr


# ------------------------------------------------------------------ emulation against the bounds
def _rule(kind, B):
    if kind == "dpm":
        s = cases.dpm_sampler()
        return [dict(row=s.coef[i]) for i in dpm.kernel_rows(s)]
    t, tp = cfg.timesteps(B)
    return [dict(t=t, tp=tp, acp=cases.acp_table())]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("B,P", cases.SHAPES)
def test_fp32_emulation_stays_inside_the_bounds(B, P, kind, bf16):
    """The bounds of tests/test_gpu_thr.py hold for the reference arithmetic alone: x0 formed in
    fp32 on the CPU (every operation rounded, no fused multiply-add), the exact order statistic
    of those fp32 values, the clamp and the divide, against the fp64 references on the GPU
    test's own inputs.  The threshold is live on them: q > 1 for every sample."""
    xt, c, u, z = cfg.inputs(B, P, bf16)
    worst = 0.0
    for rule in _rule(kind, B):
        for guide in cases.GUIDES:
            base, K = cases.base64(kind, xt, c, u, z, guide, **rule)
            for tmax in (math.inf, 2.0):
                ref = cases.thresholded(base, K, tmax=tmax)
                what = f"{kind} B={B} P={P} bf16={bf16} guide={guide} tmax={tmax}"
                assert (ref["q"] > 1).all(), (what, ref["q"])
                s, y, xp = cases.emulate32(kind, xt, c, u, z, guide, tmax=tmax, **rule)
                s_ref, Delta = ref["s"]
                assert ((s.double() - s_ref).abs() <= Delta).all(), what
                if tmax == 2.0:
                    assert (s == 2).all() and (s_ref == 2).all(), what
                if bf16:
                    y, xp = y.bfloat16().float(), xp.bfloat16().float()
                for name, got in (("x0", y), ("x_prev", xp)):
                    r, m, n, ce = ref[name]
                    worst = max(worst, assert_elementwise(got, r, m, n, bf16, ce,
                                                          what=f"{name} {what}"))
    assert 0 < worst <= 1


def test_floor_case_is_the_static_clamp():
    """Inputs scaled by 0.2 at t = 0: q = 0.84 < 1, s is exactly 1 and the thresholded
    references are the clamped ones."""
    B, P = 2, 5000
    xt, c, u, z = (0.2 * v for v in cfg.inputs(B, P, False))
    t, tp = torch.zeros(B, dtype=torch.int64), torch.full((B,), -1)
    base, K = cases.base64("ddim-eps", xt, c, u, z, None, t=t, tp=tp, acp=cases.acp_table())
    ref = cases.thresholded(base, K)
    assert (ref["q"] < 1).all() and (ref["q"] > 0.5).all(), ref["q"]
    assert (ref["s"][0] == 1).all()
    clip = cases.clipped(base, K)
    assert torch.equal(ref["x0"][0], clip["x0"][0])
    assert torch.equal(ref["x_prev"][0], clip["x_prev"][0])
    s, y, xp = cases.emulate32("ddim-eps", xt, c, u, z, None, t=t, tp=tp, acp=cases.acp_table())
    assert (s == 1).all() and y.abs().max() <= 1


def test_heavy_ties_in_the_bf16_inputs():
    """The tie case of the GPU selection test, counted here: bf16 keeps 8 significant bits, so
    5000 values of a few binades hold far fewer than 2500 distinct magnitudes (875 and 881 in
    xt's two rows); the fp32 ones are all distinct."""
    xt = cfg.inputs(2, 5000, bf16=True)[0]
    assert all(int(r.abs().unique().numel()) < 2500 for r in xt)
    assert all(int(r.abs().unique().numel()) == 5000 for r in cfg.inputs(2, 5000, False)[0])
