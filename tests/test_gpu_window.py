"""Long-clip sampling on the GPU: vd_window_gather against torch indexing (exact),
vd_window_blend against fp64 with element-wise bounds (tests/_window_cases.py), sample_long
against the samplers on the whole clip through a frame-local model (bit for bit), the single
window as the old path, the replayed graph against the eager loop, argument checks and the
entry point."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import DROPIN, record_metric

import _dpm_cases as dpm_cases
import _window_cases as cases
from _bounds import assert_elementwise

pytestmark = pytest.mark.gpu
dev = "cuda"
DTYPES = pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])


def _plan(*a, **kw):
    from vdiff.schedulers import WindowPlan
    return WindowPlan(*a, **kw)


def _dt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


# ------------------------------------------------------------------ 4. gather
@DTYPES
@pytest.mark.parametrize("B,C,L,T,S,HW", cases.KERNEL_SHAPES)
def test_gather_is_exact(B, C, L, T, S, HW, bf16):
    from vdiff import ops
    p = _plan(L, T, S)
    x = cases.inputs(B, C, L, HW, bf16, seed=1)
    want = cases.gather_ref(x, L, T, S).to(_dt(bf16))
    x_d = x.to(device=dev, dtype=_dt(bf16))
    win = ops.window_gather(x_d, p)
    assert tuple(win.shape) == (B * p.num_windows, C, T, HW) and win.dtype == x_d.dtype
    assert torch.equal(win.cpu(), want)
    # into the halves of a doubled window batch, as a guided step does
    n = B * p.num_windows
    buf = torch.full((2 * n, C, T, HW), float("nan"), dtype=x_d.dtype, device=dev)
    got = ops.window_gather(x_d, p, out=buf[:n], dup=buf[n:])
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:n], win) and torch.equal(buf[n:], win)
    # a 5-d clip [B, C, L, H, W] is the same memory
    if HW % 4 == 0:
        win5 = ops.window_gather(x_d.view(B, C, L, 4, HW // 4), p)
        assert tuple(win5.shape) == (n, C, T, 4, HW // 4) and torch.equal(win5.flatten(3), win)


# ------------------------------------------------------------------ 5. blend against fp64
@DTYPES
@pytest.mark.parametrize("blend", cases.BLENDS)
def test_blend_against_fp64(blend, bf16):
    """Every kernel shape; n_terms is the plan's largest coverage K: the kernel rounds the first
    product and each of the K - 1 fused multiply-adds once (_window_cases.blend_ref64).  Each
    shape lies inside its bound element by element; 0 < worst is asserted on the largest error /
    bound over the shapes, because the one-window shape has the weight exactly 1 and returns its
    input's own bits (error 0).  Measured on an MI355X: 0.19 (fp32) and 0.996 (bf16: the output's
    own rounding, half an ulp of a value just above a power of two)."""
    worst = 0.0
    for B, C, L, T, S, HW in cases.KERNEL_SHAPES:
        worst = max(worst, _blend_case(B, C, L, T, S, HW, blend, bf16))
    assert 0 < worst <= 1


def _blend_case(B, C, L, T, S, HW, blend, bf16):
    from vdiff import ops
    p = _plan(L, T, S, blend)
    W, st = p.num_windows, p.starts.tolist()
    win = cases.inputs(B * W, C, T, HW, bf16, seed=2)
    win_d = win.to(device=dev, dtype=_dt(bf16))
    ref, mag = cases.blend_ref64(win, st, p.cover_win, p.cover_wgt, L)
    out = ops.window_blend(win_d, p)
    assert tuple(out.shape) == (B, C, L, HW) and out.dtype == win_d.dtype
    what = f"B={B} C={C} L={L} T={T} S={S} HW={HW} {blend} bf16={bf16}"
    worst = assert_elementwise(out, ref, mag, p.max_coverage, bf16, what=what)
    print(f"window_blend {what}: largest error / bound {worst:.3g}")
    record_metric(test="window_blend_fp64", B=B, C=C, L=L, T=T, S=S, HW=HW, blend=blend,
                  dtype="bf16" if bf16 else "fp32", worst=worst)
    assert worst <= 1
    # out= into a preallocated buffer: the same bits
    buf = torch.full((B, C, L, HW), float("nan"), dtype=win_d.dtype, device=dev)
    got = ops.window_blend(win_d, p, out=buf)
    assert got.data_ptr() == buf.data_ptr() and torch.equal(buf, out)
    # a frame covered once is the window's own values
    w5 = win_d.view(B, W, C, T, HW)
    single = [l for l in range(L) if int((p.cover_win[l] >= 0).sum()) == 1]
    assert single and 0 in single and L - 1 in single
    for l in single:
        w = int(p.cover_win[l, 0])
        assert torch.equal(out[:, :, l], w5[:, w, :, l - st[w]]), (what, l)
    return worst


@DTYPES
@pytest.mark.parametrize("B,C,L,T,S,HW", cases.KERNEL_SHAPES)
def test_blend_skips_unused_slots(B, C, L, T, S, HW, bf16):
    """Only the table decides what is read.  Every frame keeps its first covering window alone
    (weight 1, the other slots -1 with a NaN weight), and the window tensor is NaN at every
    frame the table no longer names: the output is finite and is the named frames' own bits."""
    from vdiff import ops
    base = _plan(L, T, S)
    W, st = base.num_windows, base.starts.tolist()
    p = copy.copy(base)
    p._dev = {}
    p.cover_win = base.cover_win.clone()
    p.cover_win[:, 1:] = -1
    p.cover_wgt = torch.full_like(base.cover_wgt, float("nan"))
    p.cover_wgt[:, 0] = 1.0
    win = cases.inputs(B * W, C, T, HW, bf16, seed=3).view(B, W, C, T, HW)
    named = torch.zeros((W, T), dtype=torch.bool)
    for l in range(L):
        w = int(p.cover_win[l, 0])
        named[w, l - st[w]] = True
    assert bool((~named).any()) == (base.max_coverage > 1)
    win = torch.where(named.view(1, W, 1, T, 1), win, torch.full_like(win, float("nan")))
    win_d = win.to(device=dev, dtype=_dt(bf16)).view(B * W, C, T, HW)
    out = ops.window_blend(win_d, p)
    assert torch.isfinite(out).all()
    for l in range(L):
        w = int(p.cover_win[l, 0])
        assert torch.equal(out[:, :, l], win_d.view(B, W, C, T, HW)[:, w, :, l - st[w]]), l
    # window indices and local frames outside their ranges are skipped too, not followed
    p2 = copy.copy(base)
    p2._dev = {}
    p2.cover_win = base.cover_win.clone()
    p2.cover_wgt = base.cover_wgt.clone()
    for k, bad in ((base.max_coverage, W), (base.max_coverage + 1, 1 << 30),
                   (base.max_coverage + 2, -7)):
        p2.cover_win[:, k] = bad
        p2.cover_wgt[:, k] = float("nan")
    if W > 1:  # a window that does not hold the frame: local frame outside [0, T)
        p2.cover_win[0, base.max_coverage + 3] = W - 1
        p2.cover_wgt[0, base.max_coverage + 3] = float("nan")
    clean = cases.inputs(B * W, C, T, HW, bf16, seed=3).to(device=dev, dtype=_dt(bf16))
    assert torch.equal(ops.window_blend(clean, p2), ops.window_blend(clean, base))


# ------------------------------------------------------------------ 6. frame-local model
class FrameLocalEps(torch.nn.Module):
    """eps = c[t] x + feats[b T + f, 0] + mean(cond[b]) per frame, in fp32: GaussEps's shape
    (tests/test_gpu_dpm.py) plus the frame's own audio feature and the clip's reference image.
    Its output at a frame does not depend on the window the frame arrives in.  Every operation
    is elementwise but the mean, which is written as sum / count over values that are multiples
    of 1/8 (_frame_local_case): the sum is exact in fp32 in any order, so the mean has the same
    bits at every batch size."""

    def __init__(self, acp, s):
        super().__init__()
        a = acp.double()
        self.register_buffer("c", (torch.sqrt(1 - a) / (a * s * s + 1 - a)).float())

    def forward(self, x, cond, feats, t):
        B, _, T = x.shape[:3]
        a = feats[:, 0].reshape(B, 1, T, 1, 1)
        m = (cond.sum(dim=(1, 2, 3)) / cond[0].numel()).view(B, 1, 1, 1, 1)
        return self.c[t].view(B, 1, 1, 1, 1) * x + a + m


def _frame_local_case(B=2, L=10, H=8):
    g = torch.Generator(device=dev).manual_seed(31)
    cond = torch.randint(-8, 9, (B, 3, H, H), device=dev, generator=g).float() / 8
    feats = torch.randn((B * L, 16), device=dev, generator=g)
    return (B, 3, L, H, H), cond, feats


def _samplers(name, steps):
    from vdiff.engine import sample_ddim, sample_dpm
    from vdiff.schedulers import DDIMSampler, DPMSolverSampler
    sch = dpm_cases.v2_scheduler()
    if name == "ddim":
        return DDIMSampler(sch, steps=steps), sample_ddim
    return DPMSolverSampler(sch, steps=steps), sample_dpm


@pytest.mark.parametrize("graph", ["0", "1"], ids=["eager", "graph"])
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("name", ["ddim", "dpm++"])
def test_frame_local_model_gives_the_long_clips_own_bits(name, guided, graph, monkeypatch):
    """L = 10, T = 4, S = 2, uniform blend: every weight is 0.5 or 1, and 0.5 v + 0.5 v = v
    exactly, so with a model whose output at a frame is the same in every window the blended
    prediction IS the whole-clip prediction and sample_long must return the bits of the sampler
    run on the full 10-frame shape.  A wrong audio-feature, cond or guided-half routing changes
    the values."""
    from vdiff.engine import sample_long
    monkeypatch.setenv("VDIFF_DDIM_GRAPH", graph)
    shape, cond, feats = _frame_local_case()
    sampler, sample = _samplers(name, 6)
    model = FrameLocalEps(dpm_cases.v2_scheduler().alpha_cum_prod.float(), 0.5).to(dev)
    kw = dict(guidance_scale=3.0, guidance_rescale=0.7) if guided else {}
    want_traj = []
    want = sample(model, sampler, cond, feats, shape,
                  generator=torch.Generator(device=dev).manual_seed(5),
                  callback=lambda i, xt, x0: want_traj.append((xt.clone(), x0.clone())), **kw)
    assert torch.isfinite(want[1]).all() and want[1].abs().max() > 0
    for window_batch in (None, 1):
        traj = []
        got = sample_long(model, sampler, cond, feats, shape, window=4, stride=2,
                          blend="uniform", window_batch=window_batch,
                          generator=torch.Generator(device=dev).manual_seed(5),
                          callback=lambda i, xt, x0: traj.append((xt.clone(), x0.clone())), **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), window_batch
        assert len(traj) == len(want_traj) == sampler.steps
        for i, ((xa, x0a), (xb, x0b)) in enumerate(zip(traj, want_traj)):
            assert torch.equal(xa, xb) and torch.equal(x0a, x0b), (window_batch, i)
    # the feature and the reference image do reach the output
    other = sample_long(model, sampler, cond, feats.flip(0).contiguous(), shape, window=4,
                        stride=2, blend="uniform",
                        generator=torch.Generator(device=dev).manual_seed(5), **kw)
    assert not torch.equal(other[1], want[1])


# ------------------------------------------------------------------ 7., 8. the tiny UNet
def _unet_case(L):
    g = torch.Generator(device=dev).manual_seed(77)
    cond = torch.rand((1, 3, 32, 32), device=dev, generator=g) * 2 - 1
    feats = torch.randn((L, 64), device=dev, generator=g)
    return (1, 3, L, 32, 32), cond, feats


_models = {}


def _model(bf16):
    from test_gpu_dpm import _model as tiny
    if bf16 not in _models:
        _models[bf16] = tiny(3, bf16)
    return _models[bf16]


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("name", ["ddim", "dpm++"])
def test_single_window_is_the_old_path(name, guided):
    from vdiff.engine import sample_long
    m = _model(True)
    shape, cond, feats = _unet_case(4)
    sampler, sample = _samplers(name, 3)
    kw = dict(guidance_scale=3.0, guidance_rescale=0.7) if guided else {}
    want = sample(m, sampler, cond, feats, shape,
                  generator=torch.Generator(device=dev).manual_seed(9), **kw)
    got = sample_long(m, sampler, cond, feats, shape, window=4,
                      generator=torch.Generator(device=dev).manual_seed(9), **kw)
    assert torch.isfinite(got[1]).all() and got[1].abs().max() > 0
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", ["ddim", "dpm++"])
def test_long_graph_matches_eager(name, bf16, guided, monkeypatch):
    from vdiff.engine import sample_long
    m = _model(bf16)
    shape, cond, feats = _unet_case(8)
    sampler, _ = _samplers(name, 6)
    assert sampler.steps == 6
    kw = dict(guidance_scale=3.0, guidance_rescale=0.7) if guided else {}
    out, traj = {}, {}
    for mode in ("0", "1"):
        monkeypatch.setenv("VDIFF_DDIM_GRAPH", mode)
        seen = traj[mode] = []
        out[mode] = sample_long(m, sampler, cond, feats, shape, window=4, stride=2,
                                generator=torch.Generator(device=dev).manual_seed(9),
                                callback=lambda i, xt, x0: seen.append((xt, x0)), **kw)
    for a, b in zip(out["0"], out["1"]):
        assert tuple(a.shape) == shape
        assert torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b)
    assert len(traj["0"]) == len(traj["1"]) == 6
    for i, ((xa, x0a), (xb, x0b)) in enumerate(zip(traj["0"], traj["1"])):
        assert torch.equal(xa, xb) and torch.equal(x0a, x0b), i
    x0s = [x0 for _, x0 in traj["1"]]
    assert all(not torch.equal(x0s[i], x0s[i + 1]) for i in range(5))
    assert torch.equal(traj["1"][-1][1], out["1"][1])


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("name", ["ddim", "dpm++"])
def test_long_graph_holds_no_memset_node(name, guided):
    from vdiff import ops
    from vdiff.engine import LongDDIMGraph, LongDPMGraph, WindowedDenoiser
    m = _model(True)
    shape, cond, feats = _unet_case(8)
    sampler, _ = _samplers(name, 6)
    plan = _plan(8, 4, 2)
    kw = dict(guidance_scale=3.0, guidance_rescale=0.7) if guided else {}
    with torch.no_grad(), ops.frozen_weights():
        xt = torch.randn(shape, device=dev)
        windows = WindowedDenoiser(m, plan, cond, feats, xt, guided)
        assert windows.rows == (6 if guided else 3)
        gr = (LongDDIMGraph if name == "ddim" else LongDPMGraph)(m, sampler, windows, xt, **kw)
        assert gr.t.numel() == windows.rows
        gr.capture()
        types = gr.node_types()
        assert types.get("memset", 0) == 0 and types.get("kernel", 0) > 20, types
        got, x0 = gr.step(0)
        assert tuple(got.shape) == shape and tuple(x0.shape) == shape
        assert torch.isfinite(got).all() and torch.isfinite(x0).all()
        assert not torch.equal(got, xt)


# ------------------------------------------------------------------ 9. argument checks
def test_argument_checks():
    from vdiff import ops
    from vdiff.engine import sample_long
    p = _plan(10, 4, 2)
    x = torch.randn(2, 3, 10, 64, device=dev)
    win = ops.window_gather(x, p)
    assert tuple(win.shape) == (8, 3, 4, 64)
    for bad_x in (x[:, :, :9].contiguous(), x[0]):
        with pytest.raises(ValueError):
            ops.window_gather(bad_x, p)
    with pytest.raises(ValueError):
        ops.window_gather(x.transpose(0, 1).contiguous().transpose(0, 1), p)
    for bad_out in (win[:7], win.bfloat16(), torch.empty(8, 3, 4, 128, device=dev)[..., ::2]):
        with pytest.raises(ValueError):
            ops.window_gather(x, p, out=bad_out)
        with pytest.raises(ValueError):
            ops.window_gather(x, p, dup=bad_out)
    for bad_win in (win[:7], win[:, :, :3].contiguous(),
                    torch.empty(8, 3, 4, 128, device=dev)[..., ::2]):
        with pytest.raises(ValueError):
            ops.window_blend(bad_win, p)
    for bad_out in (x[:1], x.bfloat16(), torch.empty(2, 3, 10, 128, device=dev)[..., ::2]):
        with pytest.raises(ValueError):
            ops.window_blend(win, p, out=bad_out)
    with pytest.raises(RuntimeError):
        ops.window_gather(x.cpu(), p)
    with pytest.raises(RuntimeError):
        ops.window_gather(x, p, out=win.cpu())
    with pytest.raises(RuntimeError):
        ops.window_blend(win.cpu(), p)
    with pytest.raises(RuntimeError):
        ops.window_blend(win, p, out=x.cpu())
    # the sampler's type, and conditioning that does not fit the clip
    sch = dpm_cases.v2_scheduler()
    shape, cond, feats = _frame_local_case()
    model = FrameLocalEps(sch.alpha_cum_prod.float(), 0.5).to(dev)
    with pytest.raises(TypeError):
        sample_long(model, sch, cond, feats, shape, window=4)
    sampler, _ = _samplers("ddim", 3)
    with pytest.raises(ValueError):
        sample_long(model, sampler, cond, feats[:-1], shape, window=4)
    with pytest.raises(ValueError):
        sample_long(model, sampler, cond[:1], feats, shape, window=4)


# ------------------------------------------------------------------ 10. entry point
def _entry(tmp_path, *extra):
    out_dir = tmp_path / "imgs"
    out = subprocess.run([sys.executable, os.path.join(DROPIN, "test.py"), "--random-init",
                          "--dims", "3", "--frames", "4", "--steps", "3", "--image-size", "32",
                          "--save-every", "1", "--out-dir", str(out_dir)] + list(extra),
                         cwd=tmp_path, capture_output=True, text=True, timeout=600)
    files = sorted(p for p in os.listdir(out_dir) if p.endswith(".npy")) \
        if os.path.isdir(out_dir) else []
    return out, out_dir, files


def test_entry_point_long_clip(tmp_path):
    out, out_dir, files = _entry(tmp_path, "--clip-frames", "10", "--window-stride", "2",
                                 "--sampler", "dpm++")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert files == ["x0_0.npy", "x0_1.npy", "x0_2.npy"], files
    for f in files:
        x0 = np.load(out_dir / f)
        assert x0.shape == (1, 3, 10, 32, 32) and np.isfinite(x0).all()


def test_entry_point_refuses_the_ancestral_sampler(tmp_path):
    out, _, files = _entry(tmp_path, "--clip-frames", "10", "--window-stride", "2", "--sampler",
                           "ddpm-v2")
    assert out.returncode != 0 and not files
    assert "--sampler ddim or dpm++" in out.stderr


def test_entry_point_without_clip_frames(tmp_path):
    out, out_dir, files = _entry(tmp_path, "--sampler", "dpm++")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert files == ["x0_0.npy", "x0_1.npy", "x0_2.npy"], files
    for f in files:
        x0 = np.load(out_dir / f)
        assert x0.shape == (1, 3, 4, 32, 32) and np.isfinite(x0).all()
