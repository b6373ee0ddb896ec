"""Run-to-run bit identity and fp64 checks of the LDS-DMA ring kernels at full ring depth.

Every bf16 GEMM-like kernel streams its operands through an LDS ring filled by buffer_load ...
lds and ordered by a counted vmcnt plus s_barrier (csrc/vd_common.h).  A barrier that lets
another wave's refill land in a stage while a read of that stage is still in flight shows as a
result that differs from launch to launch, and only at sizes where the ring runs many rounds on
a grid that fills the chip: the element-wise suites (a few hundred pixels or tokens) cannot see
it.  test_gpu_conv.py::test_halo_conv_is_deterministic covers the halo kernel; this file covers
the gathered conv GEMM (igemm_dma_kernel), wgrad_dma_kernel and the compiled attention rings.
profiles/ring_barriers.md is the reading of each ring barrier in the gfx950 ISA.

Each case launches 12 times (the count of the halo test) into separate outputs, from the same
device-built inputs, without a synchronisation in between; every output must be torch.equal to
launch 0, and launch 0 must be inside the fp64 bound of the same bf16-rounded operands, so a
kernel that is repeatably wrong fails too.  Conv: tests/_bounds.py assert_elementwise at sampled
elements (conv_ref64_at: the full fp64 conv is ~30 GFLOP at these sizes); linear: the whole fp64
matmul; attention: tests/_attn_rows.py Host.judge on the whole case.
"""
import functools

import pytest
import torch

from conftest import record_metric  # first: puts the repository on sys.path

import _attn_rows as A
from _bounds import (assert_elementwise, conv_ref64_at, gather_pixels, sample_channels,
                     sample_pixels)
from test_gpu_attention import CONFIGS

pytestmark = pytest.mark.gpu
dev = "cuda"
bf = torch.bfloat16
LAUNCHES = 12
S122 = (1, 2, 2)


def _assert_same_bits(runs, names, what):
    """runs: per launch a tuple of tensors.  Synchronises once, then every launch against
    launch 0."""
    torch.cuda.synchronize()
    bad = {n: [i for i, r in enumerate(runs) if not torch.equal(r[j], runs[0][j])]
           for j, n in enumerate(names)}
    bad = {n: v for n, v in bad.items() if v}
    assert not bad, f"{what}: launches that differ from launch 0: {bad}"


# ------------------------------------------------------------------ gathered conv GEMM
# (x shape, Co, kernel, stride): notation of test_gpu_conv_bounds.py (fwd sC = Ci, N = Co;
# bwd-data sC = Co, N = Ci; M pixels).  Tile selection of launch_igemm_dma: N <= 64, or N % 128
# != 0 and N % 64 == 0 -> 128 x 64; else cdiv(M, 128) * cdiv(N, 128) >= 512 -> 128 x 128;
# else 64 x 128.
CONV_CASES = [
    # config-2 Downsample: fwd N = 64 -> 128 x 64, 512 M tiles, 27 K steps.  bwd-data runs as the
    # unit-stride conv of the zero-dilated dY, which ops allocates at 16 x 128 x 128 (W % 16 ==
    # 0), so it takes halo_conv_kernel<true, 32>, not the gathered GEMM: its bits are pinned
    # here all the same.  wgrad: strided -> the generic conv_wgrad_kernel
    ((1, 64, 16, 128, 128), 64, 3, S122),
    # fwd N = 128, 128 * 1 < 512 tiles -> 64 x 128; bwd-data: dilated dY 16 x 64 x 64 ->
    # halo_conv_kernel<true, 64>
    ((1, 128, 16, 64, 64), 128, 3, S122),
    # W % 16 != 0 (no halo tile): fwd N = 256, 256 * 2 = 512 tiles -> 128 x 128; bwd-data
    # N = 64 -> 128 x 64 <TR>, sC = 256: 108 K steps
    ((1, 64, 4, 91, 90), 256, 3, 1),
    # dims = 2: kt = 1, not the halo tile; N = 64 -> 128 x 64 fwd and <TR>
    ((1, 64, 128, 128), 64, 3, 1),
    # 1x1 with K = 384 > 256 (skip conv on concatenated channels): pw_gemm rejects it -> gathered
    # GEMM, N = 256, 128 * 2 < 512 -> 64 x 128; bwd-data K = 256 -> pw_gemm_kernel<8>
    ((1, 384, 16, 32, 32), 256, 1, 1),
    # qkv: fwd is pw_gemm_kernel<8> (its bits are pinned too); bwd-data K = 768 > 256 -> gathered
    # GEMM <TR>, N = 256, 128 * 2 < 512 -> 64 x 128, 12 K steps
    ((1, 256, 16384), 768, 1, 1),
]


def _conv_inputs(case):
    shape, Co, k, stride = CONV_CASES[case]
    nd, (B, Ci) = len(shape) - 2, shape[:2]
    g = torch.Generator(device=dev).manual_seed(7000 + case)

    def cl(C, sp, fn=torch.rand):  # channels-last, logical [B, C, *sp]
        t = fn((B,) + tuple(sp) + (C,), generator=g, device=dev)
        return ((t * 2 - 1) if fn is torch.rand else t).bfloat16().movedim(-1, 1)

    x = cl(Ci, shape[2:])
    w = (torch.randn((Co, Ci) + (k,) * nd, generator=g, device=dev)
         / (Ci * k ** nd) ** 0.5).bfloat16().float()
    b = 0.1 * torch.randn(Co, generator=g, device=dev)
    s = (stride,) * nd if isinstance(stride, int) else stride[-nd:]
    out = tuple((shape[2 + a] + 2 * (k // 2) - k) // s[a] + 1 for a in range(nd))
    dy = cl(Co, out)
    return x, w, b, dy, s, k // 2


@pytest.mark.parametrize("case", range(len(CONV_CASES)))
def test_gathered_conv_gemm_same_bits_and_inside_the_bound(case):
    """fwd, bwd-data and the fixed-order weight gradient of ops.conv, 12 launches each.  The
    kernels each row launches (the tile named in CONV_CASES) were confirmed once with a kernel
    trace.  Launch 0 at >= 256 sampled pixels per tensor (sample_pixels: all corners, a pixel on
    each face, both ends of the first / middle / last 128-row M tile, every (h, w) parity for
    dx) and at 8 x 8 (co, ci) pairs of dw, all taps, against conv_ref64_at.  Largest error /
    bound measured on an MI355X over the rows: y 0.96, dx 0.95 (the final bf16 rounding), dw
    below 1e-3 (its worst-case fp32 term grows with the 16384 - 262144 pixels summed)."""
    from vdiff import ops
    shape, Co, k, stride = CONV_CASES[case]
    x, w, b, dy, s, pad = _conv_inputs(case)
    xd, wd = x.requires_grad_(True), w.requires_grad_(True)
    runs = []
    for _ in range(LAUNCHES):
        y = ops.conv(xd, wd, b, stride=s, padding=pad)
        dx, dw = torch.autograd.grad(y, (xd, wd), dy)
        runs.append((y.detach(), dx, dw))
    what = f"conv case {case} {CONV_CASES[case]}"
    _assert_same_bits(runs, ("y", "dx", "dw"), what)
    y, dx, dw = runs[0]
    assert y.dtype == bf and dx.dtype == bf and dw.dtype == torch.float32

    B = shape[0]
    y_pix = sample_pixels((B,) + tuple(y.shape[2:]), 256, 100 + case)
    x_pix = sample_pixels((B,) + tuple(shape[2:]), 256, 200 + case, parity=True)
    cos, cis = sample_channels(Co, 8, 300 + case), sample_channels(shape[1], 8, 400 + case)
    assert len(y_pix) >= 256 and len(x_pix) >= 256 and len(cos) >= 8 and len(cis) >= 8
    ref = conv_ref64_at(x.detach().float().cpu(), w.detach().cpu(), b.cpu(), dy.float().cpu(),
                        s, pad, y_pix, x_pix, cos, cis)
    got = {"y": gather_pixels(y, y_pix.to(dev)), "dx": gather_pixels(dx, x_pix.to(dev)),
           "dw": dw[cos][:, cis]}
    r = {n: assert_elementwise(got[n], *ref[n], n != "dw", what=f"{what} {n}")
         for n in ("y", "dx", "dw")}
    print(f"ring {what}: err/bound y {r['y']:.3f} dx {r['dx']:.3f} dw {r['dw']:.2e}")
    record_metric(test="ring_conv", case=case, **r)


# ViViT MLP: rows = 2 clips x 3137 tokens (ragged M: 6274 = 49 * 128 + 2); K = 768 / 3072 are the
# longest K rings in the product (12 and 48 ring steps of kIgBK = 64 channels: 24 and 96 MFMA K
# steps).  768 -> 3072: fwd 50 * 24 tiles -> 128 x 128, bwd-data N = 768, 50 * 6 < 512 -> 64 x
# 128 <TR>; 3072 -> 768 the other way round.
@pytest.mark.parametrize("cin,cout", [(768, 3072), (3072, 768)])
def test_vivit_linear_same_bits_and_inside_the_bound(cin, cout):
    """ops.linear with bias and residual (the gathered GEMM as a 1x1 conv: K > 256), fwd,
    bwd-data and weight gradient, 12 launches; launch 0 against the whole fp64 matmul."""
    from vdiff import ops
    rows = 2 * 3137
    g = torch.Generator(device=dev).manual_seed(cin)
    x = (torch.rand(2, 3137, cin, generator=g, device=dev) * 2 - 1).bfloat16()
    res = (torch.rand(2, 3137, cout, generator=g, device=dev) * 2 - 1).bfloat16()
    dy = (torch.rand(2, 3137, cout, generator=g, device=dev) * 2 - 1).bfloat16()
    w = (torch.randn(cout, cin, generator=g, device=dev) / cin ** 0.5).bfloat16().float()
    b = 0.1 * torch.randn(cout, generator=g, device=dev)
    xd, wd = x.requires_grad_(True), w.requires_grad_(True)
    runs = []
    for _ in range(LAUNCHES):
        y = ops.linear(xd, wd, b, residual=res)
        dx, dw = torch.autograd.grad(y, (xd, wd), dy)
        runs.append((y.detach(), dx, dw))
    what = f"linear {cin} -> {cout}"
    _assert_same_bits(runs, ("y", "dx", "dw"), what)
    y, dx, dw = (t.reshape(-1, t.shape[-1]) for t in runs[0])
    assert y.dtype == bf and dx.dtype == bf and dw.dtype == torch.float32

    x64 = x.detach().double().cpu().reshape(rows, cin)
    dy64 = dy.double().cpu().reshape(rows, cout)
    w64, b64 = w.detach().double().cpu(), b.double().cpu()
    r64 = res.double().cpu().reshape(rows, cout)
    r = {"y": assert_elementwise(y, x64 @ w64.T + b64 + r64,
                                 x64.abs() @ w64.abs().T + b64.abs() + r64.abs(), cin, True,
                                 what=what + " y"),
         "dx": assert_elementwise(dx, dy64 @ w64, dy64.abs() @ w64.abs(), cout, True,
                                  what=what + " dx"),
         "dw": assert_elementwise(dw, dy64.T @ x64, dy64.abs().T @ x64.abs(), rows, False,
                                  what=what + " dw")}
    print(f"ring {what}: err/bound y {r['y']:.3f} dx {r['dx']:.3f} dw {r['dw']:.2e}")
    record_metric(test="ring_linear", cin=cin, cout=cout, **r)


# ------------------------------------------------------------------ wgrad_dma_kernel
# (x shape, Co, vd_conv_set_wgrad mode or None for the default selection); 3x3x3, stride 1
WGRAD_CASES = [
    # kw strip, wc = 32, Ho % (64 / wc) = 33 % 2 != 0 -> the default selection takes
    # wgrad_dma_kernel<96, 64, 2, false, false>
    ((1, 64, 8, 33, 32), 64, None),
    # mode 0: the round-5 kernel instead of the stage-unrolled strip kernel, at train size
    ((1, 64, 16, 128, 128), 64, 0),     # one 64-pixel row per step
    ((1, 256, 16, 32, 32), 256, 0),     # two rows per step
]


@pytest.mark.parametrize("case", range(len(WGRAD_CASES)))
def test_wgrad_dma_kernel_same_bits_and_inside_the_bound(case):
    """The fixed-order weight gradient on wgrad_dma_kernel (confirmed once with a kernel trace),
    12 launches; launch 0 at 8 x 8 (co, ci) pairs, all 27 taps, against conv_ref64_at."""
    from vdiff import _lib, ops
    shape, Co, mode = WGRAD_CASES[case]
    B, Ci = shape[:2]
    g = torch.Generator(device=dev).manual_seed(7100 + case)
    x = (torch.rand((B,) + shape[2:] + (Ci,), generator=g, device=dev) * 2 - 1) \
        .bfloat16().movedim(-1, 1)
    dy = (torch.rand((B,) + shape[2:] + (Co,), generator=g, device=dev) * 2 - 1) \
        .bfloat16().movedim(-1, 1)
    w = (torch.randn(Co, Ci, 3, 3, 3, generator=g, device=dev) / (27 * Ci) ** 0.5) \
        .bfloat16().float().requires_grad_(True)
    lib = _lib.lib()
    prev = lib.vd_conv_set_wgrad(mode) if mode is not None else None
    try:
        y = ops.conv(x, w, None, padding=1)
        runs = [torch.autograd.grad(y, (w,), dy, retain_graph=True) for _ in range(LAUNCHES)]
        what = f"wgrad case {case} {WGRAD_CASES[case]}"
        _assert_same_bits(runs, ("dw",), what)
    finally:
        if prev is not None:
            lib.vd_conv_set_wgrad(prev)
    dw, = runs[0]
    cos, cis = sample_channels(Co, 8, 500 + case), sample_channels(Ci, 8, 600 + case)
    pix = sample_pixels((B,) + shape[2:], 1, 0)[:1]  # y / dx are not under test here
    ref = conv_ref64_at(x.float().cpu(), w.detach().cpu(), None, dy.float().cpu(), 1, 1, pix, pix,
                        cos, cis)
    r = assert_elementwise(dw[cos][:, cis], *ref["dw"], False, what=what + " dw")
    print(f"ring {what}: err/bound dw {r:.2e}")
    record_metric(test="ring_wgrad", case=case, dw=r)


# ------------------------------------------------------------------ compiled attention rings
@functools.lru_cache(maxsize=None)
def _self_host(case, legacy):
    """Inputs and fp64 reference of a case: computed once, shared by its configs, not modified."""
    B, C, heads, T, HW, mode, seed, amp = case
    qkv, g, host = A.self_inputs(B, C, T, HW, mode, seed, amp, heads, legacy)
    host.assert_cap()
    return qkv, g, host


def _self_params():
    out = []
    for c in A.RING_SELF_CASES:
        if c[2] == 1:
            out += [pytest.param(c, True, cfg, id=f"{A.case_id(c)}-{cfg}")
                    for cfg in CONFIGS if cfg != "asm"]
        else:
            out += [pytest.param(c, legacy, "auto", id=f"{A.case_id(c)}-legacy{int(legacy)}")
                    for legacy in (True, False)]
    return out


@pytest.mark.parametrize("case,legacy,cfg", _self_params())
def test_attention_rings_same_bits_and_inside_the_row_limits(case, legacy, cfg):
    """ops.attention (joint) forward (O, lse) and backward (dq, dk, dv), 12 launches, under
    every compiled kernel shape; launch 0 through Host.judge (4 x the CPU emulation per row, the
    lse bound), unchanged.  Measured on an MI355X: kernel / emulation at most 1.25 (O under
    "base" at C = 64, N = 4096: 5.8e-3 against 4.7e-3), lse at most 0.17 of its bound."""
    from vdiff import ops
    B, C, heads, T, HW, mode, seed, amp = case
    qkv, g, host = _self_host(case, legacy)
    qd = ops.to_cl(qkv.to(dev)).requires_grad_(True)
    gd = ops.to_cl(g.to(dev))
    runs = []
    with ops.attention_config(cfg):
        for _ in range(LAUNCHES):
            out = ops.attention(qd, heads=heads, mode=mode, spatial=(T, HW, 1), legacy=legacy)
            lse, = out.grad_fn.saved_tensors[2:]  # the one launch of joint mode
            dqkv, = torch.autograd.grad(out, (qd,), gd)
            runs.append((out.detach(), lse, dqkv))
    what = f"attention ring C={C} N={T * HW} heads={heads} legacy={legacy} {cfg}"
    _assert_same_bits(runs, ("o", "lse", "dqkv"), what)
    out, lse, dqkv = runs[0]
    got = dict(zip(("dq", "dk", "dv"), A.sequences(dqkv.float().cpu(), C, T, HW, mode, heads, legacy)))
    got["o"], = A.sequences(out.float().cpu(), C, T, HW, mode, heads, legacy)
    host.judge(got, lse, what, record_metric, test="ring_attention", C=C, N=T * HW, heads=heads,
               legacy=legacy, cfg=cfg)


@pytest.mark.parametrize("case", A.RING_CROSS_CASES, ids=A.case_id)
def test_cross_attention_ring_same_bits_and_inside_the_row_limits(case):
    """Clip-level cross-attention with 640 keys (10 key tiles through tile_loop), 12 launches of
    forward (O, lse) and backward (dq, dk | dv); launch 0 through Host.judge (measured: O 6.9e-3
    against the emulation's 5.2e-3, the other outputs at the emulation's value)."""
    from vdiff import ops
    B, C, heads, T, HW, L, per_frame, seed, amp = case
    q, kv, g, host = A.cross_inputs(*case)
    host.assert_cap()
    qd = ops.to_cl(q.to(dev)).requires_grad_(True)
    kvd = kv.to(dev).requires_grad_(True)
    gd = ops.to_cl(g.to(dev))
    runs = []
    for _ in range(LAUNCHES):
        out = ops.cross_attention(qd, kvd, heads, T, per_frame)
        lse = out.grad_fn.saved_tensors[3]
        dq, dkv = torch.autograd.grad(out, (qd, kvd), gd)
        runs.append((out.detach(), lse, dq, dkv))
    what = f"cross-attention ring {case}"
    _assert_same_bits(runs, ("o", "lse", "dq", "dkv"), what)
    out, lse, dq, dkv = runs[0]
    got = dict(o=A.cross_q_sequences(out.float().cpu(), heads, T, per_frame),
               dq=A.cross_q_sequences(dq.float().cpu(), heads, T, per_frame))
    got["dk"], got["dv"] = A.cross_kv_sequences(dkv.float().cpu(), heads, T, per_frame)
    host.judge(got, lse, what, record_metric, test="ring_cross_attention", C=C, heads=heads, T=T,
               HW=HW, L=L)
