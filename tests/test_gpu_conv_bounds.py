"""Element-wise error bounds (tests/_bounds.py) on every bf16 conv dispatch path: forward with
bias, bwd-data and the deterministic bwd-weight through ops.conv, against an fp64 conv of the
same bf16-rounded operands.  The whole-tensor rel-L2 of test_gpu_conv.py lets one wrong pixel,
tap or channel tail through (tests/test_bounds_host.py); this bound does not.

Each row of CASES names the branch of conv.hip it is meant to take and the condition that
selects it.  Notation: fwd has sC = Ci, N = Co, dW = Wo; bwd-data has sC = Co (padded to 8),
N = Ci, dW = Wi; M = B * T * H * W pixels of the GEMM's output.  A strided bf16 bwd-data runs as
the unit-stride transposed gather of a zero-dilated dY (ops.ConvFn.backward).
"""
import os
import subprocess
import sys

import pytest
import torch

from conftest import record_metric  # first: puts the repository on sys.path in the child process

from oracle.fixtures import seeded

from _bounds import assert_elementwise, bf16r, conv_bwd_ref64, conv_fwd_ref64

pytestmark = pytest.mark.gpu
dev = "cuda"

S122 = (1, 2, 2)
CASES = [
    # (x shape, Co, kernel, stride, padding, fused epilogue)
    # ---- halo tile (launch_gemm: halo_ok = 3x3x3, stride 1, pad 1, W % 16 == 0); odd T, H % 4
    # != 0, Co = 80 (ragged 64-wide column tile), B = 2
    # fwd + bwd-data halo_ks = 32: dW = 48 > 32 && sC = 96 / 80 < 128; wgrad: Wo = 48 neither
    # divides nor is divided by 64 -> generic conv_wgrad_kernel
    ((2, 96, 3, 5, 48), 80, 3, 1, 1, False),
    # fwd + bwd-data halo_ks = 64 by dW = 32 <= 32 (sC = 96: a ragged second 64-channel step);
    # wgrad: strip, wc = 32, Ho % (64 / wc) = 5 % 2 != 0 -> !v2 -> wgrad_dma_kernel<.., false>
    ((2, 96, 3, 5, 32), 80, 3, 1, 1, False),
    # fwd halo_ks = 64 by sC = 128 >= 128 at dW = 48; bwd-data halo_ks = 32 (sC = 80), N = 128
    ((2, 128, 3, 5, 48), 80, 3, 1, 1, False),
    # halo (ks = 64, dW = 16) with bias + chan_add + residual; wgrad: strip, wc = 16,
    # Ho % 4 != 0 -> wgrad_dma_kernel, rows = 4 * 18 = 72 <= 96
    ((2, 64, 3, 6, 16), 80, 3, 1, 1, True),
    # ---- gathered LDS-DMA GEMM (launch_igemm_dma), tile by N and M
    # 3x3x3 with W % 16 != 0; N = 64 <= 64 -> 128 x 64 (fwd and bwd-data); wgrad generic
    ((1, 64, 2, 9, 9), 64, 3, 1, 1, False),
    # N = 192: N % 128 != 0 && N % 64 == 0 -> 128 x 64, three column tiles; bwd-data N = 64
    ((1, 64, 2, 7, 9), 192, 3, 1, 1, False),
    # stride (1,2,2); fwd N = 256, cdiv(108,128) * 2 < 512 -> 64 x 128; bwd-data: dilated dY,
    # sT/sH/sW = 3/11/11 (W % 16 != 0), N = 128 -> 64 x 128; wgrad: strided -> generic
    ((1, 128, 3, 11, 11), 256, 3, S122, 1, False),
    # 2-D 3x3 (kt = 1: not halo_ok) at W % 16 == 0; N = 64 -> 128 x 64; wgrad: strip with
    # kt = 1, wc = 32, Ho % 2 == 0 -> v2 -> wgrad_strip_kernel<96, 64, 2, 0>
    ((2, 64, 8, 32), 64, 3, 1, 1, False),
    # 128 x 128: N = 256, cdiv(32760,128) * cdiv(256,128) = 512 >= 512 on a 3x3x3 with
    # W = 90; bwd-data: sC = 256, N = 16 <= 64 -> 128 x 64; wgrad generic, 19 pixel splits
    ((1, 16, 4, 91, 90), 256, 3, 1, 1, False),
    # DMA GEMM (64 x 128: N = 128, N % 128 == 0, few tiles) with bias + chan_add + residual;
    # bwd-data N = 64 -> 128 x 64
    ((2, 64, 2, 7, 9), 128, 3, 1, 1, True),
    # ---- streaming 1x1 (pw_gemm_launch: K % 32 == 0, K <= 256, N % 16 == 0):
    # pw_gemm_kernel<K / 32> for every K, M = 2 * 70 = 140 (% 16 != 0, 9 tiles over 3
    # workgroups), N = 80 (a 16-channel tail of the second 64-channel chunk).  bwd-data: K = 80,
    # K % 32 != 0 -> the 1x1 falls back onto launch_igemm_dma (TR: the general tiles; N = K <=
    # 64 or % 64 == 0 but not % 128 -> 128 x 64, N = 128 / 256 -> 64 x 128, else 64 x 128).
    # wgrad: `one` && v2 -> the 1x1 form wgrad_strip_kernel<64, 64, 4, 2, false>
    ((2, 32, 2, 5, 7), 80, 1, 1, 0, False),
    ((2, 64, 2, 5, 7), 80, 1, 1, 0, False),
    ((2, 96, 2, 5, 7), 80, 1, 1, 0, False),
    ((2, 128, 2, 5, 7), 80, 1, 1, 0, False),
    ((2, 160, 2, 5, 7), 80, 1, 1, 0, False),
    ((2, 192, 2, 5, 7), 80, 1, 1, 0, False),
    ((2, 224, 2, 5, 7), 80, 1, 1, 0, False),
    ((2, 256, 2, 5, 7), 80, 1, 1, 0, False),
    # bwd-data on the streaming kernel too: fwd K = 96, N = 160; bwd-data K = 160 (KS = 5),
    # N = 96
    ((2, 96, 1, 5, 7), 160, 1, 1, 0, False),
    # persistent loop: K = 256, N = 768 -> NS = 64, 12 slices, cap = 1024 / 12 = 85 -> 256
    # workgroups; tiles = cdiv(18437,16) = 1153, cdiv(1153,4) = 289 > 256 and 1153 wave tiles
    # over 1024 waves: unequal tile counts, prefetch past the end.  bwd-data: K = 768 > 256 ->
    # launch_igemm_dma, N = 256, 145 * 2 < 512 -> 64 x 128
    ((1, 256, 18437), 768, 1, 1, 0, False),
    # streaming 1x1 (KS = 2) with bias + chan_add + residual, M = 210 (% 16 != 0), three
    # 64-channel chunks; bwd-data K = 192, N = 64 -> pw_gemm_kernel<6>
    ((2, 64, 3, 5, 7), 192, 1, 1, 0, True),
    # ---- 1x1 that pw_gemm_launch rejects -> launch_igemm_dma
    # N = 40, N % 16 != 0; fwd sC = 64 <= kIgBK -> conv_1x1_variant 3: 64 x 64 tiles; bwd-data
    # K = 40, N = 64 -> 128 x 64
    ((1, 64, 1, 3, 7), 40, 1, 1, 0, False),
    # K = 72, K % 32 != 0 (sC > kIgBK: general tiles, N = 48 <= 64 -> 128 x 64); bwd-data
    # K = 48, N = 72 -> 64 x 128 with a ragged column tile
    ((1, 72, 2, 3, 7), 48, 1, 1, 0, False),
    # ---- weight-gradient kernels (wgrad_run), on top of the rows above
    # strip, wc = 64 (Wo % 64 == 0) -> v2 -> wgrad_strip_kernel<96, 64, 2, 1>: one 64-pixel
    # row per step; Co = 128 but the grid is far under w3_fill128 -> cot = 64.  fwd halo
    # ks = 32 (dW = 64, sC = 64), bwd-data halo ks = 64 (sC = 128)
    ((1, 64, 2, 3, 64), 128, 3, 1, 1, False),
    # strip, wc = 32, Ho % 2 == 0 -> wgrad_strip_kernel<96, 64, 2, 0>, 3x3x3, two clips
    ((2, 64, 3, 4, 32), 64, 3, 1, 1, False),
    # strip, wc = 128 > 64 -> two 64-pixel steps per row, Ci = 96 (ragged second ci tile),
    # Co = 80 -> wgrad_strip_kernel<96, 64, 2, 1>
    ((1, 96, 2, 3, 128), 80, 3, 1, 1, False),
]
# (wgrad_strip_kernel's 128-channel tiles need cdiv(Co,128) * cdiv(Ci,64) * 9 * cdiv(M,2048)
# >= 461 workgroups, > 40 GFLOP: test_gpu_conv.py::test_conv_wgrad_round4_split_rule holds them
# to 1e-5 of the fp32 kernel at full size.  wgrad_dma_kernel's plane mode and wgrad_bf16_kernel
# are selected by environment variables read once per process: test_env_selected_kernels.)


def _inputs(case):
    shape, Co, k, stride, pad, epi = CASES[case]
    nd = len(shape) - 2
    Ci = shape[1]
    x = bf16r(seeded(shape, 1000 + case))
    w = bf16r(seeded((Co, Ci) + (k,) * nd, 2000 + case) / (Ci * k ** nd) ** 0.5)
    b = 0.1 * seeded((Co,), 3000 + case)
    return x, w, b


def _check_case(case, tag=""):
    """Runs case `case` through ops.conv and checks y, dx, dw; returns the three largest
    error / bound ratios."""
    from vdiff import ops
    shape, Co, k, stride, pad, epi = CASES[case]
    x, w, b = _inputs(case)
    ca = res = None
    ref, mag, n = conv_fwd_ref64(x, w, b, stride, pad)
    if epi:
        ca = seeded((shape[0], Co), 4000 + case)
        res = bf16r(seeded(tuple(ref.shape), 5000 + case))
        ref, mag, n = conv_fwd_ref64(x, w, b, stride, pad, ca, res)
    dy = bf16r(seeded(tuple(ref.shape), 6000 + case))
    dx, dxm, n_dx, dw, dwm, n_dw = conv_bwd_ref64(x, w, dy, stride, pad)

    bf = torch.bfloat16
    xd = ops.to_cl(x.to(dev, bf)).requires_grad_(True)
    wd = w.to(dev).requires_grad_(True)
    y = ops.conv(xd, wd, b.to(dev), stride=stride, padding=pad,
                 chan_add=None if ca is None else ca.to(dev),
                 residual=None if res is None else ops.to_cl(res.to(dev, bf)))
    assert y.dtype == bf and xd.dtype == bf
    y.backward(ops.to_cl(dy.to(dev, bf)))
    torch.cuda.synchronize()
    assert wd.grad.dtype == torch.float32
    what = f"{tag}case {case} {CASES[case]}"
    r = (assert_elementwise(y, ref, mag, n, True, what=what + " y"),
         assert_elementwise(xd.grad, dx, dxm, n_dx, True, what=what + " dx"),
         assert_elementwise(wd.grad, dw, dwm, n_dw, False, what=what + " dw"))
    print(f"conv bounds {what}: err/bound y {r[0]:.3f} dx {r[1]:.3f} dw {r[2]:.3f}")
    record_metric(test="conv_bounds", tag=tag, case=case, y=r[0], dx=r[1], dw=r[2])
    return r


@pytest.mark.parametrize("case", range(len(CASES)))
def test_conv_elementwise_bounds(case):
    """y (bf16, n = taps * Ci products + bias, chan_add, residual), dx (bf16, n = taps * Co)
    and the fixed-order dw (fp32: no relative term, n = B * To * Ho * Wo) inside the bound of
    tests/_bounds.py at every element.  Largest error / bound measured on an MI355X over the
    rows: y 0.98, dx 0.99 (the final bf16 rounding: the 1x1 rows, whose fp32 term is smallest),
    dw 0.02.  The kernels each row launches were confirmed once with a kernel trace."""
    _check_case(case)


# halo rows of CASES on the other halo kernels (vd_conv_set_halo): 0 = the gathered tiles for the
# same shapes, 3 = 8-wave workgroups, 5 = forward without early halo pieces
@pytest.mark.parametrize("mode", [0, 3, 5])
@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_conv_elementwise_bounds_halo_modes(case, mode):
    from vdiff import ops
    with ops.conv_halo(mode):
        _check_case(case, tag=f"halo mode {mode} ")


# Kernels that only an environment variable read once per process selects; a child process each.
ENV_CASES = [
    # VDIFF_CONV_WPLANE=1: `plane` = strip && Wo % 64 == 0 -> wgrad_dma_kernel<224, 64, 2,
    # false, true> (nine-tap planes); rows 23 (wc = 64) and 25 (two steps per row, ragged Ci/Co)
    ({"VDIFF_CONV_WPLANE": "1"}, [23, 25]),
    # VDIFF_CONV_DMA=0: `dma` false -> strip -> wgrad_bf16_kernel<96> (rows 1, 23, 24); fwd and
    # bwd-data on the register-staged igemm_bf16_kernel (launch_igemm)
    ({"VDIFF_CONV_DMA": "0"}, [1, 23, 24]),
]


@pytest.mark.parametrize("env,cases", ENV_CASES, ids=["wplane", "nodma"])
def test_env_selected_kernels(env, cases):
    """The same element-wise check in a child process that starts with the variable set."""
    e = dict(os.environ, **env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(c) for c in cases],
                       env=e, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("conv bounds") == len(cases)


if __name__ == "__main__":
    for c in sys.argv[1:]:
        _check_case(int(c), tag="env ")
