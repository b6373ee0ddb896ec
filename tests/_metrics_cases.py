"""Inputs and references of the clip-metric tests (vd_clip_metrics: per-frame MSE and SSIM).

oracle64 is the definition of include/vdiff.h in float64 on the CPU, written independently of the
kernel's plan: the direct 2-D 11 x 11 window (F.conv2d), E[u^2] - E[u]^2 without a pivot, the
weight at the window's centre.  naive32 is the obvious fp32 evaluation (the same expressions in
float32): its error against the oracle is the yardstick of the map tolerance,

    tol = 2 * max|naive32 map - oracle map| + 2 * (22 + 2) * 2^-24,

the maximum taken over the map of the same input.  The factor 2 covers a different summation
order (separable against 2-D); the floor is the any-order fp32 bound (tests/_bounds.py) of the 22
terms of the separable sum at unit magnitude.  A kernel that pivots its moments sits far below
the naive error where frames are smooth or flat.
"""
import math

import torch
import torch.nn.functional as F

from _bounds import U_FP32, bf16r

WIN = 11
C1, C2 = 0.01 ** 2, 0.03 ** 2
MAP_FLOOR = 2.0 * (2 * WIN + 2) * U_FP32

# (shape, dtypes): ragged tiles on both axes with unaligned rows; a 4-D input whose plane has
# one map position and is all border for the MSE; one map row / one map column over many tiles
SHAPES = [((2, 3, 3, 45, 77), ("fp32", "bf16")),
          ((1, 3, 11, 11), ("fp32",)),
          ((1, 1, 2, 11, 140), ("fp32",)),
          ((1, 1, 2, 140, 11), ("fp32",))]
CONTENTS = ("noise", "near", "smooth", "flat_same", "flat_apart", "overshoot")


def window1d():
    """The 11 taps: normalised in double, rounded to fp32 (returned as float64)."""
    d = torch.arange(WIN, dtype=torch.float64) - WIN // 2
    g = torch.exp(-d * d / (2.0 * 1.5 ** 2))
    return (g / g.sum()).float().double()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def pair(shape, content, seed=0):
    """(x, y) fp32 CPU clips of `shape` in [-1, 1] (overshoot: x reaches +-1.5)."""
    g = _gen(1000 * seed + sum(shape) + 17 * CONTENTS.index(content))
    H, W = shape[-2:]
    if content == "noise":
        return (torch.rand(shape, generator=g) * 2 - 1, torch.rand(shape, generator=g) * 2 - 1)
    if content == "near":
        x = torch.rand(shape, generator=g) * 2 - 1
        return x, x + 0.1 * torch.randn(shape, generator=g)
    if content == "smooth":
        yy = torch.linspace(0, 1, H).view(H, 1)
        xx = torch.linspace(0, 1, W).view(1, W)
        f = (0.6 * torch.sin(3 * yy) + 0.4 * xx).expand(shape).contiguous()
        return f, f + 0.02
    if content == "flat_same":
        return torch.full(shape, 0.3), torch.full(shape, 0.3)
    if content == "flat_apart":
        return torch.full(shape, 0.7), torch.full(shape, -0.9)
    if content == "overshoot":
        x = torch.rand(shape, generator=g) * 2 - 1
        y = torch.rand(shape, generator=g) * 2 - 1
        flat = x.view(-1)
        idx = torch.randperm(flat.numel(), generator=g)[:max(4, flat.numel() // 7)]
        flat[idx[0::2]] = 1.5
        flat[idx[1::2]] = -1.5
        return x, y
    raise KeyError(content)


def rounded(t, dtype):
    """What the kernel reads: t in fp32, bf16-rounded for dtype 'bf16'."""
    return bf16r(t) if dtype == "bf16" else t.float()


def _five_d(t):
    return t.unsqueeze(2) if t.dim() == 4 else t


def _moments(u, v, w2):
    """Window-weighted sums at the valid positions of planes u, v [N, 1, H, W]."""
    k = w2.view(1, 1, WIN, WIN)
    return (F.conv2d(u, k), F.conv2d(v, k), F.conv2d(u * u, k), F.conv2d(v * v, k),
            F.conv2d(u * v, k))


def _ssim_map(x, y, lo, hi, dtype):
    """[B, C, T, H - 10, W - 10] in `dtype` (float64: the oracle, float32: the naive one)."""
    x, y = _five_d(x), _five_d(y)
    B, C, T, H, W = x.shape
    u = ((x.to(dtype) - lo) / (hi - lo)).clamp(0, 1).reshape(-1, 1, H, W)
    v = ((y.to(dtype) - lo) / (hi - lo)).clamp(0, 1).reshape(-1, 1, H, W)
    g = window1d()
    w2 = torch.outer(g, g).to(dtype)
    mx, my, exx, eyy, exy = _moments(u, v, w2)
    vx, vy, cxy = exx - mx * mx, eyy - my * my, exy - mx * my
    s = ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return s.view(B, C, T, H - WIN + 1, W - WIN + 1)


def oracle64(x, y, weight=None, value_range=(-1.0, 1.0)):
    """dict of float64 CPU tensors: map [B, C, T, MH, MW], mse, ssim [B, T], ssim_mag [B, T] (the
    weighted mean of |s|), wsum_px, wsum_valid [T].  x, y: fp32 CPU clips as the kernel reads
    them; weight [T, H, W] or None."""
    lo, hi = (float(v) for v in value_range)
    x5, y5 = _five_d(x), _five_d(y)
    B, C, T, H, W = x5.shape
    w = torch.ones(T, H, W, dtype=torch.float64) if weight is None else \
        weight.double().view(T, H, W)
    u = ((x5.double() - lo) / (hi - lo)).clamp(0, 1)
    v = ((y5.double() - lo) / (hi - lo)).clamp(0, 1)
    wpx = w.sum(dim=(1, 2))
    mse = ((u - v) ** 2 * w.view(1, 1, T, H, W)).sum(dim=(1, 3, 4)) / (C * wpx.view(1, T))
    smap = _ssim_map(x, y, lo, hi, torch.float64)
    wc = w[:, WIN // 2:H - WIN // 2, WIN // 2:W - WIN // 2]
    wv = wc.sum(dim=(1, 2))
    ssim = (smap * wc.view(1, 1, T, *wc.shape[1:])).sum(dim=(1, 3, 4)) / (C * wv.view(1, T))
    mag = (smap.abs() * wc.view(1, 1, T, *wc.shape[1:])).sum(dim=(1, 3, 4)) / (C * wv.view(1, T))
    return dict(map=smap, mse=mse, ssim=ssim, ssim_mag=mag, wsum_px=wpx, wsum_valid=wv)


def naive32_map(x, y, value_range=(-1.0, 1.0)):
    """The plain fp32 evaluation of the map (2-D window, E[u^2] - E[u]^2), as float64."""
    lo, hi = (float(v) for v in value_range)
    return _ssim_map(x, y, lo, hi, torch.float32).double()


def map_tolerance(x, y, ref_map, value_range=(-1.0, 1.0)):
    """(tol, naive error): see the module docstring."""
    naive = float((naive32_map(x, y, value_range) - ref_map).abs().max())
    return 2.0 * naive + MAP_FLOOR, naive


_CACHE = {}


def case(shape, dtype, content):
    """(x, y, ref, tol, naive_err) of one seeded input, computed once and shared: x, y the fp32
    CPU clips as the kernel reads them (bf16-rounded for dtype 'bf16'), ref = oracle64 on them."""
    key = (tuple(shape), dtype, content)
    if key not in _CACHE:
        x, y = (rounded(t, dtype) for t in pair(shape, content))
        ref = oracle64(x, y)
        tol, naive = map_tolerance(x, y, ref["map"])
        _CACHE[key] = (x, y, ref, tol, naive)
    return _CACHE[key]


def mean_bound(ref, tol, n_pos):
    """Bound of ssim[b, t]: the map tolerance plus the any-order fp32 term of the mean's n_pos
    terms at the magnitude of the weighted mean of |s|."""
    return tol + 2.0 * (n_pos + 2) * U_FP32 * ref["ssim_mag"]


def hand_mse_pair():
    """A 1 x 1 x 11 x 11 pair whose MSE is known by hand: x = 0 everywhere but one pixel at 1, y
    = 0: u differs by 0.5 at one of 121 pixels, mse = 0.25 / 121."""
    x = torch.zeros(1, 1, 11, 11)
    x[0, 0, 3, 7] = 1.0
    return x, torch.zeros(1, 1, 11, 11), 0.25 / 121.0


def flat_ssim(a, b):
    """SSIM of two constant planes a, b (already mapped to [0, 1]) for a window that sums to 1."""
    return (2 * a * b + C1) / (a * a + b * b + C1)


assert math.isclose(float(window1d().sum()), 1.0, abs_tol=1e-6)
