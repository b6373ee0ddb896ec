"""Clip quality metrics: per-frame PSNR and SSIM of a generated clip against a ground-truth
clip, over the whole frame or over a region (the generated region of masked sampling), computed
on the GPU by vd_clip_metrics (csrc/metrics.hip; the definition is in include/vdiff.h and DESIGN
section 4.3).

    m = clip_metrics(sample, truth)                                  # whole frame
    m = clip_metrics(sample, truth, weight=region_weight(keep))      # the generated region
    m.psnr, m.ssim            # [B, T] device tensors
    m.mean()                  # {"mse", "psnr", "ssim", "frames"}: floats over the frames that count

    python -m vdiff.metrics A.npy B.npy [--weight W.npy] [--range LO HI] [--json OUT]

Values are mapped to [0, 1] from `value_range` (default (-1, 1), what the samplers return) and
clamped; PSNR = -10 log10(mse), +inf for identical frames.  There is no CPU path: the clips must
be on the GPU.
"""
from __future__ import annotations

import json
import math

import torch

from . import ops


class ClipMetrics:
    """mse, psnr, ssim: fp32 [B, T] on the device; wsum_px, wsum_valid: fp32 [T], the weight over a
    frame's pixels (mse, psnr) and over the centres of its valid window positions (ssim).  A frame
    whose weight sum is 0 holds NaN."""

    def __init__(self, mse, ssim, wsum_px, wsum_valid):
        self.mse, self.ssim, self.wsum_px, self.wsum_valid = mse, ssim, wsum_px, wsum_valid

    @property
    def psnr(self):
        return -10.0 * torch.log10(self.mse)  # mse = 0: +inf

    def mean(self):
        """Averages over the batch and the frames with a positive weight sum (synchronises):
        {"mse", "psnr", "ssim"} as floats, NaN when no frame counts; "psnr" is the mean of the
        per-frame values (inf as soon as one frame is identical); "frames": how many frames
        counted for mse / psnr and for ssim."""
        out, frames = {}, {}
        for name, val, ws in (("mse", self.mse, self.wsum_px), ("psnr", self.psnr, self.wsum_px),
                              ("ssim", self.ssim, self.wsum_valid)):
            on = (ws > 0).cpu()
            v = val.detach().double().cpu()[:, on]
            out[name] = float(v.mean()) if v.numel() else math.nan
            frames[name] = int(on.sum())
        out["frames"] = {"mse": frames["mse"], "ssim": frames["ssim"]}
        return out

    def to_json(self):
        """Per-frame lists [B][T], the weight sums [T] and the means, for json.dump: JSON has no
        NaN and no infinity, so a NaN is written as null and an infinite PSNR as "inf"."""
        def rows(t):
            return [[_num(v) for v in r] for r in t.detach().double().cpu().tolist()]
        m = self.mean()
        return {"mse": rows(self.mse), "psnr": rows(self.psnr), "ssim": rows(self.ssim),
                "wsum_px": self.wsum_px.cpu().tolist(),
                "wsum_valid": self.wsum_valid.cpu().tolist(),
                "mean": {k: (_num(v) if k != "frames" else v) for k, v in m.items()}}


def _num(v):
    if math.isnan(v):
        return None
    if math.isinf(v):
        return "inf" if v > 0 else "-inf"
    return v


def clip_metrics(x, y, weight=None, value_range=(-1, 1)):
    """ClipMetrics of clips x, y [B, C, T, H, W] (or [B, C, H, W], T = 1), fp32 or bf16 on the
    GPU; weight: [T, H, W] ([H, W]) or anything region_weight accepts, >= 0."""
    if weight is not None:
        weight = _as_weight(weight, x)
    r = ops.clip_metrics(x, y, weight, value_range)
    return ClipMetrics(r.mse, r.ssim, r.wsum_px, r.wsum_valid)


def psnr(x, y, weight=None, value_range=(-1, 1)):
    """Per-frame PSNR [B, T] in dB."""
    return clip_metrics(x, y, weight, value_range).psnr


def ssim(x, y, weight=None, value_range=(-1, 1)):
    """Per-frame SSIM [B, T]."""
    return clip_metrics(x, y, weight, value_range).ssim


def _frames_pixels(w):
    """A (1, 1, T, H, W) / (1, 1, H, W) mask (schedulers.keep_mask) or a [T, H, W] / [H, W] one
    without its two leading axes."""
    if w.dim() in (4, 5) and tuple(w.shape[:2]) == (1, 1):
        return w[0, 0]
    if w.dim() in (2, 3):
        return w
    raise ValueError(f"mask {tuple(w.shape)}: (1, 1, [T,] H, W) or ([T,] H, W)")


def region_weight(keep):
    """The weight of the GENERATED region from the `keep` mask of masked sampling
    (schedulers.keep_mask: (1, 1, T, H, W) or (1, 1, H, W); 1 = known pixel): 1 - keep as fp32
    [T, H, W] resp. [H, W], the feather included."""
    k = _frames_pixels(torch.as_tensor(keep)).float()
    return (1.0 - k.clamp(0.0, 1.0)).contiguous()


def _as_weight(weight, like):
    w = _frames_pixels(torch.as_tensor(weight)).float()
    return w.to(like.device).contiguous()


def main(argv=None):
    import argparse

    import numpy as np
    ap = argparse.ArgumentParser(
        prog="python -m vdiff.metrics",
        description="PSNR and SSIM of two saved clips (C, [T,] H, W), frame by frame")
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--weight", default=None, metavar="W.npy",
                    help="region weight over the frames and pixels ([T,] H, W), >= 0")
    ap.add_argument("--range", type=float, nargs=2, default=(-1.0, 1.0), metavar=("LO", "HI"),
                    help="the values' range (default -1 1; saved frames: 0 1)")
    ap.add_argument("--json", default=None, metavar="OUT")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("vdiff.metrics runs on the GPU kernels only")
    a, b = (np.load(p, allow_pickle=False) for p in (args.a, args.b))
    if a.shape != b.shape or a.ndim not in (3, 4) or not (
            np.issubdtype(a.dtype, np.floating) and np.issubdtype(b.dtype, np.floating)):
        raise SystemExit(f"vdiff.metrics: two float clips (C, [T,] H, W) of one shape, got "
                         f"{a.dtype} {a.shape} and {b.dtype} {b.shape}")
    w = None
    if args.weight is not None:
        w = np.load(args.weight, allow_pickle=False)
        if tuple(w.shape) != tuple(a.shape[1:]) or not np.issubdtype(w.dtype, np.floating):
            raise SystemExit(f"vdiff.metrics: --weight holds {w.dtype} {w.shape}; the clips' "
                             f"frames and pixels are float {a.shape[1:]}")
        w = torch.from_numpy(w).float()
    dev = torch.device("cuda")
    x, y = (torch.from_numpy(v).float()[None].contiguous().to(dev) for v in (a, b))
    try:
        m = clip_metrics(x, y, w, tuple(args.range))
    except ValueError as e:
        raise SystemExit(f"vdiff.metrics: {e}") from None
    print_report(m)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(m.to_json(), f)
    return m


def print_report(m, title=None):
    """One line per frame and the means."""
    if title:
        print(title)
    mse, ps, ss = (t.detach().double().cpu() for t in (m.mse, m.psnr, m.ssim))
    for b in range(mse.shape[0]):
        for t in range(mse.shape[1]):
            print(f"clip {b} frame {t}: mse {float(mse[b, t]):.9g} psnr {float(ps[b, t]):.6f} dB "
                  f"ssim {float(ss[b, t]):.9g}")
    mean = m.mean()
    print(f"mean over {mean['frames']['mse']} / {mean['frames']['ssim']} frames: mse "
          f"{mean['mse']:.9g} psnr {mean['psnr']:.6f} dB ssim {mean['ssim']:.9g}")


if __name__ == "__main__":
    main()
