"""Clip metrics without a GPU: the C-ABI names, the float64 oracle of tests/_metrics_cases.py
against closed forms, the CPU-tensor refusal, test.py's --score flags and region_weight."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import DROPIN, ROOT

import _metrics_cases as mc


def test_header_and_binding_declare_the_entry_points():
    from vdiff import _lib
    src = open(os.path.join(ROOT, "include", "vdiff.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("vd_clip_metrics", "vd_clip_metrics_workspace_size"):
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in _lib._SIGS, name
    assert _lib.ABI_VERSION == 1
    lib = _lib.load()
    # host-side argument checks, no GPU: a frame below the window, hi <= lo, null pointers
    assert lib.vd_clip_metrics_workspace_size(2, 3, 3, 45, 77) == 2 * 3 * 3 * 2 * 3 * 16
    assert lib.vd_clip_metrics_workspace_size(1, 1, 1, 10, 77) == 0
    one = 16  # a non-null address that is never dereferenced: the checks come first
    bad = [dict(H=10), dict(W=10), dict(hi=-1.0), dict(x=None), dict(mse=None), dict(ws=None),
           dict(dtype=7), dict(B=0)]
    for kw in bad:
        a = dict(x=one, y=one, lo=-1.0, hi=1.0, B=1, C=1, T=1, H=11, W=11, dtype=0, mse=one,
                 ssim=one, wpx=one, wv=one, ws=one)
        a.update(kw)
        rc = lib.vd_clip_metrics(a["x"], a["y"], None, a["lo"], a["hi"], a["B"], a["C"], a["T"],
                                 a["H"], a["W"], a["dtype"], a["mse"], a["ssim"], a["wpx"],
                                 a["wv"], None, a["ws"], None)
        assert rc != 0 and lib.vd_last_error(), kw


def test_oracle_identical_clips():
    x, _ = mc.pair((1, 2, 2, 17, 23), "noise")
    r = mc.oracle64(x, x.clone())
    assert torch.equal(r["mse"], torch.zeros(1, 2, dtype=torch.float64))
    assert (r["map"] - 1.0).abs().max() < 1e-12 and (r["ssim"] - 1.0).abs().max() < 1e-12
    assert r["map"].shape == (1, 2, 2, 7, 13)
    assert torch.equal(r["wsum_px"], torch.full((2,), 17.0 * 23.0, dtype=torch.float64))
    assert torch.equal(r["wsum_valid"], torch.full((2,), 7.0 * 13.0, dtype=torch.float64))


@pytest.mark.parametrize("a,b", [(0.7, -0.9), (0.0, 0.0), (-1.0, 1.0), (0.25, 0.5)])
def test_oracle_constant_planes(a, b):
    """Two constant planes: SSIM = (2 a b + C1) / (a^2 + b^2 + C1) on the mapped values (the
    window's fp32 taps sum to 1 within 1e-7, hence the tolerance), MSE = (a - b)^2."""
    shape = (1, 1, 1, 13, 12)
    r = mc.oracle64(torch.full(shape, a), torch.full(shape, b))
    ua, ub = (float(torch.tensor(a)) + 1) / 2, (float(torch.tensor(b)) + 1) / 2
    assert (r["map"] - mc.flat_ssim(ua, ub)).abs().max() < 1e-6
    assert abs(float(r["mse"]) - (ua - ub) ** 2) < 1e-14
    if (a, b) == (0.7, -0.9):
        # the reason for the range mapping: on raw [-1, 1] data the luminance term is negative
        raw = mc.flat_ssim(a, b)
        assert abs(raw + 0.97) < 0.01 and float(r["ssim"]) > 0


def test_oracle_mse_by_hand_and_clamp():
    x, y, want = mc.hand_mse_pair()
    r = mc.oracle64(x, y)
    assert abs(float(r["mse"]) - want) < 1e-15
    assert r["map"].shape == (1, 1, 1, 1, 1)
    # a weight that selects the one differing pixel: its squared difference alone
    w = torch.zeros(1, 11, 11)
    w[0, 3, 7] = 2.0
    r = mc.oracle64(x, y, w)
    assert abs(float(r["mse"]) - 0.25) < 1e-15 and float(r["wsum_px"]) == 2.0
    assert math.isnan(float(r["ssim"]))  # the only valid centre (5, 5) has weight 0
    # values outside the range score as their clamp
    xo, yo = mc.pair((1, 1, 1, 12, 12), "overshoot")
    a, b = mc.oracle64(xo, yo), mc.oracle64(xo.clamp(-1, 1), yo)
    assert (xo.abs() > 1).any() and torch.equal(a["map"], b["map"]) \
        and torch.equal(a["mse"], b["mse"])


def test_naive_fp32_loses_accuracy_on_smooth_frames():
    """The yardstick itself: E[u^2] - E[u]^2 in fp32 is orders of magnitude worse on the smooth
    field than on noise (the reason the kernel pivots its moments)."""
    shape = (1, 1, 1, 45, 77)
    tn = mc.map_tolerance(*mc.pair(shape, "noise"), mc.oracle64(*mc.pair(shape, "noise"))["map"])
    ts = mc.map_tolerance(*mc.pair(shape, "smooth"),
                          mc.oracle64(*mc.pair(shape, "smooth"))["map"])
    assert tn[1] < 5e-6 and ts[1] > 10 * tn[1], (tn, ts)


def test_clip_metrics_raises_on_cpu_tensors():
    from vdiff import metrics, ops
    x = torch.zeros(1, 3, 2, 16, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.clip_metrics(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.clip_metrics(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.psnr(x, x)
    import vdiff
    assert vdiff.metrics is metrics


def test_region_weight_of_a_keep_mask():
    from vdiff.metrics import region_weight
    from vdiff.schedulers import keep_mask
    keep = keep_mask(3, 16, 20, generate_box=(0.5, 1.0, 0.25, 0.75), keep_frames=1, feather=3)
    w = region_weight(keep)
    assert w.shape == (3, 16, 20) and w.dtype == torch.float32 and w.is_contiguous()
    assert torch.equal(w, 1.0 - keep[0, 0])
    assert float(w[0].abs().max()) == 0.0          # the kept frame carries no weight
    assert float(w[1, 15, 10]) == 1.0 and float(w[1, 0, 0]) == 0.0
    assert 0.0 < float(w[1, 8, 10]) < 1.0          # the feather is part of the weight
    w2 = region_weight(keep_mask(1, 16, 20).view(1, 1, 16, 20))
    assert w2.shape == (16, 20) and float(w2[15, 0]) == 1.0 and float(w2[0, 0]) == 0.0
    with pytest.raises(ValueError):
        region_weight(torch.zeros(2, 1, 3, 16, 20))


def test_entry_point_score_flags():
    """parse() takes --score / --score-against / --score-out, leaves them off by default, and
    refuses --score without a target, a sampler other than ddim / dpm++ and --score-out alone
    (argparse errors: exit status 2).  A fresh interpreter: test.py is a module named `test`."""
    code = f"""
import contextlib, io, sys
sys.path.insert(0, {DROPIN!r}); sys.path.insert(1, {ROOT!r})
import test
base = ["--random-init", "--sampler", "ddim", "--steps", "2"]
a = test.parse(base + ["--known", "k.npy", "--score"])
assert a.score and a.score_against is None and a.score_out is None
a = test.parse(base + ["--score-against", "gt.npy", "--score-out", "m.json"])
assert a.score_against == "gt.npy" and a.score_out == "m.json"
a = test.parse(["--random-init", "--sampler", "dpm++", "--known", "k.npy", "--score-against",
                "gt.npy", "--score"])
assert a.score and a.score_against == "gt.npy"
a = test.parse(base)
assert not a.score and a.score_against is None and a.score_out is None
for argv, word in ((base + ["--score"], "--known or --score-against"),
                   (["--random-init", "--known", "k.npy", "--score"], "ddim or dpm++"),
                   (["--random-init", "--sampler", "ddpm-v2", "--score-against", "gt.npy"],
                    "ddim or dpm++"),
                   (base + ["--score-out", "m.json"], "--score")):
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            test.parse(argv)
    except SystemExit as e:
        assert e.code == 2 and word in err.getvalue(), (argv, err.getvalue())
    else:
        raise AssertionError(f"accepted {{argv}}")
print("OK")
"""
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout, out.stderr[-3000:]
