"""test.py --score end to end, and the vdiff.metrics command line (fresh child processes, as
tests/test_gpu_entrypoints.py starts them): a masked DDIM sample of 2 steps at 32 x 32 x 4 is
scored against its known clip, whole frame and generated region; metrics.json holds what
vdiff.metrics.clip_metrics gives on the saved sample; the kept region alone is the known clip."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import DROPIN, PKG

import _metrics_cases as mc

pytestmark = pytest.mark.gpu
dev = "cuda"
SHAPE = (3, 4, 32, 32)
BOX = ("0.5", "1", "0", "1")   # the lower half of every frame is generated


def _child(argv, cwd):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(
        [PKG] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    out = subprocess.run([sys.executable] + argv, cwd=cwd, capture_output=True, text=True,
                         timeout=900, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


def _rows(t):
    return [[float(v) for v in r] for r in t.detach().double().cpu().tolist()]


def test_score_entry_and_command_line(tmp_path):
    from vdiff import metrics, ops
    from vdiff.schedulers import keep_mask
    g = torch.Generator().manual_seed(3)
    known = (torch.rand(SHAPE, generator=g) * 2 - 1).bfloat16().float()  # exact in either dtype
    np.save(tmp_path / "K.npy", known.numpy())
    out_dir = tmp_path / "imgs"
    out = _child([os.path.join(DROPIN, "test.py"), "--random-init", "--sampler", "ddim",
                  "--steps", "2", "--image-size", "32", "--dims", "3", "--frames", "4",
                  "--save-every", "1", "--out-dir", str(out_dir), "--known",
                  str(tmp_path / "K.npy"), "--generate-box", *BOX, "--score"], tmp_path)
    assert "generated region" in out and "whole frame" in out
    rep = json.load(open(out_dir / "metrics.json"))
    assert rep["against"] == "known" and set(rep) >= {"whole", "region"}
    sample = torch.from_numpy(np.load(out_dir / "sample.npy"))
    assert tuple(sample.shape) == SHAPE and torch.isfinite(sample).all()
    S, K = sample[None].to(dev), known[None].to(dev)
    keep = keep_mask(4, 32, 32, generate_box=tuple(float(v) for v in BOX))
    for name, w in (("whole", None), ("region", metrics.region_weight(keep))):
        m = metrics.clip_metrics(S, K, weight=w)
        for q in ("mse", "psnr", "ssim"):
            assert rep[name][q] == _rows(getattr(m, q)), (name, q)
        mean = m.mean()
        assert rep[name]["mean"]["ssim"] == mean["ssim"] and rep[name]["mean"]["mse"] == mean["mse"]
    # kept pixels are the known clip: the whole-frame score flatters, the region's is lower
    assert rep["whole"]["mean"]["ssim"] > rep["region"]["mean"]["ssim"]
    assert rep["whole"]["mean"]["mse"] < rep["region"]["mean"]["mse"]
    # the kept region alone: MSE 0, and SSIM 1 where the window lies inside it (map rows 0 .. 5:
    # window rows y .. y + 10 <= 15)
    kept = ops.clip_metrics(S, K, keep[0, 0].to(dev), want_map=True)
    assert torch.equal(kept.mse.cpu(), torch.zeros(1, 4))
    assert (kept.ssim_map[..., :6, :].cpu() - 1).abs().max() <= mc.MAP_FLOOR

    # the command line on the two saved clips prints the same numbers
    cli = _child(["-m", "vdiff.metrics", str(out_dir / "sample.npy"), str(tmp_path / "K.npy"),
                  "--weight", str(out_dir / "score_weight.npy"), "--json",
                  str(tmp_path / "cli.json")], tmp_path)
    lines = [ln for ln in cli.splitlines() if ln.startswith("clip 0 frame")]
    assert len(lines) == 4
    region = metrics.clip_metrics(S, K, weight=metrics.region_weight(keep))
    for t, ln in enumerate(lines):
        got = [float(v) for v in re.findall(r"(?:mse|psnr|ssim) (\S+)", ln)]
        want = [float(f"{float(region.mse[0, t]):.9g}"), float(f"{float(region.psnr[0, t]):.6f}"),
                float(f"{float(region.ssim[0, t]):.9g}")]
        assert got == want, (ln, want)
    assert json.load(open(tmp_path / "cli.json")) == rep["region"]


def test_score_against_a_ground_truth_clip(tmp_path):
    """--score-against needs no masked sampling: whole-frame values only, --score-out honoured,
    with the dpm++ sampler."""
    from vdiff import metrics
    g = torch.Generator().manual_seed(4)
    truth = torch.rand(SHAPE, generator=g) * 2 - 1
    np.save(tmp_path / "gt.npy", truth.numpy())
    out_dir = tmp_path / "imgs"
    _child([os.path.join(DROPIN, "test.py"), "--random-init", "--sampler", "dpm++", "--steps", "2",
            "--image-size", "32", "--dims", "3", "--frames", "4", "--save-every", "1",
            "--out-dir", str(out_dir), "--score-against", str(tmp_path / "gt.npy"),
            "--score-out", str(tmp_path / "m.json")], tmp_path)
    rep = json.load(open(tmp_path / "m.json"))
    assert rep["against"] == "score-against" and "region" not in rep
    sample = torch.from_numpy(np.load(out_dir / "sample.npy"))
    m = metrics.clip_metrics(sample[None].to(dev), truth[None].to(dev))
    assert rep["whole"]["ssim"] == _rows(m.ssim) and rep["whole"]["psnr"] == _rows(m.psnr)
    assert not os.path.exists(out_dir / "metrics.json")
