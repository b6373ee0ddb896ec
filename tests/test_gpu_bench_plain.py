"""A plain `bench.py --gpus 1 --steps K --warmup W` run: only the headline train steps (no leg
of --full in the line), K really sets the number of timed steps, and --dump-outputs DIR writes
the last timed step's outputs as float32 / float64 .npy files; the same arguments build the
same initial weights and clips again.  bench.main() runs in this process on a 32x32x4 clip."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ("ddim", "ddim_st", "ddim_config4", "audio_xattn", "spatial_temporal", "train_graph",
             "vivit", "conv_kernels")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _with_argv(fn, out_dir, steps):
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--size",
                    "32", "--frames", "4", "--dump-outputs", str(out_dir)]
        return fn()
    finally:
        sys.argv = argv


def _run(b, capsys, out_dir, steps):
    _with_argv(b.main, out_dir, steps)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f))
                                  for f in sorted(os.listdir(out_dir))}


def test_plain_run_line_and_dumped_outputs(capsys, tmp_path):
    b = _bench()
    r, a = _run(b, capsys, tmp_path / "a", 3)
    assert r["metric"] == b.METRIC and r["unit"] == "frames/s" and r["higher_is_better"] is True
    assert r["dtype"] == "bf16" and r["n_gpus"] == 1
    assert r["steps"] == 3 and len(r["train_losses"]) == 1 + 3
    assert r["ms_per_step"] > 0
    # value = frames of the timed steps / their time: 4 frames per step
    assert r["value"] == pytest.approx(4 / (r["ms_per_step"] / 1e3), rel=2e-2)
    assert not [k for k in FULL_ONLY if k in r] and r["cpu_baseline"] is None
    assert sorted(a) == ["loss", "param_delta_sample", "param_norms", "param_sample",
                         "train_losses"]
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 * 2 ** 20
    assert all(np.isfinite(x).all() for x in a.values())
    assert a["train_losses"].shape == (4,) and a["loss"][0] == a["train_losses"][-1]
    np.testing.assert_allclose(a["train_losses"], r["train_losses"], rtol=0, atol=1e-5)
    # the steps trained: one Adam step moves a parameter by lr |m^ / sqrt(v^)|, and over the
    # first 4 steps that ratio is <= 1.007 (Cauchy-Schwarz on the bias-corrected averages)
    assert 0 < np.abs(a["param_delta_sample"]).max() <= 4 * 1e-4 * 1.01
    # the same arguments again give the same inputs: the initial weights of a second build are
    # the ones the run started from (the dumped sample minus its change; the subtraction
    # rounds, hence 1e-6 on values of order 1), and the seeded clips come out bit for bit
    import torch
    args = _with_argv(b.parse, tmp_path / "a", 3)
    dev = torch.device("cuda", 0)
    b.seed_host(1234)
    again = b.OutputDump(b.build_model(args, dev)).before.numpy()
    np.testing.assert_allclose(again, a["param_sample"] - a["param_delta_sample"], rtol=0,
                               atol=1e-6)
    for c1, c2 in zip(b.clip_bank(args, 2, dev, 0), b.clip_bank(args, 2, dev, 0)):
        assert all(torch.equal(x, y) for x, y in ((c1.x0, c2.x0), (c1.cond, c2.cond),
                                                  (c1.eps, c2.eps), (c1.t, c2.t)))
        assert torch.equal(c1.audio["input_values"], c2.audio["input_values"])
    assert not torch.equal(c1.x0, b.clip_bank(args, 1, dev, 0)[0].x0)  # a clip of its own per step
