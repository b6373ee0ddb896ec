"""Masked sampling on the GPU, the samplers: sample_ddim / sample_dpm / sample_long with `known`
and `keep` on the tiny random-init UNetAudio of tests/test_gpu_ddim_graph.py.  For the elements
with keep == 1 and any model: the replayed graph equals the eager loop bit for bit, the sample
after every step lies on sqrt(a_p) x_k + sqrt(1 - a_p) z within the trajectory bound of
tests/_known_cases.py, and the final x0 and sample ARE the known clip.  keep == 0 everywhere is the
unmasked sample; the captured step has the unmasked graph's node counts; the entry point runs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import DROPIN

import _dpm_cases as dpm
import _known_cases as cases

pytestmark = pytest.mark.gpu
dev = "cuda"
STEPS = 6
GUIDE = dict(guidance_scale=7.5, guidance_rescale=0.7)
_models = {}


def _model():
    from test_gpu_ddim_graph import _model as tiny
    if "m" not in _models:
        _models["m"] = tiny(3, True)
    return _models["m"]


def _case(L):
    g = torch.Generator(device=dev).manual_seed(77)
    cond = torch.rand((1, 3, 32, 32), device=dev, generator=g) * 2 - 1
    feats = torch.randn((L, 64), device=dev, generator=g)
    known = torch.rand((1, 3, L, 32, 32), device=dev, generator=g) * 2 - 1
    return (1, 3, L, 32, 32), cond, feats, known


def _sampler(name):
    from vdiff.schedulers import DDIMSampler, DPMSolverSampler
    cls = DDIMSampler if name == "ddim" else DPMSolverSampler
    s = cls(dpm.v2_scheduler(), steps=STEPS)
    assert s.steps == STEPS
    return s


def _gen():
    return torch.Generator(device=dev).manual_seed(9)


def _sample(name, long_, sampler, **kw):
    from vdiff.engine import sample_ddim, sample_dpm, sample_long
    shape, cond, feats, _ = _case(8 if long_ else 4)
    if long_:
        return sample_long(_model(), sampler, cond, feats, shape, window=4, stride=2,
                           generator=_gen(), **kw)
    return (sample_ddim if name == "ddim" else sample_dpm)(_model(), sampler, cond, feats, shape,
                                                           generator=_gen(), **kw)


def _mask(long_):
    from vdiff.schedulers import WindowPlan, keep_mask
    if long_:
        assert WindowPlan(8, 4, 2).num_windows == 3
        return keep_mask(8, 32, 32, generate_box=(0, 1, 0, 1), keep_frames=2)
    return keep_mask(4, 32, 32, keep_frames=1, feather=2)


def _check_invariants(name, long_, guided, monkeypatch):
    sampler = _sampler(name)
    shape, _, _, known = _case(8 if long_ else 4)
    keep = _mask(long_)
    one = (keep >= 1).expand(shape).to(dev)
    assert one.any() and not one.all()
    if not long_:
        assert ((keep > 0) & (keep < 1)).any()
    z = torch.randn(shape, generator=_gen(), device=dev)   # the driver's own first draw
    kw = dict(GUIDE) if guided else {}
    out, traj = {}, {}
    for mode in ("0", "1"):
        monkeypatch.setenv("VDIFF_DDIM_GRAPH", mode)
        seen = traj[mode] = []
        out[mode] = _sample(name, long_, sampler, known=known, keep=keep,
                            callback=lambda i, xt, x0: seen.append((xt.clone(), x0.clone())),
                            **kw)
    # 1. replayed == eager, at every step
    assert len(traj["0"]) == len(traj["1"]) == STEPS
    for i, ((xa, x0a), (xb, x0b)) in enumerate(zip(traj["0"], traj["1"])):
        assert torch.equal(xa[one], xb[one]) and torch.equal(x0a[one], x0b[one]), i
        assert torch.equal(xa, xb) and torch.equal(x0a, x0b), i
    for a, b in zip(out["0"], out["1"]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    # 2. the kept elements stay on the line from the known clip to the initial noise
    rows = sampler.coef if name != "ddim" else None
    tr = cases.trajectory(sampler.acp, sampler.timesteps, sampler.prev_timesteps, known[one].cpu(),
                          z[one].cpu(), rows=rows)
    worst = 0.0
    for i, (ap, E) in enumerate(tr):
        line = cases.on_line(ap, known[one].cpu(), z[one].cpu())
        for mode in ("0", "1"):
            err = (traj[mode][i][0][one].cpu().double() - line).abs()
            ratio = float((err / E).max())
            print(f"{name} long={long_} guided={guided} graph={mode} step {i}: a_p {ap:.6f} "
                  f"largest |xt - line| / bound {ratio:.3g}")
            assert (err <= E).all(), (name, long_, guided, mode, i, ratio)
            worst = max(worst, ratio)
            # x0 at a kept element is the known value at every step
            assert torch.equal(traj[mode][i][1][one], known[one]), (mode, i)
    assert worst > 0
    # 3. the result is the known clip there, and something else elsewhere
    xt, x0 = out["1"]
    assert torch.equal(x0[one], known[one]) and torch.equal(xt[one], known[one])
    gen = (keep <= 0).expand(shape).to(dev)
    assert not torch.equal(x0[gen], known[gen])
    return out["1"]


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("name", ["ddim", "dpm++"])
def test_masked_sampling_invariants(name, guided, monkeypatch):
    _check_invariants(name, False, guided, monkeypatch)


@pytest.mark.parametrize("name", ["ddim", "dpm++"])
def test_masked_long_clip_continues_the_given_frames(name, monkeypatch):
    """Three windows over 8 frames, the first two frames given: the long latent is what the step
    kernel sees, so the same invariants hold on it."""
    _check_invariants(name, True, True, monkeypatch)


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("name", ["ddim", "dpm++"])
def test_keep_zero_everywhere_is_the_unmasked_sample(name, guided):
    sampler = _sampler(name)
    shape, _, _, known = _case(4)
    kw = dict(GUIDE) if guided else {}
    want = _sample(name, False, sampler, **kw)
    got = _sample(name, False, sampler, known=known, keep=torch.zeros((1, 1) + shape[2:]), **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("long_", [False, True], ids=["short", "long"])
@pytest.mark.parametrize("name", ["ddim", "dpm++"])
def test_masked_graph_nodes(name, long_, guided):
    """The masked step kernel takes the unmasked one's place: no memset node and the same node
    counts."""
    from vdiff import ops
    from vdiff.engine import (DDIMGraph, DPMGraph, LongDDIMGraph, LongDPMGraph,
                              WindowedDenoiser)
    from vdiff.sampling import _masked_start
    from vdiff.schedulers import WindowPlan
    m = _model()
    shape, cond, feats, known = _case(8 if long_ else 4)
    kw = dict(GUIDE) if guided else {}
    counts = {}
    with torch.no_grad(), ops.frozen_weights():
        for masked in (False, True):
            sampler = _sampler(name)
            xt = torch.randn(shape, device=dev, generator=torch.Generator(dev).manual_seed(3))
            mask = {}
            if masked:
                xt, kn, kp = _masked_start(sampler, xt, known, _mask(long_))
                mask = dict(known=kn, keep=kp)
            if long_:
                windows = WindowedDenoiser(m, WindowPlan(8, 4, 2), cond, feats, xt, guided)
                gr = (LongDDIMGraph if name == "ddim" else LongDPMGraph)(m, sampler, windows, xt,
                                                                         **kw, **mask)
            else:
                gr = (DDIMGraph if name == "ddim" else DPMGraph)(m, sampler, cond, feats, xt, **kw,
                                                                 **mask)
            gr.capture()
            counts[masked] = gr.node_types()
            got, x0 = gr.step(0)
            assert torch.isfinite(got).all() and torch.isfinite(x0).all()
    assert counts[True].get("memset", 0) == 0 and counts[False].get("memset", 0) == 0, counts
    assert counts[True] == counts[False], counts


def test_sampling_entry(tmp_path):
    """test.py as a fresh process: 4 steps of 2M on a 2-frame clip whose first frame is given."""
    out_dir = tmp_path / "imgs"
    known = np.random.default_rng(5).uniform(-1, 1, (3, 2, 32, 32)).astype(np.float32)
    np.save(tmp_path / "known.npy", known)
    out = subprocess.run([sys.executable, os.path.join(DROPIN, "test.py"), "--random-init",
                          "--dims", "3", "--frames", "2", "--image-size", "32", "--sampler",
                          "dpm++", "--steps", "4", "--save-every", "1", "--out-dir", str(out_dir),
                          "--known", str(tmp_path / "known.npy"), "--keep-frames", "1"],
                         cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    files = sorted(p for p in os.listdir(out_dir) if p.endswith(".npy"))
    assert len(files) == 4, files
    for f in files:
        x0 = np.load(out_dir / f)
        assert x0.shape == (1, 3, 2, 32, 32) and np.isfinite(x0).all()
        # frame 0 is kept whole, and the upper half of frame 1 (the default box): the saved image
        # is (x0 + 1) / 2 of the known clip, bit for bit
        want = (np.clip(known, -1, 1) + 1) / 2
        assert np.array_equal(x0[0, :, 0], want[:, 0]), f
        assert np.array_equal(x0[0, :, 1, :16], want[:, 1, :16]), f
        assert not np.array_equal(x0[0, :, 1, 16:], want[:, 1, 16:]), f
