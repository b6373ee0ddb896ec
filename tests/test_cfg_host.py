"""Classifier-free audio guidance, host side (CPU, no GPU): the C-ABI additions, the entry
points' new options, the conditioning-dropout mask, and the bound the GPU test puts on the
rescale factor."""
import inspect
import math
import os
import re
import subprocess
import sys
import textwrap

import pytest
import torch

from conftest import DROPIN, ROOT

import _cfg_cases as cases
from vdiff import _lib

CFG_SYMBOLS = ("vd_cfg_workspace_size", "vd_cfg_stats", "vd_ddim_step_cfg", "vd_cfg_combine")


def test_symbols_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "vdiff.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(vd_[a-z0-9_]+)\s*\(", src))
    for name in CFG_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTED_SYMBOLS, name
    assert re.search(r"#define\s+VDIFF_ABI_VERSION\s+1\b", src) and _lib.ABI_VERSION == 1


def test_null_arguments_fail_without_a_gpu():
    lib = _lib.load()
    rc = lib.vd_ddim_step_cfg(None, None, None, None, None, None, None, None, None, None,
                              2.0, 0.0, None, 0.0, 0, 0, 0, 0, None)
    assert rc == 1 and b"null" in lib.vd_last_error()
    rc = lib.vd_cfg_combine(None, None, None, 2.0, 0.0, None, 0, 0, 0, None)
    assert rc == 1 and b"null" in lib.vd_last_error()
    rc = lib.vd_cfg_stats(None, None, 2.0, 0, 0, 0, None, 0, None)
    assert rc == 1 and b"null" in lib.vd_last_error()


def test_workspace_size_monotone():
    lib = _lib.load()
    ps = [1, 7, 8, 105, 768, 2048, 2049, 5000, 19200, 786432, 1 << 24, (1 << 31) + 8]
    for B in (1, 2, 3, 64):
        sizes = [lib.vd_cfg_workspace_size(B, p) for p in ps]
        assert all(s > 0 for s in sizes)
        assert sizes == sorted(sizes), (B, sizes)
    for p in ps:
        sizes = [lib.vd_cfg_workspace_size(B, p) for B in (1, 2, 3, 64)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1], (p, sizes)
    # four fp32 slots per partial: the split the emulation below walks
    for B, P in cases.SHAPES:
        assert lib.vd_cfg_workspace_size(B, P) == B * cases.partials(P)[0] * 16


def _dropin(code):
    src = f"import sys; sys.path.insert(0, {DROPIN!r}); sys.path.insert(1, {ROOT!r})\n"
    out = subprocess.run([sys.executable, "-c", src + textwrap.dedent(code)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.strip().splitlines()[-1]


def test_entry_point_defaults_and_signature():
    out = _dropin("""
        import inspect, json, train, test
        a, b = train.parse([]), test.parse([])
        c = test.parse(["--guidance-scale", "2.5", "--guidance-rescale", "0.7"])
        ps = inspect.signature(test.sample_images).parameters
        print(json.dumps({"drop": a.audio_drop_prob, "w": b.guidance_scale,
                          "phi": b.guidance_rescale, "set": [c.guidance_scale, c.guidance_rescale],
                          "drop_set": train.parse(["--audio-drop-prob", "0.2"]).audio_drop_prob,
                          "names": list(ps), "kinds": {n: ps[n].kind.name for n in ps},
                          "defaults": [ps["guidance_scale"].default,
                                       ps["guidance_rescale"].default]}))
    """)
    import json
    d = json.loads(out)
    assert d["drop"] == 0.0 and d["w"] == 1.0 and d["phi"] == 0.0
    assert d["set"] == [2.5, 0.7] and d["drop_set"] == 0.2
    assert d["names"][:5] == ["model", "scheduler", "img_cond", "audio_cond", "n_timesteps"]
    for n in ("guidance_scale", "guidance_rescale"):
        assert d["names"].index(n) >= 5 and d["kinds"][n] == "KEYWORD_ONLY"
    assert d["defaults"] == [1.0, 0.0]


def test_engine_signatures_default_to_unguided():
    from vdiff import engine
    from vdiff.schedulers import DDIMSampler
    from vdiff.unet_audio import UNetAudio
    for fn in (engine.sample_ddim, engine.sample_ddpm):
        ps = inspect.signature(fn).parameters
        assert ps["guidance_scale"].default == 1.0 and ps["guidance_rescale"].default == 0.0
    ps = inspect.signature(engine.DDIMGraph.__init__).parameters
    assert ps["guidance_scale"].default == 1.0 and ps["guidance_rescale"].default == 0.0
    ps = inspect.signature(engine.Trainer.__init__).parameters
    assert ps["audio_drop_prob"].default == 0.0 and ps["drop_generator"].default is None
    assert inspect.signature(UNetAudio.forward).parameters["audio_keep"].default is None
    assert list(inspect.signature(DDIMSampler.step_guided).parameters)[1:] == [
        "xt", "eps_c", "eps_u", "i", "scale", "rescale", "z"]


def test_audio_keep_mask():
    from vdiff.engine import audio_keep_mask
    g = torch.Generator().manual_seed(3)
    assert torch.equal(audio_keep_mask(64, 0.0, "cpu", g), torch.ones(64))
    assert torch.equal(audio_keep_mask(64, 1.0, "cpu", g), torch.zeros(64))
    n, p = 4096, 0.25
    m = audio_keep_mask(n, p, "cpu", torch.Generator().manual_seed(11))
    assert m.shape == (n,) and m.dtype == torch.float32
    assert set(m.unique().tolist()) <= {0.0, 1.0}
    dropped = float((m == 0).float().mean())
    assert abs(dropped - p) <= 4 * math.sqrt(p * (1 - p) / n), dropped
    assert torch.equal(m, audio_keep_mask(n, p, "cpu", torch.Generator().manual_seed(11)))
    assert not torch.equal(m, audio_keep_mask(n, p, "cpu", torch.Generator().manual_seed(12)))
    with pytest.raises(ValueError):
        audio_keep_mask(4, 1.5, "cpu")


def test_apply_audio_keep_zeroes_whole_clips():
    from vdiff.unet_audio import apply_audio_keep
    keep = torch.tensor([1.0, 0.0, 1.0])
    for shape in ((6, 5), (6, 4, 5)):  # pooled features, tokens; T = 2 windows per clip
        enc = torch.randn(shape)
        out = apply_audio_keep(enc, keep)
        assert torch.equal(out[:2], enc[:2]) and torch.equal(out[4:], enc[4:])
        assert (out[2:4] == 0).all()
    with pytest.raises(ValueError):
        apply_audio_keep(torch.randn(5, 4), keep)


def test_trainer_draws_no_mask_without_dropout():
    """audio_drop_prob = 0: the model is called exactly as before (no audio_keep keyword, so a
    model without it keeps working); > 0 hands the drawn mask over."""
    import torch.nn.functional as F
    from vdiff.engine import Clip, Trainer

    class Sched:
        def add_noise(self, x0, eps, t):
            return x0 + eps

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(()))
            self.seen = []

        def forward(self, x, cond, audio, t, **kw):
            self.seen.append(kw)
            return x * self.w

    clip = Clip(torch.randn(4, 3, 2, 2), torch.randn(4, 3, 2, 2), torch.randn(4, 8),
                torch.randn(4, 3, 2, 2), torch.zeros(4, dtype=torch.int64))
    m = Model()
    Trainer(m, Sched(), loss_fn=F.mse_loss, fused_adam=False, batch_pack=False).step(clip)
    assert m.seen == [{}]
    m = Model()
    g = torch.Generator().manual_seed(5)
    Trainer(m, Sched(), loss_fn=F.mse_loss, fused_adam=False, batch_pack=False,
            audio_drop_prob=0.5, drop_generator=g).step(clip)
    from vdiff.engine import audio_keep_mask
    want = audio_keep_mask(4, 0.5, "cpu", torch.Generator().manual_seed(5))
    assert list(m.seen[0]) == ["audio_keep"] and torch.equal(m.seen[0]["audio_keep"], want)
    with pytest.raises(ValueError):
        Trainer(Model(), Sched(), loss_fn=F.mse_loss, fused_adam=False, batch_pack=False,
                audio_drop_prob=-0.1)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("B,P", cases.SHAPES)
@pytest.mark.parametrize("w", [0.0, 1.0, 2.5, 7.5])
def test_rescale_factor_bound_holds_for_the_shipped_order(B, P, bf16, w):
    """The bound the GPU test folds into c_extra for phi > 0 (_cfg_cases.ratio_rel_bound): the
    relative error of r = sqrt(SS(c) / SS(g)), SS(x) = sum (x_i - mean(x))^2, is at most

        2 (P + 2) u32 + 4 u32 (rms|c| / sigma_c + rms(mag_g) / sigma_g),

    mag_g = |u| + |w| (|c| + |u|), sigma^2 = SS / P, u32 = 2^-24.  Derivation, for a two-pass
    fp32 reduction (a mean, then sum (x_i - mean)^2 with fused multiply-adds):
      * Summation.  Each SS is a sum of P non-negative terms, so its rounding error is at most
        (P + 2) u32 relative in any order.  r is the square root of a quotient of two such
        sums, each entering with weight 1/2: (P + 2) u32.  The second (P + 2) u32 covers the
        divide, the square root and the two roundings of phi r + (1 - phi).
      * Element errors.  d_i = x_i - mean carries an absolute error delta_i: for g the two
        roundings of u + w (c - u), at most 2 u32 mag_g,i; the elements of c are exact and the
        rounding of the subtraction belongs to the summation term.  To first order SS changes
        by 2 sum d_i delta_i <= 2 sqrt(SS) sqrt(sum delta_i^2), relative 4 u32 rms(mag) /
        sigma, and half of that through the square root; the bound keeps the full 4 u32 for
        each of c and g.
      * The mean.  A computed mean off by dm leaves the first order untouched (sum d_i = 0)
        and adds P dm^2 to SS, relative (dm / sigma)^2: second order, not part of the bound.
        The mean is a sum of the elements themselves, so dm <= k u32 rms|x| with k the number
        of adds on the longest path of the shipped order: 8 per lane, 8 levels of the LDS
        tree, 8 more over the partials, the divide, k = 25 at these shapes.  At |mean| = 64
        sigma that is (25 * 64 u32)^2 / 2 = 5e-9 against 4 u32 * 64 = 1.5e-5 of the line above.

    The test: the workspace holds the partials the emulation walks (so it follows the shipped
    split), and an fp32 emulation of the shipped reduction order (per lane, LDS tree, partials
    one per lane through the same tree, mean, centred fused multiply-adds) on the GPU test's
    own inputs -- the sample with mean 16 and sigma 0.25 included -- stays inside the bound,
    against the fp64 ratio of the same inputs."""
    assert _lib.load().vd_cfg_workspace_size(B, P) == B * cases.partials(P)[0] * 16
    _, c, u, _ = cases.inputs(B, P, bf16)
    got = cases.emulate_ratio_fp32(c, u, w).double()
    want = cases.factor64(c, u, w, 1.0).view(-1)
    bound = cases.ratio_rel_bound(c, u, w).view(-1)
    rel = (got - want).abs() / want
    assert (rel <= bound).all(), (rel.tolist(), bound.tolist())
    assert (bound < 2.0 ** -8).all(), bound.tolist()  # stays below one bf16 rounding
    print(f"P={P} bf16={bf16} w={w}: rel/bound {float((rel / bound).max()):.3g}")

