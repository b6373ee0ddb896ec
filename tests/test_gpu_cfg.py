"""Classifier-free audio guidance on the GPU: the statistics / fused-step / combine kernels
against fp64 with element-wise bounds (tests/_cfg_cases.py derives them), their exactness
properties, the guided samplers (graph replay against the eager loop, bit for bit), audio
dropout in training, and the entry points' new options."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import DROPIN, record_metric

import _cfg_cases as cases
from _bounds import assert_elementwise

pytestmark = pytest.mark.gpu
dev = "cuda"

WS = (0.0, 1.0, 2.5, 7.5)


def _acp():
    from vdiff.schedulers import LinearNoiseSchedulerV2
    return LinearNoiseSchedulerV2(500, 0.00005, 0.015).alpha_cum_prod.float()


def _to_dev(bf16, *xs):
    dt = torch.bfloat16 if bf16 else torch.float32
    return tuple(x.to(device=dev, dtype=dt).contiguous() for x in xs)


# ------------------------------------------------------------------ kernels against fp64
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,P", cases.SHAPES)
def test_kernels_against_fp64(B, P, bf16):
    """x_prev and x0 of the fused step, eps of cfg_combine, and the composed ddim_step(
    cfg_combine) each against fp64 on the same dtype-rounded inputs, for every w, phi, eta and
    clip; the f_b bound is folded into c_extra when phi > 0 (_cfg_cases.ref64)."""
    from vdiff import _lib, ops
    xt, c, u, z = cases.inputs(B, P, bf16)
    t, tp = cases.timesteps(B)
    acp = _acp()
    nb, chunk = cases.partials(P)
    assert _lib.lib().vd_cfg_workspace_size(B, P) == B * nb * 16
    if P == 5000:  # whole 8-vectors, at least three partials, ranges no multiple of a block's
        assert P % 8 == 0 and nb >= 3 and chunk % (cases.K_BLOCK * 8) != 0 and P % chunk != 0
    xt_d, c_d, u_d, z_d = _to_dev(bf16, xt, c, u, z)
    t_d, tp_d, acp_d = t.to(dev), tp.to(dev), acp.to(dev)
    worst = {"fused": 0.0, "eps": 0.0, "composed": 0.0}
    for w in WS:
        for phi in (0.0, 0.7):
            eps_k = ops.cfg_combine(c_d, u_d, w, phi)
            for eta in (0.0, 0.5):
                zz = z_d if eta else None
                for clip in (False, True):
                    what = f"B={B} P={P} bf16={bf16} w={w} phi={phi} eta={eta} clip={clip}"
                    ref = cases.ref64(xt, c, u, z, t, tp, acp, w, phi, eta, clip)
                    xp, x0 = ops.ddim_step_cfg(xt_d, c_d, u_d, t_d, tp_d, acp_d, w, phi,
                                               eta=eta, z=zz, clip=clip)
                    for name, got in (("x_prev", xp), ("x0", x0)):
                        r, m, n, ce = ref[name]
                        worst["fused"] = max(worst["fused"], assert_elementwise(
                            got, r, m, n, bf16, ce, what=f"fused {name} {what}"))
                    r, m, n, ce = ref["eps"]
                    worst["eps"] = max(worst["eps"], assert_elementwise(
                        eps_k, r, m, n, bf16, ce, what=f"cfg_combine {what}"))
                    # composed: eps rounded to the dtype between the two kernels (bf16: 2^-8 on
                    # the eps terms; fp32: one more rounding)
                    refc = cases.ref64(xt, c, u, z, t, tp, acp, w, phi, eta, clip,
                                       composed_bf16=bf16)
                    xpc, x0c = ops.ddim_step(xt_d, eps_k, t_d, tp_d, acp_d, eta=eta, z=zz,
                                             clip=clip)
                    for name, got in (("x_prev", xpc), ("x0", x0c)):
                        r, m, n, ce = refc[name]
                        worst["composed"] = max(worst["composed"], assert_elementwise(
                            got, r, m, n + 1, bf16, ce, what=f"composed {name} {what}"))
    print(f"cfg kernels B={B} P={P} {'bf16' if bf16 else 'fp32'}: largest error / bound {worst}")
    record_metric(test="cfg_kernels_fp64", B=B, P=P, dtype="bf16" if bf16 else "fp32", **worst)
    assert all(0 < v <= 1 for v in worst.values()), worst


@pytest.mark.parametrize("B,P", cases.SHAPES)
def test_rescale_factor_is_one_for_equal_halves(B, P):
    """c = u: g = u exactly, both sums of squares take the same adds in the same order, so
    f_b = 1 exactly and full rescale returns u bit for bit."""
    from vdiff import ops
    _, _, u, _ = cases.inputs(B, P, False)
    (u_d,) = _to_dev(False, u)
    assert torch.equal(ops.cfg_combine(u_d.clone(), u_d, 2.5, 1.0), u_d)


@pytest.mark.parametrize("B,P", cases.SHAPES)
def test_constant_guided_noise_is_not_rescaled(B, P):
    """SS(g) = 0 (the all-zero eps of a freshly initialised model; a constant sample): f_b = 1,
    the guided noise unscaled and finite, not the NaN of 0 / 0; the other samples keep their
    factor."""
    from vdiff import ops
    xt, c, u, _ = cases.inputs(B, P, False)
    t, tp = cases.timesteps(B)
    c[0], u[0] = 0.0, 0.0
    c[1], u[1] = 0.5, 0.25  # g = 0.25 + 3 * 0.25 = 1 in every element, exactly
    xt_d, c_d, u_d = _to_dev(False, xt, c, u)
    eps = ops.cfg_combine(c_d, u_d, 3.0, 0.7)
    assert (eps[0] == 0).all() and (eps[1] == 1).all() and torch.isfinite(eps).all()
    if B > 2:
        assert torch.equal(eps[2], ops.cfg_combine(c_d[2:], u_d[2:], 3.0, 0.7)[0])
        assert not torch.equal(eps[2], ops.cfg_combine(c_d[2:], u_d[2:], 3.0, 0.0)[0])
    xp, x0 = ops.ddim_step_cfg(xt_d, c_d, u_d, t.to(dev), tp.to(dev), _acp().to(dev), 3.0, 0.7)
    want = ops.ddim_step_cfg(xt_d, c_d, u_d, t.to(dev), tp.to(dev), _acp().to(dev), 3.0, 0.0)
    assert torch.isfinite(xp).all() and torch.isfinite(x0).all()
    assert torch.equal(xp[:2], want[0][:2]) and torch.equal(x0[:2], want[1][:2])


# ------------------------------------------------------------------ exactness
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,P", cases.SHAPES)
def test_fused_step_exactness(B, P, bf16):
    from vdiff import ops
    xt, c, u, z = cases.inputs(B, P, bf16, seed=1)
    t, tp = cases.timesteps(B)
    xt_d, c_d, u_d, z_d = _to_dev(bf16, xt, c, u, z)
    t_d, tp_d, acp_d = t.to(dev), tp.to(dev), _acp().to(dev)
    kw = dict(eta=0.5, z=z_d, clip=True)
    a = ops.ddim_step_cfg(xt_d, c_d, u_d, t_d, tp_d, acp_d, 2.5, 0.7, **kw)
    b = ops.ddim_step_cfg(xt_d, c_d, u_d, t_d, tp_d, acp_d, 2.5, 0.7, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])  # two launches, the same bits
    assert torch.equal(ops.cfg_combine(c_d, u_d, 2.5, 0.7), ops.cfg_combine(c_d, u_d, 2.5, 0.7))
    out, dup = torch.empty_like(xt_d), torch.empty_like(xt_d)
    xp, x0 = ops.ddim_step_cfg(xt_d, c_d, u_d, t_d, tp_d, acp_d, 2.5, 0.7, out=out, dup=dup,
                               **kw)
    assert xp.data_ptr() == out.data_ptr()
    assert torch.equal(out, a[0]) and torch.equal(dup, out) and torch.equal(x0, a[1])
    alias = xt_d.clone()  # x_prev written over xt
    xp, x0 = ops.ddim_step_cfg(alias, c_d, u_d, t_d, tp_d, acp_d, 2.5, 0.7, out=alias, **kw)
    assert torch.equal(alias, a[0]) and torch.equal(x0, a[1])
    # cond == uncond without rescale: the unguided step, whatever the weight.  g = u exactly
    # and both are instantiations of the one step kernel with the same rule, so the bits agree
    # wherever the compiler fuses the same products.  It does on the 8-wide path, the one every
    # sample shape takes (3 T H W elements).  On the scalar path nothing but the compiler's
    # choice keeps two instantiations alike -- vd_ddim_step's scalar one used to evaluate
    # sqrt(a_p) x0 + dir eps as two rounded products and an add (a packed multiply) where every
    # other one fuses one product, a last-bit difference that only explicit rounding inside
    # the rule could exclude.  There the two results are held to the fp64 bound of each, and to
    # each other: one more rounding of a product, and the (at most two) later roundings of
    # x_prev landing differently, each at most u32 mag: 3 u32 mag in fp32, plus for a bf16
    # output the one ulp by which such a difference can move the final rounding.  (One ulp of
    # the result itself does not hold where sqrt(a_p) x0 and dir eps cancel.)
    want = ops.ddim_step(xt_d, u_d, t_d, tp_d, acp_d, **kw)
    for w in WS:
        got = ops.ddim_step_cfg(xt_d, u_d.clone(), u_d, t_d, tp_d, acp_d, w, 0.0, **kw)
        if P % 8 == 0:
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), w
            continue
        ref = cases.ref64(xt, u, u, z, t, tp, _acp(), 0.0, 0.0, 0.5, True)
        for name, a_, b_ in (("x_prev", got[0], want[0]), ("x0", got[1], want[1])):
            r, m, n, ce = ref[name]
            assert_elementwise(a_, r, m, n, bf16, ce, what=f"c == u fused {name} w={w}")
            assert_elementwise(b_, r, m, n, bf16, ce, what=f"c == u ddim_step {name}")
            a64, b64 = a_.cpu().double(), b_.cpu().double()
            allowed = 3 * cases.U_FP32 * m
            if bf16:  # frexp: |x| = f 2^e, f in [0.5, 1), so a bf16 ulp is 2^(e - 8)
                allowed = allowed + torch.ldexp(
                    torch.ones_like(a64), torch.frexp(torch.maximum(a64.abs(), b64.abs()))[1] - 8)
            far = (a64 - b64).abs() > allowed
            assert not far.any(), (name, w, int(far.sum()), float((a64 - b64).abs().max()))


def test_argument_checks():
    from vdiff import ops
    x = torch.randn(2, 64, device=dev)
    t = torch.tensor([5, 3], device=dev)
    acp = _acp().to(dev)
    with pytest.raises(ValueError):
        ops.cfg_combine(x, x, 2.0, 1.5)
    with pytest.raises(ValueError):
        ops.ddim_step_cfg(x, x, x[:1], t, t - 1, acp, 2.0)
    with pytest.raises(RuntimeError):
        ops.cfg_combine(x.cpu(), x.cpu(), 2.0)


# ------------------------------------------------------------------ samplers
def _model(dims, bf16, dropout=0.1):
    from vdiff.engine import reinit_nonzero
    from vdiff.unet_audio import UNetAudio
    torch.manual_seed(4321)
    m = UNetAudio(image_size=32, in_channels=3, model_channels=32, out_channels=3,
                  num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2),
                  audio_feature_dim=64, projected_audio_dim=32, dims=dims, use_bf16=bf16,
                  audio_encoder=False, dropout=dropout)
    reinit_nonzero(m, seed=4321)
    return m.to(dev)


def _sampling_case(dims):
    from vdiff.schedulers import DDIMSampler, LinearNoiseSchedulerV2
    T = 4 if dims == 3 else 1
    shape = (1, 3, T, 32, 32) if dims == 3 else (1, 3, 32, 32)
    g = torch.Generator(device=dev).manual_seed(77)
    cond = torch.rand((1, 3, 32, 32), device=dev, generator=g) * 2 - 1
    feats = torch.randn((T, 64), device=dev, generator=g)
    sampler = DDIMSampler(LinearNoiseSchedulerV2(500, 0.00005, 0.015), steps=5)
    return shape, cond, feats, sampler


def _sample(m, sampler, cond, feats, shape, seen=None, **kw):
    from vdiff.engine import sample_ddim
    g = torch.Generator(device=dev).manual_seed(9)
    cb = None if seen is None else (lambda i, xt, x0: seen.append((xt, x0)))
    return sample_ddim(m, sampler, cond, feats, shape, generator=g, callback=cb, **kw)


@pytest.mark.parametrize("dims", [3, 2])
def test_guided_ddim_graph_matches_eager(dims, monkeypatch):
    m = _model(dims, True).eval()
    shape, cond, feats, sampler = _sampling_case(dims)
    out, traj = {}, {}
    for mode in ("0", "1"):
        monkeypatch.setenv("VDIFF_DDIM_GRAPH", mode)
        traj[mode] = []
        out[mode] = _sample(m, sampler, cond, feats, shape, traj[mode], guidance_scale=3.0,
                            guidance_rescale=0.7)
    assert len(traj["0"]) == len(traj["1"]) == 5
    for i, ((xa, x0a), (xb, x0b)) in enumerate(zip(traj["0"], traj["1"])):
        assert torch.isfinite(xa).all() and xa.abs().max() > 0
        assert torch.equal(xa, xb) and torch.equal(x0a, x0b), i
    for a, b in zip(out["0"], out["1"]):
        assert torch.equal(a, b)
    assert not torch.equal(traj["1"][0][1], traj["1"][-1][1])


def test_guided_graph_holds_no_memset_node():
    from vdiff import ops
    from vdiff.engine import DDIMGraph
    m = _model(3, True).eval()
    shape, cond, feats, sampler = _sampling_case(3)
    with torch.no_grad(), ops.frozen_weights():
        xt = torch.randn(shape, device=dev)
        gr = DDIMGraph(m, sampler, cond, feats, xt, guidance_scale=3.0, guidance_rescale=0.7)
        gr.capture()
        types = gr.node_types()
        assert types.get("memset", 0) == 0 and types.get("kernel", 0) > 20, types
        # the doubled input stays current: both halves hold the step's x_prev
        got, _ = gr.step(0)
        assert torch.equal(gr.x2[:1], gr.x2[1:]) and got.data_ptr() == gr.x2.data_ptr()
        assert not torch.equal(got, xt)


def test_guidance_scale_semantics(monkeypatch):
    from vdiff.engine import sample_ddim
    m = _model(3, True).eval()
    shape, cond, feats, sampler = _sampling_case(3)
    for mode in ("0", "1"):
        monkeypatch.setenv("VDIFF_DDIM_GRAPH", mode)
        g = torch.Generator(device=dev).manual_seed(9)
        plain = sample_ddim(m, sampler, cond, feats, shape, generator=g)
        w1 = _sample(m, sampler, cond, feats, shape, guidance_scale=1.0)
        assert torch.equal(plain[0], w1[0]) and torch.equal(plain[1], w1[1])
        # the null audio as the condition: cond == uncond, so the weight drops out
        zero = torch.zeros_like(feats)
        w3 = _sample(m, sampler, cond, zero, shape, guidance_scale=3.0)
        w7 = _sample(m, sampler, cond, zero, shape, guidance_scale=7.0)
        assert torch.equal(w3[0], w7[0]) and torch.equal(w3[1], w7[1])
        g3 = _sample(m, sampler, cond, feats, shape, guidance_scale=3.0)
        assert torch.isfinite(g3[0]).all() and not torch.equal(g3[0], w1[0])


def test_guided_ddpm_first_step_against_fp64():
    from vdiff.engine import sample_ddpm
    from vdiff.schedulers import LinearNoiseSchedulerV2
    m = _model(3, True).eval()
    shape, cond, feats, _ = _sampling_case(3)
    sch = LinearNoiseSchedulerV2(500, 0.00005, 0.015)
    halves, steps = [], []
    hook = m.register_forward_hook(lambda mod, args, out: halves.append(out.detach().clone()))
    try:
        g = torch.Generator(device=dev).manual_seed(21)
        xt, x0 = sample_ddpm(m, sch, cond, feats, shape, n_timesteps=4, generator=g,
                             callback=lambda i, x, x0_: steps.append((i, x.clone())),
                             guidance_scale=3.0)
    finally:
        hook.remove()
    assert len(steps) == 4 and len(halves) == 4 and halves[0].shape[0] == 2
    assert torch.isfinite(xt).all() and torch.isfinite(x0).all()
    # the same draws: x_T, then the first step's z
    g = torch.Generator(device=dev).manual_seed(21)
    x_T = torch.randn(shape, generator=g, device=dev).cpu().double()
    z = torch.randn(shape, generator=g, device=dev).cpu().double()
    c, u = (h.cpu().double() for h in halves[0].chunk(2))
    w, i = 3.0, steps[0][0]
    assert i == 3
    eps = u + w * (c - u)
    mag_eps = u.abs() + w * (c.abs() + u.abs())
    s1 = sch.sqrt_one_minus_alpha_cum_prod.double()[i]
    sq_alpha = sch.alphas.double()[i].sqrt()
    sigma = ((1 - sch.alpha_cum_prod.double()[i]) * sch.betas.double()[i]).sqrt()
    ref = x_T - s1 * eps / sq_alpha + sigma * z
    mag = x_T.abs() + s1 * mag_eps / sq_alpha + sigma * z.abs()
    # roundings: eps 2 + its store, s1 eps, sqrt(alpha), the divide, the subtraction, sigma's
    # subtraction / product / square root, the fma: 11
    r = assert_elementwise(steps[0][1], ref, mag, 11, False, what="guided p_sample_v2 x_prev")
    print(f"guided ddpm first step: error / bound {r:.3g}")


# ------------------------------------------------------------------ training
def _clip(B, seed=0):
    from vdiff.engine import Clip
    g = torch.Generator(device=dev).manual_seed(100 + seed)
    T = 2
    x0 = torch.rand((B, 3, T, 32, 32), generator=g, device=dev) * 2 - 1
    cond = torch.rand((B, 3, 32, 32), generator=g, device=dev) * 2 - 1
    eps = torch.randn((B, 3, T, 32, 32), generator=g, device=dev)
    t = torch.randint(0, 100, (B,), generator=g, device=dev)
    feats = torch.randn((B * T, 64), generator=g, device=dev)
    return Clip(x0, cond, feats, eps, t)


def _first_loss(clip, feats=None, **kw):
    """The first step's loss of a freshly built fp32 model (same seeded weights every time)."""
    from vdiff.engine import Clip, Trainer
    from vdiff.schedulers import LinearNoiseScheduler
    m = _model(3, False, dropout=0.0)
    tr = Trainer(m, LinearNoiseScheduler(100, 0.00085, 0.012), lr=1e-3, **kw)
    if feats is not None:
        clip = Clip(clip.x0, clip.cond, feats, clip.eps, clip.t)
    loss = tr.step(clip)
    tr.check_finite()
    return loss.clone()


def test_audio_dropout_training_step():
    from vdiff.engine import audio_keep_mask
    B = 4
    clip = _clip(B)
    other = torch.randn_like(clip.audio) * 3
    zero = torch.zeros_like(clip.audio)
    base = _first_loss(clip)
    # p = 1: the audio never reaches the loss
    a = _first_loss(clip, audio_drop_prob=1.0)
    b = _first_loss(clip, feats=other, audio_drop_prob=1.0)
    assert torch.equal(a, b) and torch.equal(a, _first_loss(clip, feats=zero))
    assert not torch.equal(a, base)
    # p = 0: the step as it was
    assert torch.equal(_first_loss(clip, audio_drop_prob=0.0), base)
    # p = 0.5: the features of the drawn clips zeroed by hand
    keep = audio_keep_mask(B, 0.5, dev, torch.Generator(device=dev).manual_seed(31))
    assert 0 < int(keep.sum()) < B, keep
    hand = clip.audio.clone().view(B, -1, 64)
    hand[keep == 0] = 0
    got = _first_loss(clip, audio_drop_prob=0.5,
                      drop_generator=torch.Generator(device=dev).manual_seed(31))
    assert torch.equal(got, _first_loss(clip, feats=hand.view(-1, 64)))
    assert not torch.equal(got, base) and not torch.equal(got, a)


def test_audio_dropout_reaches_the_graphed_step(monkeypatch):
    """Trainer(graph=True) masks the encoded audio eagerly, before the copy into the graph's
    static buffer: with p = 1 the replayed steps' losses do not depend on the features (two
    eager warm-up steps, then the capture and one replay), with p = 0 they do."""
    from vdiff.engine import Clip, Trainer
    from vdiff.schedulers import LinearNoiseScheduler
    monkeypatch.setenv("VDIFF_TRAIN_GRAPH_EXPERIMENTAL", "1")
    clip = _clip(2)
    other = torch.randn_like(clip.audio) * 3

    def losses(feats, p):
        m = _model(3, False, dropout=0.0)
        tr = Trainer(m, LinearNoiseScheduler(100, 0.00085, 0.012), lr=1e-3, graph=True,
                     audio_drop_prob=p)
        c = Clip(clip.x0, clip.cond, feats, clip.eps, clip.t)
        out = torch.stack([tr.step(c).clone() for _ in range(4)])
        assert tr.graph.g is not None and torch.isfinite(out).all()
        return out

    assert torch.equal(losses(clip.audio, 1.0), losses(other, 1.0))
    assert not torch.equal(losses(clip.audio, 0.0), losses(other, 0.0))


# ------------------------------------------------------------------ entry points
def _run(script, args, cwd):
    out = subprocess.run([sys.executable, os.path.join(DROPIN, script)] + args, cwd=cwd,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.parametrize("sampler", ["ddim", "ddpm-v2"])
def test_sampling_entry_with_guidance(tmp_path, sampler):
    out_dir = tmp_path / "imgs"
    _run("test.py", ["--random-init", "--sampler", sampler, "--steps", "3", "--guidance-scale",
                     "2", "--guidance-rescale", "0.5", "--dims", "3", "--frames", "4",
                     "--image-size", "32", "--save-every", "1", "--out-dir", str(out_dir)],
         tmp_path)
    files = sorted(p for p in os.listdir(out_dir) if p.endswith(".npy"))
    assert files
    x0 = np.load(out_dir / files[0])
    assert x0.shape == (1, 3, 4, 32, 32) and np.isfinite(x0).all()


def test_train_entry_with_audio_dropout(tmp_path):
    ck = str(tmp_path / "m.pth")
    out = _run("train.py", ["--dims", "3", "--frames", "8", "--image-size", "64",
                            "--model-channels", "32", "--channel-mult", "1", "2",
                            "--num-res-blocks", "1", "--attention-resolutions", "2",
                            "--random-audio-encoder", "--batch-size", "2", "--epochs", "1",
                            "--steps-per-epoch", "1", "--audio-drop-prob", "0.5", "--ckpt", ck],
               tmp_path)
    assert "Finished epoch 1" in out and os.path.exists(ck)
