"""use_scale_shift_norm (FiLM time conditioning): ops.group_norm_film_silu against the plain
GroupNorm kernels (zero film = the same bits), its reproducibility and dropout counter, the
FiLM ResBlock / UNetModel / train step against the reference's golden vectors
(tests/golden/film_*.npz, gen_film_golden.py), EmbTable against the per-block embedding, and
the sampling / training graphs of a FiLM model.

The UNet and train-step goldens run the model forward, hence the one-GEMM EmbTable path; the
two ResBlock goldens are called with the embedding tensor itself, hence the per-block
emb_layers path.  test_emb_table_equals_per_block ties the two together.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle.fixtures import TINY3D, TINY3D_SHAPE, rel_l2, seeded
from oracle.unet import audio_param_shapes, init_params

from conftest import golden, record_metric

pytestmark = pytest.mark.gpu
dev = "cuda"

GOLDEN = 0x9E3779B97F4A7C15


def _load(module, seed):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict(init_params(shapes, seed))


# ------------------------------------------------------------------ the op
def _inputs(shape, dtype, seed=0):
    from vdiff import ops
    B, C = shape[:2]
    x = ops.to_cl((seeded(shape, 60 + seed) * 1.5 + 2.0).to(dev, dtype))
    dy = ops.to_cl(seeded(shape, 61 + seed).to(dev, dtype))
    gamma = (1 + 0.3 * seeded((C,), 62)).to(dev)
    beta = (0.3 * seeded((C,), 63)).to(dev)
    return x, dy, gamma, beta


def _run(fn, x, dy, gamma, beta, film=None, **kw):
    xx = x.detach().clone().requires_grad_(True)
    g, b = gamma.detach().clone().requires_grad_(True), beta.detach().clone().requires_grad_(True)
    if film is None:
        y = fn(xx, g, b, 32, 1e-5, True, **kw)
        y.backward(dy)
        return y.detach(), xx.grad, g.grad, b.grad
    f = film.detach().clone().requires_grad_(True)
    y = fn(xx, g, b, f, 32, 1e-5, True, **kw)
    y.backward(dy)
    return y.detach(), xx.grad, g.grad, b.grad, f.grad


@pytest.mark.parametrize("dropout", [0.0, 0.25])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", [(2, 192, 3, 9, 11), (1, 64, 1, 1, 4100)])
def test_zero_film_equals_plain_bit_for_bit(shape, dtype, dropout):
    """film = 0: gamma' = gamma and beta' = beta exactly, and the FiLM kernels evaluate the
    plain kernels' expressions on them -- y, dx, dgamma, dbeta equal group_norm_silu's bits."""
    from vdiff import ops
    x, dy, gamma, beta = _inputs(shape, dtype)
    film = torch.zeros(shape[0], 2 * shape[1], device=dev)
    kw = dict(dropout=dropout, seed=77) if dropout else {}
    plain = _run(ops.group_norm_silu, x, dy, gamma, beta, **kw)
    got = _run(ops.group_norm_film_silu, x, dy, gamma, beta, film, **kw)
    for name, a, b in zip(("y", "dx", "dgamma", "dbeta"), got, plain):
        assert torch.equal(a, b), name
    assert torch.isfinite(got[4]).all() and got[4].abs().max() > 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_backward_is_run_to_run_reproducible(dtype):
    """No atomics, fixed summation order: two backward calls on the same inputs give equal
    bits for dx, dgamma, dbeta, dscale and dshift (129 chunks, ksplit = 3, and B = 2)."""
    from vdiff import ops
    for shape in ((1, 64, 1, 1, 4100), (2, 192, 3, 9, 11)):
        x, dy, gamma, beta = _inputs(shape, dtype)
        B, C = shape[:2]
        film = torch.cat([0.5 * seeded((B, C), 65), 0.5 * seeded((B, C), 66)], 1).to(dev)
        a = _run(ops.group_norm_film_silu, x, dy, gamma, beta, film, dropout=0.1, seed=5)
        b = _run(ops.group_norm_film_silu, x, dy, gamma, beta, film, dropout=0.1, seed=5)
        for name, u, v in zip(("y", "dx", "dgamma", "dbeta", "dfilm"), a, b):
            assert torch.equal(u, v), (shape, name)
        assert a[4].dtype == film.dtype and a[4].shape == film.shape


def test_film_gradient_dtype_and_cpu_raise():
    """film in bf16 is read as fp32 and its gradient returns in bf16; CPU tensors raise."""
    from vdiff import ops
    x, dy, gamma, beta = _inputs((2, 64, 1, 4, 4), torch.bfloat16)
    film = (0.5 * seeded((2, 128), 65)).to(dev).bfloat16()
    out = _run(ops.group_norm_film_silu, x, dy, gamma, beta, film)
    ref = _run(ops.group_norm_film_silu, x, dy, gamma, beta, film.float())
    assert out[4].dtype == torch.bfloat16 and torch.equal(out[0], ref[0])
    assert torch.equal(out[4], ref[4].bfloat16())
    with pytest.raises(RuntimeError):
        ops.group_norm_film_silu(x.cpu(), gamma.cpu(), beta.cpu(), film.cpu())
    with pytest.raises(ValueError):
        ops.group_norm_film_silu(x, gamma, beta, film[:, :64])


def test_dropout_counter_mixes_into_seed():
    """vd_set_dropout_counter: a FiLM launch that reads counter value k equals the launch with
    seed ^ ((k + 1) * 0x9E3779B97F4A7C15) and no counter, forward and backward."""
    from vdiff import _lib, ops
    lib = _lib.lib()
    torch.manual_seed(3)
    x = ops.to_cl(torch.randn(1, 64, 4, 8, 8, device=dev).bfloat16())
    g = torch.randn(64, device=dev, requires_grad=True)
    b = torch.randn(64, device=dev, requires_grad=True)
    film = 0.5 * torch.randn(1, 128, device=dev)
    dy = torch.randn(x.shape, device=dev).bfloat16()

    def run(seed, ctr=None):
        xx = x.detach().clone().requires_grad_(True)
        lib.vd_set_dropout_counter(ctr.data_ptr() if ctr is not None else None)
        try:
            y = ops.group_norm_film_silu(xx, g, b, film, 32, 1e-5, True, dropout=0.1, seed=seed)
            dx, = torch.autograd.grad(y, xx, ops.to_cl(dy))
        finally:
            lib.vd_set_dropout_counter(None)
        return y.detach(), dx

    ctr = torch.full((), 5, dtype=torch.int64, device=dev)
    y1, d1 = run(123, ctr)
    y2, d2 = run(123 ^ ((6 * GOLDEN) % 2 ** 64))
    y0, _ = run(123)
    assert torch.equal(y1, y2) and torch.equal(d1, d2)
    assert not torch.equal(y1, y0)


# ------------------------------------------------------------------ module goldens
def _metric(name, value, bar):
    print(f"film golden {name}: {value:.3g} (bar {bar:g})", flush=True)
    record_metric(test="film_golden", name=name, value=value, bar=bar)
    return value


BLOCK_GRADS = ("in_layers.2.weight", "out_layers.0.weight", "out_layers.0.bias",
               "emb_layers.1.weight", "emb_layers.1.bias", "skip_connection.weight")


@pytest.mark.parametrize("tag", ["rb", "rb2"])
def test_film_resblock_golden(tag):
    """The reference's ResBlock(use_scale_shift_norm=True): 3-D 64 -> 128 with the 1x1x1 skip
    (rb) and 2-D with the identity skip (rb2); rel-L2 < 1e-5, the bar of
    test_resblock3d_golden (the same conv and GroupNorm arithmetic)."""
    from vdiff.nn import ResBlock
    g = golden("film_blocks.npz")
    if tag == "rb":
        rb, shape, seed = ResBlock(64, 256, 0.0, out_channels=128, dims=3,
                                   use_scale_shift_norm=True), (2, 64, 2, 6, 6), 130
    else:
        rb, shape, seed = ResBlock(64, 256, 0.0, dims=2,
                                   use_scale_shift_norm=True), (2, 64, 10, 10), 134
    assert rb.emb_layers[1].out_features == 2 * rb.out_channels
    _load(rb, seed)
    rb = rb.to(dev)
    x = seeded(shape, seed + 1).to(dev).requires_grad_(True)
    emb = seeded((2, 256), seed + 2).to(dev).requires_grad_(True)
    y = rb(x, emb)
    y.backward(seeded(y.shape, seed + 3).to(dev))
    errs = {"y": rel_l2(y, g[f"{tag}_y"]), "dx": rel_l2(x.grad, g[f"{tag}_dx"]),
            "demb": rel_l2(emb.grad, g[f"{tag}_demb"])}
    named = dict(rb.named_parameters())
    for k in BLOCK_GRADS:
        if k in named:
            errs[k] = rel_l2(named[k].grad, g[f"{tag}_d_{k}"])
    assert len(errs) == (9 if tag == "rb" else 8)
    for k, e in errs.items():
        _metric(f"{tag} {k}", e, 1e-5)
    for k, e in errs.items():
        assert e < 1e-5, (k, e)


def _tiny3d(bf16=False):
    from vdiff.nn import UNetModel
    m = UNetModel(image_size=64, **TINY3D, use_scale_shift_norm=True, use_bf16=bf16)
    _load(m, 1234)
    return m.to(dev).eval()


UNET_GRADS = ("input_blocks.0.0.weight", "out.2.weight", "input_blocks.3.1.qkv.weight",
              "middle_block.0.in_layers.0.weight", "output_blocks.0.0.skip_connection.weight",
              "time_embed.0.weight", "middle_block.0.emb_layers.1.weight")


def test_film_tiny3d_unet_golden_fp32():
    """y and seven gradients < 1e-4, the loss < 1e-5 relative (test_tiny3d_unet_golden_fp32)."""
    g = golden("film_unet_tiny3d.npz")
    m = _tiny3d()
    y = m(seeded(TINY3D_SHAPE, 60, "uniform").to(dev), g["t"].to(dev))
    e = _metric("unet fp32 y", rel_l2(y, g["y"]), 1e-4)
    loss = F.mse_loss(y, seeded((1, 3) + TINY3D_SHAPE[2:], 61).to(dev))
    el = _metric("unet fp32 loss", abs(loss.item() - g["loss"].item()) / g["loss"].item(), 1e-5)
    loss.backward()
    named = dict(m.named_parameters())
    eg = {k: _metric(f"unet fp32 grad {k}", rel_l2(named[k].grad, g["grad_" + k]), 1e-4)
          for k in UNET_GRADS}
    assert e < 1e-4, e
    assert el < 1e-5, el
    for k, v in eg.items():
        assert v < 1e-4, (k, v)


def test_film_tiny3d_unet_bf16_tolerance():
    g = golden("film_unet_tiny3d.npz")
    m = _tiny3d(bf16=True)
    y = m(seeded(TINY3D_SHAPE, 60, "uniform").to(dev), g["t"].to(dev))
    assert y.dtype == torch.float32
    e = _metric("unet bf16 y", rel_l2(y, g["y"]), 3e-2)
    assert e < 3e-2, e


def test_emb_table_equals_per_block(monkeypatch):
    """The model forward through EmbTable (one GEMM over the stacked [sum 2 Cout, 256] weights)
    equals the forward with emb_table bypassed (each block's own emb_layers) to fp32 rounding,
    and every emb_layers weight gets its gradient through the stacking."""
    from vdiff import nn as vnn
    m = _tiny3d()
    x = seeded(TINY3D_SHAPE, 60, "uniform").to(dev)
    t = torch.tensor([37], device=dev)
    y_table = m(x, t)
    y_table.square().mean().backward()
    g_table = m.middle_block[0].emb_layers[1].weight.grad.clone()
    m.zero_grad(set_to_none=True)
    monkeypatch.setattr(vnn, "emb_table", lambda model, emb: emb)
    y_block = m(x, t)
    y_block.square().mean().backward()
    g_block = m.middle_block[0].emb_layers[1].weight.grad
    e = _metric("emb table vs per block y", rel_l2(y_table, y_block), 1e-5)
    eg = _metric("emb table vs per block grad", rel_l2(g_table, g_block), 1e-5)
    assert e < 1e-5 and eg < 1e-5, (e, eg)


def _adam_delta_close(delta, delta_ref, grad_ref, lr=1e-2, min_cover=0.9):
    """oracle.fixtures.adam_delta_close with its own mask and bars; only the guard on the share
    of the REFERENCE gradient's elements above the mask's threshold is a parameter."""
    delta, delta_ref, grad_ref = (u.detach().double().cpu() for u in (delta, delta_ref, grad_ref))
    mask = grad_ref.abs() > 1e-2 * grad_ref.pow(2).mean().sqrt()
    assert mask.float().mean() > min_cover
    assert float(delta.abs().max()) <= lr * (1 + 1e-5)
    return float((delta - delta_ref)[mask].abs().max())


def test_film_trainer_step_matches_reference_adam_step():
    """One fp32 Trainer.step of a FiLM UNetAudio against the reference train step's loss,
    gradients and one-step Adam deltas (film_train_step_tiny3d.npz): the assertions of
    test_trainer_step_matches_reference_adam_step.

    adam_delta_close also guards its own mask: more than 90 % of the reference gradient's
    elements must lie above 1e-2 of its RMS.  That is a statement about the stored reference
    gradient alone, and the FiLM reference's time_embed.0.weight gradient has 86.3 % there (the
    plain fixture's: 90.9 %; the columns fed by the near-constant high-index sinusoids are
    small).  For that one parameter the same mask, the same 1e-6 bar on it and the same lr
    bound are applied with the guard at 85 %; the other eight go through the helper as is.
    Measured on an MI355X: loss equal to the last bit, gradients 5.7e-7 .. 1.9e-6."""
    from oracle.fixtures import adam_delta_close, train_step_inputs
    from vdiff.engine import Clip, Trainer
    from vdiff.schedulers import LinearNoiseScheduler
    from vdiff.unet_audio import UNetAudio
    g = golden("film_train_step_tiny3d.npz")
    m = UNetAudio(image_size=64, in_channels=3, model_channels=32, out_channels=3,
                  num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2), dims=3,
                  audio_feature_dim=64, projected_audio_dim=16, im_cond_output_ch=16,
                  dropout=0.0, audio_encoder=False, use_scale_shift_norm=True)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    P = init_params({k: v for k, v in shapes.items() if not k.startswith(("audio_", "cond_"))},
                    1234)
    P.update(init_params(audio_param_shapes(64, 16, im_cond_output_ch=16), 77))
    m.load_state_dict(P)
    m = m.to(dev)
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    x0, cond, feat, eps = (u.to(dev) for u in train_step_inputs())
    tr = Trainer(m, LinearNoiseScheduler(100, 0.00085, 0.012), lr=1e-2)
    grads = {}
    hooks = [p.register_post_accumulate_grad_hook(
        lambda p, n=n: grads.__setitem__(n, p.grad.detach().clone()))
        for n, p in m.named_parameters()]
    loss = tr.step(Clip(x0, cond, feat, eps, g["t"].to(dev)))
    for h in hooks:
        h.remove()
    _metric("train step loss", abs(float(loss) - float(g["loss"])) / float(g["loss"]), 1e-5)
    assert abs(float(loss) - float(g["loss"])) < 1e-5 * float(g["loss"])
    named = dict(m.named_parameters())
    keys = [k[len("delta_"):] for k in g if k.startswith("delta_")]
    assert len(keys) == 9
    for k in keys:
        _metric(f"train step grad {k}", rel_l2(grads[k], g["grad_" + k]), 1e-4)
    for k in keys:
        assert rel_l2(grads[k], g["grad_" + k]) < 1e-4, k
        d = named[k].detach() - before[k]
        if k == "time_embed.0.weight":
            dev_ = _adam_delta_close(d, g["delta_" + k], g["grad_" + k], min_cover=0.85)
        else:
            dev_ = adam_delta_close(d, g["delta_" + k], g["grad_" + k])
        _metric(f"train step delta {k}", dev_, 1e-6)
        assert dev_ < 1e-6, k


# ------------------------------------------------------------------ graphs
def _audio_model(dims, bf16, dropout=0.0):
    from vdiff.engine import reinit_nonzero
    from vdiff.unet_audio import UNetAudio
    torch.manual_seed(4321)
    m = UNetAudio(image_size=32, in_channels=3, model_channels=32, out_channels=3,
                  num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2),
                  audio_feature_dim=64, projected_audio_dim=32, dims=dims, use_bf16=bf16,
                  audio_encoder=False, use_scale_shift_norm=True, dropout=dropout)
    reinit_nonzero(m, seed=4321)
    return m.to(dev)


@pytest.mark.parametrize("dims,bf16", [(3, True), (3, False), (2, True)])
def test_film_ddim_graph_matches_eager(dims, bf16, monkeypatch):
    """sample_ddim over 4 steps replayed from DDIMGraph equals the eager loop bit for bit, and
    the captured step raises no GraphUnsafe (it holds no memset node)."""
    from vdiff import ops
    from vdiff.engine import DDIMGraph, sample_ddim
    from vdiff.schedulers import DDIMSampler, LinearNoiseSchedulerV2
    m = _audio_model(dims, bf16).eval()
    T = 4 if dims == 3 else 1
    shape = (1, 3, T, 32, 32) if dims == 3 else (1, 3, 32, 32)
    cond = torch.rand((1, 3, 32, 32), device=dev) * 2 - 1
    feats = torch.randn((T, 64), device=dev)
    sampler = DDIMSampler(LinearNoiseSchedulerV2(500, 0.00005, 0.015), steps=4)
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("VDIFF_DDIM_GRAPH", mode)
        g = torch.Generator(device=dev).manual_seed(9)
        out[mode] = sample_ddim(m, sampler, cond, feats, shape, generator=g)
    for a, b in zip(out["0"], out["1"]):
        assert torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b)
    with torch.no_grad(), ops.frozen_weights():
        gr = DDIMGraph(m, sampler, cond, feats, torch.randn(shape, device=dev))
        gr.capture()  # raises GraphUnsafe on a memset node
        types = gr.node_types()
    assert types.get("memset", 0) == 0 and types.get("kernel", 0) > 20, types


def test_film_graph_replays_draw_new_dropout_masks(monkeypatch):
    """A FiLM model with dropout 0.1 in the train-step graph at lr 0: the same clip replayed
    twice gives two different losses (test_graph_replays_draw_new_dropout_masks's check)."""
    from vdiff.engine import Clip, Trainer
    from vdiff.schedulers import LinearNoiseScheduler
    monkeypatch.setenv("VDIFF_TRAIN_GRAPH_EXPERIMENTAL", "1")
    m = _audio_model(3, False, dropout=0.1)
    gen = torch.Generator(device=dev).manual_seed(100)
    x0 = torch.rand((1, 3, 4, 32, 32), generator=gen, device=dev) * 2 - 1
    cond = torch.rand((1, 3, 32, 32), generator=gen, device=dev) * 2 - 1
    a = torch.randn((4, 64), generator=gen, device=dev)
    eps = torch.randn(x0.shape, generator=gen, device=dev)
    c = Clip(x0, cond, a, eps, torch.tensor([3], device=dev))
    tr = Trainer(m, LinearNoiseScheduler(100, 0.00085, 0.012), lr=0.0, graph=True)
    losses = [float(tr.step(c)) for _ in range(5)]
    assert tr.graph.g is not None
    assert abs(losses[4] - losses[3]) > 1e-6 * abs(losses[3]), losses
