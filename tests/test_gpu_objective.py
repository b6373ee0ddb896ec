"""v-prediction and Min-SNR weighting on the GPU: vd_diffusion_loss / _bwd against fp64 with
element-wise bounds (tests/_objective_cases.py derives them), the same bits eager and replayed
from a HIP graph, the clamped timestep, the prediction-aware DDIM entry points, DPM-Solver++ on
v rows, the three samplers with prediction="v", the Trainer and the entry points."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import DROPIN, record_metric

import _cfg_cases as cfg
import _dpm_cases as dpm
import _objective_cases as cases
from _bounds import U_FP32, assert_elementwise, bound

pytestmark = pytest.mark.gpu
dev = "cuda"


def _to_dev(bf16, *xs):
    dt = torch.bfloat16 if bf16 else torch.float32
    return tuple(x.to(device=dev, dtype=dt).contiguous() for x in xs)


def _tables_dev():
    sa, s1m = cases.tables()
    return sa, s1m, sa.to(dev), s1m.to(dev)


def _check(got, ref, name, bf16, what):
    r, m, n, ce = ref[name]
    return assert_elementwise(got, r, m, n, bf16, ce, what=f"{name} {what}")


# ------------------------------------------------------------------ loss and gradient
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,P", cases.SHAPES)
def test_loss_and_gradient_against_fp64(B, P, bf16):
    from vdiff import ops
    sa, s1m, sa_d, s1m_d = _tables_dev()
    t = cases.timesteps(B, sa.numel())
    assert len(set(t.tolist())) == B and 0 in t and sa.numel() - 1 in t
    pred, x0, eps = cases.inputs(B, P, bf16)
    pred_d, x0_d, eps_d = _to_dev(bf16, pred, x0, eps)
    t_d = t.to(dev)
    g = 2.5  # the incoming gradient, exact in fp32
    worst = 0.0
    for prediction in cases.PREDICTIONS:
        for weighting in cases.WEIGHTINGS:
            what = f"B={B} P={P} bf16={bf16} {prediction} {weighting}"
            ref = cases.ref64(pred, x0, eps, t, sa, s1m, prediction, weighting, cases.GAMMA, g)
            p = pred_d.clone().requires_grad_(True)
            loss, per = ops.diffusion_loss(p, x0_d, eps_d, t_d, sa_d, s1m_d, prediction,
                                           weighting, cases.GAMMA, return_per_sample=True)
            (g * loss).backward()
            assert loss.dtype == torch.float32 and loss.dim() == 0
            assert per.dtype == torch.float32 and per.shape == (B,) and not per.requires_grad
            assert p.grad.dtype == p.dtype and p.grad.shape == p.shape
            for name, got, out_bf16 in (("loss", loss.detach(), False), ("per_sample", per, False),
                                        ("grad", p.grad, bf16)):
                r, m, n = ref[name]
                ratio = assert_elementwise(got, r, m, n, out_bf16, what=f"{name} {what}")
                print(f"{name} {what}: error / bound {ratio:.3g} (n_terms {n})")
                worst = max(worst, ratio)
            only = ops.diffusion_loss(pred_d, x0_d, eps_d, t_d, sa_d, s1m_d, prediction,
                                      weighting, cases.GAMMA)
            assert torch.equal(only, loss.detach()), what
    record_metric(test="diffusion_loss_fp64", B=B, P=P, dtype="bf16" if bf16 else "fp32",
                  worst=worst)
    assert 0 < worst <= 1


def test_default_objective_is_the_plain_mse():
    """eps with no weighting is the mean squared error: the per-sample values average to the
    loss, and the loss lies inside the same fp64 bound as a reference on (pred, eps) alone."""
    from vdiff import ops
    sa, s1m, sa_d, s1m_d = _tables_dev()
    B, P = 3, 768
    pred, x0, eps = cases.inputs(B, P, False)
    pred_d, x0_d, eps_d = _to_dev(False, pred, x0, eps)
    t_d = cases.timesteps(B, sa.numel()).to(dev)
    loss, per = ops.diffusion_loss(pred_d, x0_d, eps_d, t_d, sa_d, s1m_d,
                                   return_per_sample=True)
    ref = ((pred.double() - eps.double()) ** 2).mean()
    mag = ((pred.double().abs() + eps.double().abs()) ** 2).mean()
    assert_elementwise(loss, ref, mag, cases.n_loss(B, P), False, what="mse")
    # x0 is not read for eps: a buffer of NaN changes nothing
    nan = torch.full_like(x0_d, float("nan"))
    again = ops.diffusion_loss(pred_d, nan, eps_d, t_d, sa_d, s1m_d)
    assert torch.equal(again, loss)


# ------------------------------------------------------------------ same bits
def _fresh(B, P, bf16, seed):
    return _to_dev(bf16, *cases.inputs(B, P, bf16, seed))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_same_bits_eager_and_replayed(bf16):
    from vdiff import hipgraph, ops
    sa, s1m, sa_d, s1m_d = _tables_dev()
    B, P = 2, 5000
    T = sa.numel()
    ts = [torch.tensor(v, device=dev) for v in ([T - 1, 0], [3, 250], [499, 498], [0, 17])]

    def run(p, x, e, t):
        p = p.detach().requires_grad_(True)
        loss, per = ops.diffusion_loss(p, x, e, t, sa_d, s1m_d, "v", "min-snr", cases.GAMMA,
                                       return_per_sample=True)
        (grad,) = torch.autograd.grad(loss, p)
        return loss.detach(), per, grad

    first = run(*_fresh(B, P, bf16, 0), ts[0])
    second = run(*_fresh(B, P, bf16, 0), ts[0])
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    # captured: static inputs, the forward and the backward inside the graph
    sp, sx, se = _fresh(B, P, bf16, 0)
    st = ts[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(sp, sx, se, st)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with hipgraph.capture(g, capture_error_mode="thread_local"):
        out = run(sp, sx, se, st)
    g.instantiate()
    counts = hipgraph.node_counts(g)
    assert counts.get("memset", 0) == 0 and counts.get("kernel", 0) >= 3, counts
    seen = []
    for k in (1, 2, 3):
        p, x, e = _fresh(B, P, bf16, k)
        for dst, src in ((sp, p), (sx, x), (se, e), (st, ts[k])):
            dst.copy_(src)
        g.replay()
        want = run(p, x, e, ts[k])
        for a, b in zip(out, want):
            assert torch.equal(a, b), k
        seen.append(float(out[0]))
    assert len(set(seen)) == 3, seen


def test_out_of_range_timestep_is_clamped():
    from vdiff import ops
    sa, s1m, sa_d, s1m_d = _tables_dev()
    T = sa.numel()
    B, P = 2, 105
    p, x, e = _fresh(B, P, False, 0)
    t = torch.zeros(B, dtype=torch.int64, device=dev)

    def run():
        pr = p.clone().requires_grad_(True)
        loss, per = ops.diffusion_loss(pr, x, e, t, sa_d, s1m_d, "v", "min-snr", cases.GAMMA,
                                       return_per_sample=True)
        loss.backward()
        return loss.detach(), per, pr.grad

    for values, clamped in (([-7, T], [0, T - 1]), ([1 << 40, -(1 << 40)], [T - 1, 0]),
                            ([T - 1, T + 5], [T - 1, T - 1])):
        t.copy_(torch.tensor(clamped))
        want = run()
        t.copy_(torch.tensor(values))
        got = run()
        for a, b in zip(got, want):
            assert torch.isfinite(a).all() and torch.equal(a, b), values


def test_argument_checks():
    from vdiff import ops
    sa, s1m, sa_d, s1m_d = _tables_dev()
    x = torch.randn(2, 64, device=dev)
    t = torch.zeros(2, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        ops.diffusion_loss(x, x, x, t, sa_d, s1m_d, "x0")
    with pytest.raises(ValueError):
        ops.diffusion_loss(x, x, x, t, sa_d, s1m_d, "v", "p2")
    for gamma in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ops.diffusion_loss(x, x, x, t, sa_d, s1m_d, "v", "min-snr", gamma)
    with pytest.raises(ValueError):
        ops.diffusion_loss(x, x[:1], x, t, sa_d, s1m_d)
    with pytest.raises(ValueError):
        ops.diffusion_loss(x, x, x, t[:1].expand(3), sa_d, s1m_d)
    with pytest.raises(ValueError):
        ops.diffusion_loss(x, x, x, t, sa_d.double(), s1m_d)
    with pytest.raises(RuntimeError):
        ops.diffusion_loss(x, x, x, t, sa, s1m_d)
    with pytest.raises(ValueError):
        ops.ddim_step(x, x, t, t, sa_d, prediction="x0")


# ------------------------------------------------------------------ DDIM
def _old_ddim(xt, eps, t, tp, acp, clip):
    """vd_ddim_step, the entry point as it was, called directly."""
    from vdiff import _lib, ops
    xp, x0 = torch.empty_like(xt), torch.empty_like(xt)
    B = xt.shape[0]
    _lib.call("vd_ddim_step", xt.data_ptr(), eps.data_ptr(), None, xp.data_ptr(), x0.data_ptr(),
              t.data_ptr(), tp.data_ptr(), acp.data_ptr(), 0.0, int(clip), B, xt.numel() // B,
              ops._dtype(xt), ops._stream(xt))
    return xp, x0


def _old_ddim_cfg(xt, c, u, t, tp, acp, w, phi, clip):
    from vdiff import _lib, ops
    xp, x0 = torch.empty_like(xt), torch.empty_like(xt)
    B = xt.shape[0]
    P = xt.numel() // B
    ws = None
    if phi > 0:
        nws = _lib.lib().vd_cfg_workspace_size(B, P)
        ws = torch.empty(nws, dtype=torch.uint8, device=xt.device)
        _lib.call("vd_cfg_stats", c.data_ptr(), u.data_ptr(), float(w), B, P, ops._dtype(xt),
                  ws.data_ptr(), nws, ops._stream(xt))
    _lib.call("vd_ddim_step_cfg", xt.data_ptr(), c.data_ptr(), u.data_ptr(), None, xp.data_ptr(),
              None, x0.data_ptr(), t.data_ptr(), tp.data_ptr(), acp.data_ptr(), float(w),
              float(phi), None if ws is None else ws.data_ptr(), 0.0, int(clip), B, P,
              ops._dtype(xt), ops._stream(xt))
    return xp, x0


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,P", cases.SHAPES)
def test_ddim_eps_is_the_old_entry_point(B, P, bf16):
    from vdiff import ops
    acp = dpm.schedules()["v2"].to(dev)
    xt, c, u, _ = cfg.inputs(B, P, bf16)
    xt_d, c_d, u_d = _to_dev(bf16, xt, c, u)
    t, tp = (v.to(dev) for v in cfg.timesteps(B))
    for clip in (False, True):
        new = ops.ddim_step(xt_d, c_d, t, tp, acp, clip=clip, prediction="eps")
        old = _old_ddim(xt_d, c_d, t, tp, acp, clip)
        assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1]), (B, P, clip)
        for w, phi in ((2.5, 0.0), (7.5, 0.7)):
            new = ops.ddim_step_cfg(xt_d, c_d, u_d, t, tp, acp, w, phi, clip=clip,
                                    prediction="eps")
            old = _old_ddim_cfg(xt_d, c_d, u_d, t, tp, acp, w, phi, clip)
            assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1]), (B, P, w, phi)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,P", cases.SHAPES)
def test_ddim_v_against_fp64(B, P, bf16):
    from vdiff import ops
    acp = dpm.schedules()["v2"]
    acp_d = acp.to(dev)
    xt, c, u, z = cfg.inputs(B, P, bf16)
    xt_d, c_d, u_d, z_d = _to_dev(bf16, xt, c, u, z)
    t, tp = cfg.timesteps(B)
    t_d, tp_d = t.to(dev), tp.to(dev)
    worst = 0.0
    for clip in (False, True):
        for eta in (0.0, 0.5):
            what = f"B={B} P={P} bf16={bf16} clip={clip} eta={eta}"
            zz = z_d if eta > 0 else None
            ref = cases.ddim_ref64(xt, c, u, z, t, tp, acp, 0.0, 0.0, eta, clip, guided=False)
            xp, x0 = ops.ddim_step(xt_d, c_d, t_d, tp_d, acp_d, eta=eta, z=zz, clip=clip,
                                   prediction="v")
            worst = max(worst, _check(xp, ref, "x_prev", bf16, what),
                        _check(x0, ref, "x0", bf16, what))
            for w, phi in ((2.5, 0.0), (7.5, 0.7)):
                ref = cases.ddim_ref64(xt, c, u, z, t, tp, acp, w, phi, eta, clip, guided=True)
                dup = torch.empty_like(xt_d)
                xp, x0 = ops.ddim_step_cfg(xt_d, c_d, u_d, t_d, tp_d, acp_d, w, phi, eta=eta,
                                           z=zz, clip=clip, dup=dup, prediction="v")
                assert torch.equal(dup, xp)
                worst = max(worst, _check(xp, ref, "x_prev", bf16, f"guided w={w} {what}"),
                            _check(x0, ref, "x0", bf16, f"guided w={w} {what}"))
    print(f"ddim v B={B} P={P} {'bf16' if bf16 else 'fp32'}: largest error / bound {worst:.3g}")
    record_metric(test="ddim_v_fp64", B=B, P=P, dtype="bf16" if bf16 else "fp32", worst=worst)
    assert 0 < worst <= 1


# ------------------------------------------------------------------ DPM-Solver++ on v rows
def _dpm_sampler(**kw):
    from vdiff.schedulers import DPMSolverSampler
    kw.setdefault("steps", 8)
    return DPMSolverSampler(dpm.v2_scheduler(), **kw)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,P", cases.SHAPES)
def test_dpm_step_on_v_rows_against_fp64(B, P, bf16):
    """vd_dpm_step / vd_dpm_step_cfg read the v sampler's rows [1 / alpha, sigma / alpha, A, B,
    C]: the kernel's own expression on its own fp32 row, so _dpm_cases.ref64 and its counts
    apply as they stand, with the model's v in eps's place."""
    from vdiff import ops
    s = _dpm_sampler(prediction="v")
    coef, idx = s._tables(dev)
    xt, c, u, last = dpm.inputs(B, P, bf16)
    xt_d, c_d, u_d, last_d = _to_dev(bf16, xt, c, u, last)
    worst = 0.0
    for i in dpm.kernel_rows(s):
        for clip in (False, True):
            what = f"B={B} P={P} bf16={bf16} row={i} clip={clip}"
            ref = dpm.ref64(xt, c, last, s.coef[i], clip)
            xp, x0 = ops.dpm_step(xt_d, c_d, last_d.clone(), coef, idx[i:i + 1], clip=clip)
            worst = max(worst, _check(xp, ref, "x_prev", bf16, what),
                        _check(x0, ref, "x0", bf16, what))
            ref = dpm.ref64(xt, c, last, s.coef[i], clip, guide=(u, 2.5, 0.7))
            xp, x0 = ops.dpm_step_cfg(xt_d, c_d, u_d, last_d.clone(), coef, idx[i:i + 1], 2.5,
                                      0.7, clip=clip)
            worst = max(worst, _check(xp, ref, "x_prev", bf16, "guided " + what),
                        _check(x0, ref, "x0", bf16, "guided " + what))
    # and the row is what makes it v: x0 = alpha xt - sigma v in fp64, to the same bound
    i = dpm.kernel_rows(s)[1]
    al, sg = (float(v) for v in _dpm_sampler().coef64[i, :2])
    _, x0 = ops.dpm_step(xt_d, c_d, last_d.clone(), coef, idx[i:i + 1])
    r, m, n, ce = dpm.ref64(xt, c, last, s.coef[i], False)["x0"]
    want = al * xt.double() - sg * c.double()
    # + the two row entries' own rounding from fp64 (one each)
    assert_elementwise(x0, want, m, n + 2, bf16, ce, what="x0 = alpha xt - sigma v")
    record_metric(test="dpm_v_rows_fp64", B=B, P=P, dtype="bf16" if bf16 else "fp32",
                  worst=worst)
    assert 0 < worst <= 1


# ------------------------------------------------------------------ samplers, graph and eager
def _model(dims, bf16):
    from vdiff.engine import reinit_nonzero
    from vdiff.unet_audio import UNetAudio
    torch.manual_seed(4321)
    m = UNetAudio(image_size=32, in_channels=3, model_channels=32, out_channels=3,
                  num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2),
                  audio_feature_dim=64, projected_audio_dim=32, dims=dims, use_bf16=bf16,
                  audio_encoder=False)
    reinit_nonzero(m, seed=4321)
    return m.to(dev).eval()


def _sampling_case(dims):
    T = 4 if dims == 3 else 1
    shape = (1, 3, T, 32, 32) if dims == 3 else (1, 3, 32, 32)
    g = torch.Generator(device=dev).manual_seed(77)
    cond = torch.rand((1, 3, 32, 32), device=dev, generator=g) * 2 - 1
    feats = torch.randn((T, 64), device=dev, generator=g)
    return shape, cond, feats


@pytest.fixture(scope="module")
def tiny_model():
    return _model(3, True)


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_v_sampling_graph_matches_eager(which, guided, tiny_model, monkeypatch):
    """The rule of test_gpu_dpm.py::test_dpm_graph_matches_eager: the replayed graph and the
    eager loop launch the same kernels on the same operands, so every step's x_prev and x0 are
    the same bits -- and they are not the eps sampler's."""
    from vdiff.engine import sample_ddim, sample_dpm
    from vdiff.schedulers import DDIMSampler
    shape, cond, feats = _sampling_case(3)
    if which == "dpm":
        sampler, other, sample = _dpm_sampler(steps=6, prediction="v"), _dpm_sampler(steps=6), \
            sample_dpm
    else:
        sampler = DDIMSampler(dpm.v2_scheduler(), steps=6, prediction="v")
        other, sample = DDIMSampler(dpm.v2_scheduler(), steps=6), sample_ddim
    assert sampler.prediction == "v" and other.prediction == "eps" and sampler.steps == 6
    kw = dict(guidance_scale=3.0, guidance_rescale=0.7) if guided else {}
    out, traj = {}, {}
    for mode in ("0", "1"):
        monkeypatch.setenv("VDIFF_DDIM_GRAPH", mode)
        g = torch.Generator(device=dev).manual_seed(9)
        seen = traj[mode] = []
        out[mode] = sample(tiny_model, sampler, cond, feats, shape, generator=g,
                           callback=lambda i, xt, x0: seen.append((xt, x0)), **kw)
    for a, b in zip(out["0"], out["1"]):
        assert torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b)
    assert len(traj["0"]) == len(traj["1"]) == 6
    for i, ((xa, x0a), (xb, x0b)) in enumerate(zip(traj["0"], traj["1"])):
        assert torch.equal(xa, xb) and torch.equal(x0a, x0b), i
    g = torch.Generator(device=dev).manual_seed(9)
    eps_out = sample(tiny_model, other, cond, feats, shape, generator=g, **kw)
    assert not torch.equal(eps_out[1], out["1"][1])


@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_v_sampling_graph_holds_no_memset_node(which, tiny_model):
    from vdiff import ops
    from vdiff.engine import DDIMGraph, DPMGraph
    from vdiff.schedulers import DDIMSampler
    shape, cond, feats = _sampling_case(3)
    if which == "dpm":
        sampler, Graph = _dpm_sampler(steps=6, prediction="v"), DPMGraph
    else:
        sampler, Graph = DDIMSampler(dpm.v2_scheduler(), steps=6, prediction="v"), DDIMGraph
    with torch.no_grad(), ops.frozen_weights():
        xt = torch.randn(shape, device=dev)
        gr = Graph(tiny_model, sampler, cond, feats, xt, guidance_scale=3.0,
                   guidance_rescale=0.7)
        gr.capture()
        types = gr.node_types()
        assert types.get("memset", 0) == 0 and types.get("kernel", 0) > 20, types
        got, x0 = gr.step(0)
        assert torch.isfinite(got).all() and torch.isfinite(x0).all()


# ------------------------------------------------------------------ ancestral sampling with v
class GaussModel(torch.nn.Module):
    """The optimal prediction for data N(0, s^2) (the GaussEps pattern of test_gpu_dpm.py): out =
    c_t x from one fp32 table (rounded once from fp64) and one rounded product; c_t =
    _objective_cases.gauss_coefs(a_t, s)[0] for eps*, [1] for v*."""

    def __init__(self, acp, s, pick):
        super().__init__()
        tab = [cases.gauss_coefs(float(a), s)[pick] for a in acp.double()]
        self.register_buffer("c", torch.tensor(tab, dtype=torch.float64).float())

    def forward(self, x, cond, feats, t):
        return self.c[t].view(-1, *([1] * (x.dim() - 1))) * x


def _ddpm_bound(x_T, zs, sch, n, s):
    """(bound on |x_prev_v - x_prev_eps|, bound on |x0_v - x0_eps|) after sample_ddpm's n steps
    (t = n - 1 .. 0) of LinearNoiseSchedulerV2 on the Gaussian model, per element in fp64.

    Both paths run the same p_sample_v2 kernel with the same coefficients on the same x_T and
    z; they differ in the noise they feed it.  eps path: eps = c x, the table's rounding and the
    product: 2 roundings of |c x|.  v path: eps = s1m x + sa v, v = c_v x: the conversion's 3
    roundings (two products, the sum) on top of what its operands carry -- s1m x: the fp32
    table's own 2 (1 - a, the sqrt); sa v: the table's 2 (the sqrt of a product) and v's 2 -- 6
    + 3 = 9 on mag_eps = s1m |x| + sa |c_v x|.  In exact arithmetic the two are equal (s1m + sa
    c_v = c).  So per step, with d the difference of the two x:
        d' <= |1 - k c| d + k D_eps + 2 local,   k = s1m / sqrt(alpha_t),
    D_eps = 2 (2 + 2) u32 |c x| + 2 (9 + 2) u32 mag_eps, local = 2 (4 + 2) u32 (|x| + k |eps| +
    sigma |z|): the kernel's data-dependent roundings (product, divide, subtraction, fused
    multiply-add), once per path; its coefficient roundings are common to both.  x0 =
    clamp((x - s1m eps) / sa): |1 - s1m c| / sa d + (s1m / sa) D_eps + 2 * 2 (3 + 2) u32 mag_x0;
    the clamp moves no value further apart."""
    a = sch.alpha_cum_prod.double()
    s1m = sch.sqrt_one_minus_alpha_cum_prod.double()
    sa = sch.sqrt_alpha_cum_prod.double()
    alphas, betas = sch.alphas.double(), sch.betas.double()
    x = x_T.detach().cpu().double()
    d = torch.zeros_like(x)
    d0 = None
    for j, t in enumerate(reversed(range(n))):
        ce, cv = cases.gauss_coefs(float(a[t]), s)
        k = float(s1m[t]) / math.sqrt(float(alphas[t]))
        sigma = math.sqrt((1 - float(a[t])) * float(betas[t]))
        z = zs[j].detach().cpu().double()
        eps = ce * x
        mag_eps = float(s1m[t]) * x.abs() + float(sa[t]) * abs(cv) * x.abs()
        D = bound(torch.zeros_like(x), eps.abs(), 2, False) \
            + bound(torch.zeros_like(x), mag_eps, 9, False)
        local = bound(torch.zeros_like(x), x.abs() + k * eps.abs() + sigma * z.abs(), 4, False)
        mag_x0 = (x.abs() + float(s1m[t]) * eps.abs()) / float(sa[t])
        d0 = abs(1 - float(s1m[t]) * ce) / float(sa[t]) * d + float(s1m[t]) / float(sa[t]) * D \
            + 2 * bound(torch.zeros_like(x), mag_x0, 3, False)
        d = abs(1 - k * ce) * d + k * D + 2 * local
        x = x - k * eps + sigma * z
    return d, d0


def test_sample_ddpm_v_matches_the_eps_path():
    from vdiff.engine import sample_ddpm
    sch = dpm.v2_scheduler()
    acp = sch.alpha_cum_prod.float()
    # the whole schedule: at the low-noise end alone the noise term is below x's last bit and
    # the two paths agree exactly, which would show nothing
    s, n = 0.5, sch.num_timesteps
    shape = (2, 3, 8, 8)
    cond = torch.zeros((2, 3, 8, 8), device=dev)
    out = {}
    for prediction, pick in (("eps", 0), ("v", 1)):
        model = GaussModel(acp, s, pick).to(dev)
        g = torch.Generator(device=dev).manual_seed(5)
        out[prediction] = sample_ddpm(model, sch, cond, None, shape, n_timesteps=n, generator=g,
                                      prediction=prediction)
    g = torch.Generator(device=dev).manual_seed(5)  # the draws sample_ddpm made, in its order
    x_T = torch.randn(shape, generator=g, device=dev)
    zs = [torch.randn(shape, generator=g, device=dev) for _ in range(n)]
    d, d0 = _ddpm_bound(x_T, zs, sch, n, s)
    for name, k, bnd in (("x_prev", 0, d), ("x0", 1, d0)):
        a, b = out["v"][k].cpu().double(), out["eps"][k].cpu().double()
        assert torch.isfinite(a).all() and a.abs().max() > 0
        ratio = float(((a - b).abs() / bnd).max())
        print(f"sample_ddpm v vs eps, {name}: largest difference / bound {ratio:.3g}")
        record_metric(test="ddpm_v_vs_eps", output=name, ratio=ratio)
        assert 0 < ratio <= 1, name
    with pytest.raises(ValueError):
        sample_ddpm(model, sch, cond, None, shape, n_timesteps=1, prediction="x0")


# ------------------------------------------------------------------ Trainer
class Stub(torch.nn.Module):
    """pred = s xt, one learnable scalar, pure torch."""

    def __init__(self):
        super().__init__()
        self.s = torch.nn.Parameter(torch.tensor(0.75))

    def forward(self, xt, cond, audio, t):
        return self.s * xt


def _stub_clip(T):
    from vdiff.engine import Clip
    g = torch.Generator(device=dev).manual_seed(3)
    x0 = torch.rand((3, 3, 4, 8, 8), generator=g, device=dev) * 2 - 1
    eps = torch.randn(x0.shape, generator=g, device=dev)
    t = torch.tensor([0, T // 2, T - 1], device=dev)
    return Clip(x0, x0[:, :, 0].contiguous(), {}, eps, t)


def test_trainer_objective_step():
    from vdiff import ops
    from vdiff.engine import Trainer
    from vdiff.schedulers import LinearNoiseScheduler
    sch = LinearNoiseScheduler(100, 0.00085, 0.012)
    clip = _stub_clip(100)
    m = Stub().to(dev)
    tr = Trainer(m, sch, lr=1e-3, batch_pack=False, prediction="v", loss_weighting="min-snr",
                 snr_gamma=5.0)
    assert tr.loss_per_sample is None
    with torch.no_grad():
        pred = m.s * sch.add_noise(clip.x0, clip.eps, clip.t)
    sa = sch.sqrt_alpha_cum_prod.float().to(dev)
    s1m = sch.sqrt_one_minus_alpha_cum_prod.float().to(dev)
    want, per = ops.diffusion_loss(pred, clip.x0, clip.eps, clip.t, sa, s1m, "v", "min-snr", 5.0,
                                   return_per_sample=True)
    before = float(m.s.detach())
    loss = tr.step(clip)
    assert torch.equal(loss, want) and torch.isfinite(loss) and float(loss) > 0
    assert tr.loss_per_sample.shape == (3,) and torch.equal(tr.loss_per_sample, per)
    assert not tr.loss_per_sample.requires_grad
    assert float(m.s.detach()) != before  # the gradient reached the parameter
    tr.check_finite()


def test_trainer_defaults_never_call_the_objective(monkeypatch):
    from vdiff import ops
    from vdiff.engine import Trainer
    from vdiff.schedulers import LinearNoiseScheduler
    calls = {"objective": 0, "mse": 0}
    real_obj, real_mse = ops.diffusion_loss, ops.mse_loss

    def counted_obj(*a, **k):
        calls["objective"] += 1
        return real_obj(*a, **k)

    def counted_mse(*a, **k):
        calls["mse"] += 1
        return real_mse(*a, **k)

    monkeypatch.setattr(ops, "diffusion_loss", counted_obj)
    monkeypatch.setattr(ops, "mse_loss", counted_mse)
    sch = LinearNoiseScheduler(100, 0.00085, 0.012)
    clip = _stub_clip(100)
    tr = Trainer(Stub().to(dev), sch, lr=1e-3, batch_pack=False)
    for _ in range(2):
        loss = tr.step(clip)
    assert calls == {"objective": 0, "mse": 2} and tr.loss_per_sample is None
    assert torch.isfinite(loss)
    tv = Trainer(Stub().to(dev), sch, lr=1e-3, batch_pack=False, prediction="v")
    tv.step(clip)
    assert calls == {"objective": 1, "mse": 2}


def test_trainer_graph_objective_equals_eager(monkeypatch):
    """Trainer(graph=True) with the objective inside the captured step (two eager warm-up steps,
    the capture, three replays on fresh clips) against the eager trainer on a twin model: the
    same loss and per-sample bits every step, and no memset node in the captured step."""
    import test_gpu_clip as t
    from vdiff.engine import Trainer
    monkeypatch.setenv("VDIFF_TRAIN_GRAPH_EXPERIMENTAL", "1")
    kw = dict(lr=1e-3, prediction="v", loss_weighting="min-snr", snr_gamma=5.0, check_every=100)
    te = Trainer(t._model(), t._sched(), **kw)
    tg = Trainer(t._model(), t._sched(), graph=True, **kw)
    losses = []
    for s in range(5):
        clip = t._clip(seed=s)
        a, b = te.step(clip), tg.step(clip)
        assert torch.equal(a, b) and torch.isfinite(a), s
        assert torch.equal(te.loss_per_sample, tg.loss_per_sample), s
        assert tg.loss_per_sample.shape == (2,)
        losses.append(float(b))
    assert tg.graph.g is not None and len(set(losses)) == 5, losses
    types = tg.graph.node_types()
    assert types.get("memset", 0) == 0 and types.get("kernel", 0) > 20, types
    tg.check_finite()


# ------------------------------------------------------------------ entry points
TINY = ["--dims", "3", "--frames", "8", "--image-size", "64", "--model-channels", "32",
        "--channel-mult", "1", "2", "--num-res-blocks", "1", "--attention-resolutions", "2",
        "--random-audio-encoder"]


def _run(script, args, cwd):
    out = subprocess.run([sys.executable, os.path.join(DROPIN, script)] + args, cwd=cwd,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


def test_train_entry_with_the_objective(tmp_path):
    ck = str(tmp_path / "m.pth")
    out = _run("train.py", TINY + ["--batch-size", "1", "--epochs", "1", "--steps-per-epoch", "2",
                                   "--ckpt", ck, "--prediction", "v", "--loss-weighting",
                                   "min-snr", "--snr-gamma", "4"], tmp_path)
    line = [ln for ln in out.splitlines() if ln.startswith("Finished epoch 1")][0]
    assert "mse by t quartile" in line, line
    state = torch.load(ck + ".resume", map_location="cpu", weights_only=True)
    assert state["prediction"] == "v"
    sd = torch.load(ck, map_location="cpu", weights_only=True)
    assert all(isinstance(v, torch.Tensor) for v in sd.values())  # a plain state dict


def test_sampling_entry_with_v(tmp_path):
    out_dir = tmp_path / "imgs"
    _run("test.py", ["--random-init", "--sampler", "dpm++", "--prediction", "v", "--steps", "4",
                     "--image-size", "32", "--save-every", "1", "--out-dir", str(out_dir)],
         tmp_path)
    files = sorted(p for p in os.listdir(out_dir) if p.endswith(".npy"))
    assert len(files) == 4, files
    for f in files:
        x0 = np.load(out_dir / f)
        assert x0.shape == (1, 3, 32, 32) and np.isfinite(x0).all()
