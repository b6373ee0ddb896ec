"""DPM-Solver++(2M) sampling on the GPU: vd_dpm_step / vd_dpm_step_cfg against fp64 with
element-wise bounds (tests/_dpm_cases.py derives them), the C == 0 rule, aliasing, the replayed
graph against the eager loop (bit for bit), order = 1 against DDIM through the samplers, the
order of accuracy on the analytic Gaussian model with the real kernel, and the entry point."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import DROPIN, record_metric

import _cfg_cases as cfg
import _dpm_cases as cases
from _bounds import U_FP32, assert_elementwise, bound

pytestmark = pytest.mark.gpu
dev = "cuda"


def _sampler(**kw):
    from vdiff.schedulers import DPMSolverSampler
    kw.setdefault("steps", 8)
    return DPMSolverSampler(cases.v2_scheduler(), **kw)


def _to_dev(bf16, *xs):
    dt = torch.bfloat16 if bf16 else torch.float32
    return tuple(x.to(device=dev, dtype=dt).contiguous() for x in xs)


def _check(got, ref, name, bf16, what):
    r, m, n, ce = ref[name]
    return assert_elementwise(got, r, m, n, bf16, ce, what=f"{name} {what}")


# ------------------------------------------------------------------ 6. kernel against fp64
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,P", cases.SHAPES)
def test_step_against_fp64(B, P, bf16):
    from vdiff import ops
    s = _sampler()
    coef, idx = s._tables(dev)
    xt, eps, _, last = cases.inputs(B, P, bf16)
    xt_d, eps_d, last_d = _to_dev(bf16, xt, eps, last)
    rows = cases.kernel_rows(s)
    assert s.coef[rows[0], 4] == 0 and s.coef[rows[1], 4] != 0
    assert s.coef[rows[2], 2:5].tolist() == [0.0, 1.0, 0.0]
    worst = 0.0
    for i in rows:
        for clip in (False, True):
            what = f"B={B} P={P} bf16={bf16} row={i} clip={clip}"
            ref = cases.ref64(xt, eps, last, s.coef[i], clip)
            hist = last_d.clone()
            if i == 0:  # the C == 0 rule: an uninitialised history is never read
                hist.fill_(float("nan"))
            xp, x0 = ops.dpm_step(xt_d, eps_d, hist, coef, idx[i:i + 1], clip=clip)
            assert x0.data_ptr() == hist.data_ptr()
            assert torch.isfinite(xp).all() and torch.isfinite(x0).all(), what
            worst = max(worst, _check(xp, ref, "x_prev", bf16, what),
                        _check(x0, ref, "x0", bf16, what))
            if i == rows[2] and not bf16:
                assert torch.equal(xp, x0), what
            # x_prev over xt, the history in place: the same bits
            alias, hist2 = xt_d.clone(), last_d.clone()
            xa, x0a = ops.dpm_step(alias, eps_d, hist2, coef, idx[i:i + 1], clip=clip, out=alias)
            assert xa.data_ptr() == alias.data_ptr()
            assert torch.equal(alias, xp) and torch.equal(x0a, x0), what
    print(f"dpm_step B={B} P={P} {'bf16' if bf16 else 'fp32'}: largest error / bound {worst:.3g}")
    record_metric(test="dpm_step_fp64", B=B, P=P, dtype="bf16" if bf16 else "fp32", worst=worst)
    assert 0 < worst <= 1


def test_step_index_is_clamped_and_read_on_the_device():
    from vdiff import ops
    s = _sampler()
    coef, idx = s._tables(dev)
    xt, eps, _, last = cases.inputs(2, 105, False)
    xt_d, eps_d, last_d = _to_dev(False, xt, eps, last)
    want = {i: ops.dpm_step(xt_d, eps_d, last_d.clone(), coef, idx[i:i + 1])
            for i in (0, 3, s.steps - 1)}
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    for value, row in ((-5, 0), (3, 3), (s.steps, s.steps - 1), (1 << 40, s.steps - 1)):
        step.fill_(value)  # the same launch arguments, another row
        xp, x0 = ops.dpm_step(xt_d, eps_d, last_d.clone(), coef, step)
        assert torch.equal(xp, want[row][0]) and torch.equal(x0, want[row][1]), value


def test_argument_checks():
    from vdiff import ops
    s = _sampler()
    coef, idx = s._tables(dev)
    x = torch.randn(2, 64, device=dev)
    with pytest.raises(ValueError):
        ops.dpm_step(x, x[:1], x.clone(), coef, idx[:1])
    with pytest.raises(ValueError):
        ops.dpm_step(x, x, None, coef, idx[:1])
    with pytest.raises(ValueError):
        ops.dpm_step(x, x, x.clone().bfloat16(), coef, idx[:1])
    with pytest.raises(ValueError):
        ops.dpm_step(x, x, x.clone(), coef[:, :5].contiguous(), idx[:1])
    with pytest.raises(ValueError):
        ops.dpm_step(x, x, x.clone(), coef, idx[:2])
    with pytest.raises(ValueError):
        ops.dpm_step_cfg(x, x, x, x.clone(), coef, idx[:1], 2.0, 1.5)
    with pytest.raises(RuntimeError):
        ops.dpm_step(x, x, x.clone(), coef.cpu(), idx[:1])
    with pytest.raises(ValueError):
        s.step(x, x, 2)


# ------------------------------------------------------------------ 7. guided kernel
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,P", cases.SHAPES)
def test_guided_step_against_fp64(B, P, bf16):
    """dpm_step_cfg against the fp64 step on the fp64 guided noise: the unguided bound plus the
    guide's 3 roundings, and for rescale = 0.7 the f_b allowance of _cfg_cases; in fp32 the
    composed dpm_step(cfg_combine) -- dpm_step fed the fp32 guided noise -- lies inside the same
    bound about the same reference."""
    from vdiff import ops
    s = _sampler()
    coef, idx = s._tables(dev)
    xt, c, u, last = cases.inputs(B, P, bf16)
    xt_d, c_d, u_d, last_d = _to_dev(bf16, xt, c, u, last)
    worst = 0.0
    for i in cases.kernel_rows(s):
        for w in (0.0, 2.5, 7.5):
            for phi in (0.0, 0.7):
                clip = w == 2.5
                what = f"B={B} P={P} bf16={bf16} row={i} w={w} phi={phi}"
                ref = cases.ref64(xt, c, last, s.coef[i], clip, guide=(u, w, phi))
                hist = last_d.clone()
                if i == 0:
                    hist.fill_(float("nan"))
                dup = torch.empty_like(xt_d)
                xp, x0 = ops.dpm_step_cfg(xt_d, c_d, u_d, hist, coef, idx[i:i + 1], w, phi,
                                          clip=clip, dup=dup)
                assert torch.equal(dup, xp) and x0.data_ptr() == hist.data_ptr()
                assert torch.isfinite(xp).all() and torch.isfinite(x0).all(), what
                worst = max(worst, _check(xp, ref, "x_prev", bf16, what),
                            _check(x0, ref, "x0", bf16, what))
                if not bf16:
                    g = ops.cfg_combine(c_d, u_d, w, phi)
                    hist2 = last_d.clone()
                    xc, x0c = ops.dpm_step(xt_d, g, hist2, coef, idx[i:i + 1], clip=clip)
                    _check(xc, ref, "x_prev", bf16, "composed " + what)
                    _check(x0c, ref, "x0", bf16, "composed " + what)
                # in place, into the doubled input's halves
                x2 = torch.cat([xt_d, xt_d])
                hist3 = last_d.clone()
                ops.dpm_step_cfg(x2[:B], c_d, u_d, hist3, coef, idx[i:i + 1], w, phi, clip=clip,
                                 out=x2[:B], dup=x2[B:])
                assert torch.equal(x2[:B], xp) and torch.equal(x2[B:], xp), what
                assert torch.equal(hist3, x0), what
        # w = 1 on equal halves: the guide is exact (c - u = 0, f_b off), so the guided kernel
        # lies inside the UNGUIDED bound
        ref = cases.ref64(xt, u, last, s.coef[i], False)
        hist = last_d.clone()
        xp, x0 = ops.dpm_step_cfg(xt_d, u_d.clone(), u_d, hist, coef, idx[i:i + 1], 1.0, 0.0)
        _check(xp, ref, "x_prev", bf16, f"c == u row={i}")
        _check(x0, ref, "x0", bf16, f"c == u row={i}")
    print(f"dpm_step_cfg B={B} P={P} {'bf16' if bf16 else 'fp32'}: largest error / bound "
          f"{worst:.3g}")
    record_metric(test="dpm_step_cfg_fp64", B=B, P=P, dtype="bf16" if bf16 else "fp32",
                  worst=worst)
    assert 0 < worst <= 1


# ------------------------------------------------------------------ 8. graph against eager
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


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("dims,bf16", [(3, True), (3, False), (2, True)])
def test_dpm_graph_matches_eager(dims, bf16, guided, monkeypatch):
    from vdiff.engine import sample_dpm
    m = _model(dims, bf16)
    shape, cond, feats = _sampling_case(dims)
    sampler = _sampler(steps=6)
    assert sampler.steps == 6
    kw = dict(guidance_scale=3.0, guidance_rescale=0.7) if guided else {}
    out, traj = {}, {}
    for mode in ("0", "1"):
        monkeypatch.setenv("VDIFF_DDIM_GRAPH", mode)
        g = torch.Generator(device=dev).manual_seed(9)
        seen = traj[mode] = []
        out[mode] = sample_dpm(m, sampler, cond, feats, shape, generator=g,
                               callback=lambda i, xt, x0: seen.append((xt, x0)), **kw)
    for a, b in zip(out["0"], out["1"]):
        assert torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b)
    # a callback that keeps references sees every step's own values on both paths
    assert len(traj["0"]) == len(traj["1"]) == 6
    for i, ((xa, x0a), (xb, x0b)) in enumerate(zip(traj["0"], traj["1"])):
        assert torch.equal(xa, xb) and torch.equal(x0a, x0b), i
    x0s = [x0 for _, x0 in traj["1"]]
    assert all(not torch.equal(x0s[i], x0s[i + 1]) for i in range(5))
    assert torch.equal(out["1"][0], out["1"][1])  # the last row: x_prev is x0
    assert torch.equal(traj["1"][-1][1], out["1"][1])


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
def test_dpm_graph_holds_no_memset_node(guided):
    from vdiff import ops
    from vdiff.engine import DPMGraph
    m = _model(3, True)
    shape, cond, feats = _sampling_case(3)
    sampler = _sampler(steps=6)
    kw = dict(guidance_scale=3.0, guidance_rescale=0.7) if guided else {}
    with torch.no_grad(), ops.frozen_weights():
        xt = torch.randn(shape, device=dev)
        gr = DPMGraph(m, sampler, cond, feats, xt, **kw)
        gr.capture()
        types = gr.node_types()
        assert types.get("memset", 0) == 0 and types.get("kernel", 0) > 20, types
        got, x0 = gr.step(0)
        assert torch.isfinite(got).all() and torch.isfinite(x0).all()
        assert not torch.equal(got, xt)
        if guided:
            assert torch.equal(gr.x2[:1], gr.x2[1:]) and got.data_ptr() == gr.x2.data_ptr()


# ------------------------------------------------------------------ 9., 10. the Gaussian model
class GaussEps(torch.nn.Module):
    """The optimal noise prediction for data N(0, s^2), eps*(x, t) = c_t x with c_t = sqrt(1 -
    a_t) / (a_t s^2 + 1 - a_t): one fp32 table (taken as exact) and one rounded product."""

    def __init__(self, acp, s):
        super().__init__()
        a = acp.double()
        self.register_buffer("c", (torch.sqrt(1 - a) / (a * s * s + 1 - a)).float())

    def forward(self, x, cond, feats, t):
        return self.c[t].view(-1, *([1] * (x.dim() - 1))) * x


def _order1_bound(x_T, acp, ts, c32, rows64):
    """(exact final sample, bound on |x0_dpm - x0_ddim|) for the elementwise-linear model eps =
    c_t x, per element in fp64.

    Both samplers follow, in exact arithmetic, the one recurrence x_prev = sqrt(a_p) x0 +
    sqrt(1 - a_p) eps = A x + B x0 (the order-1 identity).  Each computed trajectory leaves it
    by d_i, and to first order in u32
        d_{i+1} <= |G_i| d_i + |dx_prev / deps|_i u32 |eps_i| + allowance_i
    where G_i = sqrt(a_p) (1 - s c) / alpha + sqrt(1 - a_p) c is the step's exact gain through
    the linear model (s = sigma_t), dx_prev / deps = sqrt(1 - a_p) - sqrt(a_p) s / alpha, u32
    |eps| the model's one rounded product, and allowance_i the kernel's own bound about the
    fp64 recurrence, with magnitudes on the exact trajectory (their change along the computed
    one is second order, inside the factor 2 of _bounds.bound):
      * vd_dpm_step: the 6 roundings of _dpm_cases.ref64 plus the fp32 rounding of the row's
        alpha, sigma and B (or A) on the same longest path: n = 9, mag = A |x| + |B| mag_x0;
      * vd_ddim_step: _cfg_cases.ref64's x_prev bound (n = 16 and the allowance for dir = sqrt(1
        - a_p), whose coefficients the kernel derives in fp32), with w = 0 so that the guide is
        the identity.
    On the last step a_p = 1 and x_prev = x0, so the x_prev allowance also bounds the x0 the
    samplers return.  The two deviations add."""
    a = acp.double()
    x = x_T.detach().cpu().double().flatten(1)
    B = x.shape[0]
    d_dpm, d_ddim = torch.zeros_like(x), torch.zeros_like(x)
    z = torch.zeros_like(x)
    for i, t in enumerate(ts):
        tp = ts[i + 1] if i + 1 < len(ts) else -1
        at, ap = float(a[t]), (float(a[tp]) if tp >= 0 else 1.0)
        c = float(c32[t])
        s, al = math.sqrt(1 - at), math.sqrt(at)
        eps = c * x
        x0 = (x - s * eps) / al
        gain = abs(math.sqrt(ap) * (1 - s * c) / al + math.sqrt(1 - ap) * c)
        deps = abs(math.sqrt(1 - ap) - math.sqrt(ap) * s / al)
        A, Bc = float(rows64[i][2]), float(rows64[i][3])
        mag_dpm = abs(A) * x.abs() + abs(Bc) * (x.abs() + s * eps.abs()) / al
        allow_dpm = bound(torch.zeros_like(x), mag_dpm, 9, False)
        r, m, n, ce = cfg.ref64(x, eps, eps, z, torch.full((B,), t), torch.full((B,), tp), acp,
                                0.0, 0.0, 0.0, False)["x_prev"]
        allow_ddim = bound(torch.zeros_like(x), m, n, False, ce)
        common = deps * U_FP32 * eps.abs()
        d_dpm = gain * d_dpm + common + allow_dpm
        d_ddim = gain * d_ddim + common + allow_ddim
        x = math.sqrt(ap) * x0 + math.sqrt(1 - ap) * eps
    return x, d_dpm + d_ddim


@pytest.mark.parametrize("graph", ["0", "1"], ids=["eager", "graph"])
def test_order1_matches_ddim_through_the_samplers(graph, monkeypatch):
    """order = 1 on DDIM's linspace timesteps is the DDIM recurrence: sample_dpm and sample_ddim
    from the same seed agree in the final x0 within the bound _order1_bound derives.  The
    model is the elementwise-linear Gaussian one, the only kind whose sensitivity to its input
    is known exactly (a UNet's is not, and no bound could be derived through it).  Measured on
    an MI355X: largest difference / bound 0.0075 (eager and graph alike)."""
    from vdiff.engine import sample_ddim, sample_dpm
    from vdiff.schedulers import DDIMSampler
    monkeypatch.setenv("VDIFF_DDIM_GRAPH", graph)
    sch = cases.v2_scheduler()
    acp = sch.alpha_cum_prod.float()
    model = GaussEps(acp, 0.5).to(dev)
    shape = (2, 3, 16, 16)
    cond = torch.zeros((2, 3, 16, 16), device=dev)
    dpm = _sampler(steps=6, order=1, spacing="linspace")
    ddim = DDIMSampler(sch, steps=6)
    assert torch.equal(dpm.timesteps, ddim.timesteps)
    g = torch.Generator(device=dev).manual_seed(5)
    _, x0_dpm = sample_dpm(model, dpm, cond, None, shape, generator=g)
    g = torch.Generator(device=dev).manual_seed(5)
    _, x0_ddim = sample_ddim(model, ddim, cond, None, shape, generator=g)
    g = torch.Generator(device=dev).manual_seed(5)
    x_T = torch.randn(shape, generator=g, device=dev)
    exact, bnd = _order1_bound(x_T, acp, dpm.timesteps.tolist(), model.c.cpu(),
                               dpm.coef64.tolist())
    a, b = (v.cpu().double().flatten(1) for v in (x0_dpm, x0_ddim))
    assert torch.isfinite(a).all() and a.abs().max() > 0
    # both are the exact recurrence's final sample to fp32 accuracy
    assert ((a - exact).abs() <= bnd).all() and ((b - exact).abs() <= bnd).all()
    ratio = float(((a - b).abs() / bnd).max())
    print(f"order-1 dpm vs ddim, graph={graph}: largest difference / bound {ratio:.3g}")
    record_metric(test="dpm_order1_vs_ddim", graph=graph, ratio=ratio)
    assert ratio <= 1


def test_order_of_accuracy_with_the_kernel():
    """Conditions 4(a) and 4(b) of tests/test_dpm_host.py with eps* from torch ops in fp32 and
    the real kernels as the step: fp32 rounding is about 1e-6 against errors of 1e-3 to 1e-2.
    Every element is its own (linear) trajectory; the conditions are asserted on the least
    favourable elements."""
    from vdiff.schedulers import DDIMSampler
    sch = cases.v2_scheduler()
    acp = sch.alpha_cum_prod.float()
    g = torch.Generator().manual_seed(3)
    x_T = (torch.randn((2, 256), generator=g).abs() + 0.1).to(dev)
    a_T = float(acp.double()[-1])

    def rel(x_end, s):
        return (x_end.cpu().double() / (x_T.cpu().double() * cases.gauss_exact(a_T, s)) - 1).abs()

    for s in cases.S_VALUES:
        model = GaussEps(acp, s).to(dev)
        errs = {}
        for steps in (10, 20):
            smp = _sampler(steps=steps)
            x, x0 = x_T.clone(), None
            for i in range(smp.steps):
                t = torch.full((2,), int(smp.timesteps[i]), dtype=torch.int64, device=dev)
                x, x0 = smp.step(x, model(x, None, None, t), i, x0_last=x0)
            errs[steps] = rel(x, s)
        ddim = DDIMSampler(sch, steps=50)
        x = x_T.clone()
        for i in range(50):
            t = torch.full((2,), int(ddim.timesteps[i]), dtype=torch.int64, device=dev)
            x, _ = ddim.step(x, model(x, None, None, t), i)
        e_ddim = rel(x, s)
        print(f"s={s}: ddim50 {float(e_ddim.min()):.3e} 2M10 {float(errs[10].min()):.3e} "
              f"2M20 {float(errs[20].max()):.3e}")
        assert float(errs[20].max()) <= 0.5 * float(e_ddim.min()), s
        assert float(errs[10].min()) / float(errs[20].max()) >= 2.5, s


# ------------------------------------------------------------------ 11. entry point
@pytest.mark.parametrize("extra", [[], ["--spacing", "linspace", "--guidance-scale", "2",
                                        "--guidance-rescale", "0.5"]], ids=["plain", "guided"])
def test_sampling_entry(tmp_path, extra):
    out_dir = tmp_path / "imgs"
    out = subprocess.run([sys.executable, os.path.join(DROPIN, "test.py"), "--random-init",
                          "--sampler", "dpm++", "--steps", "4", "--image-size", "32",
                          "--save-every", "1", "--out-dir", str(out_dir)] + extra, cwd=tmp_path,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    files = sorted(p for p in os.listdir(out_dir) if p.endswith(".npy"))
    assert len(files) == 4, files
    for f in files:
        x0 = np.load(out_dir / f)
        assert x0.shape == (1, 3, 32, 32) and np.isfinite(x0).all()
