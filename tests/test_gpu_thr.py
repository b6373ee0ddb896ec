"""Dynamic thresholding on the GPU: vd_x0_abs_quantile bit for bit against a CPU sort, crafted
rows, reproducibility on a dirty workspace, the source rules and the four thresholded step ops
against fp64 with the bounds tests/_thr_cases.py derives, the floor and aliasing rules, the
samplers eager against replayed, the graphs' node counts and the entry point."""
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
import _thr_cases as cases
from _bounds import assert_elementwise

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = math.inf
SELECT_LAUNCHES = 8  # include/vdiff.h: four histogram and four scan launches


def _dt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _to_dev(bf16, *xs):
    return tuple(x.to(device=dev, dtype=_dt(bf16)).contiguous() for x in xs)


def _select(x, rank, floor=0.0, cap=INF, ws=None, src=None):
    """vd_x0_abs_quantile by rank on x [B, P] (identity source unless src is given)."""
    from vdiff import _lib, ops
    B, P = x.shape
    n = _lib.lib().vd_x0_quantile_workspace_size(B, P)
    if ws is None:
        ws = torch.empty(n, dtype=torch.uint8, device=dev)
    assert ws.numel() >= n
    s = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    if src is None:
        src = _lib.X0Source(x=x.data_ptr(), rule=_lib.X0_IDENTITY)
    _lib.call("vd_x0_abs_quantile", src, rank, floor, cap, B, P, ops._dtype(x), s.data_ptr(),
              ws.data_ptr(), ws.numel(), ops._stream(x))
    return s


def _sorted_abs(x):
    """Rows of |x| as fp32 in the order of their bit patterns (a NaN above +inf)."""
    bits = x.detach().cpu().float().abs().view(torch.int32)
    return bits.sort(dim=1).values.view(torch.float32)


# ------------------------------------------------------------------ 1. the selection, bit for bit
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,P", cases.SELECT_SHAPES)
def test_abs_quantile_is_the_sorted_element(B, P, bf16):
    from vdiff import ops
    g = torch.Generator().manual_seed(P)
    x = (torch.randn((B, P), generator=g) * 1.5).to(_dt(bf16))
    want = _sorted_abs(x)
    x_d = x.to(dev)
    if (B, P) == (2, 105):
        assert cases.rank(0.995, P) == P - 1  # the scalar-path case asks for the maximum
    for p in cases.SELECT_PS:
        k = cases.rank(p, P)
        got = ops.abs_quantile(x_d, p)
        assert got.dtype == torch.float32 and tuple(got.shape) == (B,)
        assert torch.equal(got.cpu(), want[:, k]), (p, k)
    got = _select(x_d, 0)
    assert torch.equal(got.cpu(), want[:, 0])
    # two calls, and a workspace full of 0xFF bytes: the same bits
    k = cases.rank(0.995, P)
    a = _select(x_d, k)
    dirty = torch.full((ops._lib.lib().vd_x0_quantile_workspace_size(B, P),), 0xFF,
                       dtype=torch.uint8, device=dev)
    b = _select(x_d, k, ws=dirty)
    assert torch.equal(a, b) and torch.equal(a.cpu(), want[:, k])


def _row_cases():
    nan, inf = float("nan"), INF
    tiny = 2.0 ** -140  # a denormal
    one = torch.tensor(1.0)
    up = torch.nextafter(one, torch.tensor(2.0))
    rows = {
        "equal": torch.full((1, 300), -3.25),
        # only the lowest mantissa bit differs: the last digit decides
        "last_bit": torch.stack([torch.where(torch.arange(300) % 3 == 0, up, one)]),
        "specials": torch.tensor([[0.0, -0.0, tiny, -tiny, 3 * tiny, inf, -inf, -2.5, 1.0, -1.0,
                                   7.0, -0.5, 2.0 ** -126, 65504.0, -1e30, 1e-30, 0.0]]),
        "nans": torch.cat([torch.linspace(-4, 4, 96), torch.tensor([nan, -nan, nan, inf])])[None],
        "single": torch.tensor([[-2.5], [0.75]]),
    }
    return rows


@pytest.mark.parametrize("name", ["equal", "last_bit", "specials", "nans", "single"])
def test_crafted_rows(name):
    x = _row_cases()[name]
    want = _sorted_abs(x)
    x_d = x.to(dev)
    B, P = x.shape
    for k in range(P):
        got = _select(x_d, k).cpu()
        # bit for bit (the sign of a zero included); a NaN quantile gives the floor, here 0
        w = torch.where(torch.isnan(want[:, k]), torch.zeros(B), want[:, k])
        assert torch.equal(got.view(torch.int32), w.view(torch.int32)), (name, k, got, w)
    if name == "nans":
        n_nan = int(torch.isnan(x).sum())
        assert n_nan == 3
        below = _select(x_d, P - n_nan - 1, 1.0, INF).cpu()   # the rank below the NaNs: +inf
        assert torch.equal(below, torch.tensor([INF]))
        finite = _select(x_d, P - n_nan - 2, 1.0, INF).cpu()  # and the largest finite value
        assert torch.equal(finite, torch.tensor([4.0]))
        for k in range(P - n_nan, P):                         # a NaN quantile: s is the floor
            assert torch.equal(_select(x_d, k, 1.0, INF).cpu(), torch.tensor([1.0])), k
            assert torch.equal(_select(x_d, k, 1.0, 2.0).cpu(), torch.tensor([1.0])), k
    if name == "single":
        assert torch.equal(_select(x_d, 0, 1.0, 2.0).cpu(), torch.tensor([2.0, 1.0]))


def test_heavy_ties_in_bf16():
    """bf16 rows hold far fewer distinct magnitudes than elements (tests/test_thr_host.py counts
    them): every rank of a stride through the row is the sorted element."""
    from vdiff import ops
    xt = cfg.inputs(2, 5000, bf16=True)[0]
    want = _sorted_abs(xt)
    x_d = xt.to(device=dev, dtype=torch.bfloat16)
    for k in list(range(0, 5000, 499)) + [4999]:
        assert torch.equal(_select(x_d, k).cpu(), want[:, k]), k
    assert torch.equal(ops.abs_quantile(x_d, 0.5).cpu(), want[:, cases.rank(0.5, 5000)])


# ------------------------------------------------------------------ 2. the source rules
def _rules(kind, B):
    if kind == "dpm":
        s = cases.dpm_sampler()
        coef, idx = s._tables(dev)
        return [(dict(row=s.coef[i]), dict(coef=coef, step=idx[i:i + 1], n=s.steps))
                for i in dpm.kernel_rows(s)]
    t, tp = cfg.timesteps(B)
    acp = cases.acp_table()
    return [(dict(t=t, tp=tp, acp=acp), dict(t=t.to(dev), tp=tp.to(dev), acp=acp.to(dev)))]


def _source(kind, xt_d, c_d, u_d, guide, d):
    """(vd_x0_source of the rule, what must stay alive while it is used)."""
    from vdiff import _lib, ops
    kw = dict(x=xt_d.data_ptr(), eps=c_d.data_ptr())
    keep = None
    if guide is not None:
        w, phi = guide
        *_, keep = ops._cfg_args(c_d, u_d, w, phi)
        kw.update(eps_u=u_d.data_ptr(), w=w, rescale=phi,
                  cfg_workspace=None if keep is None else keep.data_ptr())
    if kind == "dpm":
        kw.update(rule=_lib.X0_DPM, coef=d["coef"].data_ptr(), step=d["step"].data_ptr(),
                  n_steps=d["n"])
    else:
        kw.update(rule=_lib.X0_DDIM, t=d["t"].data_ptr(), acp=d["acp"].data_ptr(),
                  prediction=int(kind == "ddim-v"))
    return _lib.X0Source(**kw), keep


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("B,P", cases.SHAPES)
def test_source_rules_against_fp64(B, P, kind, bf16):
    """|s - s_ref| <= max_i bound(x0_i): an order statistic, the floor and the cap are each
    1-Lipschitz in the sup norm (tests/_thr_cases.py)."""
    xt, c, u, z = cfg.inputs(B, P, bf16)
    xt_d, c_d, u_d = _to_dev(bf16, xt, c, u)
    k = cases.rank(cases.P_THR, P)
    worst = 0.0
    for host, d in _rules(kind, B):
        for guide in cases.GUIDES:
            base, K = cases.base64(kind, xt, c, u, z, guide, **host)
            src, keep = _source(kind, xt_d, c_d, u_d, guide, d)
            for tmax in (INF, 2.0):
                ref = cases.thresholded(base, K, tmax=tmax)
                s_ref, Delta = ref["s"]
                assert (ref["q"] > 1).all()
                got = _select(xt_d, k, 1.0, tmax, src=src).cpu().double().view(-1, 1)
                err = (got - s_ref).abs()
                what = f"{kind} B={B} P={P} bf16={bf16} guide={guide} tmax={tmax}"
                print(f"s {what}: got {got.flatten().tolist()} ref {s_ref.flatten().tolist()} "
                      f"bound {Delta.flatten().tolist()}")
                assert (err <= Delta).all(), (what, got, s_ref, Delta)
                if tmax == 2.0:
                    assert (got == 2).all(), what
                worst = max(worst, float((err / Delta).max()))
    record_metric(test="thr_source_fp64", kind=kind, B=B, P=P, dtype="bf16" if bf16 else "fp32",
                  worst=worst)


# ------------------------------------------------------------------ 3. the thresholded steps
def _step(kind, xt_d, c_d, u_d, other_d, guide, d, thresh=None, clip=False, out=None, dup=None):
    """(x_prev, x0) of the op under test; other_d: z (unused, eta = 0) or the history."""
    from vdiff import ops
    kw = dict(clip=clip) if thresh is None else dict(thresh=thresh)
    if kind == "dpm":
        hist = other_d.clone()
        if guide is None:
            return ops.dpm_step(xt_d, c_d, hist, d["coef"], d["step"], out=out, **kw)
        return ops.dpm_step_cfg(xt_d, c_d, u_d, hist, d["coef"], d["step"], guide[0], guide[1],
                                out=out, dup=dup, **kw)
    pred = "v" if kind == "ddim-v" else "eps"
    if guide is None:
        return ops.ddim_step(xt_d, c_d, d["t"], d["tp"], d["acp"], prediction=pred, **kw)
    return ops.ddim_step_cfg(xt_d, c_d, u_d, d["t"], d["tp"], d["acp"], guide[0], guide[1],
                             out=out, dup=dup, prediction=pred, **kw)


def _check(got, ref, name, bf16, what):
    r, m, n, ce = ref[name]
    return assert_elementwise(got, r, m, n, bf16, ce, what=f"{name} {what}")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("B,P", cases.SHAPES)
def test_thresholded_steps_against_fp64(B, P, kind, bf16):
    xt, c, u, z = cfg.inputs(B, P, bf16)
    xt_d, c_d, u_d, z_d = _to_dev(bf16, xt, c, u, z)
    worst = 0.0
    for host, d in _rules(kind, B):
        for guide in cases.GUIDES:
            base, K = cases.base64(kind, xt, c, u, z, guide, **host)
            for tmax in (INF, 2.0):
                ref = cases.thresholded(base, K, tmax=tmax)
                what = f"{kind} B={B} P={P} bf16={bf16} guide={guide} tmax={tmax}"
                dup = torch.empty_like(xt_d) if guide is not None else None
                xp, x0 = _step(kind, xt_d, c_d, u_d, z_d, guide, d, (cases.P_THR, tmax), dup=dup)
                assert x0.abs().max() <= 1, what
                r = max(_check(xp, ref, "x_prev", bf16, what), _check(x0, ref, "x0", bf16, what))
                worst = max(worst, r)
                if dup is not None:
                    assert torch.equal(dup, xp), what
                # x_prev over xt (and the doubled input's halves, guided): the same bits
                if kind == "dpm" or guide is not None:
                    x2 = torch.cat([xt_d, xt_d])
                    xa, x0a = _step(kind, x2[:B], c_d, u_d, z_d, guide, d, (cases.P_THR, tmax),
                                    out=x2[:B], dup=x2[B:] if guide is not None else None)
                    assert xa.data_ptr() == x2.data_ptr()
                    assert torch.equal(x2[:B], xp) and torch.equal(x0a, x0), what
                    if guide is not None:
                        assert torch.equal(x2[B:], xp), what
    print(f"thresholded {kind} B={B} P={P} {'bf16' if bf16 else 'fp32'}: largest error / bound "
          f"{worst:.3g}")
    record_metric(test="thr_step_fp64", kind=kind, B=B, P=P, dtype="bf16" if bf16 else "fp32",
                  worst=worst)
    assert 0 < worst <= 1


def test_dpm_history_is_written_in_place():
    xt, c, u, last = cfg.inputs(2, 5000, False)
    xt_d, c_d, u_d, last_d = _to_dev(False, xt, c, u, last)
    host, d = _rules("dpm", 2)[1]
    from vdiff import ops
    hist = last_d.clone()
    xp, x0 = ops.dpm_step_cfg(xt_d, c_d, u_d, hist, d["coef"], d["step"], cases.W, 0.7,
                              thresh=(cases.P_THR, INF))
    assert x0.data_ptr() == hist.data_ptr() and not torch.equal(hist, last_d)
    base, K = cases.base64("dpm", xt, c, u, last, (cases.W, 0.7), **host)
    ref = cases.thresholded(base, K)
    _check(hist, ref, "x0", False, "history")
    _check(xp, ref, "x_prev", False, "x_prev from the history row")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", cases.KINDS)
def test_floor_case_is_the_static_clamp(kind, bf16):
    """Inputs scaled by 0.2 at t = 0 (the last row for 2M): q < 1, s is exactly 1, and the
    thresholded step and the clip=True step both lie inside the same bounds about the one fp64
    reference."""
    B, P = 2, 5000
    xt, c, u, z = (cfg.rounded(0.2 * v, bf16) for v in cfg.inputs(B, P, bf16))
    xt_d, c_d, u_d, z_d = _to_dev(bf16, xt, c, u, z)
    if kind == "dpm":
        host, d = _rules(kind, B)[-1]
    else:
        t, tp = torch.zeros(B, dtype=torch.int64), torch.full((B,), -1)
        acp = cases.acp_table()
        host, d = dict(t=t, tp=tp, acp=acp), dict(t=t.to(dev), tp=tp.to(dev), acp=acp.to(dev))
    for guide in (None, (cases.W, 0.7)):
        base, K = cases.base64(kind, xt, c, u, z, guide, **host)
        ref = cases.thresholded(base, K)
        if guide is None:
            assert (ref["q"] < 1).all() and (ref["q"] > 0.5).all(), ref["q"]
        if not (ref["q"] < 1).all():
            continue
        assert (ref["s"][0] == 1).all()
        src, keep = _source(kind, xt_d, c_d, u_d, guide, d)
        s = _select(xt_d, cases.rank(cases.P_THR, P), 1.0, INF, src=src)
        assert torch.equal(s.cpu(), torch.ones(B))
        thr = _step(kind, xt_d, c_d, u_d, z_d, guide, d, (cases.P_THR, INF))
        clip = _step(kind, xt_d, c_d, u_d, z_d, guide, d, clip=True)
        for got in (thr, clip):
            _check(got[0], ref, "x_prev", bf16, f"floor {kind} {guide}")
            _check(got[1], ref, "x0", bf16, f"floor {kind} {guide}")


# ------------------------------------------------------------------ 4. the samplers
_models = {}


def _model(bf16):
    from test_gpu_dpm import _model as tiny
    if bf16 not in _models:
        _models[bf16] = tiny(3, bf16)
    return _models[bf16]


def _case(L):
    g = torch.Generator(device=dev).manual_seed(77)
    cond = torch.rand((1, 3, 32, 32), device=dev, generator=g) * 2 - 1
    feats = torch.randn((L, 64), device=dev, generator=g)
    return (1, 3, L, 32, 32), cond, feats


def _sampler(name, **kw):
    from vdiff.schedulers import DDIMSampler, DPMSolverSampler
    cls = DDIMSampler if name == "ddim" else DPMSolverSampler
    return cls(dpm.v2_scheduler(), steps=6, **kw)


def _sample(name, long_, m, sampler, **kw):
    from vdiff.engine import sample_ddim, sample_dpm, sample_long
    shape, cond, feats = _case(8 if long_ else 4)
    g = torch.Generator(device=dev).manual_seed(9)
    if long_:
        return sample_long(m, sampler, cond, feats, shape, window=4, stride=2, generator=g, **kw)
    return (sample_ddim if name == "ddim" else sample_dpm)(m, sampler, cond, feats, shape,
                                                           generator=g, **kw)


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("long_", [False, True], ids=["short", "long"])
@pytest.mark.parametrize("name", ["ddim", "dpm++"])
def test_thresholded_sampling_graph_matches_eager(name, long_, bf16, monkeypatch):
    """Guidance 7.5 with the std-rescale and dynamic_threshold = 0.995: the replayed graph and
    the eager loop give the same bits at every step (the callback's clones are host work between
    replays), every x0 lies in [-1, 1], and the result is not the unthresholded one."""
    m = _model(bf16)
    sampler = _sampler(name, dynamic_threshold=0.995)
    assert sampler.steps == 6
    kw = dict(guidance_scale=7.5, guidance_rescale=0.7)
    out, traj = {}, {}
    for mode in ("0", "1"):
        monkeypatch.setenv("VDIFF_DDIM_GRAPH", mode)
        seen = traj[mode] = []
        out[mode] = _sample(name, long_, m, sampler,
                            callback=lambda i, xt, x0: seen.append((xt.clone(), x0.clone())),
                            **kw)
    for a, b in zip(out["0"], out["1"]):
        assert torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b)
    assert len(traj["0"]) == len(traj["1"]) == 6
    for i, ((xa, x0a), (xb, x0b)) in enumerate(zip(traj["0"], traj["1"])):
        assert torch.equal(xa, xb) and torch.equal(x0a, x0b), i
        assert x0b.abs().max() <= 1, i
    assert out["1"][1].abs().max() <= 1
    plain = _sample(name, long_, m, _sampler(name), **kw)
    assert not torch.equal(plain[1], out["1"][1])


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("long_", [False, True], ids=["short", "long"])
@pytest.mark.parametrize("name", ["ddim", "dpm++"])
def test_thresholded_graph_nodes(name, long_, guided):
    """No memset node, and exactly the select's launches more kernel nodes than with the option
    off (the thresholded step kernel takes the place of the plain one)."""
    from vdiff import ops
    from vdiff.engine import (DDIMGraph, DPMGraph, LongDDIMGraph, LongDPMGraph,
                              WindowedDenoiser)
    from vdiff.schedulers import WindowPlan
    m = _model(True)
    shape, cond, feats = _case(8 if long_ else 4)
    kw = dict(guidance_scale=7.5, guidance_rescale=0.7) if guided else {}
    counts = {}
    with torch.no_grad(), ops.frozen_weights():
        for thr in (False, True):
            sampler = _sampler(name, **(dict(dynamic_threshold=0.995) if thr else {}))
            xt = torch.randn(shape, device=dev, generator=torch.Generator(dev).manual_seed(3))
            if long_:
                windows = WindowedDenoiser(m, WindowPlan(8, 4, 2), cond, feats, xt, guided)
                gr = (LongDDIMGraph if name == "ddim" else LongDPMGraph)(m, sampler, windows, xt,
                                                                         **kw)
            else:
                gr = (DDIMGraph if name == "ddim" else DPMGraph)(m, sampler, cond, feats, xt, **kw)
            gr.capture()
            counts[thr] = gr.node_types()
            got, x0 = gr.step(0)
            assert torch.isfinite(got).all() and torch.isfinite(x0).all()
            if thr:
                assert x0.abs().max() <= 1
    assert counts[True].get("memset", 0) == 0 and counts[False].get("memset", 0) == 0, counts
    assert counts[True]["kernel"] == counts[False]["kernel"] + SELECT_LAUNCHES, counts
    assert {k: v for k, v in counts[True].items() if k != "kernel"} == \
        {k: v for k, v in counts[False].items() if k != "kernel"}, counts


# ------------------------------------------------------------------ 5. the entry point
@pytest.mark.parametrize("extra", [["--sampler", "ddim", "--dynamic-threshold", "0.995"],
                                   ["--sampler", "dpm++", "--dynamic-threshold", "0.9",
                                    "--threshold-max", "1.5", "--guidance-rescale", "0.5"]],
                         ids=["ddim", "dpm++"])
def test_sampling_entry(tmp_path, extra):
    out_dir = tmp_path / "imgs"
    out = subprocess.run([sys.executable, os.path.join(DROPIN, "test.py"), "--random-init",
                          "--steps", "4", "--image-size", "32", "--save-every", "1",
                          "--guidance-scale", "7.5", "--out-dir", str(out_dir)] + extra,
                         cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    files = sorted(p for p in os.listdir(out_dir) if p.endswith(".npy"))
    assert len(files) == 4, files
    for f in files:
        x0 = np.load(out_dir / f)
        assert x0.shape == (1, 3, 32, 32) and np.isfinite(x0).all()
