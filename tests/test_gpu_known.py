"""Masked sampling on the GPU, the step kernel: the `known` / `keep` keywords of the four step ops
(vd_ddim_step_known, vd_dpm_step_known) over kinds {ddim-eps, ddim-v, dpm} x guide {none, (7.5,
0), (7.5, 0.7)} x {plain, clip, threshold} x {bf16, fp32} and the shapes of tests/_known_cases.py:
keep == 0 is today's step bit for bit; a mixed mask lies inside the per-element bounds of the
fp64 reference; the model output under keep == 1 reaches no output, NaN included; in-place
operands give the out-of-place bits.  The guard-band tests are tests/test_gpu_guarded_known.py."""
import math

import pytest
import torch

from conftest import record_metric

import _cfg_cases as cfg
import _dpm_cases as dpm
import _known_cases as cases
import _thr_cases as thr
from _bounds import assert_elementwise

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = math.inf


def _dt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _dev3(bf16, shape, *xs):
    """[B, P] CPU tensors as [B, C, S] device tensors of the kernel dtype."""
    return tuple(x.to(device=dev, dtype=_dt(bf16)).view(shape).contiguous() for x in xs)


def _rules(kind, B):
    """[(the reference's operands, the op's)]: the three kernel rows of the 8-step 2M sampler, or
    the per-sample DDIM timesteps (t_prev = -1 among them)."""
    if kind == "dpm":
        s = thr.dpm_sampler()
        coef, idx = s._tables(dev)
        return [(dict(row=s.coef[i]), dict(coef=coef, step=idx[i:i + 1]))
                for i in dpm.kernel_rows(s)]
    t, tp = cases.timesteps(B)
    acp = thr.acp_table()
    return [(dict(t=t, tp=tp, acp=acp), dict(t=t.to(dev), tp=tp.to(dev), acp=acp.to(dev)))]


def _mode_kw(mode):
    return {"plain": {}, "clip": dict(clip=True),
            "threshold": dict(thresh=(cases.P_THR, INF))}[mode]


def _step(kind, xt_d, c_d, u_d, other_d, guide, d, mode, out=None, dup=None, hist=None, **mask):
    """(x_prev, x0) of the op under test; other_d: z (unused, eta = 0) or the 2M history, which
    is cloned unless `hist` is given."""
    from vdiff import ops
    kw = dict(_mode_kw(mode), **mask)
    if kind == "dpm":
        hist = other_d.clone() if hist is None else hist
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
    return assert_elementwise(got.reshape(r.shape), r, m, n, bf16, ce, what=f"{name} {what}")


def _combos(shape):
    """(guide, mode) of a shape: the large batch runs the unguided step's layered grid, which the
    guided and the thresholded steps (B <= 65535) do not have."""
    if shape == cases.BIG_SHAPE:
        return [(None, "plain"), (None, "clip")]
    return [(g, m) for g in cases.GUIDES for m in cases.MODES]


def _keeps(shape):
    B, _, S = shape
    if shape == cases.BIG_SHAPE:
        return [cases.keep_big(B, S), cases.keep(B, S, False)]
    return [cases.keep(B, S, False), cases.keep(B, S, True)]


ALL_SHAPES = cases.SHAPES + [cases.BIG_SHAPE]
_ids = [f"{B}x{C}x{S}" for B, C, S in ALL_SHAPES]


# ------------------------------------------------------------------ 1. keep == 0: today's bits
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_ids)
def test_keep_zero_is_the_unmasked_step(shape, kind, bf16):
    """x_prev, dup and x0 of the masked entry points with keep == 0 (and below 0) everywhere are
    bit-equal to the unmasked entry points'.  (2, 8, 13) is where this needs the masked step to
    run at the unmasked step's width: P = 104 is a multiple of 8, S = 13 is not, and the unmasked
    step's 8-wide and scalar fp32 v-prediction thresholded instantiations differ in the last bit
    of x0 -- 51 of 208 values when the masked step ran scalar there."""
    B, C, S = shape
    xt, c, u, other, xk = cases.inputs(B, C, S, bf16)
    xt_d, c_d, u_d, o_d, xk_d = _dev3(bf16, shape, xt, c, u, other, xk)
    n, bad = 0, []
    for _, d in _rules(kind, B):
        for guide, mode in _combos(shape):
            for Bk in (1, B):
                keep = torch.zeros((Bk, S), device=dev)
                if Bk == B:
                    keep[-1, S // 2] = -0.0
                    keep[0, 0] = -3.0      # k <= 0 is read as 0
                what = f"{kind} {shape} bf16={bf16} guide={guide} {mode} Bk={Bk}"
                dups = [torch.empty_like(xt_d) if guide is not None else None for _ in range(2)]
                want = _step(kind, xt_d, c_d, u_d, o_d, guide, d, mode, dup=dups[0])
                got = _step(kind, xt_d, c_d, u_d, o_d, guide, d, mode, dup=dups[1], known=xk_d,
                            keep=keep)
                for name, g, w_ in (("x_prev", got[0], want[0]), ("x0", got[1], want[1])):
                    if not torch.equal(g, w_):
                        diff = g != w_
                        rel = ((g.double() - w_.double()).abs()[diff]
                               / w_.double().abs()[diff].clamp_min(1e-300)).max()
                        bad.append(f"{name} {what}: {int(diff.sum())} of {diff.numel()} elements "
                                   f"differ, largest relative difference {float(rel):.3g}")
                        print(bad[-1])
                if guide is not None:
                    assert torch.equal(dups[1], dups[0]) and torch.equal(dups[1], got[0]), what
                n += 1
    assert n == len(_rules(kind, B)) * len(_combos(shape)) * 2
    assert not bad, bad


# ------------------------------------------------------------------ 2. a mixed mask against fp64
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_ids)
def test_mixed_mask_against_fp64(shape, kind, bf16):
    B, C, S = shape
    xt, c, u, other, xk = cases.inputs(B, C, S, bf16)
    xt_d, c_d, u_d, o_d, xk_d = _dev3(bf16, shape, xt, c, u, other, xk)
    worst = 0.0
    for host, d in _rules(kind, B):
        for guide, mode in _combos(shape):
            for keep in _keeps(shape):
                what = f"{kind} {shape} bf16={bf16} guide={guide} {mode} Bk={keep.shape[0]}"
                ref = cases.masked(kind, mode, xt, c, u, other, guide, xk, keep, **host)
                dup = torch.empty_like(xt_d) if guide is not None else None
                xp, x0 = _step(kind, xt_d, c_d, u_d, o_d, guide, d, mode, dup=dup, known=xk_d,
                               keep=keep.to(dev))
                r = max(_check(xp, ref, "x_prev", bf16, what), _check(x0, ref, "x0", bf16, what))
                worst = max(worst, r)
                # where keep >= 1, x0 is the known value itself
                one = ref["one"].view(shape).to(dev)
                assert torch.equal(x0.view(shape)[one], xk_d[one]), what
                if dup is not None:
                    assert torch.equal(dup, xp), what
    tag = "bf16" if bf16 else "fp32"
    print(f"masked {kind} {shape} {tag}: largest error / bound {worst:.3g}")
    record_metric(test="known_step_fp64", kind=kind, shape=list(shape), dtype=tag, worst=worst)
    assert 0 < worst <= 1


# ------------------------------------------------------------------ 3. the model under keep == 1
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("shape", cases.SHAPES[:2], ids=_ids[:2])
def test_model_output_under_keep_one_reaches_no_output(shape, kind, bf16):
    B, C, S = shape
    xt, c, u, other, xk = cases.inputs(B, C, S, bf16)
    keep = cases.keep(B, S, True)
    one = (cases.expand(keep, B, C) >= 1)
    # the second model: large, finite and different exactly where keep >= 1
    c2 = torch.where(one, cfg.rounded(1000.0 + 37.5 * c, bf16), c)
    u2 = torch.where(one, cfg.rounded(-800.0 + 21.0 * u, bf16), u)
    assert torch.isfinite(c2).all() and (c2[one] != c[one]).all() and c2[one].abs().min() > 10
    assert torch.equal(c2[~one], c[~one]) and torch.equal(u2[~one], u[~one])
    nan = float("nan")
    c3 = torch.where(one, torch.full_like(c, nan), c)
    u3 = torch.where(one, torch.full_like(u, nan), u)
    xt_d, c_d, u_d, o_d, xk_d = _dev3(bf16, shape, xt, c, u, other, xk)
    c2_d, u2_d, c3_d, u3_d = _dev3(bf16, shape, c2, u2, c3, u3)
    keep_d, one_d = keep.to(dev), one.view(shape).to(dev)
    for host, d in _rules(kind, B):
        for guide in cases.GUIDES:
            for mode in cases.MODES:
                what = f"{kind} {shape} bf16={bf16} guide={guide} {mode}"
                a = _step(kind, xt_d, c_d, u_d, o_d, guide, d, mode, known=xk_d, keep=keep_d)
                b = _step(kind, xt_d, c2_d, u2_d, o_d, guide, d, mode, known=xk_d, keep=keep_d)
                for x, y, name in zip(a, b, ("x_prev", "x0")):
                    assert torch.isfinite(x).all() and torch.isfinite(y).all(), (name, what)
                    assert torch.equal(x.view(shape)[one_d], y.view(shape)[one_d]), (name, what)
                if mode == "threshold" or (guide is not None and guide[1] > 0):
                    continue  # f_b and the quantile are statistics of the model's whole output
                n = _step(kind, xt_d, c3_d, u3_d, o_d, guide, d, mode, known=xk_d, keep=keep_d)
                ref = cases.masked(kind, mode, xt, c, u, other, guide, xk, keep, **host)
                for x, y, name in zip(n, a, ("x_prev", "x0")):
                    assert torch.isfinite(x).all(), (name, what)
                    assert torch.equal(x.view(shape)[one_d], y.view(shape)[one_d]), (name, what)
                    # k == 0 elements saw the same model; fractions blend a NaN and are not kept
                    _check(torch.where(one_d, x.view(shape), y.view(shape)), ref, name, bf16, what)


# ------------------------------------------------------------------ 4. aliasing
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("shape", cases.SHAPES[:2], ids=_ids[:2])
def test_in_place_operands_give_the_same_bits(shape, kind, bf16):
    """x_prev written over xt (with the doubled input's second half as dup when guided), and the
    2M history read and written in place: the bits of the out-of-place call."""
    B, C, S = shape
    xt, c, u, other, xk = cases.inputs(B, C, S, bf16)
    xt_d, c_d, u_d, o_d, xk_d = _dev3(bf16, shape, xt, c, u, other, xk)
    keep_d = cases.keep(B, S, True).to(dev)
    n = 0
    for _, d in _rules(kind, B):
        for guide in cases.GUIDES:
            if kind != "dpm" and guide is None:
                continue  # ops.ddim_step has no `out`
            for mode in cases.MODES:
                what = f"{kind} {shape} bf16={bf16} guide={guide} {mode}"
                xp, x0 = _step(kind, xt_d, c_d, u_d, o_d, guide, d, mode, known=xk_d, keep=keep_d)
                x2 = torch.cat([xt_d, xt_d])
                hist = o_d.clone()
                xa, x0a = _step(kind, x2[:B], c_d, u_d, o_d, guide, d, mode, out=x2[:B],
                                dup=x2[B:] if guide is not None else None, hist=hist,
                                known=xk_d, keep=keep_d)
                assert xa.data_ptr() == x2.data_ptr(), what
                assert torch.equal(x2[:B], xp) and torch.equal(x0a, x0), what
                if guide is not None:
                    assert torch.equal(x2[B:], xp), what
                if kind == "dpm":
                    assert x0a.data_ptr() == hist.data_ptr() and torch.equal(hist, x0), what
                n += 1
    assert n > 0
