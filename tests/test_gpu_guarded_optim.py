"""The multi-tensor kernels -- vd_adam_step, vd_ema_update, vd_grad_sumsq, vd_grad_clip -- on
guarded, NaN-poisoned buffers (tests/_guarded.py), through vdiff._lib.call with the operands and
call order of vdiff.ops.

Each pointer array of a descriptor table (p, m, v, g; src and each dst[j]; the gradients) is one
Guarded.ranges payload of its own: the ranges a table row points at, a NaN pattern between them and
1 MiB of it around them.  The tables themselves, the step counts, state[4], the scalars (loss,
num_updates, the skip flag) and the records (lr_out, skip_flag_out, the clip record) are guarded
too; every workspace is exactly vd_grad_clip_workspace_size bytes of 0xFF.

RANGES is the "edge" table: the lengths around one 8-vector and around one block's 2048 elements, a
17-element range that starts one element past a 16-byte boundary in every array, a 24-element range
that starts there in ONE array only (the vector test has to look at every pointer), and a tensor of
three consecutive rows.  MANY is 2051 ranges of 5 elements: more descriptors than the 2048 blocks
the launches cap their grids at, so the grid-stride walk over the table runs.

After each call the gaps and guards of every array are bit-intact, read-only arrays (gradients
for Adam, parameters for EMA) bit-identical, the records fully written, and the values inside the
fp64 comparisons of _adam_cases, _ema_cases and _clip_cases, imported unchanged.

Largest error / bound measured on an MI355X: Adam p 0.96, m 0.56, v 0.65; EMA 0.99; clip norm 0.022.
"""
import math

import numpy as np
import pytest
import torch

from conftest import record_metric

import _adam_cases as ac
import _clip_cases as cc
import _ema_cases as ec
from _guarded import Guarded, assert_clean, assert_finite

pytestmark = pytest.mark.gpu
dev = "cuda"
f32, i64, u8 = torch.float32, torch.int64, torch.uint8


def _st():
    return torch.cuda.current_stream().cuda_stream


class Ranges:
    """Lengths, per-array starts (elements) and the tensor index of every range."""

    def __init__(self, kind):
        self.lengths, self.base, self.off_all, self.off_one, self.tensor = [], [], [], [], []
        pos, tensor = 0, 0

        def add(n, off_all=0, off_one=0, same_tensor=False, gap=True):
            nonlocal pos, tensor
            if gap:
                pos = -(-(pos + 8) // 8) * 8         # >= 8 pattern elements, then 16-B aligned
            if not same_tensor:
                tensor += 1
            self.lengths.append(n)
            self.base.append(pos)
            self.off_all.append(off_all)
            self.off_one.append(off_one)
            self.tensor.append(tensor - 1)
            pos += n + max(off_all, off_one)

        if kind == "edge":
            for n in (1, 7, 8, 9, 2047, 2048, 2049, 2048 + 8 + 3):
                add(n)
            add(17, off_all=1)
            add(24, off_one=1)
            add(16)                                  # one tensor, three consecutive rows
            add(16, same_tensor=True, gap=False)
            add(5, same_tensor=True, gap=False)
        else:
            for _ in range(2051):
                add(5)
        self.n = len(self.lengths)
        self.n_tensors = tensor

    def starts(self, odd_one=False):
        """Starts of one array; odd_one: this is the array whose 24-element range is unaligned."""
        return [b + a + (o if odd_one else 0)
                for b, a, o in zip(self.base, self.off_all, self.off_one)]

    def array(self, name, data=None, odd_one=False):
        return Guarded.ranges(self.lengths, self.starts(odd_one), f32, dev,
                              None if data is None else [torch.from_numpy(d) for d in data],
                              name=name)


def _table(rows, name):
    img = torch.from_numpy(rows.view(np.uint8).copy())
    return Guarded((img.numel(),), u8, dev, img, name=name)


def _scalar(value, dtype, name):
    return Guarded((1,), dtype, dev, torch.tensor([value], dtype=dtype), name=name)


def _cat(arrs):
    return np.concatenate([np.asarray(a) for a in arrs])


def _got(g):
    return _cat([t.numpy() for t in g.range_payloads()])


# ------------------------------------------------------------------ Adam
_ADAM = np.dtype([("p", "<u8"), ("m", "<u8"), ("v", "<u8"), ("g", "<u8"), ("n", "<i8"),
                  ("tensor", "<i8")])
assert _ADAM.itemsize == 48


def _adam_data(R, seed):
    """p, m, v, g per range as _adam_cases.Case draws them: |g| >= 1e-3; tensors with an even
    index are new (count 0, zero moments), the others have count OLD and moments of g's scale."""
    rng = np.random.default_rng(seed)
    counts = np.where(np.arange(R.n_tensors) % 2 == 0, 0, ac.OLD).astype(np.int64)
    p, m, v, g = [], [], [], []
    for n, t in zip(R.lengths, R.tensor):
        gg = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)
        gg = np.where(gg < 0, -1.0, 1.0) * np.maximum(np.abs(gg), 1e-3)
        pp = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 2, n)
        a = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
        b = rng.uniform(0.5, 1.5, n)
        old = counts[t] == ac.OLD
        p.append(pp.astype(np.float32))
        g.append(gg.astype(np.float32))
        m.append((gg * a if old else np.zeros(n)).astype(np.float32))
        v.append((gg * gg * b if old else np.zeros(n)).astype(np.float32))
    return p, m, v, g, counts


def _adam_run(R, mode, skip):
    from vdiff import _lib, ops
    p, m, v, g, counts = _adam_data(R, 7)
    odd = "v"   # the one array whose 24-element range is unaligned
    Pb, Mb, Vb = R.array("p", p), R.array("m", m), R.array("v", v, odd_one=(odd == "v"))
    Gb = R.array("g", g)
    rows = np.zeros(R.n, _ADAM)
    for i in range(R.n):
        rows[i] = (Pb.range_ptr(i), Mb.range_ptr(i), Vb.range_ptr(i), Gb.range_ptr(i),
                   R.lengths[i], R.tensor[i])
    TAB = _table(rows, "adam table")
    STEPS = Guarded((R.n_tensors,), i64, dev, torch.from_numpy(counts), name="steps")
    STATE = Guarded((4,), i64, dev, torch.tensor([3, 1, 0, -1]), name="state")
    LOSS = _scalar(float("nan") if skip else 0.25, f32, "loss")
    NORM = _scalar(1.5, f32, "grad_norm")
    LR, FLAG = Guarded((1,), f32, dev, name="lr_out"), Guarded((1,), i64, dev, name="skip_flag_out")
    h = ops.adam_hyper(ac.LR, ac.BETAS, ac.EPS, max_bad_run=2, **ac.MODES[mode])
    _lib.call("vd_adam_step", TAB.ptr, R.n, _lib.C.byref(h), STEPS.ptr, STATE.ptr, LOSS.ptr,
              NORM.ptr, LR.ptr, FLAG.ptr, _st())
    what = f"adam {mode} ranges={R.n} skip={skip}"
    fixed = [TAB, Gb, LOSS, NORM]
    if skip:    # "launch 1 writes nothing": every array and the counts bit-identical
        assert_clean([LR, FLAG], fixed + [Pb, Mb, Vb, STEPS], what=what, inouts=[STATE])
        assert STATE.payload().tolist() == [3, 2, 1, -1]
        assert FLAG.payload().tolist() == [4]
        assert LR.payload().numpy()[0] == np.float32(ac.LR)
        return None
    assert_clean([LR, FLAG], fixed, what=what, inouts=[Pb, Mb, Vb, STEPS, STATE])
    assert_finite([Pb, Mb, Vb], what=what)
    assert STATE.payload().tolist() == [4, 1, 0, -1]
    assert FLAG.payload().tolist() == [-1] and LR.payload().numpy()[0] == np.float32(ac.LR)
    assert np.array_equal(STEPS.payload().numpy(), counts + 1)
    t = _cat([np.full(n, counts[k] + 1, np.float64) for n, k in zip(R.lengths, R.tensor)])
    args = (_cat(p), _cat(m), _cat(v), _cat(g), t)
    Pr, Mr, Vr, _ = ac.reference(*args, **ac.MODES[mode])
    ep, em, ev = ac.bounds(*args, **ac.MODES[mode])
    every = np.ones(len(t), bool)
    ratios = {"p": ac.worst_ratio(_got(Pb), Pr, ep, every),
              "m": ac.worst_ratio(_got(Mb), Mr, em, every),
              "v": ac.worst_ratio(_got(Vb), Vr, ev, every)}
    assert all(r <= 1.0 for r in ratios.values()), (what, ratios)
    # every element moved: |g| >= 1e-3 and lr = 1e-2 (the _adam_cases docstring)
    assert bool((_got(Pb) != _cat(p)).all())
    return ratios


@pytest.mark.parametrize("mode", list(ac.MODES))
def test_guarded_adam_edge_ranges(mode):
    ratios = _adam_run(Ranges("edge"), mode, False)
    print(f"guarded adam {mode}: largest error / bound {ratios}")
    record_metric(test="guarded_adam", mode=mode, **ratios)


def test_guarded_adam_many_ranges():
    ratios = _adam_run(Ranges("many"), "decoupled", False)
    record_metric(test="guarded_adam_many", **ratios)


@pytest.mark.parametrize("kind", ["edge", "many"])
def test_guarded_adam_skipped_step_writes_nothing(kind):
    _adam_run(Ranges(kind), "l2", True)


# ------------------------------------------------------------------ EMA
_EMA = np.dtype([("src", "<u8"), ("dst", "<u8", (4,)), ("n", "<i8")])
assert _EMA.itemsize == 48
RATES = (0.9999, 0.25)


def _ema_run(R, skip):
    from vdiff import _lib
    rng = np.random.default_rng(11)
    src = [(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 2, n)).astype(np.float32)
           for n in R.lengths]
    dst = [[(s + rng.standard_normal(len(s)) * 0.1).astype(np.float32) for s in src]
           for _ in RATES]
    S = R.array("src", src)
    D = [R.array(f"dst[{j}]", d, odd_one=(j == 1)) for j, d in enumerate(dst)]
    rows = np.zeros(R.n, _EMA)
    for i in range(R.n):
        rows["src"][i] = S.range_ptr(i)
        for j, d in enumerate(D):
            rows["dst"][i, j] = d.range_ptr(i)
        rows["n"][i] = R.lengths[i]
    TAB = _table(rows, "ema table")
    n_upd = 3
    NUM, SKIP = _scalar(n_upd, i64, "num_updates"), _scalar(5 if skip else -1, i64, "skip")
    arr = (_lib.C.c_float * len(RATES))(*RATES)
    _lib.call("vd_ema_update", TAB.ptr, R.n, len(RATES), arr, 1, NUM.ptr, SKIP.ptr, _st())
    what = f"ema ranges={R.n} skip={skip}"
    if skip:
        assert_clean([], [TAB, S, NUM, SKIP] + D, what=what)
        return None
    assert_clean([], [TAB, S, NUM, SKIP], what=what, inouts=D)
    assert_finite(D, what=what)
    worst = 0.0
    for j, rate in enumerate(RATES):
        d = ec.decay32(rate, True, n_upd)
        p_, e_ = _cat(src), _cat(dst[j])
        err = np.abs(_got(D[j]).astype(np.float64) - ec.ref64(p_, e_, d))
        b = ec.bound(p_, e_, d)
        assert (err <= b).all(), (what, j, int(np.argmax(err / b)))
        worst = max(worst, float(np.max(err / b)))
        assert bool((_got(D[j]) != e_).any())
    assert ec.decay32(RATES[0], True, n_upd) < np.float32(RATES[0])     # the warm-up cap acts
    return worst


@pytest.mark.parametrize("kind", ["edge", "many"])
def test_guarded_ema(kind):
    worst = _ema_run(Ranges(kind), False)
    print(f"guarded ema {kind}: largest error / bound {worst:.3g}")
    record_metric(test="guarded_ema", kind=kind, worst=worst)


def test_guarded_ema_skip_flag_writes_nothing():
    _ema_run(Ranges("edge"), True)


# ------------------------------------------------------------------ gradient clipping
_GRAD = np.dtype([("g", "<u8"), ("n", "<i8")])
assert _GRAD.itemsize == 16


def _clip_run(R, clip):
    """vd_grad_sumsq into a fresh workspace, then vd_grad_clip on it.  clip: max_norm = a quarter
    of the norm (coef < 1, every element one fp32 multiply); else max_norm = 4 norms: coef == 1,
    nothing is written."""
    from vdiff import _lib
    rng = np.random.default_rng(2024)
    g = [(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)).astype(np.float32)
         for n in R.lengths]
    Gb = R.array("g", g)
    rows = np.zeros(R.n, _GRAD)
    for i in range(R.n):
        rows[i] = (Gb.range_ptr(i), R.lengths[i])
    TAB = _table(rows, "grad table")
    nws = _lib.lib().vd_grad_clip_workspace_size(R.n)
    assert nws == 4 * R.n
    WS = Guarded.workspace(nws, dev)
    what = f"clip ranges={R.n} clip={clip}"
    _lib.call("vd_grad_sumsq", TAB.ptr, R.n, WS.ptr, nws, _st())
    assert_clean([], [TAB, Gb], [WS], what=what + " sumsq")
    parts = WS.t.view(f32).cpu().numpy().astype(np.float64)
    assert not bool((WS.t.view(torch.int32) == -1).any()), f"{what}: partial left as 0xFF"
    want = np.array([np.sum(x.astype(np.float64) ** 2) for x in g])
    # every partial: a chain of at most depth() fp32 roundings of non-negative terms
    rel = math.expm1(cc.depth() * math.log1p(cc.U)) + cc.REF
    assert (np.abs(parts - want) <= rel * want).all(), what
    ref = float(np.sqrt(want.sum()))
    max_norm = float(np.float32(ref / 4 if clip else ref * 4))
    WS.freeze()
    REC = Guarded((2,), f32, dev, name="record")
    _lib.call("vd_grad_clip", TAB.ptr, R.n, WS.ptr, max_norm, REC.ptr, _st())
    norm, coef = REC.payload().numpy()
    if clip:
        assert_clean([REC], [TAB, WS], what=what, inouts=[Gb])
        assert_finite([Gb], what=what)
    else:   # "with coef == 1 nothing is written"
        assert_clean([REC], [TAB, WS, Gb], what=what)
    r_norm = abs(float(norm) - ref) / (cc.norm_bound(R.n) * ref)
    wantc = min(1.0, max_norm / (ref + 1e-6))
    assert r_norm <= 1.0, (what, norm, ref)
    if clip:
        assert abs(float(coef) - wantc) <= cc.coef_bound(R.n) * wantc and coef < 1
        assert np.array_equal(_got(Gb), _cat(g) * np.float32(coef))     # one fp32 multiply
    else:
        assert coef == np.float32(1.0)
    return r_norm


@pytest.mark.parametrize("clip", [True, False], ids=["clipped", "coef1"])
@pytest.mark.parametrize("kind", ["edge", "many"])
def test_guarded_grad_clip(kind, clip):
    r = _clip_run(Ranges(kind), clip)
    print(f"guarded clip {kind} clip={clip}: norm error / bound {r:.3g}")
    record_metric(test="guarded_clip", kind=kind, clip=clip, norm_ratio=r)
