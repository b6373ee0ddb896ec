"""Weight packing (vd_conv_pack_weight, vd_conv_pack_weights), the long-clip window kernels
(vd_window_gather, vd_window_blend) and the frame transform (vd_frames_resize_normalize) on
guarded, NaN-poisoned buffers (tests/_guarded.py), through vdiff._lib.call with the operands and
call order of vdiff.ops / vdiff.data.

Every input -- each fp32 weight, the pack descriptor table, the window tables, the frames, both
resize plans -- lives between two 1 MiB guards of a NaN pattern (integer tables: a value far
outside every index range); every output starts out as the pattern; the frame transform's tmp is
scratch of exactly n * H * OW * 3 bytes.  After each call the outputs are fully written, guards
and gaps bit-intact, the inputs bit-identical.  Comparisons are the unguarded tests': bit-exact
packing against the torch layout, torch indexing for the gather, _window_cases.blend_ref64 for the
blend, PIL bit for bit for the frames.
"""
import numpy as np
import pytest
import torch

from conftest import record_metric

from oracle.fixtures import seeded

import _window_cases as wc
from _bounds import assert_elementwise
from _guarded import Guarded, assert_clean

pytestmark = pytest.mark.gpu
dev = "cuda"
DTYPES = [torch.bfloat16, torch.float32]
f32, i32, u8 = torch.float32, torch.int32, torch.uint8


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dt(dtype):
    from vdiff import _lib
    return _lib.VD_BF16 if dtype == torch.bfloat16 else _lib.VD_F32


# ------------------------------------------------------------------ weight packing
# the jobs of test_conv_pack_weights_batched_equals_per_job (ragged 195 -> 200 and 3 -> 8; 27, 9
# and 1 taps; the 512-tap element-wise fallback; both layouts) and a generic tap count, 8
JOBS = [(64, 195, 27, 0), (64, 195, 27, 1), (3, 64, 27, 0), (3, 64, 27, 1), (256, 512, 1, 0),
        (256, 512, 1, 1), (130, 70, 9, 0), (130, 70, 9, 1), (16, 4, 512, 0), (16, 4, 512, 1),
        (20, 13, 8, 0), (20, 13, 8, 1)]
_PACK = np.dtype([("w", "<u8"), ("out", "<u8"), ("Co", "<i4"), ("Ci", "<i4"), ("taps", "<i4"),
                  ("Cip", "<i4"), ("Cop", "<i4"), ("tr", "<i4"), ("start", "<i8")])
assert _PACK.itemsize == 48


def _pack_ref(w, Co, Ci, taps, Cip, Cop, tr, dtype):
    """The packed operand by torch indexing (test_conv_pack_weight): zero-padded channels, one
    rounding to the dtype."""
    wr = w.reshape(Co, Ci, taps).to(dtype)
    if tr:
        ref = torch.zeros(Cip, taps, Cop, dtype=dtype)
        ref[:Ci, :, :Co] = wr.permute(1, 2, 0)
    else:
        ref = torch.zeros(Co, taps, Cip, dtype=dtype)
        ref[:, :, :Ci] = wr.permute(0, 2, 1)
    return ref


@pytest.mark.parametrize("dtype", DTYPES)
def test_guarded_conv_pack_weights(dtype):
    """Every job through vd_conv_pack_weight on its own and through ONE vd_conv_pack_weights
    launch whose descriptor table is guarded: both bit-equal to the torch layout, hence to each
    other, with no byte written outside an output and no fp32 read outside a weight (a NaN read
    past a ragged channel count would land in the zero padding or in a packed value)."""
    from vdiff import _lib
    DT = _dt(dtype)
    rows = np.zeros(len(JOBS), _PACK)
    W, OUT1, OUTN, refs, total = [], [], [], [], 0
    for r, (Co, Ci, taps, tr) in enumerate(JOBS):
        Cip, Cop = (Ci + 7) // 8 * 8, (Co + 7) // 8 * 8
        w = seeded((Co, Ci, taps), 80 + r)
        shape = (Cip, taps, Cop) if tr else (Co, taps, Cip)
        Wg = Guarded((Co, Ci, taps), f32, dev, w, name=f"w[{r}]")
        O1 = Guarded(shape, dtype, dev, name=f"out[{r}] (one job)")
        ON = Guarded(shape, dtype, dev, name=f"out[{r}] (batched)")
        _lib.call("vd_conv_pack_weight", Wg.ptr, Co, Ci, taps, Cip, Cop, tr, DT, O1.ptr, _st())
        assert_clean([O1], [Wg], what=f"pack_weight job {JOBS[r]} {dtype}")
        ref = _pack_ref(w, Co, Ci, taps, Cip, Cop, tr, dtype)
        assert torch.equal(O1.payload(), ref), JOBS[r]
        rows[r] = (Wg.ptr, ON.ptr, Co, Ci, taps, Cip, Cop, tr, total)
        total += ref.numel()
        W.append(Wg), OUT1.append(O1), OUTN.append(ON), refs.append(ref)
    img = torch.from_numpy(rows.view(np.uint8).copy())
    TAB = Guarded((img.numel(),), u8, dev, img, name="pack table")
    _lib.call("vd_conv_pack_weights", TAB.ptr, len(JOBS), total, DT, _st())
    assert_clean(OUTN, W + [TAB], what=f"pack_weights {dtype}")
    for j, (o, ref) in enumerate(zip(OUTN, refs)):
        assert torch.equal(o.payload(), ref), JOBS[j]


# ------------------------------------------------------------------ long-clip windows
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,L,T,S,HW", wc.KERNEL_SHAPES)
def test_guarded_window_gather(B, C, L, T, S, HW, dtype):
    """vd_window_gather with win_dup given and NULL: torch indexing, bit-exact.  Then with start
    entries outside [0, L - T] (negative, L, a huge one): the kernel clamps them, so the result is
    the gather at the clamped starts and nothing outside x is read."""
    from vdiff import _lib
    bf = dtype == torch.bfloat16
    st = wc.starts(L, T, S)
    Wn = len(st)
    x = wc.inputs(B, C, L, HW, bf, seed=1)
    X = Guarded((B, C, L, HW), dtype, dev, x, name="x")
    want = wc.gather_ref(x, L, T, S).to(dtype)
    wild = [(-3, 0), (L, L - T), (1 << 30, L - T), (-(1 << 30), 0)]
    for starts, dup in ((st, True), (st, False),
                        ([wild[w % 4][0] if w % 2 == 0 else s for w, s in enumerate(st)], True)):
        ST = Guarded((Wn,), i32, dev, torch.tensor(starts, dtype=i32), name="starts")
        WIN = Guarded((B * Wn, C, T, HW), dtype, dev, name="win")
        DUP = Guarded((B * Wn, C, T, HW), dtype, dev, name="win_dup") if dup else None
        _lib.call("vd_window_gather", X.ptr, WIN.ptr, DUP and DUP.ptr, ST.ptr, B, C, L, T, Wn, HW,
                  _dt(dtype), _st())
        assert_clean([g for g in (WIN, DUP) if g], [X, ST], what=f"gather {starts} {dtype}")
        if starts is st:
            ref = want
        else:
            clamped = [min(max(s, 0), L - T) for s in starts]
            ref = torch.stack([x[:, :, s:s + T] for s in clamped], 1).reshape(
                -1, C, T, HW).to(dtype)
        assert torch.equal(WIN.payload(), ref), starts
        if DUP:
            assert torch.equal(DUP.payload(), ref), starts


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("blend", wc.BLENDS)
@pytest.mark.parametrize("B,C,L,T,S,HW", wc.KERNEL_SHAPES)
def test_guarded_window_blend(B, C, L, T, S, HW, blend, dtype):
    """vd_window_blend against _window_cases.blend_ref64 with n_terms = the plan's largest
    coverage, as test_blend_against_fp64.  The tables the kernel reads are the plan's with every
    unused slot made hostile: its weight is NaN, and its window index is -1, W (outside [0, W)) or
    a real window that does not hold the frame (local frame outside [0, T)) -- all three must be
    skipped without their weight or any window element being read."""
    from vdiff import _lib
    from vdiff.schedulers import WindowPlan
    bf = dtype == torch.bfloat16
    p = WindowPlan(L, T, S, blend)
    Wn, st = p.num_windows, p.starts.tolist()
    K = p.cover_win.shape[1]
    win = wc.inputs(B * Wn, C, T, HW, bf, seed=2)
    ref, mag = wc.blend_ref64(win, st, p.cover_win, p.cover_wgt, L)
    cw, cg = p.cover_win.clone(), p.cover_wgt.clone()
    for l in range(L):
        away = [w for w in range(Wn) if not 0 <= l - st[w] < T]
        for k in range(K):
            if int(p.cover_win[l, k]) >= 0:
                continue
            cg[l, k] = float("nan")
            cw[l, k] = (-1, Wn, away[0] if away else Wn + 5)[k % 3]
    WIN = Guarded((B * Wn, C, T, HW), dtype, dev, win, name="win")
    ST = Guarded((Wn,), i32, dev, p.starts, name="starts")
    CW = Guarded((L, K), i32, dev, cw, name="cover_win")
    CG = Guarded((L, K), f32, dev, cg, name="cover_wgt")
    OUT = Guarded((B, C, L, HW), dtype, dev, name="out")
    _lib.call("vd_window_blend", WIN.ptr, OUT.ptr, ST.ptr, CW.ptr, CG.ptr, K, B, C, L, T, Wn, HW,
              _dt(dtype), _st())
    what = f"blend B={B} C={C} L={L} T={T} S={S} HW={HW} {blend} {dtype}"
    assert_clean([OUT], [WIN, ST, CW, CG], what=what)
    worst = assert_elementwise(OUT.payload().float(), ref, mag, p.max_coverage, bf, what=what)
    record_metric(test="guarded_window_blend", B=B, C=C, L=L, T=T, S=S, HW=HW, blend=blend,
                  dtype=str(dtype), worst=worst)


# ------------------------------------------------------------------ frames
def _frames(n, H, W, seed):
    """The content of test_gpu_data._frames: smooth ramps plus noise."""
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    base = (np.stack([yy, xx, (yy + xx) / 2], -1) * 255)[None]
    return np.clip(base + g.integers(-40, 40, (n, H, W, 3)), 0, 255).astype(np.uint8)


def _plan(in_size, out_size):
    """vdiff.data._plan: one axis of PIL's plan from vd_resize_plan (host), as guarded inputs."""
    from vdiff import _lib
    cap = 2 * -(-in_size // out_size) + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, cap), np.int32)
    _lib.call("vd_resize_plan", in_size, out_size, bounds.ctypes.data, coef.ctypes.data, cap)
    return (Guarded(bounds.shape, i32, dev, torch.from_numpy(bounds), name="bounds"),
            Guarded(coef.shape, i32, dev, torch.from_numpy(coef), name="coef"), cap)


def _pil(frame, OH, OW):
    """oracle.data.frame_transform with a rectangular size: PIL's resize to (OW, OH), then the
    normalisation; [OH, OW, 3] fp32."""
    from PIL import Image
    im = Image.fromarray(frame).resize((OW, OH), Image.BILINEAR)
    a = np.asarray(im, dtype=np.float32) / 255.0
    return (a - 0.5) / 0.5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W,OH,OW", [(100, 181, 128, 128), (64, 64, 96, 80), (37, 53, 16, 24)])
def test_guarded_frames_resize_normalize(H, W, OH, OW, dtype):
    """vd_frames_resize_normalize, n = 2, beyond its one call site: channels_last 0 and 1, a
    frame stride of the natural size and of 40 elements more (the gap between the frames stays
    the pattern), OH != OW.  Bit for bit PIL's resize to (OW, OH) and the normalisation, rounded
    to bf16 for that dtype, as test_frame_transform_matches_pil_bit_for_bit."""
    from vdiff import _lib
    n = 2
    fr = _frames(n, H, W, H + W)
    ref = torch.from_numpy(np.stack([_pil(f, OH, OW) for f in fr]))        # [n, OH, OW, 3]
    FR = Guarded((n, H, W, 3), u8, dev, torch.from_numpy(fr), name="frames")
    XB, XC, xk = _plan(W, OW)
    YB, YC, yk = _plan(H, OH)
    nat = 3 * OH * OW
    for cl in (0, 1):
        for stride in (nat, nat + 40):
            what = f"frames {H}x{W}->{OH}x{OW} {dtype} channels_last={cl} stride={stride}"
            TMP = Guarded.workspace(n * H * OW * 3, dev, name="tmp")
            shape = (n, OH, OW, 3) if cl else (n, 3, OH, OW)
            inner = (OW * 3, 3, 1) if cl else (OH * OW, OW, 1)
            OUT = Guarded(shape, dtype, dev, strides=(stride,) + inner, span=n * stride,
                          name="out")
            _lib.call("vd_frames_resize_normalize", FR.ptr, n, H, W, OH, OW, XB.ptr, XC.ptr, xk,
                      YB.ptr, YC.ptr, yk, TMP.ptr, OUT.ptr, _dt(dtype), stride, cl, _st())
            assert_clean([OUT], [FR, XB, XC, YB, YC], [TMP], what=what)
            want = (ref if cl else ref.permute(0, 3, 1, 2)).to(dtype)
            assert torch.equal(OUT.payload(), want), what
