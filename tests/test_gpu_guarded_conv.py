"""The conv entry points on guarded, NaN-poisoned buffers (tests/_guarded.py): vd_conv3d_fwd,
vd_conv3d_bwd_data, vd_conv3d_bwd_weight_det and vd_channel_sums through vdiff._lib.call, with the
operands, descriptors and call order of vdiff.ops.ConvFn, on buffers that are the test's own.
The accumulating vd_conv3d_bwd_weight runs after the deterministic one, into a zeroed guarded
[Cop][taps][Cip] buffer that is read and written in place, and is held to the same bound.

Every operand (x, packed weights, bias, chan_add, residual, dy) lives between two 1 MiB guards of
a NaN pattern, and so do y, dx and dw, which start out as the pattern; every workspace is exactly
*_workspace_size() bytes of 0xFF.  After each call: the outputs are fully written, guards and gap
lanes of the outputs are bit-intact, the inputs are bit-identical to before, and the values are
inside the element-wise bound of tests/_bounds.py against the fp64 conv -- the check of
test_gpu_conv_bounds._check_case, unchanged, in which a NaN that leaked in from a guard, a gap lane
or a stale workspace slot is a violation by construction.

The rows are test_gpu_conv_bounds.CASES (its comments say which branch of conv.hip each takes),
in bf16 on the default kernel selection, plus:
  halo   rows 0-3 under ops.conv_halo(0) and ops.conv_halo(3);
  fp32   rows 4, 5, 6, 21 in parity mode, operands not rounded to bf16 (conv_gemm_kernel<float>,
         conv_wgrad_kernel<float>; the strided row 6 runs the strided bwd-data directly, as
         ConvFn.backward does in fp32).  The bound is the fp32 term of _bounds alone,
         2 (n + 2) 2^-24 mag: v_mfma_f32_16x16x4_f32 rounds each product-and-add once, so a
         length-n dot product in any order is within gamma_n mag <= 1.001 n 2^-24 mag (Higham,
         Accuracy and Stability, eq. 3.5) and the epilogue adds three more roundings; the existing
         term holds with a factor of two to spare and nothing new is derived;
  pad    Ci = 3 -> 8, Ci = 195 -> 200, and Co = 3 (dy padded to 8 for the backward, dw written as
         [3][Ci][taps]), the channel padding of the model's first and last convs;
  cs     rows 3, 4, 9, 12, 20, 24 with x_cstride = Ci + 8 and y_cstride = Co + 8 (pixel strides
         with 8 gap lanes: NaN under x, dy and the residual, bit-intact under y and dx), and rows
         3 and 11 forward-only with Co = 80 in y_cstride = 84, which check_desc allows for the
         forward alone: it forces the scalar epilogue and, on row 11, the fall-through from
         pw_gemm_launch (dNs % 8 != 0).
"""
import functools

import pytest
import torch

from conftest import record_metric  # first: puts the repository on sys.path

from oracle.fixtures import rel_l2, seeded

from _bounds import assert_elementwise, bf16r, conv_bwd_ref64, conv_fwd_ref64
from _guarded import Guarded, assert_clean
from test_gpu_conv_bounds import CASES, _inputs

pytestmark = pytest.mark.gpu
dev = "cuda"

# channel padding as the model has it (same tuple layout as CASES)
PAD_CASES = [
    ((2, 3, 2, 6, 7), 64, 3, 1, 1, False),
    ((1, 195, 2, 8, 8), 64, 3, 1, 1, False),
    ((2, 64, 2, 6, 7), 3, 3, 1, 1, False),
]


def _spec(kind, i):
    return PAD_CASES[i] if kind == "pad" else CASES[i]


@functools.lru_cache(maxsize=2)
def _host(kind, i, rounded):
    """Operands and fp64 references of one row, computed once for all its variants.  CASES rows
    in bf16 use test_gpu_conv_bounds._inputs itself; fp32 takes the same seeds without the
    rounding; the padding rows have seeds of their own."""
    shape, Co, k, stride, pad, epi = _spec(kind, i)
    nd, Ci = len(shape) - 2, shape[1]
    r = bf16r if rounded else (lambda t: t)
    if kind == "case" and rounded:
        x, w, b = _inputs(i)
    else:
        s = i if kind == "case" else 100 + i
        x = r(seeded(shape, 1000 + s))
        w = r(seeded((Co, Ci) + (k,) * nd, 2000 + s) / (Ci * k ** nd) ** 0.5)
        b = 0.1 * seeded((Co,), 3000 + s)
    s = i if kind == "case" else 100 + i
    ca = res = None
    ref, mag, n = conv_fwd_ref64(x, w, b, stride, pad)
    if epi:
        ca = seeded((shape[0], Co), 4000 + s)
        res = r(seeded(tuple(ref.shape), 5000 + s))
        ref, mag, n = conv_fwd_ref64(x, w, b, stride, pad, ca, res)
    dy = r(seeded(tuple(ref.shape), 6000 + s))
    return dict(x=x, w=w, b=b, ca=ca, res=res, dy=dy, y=(ref, mag, n),
                bwd=conv_bwd_ref64(x, w, dy, stride, pad))


def _run(kind, i, dt=torch.bfloat16, x_gap=0, y_cs=None, fwd_only=False, tag=""):
    """One row through the three entry points as ConvFn.forward / .backward call them; returns
    the largest error / bound ratios (y, dx, dw)."""
    from vdiff import _lib, ops
    spec = _spec(kind, i)
    shape, Co, k, stride, pad, epi = spec
    h = _host(kind, i, dt == torch.bfloat16)
    nd, B, Ci = len(shape) - 2, shape[0], shape[1]
    tup = lambda v: (v,) * nd if isinstance(v, int) else tuple(v)  # noqa: E731
    _, kk, s, p, sp, out = ops._geom(shape, (Co, Ci) + (k,) * nd, tup(stride), tup(pad))
    taps = kk[0] * kk[1] * kk[2]
    Cip, Cop = (Ci + 7) // 8 * 8, (Co + 7) // 8 * 8
    x_cs = Cip + x_gap if x_gap else 0
    y_cs = y_cs or 0
    DT, bf = ops._DT[dt], dt == torch.bfloat16
    st = torch.cuda.current_stream().cuda_stream
    what = f"{tag}{kind} {i} {spec} {'bf16' if bf else 'fp32'} x_cs={x_cs} y_cs={y_cs}"
    wd = h["w"].to(dev)

    def packed(Cop_, transpose, name):
        t = ops._pack_weight_now(wd, Co, Ci, taps, Cip, Cop_, transpose, dt)
        return Guarded(t.shape, dt, dev, data=t, name=name)

    # ---- forward (ConvFn.forward)
    X = Guarded.cl([B, Cip] + sp, dt, dev, ops._pad_channels(h["x"].reshape([B, Ci] + sp), Cip),
                   x_cs, "x")
    WF = packed(Co, False, "w_fwd")
    Bi = Guarded((Co,), torch.float32, dev, h["b"], name="bias")
    CA = RES = None
    if epi:
        CA = Guarded((B, Co), torch.float32, dev, h["ca"], name="chan_add")
        # the residual has y's pixel stride: the kernels read residual + m * dNs + n
        RES = Guarded.cl([B, Co] + out, dt, dev, h["res"].reshape([B, Co] + out), y_cs, "residual")
    Y = Guarded.cl([B, Co] + out, dt, dev, cstride=y_cs, name="y")
    d = ops._desc(B, sp, Cip, out, Co, kk, s, p, DT, x_cs, y_cs)
    _lib.call("vd_conv3d_fwd", d, X.ptr, WF.ptr, Bi.ptr, CA and CA.ptr, RES and RES.ptr, Y.ptr, st)
    assert_clean([Y], [g for g in (X, WF, Bi, CA, RES) if g is not None], what=what + " fwd")
    ref, mag, n = h["y"]
    ry = assert_elementwise(Y.payload().float().reshape(ref.shape), ref, mag, n, bf,
                            what=what + " y")
    if fwd_only:
        print(f"guarded conv {what}: err/bound y {ry:.3f}")
        record_metric(test="guarded_conv", tag=tag, kind=kind, case=i, fp32=not bf, x_cs=x_cs,
                      y_cs=y_cs, y=ry)
        return ry, None, None

    # ---- backward (ConvFn.backward): dy and the descriptor's Co padded to a multiple of 8
    dx, dxm, n_dx, dw, dwm, n_dw = h["bwd"]
    dyp = ops._pad_channels(h["dy"].reshape([B, Co] + out), Cop)
    db = ops._desc(B, sp, Cip, out, Cop, kk, s, p, DT, x_cs, y_cs)
    DY = Guarded.cl([B, Cop] + out, dt, dev, dyp, y_cs, "dy")
    WB = packed(Cop, True, "w_bwd")
    DX = Guarded.cl([B, Cip] + sp, dt, dev, cstride=x_cs, name="dx")
    if bf and any(v > 1 for v in s):
        # the zero-dilated unit-stride form of a strided bf16 bwd-data
        uo = [sp[j] + 2 * p[j] - kk[j] + 1 for j in range(3)]
        dyd = torch.zeros([B, Cop] + uo)
        dyd[:, :, ::s[0], ::s[1], ::s[2]] = dyp
        DYD = Guarded.cl([B, Cop] + uo, dt, dev, dyd, y_cs, "dy (dilated)")
        d1 = ops._desc(B, sp, Cip, uo, Cop, kk, [1, 1, 1], p, DT, x_cs, y_cs)
        _lib.call("vd_conv3d_bwd_data", d1, DYD.ptr, WB.ptr, DX.ptr, st)
        assert_clean([DX], [DYD, WB], what=what + " bwd_data")
    else:
        _lib.call("vd_conv3d_bwd_data", db, DY.ptr, WB.ptr, DX.ptr, st)
        assert_clean([DX], [DY, WB], what=what + " bwd_data")
    got = DX.payload().float()
    assert not bool(got[:, Ci:].any()), what + " dx: padding channels are not zero"
    rdx = assert_elementwise(got[:, :Ci].reshape(dx.shape), dx, dxm, n_dx, bf, what=what + " dx")

    # dw is [Co_out][Ci_out][taps], exactly that many floats
    DW = Guarded(tuple(h["w"].shape), torch.float32, dev, name="dw")
    nws = _lib.lib().vd_conv3d_bwd_weight_workspace_size(db)
    WS = Guarded.workspace(nws, dev, "wgrad workspace")
    _lib.call("vd_conv3d_bwd_weight_det", db, X.ptr, DY.ptr, DW.ptr, Co, Ci, WS.ptr, nws, st)
    assert_clean([DW], [X, DY], [WS], what=what + " bwd_weight_det")
    rdw = assert_elementwise(DW.payload(), dw, dwm, n_dw, False, what=what + " dw")
    # the accumulating form (ConvFn's split-K A/B path): dw [Cop][taps][Cip] fp32, zeroed by the
    # caller, read and written in place; any summation order lies inside the same bound
    DWA = Guarded((Cop, taps, Cip), torch.float32, dev, torch.zeros(Cop, taps, Cip), name="dw +=")
    _lib.call("vd_conv3d_bwd_weight", db, X.ptr, DY.ptr, DWA.ptr, st)
    assert_clean([], [X, DY], what=what + " bwd_weight", inouts=[DWA])
    acc = DWA.payload()
    assert not bool(acc[Co:].any()) and not bool(acc[:, :, Ci:].any()), what + " dw += padding"
    assert_elementwise(acc[:Co, :, :Ci].permute(0, 2, 1).reshape(dw.shape), dw, dwm, n_dw, False,
                       what=what + " dw +=")
    print(f"guarded conv {what}: err/bound y {ry:.3f} dx {rdx:.3f} dw {rdw:.3f}")
    record_metric(test="guarded_conv", tag=tag, kind=kind, case=i, fp32=not bf, x_cs=x_cs,
                  y_cs=y_cs, y=ry, dx=rdx, dw=rdw)
    return ry, rdx, rdw


CS_ROWS = (3, 4, 9, 12, 20, 24)
FP32_ROWS = (4, 5, 6, 21)


def _variants():
    """Every variant of a row next to the others, so that _host's references are computed once."""
    ps = []
    for i in range(len(CASES)):
        ps.append(pytest.param("case", i, "bf16", id=f"row{i}-bf16"))
        if i < 4:
            ps += [pytest.param("case", i, f"halo{m}", id=f"row{i}-halo{m}") for m in (0, 3)]
        if i in CS_ROWS:
            ps.append(pytest.param("case", i, "cs", id=f"row{i}-cstride"))
        if i in (3, 11):
            ps.append(pytest.param("case", i, "ycs84", id=f"row{i}-ycs84"))
    ps += [pytest.param("case", i, "fp32", id=f"row{i}-fp32") for i in FP32_ROWS]
    ps += [pytest.param("pad", i, "bf16", id=f"pad{i}-bf16") for i in range(len(PAD_CASES))]
    return ps


@pytest.mark.parametrize("kind,i,variant", _variants())
def test_guarded_conv(kind, i, variant):
    """Guards, gaps, full overwrite, untouched inputs and the element-wise bound of
    test_gpu_conv_bounds on fwd, bwd-data and the deterministic bwd-weight (module docstring).
    Largest error / bound measured on an MI355X: bf16 rows y 0.98, dx 0.99, dw 0.02 (the figures
    of test_conv_elementwise_bounds; the halo modes, the strided and the padded variants give
    their rows' own figures to three digits); fp32 y 0.022, dx 0.029, dw 0.074."""
    from vdiff import ops
    if variant == "bf16":
        _run(kind, i)
    elif variant.startswith("halo"):
        with ops.conv_halo(int(variant[4:])):
            _run(kind, i, tag=f"halo mode {variant[4:]} ")
    elif variant == "fp32":
        _run(kind, i, dt=torch.float32)
    elif variant == "cs":
        _run(kind, i, x_gap=8, y_cs=CASES[i][1] + 8)
    else:
        assert CASES[i][1] == 80
        _run(kind, i, y_cs=84, fwd_only=True)


def test_backward_rejects_unaligned_y_cstride():
    """y_cstride = 84 is legal for the forward alone (include/vdiff.h): bwd_data and both weight
    gradients read dy in 16-byte chunks and refuse it before any launch, touching nothing."""
    from vdiff import _lib, ops
    B, Ci, Co, sp = 2, 64, 80, [2, 5, 7]
    d = ops._desc(B, sp, Ci, sp, Co, [1, 1, 1], [1, 1, 1], [0, 0, 0], _lib.VD_BF16, 0, 84)
    bf = torch.bfloat16
    X = Guarded.cl([B, Ci] + sp, bf, dev, torch.zeros([B, Ci] + sp), name="x")
    DY = Guarded.cl([B, Co] + sp, bf, dev, torch.zeros([B, Co] + sp), 84, "dy")
    W = Guarded((Ci, 1, Co), bf, dev, torch.zeros(Ci, 1, Co), name="w_bwd")
    DX = Guarded.cl([B, Ci] + sp, bf, dev, name="dx")
    DW = Guarded((Co, Ci, 1, 1, 1), torch.float32, dev, name="dw")
    WS = Guarded.workspace(1 << 16, dev)
    st = torch.cuda.current_stream().cuda_stream
    assert _lib.lib().vd_conv3d_bwd_weight_workspace_size(d) == 0
    for name, args in (("vd_conv3d_bwd_data", (d, DY.ptr, W.ptr, DX.ptr, st)),
                       ("vd_conv3d_bwd_weight", (d, X.ptr, DY.ptr, DW.ptr, st)),
                       ("vd_conv3d_bwd_weight_det", (d, X.ptr, DY.ptr, DW.ptr, Co, Ci, WS.ptr,
                                                     1 << 16, st))):
        with pytest.raises(RuntimeError, match="y_cstride"):
            _lib.call(name, *args)
    torch.cuda.synchronize()
    assert bool(DX.unwritten().all()) and bool(DW.unwritten().all())
    assert_clean(inputs=[X, DY, W], scratch=[DX, DW, WS], what="rejected y_cstride")


@pytest.mark.parametrize("gap", [0, 8])
@pytest.mark.parametrize("i", [0, 20])
def test_guarded_channel_sums(i, gap):
    """vd_channel_sums on the guarded dy of rows 0 and 20 with cstride 0 and C + 8 (the gap lanes
    NaN), a poisoned workspace and a pattern-filled output, against the fp64 sum at the bar of
    test_gpu_elementwise.test_channel_sums (rel-L2 < 1e-5)."""
    from vdiff import _lib, ops
    shape, C = CASES[i][0], CASES[i][1]
    dy = bf16r(seeded((shape[0], C) + tuple(shape[2:]), 6000 + i))  # "same" convs: y has x's extent
    B, S = shape[0], dy[0, 0].numel()
    cs = C + gap if gap else 0
    DY = Guarded.cl(list(dy.shape), torch.bfloat16, dev, dy, cs, "dy")
    OUT = Guarded((B, C), torch.float32, dev, name="sums")
    WS = Guarded.workspace(_lib.lib().vd_channel_sums_workspace_size(B, C), dev)
    _lib.call("vd_channel_sums", DY.ptr, B, S, C, cs, ops._DT[torch.bfloat16], OUT.ptr, WS.ptr,
              torch.cuda.current_stream().cuda_stream)
    assert_clean([OUT], [DY], [WS], what=f"channel_sums row {i} cstride {cs}")
    ref = dy.double().reshape(B, C, S).sum(-1)
    e = rel_l2(OUT.payload(), ref)
    print(f"guarded channel_sums row {i} cstride {cs}: rel-L2 {e:.3e}")
    assert e < 1e-5
