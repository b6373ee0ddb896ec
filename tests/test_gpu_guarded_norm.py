"""GroupNorm(+SiLU), FiLM GroupNorm, LayerNorm, the conditioning concat and the nearest upsample on
guarded, NaN-poisoned buffers (tests/_guarded.py), through vdiff._lib.call with the operands and
call order of vdiff.ops (GroupNormSiLUFn, GroupNormFiLMSiLUFn, LayerNormFn, CondConcatFn,
UpsampleFn), on buffers that are the test's own.

Every input lives between two 1 MiB guards of a NaN pattern; every output (y, mean, rstd, dx,
dgamma, dbeta, dfilm, dw, db, d_imc, d_audio) starts out as the pattern; every workspace is exactly
*_workspace_size() bytes of 0xFF, a fresh one per call as in vdiff.ops.  After each call the
outputs are fully written, all guards are bit-intact and the inputs bit-identical to before.  The
values are judged by the references and element-wise terms of test_gpu_groupnorm_bounds.py,
test_gpu_film_bounds.py and test_gpu_layernorm_bounds.py, imported unchanged (a NaN read from a
guard or a stale workspace slot is a violation there by construction); the concat and the
upsample bit-exactly, or at the tolerances of tests/test_gpu_elementwise.py where that file has
one (the backward sums).
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import record_metric

from oracle.fixtures import rel_l2, seeded

from _bounds import assert_elementwise, bf16r
from _guarded import Guarded, assert_clean
from test_gpu_film_bounds import film_ref
from test_gpu_groupnorm_bounds import EPS, G, SHAPES, gn_ref
from test_gpu_layernorm_bounds import CASES as LN_CASES
from test_gpu_layernorm_bounds import EPS as LN_EPS
from test_gpu_layernorm_bounds import case_id, ln_inputs, ln_judge, ln_stat_bounds

pytestmark = pytest.mark.gpu
dev = "cuda"
DTYPES = [torch.bfloat16, torch.float32]
f32 = torch.float32


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ GroupNorm / FiLM
BIG = (2, 192, 3, 9, 11)
GN_CASES = [(s, "plain") for s in SHAPES] + [(BIG, "dropout"), (BIG, "dadd")]


@pytest.mark.parametrize("film", [False, True], ids=["gn", "film"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,variant", GN_CASES)
def test_guarded_groupnorm(shape, variant, dtype, film):
    """vd_groupnorm_silu_fwd + vd_groupnorm_silu_bwd_add (dadd NULL, or given in the "dadd"
    variant) and vd_groupnorm_film_silu_fwd + _bwd_add, SiLU on; "dropout": p = 0.25, the mask
    recovered from y != 0 as in test_gpu_groupnorm_bounds._check.  Same inputs, seeds, reference,
    n_terms and __expf allowance as that file's and test_gpu_film_bounds'.  Largest error / bound
    measured on an MI355X, GN | FiLM: bf16 y 0.96 | 0.98, dx 0.93 | 0.87; fp32 y 0.051 | 0.061,
    dx 0.016 | 0.018; dgamma 0.014 | 0.017, dbeta 0.022 | 0.025, dscale 0.037, dshift 0.054."""
    from vdiff import _lib, ops
    B, C = shape[:2]
    S = 1
    for n in shape[2:]:
        S *= n
    bf = dtype == torch.bfloat16
    rnd = bf16r if bf else (lambda u: u)
    drop = 0.25 if variant == "dropout" else 0.0
    seed = 1234 if drop else 0
    x = rnd(seeded(shape, 60) * 1.5 + 2.0)
    dy = rnd(seeded(shape, 61))
    gamma, beta = 1 + 0.3 * seeded((C,), 62), 0.3 * seeded((C,), 63)
    dadd = rnd(seeded(shape, 64)) if variant == "dadd" else None
    s, t = 0.5 * seeded((B, C), 65), 0.5 * seeded((B, C), 66)
    DT = ops._DT[dtype]
    what = f"{'film' if film else 'gn'} {variant} {shape} {dtype}"
    nws = _lib.lib().vd_groupnorm_workspace_size(B, S, C, G)

    X = Guarded.cl(shape, dtype, dev, x, name="x")
    GA = Guarded((C,), f32, dev, gamma, name="gamma")
    BE = Guarded((C,), f32, dev, beta, name="beta")
    FI = Guarded((B, 2 * C), f32, dev, torch.cat([s, t], 1), name="film") if film else None
    Y = Guarded.cl(shape, dtype, dev, name="y")
    MEAN = Guarded((B * G,), f32, dev, name="mean")
    RSTD = Guarded((B * G,), f32, dev, name="rstd")
    WS = Guarded.workspace(nws, dev)
    if film:
        _lib.call("vd_groupnorm_film_silu_fwd", X.ptr, GA.ptr, BE.ptr, FI.ptr, Y.ptr, MEAN.ptr,
                  RSTD.ptr, B, S, C, G, EPS, 1, drop, seed, DT, WS.ptr, _st())
    else:
        _lib.call("vd_groupnorm_silu_fwd", X.ptr, GA.ptr, BE.ptr, Y.ptr, MEAN.ptr, RSTD.ptr, B, S,
                  C, G, EPS, 1, drop, seed, DT, WS.ptr, _st())
    ins = [g for g in (X, GA, BE, FI) if g is not None]
    assert_clean([Y, MEAN, RSTD], ins, [WS], what=what + " fwd")

    DY = Guarded.cl(shape, dtype, dev, dy, name="dy")
    DA = Guarded.cl(shape, dtype, dev, dadd, name="dadd") if dadd is not None else None
    DX = Guarded.cl(shape, dtype, dev, name="dx")
    DG = Guarded((C,), f32, dev, name="dgamma")
    DB = Guarded((C,), f32, dev, name="dbeta")
    DF = Guarded((B, 2 * C), f32, dev, name="dfilm") if film else None
    WS2 = Guarded.workspace(nws, dev)
    MEAN.freeze(), RSTD.freeze()
    if film:
        _lib.call("vd_groupnorm_film_silu_bwd_add", X.ptr, DY.ptr, DA and DA.ptr, GA.ptr, BE.ptr,
                  FI.ptr, MEAN.ptr, RSTD.ptr, DX.ptr, DG.ptr, DB.ptr, DF.ptr, B, S, C, G, 1, drop,
                  seed, DT, WS2.ptr, _st())
    else:
        _lib.call("vd_groupnorm_silu_bwd_add", X.ptr, DY.ptr, DA and DA.ptr, GA.ptr, BE.ptr,
                  MEAN.ptr, RSTD.ptr, DX.ptr, DG.ptr, DB.ptr, B, S, C, G, 1, drop, seed, DT,
                  WS2.ptr, _st())
    assert_clean([g for g in (DX, DG, DB, DF) if g is not None],
                 ins + [g for g in (DY, DA, MEAN, RSTD) if g is not None], [WS2],
                 what=what + " bwd")

    got = [Y.payload().float().reshape(B, C, -1), DX.payload().float().reshape(B, C, -1),
           DG.payload(), DB.payload()]
    if film:
        got += [DF.payload()[:, :C], DF.payload()[:, C:]]
    mask = torch.ones(shape)
    if drop:
        keep = got[0].reshape(shape) != 0
        frac = float(keep.float().mean())
        assert abs(frac - (1 - drop)) < 4 * (drop * (1 - drop) / keep.numel()) ** 0.5 + 1e-3
        mask = keep.double() / (1 - drop)
    n_g = C // G * S
    if film:
        ref, mag = film_ref(x, dy, gamma, beta, s, t, True, mask, dadd, torch.float64)
        r32, _ = film_ref(x, dy, gamma, beta, s, t, True, mask, dadd, torch.float32)
        names = ("y", "dx", "dgamma", "dbeta", "dscale", "dshift")
        n_terms = (n_g, 2 * n_g, n_g + B * S, n_g + B * S, n_g + S, n_g + S)
    else:
        ref, mag = gn_ref(x, dy, gamma, beta, True, mask, dadd, torch.float64)
        r32, _ = gn_ref(x, dy, gamma, beta, True, mask, dadd, torch.float32)
        names = ("y", "dx", "dgamma", "dbeta")
        n_terms = (n_g, 2 * n_g, n_g + B * S, n_g + B * S)
    out = {}
    for name, g_, r_, m_, f_, n_ in zip(names, got, ref, mag, r32, n_terms):
        c = 2 * float(((f_.double() - r_).abs() / m_.clamp_min(1e-300)).max())
        assert c < 1e-4, (name, c)
        out[name] = assert_elementwise(g_, r_, m_, n_, bf and name in ("y", "dx"), c_extra=c,
                                       what=f"{what} {name}")
    print(f"guarded {what}: " + " ".join(f"{k} {v:.3g}" for k, v in out.items()))
    record_metric(test="guarded_gn", film=film, variant=variant, shape=list(shape),
                  dtype=str(dtype), **out)


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", LN_CASES, ids=case_id)
def test_guarded_layernorm(case, dtype):
    """vd_layernorm_fwd / vd_layernorm_bwd: y, dx, dw, db by ln_judge, mean and rstd by
    ln_stat_bounds, as test_ln_elementwise_bounds.  Largest error / bound measured on an MI355X:
    bf16 y 0.97, dx 0.95; fp32 y 0.049, dx 0.013; dw 0.046, db 0.11; mean 0.017, rstd 0.044
    (that test's figures)."""
    from vdiff import _lib, ops
    rows, C, _ = case
    bf = dtype == torch.bfloat16
    x, dy, w, b = ln_inputs(case, bf)
    DT = ops._DT[dtype]
    what = f"layernorm {case_id(case)} {dtype}"
    X = Guarded((rows, C), dtype, dev, x, name="x")
    W = Guarded((C,), f32, dev, w, name="w")
    Bb = Guarded((C,), f32, dev, b, name="b")
    Y = Guarded((rows, C), dtype, dev, name="y")
    MEAN = Guarded((rows,), f32, dev, name="mean")
    RSTD = Guarded((rows,), f32, dev, name="rstd")
    _lib.call("vd_layernorm_fwd", X.ptr, W.ptr, Bb.ptr, Y.ptr, MEAN.ptr, RSTD.ptr, rows, C, LN_EPS,
              DT, _st())
    assert_clean([Y, MEAN, RSTD], [X, W, Bb], what=what + " fwd")
    DY = Guarded((rows, C), dtype, dev, dy, name="dy")
    DX = Guarded((rows, C), dtype, dev, name="dx")
    DW = Guarded((C,), f32, dev, name="dw")
    DB = Guarded((C,), f32, dev, name="db")
    nb = _lib.lib().vd_layernorm_workspace_size(rows, C)
    WS = Guarded.workspace(nb, dev)
    MEAN.freeze(), RSTD.freeze()
    _lib.call("vd_layernorm_bwd", DY.ptr, X.ptr, W.ptr, MEAN.ptr, RSTD.ptr, DX.ptr, DW.ptr, DB.ptr,
              rows, C, DT, WS.ptr, nb, _st())
    assert_clean([DX, DW, DB], [DY, X, W, MEAN, RSTD], [WS], what=what + " bwd")
    got = [g.payload().float() for g in (Y, DX, DW, DB)]
    out = ln_judge(got, x, dy, w, b, bf, what=what)
    mu, rs, e_mu, e_rs = ln_stat_bounds(x)
    out["mean"] = float(((MEAN.payload().double() - mu).abs() / e_mu.clamp_min(1e-300)).max())
    out["rstd"] = float(((RSTD.payload().double() - rs).abs() / e_rs).max())
    print(f"guarded {what}: " + " ".join(f"{k} {v:.3g}" for k, v in out.items()))
    record_metric(test="guarded_ln", rows=rows, C=C, kind=case[2], dtype=str(dtype), **out)
    assert out["mean"] <= 1.0 and out["rstd"] <= 1.0, out


# ------------------------------------------------------------------ conditioning concat
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("five,cpad", [(True, 200), (True, 0), (False, 72)])
def test_guarded_cond_concat(dtype, five, cpad):
    """vd_cond_concat at the shapes of test_cond_concat_matches_torch, bit-exact.  The library
    takes out_cstride >= Cx + Ci + Ca; cpad 0 / 72 is CondConcatFn's out_cstride = Cx + Ci + Ca =
    195 (the per-element kernel), cpad 200 the 16-B chunk kernel, where the five lanes up to
    out_cstride are written as zeros: the comparison with the zero-padded reference asserts
    exactly that, and the next pixel and the back guard that nothing lies beyond."""
    from vdiff import _lib, ops
    B, T, H, W, Cx, Ci, Ca, h, w = 2, 3, 12, 10, 3, 64, 128, 5, 7
    if not five:
        T = 1
    g = torch.Generator().manual_seed(5)
    img = torch.randn((B, Cx, T, H, W), generator=g).to(dtype)
    imc = torch.randn(B, Ci, h, w, generator=g).to(dtype)
    aud = torch.randn(B, T, Ca, generator=g).to(dtype)
    ic = F.interpolate(imc.float(), size=(H, W), mode="nearest").to(dtype)
    ic = ic[:, :, None].expand(B, Ci, T, H, W)
    au = aud.permute(0, 2, 1)[:, :, :, None, None].expand(B, Ca, T, H, W)
    ref = torch.cat([img, ic, au], 1)
    Ct = Cx + Ci + Ca
    cs = max(cpad, Ct)
    if cs > Ct:
        ref = F.pad(ref, [0, 0, 0, 0, 0, 0, 0, cs - Ct])
    IMG = Guarded.cl((B, Cx, T, H, W), dtype, dev, img, name="image")
    IMC = Guarded.cl((B, Ci, h, w), dtype, dev, imc, name="imc")
    AUD = Guarded((B, T, Ca), dtype, dev, aud, name="audio")
    OUT = Guarded.cl((B, cs, T, H, W), dtype, dev, name="out")
    _lib.call("vd_cond_concat", IMG.ptr, IMC.ptr, AUD.ptr, OUT.ptr, B, T, H, W, Cx, h, w, Ci, Ca,
              cs, ops._DT[dtype], _st())
    assert_clean([OUT], [IMG, IMC, AUD], what=f"cond_concat {dtype} five={five} cs={cs}")
    got = OUT.payload()
    assert torch.equal(got, ref)
    assert not bool(got[:, Ct:].any())      # the tail up to out_cstride: zeros


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cs", [43, 200])
@pytest.mark.parametrize("hw", [(5, 7), (12, 10), (4, 5)])
def test_guarded_cond_concat_bwd(dtype, hw, cs):
    """vd_cond_concat_bwd at the shapes and tolerances of test_cond_concat_bwd_matches_torch, with
    out_cstride = Cx + Ci + Ca = 43 (no tail) and 200: d_imc and d_audio fully overwritten from a
    poisoned workspace."""
    from vdiff import _lib, ops
    B, T, H, W, Cx, Ci, Ca = 2, 3, 12, 10, 3, 16, 24
    h, w = hw
    g = torch.Generator().manual_seed(6)
    imc = torch.randn(B, Ci, h, w, generator=g).to(dtype)
    aud = torch.randn(B, T, Ca, generator=g).to(dtype)
    gout = torch.randn((B, cs, T, H, W), generator=g).to(dtype)
    ir = imc.float().clone().requires_grad_(True)
    ar = aud.float().clone().requires_grad_(True)
    ic = F.interpolate(ir, size=(H, W), mode="nearest")[:, :, None].expand(B, Ci, T, H, W)
    au = ar.permute(0, 2, 1)[:, :, :, None, None].expand(B, Ca, T, H, W)
    torch.cat([ic, au], 1).backward(gout.float()[:, Cx:Cx + Ci + Ca])
    DOUT = Guarded.cl((B, cs, T, H, W), dtype, dev, gout, name="dout")
    DI = Guarded((B, h, w, Ci), f32, dev, name="d_imc")
    DA = Guarded((B, T, Ca), f32, dev, name="d_audio")
    WS = Guarded.workspace(_lib.lib().vd_cond_concat_bwd_workspace_size(B, T, H, W, Ca), dev)
    _lib.call("vd_cond_concat_bwd", DOUT.ptr, DI.ptr, DA.ptr, B, T, H, W, Cx, h, w, Ci, Ca, cs,
              ops._DT[dtype], WS.ptr, _st())
    assert_clean([DI, DA], [DOUT], [WS], what=f"cond_concat_bwd {dtype} hw={hw} cs={cs}")
    tol = 1e-6 if dtype == torch.float32 else 1e-2
    e_i = rel_l2(DI.payload().permute(0, 3, 1, 2), ir.grad)
    e_a = rel_l2(DA.payload(), ar.grad)
    assert e_i < tol and e_a < tol, (e_i, e_a)


# ------------------------------------------------------------------ nearest upsample
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [64, 3])
def test_guarded_upsample(dtype, C):
    """vd_upsample_nearest_hw (a pure gather: bit-exact) and _bwd (the sum of the four children
    at the tolerance of test_upsample_fwd_bwd) at that test's shape."""
    from vdiff import _lib, ops
    B, T, H, W = 2, 3, 5, 7
    x = seeded((B, C, T, H, W), 7).to(dtype)
    gy = seeded((B, C, T, 2 * H, 2 * W), 8).to(dtype)
    DT = ops._DT[dtype]
    X = Guarded.cl((B, C, T, H, W), dtype, dev, x, name="x")
    Y = Guarded.cl((B, C, T, 2 * H, 2 * W), dtype, dev, name="y")
    _lib.call("vd_upsample_nearest_hw", X.ptr, Y.ptr, B, T, H, W, C, DT, _st())
    assert_clean([Y], [X], what=f"upsample {dtype} C={C}")
    ref = x.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)
    assert torch.equal(Y.payload(), ref)
    DY = Guarded.cl((B, C, T, 2 * H, 2 * W), dtype, dev, gy, name="dy")
    DX = Guarded.cl((B, C, T, H, W), dtype, dev, name="dx")
    _lib.call("vd_upsample_nearest_hw_bwd", DY.ptr, DX.ptr, B, T, H, W, C, DT, _st())
    assert_clean([DX], [DY], what=f"upsample_bwd {dtype} C={C}")
    gref = gy.double().reshape(B, C, T, H, 2, W, 2).sum((4, 6))
    tol = 1e-6 if dtype == torch.float32 else 3e-2
    torch.testing.assert_close(DX.payload().double(), gref, atol=tol, rtol=tol)
