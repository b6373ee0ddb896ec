"""The losses (vd_mse_loss, vd_diffusion_loss and their backwards), the flat activations (vd_silu,
vd_gelu_tanh and their backwards) and vd_groupnorm_silu_bwd on guarded, NaN-poisoned buffers
(tests/_guarded.py), through vdiff._lib.call with the operands and call order of vdiff.ops
(MSELossFn, DiffusionLossFn, SiLUFn, GeluTanhFn).

Every input lives between two 1 MiB guards of a NaN pattern; every output (loss, per-sample MSE,
gradients, y, dx, dgamma, dbeta) starts out as the pattern; every workspace is exactly
*_workspace_size() bytes of 0xFF, a fresh one per call.  After each call the outputs are fully
written, all guards bit-intact and the inputs bit-identical.  Values are judged as the unguarded
tests judge them, with their references imported unchanged: test_mse_loss's fp64 comparison,
_objective_cases.ref64, the activation references and allowance of test_gpu_activation_bounds.py
and gn_ref of test_gpu_groupnorm_bounds.py.

Largest error / bound measured on an MI355X, bf16 | fp32: diffusion loss 0.995 | 0.14, SiLU 0.995 |
0.62, GELU 0.97 | 0.21, GroupNorm y 0.96 | 0.051, dx 0.93 | 0.016, dgamma 0.014, dbeta 0.022: the
unguarded tests' figures.
"""
import pytest
import torch

from conftest import record_metric

from oracle.fixtures import rel_l2, seeded

import _objective_cases as obj
from _bounds import assert_elementwise, bf16r
from _guarded import Guarded, assert_clean
from test_gpu_activation_bounds import gelu_ref, silu_ref
from test_gpu_groupnorm_bounds import EPS, G, SHAPES, gn_ref

pytestmark = pytest.mark.gpu
dev = "cuda"
DTYPES = [torch.bfloat16, torch.float32]
f32 = torch.float32


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dt(dtype):
    from vdiff import _lib
    return _lib.VD_BF16 if dtype == torch.bfloat16 else _lib.VD_F32


def _in(x, dtype, name, off=0):
    return Guarded.flat(x.shape, dtype, dev, x, off, name)


def _out(shape, dtype, name, off=0):
    return Guarded.flat(shape, dtype, dev, None, off, name)


# ------------------------------------------------------------------ MSE
# 1 .. 9: around one vector; 2048 = one block's range, 2049: two blocks of (1032, 1017); 2059: two
# blocks, the last one ragged (1032, 1027) and a scalar tail; 4101: three blocks (1368, 1368,
# 1365), a ragged last one
MSE_N = [1, 7, 8, 9, 2048, 2049, 2056 + 3, 2 * 2048 + 5]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", MSE_N)
def test_guarded_mse_loss(n, dtype):
    """vd_mse_loss / vd_mse_loss_bwd as test_mse_loss judges them: the loss within 1e-6 relative
    of torch's MSELoss in fp64 on the same values, the gradient 2 (p - e) / n * g at that test's
    rel_l2; the partial sums go through a poisoned workspace of exactly the advertised size."""
    from vdiff import _lib
    bf = dtype == torch.bfloat16
    rnd = bf16r if bf else (lambda v: v)
    g = torch.Generator().manual_seed(n)
    p, e = rnd(torch.randn(n, generator=g)), rnd(torch.randn(n, generator=g))
    DT = _dt(dtype)
    what = f"mse n={n} {dtype}"
    P, E = _in(p, dtype, "pred"), _in(e, dtype, "target")
    OUT = _out((1,), f32, "loss")
    nws = _lib.lib().vd_mse_loss_workspace_size(n)
    assert nws == 4 * max(1, -(-n // 2048))
    WS = Guarded.workspace(nws, dev)
    _lib.call("vd_mse_loss", P.p, E.p, n, DT, OUT.p, WS.ptr, nws, _st())
    assert_clean([OUT], [P, E], [WS], what=what)
    assert not bool((WS.t.view(torch.int32) == -1).any()), f"{what}: partial left as 0xFF"
    loss = float(OUT.value())
    ref = float(torch.nn.functional.mse_loss(p.double(), e.double()))
    assert abs(loss - ref) <= 1e-6 * ref, (loss, ref)
    GS = _in(torch.tensor([0.37]), f32, "grad_loss")
    DP = _out((n,), dtype, "grad_pred")
    _lib.call("vd_mse_loss_bwd", P.p, E.p, GS.p, n, DT, DP.p, _st())
    assert_clean([DP], [P, E, GS], what=what + " bwd")
    gr = (2.0 / n) * (p - e) * 0.37
    assert rel_l2(DP.value(), gr) < (1e-6 if not bf else 4e-3)


def test_mse_loss_refuses_unaligned_pointers():
    """pred / target (and grad_pred) must be 16-byte aligned: VD_EINVAL from the host check, no
    launch -- the outputs keep the pattern."""
    from vdiff import _lib
    n = 64
    x = seeded((n,), 3)
    P, E = _in(x, f32, "pred"), _in(x, f32, "target")
    PO, EO = _in(x, f32, "pred+1", 1), _in(x, f32, "target+1", 1)
    OUT, GS = _out((1,), f32, "loss"), _in(torch.tensor([1.0]), f32, "grad_loss")
    DP, DPO = _out((n,), f32, "grad_pred"), _out((n,), f32, "grad_pred+1", 1)
    nws = _lib.lib().vd_mse_loss_workspace_size(n)
    WS = Guarded.workspace(nws, dev)
    lib = _lib.lib()
    for a, b in ((PO, E), (P, EO)):
        assert lib.vd_mse_loss(a.p, b.p, n, _lib.VD_F32, OUT.p, WS.ptr, nws, _st()) == 1
        assert b"16-B aligned" in lib.vd_last_error()
    for a, b, d in ((PO, E, DP), (P, EO, DP), (P, E, DPO)):
        assert lib.vd_mse_loss_bwd(a.p, b.p, GS.p, n, _lib.VD_F32, d.p, _st()) == 1
        assert b"16-B aligned" in lib.vd_last_error()
    torch.cuda.synchronize()
    for o in (OUT, DP, DPO):
        assert bool(o.unwritten()[o._cover].all()) and o.gaps_intact() and o.guards_intact()
    assert bool((WS.t == 0xFF).all())
    _lib.call("vd_mse_loss", P.p, E.p, n, _lib.VD_F32, OUT.p, WS.ptr, nws, _st())  # aligned: fine
    assert_clean([OUT], [P, E], [WS], what="aligned")


# ------------------------------------------------------------------ the diffusion objective
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,P", obj.SHAPES)
def test_guarded_diffusion_loss(B, P, dtype):
    """vd_diffusion_loss / _bwd for both predictions and both weightings against
    _objective_cases.ref64, as test_loss_and_gradient_against_fp64.  The two tables are guarded;
    VD_PRED_EPS gets an x0 buffer that holds the pattern and must stay untouched; then t below 0
    and above T - 1, which the clamp must keep inside the tables (the bits of the clamped t)."""
    from vdiff import _lib
    bf = dtype == torch.bfloat16
    sa, s1m = obj.tables()
    T = sa.numel()
    t = obj.timesteps(B, T)
    pred, x0, eps = obj.inputs(B, P, bf)
    DT = _dt(dtype)
    PR, X0, EP = _in(pred, dtype, "pred"), _in(x0, dtype, "x0"), _in(eps, dtype, "eps")
    X0P = _out((B, P), dtype, "x0 (not read)").freeze()
    SA, S1 = _in(sa, f32, "sqrt_acp"), _in(s1m, f32, "sqrt_1m_acp")
    g = 2.5
    GS = _in(torch.tensor([g]), f32, "grad_loss")
    nws = _lib.lib().vd_diffusion_loss_workspace_size(B, P)
    assert nws == B * obj.partials(P)[0] * 4

    def run(TT, pid, wid, X, what):
        LOSS, PER = _out((1,), f32, "loss"), _out((B,), f32, "per_sample_mse")
        WS = Guarded.workspace(nws, dev)
        _lib.call("vd_diffusion_loss", PR.p, X.p, EP.p, TT.p, SA.p, S1.p, T, pid, wid, obj.GAMMA,
                  B, P, DT, LOSS.p, PER.p, WS.ptr, nws, _st())
        assert_clean([LOSS, PER], [PR, X, EP, TT, SA, S1], [WS], what=what)
        assert not bool((WS.t.view(torch.int32) == -1).any()), f"{what}: partial left as 0xFF"
        DP = _out((B, P), dtype, "grad_pred")
        _lib.call("vd_diffusion_loss_bwd", PR.p, X.p, EP.p, TT.p, SA.p, S1.p, T, pid, wid,
                  obj.GAMMA, GS.p, B, P, DT, DP.p, _st())
        assert_clean([DP], [PR, X, EP, TT, SA, S1, GS], what=what + " bwd")
        return LOSS.value().reshape(()), PER.value(), DP.value()

    worst = 0.0
    TT = _in(t, torch.int64, "t")
    for prediction in obj.PREDICTIONS:
        for weighting in obj.WEIGHTINGS:
            what = f"diffusion_loss {dtype} B={B} P={P} {prediction} {weighting}"
            pid, wid = _lib.PREDICTIONS[prediction], _lib.LOSS_WEIGHTINGS[weighting]
            got = run(TT, pid, wid, X0P if prediction == "eps" else X0, what)
            ref = obj.ref64(pred, x0, eps, t, sa, s1m, prediction, weighting, obj.GAMMA, g)
            for name, v, ob in zip(("loss", "per_sample", "grad"), got, (False, False, bf)):
                r, m, n = ref[name]
                worst = max(worst, assert_elementwise(v, r, m, n, ob, what=f"{what} {name}"))
    # out-of-range t: the same bits as the clamped t (test_out_of_range_timestep_is_clamped)
    pid, wid = _lib.PREDICTIONS["v"], _lib.LOSS_WEIGHTINGS["min-snr"]
    lo_hi = {2: ([-7, T], [0, T - 1]), 3: ([-7, 1 << 40, T], [0, T - 1, T - 1])}[B]
    want = run(_in(torch.tensor(lo_hi[1]), torch.int64, "t"), pid, wid, X0, "clamped t")
    got = run(_in(torch.tensor(lo_hi[0]), torch.int64, "t"), pid, wid, X0, "out-of-range t")
    for a, b in zip(got, want):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    print(f"guarded diffusion_loss {dtype} B={B} P={P}: largest error / bound {worst:.3g}")
    record_metric(test="guarded_diffusion_loss", B=B, P=P, dtype=str(dtype), worst=worst)


# ------------------------------------------------------------------ SiLU / GELU on flat tensors
# the sizes of test_silu_elementwise_bounds / test_gelu_tanh_elementwise_bounds, and the smallest
# legal one (vd_gelu_tanh needs n % 8 == 0)
ACT = [("silu", n) for n in (1, 7, 8, 1003)] + [("gelu_tanh", n) for n in (8, 1000)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,n", ACT)
def test_guarded_activation(name, n, dtype):
    """vd_silu / vd_silu_bwd and vd_gelu_tanh / vd_gelu_tanh_bwd with the inputs, references,
    n_terms = 1 and fp32-transcendental allowance of test_gpu_activation_bounds._check."""
    from vdiff import _lib
    bf = dtype == torch.bfloat16
    rnd = bf16r if bf else (lambda v: v)
    x, dy = rnd(2 * seeded((n,), 70 + n)), rnd(seeded((n,), 71 + n))
    DT = _dt(dtype)
    X, DY = _in(x, dtype, "x"), _in(dy, dtype, "dy")
    Y, DX = _out((n,), dtype, "y"), _out((n,), dtype, "dx")
    fwd, bwd, ref_fn = {"silu": ("vd_silu", "vd_silu_bwd", silu_ref),
                        "gelu_tanh": ("vd_gelu_tanh", "vd_gelu_tanh_bwd", gelu_ref)}[name]
    _lib.call(fwd, X.p, Y.p, n, DT, _st())
    assert_clean([Y], [X], what=f"{fwd} n={n} {dtype}")
    _lib.call(bwd, X.p, DY.p, DX.p, n, DT, _st())
    assert_clean([DX], [X, DY], what=f"{bwd} n={n} {dtype}")
    ref, mag = ref_fn(x, dy, torch.float64)
    r32, _ = ref_fn(x, dy, torch.float32)
    out = {}
    for what, got, r, m, f in zip(("fwd", "bwd"), (Y.value(), DX.value()), ref, mag, r32):
        c = 2 * float(((f.double() - r).abs() / m.clamp_min(1e-300)).max())
        assert c < 1e-6, c
        out[what] = assert_elementwise(got, r, m, 1, bf, c_extra=c,
                                       what=f"guarded {name} {what} n={n} {dtype}")
    record_metric(test="guarded_" + name, n=n, dtype=str(dtype), **out)


# ------------------------------------------------------------------ GroupNorm backward, no dadd
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_guarded_groupnorm_silu_bwd(shape, dtype):
    """vd_groupnorm_silu_bwd (the entry point without dadd) after vd_groupnorm_silu_fwd, on the
    "plain" cases of test_gpu_guarded_norm.py with its inputs, reference, n_terms and allowance."""
    from vdiff import _lib
    B, C = shape[:2]
    S = 1
    for n in shape[2:]:
        S *= n
    bf = dtype == torch.bfloat16
    rnd = bf16r if bf else (lambda v: v)
    x = rnd(seeded(shape, 60) * 1.5 + 2.0)
    dy = rnd(seeded(shape, 61))
    gamma, beta = 1 + 0.3 * seeded((C,), 62), 0.3 * seeded((C,), 63)
    DT = _dt(dtype)
    what = f"gn_bwd {shape} {dtype}"
    nws = _lib.lib().vd_groupnorm_workspace_size(B, S, C, G)
    X = Guarded.cl(shape, dtype, dev, x, name="x")
    GA = Guarded((C,), f32, dev, gamma, name="gamma")
    BE = Guarded((C,), f32, dev, beta, name="beta")
    Y = Guarded.cl(shape, dtype, dev, name="y")
    MEAN, RSTD = Guarded((B * G,), f32, dev, name="mean"), Guarded((B * G,), f32, dev, name="rstd")
    WS = Guarded.workspace(nws, dev)
    _lib.call("vd_groupnorm_silu_fwd", X.ptr, GA.ptr, BE.ptr, Y.ptr, MEAN.ptr, RSTD.ptr, B, S, C,
              G, EPS, 1, 0.0, 0, DT, WS.ptr, _st())
    assert_clean([Y, MEAN, RSTD], [X, GA, BE], [WS], what=what + " fwd")
    DY = Guarded.cl(shape, dtype, dev, dy, name="dy")
    DX = Guarded.cl(shape, dtype, dev, name="dx")
    DG, DB = Guarded((C,), f32, dev, name="dgamma"), Guarded((C,), f32, dev, name="dbeta")
    WS2 = Guarded.workspace(nws, dev)
    MEAN.freeze(), RSTD.freeze()
    _lib.call("vd_groupnorm_silu_bwd", X.ptr, DY.ptr, GA.ptr, BE.ptr, MEAN.ptr, RSTD.ptr, DX.ptr,
              DG.ptr, DB.ptr, B, S, C, G, 1, 0.0, 0, DT, WS2.ptr, _st())
    assert_clean([DX, DG, DB], [X, DY, GA, BE, MEAN, RSTD], [WS2], what=what)
    got = [Y.payload().float().reshape(B, C, -1), DX.payload().float().reshape(B, C, -1),
           DG.payload(), DB.payload()]
    mask = torch.ones(shape)
    ref, mag = gn_ref(x, dy, gamma, beta, True, mask, None, torch.float64)
    r32, _ = gn_ref(x, dy, gamma, beta, True, mask, None, torch.float32)
    n_g = C // G * S
    out = {}
    for name, g_, r_, m_, f_, n_ in zip(("y", "dx", "dgamma", "dbeta"), got, ref, mag, r32,
                                        (n_g, 2 * n_g, n_g + B * S, n_g + B * S)):
        c = 2 * float(((f_.double() - r_).abs() / m_.clamp_min(1e-300)).max())
        assert c < 1e-4, (name, c)
        out[name] = assert_elementwise(g_, r_, m_, n_, bf and name in ("y", "dx"), c_extra=c,
                                       what=f"{what} {name}")
    record_metric(test="guarded_gn_bwd", shape=list(shape), dtype=str(dtype), **out)
