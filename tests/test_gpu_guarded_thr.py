"""Dynamic thresholding (vd_x0_abs_quantile, vd_ddim_step_thr, vd_dpm_step_thr) on guarded,
NaN-poisoned buffers (tests/_guarded.py), through vdiff._lib.call with the operands and call order
of vdiff.ops.

Every tensor, table, timestep vector, the DPM step word, the threshold vector s and both
workspaces live between two guards of a NaN pattern; s and every output start out as the pattern;
the select's workspace is exactly vd_x0_quantile_workspace_size bytes of 0xFF, a fresh one per
call, and the statistics workspace is the one vd_cfg_stats just filled.  After each call the
outputs are fully written (s: all B entries), guards and gaps bit-intact, inputs bit-identical.
Values are judged by tests/_thr_cases.py, as tests/test_gpu_thr.py judges them.

Alignment: the three shapes of _cfg_cases (P = 105 and the ragged 5000 among them), and the 8-wide
shape with one operand's pointer one element past a 16-byte boundary (off = 1), which must take
the scalar path: the same values, no access past the tensor."""
import math

import pytest
import torch

from conftest import record_metric

import _cfg_cases as cfg
import _dpm_cases as dpm
import _thr_cases as cases
from _bounds import assert_elementwise
from _guarded import Guarded, assert_clean, assert_finite

pytestmark = pytest.mark.gpu
dev = "cuda"
DTYPES = [torch.bfloat16, torch.float32]
f32 = torch.float32
CASES = [(B, P, 0) for B, P in cfg.SHAPES] + [(cfg.SHAPES[0][0], cfg.SHAPES[0][1], 1)]
assert cfg.SHAPES[0][1] % 8 == 0 and cfg.SHAPES[1][1] % 8 != 0
W = cases.W


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dt(dtype):
    from vdiff import _lib
    return _lib.VD_BF16 if dtype == torch.bfloat16 else _lib.VD_F32


def _in(x, dtype, name, off=0):
    return Guarded.flat(x.shape, dtype, dev, x, off, name)


def _out(shape, dtype, name, off=0):
    return Guarded.flat(shape, dtype, dev, None, off, name)


def _tab(t, name):
    return Guarded.flat(t.shape, t.dtype, dev, t, 0, name)


def _p(g):
    return g.p if g is not None else None


def _check(got, ref, name, bf, what):
    r, m, n, ce = ref[name]
    return assert_elementwise(got, r, m, n, bf, ce, what=f"{what} {name}")


def _stats(C, U, w, B, P, DT, what):
    from vdiff import _lib
    nws = _lib.lib().vd_cfg_workspace_size(B, P)
    WS = Guarded.workspace(nws, dev, name="cfg workspace")
    _lib.call("vd_cfg_stats", C.p, U.p, w, B, P, DT, WS.ptr, nws, _st())
    assert_clean([], [C, U], [WS], what=what + " stats")
    return WS.freeze()


def _threshold(src, ins, rank, tmax, B, P, DT, what):
    """vd_x0_abs_quantile (floor 1) into a guarded s [B] with a fresh 0xFF workspace of exactly
    the advertised size: s fully written and finite, the operands untouched."""
    from vdiff import _lib
    lib = _lib.lib()
    nws = lib.vd_x0_quantile_workspace_size(B, P)
    assert nws == B * (cfg.partials(P)[0] * 256 + 4) * 4
    WS = Guarded.workspace(nws, dev, name="select workspace")
    S = _out((B,), f32, "s")
    _lib.call("vd_x0_abs_quantile", src, rank, 1.0, tmax, B, P, DT, S.p, WS.ptr, nws, _st())
    assert_clean([S], ins, [WS], what=what + " select")
    assert_finite([S], what=what + " select")
    return S.freeze()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,P,off", CASES)
def test_guarded_ddim_thr(B, P, off, dtype):
    """The select on the DDIM rules (eps and v; unguided, guided with rescale 0 and a NULL
    statistics workspace, guided with 0.7) and vd_ddim_step_thr on its s: x_prev_dup and x0 given
    and NULL, z NULL (eta = 0) and given (0.5), x_prev written over xt."""
    from vdiff import _lib
    bf = dtype == torch.bfloat16
    xt, c, u, z = cfg.inputs(B, P, bf)
    t, tp = cfg.timesteps(B)
    acp = cases.acp_table()
    DT = _dt(dtype)
    XT, C, U, Z = (_in(xt, dtype, "xt"), _in(c, dtype, "eps_c"), _in(u, dtype, "eps_u", off),
                   _in(z, dtype, "z"))
    XTo = _in(xt, dtype, "xt (offset)", off)
    Tt, Tp, ACP = _tab(t, "t"), _tab(tp, "t_prev"), _tab(acp, "acp")
    rank = cases.rank(cases.P_THR, P)
    worst = 0.0
    for kind, pid in (("ddim-eps", 0), ("ddim-v", 1)):
        for guide, eta, tmax, dup, want_x0, alias in ((None, 0.0, math.inf, False, True, False),
                                                      (None, 0.5, 2.0, False, False, False),
                                                      ((W, 0.0), 0.0, math.inf, True, True, False),
                                                      ((W, 0.7), 0.5, math.inf, False, True, True),
                                                      ((W, 0.7), 0.0, 2.0, True, False, False)):
            what = (f"{kind} {dtype} B={B} P={P} off={off} guide={guide} eta={eta} tmax={tmax} "
                    f"dup={dup} x0={want_x0} alias={alias}")
            w, phi = guide or (1.0, 0.0)
            WS = _stats(C, U, w, B, P, DT, what) if phi else None
            X = XTo if guide is None else XT   # unguided: xt carries the odd offset (U is not read)
            XA = _in(xt, dtype, "xt (x_prev in place)") if alias else None
            xin = XA or X
            src = _lib.X0Source(x=xin.p, eps=C.p, eps_u=U.p if guide else None, t=Tt.p, acp=ACP.p,
                                cfg_workspace=WS and WS.ptr, rule=_lib.X0_DDIM, prediction=pid,
                                w=w, rescale=phi)
            ins = [xin.freeze() if alias else xin, C, Tt, ACP] + ([U] if guide else []) \
                + ([WS] if WS else [])
            S = _threshold(src, ins, rank, tmax, B, P, DT, what)
            XP = XA if alias else _out((B, P), dtype, "x_prev")
            DUP = _out((B, P), dtype, "x_prev_dup") if dup else None
            X0 = _out((B, P), dtype, "x0") if want_x0 else None
            zz = Z if eta else None
            _lib.call("vd_ddim_step_thr", xin.p, C.p, U.p if guide else None, _p(zz), XP.p, _p(DUP),
                      _p(X0), Tt.p, Tp.p, ACP.p, w, phi, WS and WS.ptr, eta, pid, S.p, B, P, DT,
                      _st())
            assert_clean([g for g in (None if alias else XP, DUP, X0) if g],
                         [C, Tt, Tp, ACP, S] + ([U] if guide else []) + ([WS] if WS else [])
                         + ([Z] if zz else []) + ([] if alias else [xin]), what=what,
                         inouts=[XA] if alias else [])
            assert_finite([XP], what=what)
            base, K = cases.base64(kind, xt, c, u, z, guide, t=t, tp=tp, acp=acp, eta=eta)
            ref = cases.thresholded(base, K, tmax=tmax)
            s_ref, Delta = ref["s"]
            assert ((S.value().double().view(-1, 1) - s_ref).abs() <= Delta).all(), what
            worst = max(worst, _check(XP.value(), ref, "x_prev", bf, what))
            if DUP:
                assert torch.equal(DUP.value(), XP.value()), what
            if X0:
                worst = max(worst, _check(X0.value(), ref, "x0", bf, what))
    print(f"guarded ddim thr {dtype} B={B} P={P} off={off}: largest error / bound {worst:.3g}")
    record_metric(test="guarded_ddim_thr", B=B, P=P, off=off, dtype=str(dtype), worst=worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,P,off", CASES)
def test_guarded_dpm_thr(B, P, off, dtype):
    """The select on the DPM rule and vd_dpm_step_thr on the rows of _dpm_cases.kernel_rows, the
    step word below 0, exact and above n_steps - 1, as test_guarded_dpm: row 0 leaves x0_hist as
    the pattern, which must not reach x_prev and must be fully overwritten; otherwise the history
    is read and written in place."""
    from vdiff import _lib
    bf = dtype == torch.bfloat16
    s = cases.dpm_sampler()
    rows = dpm.kernel_rows(s)
    n = s.steps
    xt, c, u, last = dpm.inputs(B, P, bf)
    DT = _dt(dtype)
    XT, C, U = _in(xt, dtype, "xt"), _in(c, dtype, "eps_c", off), _in(u, dtype, "eps_u")
    COEF = _tab(s.coef, "coef")
    rank = cases.rank(cases.P_THR, P)
    worst = 0.0
    for row, word in ((rows[0], -5), (rows[1], rows[1]), (rows[2], n + 3)):
        STEP = _tab(torch.tensor([word]), "step")
        first = row == rows[0]
        for guide, tmax, dup, alias in ((None, math.inf, False, False), (None, 2.0, False, True),
                                        ((W, 0.0), math.inf, True, False),
                                        ((W, 0.7), math.inf, False, True),
                                        ((W, 0.7), 2.0, True, False)):
            what = (f"dpm {dtype} B={B} P={P} off={off} row={row} step={word} guide={guide} "
                    f"tmax={tmax} dup={dup} alias={alias}")
            w, phi = guide or (1.0, 0.0)
            WS = _stats(C, U, w, B, P, DT, what) if phi else None
            H = _out((B, P), dtype, "x0_hist") if first else _in(last, dtype, "x0_hist")
            XA = _in(xt, dtype, "xt (x_prev in place)") if alias else None
            xin = XA or XT
            src = _lib.X0Source(x=xin.p, eps=C.p, eps_u=U.p if guide else None, coef=COEF.p,
                                step=STEP.p, n_steps=n, cfg_workspace=WS and WS.ptr,
                                rule=_lib.X0_DPM, w=w, rescale=phi)
            ins = [xin.freeze() if alias else xin, C, COEF, STEP] + ([U] if guide else []) \
                + ([WS] if WS else [])
            S = _threshold(src, ins, rank, tmax, B, P, DT, what)
            XP = XA if alias else _out((B, P), dtype, "x_prev")
            DUP = _out((B, P), dtype, "x_prev_dup") if dup else None
            _lib.call("vd_dpm_step_thr", xin.p, C.p, U.p if guide else None, XP.p, _p(DUP), H.p,
                      COEF.p, n, STEP.p, w, phi, WS and WS.ptr, S.p, B, P, DT, _st())
            outs = [g for g in (None if alias else XP, DUP, H if first else None) if g]
            inouts = [g for g in (XA, None if first else H) if g]
            assert_clean(outs, [C, COEF, STEP, S] + ([U] if guide else [])
                         + ([WS] if WS else []) + ([] if alias else [XT]), what=what,
                         inouts=inouts)
            assert_finite([XP, H], what=what)
            base, K = cases.base64("dpm", xt, c, u, last, guide, row=s.coef[row])
            ref = cases.thresholded(base, K, tmax=tmax)
            s_ref, Delta = ref["s"]
            assert ((S.value().double().view(-1, 1) - s_ref).abs() <= Delta).all(), what
            worst = max(worst, _check(XP.value(), ref, "x_prev", bf, what),
                        _check(H.value(), ref, "x0", bf, what))
            if DUP:
                assert torch.equal(DUP.value(), XP.value()), what
    print(f"guarded dpm thr {dtype} B={B} P={P} off={off}: largest error / bound {worst:.3g}")
    record_metric(test="guarded_dpm_thr", B=B, P=P, off=off, dtype=str(dtype), worst=worst)


def test_guarded_identity_select():
    """The stand-alone op's source: x alone, at an odd element offset with P % 8 != 0 and at the
    8-wide shape, every rank's s the sorted element."""
    from vdiff import _lib
    for dtype in DTYPES:
        for (B, P), off in (((2, 105), 1), ((3, 768), 0), ((3, 768), 1)):
            x = cfg.inputs(B, P, dtype == torch.bfloat16)[0]
            X = _in(x, dtype, "x", off)
            want = x.abs().sort(dim=1).values
            for k in (0, cases.rank(0.5, P), P - 1):
                nws = _lib.lib().vd_x0_quantile_workspace_size(B, P)
                WS = Guarded.workspace(nws, dev, name="select workspace")
                S = _out((B,), f32, "s")
                src = _lib.X0Source(x=X.p, rule=_lib.X0_IDENTITY)
                _lib.call("vd_x0_abs_quantile", src, k, 0.0, math.inf, B, P, _dt(dtype), S.p,
                          WS.ptr, nws, _st())
                assert_clean([S], [X], [WS], what=f"identity {dtype} P={P} off={off} k={k}")
                assert torch.equal(S.value(), want[:, k]), (dtype, P, off, k)
