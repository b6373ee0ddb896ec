"""The masked step (vd_ddim_step_known, vd_dpm_step_known) on guarded, NaN-poisoned buffers
(tests/_guarded.py), through vdiff._lib.call with the operands of vdiff.ops.

Every tensor, table, timestep vector, the 2M step word and the threshold vector live between two
guards of a NaN pattern; `known` and `keep` are frozen inputs, every output starts out as the
pattern.  After each call the outputs are fully written, guards and gaps bit-intact, the inputs
bit-identical.  Values are judged by tests/_known_cases.py, as tests/test_gpu_known.py judges them.

Alignment: the scalar shape, the 8-wide shape, the straddle shape (P % 8 == 0, S % 8 != 0: 8-wide
on the tensors, the mask read one element at a time and wrapped at the end of its row, which the
guards around `keep` would show if it were not), and the 8-wide shape with `known` or `keep` one
element past a 16-byte boundary, which must take the scalar path: the same values, no access past
the tensor."""
import math

import pytest
import torch

from conftest import record_metric

import _dpm_cases as dpm
import _known_cases as cases
import _thr_cases as thr
from _bounds import assert_elementwise
from _guarded import Guarded, assert_clean, assert_finite

pytestmark = pytest.mark.gpu
dev = "cuda"
DTYPES = [torch.bfloat16, torch.float32]
CASES = [cases.SHAPES[0] + ("",), cases.SHAPES[1] + ("",), cases.SHAPES[2] + ("",),
         cases.SHAPES[1] + ("known",), cases.SHAPES[1] + ("keep",)]
W = cases.W
# (guide, mode, x_prev_dup given, x0 given (DDIM), x_prev over xt, keep rows per sample)
COMBOS = [(None, "plain", False, True, False, False),
          (None, "clip", False, False, True, True),
          ((W, 0.0), "plain", True, True, False, True),
          ((W, 0.7), "clip", False, True, True, False),
          ((W, 0.7), "threshold", True, False, False, True),
          (None, "threshold", False, True, False, False)]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dt(dtype):
    from vdiff import _lib
    return _lib.VD_BF16 if dtype == torch.bfloat16 else _lib.VD_F32


def _in(x, dtype, name, off=0):
    return Guarded.flat(x.shape, dtype, dev, x, off, name)


def _out(shape, dtype, name):
    return Guarded.flat(shape, dtype, dev, None, 0, name)


def _tab(t, name):
    return Guarded.flat(t.shape, t.dtype, dev, t, 0, name)


def _p(g):
    return g.p if g is not None else None


def _check(got, ref, name, bf, what):
    r, m, n, ce = ref[name]
    return assert_elementwise(got, r, m, n, bf, ce, what=f"{what} {name}")


def _stats(C, U, w, B, P, DT):
    from vdiff import _lib
    nws = _lib.lib().vd_cfg_workspace_size(B, P)
    WS = Guarded.workspace(nws, dev, name="cfg workspace")
    _lib.call("vd_cfg_stats", C.p, U.p, w, B, P, DT, WS.ptr, nws, _st())
    return WS.freeze()


def _thresh(src, B, P, like):
    """s of the step's own x0 (the select is tests/test_gpu_guarded_thr.py's subject), as a
    guarded input."""
    from vdiff import ops
    s = ops._x0_quantile(src, thr.rank(cases.P_THR, P), 1.0, math.inf, B, P, like)
    return _tab(s.cpu(), "s")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,S,odd", CASES)
def test_guarded_ddim_known(B, C, S, odd, dtype):
    from vdiff import _lib
    bf = dtype == torch.bfloat16
    P = C * S
    xt, c, u, z, xk = cases.inputs(B, C, S, bf)
    t, tp = cases.timesteps(B)
    acp = thr.acp_table()
    DT = _dt(dtype)
    XT, Cc, U = _in(xt, dtype, "xt"), _in(c, dtype, "eps_c"), _in(u, dtype, "eps_u")
    XK = _in(xk, dtype, "known", int(odd == "known"))
    Tt, Tp, ACP = _tab(t, "t"), _tab(tp, "t_prev"), _tab(acp, "acp")
    worst = 0.0
    for kind, pid in (("ddim-eps", 0), ("ddim-v", 1)):
        for guide, mode, dup, want_x0, alias, rows in COMBOS:
            what = (f"{kind} {dtype} {(B, C, S)} odd={odd!r} guide={guide} {mode} dup={dup} "
                    f"x0={want_x0} alias={alias} Bk={B if rows else 1}")
            keep = cases.keep(B, S, rows)
            KEEP = _in(keep, torch.float32, "keep", int(odd == "keep"))
            w, phi = guide or (1.0, 0.0)
            WS = _stats(Cc, U, w, B, P, DT) if phi else None
            XA = _in(xt, dtype, "xt (x_prev in place)") if alias else None
            xin = XA or XT
            Sg = None
            if mode == "threshold":
                src = _lib.X0Source(x=xin.p, eps=Cc.p, eps_u=U.p if guide else None, t=Tt.p,
                                    acp=ACP.p, cfg_workspace=WS and WS.ptr, rule=_lib.X0_DDIM,
                                    prediction=pid, w=w, rescale=phi)
                Sg = _thresh(src, B, P, xin.t)
            XP = XA if alias else _out((B, P), dtype, "x_prev")
            DUP = _out((B, P), dtype, "x_prev_dup") if dup else None
            X0 = _out((B, P), dtype, "x0") if want_x0 else None
            if alias:
                XA.freeze()
            _lib.call("vd_ddim_step_known", xin.p, Cc.p, U.p if guide else None, None, XP.p,
                      _p(DUP), _p(X0), Tt.p, Tp.p, ACP.p, w, phi, WS and WS.ptr, 0.0,
                      int(mode == "clip"), pid, _p(Sg), XK.p, KEEP.p, keep.shape[0], S, B, P, DT,
                      _st())
            assert_clean([g for g in (None if alias else XP, DUP, X0) if g],
                         [Cc, Tt, Tp, ACP, XK, KEEP] + ([U] if guide else [])
                         + ([WS] if WS else []) + ([Sg] if Sg else [])
                         + ([] if alias else [xin]), what=what, inouts=[XA] if alias else [])
            assert_finite([g for g in (XP, DUP, X0) if g], what=what)
            ref = cases.masked(kind, mode, xt, c, u, z, guide, xk, keep, t=t, tp=tp, acp=acp)
            worst = max(worst, _check(XP.value(), ref, "x_prev", bf, what))
            if DUP:
                assert torch.equal(DUP.value(), XP.value()), what
            if X0:
                worst = max(worst, _check(X0.value(), ref, "x0", bf, what))
    print(f"guarded ddim known {dtype} {(B, C, S)} odd={odd!r}: largest error / bound {worst:.3g}")
    record_metric(test="guarded_ddim_known", shape=[B, C, S], odd=odd, dtype=str(dtype),
                  worst=worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,S,odd", CASES)
def test_guarded_dpm_known(B, C, S, odd, dtype):
    """The rows of _dpm_cases.kernel_rows: row 0 leaves x0_hist as the pattern, which must not
    reach x_prev and must be fully overwritten; otherwise the history is read and written in
    place."""
    from vdiff import _lib
    bf = dtype == torch.bfloat16
    P = C * S
    s = thr.dpm_sampler()
    rows_ = dpm.kernel_rows(s)
    n = s.steps
    xt, c, u, last, xk = cases.inputs(B, C, S, bf)
    DT = _dt(dtype)
    XT, Cc, U = _in(xt, dtype, "xt"), _in(c, dtype, "eps_c"), _in(u, dtype, "eps_u")
    XK = _in(xk, dtype, "known", int(odd == "known"))
    COEF = _tab(s.coef, "coef")
    worst = 0.0
    for row in rows_:
        STEP = _tab(torch.tensor([row]), "step")
        first = row == rows_[0]
        for guide, mode, dup, _, alias, rows in COMBOS:
            what = (f"dpm {dtype} {(B, C, S)} odd={odd!r} row={row} guide={guide} {mode} "
                    f"dup={dup} alias={alias} Bk={B if rows else 1}")
            keep = cases.keep(B, S, rows)
            KEEP = _in(keep, torch.float32, "keep", int(odd == "keep"))
            w, phi = guide or (1.0, 0.0)
            WS = _stats(Cc, U, w, B, P, DT) if phi else None
            H = _out((B, P), dtype, "x0_hist") if first else _in(last, dtype, "x0_hist")
            XA = _in(xt, dtype, "xt (x_prev in place)") if alias else None
            xin = XA or XT
            Sg = None
            if mode == "threshold":
                src = _lib.X0Source(x=xin.p, eps=Cc.p, eps_u=U.p if guide else None, coef=COEF.p,
                                    step=STEP.p, n_steps=n, cfg_workspace=WS and WS.ptr,
                                    rule=_lib.X0_DPM, w=w, rescale=phi)
                Sg = _thresh(src, B, P, xin.t)
            XP = XA if alias else _out((B, P), dtype, "x_prev")
            DUP = _out((B, P), dtype, "x_prev_dup") if dup else None
            if alias:
                XA.freeze()
            _lib.call("vd_dpm_step_known", xin.p, Cc.p, U.p if guide else None, XP.p, _p(DUP),
                      H.p, COEF.p, n, STEP.p, w, phi, WS and WS.ptr, int(mode == "clip"), _p(Sg),
                      XK.p, KEEP.p, keep.shape[0], S, B, P, DT, _st())
            outs = [g for g in (None if alias else XP, DUP, H if first else None) if g]
            inouts = [g for g in (XA, None if first else H) if g]
            assert_clean(outs, [Cc, COEF, STEP, XK, KEEP] + ([U] if guide else [])
                         + ([WS] if WS else []) + ([Sg] if Sg else [])
                         + ([] if alias else [XT]), what=what, inouts=inouts)
            assert_finite([g for g in (XP, DUP, H) if g], what=what)
            ref = cases.masked("dpm", mode, xt, c, u, last, guide, xk, keep, row=s.coef[row])
            worst = max(worst, _check(XP.value(), ref, "x_prev", bf, what),
                        _check(H.value(), ref, "x0", bf, what))
            if DUP:
                assert torch.equal(DUP.value(), XP.value()), what
    print(f"guarded dpm known {dtype} {(B, C, S)} odd={odd!r}: largest error / bound {worst:.3g}")
    record_metric(test="guarded_dpm_known", shape=[B, C, S], odd=odd, dtype=str(dtype),
                  worst=worst)
