"""The sampler-step kernels (q_sample, the three p_sample forms, the DDIM step in both
parameterisations, the guidance statistics / combine / fused steps, DPM-Solver++) and the timestep
embedding on guarded, NaN-poisoned buffers (tests/_guarded.py), through vdiff._lib.call with the
operands and call order of vdiff.ops.

Every tensor, every schedule table, every timestep vector and the DPM step word live between two
1 MiB guards of a NaN pattern; every output starts out as the pattern; the statistics workspace is
exactly vd_cfg_workspace_size bytes of 0xFF, a fresh one per use.  t holds both ends of the table
(0 and T - 1) and t_prev = -1, so an index one off either end reads a NaN.  After each call the
outputs are fully written, all guards and gaps bit-intact and the inputs bit-identical.  Values
are judged by what the unguarded tests use, imported unchanged: _cfg_cases.ref64,
_objective_cases.ddim_ref64 and _dpm_cases.ref64 through _bounds.assert_elementwise, and the
oracle at the tolerances of tests/test_gpu_elementwise.py for q_sample / p_sample_*.

Alignment (include/vdiff.h, "Alignment of the per-sample kernels"): every entry point here takes
the 8-wide path only when per_sample % 8 == 0 and every non-null tensor pointer is 16-byte
aligned, and otherwise runs one element at a time.  `off = 1` offsets one operand's pointer by one
element at the 8-wide shape: the same values, no store past the tensor.

Largest error / bound measured on an MI355X, bf16 | fp32: DDIM 0.994 | 0.26, guidance 0.996 | 0.13,
DPM-Solver++ 0.995 | 0.19 -- the figures of the unguarded tests of the same cases (a bf16 figure is
the output's own rounding).

What the three shapes do not reach in the step kernel has tests of its own: a sample one
element-block longer than a full grid of 4096 blocks covers (the grid-stride loop), and 65537
samples, two more than a grid has rows (the second layer of rows); measured: grid stride 0.996 |
0.22, sample stride 0.996 | 0.42.
"""
import math

import pytest
import torch

from conftest import golden, record_metric

from oracle import schedulers as osch
from oracle.fixtures import seeded

import _cfg_cases as cfg
import _dpm_cases as dpm
import _objective_cases as obj
import _thr_cases as thr
from _bounds import assert_elementwise
from _guarded import Guarded, assert_clean, assert_finite

pytestmark = pytest.mark.gpu
dev = "cuda"
DTYPES = [torch.bfloat16, torch.float32]
f32, i64 = torch.float32, torch.int64
# (B, P, element offset of one operand): the three shapes, and the 8-wide one unaligned
CASES = [(B, P, 0) for B, P in cfg.SHAPES] + [(cfg.SHAPES[0][0], cfg.SHAPES[0][1], 1)]
assert cfg.SHAPES[0][1] % 8 == 0


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


# ------------------------------------------------------------------ q_sample / p_sample_*
def _ends(B, T):
    return torch.tensor({2: [0, T - 1], 3: [0, T // 2, T - 1]}[B])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,P,off", CASES)
def test_guarded_q_and_p_sample(B, P, off, dtype):
    """vd_q_sample, vd_p_sample_v1, _v2 and _cosine against the oracle formulas evaluated in fp64
    on the same dtype-rounded inputs and fp32 tables, at the tolerances of test_q_sample and
    test_p_sample_golden (cosine at its last timestep: that test's 1e-4 in fp32).  off = 1: the
    first output's pointer is one element past a 16-byte boundary."""
    from vdiff import _lib
    bf = dtype == torch.bfloat16
    rnd = (lambda v: v.bfloat16().float()) if bf else (lambda v: v)
    xt, ep, z = (rnd(seeded((B, P), s)) for s in (11, 12, 13))
    DT = _dt(dtype)
    XT, EP, Z = _in(xt, dtype, "xt"), _in(ep, dtype, "eps"), _in(z, dtype, "z")
    tabs = {"v1": osch.linear_tables(100, 0.00085, 0.012),
            "v2": osch.linear_tables(500, 0.00005, 0.015), "cos": osch.cosine_tables(2000)}
    G = {k: {n: _tab(v.float(), f"{k}.{n}") for n, v in tab.items()} for k, tab in tabs.items()}
    tq = 1e-6 if not bf else 2e-2
    tp_ = 2e-6 if not bf else 3e-2

    def close(got, ref, tol, what):
        torch.testing.assert_close(got.double(), ref, atol=tol, rtol=tol,
                                   msg=lambda m: f"{what}: {m}")

    # q_sample (x0 := xt)
    tab, g = tabs["v1"], G["v1"]
    t = _ends(B, 100)
    Tq = _tab(t, "t")
    O = _out((B, P), dtype, "xt_out", off)
    _lib.call("vd_q_sample", XT.p, EP.p, O.p, Tq.p, g["sqrt_acp"].p, g["sqrt_1m_acp"].p, B, P, DT,
              _st())
    assert_clean([O], [XT, EP, Tq, g["sqrt_acp"], g["sqrt_1m_acp"]], what=f"q_sample {dtype}")
    close(O.value(), osch.q_sample(tab, xt.double(), ep.double(), t), tq, "q_sample")

    for kind, T in (("v1", 100), ("v2", 500), ("cos", 2000)):
        tab, g = tabs[kind], G[kind]
        t = _ends(B, T)
        Tk = _tab(t, "t")
        XP, X0 = _out((B, P), dtype, "x_prev", off), _out((B, P), dtype, "x0")
        if kind == "v1":
            _lib.call("vd_p_sample_v1", XT.p, EP.p, Z.p, XP.p, X0.p, Tk.p, g["betas"].p,
                      g["alphas"].p, g["acp"].p, g["sqrt_1m_acp"].p, B, P, DT, _st())
            ref = osch.p_sample_v1(tab, xt.double(), ep.double(), t, z.double())
            used = ("betas", "alphas", "acp", "sqrt_1m_acp")
        elif kind == "v2":
            _lib.call("vd_p_sample_v2", XT.p, EP.p, Z.p, XP.p, X0.p, Tk.p, g["betas"].p,
                      g["alphas"].p, g["acp"].p, g["sqrt_acp"].p, g["sqrt_1m_acp"].p, B, P, DT,
                      _st())
            ref = osch.p_sample_v2(tab, xt.double(), ep.double(), t, z.double())
            used = ("betas", "alphas", "acp", "sqrt_acp", "sqrt_1m_acp")
        else:
            _lib.call("vd_p_sample_cosine", XT.p, EP.p, Z.p, XP.p, X0.p, Tk.p, g["acp"].p,
                      g["sqrt_acp"].p, g["sqrt_1m_acp"].p, B, P, DT, _st())
            ref = osch.p_sample_cosine(tab, xt.double(), ep.double(), t, z.double())
            used = ("acp", "sqrt_acp", "sqrt_1m_acp")
        assert_clean([XP, X0], [XT, EP, Z, Tk] + [g[n] for n in used],
                     what=f"p_sample_{kind} {dtype} off={off}")
        for b in range(B):
            tol = tp_ if not (kind == "cos" and int(t[b]) == T - 1) else max(tp_, 1e-4)
            close(XP.value()[b], ref[0][b].double(), tol, f"p_sample_{kind} x_prev t={int(t[b])}")
            close(X0.value()[b], ref[1][b].double(), tol, f"p_sample_{kind} x0 t={int(t[b])}")


# ------------------------------------------------------------------ DDIM step, both predictions
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,P,off", CASES)
def test_guarded_ddim_step(B, P, off, dtype):
    """vd_ddim_step and vd_ddim_step_pred (eps and v): z NULL at eta = 0 and given at 0.5, x0
    given and NULL, clip on and off; _cfg_cases.ref64 with c = u (the unguided step, as
    test_fused_step_exactness judges ddim_step) and _objective_cases.ddim_ref64 for v."""
    from vdiff import _lib
    bf = dtype == torch.bfloat16
    xt, c, _, z = cfg.inputs(B, P, bf)
    t, tp = cfg.timesteps(B)
    assert 0 in t.tolist() and 499 in t.tolist() and -1 in tp.tolist()
    acp = dpm.schedules()["v2"]
    assert acp.numel() == 500
    DT = _dt(dtype)
    XT, E, Z = _in(xt, dtype, "xt"), _in(c, dtype, "eps"), _in(z, dtype, "z", off)
    Tt, Tp, ACP = _tab(t, "t"), _tab(tp, "t_prev"), _tab(acp, "acp")
    worst = 0.0
    for fn, pred in (("vd_ddim_step", "eps"), ("vd_ddim_step_pred", "eps"),
                     ("vd_ddim_step_pred", "v")):
        for eta, clip, want_x0 in ((0.0, 0, True), (0.5, 1, True), (0.5, 0, False)):
            what = f"{fn} {pred} {dtype} B={B} P={P} off={off} eta={eta} clip={clip} x0={want_x0}"
            XP = _out((B, P), dtype, "x_prev", off if not eta else 0)
            X0 = _out((B, P), dtype, "x0") if want_x0 else None
            zz = Z if eta else None
            args = [XT.p, E.p, _p(zz), XP.p, _p(X0), Tt.p, Tp.p, ACP.p, eta, clip]
            if fn == "vd_ddim_step_pred":
                args.append(_lib.PREDICTIONS[pred])
            _lib.call(fn, *args, B, P, DT, _st())
            assert_clean([g for g in (XP, X0) if g], [XT, E, Z, Tt, Tp, ACP], what=what)
            if pred == "v":
                ref = obj.ddim_ref64(xt, c, c, z, t, tp, acp, 0.0, 0.0, eta, bool(clip), False)
            else:
                ref = cfg.ref64(xt, c, c, z, t, tp, acp, 0.0, 0.0, eta, bool(clip))
            worst = max(worst, _check(XP.value(), ref, "x_prev", bf, what))
            if X0:
                worst = max(worst, _check(X0.value(), ref, "x0", bf, what))
    print(f"guarded ddim {dtype} B={B} P={P} off={off}: largest error / bound {worst:.3g}")
    record_metric(test="guarded_ddim", B=B, P=P, off=off, dtype=str(dtype), worst=worst)


# ------------------------------------------------------------------ guidance
def _stats(C, U, w, B, P, DT, what):
    """vd_cfg_stats into a fresh workspace of exactly the advertised size, every slot written."""
    from vdiff import _lib
    nws = _lib.lib().vd_cfg_workspace_size(B, P)
    assert nws == B * cfg.partials(P)[0] * 16
    WS = Guarded.workspace(nws, dev, name="cfg workspace")
    _lib.call("vd_cfg_stats", C.p, U.p, w, B, P, DT, WS.ptr, nws, _st())
    assert_clean([], [C, U], [WS], what=what + " stats")
    slots = WS.t.view(torch.int32)
    assert not bool((slots == -1).any()), f"{what}: workspace slot left as 0xFF"
    assert bool(torch.isfinite(WS.t.view(f32)).all()), f"{what}: non-finite statistic"
    return WS.freeze()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,P,off", CASES)
def test_guarded_cfg(B, P, off, dtype):
    """vd_cfg_stats, vd_cfg_combine, vd_ddim_step_cfg and vd_ddim_step_cfg_pred: rescale = 0 with
    a NULL workspace and rescale = 0.7 with the workspace vd_cfg_stats just filled; x_prev_dup
    given and NULL, x0 given and NULL, z NULL at eta = 0, x_prev written over xt, v-prediction.
    Judged as test_kernels_against_fp64 / the guided v test do."""
    from vdiff import _lib
    bf = dtype == torch.bfloat16
    xt, c, u, z = cfg.inputs(B, P, bf)
    t, tp = cfg.timesteps(B)
    acp = dpm.schedules()["v2"]
    DT = _dt(dtype)
    C, U, Z = _in(c, dtype, "eps_c"), _in(u, dtype, "eps_u", off), _in(z, dtype, "z")
    XT = _in(xt, dtype, "xt")
    Tt, Tp, ACP = _tab(t, "t"), _tab(tp, "t_prev"), _tab(acp, "acp")
    fixed = [C, U, Z, Tt, Tp, ACP]
    w = 2.5
    worst = 0.0
    for phi in (0.0, 0.7):
        what = f"cfg {dtype} B={B} P={P} off={off} phi={phi}"
        WS = _stats(C, U, w, B, P, DT, what) if phi else None
        ws_in = [WS] if WS else []
        EO = _out((B, P), dtype, "eps_out")
        _lib.call("vd_cfg_combine", C.p, U.p, EO.p, w, phi, WS and WS.ptr, B, P, DT, _st())
        assert_clean([EO], [C, U] + ws_in, what=what + " combine")
        ref = cfg.ref64(xt, c, u, z, t, tp, acp, w, phi, 0.0, False)
        worst = max(worst, _check(EO.value(), ref, "eps", bf, what + " combine"))
        # (entry point, prediction, eta, clip, dup, x0, alias)
        for fn, pred, eta, clip, dup, want_x0, alias in (
                ("vd_ddim_step_cfg", "eps", 0.0, 0, True, True, False),
                ("vd_ddim_step_cfg", "eps", 0.5, 1, False, False, False),
                ("vd_ddim_step_cfg", "eps", 0.5, 0, True, True, True),
                ("vd_ddim_step_cfg_pred", "eps", 0.0, 1, False, True, False),
                ("vd_ddim_step_cfg_pred", "v", 0.5, 0, True, True, False),
                ("vd_ddim_step_cfg_pred", "v", 0.0, 1, False, False, True)):
            wh = f"{what} {fn} {pred} eta={eta} clip={clip} dup={dup} x0={want_x0} alias={alias}"
            XA = _in(xt, dtype, "xt (x_prev in place)") if alias else None
            XP = XA if alias else _out((B, P), dtype, "x_prev")
            DUP = _out((B, P), dtype, "x_prev_dup") if dup else None
            X0 = _out((B, P), dtype, "x0") if want_x0 else None
            zz = Z if eta else None
            args = [(XA or XT).p, C.p, U.p, _p(zz), XP.p, _p(DUP), _p(X0), Tt.p, Tp.p, ACP.p, w,
                    phi, WS and WS.ptr, eta, clip]
            if fn.endswith("_pred"):
                args.append(_lib.PREDICTIONS[pred])
            _lib.call(fn, *args, B, P, DT, _st())
            assert_clean([g for g in (None if alias else XP, DUP, X0) if g],
                         fixed + ws_in + ([] if alias else [XT]), what=wh,
                         inouts=[XA] if alias else [])
            assert_finite([XP], what=wh)
            if pred == "v":
                ref = obj.ddim_ref64(xt, c, u, z, t, tp, acp, w, phi, eta, bool(clip), True)
            else:
                ref = cfg.ref64(xt, c, u, z, t, tp, acp, w, phi, eta, bool(clip))
            worst = max(worst, _check(XP.value(), ref, "x_prev", bf, wh))
            if DUP:
                assert torch.equal(DUP.value(), XP.value()), wh
            if X0:
                worst = max(worst, _check(X0.value(), ref, "x0", bf, wh))
    print(f"guarded cfg {dtype} B={B} P={P} off={off}: largest error / bound {worst:.3g}")
    record_metric(test="guarded_cfg", B=B, P=P, off=off, dtype=str(dtype), worst=worst)


# ------------------------------------------------------------------ DPM-Solver++(2M)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,P,off", CASES)
def test_guarded_dpm(B, P, off, dtype):
    """vd_dpm_step and vd_dpm_step_cfg on the rows of _dpm_cases.kernel_rows.  The device step
    word is guarded and takes a value below 0 (row 0), an exact one and one above n_steps - 1 (the
    last row); the coefficient table is guarded, so a row index one off either end reads NaN.
    Row 0 (first order, C = 0): x0_hist is left as the pattern, which must not reach x_prev and
    must be fully overwritten.  Otherwise x0_hist is read and written in place.  x_prev_dup given
    and NULL, x_prev written over xt, rescale 0 with a NULL workspace and 0.7 with a fresh one."""
    from vdiff import _lib
    from vdiff.schedulers import DPMSolverSampler
    bf = dtype == torch.bfloat16
    s = DPMSolverSampler(dpm.v2_scheduler(), steps=8)
    rows = dpm.kernel_rows(s)
    n = s.steps
    assert s.coef[rows[0], 4] == 0 and s.coef[rows[1], 4] != 0
    xt, c, u, last = dpm.inputs(B, P, bf)
    DT = _dt(dtype)
    XT, C, U = _in(xt, dtype, "xt"), _in(c, dtype, "eps_c", off), _in(u, dtype, "eps_u")
    COEF = _tab(s.coef, "coef")
    w = 2.5
    worst = 0.0
    for row, word in ((rows[0], -5), (rows[1], rows[1]), (rows[2], n + 3)):
        STEP = _tab(torch.tensor([word]), "step")
        first = row == rows[0]
        for guided, phi, dup, alias, clip in ((False, 0.0, False, False, 0),
                                              (False, 0.0, False, True, 1),
                                              (True, 0.0, True, False, 1),
                                              (True, 0.7, False, True, 0),
                                              (True, 0.7, True, False, 0)):
            wh = (f"dpm {dtype} B={B} P={P} off={off} row={row} step={word} guided={guided} "
                  f"phi={phi} dup={dup} alias={alias} clip={clip}")
            WS = _stats(C, U, w, B, P, DT, wh) if phi else None
            H = _out((B, P), dtype, "x0_hist") if first else _in(last, dtype, "x0_hist")
            XA = _in(xt, dtype, "xt (x_prev in place)") if alias else None
            XP = XA if alias else _out((B, P), dtype, "x_prev")
            DUP = _out((B, P), dtype, "x_prev_dup") if dup else None
            if guided:
                _lib.call("vd_dpm_step_cfg", (XA or XT).p, C.p, U.p, XP.p, _p(DUP), H.p, COEF.p, n,
                          STEP.p, w, phi, WS and WS.ptr, clip, B, P, DT, _st())
            else:
                _lib.call("vd_dpm_step", (XA or XT).p, C.p, XP.p, H.p, COEF.p, n, STEP.p, clip, B,
                          P, DT, _st())
            outs = [g for g in (None if alias else XP, DUP, H if first else None) if g]
            inouts = [g for g in (XA, None if first else H) if g]
            ins = [C, COEF, STEP] + ([U] if guided else []) + ([WS] if WS else []) \
                + ([] if alias else [XT])
            assert_clean(outs, ins, what=wh, inouts=inouts)
            assert_finite([XP, H], what=wh)
            ref = dpm.ref64(xt, c, last, s.coef[row], bool(clip),
                            guide=(u, w, phi) if guided else None)
            worst = max(worst, _check(XP.value(), ref, "x_prev", bf, wh),
                        _check(H.value(), ref, "x0", bf, wh))
            if DUP:
                assert torch.equal(DUP.value(), XP.value()), wh
    print(f"guarded dpm {dtype} B={B} P={P} off={off}: largest error / bound {worst:.3g}")
    record_metric(test="guarded_dpm", B=B, P=P, off=off, dtype=str(dtype), worst=worst)


# ------------------------------------------------------------------ the step kernel's two loops
# one element-block past the cap of 4096 blocks x 256 lanes on the elements of a sample: odd, so
# the scalar path, whose blocks take a second trip
P_STRIDE = 4096 * 256 + 257
# one sample past the 65535 rows of a grid: the plain entry points stride the samples over the
# rows, the guided and thresholded ones refuse
B_ROWS = 65537


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rule", ["ddim-eps", "dpm"])
def test_guarded_step_grid_stride(rule, dtype):
    """The grid-stride loop within a sample: B = 2, P = P_STRIDE, on the plain, the guided (7.5,
    0.7) and the thresholded guided step of DDIM-eps and of DPM-Solver++ on its middle row.
    Outputs fully written, guards intact, inputs unchanged, values inside the fp64 bounds of
    _cfg_cases / _dpm_cases (the thresholded ones through _thr_cases, whose quantile lies above
    the floor 1 in both samples, so the threshold is no clamp to [-1, 1])."""
    from vdiff import _lib
    bf = dtype == torch.bfloat16
    B, P = 2, P_STRIDE
    assert P % 8 and P > 4096 * 256
    DT = _dt(dtype)
    w, phi = thr.W, 0.7
    xt, c, u, other = cfg.inputs(B, P, bf)   # other: z, or the x0 history
    XT, C, U, O = (_in(xt, dtype, "xt"), _in(c, dtype, "eps_c"), _in(u, dtype, "eps_u"),
                   _in(other, dtype, "z / x0_last"))
    if rule == "dpm":
        s = thr.dpm_sampler()
        row, n = dpm.kernel_rows(s)[1], s.steps
        assert s.coef[row, 4] != 0
        COEF, STEP = _tab(s.coef, "coef"), _tab(torch.tensor([row]), "step")
        tabs, kw = [COEF, STEP], dict(row=s.coef[row])
        src_kw = dict(coef=COEF.p, step=STEP.p, n_steps=n, rule=_lib.X0_DPM)
    else:
        t, tp = cfg.timesteps(B)
        acp = dpm.schedules()["v2"]
        Tt, Tp, ACP = _tab(t, "t"), _tab(tp, "t_prev"), _tab(acp, "acp")
        tabs, kw = [Tt, Tp, ACP], dict(t=t, tp=tp, acp=acp, eta=0.5)
        src_kw = dict(t=Tt.p, acp=ACP.p, rule=_lib.X0_DDIM, prediction=0)
    WS = _stats(C, U, w, B, P, DT, f"{rule} {dtype} grid stride")
    worst = 0.0
    for path in ("plain", "guided", "thresholded"):
        what = f"grid stride {rule} {path} {dtype}"
        guide = None if path == "plain" else (w, phi)
        base, K = thr.base64(rule, xt, c, u, other, guide, **kw)
        ins = [XT, C] + tabs + ([] if path == "plain" else [U, WS])
        XP = _out((B, P), dtype, "x_prev")
        DUP = None if path == "plain" else _out((B, P), dtype, "x_prev_dup")
        # DPM: the history, read and written in place
        X0 = _in(other, dtype, "x0_hist") if rule == "dpm" else _out((B, P), dtype, "x0")
        if path == "thresholded":
            ref = thr.thresholded(base, K)
            assert bool((ref["q"] > 1).all()), ref["q"]
            nws = _lib.lib().vd_x0_quantile_workspace_size(B, P)
            QWS = Guarded.workspace(nws, dev, name="select workspace")
            S = _out((B,), f32, "s")
            src = _lib.X0Source(x=XT.p, eps=C.p, eps_u=U.p, cfg_workspace=WS.ptr, w=w, rescale=phi,
                                **src_kw)
            _lib.call("vd_x0_abs_quantile", src, thr.rank(thr.P_THR, P), 1.0, math.inf, B, P, DT,
                      S.p, QWS.ptr, nws, _st())
            assert_clean([S], ins, [QWS], what=what + " select")
            s_ref, Delta = ref["s"]
            assert ((S.value().double().view(-1, 1) - s_ref).abs() <= Delta).all(), what
            ins.append(S.freeze())
            if rule == "dpm":
                _lib.call("vd_dpm_step_thr", XT.p, C.p, U.p, XP.p, DUP.p, X0.p, COEF.p, n, STEP.p,
                          w, phi, WS.ptr, S.p, B, P, DT, _st())
            else:
                _lib.call("vd_ddim_step_thr", XT.p, C.p, U.p, O.p, XP.p, DUP.p, X0.p, Tt.p, Tp.p,
                          ACP.p, w, phi, WS.ptr, 0.5, 0, S.p, B, P, DT, _st())
        else:
            ref = base
            guided = [] if path == "plain" else [w, phi, WS.ptr]
            mid = [] if path == "plain" else [U.p]
            dupl = [] if path == "plain" else [DUP.p]
            if rule == "dpm":
                _lib.call("vd_dpm_step" if path == "plain" else "vd_dpm_step_cfg", XT.p, C.p, *mid,
                          XP.p, *dupl, X0.p, COEF.p, n, STEP.p, *guided, 0, B, P, DT, _st())
            else:
                _lib.call("vd_ddim_step" if path == "plain" else "vd_ddim_step_cfg", XT.p, C.p,
                          *mid, O.p, XP.p, *dupl, X0.p, Tt.p, Tp.p, ACP.p, *guided, 0.5, 0, B, P,
                          DT, _st())
        if rule == "dpm":
            assert_clean([g for g in (XP, DUP) if g], ins, what=what, inouts=[X0])
        else:
            assert_clean([g for g in (XP, DUP, X0) if g], ins + [O], what=what)
        assert_finite([XP, X0], what=what)
        worst = max(worst, _check(XP.value(), ref, "x_prev", bf, what),
                    _check(X0.value(), ref, "x0", bf, what))
        if DUP:
            assert torch.equal(DUP.value(), XP.value()), what
    print(f"guarded grid stride {rule} {dtype}: largest error / bound {worst:.3g}")
    record_metric(test="guarded_step_grid_stride", rule=rule, dtype=str(dtype), worst=worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [1, 8])
def test_guarded_step_sample_stride(P, dtype):
    """More samples than a grid has rows, B = B_ROWS, one element and one 8-vector each:
    vd_ddim_step, vd_ddim_step_pred on v and vd_dpm_step (the middle row) stride the samples.  t
    cycles over the whole table, 0 and T - 1 included, with t_prev = -1 below t = 10.  Outputs
    fully written, guards intact, inputs unchanged, values inside the fp64 bounds.  The guided
    and the thresholded entry points refuse this B with VD_EINVAL and launch nothing: their
    outputs keep the pattern."""
    from vdiff import _lib
    bf = dtype == torch.bfloat16
    B = B_ROWS
    DT = _dt(dtype)
    xt, c, u, other = cfg.inputs(B, P, bf)
    acp = dpm.schedules()["v2"]
    T = acp.numel()
    t = torch.arange(B) % T
    tp = torch.where(t >= 10, t - 10, torch.full_like(t, -1))
    assert 0 in t.tolist() and T - 1 in t.tolist() and -1 in tp.tolist()
    s = thr.dpm_sampler()
    row, n = dpm.kernel_rows(s)[1], s.steps
    XT, C, O = _in(xt, dtype, "xt"), _in(c, dtype, "eps"), _in(other, dtype, "z / x0_last")
    Tt, Tp, ACP = _tab(t, "t"), _tab(tp, "t_prev"), _tab(acp, "acp")
    COEF, STEP = _tab(s.coef, "coef"), _tab(torch.tensor([row]), "step")
    worst = 0.0
    for fn, pred in (("vd_ddim_step", "eps"), ("vd_ddim_step_pred", "v")):
        what = f"sample stride {fn} {pred} {dtype} P={P}"
        XP, X0 = _out((B, P), dtype, "x_prev"), _out((B, P), dtype, "x0")
        args = [XT.p, C.p, O.p, XP.p, X0.p, Tt.p, Tp.p, ACP.p, 0.5, 1]
        if fn == "vd_ddim_step_pred":
            args.append(_lib.PREDICTIONS[pred])
        _lib.call(fn, *args, B, P, DT, _st())
        assert_clean([XP, X0], [XT, C, O, Tt, Tp, ACP], what=what)
        if pred == "v":
            ref = obj.ddim_ref64(xt, c, c, other, t, tp, acp, 0.0, 0.0, 0.5, True, False)
        else:
            ref = cfg.ref64(xt, c, c, other, t, tp, acp, 0.0, 0.0, 0.5, True)
        worst = max(worst, _check(XP.value(), ref, "x_prev", bf, what),
                    _check(X0.value(), ref, "x0", bf, what))
    what = f"sample stride vd_dpm_step {dtype} P={P}"
    XP, H = _out((B, P), dtype, "x_prev"), _in(other, dtype, "x0_hist")
    _lib.call("vd_dpm_step", XT.p, C.p, XP.p, H.p, COEF.p, n, STEP.p, 0, B, P, DT, _st())
    assert_clean([XP], [XT, C, COEF, STEP], what=what, inouts=[H])
    ref = dpm.ref64(xt, c, other, s.coef[row], False)
    worst = max(worst, _check(XP.value(), ref, "x_prev", bf, what),
                _check(H.value(), ref, "x0", bf, what))
    # B > 65535 on a per-sample-only entry point: VD_EINVAL (1) before anything is launched
    U = _in(u, dtype, "eps_u")
    S = _in(torch.ones(B), f32, "s")
    XP, DUP, X0 = (_out((B, P), dtype, n_) for n_ in ("x_prev", "x_prev_dup", "x0"))
    H = _in(other, dtype, "x0_hist")
    lib = _lib.lib()
    w = thr.W
    for rc in (lib.vd_ddim_step_cfg(XT.p, C.p, U.p, O.p, XP.p, DUP.p, X0.p, Tt.p, Tp.p, ACP.p, w,
                                    0.0, None, 0.5, 1, B, P, DT, _st()),
               lib.vd_dpm_step_cfg(XT.p, C.p, U.p, XP.p, DUP.p, H.p, COEF.p, n, STEP.p, w, 0.0,
                                   None, 0, B, P, DT, _st()),
               lib.vd_ddim_step_thr(XT.p, C.p, U.p, O.p, XP.p, DUP.p, X0.p, Tt.p, Tp.p, ACP.p, w,
                                    0.0, None, 0.5, 0, S.p, B, P, DT, _st()),
               lib.vd_dpm_step_thr(XT.p, C.p, U.p, XP.p, DUP.p, H.p, COEF.p, n, STEP.p, w, 0.0,
                                   None, S.p, B, P, DT, _st())):
        assert rc == 1 and b"bad shape" in lib.vd_last_error()
    assert_clean([], [XT, C, U, O, Tt, Tp, ACP, COEF, STEP, S, H], what="refused B")
    for g in (XP, DUP, X0):
        assert bool(g.unwritten().all()) and g.guards_intact(), g.name
    print(f"guarded sample stride {dtype} P={P}: largest error / bound {worst:.3g}")
    record_metric(test="guarded_step_sample_stride", P=P, dtype=str(dtype), worst=worst)


# ------------------------------------------------------------------ timestep embedding
TEMB_T = [0, 1, 499, 999, 1999]
TEMB_DIMS = [1, 2, 64, 65, 128]
MAX_PERIOD = 10000.0


def test_guarded_timestep_embedding_tab():
    """vd_timestep_embedding_tab with ops._temb_freqs' table (the reference's host computation),
    the table and the output guarded.  dim 64 / 65 / 128 on the golden timesteps are judged as
    test_timestep_embedding_golden judges them; every (dim, t) of this file, those included,
    against cos / sin in fp64 of the fp32 argument t * f the kernel forms, at the same 3e-5; the
    zero column of an odd dim is exactly zero."""
    from vdiff import _lib, ops
    g = golden("schedulers.npz")
    for dim in TEMB_DIMS:
        half = dim // 2
        fr = ops._temb_freqs(dim, MAX_PERIOD, "cpu").float() if half else None
        FR = _tab(fr, "freqs") if half else None
        for name, t in (("edge", torch.tensor(TEMB_T)), ("golden", g["temb_t"].long())):
            Bt = t.numel()
            T = _tab(t, "t")
            O = _out((Bt, dim), f32, "out")
            _lib.call("vd_timestep_embedding_tab", T.p, Bt, dim, _p(FR), O.p, _st())
            assert_clean([O], [T] + ([FR] if FR else []), what=f"temb_tab dim={dim} {name}")
            out = O.value()
            if dim % 2:
                assert not bool(out[:, 2 * half:].any())
            if half:
                arg = (t.float()[:, None] * fr[None]).double()
                ref = torch.cat([arg.cos(), arg.sin()], 1)
                torch.testing.assert_close(out[:, :2 * half].double(), ref, atol=3e-5, rtol=0)
            if name == "golden" and f"temb_{dim}" in g:
                ref = g[f"temb_{dim}"]
                torch.testing.assert_close(out, ref, atol=3e-5, rtol=0)
                assert ((out - ref).abs() > 1e-6).float().mean() < 0.03


# sinf / cosf: the device library (OCML) documents the accuracy the OpenCL C specification
# requires of the full profile, at most 4 ulp for sin and cos; the result lies in [-1, 1], where an
# ulp is at most 2^-23
SINCOS_ULP = 4


def test_guarded_timestep_embedding_computed_frequencies():
    """vd_timestep_embedding: the branch that computes f_i = expf(-ln(max_period) * i / half)
    itself, which vdiff.ops never reaches for dim >= 2.  Element by element against the formula
    in fp64: out[b, i] = cos(t_b f_i) | sin(t_b f_i), f_i = exp(-a_i), a_i = ln(max_period) i /
    half; an odd dim's last column is exactly zero.

    Bound, from the kernel's own roundings (u = 2^-24, the relative error of one fp32 rounding):
      the argument of expf, -L * (float)i / (float)half, rounds twice (the product, the divide):
        it is a_i (1 + d), |d| <= 2 u, an absolute error 2 a_i u of the argument, which exp turns
        into a relative error 2 a_i u of f_i;
      the value expf returns is rounded once more, and the rounding of L = logf(max_period)
        itself is one relative u of a_i <= 9.3: together within 2 u for the a_i where it matters
        (for small a_i the term is dominated by expf's rounding, for large a_i by t f_i -> 0);
      so |f~_i - f_i| <= f_i (2 a_i + 2) u, and (float)t being exact (t < 2^24) the argument of
        cos / sin is off by at most t f_i (2 a_i + 2) u, plus the one rounding of the product t
        f~_i: t f_i u;
      cos and sin are 1-Lipschitz, so that is also the error of the exact cos / sin, to which
        cosf / sinf add their documented SINCOS_ULP ulp of a result in [-1, 1].
    bound = t f_i (2 a_i + 3) 2^-24 + SINCOS_ULP 2^-23: 3.6e-4 at t = 1999, i = 0; 4.8e-7 at t =
    0.  Largest error / bound measured on an MI355X: 0.36 (dim 128; 0.33 at dim 64 and 65, 0.045 at
    dim 2), largest error 6.4e-5; recorded as guarded_temb_computed and asserted <= 1."""
    from vdiff import _lib
    u = 2.0 ** -24
    t = torch.tensor(TEMB_T)
    Bt = t.numel()
    worst = 0.0
    for dim in TEMB_DIMS:
        half = dim // 2
        T = _tab(t, "t")
        O = _out((Bt, dim), f32, "out")
        _lib.call("vd_timestep_embedding", T.p, Bt, dim, MAX_PERIOD, O.p, _st())
        assert_clean([O], [T], what=f"temb dim={dim}")
        out = O.value().double()
        if dim % 2:
            assert not bool(out[:, 2 * half:].any())
        if not half:
            continue
        a = math.log(MAX_PERIOD) * torch.arange(half, dtype=torch.float64) / half
        f = torch.exp(-a)
        arg = t.double()[:, None] * f[None]
        ref = torch.cat([arg.cos(), arg.sin()], 1)
        b1 = arg * (2 * a + 3)[None] * u + SINCOS_ULP * 2.0 ** -23
        bnd = torch.cat([b1, b1], 1)
        ratio = ((out[:, :2 * half] - ref).abs() / bnd)
        assert not bool(torch.isnan(ratio).any())
        worst = max(worst, float(ratio.max()))
        print(f"temb computed dim={dim}: largest error / bound {float(ratio.max()):.3g}, "
              f"largest error {float((out[:, :2 * half] - ref).abs().max()):.3g}")
        bad = ratio > 1
        assert not bool(bad.any()), (dim, [int(i) for i in bad.nonzero()[0]], float(ratio.max()))
    record_metric(test="guarded_temb_computed", worst=worst)
    assert 0 < worst <= 1
