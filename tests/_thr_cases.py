"""Inputs, fp64 references and error bounds of dynamic thresholding (vd_x0_abs_quantile,
vd_ddim_step_thr, vd_dpm_step_thr), shared by tests/test_thr_host.py (CPU) and the GPU tests so
that the host test bounds the very inputs the GPU tests run.  Nothing here imports the sampler's
step code: the formulas are written again.

Semantics, per sample b over its P elements, x0 in fp32 as the step kernel forms it:

    q_b  = sort(|x0|)[k],  k = min(P - 1, ceil(p (P - 1)))      (rank)
    s_b  = min(max(q_b, 1), threshold_max)                       (threshold)
    y_i  = clamp(x0_i, -s_b, s_b) / s_b                          (the thresholded x0)
    x_prev = K y + (the step's other terms, unchanged)           K = sqrt(a_prev) (DDIM), B (2M)

Bounds.  Let delta_i be the bound the case files already derive for the UNCLAMPED fp32 x0
(_bounds.bound of their "x0" entry with an fp32 output: their n_terms and c_extra) and Delta =
max_i delta_i over the sample.

  s:  an order statistic moves by at most the sup-norm distance of the data (the k-th smallest
      of a_i + e_i lies within max|e_i| of the k-th smallest of a_i), | |x| - |x'| | <= |x - x'|,
      and max(., 1) and min(., threshold_max) are 1-Lipschitz: |s - s_ref| <= Delta.  Selecting
      is exact: no rounding is added.

  y:  with f(x, s) = clamp(x / s, -1, 1): |f(x, s) - f(x', s)| <= |x - x'| / s, and |f(x', s) -
      f(x', s')| <= |s - s'| / max(s, s') (inside both ranges |x'| <= min(s, s') and the
      difference is |x'| |s - s'| / (s s'); a clipped value lies between).  So
          |y - y_ref| <= (|x0 - x0_ref| + |s - s_ref|) / min(s, s_ref) <= delta_i + Delta
      because s >= 1.  The kernel's divide is one more fp32 rounding of a value in [-1, 1]: +
      u32; the output rounding is u_out |y_ref|.  _bounds.assert_elementwise takes this as mag
      = delta_i + Delta + u32 with n_terms = 0 and c_extra = 1 - 4 u32, which makes its factor 2
      (n_terms + 2) u32 + c_extra exactly 1.

  x_prev: the case files' own x_prev bound stands -- |y| <= |x0| <= mag_x0, so every rounding
      of K y and of the sums is covered by the same magnitudes, and the share K delta_i of x0's
      own error is inside it already -- plus what thresholding adds to x0's error, K (Delta +
      u32): c_extra grows by K (Delta + u32) / mag_x_prev.  The fp64 reference is the case
      file's unclamped x_prev + K (y_ref - x0_ref).

No tolerance here is tuned: every number above comes from the case files' derivations.
u32 = 2^-24.
"""
import math

import torch

import _cfg_cases as cfg
import _dpm_cases as dpm
import _objective_cases as obj
from _bounds import U_FP32, bound

P_THR = 0.995
W = 7.5
PHIS = (0.0, 0.7)
KINDS = ("ddim-eps", "ddim-v", "dpm")
GUIDES = [None] + [(W, phi) for phi in PHIS]
SHAPES = cfg.SHAPES
# the selection's own shapes: the scalar path (rank = max at 0.995); 8-wide in one block; three
# ranges that are no multiple of a block; the cap on partial blocks, where a block loops over
# its range, 8-wide and scalar
SELECT_SHAPES = [(2, 105), (3, 768), (2, 5000), (2, 2 * 262144 + 8), (2, 2 * 262144 + 13)]
SELECT_PS = (1e-9, 0.5, 0.995, 1.0)  # a tiny p is rank 1 (ceil); rank 0 is tested by rank


def rank(p, P):
    """0-based rank of the "higher" p-quantile of P values, p a Python float (double)."""
    return min(P - 1, math.ceil(p * (P - 1)))


def order_stat(a, k):
    """[B] the k-th smallest of every row of a [B, P]."""
    return a.sort(dim=1).values[:, k]


def threshold(x0, p, tmax=math.inf):
    """[B, 1] s_b of x0 [B, P] in x0's own precision."""
    q = order_stat(x0.abs(), rank(p, x0.shape[1]))
    return q.clamp_min(1.0).clamp_max(tmax).view(-1, 1)


def acp_table():
    return dpm.schedules()["v2"]


def dpm_sampler(**kw):
    """The 8-step 2M sampler whose rows the kernel tests read (as tests/test_gpu_dpm.py)."""
    from vdiff.schedulers import DPMSolverSampler
    kw.setdefault("steps", 8)
    return DPMSolverSampler(dpm.v2_scheduler(), **kw)


def _prev_acp(acp, tp):
    a = acp.double()
    return torch.where(tp >= 0, a[tp.clamp_min(0)], torch.ones(tp.shape, dtype=torch.float64))


def base64(kind, xt, c, u, other, guide, *, t=None, tp=None, acp=None, row=None, eta=0.0):
    """(the case files' UNCLAMPED references {"x0", "x_prev"}, K): kind "ddim-eps" / "ddim-v"
    with t, tp, acp (other = z), "dpm" with the kernel's fp32 row (other = the x0 history).
    guide: None (the step runs on c alone) or (w, phi)."""
    if kind == "dpm":
        g = None if guide is None else (u, guide[0], guide[1])
        return dpm.ref64(xt, c, other, row, False, guide=g), abs(float(row[3]))
    K = _prev_acp(acp, tp).sqrt().view(-1, 1)
    if kind == "ddim-v":
        w, phi = guide or (0.0, 0.0)
        return obj.ddim_ref64(xt, c, u, other, t, tp, acp, w, phi, eta, False,
                              guided=guide is not None), K
    if guide is None:  # w = 0 on equal halves: the guide is the identity, eps = c
        return cfg.ref64(xt, c, c, other, t, tp, acp, 0.0, 0.0, eta, False), K
    return cfg.ref64(xt, c, u, other, t, tp, acp, guide[0], guide[1], eta, False), K


def thresholded(base, K, p=P_THR, tmax=math.inf):
    """The thresholded step's references and bounds (module docstring): "s" -> (s_ref [B, 1],
    Delta [B, 1]); "x0", "x_prev" -> (ref, mag, n_terms, c_extra) for assert_elementwise; "q" ->
    the unclamped quantile [B]."""
    x0, mag0, n0, ce0 = base["x0"]
    xp, magp, np_, cep = base["x_prev"]
    delta = bound(x0, mag0, n0, False, ce0)
    Delta = delta.max(dim=1, keepdim=True).values
    s = threshold(x0, p, tmax)
    y = torch.minimum(torch.maximum(x0, -s), s) / s
    return {"q": order_stat(x0.abs(), rank(p, x0.shape[1])),
            "s": (s, Delta),
            "x0": (y, delta + Delta + U_FP32, 0, 1.0 - 4.0 * U_FP32),
            "x_prev": (xp + K * (y - x0), magp, np_,
                       cep + K * (Delta + U_FP32) / magp.clamp_min(1e-300))}


def clipped(base, K):
    """The static clamp's references from the same unclamped ones, with the thresholded
    bounds (the floor case: s = 1 exactly, where thresholding IS the clamp)."""
    x0, mag0, n0, ce0 = base["x0"]
    xp, magp, np_, cep = base["x_prev"]
    y = x0.clamp(-1, 1)
    return {"x0": (y, mag0, n0, ce0), "x_prev": (xp + K * (y - x0), magp, np_, cep)}


# ------------------------------------------------------------------ fp32 emulation (host test)
def emulate32(kind, xt, c, u, other, guide, p=P_THR, tmax=math.inf, *, t=None, tp=None,
              acp=None, row=None):
    """(s [B, 1], y, x_prev) of the thresholded step with every operation rounded to fp32 (torch
    CPU, no fused multiply-add; f_b rounded once from fp64, its own error is the case files'
    allowance), the exact order statistic of those fp32 x0, eta = 0."""
    xt, c, u, other = (v.float() for v in (xt, c, u, other))
    out = c
    if guide is not None:
        w, phi = guide
        f = cfg.factor64(c, u, w, phi).float()
        out = torch.tensor(w, dtype=torch.float32) * (c - u) + u
        if phi > 0:
            out = f * out
    if kind == "dpm":
        al, sg, A, B, C = (row[i].float() for i in range(5))
        x0 = (xt - sg * out) / al
    else:
        at = acp.float()[t].view(-1, 1)
        ap = _prev_acp(acp, tp).float().view(-1, 1)
        sa, s1m = at.sqrt(), (1 - at).sqrt()
        if kind == "ddim-v":
            x0 = sa * xt - s1m * out
            eps = s1m * xt + sa * out
        else:
            x0, eps = (xt - s1m * out) / sa, out
    s = threshold(x0, p, tmax)
    y = torch.minimum(torch.maximum(x0, -s), s) / s
    if kind == "dpm":
        xp = A * xt + B * y
        if float(C) != 0.0:
            xp = xp + C * other
    else:
        xp = ap.sqrt() * y + (1 - ap).clamp_min(0).sqrt() * eps
    return s, y, xp
