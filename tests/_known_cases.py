"""Inputs, fp64 references and error bounds of masked sampling (vd_ddim_step_known,
vd_dpm_step_known, the `known` / `keep` keywords of the step ops and of the samplers), shared by
tests/test_known_host.py (CPU) and the GPU tests so that the host test checks the very cases the
GPU tests run.  Nothing here imports the sampler's step code: the formulas are written again.

Semantics, per element, with y the x0 the unmasked step forms (rule -> static clamp or dynamic
threshold), e its direction term, x_k the known value and k the mask (k <= 0 read as 0, k >= 1 as
1):

    k == 0:  x0' = y,                  e' = e
    k == 1:  x0' = x_k,                e' = e_k
    else:    x0' = (1 - k) y + k x_k,  e' = (1 - k) e + k e_k
    e_k    = (xt - sa x_k) / s1m,      sa = sqrt(a_t), s1m = sqrt(1 - a_t)        (DDIM)
    x_prev = sqrt(a_p) x0' + dir e'                          (DDIM, eta = 0: dir = sqrt(1 - a_p))
    x_prev = A xt + B x0' + C x0_last                        (2M)

Bounds.  u32 = 2^-24.  bnd(ref, mag, n, ce) = (2 (n + 2) u32 + ce) mag is _bounds.bound for an
fp32 value; the output's own rounding (2^-8 |ref| for bf16) is added by assert_elementwise.  From
the case files (_cfg_cases, _objective_cases, _dpm_cases, through _thr_cases.base64 / clipped /
thresholded) come, unchanged, d_y = the bound of the unmasked x0 under the step's mode and d_xp =
that of the unmasked x_prev.  Every reference below is handed to assert_elementwise as (ref, D, 0,
1 - 4 u32), which makes its factor exactly 1: D is the absolute bound.

  k == 0: the unmasked references and d_y, d_xp themselves (the same expressions).
  k == 1: x0' is a select of an input: D = 0.
  0 < k < 1, x0': one blend -- 1 - k, two products and a sum, at most 3 roundings on a path -- of
      a y that is off by d_y:  D_x0 = (1 - k) d_y + bnd(3) on (1 - k) (|y| + d_y) + k |x_k|.
  e (DDIM): eps-prediction e is the model's output m, d_e = d_m = 0 unguided and the case file's
      "eps" bound guided (4 roundings and f_b's relative allowance f_rel); v-prediction e = s1m xt
      + sa m has two table square roots of two roundings each, the product and the fused add on
      top of the guide's 4: bnd(8) on s1m |xt| + sa mag_m with ce = f_rel sa mag_m / mag.
  e_k: two roundings each for sa and s1m, the product, the subtraction and the divide:
      d_ek = bnd(7) on mag_ek = (|xt| + sa |x_k|) / s1m.
  e' in between: D_e = (1 - k) d_e + k d_ek + bnd(3) on (1 - k) (|e| + d_e) + k (|e_k| + d_ek).
  x_prev (DDIM), k > 0: sqrt(a_p) (2 roundings), the product and the fused add: bnd(4) on
      sqrt(a_p) (|x0'| + D_x0) + dir (|e'| + D_e), plus the errors carried in, sqrt(a_p) D_x0 +
      dir D_e, plus dir's own allowance k_dir u32 dir (|e'| + D_e) with _cfg_cases' k_dir at
      sigma = 0: ((1 - a_p) / v + 1) / 2 + 1 = 2 (0 where dir = 0).
  x_prev (2M), k > 0: each path has its product and two additions: bnd(3) on |A| |xt| + |B| (|x0'|
      + D_x0) + |C| |x0_last|, plus |B| D_x0.  The row is the kernel's own fp32 row, exact.

Trajectory (the sampler test).  With eta = 0 an element with k == 1 obeys, for any model output,
xt_i = sqrt(a_p) x_k + sqrt(1 - a_p) z after step i (module docstring of the sampler; a_p the
cumulative alpha of prev_timesteps[i], z the initial noise).  In fp32 the error E_i of xt_i about
that line follows E_i <= g_i E_(i-1) + L_i with the contraction g_i = dir / s1m = sigma_prev /
sigma_t <= 1 (DDIM: x_prev = sqrt(a_p) x_k + dir e_k and e_k = z + E / s1m) or g_i = |A| =
sigma_prev / sigma_t (2M: x_prev = A xt + (B + C) x_k), and the step's own roundings
    L_i = bnd(13) on sqrt(a_p) |x_k| + dir mag_ek + 2 u32 dir mag_ek          (DDIM: e_k's 7, the
          4 of x_prev and k_dir, |xt| <= sa |x_k| + s1m |z| + E_(i-1) inside mag_ek)
    L_i = bnd(4) on |A| |xt| + (|B| + |C|) |x_k|                              (2M: the table's
          one rounding and the path's three; the fp64 rows satisfy A alpha_t + B + C = alpha_prev).
E_(-1), the initial sample q_sample(x_k, z, t0) with two fp32 table square roots: bnd(5) on sa
|x_k| + s1m |z|.  No tolerance here is tuned.
"""
import torch

import _cfg_cases as cfg
import _dpm_cases as dpm
import _thr_cases as thr
from _bounds import U_FP32, bound

W = thr.W
KINDS = thr.KINDS                                  # "ddim-eps", "ddim-v", "dpm"
GUIDES = thr.GUIDES                                # None, (7.5, 0), (7.5, 0.7)
MODES = ("plain", "clip", "threshold")
P_THR = thr.P_THR
EXACT = 1.0 - 4.0 * U_FP32        # the c_extra that makes assert_elementwise's factor exactly 1

# (B, C, S): the scalar path; the 8-wide path; P % 8 == 0 but S % 8 != 0 (a vector straddles two
# channels of the mask: its mask values must be read one element at a time); several blocks per
# sample; the layered grid of the unguided step (more samples than a grid has rows)
SHAPES = [(2, 3, 35), (3, 3, 256), (2, 8, 13), (2, 3, 5000)]
BIG_SHAPE = (65537, 3, 8)
assert (8 * 13) % 8 == 0 and 13 % 8 != 0 and 35 % 8 != 0 and 256 % 8 == 0 and 5000 % 8 == 0


def timesteps(B):
    """Per-sample (t, t_prev) on the 500-step V2 table: _cfg_cases.timesteps for B = 2, 3, its
    three pairs in turn for a larger batch."""
    if B in (2, 3):
        return cfg.timesteps(B)
    idx = torch.arange(B) % 3
    return torch.tensor(cfg.T_ALL)[idx], torch.tensor(cfg.TP_ALL)[idx]


def inputs(B, C, S, bf16, seed=0):
    """xt, c, u, other (z | the 2M history), x_k: fp32 CPU [B, C * S], exact in the kernel dtype.
    The first four are _cfg_cases.inputs; x_k lies in [-1, 1]."""
    P = C * S
    xt, c, u, z = cfg.inputs(B, P, bf16, seed)
    g = torch.Generator().manual_seed(7000 + 10 * P + B % 1000 + seed)
    xk = cfg.rounded((0.6 * torch.randn((B, P), generator=g)).clamp(-1, 1), bf16)
    return xt, c, u, z, xk


# runs of (length, value): exact 0, exact 1, fractions (exact and inexact in binary), values
# outside [0, 1] that the kernel reads as 0 and 1; every kind within the first 13 positions (the
# shortest row).  The period, 39, is odd: over a row the runs start and end at every position of
# an 8-vector.
_RUNS = ((2, 0.0), (3, 1.0), (1, 1.5), (2, 0.25), (1, -0.5), (2, 0.3), (2, 1.0), (5, 0.0),
         (9, 1.0), (4, 0.9), (8, 0.0))
_PERIOD = sum(n for n, _ in _RUNS)
assert _PERIOD == 39


def keep(B, S, per_sample_rows):
    """fp32 [Bk, S], Bk = B (row b shifted by 5 b positions) or 1."""
    pat = torch.cat([torch.full((n,), v) for n, v in _RUNS])
    rows = []
    for b in range(B if per_sample_rows else 1):
        idx = (torch.arange(S) + 5 * b) % _PERIOD
        rows.append(pat[idx])
    return torch.stack(rows).float().contiguous()


def keep_big(B, S):
    """[B, S] for the large batch: the pattern continued across the rows."""
    pat = torch.cat([torch.full((n,), v) for n, v in _RUNS])
    return pat[torch.arange(B * S) % _PERIOD].view(B, S).float().contiguous()


def expand(keep_, B, C):
    """keep [Bk, S] as the kernel reads it for a [B, C * S] sample: element i takes keep[i % S]."""
    return keep_.expand(B, keep_.shape[1]).repeat(1, C).double()


def _bnd(mag, n, ce=0.0):
    return (2.0 * (n + 2) * U_FP32 + ce) * mag


def _mode_refs(base, K, mode):
    if mode == "plain":
        return base
    if mode == "clip":
        return thr.clipped(base, K)
    return thr.thresholded(base, K)


def masked(kind, mode, xt, c, u, other, guide, xk, keep_, *, t=None, tp=None, acp=None,
           row=None):
    """{"x0", "x_prev"} -> (ref, D, 0, EXACT) of the masked step (module docstring), eta = 0.
    kind / guide / t, tp, acp / row as _thr_cases.base64; keep_ [Bk, S]."""
    B, P = xt.shape
    k = expand(keep_, B, P // keep_.shape[1])
    one, zero = k >= 1, k <= 0
    kk = k.clamp(0, 1)
    base, K = thr.base64(kind, xt, c, u, other, guide, t=t, tp=tp, acp=acp, row=row)
    refs = _mode_refs(base, K, mode)
    y, d_y = refs["x0"][0], bound(refs["x0"][0], *refs["x0"][1:3], False, refs["x0"][3])
    xp0, d_xp0 = refs["x_prev"][0], bound(refs["x_prev"][0], *refs["x_prev"][1:3], False,
                                          refs["x_prev"][3])
    xt, c, u, other, xk = (v.double() for v in (xt, c, u, other, xk))
    x0 = torch.where(one, xk, torch.where(zero, y, (1 - kk) * y + kk * xk))
    D_x0 = (1 - kk) * d_y + _bnd((1 - kk) * (y.abs() + d_y) + kk * xk.abs(), 3)
    D_x0 = torch.where(one, torch.zeros_like(D_x0), torch.where(zero, d_y, D_x0))
    if kind == "dpm":
        A, Bc, Cc = (float(v) for v in row[2:5])
        xp = A * xt + Bc * x0 + (Cc * other if Cc != 0.0 else 0.0)
        mag = abs(A) * xt.abs() + abs(Bc) * (x0.abs() + D_x0) + abs(Cc) * other.abs()
        D_xp = _bnd(mag, 3) + abs(Bc) * D_x0
    else:
        # the guided model output and its bound (restated from _cfg_cases.ref64)
        if guide is None:
            m, mag_m = c, c.abs()
            f_rel = torch.zeros((B, 1), dtype=torch.float64)
            d_m = torch.zeros_like(m)
        else:
            w, phi = guide
            f = cfg.factor64(c, u, w, phi)
            m = f * (u + w * (c - u))
            mag_m = f * (u.abs() + abs(w) * (c.abs() + u.abs()))
            f_rel = (cfg.ratio_rel_bound(c, u, w) + 2 * U_FP32) if phi > 0 \
                else torch.zeros_like(f)
            d_m = _bnd(mag_m, 4, f_rel)
        a64 = acp.double()
        at = a64[t].view(-1, 1)
        ap = torch.where(tp >= 0, a64[tp.clamp_min(0)], torch.ones_like(a64[t])).view(-1, 1)
        sa, s1m, sap, dirc = at.sqrt(), (1 - at).sqrt(), ap.sqrt(), (1 - ap).clamp_min(0).sqrt()
        if kind == "ddim-v":
            e = s1m * xt + sa * m
            mag_e = s1m * xt.abs() + sa * mag_m
            d_e = _bnd(mag_e, 8, f_rel * sa * mag_m / mag_e.clamp_min(1e-300))
        else:
            e, d_e = m, d_m
        ek = (xt - sa * xk) / s1m
        mag_ek = (xt.abs() + sa * xk.abs()) / s1m
        d_ek = _bnd(mag_ek, 7)
        e1 = torch.where(one, ek, (1 - kk) * e + kk * ek)
        D_e = (1 - kk) * d_e + kk * d_ek \
            + _bnd((1 - kk) * (e.abs() + d_e) + kk * (ek.abs() + d_ek), 3)
        D_e = torch.where(one, d_ek.expand_as(D_e), D_e)
        k_dir = torch.where(dirc > 0, torch.full_like(dirc, 2.0), torch.zeros_like(dirc))
        xp = sap * x0 + dirc * e1
        mag = sap * (x0.abs() + D_x0) + dirc * (e1.abs() + D_e)
        D_xp = _bnd(mag, 4) + sap * D_x0 + dirc * D_e + k_dir * U_FP32 * dirc * (e1.abs() + D_e)
    xp = torch.where(zero, xp0, xp)
    D_xp = torch.where(zero, d_xp0, D_xp)
    return {"x0": (x0, D_x0, 0, EXACT), "x_prev": (xp, D_xp, 0, EXACT), "one": one,
            "unmasked": refs}


# ------------------------------------------------------------------ the kept line
def on_line(a, xk, z):
    """sqrt(a) x_k + sqrt(1 - a) z in fp64; a: a Python float or a [B, 1] tensor."""
    a = torch.as_tensor(a, dtype=torch.float64)
    return a.sqrt() * xk.double() + (1 - a).clamp_min(0).sqrt() * z.double()


def trajectory(acp, ts, tps, xk, z, rows=None):
    """[(ref_i, E_i)] over the steps for the elements with k == 1 (module docstring): the line at
    prev_timesteps[i] and the absolute bound on an fp32 sample's distance from it.  acp: the
    fp32 table; ts / tps: the sampler's timesteps and previous timesteps; rows: the 2M sampler's
    fp32 coefficient table (None: DDIM).  xk, z: the known clip and the initial noise, any shape."""
    a = [float(v) for v in acp.double()]
    xk, z = xk.double().abs(), z.double().abs()
    t0 = int(ts[0])
    sa, s1m = a[t0] ** 0.5, (1 - a[t0]) ** 0.5
    E = _bnd(sa * xk + s1m * z, 5)
    out = []
    for i, (t, tp) in enumerate(zip(ts, tps)):
        at, ap = a[int(t)], (a[int(tp)] if int(tp) >= 0 else 1.0)
        sa, s1m, sap, dirc = at ** 0.5, (1 - at) ** 0.5, ap ** 0.5, max(1 - ap, 0.0) ** 0.5
        mag_xt = sa * xk + s1m * z + E
        if rows is None:
            mag_ek = (mag_xt + sa * xk) / s1m
            L = _bnd(sap * xk + dirc * mag_ek, 13) + 2 * U_FP32 * dirc * mag_ek
            E = (dirc / s1m) * E + L
        else:
            A, Bc, Cc = (abs(float(v)) for v in rows[i][2:5])
            E = A * E + _bnd(A * mag_xt + (Bc + Cc) * xk, 4)
        out.append((ap, E))
    return out
