"""Inputs, independent fp64 references and error bounds of the training objective and the
v-prediction samplers (vd_diffusion_loss, vd_diffusion_loss_bwd, vd_ddim_step_pred,
vd_ddim_step_cfg_pred, DPMSolverSampler(prediction="v"), sample_ddpm(prediction="v")), shared
by tests/test_objective_host.py (CPU) and tests/test_gpu_objective.py.  Nothing here imports
the product code except the three shipped schedule tables (through _dpm_cases.schedules): every
formula is written again, in plain Python floats or fp64 tensors.

Notation per sample b: sa = sqrt_acp[t_b], s1m = sqrt_1m_acp[t_b] (the fp32 tables q_sample
reads, taken as exact like the kernel-dtype inputs), snr = (sa / s1m)^2;
  target  eps: eps;  v: sa eps - s1m x0;
  w_b     none: 1;  min-snr: min(snr, gamma) / snr (eps), min(snr, gamma) / (snr + 1) (v);
  mse_b = 1 / P sum_i (pred - target)^2;  loss = 1 / B sum_b w_b mse_b;
  grad = g 2 w_b / (B P) (pred - target).
u32 = 2^-24, u64 = 2^-53.

Rounding counts (n_terms of _bounds.assert_elementwise), every operation rounded to fp32, a
fused multiply-add only removing one; counted on the longest path, for v with min-snr (the
other three combinations have fewer):
  one term d^2: sa eps, s1m x0 and their difference round once each, so the target carries 3;
    pred - target adds 1 and the square adds 1: 5.
  the sum of a sample: a lane adds its LANE(P) squares one after the other, the LDS tree adds
    log2(256) = 8 levels, the finish kernel adds the sample's NB(P) partials in block order, and
    the division by P rounds once: per-sample n = 5 + LANE + 8 + NB + 1.
  w_b: the divide sa / s1m, the square, snr + 1 and the final divide round once each (min is
    exact): 4.
  the loss: w_b mse_b rounds once, the B weighted samples are added in sample order, the
    division by B rounds once: n = per-sample n + 4 + 1 + B + 1.
  the gradient: d has 4; the host rounds scale = 2 / (B P) once, g scale, its product with w_b
    (4 of its own) and the product with d round once each: n = 4 + 1 + 1 + 4 + 1 + 1 = 12.
NB and LANE restate the kernel's partition rule (partials): NB = min(max(ceil(P / 2048), 1),
128) ranges of CHUNK = ceil(ceil(P / NB) / 8) 8 elements, the last one ragged; a lane of the 256
takes VEC elements at a time, so LANE = ceil(CHUNK / (256 VEC)) VEC, at most for VEC = 8.
mag is the same expression with every term replaced by its absolute value: mag_d = |pred| + sa
|eps| + s1m |x0| (eps: |pred| + |eps|), and mag_d^2 in place of d^2.

DDIM with v (ddim_ref64), counted as _cfg_cases.ref64 counts the eps form (guide 4, two
roundings each for sqrt(a_t) and sqrt(1 - a_t), then the arithmetic): x0 = sa xt - s1m v and
eps = s1m xt + sa v have 3 roundings each (two products and the sum) on top of the guide's 4
and the coefficients' 4: 11 for x0, and the derived eps likewise.  x_prev = sqrt(a_p) x0 + dir
eps + sigma z adds what it adds there (2 for sqrt(a_p), the multiply, two fused multiply-adds,
counted 6): 17; the dir eps term is shorter.  Unguided, the guide's 4 leave: 7 and 13.

The Gaussian model in v (host test): data N(0, s^2), V = a s^2 + (1 - a), alpha = sqrt(a), sigma
= sqrt(1 - a): eps* = sigma x / V, x0* = alpha s^2 x / V, v* = alpha eps* - sigma x0* = alpha
sigma (1 - s^2) x / V.  The v recurrence and the eps recurrence are the same map in exact
arithmetic; in fp64 each leaves it by at most (steps N_STEP) u64 mag, mag the recurrence with
every coefficient and term absolute (a running error bound: the absolute map dominates the
propagation of what earlier steps left).  N_STEP adds ALL roundings that feed one step, not
the longest path only, with the rows' A, B, C taken as exact (both forms read the same fp64
numbers):
  c_v: sqrt(a), 1 - a, its sqrt, their product, s s, 1 - s s, the product, V's 4 (s s, a s s, 1 -
    a, the sum; no cancellation), the divide: 12; v = c_v x: 13.  c_eps has 8, eps: 9.
  table step, v rows: sigma / alpha 4 (1 - a, two sqrt, the divide), its product with v 1, the
    subtraction 1, 1 / alpha 2, the divide 1: x0 carries 13 + 9 = 22; A x, B x0, C x0_last and
    the two additions: N_STEP_TABLE = 27 (the eps rows: 20).
  DDIM step in v: alpha x 2, sigma v 2 + 13 + 1, the difference 1: x0 19; eps likewise 19;
    sqrt(a_p) and sqrt(1 - a_p) 3, two products and the sum 3: N_STEP_DDIM = 44 (eps form: 31).
"""
import math

import torch

import _cfg_cases as cfg
import _dpm_cases as dpm
from _bounds import U_FP32

K_BLOCK = 256
K_OBJ_BLOCKS = 128
GAMMA = 5.0
PREDICTIONS = ("eps", "v")
WEIGHTINGS = ("none", "min-snr")
U_FP64 = 2.0 ** -53
N_STEP_TABLE = 27
N_STEP_DDIM = 44


def partials(P):
    """(ranges per sample, elements per range) as vd_diffusion_loss splits a sample."""
    nb = min(max(-(-P // (K_BLOCK * 8)), 1), K_OBJ_BLOCKS)
    chunk = -(-(-(-P // nb)) // 8) * 8
    return nb, chunk


# Two full blocks' worth of elements and three more: the partition rule gives three ranges
# (1368, 1368, 1363), the last one ragged, and P % 8 != 0 takes the element path.
P_RAGGED = 2 * K_BLOCK * 8 + 3
assert partials(P_RAGGED)[0] >= 3
assert 0 < P_RAGGED - (partials(P_RAGGED)[0] - 1) * partials(P_RAGGED)[1] < partials(P_RAGGED)[1]

# _cfg_cases.SHAPES: (3, 768) 8-wide, (2, 105) the element path, (2, 5000) three whole-vector
# ranges; and the ragged one
SHAPES = list(cfg.SHAPES) + [(2, P_RAGGED)]


def lane_adds(P):
    nb, chunk = partials(P)
    return max(-(-chunk // (K_BLOCK * vec)) * vec for vec in (1, 8))


def n_per_sample(P):
    return 5 + lane_adds(P) + 8 + partials(P)[0] + 1


def n_loss(B, P):
    return n_per_sample(P) + 4 + 1 + B + 1


N_GRAD = 12


def tables():
    """(sqrt_acp, sqrt_1m_acp) fp32 of the 500-step V2 schedule, as its q_sample reads them."""
    s = dpm.v2_scheduler()
    return s.sqrt_alpha_cum_prod.float(), s.sqrt_one_minus_alpha_cum_prod.float()


def timesteps(B, T):
    """Per-sample t, all different, with 0 and T - 1 among them."""
    return torch.tensor({2: [T - 1, 0], 3: [0, T // 3, T - 1]}[B])


def inputs(B, P, bf16, seed=0):
    """pred, x0, eps: fp32 CPU tensors [B, P] holding values exact in the kernel dtype."""
    g = torch.Generator().manual_seed(7000 * seed + 10 * P + B)
    x0 = torch.rand((B, P), generator=g) * 2 - 1
    eps = torch.randn((B, P), generator=g)
    pred = 0.7 * eps + 0.5 * torch.randn((B, P), generator=g)
    return tuple(cfg.rounded(x, bf16) for x in (pred, x0, eps))


def weight64(sa, s1m, prediction, weighting, gamma):
    """w_b in fp64 from the fp32 table values ([B] fp64 tensors)."""
    if weighting == "none":
        return torch.ones_like(sa)
    snr = (sa / s1m) ** 2
    m = snr.clamp(max=gamma)
    return m / (snr + 1) if prediction == "v" else m / snr


def ref64(pred, x0, eps, t, sa_tab, s1m_tab, prediction, weighting, gamma=GAMMA, g=1.0):
    """dict name -> (ref, mag, n_terms) for "loss" ([] fp64), "per_sample" ([B]) and "grad"
    ([B, P], for the incoming gradient g)."""
    pred, x0, eps = pred.double(), x0.double(), eps.double()
    B, P = pred.shape
    sa = sa_tab.double()[t].view(-1, 1)
    s1m = s1m_tab.double()[t].view(-1, 1)
    if prediction == "v":
        d = pred - (sa * eps - s1m * x0)
        mag_d = pred.abs() + sa * eps.abs() + s1m * x0.abs()
    else:
        d = pred - eps
        mag_d = pred.abs() + eps.abs()
    w = weight64(sa, s1m, prediction, weighting, gamma)
    per = (d * d).sum(dim=1) / P
    per_mag = (mag_d * mag_d).sum(dim=1) / P
    loss = (w.view(-1) * per).sum() / B
    loss_mag = (w.view(-1) * per_mag).sum() / B
    c = abs(g) * 2.0 * w / (B * P)
    grad = math.copysign(1.0, g) * c * d
    return {"loss": (loss, loss_mag, n_loss(B, P)),
            "per_sample": (per, per_mag, n_per_sample(P)),
            "grad": (grad, c * mag_d, N_GRAD)}


# ------------------------------------------------------------------ DDIM with v
def ddim_ref64(xt, c, u, z, t, tp, acp, w, phi, eta, clip, guided):
    """fp64 references of vd_ddim_step_pred / vd_ddim_step_cfg_pred with prediction v: dict name
    -> (ref, mag, n_terms, c_extra).  c, u: the model's v with / without the audio; guided =
    False steps on c alone.  The guide, f_b and the coefficient allowances are _cfg_cases.ref64's
    (its sigma / dir analysis does not depend on the parameterisation); the terms that carried
    eps there carry the guided v here (module docstring for the counts)."""
    xt, c, u, z = (x.double() for x in (xt, c, u, z))
    acp = acp.double()
    if guided:
        f = cfg.factor64(c, u, w, phi)
        v = f * (u + w * (c - u))
        mag_v = f * (u.abs() + abs(w) * (c.abs() + u.abs()))
        f_rel = (cfg.ratio_rel_bound(c, u, w) + 2 * U_FP32) if phi > 0 else torch.zeros_like(f)
        n_guide = 4
    else:
        v, mag_v = c, c.abs()
        f_rel = torch.zeros((c.shape[0], 1), dtype=torch.float64)
        n_guide = 0
    at = acp[t].view(-1, 1)
    ap = torch.where(tp >= 0, acp[tp.clamp_min(0)], torch.ones_like(acp[t])).view(-1, 1)
    rho = at / ap
    sigma = eta * ((1 - ap) / (1 - at) * (1 - rho)).sqrt()
    var = (1 - ap - sigma ** 2).clamp_min(0)
    dirc = var.sqrt()
    k_sigma = (5 + rho / (1 - rho)) / 2 + 2
    k_dir = torch.where(var > 0, (((1 - ap) + (2 * k_sigma + 1) * sigma ** 2)
                                  / var.clamp_min(1e-300) + 1) / 2 + 1, torch.zeros_like(var))
    s1m, sa = (1 - at).sqrt(), at.sqrt()
    x0 = sa * xt - s1m * v
    mag_x0 = sa * xt.abs() + s1m * mag_v
    eps = s1m * xt + sa * v
    mag_eps = s1m * xt.abs() + sa * mag_v
    x0c = x0.clamp(-1, 1) if clip else x0
    xp = ap.sqrt() * x0c + dirc * eps
    mag_xp = ap.sqrt() * mag_x0 + dirc * mag_eps
    extra_xp = f_rel * (ap.sqrt() * s1m + dirc * sa) * mag_v + k_dir * U_FP32 * dirc * mag_eps
    if eta > 0:
        xp = xp + sigma * z
        mag_xp = mag_xp + sigma * z.abs()
        extra_xp = extra_xp + k_sigma * U_FP32 * sigma * z.abs()
    tiny = 1e-300
    return {"x0": (x0c, mag_x0, 7 + n_guide, f_rel * s1m * mag_v / mag_x0.clamp_min(tiny)),
            "x_prev": (xp, mag_xp, 13 + n_guide, extra_xp / mag_xp.clamp_min(tiny))}


# ------------------------------------------------------------------ DPM-Solver++ rows for v
def coef_rows_v(acp, ts, order):
    """_dpm_cases.coef_rows with columns 0 and 1 replaced by 1 / alpha_t and sigma_t / alpha_t,
    in fp64: x0 = (xt - (sigma / alpha) v) / (1 / alpha) = alpha xt - sigma v."""
    a = [float(v) for v in acp.double()]
    rows = []
    for row, t in zip(dpm.coef_rows(acp, ts, order), ts):
        al, sg = math.sqrt(a[t]), math.sqrt(1.0 - a[t])
        rows.append([1.0 / al, sg / al] + row[2:])
    return rows


# ------------------------------------------------------------------ the Gaussian model in v
def gauss_coefs(a, s):
    """(c_eps, c_v): eps* = c_eps x, v* = c_v x, with V summed from positive terms."""
    V = a * s * s + (1.0 - a)
    al, sg = math.sqrt(a), math.sqrt(1.0 - a)
    return sg / V, al * sg * (1.0 - s * s) / V


def run_table_both(rows_eps, rows_v, a_ts, s):
    """(x_eps, x_v, mag_eps, mag_v): the final sample of x_prev = A x + B x0 + C x0_last from x =
    1 over the eps rows fed eps* and over the v rows fed v*, with each recurrence's magnitude
    (every coefficient and term absolute)."""
    out = []
    for rows, pick in ((rows_eps, 0), (rows_v, 1)):
        x, last, mx, mlast = 1.0, 0.0, 1.0, 0.0
        for row, a in zip(rows, a_ts):
            c = gauss_coefs(a, s)[pick]
            x0 = (x - row[1] * (c * x)) / row[0]
            m0 = (mx + row[1] * abs(c) * mx) / row[0]
            hist = row[4] != 0.0
            x = row[2] * x + row[3] * x0 + (row[4] * last if hist else 0.0)
            mx = abs(row[2]) * mx + abs(row[3]) * m0 + (abs(row[4]) * mlast if hist else 0.0)
            last, mlast = x0, m0
        out.append((x, mx))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def run_ddim_both(acp, ts, s):
    """The same for the DDIM (eta = 0) recurrence: eps form x0 = (x - sigma eps) / alpha; v form
    x0 = alpha x - sigma v, eps = sigma x + alpha v; x_prev = sqrt(a_p) x0 + sqrt(1 - a_p) eps."""
    a = [float(v) for v in acp.double()]
    xe = xv = me = mv = 1.0
    for i, t in enumerate(ts):
        ap = a[ts[i + 1]] if i + 1 < len(ts) else 1.0
        al, sg = math.sqrt(a[t]), math.sqrt(1.0 - a[t])
        ce, cv = gauss_coefs(a[t], s)
        sp, dp = math.sqrt(ap), math.sqrt(1.0 - ap)
        eps = ce * xe
        xe, me = (sp * ((xe - sg * eps) / al) + dp * eps,
                  sp * ((me + sg * abs(ce) * me) / al) + dp * abs(ce) * me)
        v = cv * xv
        xv, mv = (sp * (al * xv - sg * v) + dp * (sg * xv + al * v),
                  sp * (al * mv + sg * abs(cv) * mv) + dp * (sg * mv + al * abs(cv) * mv))
    return xe, xv, me, mv


def bound64(n_steps, n_step, mag_eps, mag_v):
    """|x_v - x_eps| <= 2 (n + 2) u64 (mag_eps + mag_v), n = n_steps n_step: each form's own
    deviation from the exact recurrence, in the idiom of _bounds.bound at u = 2^-53."""
    return 2.0 * (n_steps * n_step + 2) * U_FP64 * (mag_eps + mag_v)
