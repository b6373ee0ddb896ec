"""Inputs, fp64 references and error bounds of the classifier-free guidance kernels
(vd_cfg_stats, vd_ddim_step_cfg, vd_cfg_combine), shared by tests/test_cfg_host.py (CPU) and
tests/test_gpu_cfg.py so that the host test bounds the very inputs the GPU test runs.

Notation: c / u the conditional / unconditional noise, g = u + w (c - u), f_b = phi r_b +
(1 - phi) with r_b = sqrt(SS(c_b) / SS(g_b)), SS(x) = sum (x_i - mean(x))^2, eps = f_b g.
u32 = 2^-24.

The bound on r_b (ratio_rel_bound) is the one the feature's specification gives, unchanged:
r_rel <= 2 (P + 2) u32 + 4 u32 (rms|c| / sigma_c + rms(mag_g) / sigma_g),
mag_g = |u| + |w| (|c| + |u|), sigma^2 = SS / P.  Its derivation stands in the docstring of
tests/test_cfg_host.py::test_rescale_factor_bound_holds_for_the_shipped_order, which also shows
that an fp32 emulation of the shipped reduction order stays inside it on these inputs.  Since
phi r <= f, the same number bounds the relative error of f_b.
"""
import torch

from _bounds import U_FP32

# (B, per_sample): the conv-shaped sample, the scalar path (P % 8 != 0), and whole 8-vectors
# over three partials whose ranges (1672, 1672, 1656) are no multiple of a block's 2048
SHAPES = [(3, 3 * 4 * 8 * 8), (2, 105), (2, 5000)]
T_ALL, TP_ALL = [499, 10, 0], [489, 0, -1]
OFFSET_SAMPLE = 1  # mean 16, sigma 0.25 in both halves
K_BLOCK = 256      # threads per block, 8 elements per lane per iteration (elementwise.hip)
K_CFG_BLOCKS = 128


def timesteps(B):
    """Per-sample (t, t_prev) on the 500-step V2 table; B = 2 keeps the first and the last
    (t_prev = -1) pair."""
    idx = {3: [0, 1, 2], 2: [0, 2]}[B]
    return (torch.tensor([T_ALL[i] for i in idx]), torch.tensor([TP_ALL[i] for i in idx]))


def rounded(x, bf16):
    return x.bfloat16().float() if bf16 else x.float()


def inputs(B, P, bf16, seed=0):
    """xt, c, u, z: fp32 CPU tensors [B, P] holding values exact in the kernel dtype."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * P + B)
    xt = torch.randn((B, P), generator=g) * 1.5
    c = torch.randn((B, P), generator=g)
    u = 0.8 * c + 0.6 * torch.randn((B, P), generator=g)
    z = torch.randn((B, P), generator=g)
    c[OFFSET_SAMPLE] = 16 + 0.25 * c[OFFSET_SAMPLE]
    u[OFFSET_SAMPLE] = 16 + 0.25 * u[OFFSET_SAMPLE]
    return tuple(rounded(x, bf16) for x in (xt, c, u, z))


def partials(P):
    """(number of partials per sample, elements per range) as vd_cfg_stats splits a sample."""
    nb = min(max(-(-P // (K_BLOCK * 8)), 1), K_CFG_BLOCKS)
    chunk = -(-(-(-P // nb)) // 8) * 8
    return nb, chunk


def _ss(x):
    return ((x - x.mean(dim=1, keepdim=True)) ** 2).sum(dim=1, keepdim=True)


def ratio_rel_bound(c, u, w):
    """[B, 1] fp64: the bound on the relative error of sqrt(SS(c) / SS(g)) (module docstring)."""
    c, u = c.double(), u.double()
    P = c.shape[1]
    mag_g = u.abs() + abs(w) * (c.abs() + u.abs())
    g = u + w * (c - u)

    def rms(x):
        return (x ** 2).mean(dim=1, keepdim=True).sqrt()

    kc = rms(c) / (_ss(c) / P).sqrt()
    kg = rms(mag_g) / (_ss(g) / P).sqrt()
    return 2 * (P + 2) * U_FP32 + 4 * U_FP32 * (kc + kg)


def factor64(c, u, w, phi):
    """[B, 1] fp64 f_b."""
    c, u = c.double(), u.double()
    if phi == 0:
        return torch.ones((c.shape[0], 1), dtype=torch.float64)
    return phi * (_ss(c) / _ss(u + w * (c - u))).sqrt() + (1 - phi)


def _fma32(a, b, s):
    """fp32 fma: the product of two fp32 values is exact in fp64; one fp64 add, then fp32."""
    return (a.double() * b.double() + s.double()).float()


def _lane_layout(x, lo, hi, vec):
    """Elements [lo, hi) of the 1-D x as [256 lanes, steps]: lane l takes vec consecutive
    elements at lo + (l + 256 k) vec, k = 0, 1, ...; absent elements are 0 (adding 0, or
    fma(0, 0, s), changes nothing)."""
    n = hi - lo
    iters = -(-n // (K_BLOCK * vec))
    buf = torch.zeros(iters * K_BLOCK * vec, dtype=x.dtype)
    buf[:n] = x[lo:hi]
    return buf.view(iters, K_BLOCK, vec).permute(1, 0, 2).reshape(K_BLOCK, iters * vec)


def _tree(red):
    red = red.clone()
    w = K_BLOCK // 2
    while w > 0:
        red[:w] = red[:w] + red[w:2 * w]
        w //= 2
    return red[0]


def emulate_ratio_fp32(c, u, w):
    """[B] fp32: sqrt(SS(c) / SS(g)) in the shipped reduction order, every operation rounded to
    fp32 -- per lane in element order, the 256-lane LDS tree, the blocks' partials one per lane
    through the same tree, the mean as sum / P, then the centred fused multiply-adds the same
    way."""
    B, P = c.shape
    nb, chunk = partials(P)
    vec = 8 if P % 8 == 0 else 1
    wf = torch.tensor(w, dtype=torch.float32)
    out = []
    for b in range(B):
        cb, ub = c[b].float(), u[b].float()
        gb = _fma32(wf, cb - ub, ub)
        res = []
        for x in (cb, gb):
            total = torch.zeros(K_BLOCK, dtype=torch.float32)  # partial k in lane k
            lanes = []
            for k in range(nb):
                lo, hi = k * chunk, min((k + 1) * chunk, P)
                lay = _lane_layout(x, lo, hi, vec)
                lanes.append((lay, _lane_layout(torch.ones_like(x), lo, hi, vec)))
                s = torch.zeros(K_BLOCK, dtype=torch.float32)
                for j in range(lay.shape[1]):
                    s = s + lay[:, j]
                total[k] = _tree(s)
            mean = _tree(total) / torch.tensor(float(P), dtype=torch.float32)
            q = torch.zeros(K_BLOCK, dtype=torch.float32)
            for k, (lay, present) in enumerate(lanes):
                s = torch.zeros(K_BLOCK, dtype=torch.float32)
                for j in range(lay.shape[1]):
                    d = (lay[:, j] - mean) * present[:, j]
                    s = _fma32(d, d, s)
                q[k] = _tree(s)
            res.append(_tree(q))
        out.append(torch.sqrt(res[0] / res[1]))
    return torch.stack(out)


def ref64(xt, c, u, z, t, tp, acp, w, phi, eta, clip, composed_bf16=False):
    """fp64 references, magnitudes (every term absolute) and allowances of eps, x0 and x_prev:
    dict name -> (ref, mag, n_terms, c_extra).

    n_terms counts the fp32 roundings on the longest path.  eps: c - u, the fma, f * g: 3 -> 4.
    x0 = (xt - s eps) / a: + the fma and the divide, and two roundings each for s = sqrt(1 -
    a_t) and a = sqrt(a_t): 9 -> 10.  x_prev = sqrt(a_p) x0 + dir eps + sigma z: + 2 for
    sqrt(a_p), the multiply and two fmas: 14 -> 16.  c_extra holds what is no plain rounding
    count: f_b (ratio_rel_bound + 2 u32, on every term that carries eps) and the two
    coefficients that subtract nearly equal numbers, in units of u32 relative:
      sigma = eta sqrt((1 - a_p) / (1 - a_t) (1 - rho)), rho = a_t / a_p: 1 - a is one rounding
      (exact above 0.5), the quotient one more, rho's rounding is amplified by rho / (1 - rho),
      then the product, the square root (halving what came before) and eta:
      k_sigma = (3 + 1 + rho / (1 - rho) + 1) / 2 + 2;
      dir = sqrt(v), v = 1 - a_p - sigma^2: absolute error u32 ((1 - a_p) + (2 k_sigma + 1)
      sigma^2 + v): k_dir = (((1 - a_p) + (2 k_sigma + 1) sigma^2) / v + 1) / 2 + 1.
    They weigh the sigma |z| and dir mag_eps terms only.  composed_bf16: eps was rounded to bf16
    between cfg_combine and ddim_step, a relative 2^-8 on every term that carries eps."""
    xt, c, u, z = (x.double() for x in (xt, c, u, z))
    acp = acp.double()
    f = factor64(c, u, w, phi)
    g = u + w * (c - u)
    mag_g = u.abs() + abs(w) * (c.abs() + u.abs())
    eps, mag_eps = f * g, f * mag_g
    f_rel = (ratio_rel_bound(c, u, w) + 2 * U_FP32) if phi > 0 else torch.zeros_like(f)
    if composed_bf16:
        f_rel = f_rel + 2.0 ** -8
    at = acp[t].view(-1, 1)
    ap = torch.where(tp >= 0, acp[tp.clamp_min(0)], torch.ones_like(acp[t])).view(-1, 1)
    rho = at / ap
    sigma = eta * ((1 - ap) / (1 - at) * (1 - rho)).sqrt()
    v = (1 - ap - sigma ** 2).clamp_min(0)
    dirc = v.sqrt()
    k_sigma = (5 + rho / (1 - rho)) / 2 + 2
    k_dir = torch.where(v > 0, (((1 - ap) + (2 * k_sigma + 1) * sigma ** 2)
                                / v.clamp_min(1e-300) + 1) / 2 + 1, torch.zeros_like(v))
    s, a = (1 - at).sqrt(), at.sqrt()
    x0 = (xt - s * eps) / a
    mag_x0 = (xt.abs() + s * mag_eps) / a
    x0c = x0.clamp(-1, 1) if clip else x0
    xp = ap.sqrt() * x0c + dirc * eps
    mag_xp = ap.sqrt() * mag_x0 + dirc * mag_eps
    extra_xp = f_rel * (ap.sqrt() * s / a + dirc) * mag_eps + k_dir * U_FP32 * dirc * mag_eps
    if eta > 0:
        xp = xp + sigma * z
        mag_xp = mag_xp + sigma * z.abs()
        extra_xp = extra_xp + k_sigma * U_FP32 * sigma * z.abs()
    tiny = 1e-300
    return {
        "eps": (eps, mag_eps, 4, f_rel.expand_as(eps)),
        "x0": (x0c, mag_x0, 10, f_rel * (s / a) * mag_eps / mag_x0.clamp_min(tiny)),
        "x_prev": (xp, mag_xp, 16, extra_xp / mag_xp.clamp_min(tiny)),
    }
