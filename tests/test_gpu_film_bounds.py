"""FiLM-conditioned GroupNorm(+SiLU)(+dropout), y = dropout(silu(GN(x) (1 + s) + t)), forward
and backward, bf16 and fp32, against the same formulas in fp64 on the rounded operands, element
by element (tests/_bounds.py), in the manner of test_gpu_groupnorm_bounds.py.

Error model: that file's, with the per-(sample, channel) affine in place of the per-channel one
(s = scale[b, c], t = shift[b, c], broadcast over S):

    |gamma| -> |gamma| |1 + s|           |beta| -> |beta| |1 + s| + |t|

    m_dshift = sum_S m_dz                                          n_terms = n_g + S
    m_dscale = |gamma| sum_S m_dz m_xh + |beta| sum_S m_dz         n_terms = n_g + S
    m_dgamma = sum_{b,S} |1 + s| m_dz m_xh                         n_terms = n_g + B S
    m_dbeta  = sum_{b,S} |1 + s| m_dz                              n_terms = n_g + B S

y and dx keep n_g and 2 n_g.  The __expf allowance c is derived as there: 2 * max |f32 - f64| /
mag of torch's fp32 CPU evaluation of the reference function below against its fp64 evaluation,
per output and case; nothing is taken from the kernels' output, and c < 1e-4 is asserted.

Largest error / bound measured on an MI355X over all cases: bf16 y 0.98, dx 0.95 (the final
rounding); fp32 y 0.10, dx 0.026; dgamma 0.044, dbeta 0.047, dscale 0.052, dshift 0.054; the
allowance c at most 5.5e-7 (0 where the fp32 and fp64 evaluations agree exactly).
"""
import pytest
import torch

from conftest import record_metric

from oracle.fixtures import seeded

from _bounds import assert_elementwise, bf16r

pytestmark = pytest.mark.gpu
dev = "cuda"
G, EPS = 32, 1e-5

SHAPES = [
    (2, 192, 3, 9, 11),   # 6 channels per group: groups straddle a lane's 8-vector; 10 rows / iter
    (1, 32, 2, 4, 4),     # one channel per group
    (2, 1024, 1, 2, 3),   # the largest C
    (2, 64, 1, 1, 3),     # S smaller than the rows per iteration
    (1, 64, 1, 1, 4100),  # 129 chunks: ksplit = 3 with a ragged last chunk
]


def film_ref(x, dy, gamma, beta, s, t, silu, mask, dadd, dt):
    """(y, dx, dgamma, dbeta, dscale, dshift) and their magnitude bounds, evaluated in dtype dt.
    x, dy, mask, dadd: [B, C, *spatial]; s, t: [B, C]; mask holds 0 or 1 / (1 - p)."""
    B, C = x.shape[:2]
    x, dy, mask = (u.to(dt).reshape(B, C, -1) for u in (x, dy, mask))
    g0, b0 = gamma.to(dt)[None, :, None], beta.to(dt)[None, :, None]
    s1, t = 1 + s.to(dt)[:, :, None], t.to(dt)[:, :, None]
    ga, be = g0 * s1, b0 * s1 + t
    m_ga, m_be = g0.abs() * s1.abs(), b0.abs() * s1.abs() + t.abs()
    S = x.shape[2]
    grp = lambda u: u.reshape(B, G, -1)  # noqa: E731
    gmean = lambda u: grp(u).mean(2, keepdim=True).expand(B, G, C // G * S).reshape(B, C, S)  # noqa: E731
    mean = gmean(x)
    rstd = (gmean((x - mean) ** 2) + EPS).rsqrt()
    xh, m_xh = (x - mean) * rstd, (x.abs() + gmean(x.abs())) * rstd
    z, m_z = xh * ga + be, m_xh * m_ga + m_be
    if silu:
        sg = torch.sigmoid(z)
        a, da, L1, L2 = z * sg, sg * (1 + z * (1 - sg)), 1.1, 0.5
    else:
        a, da, L1, L2 = z, torch.ones_like(z), 1.0, 0.0
    y, m_y = a * mask, L1 * m_z * mask
    dz, m_dz = dy * mask * da, dy.abs() * mask * (da.abs() + L2 * m_z)
    A, m_A = dz.sum(2), m_dz.sum(2)                    # [B, C]
    Bs, m_Bs = (dz * xh).sum(2), (m_dz * m_xh).sum(2)  # [B, C]
    dshift, m_dshift = A, m_A
    dscale = g0[:, :, 0] * Bs + b0[:, :, 0] * A
    m_dscale = g0[:, :, 0].abs() * m_Bs + b0[:, :, 0].abs() * m_A
    dbeta, m_dbeta = (s1[:, :, 0] * A).sum(0), (s1[:, :, 0].abs() * m_A).sum(0)
    dgamma, m_dgamma = (s1[:, :, 0] * Bs).sum(0), (s1[:, :, 0].abs() * m_Bs).sum(0)
    dx = rstd * (ga * dz - gmean(ga * dz) - xh * gmean(ga * dz * xh))
    m_dx = rstd * (m_ga * m_dz + gmean(m_ga * m_dz) + m_xh * gmean(m_ga * m_dz * m_xh))
    if dadd is not None:
        dadd = dadd.to(dt).reshape(B, C, S)
        dx, m_dx = dx + dadd, m_dx + dadd.abs()
    return ((y, dx, dgamma, dbeta, dscale, dshift),
            (m_y, m_dx, m_dgamma, m_dbeta, m_dscale, m_dshift))


NAMES = ("y", "dx", "dgamma", "dbeta", "dscale", "dshift")


def _check(shape, dtype, silu, dropout=0.0, with_dadd=False, tag=""):
    from vdiff import ops
    B, C = shape[:2]
    S = 1
    for n in shape[2:]:
        S *= n
    bf = dtype == torch.bfloat16
    rnd = bf16r if bf else (lambda u: u)
    x = rnd(seeded(shape, 60) * 1.5 + 2.0)
    dy = rnd(seeded(shape, 61))
    gamma = 1 + 0.3 * seeded((C,), 62)
    beta = 0.3 * seeded((C,), 63)
    dadd = rnd(seeded(shape, 64)) if with_dadd else None
    s = 0.5 * seeded((B, C), 65)
    t = 0.5 * seeded((B, C), 66)

    xd = ops.to_cl(x.to(dev, dtype)).requires_grad_(True)
    gd, bd = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    fd = torch.cat([s, t], dim=1).to(dev).requires_grad_(True)
    dyd = ops.to_cl(dy.to(dev, dtype))
    if with_dadd:
        y, xs = ops.GroupNormFiLMSiLUFn.apply(xd, gd, bd, fd, G, EPS, silu, 0.0, 0, True)
        torch.autograd.backward([y, xs], [dyd, ops.to_cl(dadd.to(dev, dtype))])
    else:
        y = ops.group_norm_film_silu(xd, gd, bd, fd, G, EPS, silu, dropout=dropout, seed=1234)
        y.backward(dyd)
    torch.cuda.synchronize()
    assert fd.grad.shape == (B, 2 * C) and fd.grad.dtype == torch.float32
    got = [u.detach().float().cpu().reshape(B, C, -1) for u in (y, xd.grad)] + \
        [u.detach().float().cpu() for u in (gd.grad, bd.grad, fd.grad[:, :C], fd.grad[:, C:])]
    mask = torch.ones(shape)
    if dropout > 0:  # the kernel's mask, recovered from y != 0
        keep = got[0].reshape(shape) != 0
        frac = float(keep.float().mean())
        assert abs(frac - (1 - dropout)) < 4 * (dropout * (1 - dropout) / keep.numel()) ** 0.5 + 1e-3
        mask = keep.double() / (1 - dropout)

    ref, mag = film_ref(x, dy, gamma, beta, s, t, silu, mask, dadd, torch.float64)
    r32, _ = film_ref(x, dy, gamma, beta, s, t, silu, mask, dadd, torch.float32)
    n_g = C // G * S
    n_terms = (n_g, 2 * n_g, n_g + B * S, n_g + B * S, n_g + S, n_g + S)
    out = {}
    for name, g_, r_, m_, f_, n_, obf in zip(NAMES, got, ref, mag, r32, n_terms,
                                             (bf, bf, False, False, False, False)):
        c = 2 * float(((f_.double() - r_).abs() / m_.clamp_min(1e-300)).max())
        out["c_" + name] = c
        print(f"film bounds {tag}{shape} {dtype} silu={silu} {name}: c {c:.3g}", flush=True)
        assert c < 1e-4, (name, c)  # the allowance itself stays at fp32 rounding level
        out[name] = assert_elementwise(g_, r_, m_, n_, obf, c_extra=c,
                                       what=f"{tag}{shape} {dtype} silu={silu} {name}")
    print(f"film bounds {tag}{shape} {dtype} silu={silu}: " +
          " ".join(f"{k} {v:.3g}" for k, v in out.items()))
    record_metric(test="film_bounds", tag=tag, shape=list(shape), dtype=str(dtype), silu=silu,
                  **out)


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_film_elementwise_bounds(shape, dtype, silu):
    """y, dx, dgamma, dbeta, dscale and dshift of vd_groupnorm_film_silu_fwd / _bwd_add inside
    the bound of the module docstring at every element; the two samples of a batch carry
    different film rows."""
    _check(shape, dtype, silu)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_film_dropout_elementwise_bounds(dtype):
    """dropout = 0.25 fused after the SiLU, the mask recovered from y != 0."""
    _check((2, 192, 3, 9, 11), dtype, True, dropout=0.25, tag="dropout ")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_film_bwd_add_elementwise_bounds(dtype):
    """vd_groupnorm_film_silu_bwd_add with a dadd, added before the one rounding of dx."""
    _check((2, 192, 3, 9, 11), dtype, True, with_dadd=True, tag="dadd ")
