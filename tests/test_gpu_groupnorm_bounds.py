"""GroupNorm(+SiLU)(+dropout) forward and backward, bf16 and fp32, against the same formulas in
fp64 on the bf16-rounded operands, element by element (tests/_bounds.py).

Error model.  n_g = (C / G) * S is the length of the statistics sums.  With |.| bounds written
m_*, the reference below carries, next to every value, the same formula on absolute values of
its summed terms, and first-order bounds through the nonlinearity (|silu'| <= 1.1,
|silu''| <= 0.5):

    m_xh = (|x| + mean|x|) rstd          m_z  = m_xh |gamma| + |beta|
    m_y  = L1 m_z mask                   m_dz = |dy| mask (|silu'(z)| + L2 m_z)
    m_dbeta = sum m_dz                   m_dgamma = sum m_dz m_xh
    m_dx = rstd (|gamma| m_dz + mean(|gamma| m_dz) + m_xh mean(|gamma| m_dz m_xh)) + |dadd|

(L1, L2 = 1.1, 0.5 with SiLU, 1, 0 without.)  n_terms is the number of fp32 additions an output
depends on: n_g for y; n_g (statistics) + n_g (the group sums of the backward) for dx;
n_g + B * S for dgamma / dbeta.

The kernels evaluate the sigmoid with __expf.  Its allowance is the term c * mag of
assert_elementwise, c = 2 * max |f32 - f64| / mag of torch's fp32 CPU evaluation of the same
reference function against its fp64 evaluation (measured 2e-9 .. 5e-7), per output and case;
nothing is taken from the kernels' output.

Largest error / bound measured on an MI355X: bf16 y 0.97, dx 0.97 (the final rounding); fp32
y 0.10, dx 0.033; dgamma / dbeta 0.034 (all at S = 3, where n_terms is smallest).
"""
import pytest
import torch

from conftest import record_metric

from oracle.fixtures import seeded

from _bounds import assert_elementwise, bf16r

pytestmark = pytest.mark.gpu
dev = "cuda"
G, EPS = 32, 1e-5


def gn_ref(x, dy, gamma, beta, silu, mask, dadd, dt):
    """(y, dx, dgamma, dbeta) and their magnitude bounds, evaluated in dtype dt.
    x, dy, mask, dadd: [B, C, *spatial]; mask holds 0 or 1 / (1 - p)."""
    B, C = x.shape[:2]
    x, dy, mask = (t.to(dt).reshape(B, C, -1) for t in (x, dy, mask))
    ga, be = gamma.to(dt)[None, :, None], beta.to(dt)[None, :, None]
    S = x.shape[2]
    grp = lambda t: t.reshape(B, G, -1)  # noqa: E731
    gmean = lambda t: grp(t).mean(2, keepdim=True).expand(B, G, C // G * S).reshape(B, C, S)  # noqa: E731
    mean = gmean(x)
    rstd = (gmean((x - mean) ** 2) + EPS).rsqrt()
    xh, m_xh = (x - mean) * rstd, (x.abs() + gmean(x.abs())) * rstd
    z, m_z = xh * ga + be, m_xh * ga.abs() + be.abs()
    if silu:
        sg = torch.sigmoid(z)
        a, da, L1, L2 = z * sg, sg * (1 + z * (1 - sg)), 1.1, 0.5
    else:
        a, da, L1, L2 = z, torch.ones_like(z), 1.0, 0.0
    y, m_y = a * mask, L1 * m_z * mask
    dz, m_dz = dy * mask * da, dy.abs() * mask * (da.abs() + L2 * m_z)
    dbeta, m_dbeta = dz.sum((0, 2)), m_dz.sum((0, 2))
    dgamma, m_dgamma = (dz * xh).sum((0, 2)), (m_dz * m_xh).sum((0, 2))
    dx = rstd * (ga * dz - gmean(ga * dz) - xh * gmean(ga * dz * xh))
    m_dx = rstd * (ga.abs() * m_dz + gmean(ga.abs() * m_dz) + m_xh * gmean(ga.abs() * m_dz * m_xh))
    if dadd is not None:
        dadd = dadd.to(dt).reshape(B, C, S)
        dx, m_dx = dx + dadd, m_dx + dadd.abs()
    return (y, dx, dgamma, dbeta), (m_y, m_dx, m_dgamma, m_dbeta)


def _check(shape, dtype, silu, dropout=0.0, with_dadd=False, tag=""):
    from vdiff import ops
    B, C = shape[:2]
    S = 1
    for s in shape[2:]:
        S *= s
    bf = dtype == torch.bfloat16
    rnd = bf16r if bf else (lambda t: t)
    x = rnd(seeded(shape, 60) * 1.5 + 2.0)
    dy = rnd(seeded(shape, 61))
    gamma = 1 + 0.3 * seeded((C,), 62)
    beta = 0.3 * seeded((C,), 63)
    dadd = rnd(seeded(shape, 64)) if with_dadd else None

    xd = ops.to_cl(x.to(dev, dtype)).requires_grad_(True)
    gd, bd = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    dyd = ops.to_cl(dy.to(dev, dtype))
    if with_dadd:
        y, xs = ops.group_norm_silu_pass(xd, gd, bd, G, EPS, silu)
        torch.autograd.backward([y, xs], [dyd, ops.to_cl(dadd.to(dev, dtype))])
    else:
        y = ops.group_norm_silu(xd, gd, bd, G, EPS, silu, dropout=dropout, seed=1234)
        y.backward(dyd)
    torch.cuda.synchronize()
    got = [t.detach().float().cpu().reshape(B, C, -1) if t.dim() > 1 else t.detach().float().cpu()
           for t in (y, xd.grad, gd.grad, bd.grad)]
    mask = torch.ones(shape)
    if dropout > 0:  # the kernel's mask, as test_fused_dropout_mask_consistency recovers it
        keep = got[0].reshape(shape) != 0
        frac = float(keep.float().mean())
        assert abs(frac - (1 - dropout)) < 4 * (dropout * (1 - dropout) / keep.numel()) ** 0.5 + 1e-3
        mask = keep.double() / (1 - dropout)

    ref, mag = gn_ref(x, dy, gamma, beta, silu, mask, dadd, torch.float64)
    r32, _ = gn_ref(x, dy, gamma, beta, silu, mask, dadd, torch.float32)
    n_g = C // G * S
    n_terms = (n_g, 2 * n_g, n_g + B * S, n_g + B * S)
    out = {}
    for name, g_, r_, m_, f_, n_, obf in zip(("y", "dx", "dgamma", "dbeta"), got, ref, mag, r32,
                                             n_terms, (bf, bf, False, False)):
        c = 2 * float(((f_.double() - r_).abs() / m_.clamp_min(1e-300)).max())
        assert c < 1e-4, (name, c)  # the allowance itself stays at fp32 rounding level
        out[name] = assert_elementwise(g_, r_, m_, n_, obf, c_extra=c,
                                       what=f"{tag}{shape} {dtype} silu={silu} {name}")
        out["c_" + name] = c
    print(f"gn bounds {tag}{shape} {dtype} silu={silu}: " +
          " ".join(f"{k} {v:.3g}" for k, v in out.items()))
    record_metric(test="gn_bounds", tag=tag, shape=list(shape), dtype=str(dtype), silu=silu, **out)


SHAPES = [
    (2, 192, 3, 9, 11),   # 6 channels per group: groups straddle a lane's 8-vector; 10 rows / iter
    (1, 32, 2, 4, 4),     # one channel per group
    (2, 1024, 1, 2, 3),   # the largest C
    (2, 64, 1, 1, 3),     # S smaller than the rows per iteration
    (1, 64, 1, 1, 4100),  # 129 chunks: ksplit = 3 with a ragged last chunk
]


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_gn_elementwise_bounds(shape, dtype, silu):
    """y, dx, dgamma and dbeta of vd_groupnorm_silu_fwd / _bwd_add inside the bound of the
    module docstring at every element."""
    _check(shape, dtype, silu)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_gn_dropout_elementwise_bounds(dtype):
    """dropout = 0.25 fused after the SiLU: with the mask recovered from y != 0, y, dx and
    (which test_fused_dropout_mask_consistency does not compare) dgamma and dbeta."""
    _check((2, 192, 3, 9, 11), dtype, True, dropout=0.25, tag="dropout ")


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_gn_bwd_add_elementwise_bounds(dtype, silu):
    """vd_groupnorm_silu_bwd_add with a dadd (the passthrough alias's gradient), added before
    the one rounding of dx."""
    _check((2, 192, 3, 9, 11), dtype, silu, with_dadd=True, tag="dadd ")
