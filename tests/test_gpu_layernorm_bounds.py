"""LayerNorm forward and backward (layernorm.hip, the ViViT encoder), bf16 and fp32, against the
same formulas in fp64 on the same (bf16-rounded) operands, element by element (tests/_bounds.py);
the saved mean / rstd against fp64; dw / db bit-identical on a second run.

Error model.  m(.) is the mean over the C columns of a row, eps = 1e-6.  Next to every value the
reference carries the same formula on the absolute values of its summed terms:

    mu = m(x)                  rstd = (m((x - mu)^2) + eps)^-1/2
    xh = (x - mu) rstd         m_xh = (|x| + m(|x|)) rstd
    y  = xh w + b              m_y  = m_xh |w| + |b|
    g  = dy w                  m_g  = |dy| |w|
    dx = rstd (g - m(g) - xh m(g xh))
    m_dx = rstd (m_g + m(m_g) + m_xh m(m_g m_xh))
    dw = sum_rows dy xh        m_dw = sum_rows |dy| m_xh
    db = sum_rows dy           m_db = sum_rows |dy|

n_terms is the number of fp32 additions an output depends on: C for y (the row statistics), 2 C
for dx (statistics and the two row sums of the backward), rows + C for dw, rows for db.  y and dx
are rounded to bf16 in bf16 mode; dw and db are fp32 in both.

The kernel evaluates rstd with the fp32 rsqrtf.  Its allowance is the term c * mag of
assert_elementwise, c = 2 * max |f32 - f64| / mag of torch's fp32 CPU evaluation of ln_ref
against its fp64 evaluation (measured 6e-11 .. 4e-7), per output and case, asserted < 1e-4;
nothing is taken from the kernel's output.

mean and rstd (vd_layernorm_fwd called directly), u = 2^-24:

    |mean - mu| <= 2 (C + 2) u m(|x|) =: e_mu
        an fp32 sum of C terms in any order is off by at most (C - 1) u sum|x|, the division by C
        adds u; the factor 2 is the slack of tests/_bounds.py.
    |rstd - rstd_ref| <= rstd_ref (2 (C + 2) u + e_mu^2 / (2 (var + eps)))
        The kernel sums (x - mean)^2 with its own mean.  Exactly, sum (x - mean)^2 =
        sum (x - mu)^2 + C (mean - mu)^2 (the cross term vanishes, sum (x - mu) = 0), so the
        mean's error enters the variance only in second order, by at most e_mu^2.  Every term of
        the sum is positive, so the fp32 roundings (the subtraction, the square: 3 u per term;
        the sum of C terms: (C - 1) u; the division and + eps: 2 u) move var + eps by at most a
        relative (C + 4) u.  d rstd / rstd = -1/2 d(var + eps) / (var + eps) turns that into
        (C + 4) u / 2, rsqrtf adds at most 2 ulp = 4 u: together <= 2 (C + 2) u for C >= 8, the
        same relative first-order bound as the mean's; the second-order term is added to it.

Largest error / bound measured on an MI355X: bf16 y 0.97, dx 0.95 (the final rounding); fp32
y 0.049, dx 0.013; dw 0.046, db 0.11; mean 0.017, rstd 0.044 (the fp32 figures at C = 8 and at
5 rows, where n_terms is smallest).  With x = 0.05 randn + 8: bf16 y 0.20, fp32 y 3e-4.
"""
import pytest
import torch

from conftest import record_metric

from oracle.fixtures import seeded

from _bounds import U_FP32, assert_elementwise, bf16r

pytestmark = pytest.mark.gpu
dev = "cuda"
EPS = 1e-6
NAMES = ("y", "dx", "dw", "db")

# (rows, C, kind)
CASES = [
    (1, 8, "randn"),        # a single lane, a single wave
    (3, 8, "randn"),        # rows fewer than the waves of a block
    (37, 256, "randn"),     # the ViViT width
    (64, 512, "randn"),     # one full chunk; one full backward block
    (65, 520, "randn"),     # one 8-vector into chunk 1; a last backward block of one row
    (5, 504, "randn"),      # one 8-vector short of a chunk
    (67, 1544, "randn"),    # one 8-vector into chunk 3
    (130, 2048, "randn"),   # the widest: three backward blocks, the last with 2 rows
    (67, 1544, "offset"),   # x = 0.05 randn + 8: cancellation in x - mean
    (9, 520, "const"),      # a constant row and an all-zero row among ordinary ones
]


def case_id(c):
    return f"{c[0]}x{c[1]}-{c[2]}"


def ln_inputs(case, bf):
    """x, dy [rows, C] (bf16-rounded in bf16 mode, as fp32), w, b [C] fp32."""
    rows, C, kind = case
    rnd = bf16r if bf else (lambda t: t)
    x = seeded((rows, C), 70)
    x = 0.05 * x + 8.0 if kind == "offset" else 1.5 * x + 0.5
    if kind == "const":
        x[2] = 0.7
        x[5] = 0.0
    return rnd(x), rnd(seeded((rows, C), 71)), 1 + 0.3 * seeded((C,), 72), 0.3 * seeded((C,), 73)


def ln_ref(x, dy, w, b, dt):
    """(y, dx, dw, db), their magnitude bounds and (mu, rstd, m(|x|), var), evaluated in dt."""
    x, dy, w, b = (t.to(dt) for t in (x, dy, w, b))
    m = lambda t: t.mean(1, keepdim=True)  # noqa: E731
    mu = m(x)
    var = m((x - mu) ** 2)
    rstd = (var + EPS).rsqrt()
    xh, m_xh = (x - mu) * rstd, (x.abs() + m(x.abs())) * rstd
    y, m_y = xh * w + b, m_xh * w.abs() + b.abs()
    g, m_g = dy * w, dy.abs() * w.abs()
    dx = rstd * (g - m(g) - xh * m(g * xh))
    m_dx = rstd * (m_g + m(m_g) + m_xh * m(m_g * m_xh))
    dw, m_dw = (dy * xh).sum(0), (dy.abs() * m_xh).sum(0)
    db, m_db = dy.sum(0), dy.abs().sum(0)
    return (y, dx, dw, db), (m_y, m_dx, m_dw, m_db), (mu[:, 0], rstd[:, 0], m(x.abs())[:, 0],
                                                      var[:, 0])


def ln_terms(rows, C):
    return C, 2 * C, rows + C, rows


def ln_judge(got, x, dy, w, b, bf, what=""):
    """got = (y, dx, dw, db): asserts every element inside the bound of the module docstring;
    returns {name: largest error / bound, c_name: the rsqrt allowance}."""
    rows, C = x.shape
    ref, mag, _ = ln_ref(x, dy, w, b, torch.float64)
    r32, _, _ = ln_ref(x, dy, w, b, torch.float32)
    out = {}
    for name, g_, r_, m_, f_, n_, obf in zip(NAMES, got, ref, mag, r32, ln_terms(rows, C),
                                             (bf, bf, False, False)):
        pos = m_ > 0
        c = 2 * float(((f_.double() - r_).abs()[pos] / m_[pos]).max()) if pos.any() else 0.0
        assert c < 1e-4, (name, c)  # the allowance itself stays at fp32 rounding level
        assert bool(torch.isfinite(g_).all()), (what, name)
        out[name] = assert_elementwise(g_, r_, m_, n_, obf, c_extra=c, what=f"{what} {name}")
        out["c_" + name] = c
    return out


def ln_stat_bounds(x):
    """fp64 (mu, rstd) and the bounds of |mean - mu| and |rstd - rstd_ref| (module docstring)."""
    C = x.shape[1]
    _, _, (mu, rstd, mabs, var) = ln_ref(x, x, torch.ones(C), torch.zeros(C), torch.float64)
    e_mu = 2 * (C + 2) * U_FP32 * mabs
    e_rs = rstd * (2 * (C + 2) * U_FP32 + e_mu ** 2 / (2 * (var + EPS)))
    return mu, rstd, e_mu, e_rs


def _run(x, dy, w, b, dtype):
    """ops.layer_norm forward and backward, and vd_layernorm_fwd once more for mean / rstd."""
    from vdiff import _lib, ops
    rows, C = x.shape
    xd = x.to(dev, dtype).requires_grad_(True)
    wd, bd = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    y = ops.layer_norm(xd, wd, bd, EPS)
    y.backward(dy.to(dev, dtype))
    y2 = torch.empty_like(y)
    mean = torch.empty(rows, device=dev, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    xc = xd.detach()
    _lib.call("vd_layernorm_fwd", ops._p(xc), ops._p(wd.detach()), ops._p(bd.detach()),
              ops._p(y2), ops._p(mean), ops._p(rstd), rows, C, EPS, ops._dtype(xc),
              ops._stream(xc))
    torch.cuda.synchronize()
    assert torch.equal(y2, y.detach())
    return [t.detach().float().cpu() for t in (y, xd.grad, wd.grad, bd.grad, mean, rstd)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_ln_elementwise_bounds(case, dtype):
    """y, dx, dw and db of vd_layernorm_fwd / _bwd inside the bound of the module docstring at
    every element, all finite; mean and rstd inside theirs; dw and db of a second run
    bit-identical (the fixed-order finish of the per-block partials)."""
    bf = dtype == torch.bfloat16
    x, dy, w, b = ln_inputs(case, bf)
    *got, mean, rstd = _run(x, dy, w, b, dtype)
    out = ln_judge(got, x, dy, w, b, bf, what=f"{case_id(case)} {dtype}")
    mu, rs, e_mu, e_rs = ln_stat_bounds(x)
    r_mu, r_rs = (mean.double() - mu).abs() / e_mu.clamp_min(1e-300), \
        (rstd.double() - rs).abs() / e_rs
    out["mean"], out["rstd"] = float(r_mu.max()), float(r_rs.max())
    print(f"ln bounds {case_id(case)} {dtype}: " + " ".join(f"{k} {v:.3g}" for k, v in out.items()))
    record_metric(test="ln_bounds", rows=case[0], C=case[1], kind=case[2], dtype=str(dtype), **out)
    assert out["mean"] <= 1.0 and out["rstd"] <= 1.0, out
    again = _run(x, dy, w, b, dtype)
    assert torch.equal(again[2], got[2]) and torch.equal(again[3], got[3])
