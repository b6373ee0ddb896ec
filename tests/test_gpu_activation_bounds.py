"""vd_silu / vd_silu_bwd and vd_gelu_tanh / vd_gelu_tanh_bwd against fp64, element by element
(tests/_bounds.py, n_terms = 1).  mag is the formula with the absolute value of every summed
term; the allowance c for the fp32 exp / tanh is twice the largest |f32 - f64| / mag of torch's
fp32 CPU evaluation of the same formula (3e-9 .. 8e-7), never the kernels' output.
Largest error / bound measured on an MI355X: bf16 0.995 (the final rounding), fp32 0.62."""
import pytest
import torch

from conftest import record_metric

from oracle.fixtures import seeded

from _bounds import assert_elementwise, bf16r

pytestmark = pytest.mark.gpu
dev = "cuda"
K0, K1 = (2.0 / torch.pi) ** 0.5, 0.044715


def silu_ref(x, dy, dt):
    x, dy = x.to(dt), dy.to(dt)
    s = torch.sigmoid(x)
    return (x * s, dy * s * (1 + x * (1 - s))), \
        ((x * s).abs(), dy.abs() * s * (1 + x.abs() * (1 - s)))


def gelu_ref(x, dy, dt):
    x, dy = x.to(dt), dy.to(dt)
    t = torch.tanh(K0 * x * (1 + K1 * x * x))
    d = 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * K0 * (1 + 3 * K1 * x * x)
    m_d = 0.5 * (1 + t.abs()) + 0.5 * x.abs() * (1 + t * t) * K0 * (1 + 3 * K1 * x * x)
    return (0.5 * x * (1 + t), dy * d), (0.5 * x.abs() * (1 + t.abs()), dy.abs() * m_d)


def _check(name, fn, ref_fn, n, dtype):
    bf = dtype == torch.bfloat16
    rnd = bf16r if bf else (lambda t: t)
    x, dy = rnd(2 * seeded((n,), 70 + n)), rnd(seeded((n,), 71 + n))
    xd = x.to(dev, dtype).requires_grad_(True)
    y = fn(xd)
    y.backward(dy.to(dev, dtype))
    torch.cuda.synchronize()
    assert y.dtype == dtype and xd.grad.dtype == dtype
    ref, mag = ref_fn(x, dy, torch.float64)
    r32, _ = ref_fn(x, dy, torch.float32)
    out = {}
    for what, g, r, m, f in zip(("fwd", "bwd"), (y, xd.grad), ref, mag, r32):
        c = 2 * float(((f.double() - r).abs() / m.clamp_min(1e-300)).max())
        assert c < 1e-6, c
        out[what] = assert_elementwise(g.float(), r, m, 1, bf, c_extra=c,
                                       what=f"{name} {what} n={n} {dtype}")
        out["c_" + what] = c
    print(f"{name} bounds n={n} {dtype}: " + " ".join(f"{k} {v:.3g}" for k, v in out.items()))
    record_metric(test=name + "_bounds", n=n, dtype=str(dtype), **out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [1, 7, 8, 1003])
def test_silu_elementwise_bounds(n, dtype):
    from vdiff import ops
    _check("silu", ops.silu, silu_ref, n, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [8, 1000])
def test_gelu_tanh_elementwise_bounds(n, dtype):
    from vdiff import ops
    _check("gelu_tanh", ops.gelu_tanh, gelu_ref, n, dtype)
