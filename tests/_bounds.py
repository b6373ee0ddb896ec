"""Element-wise error bounds for the bf16 / fp32 kernels, and the fp64 references they are
checked against.

A kernel that multiplies bf16 operands exactly (MFMA), sums the products in fp32 in any order and
rounds once to bf16 satisfies, for every output element,

    |got - ref| <= u_out * |ref| + 2 * (n + 2) * 2^-24 * mag

where ref is the fp64 result on the same bf16-rounded operands, mag the same expression with
every operand and term replaced by its absolute value, n the reduction length, u_out = 2^-8 (the
bf16 unit roundoff) for a bf16 output and 0 for an fp32 one.  (n + 2) * 2^-24 * mag is the
standard worst-case bound of an fp32 sum of n exact products in any order; the factor 2 covers the
fused epilogue adds and the fp32 -> bf16 double rounding.  The terms are derived, not tuned.
"""
import torch
import torch.nn.functional as F

U_BF16 = 2.0 ** -8
U_FP32 = 2.0 ** -24


def bf16r(t):
    """t rounded to bf16, as fp32."""
    return t.bfloat16().float()


def bound(ref64, mag64, n_terms, out_bf16, c_extra=0.0):
    return (U_BF16 if out_bf16 else 0.0) * ref64.abs() \
        + (2.0 * (n_terms + 2) * U_FP32 + c_extra) * mag64


def max_ratio(got, ref64, mag64, n_terms, out_bf16, c_extra=0.0):
    """Largest |got - ref| / bound over the elements (0 where both are 0)."""
    got = got.detach().cpu().double()
    err = (got - ref64).abs()
    bnd = bound(ref64, mag64, n_terms, out_bf16, c_extra)
    r = torch.where(err > 0, err / bnd.clamp_min(1e-300), torch.zeros_like(err))
    return float(r.max()) if r.numel() else 0.0


def violations(got, ref64, mag64, n_terms, out_bf16, c_extra=0.0):
    """Boolean mask of the elements outside the bound (non-finite values count)."""
    got = got.detach().cpu().double()
    err = (got - ref64).abs()
    return ~(err <= bound(ref64, mag64, n_terms, out_bf16, c_extra))


def assert_elementwise(got, ref64, mag64, n_terms, out_bf16, c_extra=0.0, what=""):
    """Fail on the first element with |got - ref| > (2^-8 if out_bf16 else 0) |ref| +
    (2 (n_terms + 2) 2^-24 + c_extra) mag; returns the largest error / bound ratio.
    c_extra (default 0) is an allowance for a transcendental evaluated in fp32, stated and
    derived by the caller."""
    assert tuple(got.shape) == tuple(ref64.shape), (what, tuple(got.shape), tuple(ref64.shape))
    assert ref64.dtype == torch.float64 and mag64.dtype == torch.float64
    mag64 = mag64.expand_as(ref64)
    bad = violations(got, ref64, mag64, n_terms, out_bf16, c_extra)
    if bad.any():
        g = got.detach().cpu().double()
        idx = tuple(int(i) for i in bad.nonzero()[0])
        b = bound(ref64, mag64, n_terms, out_bf16, c_extra)
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at "
            f"{idx}: got {float(g[idx])!r}, ref {float(ref64[idx])!r}, "
            f"|err| {abs(float(g[idx]) - float(ref64[idx])):.4e} > bound {float(b[idx]):.4e}")
    return max_ratio(got, ref64, mag64, n_terms, out_bf16, c_extra)


# ------------------------------------------------------------------ conv references (fp64)
_CONV = {1: F.conv1d, 2: F.conv2d, 3: F.conv3d}


def _tup(v, nd):
    return (v,) * nd if isinstance(v, int) else tuple(v)


def conv_fwd_ref64(x, w, bias, stride, padding, chan_add=None, residual=None):
    """(ref, mag, n_terms) of y = conv(x, w) + bias + chan_add[b, co] + residual in fp64;
    mag = conv(|x|, |w|) + |bias| + |chan_add| + |residual|."""
    nd = w.dim() - 2
    s, p = _tup(stride, nd), _tup(padding, nd)
    x, w = x.double(), w.double()
    ref = _CONV[nd](x, w, None, s, p)
    mag = _CONV[nd](x.abs(), w.abs(), None, s, p)
    ex = (slice(None), slice(None)) + (None,) * nd
    if bias is not None:
        ref = ref + bias.double()[(None, slice(None)) + (None,) * nd]
        mag = mag + bias.double().abs()[(None, slice(None)) + (None,) * nd]
    if chan_add is not None:
        ref = ref + chan_add.double()[ex]
        mag = mag + chan_add.double().abs()[ex]
    if residual is not None:
        ref = ref + residual.double()
        mag = mag + residual.double().abs()
    return ref, mag, w[0].numel()


def conv_bwd_ref64(x, w, dy, stride, padding):
    """fp64 gradients of sum(conv(x, w) * dy): (dx, |dx| bound, n_dx, dw, |dw| bound, n_dw).
    The magnitudes are the same (bilinear) gradients of |x|, |w|, |dy|; n_dx = Co * taps (the
    longest dX reduction), n_dw = B * To * Ho * Wo."""
    nd = w.dim() - 2
    s, p = _tup(stride, nd), _tup(padding, nd)

    def grads(x_, w_, dy_):
        x_ = x_.double().requires_grad_(True)
        w_ = w_.double().requires_grad_(True)
        y = _CONV[nd](x_, w_, None, s, p)
        return torch.autograd.grad(y, (x_, w_), dy_.double())

    dx, dw = grads(x, w, dy)
    dxm, dwm = grads(x.abs(), w.abs(), dy.abs())
    n_dx = w.shape[0] * w[0, 0].numel()
    n_dw = dy.numel() // dy.shape[1]
    return dx, dxm, n_dx, dw, dwm, n_dw

