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



# ------------------------------------------------------------------ sampled conv reference
def sample_pixels(dims, n, seed, parity=False, tile=128):
    """Rows (b, i_1, ..., i_nd) of a [B, *spatial] grid `dims`: n seeded draws plus every corner,
    one pixel on each face, the first and last pixel of the first, a middle and the last
    `tile`-row tile of the flattened grid (the GEMM's M tiles) and, with parity, one interior
    pixel of each (h, w) parity.  Sorted, without duplicates."""
    import itertools
    dims = tuple(int(d) for d in dims)
    sp = dims[1:]
    total = 1
    for d in dims:
        total *= d
    g = torch.Generator().manual_seed(seed)
    flat = set()
    while len(flat) < min(n, total):  # repeated draws are topped up: at least n distinct pixels
        for m in torch.randint(0, total, (n,), generator=g).tolist():
            if len(flat) < n:
                flat.add(m)

    def lin(idx):
        m = 0
        for i, d in zip(idx, dims):
            m = m * d + i
        return m

    for b in {0, dims[0] - 1}:
        for c in itertools.product(*[(0, d - 1) for d in sp]):
            flat.add(lin((b,) + c))
        mid = tuple(d // 2 for d in sp)
        for a in range(len(sp)):
            for side in (0, sp[a] - 1):
                flat.add(lin((b,) + mid[:a] + (side,) + mid[a + 1:]))
    ntile = (total + tile - 1) // tile
    for t in {0, ntile // 2, ntile - 1}:
        flat.add(t * tile)
        flat.add(min(t * tile + tile - 1, total - 1))
    if parity and len(sp) >= 2:
        mid = [d // 2 for d in sp]
        for ph in (0, 1):
            for pw in (0, 1):
                c = list(mid)
                c[-2] = min(mid[-2] - mid[-2] % 2 + ph, sp[-2] - 1)
                c[-1] = min(mid[-1] - mid[-1] % 2 + pw, sp[-1] - 1)
                flat.add(lin((0,) + tuple(c)))
    m = torch.tensor(sorted(flat), dtype=torch.int64)
    cols = []
    for d in reversed(dims):
        cols.append(m % d)
        m = m // d
    return torch.stack(cols[::-1], 1)


def sample_channels(C, n, seed, tile=64):
    """At least n channels of C (all of them if C < n): channel 0, the last channel of every
    `tile`-wide tile, then seeded draws up to n."""
    want = [0] + [min(t + tile, C) - 1 for t in range(0, C, tile)]
    g = torch.Generator().manual_seed(seed)
    for c in torch.randperm(C, generator=g).tolist():
        if len(set(want)) >= min(n, C):
            break
        want.append(c)
    return sorted(set(want))


def gather_pixels(t, pix):
    """t [B, C, *spatial] at the rows of pix -> [P, C]."""
    idx = (pix[:, 0], slice(None)) + tuple(pix[:, 1 + a] for a in range(pix.shape[1] - 1))
    return t[idx]


def _crops(t, pix_b, start, length):
    """Zero-padded crops of t [B, C, *spatial]: for pixel row r the box start[r] .. start[r] +
    length (per dim, may reach outside) -> fp64 [P, C, *length]."""
    nd = len(length)
    P, C = start.shape[0], t.shape[1]
    out = torch.zeros((P, C) + tuple(length), dtype=torch.float64)
    for r in range(P):
        src, dst = [int(pix_b[r]), slice(None)], [r, slice(None)]
        empty = False
        for a in range(nd):
            lo = int(start[r, a])
            s0, s1 = max(lo, 0), min(lo + length[a], t.shape[2 + a])
            if s1 <= s0:
                empty = True
                break
            src.append(slice(s0, s1))
            dst.append(slice(s0 - lo, s1 - lo))
        if not empty:
            out[tuple(dst)] = t[tuple(src)].double()
    return out


def conv_ref64_at(x, w, bias, dy, stride, padding, y_pix, x_pix, cos, cis, chan_add=None,
                  residual=None):
    """The references of conv_fwd_ref64 / conv_bwd_ref64 at sampled elements only, in fp64 on
    crops, never the full conv: y [P, Co] at the output pixels y_pix (rows (b, o_1..o_nd)) from
    the receptive field of each pixel; dx [Q, Ci] at the input pixels x_pix from the outputs that
    read that pixel (autograd of the conv of the crop that feeds them); dw [len(cos), len(cis),
    *k] for the channel pairs cos x cis, all taps, over all pixels (autograd of the conv cropped
    to those channels).  Returns {"y" | "dx" | "dw": (ref, mag, n_terms)} with the magnitudes and
    term counts of the full references."""
    nd = w.dim() - 2
    conv = _CONV[nd]
    s, p = _tup(stride, nd), _tup(padding, nd)
    k = tuple(w.shape[2:])
    w64 = w.double()
    out = {}
    # ---- y: the k-box of x that pixel o reads starts at o * s - p
    start = y_pix[:, 1:] * torch.tensor(s) - torch.tensor(p)
    xc = _crops(x, y_pix[:, 0], start, k)
    ref = conv(xc, w64).reshape(len(y_pix), -1)
    mag = conv(xc.abs(), w64.abs()).reshape(len(y_pix), -1)
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    if chan_add is not None:
        ca = chan_add.double()[y_pix[:, 0]]
        ref, mag = ref + ca, mag + ca.abs()
    if residual is not None:
        r = gather_pixels(residual, y_pix).double()
        ref, mag = ref + r, mag + r.abs()
    out["y"] = (ref, mag, w[0].numel())
    # ---- dx: input i is read by the outputs o with o * s - p <= i <= o * s - p + k - 1; a fixed
    # window of n_o = (k - 1) // s + 1 outputs from o_lo = ceil((i + p - k + 1) / s) holds them
    # (outputs outside the tensor carry zero dy; window members that do not read i give zero)
    n_o = tuple((k[a] - 1) // s[a] + 1 for a in range(nd))
    i_p = x_pix[:, 1:] + torch.tensor(p)
    o_lo = -((-(i_p - torch.tensor(k) + 1)) // torch.tensor(s))  # ceil division
    dyc = _crops(dy, x_pix[:, 0], o_lo, n_o)
    box = tuple((n_o[a] - 1) * s[a] + k[a] for a in range(nd))
    pos = x_pix[:, 1:] - (o_lo * torch.tensor(s) - torch.tensor(p))
    assert bool((pos >= 0).all()) and bool((pos < torch.tensor(box)).all())
    sel = (torch.arange(len(x_pix)), slice(None)) + tuple(pos[:, a] for a in range(nd))

    def dx_of(dy_, w_):
        z = torch.zeros((len(x_pix), w.shape[1]) + box, dtype=torch.float64, requires_grad=True)
        g, = torch.autograd.grad(conv(z, w_, None, s), z, dy_)
        return g[sel]

    out["dx"] = (dx_of(dyc, w64), dx_of(dyc.abs(), w64.abs()), w.shape[0] * w[0, 0].numel())
    # ---- dw: all pixels, the sampled channels only
    xs, dys = x[:, cis].double(), dy[:, cos].double()

    def dw_of(x_, dy_):
        z = torch.zeros((len(cos), len(cis)) + k, dtype=torch.float64, requires_grad=True)
        g, = torch.autograd.grad(conv(x_, z, None, s, p), z, dy_)
        return g

    out["dw"] = (dw_of(xs, dys), dw_of(xs.abs(), dys.abs()), dy.numel() // dy.shape[1])
    return out
