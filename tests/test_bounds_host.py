"""CPU self-test of tests/_bounds.py: an honest bf16 conv stays inside the element-wise bound,
and a one-pixel missing-tap corruption, which the whole-tensor rel-L2 < 1e-2 of the parity tests
lets through, violates it."""
import pytest
import torch
import torch.nn.functional as F

from oracle.fixtures import rel_l2, seeded

from _bounds import assert_elementwise, bf16r, conv_fwd_ref64, violations

# (x shape, Co): 3x3x3, stride 1, pad 1 (entries of test_gpu_conv.CASES)
SHAPES = [((2, 96, 3, 5, 32), 80), ((1, 512, 2, 4, 6), 256), ((1, 64, 2, 4, 16), 64)]
PIXEL = {0: (1, 1, 2, 17), 1: (0, 1, 2, 3), 2: (0, 0, 1, 9)}  # (b, t, h, w), interior


def _case(i):
    shape, Co = SHAPES[i]
    Ci = shape[1]
    x = bf16r(seeded(shape, 100 + i))
    w = bf16r(seeded((Co, Ci, 3, 3, 3), 200 + i) / (Ci * 27) ** 0.5)
    b = 0.1 * seeded((Co,), 201 + i)
    y32 = F.conv3d(x, w, b, 1, 1)  # fp32 accumulation of exact products
    ref, mag, n = conv_fwd_ref64(x, w, b, 1, 1)
    return x, w, b, y32, ref, mag, n


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_honest_bf16_conv_is_inside_the_bound(i):
    """(a) F.conv3d in fp32 on bf16 operands, rounded to bf16, against fp64: largest
    error / bound measured 0.77."""
    x, w, b, y32, ref, mag, n = _case(i)
    r = assert_elementwise(bf16r(y32), ref, mag, n, True, what=f"emulated conv {SHAPES[i]}")
    assert 0.0 < r <= 1.0
    # the fp32 result itself, no final rounding: inside the fp32-sum term alone
    assert_elementwise(y32, ref, mag, n, False, what="fp32 conv")


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_missing_tap_at_one_pixel_violates_the_bound(i):
    """(b) the centre tap dropped from one output pixel, all channels: at least 90 % of that
    pixel's channels are outside the bound on the 96- and 64-channel shapes (measured 94 % and
    95 %), every other element is still inside; on the first shape the corrupted tensor still
    passes rel_l2 < 1e-2.  At 512 channels (n = 13824) the worst-case fp32-sum term, linear in
    n, is 0.65 of one tap's standard deviation, so only the channels whose centre-tap product
    is not small can violate: measured 62 %; there the test asserts detection alone."""
    x, w, b, y32, ref, mag, n = _case(i)
    bb, t, h, ww = PIXEL[i]
    bad = y32.clone()
    bad[bb, :, t, h, ww] -= w[:, :, 1, 1, 1] @ x[bb, :, t, h, ww]
    bad = bf16r(bad)
    v = violations(bad, ref, mag, n, True)
    Co = SHAPES[i][1]
    at_pixel = int(v[bb, :, t, h, ww].sum())
    print(f"{SHAPES[i]}: {at_pixel} of {Co} channels of the pixel outside the bound")
    assert at_pixel >= (0.9 * Co if SHAPES[i][0][1] <= 96 else 1), (at_pixel, Co)
    assert int(v.sum()) == at_pixel
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_elementwise(bad, ref, mag, n, True, what="corrupted")
    if i == 0:
        assert rel_l2(bad, y32) < 1e-2            # today's whole-tensor check passes it
        assert rel_l2(bf16r(y32), y32) < 3e-3     # an honest bf16 result is ~2e-3


def test_assert_elementwise_reports_and_handles_edges():
    ref = torch.tensor([1.0, -2.0, 0.0], dtype=torch.float64)
    mag = ref.abs()
    assert assert_elementwise(ref.float(), ref, mag, 1, False) == 0.0
    with pytest.raises(AssertionError, match=r"1 of 3 .*first at \(1,\): got -2\.0\d*, ref -2\.0"):
        assert_elementwise(torch.tensor([1.0, -2.0 - 2 ** -7 - 1e-5, 0.0]), ref, mag, 1, True)
    # an fp32 output has no relative term; a non-finite value is a violation
    with pytest.raises(AssertionError):
        assert_elementwise(torch.tensor([1.0, -2.0 - 2 ** -10, 0.0]), ref, mag, 1, False)
    with pytest.raises(AssertionError):
        assert_elementwise(torch.tensor([1.0, float("nan"), 0.0]), ref, mag, 1, True)
    with pytest.raises(AssertionError):
        assert_elementwise(torch.tensor([1.0, -2.0, 1e-30]), ref, mag, 1, True)


# ------------------------------------------- the fp64 references of the GPU bound tests
def test_groupnorm_reference_matches_autograd():
    """gn_ref (tests/test_gpu_groupnorm_bounds.py) in fp64 against torch's own GroupNorm (+ SiLU)
    and its autograd, with a dadd."""
    from test_gpu_groupnorm_bounds import EPS, G, gn_ref
    shape = (2, 192, 3, 9, 11)
    x, dy, dadd = seeded(shape, 1) * 1.5 + 2, seeded(shape, 2), seeded(shape, 5)
    ga, be = 1 + 0.3 * seeded((192,), 3), 0.3 * seeded((192,), 4)
    for silu in (True, False):
        xr, gr, br = (t.double().requires_grad_(True) for t in (x, ga, be))
        y = F.group_norm(xr, G, gr, br, EPS)
        y = F.silu(y) if silu else y
        y.backward(dy.double())
        (ry, rdx, rdg, rdb), mag = gn_ref(x, dy, ga, be, silu, torch.ones(shape), dadd,
                                          torch.float64)
        for a, b in ((ry.reshape(shape), y), (rdx.reshape(shape), xr.grad + dadd.double()),
                     (rdg, gr.grad), (rdb, br.grad)):
            assert float((a - b.detach()).abs().max()) < 1e-11
        for r, m in zip((ry, rdx, rdg, rdb), mag):
            assert bool((m >= r.abs() * (1 - 1e-12)).all())  # a magnitude bounds its value


def test_activation_references_match_autograd():
    from test_gpu_activation_bounds import gelu_ref, silu_ref
    x, dy = 2 * seeded((1000,), 1), seeded((1000,), 2)
    for ref_fn, fn in ((silu_ref, F.silu), (gelu_ref, lambda t: F.gelu(t, approximate="tanh"))):
        xr = x.double().requires_grad_(True)
        y = fn(xr)
        y.backward(dy.double())
        (ry, rdx), (my, mdx) = ref_fn(x, dy, torch.float64)
        assert float((ry - y.detach()).abs().max()) < 1e-13
        assert float((rdx - xr.grad).abs().max()) < 1e-13
        assert bool((my >= ry.abs() * (1 - 1e-12)).all() and (mdx >= rdx.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("mode,B,C,T,HW", [("joint", 2, 64, 3, 67), ("spatial", 2, 32, 5, 13),
                                           ("temporal", 1, 64, 9, 7)])
def test_attention_reference_and_row_statistic(mode, B, C, T, HW):
    """tests/_attn_rows.py: the fp64 reference equals the oracle's attention and its autograd
    through every regrouping (to the oracle's fp32 softmax); the bf16 emulation's worst-row
    statistic is a few 1e-3; and one dQ row that is 10 % off, which moves the whole-tensor
    rel-L2 of d(qkv) by less than 1e-2 (its bar is 4e-2), exceeds 4 x the emulated statistic."""
    from oracle import nn as onn
    import _attn_rows as A
    N = T * HW
    qkv = seeded((B, 3 * C, N), 5).bfloat16().float()
    g = seeded((B, C, N), 6).bfloat16().float()
    qr = qkv.double().requires_grad_(True)
    out = onn.qkv_attention(qr, 1, legacy=True, mode=mode, spatial=(T, HW, 1))
    out.backward(g.double())
    q, k, v = A.sequences(qkv, C, T, HW, mode)
    do, = A.sequences(g, C, T, HW, mode)
    ref, lse, smax = A.reference(q, k, v, do, False)
    emu, lse_e, _ = A.reference(q, k, v, do, True)
    want = dict(zip(("dq", "dk", "dv"), A.sequences(qr.grad, C, T, HW, mode)))
    want["o"], = A.sequences(out.detach(), C, T, HW, mode)
    for name in ref:
        assert float((ref[name] - want[name]).abs().max()) < 2e-6, name
        assert 1e-3 < A.row_stat(emu[name], ref[name]) < 1.2e-2, name
    s = torch.einsum("slc,smc->slm", q, k) / C ** 0.5
    assert float((lse - torch.logsumexp(s, -1)).abs().max()) < 1e-12
    assert bool(((lse_e - lse).abs() <= 2.0 ** -8 * smax + 1e-5).all())
    bad = emu["dq"].clone()
    bad[0, 3] *= 0.9
    cat = lambda d, dq: torch.cat([dq, d["dk"], d["dv"]], -1)  # noqa: E731
    moved = rel_l2(cat(emu, bad), cat(ref, ref["dq"])) - rel_l2(cat(emu, emu["dq"]),
                                                                 cat(ref, ref["dq"]))
    assert moved < 1e-2
    assert A.row_stat(bad, ref["dq"]) > 4 * A.row_stat(emu["dq"], ref["dq"])
