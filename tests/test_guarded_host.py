"""CPU self-test of tests/_guarded.py: every fault the guarded GPU tests rely on is planted on
CPU tensors and must be reported, and an honest "kernel" must pass."""
import pytest
import torch

from _guarded import ALIGN, GUARD, PATTERN, Guarded, assert_clean, assert_finite

DTYPES = [torch.float32, torch.bfloat16]


def _es(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _pair(dtype):
    """An input x and a pattern-filled output y of an odd shape."""
    x = Guarded((3, 5, 7), dtype, "cpu", data=torch.randn(3, 5, 7), name="x")
    y = Guarded((3, 5, 7), dtype, "cpu", name="y")
    return x, y


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_alignment_and_fill(dtype):
    x, y = _pair(dtype)
    ge = GUARD // _es(dtype)
    for g in (x, y):
        assert g.ptr % ALIGN == 0 and g.ptr % 16 == 0
        assert g.ptr == g.t.data_ptr()
        assert g.off >= ge and g.raw.numel() - g.end >= ge      # 1 MiB on both sides
        assert g.guards_intact() and g.gaps_intact()
    assert bool(y.unwritten().all()) and y.t.shape == (3, 5, 7)
    assert bool(torch.isnan(y.t.float()).all())                 # the pattern reads as NaN
    assert not bool(x.unwritten().any())
    assert torch.equal(x.payload(), x.t) and x.payload().is_contiguous()
    # an odd element offset keeps 16-byte alignment too: the payload never starts mid-vector
    z = Guarded((1,), dtype, "cpu")
    assert z.ptr % 16 == 0
    ws = Guarded.workspace(1000, "cpu")
    assert ws.span == 1000 and ws.ptr % ALIGN == 0 and bool((ws.t == 0xFF).all())
    assert bool(torch.isnan(ws.t[:1000].view(torch.float32)).all())
    assert bool(torch.isnan(ws.t[:1000].view(torch.bfloat16).float()).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_honest_kernel_passes(dtype):
    x, y = _pair(dtype)
    torch.mul(x.t, 2, out=y.t)
    assert_clean(outputs=[y], inputs=[x], what="honest")
    assert torch.equal(y.t, x.t * 2)
    # strided: a channels-last tensor with 8 gap lanes per pixel, an attention buffer with 37
    # gap rows per batch
    xs = Guarded.cl((2, 5, 3, 4), dtype, "cpu", data=torch.randn(2, 5, 3, 4), cstride=13)
    ys = Guarded.cl((2, 5, 3, 4), dtype, "cpu", cstride=13, name="ys")
    assert xs.t.stride() == (3 * 4 * 13, 1, 4 * 13, 13) and xs.span == 2 * 3 * 4 * 13
    assert bool(torch.isnan(xs.raw.view(dtype)[xs.off:xs.end][xs._gap].float()).all())
    ys.t.copy_(xs.t + 1)
    assert_clean(outputs=[ys], inputs=[xs], what="honest strided")
    r = Guarded.rows(2, 7, 6, dtype, "cpu", pad_rows=37, name="rows")
    assert r.t.stride() == (44 * 6, 6, 1) and r.span == 2 * 44 * 6
    r.t.zero_()
    assert_clean(outputs=[r], what="honest rows")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["front", "back", "far_front", "far_back"])
def test_guard_write_is_reported(dtype, where):
    x, y = _pair(dtype)
    torch.mul(x.t, 2, out=y.t)
    at = {"front": y.off - 1, "back": y.end, "far_front": y.off - GUARD // _es(dtype),
          "far_back": y.end + GUARD // _es(dtype) - 1}[where]
    y.raw.view(dtype)[at] = 0.0      # a zero: the value a ragged store most often spills
    assert not y.guards_intact()
    with pytest.raises(AssertionError, match=rf"y: guard written at payload offset {at - y.off} "):
        assert_clean(outputs=[y], inputs=[x], what="planted")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gap_write_is_reported(dtype):
    y = Guarded.cl((2, 5, 3, 4), dtype, "cpu", cstride=13, name="ys")
    y.t.zero_()
    assert y.gaps_intact()
    y.raw.view(dtype)[y.off + 13 + 5] = 1.0      # pixel 1, the first lane past C = 5
    assert y.guards_intact() and not y.gaps_intact()
    with pytest.raises(AssertionError, match="ys: gap written at payload offset 18"):
        assert_clean(outputs=[y], what="planted")
    r = Guarded.rows(2, 7, 6, dtype, "cpu", pad_rows=37, name="rows")
    r.t.zero_()
    r.raw.view(dtype)[r.off + 7 * 6] = 0.0       # the row after the first sequence
    with pytest.raises(AssertionError, match="rows: gap written at payload offset 42"):
        assert_clean(outputs=[r], what="planted")


@pytest.mark.parametrize("dtype", DTYPES)
def test_unwritten_element_is_reported(dtype):
    x, y = _pair(dtype)
    torch.mul(x.t, 2, out=y.t)
    y.raw[y.off + 2 * 35 + 4 * 7 + 6] = PATTERN[dtype]       # the last element
    assert int(y.unwritten().sum()) == 1
    with pytest.raises(AssertionError,
                       match=r"y: 1 of 105 elements unwritten, first at \(2, 4, 6\) "
                             r"\(payload offset 104\)"):
        assert_clean(outputs=[y], inputs=[x], what="planted")


@pytest.mark.parametrize("dtype", DTYPES)
def test_modified_input_is_reported(dtype):
    x, y = _pair(dtype)
    torch.mul(x.t, 2, out=y.t)
    x.t[1, 2, 3] += 1.0
    assert not x.unchanged()
    with pytest.raises(AssertionError, match="x: input modified at payload offset 52"):
        assert_clean(outputs=[y], inputs=[x], what="planted")
    # an input's guard or gap counts as the input
    xs = Guarded.cl((2, 5, 3, 4), dtype, "cpu", data=torch.randn(2, 5, 3, 4), cstride=13,
                    name="xs")
    xs.raw.view(dtype)[xs.off + 5] = 0.0
    with pytest.raises(AssertionError, match="xs: input modified at payload offset 5"):
        assert_clean(inputs=[xs], what="planted")
    x2, _ = _pair(dtype)
    x2.raw[x2.off - 3] = 0
    with pytest.raises(AssertionError, match="x: input modified at payload offset -3"):
        assert_clean(inputs=[x2], what="planted")
    # an output handed on as an input has to be frozen first
    with pytest.raises(AssertionError, match="freeze"):
        assert_clean(inputs=[y], what="unfrozen")
    assert_clean(inputs=[y.freeze()], what="frozen")


def test_no_nan_free_value_equals_the_pattern():
    """The pattern is a NaN in its format, so a finite or infinite payload value can never be
    mistaken for "unwritten": bf16 exhaustively, fp32 by its bit fields."""
    allb = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    same = allb == PATTERN[torch.bfloat16]
    assert int(same.sum()) == 1
    assert bool(torch.isnan(allb.view(torch.bfloat16).float()[same]).all())
    p = PATTERN[torch.float32]
    assert (p >> 23) & 0xFF == 0xFF and p & 0x7FFFFF != 0 and p & 0x400000      # quiet NaN
    assert bool(torch.isnan(torch.tensor([p], dtype=torch.int32).view(torch.float32)).all())
    q = PATTERN[torch.bfloat16]
    assert (q >> 7) & 0xFF == 0xFF and q & 0x7F != 0 and q & 0x40
    # and it is not the NaN arithmetic produces (the canonical quiet NaN), so a computed NaN is
    # reported by the value check, not as "unwritten"
    nan32 = (torch.tensor([float("inf")]) - torch.tensor([float("inf")])).view(torch.int32)
    assert int(nan32) & 0x7FFFFFFF != p
    assert int(nan32.view(torch.float32).bfloat16().view(torch.int16)) & 0x7FFF != q


# ------------------------------------------------------------------ ragged ranges in one payload
LENGTHS = [1, 7, 8, 9, 17, 2049]
STARTS = [0, 8, 16, 32, 49, 80]      # 49: 4-byte but not 16-byte aligned in fp32


def _range_pair(dtype):
    """Ranged input src, ranged in-place operand dst (a shadow, a moment), ranged output out."""
    g = torch.Generator().manual_seed(3)
    data = [torch.randn(n, generator=g) for n in LENGTHS]
    src = Guarded.ranges(LENGTHS, STARTS, dtype, "cpu", data, name="src")
    dst = Guarded.ranges(LENGTHS, STARTS, dtype, "cpu", [d * 0.5 for d in data], name="dst")
    out = Guarded.ranges(LENGTHS, STARTS, dtype, "cpu", name="out")
    return src, dst, out


def _honest_ranges(src, dst, out):
    for i in range(len(LENGTHS)):
        dst.range(i).add_(src.range(i))
        out.range(i).copy_(src.range(i) * 2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ranges_layout_and_honest_kernel(dtype):
    src, dst, out = _range_pair(dtype)
    es = _es(dtype)
    assert src.span == STARTS[-1] + LENGTHS[-1]
    for i, (s, n) in enumerate(zip(STARTS, LENGTHS)):
        assert src.range_ptr(i) == src.ptr + s * es == src.range(i).data_ptr()
        assert src.range(i).numel() == n
    assert src.range_ptr(4) % es == 0 and src.range_ptr(4) % 16 != 0
    gaps = sorted(set(range(src.span)) - {s + k for s, n in zip(STARTS, LENGTHS) for k in range(n)})
    assert gaps and bool(torch.isnan(src.t[gaps].float()).all())      # NaN under an input
    assert int(out.unwritten().sum()) == sum(LENGTHS)                 # the gaps are not counted
    assert not bool(src.unwritten().any())
    _honest_ranges(src, dst, out)
    assert_clean(outputs=[out], inputs=[src], inouts=[dst], what="honest ranges")
    assert_finite([out, dst], what="honest ranges")
    for a, b in zip(out.range_payloads(), src.range_payloads()):
        assert torch.equal(a, b * 2)
    # an in-place operand has to be frozen before the call, like an input
    fresh = Guarded.ranges(LENGTHS, STARTS, dtype, "cpu", name="fresh")
    with pytest.raises(AssertionError, match="freeze"):
        assert_clean(inouts=[fresh], what="unfrozen")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("back", [1, 7])
def test_wide_tail_store_into_the_gap_is_reported(dtype, back):
    """An 8-element store that starts `back` elements before the end of a range (the vector body
    run one vector too far) and so writes 8 - back elements of the gap behind it: reported on an
    output and on an in-place operand, by buffer and by the offset of the first gap element."""
    src, dst, out = _range_pair(dtype)
    _honest_ranges(src, dst, out)
    i = 3                                            # [32, 41): 8 gap elements follow it
    at = STARTS[i] + LENGTHS[i] - back
    for buf in (out, dst):
        buf.t[at:at + 8] = 1.0
    first = STARTS[i] + LENGTHS[i]
    with pytest.raises(AssertionError, match=f"out: gap written at payload offset {first}$"):
        assert_clean(outputs=[out], inputs=[src], what="planted")
    with pytest.raises(AssertionError, match=rf"dst: gap written at payload offset {first} "):
        assert_clean(inputs=[src], inouts=[dst], what="planted")
    # past the last range the same store runs into the back guard
    src, dst, out = _range_pair(dtype)
    _honest_ranges(src, dst, out)
    at = dst.span - back
    dst.raw.view(dtype)[dst.off + at:dst.off + at + 8] = 1.0
    with pytest.raises(AssertionError, match=rf"dst: guard written at payload offset {dst.span} "):
        assert_clean(inputs=[src], inouts=[dst], what="planted")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gap_read_that_reaches_an_output_is_reported(dtype):
    """A vector body that reads 8 elements from the last element of a source range on: the gap's
    NaN enters the arithmetic and arrives in the output and in the in-place operand.  Nothing was
    written out of place, so the layout check alone may pass; the value check names the buffer
    and the offset."""
    src, dst, out = _range_pair(dtype)
    _honest_ranges(src, dst, out)
    i = 2                                            # [16, 24), then 8 gap elements
    s, n = STARTS[i], LENGTHS[i]
    leak = src.t[s + n - 1:s + n + 7].float().sum()  # one element of the range, seven of the gap
    assert bool(torch.isnan(leak))
    out.range(i)[n - 1] = leak
    dst.range(i)[n - 1] += leak
    assert src.unchanged() and out.gaps_intact() and out.guards_intact()
    with pytest.raises(AssertionError,
                       match=rf"out: 1 non-finite elements, first at \({s + n - 1},\) "
                             rf"\(payload offset {s + n - 1}\)"):
        assert_finite([out], what="planted")
    with pytest.raises(AssertionError, match=rf"dst: 1 non-finite elements, first at "
                                             rf"\({s + n - 1},\)"):
        assert_finite([dst], what="planted")
    # the gaps themselves are NaN and are not the value check's business
    assert_finite([src], what="gaps")


@pytest.mark.parametrize("dtype", DTYPES)
def test_unwritten_range_is_reported(dtype):
    src, dst, out = _range_pair(dtype)
    for i in range(len(LENGTHS)):
        if i != 4:                                   # the 17 elements at 49 are skipped
            out.range(i).copy_(src.range(i) * 2)
    with pytest.raises(AssertionError,
                       match=rf"out: 17 of {out.span} elements unwritten, first at \(49,\) "
                             r"\(payload offset 49\)"):
        assert_clean(outputs=[out], inputs=[src], what="planted")
