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


# ------------------------------------------- the sampled conv reference of the ring tests
@pytest.mark.parametrize("case", [6, 7], ids=["stride122", "dims2"])
def test_conv_ref64_at_equals_the_full_references(case):
    """conv_ref64_at (crops only) against conv_fwd_ref64 / conv_bwd_ref64 (the whole conv) at
    the same indices, to 1e-12 of the element's magnitude and of the largest value: a row of
    test_gpu_conv_bounds.CASES with stride (1, 2, 2) (the dx window holds 1 or 2 outputs per
    strided dim) and a 2-D one, with bias, chan_add and residual.  The sample holds every corner
    and face, so the zero padding of the crops is compared too."""
    from test_gpu_conv_bounds import CASES
    from _bounds import (conv_bwd_ref64, conv_ref64_at, gather_pixels, sample_channels,
                         sample_pixels)
    shape, Co, k, stride, pad, _ = CASES[case]
    assert (case == 6 and stride == (1, 2, 2)) or (case == 7 and len(shape) == 4)
    nd, Ci = len(shape) - 2, shape[1]
    x = bf16r(seeded(shape, 1))
    w = bf16r(seeded((Co, Ci) + (k,) * nd, 2) / (Ci * k ** nd) ** 0.5)
    b = 0.1 * seeded((Co,), 3)
    ref, mag, n = conv_fwd_ref64(x, w, b, stride, pad)
    ca = seeded((shape[0], Co), 4)
    res = bf16r(seeded(tuple(ref.shape), 5))
    ref, mag, n = conv_fwd_ref64(x, w, b, stride, pad, ca, res)
    dy = bf16r(seeded(tuple(ref.shape), 6))
    dx, dxm, n_dx, dw, dwm, n_dw = conv_bwd_ref64(x, w, dy, stride, pad)
    y_pix = sample_pixels((shape[0],) + tuple(ref.shape[2:]), 64, 7)
    x_pix = sample_pixels((shape[0],) + tuple(shape[2:]), 64, 8, parity=True)
    if case == 6:
        assert {(int(h) % 2, int(v) % 2) for h, v in x_pix[:, -2:]} == {(0, 0), (0, 1), (1, 0),
                                                                         (1, 1)}
    cos, cis = sample_channels(Co, 8, 9), sample_channels(Ci, 8, 10)
    assert 0 in cos and Co - 1 in cos and 63 in cis and len(cos) >= 8 and len(cis) >= 8
    got = conv_ref64_at(x, w, b, dy, stride, pad, y_pix, x_pix, cos, cis, ca, res)
    want = {"y": (gather_pixels(ref, y_pix), gather_pixels(mag, y_pix), n),
            "dx": (gather_pixels(dx, x_pix), gather_pixels(dxm, x_pix), n_dx),
            "dw": (dw[cos][:, cis], dwm[cos][:, cis], n_dw)}
    for name in ("y", "dx", "dw"):
        (r, m, nt), (wr, wm, wn) = got[name], want[name]
        assert nt == wn and r.shape == wr.shape and r.dtype == torch.float64, name
        assert bool(((r - wr).abs() <= 1e-12 * wm).all()), name
        assert bool(((m - wm).abs() <= 1e-12 * wm).all()), name
        assert float((r - wr).abs().max()) <= 1e-12 * float(wr.abs().max()), name


def test_sample_pixels_holds_the_required_points():
    """At least n pixels, no duplicates, all 8 corners, both ends of the first / middle / last
    128-row tile."""
    from _bounds import sample_pixels
    dims = (1, 4, 91, 90)
    pix = sample_pixels(dims, 256, 3)
    rows = {tuple(int(v) for v in r) for r in pix}
    assert len(rows) == len(pix) >= 256
    for t in (0, 3):
        for h in (0, 90):
            for v in (0, 89):
                assert (0, t, h, v) in rows
    total = 4 * 91 * 90
    flat = {(r[1] * 91 + r[2]) * 90 + r[3] for r in rows}
    nt = (total + 127) // 128
    for t in (0, nt // 2, nt - 1):
        assert t * 128 in flat and min(t * 128 + 127, total - 1) in flat


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


# ------------------------------------------- multi-head and cross-attention per-row checks
@pytest.mark.parametrize("legacy", [True, False])
@pytest.mark.parametrize("mode,B,C,heads,T,HW", [("joint", 2, 64, 2, 3, 23),
                                                 ("spatial", 2, 64, 4, 5, 13),
                                                 ("temporal", 1, 64, 2, 9, 7)])
def test_attention_sequences_split_heads_like_the_oracle(mode, B, C, heads, T, HW, legacy):
    """tests/_attn_rows.py sequences(heads, legacy): the fp64 reference on the split sequences
    equals oracle.nn.qkv_attention(heads, legacy) and its autograd in all three groupings, to the
    oracle's fp32 softmax."""
    from oracle import nn as onn
    import _attn_rows as A
    N = T * HW
    qkv = seeded((B, 3 * C, N), 7).bfloat16().float()
    g = seeded((B, C, N), 8).bfloat16().float()
    qr = qkv.double().requires_grad_(True)
    out = onn.qkv_attention(qr, heads, legacy=legacy, mode=mode, spatial=(T, HW, 1))
    out.backward(g.double())
    q, k, v = A.sequences(qkv, C, T, HW, mode, heads, legacy)
    do, = A.sequences(g, C, T, HW, mode, heads, legacy)
    assert q.shape[-1] == C // heads
    ref, _, _ = A.reference(q, k, v, do, False)
    want = dict(zip(("dq", "dk", "dv"), A.sequences(qr.grad, C, T, HW, mode, heads, legacy)))
    want["o"], = A.sequences(out.detach(), C, T, HW, mode, heads, legacy)
    for name in ref:
        assert float((ref[name] - want[name]).abs().max()) < 2e-6, name


@pytest.mark.parametrize("heads", [1, 2, 4])
@pytest.mark.parametrize("per_frame", [True, False])
def test_cross_attention_reference_matches_the_oracle(per_frame, heads):
    """The cross reference (cross_q_sequences / cross_kv_sequences + reference), per frame and at
    clip level, equals oracle.nn.cross_attention and its autograd to the oracle's fp32 softmax."""
    from oracle import nn as onn
    import _attn_rows as A
    B, C, T, HW, L = 2, 64, 3, 13, 5
    q = seeded((B, C, T * HW), 9).bfloat16().float()
    kv = seeded((B * T, L, 2 * C), 10).bfloat16().float()
    g = seeded((B, C, T * HW), 11).bfloat16().float()
    qr, kvr = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    out = onn.cross_attention(qr, kvr, heads, T, per_frame)
    out.backward(g.double())
    k, v = A.cross_kv_sequences(kv, heads, T, per_frame)
    ref, lse, _ = A.reference(A.cross_q_sequences(q, heads, T, per_frame), k, v,
                              A.cross_q_sequences(g, heads, T, per_frame), False)
    assert ref["o"].shape == ((B * T if per_frame else B) * heads, HW if per_frame else T * HW,
                              C // heads)
    assert k.shape[1] == (L if per_frame else T * L)
    want = dict(o=A.cross_q_sequences(out.detach(), heads, T, per_frame),
                dq=A.cross_q_sequences(qr.grad, heads, T, per_frame))
    want["dk"], want["dv"] = A.cross_kv_sequences(kvr.grad, heads, T, per_frame)
    for name in ref:
        assert float((ref[name] - want[name]).abs().max()) < 2e-6, name


def _self_case_params():
    import _attn_rows as A
    return [pytest.param(c, legacy, id=A.case_id(c[:8]) + f"-legacy{int(legacy)}")
            for c in A.SELF_CASES if c[8] == "auto"
            for legacy in ((True, False) if c[2] > 1 else (True,))]


@pytest.mark.parametrize("case,legacy", _self_case_params())
def test_attention_gpu_self_cases_keep_the_emulation_cap(case, legacy):
    """Every multi-head / amp self-attention GPU case: the emulation's own statistic <= 1.5e-2
    for every output and its lse error <= 1.0 of the bound (measured 4.0e-3 - 8.7e-3, lse at most
    0.28; amp = 1.5: 1.37e-2 and 0.24)."""
    import _attn_rows as A
    B, C, heads, T, HW, mode, seed, amp, _ = case
    _, _, host = A.self_inputs(B, C, T, HW, mode, seed, amp, heads, legacy)
    print(case, legacy, host.emu_stat)
    host.assert_cap()


def _cross_case_params():
    import _attn_rows as A
    return [pytest.param(c, id=A.case_id(c)) for c in A.CROSS_CASES]


@pytest.mark.parametrize("case", _cross_case_params())
def test_attention_gpu_cross_cases_keep_the_emulation_cap(case):
    """Every cross-attention GPU case: the same cap (measured 3.1e-3 - 8.6e-3, lse at most 0.48;
    amp = 1.5: 1.21e-2 and 0.54)."""
    import _attn_rows as A
    _, _, _, host = A.cross_inputs(*case)
    print(case, host.emu_stat)
    host.assert_cap()


def _ring_case_params():
    import _attn_rows as A
    return [pytest.param(c, legacy, id=A.case_id(c) + f"-legacy{int(legacy)}")
            for c in A.RING_SELF_CASES for legacy in ((True, False) if c[2] > 1 else (True,))] + [
        pytest.param(c, None, id="cross-" + A.case_id(c)) for c in A.RING_CROSS_CASES]


@pytest.mark.parametrize("case,legacy", _ring_case_params())
def test_attention_gpu_ring_cases_keep_the_emulation_cap(case, legacy):
    """Every case of tests/test_gpu_ring_determinism.py (N = 4096 / 5000 self-attention, head
    dims 32 / 64 / 128, and the 640-key clip-level cross-attention): the same cap."""
    import _attn_rows as A
    if legacy is None:
        _, _, _, host = A.cross_inputs(*case)
    else:
        B, C, heads, T, HW, mode, seed, amp = case
        _, _, host = A.self_inputs(B, C, T, HW, mode, seed, amp, heads, legacy)
    print(case, legacy, host.emu_stat)
    host.assert_cap()


def test_cross_mutations_pass_the_whole_tensor_bar_and_fail_per_row():
    """At (nseq, Lq, Lk, C) = (1, 3000, 12, 64), the query-split case: (a) dK row 5 summed
    without queries 2944..2999, the last, partial query tile, moves the whole-tensor rel-L2 of
    d(kv) to 0.025 (bar 4e-2) and the row statistic to 0.125, against 4 x 4.3e-3; (b) one dQ row
    of 3000 scaled by 0.9 leaves the rel-L2 of dq at 5e-3 and the row statistic at 0.099, against
    4 x 7.5e-3."""
    import _attn_rows as A
    _, _, _, h = A.cross_inputs(1, 64, 1, 1, 3000, 12, True, 410)
    bad = h.emu["dk"].clone()
    part, _, _ = A.reference(h.q[:, :2944], h.k, h.v, h.do[:, :2944], True)
    # the softmax is per query row, so dK over a subset of the queries is the reference on them
    bad[0, 5] = part["dk"][0, 5]
    cat = lambda dk, dv: torch.cat([dk, dv], -1)  # noqa: E731
    whole = rel_l2(cat(bad, h.emu["dv"]), cat(h.ref["dk"], h.ref["dv"]))
    row = A.row_stat(bad, h.ref["dk"])
    print("dK without the last query tile:", whole, row, h.emu_stat["dk"])
    assert whole < 4e-2
    assert row > 4 * h.emu_stat["dk"]
    bad = h.emu["dq"].clone()
    bad[0, 1234] *= 0.9
    whole = rel_l2(bad, h.ref["dq"])
    row = A.row_stat(bad, h.ref["dq"])
    print("one dQ row x 0.9:", whole, row, h.emu_stat["dq"])
    assert whole < 4e-2
    assert row > 4 * h.emu_stat["dq"]


def test_cross_wrong_audio_window_exceeds_the_row_limit_on_o():
    """The last frame of a batch element attending to the previous frame's audio window (an
    off-by-one in the frame -> window mapping): O of that frame's rows is far outside 4 x the
    emulation's statistic (measured 2.1 against 4 x 4.0e-3)."""
    import _attn_rows as A
    B, C, heads, T, HW, L = 2, 64, 1, 3, 67, 12
    _, _, _, h = A.cross_inputs(B, C, heads, T, HW, L, True, 464)
    seq = (0 * T + T - 1) * heads      # sequence (b = 0, t = T - 1, h = 0)
    wrong, _, _ = A.reference(h.q[seq:seq + 1], h.k[seq - heads:seq - heads + 1],
                              h.v[seq - heads:seq - heads + 1], h.do[seq:seq + 1], True)
    bad = h.emu["o"].clone()
    bad[seq] = wrong["o"][0]
    row = A.row_stat(bad, h.ref["o"])
    print("wrong audio window:", row, h.emu_stat["o"])
    assert row > 4 * h.emu_stat["o"]
    assert A.row_stat(h.emu["o"], h.ref["o"]) <= 4 * h.emu_stat["o"]


# ------------------------------------------- LayerNorm (tests/test_gpu_layernorm_bounds.py)
def _ln_torch(x, dy, w, b, dt, bf=False):
    """torch's own layer_norm and its autograd in dt; y and dx rounded to bf16 in bf16 mode."""
    from test_gpu_layernorm_bounds import EPS
    xr, wr, br = (t.detach().to(dt).clone().requires_grad_(True) for t in (x, w, b))
    y = F.layer_norm(xr, (x.shape[1],), wr, br, EPS)
    y.backward(dy.to(dt))
    r = bf16r if bf else (lambda t: t)
    return r(y.detach()), r(xr.grad), wr.grad, br.grad


def test_layernorm_reference_matches_autograd():
    """ln_ref in fp64 against F.layer_norm and its autograd; every magnitude bounds its value."""
    from test_gpu_layernorm_bounds import ln_inputs, ln_ref
    for case in ((37, 256, "randn"), (67, 1544, "offset"), (9, 520, "const")):
        x, dy, w, b = ln_inputs(case, True)
        ref, mag, (mu, rstd, mabs, var) = ln_ref(x, dy, w, b, torch.float64)
        for a, t, m in zip(ref, _ln_torch(x, dy, w, b, torch.float64), mag):
            assert float((a - t).abs().max()) < 1e-11, case
            assert bool((m >= a.abs() * (1 - 1e-12)).all())
        assert bool((mabs >= mu.abs()).all())


def _ln_case_params():
    from test_gpu_layernorm_bounds import CASES, case_id
    return [pytest.param(c, id=case_id(c)) for c in CASES]


@pytest.mark.parametrize("bf", [True, False])
@pytest.mark.parametrize("case", _ln_case_params())
def test_layernorm_torch_fp32_is_inside_the_bound(case, bf):
    """torch's fp32 F.layer_norm and its autograd on the CPU, y and dx rounded to bf16 in bf16
    mode, lie inside the element-wise bound at every GPU case (the constant / zero row case
    included, which is what keeps it among the GPU cases): the reference alone passes.  Measured
    largest error / bound: bf16 y 0.97, dx 0.94 (the final rounding); fp32 <= 0.06."""
    from test_gpu_layernorm_bounds import ln_inputs, ln_judge
    x, dy, w, b = ln_inputs(case, bf)
    out = ln_judge(_ln_torch(x, dy, w, b, torch.float32, bf), x, dy, w, b, bf, what=str(case))
    print(case, bf, out)
    assert all(v <= 1.0 for k, v in out.items() if not k.startswith("c_"))


@pytest.mark.parametrize("bf", [True, False])
def test_layernorm_mutations_violate_the_bound(bf):
    """(a) dw without the last row's contribution at (65, 520), the row that is alone in the
    last backward block: at least 90 % of the columns are outside the bound; (b) one 8-vector of
    y normalised with the neighbouring row's mean: violations, all inside that vector; both with
    every other output still inside."""
    from test_gpu_layernorm_bounds import ln_inputs, ln_judge, ln_ref
    from _bounds import violations
    case = (65, 520, "randn")
    rows, C, _ = case
    x, dy, w, b = ln_inputs(case, bf)
    ref, mag, (mu, rstd, _, _) = ln_ref(x, dy, w, b, torch.float64)
    y, dx, dw, db = _ln_torch(x, dy, w, b, torch.float32, bf)
    ln_judge((y, dx, dw, db), x, dy, w, b, bf)
    xh_last = (x[-1].double() - mu[-1]) * rstd[-1]
    bad_dw = (dw.double() - dy[-1].double() * xh_last).float()
    n_bad = int(violations(bad_dw, ref[2], mag[2], rows + C, False, 1e-4).sum())
    print("dw without the last row:", n_bad, "of", C)
    assert n_bad >= 0.9 * C
    with pytest.raises(AssertionError, match="outside the bound"):
        ln_judge((y, dx, bad_dw, db), x, dy, w, b, bf)
    r, c0 = 40, 512                     # the one 8-vector of chunk 1
    bad_y = y.clone()
    rnd = bf16r if bf else (lambda t: t)
    bad_y[r, c0:c0 + 8] = rnd(((x[r, c0:c0 + 8].double() - mu[r + 1]) * rstd[r] * w[c0:].double()
                               + b[c0:].double()).float())
    v = violations(bad_y, ref[0], mag[0], C, bf, 1e-4)
    print("8-vector with the neighbour's mean:", int(v.sum()), "of 8")
    assert int(v.sum()) >= 1 and int(v.sum()) == int(v[r, c0:c0 + 8].sum())
    with pytest.raises(AssertionError, match="outside the bound"):
        ln_judge((bad_y, dx, dw, db), x, dy, w, b, bf)
