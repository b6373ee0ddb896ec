"""Self- and cross-attention on guarded, NaN-poisoned buffers (tests/_guarded.py), through
vdiff._lib.call with the descriptors of ops._attn_desc / ops._xattn_desc and the call order of
ops.AttentionFn / ops.CrossAttentionFn, on buffers that are the test's own.

qkv (q, kv), dout and, once written, o and lse are inputs between two 1 MiB guards of a NaN
pattern; o, lse, dqkv (dq, dkv) start out as the pattern; every workspace is exactly
*_workspace_size() bytes of 0xFF, a fresh one per launch as in vdiff.ops.  After the forward and
after the backward: outputs fully written, guards and gap rows bit-intact, inputs bit-identical.
O, dQ, dK, dV and lse are judged by _attn_rows.Host.assert_cap() and .judge(), unchanged (4 x the
CPU emulation per row, the lse bound); the cases are those whose emulation cap
tests/test_bounds_host.py and the unguarded GPU tests already hold, same tuples and seeds.

Two layouts:
  exact   the layout the descriptors describe; outside is the guards only.  The last sequence's
          tail tile, the short kernels' last wave and the hand-scheduled kernels' buffer ranges
          (kv_bytes, o_bytes of fwd_asm_launch: they DMA up to 12 tiles past the sequence) are
          exercised against NaN.
  padded  joint, spatial and cross cases: batch_stride = (seq_len + 37) * row for q / k / v and
          dqkv, o_batch_stride = (seq_len + 37) * orow for o and dout, kv_batch_stride =
          (kv_len + 5) * 2C: every sequence is followed by 37 (5) gap rows, NaN under the inputs
          and bit-intact under o, dq, dk, dv.  Temporal sequences interleave and keep the exact
          fit.  All strides stay multiples of 8 elements, so the alignment conditions of
          asm_fwd_ok / asm_dq_ok and of the short-path predicate hold as in the exact layout.

Besides the pair vd_attention_bwd_dq / _dkdv that AttentionFn launches, every flash case also runs
the one-call vd_attention_bwd into a second guarded dqkv and a poisoned workspace of its own; the
two must agree bit for bit.  The short path (vd_attention_short_path, asserted) runs
vd_attention_bwd alone, without a workspace, as AttentionFn does.

Kernel selection is not asserted beyond the short path.  It was confirmed once by hand with a
kernel trace of this file on an MI355X, the exact and the padded cases (temporal ones left out of
both) in a process each: every kernel of the library was dispatched the same number of times in
both layouts.  Among them the hand-scheduled vd_attn_fwd_d64 / _d128 / _d256 (once each) and
vd_attn_bwd_dq_* / vd_attn_bwd_dkdv_* (twice each: the pair and vd_attention_bwd) of the 1157-token
"auto" rows; attn_fwd_kernel<.., 4 waves> with attn_fwd_combine_kernel, attn_bwd_dq_kernel with
attn_dq_sum_kernel and attn_bwd_dkdv_kernel (the KV-split workspace path) under "base";
attn_fwd_defer_kernel, attn_bwd_dq_pipe_kernel, attn_bwd_dkdv_pipe_kernel and
attn_bwd_dkdv_pair_kernel for the shorter default rows; attn_dkdv_sum_kernel for the cross
query split; the <float> instantiations for the fp32 case.
"""
import functools

import pytest
import torch

from conftest import record_metric

from oracle.fixtures import rel_l2, seeded

import _attn_rows as A
from _guarded import Guarded, assert_clean

pytestmark = pytest.mark.gpu
dev = "cuda"
bf16, f32 = torch.bfloat16, torch.float32
QPAD, KVPAD = 37, 5


def _st():
    return torch.cuda.current_stream().cuda_stream


# (B, C, heads, T, HW, mode, seed, amp, legacy, config)
def _self_cases():
    cs = [(2, C, 1, 3, 67, "joint", 90 + C, 1.0, True, "auto") for C in (32, 64, 128, 256)]
    for C in (32, 64, 128, 256):  # N >= 1024: the hand-scheduled forward and backward
        cs += [(1, C, 1, 1, 1157, "joint", 91 + C, 1.0, True, cfg) for cfg in ("auto", "base")]
    cs += [(2, 64, 1, 5, 130, "spatial", 95, 1.0, True, "auto"),
           (2, 64, 1, 40, 9, "temporal", 95, 1.0, True, "auto")]
    for B, C, heads, T, HW, mode, seed, amp, cfg in A.SELF_CASES:
        cs += [(B, C, heads, T, HW, mode, seed, amp, legacy, cfg)
               for legacy in ((True, False) if heads > 1 else (True,))]
    cs += [(2, 64, 1, T, 37, "temporal", 600 + T, 1.0, True, "auto") for T in (9, 17, 25)]
    out = []
    for c in cs:
        for layout in (("exact",) if c[5] == "temporal" else ("exact", "padded")):
            out.append(pytest.param(c, layout, id=A.case_id(c) + "-" + layout))
    return out


@functools.lru_cache(maxsize=2)
def _self_host(B, C, heads, T, HW, mode, seed, amp, legacy):
    qkv, g, host = A.self_inputs(B, C, T, HW, mode, seed, amp, heads, legacy)
    host.assert_cap()
    return qkv, g, host


def _self_run(B, C, heads, T, HW, mode, legacy, layout, dt, qkv, g, what, no_ws=False):
    """The launches of AttentionFn.forward / .backward on guarded buffers; returns the logical
    o [B, C, N], dqkv [B, 3C, N] (fp32, CPU) and lse in the reference's sequence order.
    no_ws: the forward is vd_attention_fwd, the form without a workspace, and the backward's
    path predicate vd_attention_bwd_short_path is asserted on the guarded pointers."""
    from vdiff import _lib, ops
    lib = _lib.lib()
    N, row, orow, es = T * HW, 3 * C, C, 2 if dt == bf16 else 4
    launches = ops._attn_desc(B, N, C, heads, C // heads, mode, (T, HW, 1), ops._DT[dt], legacy)
    d0 = launches[0][0]
    pad = QPAD if layout == "padded" else 0
    if mode == "temporal":
        assert pad == 0
        nb, L = B, N
    else:
        nb, L = d0.nseq // d0.groups, d0.seq_len
        assert nb * L == B * N and d0.batch_stride == L * row and d0.o_batch_stride == L * orow
    for d, *_ in launches:
        if pad:
            d.batch_stride = (L + pad) * row
            d.o_batch_stride = (L + pad) * orow
        short = lib.vd_attention_short_path(d)
        assert short == int(dt == bf16 and d.seq_len <= 32), (what, short)
    to_rows = lambda t, r: t.transpose(1, 2).reshape(nb, L, r)  # noqa: E731
    back = lambda G_, r: G_.payload().float().reshape(B, N, r).transpose(1, 2)  # noqa: E731

    QKV = Guarded.rows(nb, L, row, dt, dev, to_rows(qkv, row), pad, "qkv")
    O = Guarded.rows(nb, L, orow, dt, dev, None, pad, "o")
    LSE, WS = [], []
    for d, qo, ko, vo, oo in launches:
        lse = Guarded((d.nseq * d.seq_len,), f32, dev, name="lse")
        nws = 0 if no_ws else lib.vd_attention_fwd_workspace_size(d)
        ws = Guarded.workspace(nws, dev, "fwd workspace") if nws else None
        if no_ws:
            _lib.call("vd_attention_fwd", d, QKV.ptr + qo * es, QKV.ptr + ko * es,
                      QKV.ptr + vo * es, O.ptr + oo * es, lse.ptr, _st())
        else:
            _lib.call("vd_attention_fwd_ws", d, QKV.ptr + qo * es, QKV.ptr + ko * es,
                      QKV.ptr + vo * es, O.ptr + oo * es, lse.ptr, ws and ws.ptr, nws, _st())
        LSE.append(lse)
        if ws is not None:
            WS.append(ws)
    assert_clean([O] + LSE, [QKV], WS, what=what + " fwd")

    DOUT = Guarded.rows(nb, L, orow, dt, dev, to_rows(g, orow), pad, "dout")
    DQKV = Guarded.rows(nb, L, row, dt, dev, None, pad, "dqkv")
    DQKV2 = Guarded.rows(nb, L, row, dt, dev, None, pad, "dqkv (vd_attention_bwd)")
    O.freeze()
    WS, flash = [], False
    for (d, qo, ko, vo, oo), lse in zip(launches, LSE):
        lse.freeze()
        q, k, v = (QKV.ptr + o_ * es for o_ in (qo, ko, vo))
        o, do = O.ptr + oo * es, DOUT.ptr + oo * es
        dq, dk, dv = (DQKV.ptr + o_ * es for o_ in (qo, ko, vo))
        if no_ws:  # every guarded buffer is 16-B aligned: the shape alone decides; one
            # element off in any one buffer sends the call to the flash kernels
            assert lib.vd_attention_bwd_short_path(d, q, k, v, o, do, dq, dk, dv) == \
                lib.vd_attention_short_path(d), what
            ptrs = [q, k, v, o, do, dq, dk, dv]
            for i in range(len(ptrs)):
                off = ptrs[:i] + [ptrs[i] + es] + ptrs[i + 1:]
                assert lib.vd_attention_bwd_short_path(d, *off) == 0, (what, i)
        if lib.vd_attention_bwd_short_path(d, q, k, v, o, do, dq, dk, dv):
            _lib.call("vd_attention_bwd", d, q, k, v, o, do, lse.ptr, dq, dk, dv, None, _st())
            continue
        flash = True
        nws = lib.vd_attention_bwd_workspace_size(d)
        ws = Guarded.workspace(nws, dev, "bwd workspace")
        _lib.call("vd_attention_bwd_dq", d, q, k, v, o, do, lse.ptr, dq, ws.ptr, _st())
        _lib.call("vd_attention_bwd_dkdv", d, q, k, v, do, lse.ptr, dk, dv, ws.ptr, _st())
        ws2 = Guarded.workspace(nws, dev, "bwd workspace (vd_attention_bwd)")
        dq, dk, dv = (DQKV2.ptr + o_ * es for o_ in (qo, ko, vo))
        _lib.call("vd_attention_bwd", d, q, k, v, o, do, lse.ptr, dq, dk, dv, ws2.ptr, _st())
        WS += [ws, ws2]
    assert_clean([DQKV] + ([DQKV2] if flash else []), [QKV, O, DOUT] + LSE, WS,
                 what=what + " bwd")
    if flash:
        assert torch.equal(DQKV.raw, DQKV2.raw), what + ": vd_attention_bwd != _dq + _dkdv"
    if mode == "temporal":  # one launch per head over (b, p) sequences -> (b, p, h)
        lse = torch.stack([l_.payload() for l_ in LSE]).reshape(heads, B * HW, T).transpose(0, 1)
    else:
        lse = LSE[0].payload()
    return back(O, orow), back(DQKV, row), lse


@pytest.mark.parametrize("case,layout", _self_cases())
def test_guarded_self_attention(case, layout):
    """vd_attention_fwd_ws, vd_attention_bwd_dq / _dkdv and vd_attention_bwd (module docstring).
    Measured on an MI355X, kernel / emulation at most: O 1.50 x (head_dim 128 at N = 1157), dQ
    1.06 x, dK 1.10 x, dV 1.00 x, lse 0.28 of its bound, in both layouts: the figures of the
    unguarded tests of the same cases."""
    from vdiff import ops
    B, C, heads, T, HW, mode, seed, amp, legacy, cfg = case
    qkv, g, host = _self_host(B, C, heads, T, HW, mode, seed, amp, legacy)
    what = f"guarded attention {A.case_id(case)} {layout}"
    with ops.attention_config(cfg):
        o, dqkv, lse = _self_run(B, C, heads, T, HW, mode, legacy, layout, bf16, qkv, g, what)
    got = dict(zip(("dq", "dk", "dv"), A.sequences(dqkv, C, T, HW, mode, heads, legacy)))
    got["o"], = A.sequences(o, C, T, HW, mode, heads, legacy)
    host.judge(got, lse, what, record_metric, test="guarded_attention", case=A.case_id(case),
               layout=layout)


def _no_ws_cases():
    """Joint at every head_dim, spatial, temporal (flash and, T <= 32, the short kernels) and one
    1157-token row (the hand-scheduled forward): cases of _self_cases, same tuples and seeds."""
    cs = [(2, C, 1, 3, 67, "joint", 90 + C, 1.0, True, "auto") for C in (32, 64, 128, 256)]
    cs += [(1, 64, 1, 1, 1157, "joint", 91 + 64, 1.0, True, "auto"),
           (2, 64, 1, 5, 130, "spatial", 95, 1.0, True, "auto"),
           (2, 64, 1, 40, 9, "temporal", 95, 1.0, True, "auto")]
    cs += [(2, 64, 1, T, 37, "temporal", 600 + T, 1.0, True, "auto") for T in (9, 25)]
    return [pytest.param(c, layout, id=A.case_id(c) + "-" + layout) for c in cs
            for layout in (("exact",) if c[5] == "temporal" else ("exact", "padded"))]


@pytest.mark.parametrize("case,layout", _no_ws_cases())
def test_guarded_attention_fwd_without_workspace(case, layout):
    """vd_attention_fwd, the entry point without a workspace, in place of vd_attention_fwd_ws, and
    vd_attention_bwd_short_path on the guarded pointers (1 exactly for the short shapes, 0 as soon
    as one buffer is an element off 16-byte alignment); the backward and the judgement are those
    of test_guarded_self_attention."""
    from vdiff import ops
    B, C, heads, T, HW, mode, seed, amp, legacy, cfg = case
    qkv, g, host = _self_host(B, C, heads, T, HW, mode, seed, amp, legacy)
    what = f"guarded attention_fwd {A.case_id(case)} {layout}"
    with ops.attention_config(cfg):
        o, dqkv, lse = _self_run(B, C, heads, T, HW, mode, legacy, layout, bf16, qkv, g, what,
                                 no_ws=True)
    got = dict(zip(("dq", "dk", "dv"), A.sequences(dqkv, C, T, HW, mode, heads, legacy)))
    got["o"], = A.sequences(o, C, T, HW, mode, heads, legacy)
    host.judge(got, lse, what, record_metric, test="guarded_attention_fwd", case=A.case_id(case),
               layout=layout)


@pytest.mark.parametrize("layout", ["exact", "padded"])
def test_guarded_self_attention_fp32(layout):
    """(2, 64, 3, 67, "joint") in fp32 (the generic kernels' fp32 instantiation) against the fp64
    reference without emulation, at the fp32 bar of test_joint_head_dims, 2e-5 rel-L2, for each of
    O, dQ, dK, dV; lse inside the bound of _attn_rows.  Measured: O 4.1e-7, dQ, dK, dV 1.1e-6."""
    B, C, T, HW, mode = 2, 64, 3, 67, "joint"
    qkv, g = seeded((B, 3 * C, T * HW), 90 + C), seeded((B, C, T * HW), 91 + C)
    q, k, v = A.sequences(qkv, C, T, HW, mode)
    do, = A.sequences(g, C, T, HW, mode)
    ref, lse_ref, smax = A.reference(q, k, v, do, False)
    what = f"guarded attention fp32 {layout}"
    o, dqkv, lse = _self_run(B, C, 1, T, HW, mode, True, layout, f32, qkv, g, what)
    got = dict(zip(("dq", "dk", "dv"), A.sequences(dqkv, C, T, HW, mode)))
    got["o"], = A.sequences(o, C, T, HW, mode)
    errs = {n: rel_l2(got[n], ref[n]) for n in A.NAMES}
    print(what, errs)
    for n in A.NAMES:
        assert errs[n] < 2e-5, errs
    lse_err = (lse.double().reshape(lse_ref.shape) - lse_ref).abs()
    assert bool((lse_err <= 2.0 ** -8 * smax + 1e-5).all())


# ------------------------------------------------------------------ cross-attention
def _cross_cases():
    return [pytest.param(c, layout, id=A.case_id(c) + "-" + layout)
            for c in A.CROSS_CASES for layout in ("exact", "padded")]


@functools.lru_cache(maxsize=2)
def _cross_host(case):
    q, kv, g, host = A.cross_inputs(*case)
    host.assert_cap()
    return q, kv, g, host


@pytest.mark.parametrize("case,layout", _cross_cases())
def test_guarded_cross_attention(case, layout):
    """vd_cross_attention_fwd, _bwd_dq and _bwd_dkdv as CrossAttentionFn calls them.  Measured on
    an MI355X, kernel / emulation at most: O 1.02 x, dQ, dK, dV 1.00 x, lse 0.54 of its bound, in
    both layouts."""
    from vdiff import _lib, ops
    lib = _lib.lib()
    B, C, heads, T, HW, L, per_frame, seed, amp = case
    q, kv, g, host = _cross_host(case)
    what = f"guarded cross-attention {A.case_id(case)} {layout}"
    x = ops._xattn_desc(B, T, HW, C, heads, L, _lib.VD_BF16, per_frame)
    nb, Lq, Lk = x.q.nseq // x.q.groups, x.q.seq_len, x.kv_len
    assert nb * Lq == B * T * HW and nb * Lk == B * T * L
    assert x.q.batch_stride == Lq * C and x.kv_batch_stride == Lk * 2 * C
    qp, kp = (QPAD, KVPAD) if layout == "padded" else (0, 0)
    x.q.batch_stride = x.q.o_batch_stride = (Lq + qp) * C
    x.kv_batch_stride = (Lk + kp) * 2 * C
    Q = Guarded.rows(nb, Lq, C, bf16, dev, q.transpose(1, 2).reshape(nb, Lq, C), qp, "q")
    KV = Guarded.rows(nb, Lk, 2 * C, bf16, dev, kv.reshape(nb, Lk, 2 * C), kp, "kv")
    O = Guarded.rows(nb, Lq, C, bf16, dev, None, qp, "o")
    LSE = Guarded((x.q.nseq * Lq,), f32, dev, name="lse")
    nws = lib.vd_cross_attention_fwd_workspace_size(x)
    WS = Guarded.workspace(nws, dev, "fwd workspace")
    _lib.call("vd_cross_attention_fwd", x, Q.ptr, KV.ptr, KV.ptr + C * 2, O.ptr, LSE.ptr, WS.ptr,
              nws, _st())
    assert_clean([O, LSE], [Q, KV], [WS], what=what + " fwd")

    DOUT = Guarded.rows(nb, Lq, C, bf16, dev, g.transpose(1, 2).reshape(nb, Lq, C), qp, "dout")
    DQ = Guarded.rows(nb, Lq, C, bf16, dev, None, qp, "dq")
    DKV = Guarded.rows(nb, Lk, 2 * C, bf16, dev, None, kp, "dkv")
    WS2 = Guarded.workspace(lib.vd_cross_attention_bwd_workspace_size(x), dev, "bwd workspace")
    O.freeze(), LSE.freeze()
    _lib.call("vd_cross_attention_bwd_dq", x, Q.ptr, KV.ptr, KV.ptr + C * 2, O.ptr, DOUT.ptr,
              LSE.ptr, DQ.ptr, WS2.ptr, _st())
    _lib.call("vd_cross_attention_bwd_dkdv", x, Q.ptr, KV.ptr, KV.ptr + C * 2, DOUT.ptr, LSE.ptr,
              DKV.ptr, DKV.ptr + C * 2, WS2.ptr, _st())
    assert_clean([DQ, DKV], [Q, KV, O, DOUT, LSE], [WS2], what=what + " bwd")

    back = lambda G_: G_.payload().float().reshape(B, T * HW, C).transpose(1, 2)  # noqa: E731
    got = dict(o=A.cross_q_sequences(back(O), heads, T, per_frame),
               dq=A.cross_q_sequences(back(DQ), heads, T, per_frame))
    got["dk"], got["dv"] = A.cross_kv_sequences(DKV.payload().float().reshape(B * T, L, 2 * C),
                                                heads, T, per_frame)
    host.judge(got, LSE.payload(), what, record_metric, test="guarded_cross_attention",
               case=A.case_id(case), layout=layout)
