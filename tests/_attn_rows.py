"""Per-row, per-output attention checks (single head): O, dQ, dK, dV and lse of the bf16 kernels
against an fp64 reference on the same bf16-rounded operands.

For each of O, dQ, dK, dV and every token row: ||got_row - ref_row|| / max(||ref_row||, median
row norm); the test asserts on the maximum over the rows.  The whole-tensor rel-L2 of the
concatenated d(qkv) is dominated by dV and dilutes one wrong row among thousands; this does not.

The limit is 4 x the same statistic of a CPU emulation of bf16 attention against fp64: the
fp64 math with the kernels' documented roundings (q scale log2(e) -- k for dK / dV -- rounded to
bf16, P and dS rounded to bf16 as MFMA operands, delta from the stored bf16 O, outputs rounded to
bf16; tests/test_gpu_fullsize.py `_prescale`, `_reference(rounded=True)`).  The kernels'
summation order, exp2 approximation and lagged-max rescale are not emulated, each an effect of
the same size: hence the factor 4.

lse: |lse - lse_ref| <= 2^-8 max_j |s_ij| + 1e-5 per row (the bf16-rounded score operand moves
every score of the row by at most 2^-8 of its size).
"""
import math

import torch

LOG2E = 1.4426950408889634


def _bf(t):
    return t.float().bfloat16().double()


def sequences(t, C, T, HW, mode):
    """[B, n*C, T*HW] (channels-first, token n = t * HW + p) -> n tensors [nseq, L, C]."""
    B, nC, N = t.shape
    t = t.double().reshape(B, nC // C, C, T, HW)
    if mode == "joint":
        s = t.permute(0, 1, 3, 4, 2).reshape(B, nC // C, N, C)
    elif mode == "spatial":
        s = t.permute(0, 3, 1, 4, 2).reshape(B * T, nC // C, HW, C)
    else:  # temporal: one sequence per pixel
        s = t.permute(0, 4, 1, 3, 2).reshape(B * HW, nC // C, T, C)
    return s.unbind(1)


def reference(q, k, v, do, emulate):
    """O, lse (natural log), dQ, dK, dV and max_j |s_ij| in fp64 for [nseq, L, C] operands;
    emulate=True applies the bf16 kernels' roundings."""
    C = q.shape[-1]
    scale = 1.0 / math.sqrt(C)
    r = _bf if emulate else (lambda t: t)
    c = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)) \
        if emulate else scale * LOG2E
    qs, ks = r(q * c), r(k * c)
    s2 = qs @ k.transpose(1, 2)                     # log2 units
    m = s2.amax(-1, keepdim=True)
    p = torch.exp2(s2 - m)
    l = p.sum(-1, keepdim=True)
    o = r((r(p) @ v) / l)
    lse2 = m + torch.log2(l)
    delta = (do * o).sum(-1, keepdim=True)
    p = torch.exp2(s2 - lse2)
    ds = r(p * (do @ v.transpose(1, 2) - delta))
    dq = r((ds @ k) * scale)
    pc = torch.exp2(q @ ks.transpose(1, 2) - lse2)  # the dK / dV kernel scales k
    dv = r(r(pc).transpose(1, 2) @ do)
    dsc = r(pc * (do @ v.transpose(1, 2) - delta))
    dk = r((dsc.transpose(1, 2) @ q) * scale)
    smax = (s2 / LOG2E).abs().amax(-1)
    return dict(o=o, dq=dq, dk=dk, dv=dv), (lse2 / LOG2E).squeeze(-1), smax


def row_stat(got, ref):
    """max over token rows of ||got - ref|| / max(||ref||, median row norm)."""
    got, ref = got.double().reshape(-1, ref.shape[-1]), ref.reshape(-1, ref.shape[-1])
    n = ref.norm(dim=1)
    return float(((got - ref).norm(dim=1) / torch.maximum(n, n.median())).max())


def check(B, C, T, HW, mode, seed, record=None, amp=1.0):
    """Runs ops.attention (heads = 1, bf16) forward and backward, and the forward launch once
    more for its lse; returns {name: (kernel statistic, emulated statistic)}."""
    from oracle.fixtures import seeded
    from vdiff import _lib, ops
    dev = "cuda"
    N = T * HW
    qkv = (seeded((B, 3 * C, N), seed) * amp).bfloat16()
    g = seeded((B, C, N), seed + 1).bfloat16()
    q, k, v = sequences(qkv, C, T, HW, mode)
    do, = sequences(g, C, T, HW, mode)
    ref, lse_ref, smax = reference(q, k, v, do, False)
    emu, lse_emu, _ = reference(q, k, v, do, True)

    qd = ops.to_cl(qkv.to(dev)).requires_grad_(True)
    out = ops.attention(qd, heads=1, mode=mode, spatial=(T, HW, 1), legacy=True)
    out.backward(ops.to_cl(g.to(dev)))
    (d, qo, ko, vo, oo), = ops._attn_desc(B, N, C, 1, C, mode, (T, HW, 1), _lib.VD_BF16, True)
    x = qd.detach()
    o2 = ops.empty_cl([B, C, N], torch.bfloat16, dev)
    lse = torch.empty(d.nseq * d.seq_len, dtype=torch.float32, device=dev)
    nws = _lib.lib().vd_attention_fwd_workspace_size(d)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
    base = x.data_ptr()
    _lib.call("vd_attention_fwd_ws", d, base + qo * 2, base + ko * 2, base + vo * 2,
              o2.data_ptr(), lse.data_ptr(), None if ws is None else ws.data_ptr(), nws,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()

    got = dict(zip(("dq", "dk", "dv"), sequences(qd.grad.float().cpu(), C, T, HW, mode)))
    got["o"], = sequences(out.detach().float().cpu(), C, T, HW, mode)
    res = {}
    for name in ("o", "dq", "dk", "dv"):
        res[name] = (row_stat(got[name], ref[name]), row_stat(emu[name], ref[name]))
    lse_err = (lse.cpu().double().reshape(lse_ref.shape) - lse_ref).abs()
    lse_bound = 2.0 ** -8 * smax + 1e-5
    res["lse"] = (float((lse_err / lse_bound).max()),
                  float(((lse_emu - lse_ref).abs() / lse_bound).max()))
    print(f"attention rows B={B} C={C} T={T} HW={HW} {mode}: " +
          " ".join(f"{k_} {a:.3g}/{b:.3g}" for k_, (a, b) in res.items()))
    if record is not None:
        record(test="attention_rows", B=B, C=C, T=T, HW=HW, mode=mode,
               **{k_: a for k_, (a, b) in res.items()},
               **{"emu_" + k_: b for k_, (a, b) in res.items()})
    for name in ("o", "dq", "dk", "dv"):
        a, b = res[name]
        assert a <= 4 * b, (name, a, b, res)
    assert res["lse"][0] <= 1.0, res
    return res
