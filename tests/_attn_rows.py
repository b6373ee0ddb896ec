"""Per-row, per-output attention checks: O, dQ, dK, dV and lse of the bf16 kernels against an
fp64 reference on the same bf16-rounded operands.  Self-attention (one or several heads, both
qkv channel orders, all three token groupings) and audio cross-attention (per frame or over the
whole clip).

For each of O, dQ, dK, dV and every token row: ||got_row - ref_row|| / max(||ref_row||, median
row norm); the test asserts on the maximum over the rows.  The whole-tensor rel-L2 of the
concatenated d(qkv) is dominated by dV and dilutes one wrong row among thousands; this does not.

The limit is 4 x the same statistic of a CPU emulation of bf16 attention against fp64: the
fp64 math with the kernels' documented roundings (q scale log2(e) -- k for dK / dV -- rounded to
bf16, P and dS rounded to bf16 as MFMA operands, delta from the stored bf16 O, outputs rounded to
bf16; tests/test_gpu_fullsize.py `_prescale`, `_reference(rounded=True)`).  The kernels'
summation order, exp2 approximation and lagged-max rescale are not emulated, each an effect of
the same size: hence the factor 4.

Cross-attention runs on the generic 4-wave kernels (attention.hip: attn_fwd_kernel,
attn_bwd_dq_kernel, attn_bwd_dkdv_kernel with a KvAddr of their own) and rounds at the same
places: RowFrag::scale rounds q scale log2(e) in the forward and in dQ, and k scale log2(e) in
dK / dV; XOp rounds P and dS; attn_delta_kernel reads the stored bf16 O; store_transposed /
store8 round each output once.  Under the key split (forward, dQ) and the query split (dK / dV)
the partials are fp32 and their sum is rounded once (attn_fwd_combine_kernel,
attn_dq_sum_kernel, attn_dkdv_sum_kernel), which is what one rounding of the fp64 sum emulates.
So `reference(emulate=True)` serves the cross path unchanged.

lse: |lse - lse_ref| <= 2^-8 max_j |s_ij| + 1e-5 per row (the bf16-rounded score operand moves
every score of the row by at most 2^-8 of its size).

Condition on every case (CAP): the emulation's own statistic is at most 1.5e-2 for every output
and its lse error at most 1.0 of the bound, so that a loose reference cannot hide a kernel
failure behind the factor 4.  `assert_cap` checks it before the kernel runs;
tests/test_bounds_host.py checks it for every GPU case on the CPU.
"""
import math

import torch

LOG2E = 1.4426950408889634
CAP = 1.5e-2
NAMES = ("o", "dq", "dk", "dv")


def _bf(t):
    return t.float().bfloat16().double()


def sequences(t, C, T, HW, mode, heads=1, legacy=True):
    """[B, n*C, T*HW] (channels-first, token n = t * HW + p) -> n tensors [nseq, L, C / heads].
    n = 3 (qkv): channel order [h][q|k|v][ch] (legacy) or [q|k|v][h][ch]; n = 1: [h][ch].
    Sequence order: (b, h) joint, (b, t, h) spatial, (b, p, h) temporal."""
    B, nC, N = t.shape
    n, ch = nC // C, C // heads
    t = t.double()
    if legacy:
        t = t.reshape(B, heads, n, ch, T, HW)
    else:
        t = t.reshape(B, n, heads, ch, T, HW).transpose(1, 2)
    # [B, heads, n, ch, T, HW]
    if mode == "joint":
        s = t.permute(0, 1, 2, 4, 5, 3).reshape(B * heads, n, N, ch)
    elif mode == "spatial":
        s = t.permute(0, 4, 1, 2, 5, 3).reshape(B * T * heads, n, HW, ch)
    else:  # temporal: one sequence per pixel
        s = t.permute(0, 5, 1, 2, 4, 3).reshape(B * HW * heads, n, T, ch)
    return s.unbind(1)


def cross_q_sequences(t, heads, T, per_frame):
    """Video-side tensor (q, O, dO, dQ) [B, C, T*HW], channels [h][ch] -> [nseq, Lq, ch]:
    per frame sequence (b, t, h) holds the HW tokens of frame t, else (b, h) all T*HW tokens."""
    B, C, N = t.shape
    ch, HW = C // heads, N // T
    t = t.double().reshape(B, heads, ch, T, HW)
    if per_frame:
        return t.permute(0, 3, 1, 4, 2).reshape(B * T * heads, HW, ch)
    return t.permute(0, 1, 3, 4, 2).reshape(B * heads, N, ch)


def cross_kv_sequences(kv, heads, T, per_frame):
    """Audio-side tensor (kv, dkv) [B*T, L, 2C] (k | v channel halves, head h at h*ch of each
    half) -> k, v [nseq, Lk, ch]: per frame the L rows of kv[b*T + t], else the T*L rows of
    kv[b*T : (b+1)*T] in order."""
    BT, L, C2 = kv.shape
    C = C2 // 2
    ch, B = C // heads, BT // T
    t = kv.double().reshape(BT, L, 2, heads, ch)
    if per_frame:
        s = t.permute(2, 0, 3, 1, 4).reshape(2, BT * heads, L, ch)
    else:
        s = t.reshape(B, T * L, 2, heads, ch).permute(2, 0, 3, 1, 4)
        s = s.reshape(2, B * heads, T * L, ch)
    return s[0], s[1]


def reference(q, k, v, do, emulate):
    """O, lse (natural log), dQ, dK, dV and max_j |s_ij| in fp64 for q, do [nseq, Lq, C] and
    k, v [nseq, Lk, C]; emulate=True applies the bf16 kernels' roundings."""
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


class Host:
    """The fp64 reference of one case, its bf16 emulation and the emulation's statistics."""

    def __init__(self, q, k, v, do):
        self.q, self.k, self.v, self.do = q, k, v, do
        self.ref, self.lse_ref, self.smax = reference(q, k, v, do, False)
        self.emu, self.lse_emu, _ = reference(q, k, v, do, True)
        self.lse_bound = 2.0 ** -8 * self.smax + 1e-5
        self.emu_stat = {n: row_stat(self.emu[n], self.ref[n]) for n in NAMES}
        self.emu_stat["lse"] = float(((self.lse_emu - self.lse_ref).abs() / self.lse_bound).max())

    def assert_cap(self):
        for n in NAMES:
            assert self.emu_stat[n] <= CAP, (n, self.emu_stat)
        assert self.emu_stat["lse"] <= 1.0, self.emu_stat

    def judge(self, got, lse, what, record, **fields):
        """got: {name: [nseq, L, ch]}, lse in the reference's sequence order.  Prints and
        records kernel / emulation, then asserts the limits."""
        res = {n: (row_stat(got[n], self.ref[n]), self.emu_stat[n]) for n in NAMES}
        lse_err = (lse.cpu().double().reshape(self.lse_ref.shape) - self.lse_ref).abs()
        res["lse"] = (float((lse_err / self.lse_bound).max()), self.emu_stat["lse"])
        print(f"{what}: " + " ".join(f"{k_} {a:.3g}/{b:.3g}" for k_, (a, b) in res.items()))
        if record is not None:
            record(**fields, **{k_: a for k_, (a, b) in res.items()},
                   **{"emu_" + k_: b for k_, (a, b) in res.items()})
        for name in NAMES:
            a, b = res[name]
            assert a <= 4 * b, (name, a, b, res)
        assert res["lse"][0] <= 1.0, res
        return res


def self_inputs(B, C, T, HW, mode, seed, amp=1.0, heads=1, legacy=True):
    """bf16 qkv [B, 3C, T*HW] and dO [B, C, T*HW] of a self-attention case, and its Host."""
    from oracle.fixtures import seeded
    N = T * HW
    qkv = (seeded((B, 3 * C, N), seed) * amp).bfloat16()
    g = seeded((B, C, N), seed + 1).bfloat16()
    q, k, v = sequences(qkv, C, T, HW, mode, heads, legacy)
    do, = sequences(g, C, T, HW, mode, heads, legacy)
    return qkv, g, Host(q, k, v, do)


def cross_inputs(B, C, heads, T, HW, L, per_frame, seed, amp=1.0):
    """bf16 q [B, C, T*HW], kv [B*T, L, 2C] and dO [B, C, T*HW] of a cross-attention case, and
    its Host."""
    from oracle.fixtures import seeded
    q = (seeded((B, C, T * HW), seed) * amp).bfloat16()
    kv = (seeded((B * T, L, 2 * C), seed + 1) * amp).bfloat16()
    g = seeded((B, C, T * HW), seed + 2).bfloat16()
    k, v = cross_kv_sequences(kv, heads, T, per_frame)
    return q, kv, g, Host(cross_q_sequences(q, heads, T, per_frame), k, v,
                          cross_q_sequences(g, heads, T, per_frame))


def check(B, C, T, HW, mode, seed, record=None, amp=1.0, heads=1, legacy=True):
    """Runs ops.attention (bf16) forward and backward, and the forward launches once more for
    their lse; returns {name: (kernel statistic, emulated statistic)}."""
    from vdiff import _lib, ops
    dev = "cuda"
    N = T * HW
    qkv, g, host = self_inputs(B, C, T, HW, mode, seed, amp, heads, legacy)
    host.assert_cap()

    qd = ops.to_cl(qkv.to(dev)).requires_grad_(True)
    out = ops.attention(qd, heads=heads, mode=mode, spatial=(T, HW, 1), legacy=legacy)
    out.backward(ops.to_cl(g.to(dev)))
    x = qd.detach()
    o2 = ops.empty_cl([B, C, N], torch.bfloat16, dev)
    base, lses = x.data_ptr(), []
    for d, qo, ko, vo, oo in ops._attn_desc(B, N, C, heads, C // heads, mode, (T, HW, 1),
                                            _lib.VD_BF16, legacy):
        lse = torch.empty(d.nseq * d.seq_len, dtype=torch.float32, device=dev)
        nws = _lib.lib().vd_attention_fwd_workspace_size(d)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
        _lib.call("vd_attention_fwd_ws", d, base + qo * 2, base + ko * 2, base + vo * 2,
                  o2.data_ptr() + oo * 2, lse.data_ptr(), None if ws is None else ws.data_ptr(),
                  nws, torch.cuda.current_stream().cuda_stream)
        lses.append(lse)
    torch.cuda.synchronize()
    if mode == "temporal":  # one launch per head over (b, p) sequences -> (b, p, h)
        lse = torch.stack(lses).reshape(heads, B * HW, T).transpose(0, 1)
    else:
        lse, = lses

    got = dict(zip(("dq", "dk", "dv"),
                   sequences(qd.grad.float().cpu(), C, T, HW, mode, heads, legacy)))
    got["o"], = sequences(out.detach().float().cpu(), C, T, HW, mode, heads, legacy)
    extra = dict(heads=heads, legacy=legacy) if heads > 1 else {}
    return host.judge(got, lse, f"attention rows B={B} C={C} T={T} HW={HW} {mode} heads={heads}"
                      f" legacy={legacy} amp={amp}", record, test="attention_rows", B=B, C=C, T=T,
                      HW=HW, mode=mode, **extra)


def check_cross(B, C, heads, T, HW, L, per_frame, seed, record=None, amp=1.0):
    """Runs ops.cross_attention (bf16) forward and backward, and the forward launch once more
    for its lse; returns {name: (kernel statistic, emulated statistic)}."""
    from vdiff import _lib, ops
    dev = "cuda"
    q, kv, g, host = cross_inputs(B, C, heads, T, HW, L, per_frame, seed, amp)
    host.assert_cap()

    qd = ops.to_cl(q.to(dev)).requires_grad_(True)
    kvd = kv.to(dev).requires_grad_(True)
    out = ops.cross_attention(qd, kvd, heads, T, per_frame)
    out.backward(ops.to_cl(g.to(dev)))
    x = ops._xattn_desc(B, T, HW, C, heads, L, _lib.VD_BF16, per_frame)
    qx, kx = qd.detach(), kvd.detach()
    o2 = ops.empty_cl([B, C, T * HW], torch.bfloat16, dev)
    lse = torch.empty(x.q.nseq * x.q.seq_len, dtype=torch.float32, device=dev)
    nws = _lib.lib().vd_cross_attention_fwd_workspace_size(x)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)
    _lib.call("vd_cross_attention_fwd", x, qx.data_ptr(), kx.data_ptr(), kx.data_ptr() + C * 2,
              o2.data_ptr(), lse.data_ptr(), ws.data_ptr(), nws,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(o2, out.detach())  # the second launch is the first one again

    got = dict(o=cross_q_sequences(out.detach().float().cpu(), heads, T, per_frame),
               dq=cross_q_sequences(qd.grad.float().cpu(), heads, T, per_frame))
    got["dk"], got["dv"] = cross_kv_sequences(kvd.grad.float().cpu(), heads, T, per_frame)
    return host.judge(got, lse, f"cross-attention rows B={B} C={C} heads={heads} T={T} HW={HW} "
                      f"L={L} per_frame={per_frame} amp={amp}", record,
                      test="cross_attention_rows", B=B, C=C, heads=heads, T=T, HW=HW, L=L,
                      per_frame=per_frame, amp=amp)


# ------------------------------------------------------------------ the GPU cases
# (B, C, heads, T, HW, L, per_frame, seed, amp)
CROSS_CASES = [(2, C, 1, 3, 67, 12, True, 400 + C, 1.0) for C in (32, 64, 128, 256)] + [
    (1, 64, 1, 1, 3000, 12, True, 410, 1.0),   # key grid too small: the query split
    (1, 64, 1, 2, 700, 150, True, 411, 1.0),   # two key tiles and a ragged one
    (1, 64, 1, 1, 130, 64, True, 412, 1.0),    # exactly one key tile
    (1, 64, 1, 1, 130, 65, True, 413, 1.0),    # one key past it
    (1, 128, 4, 2, 50, 7, True, 414, 1.0),
    (2, 128, 2, 4, 36, 12, False, 415, 1.0),   # clip level
    (2, 64, 1, 3, 67, 12, True, 425, 1.5),     # a moderately peaked softmax (*)
]
# (B, C, heads, T, HW, mode, seed, amp, config); each runs with legacy True and False when
# heads > 1
SELF_CASES = [
    (2, 128, 2, 1, 300, "joint", 420, 1.0, "auto"),
    (2, 128, 2, 1, 300, "joint", 420, 1.0, "base"),
    (2, 128, 2, 3, 70, "spatial", 421, 1.0, "auto"),
    (1, 128, 4, 40, 9, "temporal", 422, 1.0, "auto"),  # T > 32: the flash kernels
    (2, 64, 1, 3, 67, "joint", 435, 1.5, "auto"),  # (*)
]
# (*) at amp = 1.5 the emulation's statistic is 0.9e-2 - 2.3e-2 depending on the seed; these
# seeds were taken from the emulation on the CPU (1.37e-2 and 1.21e-2), before any kernel ran.


# Ring-depth cases of tests/test_gpu_ring_determinism.py: sequences of 64 and 79 key tiles (5000:
# a ragged last tile and a tile count that is no multiple of the 4 ring stages), so that the
# stage-unrolled ring loops run many rounds on a grid of many workgroups.
# (B, C, heads, T, HW, mode, seed, amp); the head-dim-32 row runs with legacy True and False.
# The seeds were checked against CAP with the emulation on the CPU before any kernel ran
# (tests/test_bounds_host.py).
RING_SELF_CASES = [(1, C, 1, 1, N, "joint", 500 + C + N, 1.0)
                   for N in (4096, 5000) for C in (64, 128)] + [
    (1, 128, 4, 1, 4096, "joint", 540, 1.0),   # head dim 32: the generic kernels
]
# (B, C, heads, T, HW, L, per_frame, seed, amp): clip level, 16 * 40 = 640 keys = 10 key tiles
RING_CROSS_CASES = [(1, 64, 1, 16, 1024, 40, False, 550, 1.0)]


def case_id(c):
    return "-".join(str(v) for v in c)
