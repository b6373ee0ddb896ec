"""Head_dim-64 attention, hand-scheduled forward + backward (config "asm"), against a
materialised fp64 reference of softmax(Q K^T / sqrt 64) V and its autograd, element by element.

Shapes: the smallest at which each path of the backward kernels exists -- N = 1024 (one
workgroup per role, the 4 ring stages exactly once), 1280 (the tail after a partial turn of the
ring), 1500 (ragged last tile, zero-filled keys and queries), B = 2 x N = 3000 (sequences on
grid.z), spatial (4, 32, 32) (groups on grid.y), and N = 1500 with Q x 8 (P spans many binades
inside a tile).  Inputs as tests/test_gpu_attention_asm.py `_inputs` (randn * 1.3, seeded).

The bound of every output element is derived, not tuned: |got - ref| <= |emu - ref| + R.
ref is the fp64 result on the bf16 inputs.  emu is the same fp64 math with the kernels'
documented, deterministic roundings (tests/_attn_rows.py `reference(emulate=True)`: Q c or K c
rounded to bf16, c = log2(e) / 8 in fp32; P and dS rounded to bf16 as MFMA operands; delta from
the bf16 O; outputs rounded to bf16), so |emu - ref| is known exactly, element by element.  R
bounds what the emulation leaves out -- fp32 summation order, v_exp_f32, and bf16 roundings that
fall the other way because of those (the forward also rounds P relative to a lagged maximum
that is not emulated) -- in the worst case, with u = 2^-8 (tests/_bounds.py U_BF16), a_qj =
c sum_i |q_i| |k_ji| and P, T = dP - delta, dS = P T of the reference:
 * exponent (log2 units): x_qj = 2 (64 + 2) 2^-24 a_qj (the 64-term fp32 sum) + the forward's
   lse': 2 (L + 2) 2^-24 log2 e (row sum) + 2 (64 + 2) 2^-24 max_j a_qj + 2^-22 |lse'| (the
   conversion to -lse' log2 e) + 2^-22 a_qj (the fp32 scale constant) + 2^-22 (v_exp_f32);
   r = 2^x - 1.  The rounded operand bf16(P) moves by at most P (r + u (1 + r)) =: P e.
   (P of the kernels is at most P_ref 2^(u (a_qj + max_j a_qj)) =: Pu, the pre-scaled operand's
   rounding; Pu stands for P below.)
 * O:  R_O = sum_j Pu e |v_jd| + 2 (L + 2) 2^-24 |O| (row sum l), + the fp32 sum and the output
   rounding, _bounds.bound(O, sum_j Pu |v_jd|, L, bf16).
 * T:  eta_q = 2 (64 + 2) 2^-24 (sum_d |dO| |v| + sum_d |dO| |O|) + sum_d |dO_qd| R_O[q, d].
 * dS = bf16(P T):  E = Pu (r |T| + (1 + r) eta) + u Pu (1 + r) (|T| + eta).
 * dQ, dK, dV:  R = sum_j E |k_jd| / 8,  sum_q E |q_qd| / 8,  sum_q Pu e |dO_qd|,  each + the
   fp32 sum of L products and the output rounding, _bounds.bound(ref, mag, L, bf16).
"""
import functools
import math

import pytest
import torch

import _attn_rows
import _bounds

pytestmark = pytest.mark.gpu
dev = "cuda"
C = 64
U = _bounds.U_BF16
LOG2E = 1.4426950408889634

# (B, N, spatial, seed, q_amp)
CASES = [(1, 1024, None, 20, 1.0), (1, 1280, None, 21, 1.0), (1, 1500, None, 22, 1.0),
         (2, 3000, None, 23, 1.0), (1, None, (4, 32, 32), 24, 1.0), (1, 1500, None, 25, 8.0)]
IDS = ["n1024", "n1280", "n1500", "b2-n3000", "spatial-4x32x32", "n1500-q8"]


def _inputs(B, N, seed, spatial=None, q_amp=1.0):
    from vdiff import ops
    gen = torch.Generator(device=dev).manual_seed(seed)
    shape = (B, 3 * C, N if spatial is None else math.prod(spatial))
    qkv = torch.randn(shape, generator=gen, device=dev) * 1.3
    qkv[:, :C] *= q_amp
    gout = torch.randn((B, C, shape[2]), generator=gen, device=dev)
    return ops.to_cl(qkv.bfloat16()), ops.to_cl(gout.bfloat16())


def _run(qkv, g, **kw):
    from vdiff import ops
    x = qkv.detach().clone().requires_grad_(True)
    with ops.attention_config("asm"):
        y = ops.attention(x, 1, **kw)
        y.backward(g)
    torch.cuda.synchronize()
    return y.detach(), x.grad.detach()


def _sequence_bounds(q, k, v, do):
    """q, k, v, do [L, 64] fp64 (bf16 values) -> {name: (ref, bound)} for o, dq, dk, dv."""
    L = q.shape[0]
    emu, _, _ = _attn_rows.reference(q[None], k[None], v[None], do[None], True)
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = (q @ k.T) / math.sqrt(C)
    P = torch.softmax(s, -1)
    o = P @ v
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
    with torch.no_grad():
        P, o = P.detach(), o.detach()
        qa, ka, va, da, oa = q.abs(), k.abs(), v.abs(), do.abs(), o.abs()
        f32, acc = _bounds.U_FP32, 2 * (C + 2) * _bounds.U_FP32
        a = LOG2E / math.sqrt(C) * (qa @ ka.T)
        amax = a.amax(-1, keepdim=True)
        lse2 = torch.logsumexp(s, -1, keepdim=True).abs() * LOG2E
        x = acc * a + 2 * (L + 2) * f32 * LOG2E + acc * amax + 4 * f32 * (lse2 + a) + 4 * f32
        r = torch.exp2(x) - 1
        e = r + U * (1 + r)
        Pu = P * torch.exp2(U * (a + amax))
        r_o = (Pu * e) @ va + 2 * (L + 2) * f32 * oa + _bounds.bound(o, Pu @ va, L, True)
        T = (do @ v.T - (do * o).sum(-1, keepdim=True)).abs()
        eta = acc * (da @ va.T + (da * oa).sum(-1, keepdim=True)) + (da * r_o).sum(-1, keepdim=True)
        E = Pu * (r * T + (1 + r) * eta) + U * Pu * (1 + r) * (T + eta)
        dS = Pu * T
        sc = 1.0 / math.sqrt(C)
        rem = {"o": r_o,
               "dq": sc * (E @ ka) + _bounds.bound(dq, sc * (dS @ ka), L, True),
               "dk": sc * (E.T @ qa) + _bounds.bound(dk, sc * (dS.T @ qa), L, True),
               "dv": (Pu * e).T @ da + _bounds.bound(dv, Pu.T @ da, L, True)}
        ref = {"o": o, "dq": dq, "dk": dk, "dv": dv}
        return {n: (ref[n].detach(), (emu[n][0] - ref[n]).abs() + rem[n]) for n in ref}


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs, the kernels' outputs (two launches) and the per-sequence references of case i,
    computed once and shared by the tests."""
    B, N, spatial, seed, q_amp = CASES[i]
    qkv, g = _inputs(B, N, seed, spatial, q_amp)
    kw = {} if spatial is None else dict(mode="spatial", spatial=spatial)
    y, gr = _run(qkv, g, **kw)
    y2, gr2 = _run(qkv, g, **kw)
    nseq, L = (1, qkv.shape[2]) if spatial is None else (spatial[0], spatial[1] * spatial[2])
    refs = []
    for b in range(B):
        for f in range(nseq):
            t = qkv[b, :, f * L:(f + 1) * L].double()
            do = g[b, :, f * L:(f + 1) * L].double().T
            refs.append(((b, slice(f * L, (f + 1) * L)),
                         _sequence_bounds(t[:C].T, t[C:2 * C].T, t[2 * C:].T, do)))
    return y, gr, y2, gr2, refs


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_elementwise_against_fp64(i):
    y, gr, _, _, refs = _case(i)
    worst = {}
    for (b, sl), ref in refs:
        got = {"o": y[b, :, sl], "dq": gr[b, :C, sl], "dk": gr[b, C:2 * C, sl],
               "dv": gr[b, 2 * C:, sl]}
        for name, (r, bnd) in ref.items():
            err = (got[name].double().T - r).abs()
            ratio = float((err / bnd.clamp_min(1e-300)).max())
            worst[name] = max(worst.get(name, 0.0), ratio)
    print(f"{IDS[i]}: largest |err| / bound " + " ".join(f"{n} {w:.3f}" for n, w in worst.items()))
    for name, w in worst.items():
        assert w <= 1.0, (IDS[i], name, w)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_two_launches_are_equal(i):
    y, gr, y2, gr2, _ = _case(i)
    assert torch.equal(y, y2) and torch.equal(gr, gr2)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_gradients_finite_and_nonzero(i):
    _, gr, _, _, _ = _case(i)
    assert torch.isfinite(gr.float()).all()
    for name, sl in (("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))):
        assert float(gr[:, sl].float().abs().max()) > 0, name
        # every token of every sequence received a gradient (a skipped tile leaves zeros)
        assert bool((gr[:, sl].float().abs().amax(1) > 0).all()), name
