"""Cases, independent references and error bounds of long-clip sampling (vdiff.schedulers.
WindowPlan, vd_window_gather, vd_window_blend, vdiff.engine.sample_long), shared by
tests/test_window_host.py (CPU) and tests/test_gpu_window.py.  Nothing here imports the plan: the
window starts, the coverage and the weights are written again from the formulas, in integers and
exact fractions.

Notation: a clip of L frames, windows of T frames every S frames, W = ceil((L - T) / S) + 1
windows, starts[w] = min(w S, L - T); profile g[f] = min(f + 1, T - f) ("triangle") or 1
("uniform"); frame l is covered by the windows w with 0 <= l - starts[w] < T, in ascending
order, with the weights g[l - starts[w]] / (their sum).
"""
from fractions import Fraction

import torch

BLENDS = ("triangle", "uniform")
# (L, T, S): one window; even overlap; a shifted last window; a shift that makes coverage 3;
# stride 1 (coverage 4); the flagship window at twice and a half its length
PLANS = [(4, 4, 4), (10, 4, 2), (11, 4, 3), (9, 4, 2), (9, 4, 1), (40, 16, 8)]
# (B, C, L, T, S, HW) of the kernel tests
KERNEL_SHAPES = [
    (1, 3, 10, 4, 2, 35),   # odd HW: the scalar path
    (2, 3, 11, 4, 3, 64),   # shifted last window, the vector path, B = 2
    (1, 3, 4, 4, 4, 16),    # one window
    (2, 1, 9, 4, 1, 20),    # coverage 4
    (1, 3, 9, 4, 2, 36),    # coverage 3 from the shift
]


def n_windows(L, T, S):
    return -(-(L - T) // S) + 1


def starts(L, T, S):
    return [min(w * S, L - T) for w in range(n_windows(L, T, S))]


def profile(T, blend):
    return [min(f + 1, T - f) if blend == "triangle" else 1 for f in range(T)]


def cover(L, T, S):
    """Per clip frame, the windows that hold it, ascending."""
    st = starts(L, T, S)
    return [[w for w, s in enumerate(st) if 0 <= l - s < T] for l in range(L)]


def weights(L, T, S, blend):
    """Per clip frame, the exact weights of its covering windows (Fractions)."""
    st, g = starts(L, T, S), profile(T, blend)
    out = []
    for l, ws in enumerate(cover(L, T, S)):
        gs = [g[l - st[w]] for w in ws]
        out.append([Fraction(v, sum(gs)) for v in gs])
    return out


def max_coverage(L, T, S):
    return max(len(ws) for ws in cover(L, T, S))


# ------------------------------------------------------------------ kernel references
def inputs(rows, C, frames, HW, bf16, seed=0):
    """A fp32 CPU tensor [rows, C, frames, HW] ~ N(0, 1), exact in the kernel dtype."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, C, frames, HW), generator=g)
    return x.bfloat16().float() if bf16 else x


def gather_ref(x, L, T, S):
    """Torch indexing: [B * W, C, T, HW], row b * W + w = x[b, :, starts[w] : starts[w] + T]."""
    wins = [x[:, :, s:s + T] for s in starts(L, T, S)]
    return torch.stack(wins, dim=1).reshape(-1, x.shape[1], T, x.shape[3]).contiguous()


def blend_ref64(win, st, cover_win, cover_wgt, L):
    """(ref, mag) of the blend in fp64 on the tables the kernel reads: the fp32 weights taken as
    exact, like the kernel-dtype operands; mag is the same sum of absolute values.  A slot whose
    window is negative is unused.  With K terms the kernel rounds at most K times (the first
    product, then one fused multiply-add per further term), inside _bounds.bound's (n + 2)
    roundings for n_terms = K; the result is rounded once to the output dtype (u_out)."""
    W = len(st)
    B = win.shape[0] // W
    w5 = win.double().view(B, W, win.shape[1], win.shape[2], win.shape[3])
    ref = torch.zeros((B, win.shape[1], L, win.shape[3]), dtype=torch.float64)
    mag = torch.zeros_like(ref)
    for l in range(L):
        for k in range(cover_win.shape[1]):
            w = int(cover_win[l, k])
            if w < 0:
                continue
            g = float(cover_wgt[l, k].double())
            v = w5[:, w, :, l - st[w]]
            ref[:, :, l] += g * v
            mag[:, :, l] += abs(g) * v.abs()
    return ref, mag
