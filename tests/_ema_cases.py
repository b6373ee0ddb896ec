"""Shared by tests/test_ema_host.py and tests/test_gpu_ema.py (not collected): the tensor
lists, the fp64 reference of one EMA update and the per-element bound both files use.

Reference: e + (1 - d)(p - e) in fp64 on the fp32 inputs and on the fp32 value of d.  Bound:

    |got - ref| <= 2^-24 |ref| + 4 * 2^-24 (1 - d) |p - e|

-- the output rounding, plus the roundings of 1 - d, p - e and their product (3 units), plus
one unit for the output rounding being relative to the computed, not the exact, sum."""
import numpy as np

from vdiff.ema import CHUNK

U = 2.0 ** -24
C = CHUNK
SIZES = (1, 7, 8, 9, C - 1, C, C + 1, 2 * C + 3)
N_ONES = 3000


def decay32(rate, warmup=False, n=0):
    """The fp32 decay the kernel uses: rate, or min(rate, (float)(1 + n) / (float)(10 + n))."""
    d = np.float32(rate)
    if warmup:
        d = min(d, np.float32(np.float32(1 + n) / np.float32(10 + n)))
    return np.float32(d)


def ref64(p, e, d):
    """fp64 update of fp32 arrays p (parameter), e (shadow) at the fp32 decay d."""
    p, e, d = p.astype(np.float64), e.astype(np.float64), float(d)
    return e + (1.0 - d) * (p - e)


def bound(p, e, d):
    p, e, d = p.astype(np.float64), e.astype(np.float64), float(d)
    return U * np.abs(e + (1.0 - d) * (p - e)) + 4 * U * (1.0 - d) * np.abs(p - e)


def emulate(p, e, d, fused):
    """The update in fp32 arithmetic: w = fl(1 - d), t = fl(p - e), then fl(e + fl(w t)) or the
    fused fl(e + w t) (w t is exact in fp64; the second rounding of the sum is far below the
    bound's slack)."""
    w = np.float32(1) - np.float32(d)
    t = (p - e).astype(np.float32)
    if fused:
        return (e.astype(np.float64) + w.astype(np.float64) * t.astype(np.float64)).astype(
            np.float32)
    return (e + (w * t).astype(np.float32)).astype(np.float32)
