"""Shared by tests/test_clip_host.py and tests/test_gpu_clip.py (not collected): the gradient
list of the kernel tests, a numpy fp32 emulation of the summation layout csrc/gradclip.hip
documents, and the error bounds both files hold the kernels to.

The bound (derived, not tuned).  Every term of a sum of squares is non-negative, so a value
computed through a chain of D fp32 roundings lies within a factor (1 + U)^D, U = 2^-24, of the
exact sum.  The layout gradclip.hip states: a lane adds its squares with one fused
multiply-add each (one rounding per element), then a log2(kBlock)-round LDS tree joins the
lanes (one rounding per round).  A range of n <= chunk elements whose pointer is 16-B aligned
gives a lane at most ceil(chunk / (kVec kBlock)) vectors of kVec elements plus one tail element;
any other range ceil(chunk / kBlock) elements, which is no more.  So

    D = kVec * ceil(chunk / (kVec * kBlock)) + 1 + log2(kBlock)          (73 at chunk 16384)

for every partial, with kBlock and kVec READ FROM THE KERNEL SOURCE below.  The finish block
adds the partials in fp64: ceil(n_desc / kBlock) adds per lane and the same tree, each within
2^-53 -- this is what an fp64 combine buys: the combine's depth (20 roundings for the 3017
partials of the list here) leaves the bound.

    total:  T = (1 + U)^D (1 + 2^-53)^(ceil(n_desc / kBlock) + log2 kBlock) - 1
    norm :  sqrt halves a relative error (sqrt(1 +- T) within 1 +- (T / 2 + T^2)), then the fp64
            square root and the conversion to fp32 round once each:
            N = (1 + T / 2 + T^2)(1 + 2^-53)(1 + U) - 1
    coef :  max_norm / (norm + 1e-6) in fp32: the denominator inherits N (the fp32 constant
            1e-6f is within U <= N of 1e-6), the add and the divide round once each, min is exact:
            C = (1 + U) / ((1 - N)(1 - U)) - 1
    norm after clipping, measured again: each product g * coef rounds once, coef * norm <=
            max_norm (1 + U)^2 (1 + N), and the second measurement is again within N:
            max_norm (1 + N)^2 (1 + U)^4

The fp64 reference (numpy's pairwise sum, one sqrt) is itself within REF = 64 * 2^-53 of the
exact value, which is added to each bound.  test_clip_host.py emulates the layout in fp32 on the
list and asserts error / bound <= 1 there, before any kernel runs."""
import math
import os
import re

import numpy as np

from conftest import PKG
from vdiff.ema import CHUNK, chunk_ranges

U = 2.0 ** -24
U64 = 2.0 ** -53
REF = 64 * U64
C = CHUNK
SIZES = (1, 7, 8, 9, C - 1, C, C + 1, 2 * C + 3)
SLICES = ((37, 1), (C + 5, 2), (2 * C + 1, 3))     # (numel, elements off 16-B alignment)
N_ONES = 3000
GUARD = 8
SENTINEL = 12345.0

_SRC = open(os.path.join(PKG, "csrc", "gradclip.hip")).read()


def _const(name):
    m = re.search(rf"constexpr\s+int\s+{name}\s*=\s*(\d+)\s*;", _SRC)
    assert m, f"gradclip.hip states no {name}"
    return int(m.group(1))


KBLOCK = _const("kBlock")
KVEC = _const("kVec")
LOG_BLOCK = KBLOCK.bit_length() - 1
assert 1 << LOG_BLOCK == KBLOCK


# ------------------------------------------------------------------ bounds
def depth(chunk=C):
    """Longest chain of fp32 roundings behind one partial of a range of <= chunk elements."""
    return KVEC * -(-chunk // (KVEC * KBLOCK)) + 1 + LOG_BLOCK


def total_bound(n_desc, chunk=C):
    d64 = -(-n_desc // KBLOCK) + LOG_BLOCK
    return math.expm1(depth(chunk) * math.log1p(U) + d64 * math.log1p(U64))


def norm_bound(n_desc, chunk=C):
    t = total_bound(n_desc, chunk)
    return (1 + t / 2 + t * t) * (1 + U64) * (1 + U) - 1 + REF


def coef_bound(n_desc, chunk=C):
    n = norm_bound(n_desc, chunk)
    return (1 + U) / ((1 - n) * (1 - U)) - 1


def clipped_norm_bound(n_desc, chunk=C):
    n = norm_bound(n_desc, chunk)
    return (1 + n) ** 2 * (1 + U) ** 4 - 1


# ------------------------------------------------------------------ the gradient list
class Layout:
    """One flat fp32 buffer holding every gradient tensor between guard bands of SENTINEL:
    one 16-B aligned tensor per size of SIZES, the three SLICES starting 1, 2 and 3 elements
    off 16-B alignment, and N_ONES one-element tensors with two guard elements between them.
    offsets / numels are in elements of the buffer (whose base must be 16-B aligned)."""

    def __init__(self, seed=2024):
        self.offsets, self.numels = [], []
        pos = 0
        for n, mis in [(n, 0) for n in SIZES] + list(SLICES):
            pos = -(-(pos + GUARD) // 8) * 8 + mis
            self.offsets.append(pos)
            self.numels.append(n)
            pos += n
        pos = -(-(pos + GUARD) // 8) * 8
        self.first_one = len(self.numels)
        for i in range(N_ONES):
            self.offsets.append(pos + 3 * i)
            self.numels.append(1)
        self.size = pos + 3 * N_ONES + GUARD
        self.mask = np.zeros(self.size, bool)       # True where a gradient lives
        for o, n in zip(self.offsets, self.numels):
            assert not self.mask[o - 1:o + n + 1].any()   # a guard on either side
            self.mask[o:o + n] = True
        rng = np.random.default_rng(seed)
        vals = rng.standard_normal(self.size) * 10.0 ** rng.integers(-3, 3, self.size)
        self.host = np.full(self.size, SENTINEL, np.float32)
        self.host[self.mask] = vals.astype(np.float32)[self.mask]
        self.ranges = chunk_ranges(self.numels, C)  # (tensor, first element, elements)

    def zeros(self):
        """The buffer with every gradient +0 (the guard bands keep the sentinel)."""
        z = self.host.copy()
        z[self.mask] = 0.0
        return z

    def range_of(self, tensor, element):
        """Descriptor index of `element` of `tensor`."""
        for r, (i, s, n) in enumerate(self.ranges):
            if i == tensor and s <= element < s + n:
                return r
        raise KeyError((tensor, element))

    def tensor_of_range(self, r):
        return self.ranges[r][0]

    def one_hot_positions(self):
        """{what: (tensor, element)} of the one-hot test: the places a skipped tail, vector,
        range or descriptor would hide."""
        big = SIZES.index(2 * C + 3)
        n_desc = len(self.ranges)
        out = {
            "first of a multi-chunk tensor": (big, 0),
            "last of a multi-chunk tensor": (big, 2 * C + 2),
            "after the last full 8-vector (n = 9)": (SIZES.index(9), 8),
            "after the last full 8-vector (n = C - 1)": (SIZES.index(C - 1), (C - 1) // 8 * 8),
            "last element before a chunk boundary": (big, C - 1),
            "first element after a chunk boundary": (big, C),
        }
        for k, (n, mis) in enumerate(SLICES):
            out[f"first of the slice {mis} off alignment"] = (len(SIZES) + k, 0)
        for d in (0, 255, 256, 2047, 2048, n_desc - 1):
            t = self.tensor_of_range(d)
            assert self.numels[t] == 1
            out[f"one-element tensor at descriptor {d}"] = (t, 0)
        return out


def ref_norm64(buf, mask):
    return float(np.sqrt(np.sum(buf[mask].astype(np.float64) ** 2)))


# ------------------------------------------------------------------ fp32 emulation of the layout
def _fma_chain(s, x):
    """s <- fl32(x * x + s) for fp32 arrays (x * x is exact in fp64; rounding the fp64 sum to
    fp32 differs from the fused operation's single rounding only in a double-rounding tie, far
    below the bound's slack)."""
    return (x.astype(np.float64) ** 2 + s.astype(np.float64)).astype(np.float32)


def emulate_partial(x, aligned):
    """The partial of one range (fp32 array x) as grad_sumsq_kernel computes it."""
    n = len(x)
    nv = n // KVEC if aligned else 0
    s = np.zeros(KBLOCK, np.float32)
    steps = -(-nv // KBLOCK)
    if steps:
        v = np.zeros((steps * KBLOCK, KVEC), np.float32)   # zero padding: fma(0, 0, s) = s
        v[:nv] = x[:nv * KVEC].reshape(nv, KVEC)
        v = v.reshape(steps, KBLOCK, KVEC)
        for j in range(steps):
            for k in range(KVEC):
                s = _fma_chain(s, v[j, :, k])
    tail = x[nv * KVEC:]
    steps = -(-len(tail) // KBLOCK)
    if steps:
        t = np.zeros(steps * KBLOCK, np.float32)
        t[:len(tail)] = tail
        for row in t.reshape(steps, KBLOCK):
            s = _fma_chain(s, row)
    w = KBLOCK // 2
    while w:
        s = (s[:w] + s[w:2 * w]).astype(np.float32)
        w //= 2
    return s[0]


def emulate(layout, buf):
    """(norm, partials) as the three launches compute them on the buffer `buf`."""
    parts = np.empty(len(layout.ranges), np.float32)
    for r, (i, s, n) in enumerate(layout.ranges):
        o = layout.offsets[i] + s
        parts[r] = emulate_partial(buf[o:o + n], o % 4 == 0)
    lanes = np.zeros(-(-len(parts) // KBLOCK) * KBLOCK, np.float64)
    lanes[:len(parts)] = parts
    acc = np.zeros(KBLOCK, np.float64)
    for row in lanes.reshape(-1, KBLOCK):
        acc = acc + row
    w = KBLOCK // 2
    while w:
        acc = acc[:w] + acc[w:2 * w]
        w //= 2
    return np.float32(np.sqrt(acc[0])), parts


def emulate_coef(norm, max_norm):
    norm, max_norm = np.float32(norm), np.float32(max_norm)
    if not np.isfinite(norm):
        return np.float32(1)
    with np.errstate(divide="ignore"):
        return min(np.float32(1), np.float32(max_norm / np.float32(norm + np.float32(1e-6))))
