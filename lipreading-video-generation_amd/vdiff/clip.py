"""Gradient clipping by global L2 norm on vd_grad_sumsq / vd_grad_clip.

torch.nn.utils.clip_grad_norm_'s result -- norm over every gradient of the step, coef =
min(1, max_norm / (norm + 1e-6)), gradients times coef when coef < 1 -- in KERNEL_LAUNCHES = 3
launches whatever the number of tensors, written to the rules of the code next to a captured
step: fixed summation order, no memset, no semaphore, norm and coef stay on
the device and are read there.  The same bits eager and replayed from a HIP graph.

    clipper = GradClipper(1.0)
    loss.backward(); clipper.clip([p.grad for p in params if p.grad is not None]); opt.step()
    clipper.norm, clipper.coef      # 0-dim device views, rewritten by the next clip()
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch

from . import ops
from .ema import CHUNK, range_arrays

# kernel nodes of one captured clip(): per-range sums of squares, the one-block finish (norm,
# coef), the scaling pass (returns at once when coef == 1)
KERNEL_LAUNCHES = 3

_DESC = np.dtype([("g", "<u8"), ("n", "<i8")])
assert _DESC.itemsize == 16


def check_max_norm(max_norm, what="max_norm"):
    """float(max_norm) if it is a number > 0 (inf: measure only), else ValueError."""
    ok = isinstance(max_norm, numbers.Real) and not isinstance(max_norm, bool)
    if not (ok and float(max_norm) > 0.0):  # NaN fails the comparison
        raise ValueError(f"{what} = {max_norm!r}: a number > 0 (inf measures only)")
    return float(max_norm)


def descriptor_rows(ptrs, numels, chunk=CHUNK):
    """The vd_grad_desc table (numpy, 16-byte rows) of fp32 tensors at addresses ptrs[i] with
    numels[i] elements, cut by vdiff.ema's chunk rule; vectorised, no Python loop per range."""
    index, start, n = range_arrays(numels, chunk)
    rows = np.empty(len(index), _DESC)
    rows["g"] = np.asarray(ptrs, dtype=np.uint64).reshape(-1)[index] + 4 * start.astype(np.uint64)
    rows["n"] = n
    return rows


class GradClipper:
    """Clips the gradients of one step to the global norm `max_norm` (inf: measure only).

    Owns the device descriptor table over the step's gradient tensors, the partial-sum
    workspace and the static 2-float record.  clip() launches KERNEL_LAUNCHES kernels on the
    current stream and returns nothing the host has to wait for.  The table is rebuilt only
    when the list of (data_ptr, numel) changes (`rebuilds` counts).  Gradient buckets never
    move (one build); gradients released every step (zero_grad(set_to_none=True)) come back at
    other addresses more often than not (12 rebuilds in 15 config-2 steps),
    as does a list whose members change (wav2vec2's LayerDrop).  A rebuild is numpy over the
    ranges (0.2 ms for 14 660 of them) and one non-blocking upload from pinned memory.

    Under graph capture clip() must find its table current (call it once eagerly on the same
    tensors first): an upload has no place in the captured step."""

    def __init__(self, max_norm, chunk=CHUNK):
        self.max_norm = check_max_norm(max_norm)
        self.chunk = int(chunk)
        range_arrays([], self.chunk)  # the chunk rule's own check
        self.rebuilds = 0
        self.n_desc = 0
        self._key = None
        self._record = None   # device fp32 [norm, coef]
        self._table = None    # device uint8 image of the descriptors (capacity >= n_desc)
        self._work = None     # device fp32 partials (capacity >= n_desc)
        self._stage = None    # pinned host image of the table
        self._stage_evt = None

    # ------------------------------------------------------------------ the record
    @property
    def norm(self):
        """The last clip()'s global norm before clipping: 0-dim device view (None before the
        first clip)."""
        return None if self._record is None else self._record[0]

    @property
    def coef(self):
        """The last clip()'s factor, 1 where nothing was scaled: 0-dim device view."""
        return None if self._record is None else self._record[1]

    # ------------------------------------------------------------------ descriptor table
    def _check(self, tensors, names):
        key = []
        for i, t in enumerate(tensors):
            name = names[i] if names is not None else f"tensor {i}"
            if not torch.is_tensor(t):
                raise TypeError(f"GradClipper: {name} is {type(t).__name__}, not a tensor")
            if t.dtype != torch.float32:
                raise TypeError(f"GradClipper expects fp32 gradients ({name} is {t.dtype})")
            if t.layout != torch.strided or not t.is_contiguous():
                raise ValueError(f"GradClipper expects contiguous gradients ({name} is not)")
            key.append((t.data_ptr(), t.numel()))
        return key

    def _build(self, key, device):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("GradClipper.clip: the gradient list changed under graph capture "
                               "(call clip() once eagerly on the same tensors first)")
        rows = descriptor_rows([k[0] for k in key], [k[1] for k in key], self.chunk)
        n = len(rows)
        if self._record is None:
            # norm 0, coef 1 until the first launch; written once, outside any capture
            self._record = torch.tensor([0.0, 1.0], dtype=torch.float32, device=device)
        if n > 0:
            if self._stage is None or self._stage.numel() < 16 * n:
                cap = 16 * max(n + n // 2, 1024)
                self._stage = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
                self._stage_evt = torch.cuda.Event()
                self._table = torch.empty(cap, dtype=torch.uint8, device=device)
                self._work = torch.empty(cap // 16, dtype=torch.float32, device=device)
            else:
                self._stage_evt.synchronize()  # the previous upload has left the buffer
            self._stage.numpy()[:16 * n] = rows.view(np.uint8)
            self._table[:16 * n].copy_(self._stage[:16 * n], non_blocking=True)
            self._stage_evt.record()
        self.n_desc = n
        self._key = key
        self.rebuilds += 1

    # ------------------------------------------------------------------ the step
    def clip(self, tensors, names=None):
        """Clip the fp32, contiguous gradient tensors of one step in place.  names: what to
        call them in errors.  Anything else raises TypeError / ValueError naming the tensor; CPU
        tensors raise (no CPU fallback)."""
        tensors = list(tensors)
        key = self._check(tensors, names)
        ops._gpu(*tensors)
        if key != self._key:
            if not tensors:
                raise ValueError("GradClipper.clip: no gradient tensor")
            self._build(key, tensors[0].device)
        if self.n_desc == 0:  # only empty tensors: norm 0, nothing to scale
            self._record.copy_(torch.tensor([0.0, 1.0]))
            return
        ops.grad_sumsq(self._table, self.n_desc, self._work)
        ops.grad_clip(self._table, self.n_desc, self._work, self.max_norm, self._record)

    def __repr__(self):
        m = "inf" if math.isinf(self.max_norm) else f"{self.max_norm:g}"
        return f"GradClipper(max_norm={m}, chunk={self.chunk}, ranges={self.n_desc})"
