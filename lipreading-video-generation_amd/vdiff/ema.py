"""Exponential moving averages of the training weights, updated by one HIP launch per step.

The reference ships update_ema (utils.py:92-102; nn.update_ema here) and never calls it: a
Python loop of two torch ops per tensor and rate.  EMA below keeps up to four shadow sets of a
model's trainable parameters and updates all of them with ONE vd_ema_update launch: each
parameter is read once for every rate, the update count of the warm-up decay and Trainer's
bad-step flag are read on the device (no host sync, replayable from a HIP graph), and a step
whose loss went non-finite never reaches the shadows.

    e <- e + (1 - d) (p - e),   d = rate,  or with warmup  min(rate, (1 + n) / (10 + n))

with n the number of updates done before this one (the guided-diffusion / diffusers
convention).
"""
from __future__ import annotations

import contextlib
from collections import OrderedDict

import numpy as np
import torch

from . import ops

# Elements per descriptor (one block's share of a tensor at a time).  Measured on the config-2
# parameter list (tools/ema_bench.py, profiles/ema_bench.txt: 2048 .. 262144 tried); a multiple
# of 8 so that every range of a 16-B aligned tensor stays 16-B aligned.
CHUNK = 16384
MAX_RATES = 4

_DESC = np.dtype([("src", "<u8"), ("dst", "<u8", (4,)), ("n", "<i8")])
assert _DESC.itemsize == 48


def range_arrays(numels, chunk=CHUNK):
    """The chunk rule as three int64 arrays (tensor index, first element, elements), one entry
    per range: every tensor cut into ranges of at most `chunk` elements, in order; no range
    crosses a tensor and empty tensors get none.  No Python loop per range (vdiff.clip rebuilds
    its table during training)."""
    if chunk <= 0 or chunk % 8:
        raise ValueError(f"chunk {chunk}: a positive multiple of 8")
    numels = np.asarray(numels, dtype=np.int64).reshape(-1)
    counts = -(-numels // chunk)                      # ranges per tensor, 0 for an empty one
    index = np.repeat(np.arange(len(numels), dtype=np.int64), counts)
    first_range = np.cumsum(counts) - counts          # a tensor's first range in the table
    start = (np.arange(len(index), dtype=np.int64) - first_range[index]) * chunk
    return index, start, np.minimum(chunk, numels[index] - start)


def chunk_ranges(numels, chunk=CHUNK):
    """[(tensor index, first element, elements)]: range_arrays as a list of Python ints."""
    return list(zip(*(a.tolist() for a in range_arrays(numels, chunk))))


def descriptor_rows(src_ptrs, dst_ptrs, numels, chunk=CHUNK):
    """The vd_ema_desc table (numpy, 48-byte rows) of fp32 tensors at addresses src_ptrs[i] with
    shadows at dst_ptrs[j][i] for rate j."""
    ranges = chunk_ranges(numels, chunk)
    rows = np.zeros(len(ranges), _DESC)
    for r, (i, s, n) in enumerate(ranges):
        rows[r]["src"] = src_ptrs[i] + 4 * s
        for j, ptrs in enumerate(dst_ptrs):
            rows[r]["dst"][j] = ptrs[i] + 4 * s
        rows[r]["n"] = n
    return rows


def _check_rates(rates):
    rates = tuple(float(r) for r in rates)
    if not 1 <= len(rates) <= MAX_RATES:
        raise ValueError(f"EMA: 1 to {MAX_RATES} rates, got {len(rates)}")
    if len(set(rates)) != len(rates):
        raise ValueError(f"EMA: duplicate rates in {rates}")
    for r in rates:
        if not 0.0 <= r < 1.0:
            raise ValueError(f"EMA: rate {r} outside [0, 1)")
    return rates


class EMA:
    """Shadows of `model`'s trainable parameters for every rate of `rates`.

    The tracked parameters must be fp32 and contiguous (the master weights, as GradBucketer
    expects them).  Each shadow starts as a copy of its parameter.  update() is one launch plus
    the device-side count increment."""

    def __init__(self, model, rates=(0.9999,), warmup=False, chunk=CHUNK):
        self.rates = _check_rates(rates)
        self.warmup = bool(warmup)
        self.chunk = int(chunk)
        self.model = model
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        if not named:
            raise ValueError("EMA: the model has no trainable parameter")
        for n, p in named:
            if p.dtype != torch.float32:
                raise TypeError(f"EMA expects fp32 master parameters ({n} is {p.dtype})")
            if not p.is_contiguous():
                raise ValueError(f"EMA expects contiguous parameters ({n} is not)")
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        self.shadows = [[p.detach().clone() for p in self.params] for _ in self.rates]
        self.num_updates = torch.zeros((), dtype=torch.int64, device=self.params[0].device)
        self._table = None
        self._ptrs = None
        self._build()

    # ------------------------------------------------------------------ descriptor table
    def _build(self):
        self._ptrs = [p.data_ptr() for p in self.params]
        rows = descriptor_rows(self._ptrs, [[s.data_ptr() for s in sh] for sh in self.shadows],
                               [p.numel() for p in self.params], self.chunk)
        self.n_desc = len(rows)
        self._table = torch.from_numpy(rows.view(np.uint8).copy()).to(self.params[0].device)

    def _index(self, rate):
        if rate is None:
            if len(self.rates) != 1:
                raise ValueError(f"EMA: name one of the rates {self.rates}")
            return 0
        try:
            return self.rates.index(float(rate))
        except ValueError:
            raise KeyError(f"EMA: no rate {rate} among {self.rates}") from None

    # ------------------------------------------------------------------ the update
    def update(self, skip_flag=None):
        """One step of every shadow towards the current parameters; no host sync.  skip_flag:
        int64 device scalar, >= 0 leaves the shadows as they are (Trainer's first bad step);
        the count advances either way."""
        ops._gpu(*self.params)
        if any(p.data_ptr() != q for p, q in zip(self.params, self._ptrs)):
            self._build()  # a parameter's storage moved (.to(), load_state_dict(assign=True))
        ops.ema_update(self._table, self.n_desc, self.rates, self.warmup, self.num_updates,
                       skip_flag)
        self.num_updates.add_(1)

    # ------------------------------------------------------------------ reading the shadows
    def state_dict(self, rate=None):
        """model.state_dict() with the tracked parameters replaced by the shadows of `rate`
        (untracked parameters and buffers are the model's): loads into the model class and
        into test.py --ckpt.  The entries are the live tensors, as state_dict() gives them."""
        sh = self.shadows[self._index(rate)]
        sd = OrderedDict(self.model.state_dict())
        for n, s in zip(self.names, sh):
            sd[n] = s
        return sd

    def copy_to(self, model, rate=None):
        """Copy the shadows of `rate` into the same-named parameters of `model`, in place (the
        storage stays, the version counters advance: cached packed operands are re-packed)."""
        sh = self.shadows[self._index(rate)]
        own = dict(model.named_parameters())
        with torch.no_grad():
            torch._foreach_copy_([own[n] for n in self.names], list(sh))

    @contextlib.contextmanager
    def swapped(self, model, rate=None):
        """The EMA weights of `rate` in `model` for the body (validation sampling during
        training), the training weights back on exit, bit for bit.  In-place copies: the
        parameters keep their storage, which step_packed_weights keys on, and their version
        counters advance, which frozen_weights keys on."""
        own = dict(model.named_parameters())
        params = [own[n] for n in self.names]
        backup = [p.detach().clone() for p in params]
        self.copy_to(model, rate)
        try:
            yield model
        finally:
            with torch.no_grad():
                torch._foreach_copy_(params, backup)

    # ------------------------------------------------------------------ checkpoints
    def checkpoint(self):
        """Rates, warm-up, count and shadows as tensors and plain Python values
        (torch.load(weights_only=True) reads it)."""
        return {"rates": list(self.rates), "warmup": self.warmup,
                "num_updates": self.num_updates.detach().clone(),
                "shadows": [{n: s.detach().clone() for n, s in zip(self.names, sh)}
                            for sh in self.shadows]}

    def load_checkpoint(self, d):
        rates = tuple(float(r) for r in d["rates"])
        if rates != self.rates:
            raise ValueError(f"EMA checkpoint holds rates {rates}, this EMA {self.rates}")
        for sh, saved in zip(self.shadows, d["shadows"]):
            missing = [n for n in self.names if n not in saved]
            if missing:
                raise KeyError(f"EMA checkpoint lacks {missing[:4]}")
            with torch.no_grad():
                for n, s in zip(self.names, sh):
                    s.copy_(saved[n])
        self.num_updates.copy_(d["num_updates"])

    def reset_to_parameters(self):
        """Every shadow <- the current parameters (after loading weights without an EMA)."""
        with torch.no_grad():
            for sh in self.shadows:
                torch._foreach_copy_(list(sh), [p.detach() for p in self.params])
