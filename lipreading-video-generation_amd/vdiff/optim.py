"""Adam / AdamW on vd_adam_step: two launches per step and parameter group whatever the number
of tensors, with everything that changes from step to step read on the device.

    opt = FusedAdamW(params, lr=1e-4, weight_decay=0.01, warmup_steps=500, schedule="cosine",
                     total_steps=100_000, min_ratio=0.1, max_bad_run=3)
    loss.backward(); clipper.clip(grads); opt.step(loss=loss.detach(), grad_norm=clipper.norm)
    opt.lr, opt.skip_flag, opt.applied, opt.skipped, opt.tripped_at     # 0-dim device views

* The learning-rate schedule (linear warm-up over `warmup_steps`, then constant, cosine or linear
  decay to min_ratio * lr at `total_steps`) is evaluated in the kernel from the device count of
  APPLIED steps: no lr tensor, no host call per step or epoch, the same launch replays from a HIP
  graph.
* With max_bad_run = K > 0 a step whose loss or gradient norm is non-finite is SKIPPED on the
  device: parameters, moments and counts keep their bits, `skipped` and the run of consecutive
  skipped steps advance, and `skip_flag` (>= 0: the step's index) tells vdiff.ema.EMA.update to
  hold still as well.  More than K skipped steps in a row set `tripped_at` (sticky): every later
  step is skipped too, so the weights stay those of the last good step until the host looks.
  K = 0 never skips (torch's behaviour).  Nothing guards against a non-finite gradient behind a
  finite loss unless grad_norm is passed.
* The bias correction uses each parameter's own count (torch's state["step"]): a parameter left
  out of a step (.grad is None) does not age.

state_dict() / load_state_dict() interchange with torch.optim.Adam / AdamW in both directions.
The kernels follow vd_ema_update's and vd_grad_clip's rules (fixed order, no atomics, no memset,
nothing read on the host); the descriptor table is vdiff.ema's chunk rule
and vdiff.clip.GradClipper's pinned upload, rebuilt only when the list of pointers changes.
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch

from . import ops
from .ema import CHUNK, range_arrays

# kernel nodes of one captured step() per parameter group: the update, the one-block advance
KERNEL_LAUNCHES = 2

SCHEDULES = tuple(ops.LR_SCHEDULES)

_DESC = np.dtype([("p", "<u8"), ("m", "<u8"), ("v", "<u8"), ("g", "<u8"), ("n", "<i8"),
                  ("tensor", "<i8")])
assert _DESC.itemsize == 48

# the int64 device words of one parameter group
_APPLIED, _SKIPPED, _RUN, _TRIPPED, _FLAG, _WORDS = 0, 1, 2, 3, 4, 8

# what torch.optim.Adam / AdamW keep in a parameter group beyond lr, betas, eps, weight_decay
_TORCH_GROUP = {"amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
                "differentiable": False}


def lr_at(s, lr, warmup_steps=0, schedule="constant", total_steps=None, min_ratio=0.0):
    """The rate of the step taken after `s` applied steps, in Python floats (fp64): the formula
    the kernel evaluates (include/vdiff.h)."""
    W = int(warmup_steps)
    warm = 1.0 if W <= 0 else min(1.0, (s + 1) / W)
    if schedule == "constant":
        return lr * warm
    q = min(max((s - W) / (int(total_steps) - W), 0.0), 1.0)
    if schedule == "cosine":
        decay = min_ratio + (1.0 - min_ratio) * (1.0 + math.cos(math.pi * q)) * 0.5
    elif schedule == "linear":
        decay = min_ratio + (1.0 - min_ratio) * (1.0 - q)
    else:
        raise ValueError(f"schedule {schedule!r}: one of {SCHEDULES}")
    return lr * warm * decay


def descriptor_rows(p_ptrs, m_ptrs, v_ptrs, g_ptrs, numels, tensors, chunk=CHUNK):
    """The vd_adam_desc table (numpy, 48-byte rows) of fp32 tensors with numels[i] elements at
    the four addresses [pmvg]_ptrs[i], cut by vdiff.ema's chunk rule; tensors[i] is the tensor's
    index into the step-count array.  Vectorised: no Python loop per range."""
    index, start, n = range_arrays(numels, chunk)
    rows = np.empty(len(index), _DESC)
    off = 4 * start.astype(np.uint64)
    for name, ptrs in (("p", p_ptrs), ("m", m_ptrs), ("v", v_ptrs), ("g", g_ptrs)):
        rows[name] = np.asarray(ptrs, dtype=np.uint64).reshape(-1)[index] + off
    rows["n"] = n
    rows["tensor"] = np.asarray(tensors, dtype=np.int64).reshape(-1)[index]
    return rows


def _number(x, what, lo=None, hi=None, hi_open=False, integer=False):
    """x as a float (or int) if it is a number with lo <= x <= hi (x < hi: hi_open), else
    ValueError.  NaN fails every comparison."""
    ok = isinstance(x, numbers.Integral if integer else numbers.Real) and not isinstance(x, bool)
    if ok:
        x = int(x) if integer else float(x)
        ok = (lo is None or x >= lo) and (hi is None or (x < hi if hi_open else x <= hi))
    if not ok:
        kind = "an integer" if integer else "a number"
        bound = f">= {lo}" if hi is None else f"in [{lo}, {hi}{')' if hi_open else ']'}"
        raise ValueError(f"FusedAdamW: {what} = {x!r}: {kind} {bound}")
    return x


def check_hyper(lr, betas, eps, weight_decay, warmup_steps, schedule, total_steps, min_ratio,
                max_bad_run):
    """ValueError for what vd_adam_step would refuse (the same ranges, checked before a GPU is
    involved)."""
    _number(lr, "lr", 0.0)
    if not (isinstance(betas, (tuple, list)) and len(betas) == 2):
        raise ValueError(f"FusedAdamW: betas = {betas!r}: two numbers in [0, 1)")
    for i, b in enumerate(betas):
        _number(b, f"betas[{i}]", 0.0, 1.0, hi_open=True)
    if not (_number(eps, "eps", 0.0) > 0.0 and math.isfinite(eps)):
        raise ValueError(f"FusedAdamW: eps = {eps!r}: a number > 0")
    _number(weight_decay, "weight_decay", 0.0)
    if not (math.isfinite(lr) and math.isfinite(weight_decay)):
        raise ValueError("FusedAdamW: lr and weight_decay must be finite")
    _number(warmup_steps, "warmup_steps", 0, integer=True)
    if schedule not in SCHEDULES:
        raise ValueError(f"FusedAdamW: schedule = {schedule!r}: one of {SCHEDULES}")
    _number(min_ratio, "min_ratio", 0.0, 1.0)
    _number(max_bad_run, "max_bad_run", 0, integer=True)
    if schedule != "constant":
        if total_steps is None:
            raise ValueError(f"FusedAdamW: schedule {schedule!r} needs total_steps")
        if _number(total_steps, "total_steps", 1, integer=True) <= warmup_steps:
            raise ValueError(f"FusedAdamW: total_steps = {total_steps} <= warmup_steps = "
                             f"{warmup_steps} with the {schedule} schedule")
    elif total_steps is not None:
        _number(total_steps, "total_steps", 0, integer=True)


class _Table:
    """One parameter group's device descriptor table: GradClipper's pinned stage, event and
    rebuild-on-change."""

    def __init__(self):
        self.key = None
        self.n_desc = 0
        self.table = None
        self.stage = None
        self.evt = None

    def build(self, key, rows, device):
        n = len(rows)
        if n > 0:
            if self.stage is None or self.stage.numel() < 48 * n:
                cap = 48 * max(n + n // 2, 1024)
                self.stage = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
                self.evt = torch.cuda.Event()
                self.table = torch.empty(cap, dtype=torch.uint8, device=device)
            else:
                self.evt.synchronize()  # the previous upload has left the buffer
            self.stage.numpy()[:48 * n] = rows.view(np.uint8)
            self.table[:48 * n].copy_(self.stage[:48 * n], non_blocking=True)
            self.evt.record()
        self.n_desc = n
        self.key = key


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.Adam / AdamW (no amsgrad, no maximize) over fp32, contiguous parameters.

    decoupled=True is AdamW's p *= 1 - lr_s * weight_decay, False adds weight_decay * p to the
    gradient (Adam's L2); with weight_decay = 0 both are Adam.  state[p] = {"step", "exp_avg",
    "exp_avg_sq"}, created when p first has a gradient; "step" is a 0-dim view into one device
    int64 array.  `rebuilds` counts table rebuilds (gradients released every step come back at
    other addresses more often than not; static gradients build once).  Hyperparameters are
    read from the parameter group at every step() and passed by value: a captured step() freezes
    them.  The properties read the FIRST parameter group's words; every group takes its own,
    identical, decision from the same loss and norm."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 decoupled=True, warmup_steps=0, schedule="constant", total_steps=None,
                 min_ratio=0.0, max_bad_run=0, chunk=CHUNK):
        check_hyper(lr, betas, eps, weight_decay, warmup_steps, schedule, total_steps, min_ratio,
                    max_bad_run)
        self.chunk = int(chunk)
        range_arrays([], self.chunk)  # the chunk rule's own check
        defaults = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                        weight_decay=float(weight_decay), decoupled=bool(decoupled),
                        warmup_steps=int(warmup_steps), schedule=schedule,
                        total_steps=None if total_steps is None else int(total_steps),
                        min_ratio=float(min_ratio), max_bad_run=int(max_bad_run))
        super().__init__(params, defaults)
        self._index = {}
        for group in self.param_groups:
            check_hyper(*(group[k] for k in ("lr", "betas", "eps", "weight_decay", "warmup_steps",
                                             "schedule", "total_steps", "min_ratio",
                                             "max_bad_run")))
            for p in group["params"]:
                i = len(self._index)
                name = f"parameter {i}"
                if p.dtype != torch.float32:
                    raise TypeError(f"FusedAdamW expects fp32 master parameters ({name} is "
                                    f"{p.dtype})")
                if p.layout != torch.strided or not p.is_contiguous():
                    raise ValueError(f"FusedAdamW expects contiguous parameters ({name} is not)")
                self._index[p] = i
        device = self.param_groups[0]["params"][0].device
        self._steps = torch.zeros(max(len(self._index), 1), dtype=torch.int64, device=device)
        words = torch.zeros(len(self.param_groups), _WORDS, dtype=torch.int64)
        words[:, _TRIPPED] = -1
        words[:, _FLAG] = -1
        self._words = words.to(device)
        self._lr = torch.zeros(len(self.param_groups), dtype=torch.float32, device=device)
        self._tables = [_Table() for _ in self.param_groups]
        self.rebuilds = 0

    # ------------------------------------------------------------------ the record
    @property
    def lr(self):
        """The rate the last step() used (or would have used, where it was skipped): 0-dim
        fp32 device view, 0 before the first step."""
        return self._lr[0]

    @property
    def skip_flag(self):
        """-1 if the last step() was applied, else its global index: 0-dim int64 device view,
        what vdiff.ema.EMA.update(skip_flag=...) reads."""
        return self._words[0, _FLAG]

    @property
    def applied(self):
        return self._words[0, _APPLIED]

    @property
    def skipped(self):
        return self._words[0, _SKIPPED]

    @property
    def bad_run(self):
        return self._words[0, _RUN]

    @property
    def tripped_at(self):
        """-1, or the global index of the step at which more than max_bad_run consecutive steps
        had been skipped (sticky)."""
        return self._words[0, _TRIPPED]

    @property
    def n_desc(self):
        return sum(t.n_desc for t in self._tables)

    # ------------------------------------------------------------------ state
    def _state_of(self, p):
        st = self.state[p]
        if not st:
            st["step"] = self._steps[self._index[p]]
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, loss=None, grad_norm=None):
        """One update of every parameter whose .grad is not None.  loss / grad_norm: fp32 device
        scalars the kernels test when max_bad_run > 0 (None: not tested).  Two launches per
        parameter group, nothing the host waits for.  CPU tensors raise (no CPU fallback)."""
        for gi, group in enumerate(self.param_groups):
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            grads = [p.grad for p in params]
            for p, g in zip(params, grads):
                if g.dtype != torch.float32:
                    raise TypeError(f"FusedAdamW expects fp32 gradients (parameter "
                                    f"{self._index[p]} has {g.dtype})")
                if g.layout != torch.strided or not g.is_contiguous() or g.shape != p.shape:
                    raise ValueError(f"FusedAdamW expects contiguous gradients of the "
                                     f"parameter's shape (parameter {self._index[p]})")
            ops._gpu(*params, *grads, loss, grad_norm)
            tab = self._tables[gi]
            new = [p for p in params if not self.state[p]]
            if new and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdamW.step: the parameter list changed under graph "
                                   "capture (call step() once eagerly on the same tensors first)")
            states = [self._state_of(p) for p in params]
            key = [(p.data_ptr(), s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr(),
                    g.data_ptr(), p.numel(), self._index[p])
                   for p, s, g in zip(params, states, grads)]
            if key != tab.key:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("FusedAdamW.step: the list of pointers changed under "
                                       "graph capture (call step() once eagerly on the same "
                                       "tensors first)")
                cols = list(zip(*key))
                tab.build(key, descriptor_rows(cols[0], cols[1], cols[2], cols[3], cols[4],
                                               cols[5], self.chunk), params[0].device)
                self.rebuilds += 1
            if tab.n_desc == 0:  # only empty tensors
                continue
            hyper = ops.adam_hyper(group["lr"], group["betas"], group["eps"],
                                   group["weight_decay"], group["decoupled"],
                                   group["warmup_steps"], group["schedule"], group["total_steps"],
                                   group["min_ratio"], group["max_bad_run"])
            ops.adam_step(tab.table, tab.n_desc, hyper, self._steps, self._words[gi, :4],
                          self._lr[gi], self._words[gi, _FLAG], loss=loss, grad_norm=grad_norm)

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """A torch.optim.Adam / AdamW state dict (torch's optimizers load it: "step" as an fp32
        tensor, their group keys) whose parameter groups also carry this optimizer's options and
        "fused_state" = [applied, skipped, run, tripped_at] as plain ints (a host read)."""
        sd = super().state_dict()
        words = self._words[:, :4].tolist()
        # new dicts: super() hands out the live per-parameter ones
        sd["state"] = {k: {**st, "step": st["step"].detach().to(torch.float32)}
                       for k, st in sd["state"].items()}
        for gi, (g, live) in enumerate(zip(sd["param_groups"], self.param_groups)):
            for k, v in _TORCH_GROUP.items():
                g.setdefault(k, v)
            g["fused"] = bool(live["params"]) and live["params"][0].is_cuda
            g["decoupled_weight_decay"] = bool(g["decoupled"])
            g["fused_state"] = [int(w) for w in words[gi]]
        return sd

    def load_state_dict(self, state_dict):
        """Load this optimizer's or torch.optim.Adam / AdamW's state dict.  torch's "step" (an
        fp32 or CPU tensor, or a number) becomes this optimizer's device count; options torch
        does not know keep their current values; without "fused_state" (a torch checkpoint) the
        words are [largest step count of the group, 0, 0, -1]."""
        mine = [dict(g) for g in self.param_groups]
        super().load_state_dict(state_dict)
        counts = [0] * self._steps.numel()
        words = []
        for group, old, saved in zip(self.param_groups, mine, state_dict["param_groups"]):
            if "decoupled" not in saved and "decoupled_weight_decay" in saved:
                group["decoupled"] = bool(saved["decoupled_weight_decay"])  # Adam or AdamW
            for k, v in old.items():
                if k != "params":
                    group.setdefault(k, v)
            top = 0
            for p in group["params"]:
                st = self.state.get(p)
                if not st:
                    continue
                i = self._index[p]
                step = st.get("step", 0)
                counts[i] = int(round(float(step)))
                top = max(top, counts[i])
                st["step"] = self._steps[i]
                for k in ("exp_avg", "exp_avg_sq"):
                    # a copy: the kernels write the moments in place, and torch hands over the
                    # checkpoint's own tensors where device and dtype already match
                    st[k] = st[k].detach().to(device=p.device, dtype=torch.float32).clone(
                        memory_format=torch.contiguous_format)
            saved = group.pop("fused_state", None)
            words.append([int(w) for w in saved] if saved is not None else [top, 0, 0, -1])
            if len(words[-1]) != 4:
                raise ValueError(f"FusedAdamW: fused_state {saved!r}: four integers")
        dev = self._steps.device
        self._steps.copy_(torch.tensor(counts, dtype=torch.int64).to(dev))
        self._words[:, :4].copy_(torch.tensor(words, dtype=torch.int64).to(dev))
        self._words[:, _FLAG] = -1
        for tab in self._tables:
            tab.key = None  # the moments are other tensors now
