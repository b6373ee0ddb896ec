"""Samplers around the drop-in model (the loop of the reference test.py:51-83): DDIM,
DPM-Solver++(2M) and long-clip sampling behind one driver (_sample) and one replayed step graph,
and ancestral DDPM sampling.

A step is two independent choices.  The denoiser is "the model's output on the sample": the
model applied directly (_Direct) or through overlapping windows (WindowedDenoiser).  The update
rule is "advance xt given that output": DDIM (DDIMGraph, DDIMSampler.step) or 2M (DPMGraph,
DPMSolverSampler.step).  The four graph classes are the four pairs; capture, replay and the
shared buffers are DDIMGraph's.

Differences from the reference loop (all deliberate): no per-step
torch.cuda.empty_cache() (test.py:58), and the audio encoder runs once per clip instead of at
every denoising step.
"""
from __future__ import annotations

import os
import warnings

import torch

from . import hipgraph, ops
from .schedulers import (DDIMSampler, DPMSolverSampler, WindowPlan, _mask_options, _sqrt_tables,
                         _thresh_kw)


def _encode(model, audio):
    """The audio features of a clip, encoded once: a model without an encoder takes them as
    they are."""
    return model.encode_audio(audio) if hasattr(model, "encode_audio") else audio


def _doubled(cond, feats):
    """The conditioning of a guided forward at batch 2B: cond repeated, and the encoded audio
    followed by the null audio (zeros of the same shape)."""
    return torch.cat([cond, cond]), torch.cat([feats, torch.zeros_like(feats)])


class GraphUnsafe(RuntimeError):
    """A captured graph holds a node type that is not safe to replay (a memset node)."""


# ------------------------------------------------------------------ denoisers
# A denoiser is called as denoise(xt, t) -> the model's output on the sample ([B, ...], or
# [2B, ...] = (conditional; unconditional) when .guided); t has .rows entries.  static(xt) hands
# a step graph its buffers: (the static sample, the buffer capture() saves and restores around
# its warm-up, the step kernel's `dup` buffer or None).  A denoiser never refers to a graph.
class _Direct:
    """The model applied to the sample itself.  Guided: one forward at batch 2B on [xt; xt]
    with the doubled conditioning -- concatenated per call, or, once static() was called, the
    static [2B, ...] input whose halves are the step kernel's `out` and `dup`, so that it stays
    current without a copy (the sample passed to the call is then that input's first half)."""

    def __init__(self, model, cond, feats, xt, guided):
        self.model, self.guided = model, guided
        self.cond, self.feats = _doubled(cond, feats) if guided else (cond, feats)
        self.rows = (2 if guided else 1) * xt.shape[0]
        self.x2 = None

    def static(self, xt):
        if not self.guided:
            xt = xt.clone()
            return xt, xt, None
        B = xt.shape[0]
        self.x2 = torch.cat([xt, xt])
        return self.x2[:B], self.x2, self.x2[B:]

    def __call__(self, xt, t):
        if self.guided:
            xt = torch.cat([xt, xt]) if self.x2 is None else self.x2
        return self.model(xt, self.cond, self.feats, t)


class WindowedDenoiser:
    """The denoiser applied to a long latent through the overlapping windows of a
    schedulers.WindowPlan: gather the windows (vd_window_gather), run the model on them as one
    batch (or in chunks of at most `window_batch` windows), blend the predictions back into the
    long clip (vd_window_blend).  Everything a step needs is built here, before the loop and
    before any capture: the per-frame audio features routed to the windows by plan.frame_index,
    cond repeated per window, the null audio of a guided run (zeros) and the static window
    buffer.  Guided, the window batch is [B * W with the audio; B * W with the null audio], the
    second half filled by the gather's `dup`, and the blend runs over 2B clips: chunk(2) of the
    result is (eps_c, eps_u) on the long clip."""

    def __init__(self, model, plan, cond, feats, xt, guided=False, window_batch=None):
        B, C, L = xt.shape[:3]
        W, T = plan.num_windows, plan.window
        if L != plan.length:
            raise ValueError(f"sample_long: {L} frames for a plan of {plan.length}")
        if cond.shape[0] != B or feats.shape[0] != B * L:
            raise ValueError(f"sample_long: cond {tuple(cond.shape)} / encoded audio "
                             f"{tuple(feats.shape)} do not fit {B} clips of {L} frames (one "
                             "reference image per clip, one audio window per frame)")
        if window_batch is not None and int(window_batch) < 1:
            raise ValueError(f"sample_long: window_batch {window_batch} < 1")
        dev = xt.device
        rows = (torch.arange(B, device=dev).view(B, 1) * L
                + plan.frame_index.to(dev).view(1, W * T)).reshape(-1)
        feats = feats.index_select(0, rows)              # [B * W * T, ...]
        cond = cond.repeat_interleave(W, dim=0)          # [B * W, ...]
        if guided:
            cond, feats = _doubled(cond, feats)
        self.model, self.plan, self.guided = model, plan, guided
        self.cond, self.feats = cond, feats
        self.half = B * W
        self.rows = (2 if guided else 1) * B * W         # of the window batch and its timesteps
        self.chunk = self.rows if window_batch is None else min(int(window_batch), self.rows)
        self.win = torch.empty((self.rows, C, T) + tuple(xt.shape[3:]), dtype=xt.dtype,
                               device=dev)

    def static(self, xt):
        # the long latent itself is what a step changes (the window buffer is rewritten from it
        # by every step's gather), and the step kernel needs no `dup`: the gather makes it
        xt = xt.clone()
        return xt, xt, None

    def __call__(self, xt, t):
        """The model's output on the long clip: [B, ...] like xt, or [2B, ...] guided.  t: the
        window batch's timesteps, [self.rows]."""
        n, T = self.half, self.plan.window
        ops.window_gather(xt, self.plan, out=self.win[:n],
                          dup=self.win[n:] if self.guided else None)
        outs = []
        for i in range(0, self.rows, self.chunk):
            j = min(i + self.chunk, self.rows)
            outs.append(self.model(self.win[i:j], self.cond[i:j], self.feats[i * T:j * T],
                                   t[i:j]))
        eps = outs[0] if len(outs) == 1 else torch.cat(outs)
        return ops.window_blend(eps.to(xt.dtype).contiguous(), self.plan)


# ------------------------------------------------------------------ the step graph
class DDIMGraph:
    """One deterministic DDIM denoising step -- UNet forward + vd_ddim_step -- captured once
    as a HIP graph and replayed per step (no per-kernel launch gaps, no host work per
    step).  The sample lives in a static buffer updated in place; the step's timesteps are
    copied device-to-device from the sampler's table before each replay.  Use inside
    ops.frozen_weights() (the graph reads the cached packed conv weights); eta must be 0.

    guidance_scale != 1 (classifier-free audio guidance): the captured step is the UNet forward
    at batch 2B + vd_cfg_stats (guidance_rescale > 0) + vd_ddim_step_cfg.  The model's output is
    read as sampler.prediction says ("eps" or "v"; the same launches either way).  The graph owns a
    static [2B, ...] input (self.x2) whose halves are the fused kernel's x_prev and x_prev_dup,
    so the doubled input stays current without a copy; the doubled cond / audio / timestep
    buffers and the null audio are built here, before capture (no memset node in the step).

    known / keep (masked sampling, _masked_start's pair): static operands of the captured step
    kernel, which takes the masked entry point in the plain one's place -- the same node counts,
    no copy per step.

    The subclasses change one thing each: DPMGraph the update rule (_rule_buffers, _update), the Long
    classes the denoiser."""

    @_mask_options
    def __init__(self, model, sampler, cond, feats, xt, guidance_scale=1.0, guidance_rescale=0.0,
                 *, known=None, keep=None):
        guided = float(guidance_scale) != 1.0
        self._setup(_Direct(model, cond, feats, xt, guided), sampler, xt, guidance_scale,
                    guidance_rescale, known, keep)
        if guided:
            self.x2 = self.saved

    def _setup(self, denoise, sampler, xt, scale, rescale, known=None, keep=None):
        """The buffers of every step graph.  The timestep buffers have denoise.rows rows (B, 2B
        guided, or one per window of the batch); the step kernels read the first B."""
        self.denoise, self.sampler = denoise, sampler
        self.mask = {} if known is None else dict(known=known, keep=keep)
        self.scale, self.rescale = float(scale), float(rescale)
        self.guided = denoise.guided
        self.graph = None
        # (destination, per-step table): step(i) copies table[i] device-to-device before replay
        self.copies = []
        self.xt, self.saved, self.dup = denoise.static(xt)
        self.t = self._per_step(sampler.timesteps.to(xt.device).view(-1, 1)
                                .expand(-1, denoise.rows).contiguous())
        self._rule_buffers(xt.device)

    def _per_step(self, table):
        buf = table[0].clone()
        self.copies.append((buf, table))
        return buf

    def _rule_buffers(self, dev):
        """The update rule's own buffers: DDIM reads the previous timesteps and the acp table,
        and returns a new x0 from every step."""
        if self.sampler.eta != 0:
            raise ValueError(f"{type(self).__name__}: eta = 0 (deterministic DDIM) only")
        self.tp = self._per_step(self.sampler.prev_timesteps.to(dev).view(-1, 1)
                                 .expand(-1, self.denoise.rows).contiguous())
        self.acp = self.sampler._acp(dev)
        self.x0 = None

    def _update(self, out):
        """Advance self.xt in place given the model's output (a (conditional, unconditional)
        pair when guided); returns x0."""
        B, s = self.xt.shape[0], self.sampler
        if self.guided:
            _, x0 = ops.ddim_step_cfg(self.xt, *out, self.t[:B], self.tp[:B], self.acp,
                                      self.scale, self.rescale, clip=s.clip_x0, out=self.xt,
                                      dup=self.dup, prediction=s.prediction, **_thresh_kw(s),
                                      **self.mask)
            return x0
        xp, x0 = ops.ddim_step(self.xt, out, self.t[:B], self.tp[:B], self.acp, eta=0.0,
                               clip=s.clip_x0, prediction=s.prediction, **_thresh_kw(s),
                               **self.mask)
        self.xt.copy_(xp.view_as(self.xt))
        return x0

    def _body(self):
        out = self.denoise(self.xt, self.t).to(self.xt.dtype)
        return self._update(out.chunk(2) if self.guided else out)

    def capture(self):
        """Warm up eagerly and capture one step (step() does this on first use).  Raises
        GraphUnsafe if the captured step holds a memset node."""
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream(device=self.xt.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):  # eager warm-up: packed weights, tables, workspaces
            keep = self.saved.clone()
            self._body()
            self.saved.copy_(keep)
        cur.wait_stream(side)
        self.graph = torch.cuda.CUDAGraph(keep_graph=True)  # node list kept (node_types)
        with hipgraph.capture(self.graph):
            self.x0 = self._body()
        self.graph.instantiate()
        types = self.node_types()
        if types.get("memset", 0):
            # a memset node replayed with eager work between replays is
            # where a captured reduction went stale on this HIP runtime; sample() steps
            # eagerly instead of trusting such a graph
            raise GraphUnsafe(f"{type(self).__name__}: captured step holds memset nodes {types}")

    def node_types(self):
        """{node type: count} of the captured step (vdiff.hipgraph; memset nodes must be 0)."""
        return hipgraph.node_counts(self.graph)

    def step(self, i):
        """Denoise from sampler.timesteps[i]; returns (x_prev, x0) (static buffers).  2M steps
        run in order: step i reads the x0 that step i - 1 left in the history."""
        for buf, table in self.copies:
            buf.copy_(table[i])
        if self.graph is None:
            self.capture()
        self.graph.replay()
        return self.xt, self.x0.view_as(self.xt)


class DPMGraph(DDIMGraph):
    """One DPM-Solver++(2M) step -- UNet forward + vd_dpm_step, or at batch 2B + vd_cfg_stats +
    vd_dpm_step_cfg when guided -- captured once and replayed for every step: the kernel picks
    its coefficient row by a device scalar, so the first-order, second-order and last steps
    differ only in the table.  On top of DDIMGraph's static sample the graph owns the x0
    history (read as the previous step's x0, written in place; x_prev is written over xt) and
    the step-index scalar, copied device-to-device before each replay like the timesteps."""

    def _rule_buffers(self, dev):
        self.coef, idx = self.sampler._tables(dev)
        self.idx = self._per_step(idx.view(-1, 1))
        # uninitialised on purpose: row 0 has C == 0 and does not read it
        self.x0 = torch.empty_like(self.xt, memory_format=torch.contiguous_format)

    def _update(self, out):
        clip, thr = self.sampler.clip_x0, _thresh_kw(self.sampler)
        if self.guided:
            ops.dpm_step_cfg(self.xt, *out, self.x0, self.coef, self.idx, self.scale,
                             self.rescale, clip=clip, out=self.xt, dup=self.dup, **thr,
                             **self.mask)
        else:
            ops.dpm_step(self.xt, out, self.x0, self.coef, self.idx, clip=clip, out=self.xt,
                         **thr, **self.mask)
        return self.x0


class LongDDIMGraph(DDIMGraph):
    """DDIMGraph for a long clip: the captured step is gather + the UNet forward at batch B * W
    (2 B * W guided) + blend + the same vd_ddim_step / vd_cfg_stats + vd_ddim_step_cfg launches
    on the long tensors.  windows: the clip's WindowedDenoiser, which says whether the step is
    guided."""

    def __init__(self, model, sampler, windows, xt, guidance_scale=1.0, guidance_rescale=0.0,
                 known=None, keep=None):
        self.windows = windows
        self._setup(windows, sampler, xt, guidance_scale, guidance_rescale, known, keep)


class LongDPMGraph(DPMGraph):
    """DPMGraph for a long clip: gather + forward + blend, then vd_dpm_step (vd_cfg_stats +
    vd_dpm_step_cfg guided) in place on the long latent and its x0 history."""

    def __init__(self, model, sampler, windows, xt, guidance_scale=1.0, guidance_rescale=0.0,
                 known=None, keep=None):
        self.windows = windows
        self._setup(windows, sampler, xt, guidance_scale, guidance_rescale, known, keep)


# ------------------------------------------------------------------ masked sampling
def _masked_start(sampler, z, known, keep):
    """Masked sampling's operands, checked once (host syncs are fine here: this runs before the
    loop and before any capture): (the initial sample, known, keep) -- or (z, None, None)
    without a mask.

    known: the clip to keep, of the sample's shape [B, C, *spatial]; it is cast to the sample's
    dtype and device.  keep: the mask, [Bk, 1, *spatial] (schedulers.keep_mask) or [Bk, S], Bk in
    (1, B), values in [0, 1]; it becomes the step kernel's contiguous fp32 [Bk, S].  The sample
    starts as z + k (q_sample(x_k, z, t0) - z) with z the driver's own noise and t0 the first
    timestep: where k == 1 it is the known clip noised to t0 with that very z (exactly
    q_sample's value), where k == 0 it is z."""
    if known is None and keep is None:
        return z, None, None
    if known is None or keep is None:
        raise ValueError("masked sampling: known and keep are given together or not at all")
    B, spatial = z.shape[0], tuple(z.shape[2:])
    if tuple(known.shape) != tuple(z.shape):
        raise ValueError(f"masked sampling: known {tuple(known.shape)} for a sample of shape "
                         f"{tuple(z.shape)}")
    S = z[0, 0].numel()
    if keep.dim() == 2:
        ok = keep.shape[0] in (1, B) and keep.shape[1] == S
    else:
        ok = keep.shape[0] in (1, B) and tuple(keep.shape[1:]) == (1,) + spatial
    if not ok:
        raise ValueError(f"masked sampling: keep {tuple(keep.shape)} is neither [Bk, 1, "
                         f"{', '.join(str(d) for d in spatial)}] nor [Bk, {S}], Bk in (1, {B})")
    known = known.to(device=z.device, dtype=z.dtype).contiguous()
    keep = keep.to(device=z.device, dtype=torch.float32).reshape(keep.shape[0], S).contiguous()
    if not bool(((keep >= 0) & (keep <= 1)).all()):
        raise ValueError("masked sampling: keep has values outside [0, 1]")
    t0 = torch.full((B,), int(sampler.timesteps[0]), dtype=torch.int64, device=z.device)
    acp = sampler.acp.to(z.device)
    q = ops.q_sample(known, z.contiguous(), t0, acp.sqrt().contiguous(),
                     (1 - acp).sqrt().contiguous())
    k = keep.view((keep.shape[0], 1) + spatial).to(z.dtype)
    return torch.where(k >= 1, q, z + k * (q - z)), known, keep


# ------------------------------------------------------------------ the driver
def _sample(model, sampler, dpm, cond, audio, shape, generator, callback, scale, rescale,
            plan=None, window_batch=None, known=None, keep=None):
    """sample_ddim / sample_dpm (dpm: the 2M update rule) and, with a plan, sample_long.  On a
    GPU one step is captured and replayed unless VDIFF_DDIM_GRAPH=0 or DDIM's eta != 0; the
    eager loop launches the same kernels on the same operands."""
    model.eval()
    device = cond.device
    feats = _encode(model, audio)
    xt = torch.randn(shape, generator=generator, device=device)
    xt, known, keep = _masked_start(sampler, xt, known, keep)
    mask = {} if known is None else dict(known=known, keep=keep)  # a sampler need not know them
    guided = scale != 1.0
    windows = None
    if plan is not None:
        windows = WindowedDenoiser(model, plan, cond, feats, xt, guided, window_batch)
    if (device.type == "cuda" and os.environ.get("VDIFF_DDIM_GRAPH", "1") != "0"
            and (dpm or sampler.eta == 0)):
        if windows is None:
            g = (DPMGraph if dpm else DDIMGraph)(model, sampler, cond, feats, xt, scale, rescale,
                                                 **mask)
        else:
            g = (LongDPMGraph if dpm else LongDDIMGraph)(model, sampler, windows, xt, scale,
                                                         rescale, **mask)
        try:
            g.capture()
        except GraphUnsafe as e:
            warnings.warn(f"{e}; sampling eagerly")
            g = None
        if g is not None:
            for i in range(sampler.steps):
                xt, x0 = g.step(i)
                if callback is not None:  # the graph's static buffers: the next replay rewrites them
                    callback(i, xt.clone(), x0.clone())
            return xt.clone(), x0.clone()
    denoise = _Direct(model, cond, feats, xt, guided) if windows is None else windows
    x0 = None
    for i in range(sampler.steps):
        t = torch.full((denoise.rows,), int(sampler.timesteps[i]), dtype=torch.int64,
                       device=device)
        out = denoise(xt, t)
        kw = dict(mask, x0_last=x0) if dpm else mask
        if guided:
            eps_c, eps_u = out.chunk(2)
            xt, x0 = sampler.step_guided(xt, eps_c, eps_u, i, scale, rescale, **kw)
        else:
            xt, x0 = sampler.step(xt, out, i, **kw)
        if callback is not None:  # 2M's x0 is the history buffer: the next step rewrites it
            callback(i, xt, x0.clone() if dpm else x0)
    return xt, x0


@_mask_options
@torch.no_grad()
def sample_ddim(model, sampler, cond, audio, shape, generator=None, callback=None,
                guidance_scale=1.0, guidance_rescale=0.0, *, known=None, keep=None):
    """DDIM sampling (build extension of test.py:51-83): audio encoded once, packed conv
    weights reused across steps (ops.frozen_weights).

    guidance_scale w != 1: classifier-free audio guidance.  Each step runs one forward at batch
    2B -- rows [0, B) with the encoded audio, rows [B, 2B) with the null audio (zeros, what
    Trainer(audio_drop_prob=...) trains on) -- and steps on eps_u + w (eps_c - eps_u),
    std-rescaled per sample by guidance_rescale (Lin et al. 2023; 0 = off).  w == 1 is the
    unguided path, unchanged.

    known / keep: masked sampling (inpainting, continuation).  `known` is a clip of `shape`,
    `keep` a mask over its frames and pixels (schedulers.keep_mask; _masked_start for the
    accepted shapes): where keep is 1 the result is the known clip -- the returned x0 and sample
    equal it there -- where it is 0 the model generates, conditioned on the kept part through
    its own receptive field, and in between the step kernel blends the two x0.  The kept part is
    replaced inside the step kernel at every step (ops.ddim_step), eager and replayed alike;
    eta must be 0 for the kept part to stay exact.  The same keywords on sample_dpm and
    sample_long."""
    with ops.frozen_weights():
        return _sample(model, sampler, False, cond, audio, shape, generator, callback,
                       float(guidance_scale), float(guidance_rescale), known=known, keep=keep)


@_mask_options
@torch.no_grad()
def sample_dpm(model, sampler, cond, audio, shape, generator=None, callback=None,
               guidance_scale=1.0, guidance_rescale=0.0, *, known=None, keep=None):
    """DPM-Solver++(2M) sampling (schedulers.DPMSolverSampler) with sample_ddim's contract:
    audio encoded once, packed conv weights reused across the steps, callback(i, xt, x0) at
    every step, classifier-free audio guidance as one forward at batch 2B, and on a GPU one
    replayed graph (DPMGraph; VDIFF_DDIM_GRAPH=0 selects the eager loop, which launches the same
    kernels on the same operands).  known / keep: masked sampling as in sample_ddim; the x0
    history holds the known clip where keep is 1."""
    with ops.frozen_weights():
        return _sample(model, sampler, True, cond, audio, shape, generator, callback,
                       float(guidance_scale), float(guidance_rescale), known=known, keep=keep)


@_mask_options
@torch.no_grad()
def sample_long(model, sampler, cond, audio, shape, window, stride=None, blend="triangle",
                window_batch=None, generator=None, callback=None, guidance_scale=1.0,
                guidance_rescale=0.0, *, known=None, keep=None):
    """Sampling of a clip longer than the denoiser's window, with sample_ddim's contract:
    returns (x_T_end, x0) of `shape` = (B, 3, L, H, W); `sampler` a DDIMSampler or a
    DPMSolverSampler (TypeError otherwise); `audio` the L frames' windows or encoded features.

    At every step the overlapping `window`-frame windows of the long latent (schedulers.
    WindowPlan(L, window, stride, blend)) are denoised as one batched forward -- at most
    `window_batch` windows at a time; None: all of them -- their predictions are blended where
    they overlap with the plan's fixed weights, and the long latent is stepped once by the
    sampler's rule in the step kernel, so guidance, its std-rescale over the whole clip,
    v-prediction and the DPM-Solver++ history work as they do for a short clip.  The audio is
    encoded once for
    the L frames and routed to the windows before the loop.  On a GPU one step is captured and
    replayed (LongDDIMGraph / LongDPMGraph; VDIFF_DDIM_GRAPH=0 selects the eager loop, which
    launches the same kernels on the same operands).  L == window is one window: sample_ddim /
    sample_dpm run as they are.

    known / keep: masked sampling as in sample_ddim, on the long latent (the step kernel sees
    it, not the windows): known is [B, 3, L, H, W]-shaped and keep covers the L frames.
    Continuing a clip from its first K frames is keep = schedulers.keep_mask(L, H, W,
    generate_box=(0, 1, 0, 1), keep_frames=K) with those frames filled into `known`."""
    if not isinstance(sampler, (DDIMSampler, DPMSolverSampler)):
        raise TypeError(f"sample_long: sampler must be a DDIMSampler or a DPMSolverSampler, "
                        f"got {type(sampler).__name__}")
    if len(shape) != 5:
        raise ValueError(f"sample_long: shape {tuple(shape)} is not (B, 3, L, H, W)")
    plan = WindowPlan(shape[2], window, stride, blend)
    if window_batch is not None and int(window_batch) < 1:
        raise ValueError(f"sample_long: window_batch {window_batch} < 1")
    dpm = isinstance(sampler, DPMSolverSampler)
    if plan.num_windows == 1:
        return (sample_dpm if dpm else sample_ddim)(
            model, sampler, cond, audio, shape, generator=generator, callback=callback,
            guidance_scale=guidance_scale, guidance_rescale=guidance_rescale, known=known,
            keep=keep)
    with ops.frozen_weights():
        return _sample(model, sampler, dpm, cond, audio, shape, generator, callback,
                       float(guidance_scale), float(guidance_rescale), plan, window_batch,
                       known, keep)


# ------------------------------------------------------------------ ancestral DDPM
@torch.no_grad()
def sample_ddpm(model, scheduler, cond, audio, shape, n_timesteps=None, generator=None,
                callback=None, guidance_scale=1.0, guidance_rescale=0.0, prediction="eps"):
    """Ancestral sampling as test.py:51-83 (V2 scheduler by default there).  guidance_scale !=
    1: classifier-free audio guidance as in sample_ddim; the guided noise (ops.cfg_combine) is
    the eps of the scheduler's p_sample kernel.  prediction="v": the model's (guided) output is
    v, and eps = sqrt_1m_acp[t] xt + sqrt_acp[t] v is formed by one extra launch per step --
    ops.q_sample(v, xt, t, ...) on the scheduler's own tables -- before the unchanged p_sample
    kernel."""
    ops.prediction_id(prediction)
    with ops.frozen_weights():
        return _sample_ddpm(model, scheduler, cond, audio, shape, n_timesteps, generator,
                            callback, float(guidance_scale), float(guidance_rescale), prediction)


def v_to_eps(scheduler, v, xt, t):
    """eps = sqrt_1m_acp[t] xt + sqrt_acp[t] v of a v-prediction model's output, in xt's dtype:
    vd_q_sample with v in x0's place and xt in the noise's."""
    sa, s1m = _v_tables(scheduler, xt.device)
    return ops.q_sample(v.contiguous().to(xt.dtype), xt.contiguous(), t, sa, s1m)


def _v_tables(scheduler, device):
    cache = scheduler.__dict__.setdefault("_v_tables_dev", {})
    key = str(device)
    if key not in cache:
        cache[key] = tuple(v.to(device) for v in _sqrt_tables(scheduler))
    return cache[key]


def _sample_ddpm(model, scheduler, cond, audio, shape, n_timesteps, generator, callback,
                 scale=1.0, rescale=0.0, prediction="eps"):
    model.eval()
    device = cond.device
    feats = _encode(model, audio)
    n = n_timesteps or scheduler.num_timesteps
    xt = torch.randn(shape, generator=generator, device=device)
    x0 = None
    if scale != 1.0:
        cond2, feats2 = _doubled(cond, feats)
    for i in reversed(range(n)):
        t = torch.full((shape[0],), i, dtype=torch.int64, device=device)
        if scale != 1.0:
            eps_c, eps_u = model(torch.cat([xt, xt]), cond2, feats2, torch.cat([t, t])).chunk(2)
            eps = ops.cfg_combine(eps_c, eps_u, scale, rescale)
        else:
            eps = model(xt, cond, feats, t)
        if prediction == "v":
            eps = v_to_eps(scheduler, eps, xt, t)
        z = torch.randn(xt.shape, generator=generator, device=device)
        xt, x0 = scheduler.sample_prev_timestep(xt, eps, t, z=z)
        if callback is not None:
            callback(i, xt, x0)
    return xt, x0
