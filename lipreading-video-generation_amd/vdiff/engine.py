"""Training step around the drop-in model (the loop of the reference train.py:107-134), plus
synthetic clip generation.  The samplers live in vdiff.sampling; their public names are
re-exported here.

Differences from the reference loop (all deliberate):
  * t ~ U{0, ..., num_timesteps-1}: the reference draws randint(0, 500) against a
    100-step schedule (train.py:125) and crashes;
  * gradients are averaged across ranks by vdiff.ddp.GradBucketer (world > 1).
"""
from __future__ import annotations

import contextlib
import math
import os
import weakref
from dataclasses import dataclass

import torch

from . import hipgraph, ops
from .ddp import GradBucketer
from .sampling import (DDIMGraph, DPMGraph, GraphUnsafe, LongDDIMGraph,  # noqa: F401
                       LongDPMGraph, WindowedDenoiser, sample_ddim, sample_ddpm, sample_dpm,
                       sample_long, v_to_eps)
from .schedulers import _sqrt_tables


@dataclass
class Clip:
    """One synthetic minibatch: target frames, reference image, audio windows, noise, t."""
    x0: torch.Tensor      # [B, 3, T, H, W] (or [B, 3, H, W])
    cond: torch.Tensor    # [B, 3, H, W]
    audio: dict           # {'input_values': [B*T, samples]}
    eps: torch.Tensor     # like x0
    t: torch.Tensor       # [B] int64


def synthetic_clip(batch, frames, size, num_timesteps, device, seed=0, samples=4000,
                   dims=3) -> Clip:
    """Seeded synthetic inputs: x0, cond ~ U[-1, 1]; eps ~ N(0, 1);
    audio ~ N(0, 1) [B*T, 4000]; t ~ U{0..N-1}.  Generated on the device."""
    g = torch.Generator(device=device).manual_seed(seed)
    shape = (batch, 3, frames, size, size) if dims == 3 else (batch, 3, size, size)
    x0 = torch.rand(shape, generator=g, device=device) * 2 - 1
    cond = torch.rand((batch, 3, size, size), generator=g, device=device) * 2 - 1
    eps = torch.randn(shape, generator=g, device=device)
    nwin = batch * (frames if dims == 3 else 1)
    audio = {"input_values": torch.randn((nwin, samples), generator=g, device=device)}
    t = torch.randint(0, num_timesteps, (batch,), generator=g, device=device)
    return Clip(x0, cond, audio, eps, t)


def reinit_nonzero(model, seed=1234, std=0.02):
    """Product-side deterministic init for benchmarks / smoke runs: the reference's
    zero_module layers (unet.py:222-224, 306, 627) would make the denoiser output 0."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.startswith("audio_encoder."):
                continue
            if p.dim() >= 2 and float(p.detach().abs().max()) == 0.0:
                fan_in = math.prod(p.shape[1:])
                p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(fan_in))
            elif p.dim() == 1 and float(p.detach().abs().max()) == 0.0 and name.endswith("bias"):
                p.copy_(std * torch.randn(p.shape, generator=g))
    return model


def audio_keep_mask(batch, p, device, generator=None):
    """Per-clip audio keep mask for conditioning dropout: float [batch], 0 with probability p
    (the clip trains on the null audio), else 1.  Drawn on `device` (the generator's device),
    no host sync.  p = 0 keeps every clip, p = 1 drops every clip."""
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"audio_drop_prob {p} outside [0, 1]")
    u = torch.rand((batch,), generator=generator, device=device)
    return (u >= p).to(torch.float32)


class Trainer:
    """q_sample -> denoiser -> MSE(eps_pred, eps) -> backward -> all-reduce -> Adam.

    train.py:102-103: Adam(model.parameters(), lr=1e-2), MSELoss."""

    def __init__(self, model, scheduler, lr=1e-2, bucket_mb=25.0, fused_adam=True,
                 check_every=50, batch_pack=True, graph=False, loss_fn=None,
                 audio_drop_prob=0.0, drop_generator=None, ema_rates=(), ema_warmup=False,
                 clip_grad_norm=None, optimizer="torch", weight_decay=0.0,
                 decoupled_weight_decay=True, lr_warmup=0, lr_schedule="constant",
                 lr_total_steps=None, lr_min_ratio=0.0, skip_bad_steps=0, prediction="eps",
                 loss_weighting="none", snr_gamma=5.0, objective_fn=None):
        """prediction, loss_weighting, snr_gamma: the training objective.  The defaults ("eps",
        "none") are the reference's: the model predicts the noise and the loss is loss_fn(pred,
        eps), ops.mse_loss, exactly as before.  prediction="v" trains the model on v =
        sqrt_acp[t] eps - sqrt_1m_acp[t] x0 (Salimans & Ho 2022); loss_weighting="min-snr"
        weighs each sample by min(snr, snr_gamma) / snr (eps) or / (snr + 1) (v), snr =
        (sqrt_acp[t] / sqrt_1m_acp[t])^2 (Hang et al. 2023).  Either one replaces the loss by
        ops.diffusion_loss(pred, x0, eps, t, ...) (vd_diffusion_loss: fixed-order, no host
        sync, graph-safe) on the scheduler's own q_sample tables, eagerly and inside
        TrainStepGraph; self.loss_per_sample is then the last step's unweighted per-sample MSE
        (a [B] device view, rewritten by the next step; None on the default path).  A loss_fn
        cannot be combined with them (ValueError), and the weighting refuses a schedule with a
        table entry sqrt_acp == 0 or sqrt_1m_acp == 0 (an infinite or zero snr).
        objective_fn: (pred, x0, eps, t) -> (loss, per-sample MSE) used in place of
        ops.diffusion_loss for a non-default objective: host-logic tests on CPU pass a torch
        restatement (the product op refuses CPU tensors).
        check_every: the loss finiteness flag (kept on the device, updated every step) is
        read on the host every `check_every` steps and by check_finite(); a non-finite
        loss raises FloatingPointError naming the first bad step.  0 disables it.
        batch_pack: re-pack the conv operands once per step in one launch
        (ops.step_packed_weights) instead of per conv call.
        graph: replay the denoiser's forward + backward as one HIP graph (TrainStepGraph);
        one process only.
        loss_fn: (pred, eps) -> scalar loss; default ops.mse_loss (vd_mse_loss, fixed-order).
        Host-logic tests on CPU pass torch's F.mse_loss (the product ops refuse CPU tensors).
        audio_drop_prob: share of the clips that train on the null audio (zero features), the
        unconditional half of classifier-free guidance; the model must take `audio_keep`
        (UNetAudio).  0: no mask is drawn and the model is called as before.
        drop_generator: torch.Generator (on the clips' device) of the keep masks.
        ema_rates: decay rates (at most 4) of the weight averages kept in self.ema (vdiff.ema.EMA,
        None for the empty default); all of them are updated by one launch after each optimizer
        step, on every path (eager, graph=True, DDP -- each rank keeps its own, identical, copy).
        The launch reads the first-bad-step record on the device and changes nothing from the
        first non-finite loss on, so the averages stay clean until check_finite() raises; with
        check_every=0 there is no record and no such guard.  Under DDP the record is this
        rank's own loss.
        ema_warmup: decay min(rate, (1 + n) / (10 + n)) after n updates.
        clip_grad_norm: None (off: no clipper, no launch, grad_norm is None) or a number > 0, the
        global L2 norm the step's gradients are clipped to before the optimizer step
        (vdiff.clip.GradClipper: three launches, fixed summation order, no host sync); inf
        measures the norm and scales nothing.  Under DDP the averaged gradients are clipped,
        identically on every rank; in one process a parameter without a gradient is left out.
        The pre-clip norm and the factor stay on the device (grad_norm, clip_coef).  A
        non-finite norm scales nothing and counts as a bad step like a non-finite loss: it
        enters the first-bad-step record, check_finite() names it and the EMA guard holds from
        that step on.  The optimizer step itself is NOT prevented (fail-fast, as for the loss):
        the weights of that step are lost, the record says when.
        optimizer: "torch" (the default: torch.optim.Adam at the constant rate lr, exactly as
        before) or "hip" (vdiff.optim.FusedAdamW: two launches per step, the schedule and the
        bad-step decision on the device).  The seven options below need "hip"; a non-default
        value with "torch" raises ValueError.
        weight_decay, decoupled_weight_decay: AdamW's decay (True) or Adam's L2 (False).
        lr_warmup, lr_schedule, lr_total_steps, lr_min_ratio: linear warm-up over lr_warmup
        steps, then "constant", or "cosine" / "linear" decay to lr_min_ratio * lr at
        lr_total_steps.  The position is the device count of APPLIED steps; self.lr is the rate
        of the last step (0-dim device view).
        skip_bad_steps: K > 0 makes a step whose loss (one process) or gradient norm (with
        clip_grad_norm, any world size) is non-finite a SKIPPED step: the kernels write nothing,
        so weights, moments and counts keep their bits, and the EMA holds still for that step
        only.  The sticky first-bad-step record is not written; self.skipped_steps counts (0-dim
        device view).  More than K skipped steps in a row trip the optimizer -- every later step
        is skipped too, the weights stay those of the last good step -- and check_finite()
        raises FloatingPointError naming the step.  Under DDP the decision must be identical on
        every rank, so only the norm of the averaged gradients decides (bit-identical
        everywhere; a rank-local loss would let the ranks diverge): clip_grad_norm is required
        there.  Without clip_grad_norm (inf measures only) nothing guards against a non-finite
        gradient behind a finite loss.  K = 0 keeps the fail-fast record above exactly."""
        if not 0.0 <= audio_drop_prob <= 1.0:
            raise ValueError(f"audio_drop_prob {audio_drop_prob} outside [0, 1]")
        self.audio_drop_prob = float(audio_drop_prob)
        self.drop_generator = drop_generator
        self.model = model
        self.clipper = None
        if clip_grad_norm is not None:
            from .clip import GradClipper, check_max_norm
            self.clipper = GradClipper(check_max_norm(clip_grad_norm, "clip_grad_norm"))
        self._bad_grad = None  # device bool: the first bad step had a finite loss (bad norm)
        ops.prediction_id(prediction)
        ops.weighting_id(loss_weighting)
        if not (isinstance(snr_gamma, (int, float)) and snr_gamma > 0
                and math.isfinite(snr_gamma)):
            raise ValueError(f"snr_gamma {snr_gamma!r} is not a positive finite number")
        self.prediction, self.loss_weighting = prediction, loss_weighting
        self.snr_gamma = float(snr_gamma)
        # None: the default objective, which runs loss_fn(pred, eps) exactly as before
        self.objective = None
        self.loss_per_sample = None
        if (prediction, loss_weighting) != ("eps", "none"):
            if loss_fn is not None:
                raise ValueError(f"Trainer(loss_fn=...) is the loss of the default objective "
                                 f"only; prediction={prediction!r}, loss_weighting="
                                 f"{loss_weighting!r} compute their own (objective_fn replaces "
                                 "it in CPU tests)")
            sa, s1m = _sqrt_tables(scheduler)
            if loss_weighting != "none":
                bad = ((sa == 0) | (s1m == 0)).nonzero().flatten()
                if bad.numel():
                    i = int(bad[0])
                    raise ValueError(
                        f"loss_weighting={loss_weighting!r}: schedule entry {i} of "
                        f"{sa.numel()} has sqrt_acp = {float(sa[i])!r}, sqrt_1m_acp = "
                        f"{float(s1m[i])!r} in fp32; the signal-to-noise ratio there is "
                        "infinite or zero and has no weight")
            self.objective = (sa, s1m)
        elif objective_fn is not None:
            raise ValueError("Trainer(objective_fn=...) stands in for ops.diffusion_loss and "
                             "needs a non-default prediction or loss_weighting")
        self.objective_fn = objective_fn
        self._objective_dev = {}
        self.loss_fn = loss_fn or ops.mse_loss
        self.scheduler = scheduler
        self.check_every = int(check_every)
        self.steps_done = 0
        self._first_bad = None  # device int64: first step with a non-finite loss, or -1
        self._named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        params = [p for p in model.parameters() if p.requires_grad]
        # one process: no all-reduce, so no bucket views -- autograd hands each gradient over
        # without the accumulate-into-view add, and zero_grad drops them (no fills)
        distributed = torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1
        if (optimizer == "hip" and distributed and self.clipper is None
                and isinstance(skip_bad_steps, int) and skip_bad_steps > 0):
            raise ValueError("Trainer(skip_bad_steps > 0) under DDP needs clip_grad_norm "
                             "(inf measures only): the ranks must take the same decision, and "
                             "only the averaged gradients' norm is identical on all of them")
        self.bucketer = GradBucketer(params, bucket_mb) if distributed else None
        if optimizer not in ("torch", "hip"):
            raise ValueError(f"optimizer {optimizer!r}: 'torch' or 'hip'")
        self.hip_opt = optimizer == "hip"
        self.skip_bad_steps = 0
        if self.hip_opt:
            from .optim import FusedAdamW
            self.opt = FusedAdamW(params, lr=lr, weight_decay=weight_decay,
                                  decoupled=decoupled_weight_decay, warmup_steps=lr_warmup,
                                  schedule=lr_schedule, total_steps=lr_total_steps,
                                  min_ratio=lr_min_ratio, max_bad_run=skip_bad_steps)
            self.skip_bad_steps = int(skip_bad_steps)
        else:
            given = dict(weight_decay=(weight_decay, 0.0),
                         decoupled_weight_decay=(decoupled_weight_decay, True),
                         lr_warmup=(lr_warmup, 0), lr_schedule=(lr_schedule, "constant"),
                         lr_total_steps=(lr_total_steps, None), lr_min_ratio=(lr_min_ratio, 0.0),
                         skip_bad_steps=(skip_bad_steps, 0))
            extra = [k for k, (v, d) in given.items() if v != d]
            if extra:
                raise ValueError(f"Trainer({', '.join(extra)}) needs optimizer='hip' "
                                 "(torch.optim.Adam runs at a constant rate without decay)")
            kw = {"fused": True} if fused_adam and params and params[0].is_cuda else {}
            self.opt = torch.optim.Adam(params, lr=lr, **kw)
        # conv operands re-packed once per step in one launch (ops.step_packed_weights)
        self.packs = ops.step_packed_weights() if batch_pack else contextlib.nullcontext()
        if graph and self.bucketer is not None:
            raise ValueError("Trainer(graph=True) is single-process (the gradient buckets are "
                             "launched from autograd hooks)")
        if graph and not batch_pack:
            raise ValueError("Trainer(graph=True) needs batch_pack (per-call packs would be "
                             "frozen into the graph)")
        if graph and os.environ.get("VDIFF_TRAIN_GRAPH_EXPERIMENTAL") != "1":
            # advisor r03: a known defect must not be one keyword away from a user
            raise RuntimeError("Trainer(graph=True) is opt-in: it measured no gain over the eager "
                               "step (kernel-bound; DESIGN section 9 item 3); set "
                               "VDIFF_TRAIN_GRAPH_EXPERIMENTAL=1 to run it")
        self.graph = TrainStepGraph(self) if graph else None
        self.ema = None
        if len(tuple(ema_rates)):
            from .ema import EMA
            self.ema = EMA(model, ema_rates, warmup=ema_warmup)

    def step(self, clip: Clip) -> torch.Tensor:
        if self.graph is not None:
            return self.graph.step(clip)
        return self._eager_step(clip)

    def audio_keep(self, clip: Clip):
        """This step's keep mask ([B], on the clip's device), or None without dropout."""
        if self.audio_drop_prob <= 0:
            return None
        return audio_keep_mask(clip.x0.shape[0], self.audio_drop_prob, clip.x0.device,
                               self.drop_generator)

    def _eager_step(self, clip: Clip) -> torch.Tensor:
        self.model.train()
        keep = self.audio_keep(clip)
        with self.packs:
            xt = self.scheduler.add_noise(clip.x0, clip.eps, clip.t)
            if keep is None:
                pred = self.model(xt, clip.cond, clip.audio, clip.t)
            else:
                pred = self.model(xt, clip.cond, clip.audio, clip.t, audio_keep=keep)
            loss = self._loss(pred, clip.x0, clip.eps, clip.t)
            loss.backward()
        if self.bucketer is not None:
            self.bucketer.finish()
            self._clip_grads()
            # DDP: the norm only (identical on every rank), never this rank's own loss
            self.bucketer.step(self.opt, **self._opt_args(None))
            self.bucketer.zero_grad()
        else:
            self._clip_grads()
            self.opt.step(**self._opt_args(loss.detach()))
            self.opt.zero_grad(set_to_none=True)
        loss = loss.detach()
        self._track_finite(loss)
        self._update_ema()
        return loss

    def _loss(self, pred, x0, eps, t):
        """The step's loss.  Default objective: loss_fn(pred, eps), as before.  Otherwise
        ops.diffusion_loss (or objective_fn) on the scheduler's q_sample tables, which also
        leaves the per-sample MSE in self.loss_per_sample."""
        if self.objective is None:
            return self.loss_fn(pred, eps)
        if self.objective_fn is not None:
            loss, per = self.objective_fn(pred, x0, eps, t)
        else:
            key = str(pred.device)
            if key not in self._objective_dev:
                self._objective_dev[key] = tuple(
                    v.to(device=pred.device, dtype=torch.float32).contiguous()
                    for v in self.objective)
            sa, s1m = self._objective_dev[key]
            loss, per = ops.diffusion_loss(pred, x0, eps, t, sa, s1m, self.prediction,
                                           self.loss_weighting, self.snr_gamma,
                                           return_per_sample=True)
        self.loss_per_sample = per.detach()
        return loss

    @property
    def grad_norm(self):
        """The last step's global gradient norm before clipping (0-dim device view, rewritten
        by the next step); None without clip_grad_norm."""
        return None if self.clipper is None else self.clipper.norm

    @property
    def clip_coef(self):
        """The last step's clipping factor, 1 where nothing was scaled (0-dim device view)."""
        return None if self.clipper is None else self.clipper.coef

    @property
    def lr(self):
        """The last step's learning rate (0-dim fp32 device view, rewritten by the next step);
        None with optimizer="torch"."""
        return self.opt.lr if self.hip_opt else None

    @property
    def skipped_steps(self):
        """Steps skipped so far (0-dim int64 device view); None with optimizer="torch"."""
        return self.opt.skipped if self.hip_opt else None

    def _opt_args(self, loss):
        """What the optimizer step reads on the device: nothing for torch's Adam; for FusedAdamW
        the loss (None under DDP) and, with a clipper, the gradient norm."""
        if not self.hip_opt:
            return {}
        if loss is not None and loss.dtype != torch.float32:
            loss = loss.float()
        return {"loss": loss, "grad_norm": None if self.clipper is None else self.clipper.norm}

    def _clip_grads(self):
        """After backward (and the gradient average under DDP), before the optimizer step."""
        if self.clipper is None:
            return
        if self.bucketer is not None:
            # the averaged buckets, identical on every rank; a parameter no rank used
            # contributes its zeros, and the flag tail of the last bucket is left out
            flats = list(self.bucketer.grad_flats())
            self.clipper.clip(flats, [f"gradient bucket {i}" for i in range(len(flats))])
            return
        named = [(n, p.grad) for n, p in self._named if p.grad is not None]
        self.clipper.clip([g for _, g in named], [f"the gradient of {n}" for n, _ in named])

    def _update_ema(self):
        """After the optimizer step and this step's entry in the first-bad-step record."""
        if self.ema is not None:
            # skip mode: still on the skipped steps only; else from the first bad step on
            self.ema.update(skip_flag=self.opt.skip_flag if self.skip_bad_steps > 0
                            else self._first_bad)

    def _track_finite(self, loss):
        """SURVEY 5 failure detection without a per-step host sync: a device-side record of
        the first step whose loss is NaN/Inf (the reference skips nothing and checks
        nothing, train.py:111-112), read every check_every steps."""
        if self.check_every <= 0:
            return
        if self.skip_bad_steps > 0:  # the optimizer's device words are the record
            self.steps_done += 1
            if self.steps_done % self.check_every == 0:
                self.check_finite()
            return
        if self._first_bad is None:
            self._first_bad = torch.full((), -1, dtype=torch.int64, device=loss.device)
        bad = ~torch.isfinite(loss)
        if self.clipper is not None and self.clipper.norm is not None:
            # a finite loss with a non-finite gradient (bf16 backward) is a bad step too
            bad_norm = ~torch.isfinite(self.clipper.norm)
            if self._bad_grad is None:
                self._bad_grad = torch.zeros((), dtype=torch.bool, device=loss.device)
            first = (bad | bad_norm) & (self._first_bad < 0)
            self._bad_grad.copy_(torch.where(first, bad_norm & ~bad, self._bad_grad))
            bad = bad | bad_norm
        bad = bad & (self._first_bad < 0)
        self._first_bad.copy_(torch.where(bad, self.steps_done, self._first_bad))
        self.steps_done += 1
        if self.steps_done % self.check_every == 0:
            self.check_finite()

    def check_finite(self):
        """Raise FloatingPointError if any step so far had a non-finite loss (host sync).

        Under DDP (the gradient bucketer active) the first bad step is MIN-all-reduced over
        the ranks first, so a loss that went non-finite on one rank makes EVERY rank raise
        here together instead of leaving the others blocked in the next gradient
        all-reduce (advisor r03).  Every rank reaches this call at the same step count."""
        if self.skip_bad_steps > 0:
            # identical on every rank (the decision reads the averaged gradients' norm only)
            at = int(self.opt.tripped_at)
            if at >= 0:
                raise FloatingPointError(
                    f"more than {self.skip_bad_steps} consecutive steps with a non-finite loss "
                    f"or gradient norm: tripped at step {at} (of {self.steps_done}), "
                    f"{int(self.opt.skipped)} steps skipped; the weights are those of the last "
                    "good step")
            return
        if self._first_bad is None and self.bucketer is None:
            return
        if self._first_bad is None:
            dev = next(self.model.parameters()).device
            self._first_bad = torch.full((), -1, dtype=torch.int64, device=dev)
        fb = self._first_bad
        if self.bucketer is not None:
            big = torch.iinfo(torch.int64).max
            v = torch.where(fb >= 0, fb, torch.full_like(fb, big)).reshape(1)
            if v.is_cuda and torch.distributed.get_backend() == "gloo":
                v = v.cpu()
            torch.distributed.all_reduce(v, op=torch.distributed.ReduceOp.MIN)
            first = int(v[0])
            first = -1 if first == big else first
        else:
            first = int(fb)
        if first >= 0:
            what = "training loss"
            if self._bad_grad is not None and bool(self._bad_grad):
                what = "gradient norm (the loss was finite)"
            raise FloatingPointError(f"non-finite {what} at step {first} "
                                     f"(of {self.steps_done})")


class TrainStepGraph:
    """Trainer.step with the denoiser replayed as one HIP graph (the
    ~600 launch gaps of an eager step).

    Captured: the batched weight pack, q_sample, the conditioning concat and the UNet forward,
    the MSE (vd_mse_loss, whose value step() returns) and the whole backward down to the UNet
    parameters' gradients and the gradient of the pooled audio features.  Eager around it: the wav2vec2 encoder (transformers draws its
    LayerDrop and SpecAugment decisions on the host every step, which changes the launch
    sequence, so it cannot be frozen), its backward (fed the replayed feature gradient) and
    the fused Adam step over all parameters.  Same math as the eager step: the first `warmup`
    steps run eagerly (lazy initialisation, the packed-weight plan), the capture itself does not
    update anything, and the ResBlock dropout draws a new mask per replay through the device
    counter the GroupNorm kernels read (vd_set_dropout_counter).  The UNet parameters' .grad
    tensors live in the graph's memory pool and are overwritten by each replay; they are never
    reset to None."""

    def __init__(self, trainer, warmup=2):
        # a weak reference: Trainer -> TrainStepGraph -> Trainer would be a reference cycle,
        # so a dropped trainer's CUDAGraph would be destroyed by the cyclic collector -- which
        # may run inside a later capture, where ~CUDAGraph's device synchronisation is refused
        # and the process aborts (round 5; DESIGN section 9.3, hipgraph.capture)
        self._tr = weakref.ref(trainer)
        self.warmup = int(warmup)
        self.g = None
        self.steps = 0

    @property
    def tr(self):
        return self._tr()

    def step(self, clip: Clip) -> torch.Tensor:
        tr = self.tr
        if self.steps < self.warmup:
            self.steps += 1
            return tr._eager_step(clip)
        model = tr.model
        model.train()
        enc = model.encode_audio(clip.audio).float()
        if self.g is not None and self._shapes(clip, enc) != self.shapes:
            # a batch of another shape (a short last batch): eager, with every gradient
            # released first so that the eager backward does not accumulate into the graph's
            tr.opt.zero_grad(set_to_none=True)
            self.steps += 1
            return tr._eager_step(clip)
        keep = tr.audio_keep(clip)
        if keep is not None:
            # conditioning dropout, eagerly and before the copy into the static buffer: the
            # graph sees features, never the mask
            from .unet_audio import apply_audio_keep
            enc = apply_audio_keep(enc, keep)
        if self.g is None:
            self._capture(clip, enc)
        for p, g in self.grads:  # (an eager step in between may have released them)
            p.grad = g
        with torch.no_grad():
            for dst, src in ((self.x0, clip.x0), (self.eps, clip.eps), (self.t, clip.t),
                             (self.cond, clip.cond), (self.feats, enc)):
                dst.copy_(src)
        self.g.replay()
        tr.loss_per_sample = self.per  # (an eager step in between left its own there)
        if enc.requires_grad:
            enc.backward(self.feats.grad)
        tr._clip_grads()  # eager, like Adam: the graph's static gradients and the encoder's
        tr.opt.step(**tr._opt_args(self.loss))  # (the replay's loss, read on the device)
        for p in self.eager_params:
            p.grad = None
        self.steps += 1
        loss = self.loss.clone()  # the replay's own MSE (vd_mse_loss, captured)
        tr._track_finite(loss)
        tr._update_ema()  # eager, like Adam: one launch and the count's increment
        return loss

    def node_types(self):
        """{node type: count} of the captured graph (vdiff.hipgraph; memset nodes must be 0)."""
        from .hipgraph import graph_nodes
        nodes = graph_nodes(self.g.raw_cuda_graph())
        return {t: sum(1 for n in nodes if n["type"] == t) for t in {n["type"] for n in nodes}}

    @staticmethod
    def _shapes(clip, enc):
        return tuple((tuple(x.shape), x.dtype) for x in (clip.x0, clip.eps, clip.t, clip.cond, enc))

    def _body(self):
        """The captured region.  The loss is vd_mse_loss (ops.mse_loss), a fixed-order
        two-launch reduction: round 4 found torch's one-launch multi-block mean (per-block
        partials, a semaphore reset by a captured hipMemsetAsync, a last-block combine)
        returning a stale value from some replay on -- the replay's output kept an earlier
        value while every gradient stayed exact -- and round 5 reproduced that with torch alone
        (tools/graph_reduce_repro.py) and saw it vanish under DEBUG_CLR_GRAPH_PACKET_CAPTURE=0
        (DESIGN section 9.3).  The captured step holds no memset node
        (tests/test_gpu_train_graph.py), and step() returns this in-graph value."""
        tr = self.tr
        with tr.packs:
            xt = tr.scheduler.add_noise(self.x0, self.eps, self.t)
            pred = tr.model(xt, self.cond, self.feats, self.t)
            # a non-default objective: vd_diffusion_loss on the static x0 / eps / t buffers,
            # built to the same rules; loss_per_sample then lives in the pool as well
            loss = tr._loss(pred, self.x0, self.eps, self.t)
            self.loss = loss.detach()  # lives in the graph's pool, rewritten by each replay
            loss.backward()

    def _capture(self, clip, enc):
        from . import _lib
        tr, model = self.tr, self.tr.model
        self.x0, self.eps = clip.x0.clone(), clip.eps.clone()
        self.t, self.cond = clip.t.clone(), clip.cond.clone()
        self.feats = enc.detach().clone().requires_grad_(enc.requires_grad)
        enc_ids = {id(p) for p in model.audio_encoder.parameters()} \
            if getattr(model, "audio_encoder", None) is not None else set()
        self.eager_params = [p for p in model.parameters() if p.requires_grad and id(p) in enc_ids]
        self.ctr = torch.zeros((), dtype=torch.int64, device=enc.device)
        tr.opt.zero_grad(set_to_none=True)
        # one run of the region on a side stream before capture (torch's graph recipe: lazy
        # allocator / autograd state), its gradients discarded
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._body()
        torch.cuda.current_stream().wait_stream(side)
        tr.opt.zero_grad(set_to_none=True)
        self.feats.grad = None
        self.g = torch.cuda.CUDAGraph(keep_graph=True)  # node list kept (graph_nodes)
        lib = _lib.lib()
        lib.vd_set_dropout_counter(self.ctr.data_ptr())
        try:
            with hipgraph.capture(self.g, capture_error_mode="thread_local"):
                self.ctr.add_(1)
                self._body()
        finally:
            lib.vd_set_dropout_counter(None)
        self.g.instantiate()
        self.per = tr.loss_per_sample  # None on the default path
        self.shapes = self._shapes(clip, enc)
        tr.packs.frozen = True  # the graph replays the pack launch into these buffers
        self.grads = [(p, p.grad) for p in model.parameters() if p.grad is not None]
        missing = [n for n, p in model.named_parameters()
                   if p.requires_grad and id(p) not in enc_ids and p.grad is None]
        if missing:  # a parameter off the captured path would silently never train
            raise RuntimeError(f"TrainStepGraph: no captured gradient for {missing[:4]}")
