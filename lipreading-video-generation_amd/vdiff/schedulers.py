"""DDPM schedulers with the reference API (linear_noise_scheduler.py, noise_scheduler.py)
plus a DDIM and a DPM-Solver++(2M) sampler, all running on the HIP scheduler kernels, and the
window plan of long-clip sampling (WindowPlan).

The schedule tables are built on the host exactly as the reference builds them (same
torch CPU ops, so they are bit-identical and keep the reference attribute names);
the per-step math runs on the GPU with per-sample timesteps.  Noise `z` may be
injected (tests) or is drawn with torch.randn_like on the tensor's device.
"""
from __future__ import annotations

import functools
import inspect
import math

import torch

from . import ops


class _Tables:
    _dev_cache: dict

    def _dev(self, name, device):
        key = (name, str(device))
        cache = self.__dict__.setdefault("_dev_cache", {})
        if key not in cache:
            cache[key] = getattr(self, name).to(device=device, dtype=torch.float32).contiguous()
        return cache[key]


def _threshold_option(name, dynamic_threshold, threshold_max, clip_x0):
    """The samplers' keyword-only dynamic-thresholding option as the step ops take it: None
    (off) or (p, threshold_max).  Imagen's dynamic thresholding (Saharia et al. 2022, section
    2.3): every step clamps x0 to [-s, s] and divides by s, s = min(max(q, 1), threshold_max)
    with q the sample's p-quantile of |x0| (the "higher" order statistic, an element of the
    data).  It replaces the static clamp, so it excludes clip_x0."""
    if dynamic_threshold is None:
        if threshold_max is not None:
            raise ValueError(f"{name}: threshold_max needs dynamic_threshold")
        return None
    p = float(dynamic_threshold)
    if not 0.0 < p <= 1.0:
        raise ValueError(f"{name}: dynamic_threshold {dynamic_threshold} outside (0, 1]")
    tmax = math.inf if threshold_max is None else float(threshold_max)
    if not tmax >= 1.0:
        raise ValueError(f"{name}: threshold_max {threshold_max} < 1")
    if clip_x0:
        raise ValueError(f"{name}: dynamic_threshold and clip_x0=True exclude each other")
    return p, tmax


def _thresh_kw(sampler):
    """{"thresh": (p, threshold_max)} of a sampler built with dynamic_threshold, else {}: with
    the option off the step ops are called exactly as before."""
    return {} if sampler.thresh is None else {"thresh": sampler.thresh}


def _sqrt_tables(scheduler):
    """(sqrt_acp, sqrt_1m_acp) of a DDPM scheduler as fp32 CPU vectors: the two tables its
    q_sample reads, under either family's attribute names."""
    for names in (("sqrt_alpha_cum_prod", "sqrt_one_minus_alpha_cum_prod"),
                  ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")):
        if all(hasattr(scheduler, n) for n in names):
            return tuple(getattr(scheduler, n).detach().float().cpu().contiguous()
                         for n in names)
    raise ValueError(f"{type(scheduler).__name__} has no sqrt_alpha_cum_prod / "
                     "sqrt_one_minus_alpha_cum_prod tables: a non-default objective and "
                     "v-prediction sampling read them")


class LinearNoiseScheduler(_Tables):
    """linear_noise_scheduler.py:6-76 (DDPM, standard posterior variance)."""

    def __init__(self, num_timesteps, beta_start, beta_end):
        self.num_timesteps = num_timesteps
        self.beta_start = beta_start
        self.beta_end = beta_end
        self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_timesteps) ** 2
        self.alphas = 1. - self.betas
        self.alpha_cum_prod = torch.cumprod(self.alphas, dim=0)
        self.sqrt_alpha_cum_prod = torch.sqrt(self.alpha_cum_prod)
        self.sqrt_one_minus_alpha_cum_prod = torch.sqrt(1 - self.alpha_cum_prod)

    def add_noise(self, original, noise, t):
        """q_sample (linear_noise_scheduler.py:24-46)."""
        d = original.device
        return ops.q_sample(original.contiguous(), noise.contiguous(), t,
                            self._dev("sqrt_alpha_cum_prod", d),
                            self._dev("sqrt_one_minus_alpha_cum_prod", d))

    def sample_prev_timestep(self, xt, noise_pred, t, z=None):
        """p_sample (linear_noise_scheduler.py:48-76); per-sample t, no noise where t == 0."""
        d = xt.device
        xt = xt.contiguous()
        if z is None:
            z = torch.randn_like(xt)
        return ops.p_sample_v1(xt, noise_pred.contiguous().to(xt.dtype), z.contiguous(), t,
                               self._dev("betas", d), self._dev("alphas", d),
                               self._dev("alpha_cum_prod", d),
                               self._dev("sqrt_one_minus_alpha_cum_prod", d))


class LinearNoiseSchedulerV2(LinearNoiseScheduler):
    """linear_noise_scheduler.py:79-101: the sampling schedule used by test.py; keeps the
    reference's non-standard mean xt - sqrt(1-acp) eps / sqrt(alpha) and adds noise at
    every step (also t == 0)."""

    def __init__(self, num_timesteps, beta_start=0.0001, beta_end=0.01):
        super().__init__(num_timesteps, beta_start, beta_end)

    def sample_prev_timestep(self, xt, noise_pred, t, z=None):
        d = xt.device
        xt = xt.contiguous()
        if z is None:
            z = torch.randn_like(xt)
        return ops.p_sample_v2(xt, noise_pred.contiguous().to(xt.dtype), z.contiguous(), t,
                               self._dev("betas", d), self._dev("alphas", d),
                               self._dev("alpha_cum_prod", d), self._dev("sqrt_alpha_cum_prod", d),
                               self._dev("sqrt_one_minus_alpha_cum_prod", d))


class CosineNoiseScheduler(_Tables):
    """noise_scheduler.py:4-29; returns (sampled, mean)."""

    def __init__(self, num_timesteps, s=0.008):
        self.num_timesteps = num_timesteps
        self.s = s
        self.timesteps = torch.arange(num_timesteps, dtype=torch.float32) / num_timesteps
        self.alphas_cumprod = torch.cos(((self.timesteps + self.s) / (1 + self.s)) * math.pi * 0.5) ** 2
        self.sqrt_alphas_cumprod = torch.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = torch.sqrt(1 - self.alphas_cumprod)

    def sample_prev_timestep(self, xt, noise_pred, t, z=None):
        d = xt.device
        xt = xt.contiguous()
        if z is None:
            z = torch.randn_like(xt)
        return ops.p_sample_cosine(xt, noise_pred.contiguous().to(xt.dtype), z.contiguous(), t,
                                   self._dev("alphas_cumprod", d),
                                   self._dev("sqrt_alphas_cumprod", d),
                                   self._dev("sqrt_one_minus_alphas_cumprod", d))


def _mask_options(fn):
    """Marks the keyword-only options known=None, keep=None of masked sampling on fn and keeps
    them out of the signature that introspection reports: the positional parameter lists of the
    samplers' steps, of the sampling functions and of the step graphs are what callers and the
    earlier tests rely on and stay exactly what they were, as _prediction_keyword keeps the
    initialisers'.  fn itself takes the two keywords; fn.__kwdefaults__ names them."""
    sig = inspect.signature(fn)
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("known", "keep"))
    fn.__signature__ = sig.replace(parameters=[p for n, p in sig.parameters.items()
                                               if n not in ("known", "keep")])
    return fn


class DDIMSampler:
    """DDIM (eta = 0: deterministic) over a subsequence of a DDPM schedule's acp table
    (build extension: the reference samples with 500-step DDPM V2, test.py:111).

    steps: number of denoising steps; timesteps = linspace(T-1, 0, steps) rounded.
    prediction: what the denoiser's output is, "eps" (the default) or "v" (v = sqrt(a_t) eps -
    sqrt(1 - a_t) x0, Salimans & Ho 2022): the step kernel then forms x0 = sqrt(a_t) xt -
    sqrt(1 - a_t) v and eps = sqrt(1 - a_t) xt + sqrt(a_t) v itself.  step() and step_guided()
    take the model's output under the name noise_pred / eps_c, eps_u either way.
    dynamic_threshold=p (keyword-only, with threshold_max; default off): dynamic thresholding
    of x0 at every step instead of clip_x0 (_threshold_option).
    """

    def __init__(self, scheduler, steps=50, eta=0.0, clip_x0=False, prediction="eps", *,
                 dynamic_threshold=None, threshold_max=None):
        ops.prediction_id(prediction)  # ValueError on anything but "eps" / "v"
        self.prediction = prediction
        self.thresh = _threshold_option("DDIMSampler", dynamic_threshold, threshold_max, clip_x0)
        acp = getattr(scheduler, "alpha_cum_prod", None)
        if acp is None:
            acp = scheduler.alphas_cumprod
        self.acp = acp.float()
        self.num_train_timesteps = acp.numel()
        self.steps = steps
        self.eta = eta
        self.clip_x0 = clip_x0
        ts = torch.linspace(self.num_train_timesteps - 1, 0, steps).round().long()
        self.timesteps = ts
        self.prev_timesteps = torch.cat([ts[1:], torch.tensor([-1])])
        self._acp_dev = {}

    def _acp(self, device):
        k = str(device)
        if k not in self._acp_dev:
            self._acp_dev[k] = self.acp.to(device).contiguous()
        return self._acp_dev[k]

    def _t_tp(self, xt, i):
        """Step i's timestep and previous timestep, one row per sample of xt."""
        return tuple(torch.full((xt.shape[0],), int(ts[i]), dtype=torch.int64, device=xt.device)
                     for ts in (self.timesteps, self.prev_timesteps))

    @_mask_options
    def step(self, xt, noise_pred, i, z=None, *, known=None, keep=None):
        """One update from self.timesteps[i] to self.prev_timesteps[i]: (x_prev, x0).  known /
        keep: a masked step (ops.ddim_step; keep_mask builds the usual masks)."""
        t, tp = self._t_tp(xt, i)
        if self.eta > 0 and z is None:
            z = torch.randn_like(xt)
        return ops.ddim_step(xt.contiguous(), noise_pred.contiguous().to(xt.dtype), t, tp,
                             self._acp(xt.device), eta=self.eta, z=z, clip=self.clip_x0,
                             prediction=self.prediction, known=known, keep=keep,
                             **_thresh_kw(self))

    @_mask_options
    def step_guided(self, xt, eps_c, eps_u, i, scale, rescale=0.0, z=None, *, known=None,
                    keep=None):
        """step() on the classifier-free guided noise eps_u + scale (eps_c - eps_u), std-rescaled
        by `rescale`: guide, rescale and update in one kernel (ops.ddim_step_cfg)."""
        t, tp = self._t_tp(xt, i)
        if self.eta > 0 and z is None:
            z = torch.randn_like(xt)
        return ops.ddim_step_cfg(xt.contiguous(), eps_c.contiguous().to(xt.dtype),
                                 eps_u.contiguous().to(xt.dtype), t, tp, self._acp(xt.device),
                                 scale, rescale, eta=self.eta, z=z, clip=self.clip_x0,
                                 prediction=self.prediction, known=known, keep=keep,
                                 **_thresh_kw(self))


def keep_mask(T, H, W, *, generate_box=(0.5, 1.0, 0.0, 1.0), keep_frames=0, feather=0):
    """The keep mask of masked sampling (the `keep` of the samplers and of sample_ddim /
    sample_dpm / sample_long): fp32 [1, 1, T, H, W], 1 where the known clip is kept, 0 where the
    model generates.

    generate_box = (y0, y1, x0, x1), fractions of the height and the width: the rows round(y0 H)
    .. round(y1 H) - 1 and the columns round(x0 W) .. round(x1 W) - 1 are generated, everything
    outside is kept.  The default is the lower half of the frame (the mouth region of a centred
    face).  keep_frames = K: the first K frames are kept whole, whatever the box says; continuing
    a clip from K given frames is generate_box=(0, 1, 0, 1), keep_frames=K.  feather = F > 0: a
    linear ramp just inside the box edges, keep = 1 - (d + 1) / (F + 1) for a pixel d = 0 .. F - 1
    pixels inside the nearest edge of the box that borders kept pixels (an edge on the frame's
    border has no ramp), so the blend of the step kernel fades from the known clip into the
    generated region."""
    T, H, W, K, F = int(T), int(H), int(W), int(keep_frames), int(feather)
    if min(T, H, W) < 1:
        raise ValueError(f"keep_mask: empty clip ({T}, {H}, {W})")
    try:
        y0, y1, x0, x1 = (float(v) for v in generate_box)
    except (TypeError, ValueError):
        raise ValueError(f"keep_mask: generate_box {generate_box!r}: four fractions y0, y1, x0, "
                         "x1") from None
    if not (0.0 <= y0 < y1 <= 1.0 and 0.0 <= x0 < x1 <= 1.0):
        raise ValueError(f"keep_mask: generate_box {generate_box!r} needs 0 <= y0 < y1 <= 1 and "
                         "0 <= x0 < x1 <= 1")
    if not 0 <= K <= T:
        raise ValueError(f"keep_mask: keep_frames {keep_frames} outside [0, {T}]")
    if F < 0:
        raise ValueError(f"keep_mask: feather {feather} < 0")
    r0, r1, c0, c1 = round(y0 * H), round(y1 * H), round(x0 * W), round(x1 * W)
    if r0 >= r1 or c0 >= c1:
        raise ValueError(f"keep_mask: generate_box {generate_box!r} is empty at {H} x {W}")
    big = float(H + W + F)  # an edge on the frame's border: no kept pixel beyond it, no ramp
    rows = torch.arange(H, dtype=torch.float64).view(H, 1)
    cols = torch.arange(W, dtype=torch.float64).view(1, W)
    d = torch.full((H, W), big, dtype=torch.float64)
    if r0 > 0:
        d = torch.minimum(d, rows - r0)
    if r1 < H:
        d = torch.minimum(d, r1 - 1 - rows)
    if c0 > 0:
        d = torch.minimum(d, cols - c0)
    if c1 < W:
        d = torch.minimum(d, c1 - 1 - cols)
    inside = (rows >= r0) & (rows < r1) & (cols >= c0) & (cols < c1)
    ramp = (1.0 - (d + 1.0) / (F + 1.0)).clamp(0.0, 1.0) if F > 0 else torch.zeros_like(d)
    frame = torch.where(inside, ramp, torch.ones_like(d))
    m = frame.view(1, H, W).repeat(T, 1, 1)
    m[:K] = 1.0
    return m.float().view(1, 1, T, H, W)


class WindowPlan:
    """Overlapping temporal windows of a long clip and the fixed weights that blend them
    (sampling.sample_long; vd_window_gather / vd_window_blend): a clip of `length` = L frames is
    covered by W = ceil((L - T) / S) + 1 windows of `window` = T frames that start every
    `stride` = S frames (default T // 2; 1 <= S <= T), starts[w] = min(w S, L - T) -- the last
    window is shifted back so that every window is full length; L == T is one window.

    blend: the profile g[f] of a window's frame f, "triangle" (min(f + 1, T - f): a window
    counts most at its centre, least at its ends) or "uniform" (1).  Frame l of the clip is
    covered by the windows w_0 < w_1 < ... and takes their predictions with the weights
    g[l - starts[w_k]] / sum_j g[l - starts[w_j]], computed in fp64 (self.weights64 [L, KMAX],
    0 in the unused slots) and rounded once to fp32 (self.cover_wgt: the table the kernel reads,
    as DPMSolverSampler.coef64 / coef); a frame covered once has the weight exactly 1.
    self.cover_win [L, KMAX] int32 names the covering windows in ascending order, -1 in the
    unused slots; KMAX = 8, and a plan that covers a frame more often is refused.
    self.frame_index [W * T] int64 is the clip frame of every window frame, starts[w] + f: it
    routes per-frame conditioning (the audio features) to the windows."""

    KMAX = 8  # VD_WINDOW_KMAX
    BLENDS = ("triangle", "uniform")

    def __init__(self, length, window, stride=None, blend="triangle"):
        L, T = int(length), int(window)
        if T < 1:
            raise ValueError(f"WindowPlan: window {window} < 1")
        if L < T:
            raise ValueError(f"WindowPlan: a clip of {length} frames is shorter than the window "
                             f"of {window}")
        S = T // 2 if stride is None else int(stride)
        if stride is None and S < 1:
            S = 1  # T == 1
        if not 1 <= S <= T:
            raise ValueError(f"WindowPlan: stride {stride} outside [1, window = {T}]")
        if blend == "triangle":
            g = [min(f + 1, T - f) for f in range(T)]
        elif blend == "uniform":
            g = [1] * T
        else:
            raise ValueError(f"WindowPlan: blend {blend!r}: 'triangle' or 'uniform'")
        self.length, self.window, self.stride, self.blend = L, T, S, blend
        self.num_windows = W = -(-(L - T) // S) + 1
        starts = [min(w * S, L - T) for w in range(W)]
        cover = [[w for w in range(W) if 0 <= l - starts[w] < T] for l in range(L)]
        self.max_coverage = max(len(c) for c in cover)
        if self.max_coverage > self.KMAX:
            raise ValueError(f"WindowPlan: stride {S} covers a frame with {self.max_coverage} "
                             f"windows of {T} frames, more than {self.KMAX}: use a larger stride")
        self.starts = torch.tensor(starts, dtype=torch.int32)
        self.cover_win = torch.full((L, self.KMAX), -1, dtype=torch.int32)
        self.weights64 = torch.zeros((L, self.KMAX), dtype=torch.float64)
        for l, ws in enumerate(cover):
            gs = torch.tensor([g[l - starts[w]] for w in ws], dtype=torch.float64)
            self.cover_win[l, :len(ws)] = torch.tensor(ws, dtype=torch.int32)
            self.weights64[l, :len(ws)] = gs / gs.sum()
        self.cover_wgt = self.weights64.float()
        self.frame_index = (self.starts.long().view(W, 1) + torch.arange(T).view(1, T)).reshape(-1)
        self._dev = {}

    def _tables(self, device):
        """(starts, cover_win, cover_wgt) on the device: the tables the kernels read."""
        k = str(device)
        if k not in self._dev:
            self._dev[k] = tuple(t.to(device).contiguous()
                                 for t in (self.starts, self.cover_win, self.cover_wgt))
        return self._dev[k]


def _prediction_keyword(init):
    """Gives a sampler's initialiser the keyword-only option prediction="eps" | "v": checked
    and stored as self.prediction before the initialiser runs.  The positional parameters, which
    callers and the 2M tests rely on, stay exactly the initialiser's own (functools.wraps: that
    is also the signature introspection reports)."""
    @functools.wraps(init)
    def with_prediction(self, *args, prediction="eps", dynamic_threshold=None,
                        threshold_max=None, **kw):
        ops.prediction_id(prediction)  # ValueError on anything but "eps" / "v"
        self.prediction = prediction
        init(self, *args, **kw)
        # keyword-only as prediction is; checked against the clip_x0 the initialiser stored
        self.thresh = _threshold_option(type(self).__name__, dynamic_threshold, threshold_max,
                                        self.clip_x0)
    return with_prediction


class DPMSolverSampler:
    """DPM-Solver++(2M) (Lu et al. 2022): a deterministic second-order multistep sampler over a
    subsequence of a DDPM schedule's acp table.  It reuses the previous step's x0 prediction
    instead of a second forward, so a step costs what a DDIM step costs.  This is diffusers'
    DPMSolverMultistepScheduler with algorithm_type="dpmsolver++", solver_type="midpoint",
    lower_order_final=True and a zero final sigma, for prediction_type "epsilon" (the default)
    or "v_prediction" (prediction="v"), and with diffusers' thresholding=True as
    dynamic_threshold=p (keyword-only, with threshold_max; _threshold_option): x0 is clamped to
    [-s, s] and divided by s before it enters x_prev and the history, s from the "higher" order
    statistic where diffusers interpolates linearly.  Not here: the stochastic (SDE) variants,
    third-order and singlestep solvers and x0-prediction.

    With alpha = sqrt(a), sigma = sqrt(1 - a), lambda = log(alpha / sigma), h = lambda_prev -
    lambda_t and k = -alpha_prev expm1(-h), a step is

        x0 = (xt - sigma_t eps) / alpha_t          (clamped to [-1, 1] if clip_x0)
        x_prev = A xt + B x0 + C x0_last

    first order (row 0, and every row with order=1): A = sigma_prev / sigma_t, B = k, C = 0 --
    the DDIM update; second order, r = (lambda_t - lambda_last) / h: B = k (1 + 1 / (2 r)), C =
    -k / (2 r); last row (t_prev = -1: a = 1, sigma = 0): A = 0, B = 1, C = 0, x_prev = x0.
    self.coef64 holds the rows [alpha_t, sigma_t, A, B, C, 0, 0, 0] in fp64, self.coef the same
    rounded once to fp32: the table the kernel reads.

    prediction="v" (the denoiser predicts v = alpha_t eps - sigma_t x0, Salimans & Ho 2022)
    needs no other kernel: x0 = alpha_t xt - sigma_t v = (xt - (sigma_t / alpha_t) v) / (1 /
    alpha_t), so columns 0 and 1 of the rows hold 1 / alpha_t and sigma_t / alpha_t instead
    (coef64 in fp64, coef rounded once from it) and vd_dpm_step / vd_dpm_step_cfg do the rest
    on the model's v, guided or not, eager or replayed; A, B and C do not depend on the
    parameterisation and keep their bits.  The guide and the std-rescale then act on v, as Lin
    et al. 2023 define the rescale.

    spacing: "logsnr" (default) picks the timesteps nearest to `steps` values of lambda spread
    uniformly from lambda[T-1] to lambda[0] (lowest index on a tie, duplicates dropped, so
    self.steps may be smaller than asked for); "linspace" is DDIMSampler's rule.  On linspace
    timesteps the last steps span a huge lambda interval and the second order buys nothing below
    about 20 steps.

    The sampler keeps no history: step() takes the previous step's x0 and returns this one's.
    """

    @_prediction_keyword
    def __init__(self, scheduler, steps=20, order=2, spacing="logsnr", clip_x0=False):
        prediction = self.prediction  # keyword-only, validated and stored by the decorator
        acp = getattr(scheduler, "alpha_cum_prod", None)
        if acp is None:
            acp = scheduler.alphas_cumprod
        if steps < 1:
            raise ValueError(f"DPMSolverSampler: steps {steps} < 1")
        if order not in (1, 2):
            raise ValueError(f"DPMSolverSampler: order {order} not in (1, 2)")
        self.acp = acp.float()
        self.num_train_timesteps = T = acp.numel()
        self.order = order
        self.spacing = spacing
        self.clip_x0 = clip_x0
        a = self.acp.double()
        if spacing == "linspace":
            ts = torch.linspace(T - 1, 0, steps).round().long()
        elif spacing == "logsnr":
            if not bool(((a > 0) & (a < 1)).all()):
                raise ValueError("DPMSolverSampler: cumulative alphas outside (0, 1)")
            lam = 0.5 * torch.log(a / (1 - a))
            targets = torch.linspace(float(lam[T - 1]), float(lam[0]), steps, dtype=torch.float64)
            # argmin returns the lowest index among equal distances
            idx = (lam.view(1, -1) - targets.view(-1, 1)).abs().argmin(dim=1)
            ts = torch.unique(idx).flip(0)  # unique sorts ascending
        else:
            raise ValueError(f"DPMSolverSampler: unknown spacing {spacing!r}")
        at = a[ts]
        if not bool(((at > 0) & (at < 1)).all()):
            raise ValueError("DPMSolverSampler: a selected cumulative alpha is outside (0, 1)")
        self.timesteps = ts
        self.prev_timesteps = torch.cat([ts[1:], torch.tensor([-1])])
        self.steps = n = ts.numel()
        alpha, sigma = at.sqrt(), (1 - at).sqrt()
        lam = torch.log(alpha / sigma)
        coef = torch.zeros((n, 8), dtype=torch.float64)
        coef[:, 0], coef[:, 1] = alpha, sigma
        for i in range(n - 1):
            h = lam[i + 1] - lam[i]
            k = -alpha[i + 1] * torch.expm1(-h)
            coef[i, 2] = sigma[i + 1] / sigma[i]
            if order == 2 and i > 0:
                r = (lam[i] - lam[i - 1]) / h
                coef[i, 3], coef[i, 4] = k * (1 + 1 / (2 * r)), -k / (2 * r)
            else:
                coef[i, 3] = k
        coef[n - 1, 3] = 1.0
        if prediction == "v":
            # the kernel's (xt - c1 out) / c0 with c0 = 1 / alpha, c1 = sigma / alpha is
            # alpha xt - sigma v: the x0 of a v-prediction model (class docstring)
            coef[:, 0], coef[:, 1] = 1.0 / alpha, sigma / alpha
        self.coef64 = coef
        self.coef = coef.float()
        self._dev = {}

    def _tables(self, device):
        """(coef, arange(steps)) on the device: the kernel takes its row index from there."""
        k = str(device)
        if k not in self._dev:
            self._dev[k] = (self.coef.to(device).contiguous(),
                            torch.arange(self.steps, dtype=torch.int64, device=device))
        return self._dev[k]

    def _row(self, xt, i, x0_last):
        """What step i's kernel reads besides xt and the model's output: (x0 history buffer,
        coefficient table, device index of row i).  Without x0_last the buffer is new and
        uninitialised, which only a row that does not read it (C == 0) may have."""
        i = int(i)
        if not 0 <= i < self.steps:
            raise IndexError(f"DPMSolverSampler: step {i} outside [0, {self.steps})")
        if x0_last is None:
            if float(self.coef[i, 4]) != 0.0:
                raise ValueError(f"DPMSolverSampler: step {i} is a second-order row and needs "
                                 "x0_last, the x0 that step i - 1 returned")
            x0_last = torch.empty_like(xt, memory_format=torch.contiguous_format)
        coef, idx = self._tables(xt.device)
        return x0_last, coef, idx[i:i + 1]

    @_mask_options
    def step(self, xt, noise_pred, i, x0_last=None, *, known=None, keep=None):
        """One update from self.timesteps[i] to self.prev_timesteps[i]: (x_prev, x0).  x0_last:
        the x0 that step i - 1 returned; it is overwritten in place with this step's x0 and
        returned.  None is allowed where the row does not read it (C == 0).  known / keep: a
        masked step (ops.dpm_step)."""
        hist, coef, idx = self._row(xt, i, x0_last)
        return ops.dpm_step(xt.contiguous(), noise_pred.contiguous().to(xt.dtype), hist, coef,
                            idx, clip=self.clip_x0, known=known, keep=keep, **_thresh_kw(self))

    @_mask_options
    def step_guided(self, xt, eps_c, eps_u, i, scale, rescale=0.0, x0_last=None, *, known=None,
                    keep=None):
        """step() on the classifier-free guided noise eps_u + scale (eps_c - eps_u), std-rescaled
        by `rescale`: guide, rescale and update in one kernel (ops.dpm_step_cfg)."""
        hist, coef, idx = self._row(xt, i, x0_last)
        return ops.dpm_step_cfg(xt.contiguous(), eps_c.contiguous().to(xt.dtype),
                                eps_u.contiguous().to(xt.dtype), hist, coef, idx, scale,
                                rescale, clip=self.clip_x0, known=known, keep=keep,
                                **_thresh_kw(self))
