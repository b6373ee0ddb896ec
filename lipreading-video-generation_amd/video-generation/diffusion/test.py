"""Sampling entry point (drop-in for video-generation/diffusion/test.py) on MI355X.

    python test.py [--ckpt model.pth | --random-init] [--sampler ddpm-v2|ddim|dpm++]
                   [--steps 500] [--spacing logsnr|linspace]
                   [--guidance-scale 1.0] [--guidance-rescale 0.0] [--prediction eps|v]
                   [--clip-frames L] [--window-stride S] [--window-blend triangle|uniform]
                   [--window-batch N]
                   [--known clip.npy [--keep-mask mask.npy | --generate-box Y0 Y1 X0 X1
                                      --keep-frames K --mask-feather PX]]
                   [--score] [--score-against truth.npy] [--score-out metrics.json]

Reference API kept (importable without running anything, unlike the reference script):
  * `config` -- the dict of test.py:33-49 (same keys; `ldm_params` may also carry the
    build's `dims` / `frames` / `attention_mode` / `dtype`);
  * `load_model_and_scheduler(config)` -- test.py:86-113: UNetAudio(128, 3, 64, 3, 2,
    (1,2,4), audio_feature_dim=768, projected_audio_dim=128), state_dict from
    config['train_params']['ldm_ckpt_name'], LinearNoiseSchedulerV2(500, 5e-5, 0.015);
  * `sample_images(model, scheduler, img_cond, audio_cond, n_timesteps=500)` --
    test.py:51-83: DDPM-V2 ancestral sampling from N(0, 1) over n_timesteps, x0 saved as
    PNG every 50 steps into lipreading_generated_images/ (plus .npy); returns the final x0
    (the reference returns None).

Deliberate differences: no nn.DataParallel wrapper (test.py:101; multi-GPU sampling runs
one process per GPU) and no per-step torch.cuda.empty_cache() (test.py:58); the audio is
encoded once per clip, not at every step.  A reference checkpoint carries the wav2vec2
weights (train.py:137 saves the whole UNetAudio), so with a checkpoint the encoder is built
from its config only; without one the model gets seeded smoke weights and a random
wav2vec2 -- only when asked for (`ldm_ckpt_name` None here, or --random-init).
Conditioning comes from --cond-npz (reference image [3, H, W] and audio [T, 4000]) or is
synthetic (the reference reads a /proj/... dataset item).
"""
import argparse
import os
import warnings

import numpy as np
import torch

import _vdiff_path  # noqa: F401
from vdiff.engine import (reinit_nonzero, sample_ddim, sample_dpm, sample_long, synthetic_clip,
                          v_to_eps)
from vdiff.ops import cfg_combine, frozen_weights
from vdiff.schedulers import keep_mask

from linear_noise_scheduler import LinearNoiseSchedulerV2
from noise_scheduler import DDIMSampler, DPMSolverSampler
from unet_audio import UNetAudio

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

config = {
    "dataset_params": {"im_path": "/path/to/data", "im_size": 128, "im_channels": 3,
                       "frame_rate": 30},
    "ldm_params": {"model_channels": 64, "num_res_blocks": 2, "attention_resolutions": (1, 2, 4),
                   "z_channels": 3},
    # the reference points at a /proj/... checkpoint; None = seeded smoke weights
    "train_params": {"ldm_ckpt_name": None},
}

OUT_DIR = "lipreading_generated_images"


def _strip_module(sd):
    """Accept checkpoints saved from an nn.DataParallel wrapper ("module." keys)."""
    if sd and all(k.startswith("module.") for k in sd):
        return {k[len("module."):]: v for k, v in sd.items()}
    return sd


def load_model_and_scheduler(config, *, seed=0):
    """test.py:86-113."""
    lp = config["ldm_params"]
    ckpt = config["train_params"].get("ldm_ckpt_name")
    model = UNetAudio(
        image_size=config["dataset_params"]["im_size"],
        in_channels=lp["z_channels"],
        model_channels=lp["model_channels"],
        out_channels=config["dataset_params"]["im_channels"],
        num_res_blocks=lp["num_res_blocks"],
        attention_resolutions=lp["attention_resolutions"],
        audio_feature_dim=768,
        projected_audio_dim=128,
        dims=lp.get("dims", 2),
        attention_mode=lp.get("attention_mode", "joint"),
        use_bf16=lp.get("dtype", "bf16") == "bf16",
        audio_attention=lp.get("audio_attention", False),
        use_scale_shift_norm=lp.get("use_scale_shift_norm", False),
        # with a checkpoint the wav2vec2 weights come from it; without one the random
        # encoder is the explicitly requested smoke mode
        audio_encoder_pretrained=False)
    if ckpt:
        sd = torch.load(ckpt, map_location="cpu", weights_only=True)
        if "model" in sd and "epoch" in sd:  # a train.py resume file: it records the flag
            from train import check_resume_scale_shift_norm
            check_resume_scale_shift_norm(sd, lp.get("use_scale_shift_norm", False))
            sd = sd["model"]
        model.load_state_dict(_strip_module(sd))
    else:
        warnings.warn("test.py: no checkpoint (ldm_ckpt_name is None): seeded smoke weights "
                      "and a random-init wav2vec2")
        reinit_nonzero(model, seed=seed)
    model = model.to(device)
    scheduler = LinearNoiseSchedulerV2(num_timesteps=500, beta_start=0.00005, beta_end=0.015)
    return model, scheduler


def save_frame(x0, path):
    """x0 in [-1, 1] -> (x0 + 1) / 2 as .npy and, for the first frame, .png (test.py:71-81).
    The PNG quantises as transforms.ToPILImage does (mul(255) then truncation to uint8); the
    clamp to [-1, 1] is a documented difference (the reference lets out-of-range values wrap
    in .byte())."""
    ims = ((x0.float().clamp(-1, 1) + 1) / 2).cpu().numpy()
    np.save(path + ".npy", ims)
    try:
        from PIL import Image
        img = ims[0] if ims.ndim == 4 else ims[0][:, 0]
        Image.fromarray((img.transpose(1, 2, 0) * 255).astype(np.uint8)).save(path + ".png")
    except ImportError:
        pass


def _frames_of(model, audio_cond):
    """Frames to generate: 1 for the reference 2-D model; for dims=3 one per audio window."""
    if getattr(model, "dims", 2) != 3:
        return None
    a = audio_cond["input_values"] if isinstance(audio_cond, dict) else audio_cond
    return a.shape[0]


@torch.no_grad()
def sample_images(model, scheduler, img_cond, audio_cond, n_timesteps=500, *, out_dir=OUT_DIR,
                  save_every=50, generator=None, noise=None, max_steps=None, callback=None,
                  guidance_scale=1.0, guidance_rescale=0.0, prediction="eps"):
    """test.py:51-83: reverse process i = n_timesteps-1 .. 0 with
    scheduler.sample_prev_timestep (LinearNoiseSchedulerV2 in test.py), x0 saved every
    `save_every` steps and at i == 0; returns the final x0.

    Keyword-only extensions: `noise(shape)` supplies x_T and each step's z instead of
    torch.randn (injected noise: the trajectory parity tests); `max_steps` stops after that
    many steps; `callback(i, xt, x0)` sees every step's output; `guidance_scale` != 1 samples
    with classifier-free audio guidance (one forward at batch 2, the second row with the null
    audio; `guidance_rescale` is the std-rescale of Lin et al. 2023), for a model trained with
    train.py --audio-drop-prob; `prediction` = "v" for a model trained with train.py
    --prediction v (its output, guided or not, is turned into the noise by one extra launch)."""
    if prediction not in ("eps", "v"):
        raise ValueError(f"prediction {prediction!r}: 'eps' or 'v'")
    model.eval()
    dev = img_cond.device
    S = config["dataset_params"]["im_size"]
    T = _frames_of(model, audio_cond)
    shape = (1, 3, S, S) if T is None else (1, 3, T, S, S)
    os.makedirs(out_dir, exist_ok=True)
    draw = noise or (lambda shp: torch.randn(shp, generator=generator, device=dev))
    feats = model.encode_audio(audio_cond)  # once per clip (the reference: every step)
    xt = draw(shape).to(dev)
    x0 = None
    guided = float(guidance_scale) != 1.0
    if guided:
        cond2 = torch.cat([img_cond, img_cond])
        feats2 = torch.cat([feats, torch.zeros_like(feats)])
    with frozen_weights():  # packed conv weights reused across the steps
        for k, i in enumerate(reversed(range(n_timesteps))):
            if max_steps is not None and k == max_steps:
                break
            t = torch.tensor([i], dtype=torch.long, device=dev)
            if guided:
                eps_c, eps_u = model(torch.cat([xt, xt]), cond2, feats2,
                                     torch.cat([t, t])).chunk(2)
                eps = cfg_combine(eps_c, eps_u, guidance_scale, guidance_rescale)
            else:
                eps = model(xt, img_cond, feats, t)
            if prediction == "v":
                eps = v_to_eps(scheduler, eps, xt, t)
            z = draw(xt.shape).to(dev)
            xt, x0 = scheduler.sample_prev_timestep(xt, eps, t, z=z)
            if callback is not None:
                callback(i, xt, x0)
            if (i + 1) % save_every == 0 or i == 0:
                save_frame(x0, os.path.join(out_dir, f"x0_{i}"))
    print("All images have been processed and saved.")
    return x0


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--random-init", action="store_true",
                    help="no checkpoint: seeded smoke weights and a random wav2vec2")
    ap.add_argument("--sampler", default="ddpm-v2", choices=["ddpm-v2", "ddim", "dpm++"],
                    help="dpm++: DPM-Solver++(2M), second-order multistep, deterministic")
    ap.add_argument("--steps", type=int, default=None,
                    help="500 (ddpm-v2) / 50 (ddim) / 20 (dpm++)")
    ap.add_argument("--spacing", default="logsnr", choices=["logsnr", "linspace"],
                    help="dpm++ timesteps: uniform in log-SNR (default) or DDIM's linspace")
    ap.add_argument("--dims", type=int, default=2)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--image-size", type=int, default=config["dataset_params"]["im_size"])
    ap.add_argument("--attention-mode", default="joint")
    ap.add_argument("--audio-attention", action="store_true",
                    help="audio cross-attention branches (build extension)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--out-dir", default=OUT_DIR)
    ap.add_argument("--cond-npz", default=None)
    ap.add_argument("--save-every", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--guidance-scale", type=float, default=1.0,
                    help="classifier-free audio guidance weight (1 = off; needs a model trained "
                         "with --audio-drop-prob)")
    ap.add_argument("--guidance-rescale", type=float, default=0.0,
                    help="std-rescale of the guided noise in [0, 1] (Lin et al. 2023)")
    ap.add_argument("--prediction", default="eps", choices=["eps", "v"],
                    help="what the checkpoint's denoiser predicts (train.py --prediction); every "
                         "sampler reads its output accordingly")
    ap.add_argument("--use-scale-shift-norm", action="store_true",
                    help="the checkpoint's ResBlocks are FiLM-conditioned (train.py "
                         "--use-scale-shift-norm)")
    ap.add_argument("--clip-frames", type=int, default=None,
                    help="frames to generate (--dims 3; default --frames).  More than --frames: "
                         "the clip is denoised as overlapping --frames windows blended at every "
                         "step (--sampler ddim|dpm++)")
    ap.add_argument("--window-stride", type=int, default=None,
                    help="frames between window starts (default frames // 2)")
    ap.add_argument("--window-blend", default="triangle", choices=["triangle", "uniform"],
                    help="weights of overlapping windows: highest at a window's centre, or equal")
    ap.add_argument("--window-batch", type=int, default=None,
                    help="windows per denoiser forward (default: all of them in one)")
    ap.add_argument("--dynamic-threshold", type=float, default=None, metavar="P",
                    help="dynamic thresholding (Saharia et al. 2022): every step clamps x0 to "
                         "[-s, s] and divides by s, s the sample's P-quantile of |x0|, at least 1 "
                         "(--sampler ddim|dpm++; for guidance scales well above 1)")
    ap.add_argument("--threshold-max", type=float, default=None, metavar="M",
                    help="upper bound of the dynamic threshold s (default: none)")
    ap.add_argument("--known", default=None, metavar="FILE.npy",
                    help="masked sampling (--sampler ddim|dpm++): a clip to keep, float in "
                         "[-1, 1], shaped like the sample without its batch axis ([3, H, W], "
                         "--dims 3: [3, frames, H, W]); the mask flags say where.  Default mask: "
                         "the lower half of every frame is generated")
    ap.add_argument("--keep-mask", default=None, metavar="FILE.npy",
                    help="the mask itself, float in [0, 1] over the frames and pixels ([H, W], "
                         "--dims 3: [frames, H, W]): 1 keeps --known, 0 generates, in between "
                         "blends; excludes the three flags below")
    ap.add_argument("--generate-box", type=float, nargs=4, default=None,
                    metavar=("Y0", "Y1", "X0", "X1"),
                    help="the generated region as fractions of the height and the width (default "
                         "0.5 1 0 1: the lower half); everything outside is kept")
    ap.add_argument("--keep-frames", type=int, default=None, metavar="K",
                    help="keep the first K frames whole (continue a clip: with --generate-box 0 1 "
                         "0 1)")
    ap.add_argument("--mask-feather", type=int, default=None, metavar="PX",
                    help="linear ramp of PX pixels just inside the box edges")
    ap.add_argument("--score", action="store_true",
                    help="PSNR and SSIM of the sample (--sampler ddim|dpm++) against the --known "
                         "clip, frame by frame: over the whole frame and, weighted with 1 - keep, "
                         "over the generated region (kept pixels ARE the known clip, so the "
                         "whole-frame score flatters); written to --score-out")
    ap.add_argument("--score-against", default=None, metavar="FILE.npy",
                    help="score against this ground-truth clip instead, float in [-1, 1], shaped "
                         "like the sample without its batch axis; needs no masked sampling")
    ap.add_argument("--score-out", default=None, metavar="FILE.json",
                    help="where the per-frame values and their means go (default "
                         "<out-dir>/metrics.json)")
    args = ap.parse_args(argv)
    scoring = args.score or args.score_against is not None
    if args.score and args.known is None and args.score_against is None:
        ap.error("--score needs --known or --score-against: a clip to score the sample against")
    if args.score_out is not None and not scoring:
        ap.error("--score-out needs --score or --score-against")
    if scoring and args.image_size < 11:
        ap.error(f"--score and --score-against need frames of at least 11 x 11, the SSIM window "
                 f"(got --image-size {args.image_size})")
    box_flags = [f for f, v in (("--generate-box", args.generate_box),
                                ("--keep-frames", args.keep_frames),
                                ("--mask-feather", args.mask_feather)) if v is not None]
    mask_flags = box_flags + (["--keep-mask"] if args.keep_mask is not None else [])
    if args.known is None and mask_flags:
        ap.error(f"{', '.join(mask_flags)}: masked sampling needs --known")
    if args.known is not None and args.sampler not in ("ddim", "dpm++"):
        ap.error(f"--known needs --sampler ddim or dpm++ (got {args.sampler}: the known clip is "
                 "kept inside their step kernel)")
    if scoring and args.sampler not in ("ddim", "dpm++"):
        ap.error(f"--score and --score-against need --sampler ddim or dpm++ (got {args.sampler}: "
                 "the final x0 of their sampling drivers is what is scored)")
    if args.keep_mask is not None and box_flags:
        ap.error(f"--keep-mask excludes {', '.join(box_flags)}")
    if args.keep_frames is not None and args.keep_frames < 0:
        ap.error("--keep-frames must be at least 0")
    if args.mask_feather is not None and args.mask_feather < 0:
        ap.error("--mask-feather must be at least 0")
    if args.dynamic_threshold is not None:
        if args.sampler not in ("ddim", "dpm++"):
            ap.error(f"--dynamic-threshold needs --sampler ddim or dpm++ (got {args.sampler}: "
                     "ancestral DDPM has no x0 clamp to replace)")
        if not 0.0 < args.dynamic_threshold <= 1.0:
            ap.error("--dynamic-threshold must be in (0, 1]")
    if args.threshold_max is not None:
        if args.dynamic_threshold is None:
            ap.error("--threshold-max needs --dynamic-threshold")
        if not args.threshold_max >= 1.0:
            ap.error("--threshold-max must be at least 1")
    if args.steps is None and args.sampler == "dpm++":
        args.steps = 20
    if args.clip_frames is not None:
        if args.clip_frames < 1:
            ap.error("--clip-frames must be at least 1")
        _check_long(args, args.clip_frames)
    return args


def _check_long(args, clip_frames):
    """A clip longer than the denoiser's window needs the windowed samplers."""
    if args.dims == 3 and clip_frames < args.frames:
        raise SystemExit(f"test.py: a clip of {clip_frames} frames is shorter than the window "
                         f"(--frames {args.frames})")
    if clip_frames > (args.frames if args.dims == 3 else 1) and (
            args.dims != 3 or args.sampler not in ("ddim", "dpm++")):
        raise SystemExit(f"test.py: a clip of {clip_frames} frames is longer than the denoiser's "
                         f"window (--frames {args.frames}); windowed sampling needs --dims 3 and "
                         f"--sampler ddim or dpm++ (got --dims {args.dims}, --sampler "
                         f"{args.sampler})")


def _load_mask(args, shape):
    """The `known` / `keep` keywords of masked sampling from --known and the mask flags ({}
    without --known).  shape: the sample's, (1, 3, [frames,] H, W)."""
    if args.known is None:
        return {}
    known = np.load(args.known, allow_pickle=False)
    if tuple(known.shape) != tuple(shape[1:]) or not np.issubdtype(known.dtype, np.floating):
        raise SystemExit(f"test.py: --known holds {known.dtype} {tuple(known.shape)}; the sample "
                         f"is float {tuple(shape[1:])}")
    if not (np.isfinite(known).all() and np.abs(known).max() <= 1.0):
        raise SystemExit("test.py: --known has values outside [-1, 1]")
    spatial = tuple(shape[2:])
    if args.keep_mask is not None:
        keep = np.load(args.keep_mask, allow_pickle=False)
        if tuple(keep.shape) != spatial or not np.issubdtype(keep.dtype, np.floating):
            raise SystemExit(f"test.py: --keep-mask holds {keep.dtype} {tuple(keep.shape)}; the "
                             f"sample's frames and pixels are float {spatial}")
        keep = torch.from_numpy(keep).float().view((1, 1) + spatial)
    else:
        frames = spatial[0] if len(spatial) == 3 else 1
        try:
            keep = keep_mask(frames, *spatial[-2:],
                             generate_box=args.generate_box or (0.5, 1.0, 0.0, 1.0),
                             keep_frames=args.keep_frames or 0, feather=args.mask_feather or 0)
        except ValueError as e:
            raise SystemExit(f"test.py: {e}") from None
        keep = keep.view((1, 1) + spatial)
    return dict(known=torch.from_numpy(known).float()[None], keep=keep)


def _load_target(args, shape):
    """The ground-truth clip of --score-against, [1, 3, [frames,] H, W] fp32 on the CPU."""
    gt = np.load(args.score_against, allow_pickle=False)
    if tuple(gt.shape) != tuple(shape[1:]) or not np.issubdtype(gt.dtype, np.floating):
        raise SystemExit(f"test.py: --score-against holds {gt.dtype} {tuple(gt.shape)}; the "
                         f"sample is float {tuple(shape[1:])}")
    if not (np.isfinite(gt).all() and np.abs(gt).max() <= 1.0):
        raise SystemExit("test.py: --score-against has values outside [-1, 1]")
    return torch.from_numpy(gt).float()[None]


def score_sample(args, x0, mask, target=None):
    """--score / --score-against: PSNR and SSIM of the final x0 against `target` (default: the
    known clip of `mask`), whole frame and, with a mask, over the generated region (weight 1 -
    keep).  Writes the report to --score-out and, beside the frames, what it scored: sample.npy
    (the fp32 x0 in [-1, 1] without its batch axis) and score_weight.npy (the region weight), so
    that `python -m vdiff.metrics sample.npy truth.npy [--weight score_weight.npy]` gives the
    same numbers.  Returns the report."""
    import json

    from vdiff import metrics
    sample = x0.detach().float().contiguous()
    against = "score-against" if target is not None else "known"
    truth = (mask["known"] if target is None else target).to(sample.device).float().contiguous()
    os.makedirs(args.out_dir, exist_ok=True)
    np.save(os.path.join(args.out_dir, "sample.npy"), sample[0].cpu().numpy())
    report = {"against": against, "sampler": args.sampler, "steps": args.steps}
    whole = metrics.clip_metrics(sample, truth)
    metrics.print_report(whole, f"whole frame, against --{against}:")
    report["whole"] = whole.to_json()
    if mask:
        weight = metrics.region_weight(mask["keep"])
        np.save(os.path.join(args.out_dir, "score_weight.npy"), weight.cpu().numpy())
        region = metrics.clip_metrics(sample, truth, weight=weight)
        metrics.print_report(region, "generated region (weight 1 - keep):")
        report["region"] = region.to_json()
    path = args.score_out or os.path.join(args.out_dir, "metrics.json")
    with open(path, "w") as f:
        json.dump(report, f, indent=1)
    print(f"metrics written to {path}")
    return report


def main(argv=None):
    args = parse(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("test.py runs on the MI355X kernels only")
    if not args.ckpt and not args.random_init:
        raise SystemExit("test.py: pass --ckpt <state_dict> (the reference loads "
                         "ldm_ckpt_name) or --random-init for seeded smoke weights")
    global device
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    cfg = {k: dict(v) for k, v in config.items()}
    cfg["dataset_params"]["im_size"] = args.image_size
    cfg["ldm_params"].update(dims=args.dims, attention_mode=args.attention_mode,
                             dtype=args.dtype, audio_attention=args.audio_attention,
                             use_scale_shift_norm=args.use_scale_shift_norm)
    cfg["train_params"]["ldm_ckpt_name"] = args.ckpt
    config.update(cfg)
    model, scheduler = load_model_and_scheduler(config, seed=args.seed)
    frames = args.frames if args.dims == 3 else 1
    clip_frames = frames if args.clip_frames is None else args.clip_frames
    if args.cond_npz:
        z = np.load(args.cond_npz, allow_pickle=False)
        cond = torch.from_numpy(z["image"]).float()[None].to(device)
        audio = {"input_values": torch.from_numpy(z["audio"]).float().to(device)}
        if args.dims == 3 and audio["input_values"].shape[0] > frames:
            # the file decides the clip's length: one frame per audio window
            if args.clip_frames not in (None, audio["input_values"].shape[0]):
                raise SystemExit(f"test.py: --clip-frames {args.clip_frames}, but {args.cond_npz} "
                                 f"holds {audio['input_values'].shape[0]} audio windows")
            clip_frames = audio["input_values"].shape[0]
            _check_long(args, clip_frames)
    else:
        clip = synthetic_clip(1, clip_frames, args.image_size, 500, device, seed=args.seed,
                              dims=args.dims)
        cond, audio = clip.cond, clip.audio
    g = torch.Generator(device=device).manual_seed(args.seed)
    if args.sampler in ("ddim", "dpm++"):
        os.makedirs(args.out_dir, exist_ok=True)
        shape = (1, 3, frames, args.image_size, args.image_size) if args.dims == 3 else \
            (1, 3, args.image_size, args.image_size)
        if args.sampler == "ddim":
            sampler = DDIMSampler(scheduler, steps=args.steps or 50, prediction=args.prediction,
                                  dynamic_threshold=args.dynamic_threshold,
                                  threshold_max=args.threshold_max)
            sample = sample_ddim
        else:
            sampler = DPMSolverSampler(scheduler, steps=args.steps or 20, spacing=args.spacing,
                                       prediction=args.prediction,
                                       dynamic_threshold=args.dynamic_threshold,
                                       threshold_max=args.threshold_max)
            sample = sample_dpm

        def cb(i, xt, x0):
            if (i + 1) % args.save_every == 0 or i == sampler.steps - 1:
                save_frame(x0, os.path.join(args.out_dir, f"x0_{i}"))

        scoring = args.score or args.score_against is not None
        if clip_frames > frames:  # (--dims 3: _check_long)
            shape = (1, 3, clip_frames, args.image_size, args.image_size)
        mask = _load_mask(args, shape)
        target = _load_target(args, shape) if args.score_against is not None else None
        if clip_frames > frames:
            _, x0 = sample_long(model, sampler, cond, audio, shape, window=frames,
                                stride=args.window_stride, blend=args.window_blend,
                                window_batch=args.window_batch, generator=g, callback=cb,
                                guidance_scale=args.guidance_scale,
                                guidance_rescale=args.guidance_rescale, **mask)
        else:
            _, x0 = sample(model, sampler, cond, audio, shape, generator=g, callback=cb,
                           guidance_scale=args.guidance_scale,
                           guidance_rescale=args.guidance_rescale, **mask)
        print("All images have been processed and saved.")
        if scoring:
            score_sample(args, x0, mask, target)
        return x0
    return sample_images(model, scheduler, cond, audio, n_timesteps=args.steps or 500,
                         out_dir=args.out_dir, save_every=args.save_every, generator=g,
                         guidance_scale=args.guidance_scale,
                         guidance_rescale=args.guidance_rescale, prediction=args.prediction)


if __name__ == "__main__":
    main()
