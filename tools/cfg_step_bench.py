"""Classifier-free guidance at the config-2 sample shape (1 x 3 x 16 x 128 x 128, bf16): the fused
guide + rescale + DDIM step (ops.ddim_step_cfg: vd_cfg_stats + vd_ddim_step_cfg) against the
unfused composition it replaces -- torch ops for the guide and the std-rescale (diffusers'
rescale_noise_cfg), then ops.ddim_step -- with phi = 0 and phi = 0.7; and a guided 50-step
sample_ddim against an unguided one on the bench's config-2 model.

Timing: HIP events around back-to-back calls after a warm-up, the two variants alternated, the
median and the range of the repeats reported.  "eager" is what a Python loop pays (launch
bound for kernels this small); "graph" replays 20 captured calls, the device time a graphed
sampler pays.  The working set (8 to 14 MB) is reused by every call, so it stays in the
last-level cache: the rates printed are cache-resident traffic, not HBM bandwidth.
python tools/cfg_step_bench.py [--no-sample]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lipreading-video-generation_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from vdiff import ops  # noqa: E402
from vdiff.schedulers import DDIMSampler, LinearNoiseSchedulerV2  # noqa: E402

SHAPE = (1, 3, 16, 128, 128)
W = 3.0
# a timed window is CALLS eager calls or REPLAYS replays of PER_GRAPH captured calls: tens of
# milliseconds at the 3.6 us of the fastest variant
CALLS, REPLAYS, REPEATS, PER_GRAPH = 2000, 500, 7, 20


def composed(xt, c, u, t, tp, acp, w, phi):
    g = u + w * (c - u)
    if phi > 0:
        dims = list(range(1, c.dim()))
        std_c = c.std(dim=dims, keepdim=True)
        std_g = g.std(dim=dims, keepdim=True)
        g = phi * (g * (std_c / std_g)) + (1 - phi) * g
    return ops.ddim_step(xt, g, t, tp, acp)


def fused(xt, c, u, t, tp, acp, w, phi):
    return ops.ddim_step_cfg(xt, c, u, t, tp, acp, w, phi)


def _time(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls  # us per call


def _graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(PER_GRAPH):
            fn()
    return g


def _ab(label, fns, calls, per_call=1):
    """Alternate the variants REPEATS times; median (min-max) us per call."""
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, fn in fns.items():
            res[k].append(_time(fn, calls) / per_call)
    out = {}
    for k, v in res.items():
        out[k] = statistics.median(v)
        print(f"{label:28s} {k:9s} {out[k]:8.2f} us  ({min(v):.2f}-{max(v):.2f})", flush=True)
    return out


def step_bench():
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    xt, c, u = (torch.randn(SHAPE, generator=g, device=dev).bfloat16() for _ in range(3))
    t = torch.tensor([250], device=dev)
    tp = torch.tensor([240], device=dev)
    acp = LinearNoiseSchedulerV2(500, 0.00005, 0.015).alpha_cum_prod.float().to(dev)
    n = xt.numel()
    print(f"shape {SHAPE} bf16, {n} elements; fused traffic xt + c + u in, x_prev + x0 out = "
          f"{5 * 2 * n / 1e6:.2f} MB (+ 2 x (c + u) = {4 * 2 * n / 1e6:.2f} MB of statistics "
          f"reads with phi > 0)", flush=True)
    for phi in (0.0, 0.7):
        a = fused(xt, c, u, t, tp, acp, W, phi)[0].float()
        b = composed(xt, c, u, t, tp, acp, W, phi)[0].float()
        print(f"phi={phi}: fused vs composed x_prev max |diff| {float((a - b).abs().max()):.3e} "
              f"(bf16 intermediates in the composition)", flush=True)
        fns = {"fused": lambda: fused(xt, c, u, t, tp, acp, W, phi),
               "composed": lambda: composed(xt, c, u, t, tp, acp, W, phi)}
        r = _ab(f"eager  phi={phi}", fns, CALLS)
        print(f"  eager  phi={phi}: composed / fused = {r['composed'] / r['fused']:.2f}x")
        graphs = {k: _graphed(fn) for k, fn in fns.items()}
        r = _ab(f"graph  phi={phi}", {k: gr.replay for k, gr in graphs.items()},
                REPLAYS, per_call=PER_GRAPH)
        print(f"  graph  phi={phi}: composed / fused = {r['composed'] / r['fused']:.2f}x; fused "
              f"moves {(5 + (4 if phi else 0)) * 2 * n / r['fused'] / 1e3:.0f} GB/s (the same "
              f"buffers every call: resident in the 256 MB last-level cache, not HBM traffic)",
              flush=True)


def sample_bench():
    import bench
    from vdiff.engine import sample_ddim, synthetic_clip
    dev = torch.device("cuda")
    ns = argparse.Namespace(size=128, frames=16, dtype="bf16", mode="joint", init="nonzero")
    m = bench.build_model(ns, dev).eval()
    clip = synthetic_clip(1, 16, 128, 500, dev, seed=5)
    sampler = DDIMSampler(LinearNoiseSchedulerV2(500, 0.00005, 0.015), steps=50)
    with torch.no_grad(), ops.frozen_weights():
        feats = m.encode_audio(clip.audio)

        def run(**kw):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            sample_ddim(m, sampler, clip.cond, feats, tuple(clip.x0.shape),
                        generator=torch.Generator(device=dev).manual_seed(1), **kw)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        variants = {"unguided": {}, "guided w=3 phi=0.7": dict(guidance_scale=W,
                                                              guidance_rescale=0.7)}
        for kw in variants.values():
            run(**kw)  # warm-up: packed weights, code objects, the capture's allocations
        res = {k: [] for k in variants}
        for _ in range(3):
            for k, kw in variants.items():
                res[k].append(run(**kw))
        for k, v in res.items():
            print(f"sample_ddim 50 steps {k:20s} {statistics.median(v):8.1f} ms  "
                  f"({min(v):.1f}-{max(v):.1f}; graph capture included)", flush=True)
        a, b = (statistics.median(res[k]) for k in variants)
        print(f"guided / unguided = {b / a:.2f}x (one forward at batch 2 per step)", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--no-sample", action="store_true", help="kernel timings only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cfg_step_bench: needs the GPU (no CPU timing is meaningful)")
    print(torch.cuda.get_device_name(0), flush=True)
    step_bench()
    if not args.no_sample:
        sample_bench()


if __name__ == "__main__":
    main()
