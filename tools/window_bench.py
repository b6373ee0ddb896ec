"""Long-clip sampling at the config-2 shape: one replayed sample_long DDIM step over L = 32
frames as three overlapping 16-frame windows (stride 8; 128 x 128, joint attention, bf16 model)
against three times the replayed single-window DDIM step, the share of the long step spent in
vd_window_gather + vd_window_blend, and the memory high-water mark of each.

Timing: HIP events around back-to-back replays after a warm-up, the two graphs alternated, the
median and the range of the repeats reported.  The gather + blend pair is timed as a graph of
20 captured pairs on the long step's own buffers (a few MB, resident in the last-level cache).
python tools/window_bench.py [--frames 32] [--guided]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lipreading-video-generation_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from vdiff import ops  # noqa: E402
from vdiff.engine import DDIMGraph, LongDDIMGraph, WindowedDenoiser  # noqa: E402
from vdiff.schedulers import DDIMSampler, LinearNoiseSchedulerV2, WindowPlan  # noqa: E402

WINDOW, STRIDE, SIZE = 16, 8, 128
REPLAYS, REPEATS, PER_GRAPH = 8, 5, 20


def _time(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for k in range(calls):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls  # ms per call


def _peak(build):
    """(what build() returns, peak bytes allocated while it ran and one step replayed)."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    g = build()
    g.step(0)
    torch.cuda.synchronize()
    return g, torch.cuda.max_memory_allocated(), base


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--frames", type=int, default=32, help="the long clip's frames L")
    ap.add_argument("--guided", action="store_true", help="guided steps (w = 3, rescale 0.7)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_bench: needs the GPU (no CPU timing is meaningful)")
    import bench
    dev = torch.device("cuda")
    print(torch.cuda.get_device_name(0), flush=True)
    ns = argparse.Namespace(size=SIZE, frames=WINDOW, dtype="bf16", mode="joint", init="nonzero")
    m = bench.build_model(ns, dev).eval()
    L = args.frames
    plan = WindowPlan(L, WINDOW, STRIDE)
    sampler = DDIMSampler(LinearNoiseSchedulerV2(500, 0.00005, 0.015), steps=50)
    g = torch.Generator(device=dev).manual_seed(5)
    cond = torch.rand((1, 3, SIZE, SIZE), device=dev, generator=g) * 2 - 1
    feats = torch.randn((L, 768), device=dev, generator=g)  # encoded audio, one row per frame
    x_long = torch.randn((1, 3, L, SIZE, SIZE), device=dev, generator=g)
    x_one = x_long[:, :, :WINDOW].contiguous()
    kw = dict(guidance_scale=3.0, guidance_rescale=0.7) if args.guided else {}
    print(f"L = {L}, T = {WINDOW}, S = {STRIDE}: {plan.num_windows} windows, largest coverage "
          f"{plan.max_coverage}; {SIZE} x {SIZE}, joint attention, bf16 model, fp32 latent"
          f"{', guided w = 3 rescale 0.7' if args.guided else ''}", flush=True)
    with torch.no_grad(), ops.frozen_weights():
        def build_long():
            windows = WindowedDenoiser(m, plan, cond, feats, x_long, bool(kw))
            gr = LongDDIMGraph(m, sampler, windows, x_long, **kw)
            gr.capture()
            return gr

        def build_one():
            gr = DDIMGraph(m, sampler, cond, feats[:WINDOW].contiguous(), x_one, **kw)
            gr.capture()
            return gr

        one, peak_one, base_one = _peak(build_one)
        long_, peak_long, base_long = _peak(build_long)
        print(f"memory high-water mark: long step {peak_long / 2**20:.0f} MiB (of which "
              f"{base_long / 2**20:.0f} MiB were allocated before: weights, inputs and the "
              f"single-window graph), single-window step {peak_one / 2**20:.0f} MiB (of which "
              f"{base_one / 2**20:.0f} MiB before)", flush=True)
        types = long_.node_types()
        print(f"long step graph nodes: {types}", flush=True)

        # gather + blend on the long step's own buffers
        windows = long_.windows
        eps = torch.randn_like(windows.win)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.window_gather(long_.xt, plan, out=windows.win[:windows.half],
                              dup=windows.win[windows.half:] if windows.guided else None)
            ops.window_blend(eps, plan)
        torch.cuda.current_stream().wait_stream(side)
        pair = torch.cuda.CUDAGraph()
        with torch.cuda.graph(pair):
            for _ in range(PER_GRAPH):
                ops.window_gather(long_.xt, plan, out=windows.win[:windows.half],
                                  dup=windows.win[windows.half:] if windows.guided else None)
                ops.window_blend(eps, plan)

        def step_of(gr, x_init):
            def run(k):
                if k == 0:
                    gr.xt.copy_(x_init)  # every timed window starts from the same latent
                gr.step(k)
            return run

        fns = {"long": step_of(long_, x_long), "single": step_of(one, x_one)}
        for fn in fns.values():
            for k in range(3):
                fn(k)
        res = {k: [] for k in fns}
        res["pair"] = []
        for _ in range(REPEATS):
            for k, fn in fns.items():
                res[k].append(_time(fn, REPLAYS))
            res["pair"].append(_time(lambda k: pair.replay(), 50) / PER_GRAPH)
        med = {k: statistics.median(v) for k, v in res.items()}
        for k, label in (("long", f"replayed sample_long DDIM step, {plan.num_windows} windows"),
                         ("single", "replayed single-window DDIM step")):
            print(f"{label:52s} {med[k]:9.2f} ms  ({min(res[k]):.2f}-{max(res[k]):.2f})",
                  flush=True)
        print(f"{plan.num_windows} x single-window step = {plan.num_windows * med['single']:.2f} "
              f"ms; long / that = {med['long'] / (plan.num_windows * med['single']):.3f}",
              flush=True)
        print(f"gather + blend {med['pair'] * 1e3:9.2f} us  ({min(res['pair']) * 1e3:.2f}-"
              f"{max(res['pair']) * 1e3:.2f}) = {100 * med['pair'] / med['long']:.3f} % of the "
              f"long step", flush=True)


if __name__ == "__main__":
    main()
