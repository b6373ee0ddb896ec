"""Dynamic thresholding at the sample shapes (1 x 3 x 16 x 128 x 128 and the long clip's 1 x 3 x
32 x 128 x 128, bf16): one thresholded guided DDIM step (ops.ddim_step_cfg(thresh=(0.995, inf)):
vd_cfg_stats + vd_x0_abs_quantile's eight launches + vd_ddim_step_thr) against the same step with
the static clamp (clip=True) and against a torch composition -- the unfused guide and x0,
torch.quantile(interpolation="higher"), the clamp and the divide, each its own op -- at w = 7.5
with phi = 0 and phi = 0.7.

Timing as tools/cfg_step_bench.py: HIP events around back-to-back calls after a warm-up, the legs
interleaved, the median and the range of the repeats.  "eager" is what a Python loop pays (launch
bound); "graph" replays PER_GRAPH captured calls, the device time a graphed sampler pays.  The
working set is reused by every call and stays in the last-level cache.  "select" is thresh minus
clip: what the option adds to a step.
python tools/thr_bench.py"""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lipreading-video-generation_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from vdiff import ops  # noqa: E402
from vdiff.schedulers import LinearNoiseSchedulerV2  # noqa: E402

SHAPES = [(1, 3, 16, 128, 128), (1, 3, 32, 128, 128)]
W, P_THR = 7.5, 0.995
CALLS, REPLAYS, REPEATS, PER_GRAPH = 500, 100, 7, 20
SELECT_LAUNCHES = 8


def composed(xt, c, u, t, tp, acp, w, phi):
    g = u + w * (c - u)
    if phi > 0:
        dims = list(range(1, c.dim()))
        g = phi * (g * (c.std(dim=dims, keepdim=True) / g.std(dim=dims, keepdim=True))) \
            + (1 - phi) * g
    at, ap = acp[t].view(-1, 1, 1, 1, 1), acp[tp].view(-1, 1, 1, 1, 1)
    x0 = (xt - (1 - at).sqrt() * g) / at.sqrt()
    q = torch.quantile(x0.float().abs().flatten(1), P_THR, dim=1, interpolation="higher")
    s = q.clamp_min(1.0).view(-1, 1, 1, 1, 1)
    x0 = (torch.minimum(torch.maximum(x0, -s), s) / s).to(xt.dtype)
    return (ap.sqrt() * x0 + (1 - ap).sqrt() * g).to(xt.dtype), x0


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
    """Alternate the legs REPEATS times; median (min-max) us per call."""
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, fn in fns.items():
            res[k].append(_time(fn, calls) / per_call)
    out = {}
    for k, v in res.items():
        out[k] = statistics.median(v)
        print(f"{label:34s} {k:9s} {out[k]:8.2f} us  ({min(v):.2f}-{max(v):.2f})", flush=True)
    return out


def _report(label, r):
    add = r["thresh"] - r["clip"]
    line = (f"  {label}: select adds {add:.2f} us and {SELECT_LAUNCHES} launches to the "
            f"{r['clip']:.2f} us step kernel chain ({add / r['clip']:.1f}x of it)")
    if "torch" in r:
        line += f"; torch composition / thresholded step = {r['torch'] / r['thresh']:.2f}x"
    print(line, flush=True)


def step_bench(shape):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    xt, c, u = (torch.randn(shape, generator=g, device=dev).bfloat16() for _ in range(3))
    t = torch.tensor([250], device=dev)
    tp = torch.tensor([240], device=dev)
    acp = LinearNoiseSchedulerV2(500, 0.00005, 0.015).alpha_cum_prod.float().to(dev)
    n = xt.numel()
    print(f"shape {shape} bf16, {n} elements; a select pass reads xt + c + u = "
          f"{3 * 2 * n / 1e6:.2f} MB, four passes {4 * 3 * 2 * n / 1e6:.2f} MB", flush=True)
    thr = (P_THR, math.inf)
    for phi in (0.0, 0.7):
        a = ops.ddim_step_cfg(xt, c, u, t, tp, acp, W, phi, thresh=thr)[1].float()
        b = composed(xt, c, u, t, tp, acp, W, phi)[1].float()
        print(f"phi={phi}: thresholded x0 in [{float(a.min()):.3f}, {float(a.max()):.3f}]; vs the "
              f"torch composition max |diff| {float((a - b).abs().max()):.3e} (bf16 "
              f"intermediates there)", flush=True)
        fns = {"thresh": lambda: ops.ddim_step_cfg(xt, c, u, t, tp, acp, W, phi, thresh=thr),
               "clip": lambda: ops.ddim_step_cfg(xt, c, u, t, tp, acp, W, phi, clip=True),
               "torch": lambda: composed(xt, c, u, t, tp, acp, W, phi)}
        _report(f"eager T={shape[2]} phi={phi}", _ab(f"eager T={shape[2]} phi={phi}", fns, CALLS))
        graphs = {}
        for k, fn in fns.items():
            try:
                graphs[k] = _graphed(fn)
            except RuntimeError as e:  # an op of the composition that cannot be captured
                print(f"  graph: leg {k} not capturable: {str(e).splitlines()[0][:120]}",
                      flush=True)
                torch.cuda.synchronize()
        r = _ab(f"graph T={shape[2]} phi={phi}", {k: gr.replay for k, gr in graphs.items()},
                REPLAYS, per_call=PER_GRAPH)
        _report(f"graph T={shape[2]} phi={phi}", r)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("thr_bench: needs the GPU (no CPU timing is meaningful)")
    print(torch.cuda.get_device_name(0), flush=True)
    for shape in SHAPES:
        step_bench(shape)


if __name__ == "__main__":
    main()
