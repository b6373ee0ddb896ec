"""Gradient clipping on the config-2 gradient list (the bench's UNetAudio with its wav2vec2
encoder, one fp32 gradient per trainable tensor): the three launches of vdiff.clip
(vd_grad_sumsq + vd_grad_clip) against torch.nn.utils.clip_grad_norm_(foreach=True) on the same
tensors -- once with a max_norm that clips and once with inf (measure only) -- and the config-2
Trainer.step with and without clip_grad_norm=1.0, with the table rebuilds over those steps.

Timing: HIP events around back-to-back calls after a warm-up, the variants alternated, the
median and the range of the repeats reported.  "eager" is what a Python loop pays; "graph"
replays PER_GRAPH captured calls, the device time.  Traffic: one read of the gradients to
measure, plus a read and a write when clipping (4, resp. 12 bytes per element), given against
the 6.29 TB/s measured float4 copy rate.  The clipping max_norm is a tenth of
the list's norm, and every call finds the gradients refilled to the same norm by a
device-to-device copy that is timed on its own and subtracted (both variants pay the same
refill, so their difference is exact; the rate after the subtraction still carries whatever the
refill's freshly written lines cost the pass that reads them next).  The launches are
therefore also timed alone, with no refill: vd_grad_sumsq only reads, and vd_grad_clip on
partials left as they are scales by the same 0.999 every call.
python tools/clip_bench.py [--out profiles/clip_bench.txt] [--no-step]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lipreading-video-generation_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from vdiff import ops  # noqa: E402
from vdiff.clip import GradClipper  # noqa: E402
from vdiff.ema import CHUNK  # noqa: E402

COPY_TBS = 6.29
REPEATS, PER_GRAPH = 7, 5

_out = None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if _out is not None:
        _out.write(line + "\n")
        _out.flush()


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
    """Alternate the variants REPEATS times; {name: (median, min, max)} us per call."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, fn in fns.items():
            res[k].append(_time(fn, calls) / per_call)
    out = {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}
    for k, (med, lo, hi) in out.items():
        say(f"{label:12s} {k:34s} {med:9.1f} us  ({lo:.1f}-{hi:.1f})")
    return out


def kernel_bench(model):
    params = [p for p in model.parameters() if p.requires_grad]
    gen = torch.Generator(device="cuda").manual_seed(0)
    grads = [torch.randn(p.shape, generator=gen, device=p.device) * 1e-2 for p in params]
    keep = [g.clone() for g in grads]
    for p, g in zip(params, grads):  # clip_grad_norm_ takes parameters: the same storage
        p.grad = g
    nel = sum(g.numel() for g in grads)
    ref = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
    clip_at = ref / 10
    clipper = {"inf": GradClipper(float("inf")), "clip": GradClipper(clip_at)}
    for c in clipper.values():  # measure first: the clipping one scales the gradients
        c.clip(grads)
    after = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
    say(f"clipped to {clip_at:.6g}: coef {float(clipper['clip'].coef):.6g}, fp64 norm afterwards "
        f"{after:.6g}")
    torch._foreach_copy_(grads, keep)
    say(f"{len(grads)} gradient tensors, {nel / 1e6:.1f} M elements ({4 * nel / 1e6:.0f} MB), "
        f"{clipper['inf'].n_desc} descriptors of at most {CHUNK} elements; fp64 norm {ref:.6g}, "
        f"vdiff.clip {float(clipper['inf'].norm):.6g}, torch "
        f"{float(torch.nn.utils.clip_grad_norm_(params, float('inf'), foreach=True)):.6g}")

    def refill():
        torch._foreach_copy_(grads, keep)

    def variants(max_norm, c):
        def ours():
            refill()
            c.clip(grads)

        def theirs():
            refill()
            torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=True)
        return {"refill only": refill, "vdiff.clip (3 launches) + refill": ours,
                "clip_grad_norm_(foreach) + refill": theirs}

    for name, max_norm, nbytes in (("clip", clip_at, 12 * nel), ("inf", float("inf"), 4 * nel)):
        say(f"-- max_norm = {name}: {nbytes / 1e6:.0f} MB per call "
            f"({nbytes / COPY_TBS / 1e6:.0f} us at the copy rate)")
        fns = variants(max_norm, clipper[name])
        for mode in ("eager", "graph"):
            if mode == "eager":
                res = _ab(f"eager {name}", fns, 20)
            else:
                graphs = {k: _graphed(fn) for k, fn in fns.items()}
                res = _ab(f"graph {name}", {k: g.replay for k, g in graphs.items()}, 10,
                          per_call=PER_GRAPH)
                del graphs
            base = res["refill only"][0]
            ours = res["vdiff.clip (3 launches) + refill"][0] - base
            theirs = res["clip_grad_norm_(foreach) + refill"][0] - base
            rate = nbytes / ours / 1e3 if ours > 0 else float("nan")
            say(f"{mode} {name}: less the refill, vdiff.clip {ours:.1f} us ({rate:.0f} GB/s = "
                f"{rate / (COPY_TBS * 1e3):.2f} of the copy rate) vs clip_grad_norm_(foreach) "
                f"{theirs:.1f} us: vdiff.clip is {'FASTER' if ours < theirs else 'SLOWER'} by "
                f"{abs(theirs - ours):.1f} us")
    # The launches alone, no refill: vd_grad_sumsq only reads, and vd_grad_clip on partials
    # that are left as they are takes the same coef = 0.999 every call, so its scaling pass
    # always writes (the gradients shrink by 0.999 per call, nothing else changes).
    c = clipper["inf"]
    refill()
    c.clip(grads)                               # measure only: the partials of the full list
    near = 0.999 * float(c.norm)
    scratch = torch.empty(c.n_desc, dtype=torch.float32, device=grads[0].device)
    alone = {"vd_grad_sumsq": lambda: ops.grad_sumsq(c._table, c.n_desc, scratch),
             "vd_grad_clip, coef 0.999": lambda: ops.grad_clip(c._table, c.n_desc, c._work, near,
                                                               c._record)}
    say("-- the launches alone (replayed, no refill between calls)")
    graphs = {k: _graphed(fn) for k, fn in alone.items()}
    res = _ab("graph alone", {k: g.replay for k, g in graphs.items()}, 10, per_call=PER_GRAPH)
    del graphs
    for k, nbytes in (("vd_grad_sumsq", 4 * nel), ("vd_grad_clip, coef 0.999", 8 * nel)):
        rate = nbytes / res[k][0] / 1e3
        say(f"{k}: {nbytes / 1e6:.0f} MB in {res[k][0]:.1f} us = {rate:.0f} GB/s = "
            f"{rate / (COPY_TBS * 1e3):.2f} of the copy rate")
    say(f"coef at the end {float(c.coef):.6g}")
    refill()
    say(f"table rebuilds over the kernel timings: clip {clipper['clip'].rebuilds}, "
        f"inf {clipper['inf'].rebuilds}")


def step_bench():
    import bench
    from vdiff.engine import Trainer, synthetic_clip
    from vdiff.schedulers import LinearNoiseScheduler
    dev = torch.device("cuda")
    ns = argparse.Namespace(size=128, frames=16, dtype="bf16", mode="joint", init="nonzero")
    trainers = {}
    for name, c in (("no clipping", None), ("clip_grad_norm=1.0", 1.0)):
        torch.manual_seed(0)
        m = bench.build_model(ns, dev)
        trainers[name] = Trainer(m, LinearNoiseScheduler(100, 0.00085, 0.012), lr=1e-4,
                                 clip_grad_norm=c)
    clips = [synthetic_clip(1, 16, 128, 100, dev, seed=i) for i in range(4)]
    for tr in trainers.values():
        for c in clips[:3]:
            tr.step(c)
    torch.cuda.synchronize()
    res = {k: [] for k in trainers}
    clipped = 0
    for i in range(12):
        for k, tr in trainers.items():
            c = clips[i % len(clips)]
            res[k].append(_time(lambda: tr.step(c), 1) / 1e3)
            if tr.clipper is not None:
                clipped += int(tr.clip_coef < 1)
    say("-- config-2 Trainer.step (1 clip x 16 x 128 x 128, bf16, eager), ms per step")
    for k, v in res.items():
        say(f"{k:22s} {statistics.median(v):8.2f} ms  ({min(v):.2f}-{max(v):.2f})")
    a, b = (statistics.median(v) for v in res.values())
    say(f"with clipping - without = {b - a:+.2f} ms ({(b / a - 1) * 100:+.2f} %)")
    tr = trainers["clip_grad_norm=1.0"]
    say(f"clip_grad_norm=1.0: {tr.clipper.rebuilds} table rebuilds over {tr.steps_done} steps "
        f"({tr.clipper.n_desc} descriptors at the last), {clipped} of the 12 timed steps "
        f"clipped, last norm {float(tr.grad_norm):.4g}")
    for tr in trainers.values():
        tr.check_finite()


def main():
    global _out
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_bench.txt"))
    ap.add_argument("--no-step", action="store_true", help="kernel timings only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench: needs the GPU (no CPU timing is meaningful)")
    import bench
    _out = open(args.out, "w")
    say(torch.cuda.get_device_name(0))
    dev = torch.device("cuda")
    ns = argparse.Namespace(size=128, frames=16, dtype="bf16", mode="joint", init="nonzero")
    model = bench.build_model(ns, dev)
    kernel_bench(model)
    del model
    torch.cuda.empty_cache()
    if not args.no_step:
        step_bench()
    _out.close()


if __name__ == "__main__":
    main()
