"""Weight EMA on the config-2 parameter list (the bench's UNetAudio with its wav2vec2 encoder):
one vd_ema_update launch at k = 1 and k = 2 rates against what the code could do before it --
torch._foreach_lerp_ (one pass per rate) and the nn.update_ema loop (two torch ops per tensor
and rate) -- on the same tensors; a sweep of the descriptor chunk size (vdiff.ema.CHUNK); and
the config-2 Trainer.step with and without ema_rates=(0.9999,).

Timing: HIP events around back-to-back calls after a warm-up, the variants alternated, the
median and the range of the repeats reported.  "eager" is what a Python loop pays; "graph"
replays PER_GRAPH captured calls, the device time.  Traffic per update is one read of the
parameters plus a read and a write of each shadow set, (1 + 2k) x 4 bytes per element; the
rate is given against the 6.29 TB/s measured float4 copy rate.  The parameter and
shadow sets together exceed the 256 MB last-level cache.
python tools/ema_bench.py [--out profiles/ema_bench.txt] [--no-step]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lipreading-video-generation_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vdiff import nn as vnn, ops  # noqa: E402
from vdiff.ema import CHUNK, EMA, descriptor_rows  # noqa: E402

COPY_TBS = 6.29
RATES = (0.9999, 0.999)
REPEATS, PER_GRAPH = 7, 5
CHUNKS = (2048, 4096, 8192, 16384, 32768, 65536, 262144)

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


def _ab(label, fns, calls, per_call=1, nbytes=None):
    """Alternate the variants REPEATS times; median (min-max) us per call."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, fn in fns.items():
            res[k].append(_time(fn, calls) / per_call)
    out = {}
    for k, v in res.items():
        out[k] = (statistics.median(v), min(v), max(v))
        rate = ""
        if nbytes:
            gbs = nbytes / out[k][0] / 1e3
            rate = f"  {gbs:7.0f} GB/s = {gbs / (COPY_TBS * 1e3):.2f} of the copy rate"
        say(f"{label:18s} {k:24s} {out[k][0]:9.1f} us  ({min(v):.1f}-{max(v):.1f}){rate}")
    return out


def _variants(params, ema, k):
    """One EMA update of k rates: the single launch, EMA.update() (launch + pointer check +
    count), k _foreach_lerp_ passes, the update_ema loop k times."""
    rates = ema.rates[:k]
    shadows = ema.shadows[:k]
    num = ema.num_updates
    rows = descriptor_rows([p.data_ptr() for p in params],
                           [[s.data_ptr() for s in sh] for sh in shadows],
                           [p.numel() for p in params], ema.chunk)
    table = torch.from_numpy(rows.view(np.uint8).copy()).to(params[0].device)
    n = len(rows)
    det = [p.detach() for p in params]

    def lerp():
        for r, sh in zip(rates, shadows):
            torch._foreach_lerp_(sh, det, 1.0 - r)

    def loop():
        for r, sh in zip(rates, shadows):
            vnn.update_ema(sh, det, rate=r)

    return {"vd_ema_update": lambda: ops.ema_update(table, n, rates, False, num, None),
            "foreach_lerp": lerp, "update_ema loop": loop}, (table, n)


def kernel_bench(model):
    params = [p for p in model.parameters() if p.requires_grad]
    nel = sum(p.numel() for p in params)
    ema = EMA(model, RATES, warmup=False)
    say(f"{len(params)} trainable tensors, {nel / 1e6:.1f} M elements ({4 * nel / 1e6:.0f} MB per "
        f"set), {ema.n_desc} descriptors of at most {CHUNK} elements; "
        f"smallest tensor {min(p.numel() for p in params)}, largest "
        f"{max(p.numel() for p in params)}")
    # same result first (one update from equal shadows; lerp rounds w (p - e) + e its own way)
    a = EMA(model, (0.9,))
    b = [p.detach().clone() for p in params]
    for p in params:
        p.data.add_(0.01 * torch.randn_like(p))
    a.update()
    torch._foreach_lerp_(b, [p.detach() for p in params], 1.0 - 0.9)
    worst = max(float((x - y).abs().max()) for x, y in zip(a.shadows[0], b))
    say(f"one update, rate 0.9: vd_ema_update vs _foreach_lerp_ max |diff| {worst:.3e}")
    del a, b
    res = {}
    for k in (1, 2):
        nbytes = (1 + 2 * k) * 4 * nel
        fns, keep = _variants(params, ema, k)
        say(f"-- k = {k}: {nbytes / 1e6:.0f} MB per update "
            f"({nbytes / COPY_TBS / 1e6:.0f} us at the copy rate)")
        if k == 2:
            fns["EMA.update()"] = ema.update
        res[k, "eager"] = _ab(f"eager k={k}", fns, 40, nbytes=nbytes)
        graphs = {name: _graphed(fn) for name, fn in fns.items() if name != "EMA.update()"}
        res[k, "graph"] = _ab(f"graph k={k}", {n: g.replay for n, g in graphs.items()}, 20,
                              per_call=PER_GRAPH, nbytes=nbytes)
        del graphs
    for mode in ("eager", "graph"):
        r1, r2 = res[1, mode], res[2, mode]
        h1, l1 = r1["vd_ema_update"], r1["foreach_lerp"]
        spread = max(l1[2] - l1[1], h1[2] - h1[1])
        say(f"{mode}: k=1 vd_ema_update {h1[0]:.1f} us vs foreach_lerp {l1[0]:.1f} us "
            f"(difference {h1[0] - l1[0]:+.1f} us, run-to-run spread {spread:.1f} us); k=2 "
            f"vd_ema_update {r2['vd_ema_update'][0]:.1f} us vs two foreach_lerp passes "
            f"{r2['foreach_lerp'][0]:.1f} us")


def chunk_sweep(model):
    say("-- chunk size sweep (graph replay, us per update)")
    for chunk in CHUNKS:
        ema = EMA(model, RATES, chunk=chunk)
        params = ema.params
        row = []
        for k in (1, 2):
            fns, keep = _variants(params, ema, k)
            g = _graphed(fns["vd_ema_update"])
            for _ in range(3):
                g.replay()
            v = [_time(g.replay, 20) / PER_GRAPH for _ in range(REPEATS)]
            row.append(f"k={k} {statistics.median(v):7.1f} ({min(v):.1f}-{max(v):.1f})")
            del g
        say(f"chunk {chunk:7d}: {ema.n_desc:6d} descriptors  " + "   ".join(row))
        del ema


def step_bench():
    import bench
    from vdiff.engine import Trainer, synthetic_clip
    from vdiff.schedulers import LinearNoiseScheduler
    dev = torch.device("cuda")
    ns = argparse.Namespace(size=128, frames=16, dtype="bf16", mode="joint", init="nonzero")
    trainers = {}
    for name, rates in (("no EMA", ()), ("ema_rates=(0.9999,)", (0.9999,))):
        torch.manual_seed(0)
        m = bench.build_model(ns, dev)
        trainers[name] = Trainer(m, LinearNoiseScheduler(100, 0.00085, 0.012), lr=1e-4,
                                 ema_rates=rates)
    clips = [synthetic_clip(1, 16, 128, 100, dev, seed=i) for i in range(4)]
    for tr in trainers.values():
        for c in clips[:3]:
            tr.step(c)
    torch.cuda.synchronize()
    res = {k: [] for k in trainers}
    for i in range(12):
        for k, tr in trainers.items():
            c = clips[i % len(clips)]
            res[k].append(_time(lambda: tr.step(c), 1) / 1e3)
    say("-- config-2 Trainer.step (1 clip x 16 x 128 x 128, bf16, eager), ms per step")
    for k, v in res.items():
        say(f"{k:22s} {statistics.median(v):8.2f} ms  ({min(v):.2f}-{max(v):.2f})")
    a, b = (statistics.median(v) for v in res.values())
    say(f"with EMA - without = {b - a:+.2f} ms ({(b / a - 1) * 100:+.2f} %)")
    for tr in trainers.values():
        tr.check_finite()


def main():
    global _out
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.txt"))
    ap.add_argument("--no-step", action="store_true", help="kernel timings only")
    ap.add_argument("--no-sweep", action="store_true", help="skip the chunk size sweep")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench: needs the GPU (no CPU timing is meaningful)")
    import bench
    _out = open(args.out, "w")
    say(torch.cuda.get_device_name(0))
    dev = torch.device("cuda")
    ns = argparse.Namespace(size=128, frames=16, dtype="bf16", mode="joint", init="nonzero")
    model = bench.build_model(ns, dev)
    kernel_bench(model)
    if not args.no_sweep:
        chunk_sweep(model)
    del model
    if not args.no_step:
        step_bench()
    _out.close()


if __name__ == "__main__":
    main()
