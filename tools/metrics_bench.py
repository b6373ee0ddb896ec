"""Clip metrics (vd_clip_metrics: per-frame MSE and SSIM in two launches) against a plain torch
implementation on the same GPU, at the sampling workload's shapes (1, 3, 16, 128, 128) and (1, 3,
32, 128, 128), fp32.  The torch leg is what one would write without the kernel: range mapping,
the five moment maps through one grouped fp32 F.conv2d with the 11 x 11 window, E[x^2] - mu^2, the
SSIM formula, the per-frame means and the MSE -- a dozen launches and temporaries per call.

Each leg is timed two ways, the two legs alternating in one process (round robin, median of the
rounds): eager calls, which include the host's cost of issuing the launches and torch's
allocations, and CALLS calls captured into one HIP graph, which leaves the kernels' time.  HIP
events over enough repeats to span > 0.25 s after warm-up.  Before timing, the two legs' results
are compared on the same seeded input.  One short run; no pass/fail threshold.

    python tools/metrics_bench.py [--out FILE]
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lipreading-video-generation_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vdiff import ops  # noqa: E402

SHAPES = [(1, 3, 16, 128, 128), (1, 3, 32, 128, 128)]
ROUNDS = 5
CALLS = 20
SPAN_MS = 250.0
C1, C2 = 0.01 ** 2, 0.03 ** 2


def timeit(fn):
    """ms per call: 3 warm-up calls, a calibration of 5, then repeats spanning SPAN_MS."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    e0.record()
    for _ in range(5):
        fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(10, int(SPAN_MS / max(e0.elapsed_time(e1) / 5, 1e-3)) + 1)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def graph_of(call):
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            call()
    return g.replay


def torch_window(device):
    d = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-d * d / (2.0 * 1.5 ** 2))
    g = (g / g.sum()).float()
    return torch.outer(g, g).to(device).view(1, 1, 11, 11).repeat(5, 1, 1, 1).contiguous()


def torch_metrics(x, y, k5):
    """(mse, ssim) [B, T] of clips [B, C, T, H, W] in [-1, 1]: plain fp32 torch."""
    B, C, T, H, W = x.shape
    u = ((x + 1) * 0.5).clamp(0, 1).reshape(B * C * T, 1, H, W)
    v = ((y + 1) * 0.5).clamp(0, 1).reshape(B * C * T, 1, H, W)
    m = F.conv2d(torch.cat([u, v, u * u, v * v, u * v], dim=1), k5, groups=5)
    mx, my, exx, eyy, exy = m.unbind(dim=1)
    vx, vy, cxy = exx - mx * mx, eyy - my * my, exy - mx * my
    s = ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    ssim = s.view(B, C, T, -1).mean(dim=(1, 3))
    mse = ((u - v) ** 2).view(B, C, T, -1).mean(dim=(1, 3))
    return mse, ssim


def main():
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench: needs the GPU (no timing is taken on a CPU)")
    emit(f"clip metrics, fp32, {torch.cuda.get_device_name(0)}; us per call, median of {ROUNDS} "
         f"interleaved rounds; graph = {CALLS} calls per replay")
    emit(f"{'shape':>22} | {'kernel eager':>12} {'torch eager':>11} {'t/k':>6} | "
         f"{'kernel graph':>12} {'torch graph':>11} {'t/k':>6} | max |dssim| |dmse|/mse")
    k5 = torch_window("cuda")
    for shape in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(5)
        x = torch.rand(shape, generator=g, device="cuda") * 2 - 1
        y = (x + 0.1 * torch.randn(shape, generator=g, device="cuda")).clamp(-1, 1)
        r = ops.clip_metrics(x, y)
        tm, ts = torch_metrics(x, y, k5)
        dss = float((r.ssim - ts).abs().max())
        dms = float(((r.mse - tm).abs() / tm).max())
        legs = {"kernel": lambda: ops.clip_metrics(x, y),
                "torch": lambda: torch_metrics(x, y, k5)}
        replays = {"kernel": graph_of(legs["kernel"])}
        try:
            replays["torch"] = graph_of(legs["torch"])
        except RuntimeError as e:  # a library call that refuses stream capture: eager time only
            emit(f"torch leg not captured: {str(e).splitlines()[0]}")
            torch.cuda.synchronize()
        t = {(k, m): [] for k in legs for m in ("eager", "graph")}
        for _ in range(ROUNDS):
            for k in legs:
                t[k, "eager"].append(timeit(legs[k]) * 1e3)
                t[k, "graph"].append(timeit(replays[k]) / CALLS * 1e3 if k in replays
                                     else float("nan"))
        m = {key: statistics.median(v) for key, v in t.items()}
        emit(f"{str(shape):>22} | {m['kernel', 'eager']:12.1f} {m['torch', 'eager']:11.1f} "
             f"{m['torch', 'eager'] / m['kernel', 'eager']:6.1f} | {m['kernel', 'graph']:12.1f} "
             f"{m['torch', 'graph']:11.1f} {m['torch', 'graph'] / m['kernel', 'graph']:6.1f} | "
             f"{dss:.2e} {dms:.2e}")
        del replays
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
