"""FiLM-conditioned GroupNorm+SiLU+dropout (ops.group_norm_film_silu) at the nine GroupNorm
shapes of the UNet3D 128x128x16 train step (tools/gn_bench.py's list), bf16, dropout 0.1,
against (2) the plain ops.group_norm_silu and (3) the composition a user would write without
the fused op: group_norm_silu(silu=False), the torch multiply-add, ops.silu, torch dropout.
The three legs are interleaved in one process (round robin, median of the rounds), forward
alone and forward + backward, timed with HIP events over enough repeats to span > 0.25 s.

--step also times one config-2 train step (128x128x16, bf16, dropout 0.1, pooled audio
features) of a model with and without use_scale_shift_norm, alternating step by step.

--capi times the C-ABI calls alone (vd_groupnorm_film_silu_* against vd_groupnorm_silu_*, back
to back on preallocated buffers, no autograd), which separates the kernels' time from the host
work of the torch wrappers at the shapes where a call is shorter than its launches take to
issue; --only C restricts the shapes to one channel count.

    python tools/film_bench.py [--capi] [--only C] [--step] [--out FILE]
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lipreading-video-generation_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vdiff import ops  # noqa: E402

from gn_bench import SHAPES  # noqa: E402

P_DROP = 0.1
ROUNDS = 3
SPAN_MS = 250.0


def timeit(fn):
    """us per call: 3 warm-up calls, a calibration of 5, then repeats spanning SPAN_MS."""
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
    return e0.elapsed_time(e1) / reps * 1e3


def legs(C, T, H):
    x = ops.to_cl(torch.randn(1, C, T, H, H, device="cuda").bfloat16()).requires_grad_(True)
    w = torch.randn(C, device="cuda", requires_grad=True)
    b = torch.randn(C, device="cuda", requires_grad=True)
    film = (0.5 * torch.randn(1, 2 * C, device="cuda")).requires_grad_(True)
    g = ops.to_cl(torch.randn(1, C, T, H, H, device="cuda").bfloat16())

    def film_op(x, w, b, film):
        return ops.group_norm_film_silu(x, w, b, film, dropout=P_DROP, seed=1)

    def plain(x, w, b, film):
        return ops.group_norm_silu(x, w, b, dropout=P_DROP, seed=1)

    def unfused(x, w, b, film):
        h = ops.group_norm_silu(x, w, b, silu=False)
        s, t = film.to(h.dtype).reshape(1, 2 * C, 1, 1, 1).chunk(2, dim=1)
        return F.dropout(ops.silu(h * (1 + s) + t), P_DROP, True)

    out = {}
    for name, fn in (("film", film_op), ("plain", plain), ("unfused", unfused)):
        ins = (x, w, b, film) if name != "plain" else (x, w, b)

        def fwd(fn=fn):
            with torch.no_grad():
                fn(x, w, b, film)

        def fwd_bwd(fn=fn, ins=ins):
            torch.autograd.grad(fn(x, w, b, film), ins, g)

        out[name] = (fwd, fwd_bwd)
    return out


def bench_shapes(emit, shapes):
    emit("FiLM GroupNorm+SiLU+dropout(0.1), bf16, B = 1; us per call, median of "
         f"{ROUNDS} interleaved rounds")
    emit(f"{'C':>4} {'TxHxW':>11} | {'fwd film':>9} {'plain':>8} {'unfused':>8} {'f/p':>5} "
         f"{'u/f':>5} | {'f+b film':>9} {'plain':>8} {'unfused':>8} {'f/p':>5} {'u/f':>5}")
    tot = {k: [0.0, 0.0] for k in ("film", "plain", "unfused")}
    for C, T, H in shapes:
        fns = legs(C, T, H)
        t = {k: ([], []) for k in fns}
        for _ in range(ROUNDS):
            for k, (fwd, fb) in fns.items():
                t[k][0].append(timeit(fwd))
                t[k][1].append(timeit(fb))
        m = {k: (statistics.median(v[0]), statistics.median(v[1])) for k, v in t.items()}
        for k in tot:
            tot[k][0] += m[k][0]
            tot[k][1] += m[k][1]
        emit(f"{C:4d} {T:3d}x{H}x{H:<3d} | " + " | ".join(
            f"{m['film'][i]:9.1f} {m['plain'][i]:8.1f} {m['unfused'][i]:8.1f} "
            f"{m['film'][i] / m['plain'][i]:5.2f} {m['unfused'][i] / m['film'][i]:5.2f}"
            for i in (0, 1)))
    emit(f"{'sum':>16} | " + " | ".join(
        f"{tot['film'][i]:9.1f} {tot['plain'][i]:8.1f} {tot['unfused'][i]:8.1f} "
        f"{tot['film'][i] / tot['plain'][i]:5.2f} {tot['unfused'][i] / tot['film'][i]:5.2f}"
        for i in (0, 1)))


def capi_legs(C, T, H):
    from vdiff import _lib
    B, S, G = 1, T * H * H, 32
    x = torch.randn(B, S, C, device="cuda").bfloat16()
    dy = torch.randn(B, S, C, device="cuda").bfloat16()
    y, dx = torch.empty_like(x), torch.empty_like(x)
    g32, b32 = torch.randn(C, device="cuda"), torch.randn(C, device="cuda")
    film = 0.5 * torch.randn(B, 2 * C, device="cuda")
    dfilm = torch.empty_like(film)
    mean = torch.empty(B * G, device="cuda")
    rstd = torch.empty_like(mean)
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    ws = torch.empty(_lib.lib().vd_groupnorm_workspace_size(B, S, C, G), dtype=torch.uint8,
                     device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    dt = ops._DT[torch.bfloat16]
    p = lambda t: t.data_ptr()  # noqa: E731

    def film_fwd():
        _lib.call("vd_groupnorm_film_silu_fwd", p(x), p(g32), p(b32), p(film), p(y), p(mean),
                  p(rstd), B, S, C, G, 1e-5, 1, P_DROP, 1, dt, p(ws), st)

    def film_bwd():
        _lib.call("vd_groupnorm_film_silu_bwd_add", p(x), p(dy), None, p(g32), p(b32), p(film),
                  p(mean), p(rstd), p(dx), p(dg), p(db), p(dfilm), B, S, C, G, 1, P_DROP, 1, dt,
                  p(ws), st)

    def plain_fwd():
        _lib.call("vd_groupnorm_silu_fwd", p(x), p(g32), p(b32), p(y), p(mean), p(rstd), B, S, C,
                  G, 1e-5, 1, P_DROP, 1, dt, p(ws), st)

    def plain_bwd():
        _lib.call("vd_groupnorm_silu_bwd_add", p(x), p(dy), None, p(g32), p(b32), p(mean),
                  p(rstd), p(dx), p(dg), p(db), B, S, C, G, 1, P_DROP, 1, dt, p(ws), st)

    film_fwd()  # mean / rstd for the backward calls
    return {"film": (film_fwd, film_bwd), "plain": (plain_fwd, plain_bwd)}


def bench_capi(emit, shapes):
    emit("C-ABI calls alone (no autograd), bf16, B = 1, dropout 0.1; us per call, median of "
         f"{ROUNDS} interleaved rounds")
    emit(f"{'C':>4} {'TxHxW':>11} | {'fwd film':>9} {'plain':>8} {'f/p':>5} | {'bwd film':>9} "
         f"{'plain':>8} {'f/p':>5}")
    tot = {"film": [0.0, 0.0], "plain": [0.0, 0.0]}
    for C, T, H in shapes:
        fns = capi_legs(C, T, H)
        t = {k: ([], []) for k in fns}
        for _ in range(ROUNDS):
            for k, (fwd, bwd) in fns.items():
                t[k][0].append(timeit(fwd))
                t[k][1].append(timeit(bwd))
        m = {k: (statistics.median(v[0]), statistics.median(v[1])) for k, v in t.items()}
        for k in tot:
            tot[k][0] += m[k][0]
            tot[k][1] += m[k][1]
        emit(f"{C:4d} {T:3d}x{H}x{H:<3d} | " + " | ".join(
            f"{m['film'][i]:9.1f} {m['plain'][i]:8.1f} {m['film'][i] / m['plain'][i]:5.2f}"
            for i in (0, 1)))
    emit(f"{'sum':>16} | " + " | ".join(
        f"{tot['film'][i]:9.1f} {tot['plain'][i]:8.1f} {tot['film'][i] / tot['plain'][i]:5.2f}"
        for i in (0, 1)))


def bench_step(emit, size=128, frames=16, steps=10):
    from vdiff.engine import Clip, Trainer, reinit_nonzero
    from vdiff.schedulers import LinearNoiseScheduler
    from vdiff.unet_audio import UNetAudio
    trainers = {}
    for flag in (False, True):
        torch.manual_seed(1234)
        m = UNetAudio(image_size=size, in_channels=3, model_channels=64, out_channels=3,
                      num_res_blocks=2, attention_resolutions=(1, 2, 4), channel_mult=(1, 2, 4),
                      audio_feature_dim=768, projected_audio_dim=128, dims=3, use_bf16=True,
                      audio_encoder=False, dropout=P_DROP, use_scale_shift_norm=flag)
        reinit_nonzero(m, seed=1234)
        trainers[flag] = Trainer(m.to("cuda"), LinearNoiseScheduler(100, 0.00085, 0.012),
                                 lr=1e-4)
    gen = torch.Generator(device="cuda").manual_seed(7)
    x0 = torch.rand((1, 3, frames, size, size), generator=gen, device="cuda") * 2 - 1
    cond = torch.rand((1, 3, size, size), generator=gen, device="cuda") * 2 - 1
    feat = torch.randn((frames, 768), generator=gen, device="cuda")
    eps = torch.randn(x0.shape, generator=gen, device="cuda")
    clip = Clip(x0, cond, feat, eps, torch.tensor([37], device="cuda"))
    times = {False: [], True: []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(3 + steps):
        for flag in (False, True):
            e0.record()
            trainers[flag].step(clip)
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                times[flag].append(e0.elapsed_time(e1))
    off, on = statistics.median(times[False]), statistics.median(times[True])
    emit(f"config-2 train step ({size}x{size}x{frames}, bf16, dropout {P_DROP}), median of "
         f"{steps} alternating steps: plain {off:.2f} ms, use_scale_shift_norm {on:.2f} ms, "
         f"difference {on - off:+.2f} ms ({(on / off - 1) * 100:+.2f} %)")


def main():
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    shapes = SHAPES
    if "--only" in sys.argv:
        only = int(sys.argv[sys.argv.index("--only") + 1])
        shapes = tuple(s for s in SHAPES if s[0] == only)
    if "--capi" in sys.argv:
        bench_capi(emit, shapes)
    else:
        bench_shapes(emit, shapes)
    if "--step" in sys.argv:
        bench_step(emit)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
