"""Gradient clipping on the GPU: vd_grad_sumsq / vd_grad_clip against fp64 within the bound
tests/_clip_cases.py derives, one-hot gradients at every place a tail or a descriptor could be
skipped, bit-exact scaling, the untouched no-clip and non-finite cases, graph capture of
GradClipper.clip(), and the clipping Trainer (measure-only, against a hand-written twin,
graph=True, the non-finite-gradient record, DDP over gloo) and train.py --clip-grad-norm."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _clip_cases as cases
from conftest import DROPIN, ROOT, record_metric

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0) if torch.cuda.is_available() else None

INF = float("inf")
_layout = cases.Layout()                     # numpy only: built at collection, never changed
POSITIONS = _layout.one_hot_positions()      # {what: (tensor, element)}


def layout():
    return _layout


class _Grads:
    """The list's buffer on the device, its descriptor table, workspace and record."""

    def __init__(self, host):
        from vdiff.clip import descriptor_rows
        L = layout()
        self.before = host.copy()
        self.buf = torch.from_numpy(self.before).to(dev)
        assert self.buf.data_ptr() % 16 == 0
        rows = descriptor_rows([self.buf.data_ptr() + 4 * o for o in L.offsets], L.numels)
        self.n = len(rows)
        assert self.n == len(L.ranges) > cases.N_ONES
        self.table = torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
        self.work = torch.full((self.n,), float("nan"), device=dev)
        self.record = torch.full((2,), float("nan"), device=dev)

    def run(self, max_norm):
        """(norm, coef) as numpy fp32 after one vd_grad_sumsq + vd_grad_clip."""
        from vdiff import ops
        ops.grad_sumsq(self.table, self.n, self.work)
        ops.grad_clip(self.table, self.n, self.work, max_norm, self.record)
        r = self.record.cpu().numpy()
        return r[0], r[1]

    def host(self):
        return self.buf.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


_ref = {}


def reference():
    """Computed once: the fp64 norm of the list and the measure-only norm of the kernels."""
    if not _ref:
        L = layout()
        G = _Grads(L.host)
        norm, coef = G.run(INF)
        _ref.update(ref=cases.ref_norm64(L.host, L.mask), norm=norm, coef=coef,
                    untouched=np.array_equal(_bits(G.host()), _bits(L.host)), n=G.n)
    return _ref


# ------------------------------------------------------------------ 1. norm against fp64
def test_norm_against_fp64():
    r = reference()
    b = cases.norm_bound(r["n"])
    ratio = abs(float(r["norm"]) - r["ref"]) / (b * r["ref"])
    print(f"norm {r['norm']!r} vs fp64 {r['ref']!r}: error / bound {ratio:.4f} (bound {b:.3e})")
    record_metric(test="clip_norm_vs_fp64", ratio=ratio, bound=b, ranges=r["n"])
    assert ratio <= 1.0
    assert r["coef"] == np.float32(1.0) and r["untouched"]


# ------------------------------------------------------------------ 2. one-hot positions
@pytest.mark.parametrize("what", list(POSITIONS))
def test_one_hot(what):
    L = layout()
    t, e = POSITIONS[what]
    at = L.offsets[t] + e
    host = L.zeros()
    host[at] = 3.0
    G = _Grads(host)
    norm, coef = G.run(1.5)
    assert norm == np.float32(3.0), (what, norm)
    want = 1.5 / (3.0 + 1e-6)
    assert abs(float(coef) - want) <= cases.coef_bound(G.n) * want and coef < 0.5
    got = G.host()
    expect = L.zeros()
    expect[at] = np.float32(3.0) * coef            # one fp32 multiply
    assert np.array_equal(_bits(got), _bits(expect)), what   # every other gradient stays +0


# ------------------------------------------------------------------ 3. scaling, bit for bit
def test_scaling_bit_for_bit():
    L = layout()
    r = reference()
    max_norm = float(np.float32(r["ref"] / 4))
    G = _Grads(L.host)
    before = G.buf.clone()
    norm, coef = G.run(max_norm)
    assert _bits(norm) == _bits(r["norm"])         # the same sum as the measure-only run
    want = max_norm / (r["ref"] + 1e-6)
    ratio = abs(float(coef) - want) / (cases.coef_bound(G.n) * want)
    print(f"coef {coef!r} vs {want!r}: error / bound {ratio:.4f}")
    assert ratio <= 1.0 and coef < 1
    mask = torch.from_numpy(L.mask).to(dev)
    scaled = before * G.record[1]                  # torch, fp32, the same device: one multiply
    assert torch.equal(G.buf[mask], scaled[mask])
    assert torch.equal(G.buf[~mask].view(torch.int32), before[~mask].view(torch.int32))
    assert not torch.equal(G.buf[mask], before[mask])
    norm2, coef2 = G.run(INF)                      # measured again
    assert norm2 <= max_norm * (1 + cases.clipped_norm_bound(G.n)), (norm2, max_norm)
    assert norm2 >= max_norm * (1 - 2 * cases.clipped_norm_bound(G.n)) and coef2 == 1


# ------------------------------------------------------------------ 4. no clipping
@pytest.mark.parametrize("factor", [4.0, INF])
def test_no_clipping_leaves_every_bit(factor):
    L = layout()
    r = reference()
    max_norm = INF if factor == INF else float(np.float32(r["ref"] * factor))
    G = _Grads(L.host)
    for _ in range(2):                             # run twice: the same bits
        norm, coef = G.run(max_norm)
        assert _bits(norm) == _bits(r["norm"])
        assert coef == np.float32(1.0)
        assert np.array_equal(_bits(G.host()), _bits(L.host))


# ------------------------------------------------------------------ 5. non-finite inputs
@pytest.mark.parametrize("case", ["nan", "inf", "overflow"])
@pytest.mark.parametrize("max_norm", [1.0, INF])
def test_nonfinite_gradients_are_left_alone(case, max_norm):
    L = layout()
    host = L.host.copy()
    big = L.offsets[cases.SIZES.index(2 * cases.C + 3)]
    if case == "nan":
        host[big + cases.C + 11] = np.nan
    elif case == "inf":
        host[L.offsets[-1]] = np.inf               # the last one-element tensor
    else:
        host[big + 5] = host[L.offsets[len(cases.SIZES) + 1] + 3] = 3e19   # squares overflow
    G = _Grads(host)
    norm, coef = G.run(max_norm)
    assert not np.isfinite(norm), (case, norm)
    assert coef == np.float32(1.0)
    assert np.array_equal(_bits(G.host()), _bits(host))


def test_all_zero_gradients():
    L = layout()
    G = _Grads(L.zeros())
    norm, coef = G.run(1.0)
    assert norm == 0 and coef == np.float32(1.0)
    got = G.host()
    assert not np.isnan(got).any() and np.array_equal(_bits(got), _bits(L.zeros()))


# ------------------------------------------------------------------ 6. graph capture
def _views(buf):
    L = layout()
    return [buf[o:o + n] for o, n in zip(L.offsets, L.numels)]


def test_graph_capture_of_clip():
    """One GradClipper.clip() over static gradient buffers, captured once and replayed with
    the gradients refilled between replays so that some steps clip and some do not: every
    gradient and record equals the eager call's, bit for bit."""
    from vdiff import hipgraph
    from vdiff.clip import KERNEL_LAUNCHES, GradClipper
    L = layout()
    r = reference()
    max_norm = float(np.float32(r["ref"] / 2))
    src = torch.from_numpy(L.host).to(dev)
    eager_buf, graph_buf = src.clone(), src.clone()
    assert eager_buf.data_ptr() % 16 == 0 and graph_buf.data_ptr() % 16 == 0
    eager, graphed = GradClipper(max_norm), GradClipper(max_norm)
    ev, gv = _views(eager_buf), _views(graph_buf)
    graphed.clip(gv)                               # builds and uploads the table
    assert graphed.rebuilds == 1 and graphed.n_desc == r["n"]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with hipgraph.capture(g):
        graphed.clip(gv)
    g.instantiate()
    counts = hipgraph.node_counts(g)
    assert counts.get("memset", 0) == 0 and counts.get("kernel", 0) == KERNEL_LAUNCHES == 3, counts
    assert set(counts) == {"kernel"}, counts
    assert graphed.rebuilds == 1
    clipped = []
    guard = ~torch.from_numpy(L.mask).to(dev)
    for scale in (1.0, 0.25, 3.0, 0.5 - 1e-3, 1e-3, 1.0):
        filled = src * scale
        for buf in (eager_buf, graph_buf):
            buf.copy_(filled)
        eager.clip(ev)
        g.replay()
        assert torch.equal(eager_buf.view(torch.int32), graph_buf.view(torch.int32)), scale
        assert torch.equal(eager.norm, graphed.norm) and torch.equal(eager.coef, graphed.coef)
        assert torch.equal(graph_buf[guard], filled[guard])
        clipped.append(bool(graphed.coef < 1))
        if clipped[-1]:
            assert torch.equal(graph_buf[~guard], (filled * graphed.coef)[~guard])
        else:
            assert torch.equal(graph_buf.view(torch.int32), filled.view(torch.int32))
    assert clipped == [True, False, True, False, False, True], clipped
    assert eager.rebuilds == 1
    # a list at other addresses rebuilds the table; the same list again does not
    other = src.clone()
    eager.clip(_views(other))
    assert float(eager.norm) == float(r["norm"])
    eager.clip(_views(other))
    assert eager.rebuilds == 2


# ------------------------------------------------------------------ 7. argument checks
def test_argument_checks():
    from vdiff import ops
    from vdiff.clip import GradClipper
    L = layout()
    G = _Grads(L.host)
    c = GradClipper(1.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        c.clip([torch.zeros(8)])
    with pytest.raises(TypeError, match="w.*bfloat16"):
        c.clip([torch.zeros(8, device=dev), torch.zeros(8, device=dev, dtype=torch.bfloat16)],
               ["b", "w"])
    with pytest.raises(ValueError, match="contiguous.*tensor 0"):
        c.clip([torch.zeros(8, 8, device=dev).t()])
    assert c.rebuilds == 0 and c.norm is None
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="vd_grad_clip"):
            ops.grad_clip(G.table, G.n, G.work, bad, G.record)
        with pytest.raises(ValueError):
            GradClipper(bad)
    with pytest.raises(RuntimeError, match="vd_grad_sumsq.*workspace"):
        ops.grad_sumsq(G.table, G.n, G.work[:G.n - 1])
    with pytest.raises(ValueError):
        ops.grad_clip(G.table, G.n, G.work[:G.n - 1], 1.0, G.record)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.grad_sumsq(G.table.cpu(), G.n, G.work)
    with pytest.raises(ValueError):
        ops.grad_sumsq(G.table[:16 * G.n - 1], G.n, G.work)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(G.host()), _bits(L.host))        # nothing ran
    assert torch.isnan(G.record).all()


# ------------------------------------------------------------------ Trainer
def _model(seed=4321):
    """The tiny 3-D UNetAudio of tests/test_gpu_ema.py, fp32."""
    from vdiff.engine import reinit_nonzero
    from vdiff.unet_audio import UNetAudio
    torch.manual_seed(seed)
    m = UNetAudio(image_size=32, in_channels=3, model_channels=32, out_channels=3,
                  num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2),
                  audio_feature_dim=64, projected_audio_dim=32, dims=3, use_bf16=False,
                  audio_encoder=False, dropout=0.0)
    reinit_nonzero(m, seed=seed)
    return m.to(dev)


def _clip(B=2, seed=0):
    from vdiff.engine import Clip
    g = torch.Generator(device=dev).manual_seed(100 + seed)
    T = 2
    x0 = torch.rand((B, 3, T, 32, 32), generator=g, device=dev) * 2 - 1
    cond = torch.rand((B, 3, 32, 32), generator=g, device=dev) * 2 - 1
    eps = torch.randn((B, 3, T, 32, 32), generator=g, device=dev)
    t = torch.randint(0, 100, (B,), generator=g, device=dev)
    feats = torch.randn((B * T, 64), generator=g, device=dev)
    return Clip(x0, cond, feats, eps, t)


def _sched():
    from vdiff.schedulers import LinearNoiseScheduler
    return LinearNoiseScheduler(100, 0.00085, 0.012)


def _trainer(m, **kw):
    from vdiff.engine import Trainer
    return Trainer(m, _sched(), lr=1e-3, **kw)


def _params(m):
    return [p.detach().clone() for p in m.parameters()]


def _three_steps(tr, m):
    """[(parameters, norm, coef) after each of three steps]; norm / coef None without clipping."""
    out = []
    for s in range(3):
        tr.step(_clip(seed=s))
        rec = (None, None) if tr.grad_norm is None else (tr.grad_norm.clone(), tr.clip_coef.clone())
        out.append((_params(m),) + rec)
    tr.check_finite()
    return out


_runs = {}


def runs():
    """Run once: three steps without the option, with clip_grad_norm=inf, and with
    clip_grad_norm = c = half the first measured norm."""
    if not _runs:
        m = _model()
        tr = _trainer(m)
        assert tr.clipper is None and tr.grad_norm is None
        _runs["plain"] = _three_steps(tr, m)
        m = _model()
        tr = _trainer(m, clip_grad_norm=INF)
        _runs["inf"] = _three_steps(tr, m)
        _runs["inf_rebuilds"] = tr.clipper.rebuilds
        _runs["c"] = float(_runs["inf"][0][1]) / 2      # a host read of that run's first norm
        m = _model()
        tr = _trainer(m, clip_grad_norm=_runs["c"])
        _runs["clipped"] = _three_steps(tr, m)
        _runs["n_desc"] = tr.clipper.n_desc
    return _runs


def test_trainer_measure_only_changes_nothing():
    r = runs()
    for s, (a, b) in enumerate(zip(r["plain"], r["inf"])):
        assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])), s
        assert torch.isfinite(b[1]) and float(b[1]) > 0 and float(b[2]) == 1.0
    assert not torch.equal(r["plain"][0][0][0], r["plain"][2][0][0])     # the weights moved
    print(f"table rebuilds over three eager steps: {r['inf_rebuilds']}")
    assert r["inf_rebuilds"] >= 1


def test_trainer_clipping_against_a_hand_written_twin():
    from vdiff import ops
    r = runs()
    c = r["c"]
    m = _model()
    m.train()
    params = [p for p in m.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-3, fused=True)
    sched = _sched()
    packs = ops.step_packed_weights()
    bound = cases.norm_bound(r["n_desc"])
    coefs = []
    for s in range(3):
        clip = _clip(seed=s)
        want_params, norm, coef = r["clipped"][s]
        with packs:
            xt = sched.add_noise(clip.x0, clip.eps, clip.t)
            loss = ops.mse_loss(m(xt, clip.cond, clip.audio, clip.t), clip.eps)
            loss.backward()
        grads = [p.grad for p in params if p.grad is not None]
        ref = float(torch.sqrt(sum((g.detach().clone().double() ** 2).sum() for g in grads)))
        ratio = abs(float(norm) - ref) / (bound * ref)
        print(f"step {s}: norm {float(norm)!r} vs fp64 {ref!r}, error / bound {ratio:.4f}, "
              f"coef {float(coef)!r}")
        record_metric(test="clip_trainer_norm_vs_fp64", step=s, ratio=ratio)
        assert ratio <= 1.0
        want = min(1.0, c / (ref + 1e-6))
        assert abs(float(coef) - want) <= cases.coef_bound(r["n_desc"]) * want
        with torch.no_grad():
            for g in grads:
                g.mul_(coef)                       # the trainer's recorded coef, one multiply
        opt.step()
        opt.zero_grad(set_to_none=True)
        for n, x, y in zip((n for n, _ in m.named_parameters()), m.parameters(), want_params):
            assert torch.equal(x.detach(), y), (s, n)
        coefs.append(float(coef))
    assert coefs[0] < 1 and min(coefs) < 1
    # and clipping changed the run
    assert not all(torch.equal(x, y) for x, y in zip(r["clipped"][2][0], r["plain"][2][0]))


def test_trainer_graph_equals_eager(monkeypatch):
    monkeypatch.setenv("VDIFF_TRAIN_GRAPH_EXPERIMENTAL", "1")
    r = runs()
    m = _model()
    tr = _trainer(m, clip_grad_norm=r["c"], graph=True)
    got = _three_steps(tr, m)
    assert tr.graph.g is not None
    for s, (a, b) in enumerate(zip(got, r["clipped"])):
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (s, a[1], b[1])
        assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])), s


def test_nonfinite_gradient_with_a_finite_loss():
    r = runs()
    m = _model()
    tr = _trainer(m, clip_grad_norm=r["c"], ema_rates=(0.5, 0.9), check_every=100)
    steps = []
    victim = [p for p in m.parameters() if p.requires_grad][-1]
    victim.register_hook(lambda g: g * float("nan") if len(steps) == 2 else g)
    losses = []
    for s in range(3):
        steps.append(s)
        losses.append(tr.step(_clip(seed=s)).clone())
        if s == 0:
            after0 = [[x.clone() for x in sh] for sh in tr.ema.shadows]
        if s == 1:
            assert not torch.isfinite(tr.grad_norm) and float(tr.clip_coef) == 1.0
    assert torch.isfinite(losses[0]) and torch.isfinite(losses[1])     # the loss saw nothing
    assert not torch.isfinite(victim).all()        # the optimizer step is not prevented
    assert not torch.equal(after0[0][0], after0[1][0])
    for sh, ref in zip(tr.ema.shadows, after0):
        for x, a in zip(sh, ref):
            assert torch.isfinite(x).all() and torch.equal(x, a)
    with pytest.raises(FloatingPointError, match=r"gradient norm.* step 1 "):
        tr.check_finite()
    # without clipping the same step goes unnoticed by the record
    m = _model()
    tr = _trainer(m, check_every=100)
    victim = [p for p in m.parameters() if p.requires_grad][-1]
    victim.register_hook(lambda g: g * float("nan"))
    tr.step(_clip(seed=0))
    tr.check_finite()


# ------------------------------------------------------------------ DDP
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_ddp_ranks_clip_identically(tmp_path):
    out = str(tmp_path / "clip")
    port = _port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), VDIFF_DIST_BACKEND="gloo")
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "tests", "_clip_ddp_worker.py"), out], env=env,
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=240)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    a, b = (torch.load(f"{out}.rank{r}.pt", weights_only=True) for r in range(2))
    assert a["bucketed"] and b["bucketed"] and a["buckets"] >= 2
    assert list(a["params"]) == list(b["params"]) and len(a["params"]) > 10
    moved = 0
    for n in a["params"]:
        assert torch.equal(a["params"][n], b["params"][n]), n
        assert torch.isfinite(a["params"][n]).all()
        moved += int(not torch.equal(a["params"][n], a["initial"][n]))
    assert moved > 10
    assert torch.equal(a["params"]["spare"], a["initial"]["spare"])   # no rank used it
    assert len(a["records"]) == 2 and a["rebuilds"] == b["rebuilds"] == 1
    for (na, ca), (nb, cb) in zip(a["records"], b["records"]):
        assert torch.equal(na, nb) and torch.equal(ca, cb)
        assert torch.isfinite(na) and float(na) > 0 and float(ca) < 1
    # the flag tail after the clipped average: 1 (two ranks of two) where used, 0 for the
    # spare parameter -- a scaled flag would hold coef
    for d in (a, b):
        spare = d["spare_index"]
        for flags, unused in zip(d["flags"], d["unused"]):
            want = torch.ones_like(flags)
            want[spare] = 0.0
            assert torch.equal(flags, want), flags
            assert unused == [spare]


# ------------------------------------------------------------------ entry point
SMALL = ["--dims", "3", "--frames", "2", "--image-size", "32", "--random-audio-encoder",
         "--batch-size", "1", "--epochs", "1", "--steps-per-epoch", "2", "--lr", "1e-4"]


def _train(args, cwd):
    out = subprocess.run([sys.executable, os.path.join(DROPIN, "train.py")] + args, cwd=cwd,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


def test_train_entry_prints_the_norm_fields(tmp_path):
    import re
    ck = str(tmp_path / "m.pth")
    out = _train(SMALL + ["--ckpt", ck, "--clip-grad-norm", "0.5"], tmp_path)
    line = [ln for ln in out.splitlines() if ln.startswith("Finished epoch 1")][0]
    m = re.search(r"\| grad norm (\S+) \(max (\S+)\) \| clipped (\d)/2 steps \|", line)
    assert m, line
    last, top, k = float(m.group(1)), float(m.group(2)), int(m.group(3))
    assert 0 < last <= top * (1 + 1e-3) and 0 <= k <= 2
    assert (k == 0) == (top <= 0.5) or abs(top - 0.5) < 1e-3     # printed with 4 digits
    res = torch.load(ck + ".resume", map_location="cpu", weights_only=True)
    assert sorted(res) == ["epoch", "model", "optimizer"]


def test_train_entry_without_the_flag_is_unchanged(tmp_path):
    ck = str(tmp_path / "m.pth")
    out = _train(SMALL + ["--ckpt", ck], tmp_path)
    line = [ln for ln in out.splitlines() if ln.startswith("Finished epoch 1")][0]
    assert "grad norm" not in out and "clipped" not in out
    assert line.count("|") == 3, line
    res = torch.load(ck + ".resume", map_location="cpu", weights_only=True)
    assert sorted(res) == ["epoch", "model", "optimizer"]
