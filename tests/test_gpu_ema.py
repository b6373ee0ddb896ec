"""Weight EMA on the GPU: vd_ema_update against the fp64 reference within the bound that
tests/test_ema_host.py derives, its skip flag, rate fusion, drift over 200 updates, graph
capture of EMA.update(), and the EMA kept by Trainer (eager, graph=True, the non-finite-loss
guard, DDP over gloo) and by the train.py / test.py entry points."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _ema_cases as cases
from conftest import DROPIN, ROOT

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0) if torch.cuda.is_available() else None

GUARD = 8            # untouched elements in front of and behind every shadow
SENTINEL = 12345.0
RATES = (0.0, 0.5, 0.999, 0.9999)


# ------------------------------------------------------------------ the tensor list
class _Tensors:
    """Parameters: one tensor per size of cases.SIZES (16-B aligned), three slices of one
    buffer starting at element offsets 1, 2 and 3 (4-byte aligned), and cases.N_ONES
    one-element tensors cut from one buffer.  Shadows: four slots (one per rate), each one
    flat buffer holding every tensor's shadow between guard bands of SENTINEL; the shadow of
    a tensor has its parameter's alignment."""

    def __init__(self):
        rng = np.random.default_rng(2024)
        C = cases.C
        self.numels, p_off, self.s_off = [], [], []
        # (numel, misalignment in elements)
        spec = [(n, 0) for n in cases.SIZES] + [(37, 1), (C + 5, 2), (2 * C + 1, 3)]
        pos = spos = 0
        for n, mis in spec:
            pos = -(-pos // 8) * 8 + mis            # parameters: packed, aligned + mis
            spos = -(-(spos + GUARD) // 8) * 8 + mis
            self.numels.append(n)
            p_off.append(pos)
            self.s_off.append(spos)
            pos += n
            spos += n
        pos = -(-pos // 8) * 8
        for i in range(cases.N_ONES):               # one-element tensors, 2 guards between
            self.numels.append(1)
            p_off.append(pos + i)
            self.s_off.append(spos + GUARD + 3 * i)
        pos += cases.N_ONES
        spos += GUARD + 3 * cases.N_ONES + GUARD
        self.p_off = p_off
        scale = 10.0 ** rng.integers(-3, 3, pos)
        self.p_host = (rng.standard_normal(pos) * scale).astype(np.float32)
        self.mask = np.zeros(spos, bool)            # True where a shadow lives
        for o, n in zip(self.s_off, self.numels):
            assert not self.mask[o - 1:o + n + 1].any()   # at least one guard on either side
            self.mask[o:o + n] = True
        self.p_in_s = np.zeros(spos, np.float32)    # the parameter under each shadow element
        for po, so, n in zip(p_off, self.s_off, self.numels):
            self.p_in_s[so:so + n] = self.p_host[po:po + n]
        self.s_host = []
        for j in range(4):
            s = np.full(spos, SENTINEL, np.float32)
            noise = rng.standard_normal(spos) * 10.0 ** rng.integers(-4, 1, spos)
            s[self.mask] = (self.p_in_s * (1 + noise)).astype(np.float32)[self.mask]
            self.s_host.append(s)
        self.p = torch.from_numpy(self.p_host).to(dev)

    def fresh_shadows(self):
        return [torch.from_numpy(s).to(dev) for s in self.s_host]

    def table(self, shadows, slots):
        """Device descriptor table with the shadow buffers `shadows[j]` in dst slot j for j in
        slots (in order); the other dst slots are null."""
        from vdiff.ema import descriptor_rows
        src = [self.p.data_ptr() + 4 * o for o in self.p_off]
        dst = [[shadows[j].data_ptr() + 4 * o for o in self.s_off] for j in slots]
        rows = descriptor_rows(src, dst, self.numels)
        t = torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
        return t, len(rows)


_tensors = None


def tensors():
    global _tensors
    if _tensors is None:
        _tensors = _Tensors()
        assert _tensors.p.data_ptr() % 16 == 0
    return _tensors


def _scalar(v):
    return torch.tensor(v, dtype=torch.int64, device=dev)


def _check_update(T, got, before, d, what):
    """got (device buffer of one slot) against the fp64 update of `before` at decay d on the
    shadow elements, bit-equal to `before` on the guard bands."""
    got = got.cpu().numpy()
    assert np.array_equal(got[~T.mask], before[~T.mask]), f"{what}: guard band written"
    m = T.mask
    ref = cases.ref64(T.p_in_s[m], before[m], d)
    b = cases.bound(T.p_in_s[m], before[m], d)
    err = np.abs(got[m].astype(np.float64) - ref)
    bad = err > b
    ratio = float((err[b > 0] / b[b > 0]).max())
    print(f"{what}: d={float(d):.7g} largest error / bound {ratio:.4f}")
    assert not bad.any(), (what, int(bad.sum()), ratio)
    assert np.isfinite(got[m]).all()


CASES = [((r,), False, 0) for r in RATES] + [
    ((0.0, 0.9999), False, 0), ((0.5, 0.999), False, 0), (RATES, False, 0),
    ((0.5, 0.9999), True, 0), ((0.5, 0.9999), True, 1), ((0.5, 0.9999), True, 89),
    ((0.5, 0.9999), True, 10 ** 6), ((0.9999,), True, 89), (RATES, True, 89)]


@pytest.mark.parametrize("rates,warmup,count", CASES)
def test_one_update_against_fp64(rates, warmup, count):
    from vdiff import ops
    T = tensors()
    k = len(rates)
    sh = T.fresh_shadows()
    # every slot of the table is filled: the slots >= k must stay unread and unwritten
    table, n = T.table(sh, range(4))
    assert n > cases.N_ONES
    num = _scalar(count)
    ops.ema_update(table, n, rates, warmup, num if warmup else None, None)
    torch.cuda.synchronize()
    assert int(num) == count    # read, never written
    for j in range(4):
        if j < k:
            _check_update(T, sh[j], T.s_host[j], cases.decay32(rates[j], warmup, count),
                          f"k={k} slot {j} warmup={warmup} n={count}")
        else:
            assert np.array_equal(sh[j].cpu().numpy(), T.s_host[j]), f"unused slot {j} written"
    assert np.array_equal(T.p.cpu().numpy(), T.p_host)


def test_warmup_takes_both_branches_of_the_min():
    r = np.float32(0.9999)
    assert [bool(cases.decay32(0.9999, True, n) < r) for n in (0, 1, 89, 10 ** 6)] == [
        True, True, True, False]
    assert cases.decay32(0.5, True, 89) == np.float32(0.5)


def test_skip_flag():
    from vdiff import ops
    T = tensors()
    for flag in (0, 17):
        sh = T.fresh_shadows()
        table, n = T.table(sh, range(2))
        ops.ema_update(table, n, (0.5, 0.999), False, None, _scalar(flag))
        for j in range(4):
            assert np.array_equal(sh[j].cpu().numpy(), T.s_host[j]), (flag, j)
    sh = T.fresh_shadows()
    table, n = T.table(sh, range(2))
    ops.ema_update(table, n, (0.5, 0.999), True, _scalar(5), _scalar(-1))
    for j, r in enumerate((0.5, 0.999)):
        _check_update(T, sh[j], T.s_host[j], cases.decay32(r, True, 5), f"flag -1 slot {j}")
        assert not np.array_equal(sh[j].cpu().numpy(), T.s_host[j])


def test_two_rates_equal_two_launches():
    from vdiff import ops
    T = tensors()
    fused, apart = T.fresh_shadows(), T.fresh_shadows()
    table, n = T.table(fused, (0, 1))
    ops.ema_update(table, n, (0.999, 0.5), True, _scalar(3), None)
    for j, r in ((0, 0.999), (1, 0.5)):
        t1, n1 = T.table(apart, (j,))
        ops.ema_update(t1, n1, (r,), True, _scalar(3), None)
    for j in range(4):
        assert torch.equal(fused[j], apart[j]), j
    assert not np.array_equal(fused[1].cpu().numpy(), T.s_host[1])


def test_argument_checks_on_tensors():
    from vdiff import ops
    T = tensors()
    sh = T.fresh_shadows()
    table, n = T.table(sh, (0,))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ema_update(table.cpu(), n, (0.5,))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ema_update(table, n, (0.5,), skip_flag=torch.tensor(-1))
    with pytest.raises(TypeError):
        ops.ema_update(table, n, (0.5,), skip_flag=torch.tensor(-1, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="vd_ema_update"):
        ops.ema_update(table, n, (0.5, 1.0))
    assert np.array_equal(sh[0].cpu().numpy(), T.s_host[0])


# ------------------------------------------------------------------ EMA over many updates
class _Params(torch.nn.Module):
    def __init__(self, sizes=(1, 7, 9, 1031), seed=5):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ps = torch.nn.ParameterList(
            [torch.nn.Parameter(torch.randn(n, generator=g)) for n in sizes])


def _move(model, g, step=1e-2):
    with torch.no_grad():
        for p in model.parameters():
            p.add_(step * torch.randn(p.shape, generator=g, device=p.device))


def _step64(e64, p, d, allowed=None):
    """fp64 update of the trajectory e64 towards p at decay d, adding the step's bound."""
    p = p.detach().double()
    new = e64 + (1.0 - float(d)) * (p - e64)
    if allowed is not None:
        allowed += cases.U * new.abs() + 4 * cases.U * (1.0 - float(d)) * (p - e64).abs()
    return new


def test_drift_over_200_updates():
    from vdiff.ema import EMA
    m = _Params().to(dev)
    rates = (0.9, 0.999)
    ema = EMA(m, rates)
    g = torch.Generator(device=dev).manual_seed(8)
    e64 = [[p.detach().double() for p in m.parameters()] for _ in rates]
    allowed = [[torch.zeros_like(e) for e in es] for es in e64]
    for _ in range(200):
        _move(m, g)
        ema.update()
        for j, r in enumerate(rates):
            d = cases.decay32(r)
            e64[j] = [_step64(e, p, d, a) for e, p, a in zip(e64[j], m.parameters(), allowed[j])]
    assert int(ema.num_updates) == 200
    worst = 0.0
    for j in range(len(rates)):
        for s, e, a in zip(ema.shadows[j], e64[j], allowed[j]):
            err = (s.double() - e).abs()
            assert bool((err <= a).all()), (j, s.numel())
            worst = max(worst, float((err / a).max()))
    print(f"200 updates: largest drift / summed bound {worst:.3f}")


def test_graph_capture_of_update():
    """EMA.update() -- the kernel and the count's increment -- captured once and replayed 20
    times with the warm-up decay on and the parameters changing between replays: the kernel
    reads the count on the device, so the replays equal 20 eager updates bit for bit."""
    from vdiff import hipgraph
    from vdiff.ema import EMA
    m = _Params(sizes=(1, 7, 9, 1031, cases.C + 1)).to(dev)
    rates = (0.9, 0.9999)
    eager, graphed = EMA(m, rates, warmup=True), EMA(m, rates, warmup=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with hipgraph.capture(g):
        graphed.update()
    g.instantiate()
    counts = hipgraph.node_counts(g)
    assert counts.get("memset", 0) == 0 and counts.get("kernel", 0) == 2, counts
    assert int(graphed.num_updates) == 0            # the capture itself updates nothing
    gen = torch.Generator(device=dev).manual_seed(13)
    for _ in range(20):
        _move(m, gen, 0.1)
        eager.update()
        g.replay()
    assert int(eager.num_updates) == 20 and int(graphed.num_updates) == 20
    for a, b in zip(eager.shadows, graphed.shadows):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(eager.shadows[1][3], m.ps[3].detach())


def test_storage_move_rebuilds_the_table():
    from vdiff.ema import EMA
    m = _Params().to(dev)
    ema = EMA(m, (0.5,))
    old = m.ps[3].detach().clone()
    with torch.no_grad():
        m.ps[3].data = old * 3.0                    # new storage
    ema.update()
    assert torch.allclose(ema.shadows[0][3], old * 2.0, rtol=1e-6)


# ------------------------------------------------------------------ Trainer
def _model(seed=4321):
    """The tiny 3-D UNetAudio of tests/test_gpu_cfg.py's train test, fp32."""
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


def _trainer(m, **kw):
    from vdiff.engine import Trainer
    from vdiff.schedulers import LinearNoiseScheduler
    return Trainer(m, LinearNoiseScheduler(100, 0.00085, 0.012), lr=1e-3, **kw)


_eager = {}


def _eager_run():
    """Three eager Trainer steps with ema_rates=(0.5, 0.9), run once: the trainer, the model,
    the parameter snapshots after each step and the shadows after the third."""
    if not _eager:
        m = _model()
        tr = _trainer(m, ema_rates=(0.5, 0.9))
        snaps = [[p.detach().clone() for p in tr.ema.params]]
        losses = []
        for s in range(3):
            losses.append(tr.step(_clip(seed=s)).clone())
            snaps.append([p.detach().clone() for p in tr.ema.params])
        tr.check_finite()
        _eager.update(m=m, tr=tr, snaps=snaps, losses=losses,
                      shadows=[[s.clone() for s in sh] for sh in tr.ema.shadows])
    return _eager


def test_trainer_eager_shadows_against_fp64():
    r = _eager_run()
    tr, snaps = r["tr"], r["snaps"]
    assert tr.ema.rates == (0.5, 0.9) and int(tr.ema.num_updates) >= 3
    assert not torch.equal(snaps[0][0], snaps[3][0])          # the weights moved
    worst = 0.0
    for j, rate in enumerate(tr.ema.rates):
        d = cases.decay32(rate)
        for i, got in enumerate(r["shadows"][j]):
            e64, allowed = snaps[0][i].double(), torch.zeros_like(snaps[0][i]).double()
            for s in range(1, 4):
                e64 = _step64(e64, snaps[s][i], d, allowed)
            err = (got.double() - e64).abs()
            assert bool((err <= allowed).all()), (rate, tr.ema.names[i])
            ok = allowed > 0
            if bool(ok.any()):
                worst = max(worst, float((err[ok] / allowed[ok]).max()))
    print(f"Trainer, 3 steps: largest error / summed bound {worst:.3f}")


def test_swapped_and_state_dict_then_training_goes_on():
    from vdiff import ops
    r = _eager_run()
    m, tr = r["m"], r["tr"]
    c = _clip(seed=9)
    before = [p.detach().clone() for p in m.parameters()]
    ptrs = [p.data_ptr() for p in m.parameters()]
    twin = _model(seed=1)
    twin.load_state_dict(tr.ema.state_dict(0.9))
    m.eval(), twin.eval()
    with torch.no_grad(), ops.frozen_weights():
        y_train = m(c.x0, c.cond, c.audio, c.t).clone()      # caches the packed operands
        with tr.ema.swapped(m, 0.9):
            for n, s in zip(tr.ema.names, tr.ema.shadows[1]):
                assert torch.equal(dict(m.named_parameters())[n], s), n
            y_ema = m(c.x0, c.cond, c.audio, c.t).clone()
        y_back = m(c.x0, c.cond, c.audio, c.t).clone()
        y_twin = twin(c.x0, c.cond, c.audio, c.t)
    assert torch.equal(y_ema, y_twin)
    assert not torch.equal(y_ema, y_train) and torch.equal(y_back, y_train)
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), before))
    assert ptrs == [p.data_ptr() for p in m.parameters()]
    # copy_to: another model takes the averages
    tr.ema.copy_to(twin, 0.5)
    own = dict(twin.named_parameters())
    assert all(torch.equal(own[n], s) for n, s in zip(tr.ema.names, tr.ema.shadows[0]))
    # the trainer goes on: the packed-operand plan still matches the parameters' storage
    n0 = int(tr.ema.num_updates)
    loss = tr.step(_clip(seed=3))
    tr.check_finite()
    assert torch.isfinite(loss) and int(tr.ema.num_updates) == n0 + 1
    assert tr.packs.plans and not tr.packs.dirty
    assert not torch.equal(before[0], next(m.parameters()).detach())


def test_trainer_graph_shadows_equal_eager(monkeypatch):
    monkeypatch.setenv("VDIFF_TRAIN_GRAPH_EXPERIMENTAL", "1")
    r = _eager_run()
    m = _model()
    tr = _trainer(m, ema_rates=(0.5, 0.9), graph=True)
    for s in range(3):
        loss = tr.step(_clip(seed=s))
        assert torch.equal(loss, r["losses"][s]), s
    assert tr.graph.g is not None and int(tr.ema.num_updates) == 3
    for a, b in zip(tr.ema.shadows, r["shadows"]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_nonfinite_step_never_reaches_the_shadows():
    from vdiff import ops
    calls = []

    def loss_fn(pred, eps):
        calls.append(1)
        loss = ops.mse_loss(pred, eps)
        return loss * float("nan") if len(calls) == 2 else loss

    m = _model()
    tr = _trainer(m, ema_rates=(0.5, 0.9), loss_fn=loss_fn, check_every=100)
    tr.step(_clip(seed=0))
    after1 = [[s.clone() for s in sh] for sh in tr.ema.shadows]
    assert not torch.equal(after1[0][0], after1[1][0])
    tr.step(_clip(seed=1))     # NaN loss: NaN gradients, NaN weights
    tr.step(_clip(seed=2))
    assert not torch.isfinite(next(m.parameters())).all()
    for sh, ref in zip(tr.ema.shadows, after1):
        for s, a in zip(sh, ref):
            assert torch.isfinite(s).all() and torch.equal(s, a)
    with pytest.raises(FloatingPointError, match="step 1 "):
        tr.check_finite()


# ------------------------------------------------------------------ DDP
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_ddp_ranks_keep_identical_shadows(tmp_path):
    out = str(tmp_path / "ema")
    port = _port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), VDIFF_DIST_BACKEND="gloo")
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "tests", "_ema_ddp_worker.py"), out], env=env,
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=240)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    a, b = (torch.load(f"{out}.rank{r}.pt", weights_only=True) for r in range(2))
    assert a["bucketed"] and b["bucketed"] and a["num_updates"] == b["num_updates"] == 2
    assert list(a["shadows"]) == list(b["shadows"]) and len(a["shadows"]) > 10
    moved = 0
    for n in a["shadows"]:
        assert torch.equal(a["shadows"][n], b["shadows"][n]), n
        assert torch.isfinite(a["shadows"][n]).all()
        moved += int(not torch.equal(a["shadows"][n], a["initial"][n]))
    assert moved > 10


# ------------------------------------------------------------------ entry points
# the reference architecture (what test.py --ckpt builds) at the smallest size of the
# existing sampling entry-point tests
SMALL = ["--dims", "3", "--frames", "2", "--image-size", "32"]


def _run(script, args, cwd):
    out = subprocess.run([sys.executable, os.path.join(DROPIN, script)] + args, cwd=cwd,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


def test_entry_points_write_and_resume_ema(tmp_path):
    ck = str(tmp_path / "m.pth")
    train = SMALL + ["--random-audio-encoder", "--batch-size", "1", "--steps-per-epoch", "2",
                     "--lr", "1e-4", "--ckpt", ck]
    out = _run("train.py", train + ["--epochs", "1", "--ema-rate", "0.9"], tmp_path)
    assert "Finished epoch 1" in out and os.path.exists(ck + ".ema_0.9")
    sd = torch.load(ck + ".ema_0.9", map_location="cpu", weights_only=True)
    last = torch.load(ck, map_location="cpu", weights_only=True)
    assert list(sd) == list(last)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    assert any(not torch.equal(sd[k], last[k]) for k in sd)
    res = torch.load(ck + ".resume", map_location="cpu", weights_only=True)
    assert res["ema"]["rates"] == [0.9] and int(res["ema"]["num_updates"]) == 2
    # the averaged weights sample
    out_dir = tmp_path / "imgs"
    _run("test.py", SMALL + ["--ckpt", ck + ".ema_0.9", "--sampler", "ddim", "--steps", "2",
                             "--save-every", "1", "--out-dir", str(out_dir)], tmp_path)
    files = sorted(p for p in os.listdir(out_dir) if p.endswith(".npy"))
    assert files and np.isfinite(np.load(out_dir / files[0])).all()
    # one more epoch from the resume file: the count goes on from 2
    out = _run("train.py", train + ["--epochs", "2", "--ema-rate", "0.9", "--resume",
                                    ck + ".resume"], tmp_path)
    assert "Finished epoch 2" in out
    res = torch.load(ck + ".resume", map_location="cpu", weights_only=True)
    assert int(res["ema"]["num_updates"]) == 4 and int(res["epoch"]) == 1


def test_train_entry_without_ema_writes_no_ema_file(tmp_path):
    ck = str(tmp_path / "m.pth")
    _run("train.py", SMALL + ["--random-audio-encoder", "--batch-size", "1", "--epochs", "1",
                              "--steps-per-epoch", "1", "--ckpt", ck], tmp_path)
    assert os.path.exists(ck) and not [f for f in os.listdir(tmp_path) if ".ema_" in f]
    res = torch.load(ck + ".resume", map_location="cpu", weights_only=True)
    assert sorted(res) == ["epoch", "model", "optimizer"]
