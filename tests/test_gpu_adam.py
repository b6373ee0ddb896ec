"""The Adam / AdamW step on the GPU: vd_adam_step against fp64 within the per-element bounds
tests/_adam_cases.py derives (three decay modes, per-tensor bias correction, every place of the
Layout an element can be lost), tensors left out of a step, the device-side skip rule and its
trip, the schedule record, graph capture of FusedAdamW.step(), state-dict interchange with
torch.optim.AdamW(fused=True), and the Trainer (eager, graph=True, DDP over gloo) and train.py
with --optimizer hip."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _adam_cases as cases
from conftest import DROPIN, ROOT, record_metric

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0) if torch.cuda.is_available() else None

INF, NAN = float("inf"), float("nan")
_case = cases.Case()                          # numpy only: built at collection, never changed
_refs = {}


def case():
    return _case


def reference(mode):
    """(P, M, V, ep, em, ev) of one step of the case in `mode`, computed once."""
    if mode not in _refs:
        c = case()
        kw = cases.MODES[mode]
        P, M, V, _ = cases.reference(c.p, c.m, c.v, c.g, c.t, **kw)
        _refs[mode] = (P, M, V) + cases.bounds(c.p, c.m, c.v, c.g, c.t, **kw)
    return _refs[mode]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _hyper(mode="adam", **kw):
    from vdiff import ops
    args = dict(lr=cases.LR, betas=cases.BETAS, eps=cases.EPS, **cases.MODES[mode])
    args.update(kw)
    return ops.adam_hyper(**args)


class _Dev:
    """The case's four buffers on the device, the count array, the state words and the record;
    step() is one vd_adam_step over the listed tensors."""

    def __init__(self):
        c = case()
        self.p, self.m, self.v, self.g = (torch.from_numpy(x.copy()).to(dev)
                                          for x in (c.p, c.m, c.v, c.g))
        for b in (self.p, self.m, self.v, self.g):
            assert b.data_ptr() % 16 == 0
        self.steps = torch.from_numpy(c.counts.copy()).to(dev)
        self.state = torch.tensor([0, 0, 0, -1], dtype=torch.int64, device=dev)
        self.lr = torch.full((1,), NAN, device=dev)
        self.flag = torch.full((1,), -7, dtype=torch.int64, device=dev)
        self._tables = {}

    def table(self, leave_out=()):
        from vdiff.optim import descriptor_rows
        key = tuple(sorted(leave_out))
        if key not in self._tables:
            L = case().L
            idx = [i for i in range(len(L.numels)) if i not in key]
            ptr = lambda b: [b.data_ptr() + 4 * L.offsets[i] for i in idx]   # noqa: E731
            rows = descriptor_rows(ptr(self.p), ptr(self.m), ptr(self.v), ptr(self.g),
                                   [L.numels[i] for i in idx], idx)
            self._tables[key] = (torch.from_numpy(rows.view(np.uint8).copy()).to(dev), len(rows))
        return self._tables[key]

    def step(self, hyper, loss=None, norm=None, leave_out=()):
        from vdiff import ops
        table, n = self.table(leave_out)
        loss, norm = (None if x is None else torch.tensor(x, dtype=torch.float32, device=dev)
                      for x in (loss, norm))
        ops.adam_step(table, n, hyper, self.steps, self.state, self.lr[0], self.flag[0],
                      loss=loss, grad_norm=norm)

    def host(self):
        return tuple(b.cpu().numpy() for b in (self.p, self.m, self.v, self.g))

    def words(self):
        return self.state.tolist(), int(self.flag[0])


# ------------------------------------------------------------------ 1. one step against fp64
@pytest.mark.parametrize("mode", list(cases.MODES))
def test_one_step_against_fp64(mode):
    c = case()
    P, M, V, ep, em, ev = reference(mode)
    D = _Dev()
    assert D.table()[1] == len(c.L.ranges) > cases.cc.N_ONES
    D.step(_hyper(mode))
    p, m, v, g = D.host()
    ratios = {}
    for name, got, want, b in (("p", p, P, ep), ("m", m, M, em), ("v", v, V, ev)):
        ratios[name] = cases.worst_ratio(got, want, b, c.mask)
    print(f"{mode}: largest error / bound {ratios}")
    record_metric(test="adam_step_vs_fp64", mode=mode,
                  **{f"ratio_{k}": r for k, r in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    for got, before in ((p, c.p), (m, c.m), (v, c.v)):
        assert np.array_equal(_bits(got[~c.mask]), _bits(before[~c.mask]))   # the guard bands
        assert not np.array_equal(got[c.mask], before[c.mask])
    assert np.array_equal(_bits(g), _bits(c.g))
    assert np.array_equal(D.steps.cpu().numpy(), c.counts + 1)
    assert D.words() == ([1, 0, 0, -1], -1)
    assert float(D.lr[0]) == float(np.float32(cases.LR))


def test_a_range_with_one_pointer_off_alignment():
    """p, m, v 16-B aligned and g one element off: the whole range goes one element at a time."""
    from vdiff import ops
    from vdiff.optim import descriptor_rows
    rng = np.random.default_rng(5)
    n = 37
    host = {k: np.full(n + 16, cases.SENTINEL, np.float32) for k in "pmvg"}
    at = {"p": 8, "m": 8, "v": 8, "g": 9}
    vals = {"p": rng.standard_normal(n), "m": rng.standard_normal(n),
            "v": rng.uniform(0.5, 2.0, n), "g": rng.standard_normal(n) + 2.0}
    for k in "pmvg":
        host[k][at[k]:at[k] + n] = vals[k].astype(np.float32)
    bufs = {k: torch.from_numpy(host[k].copy()).to(dev) for k in "pmvg"}
    rows = descriptor_rows(*([bufs[k].data_ptr() + 4 * at[k]] for k in "pmvg"), [n], [0])
    assert int(rows["p"][0]) % 16 == 0 and int(rows["g"][0]) % 16 == 4
    table = torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
    steps = torch.tensor([4], dtype=torch.int64, device=dev)
    state = torch.tensor([0, 0, 0, -1], dtype=torch.int64, device=dev)
    lr, flag = torch.zeros(1, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    ops.adam_step(table, 1, _hyper("l2"), steps, state, lr[0], flag[0])
    ins = [host[k][at[k]:at[k] + n] for k in "pmvg"]
    t = np.full(n, 5.0)
    P, M, V, _ = cases.reference(*ins, t, **cases.MODES["l2"])
    ep, em, ev = cases.bounds(*ins, t, **cases.MODES["l2"])
    every = np.ones(n, bool)
    for k, want, b in (("p", P, ep), ("m", M, em), ("v", V, ev)):
        got = bufs[k].cpu().numpy()
        assert cases.worst_ratio(got[at[k]:at[k] + n], want, b, every) <= 1.0, k
        guard = np.ones(n + 16, bool)
        guard[at[k]:at[k] + n] = False
        assert (got[guard] == cases.SENTINEL).all(), k
    assert np.array_equal(_bits(bufs["g"].cpu().numpy()), _bits(host["g"]))
    assert int(steps[0]) == 5


# ------------------------------------------------------------------ 2. tensors left out
def test_a_tensor_left_out_keeps_every_bit():
    c = case()
    L = c.L
    out = (3, 5, len(cases.cc.SIZES) + 1, L.first_one, L.first_one + 1500, len(L.numels) - 1)
    D = _Dev()
    D.step(_hyper("decoupled"), leave_out=out)
    listed = c.listed(out)
    left = c.mask & ~listed
    assert left.sum() > cases.C and listed.sum() > cases.C
    P, M, V, ep, em, ev = reference("decoupled")
    p, m, v, g = D.host()
    for got, before in ((p, c.p), (m, c.m), (v, c.v)):
        assert np.array_equal(_bits(got[~listed]), _bits(before[~listed]))
    for got, want, b in ((p, P, ep), (m, M, em), (v, V, ev)):
        assert cases.worst_ratio(got, want, b, listed) <= 1.0
    want = c.counts + 1
    want[list(out)] = c.counts[list(out)]
    assert np.array_equal(D.steps.cpu().numpy(), want)          # listed: exactly + 1


# ------------------------------------------------------------------ 3. skip
BAD = {"loss nan": dict(loss=NAN, norm=2.0), "loss +inf": dict(loss=INF, norm=2.0),
       "norm nan": dict(loss=1.0, norm=NAN)}
GOOD = dict(loss=1.0, norm=2.0)


@pytest.mark.parametrize("trigger", list(BAD))
def test_skip_rule(trigger):
    bad = BAD[trigger]
    h = _hyper("decoupled", max_bad_run=1)
    D = _Dev()
    snap = lambda: tuple(_bits(x).copy() for x in D.host()) + (D.steps.cpu().numpy(),)  # noqa: E731
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))   # noqa: E731
    s0 = snap()
    D.step(h, **GOOD)
    s1 = snap()
    assert not same(s0, s1) and D.words() == ([1, 0, 0, -1], -1)
    D.step(h, **bad)                               # skipped: nothing moves
    assert same(snap(), s1) and D.words() == ([1, 1, 1, -1], 1)
    D.step(h, **GOOD)                              # a good step resets the run
    s2 = snap()
    assert not same(s1, s2) and D.words() == ([2, 1, 0, -1], -1)
    assert np.array_equal(s2[-1], case().counts + 2)
    D.step(h, **bad)
    assert D.words() == ([2, 2, 1, -1], 3)         # K bad steps in a row: not tripped
    D.step(h, **bad)
    assert D.words() == ([2, 3, 2, 4], 4)          # K + 1: tripped at this step's index
    assert same(snap(), s2)
    D.step(h, **GOOD)                              # sticky: a later good step is skipped too
    assert same(snap(), s2) and D.words() == ([2, 4, 3, 4], 5)
    D.step(h)                                      # (and one with nothing to test)
    assert same(snap(), s2) and D.words() == ([2, 5, 4, 4], 6)


def test_max_bad_run_0_never_skips():
    c = case()
    D = _Dev()
    D.step(_hyper("adam", max_bad_run=0), loss=NAN, norm=NAN)   # today's behaviour
    P, M, V, ep, em, ev = reference("adam")
    p, m, v, _ = D.host()
    assert cases.worst_ratio(p, P, ep, c.mask) <= 1.0
    assert D.words() == ([1, 0, 0, -1], -1)
    assert np.array_equal(D.steps.cpu().numpy(), c.counts + 1)


# ------------------------------------------------------------------ 4. schedule
def test_schedule_record():
    from vdiff.optim import FusedAdamW, lr_at
    W, T, r, lr = 4, 10, 0.1, 1e-2
    torch.manual_seed(3)
    p = torch.nn.Parameter(torch.randn(9, device=dev))
    opt = FusedAdamW([p], lr, warmup_steps=W, schedule="cosine", total_steps=T, min_ratio=r,
                     max_bad_run=1)
    one, nan = torch.ones((), device=dev), torch.full((), NAN, device=dev)
    g = torch.Generator(device=dev).manual_seed(4)
    applied, two = 0, (1 + cases.U) ** 2 - 1
    for k in range(13):
        p.grad = torch.randn(9, generator=g, device=dev) + 3.0
        before = p.detach().clone()
        skip = k == 6
        opt.step(loss=nan if skip else one)
        want = lr_at(applied, lr, W, "cosine", T, r)
        got = float(opt.lr)
        assert abs(got - want) <= two * want, (k, got, want)
        assert int(opt.skip_flag) == (k if skip else -1)
        if skip:
            assert torch.equal(p.detach(), before)               # and the position stays
        else:
            applied += 1
            if applied == 1:                                     # a first step moves by lr_s
                assert torch.allclose((p.detach() - before).abs(),
                                      torch.full_like(before, want), rtol=1e-4)
        assert int(opt.applied) == applied and int(opt.skipped) == int(k >= 6)
    assert applied == 12 and opt.rebuilds >= 1
    assert float(opt.lr) == pytest.approx(lr * r, rel=1e-6)      # beyond T: the floor
    assert int(opt.state[p]["step"]) == 12


# ------------------------------------------------------------------ 5. graph
def _param_set(seed_shift=0.0):
    """Parameters and static gradients that are views of two flat buffers laid out as the case."""
    c = case()
    L = c.L
    pbuf = torch.from_numpy(c.p.copy()).to(dev)
    gbuf = torch.from_numpy(c.g.copy()).to(dev)
    params = []
    for o, n in zip(L.offsets, L.numels):
        q = torch.nn.Parameter(pbuf[o:o + n])
        q.grad = gbuf[o:o + n]
        params.append(q)
    return pbuf, gbuf, params


def _opt_state(opt, params):
    m = torch.cat([opt.state[q]["exp_avg"] for q in params])
    v = torch.cat([opt.state[q]["exp_avg_sq"] for q in params])
    return m, v, opt._steps.clone(), opt.lr.clone(), opt._words.clone()


def test_graph_capture_of_step():
    from vdiff import hipgraph
    from vdiff.optim import KERNEL_LAUNCHES, FusedAdamW
    kw = dict(lr=1e-2, weight_decay=0.1, warmup_steps=3, schedule="linear", total_steps=6,
              min_ratio=0.2, max_bad_run=1)
    ebuf, egrad, eparams = _param_set()
    gbuf, ggrad, gparams = _param_set()
    eager, graphed = FusedAdamW(eparams, **kw), FusedAdamW(gparams, **kw)
    eloss, gloss = torch.ones((), device=dev), torch.ones((), device=dev)
    eager.step(loss=eloss)
    graphed.step(loss=gloss)                       # builds the table, creates the state
    assert graphed.rebuilds == 1 and graphed.n_desc == len(case().L.ranges)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with hipgraph.capture(g):
        graphed.step(loss=gloss)
    g.instantiate()
    counts = hipgraph.node_counts(g)
    assert counts.get("memset", 0) == 0 and counts.get("kernel", 0) == KERNEL_LAUNCHES == 2, counts
    assert set(counts) == {"kernel"}, counts
    assert graphed.rebuilds == 1
    assert torch.equal(ebuf.view(torch.int32), gbuf.view(torch.int32))   # capture ran nothing
    gen = torch.Generator(device=dev).manual_seed(11)
    src = egrad.clone()
    guard = ~torch.from_numpy(case().mask).to(dev)
    for k in range(5):
        fresh = src * (0.5 + torch.rand(src.shape, generator=gen, device=dev))
        bad = k == 2
        for grad, loss in ((egrad, eloss), (ggrad, gloss)):
            grad.copy_(fresh)
            loss.fill_(NAN if bad else 1.0)
        before = gbuf.clone()
        eager.step(loss=eloss)
        g.replay()
        assert torch.equal(ebuf.view(torch.int32), gbuf.view(torch.int32)), k
        assert torch.equal(gbuf[guard].view(torch.int32), before[guard].view(torch.int32))
        assert torch.equal(gbuf, before) == bad, k                # a skipped replay holds still
        for a, b in zip(_opt_state(eager, eparams), _opt_state(graphed, gparams)):
            assert torch.equal(a, b), k
    assert int(graphed.applied) == 5 and int(graphed.skipped) == 1
    assert eager.rebuilds == 1 and graphed.rebuilds == 1
    assert int(graphed.state[gparams[0]]["step"]) == 5


def test_a_changed_list_under_capture_is_refused(monkeypatch):
    """Not uploaded: an upload has no place in a captured step.  (The capture is pretended, so
    that no half-made graph is left behind.)"""
    from vdiff.optim import FusedAdamW
    ps = [torch.nn.Parameter(torch.ones(9, device=dev)) for _ in range(2)]
    ps[0].grad = torch.ones(9, device=dev)
    opt = FusedAdamW(ps, 1e-3)
    opt.step()
    before = [p.detach().clone() for p in ps]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    ps[0].grad = torch.ones(9, device=dev)                        # another address
    with pytest.raises(RuntimeError, match="pointers changed under graph capture"):
        opt.step()
    ps[1].grad = torch.ones(9, device=dev)                        # a parameter without state
    with pytest.raises(RuntimeError, match="parameter list changed under graph capture"):
        opt.step()
    monkeypatch.undo()
    assert opt.rebuilds == 1 and int(opt.applied) == 1
    assert all(torch.equal(p.detach(), b) for p, b in zip(ps, before))


# ------------------------------------------------------------------ 6. interchange on the device
def test_state_dict_interchange_with_torch_on_the_device():
    from vdiff.optim import FusedAdamW
    c = case()
    kw = dict(lr=cases.LR, weight_decay=0.1)
    pbuf, gbuf, params = _param_set()
    opt = FusedAdamW(params, **kw)
    for _ in range(2):
        opt.step()
    sd = opt.state_dict()
    tparams = [torch.nn.Parameter(q.detach().clone()) for q in params]
    topt = torch.optim.AdamW(tparams, lr=1.0, fused=True)
    topt.load_state_dict(sd)
    st = topt.state[tparams[4]]
    assert st["step"].dtype == torch.float32 and st["step"].is_cuda and float(st["step"]) == 2.0
    assert topt.param_groups[0]["lr"] == cases.LR and topt.param_groups[0]["weight_decay"] == 0.1
    pbuf2, gbuf2, params2 = _param_set()
    pbuf2.copy_(pbuf)
    back = FusedAdamW(params2, lr=5.0)
    tsd = topt.state_dict()
    native = set(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).param_groups[0])
    tsd["param_groups"] = [{k: v for k, v in grp.items() if k in native}
                           for grp in tsd["param_groups"]]       # what torch alone would write
    assert "fused_state" not in tsd["param_groups"][0] and "decoupled" not in tsd["param_groups"][0]
    back.load_state_dict(tsd)
    assert back.param_groups[0]["lr"] == cases.LR and back.param_groups[0]["decoupled"] is True
    for q, q2 in zip(params, params2):
        a, b = opt.state[q], back.state[q2]
        assert torch.equal(a["exp_avg"], b["exp_avg"])
        assert torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
        assert a["exp_avg"].data_ptr() != b["exp_avg"].data_ptr()
    assert torch.equal(opt._steps, back._steps) and int(back._steps.min()) == 2
    assert [int(x) for x in (back.applied, back.skipped, back.bad_run, back.tripped_at)] == \
        [2, 0, 0, -1]
    # a further step from the loaded state still meets the fp64 bound
    flat = lambda key: np.concatenate([back.state[q][key].cpu().numpy().ravel()   # noqa: E731
                                       for q in params2])
    p0, g0 = pbuf2.cpu().numpy()[c.mask], gbuf2.cpu().numpy()[c.mask]
    m0, v0 = flat("exp_avg"), flat("exp_avg_sq")
    t = np.full(p0.shape, 3.0)
    mode = dict(weight_decay=0.1, decoupled=True)
    P, M, V, _ = cases.reference(p0, m0, v0, g0, t, **mode)
    ep, em, ev = cases.bounds(p0, m0, v0, g0, t, **mode)
    back.step()
    every = np.ones(p0.shape, bool)
    ratios = [cases.worst_ratio(pbuf2.cpu().numpy()[c.mask], P, ep, every),
              cases.worst_ratio(flat("exp_avg"), M, em, every),
              cases.worst_ratio(flat("exp_avg_sq"), V, ev, every)]
    print(f"third step after the round trip: error / bound {ratios}")
    assert max(ratios) <= 1.0, ratios


# ------------------------------------------------------------------ 7. Trainer
def _tiny():
    import test_gpu_clip as t
    return t._model, t._clip, t._sched


class _Poison:
    """loss_fn: the MSE times a device scalar the test sets before each step (1 or NaN) -- the
    same launches every call, so the graph=True trainer can capture it."""

    def __init__(self):
        self.factor = torch.ones((), device=dev)

    def __call__(self, pred, eps):
        from vdiff import ops
        return ops.mse_loss(pred, eps) * self.factor


def _run_trainer(pattern, graph=False, **extra):
    """One trainer over `pattern` (True: this call's loss is NaN): per step the weights, the
    EMA shadows, lr, skipped count; then the trainer."""
    from vdiff.engine import Trainer
    model, clip, sched = _tiny()
    m = model()
    poison = _Poison()
    kw = dict(optimizer="hip", lr_warmup=2, skip_bad_steps=1, ema_rates=(0.9,),
              clip_grad_norm=INF, loss_fn=poison, check_every=100, graph=graph)
    kw.update(extra)
    tr = Trainer(m, sched(), lr=1e-3, **kw)
    out = []
    for s, bad in enumerate(pattern):
        poison.factor.fill_(NAN if bad else 1.0)
        loss = tr.step(clip(seed=s))
        assert bool(torch.isfinite(loss)) != bad
        out.append(dict(w=[p.detach().clone() for p in m.parameters()],
                        e=[x.clone() for x in tr.ema.shadows[0]],
                        lr=float(tr.lr), skipped=int(tr.skipped_steps)))
    return out, tr


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_trainer_skips_one_bad_step():
    out, tr = _run_trainer([False, True, False])
    assert _same(out[0]["w"], out[1]["w"]) and _same(out[0]["e"], out[1]["e"])   # bit for bit
    assert not _same(out[1]["w"], out[2]["w"]) and not _same(out[1]["e"], out[2]["e"])
    assert all(torch.isfinite(x).all() for x in out[2]["w"] + out[2]["e"])
    assert [o["skipped"] for o in out] == [0, 1, 1]
    # the warm-up counts applied steps: 1/2, then 2/2 twice (the skipped step holds its place)
    assert [o["lr"] for o in out] == [float(np.float32(x)) for x in (5e-4, 1e-3, 1e-3)]
    assert tr._first_bad is None                     # the sticky record is not written
    tr.check_finite()
    assert int(tr.ema.num_updates) == 3
    # step 1 moved both as well
    model = _tiny()[0]
    fresh = [p.detach().clone() for p in model().parameters()]
    assert not _same(fresh, out[0]["w"]) and not _same(fresh, out[0]["e"])


def test_trainer_trips_after_two_bad_steps():
    out, tr = _run_trainer([False, True, True, False])
    for s in (1, 2, 3):                              # the weights of the last good step
        assert _same(out[0]["w"], out[s]["w"]) and _same(out[0]["e"], out[s]["e"])
    assert [o["skipped"] for o in out] == [0, 1, 2, 3]
    with pytest.raises(FloatingPointError, match=r"tripped at step 2 \(of 4\), 3 steps skipped"):
        tr.check_finite()


def test_trainer_graph_equals_eager(monkeypatch):
    monkeypatch.setenv("VDIFF_TRAIN_GRAPH_EXPERIMENTAL", "1")
    pattern = [False, False, False, True, False]
    eager, _ = _run_trainer(pattern)
    got, tr = _run_trainer(pattern, graph=True)
    assert tr.graph.g is not None
    for s, (a, b) in enumerate(zip(got, eager)):
        assert _same(a["w"], b["w"]) and _same(a["e"], b["e"]), s
        assert (a["lr"], a["skipped"]) == (b["lr"], b["skipped"]), s
    assert _same(got[2]["w"], got[3]["w"]) and not _same(got[3]["w"], got[4]["w"])
    assert [o["skipped"] for o in got] == [0, 0, 0, 1, 1]
    tr.check_finite()


def test_trainer_without_skipping_keeps_the_record():
    """optimizer='hip' with skip_bad_steps=0: the fail-fast record of the torch path."""
    out, tr = _run_trainer([False, True], skip_bad_steps=0)
    assert out[1]["skipped"] == 0
    assert not all(torch.isfinite(x).all() for x in out[1]["w"])   # the step is not prevented
    assert _same(out[0]["e"], out[1]["e"])                         # the EMA guard holds
    with pytest.raises(FloatingPointError, match="step 1 "):
        tr.check_finite()


# ------------------------------------------------------------------ 8. DDP
def test_ddp_ranks_skip_together(tmp_path):
    from test_gpu_clip import _port
    out = str(tmp_path / "adam")
    port = _port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), VDIFF_DIST_BACKEND="gloo")
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "tests", "_adam_ddp_worker.py"), out], env=env,
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=240)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    a, b = (torch.load(f"{out}.rank{r}.pt", weights_only=True) for r in range(2))
    for d in (a, b):
        assert d["bucketed"] and d["missing_clipper_error"]
    assert a["finite_loss"] == [True, True, True] and b["finite_loss"] == [True, False, True]
    for d in (a, b):
        assert d["skipped"] == [0, 1, 1] and d["flags"] == [-1, 1, -1] and d["tripped_at"] == -1
        assert len(d["params"]) == 3 and len(d["params"][0]) > 10
        moved01 = moved12 = moved23 = 0
        for n in d["params"][0]:
            moved01 += int(not torch.equal(d["initial"][n], d["params"][0][n]))
            moved12 += int(not torch.equal(d["params"][0][n], d["params"][1][n]))
            moved23 += int(not torch.equal(d["params"][1][n], d["params"][2][n]))
            assert torch.isfinite(d["params"][2][n]).all(), n
        assert moved01 > 10 and moved12 == 0 and moved23 > 10
    for s in range(3):
        for n in a["params"][s]:
            assert torch.equal(a["params"][s][n], b["params"][s][n]), (s, n)   # bit-identical
    assert a["lr"] == b["lr"] and a["lr"][0] < a["lr"][1] == a["lr"][2]


# ------------------------------------------------------------------ 9. train.py
SMALL = ["--dims", "3", "--frames", "2", "--image-size", "32", "--random-audio-encoder",
         "--batch-size", "1", "--steps-per-epoch", "2", "--lr", "1e-4"]
HIP = ["--optimizer", "hip", "--lr-warmup", "2", "--lr-schedule", "cosine", "--weight-decay",
       "0.01", "--skip-bad-steps", "2"]


def _train(args, cwd):
    out = subprocess.run([sys.executable, os.path.join(DROPIN, "train.py")] + args, cwd=cwd,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


def _epoch_line(out, epoch):
    return [ln for ln in out.splitlines() if ln.startswith(f"Finished epoch {epoch} ")][0]


def test_train_entry_with_the_hip_optimizer(tmp_path):
    from vdiff.optim import lr_at
    ck = str(tmp_path / "m.pth")
    out = _train(SMALL + HIP + ["--epochs", "2", "--ckpt", ck], tmp_path)
    rates = []
    for epoch in (1, 2):
        m = re.search(r"\| lr (\S+) \| skipped (\d+) steps \|", _epoch_line(out, epoch))
        assert m, _epoch_line(out, epoch)
        rates.append(float(m.group(1)))
        assert int(m.group(2)) == 0
    # the epoch's last step: s = 1 and s = 3 of W = 2, T = 4 (printed with 4 digits)
    for got, s in zip(rates, (1, 3)):
        assert got == pytest.approx(lr_at(s, 1e-4, 2, "cosine", 4, 0.0), rel=2e-3), (got, s)
    res = torch.load(ck + ".resume", map_location="cpu", weights_only=True)
    assert sorted(res) == ["epoch", "model", "optimizer"]
    group = res["optimizer"]["param_groups"][0]
    assert group["fused_state"] == [4, 0, 0, -1] and group["schedule"] == "cosine"
    steps = {float(s["step"]) for s in res["optimizer"]["state"].values()}
    assert steps and max(steps) == 4.0
    # the checkpoint resumes under the same optimizer ...
    ck2 = str(tmp_path / "n.pth")
    out = _train(SMALL + HIP + ["--epochs", "3", "--ckpt", ck2, "--resume", ck + ".resume"],
                 tmp_path)
    assert "Finished epoch 3" in out and "Finished epoch 2" not in out
    res2 = torch.load(ck2 + ".resume", map_location="cpu", weights_only=True)
    assert res2["optimizer"]["param_groups"][0]["fused_state"] == [6, 0, 0, -1]
    # ... and under torch's
    ck3 = str(tmp_path / "t.pth")
    out = _train(SMALL + ["--epochs", "3", "--ckpt", ck3, "--resume", ck + ".resume"], tmp_path)
    line = _epoch_line(out, 3)
    assert " lr " not in line and "skipped" not in line
    res3 = torch.load(ck3 + ".resume", map_location="cpu", weights_only=True)
    assert max(float(s["step"]) for s in res3["optimizer"]["state"].values()) == 6.0
    assert math.isfinite(sum(float(v.float().sum()) for v in res3["model"].values()))
