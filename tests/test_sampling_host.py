"""The sampling driver's contract, host side (CPU, no GPU): sample_ddim / sample_dpm / sample_long
run here on torch restatements of the samplers' step kernels and of the window gather / blend,
around a recording toy model.  Each case is compared, bit for bit, with a straight-line loop
written out below that calls the samplers' step() itself and never the driver: the trajectory the
callback sees, the return value, what the model was called with, the one draw from the generator.
The graph classes are constructed on the CPU (construction launches nothing) to show that they
die by reference count alone."""
import functools
import gc
import weakref

import pytest
import torch

from vdiff import engine, ops
from vdiff.schedulers import DDIMSampler, DPMSolverSampler, LinearNoiseSchedulerV2, WindowPlan

B, C, T, HW, F = 2, 3, 4, 8, 5          # clips, channels, the denoiser's frames, size, features
L, STRIDE = 8, 2                        # the long clip: 3 windows of 4 frames
STEPS, SEED = 4, 21
GUIDE = {"plain": (1.0, 0.0), "guided": (3.0, 0.7)}


# ------------------------------------------------------------------ torch restatements
def _guide(eps_c, eps_u, scale, rescale):
    eps = eps_u + scale * (eps_c - eps_u)
    if rescale > 0:
        dims = tuple(range(1, eps.dim()))
        eps = eps * (rescale * eps_c.std(dims, keepdim=True) / eps.std(dims, keepdim=True)
                     + (1 - rescale))
    return eps


class TorchDDIM(DDIMSampler):
    """DDIMSampler (eta = 0, eps-prediction) with the step kernels restated in torch."""

    def step(self, xt, noise_pred, i, z=None):
        a = self.acp[int(self.timesteps[i])]
        tp = int(self.prev_timesteps[i])
        ap = self.acp[tp] if tp >= 0 else torch.tensor(1.0)
        x0 = (xt - (1 - a).sqrt() * noise_pred) / a.sqrt()
        return ap.sqrt() * x0 + (1 - ap).sqrt() * noise_pred, x0

    def step_guided(self, xt, eps_c, eps_u, i, scale, rescale=0.0, z=None):
        return self.step(xt, _guide(eps_c, eps_u, scale, rescale), i)


class TorchDPM(DPMSolverSampler):
    """DPMSolverSampler with the step kernels restated in torch on its own coefficient table;
    like them it writes this step's x0 over x0_last and returns that buffer."""

    def step(self, xt, noise_pred, i, x0_last=None):
        c0, c1, A, Bc, Cc = (float(v) for v in self.coef[int(i), :5])
        assert x0_last is not None or Cc == 0.0
        hist = torch.empty_like(xt) if x0_last is None else x0_last
        x0 = (xt - c1 * noise_pred) / c0
        xp = A * xt + Bc * x0
        if Cc != 0.0:
            xp = xp + Cc * hist
        hist.copy_(x0)
        return xp, hist

    def step_guided(self, xt, eps_c, eps_u, i, scale, rescale=0.0, x0_last=None):
        return self.step(xt, _guide(eps_c, eps_u, scale, rescale), i, x0_last=x0_last)


def _sampler(kind):
    sch = LinearNoiseSchedulerV2(500, 0.00005, 0.015)
    s = TorchDDIM(sch, steps=STEPS) if kind == "ddim" else TorchDPM(sch, steps=STEPS)
    assert s.steps == STEPS
    return s


class Toy:
    """(x, cond, feats, t) -> 0.1 x + mean(feats), recording the order of eval() and
    encode_audio() and every call's arguments."""

    def __init__(self, events=None):
        self.events = [] if events is None else events
        self.calls = []

    def eval(self):
        self.events.append("eval")
        return self

    def encode_audio(self, audio):
        self.events.append("encode")
        return audio["features"]

    def __call__(self, x, cond, feats, t):
        self.calls.append((x.clone(), cond.clone(), feats.clone(), t.clone()))
        return 0.1 * x + feats.mean()


def _gather(x, plan, out=None, dup=None):
    """ops.window_gather restated: row b * W + w holds frames starts[w] .. starts[w] + T - 1."""
    W, Tw = plan.num_windows, plan.window
    win = x.index_select(2, plan.frame_index).view(x.shape[0], x.shape[1], W, Tw, *x.shape[3:])
    win = win.transpose(1, 2).reshape(x.shape[0] * W, x.shape[1], Tw, *x.shape[3:])
    for buf in (out, dup):
        if buf is not None:
            buf.copy_(win)
    return win if out is None else out


def _blend(win, plan, out=None):
    """ops.window_blend restated: the covering windows of a frame, summed in ascending order
    with the plan's weights."""
    assert out is None
    W = plan.num_windows
    v = win.view(win.shape[0] // W, W, *win.shape[1:])
    res = torch.zeros((v.shape[0], win.shape[1], plan.length) + tuple(win.shape[3:]),
                      dtype=win.dtype)
    for l in range(plan.length):
        for k in range(plan.KMAX):
            w = int(plan.cover_win[l, k])
            if w >= 0:
                res[:, :, l] += plan.cover_wgt[l, k] * v[:, w, :, l - int(plan.starts[w])]
    return res


@pytest.fixture
def window_ops(monkeypatch):
    monkeypatch.setattr(ops, "window_gather", _gather)
    monkeypatch.setattr(ops, "window_blend", _blend)


@functools.lru_cache(maxsize=None)
def _inputs(frames):
    """(cond, features, shape) of a clip of `frames` frames: built once, never written to."""
    g = torch.Generator().manual_seed(3)
    cond = torch.rand((B, C, HW, HW), generator=g) * 2 - 1
    feats = torch.randn((B * frames, F), generator=g)
    return cond, feats, (B, C, frames, HW, HW)


# ------------------------------------------------------------------ the straight-line loops
def _reference(kind, guide, frames):
    """(trajectory [(i, xt, x0)], rows of the model's batch) of `kind` sampling from seed SEED:
    the loop written out, short (frames == T) or through the windows (frames == L)."""
    scale, rescale = GUIDE[guide]
    guided = scale != 1.0
    sampler, model = _sampler(kind), Toy()
    cond, feats, shape = _inputs(frames)
    xt = torch.randn(shape, generator=torch.Generator().manual_seed(SEED))
    plan = None
    if frames != T:
        plan = WindowPlan(frames, T, STRIDE)
        W = plan.num_windows
        route = (torch.arange(B).view(B, 1) * frames + plan.frame_index.view(1, -1)).reshape(-1)
        cond, feats = cond.repeat_interleave(W, dim=0), feats.index_select(0, route)
    if guided:
        cond, feats = torch.cat([cond, cond]), torch.cat([feats, torch.zeros_like(feats)])
    rows = cond.shape[0]
    traj, x0 = [], None
    for i in range(sampler.steps):
        t = torch.full((rows,), int(sampler.timesteps[i]), dtype=torch.int64)
        x_in = xt if plan is None else _gather(xt, plan)
        out = model(torch.cat([x_in, x_in]) if guided else x_in, cond, feats, t)
        if plan is not None:
            out = _blend(out, plan)
        kw = {"x0_last": x0} if kind == "dpm++" else {}
        if guided:
            eps_c, eps_u = out.chunk(2)
            xt, x0 = sampler.step_guided(xt, eps_c, eps_u, i, scale, rescale, **kw)
        else:
            xt, x0 = sampler.step(xt, out, i, **kw)
        traj.append((i, xt.clone(), x0.clone()))
    return traj, rows


def _drive(kind, guide, frames, model=None, generator=None, callback=None, **kw):
    scale, rescale = GUIDE[guide]
    cond, feats, shape = _inputs(frames)
    model = Toy() if model is None else model
    g = torch.Generator().manual_seed(SEED) if generator is None else generator
    args = (model, _sampler(kind), cond, {"features": feats}, shape)
    opts = dict(generator=g, callback=callback, guidance_scale=scale, guidance_rescale=rescale)
    if frames != T or kw:
        return engine.sample_long(*args, window=T, stride=STRIDE, **kw, **opts)
    return (engine.sample_ddim if kind == "ddim" else engine.sample_dpm)(*args, **opts)


CASES = [(k, g, f) for k in ("ddim", "dpm++") for g in GUIDE for f in (T, L)]


# ------------------------------------------------------------------ 1. trajectory
@pytest.mark.parametrize("kind,guide,frames", CASES)
def test_trajectory_equals_the_straight_line_loop(window_ops, kind, guide, frames):
    want, _ = _reference(kind, guide, frames)
    got = []
    xt, x0 = _drive(kind, guide, frames,
                    callback=lambda i, a, b: got.append((i, a.clone(), b.clone())))
    assert [i for i, _, _ in got] == list(range(STEPS))
    for (i, a, b), (_, wa, wb) in zip(got, want):
        assert torch.equal(a, wa) and torch.equal(b, wb), (kind, guide, frames, i)
    assert torch.equal(xt, want[-1][1]) and torch.equal(x0, want[-1][2])
    assert xt.shape == x0.shape == (B, C, frames, HW, HW)


# ------------------------------------------------------------------ 2. what the model saw
@pytest.mark.parametrize("kind,guide,frames", CASES)
def test_what_the_model_saw(window_ops, kind, guide, frames):
    _, rows = _reference(kind, guide, frames)
    guided = GUIDE[guide][0] != 1.0
    W = 1 if frames == T else WindowPlan(frames, T, STRIDE).num_windows
    assert rows == (2 if guided else 1) * B * W
    model = Toy()
    _drive(kind, guide, frames, model=model)
    ts = _sampler(kind).timesteps
    assert len(model.calls) == STEPS
    for i, (x, cond, feats, t) in enumerate(model.calls):
        assert x.shape == (rows, C, T, HW, HW) and cond.shape[0] == rows
        assert feats.shape == (rows * T, F)
        assert t.dtype == torch.int64 and t.shape == (rows,) and (t == int(ts[i])).all()
        if guided:
            h = rows // 2
            assert torch.equal(x[:h], x[h:]) and torch.equal(cond[:h], cond[h:])
            assert (feats[h * T:] == 0).all() and (feats[:h * T] != 0).any()


def test_window_batch_chunks_the_window_rows(window_ops):
    model = Toy()
    _drive("ddim", "guided", L, model=model, window_batch=5)
    rows = 2 * B * WindowPlan(L, T, STRIDE).num_windows  # 12: chunks of 5, 5, 2
    assert [c[0].shape[0] for c in model.calls] == [5, 5, 2] * STEPS
    for x, cond, feats, t in model.calls:
        n = x.shape[0]
        assert cond.shape[0] == n and feats.shape[0] == n * T and t.shape == (n,)
    assert sum(c[0].shape[0] for c in model.calls[:3]) == rows


# ------------------------------------------------------------------ 3. order of work, one draw
@pytest.mark.parametrize("kind,frames", [("ddim", T), ("dpm++", T), ("ddim", L), ("dpm++", L)])
def test_eval_then_encode_then_one_draw(window_ops, monkeypatch, kind, frames):
    events = []
    randn = torch.randn

    def recording_randn(*a, **kw):
        events.append(("randn", tuple(a[0])))
        return randn(*a, **kw)

    _inputs(frames)  # (the test's own inputs: drawn before the recording starts)
    g = torch.Generator().manual_seed(SEED)
    with monkeypatch.context() as m:
        m.setattr(torch, "randn", recording_randn)
        _drive(kind, "guided", frames, model=Toy(events), generator=g)
    shape = (B, C, frames, HW, HW)
    assert events == ["eval", "encode", ("randn", shape)]
    fresh = torch.Generator().manual_seed(SEED)
    torch.randn(shape, generator=fresh)
    assert torch.equal(g.get_state(), fresh.get_state())


# ------------------------------------------------------------------ 4. callback references
@pytest.mark.parametrize("kind,guide,frames", CASES)
def test_callback_may_keep_references(window_ops, kind, guide, frames):
    """A callback that keeps what it is given, without cloning, still holds every step's own
    values at the end: 2M's in-place x0 history does not leak out."""
    want, _ = _reference(kind, guide, frames)
    kept = []
    _drive(kind, guide, frames, callback=lambda i, a, b: kept.append((a, b)))
    assert len({b.data_ptr() for _, b in kept}) == STEPS
    for (a, b), (i, wa, wb) in zip(kept, want):
        assert torch.equal(a, wa) and torch.equal(b, wb), (kind, guide, frames, i)
    assert not any(torch.equal(kept[i][1], kept[i + 1][1]) for i in range(STEPS - 1))


# ------------------------------------------------------------------ 5. one window
@pytest.mark.parametrize("kind", ["ddim", "dpm++"])
@pytest.mark.parametrize("guide", list(GUIDE))
def test_one_window_is_the_short_sampler(kind, guide):
    # no window_ops fixture: a clip of one window never reaches gather / blend
    want = _drive(kind, guide, T)
    model = Toy()
    got = _drive(kind, guide, T, model=model, window_batch=1)  # through sample_long
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert all(c[0].shape[0] == (2 if guide == "guided" else 1) * B for c in model.calls)


# ------------------------------------------------------------------ 6. no reference cycle
@pytest.mark.parametrize("guide", list(GUIDE))
@pytest.mark.parametrize("name", ["DDIMGraph", "DPMGraph", "LongDDIMGraph", "LongDPMGraph"])
def test_graphs_die_by_reference_count(name, guide):
    """A dead CUDAGraph inside a reference cycle would be destroyed by the cyclic collector,
    possibly inside a later capture (hipgraph.capture): nothing reachable from a graph object
    may point back at it."""
    scale, rescale = GUIDE[guide]
    long_ = name.startswith("Long")
    sampler = _sampler("dpm++" if "DPM" in name else "ddim")
    cond, feats, shape = _inputs(L if long_ else T)
    model, xt = Toy(), torch.randn(shape)
    was = gc.isenabled()
    gc.disable()
    try:
        windows = None
        if long_:
            windows = engine.WindowedDenoiser(model, WindowPlan(L, T, STRIDE), cond, feats, xt,
                                              scale != 1.0)
            g = getattr(engine, name)(model, sampler, windows, xt, scale, rescale)
        else:
            g = getattr(engine, name)(model, sampler, cond, feats, xt, scale, rescale)
        assert g.graph is None and g.xt.shape == xt.shape
        if not long_ and scale != 1.0:
            assert g.x2.shape[0] == 2 * B and g.xt.data_ptr() == g.x2.data_ptr()
        refs = [weakref.ref(o) for o in (g, windows) if o is not None]
        del g, windows
        assert [r() for r in refs] == [None] * len(refs)
    finally:
        if was:
            gc.enable()
