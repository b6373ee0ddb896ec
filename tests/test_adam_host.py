"""The Adam / AdamW step, host side (CPU, no kernel runs): the ABI of vd_adam_step and its
argument errors, vdiff.optim's descriptor table and schedule function, FusedAdamW's and
Trainer's argument checks, the state-dict interchange with torch.optim.Adam / AdamW, train.py's
flags -- and the check that the bounds of tests/_adam_cases.py hold for a numpy fp32 restatement
of the operation order the kernel source states, with and without fused multiply-adds."""
import ctypes
import inspect
import json
import math
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import _adam_cases as cases
from conftest import DROPIN, ROOT

from vdiff import _lib, ops
from vdiff.ema import CHUNK, chunk_ranges
from vdiff.optim import KERNEL_LAUNCHES, SCHEDULES, FusedAdamW, descriptor_rows, lr_at


# ------------------------------------------------------------------ ABI
def test_symbol_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "vdiff.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bvd_adam_step\s*\(", src)
    assert "vd_adam_step" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "vd_adam_step")
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(vd_[a-z0-9_]+)\s*\(", plain))
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert "#define VDIFF_ABI_VERSION 1" in src and _lib.ABI_VERSION == 1


def _header_struct(name):
    """[(type, field)] of `typedef struct { ... } name;` in include/vdiff.h."""
    src = open(os.path.join(ROOT, "include", "vdiff.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
        ctype = m.group(2) + m.group(3)
        out += [(ctype, f.strip()) for f in m.group(4).split(",")]
    return out


SIZES = {"float*": 8, "int64_t": 8, "double": 8, "int32_t": 4}


def test_structs_match_the_header():
    desc = _header_struct("vd_adam_desc")
    assert [f for _, f in desc] == [f for f, _ in _lib.AdamDesc._fields_]
    assert sum(SIZES[t] for t, _ in desc) == ctypes.sizeof(_lib.AdamDesc) == 48
    assert [getattr(_lib.AdamDesc, f).offset for f, _ in _lib.AdamDesc._fields_] == \
        [0, 8, 16, 24, 32, 40]
    hyper = _header_struct("vd_adam_hyper")
    assert [f for _, f in hyper] == [f for f, _ in _lib.AdamHyper._fields_]
    assert sum(SIZES[t] for t, _ in hyper) == ctypes.sizeof(_lib.AdamHyper) == 80
    for (t, f), (_, c) in zip(hyper, _lib.AdamHyper._fields_):
        assert ctypes.sizeof(c) == SIZES[t], f
    src = open(os.path.join(ROOT, "include", "vdiff.h")).read()
    for name, value in ops.LR_SCHEDULES.items():
        assert re.search(rf"VD_LR_{name.upper()}\s*=\s*{value}\b", src), name
    assert tuple(ops.LR_SCHEDULES) == SCHEDULES == ("constant", "cosine", "linear")


def _hyper(**kw):
    args = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True,
                warmup_steps=0, schedule="constant", total_steps=None, min_ratio=0.0,
                max_bad_run=0)
    args.update(kw)
    return ops.adam_hyper(**args)


def test_bad_arguments_fail_without_a_gpu():
    lib = _lib.load()
    t = ctypes.addressof((ctypes.c_char * 64)())      # never read: every call below fails first
    w = ctypes.addressof((ctypes.c_int64 * 8)())
    f = ctypes.addressof((ctypes.c_float * 2)())
    ok = _hyper()
    nan = float("nan")

    def call(descs=t, n=1, h=ok, steps=w, state=w, lr_out=f, flag=w):
        hp = ctypes.byref(h) if h is not None else None
        return lib.vd_adam_step(descs, n, hp, steps, state, None, None, lr_out, flag, None)

    bad = {
        "null descs": dict(descs=None), "null hyper": dict(h=None), "null steps": dict(steps=None),
        "null state": dict(state=None), "null lr_out": dict(lr_out=None),
        "null skip flag": dict(flag=None), "n_desc 0": dict(n=0), "n_desc -2": dict(n=-2),
        "beta1 1": dict(h=_hyper(betas=(1.0, 0.999))),
        "beta1 -0.1": dict(h=_hyper(betas=(-0.1, 0.9))),
        "beta2 1": dict(h=_hyper(betas=(0.9, 1.0))), "beta2 nan": dict(h=_hyper(betas=(0.9, nan))),
        "eps 0": dict(h=_hyper(eps=0.0)), "eps -1": dict(h=_hyper(eps=-1.0)),
        "eps nan": dict(h=_hyper(eps=nan)),
        "lr -1": dict(h=_hyper(lr=-1.0)), "lr nan": dict(h=_hyper(lr=nan)),
        "wd -1": dict(h=_hyper(weight_decay=-1.0)),
        "T = W cosine": dict(h=_hyper(schedule="cosine", warmup_steps=5, total_steps=5)),
        "T < W linear": dict(h=_hyper(schedule="linear", warmup_steps=5, total_steps=3)),
        "T unset cosine": dict(h=_hyper(schedule="cosine")),
        "r -0.1": dict(h=_hyper(min_ratio=-0.1)), "r 1.5": dict(h=_hyper(min_ratio=1.5)),
        "r nan": dict(h=_hyper(min_ratio=nan)),
        "W -1": dict(h=_hyper(warmup_steps=-1)), "K -1": dict(h=_hyper(max_bad_run=-1)),
    }
    for what, kw in bad.items():
        assert call(**kw) == 1 and lib.vd_last_error(), what
    h = _hyper()
    h.schedule = 7
    assert call(h=h) == 1 and b"schedule" in lib.vd_last_error()
    with pytest.raises(ValueError, match="schedule"):
        _hyper(schedule="step")


# ------------------------------------------------------------------ descriptor table
@pytest.mark.parametrize("chunk", [8, 64, CHUNK])
def test_rows_are_48_bytes_with_the_tensor_index(chunk):
    numels = [1, 0, 7, 8, 9, chunk - 1, chunk, chunk + 1, 2 * chunk + 3, 0, 5] + [1] * 300
    k = len(numels)
    base = {"p": 1 << 47, "m": 1 << 46, "v": 3 << 45, "g": 5 << 44}
    ptrs = {a: [b + 4096 * chunk * i + 4 * (i % 4) for i in range(k)] for a, b in base.items()}
    tensors = [1000 + 3 * i for i in range(k)]          # indices into the count array
    rows = descriptor_rows(ptrs["p"], ptrs["m"], ptrs["v"], ptrs["g"], numels, tensors, chunk)
    assert rows.dtype.itemsize == 48 and rows.view(np.uint8).size == 48 * len(rows)
    want = chunk_ranges(numels, chunk)
    assert len(rows) == len(want) == sum(-(-n // chunk) for n in numels)
    for r, (i, s, n) in zip(rows, want):
        for a in "pmvg":
            assert int(r[a]) == ptrs[a][i] + 4 * s
        assert (int(r["n"]), int(r["tensor"])) == (n, tensors[i])
    # a tensor's rows are consecutive (launch 2 advances the count at a tensor's first row)
    seen = [int(t) for t in rows["tensor"]]
    firsts = [t for j, t in enumerate(seen) if j == 0 or seen[j - 1] != t]
    assert firsts == [tensors[i] for i, n in enumerate(numels) if n > 0]
    d = _lib.AdamDesc.from_buffer_copy(rows.view(np.uint8).reshape(-1, 48)[-1].tobytes())
    i, s, n = want[-1]
    assert (d.p, d.m, d.v, d.g, d.n, d.tensor) == tuple(
        ptrs[a][i] + 4 * s for a in "pmvg") + (n, tensors[i])
    assert len(descriptor_rows([], [], [], [], [], [])) == 0
    with pytest.raises(ValueError):
        descriptor_rows([64], [64], [64], [64], [5], [0], 12)


# ------------------------------------------------------------------ schedule
def test_schedule_function():
    lr, W, T, r = 3e-4, 4, 10, 0.1
    for kind in SCHEDULES:
        def at(s, kind=kind):
            return lr_at(s, lr, warmup_steps=W, schedule=kind, total_steps=T, min_ratio=r)
        floor = lr if kind == "constant" else lr * r
        assert at(0) == pytest.approx(lr / W, rel=1e-15)        # s = 0: the first warm-up step
        assert at(W - 1) == pytest.approx(lr, rel=1e-15)        # warm = 1 from s = W - 1 on
        assert at(W) == pytest.approx(lr, rel=1e-15)            # q = 0: no decay yet
        assert at(T) == pytest.approx(floor, rel=1e-12)
        assert at(T + 1000) == pytest.approx(floor, rel=1e-12)  # clamped beyond T
        mid = at((W + T) // 2)
        if kind == "cosine":
            assert mid == pytest.approx(lr * (r + (1 - r) * 0.5), rel=1e-12)
        if kind == "linear":
            assert mid == pytest.approx(lr * (r + (1 - r) * 0.5), rel=1e-12)
            assert at(W + 1) == pytest.approx(lr * (r + (1 - r) * (1 - 1 / 6)), rel=1e-12)
        rates = [at(s) for s in range(T + 3)]
        assert all(a < b for a, b in zip(rates[:W - 1], rates[1:W]))        # warm-up rises
        assert all(a >= b for a, b in zip(rates[W:], rates[W + 1:]))        # then never rises
        # W = 0: no warm-up
        assert lr_at(0, lr, 0, kind, T, r) == pytest.approx(lr, rel=1e-15)
        assert lr_at(T, lr, 0, kind, T, r) == pytest.approx(floor, rel=1e-12)
    assert lr_at(5, lr) == lr and lr_at(0, lr, warmup_steps=1) == lr
    with pytest.raises(ValueError):
        lr_at(0, lr, 0, "step", 10)


# ------------------------------------------------------------------ FusedAdamW, Trainer, train.py
def _params(dtype=torch.float32):
    torch.manual_seed(0)
    return [torch.nn.Parameter(torch.randn(5, 3, dtype=dtype)),
            torch.nn.Parameter(torch.randn(7, dtype=dtype))]


def test_fused_adamw_argument_errors():
    assert KERNEL_LAUNCHES == 2
    sig = inspect.signature(FusedAdamW.__init__).parameters
    assert [sig[k].default for k in ("betas", "eps", "weight_decay", "decoupled", "warmup_steps",
                                     "schedule", "total_steps", "min_ratio", "max_bad_run",
                                     "chunk")] == \
        [(0.9, 0.999), 1e-8, 0.0, True, 0, "constant", None, 0.0, 0, CHUNK]
    nan = float("nan")
    bad = [dict(lr=-1.0), dict(lr=nan), dict(lr="1"), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -1)),
           dict(betas=(0.9,)), dict(betas=(0.9, nan)), dict(eps=0.0), dict(eps=-1e-8),
           dict(weight_decay=-0.1), dict(warmup_steps=-1), dict(warmup_steps=1.5),
           dict(schedule="step"), dict(schedule="cosine"), dict(schedule="linear", total_steps=0),
           dict(schedule="cosine", warmup_steps=5, total_steps=5),
           dict(schedule="linear", warmup_steps=5, total_steps=4), dict(min_ratio=-0.1),
           dict(min_ratio=1.1), dict(max_bad_run=-1), dict(max_bad_run=True), dict(chunk=12)]
    for kw in bad:
        args = dict(lr=1e-3)
        args.update(kw)
        with pytest.raises(ValueError):
            FusedAdamW(_params(), **args)
    with pytest.raises(TypeError, match="fp32 master parameters.*parameter 1.*bfloat16"):
        FusedAdamW([_params()[0], torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))], 1e-3)
    with pytest.raises(ValueError, match="contiguous parameters.*parameter 0"):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4, 4).t())], 1e-3)
    # construction works on the CPU; step() does not (no CPU fallback)
    ps = _params()
    opt = FusedAdamW(ps, 1e-3, warmup_steps=3, max_bad_run=2)
    assert int(opt.applied) == 0 and int(opt.skipped) == 0 and int(opt.tripped_at) == -1
    assert int(opt.skip_flag) == -1 and float(opt.lr) == 0.0 and opt.rebuilds == 0
    assert opt.skip_flag.dtype == torch.int64 and opt.lr.dtype == torch.float32
    opt.step()                                           # no gradient anywhere: nothing to do
    for p in ps:
        p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError, match="GPU only"):
        opt.step()
    assert opt.rebuilds == 0 and int(opt.applied) == 0


class _Sched:
    def add_noise(self, x0, eps, t):
        return x0 + eps


def test_trainer_options_and_errors():
    import torch.nn.functional as F
    from vdiff.engine import Trainer
    ps = inspect.signature(Trainer.__init__).parameters
    want = dict(optimizer="torch", weight_decay=0.0, decoupled_weight_decay=True, lr_warmup=0,
                lr_schedule="constant", lr_total_steps=None, lr_min_ratio=0.0, skip_bad_steps=0)
    assert {k: ps[k].default for k in want} == want
    m = torch.nn.Linear(4, 4)
    tr = Trainer(m, _Sched(), loss_fn=F.mse_loss)
    assert isinstance(tr.opt, torch.optim.Adam) and tr.lr is None and tr.skipped_steps is None
    nondefault = dict(weight_decay=0.01, decoupled_weight_decay=False, lr_warmup=2,
                      lr_schedule="cosine", lr_total_steps=10, lr_min_ratio=0.1, skip_bad_steps=1)
    for k, v in nondefault.items():
        with pytest.raises(ValueError, match=k):
            Trainer(m, _Sched(), loss_fn=F.mse_loss, **{k: v})
    with pytest.raises(ValueError, match="optimizer"):
        Trainer(m, _Sched(), loss_fn=F.mse_loss, optimizer="sgd")
    args = dict(nondefault)
    tr = Trainer(m, _Sched(), loss_fn=F.mse_loss, lr=3e-4, optimizer="hip", **args)
    assert isinstance(tr.opt, FusedAdamW) and tr.skip_bad_steps == 1
    g = tr.opt.param_groups[0]
    assert (g["lr"], g["weight_decay"], g["decoupled"], g["warmup_steps"], g["schedule"],
            g["total_steps"], g["min_ratio"], g["max_bad_run"]) == \
        (3e-4, 0.01, False, 2, "cosine", 10, 0.1, 1)
    assert float(tr.lr) == 0.0 and int(tr.skipped_steps) == 0
    tr.check_finite()                                   # nothing tripped
    for kw in (dict(lr_schedule="cosine"),
               dict(lr_schedule="linear", lr_warmup=5, lr_total_steps=5),
               dict(weight_decay=-1.0), dict(skip_bad_steps=-1), dict(lr_min_ratio=2.0)):
        with pytest.raises(ValueError):
            Trainer(m, _Sched(), loss_fn=F.mse_loss, optimizer="hip", **kw)
    # the default hip trainer keeps the fail-fast record
    tr = Trainer(m, _Sched(), loss_fn=F.mse_loss, optimizer="hip")
    assert tr.skip_bad_steps == 0 and tr.opt.param_groups[0]["max_bad_run"] == 0


def test_train_flags_and_defaults():
    src = f"import sys; sys.path.insert(0, {DROPIN!r}); sys.path.insert(1, {ROOT!r})\n"
    code = """
        import json, train
        keys = ("optimizer", "weight_decay", "lr_warmup", "lr_schedule", "lr_min_ratio",
                "skip_bad_steps")
        a = train.parse([])
        b = train.parse(["--optimizer", "hip", "--weight-decay", "0.01", "--lr-warmup", "2",
                         "--lr-schedule", "cosine", "--lr-min-ratio", "0.1",
                         "--skip-bad-steps", "3"])
        bad = 0
        for argv in (["--optimizer", "sgd"], ["--lr-schedule", "step"]):
            try:
                train.parse(argv)
            except SystemExit:
                bad += 1
        print(json.dumps([[getattr(a, k) for k in keys], [getattr(b, k) for k in keys], bad]))
    """
    out = subprocess.run([sys.executable, "-c", src + textwrap.dedent(code)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == [
        ["torch", 0.0, 0, "constant", 0.0, 0], ["hip", 0.01, 2, "cosine", 0.1, 3], 2]


# ------------------------------------------------------------------ state dicts
def _words(opt):
    return [int(x) for x in (opt.applied, opt.skipped, opt.bad_run, opt.tripped_at)]


def _torch_run(cls, ps, steps=3, **kw):
    opt = cls(ps, lr=1e-3, **kw)
    g = torch.Generator().manual_seed(1)
    for s in range(steps):
        for p in ps[:1] if s == 0 else ps:              # the second parameter is one step younger
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
        opt.zero_grad(set_to_none=True)
    return opt


@pytest.mark.parametrize("cls", [torch.optim.Adam, torch.optim.AdamW])
def test_state_dict_from_and_to_torch(cls):
    ps = _params()
    ref = _torch_run(cls, ps, weight_decay=0.05)
    sd = ref.state_dict()
    assert [float(sd["state"][i]["step"]) for i in (0, 1)] == [3.0, 2.0]
    opt = FusedAdamW(_params(), 5e-2, warmup_steps=7, max_bad_run=2)
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    # torch's options arrive, the ones torch does not know stay
    assert (g["lr"], g["weight_decay"], g["betas"], g["eps"]) == (1e-3, 0.05, (0.9, 0.999), 1e-8)
    assert g["decoupled"] is (cls is torch.optim.AdamW)
    assert (g["warmup_steps"], g["schedule"], g["max_bad_run"]) == (7, "constant", 2)
    assert "fused_state" not in g
    # counts: int64 views into one array; the words' defaults for a torch checkpoint
    own = [opt.state[p] for p in g["params"]]
    assert [int(s["step"]) for s in own] == [3, 2]
    assert all(s["step"].dtype == torch.int64 and s["step"].dim() == 0 for s in own)
    storage = {s["step"].untyped_storage().data_ptr() for s in own}
    assert len(storage) == 1
    assert _words(opt) == [3, 0, 0, -1]
    for s, p in zip(own, ps):
        assert torch.equal(s["exp_avg"], ref.state[p]["exp_avg"])
        assert torch.equal(s["exp_avg_sq"], ref.state[p]["exp_avg_sq"])
        assert s["exp_avg"].data_ptr() != ref.state[p]["exp_avg"].data_ptr()
    # and back: torch loads what FusedAdamW writes, and steps on it
    out = opt.state_dict()
    assert out["param_groups"][0]["fused_state"] == [3, 0, 0, -1]
    assert out["param_groups"][0]["decoupled_weight_decay"] is (cls is torch.optim.AdamW)
    assert out["state"][0]["step"].dtype == torch.float32
    assert int(opt.state[g["params"][0]]["step"]) == 3          # the live state kept its view
    assert opt.state[g["params"][0]]["step"].dtype == torch.int64
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    back = cls(ps2, lr=1.0)
    back.load_state_dict(out)
    assert back.param_groups[0]["lr"] == 1e-3 and back.param_groups[0]["weight_decay"] == 0.05
    for p, q in zip(ps2, ps):
        assert float(back.state[p]["step"]) == float(ref.state[q]["step"])
        assert torch.equal(back.state[p]["exp_avg"], ref.state[q]["exp_avg"])
        assert torch.equal(back.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"])
    gen = torch.Generator().manual_seed(9)
    grads = [torch.randn(p.shape, generator=gen) for p in ps]
    for o, params in ((ref, ps), (back, ps2)):
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        o.step()
    for p, q in zip(ps2, ps):
        assert torch.equal(p, q)                                 # the same step as never saved


def test_state_dict_round_trip_of_the_words():
    ps = _params()
    opt = FusedAdamW(ps, 1e-3, max_bad_run=2, weight_decay=0.1, decoupled=False)
    sd = opt.state_dict()
    assert sd["state"] == {} and sd["param_groups"][0]["fused_state"] == [0, 0, 0, -1]
    ref = _torch_run(torch.optim.Adam, ps)
    sd = ref.state_dict()
    sd["param_groups"][0]["fused_state"] = [5, 2, 1, -1]
    sd["state"][1]["step"] = 2                                   # a plain number (old torch)
    opt.load_state_dict(sd)
    assert _words(opt) == [5, 2, 1, -1]
    out = opt.state_dict()
    assert out["param_groups"][0]["fused_state"] == [5, 2, 1, -1]
    assert [float(out["state"][i]["step"]) for i in (0, 1)] == [3.0, 2.0]
    json.dumps(out["param_groups"])                              # plain Python values
    other = FusedAdamW(_params(), 1e-3)
    other.load_state_dict(out)
    assert _words(other) == [5, 2, 1, -1]
    assert other.param_groups[0]["decoupled"] is False and other.param_groups[0]["max_bad_run"] == 2


# ------------------------------------------------------------------ the bound
def test_kernel_source_states_the_order():
    src = cases.SRC
    for line in ("g  = fmaf(wdf, p, g)", "m  = fmaf(omb1, d, m)", "v  = fmaf(omb2, gg, a)",
                 "p  = p * keep", "r  = r / bc2s", "r  = r + epsf", "u  = m / r",
                 "p  = fmaf(-step, u, p)"):
        assert line in src, line
    assert "#pragma clang fp contract(off)" in src
    assert "-ffast-math" not in open(os.path.join(cases.PKG, "csrc", "Makefile")).read()


@pytest.mark.parametrize("mode", list(cases.MODES))
def test_bound_holds_for_fp32_restatement(mode):
    kw = cases.MODES[mode]
    worst = {}
    for seed in (7, 8):
        c = cases.Case(seed)
        P, M, V, _ = cases.reference(c.p, c.m, c.v, c.g, c.t, **kw)
        ep, em, ev = cases.bounds(c.p, c.m, c.v, c.g, c.t, **kw)
        assert (ep[c.mask] > 0).all() and (em[c.mask] > 0).all() and (ev[c.mask] > 0).all()
        # the update dwarfs the bound: an element updated zero times or twice cannot pass
        move = (np.abs(P - c.p.astype(np.float64)) / ep)[c.mask]
        # (everywhere for plain Adam; with weight decay the decay and the update cancel in a few
        # elements, so there: in all but 1 % of them)
        assert np.quantile(move, 0.01) > 100, np.quantile(move, 0.01)
        if mode == "adam":
            assert move.min() > 100, move.min()
        new = c.mask & (c.t == 1)
        if mode == "adam":                              # a first step moves by lr
            assert np.allclose(np.abs(P - c.p)[new], cases.LR, rtol=1e-4)
        for fused in (True, False):
            p, m, v = cases.emulate(c.p, c.m, c.v, c.g, c.t, fused=fused, **kw)
            for name, got, want, b in (("p", p, P, ep), ("m", m, M, em), ("v", v, V, ev)):
                r = cases.worst_ratio(got, want, b, c.mask)
                worst[name, fused] = max(worst.get((name, fused), 0.0), r)
    print(f"{mode}: largest error / bound of the fp32 restatement {worst}")
    assert max(worst.values()) <= 1.0, worst
    assert min(worst.values()) > 0.01, worst            # and the bounds are not vacuous


def test_the_bound_tells_a_wrong_step_apart():
    c = cases.Case()
    kw = cases.MODES["decoupled"]
    P, M, V, _ = cases.reference(c.p, c.m, c.v, c.g, c.t, **kw)
    ep, em, ev = cases.bounds(c.p, c.m, c.v, c.g, c.t, **kw)
    # a count off by one, the other decay mode, eps inside the square root's division
    for wrong in (dict(kw, t=c.t + 1), dict(cases.MODES["l2"], t=c.t),
                  dict(kw, t=c.t, eps=cases.EPS * 1e4)):
        t = wrong.pop("t")
        p, m, v = cases.emulate(c.p, c.m, c.v, c.g, t, **wrong)
        assert cases.worst_ratio(p, P, ep, c.mask) > 10
    assert math.isfinite(float(ep[c.mask].max()))
