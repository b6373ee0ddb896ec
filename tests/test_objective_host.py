"""v-prediction and Min-SNR weighting, host side (CPU, no kernels): the C-ABI's new symbols, the
argument checks of Trainer / the samplers / the entry points, the shipped schedules under the
weighting, the v sampler's coefficient rows against a plain-Python rederivation, the Trainer's
host logic through a torch restatement of the objective, and the analytic Gaussian model in v
(tests/_objective_cases.py)."""
import ctypes
import json
import math
import re
import subprocess
import sys
import textwrap

import pytest
import torch

from conftest import DROPIN, ROOT

import _dpm_cases as dpm
import _objective_cases as cases

NEW_SYMBOLS = ("vd_diffusion_loss_workspace_size", "vd_diffusion_loss", "vd_diffusion_loss_bwd",
               "vd_ddim_step_pred", "vd_ddim_step_cfg_pred")


# ------------------------------------------------------------------ ABI
def test_new_symbols_in_header_lib_and_binding():
    import os
    from vdiff import _lib
    src = open(os.path.join(ROOT, "include", "vdiff.h")).read()
    assert re.search(r"#define\s+VDIFF_ABI_VERSION\s+1\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(vd_[a-z0-9_]+)\s*\(", code))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 1 and _lib.load().vd_version() == 1
    # the enums' values are the binding's
    for enum, table in (("vd_prediction", {"VD_PRED_EPS": "eps", "VD_PRED_V": "v"}),
                        ("vd_loss_weighting", {"VD_WEIGHT_NONE": "none",
                                               "VD_WEIGHT_MIN_SNR": "min-snr"})):
        body = re.search(r"enum\s+%s\s*\{([^}]*)\}" % enum, code).group(1)
        got = {k.strip(): int(v) for k, v in (item.split("=") for item in body.split(","))}
        want = _lib.PREDICTIONS if enum == "vd_prediction" else _lib.LOSS_WEIGHTINGS
        assert {table[k]: v for k, v in got.items()} == want


def test_native_argument_checks_without_a_gpu():
    """An invalid call fails in the library's own checks, before any launch."""
    from vdiff import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)  # never dereferenced: the checks below fail first
    args = lambda pred, wt, gamma, B: (one, one, one, one, one, one, 500, pred, wt,  # noqa: E731
                                       ctypes.c_float(gamma), B, 64, 0, one, one, one, 1 << 20,
                                       None)
    for bad, word in ((args(2, 0, 5.0, 2), b"prediction"), (args(1, 3, 5.0, 2), b"weighting"),
                      (args(1, 1, 0.0, 2), b"gamma"), (args(1, 1, 5.0, 65536), b"shape")):
        assert lib.vd_diffusion_loss(*bad) == 1
        assert word in lib.vd_last_error(), lib.vd_last_error()
    assert lib.vd_diffusion_loss_workspace_size(3, 768) == 3 * cases.partials(768)[0] * 4
    assert lib.vd_diffusion_loss_workspace_size(2, cases.P_RAGGED) == 2 * 3 * 4
    rc = lib.vd_ddim_step_pred(one, one, None, one, one, one, one, one, ctypes.c_float(0.0), 0, 7,
                               2, 64, 0, None)
    assert rc == 1 and b"prediction" in lib.vd_last_error()


# ------------------------------------------------------------------ argument checks
class _Sched:
    def __init__(self, T=8):
        a = torch.linspace(0.95, 0.05, T)
        self.sqrt_alpha_cum_prod = a.sqrt()
        self.sqrt_one_minus_alpha_cum_prod = (1 - a).sqrt()

    def add_noise(self, x0, eps, t):
        v = [1] * (x0.dim() - 1)
        return self.sqrt_alpha_cum_prod[t].view(-1, *v) * x0 \
            + self.sqrt_one_minus_alpha_cum_prod[t].view(-1, *v) * eps


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.s = torch.nn.Parameter(torch.tensor(0.75))

    def forward(self, xt, cond, audio, t):
        return self.s * xt


def _torch_objective(sched, prediction, weighting, gamma):
    """The objective restated in torch for CPU tensors: (pred, x0, eps, t) -> (loss, per)."""
    def fn(pred, x0, eps, t):
        v = [1] * (x0.dim() - 1)
        sa = sched.sqrt_alpha_cum_prod[t].view(-1, *v)
        s1m = sched.sqrt_one_minus_alpha_cum_prod[t].view(-1, *v)
        target = sa * eps - s1m * x0 if prediction == "v" else eps
        per = ((pred - target) ** 2).flatten(1).mean(dim=1)
        w = torch.ones_like(per)
        if weighting == "min-snr":
            snr = (sa / s1m).flatten() ** 2
            w = snr.clamp(max=gamma) / (snr + 1 if prediction == "v" else snr)
        return (w * per).mean(), per
    return fn


def test_trainer_argument_checks():
    import torch.nn.functional as F
    from vdiff.engine import Trainer
    mk = lambda **kw: Trainer(_Model(), _Sched(), lr=1e-3, batch_pack=False, **kw)  # noqa: E731
    for kw in (dict(prediction="x0"), dict(prediction=None), dict(loss_weighting="p2"),
               dict(loss_weighting="min-snr", snr_gamma=0.0),
               dict(loss_weighting="min-snr", snr_gamma=-1.0),
               dict(snr_gamma=float("nan")), dict(snr_gamma=float("inf")),
               dict(prediction="v", loss_fn=F.mse_loss),
               dict(loss_weighting="min-snr", loss_fn=F.mse_loss),
               dict(objective_fn=lambda *a: None)):
        with pytest.raises(ValueError):
            mk(**kw)
    t = mk()
    assert (t.prediction, t.loss_weighting, t.snr_gamma) == ("eps", "none", 5.0)
    assert t.objective is None and t.loss_per_sample is None
    assert mk(loss_fn=F.mse_loss).objective is None
    assert mk(prediction="v").objective is not None
    assert mk(loss_weighting="min-snr", snr_gamma=3).snr_gamma == 3.0


def test_trainer_refuses_a_schedule_with_no_snr():
    from vdiff.engine import Trainer
    for name, i, value in (("sqrt_one_minus_alpha_cum_prod", 0, 0.0),
                           ("sqrt_alpha_cum_prod", 7, 0.0)):
        s = _Sched()
        getattr(s, name)[i] = value
        Trainer(_Model(), s, batch_pack=False, prediction="v")  # no weighting: no snr needed
        with pytest.raises(ValueError, match=f"entry {i} of 8"):
            Trainer(_Model(), s, batch_pack=False, loss_weighting="min-snr")
    with pytest.raises(ValueError, match="tables"):
        Trainer(_Model(), object(), batch_pack=False, prediction="v")


@pytest.mark.parametrize("prediction,weighting", [("v", "none"), ("eps", "min-snr"),
                                                  ("v", "min-snr")])
def test_trainer_host_logic_through_the_hook(prediction, weighting):
    """The step on CPU with the torch restatement as objective_fn: the loss is the restated one
    on the model's prediction, loss_per_sample its second value, and the update follows the
    objective's own gradient (checked against autograd on the closed form)."""
    from vdiff.engine import Clip, Trainer
    sched = _Sched()
    fn = _torch_objective(sched, prediction, weighting, 5.0)
    g = torch.Generator().manual_seed(0)
    x0 = torch.rand((4, 3, 2, 2), generator=g) * 2 - 1
    eps = torch.randn(x0.shape, generator=g)
    t = torch.tensor([0, 3, 5, 7])
    clip = Clip(x0, x0, {}, eps, t)
    m = _Model()
    tr = Trainer(m, sched, lr=1e-2, batch_pack=False, prediction=prediction,
                 loss_weighting=weighting, objective_fn=fn)
    s0 = m.s.detach().clone().requires_grad_(True)
    want, per = fn(s0 * sched.add_noise(x0, eps, t), x0, eps, t)
    (grad,) = torch.autograd.grad(want, s0)
    loss = tr.step(clip)
    assert torch.equal(loss, want.detach())
    assert torch.equal(tr.loss_per_sample, per.detach()) and not tr.loss_per_sample.requires_grad
    # Adam's first step moves the scalar by lr against the gradient's sign
    assert float(m.s.detach()) == pytest.approx(0.75 - 1e-2 * math.copysign(1.0, float(grad)), abs=1e-6)
    tr.check_finite()


def test_sampler_argument_checks():
    from vdiff.schedulers import DDIMSampler, DPMSolverSampler
    sch = dpm.v2_scheduler()
    for cls in (DDIMSampler, DPMSolverSampler):
        assert cls(sch, steps=5).prediction == "eps"
        assert cls(sch, steps=5, prediction="v").prediction == "v"
        for bad in ("x0", "epsilon", None, 1):
            with pytest.raises(ValueError):
                cls(sch, steps=5, prediction=bad)
    from vdiff.engine import sample_ddpm
    with pytest.raises(ValueError):
        sample_ddpm(None, sch, torch.zeros(1), None, (1, 3, 4, 4), prediction="x0")


def _dropin(code):
    src = f"import sys; sys.path.insert(0, {DROPIN!r}); sys.path.insert(1, {ROOT!r})\n"
    out = subprocess.run([sys.executable, "-c", src + textwrap.dedent(code)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.strip().splitlines()[-1]


def test_entry_point_options():
    out = _dropin("""
        import inspect, json, train, test
        def refused(mod, argv):
            try:
                mod.parse(argv)
            except SystemExit as e:
                return e.code
            return None
        a = train.parse([])
        b = train.parse(["--prediction", "v", "--loss-weighting", "min-snr", "--snr-gamma", "3"])
        c, d = test.parse([]), test.parse(["--prediction", "v", "--sampler", "ddim"])
        resume = []
        for state, run in (({}, "eps"), ({"prediction": "v"}, "v"), ({}, "v"),
                           ({"prediction": "v"}, "eps"), ({"prediction": "eps"}, "v")):
            try:
                train.check_resume_prediction(state, run)
                resume.append("ok")
            except ValueError as e:
                resume.append("raises" if "--prediction" in str(e) else "?")
        print(json.dumps({
            "train_default": [a.prediction, a.loss_weighting, a.snr_gamma],
            "train_set": [b.prediction, b.loss_weighting, b.snr_gamma],
            "test": [c.prediction, d.prediction],
            "refused": [refused(train, ["--prediction", "x0"]),
                        refused(train, ["--loss-weighting", "p2"]),
                        refused(train, ["--snr-gamma", "0"]),
                        refused(train, ["--snr-gamma", "-2"]),
                        refused(test, ["--prediction", "x0"])],
            "resume": resume,
            "sample_images": inspect.signature(test.sample_images).parameters[
                "prediction"].default,
            "quartiles": train.quartile_line([1.0, 0.0, 3.0, 4.0], [2, 0, 3, 1])}))
    """)
    d = json.loads(out)
    assert d["train_default"] == ["eps", "none", 5.0]
    assert d["train_set"] == ["v", "min-snr", 3.0]
    assert d["test"] == ["eps", "v"]
    assert d["refused"] == [2, 2, 2, 2, 2]
    assert d["resume"] == ["ok", "ok", "raises", "raises", "raises"]
    assert d["sample_images"] == "eps"
    assert d["quartiles"] == " | mse by t quartile 0.5 - 1 4"


# ------------------------------------------------------------------ the shipped schedules
@pytest.mark.parametrize("name", ["v2", "linear", "cosine"])
def test_shipped_schedules_have_a_finite_snr_everywhere(name):
    """Every sqrt_acp and sqrt_1m_acp entry is > 0 in fp32 and the Min-SNR weights (gamma = 5),
    from the fp32 tables in fp64, are finite and in (0, 1], for eps and for v."""
    from vdiff.engine import Trainer, _sqrt_tables
    from vdiff.schedulers import (CosineNoiseScheduler, LinearNoiseScheduler,
                                  LinearNoiseSchedulerV2)
    sch = {"v2": LinearNoiseSchedulerV2(500, 0.00005, 0.015),
           "linear": LinearNoiseScheduler(100, 0.00085, 0.012),
           "cosine": CosineNoiseScheduler(2000)}[name]
    acp = dpm.schedules()[name]
    sa, s1m = _sqrt_tables(sch)
    assert sa.dtype == s1m.dtype == torch.float32 and sa.numel() == acp.numel()
    assert torch.equal(sa, acp.sqrt()) and torch.equal(s1m, (1 - acp).sqrt())
    assert bool((sa > 0).all()) and bool((s1m > 0).all())
    for prediction in cases.PREDICTIONS:
        w = cases.weight64(sa.double(), s1m.double(), prediction, "min-snr", 5.0)
        assert bool(torch.isfinite(w).all()) and float(w.min()) > 0 and float(w.max()) <= 1
    Trainer(_Model(), sch, batch_pack=False, prediction="v", loss_weighting="min-snr")


# ------------------------------------------------------------------ the v sampler's rows
@pytest.mark.parametrize("name", ["v2", "linear", "cosine"])
@pytest.mark.parametrize("steps,order,spacing", [(10, 2, "logsnr"), (20, 2, "logsnr"),
                                                 (7, 1, "linspace")])
def test_v_rows_against_rederivation(name, steps, order, spacing):
    from vdiff.schedulers import DPMSolverSampler

    class Tab:
        alpha_cum_prod = dpm.schedules()[name]

    e = DPMSolverSampler(Tab, steps=steps, order=order, spacing=spacing)
    v = DPMSolverSampler(Tab, steps=steps, order=order, spacing=spacing, prediction="v")
    assert torch.equal(e.timesteps, v.timesteps) and e.steps == v.steps
    assert torch.equal(e.coef[:, 2:], v.coef[:, 2:])       # A, B, C and the padding: the same bits
    assert torch.equal(e.coef64[:, 2:], v.coef64[:, 2:])
    want = torch.tensor(cases.coef_rows_v(Tab.alpha_cum_prod, v.timesteps.tolist(), order),
                        dtype=torch.float64)
    assert torch.equal(v.coef[:, :2], want[:, :2].float())  # rounded once from fp64
    assert torch.equal(v.coef, v.coef64.float())
    # sqrt and the divide are correctly rounded in torch and in Python alike: the same fp64
    assert torch.equal(v.coef64[:, :2], want[:, :2])
    a = Tab.alpha_cum_prod.double()[v.timesteps]
    assert torch.equal(v.coef[:, 0], (1 / a.sqrt()).float())
    assert torch.equal(v.coef[:, 1], ((1 - a).sqrt() / a.sqrt()).float())


# ------------------------------------------------------------------ the Gaussian model in v
@pytest.mark.parametrize("steps", [10, 20])
def test_gaussian_model_v_ends_where_eps_ends(steps):
    """With the optimal v* the fp64 recurrences in v end at the eps value: DDIM and the 2M
    table, within the running error bound _objective_cases derives (u = 2^-53)."""
    acp = dpm.schedules()["v2"]
    a = [float(v) for v in acp.double()]
    for s in dpm.S_VALUES:
        ts = dpm.logsnr_timesteps(acp, steps)
        rows_e = dpm.coef_rows(acp, ts, 2)
        rows_v = cases.coef_rows_v(acp, ts, 2)
        xe, xv, me, mv = cases.run_table_both(rows_e, rows_v, [a[t] for t in ts], s)
        bnd = cases.bound64(len(ts), cases.N_STEP_TABLE, me, mv)
        assert abs(xe) > 0 and me >= abs(xe) and mv >= abs(xv)
        assert abs(xv - xe) <= bnd, (s, steps, xv - xe, bnd)
        # and that value is the known one: _dpm_cases' own eps recurrence
        assert xe == pytest.approx(dpm.run_table(rows_e, [a[t] for t in ts], s), rel=1e-12)
        ts = dpm.linspace_timesteps(len(a), steps)
        xe, xv, me, mv = cases.run_ddim_both(acp, ts, s)
        bnd = cases.bound64(len(ts), cases.N_STEP_DDIM, me, mv)
        assert abs(xv - xe) <= bnd, (s, steps, xv - xe, bnd)
        assert xe == pytest.approx(dpm.run_ddim(acp, ts, s), rel=1e-12)


def test_rounding_counts_follow_the_partition_rule():
    assert cases.partials(768) == (1, 768) and cases.partials(105) == (1, 112)
    assert cases.partials(5000) == (3, 1672)
    assert cases.partials(cases.P_RAGGED) == (3, 1368)
    assert cases.lane_adds(768) == 8 and cases.lane_adds(105) == 8
    assert cases.lane_adds(5000) == 8 and cases.lane_adds(cases.P_RAGGED) == 8
    assert cases.n_per_sample(5000) == 5 + 8 + 8 + 3 + 1
    assert cases.n_loss(2, 5000) == cases.n_per_sample(5000) + 4 + 1 + 2 + 1
