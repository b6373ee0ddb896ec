"""Masked sampling, host side (CPU, no GPU): the C-ABI additions, fp64 self-checks of
tests/_known_cases.py (keep == 0 is the unmasked reference; the kept line), schedulers.keep_mask,
argument validation in the library, the ops and the sampler, and the entry point's flags."""
import inspect
import json
import os
import re
import subprocess
import sys
import textwrap

import pytest
import torch

from conftest import DROPIN, ROOT

import _dpm_cases as dpm
import _known_cases as cases
import _thr_cases as thr
from vdiff import _lib

KNOWN_SYMBOLS = ("vd_ddim_step_known", "vd_dpm_step_known")


# ------------------------------------------------------------------ 1. C ABI
def test_symbols_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "vdiff.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(vd_[a-z0-9_]+)\s*\(", src))
    for name in KNOWN_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTED_SYMBOLS, name


def _ddim(lib, known, keep, Bk, S, B=2, P=24, u=None, thresh=None, clip=0):
    p = 4096  # never followed: every call below is refused before anything is launched
    return lib.vd_ddim_step_known(p, p, u, None, p, None, p, p, p, p, 1.0, 0.0, None, 0.0, clip, 0,
                                  thresh, known, keep, Bk, S, B, P, 0, None)


def _dpm(lib, known, keep, Bk, S, B=2, P=24):
    p = 4096
    return lib.vd_dpm_step_known(p, p, None, p, None, p, p, 4, p, 1.0, 0.0, None, 0, None, known,
                                 keep, Bk, S, B, P, 0, None)


def test_library_refuses_bad_masks_without_a_gpu():
    lib = _lib.load()
    p = 4096
    for call in (_ddim, _dpm):
        assert call(lib, p, None, 1, 8) == 1 and b"together" in lib.vd_last_error()
        assert call(lib, None, p, 1, 8) == 1 and b"together" in lib.vd_last_error()
        for Bk, S in ((0, 8), (3, 8), (1, 0), (1, -8), (1, 5), (1, 48)):
            assert call(lib, p, p, Bk, S) == 1, (Bk, S)
            assert b"bad keep mask" in lib.vd_last_error(), (Bk, S)
    assert _ddim(lib, p, p, 1, 8, thresh=p, clip=1) == 1 and b"exclude" in lib.vd_last_error()
    # the other operands are checked as in the unmasked entry points
    assert lib.vd_ddim_step_known(None, None, None, None, None, None, None, None, None, None, 1.0,
                                  0.0, None, 0.0, 0, 0, None, p, p, 1, 8, 2, 24, 0, None) == 1
    assert b"null" in lib.vd_last_error()
    assert _ddim(lib, p, p, 1, 8, B=70000, u=p) == 1 and b"bad shape" in lib.vd_last_error()


# ------------------------------------------------------------------ 2. the case file, in fp64
def _rules(kind, B):
    if kind == "dpm":
        s = thr.dpm_sampler()
        return [dict(row=s.coef[i]) for i in dpm.kernel_rows(s)]
    t, tp = cases.timesteps(B)
    return [dict(t=t, tp=tp, acp=thr.acp_table())]


@pytest.mark.parametrize("kind", cases.KINDS)
def test_keep_zero_is_the_unmasked_reference(kind):
    B, C, S = cases.SHAPES[0]
    xt, c, u, other, xk = cases.inputs(B, C, S, False)
    zero = torch.zeros((1, S))
    for host in _rules(kind, B):
        for guide in cases.GUIDES:
            for mode in cases.MODES:
                ref = cases.masked(kind, mode, xt, c, u, other, guide, xk, zero, **host)
                for name in ("x0", "x_prev"):
                    want = ref["unmasked"][name]
                    assert torch.equal(ref[name][0], want[0]), (kind, guide, mode, name)
                assert not ref["one"].any()


def test_keep_pattern_covers_every_case():
    for B, C, S in cases.SHAPES:
        for rows in (False, True):
            k = cases.keep(B, S, rows)
            assert tuple(k.shape) == (B if rows else 1, S) and k.dtype == torch.float32
            assert (k == 0).any() and (k == 1).any() and ((k > 0) & (k < 1)).any()
            assert (k < 0).any() and (k > 1).any()
            # a run of ones that starts and one that ends inside an 8-vector
            ones = (k[0] >= 1).int()
            starts = ((ones[1:] - ones[:-1]) == 1).nonzero().flatten() + 1
            ends = ((ones[1:] - ones[:-1]) == -1).nonzero().flatten() + 1
            assert (starts % 8 != 0).any() and (ends % 8 != 0).any()
    assert cases.keep(3, 256, True)[0].tolist() != cases.keep(3, 256, True)[1].tolist()


@pytest.mark.parametrize("kind", ["ddim-eps", "ddim-v"])
def test_kept_line_ddim(kind):
    """xt on the line at t and k == 1: x_prev is on the line at t_prev and x0 is x_k, whatever
    the model output -- random, huge or NaN."""
    B, C, S = cases.SHAPES[0]
    _, c, u, z, xk = cases.inputs(B, C, S, False)
    t, tp = cases.timesteps(B)
    acp = thr.acp_table()
    a = acp.double()
    at = a[t].view(-1, 1)
    ap = torch.where(tp >= 0, a[tp.clamp_min(0)], torch.ones_like(a[t])).view(-1, 1)
    xt = cases.on_line(at, xk, z)
    ones = torch.ones((1, S))
    for guide in (None, (cases.W, 0.0)):
        for model in (c, 1e6 * c, torch.full_like(c, float("nan"))):
            ref = cases.masked(kind, "plain", xt, model, u, z, guide, xk, ones, t=t, tp=tp,
                               acp=acp)
            assert torch.equal(ref["x0"][0], xk.double())
            err = (ref["x_prev"][0] - cases.on_line(ap, xk, z)).abs().max()
            assert err <= 1e-12, (kind, guide, float(err))
    # the last step returns x_k itself
    last = tp < 0
    assert last.any()
    assert (ref["x_prev"][0][last] - xk.double()[last]).abs().max() <= 1e-12


@pytest.mark.parametrize("order", [1, 2])
def test_kept_line_2m(order):
    """The same for every row of the fp64 table, second-order rows included: both history
    entries are x_k, and A alpha_t + B + C = alpha_prev."""
    from vdiff.schedulers import DPMSolverSampler
    B, C, S = cases.SHAPES[0]
    _, c, u, z, xk = cases.inputs(B, C, S, False)
    s = DPMSolverSampler(dpm.v2_scheduler(), steps=8, order=order)
    a = s.acp.double()
    ones = torch.ones((1, S))
    second = 0
    for i in range(s.steps):
        row = s.coef64[i]
        at = float(a[s.timesteps[i]])
        ap = float(a[s.prev_timesteps[i]]) if int(s.prev_timesteps[i]) >= 0 else 1.0
        assert abs(float(row[2]) * at ** 0.5 + float(row[3]) + float(row[4]) - ap ** 0.5) <= 1e-12
        second += float(row[4]) != 0.0
        xt = cases.on_line(at, xk, z)
        for model in (c, torch.full_like(c, float("nan"))):
            ref = cases.masked("dpm", "plain", xt, model, u, xk, None, xk, ones, row=row)
            assert torch.equal(ref["x0"][0], xk.double())
            err = (ref["x_prev"][0] - cases.on_line(ap, xk, z)).abs().max()
            assert err <= 1e-12, (order, i, float(err))
    assert second == (s.steps - 2 if order == 2 else 0)
    assert torch.equal(ref["x_prev"][0], xk.double())  # the last row: A = 0, B = 1


def test_trajectory_bound_contracts():
    """The accumulated bound stays of the order of a few hundred roundings of the values: the
    per-step errors are contracted, not summed with growing weights."""
    from vdiff.schedulers import DDIMSampler, DPMSolverSampler
    xk, z = torch.full((4,), 0.8), torch.full((4,), 2.5)
    for s, rows in ((DDIMSampler(dpm.v2_scheduler(), steps=6), None),
                    (DPMSolverSampler(dpm.v2_scheduler(), steps=6), True)):
        tr = cases.trajectory(s.acp, s.timesteps, s.prev_timesteps, xk, z,
                              rows=s.coef if rows else None)
        assert len(tr) == s.steps and tr[-1][0] == 1.0
        for ap, E in tr:
            assert (E > 0).all() and (E < 1e-3).all(), (ap, E)


# ------------------------------------------------------------------ 3. keep_mask
def test_keep_mask_values():
    from vdiff.schedulers import keep_mask
    m = keep_mask(3, 8, 6)
    assert m.dtype == torch.float32 and tuple(m.shape) == (1, 1, 3, 8, 6)
    assert (m[0, 0, :, :4] == 1).all() and (m[0, 0, :, 4:] == 0).all()  # default: lower half
    m = keep_mask(2, 8, 8, generate_box=(0.25, 0.75, 0.5, 1.0))
    want = torch.ones(8, 8)
    want[2:6, 4:] = 0
    assert torch.equal(m[0, 0, 0], want) and torch.equal(m[0, 0, 1], want)
    m = keep_mask(4, 8, 8, generate_box=(0, 1, 0, 1), keep_frames=2)      # continuation
    assert (m[0, 0, :2] == 1).all() and (m[0, 0, 2:] == 0).all()
    m = keep_mask(3, 8, 8, keep_frames=1, feather=2)
    assert (m[0, 0, 0] == 1).all()
    col = m[0, 0, 1, :, 3]
    assert torch.allclose(col, torch.tensor([1, 1, 1, 1, 2 / 3, 1 / 3, 0, 0]), atol=1e-7), col
    assert torch.equal(m[0, 0, 1], m[0, 0, 2])
    # a ramp on all four sides of an inner box, none at the frame's border
    m = keep_mask(1, 12, 12, generate_box=(0.25, 0.75, 0.25, 1.0), feather=1)[0, 0, 0]
    assert m[3, 6] == 0.5 and m[8, 6] == 0.5 and m[5, 3] == 0.5 and m[5, 11] == 0 \
        and m[4, 4] == 0 and m[2, 6] == 1 and m[3, 3] == 0.5
    assert ((m >= 0) & (m <= 1)).all()
    for bad in (dict(generate_box=(0.5, 0.5, 0, 1)), dict(generate_box=(0, 1.5, 0, 1)),
                dict(generate_box=(0, 1, 0)), dict(keep_frames=5), dict(keep_frames=-1),
                dict(feather=-1)):
        with pytest.raises(ValueError):
            keep_mask(4, 8, 8, **bad)


# ------------------------------------------------------------------ 4. validation
def test_ops_reject_bad_masks_and_cpu_tensors():
    from vdiff import ops
    x = torch.zeros(2, 3, 8)
    t, tp = torch.tensor([10, 10]), torch.tensor([0, 0])
    acp = thr.acp_table()
    s = thr.dpm_sampler()
    idx = torch.zeros(1, dtype=torch.int64)
    k = torch.zeros(1, 8)
    calls = (lambda **kw: ops.ddim_step(x, x, t, tp, acp, **kw),
             lambda **kw: ops.ddim_step_cfg(x, x, x, t, tp, acp, 7.5, **kw),
             lambda **kw: ops.dpm_step(x, x, x.clone(), s.coef, idx, **kw),
             lambda **kw: ops.dpm_step_cfg(x, x, x, x.clone(), s.coef, idx, 7.5, **kw))
    for call in calls:
        with pytest.raises(RuntimeError, match="GPU only"):
            call(known=x, keep=k)
        for bad in (dict(known=x), dict(keep=k),
                    dict(known=torch.zeros(2, 3, 9), keep=k),              # not xt's shape
                    dict(known=x.bfloat16(), keep=k),                       # not xt's dtype
                    dict(known=x, keep=torch.zeros(1, 9)),                  # S
                    dict(known=x, keep=torch.zeros(3, 8)),                  # Bk
                    dict(known=x, keep=torch.zeros(8)),                     # not [Bk, S]
                    dict(known=x, keep=k.double()),                         # not fp32
                    dict(known=x, keep=torch.zeros(8, 2).t()[:1])):         # not contiguous
            with pytest.raises(ValueError):
                call(**bad)


def test_sampler_level_validation():
    from vdiff.sampling import _masked_start
    from vdiff.schedulers import DDIMSampler, keep_mask
    s = DDIMSampler(dpm.v2_scheduler(), steps=4)
    z = torch.zeros(2, 3, 4, 8, 8)
    xk = torch.zeros_like(z)
    keep = keep_mask(4, 8, 8)
    assert _masked_start(s, z, None, None) == (z, None, None)
    bad_high, bad_low = keep.clone(), keep.clone()
    bad_high[0, 0, 0, 0, 0] = 1.5
    bad_low[0, 0, 0, 0, 0] = -0.25
    for known, k in ((xk, None), (None, keep), (xk[:1], keep), (xk[:, :, :2], keep),
                     (xk, keep[:, :, :2]), (xk, keep.expand(3, -1, -1, -1, -1)),
                     (xk, keep.view(-1)), (xk, bad_high), (xk, bad_low),
                     (xk, torch.full_like(keep, float("nan")))):
        with pytest.raises(ValueError):
            _masked_start(s, z, known, k)


def test_signatures():
    from vdiff import engine, ops
    from vdiff.schedulers import DDIMSampler, DPMSolverSampler
    for fn in (engine.sample_ddim, engine.sample_dpm, engine.sample_long, DDIMSampler.step, DDIMSampler.step_guided, DPMSolverSampler.step,
               DPMSolverSampler.step_guided, engine.DDIMGraph.__init__):
        # keyword-only, and (schedulers._mask_options) kept out of the reported signature where
        # an earlier test pins the positional list
        assert {"known": None, "keep": None}.items() <= inspect.unwrap(fn).__kwdefaults__.items()
    for fn in (ops.ddim_step, ops.ddim_step_cfg, ops.dpm_step, ops.dpm_step_cfg,
               engine.LongDDIMGraph.__init__, engine.LongDPMGraph.__init__):
        p = inspect.signature(fn).parameters
        assert p["known"].default is None and p["keep"].default is None, fn
    # ancestral DDPM sampling is out of scope: its signature is what it was
    assert list(inspect.signature(engine.sample_ddpm).parameters) == [
        "model", "scheduler", "cond", "audio", "shape", "n_timesteps", "generator", "callback",
        "guidance_scale", "guidance_rescale", "prediction"]


# ------------------------------------------------------------------ 5. the entry point
def _dropin(code, ok=True):
    src = f"import sys; sys.path.insert(0, {DROPIN!r}); sys.path.insert(1, {ROOT!r})\n"
    out = subprocess.run([sys.executable, "-c", src + textwrap.dedent(code)],
                         capture_output=True, text=True, timeout=600)
    assert (out.returncode == 0) == ok, out.stderr[-3000:]
    return out


def test_entry_point_flags():
    out = _dropin("""
        import json, test
        a = test.parse([])
        b = test.parse(["--sampler", "ddim", "--known", "k.npy"])
        c = test.parse(["--sampler", "dpm++", "--known", "k.npy", "--generate-box", "0", "1",
                        "0.25", "0.75", "--keep-frames", "2", "--mask-feather", "3"])
        d = test.parse(["--sampler", "ddim", "--known", "k.npy", "--keep-mask", "m.npy"])
        print(json.dumps([[a.known, a.keep_mask, a.generate_box, a.keep_frames, a.mask_feather],
                          [b.known, b.keep_mask, b.generate_box, b.keep_frames, b.mask_feather],
                          [c.known, c.generate_box, c.keep_frames, c.mask_feather],
                          [d.known, d.keep_mask]]))
    """)
    assert json.loads(out.stdout.strip().splitlines()[-1]) == [
        [None, None, None, None, None], ["k.npy", None, None, None, None],
        ["k.npy", [0.0, 1.0, 0.25, 0.75], 2, 3], ["k.npy", "m.npy"]]


@pytest.mark.parametrize("argv", [["--known", "k.npy"],
                                  ["--sampler", "ddpm-v2", "--known", "k.npy"],
                                  ["--sampler", "ddpm-v2", "--keep-frames", "1"],
                                  ["--sampler", "ddim", "--keep-frames", "1"],
                                  ["--sampler", "ddim", "--generate-box", "0", "1", "0", "1"],
                                  ["--sampler", "ddim", "--mask-feather", "2"],
                                  ["--sampler", "ddim", "--keep-mask", "m.npy"],
                                  ["--sampler", "ddim", "--known", "k.npy", "--keep-mask",
                                   "m.npy", "--keep-frames", "1"],
                                  ["--sampler", "dpm++", "--known", "k.npy", "--keep-frames",
                                   "-1"]])
def test_entry_point_refuses(argv):
    """Ancestral DDPM (the default sampler) has no step kernel that keeps the clip, and a mask
    needs the clip it keeps: an argparse error (exit status 2 and a usage message)."""
    out = _dropin(f"import test; test.parse({argv!r})", ok=False)
    assert out.returncode == 2 and "usage:" in out.stderr and "error:" in out.stderr, out.stderr
