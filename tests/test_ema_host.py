"""Weight EMA, host side (CPU, no kernel runs): the ABI of vd_ema_update and its argument
errors, the chunk table vdiff.ema builds, the Trainer / train.py signatures and defaults, EMA's
own errors and checkpoint format -- and the derivation of the per-element bound the GPU tests
(tests/test_gpu_ema.py) hold the kernel to.

The bound.  ref = e + (1 - d)(p - e) in fp64 on the fp32 inputs and the fp32 value of d;

    |got - ref| <= 2^-24 |ref| + 4 * 2^-24 (1 - d) |p - e|

is the rounding of the output plus the three roundings of 1 - d, p - e and the product (and
one unit of slack: the output rounding is relative to the computed sum, not to ref).  A numpy
fp32 emulation of both the fused-multiply-add and the unfused order stays below it
(test_bound_holds_for_fp32_emulation prints the largest ratio; 0.9995 when this was
written), and over N updates the allowed error is the sum of the per-step bounds (an error
carried into a step is multiplied by d <= 1); the emulated drift over 300 steps was 0.09 of
that sum."""
import ctypes
import inspect
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import _ema_cases as cases
from conftest import DROPIN, ROOT

from vdiff import _lib
from vdiff.ema import CHUNK, EMA, chunk_ranges, descriptor_rows


# ------------------------------------------------------------------ ABI
def test_symbol_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "vdiff.h")).read()
    assert re.search(r"\bint\s+vd_ema_update\s*\(", src)
    assert "vd_ema_desc" in src and "#define VDIFF_ABI_VERSION 1" in src
    assert "vd_ema_update" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "vd_ema_update")
    assert _lib.load().vd_version() == 1


def test_descriptor_is_48_bytes():
    assert ctypes.sizeof(_lib.EmaDesc) == 48
    assert descriptor_rows([0], [[0]], [1]).dtype.itemsize == 48
    assert _lib.EmaDesc.src.offset == 0 and _lib.EmaDesc.dst.offset == 8
    assert _lib.EmaDesc.n.offset == 40


def _call(descs, n_desc, k, rates, warmup, num_updates):
    lib = _lib.load()
    arr = None if rates is None else (ctypes.c_float * len(rates))(*rates)
    rc = lib.vd_ema_update(descs, n_desc, k, arr, warmup, num_updates, None, None)
    return rc, lib.vd_last_error().decode()


def test_bad_arguments_fail_without_a_gpu():
    table = (ctypes.c_char * 48)()          # never read: every call below fails first
    t = ctypes.addressof(table)
    count = ctypes.addressof((ctypes.c_int64 * 1)())
    bad = {
        "null descs": (None, 1, 1, [0.5], 0, None),
        "null rates": (t, 1, 1, None, 0, None),
        "n_desc 0": (t, 0, 1, [0.5], 0, None),
        "n_desc -3": (t, -3, 1, [0.5], 0, None),
        "k 0": (t, 1, 0, [0.5], 0, None),
        "k 5": (t, 1, 5, [0.1, 0.2, 0.3, 0.4, 0.5], 0, None),
        "rate 1": (t, 1, 1, [1.0], 0, None),
        "rate -0.1": (t, 1, 2, [0.5, -0.1], 0, None),
        "rate nan": (t, 1, 1, [float("nan")], 0, None),
        "warmup without count": (t, 1, 1, [0.5], 1, None),
    }
    for what, args in bad.items():
        rc, msg = _call(*args)
        assert rc == 1 and msg, (what, rc, msg)
    assert "warmup" in _call(t, 1, 1, [0.5], 1, None)[1]
    assert "k=5" in _call(t, 1, 5, [0.1] * 5, 0, count)[1]


# ------------------------------------------------------------------ chunk table
def _covers_exactly_once(numels, chunk):
    ranges = chunk_ranges(numels, chunk)
    seen = [np.zeros(n, np.int32) for n in numels]
    for i, s, n in ranges:
        assert 0 < n <= chunk and s >= 0 and s + n <= numels[i], (i, s, n)  # inside tensor i
        assert s % chunk == 0
        seen[i][s:s + n] += 1
    for i, c in enumerate(seen):
        assert (c == 1).all(), i
    return ranges


def test_chunk_table_covers_every_element_once():
    assert cases.C == CHUNK and CHUNK % 8 == 0
    ranges = _covers_exactly_once(list(cases.SIZES), CHUNK)
    assert len(ranges) == sum(-(-n // CHUNK) for n in cases.SIZES)
    ones = _covers_exactly_once([1] * cases.N_ONES, CHUNK)
    assert len(ones) == cases.N_ONES  # far beyond the pack kernel's 1024 jobs
    _covers_exactly_once(list(cases.SIZES) + [1] * 5, 8)
    with pytest.raises(ValueError):
        chunk_ranges([5], 12)


def test_descriptor_rows_address_the_ranges():
    numels = [9, CHUNK + 1]
    src, d0, d1 = [1 << 20, 2 << 20], [3 << 20, 4 << 20], [5 << 20, 6 << 20]
    rows = descriptor_rows(src, [d0, d1], numels)
    assert [int(r["n"]) for r in rows] == [9, CHUNK, 1]
    assert int(rows[2]["src"]) == src[1] + 4 * CHUNK
    assert [int(x) for x in rows[2]["dst"]] == [d0[1] + 4 * CHUNK, d1[1] + 4 * CHUNK, 0, 0]
    raw = rows.view(np.uint8).reshape(3, 48)
    d = _lib.EmaDesc.from_buffer_copy(raw[2].tobytes())
    assert d.src == src[1] + 4 * CHUNK and d.n == 1 and d.dst[1] == d1[1] + 4 * CHUNK
    assert d.dst[2] is None and d.dst[3] is None


# ------------------------------------------------------------------ signatures and defaults
def test_trainer_signature_defaults():
    from vdiff.engine import Trainer
    ps = inspect.signature(Trainer.__init__).parameters
    assert ps["ema_rates"].default == () and ps["ema_warmup"].default is False


def test_train_options():
    src = f"import sys; sys.path.insert(0, {DROPIN!r}); sys.path.insert(1, {ROOT!r})\n"
    code = """
        import json, train
        a = train.parse([])
        b = train.parse(["--ema-rate", "0.999", "0.9999"])
        c = train.parse(["--ema-rate", "0.9", "--ema-warmup"])
        print(json.dumps([list(a.ema_rate), a.ema_warmup, list(b.ema_rate), b.ema_warmup,
                          list(c.ema_rate), c.ema_warmup]))
    """
    out = subprocess.run([sys.executable, "-c", src + textwrap.dedent(code)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    import json
    assert json.loads(out.stdout.strip().splitlines()[-1]) == [
        [], False, [0.999, 0.9999], False, [0.9], True]


def test_trainer_builds_ema_only_when_asked():
    import torch.nn.functional as F
    from vdiff.engine import Trainer

    class Sched:
        def add_noise(self, x0, eps, t):
            return x0 + eps

    m = torch.nn.Linear(4, 4)
    assert Trainer(m, Sched(), loss_fn=F.mse_loss).ema is None
    tr = Trainer(m, Sched(), loss_fn=F.mse_loss, ema_rates=(0.5, 0.9), ema_warmup=True)
    assert tr.ema.rates == (0.5, 0.9) and tr.ema.warmup
    with pytest.raises(RuntimeError, match="GPU only"):  # no CPU fallback
        tr.ema.update()


# ------------------------------------------------------------------ EMA errors, checkpoint
def _net():
    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.BatchNorm1d(7), torch.nn.Linear(7, 3))
    m[2].bias.requires_grad_(False)
    return m


def test_ema_errors():
    with pytest.raises(TypeError):
        EMA(_net().to(torch.bfloat16))
    m = _net()
    m[0].weight = torch.nn.Parameter(torch.randn(5, 7).t())
    assert not m[0].weight.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        EMA(m)
    with pytest.raises(ValueError, match="rates"):
        EMA(_net(), rates=(0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError, match="duplicate"):
        EMA(_net(), rates=(0.9, 0.99, 0.9))
    with pytest.raises(ValueError):
        EMA(_net(), rates=(1.0,))
    with pytest.raises(ValueError):
        EMA(_net(), rates=())


def test_tracks_trainable_parameters_and_state_dict():
    m = _net()
    e = EMA(m, rates=(0.5, 0.9))
    assert e.names == ["0.weight", "0.bias", "1.weight", "1.bias", "2.weight"]
    assert int(e.num_updates) == 0 and e.num_updates.dtype == torch.int64
    for sh in e.shadows:
        for s, p in zip(sh, e.params):
            assert torch.equal(s, p) and s.data_ptr() != p.data_ptr()
    e.shadows[1][0].add_(1.0)
    sd = e.state_dict(0.9)
    assert list(sd) == list(m.state_dict())
    assert torch.equal(sd["0.weight"], m[0].weight + 1.0)
    assert sd["2.bias"].data_ptr() == m[2].bias.data_ptr()          # untracked: the model's
    assert sd["1.running_mean"].data_ptr() == m[1].running_mean.data_ptr()
    other = _net()
    other.load_state_dict(sd)
    assert torch.equal(other[0].weight, m[0].weight + 1.0)
    with pytest.raises(ValueError):
        e.state_dict()            # two rates: name one
    with pytest.raises(KeyError):
        e.state_dict(0.7)
    # swapped(): EMA weights inside, the training weights back bit for bit, same storage,
    # version counters advanced (ops.frozen_weights keys on them)
    before = [p.detach().clone() for p in m.parameters()]
    ptr, ver = m[0].weight.data_ptr(), m[0].weight._version
    with e.swapped(m, 0.9):
        assert torch.equal(m[0].weight, before[0] + 1.0) and m[0].weight.data_ptr() == ptr
        assert m[0].weight._version > ver
        inside = m[0].weight._version
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), before))
    assert m[0].weight.data_ptr() == ptr and m[0].weight._version > inside


def test_checkpoint_round_trip(tmp_path):
    e = EMA(_net(), rates=(0.5, 0.9), warmup=True)
    for j, sh in enumerate(e.shadows):
        for s in sh:
            s.add_(j + 1.0)
    e.num_updates.fill_(41)
    path = tmp_path / "ema.pt"
    torch.save(e.checkpoint(), path)
    d = torch.load(path, weights_only=True)
    assert d["rates"] == [0.5, 0.9] and d["warmup"] is True and int(d["num_updates"]) == 41
    f = EMA(_net(), rates=(0.5, 0.9), warmup=True)
    f.load_checkpoint(d)
    assert int(f.num_updates) == 41
    for a, b in zip(e.shadows, f.shadows):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="rates"):
        EMA(_net(), rates=(0.5,)).load_checkpoint(d)


# ------------------------------------------------------------------ the bound
def _inputs(n, seed):
    rng = np.random.default_rng(seed)
    scale = np.float32(10.0) ** rng.integers(-3, 3, n).astype(np.float32)
    p = (rng.standard_normal(n).astype(np.float32) * scale).astype(np.float32)
    e = (p + rng.standard_normal(n).astype(np.float32) * scale
         * np.float32(10.0) ** rng.integers(-4, 1, n).astype(np.float32)).astype(np.float32)
    return p, e


def test_bound_holds_for_fp32_emulation():
    worst = 0.0
    decays = [cases.decay32(r) for r in (0.0, 0.5, 0.999, 0.9999)]
    decays += [cases.decay32(0.9999, True, n) for n in (0, 1, 89, 10 ** 6)]
    assert float(decays[4]) == pytest.approx(0.1) and decays[7] == np.float32(0.9999)
    assert decays[6] == np.float32(np.float32(90) / np.float32(99))  # 89: the warm-up branch
    for k, d in enumerate(decays):
        p, e = _inputs(200_000, k)
        ref, b = cases.ref64(p, e, d), cases.bound(p, e, d)
        for fused in (True, False):
            err = np.abs(cases.emulate(p, e, d, fused).astype(np.float64) - ref)
            ok = b > 0
            assert (err[~ok] == 0).all()
            worst = max(worst, float((err[ok] / b[ok]).max()))
    print(f"one update: largest emulated error / bound {worst:.4f}")
    assert worst <= 1.0


def test_summed_bound_holds_for_emulated_drift():
    rng = np.random.default_rng(11)
    n, steps, d = 4096, 300, cases.decay32(0.999)
    p = rng.standard_normal(n).astype(np.float32)
    worst = 0.0
    for fused in (True, False):
        e32, e64, allowed = p.copy(), p.astype(np.float64), np.zeros(n)
        for _ in range(steps):
            p = (p + np.float32(1e-2) * rng.standard_normal(n).astype(np.float32)).astype(
                np.float32)
            e32 = cases.emulate(p, e32, d, fused)
            pe = p.astype(np.float64)
            new = e64 + (1.0 - float(d)) * (pe - e64)
            allowed += cases.U * np.abs(new) + 4 * cases.U * (1.0 - float(d)) * np.abs(pe - e64)
            e64 = new
        worst = max(worst, float((np.abs(e32 - e64) / allowed).max()))
    print(f"{steps} updates: largest emulated drift / summed bound {worst:.3f}")
    assert worst <= 1.0
