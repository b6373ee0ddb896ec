"""Gradient clipping, host side (CPU, no kernel runs): the ABI of vd_grad_sumsq / vd_grad_clip
and their argument errors, the vectorised descriptor table of vdiff.clip against a plain
per-range loop, GradBucketer's gradient views, the Trainer / train.py options -- and the check
that the bound of tests/_clip_cases.py holds for a numpy fp32 emulation of the summation layout
the kernel source documents."""
import ctypes
import inspect
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import _clip_cases as cases
from conftest import DROPIN, ROOT

from vdiff import _lib
from vdiff.clip import KERNEL_LAUNCHES, GradClipper, check_max_norm, descriptor_rows
from vdiff.ema import CHUNK, chunk_ranges, range_arrays


# ------------------------------------------------------------------ ABI
def test_symbols_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "vdiff.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vd_grad_clip_workspace_size", "vd_grad_sumsq", "vd_grad_clip"):
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "vd_grad_desc" in src and "overflow" in src.lower()


def test_descriptor_is_16_bytes():
    assert ctypes.sizeof(_lib.GradDesc) == 16
    assert _lib.GradDesc.g.offset == 0 and _lib.GradDesc.n.offset == 8
    assert descriptor_rows([0], [1]).dtype.itemsize == 16


def test_workspace_size():
    lib = _lib.load()
    assert lib.vd_grad_clip_workspace_size(1) == 4
    assert lib.vd_grad_clip_workspace_size(3017) == 4 * 3017
    assert lib.vd_grad_clip_workspace_size(0) == 0 and lib.vd_grad_clip_workspace_size(-5) == 0


def test_bad_arguments_fail_without_a_gpu():
    lib = _lib.load()
    t = ctypes.addressof((ctypes.c_char * 64)())      # never read: every call below fails first
    w = ctypes.addressof((ctypes.c_float * 4)())
    rec = ctypes.addressof((ctypes.c_float * 2)())
    sumsq = {
        "null descs": (None, 1, w, 4, None),
        "null workspace": (t, 1, None, 4, None),
        "n_desc 0": (t, 0, w, 16, None),
        "n_desc -3": (t, -3, w, 16, None),
        "short workspace": (t, 4, w, 15, None),
        "no workspace bytes": (t, 1, w, 0, None),
    }
    for what, args in sumsq.items():
        assert lib.vd_grad_sumsq(*args) == 1 and lib.vd_last_error(), what
    assert b"workspace" in lib.vd_last_error()
    clip = {
        "null descs": (None, 1, w, 1.0, rec, None),
        "null workspace": (t, 1, None, 1.0, rec, None),
        "null record": (t, 1, w, 1.0, None, None),
        "n_desc 0": (t, 0, w, 1.0, rec, None),
        "n_desc -1": (t, -1, w, 1.0, rec, None),
        "max_norm 0": (t, 1, w, 0.0, rec, None),
        "max_norm -1": (t, 1, w, -1.0, rec, None),
        "max_norm nan": (t, 1, w, float("nan"), rec, None),
        "max_norm -inf": (t, 1, w, float("-inf"), rec, None),
    }
    for what, args in clip.items():
        assert lib.vd_grad_clip(*args) == 1 and lib.vd_last_error(), what
    assert b"max_norm" in lib.vd_last_error()


# ------------------------------------------------------------------ descriptor table
def _rows_by_loop(ptrs, numels, chunk):
    """The table written out range by range (what the vectorised builder must equal)."""
    out = []
    for p, n in zip(ptrs, numels):
        s = 0
        while s < n:
            out.append((p + 4 * s, min(chunk, n - s)))
            s += chunk
    return out


@pytest.mark.parametrize("chunk", [8, 64, CHUNK])
def test_vectorised_table_equals_the_loop(chunk):
    rng = np.random.default_rng(chunk)
    numels = [1, 0, 7, 8, 9, chunk - 1, chunk, chunk + 1, 2 * chunk + 3, 0, 3 * chunk, 5]
    numels += [int(n) for n in rng.integers(0, 4 * chunk, 40)] + [1] * 300
    # 16-B aligned and 4, 8, 12 bytes off; large addresses (above 2^47 a float would round)
    ptrs = [(1 << 47) + 4096 * i + 4 * (i % 4) for i in range(len(numels))]
    rows = descriptor_rows(ptrs, numels, chunk)
    want = _rows_by_loop(ptrs, numels, chunk)
    assert len(rows) == len(want) == sum(-(-n // chunk) for n in numels)
    assert [(int(r["g"]), int(r["n"])) for r in rows] == want
    assert rows["n"].min() >= 1 and rows["n"].max() <= chunk   # empty tensors got no range
    raw = rows.view(np.uint8).reshape(-1, 16)
    d = _lib.GradDesc.from_buffer_copy(raw[-1].tobytes())
    assert (d.g, d.n) == want[-1]
    # the list form of the rule is the same rule
    idx, start, n = range_arrays(numels, chunk)
    assert chunk_ranges(numels, chunk) == list(zip(idx.tolist(), start.tolist(), n.tolist()))
    assert [(ptrs[i] + 4 * s, m) for i, s, m in chunk_ranges(numels, chunk)] == want


def test_table_edge_cases():
    assert len(descriptor_rows([], [])) == 0
    assert len(descriptor_rows([64, 128], [0, 0])) == 0
    with pytest.raises(ValueError):
        descriptor_rows([64], [5], 12)
    with pytest.raises(ValueError):
        GradClipper(1.0, chunk=12)


def test_bucket_views_leave_the_flag_tail_out():
    """GradBucketer.grad_flats(): the gradient part of every bucket; the nparams "used" flags
    behind the last bucket's gradients are in no range of the table."""
    from vdiff.ddp import GradBucketer
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.Linear(30, 20),
                            torch.nn.Linear(20, 3))
    params = list(m.parameters())
    bk = GradBucketer(params, bucket_mb=4 * 700 / 2 ** 20)      # several buckets
    assert len(bk.buckets) >= 3
    flats = list(bk.grad_flats())
    assert [f.numel() for f in flats[:-1]] == [b.flat.numel() for b in bk.buckets[:-1]]
    last = bk.buckets[-1]
    assert flats[-1].numel() == last.flat.numel() - len(params)
    assert flats[-1].data_ptr() == last.flat.data_ptr()
    assert sum(f.numel() for f in flats) == sum(p.numel() for p in params)
    assert bk.flags.data_ptr() == flats[-1].data_ptr() + 4 * flats[-1].numel()
    # every parameter's gradient view lies inside some flat view, the flags in none
    rows = descriptor_rows([f.data_ptr() for f in flats], [f.numel() for f in flats], 64)
    covered = set()
    for r in rows:
        covered.update(range(int(r["g"]), int(r["g"]) + 4 * int(r["n"]), 4))
    for p in params:
        assert p.grad.data_ptr() in covered and \
            p.grad.data_ptr() + 4 * (p.numel() - 1) in covered
    for k in range(len(params)):
        assert bk.flags.data_ptr() + 4 * k not in covered
    assert len(covered) == sum(p.numel() for p in params)


# ------------------------------------------------------------------ GradClipper, Trainer, train.py
def test_clipper_argument_errors():
    assert KERNEL_LAUNCHES == 3
    for bad in (0, 0.0, -1, float("nan"), float("-inf"), None, "x", True):
        with pytest.raises(ValueError):
            GradClipper(bad)
    assert GradClipper(float("inf")).max_norm == float("inf")
    assert check_max_norm(2) == 2.0
    c = GradClipper(1.0)
    assert c.norm is None and c.coef is None and c.rebuilds == 0 and c.chunk == CHUNK
    with pytest.raises(TypeError, match="w.grad.*bfloat16"):
        c.clip([torch.zeros(4, dtype=torch.bfloat16)], ["w.grad"])
    with pytest.raises(ValueError, match="contiguous.*tensor 1"):
        c.clip([torch.zeros(4), torch.zeros(4, 4).t()])
    with pytest.raises(TypeError, match="tensor 0"):
        c.clip([None])
    with pytest.raises(RuntimeError, match="GPU only"):          # no CPU fallback
        c.clip([torch.zeros(4)])
    assert c.rebuilds == 0


class _Sched:
    def add_noise(self, x0, eps, t):
        return x0 + eps


def test_trainer_default_and_errors():
    import torch.nn.functional as F
    from vdiff.engine import Trainer
    ps = inspect.signature(Trainer.__init__).parameters
    assert ps["clip_grad_norm"].default is None
    m = torch.nn.Linear(4, 4)
    tr = Trainer(m, _Sched(), loss_fn=F.mse_loss)
    assert tr.clipper is None and tr.grad_norm is None and tr.clip_coef is None
    for bad in (0, 0.0, -1.0, float("nan"), float("-inf"), "1", True):
        with pytest.raises(ValueError, match="clip_grad_norm"):
            Trainer(m, _Sched(), loss_fn=F.mse_loss, clip_grad_norm=bad)
    for ok in (1, 0.5, float("inf")):
        tr = Trainer(m, _Sched(), loss_fn=F.mse_loss, clip_grad_norm=ok)
        assert tr.clipper.max_norm == float(ok) and tr.grad_norm is None  # no step yet


def test_train_option_default():
    src = f"import sys; sys.path.insert(0, {DROPIN!r}); sys.path.insert(1, {ROOT!r})\n"
    code = """
        import json, train
        a = train.parse([])
        b = train.parse(["--clip-grad-norm", "0.5"])
        c = train.parse(["--clip-grad-norm", "inf"])
        print(json.dumps([a.clip_grad_norm, b.clip_grad_norm, c.clip_grad_norm == float("inf")]))
    """
    out = subprocess.run([sys.executable, "-c", src + textwrap.dedent(code)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == [0.0, 0.5, True]


# ------------------------------------------------------------------ the bound
def test_constants_come_from_the_kernel_source():
    assert cases.KBLOCK == 256 and cases.KVEC == 8 and cases.C == CHUNK
    assert cases.depth() == 8 * 8 + 1 + 8 == 73
    L = cases.Layout()
    assert len(L.ranges) == 17 + cases.N_ONES
    n = len(L.ranges)
    assert 0 < cases.total_bound(n) < 5e-6
    assert cases.total_bound(n) / 2 < cases.norm_bound(n) < cases.coef_bound(n) < 3e-6
    pos = L.one_hot_positions()
    assert len(pos) == 15 and len(set(pos.values())) == 15


def test_bound_holds_for_fp32_emulation_of_the_layout():
    worst = 0.0
    for seed in (2024, 1, 2):
        L = cases.Layout(seed)
        n_desc = len(L.ranges)
        ref = cases.ref_norm64(L.host, L.mask)
        norm, parts = cases.emulate(L, L.host)
        # every partial within the total's fp32 part of its own fp64 sum
        for r in (4, 5, 6, 9, 12, 16, 17, n_desc - 1):
            i, s, n = L.ranges[r]
            o = L.offsets[i] + s
            exact = float(np.sum(L.host[o:o + n].astype(np.float64) ** 2))
            assert abs(float(parts[r]) - exact) <= cases.total_bound(1) * exact, r
        ratio = abs(float(norm) - ref) / (cases.norm_bound(n_desc) * ref)
        worst = max(worst, ratio)
        for max_norm in (np.float32(ref / 4), np.float32(ref * 4)):
            coef = cases.emulate_coef(norm, max_norm)
            want = min(1.0, float(max_norm) / (ref + 1e-6))
            worst = max(worst, abs(float(coef) - want) / (cases.coef_bound(n_desc) * want))
    print(f"fp32 emulation of the layout: largest error / bound {worst:.4f}")
    assert worst <= 1.0


def test_emulated_one_hot_norm_is_exact():
    L = cases.Layout()
    for what, (t, e) in L.one_hot_positions().items():
        buf = L.zeros()
        buf[L.offsets[t] + e] = 3.0
        norm, parts = cases.emulate(L, buf)
        assert norm == np.float32(3.0), what
        assert parts[L.range_of(t, e)] == np.float32(9.0) and np.count_nonzero(parts) == 1
    assert cases.emulate_coef(3.0, 1.5) < np.float32(0.5)        # the 1e-6 of the formula
    assert cases.emulate_coef(np.float32("nan"), 1.5) == 1 and cases.emulate_coef(0.0, 1.5) == 1
