"""vd_clip_metrics (vdiff.ops.clip_metrics, vdiff.metrics) against the float64 oracle of
tests/_metrics_cases.py: the SSIM map per position, ssim[b, t] and mse[b, t], weights, bad sizes,
repeatability eager and replayed from a HIP graph, and independence of the workspace's content.

Tolerances (derived in _metrics_cases, never from the kernel's output): the map may be off by
2 x (the error of the naive fp32 evaluation of the same input) + 2 (22 + 2) 2^-24; ssim[b, t] by
that plus the any-order fp32 term of its mean; mse[b, t] by the any-order fp32 bound of its C H W
non-negative terms.  The kernel's and the naive evaluation's measured map errors are printed and
recorded per input (profiles/metrics_accuracy.jsonl; the table of DESIGN section 4.3)."""
import math

import pytest
import torch

from conftest import record_metric

import _metrics_cases as mc
from _bounds import U_FP32, assert_elementwise

pytestmark = pytest.mark.gpu
dev = "cuda"
TD = {"fp32": torch.float32, "bf16": torch.bfloat16}
CASES = [(shape, dt) for shape, dts in mc.SHAPES for dt in dts]
BIG = mc.SHAPES[0][0]


def _run(x, y, dtype, weight=None, want_map=True, value_range=(-1, 1)):
    from vdiff import ops
    w = None if weight is None else weight.to(dev)
    return ops.clip_metrics(x.to(dev).to(TD[dtype]), y.to(dev).to(TD[dtype]), w, value_range,
                            want_map=want_map)


def _check_frames(got, ref, tol, C, H, W, what, nan_frames=()):
    """mse and ssim [B, T] against the oracle; `nan_frames`: frames that must be NaN."""
    T = ref["mse"].shape[1]
    live = [t for t in range(T) if t not in nan_frames]
    for t in nan_frames:
        assert torch.isnan(got.mse[:, t]).all() and torch.isnan(got.ssim[:, t]).all(), (what, t)
    mse, ssim = got.mse.cpu()[:, live], got.ssim.cpu()[:, live]
    r_mse = ref["mse"][:, live]
    assert_elementwise(mse, r_mse, r_mse, C * H * W, False, what=f"{what} mse")
    n_pos = C * (H - 10) * (W - 10)
    bound = tol + 2.0 * (n_pos + 2) * U_FP32 * ref["ssim_mag"][:, live]
    err = (ssim.double() - ref["ssim"][:, live]).abs()
    assert (err <= bound).all(), (what, "ssim", float(err.max()), float(bound.min()))
    return float(err.max())


@pytest.mark.parametrize("shape,dtype", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_values_against_oracle(shape, dtype):
    """Every content of _metrics_cases.CONTENTS: map per position, ssim and mse per frame, the
    weight sums (counts, exact); an input with values at +-1.5 scores bit for bit as its clamp."""
    C, (H, W) = shape[1], shape[-2:]
    T = 1 if len(shape) == 4 else shape[2]
    for content in mc.CONTENTS:
        what = f"{shape} {dtype} {content}"
        x, y, ref, tol, naive = mc.case(shape, dtype, content)
        got = _run(x, y, dtype)
        smap = got.ssim_map.cpu()
        rs = tuple(ref["map"].shape)
        assert tuple(smap.shape) == (rs[:2] + rs[3:] if len(shape) == 4 else rs)
        err = (smap.double().view(ref["map"].shape) - ref["map"]).abs()
        kerr = float(err.max())
        print(f"{what}: map error kernel {kerr:.3e}, naive fp32 {naive:.3e}, tolerance {tol:.3e}")
        record_metric(test="metrics_map", shape=list(shape), dtype=dtype, content=content,
                      kernel_err=kerr, naive_err=naive, tol=tol)
        assert kerr <= tol, (what, kerr, naive, tol, [int(i) for i in err.argmax().view(1)])
        _check_frames(got, ref, tol, C, H, W, what)
        assert got.mse.shape == got.ssim.shape == (shape[0], T)
        assert torch.equal(got.wsum_px.cpu(), torch.full((T,), float(H * W)))
        assert torch.equal(got.wsum_valid.cpu(), torch.full((T,), float((H - 10) * (W - 10))))
        if content in ("flat_same",):
            assert torch.equal(got.mse.cpu(), torch.zeros(shape[0], T)), what
        if content == "overshoot":
            assert (x.abs() > 1).any()
            cl = _run(x.clamp(-1, 1), y, dtype)
            for a, b in ((got.mse, cl.mse), (got.ssim, cl.ssim), (got.ssim_map, cl.ssim_map)):
                assert torch.equal(a, b), what


def test_pivoted_moments_beat_naive_fp32_where_frames_are_smooth():
    """On the smooth field and the flat pair the kernel's map error is far below the naive
    fp32 evaluation's (E[u^2] - E[u]^2 against C2 = 9e-4): at least ten times."""
    for content in ("smooth", "flat_apart"):
        x, y, ref, tol, naive = mc.case(BIG, "fp32", content)
        got = _run(x, y, "fp32")
        kerr = float((got.ssim_map.cpu().double() - ref["map"]).abs().max())
        print(f"{content}: kernel {kerr:.3e}, naive {naive:.3e}")
        assert kerr * 10 <= naive, (content, kerr, naive)


def test_value_range():
    """(lo, hi) = (0, 1) on u equals (-1, 1) on 2 u - 1 within the map tolerance; hi <= lo is
    refused."""
    from vdiff import ops
    x, y, ref, tol, _ = mc.case(BIG, "fp32", "near")
    got = _run((x.clamp(-1, 1) + 1) / 2, (y.clamp(-1, 1) + 1) / 2, "fp32", value_range=(0, 1))
    assert float((got.ssim_map.cpu().double() - ref["map"]).abs().max()) <= tol
    with pytest.raises(ValueError):
        ops.clip_metrics(x.to(dev), y.to(dev), value_range=(1, 1))


def _mse_rel(C, H, W):
    """The relative bound of mse[b, t]: the any-order fp32 sum of its C H W non-negative terms."""
    return 2.0 * (C * H * W + 2) * U_FP32


def _psnr_abs(rel):
    """|d psnr| = 10 / ln 10 |d mse| / mse, plus 1e-4 dB for log10 evaluated in fp32 (a few ulp
    of a value below 100 dB)."""
    return 10.0 / math.log(10.0) * rel * (1 + rel) + 1e-4


def _feathered_weight(T, H, W):
    from vdiff.metrics import region_weight
    from vdiff.schedulers import keep_mask
    return region_weight(keep_mask(T, H, W, generate_box=(0.4, 0.9, 0.2, 0.8), feather=3))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_weights(dtype):
    """A feathered box from keep_mask; a weight that is zero on one whole frame (NaN there, the
    others right, .mean() skips it); a weight of ones against weight=None, bit for bit."""
    from vdiff import metrics
    shape = BIG
    B, C, T, H, W = shape
    x, y, _, tol, _ = mc.case(shape, dtype, "near")
    w = _feathered_weight(T, H, W)
    assert 0 < float(w.min(dim=0).values.max()) and ((w > 0) & (w < 1)).any()
    ref = mc.oracle64(x, y, w)
    got = _run(x, y, dtype, w)
    _check_frames(got, ref, tol, C, H, W, f"feathered {dtype}")
    assert_elementwise(got.wsum_px.cpu(), ref["wsum_px"], ref["wsum_px"], H * W, False)
    assert_elementwise(got.wsum_valid.cpu(), ref["wsum_valid"], ref["wsum_valid"], H * W, False)
    # the map does not depend on the weight
    assert torch.equal(got.ssim_map, _run(x, y, dtype).ssim_map)

    w0 = w.clone()
    w0[1] = 0.0
    ref0 = mc.oracle64(x, y, w0)
    got0 = _run(x, y, dtype, w0)
    _check_frames(got0, ref0, tol, C, H, W, f"zero frame {dtype}", nan_frames=(1,))
    assert torch.equal(got0.mse[:, 0], got.mse[:, 0]) and torch.equal(got0.ssim[:, 2],
                                                                      got.ssim[:, 2])
    assert float(got0.wsum_px[1]) == 0.0 and float(got0.wsum_valid[1]) == 0.0
    m = metrics.clip_metrics(x.to(dev).to(TD[dtype]), y.to(dev).to(TD[dtype]), weight=w0)
    assert torch.isnan(m.psnr[:, 1]).all()
    mean = m.mean()
    live = [0, 2]
    assert mean["frames"] == {"mse": 2, "ssim": 2}
    assert math.isclose(mean["ssim"], float(ref0["ssim"][:, live].mean()),
                        abs_tol=tol + 2.0 * (C * (H - 10) * (W - 10) + 2) * U_FP32)
    rel = _mse_rel(C, H, W)
    assert math.isclose(mean["mse"], float(ref0["mse"][:, live].mean()), rel_tol=rel)
    want_psnr = float((-10 * torch.log10(ref0["mse"][:, live])).mean())
    assert math.isclose(mean["psnr"], want_psnr, abs_tol=_psnr_abs(rel))
    # a weight only the MSE sees: the border pixels of frame 0 (no valid centre carries weight)
    wb = torch.zeros(T, H, W)
    wb[0, 0, :] = 1.0
    gb = _run(x, y, dtype, wb)
    rb = mc.oracle64(x, y, wb)
    assert torch.isnan(gb.ssim).all() and torch.isnan(gb.mse[:, 1:]).all()
    assert_elementwise(gb.mse.cpu()[:, :1], rb["mse"][:, :1], rb["mse"][:, :1], C * H * W, False)

    ones = _run(x, y, dtype, torch.ones(T, H, W))
    none = _run(x, y, dtype)
    for name in ("mse", "ssim", "wsum_px", "wsum_valid", "ssim_map"):
        assert torch.equal(getattr(ones, name), getattr(none, name)), name


def test_wrappers_and_identical_clips():
    """vdiff.metrics: psnr = -10 log10(mse), +inf for identical clips; ssim 1 there."""
    from vdiff import metrics
    x, y, ref, tol, _ = mc.case(BIG, "fp32", "near")
    xd, yd = x.to(dev), y.to(dev)
    m = metrics.clip_metrics(xd, yd)
    assert torch.equal(metrics.psnr(xd, yd), m.psnr) and torch.equal(metrics.ssim(xd, yd), m.ssim)
    want = -10 * torch.log10(ref["mse"])
    assert (m.psnr.cpu().double() - want).abs().max() <= _psnr_abs(_mse_rel(*BIG[1:2], *BIG[-2:]))
    same = metrics.clip_metrics(xd, xd.clone())
    assert torch.isinf(same.psnr).all() and (same.psnr > 0).all()
    assert (same.ssim.cpu() - 1).abs().max() <= mc.MAP_FLOOR
    assert same.mean()["psnr"] == math.inf


@pytest.mark.parametrize("shape", [(1, 3, 2, 10, 77), (1, 3, 2, 45, 10), (1, 3, 10, 10)])
def test_frames_below_the_window_are_refused(shape):
    """H = 10 or W = 10: ValueError in Python, a non-zero code from the C call, no launch."""
    from vdiff import _lib, ops
    x = torch.zeros(shape, device=dev)
    with pytest.raises(ValueError, match="11 x 11"):
        ops.clip_metrics(x, x)
    lib = _lib.lib()
    T = 1 if len(shape) == 4 else shape[2]
    out = torch.full((4, shape[0] * T), 7.0, device=dev)
    ws = torch.zeros(1024, device=dev)
    assert lib.vd_clip_metrics_workspace_size(shape[0], shape[1], T, *shape[-2:]) == 0
    rc = lib.vd_clip_metrics(x.data_ptr(), x.data_ptr(), None, -1.0, 1.0, shape[0], shape[1], T,
                             shape[-2], shape[-1], _lib.VD_F32, out[0].data_ptr(),
                             out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), None,
                             ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"window" in lib.vd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((4, shape[0] * T), 7.0))


def _call(X, Y, Wt, outs, ws):
    from vdiff import _lib
    B, C, T, H, W = X.shape
    mse, ssim, wpx, wv, smap = outs
    _lib.call("vd_clip_metrics", X.data_ptr(), Y.data_ptr(), Wt.data_ptr(), -1.0, 1.0, B, C, T, H,
              W, _lib.VD_F32 if X.dtype == torch.float32 else _lib.VD_BF16, mse.data_ptr(),
              ssim.data_ptr(), wpx.data_ptr(), wv.data_ptr(), smap.data_ptr(), ws.data_ptr(),
              torch.cuda.current_stream().cuda_stream)


def _buffers(shape):
    B, C, T, H, W = shape
    f = dict(dtype=torch.float32, device=dev)
    return [torch.empty(B * T, **f), torch.empty(B * T, **f), torch.empty(T, **f),
            torch.empty(T, **f), torch.empty(B * C * T, H - 10, W - 10, **f)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_repeatable_eager_and_replayed(dtype):
    """Two calls give the same bits; one call captured on one stream and replayed twice gives
    the eager bits, and the graph holds kernel nodes only (two of them)."""
    from vdiff import _lib, hipgraph
    shape = BIG
    x, y, _, _, _ = mc.case(shape, dtype, "near")
    X, Y = x.to(dev).to(TD[dtype]), y.to(dev).to(TD[dtype])
    Wt = _feathered_weight(*shape[2:]).to(dev)
    nws = _lib.lib().vd_clip_metrics_workspace_size(*shape)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    a, b, g = _buffers(shape), _buffers(shape), _buffers(shape)
    _call(X, Y, Wt, a, ws)
    _call(X, Y, Wt, b, ws)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with hipgraph.capture(graph):
        _call(X, Y, Wt, g, ws)
    graph.instantiate()
    types = hipgraph.node_counts(graph)
    assert types == {"kernel": 2}, types
    for _ in range(2):
        for t in g:
            t.fill_(-3.0)
        ws.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(a, g):
            assert torch.equal(u, v)


def test_workspace_content_does_not_matter():
    """A workspace of 0xFF bytes (NaN in every word) and one of zeros: the same bits."""
    from vdiff import _lib
    shape = BIG
    x, y, _, _, _ = mc.case(shape, "fp32", "noise")
    X, Y = x.to(dev), y.to(dev)
    Wt = _feathered_weight(*shape[2:]).to(dev)
    nws = _lib.lib().vd_clip_metrics_workspace_size(*shape)
    res = []
    for fill in (0xFF, 0x00):
        ws = torch.full((nws,), fill, dtype=torch.uint8, device=dev)
        outs = _buffers(shape)
        _call(X, Y, Wt, outs, ws)
        torch.cuda.synchronize()
        res.append(outs)
    for u, v in zip(*res):
        assert torch.equal(u, v) and torch.isfinite(u).all()
