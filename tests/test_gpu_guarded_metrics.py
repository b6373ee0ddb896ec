"""vd_clip_metrics on guarded, NaN-poisoned buffers (tests/_guarded.py), through vdiff._lib.call
with the operands of vdiff.ops.clip_metrics, at the 45 x 77 shape (ragged tiles on both axes,
rows that are not 16-byte aligned) in fp32 and bf16, with and without weight, with and without
map.

Both clips, the weight, the four per-frame outputs, the map and the workspace live between two
guards of a NaN pattern; every output starts out as the pattern and the workspace is exactly
vd_clip_metrics_workspace_size bytes of 0xFF.  After the call every output is fully written with
its guards intact, the inputs are bit-identical and the workspace's guards are intact: a read
past a plane's last row or a patch's halo would bring a NaN into the scores, a write past the map
or the records would land in a guard.  Values are judged by tests/_metrics_cases.py, as
tests/test_gpu_metrics.py judges them."""
import pytest
import torch

import _metrics_cases as mc
from _bounds import U_FP32, assert_elementwise
from _guarded import Guarded, assert_clean, assert_finite

pytestmark = pytest.mark.gpu
dev = "cuda"
f32 = torch.float32
TD = {"fp32": torch.float32, "bf16": torch.bfloat16}
SHAPE = mc.SHAPES[0][0]


def _st():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weighted"])
@pytest.mark.parametrize("want_map", [False, True], ids=["nomap", "map"])
def test_guarded_clip_metrics(dtype, weighted, want_map):
    from vdiff import _lib
    from vdiff.metrics import region_weight
    from vdiff.schedulers import keep_mask
    B, C, T, H, W = SHAPE
    what = f"clip metrics {dtype} weighted={weighted} map={want_map}"
    x, y, ref, tol, _ = mc.case(SHAPE, dtype, "near")
    w = None
    if weighted:
        w = region_weight(keep_mask(T, H, W, generate_box=(0.4, 0.9, 0.2, 0.8), feather=3))
        ref = mc.oracle64(x, y, w)
    X = Guarded(SHAPE, TD[dtype], dev, x, name="x")
    Y = Guarded(SHAPE, TD[dtype], dev, y, name="y")
    Wt = Guarded((T, H, W), f32, dev, w, name="weight") if weighted else None
    MSE, SSIM = Guarded((B * T,), f32, dev, name="mse"), Guarded((B * T,), f32, dev, name="ssim")
    WPX, WV = Guarded((T,), f32, dev, name="wsum_px"), Guarded((T,), f32, dev, name="wsum_valid")
    MAP = Guarded((B * C * T, H - 10, W - 10), f32, dev, name="ssim_map") if want_map else None
    nws = _lib.lib().vd_clip_metrics_workspace_size(B, C, T, H, W)
    assert nws == B * C * T * 2 * 3 * 16      # 35 x 67 map positions: 2 x 3 tiles, 16 B each
    WS = Guarded.workspace(nws, dev, name="metrics workspace")
    _lib.call("vd_clip_metrics", X.ptr, Y.ptr, Wt.ptr if Wt else None, -1.0, 1.0, B, C, T, H, W,
              _lib.VD_BF16 if dtype == "bf16" else _lib.VD_F32, MSE.ptr, SSIM.ptr, WPX.ptr,
              WV.ptr, MAP.ptr if MAP else None, WS.ptr, _st())
    outs = [MSE, SSIM, WPX, WV] + ([MAP] if MAP else [])
    assert_clean(outs, [X, Y] + ([Wt] if Wt else []), [WS], what=what)
    assert_finite(outs, what=what)
    r_mse = ref["mse"].reshape(-1)
    assert_elementwise(MSE.payload(), r_mse, r_mse, C * H * W, False, what=what + " mse")
    bound = tol + 2.0 * (C * (H - 10) * (W - 10) + 2) * U_FP32 * ref["ssim_mag"].reshape(-1)
    assert ((SSIM.payload().double() - ref["ssim"].reshape(-1)).abs() <= bound).all(), what
    assert_elementwise(WPX.payload(), ref["wsum_px"], ref["wsum_px"], H * W, False, what=what)
    assert_elementwise(WV.payload(), ref["wsum_valid"], ref["wsum_valid"], H * W, False,
                       what=what)
    if MAP:
        err = (MAP.payload().double().view(ref["map"].shape) - ref["map"]).abs().max()
        assert float(err) <= tol, (what, float(err), tol)
