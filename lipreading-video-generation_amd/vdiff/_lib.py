"""ctypes binding of libvdiff.so (the C-ABI declared in include/vdiff.h).

This is the only place that talks to the native library.  There is no
fallback: if the library or a GPU is missing, every op raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# VDIFF_LIB: alternative build of the same library (kernel A/B experiments, tools/)
LIB_PATH = os.environ.get("VDIFF_LIB") or os.path.join(_HERE, "libvdiff.so")

VD_F32 = 0
VD_BF16 = 1
ABI_VERSION = 1
# enum vd_prediction / enum vd_loss_weighting
PREDICTIONS = {"eps": 0, "v": 1}
LOSS_WEIGHTINGS = {"none": 0, "min-snr": 1}
WINDOW_KMAX = 8  # VD_WINDOW_KMAX
X0_IDENTITY, X0_DDIM, X0_DPM = 0, 1, 2  # enum vd_x0_rule

_vp = C.c_void_p
_i = C.c_int
_i64 = C.c_int64
_u64 = C.c_uint64
_f = C.c_float
_sz = C.c_size_t


class ConvDesc(C.Structure):
    _fields_ = [(n, _i) for n in (
        "B", "Ti", "Hi", "Wi", "Ci", "To", "Ho", "Wo", "Co",
        "kt", "kh", "kw", "st", "sh", "sw", "pt", "ph", "pw",
        "x_cstride", "y_cstride", "dtype")]


class AttnDesc(C.Structure):
    _fields_ = [("nseq", _i), ("seq_len", _i), ("head_dim", _i), ("groups", _i),
                ("batch_stride", _i64), ("group_stride", _i64), ("token_stride", _i64),
                ("o_batch_stride", _i64), ("o_group_stride", _i64), ("o_token_stride", _i64),
                ("scale", _f), ("dtype", _i)]


class XAttnDesc(C.Structure):
    """vd_xattn_desc: queries / output as AttnDesc, K/V rows of their own."""
    _fields_ = [("q", AttnDesc), ("kv_len", _i), ("kv_batch_stride", _i64),
                ("kv_group_stride", _i64), ("kv_token_stride", _i64)]


class EmaDesc(C.Structure):
    """vd_ema_desc: one range of a parameter and of its shadow per rate."""
    _fields_ = [("src", _vp), ("dst", _vp * 4), ("n", _i64)]


class X0Source(C.Structure):
    """vd_x0_source: where vd_x0_abs_quantile's x0 comes from (enum vd_x0_rule)."""
    _fields_ = [("x", _vp), ("eps", _vp), ("eps_u", _vp), ("t", _vp), ("acp", _vp),
                ("coef", _vp), ("step", _vp), ("cfg_workspace", _vp), ("n_steps", _i64),
                ("rule", C.c_int32), ("prediction", C.c_int32), ("w", _f), ("rescale", _f)]


class GradDesc(C.Structure):
    """vd_grad_desc: one range of one fp32 gradient tensor."""
    _fields_ = [("g", _vp), ("n", _i64)]


class AdamDesc(C.Structure):
    """vd_adam_desc: one range of a parameter, its two moments and its gradient."""
    _fields_ = [("p", _vp), ("m", _vp), ("v", _vp), ("g", _vp), ("n", _i64), ("tensor", _i64)]


class AdamHyper(C.Structure):
    """vd_adam_hyper: the host-side hyperparameters of one vd_adam_step."""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("weight_decay", C.c_double), ("min_ratio", C.c_double),
                ("warmup_steps", _i64), ("total_steps", _i64), ("schedule", C.c_int32),
                ("decoupled", C.c_int32), ("max_bad_run", C.c_int32), ("reserved", C.c_int32)]


_SIGS = {
    "vd_version": (_i, []),
    "vd_last_error": (C.c_char_p, []),
    "vd_device_info": (_i, [C.c_char_p, _i]),
    "vd_timestep_embedding": (_i, [_vp, _i, _i, _f, _vp, _vp]),
    "vd_timestep_embedding_tab": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "vd_q_sample": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _vp]),
    "vd_p_sample_v1": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _vp]),
    "vd_p_sample_v2": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i,
                            _vp]),
    "vd_p_sample_cosine": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _vp]),
    "vd_ddim_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i64, _i64, _i, _vp]),
    "vd_ddim_step_pred": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i, _i64, _i64, _i,
                               _vp]),
    "vd_ddim_step_cfg_pred": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp,
                                   _f, _i, _i, _i64, _i64, _i, _vp]),
    "vd_diffusion_loss_workspace_size": (_sz, [_i64, _i64]),
    "vd_diffusion_loss": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _f, _i64, _i64, _i,
                               _vp, _vp, _vp, _sz, _vp]),
    "vd_diffusion_loss_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _f, _vp, _i64,
                                   _i64, _i, _vp, _vp]),
    "vd_cfg_workspace_size": (_sz, [_i64, _i64]),
    "vd_cfg_stats": (_i, [_vp, _vp, _f, _i64, _i64, _i, _vp, _sz, _vp]),
    "vd_ddim_step_cfg": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _f,
                              _i, _i64, _i64, _i, _vp]),
    "vd_cfg_combine": (_i, [_vp, _vp, _vp, _f, _f, _vp, _i64, _i64, _i, _vp]),
    "vd_dpm_step": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i, _i64, _i64, _i, _vp]),
    "vd_dpm_step_cfg": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _f, _f, _vp, _i, _i64,
                             _i64, _i, _vp]),
    "vd_x0_quantile_workspace_size": (_sz, [_i64, _i64]),
    "vd_x0_abs_quantile": (_i, [C.POINTER(X0Source), _i64, _f, _f, _i64, _i64, _i, _vp, _vp, _sz,
                                _vp]),
    "vd_ddim_step_thr": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _f,
                              _i, _vp, _i64, _i64, _i, _vp]),
    "vd_dpm_step_thr": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _f, _f, _vp, _vp,
                             _i64, _i64, _i, _vp]),
    "vd_ddim_step_known": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _f,
                                _i, _i, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i, _vp]),
    "vd_dpm_step_known": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _f, _f, _vp, _i, _vp,
                               _vp, _vp, _i64, _i64, _i64, _i64, _i, _vp]),
    "vd_window_gather": (_i, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i, _vp]),
    "vd_window_blend": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i64, _i64, _i64, _i64, _i64, _i,
                             _vp]),
    "vd_set_dropout_counter": (None, [_vp]),
    "vd_groupnorm_set_unroll": (_i, [_i]),
    "vd_groupnorm_workspace_size": (_sz, [_i, _i64, _i, _i]),
    "vd_groupnorm_silu_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _f, _i, _f,
                                   _u64, _i, _vp, _vp]),
    "vd_groupnorm_silu_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i,
                                   _i, _f, _u64, _i, _vp, _vp]),
    "vd_groupnorm_silu_bwd_add": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64,
                                       _i, _i, _i, _f, _u64, _i, _vp, _vp]),
    "vd_groupnorm_film_silu_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _f,
                                        _i, _f, _u64, _i, _vp, _vp]),
    "vd_groupnorm_film_silu_bwd_add": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _vp, _i, _i64, _i, _i, _i, _f, _u64, _i, _vp, _vp]),
    "vd_silu":(_i, [_vp, _vp, _i64, _i, _vp]),
    "vd_silu_bwd": (_i, [_vp, _vp, _vp, _i64, _i, _vp]),
    "vd_cond_concat": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "vd_cond_concat_bwd_workspace_size": (_sz, [_i, _i, _i, _i, _i]),
    "vd_cond_concat_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp,
                                _vp]),
    "vd_upsample_nearest_hw": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "vd_upsample_nearest_hw_bwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "vd_channel_sums_workspace_size": (_sz, [_i, _i]),
    "vd_channel_sums": (_i, [_vp, _i, _i64, _i, _i, _i, _vp, _vp, _vp]),
    "vd_conv_pack_weight": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "vd_conv_pack_weights": (_i, [_vp, _i, _i64, _i, _vp]),
    "vd_ema_update": (_i, [_vp, _i, _i, C.POINTER(_f), _i, _vp, _vp, _vp]),
    "vd_grad_clip_workspace_size": (_sz, [_i]),
    "vd_grad_sumsq": (_i, [_vp, _i, _vp, _sz, _vp]),
    "vd_grad_clip": (_i, [_vp, _i, _vp, _f, _vp, _vp]),
    "vd_adam_step": (_i, [_vp, _i, C.POINTER(AdamHyper), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vd_conv_set_wgrad": (_i, [C.c_int]),
    "vd_conv_set_halo": (_i, [_i]),
    "vd_conv3d_fwd": (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vd_conv3d_bwd_data": (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp]),
    "vd_conv3d_bwd_weight": (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp]),
    "vd_conv3d_bwd_weight_workspace_size": (_sz, [C.POINTER(ConvDesc)]),
    "vd_conv3d_bwd_weight_det": (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _i, _i, _vp, _sz, _vp]),
    "vd_attention_fwd": (_i, [C.POINTER(AttnDesc), _vp, _vp, _vp, _vp, _vp, _vp]),
    "vd_attention_fwd_workspace_size": (_sz, [C.POINTER(AttnDesc)]),
    "vd_attention_fwd_ws": (_i, [C.POINTER(AttnDesc), _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vd_attention_bwd_workspace_size": (_sz, [C.POINTER(AttnDesc)]),
    "vd_attention_set_config": (C.c_int, [C.c_int]),
    "vd_attention_bwd": (_i, [C.POINTER(AttnDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                              _vp, _vp]),
    "vd_attention_bwd_dq": (_i, [C.POINTER(AttnDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                 _vp]),
    "vd_attention_bwd_dkdv": (_i, [C.POINTER(AttnDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _vp]),
    "vd_cross_attention_fwd_workspace_size": (_sz, [C.POINTER(XAttnDesc)]),
    "vd_cross_attention_fwd": (_i, [C.POINTER(XAttnDesc), _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                                    _vp]),
    "vd_cross_attention_bwd_workspace_size": (_sz, [C.POINTER(XAttnDesc)]),
    "vd_cross_attention_bwd_dq": (_i, [C.POINTER(XAttnDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp]),
    "vd_cross_attention_bwd_dkdv": (_i, [C.POINTER(XAttnDesc), _vp, _vp, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp]),
    "vd_resize_plan": (_i, [_i, _i, _vp, _vp, _i]),
    "vd_frames_resize_normalize": (_i, [_vp, _i64, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i,
                                        _vp, _vp, _i, _i64, _i, _vp]),
    "vd_audio_window": (_i, [_vp, _i, _i64, _i, C.c_double, _i, _i, _i, _i, _i, _vp]),
    "vd_layernorm_workspace_size": (_sz, [_i, _i]),
    "vd_layernorm_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, C.c_float, _i, _vp]),
    "vd_layernorm_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _sz,
                              _vp]),
    "vd_gelu_tanh": (_i, [_vp, _vp, _i64, _i, _vp]),
    "vd_attention_short_path": (_i, [C.POINTER(AttnDesc)]),
    "vd_attention_bwd_short_path": (_i, [C.POINTER(AttnDesc)] + [C.c_void_p] * 8),
    "vd_attention_set_short": (_i, [_i]),
    "vd_mse_loss_workspace_size": (_sz, [_i64]),
    "vd_mse_loss": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _sz, _vp]),
    "vd_mse_loss_bwd": (_i, [_vp, _vp, _vp, _i64, _i, _vp, _vp]),
    "vd_gelu_tanh_bwd": (_i, [_vp, _vp, _vp, _i64, _i, _vp]),
    "vd_clip_metrics_workspace_size": (_sz, [_i, _i, _i, _i, _i]),
    "vd_clip_metrics": (_i, [_vp, _vp, _vp, _f, _f, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp,
                             _vp, _vp, _vp]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)

_lib = None
_lock = threading.Lock()


def load(path: str = LIB_PATH):
    """Load and type the library (no GPU needed to load)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise RuntimeError(
                f"libvdiff.so not found at {path}: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
        lib = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.vd_version() != ABI_VERSION:
            raise RuntimeError(f"libvdiff ABI {lib.vd_version()} != expected {ABI_VERSION}")
        _lib = lib
        return lib


def lib():
    return _lib if _lib is not None else load()


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().vd_last_error().decode(errors="replace")
        raise RuntimeError(f"libvdiff {what} failed (code {rc}): {msg}")


def call(name: str, *args) -> None:
    check(getattr(lib(), name)(*args), name)
