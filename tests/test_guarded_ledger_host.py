"""Ledger of the guarded kernel tests: every function include/vdiff.h declares is either named in
a tests/test_gpu_guarded_*.py file -- as the "vd_..." string a vdiff._lib.call receives (directly,
or through a table of entry points the test loops over) or as a direct call on the loaded library
-- or listed in EXEMPT below with the reason it needs no guarded buffers.  Only functions that
touch no device memory are exempt: nothing that launches a kernel.  A new entry point therefore
fails this test until a guarded test calls it."""
import glob
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "vdiff.h")
HOST = "host function: no device memory is read or written"
SIZE = "returns a byte count computed on the host"
SWITCH = "process-wide host setting, no GPU call"
EXEMPT = {
    "vd_version": HOST,
    "vd_last_error": HOST,
    "vd_device_info": "queries the device properties; touches no device memory",
    "vd_mse_loss_workspace_size": SIZE,
    "vd_diffusion_loss_workspace_size": SIZE,
    "vd_cfg_workspace_size": SIZE,
    "vd_groupnorm_workspace_size": SIZE,
    "vd_cond_concat_bwd_workspace_size": SIZE,
    "vd_conv3d_bwd_weight_workspace_size": SIZE,
    "vd_channel_sums_workspace_size": SIZE,
    "vd_grad_clip_workspace_size": SIZE,
    "vd_attention_fwd_workspace_size": SIZE,
    "vd_attention_bwd_workspace_size": SIZE,
    "vd_cross_attention_fwd_workspace_size": SIZE,
    "vd_cross_attention_bwd_workspace_size": SIZE,
    "vd_layernorm_workspace_size": SIZE,
    "vd_groupnorm_set_unroll": SWITCH,
    "vd_conv_set_wgrad": SWITCH,
    "vd_conv_set_halo": SWITCH,
    "vd_attention_set_config": SWITCH,
    "vd_attention_set_short": SWITCH,
    "vd_set_dropout_counter": "stores a pointer on the host; the kernels that read it are listed",
    "vd_attention_short_path": "a predicate on the descriptor, evaluated on the host",
    "vd_resize_plan": "computes PIL's coefficient plan into host arrays",
    "vd_audio_window": "host DSP on host arrays",
}


def declared():
    """The functions of the header: a name followed by '(' at the start of a declaration, after
    comments are removed (typedefs, enums and macros declare no function)."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    names = re.findall(r"^[A-Za-z_][\w \t\*]*?\b(vd_\w+)\s*\(", src, flags=re.M)
    assert len(names) == len(set(names)) and len(names) > 60, len(names)
    return set(names)


def guarded_names(test_dir=None):
    """Every vd_* name a guarded GPU test file hands to _lib.call (a string literal) or calls on
    the library object."""
    test_dir = test_dir or os.path.join(ROOT, "tests")
    files = sorted(glob.glob(os.path.join(test_dir, "test_gpu_guarded_*.py")))
    assert files
    found = set()
    for path in files:
        body = open(path).read()
        body = re.sub(r'""".*?"""', "", body, flags=re.S)      # docstrings name, not call
        body = re.sub(r"#[^\n]*", "", body)
        found |= set(re.findall(r'"(vd_\w+)"', body))
        found |= set(re.findall(r"\.(vd_\w+)\(", body))
    return found


def test_header_parse_sees_known_declarations():
    d = declared()
    for name in ("vd_version", "vd_last_error", "vd_set_dropout_counter", "vd_conv3d_fwd",
                 "vd_mse_loss_workspace_size", "vd_adam_step", "vd_gelu_tanh_bwd",
                 "vd_frames_resize_normalize"):
        assert name in d, name
    assert "vd_conv_desc" not in d and "vd_status" not in d


def test_every_entry_point_is_guarded_or_exempt():
    d = declared()
    stale = sorted(set(EXEMPT) - d)
    assert not stale, f"EXEMPT names functions the header no longer declares: {stale}"
    called = guarded_names()
    missing = sorted(d - called - set(EXEMPT))
    assert not missing, ("declared in include/vdiff.h, in no tests/test_gpu_guarded_*.py and not "
                         f"exempt: {missing}")
    for name, reason in EXEMPT.items():
        assert reason.strip(), name


def test_ledger_reports_a_missing_and_a_stale_name(tmp_path):
    """The two failure modes, on a copy of the file set: without the optimizer file the four
    multi-tensor kernels are reported; an exemption the header does not declare is reported."""
    import shutil
    for path in glob.glob(os.path.join(ROOT, "tests", "test_gpu_guarded_*.py")):
        if not path.endswith("_optim.py"):
            shutil.copy(path, tmp_path)
    missing = declared() - guarded_names(str(tmp_path)) - set(EXEMPT)
    assert missing == {"vd_adam_step", "vd_ema_update", "vd_grad_sumsq", "vd_grad_clip"}, missing
    assert sorted(set(list(EXEMPT) + ["vd_gone"]) - declared()) == ["vd_gone"]
