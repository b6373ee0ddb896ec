"""use_scale_shift_norm without a GPU: the FiLM model's state dict against the reference's
(names and shapes recorded in tests/golden/film_unet_tiny3d.npz), the constructor options that
still raise, and the entry points' flag and resume-file check."""
import json
import subprocess
import sys
import textwrap

import pytest
import torch

from conftest import DROPIN, ROOT, golden

from oracle.fixtures import TINY3D


def _recorded_state():
    g = golden("film_unet_tiny3d.npz")
    names = bytes(g["state_names"].numpy().tolist()).decode().split("\n")
    shapes = [tuple(int(v) for v in row[:int(r)])
              for row, r in zip(g["state_shapes"], g["state_ranks"])]
    assert len(names) == len(shapes) > 50
    return list(zip(names, shapes))


def test_film_unet_state_dict_matches_reference():
    from vdiff.nn import ResBlock, UNetModel
    with torch.device("meta"):
        m = UNetModel(image_size=64, **TINY3D, use_scale_shift_norm=True)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == _recorded_state()
    blocks = [b for b in m.modules() if isinstance(b, ResBlock)]
    assert blocks and all(b.use_scale_shift_norm and
                          b.emb_layers[1].out_features == 2 * b.out_channels for b in blocks)
    # the default model is unchanged: emb_layers keeps out_channels outputs
    with torch.device("meta"):
        d = UNetModel(image_size=64, **TINY3D)
    assert all(b.emb_layers[1].out_features == b.out_channels
               for b in d.modules() if isinstance(b, ResBlock))


def test_film_unet_audio_passes_the_flag():
    from vdiff.nn import ResBlock
    from vdiff.unet_audio import UNetAudio
    with torch.device("meta"):
        m = UNetAudio(image_size=32, in_channels=3, model_channels=32, out_channels=3,
                      num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2), dims=3,
                      audio_feature_dim=64, projected_audio_dim=16, audio_encoder=False,
                      use_scale_shift_norm=True)
    assert all(b.emb_layers[1].out_features == 2 * b.out_channels
               for b in m.modules() if isinstance(b, ResBlock))


@pytest.mark.parametrize("kw", [dict(up=True), dict(down=True)])
def test_resblock_updown_still_raises(kw):
    from vdiff.nn import ResBlock
    for film in (False, True):
        with pytest.raises(NotImplementedError) as e:
            ResBlock(64, 256, 0.0, use_scale_shift_norm=film, **kw)
        assert "use_scale_shift_norm" not in str(e.value)
    from vdiff.nn import UNetModel
    with pytest.raises(NotImplementedError):
        UNetModel(image_size=64, **TINY3D, resblock_updown=True)


def test_film_op_raises_on_cpu_tensors():
    from vdiff import ops
    x = torch.zeros(1, 32, 2, 2)
    with pytest.raises(RuntimeError):
        ops.group_norm_film_silu(x, torch.ones(32), torch.zeros(32), torch.zeros(1, 64))


def _dropin(code):
    src = f"import sys; sys.path.insert(0, {DROPIN!r}); sys.path.insert(1, {ROOT!r})\n"
    out = subprocess.run([sys.executable, "-c", src + textwrap.dedent(code)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.strip().splitlines()[-1]


def test_entry_point_flag_and_resume_check():
    out = _dropin("""
        import json, train, test
        a, b = train.parse([]), train.parse(["--use-scale-shift-norm"])
        c, d = test.parse([]), test.parse(["--use-scale-shift-norm"])
        resume = []
        for state, run in (({}, False), ({"use_scale_shift_norm": True}, True),
                           ({"use_scale_shift_norm": False}, False), ({}, True),
                           ({"use_scale_shift_norm": True}, False),
                           ({"use_scale_shift_norm": False}, True)):
            try:
                train.check_resume_scale_shift_norm(state, run)
                resume.append("ok")
            except ValueError as e:
                both = "True" in str(e) and "False" in str(e)
                resume.append("raises" if both and "use_scale_shift_norm" in str(e) else "?")
        print(json.dumps({"train": [a.use_scale_shift_norm, b.use_scale_shift_norm],
                          "test": [c.use_scale_shift_norm, d.use_scale_shift_norm],
                          "resume": resume}))
    """)
    d = json.loads(out)
    assert d["train"] == [False, True]
    assert d["test"] == [False, True]
    assert d["resume"] == ["ok", "ok", "ok", "raises", "raises", "raises"]
