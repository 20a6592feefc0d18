"""CPU tests of the yardsticks of the CLIP pixel gradient (tests/clip_grad_oracle.py, tests/golden/clip_vision/*_grad.pt):

* on whole-frame windows of uint8-valued square frames the window preprocessing equals ``restated_preprocess`` of
  test_clip_score_host.py, the restatement already pinned to PIL / CLIPImageProcessor there (float64: 1e-12);
* the stored fp32 autograd gradients of transformers reproduce their stored error against float64, and that error stays under
  the cap of the forward tests (rel-L2 2e-5): the bar of the GPU test, 4 x this error, is a multiple of something small;
* the plain-torch tower of the oracle, under autograd in float64, reproduces transformers' float64 gradient (1e-10)."""
import importlib.util
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import clip_score as cs  # noqa: E402
import clip_grad_oracle as cgo  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "clip_vision")
_spec = importlib.util.spec_from_file_location("clip_score_host", os.path.join(ROOT, "tests", "test_clip_score_host.py"))
_host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_host)


@pytest.mark.parametrize("side,S", [(48, 32), (24, 32), (32, 32), (100, 32)])
def test_window_restatement_equals_restated_preprocess_on_whole_frames(side, S):
    frames = torch.stack([_host.smooth_noise_image(side, side, seed=side + i) for i in range(2)])
    want = _host.restated_preprocess(frames, S)
    x = frames.permute(0, 3, 1, 2).to(torch.float64) / 127.5 - 1
    got = cgo.preprocess_windows(x, None, S, cs.CLIP_MEAN, cs.CLIP_STD)
    assert float((got - want).abs().max()) <= 1e-12
    got = cgo.preprocess_windows(x, [(0, 0, side, side)] * 2, S, cs.CLIP_MEAN, cs.CLIP_STD)
    assert float((got - want).abs().max()) <= 1e-12


def test_tap_counts_of_the_branches():
    assert cgo.tap_count(20, 32) == 4          # upsampling: 4 taps
    assert cgo.tap_count(32, 32) == 1          # the identity: one weight of 1
    assert cgo.tap_count(64, 32) > 4           # antialiasing widens the support


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_golden_gradients(name):
    g = torch.load(os.path.join(GOLD, f"{name}.pt"))
    gg = torch.load(os.path.join(GOLD, f"{name}_grad.pt"))
    g64, g32 = gg["grad64"], gg["grad32"]
    assert g64.dtype == torch.float64 and g32.dtype == torch.float32 and g64.shape == g["pixel_values"].shape == g32.shape
    err = [float((g32[i].double() - g64[i]).norm() / g64[i].norm()) for i in range(g64.shape[0])]
    print(name, "fp32 autograd of transformers against float64:", ["%.2e" % e for e in err])
    assert err == pytest.approx(gg["err32"].tolist(), rel=1e-9)
    assert 0 < max(err) <= 2e-5
    sd = {k: (v.float() if v.is_floating_point() else v) for k, v in g["state_dict"].items()}
    vision, _, vproj, _ = cs.split_clip_state_dict(sd)
    vcfg = cs.infer_vision_config(vision, vproj, g["config"]["vision_config"])
    own = cgo.embeds_vjp(dict(vision, **{"visual_projection.weight": vproj}), vcfg, g["pixel_values"], gg["g_embeds"])
    rel = [float((own[i] - g64[i]).norm() / g64[i].norm()) for i in range(g64.shape[0])]
    print(name, "float64 restatement against transformers in float64:", ["%.2e" % e for e in rel])
    assert max(rel) <= 1e-10
