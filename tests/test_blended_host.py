"""CPU tests of the Blended Diffusion driver's host side: the seeded windows and the parser's refusals (which come before any
device work)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import blended  # noqa: E402
from loco_edit_amd.define_argparser import parse_args  # noqa: E402

BASE = ["--sh_file_name", "x.sh", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Random"]


@pytest.mark.parametrize("H,W", [(32, 32), (40, 56), (256, 256)])
def test_windows_are_seeded_and_inside_the_frame(H, W):
    a = blended.draw_boxes(torch.Generator().manual_seed(7), 8, H, W)
    assert a == blended.draw_boxes(torch.Generator().manual_seed(7), 8, H, W)
    assert a != blended.draw_boxes(torch.Generator().manual_seed(8), 8, H, W)
    assert len(a) == 8 and a[0] == (0, 0, H, W)
    lo = round(0.75 * min(H, W))
    for top, left, h, w in a[1:]:
        assert h == w and lo <= h <= min(H, W)
        assert 0 <= top and top + h <= H and 0 <= left and left + w <= W
    assert blended.draw_boxes(torch.Generator().manual_seed(7), 1, H, W) == [(0, 0, H, W)]


def test_flag_defaults_and_refusals():
    args = parse_args(BASE)
    assert not args.run_edit_blended_diffusion
    assert (args.clip_guidance_scale, args.blended_num_aug, args.range_scale) == (1000.0, 8, 50.0)
    on = BASE + ["--run_edit_blended_diffusion", "True"]
    with pytest.raises(ValueError, match="--clip_model_path"):
        parse_args(on + ["--edit_prompt", "a photo of a man wearing glasses"])
    with pytest.raises(ValueError, match="--edit_prompt"):
        parse_args(on + ["--clip_model_path", "/nowhere"])
    with pytest.raises(ValueError, match="blended_start_t"):
        parse_args(on + ["--clip_model_path", "/nowhere", "--edit_prompt", "p", "--blended_start_t", "0"])
    with pytest.raises(ValueError, match="blended_num_aug"):
        parse_args(on + ["--clip_model_path", "/nowhere", "--edit_prompt", "p", "--blended_num_aug", "0"])
    with pytest.raises(ValueError, match="unconditional"):
        parse_args(["--sh_file_name", "x.sh", "--model_name", "stable-diffusion-v1-5", "--dataset_name", "Random",
                    "--run_edit_blended_diffusion", "True", "--clip_model_path", "/nowhere", "--edit_prompt", "p"])
    ok = parse_args(on + ["--clip_model_path", "/nowhere", "--edit_prompt", "p", "--blended_start_t", "0.3"])
    assert ok.run_edit_blended_diffusion and ok.blended_start_t == 0.3
