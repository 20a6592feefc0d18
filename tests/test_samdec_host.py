"""Host tests of the Segment Anything head's HIP path (loco_edit_amd/mask_segmentation.py: head_param_shapes,
head_state_dict, prompt_coords, the scorer branch of MaskGenerator.filter_batch; define_argparser's --mask_head):

* head_param_shapes names the tensors of the tiny fixtures and of the end-to-end model with their shapes; head_state_dict
  rejects a transposed and a missing tensor;
* --mask_head parses and defaults to torch;
* prompt_coords equals what SamHead.embed_points feeds the random-Fourier features;
* MaskGenerator.filter_batch with a scorer that computes counts, boxes and masks from MaskGenerator.upsample itself returns
  what the path without a scorer returns (the branch's bookkeeping, without a GPU)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import mask_segmentation as ms  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "sam")


def _fixture(name):
    g = torch.load(os.path.join(GOLD, f"{name}.pt"))
    return ms.config_from_dict(g["config"]), ms.normalize_sam_state_dict(g["state_dict"])


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b", "end_to_end_model"])
def test_head_param_shapes_name_the_fixture_tensors(name):
    cfg, sd = _fixture(name)
    want = ms.head_param_shapes(cfg)
    assert set(want) == set(ms.head_param_names(cfg)) - {"prompt_encoder.point_embed.0.weight"}
    for k, shp in want.items():
        assert tuple(sd[k].shape) == shp, k
    got = ms.head_state_dict(sd, cfg)
    assert list(got) == list(want) and all(got[k] is sd[k] for k in want)
    # every tensor of the fixture's head is either named or one of the three the head never reads
    rest = {k for k in sd if k.startswith(("prompt_encoder.", "mask_decoder.", "shared_image_embedding."))} - set(want)
    assert rest <= {"prompt_encoder.point_embed.0.weight", "prompt_encoder.shared_embedding.positional_embedding",
                    "prompt_encoder.point_embed.2.weight", "prompt_encoder.point_embed.3.weight"}, rest


def test_head_state_dict_rejects_transposed_and_missing_tensors():
    cfg, sd = _fixture("tiny_a")
    k = "mask_decoder.transformer.layers.1.cross_attn_token_to_image.q_proj.weight"
    assert sd[k].shape[0] != sd[k].shape[1]
    with pytest.raises(ValueError, match="q_proj.weight: shape .* expected"):
        ms.head_state_dict({**sd, k: sd[k].t()}, cfg)
    k = "mask_decoder.upscale_conv2.weight"
    with pytest.raises(ValueError, match="upscale_conv2.weight: shape"):
        ms.head_state_dict({**sd, k: sd[k].transpose(0, 1)}, cfg)
    with pytest.raises(ValueError, match="missing keys of the SAM prompt encoder / mask decoder.*iou_token"):
        ms.head_state_dict({a: v for a, v in sd.items() if a != "mask_decoder.iou_token.weight"}, cfg)


def test_sam_geometry_counts_four_million_parameters():
    n = sum(torch.Size(s).numel() for s in ms.head_param_shapes(ms.SamConfig()).values())
    assert 4.0e6 < n < 4.1e6


def test_mask_head_flag_parses_and_defaults_to_torch():
    from loco_edit_amd.define_argparser import build_parser
    p = build_parser()
    assert p.parse_args([]).mask_head == "torch"
    assert p.parse_args(["--mask_head", "hip"]).mask_head == "hip"
    with pytest.raises(SystemExit):
        p.parse_args(["--mask_head", "triton"])


def test_prompt_coords_equal_what_embed_points_feeds_the_features(monkeypatch):
    cfg, sd = _fixture("tiny_b")
    head = ms.SamHead(cfg, sd)
    fed = []
    real = head._pe

    def spy(coords01):
        fed.append((2 * coords01 - 1).to(head.dtype))          # the first line of SamHead._pe
        return real(coords01)
    monkeypatch.setattr(head, "_pe", spy)
    pts = ms.MaskGenerator().grid_points((75, 100), cfg.vision.image_size)[::7]
    pts = torch.cat([pts, torch.tensor([[0.0, 0.0], [111.0, 83.5]], dtype=torch.float64)])
    head.embed_points(pts)
    (got,) = fed
    assert got.dtype == torch.float32 and tuple(got.shape) == (pts.shape[0], 2, 2)
    mine = ms.prompt_coords(pts, cfg.vision.image_size)
    assert mine.dtype == torch.float32 and torch.equal(mine, got[:, 0])
    assert float(mine.min()) > -1 and float(mine.max()) < 1


class _TorchScorer:
    """counts / boxes / masks from MaskGenerator.upsample itself: what loco_samdec_score / _binarize return, up to rounding."""

    def score(self, low, size, reshaped, image_size, thr, offset):
        m = ms.MaskGenerator.upsample(low[:, None], size, reshaped, image_size)[:, 0]
        counts = torch.stack([(m > thr + offset).flatten(1).sum(1), (m > thr - offset).flatten(1).sum(1)], dim=1).to(torch.int32)
        return counts, ms.mask_to_box(m > thr).to(torch.int32)

    def binarize(self, low, rows, size, reshaped, image_size, thr):
        return ms.MaskGenerator.upsample(low[rows][:, None], size, reshaped, image_size)[:, 0] > thr


def test_filter_batch_with_a_scorer_returns_what_the_torch_path_returns():
    g = torch.load(os.path.join(GOLD, "generator.pt"))
    gen = ms.MaskGenerator(**g["thresholds"])
    a, b = [], []
    for grp in g["groups"]:
        args = (grp["low_res"].float(), grp["scores"], grp["original_size"], grp["reshaped_size"], g["image_size"])
        a.append(gen.filter_batch(*args, crop_box=grp["crop_box"]))
        b.append(gen.filter_batch(*args, crop_box=grp["crop_box"], scorer=_TorchScorer()))
        assert b[-1][0].shape[0] == grp["kept"]
        for x, y in zip(a[-1], b[-1]):
            assert x.dtype == y.dtype and torch.equal(x, y)
    for x, y in zip(gen.finish(a), gen.finish(b)):
        assert torch.equal(x, y)
