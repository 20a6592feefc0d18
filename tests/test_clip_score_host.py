"""Host tests of the CLIP scores (loco_edit_amd/clip_score.py, eval.py, define_argparser.py); no GPU.

Also here, for the GPU tests and the fixture generator: ``smooth_noise_image`` and ``restated_preprocess``, the float64
restatement of CLIPImageProcessor's steps with torch's antialiased bicubic ``interpolate`` in place of PIL's resize (the
yardstick of the device preprocessing, csrc/clipvis.hip)."""
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import clip_score as cs  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "clip_vision")


def smooth_noise_image(H, W, seed, noise=0.15):
    """uint8 [H, W, 3]: a few low-frequency waves per channel plus uniform noise of the given amplitude (of the full range)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(H, dtype=torch.float64)[:, None] / H
    x = torch.arange(W, dtype=torch.float64)[None, :] / W
    chans = []
    for _ in range(3):
        a = torch.rand(6, generator=g, dtype=torch.float64)
        chans.append(0.5 + 0.2 * torch.sin(6.283 * (a[0] * 2 * x + a[1] * 2 * y + a[2])) + 0.1 * torch.cos(6.283 * (a[3] * 3 * x - a[4] * 3 * y + a[5])))
    img = torch.stack(chans, dim=-1) + noise * (2 * torch.rand(H, W, 3, generator=g, dtype=torch.float64) - 1)
    return (img.clamp(0, 1) * 255).round().to(torch.uint8)


def restated_preprocess(frames, S, mean=cs.CLIP_MEAN, std=cs.CLIP_STD, shift=(0, 0), normalize=True):
    """uint8 [n, H, W, 3] -> float64 [n, 3, S, S]: shortest edge -> S (other edge int(long S / short)) by bicubic interpolation
    with antialiasing, centre crop at (size - S) // 2 (shift: the resized image displaced by so many pixels first, for the
    displaced-crop check), / 255, (v - mean) / std;
    normalize=False stops after the crop (grey levels)."""
    x = torch.as_tensor(frames).permute(0, 3, 1, 2).to(torch.float64)
    H, W = x.shape[-2:]
    Hn, Wn = cs.resized_shape(H, W, S)
    if (Hn, Wn) != (H, W):
        x = F.interpolate(x, size=(Hn, Wn), mode="bicubic", antialias=True, align_corners=False)
    if tuple(shift) != (0, 0):
        x = torch.roll(x, tuple(shift), dims=(2, 3))
    top, left = (Hn - S) // 2, (Wn - S) // 2
    x = x[:, :, top:top + S, left:left + S]
    if not normalize:
        return x
    m, s = torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1), torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    return (x / 255 - m) / s


def _processor(S):
    import transformers
    return transformers.CLIPImageProcessor(size={"shortest_edge": S}, crop_size={"height": S, "width": S})


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("H,W", [(64, 64), (256, 256), (96, 80), (80, 96)])
def test_preprocess_restatement_vs_clip_image_processor(H, W):
    """The float restatement against CLIPImageProcessor (PIL backend), S = 224: rel-L2 of the normalised pixel values <= 0.02,
    about 3 x what PIL's rounding to uint8 after each pass costs (measured on these images: 0.0085 at 64^2, 0.0088 at 256^2,
    0.0084 at 96 x 80, 0.0079 at 80 x 96).  A crop displaced by one pixel must miss that bar: on these images (noise amplitude
    0.15) the resized image moved by one pixel down / right under the crop gives rel-L2 0.191 / 0.188 (64^2), 0.475 / 0.477
    (256^2), 0.232 / 0.230 (96 x 80) and 0.218 / 0.218 (80 x 96), checked when the test was written and asserted since.  The
    PIL mode of clip_score equals the processor exactly."""
    S = 224
    img = smooth_noise_image(H, W, seed=H * 1000 + W)
    want = _processor(S)(images=[img.numpy()], return_tensors="pt")["pixel_values"]
    got = restated_preprocess(img[None], S)
    err = _rel(got, want)
    # the resized image displaced by one pixel under the crop, compared away from the border the roll wraps round
    moved = [_rel(restated_preprocess(img[None], S, shift=sh)[..., 8:-8, 8:-8], want[..., 8:-8, 8:-8]) for sh in ((1, 0), (0, 1))]
    print(f"{H}x{W}: restatement vs CLIPImageProcessor rel-L2 {err:.4f}; displaced by one pixel {['%.4f' % m for m in moved]}")
    assert err <= 0.02
    assert min(moved) > 0.02
    assert torch.equal(cs.preprocess_pil(img[None], cs.ClipVisionConfig(image_size=S)), want)


def test_preprocess_without_resize_agrees():
    S = 224
    img = smooth_noise_image(300, 224, seed=7)
    want = _processor(S)(images=[img.numpy()], return_tensors="pt")["pixel_values"]
    err = _rel(restated_preprocess(img[None], S), want)
    print(f"300x224 (no resize): rel-L2 {err:.2e}")
    assert err <= 1e-6
    assert torch.equal(cs.preprocess_pil(img[None], cs.ClipVisionConfig(image_size=S)), want)


def test_loader_splits_a_clip_model_state_dict():
    g = torch.load(os.path.join(GOLD, "tiny_a.pt"))
    sd = {k: v.float() for k, v in g["state_dict"].items()}
    vision, text, vproj, tproj = cs.split_clip_state_dict(sd)
    back = {"vision_model." + k: v for k, v in vision.items()}
    back.update(text)
    back["visual_projection.weight"], back["text_projection.weight"] = vproj, tproj
    dropped = set(sd) - set(back)
    assert dropped <= {"logit_scale", "text_model.embeddings.position_ids", "vision_model.embeddings.position_ids"}
    assert set(back) <= set(sd) and all(back[k] is sd[k] for k in back)
    assert len(vision) + len(text) + 2 == len(back)                    # no key in two parts
    vcfg = cs.infer_vision_config(vision, vproj, g["config"]["vision_config"])
    assert (vcfg.image_size, vcfg.patch_size, vcfg.width, vcfg.heads, vcfg.layers, vcfg.projection_dim) == (32, 8, 64, 4, 2, 24)
    cs.check_vision_state_dict(dict(vision, **{"visual_projection.weight": vproj}), vcfg)
    assert set(cs.vision_param_shapes(vcfg)) == set(vision) | {"visual_projection.weight"}
    # the text tower goes through the text encoder's own normaliser, text_projection taken before it would be dropped
    from loco_edit_amd import text_encoder as te
    tsd = te.normalize_text_state_dict(text)
    te.check_text_state_dict(tsd, te.infer_text_config(tsd, g["config"]["text_config"]))
    with pytest.raises(ValueError, match="missing visual_projection.weight"):
        cs.split_clip_state_dict({k: v for k, v in sd.items() if k != "visual_projection.weight"})
    with pytest.raises(ValueError, match="missing text_projection.weight"):
        cs.split_clip_state_dict({k: v for k, v in sd.items() if k != "text_projection.weight"})
    with pytest.raises(ValueError, match="OpenCLIP"):
        cs.split_clip_state_dict({"visual.transformer.resblocks.0.attn.in_proj_weight": torch.zeros(3, 3), "visual.conv1.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="foreign"):
        cs.split_clip_state_dict(dict(sd, **{"lm_head.weight": torch.zeros(1)}))
    with pytest.raises(ValueError, match="shape"):
        cs.check_vision_state_dict(dict(vision, **{"visual_projection.weight": vproj[:, :3]}), vcfg)


def test_eval_clip_without_a_model_raises(tmp_path):
    from loco_edit_amd import eval as ev
    for metric in ("clip", "clip_dir"):
        with pytest.raises(NotImplementedError, match="clip_model_path"):
            ev.main(["--eval_metric", metric, "--folder_preds", str(tmp_path), "--folder_original", str(tmp_path),
                     "--for_prompt", "a", "--edit_prompt", "b"])
    assert set(ev.METRICS) == {"ssim", "mmse", "lpips"}               # the existing metrics are untouched


def test_argparser_takes_clip_model_path():
    from loco_edit_amd.define_argparser import parse_args
    scripts = json.load(open(os.path.join(ROOT, "tests", "golden", "script_args.json")))
    assert len(scripts) == 12
    for name, argv in scripts.items():
        a = parse_args(argv)
        assert a.clip_model_path == "" and a.clip_preprocess == "device", name
        b = parse_args(argv + ["--clip_model_path", "/some/clip"])
        assert b.clip_model_path == "/some/clip"
        da, db = dict(vars(a)), dict(vars(b))
        da.pop("clip_model_path"); db.pop("clip_model_path")
        assert {k: str(v) for k, v in da.items()} == {k: str(v) for k, v in db.items()}, name


class _StubScorer(cs.ClipScorer):
    """The metric algebra on given embeddings: frame k's `image` is its embedding, a prompt's `text` its embedding."""

    def __init__(self, img, text):
        self._img, self._text = img, text

    def image_embeds(self, frames):
        return self._img

    def text_embeds(self, prompts):
        return torch.stack([self._text[p] for p in prompts])


def test_metric_algebra_on_a_stub_embedder():
    g = torch.Generator().manual_seed(0)
    e0, d = torch.randn(16, generator=g), torch.randn(16, generator=g)
    text = {"src": torch.randn(16, generator=g)}
    text["edit"] = text["src"] + 0.7 * d                               # text difference parallel to d
    img = torch.stack([e0 - 2.0 * d, e0, e0 + 0.5 * d, e0 + 3.0 * d])    # a walk along d, alpha = -2, 0, 0.5, 3
    recs = _StubScorer(img, text).score(None, 1, "src", "edit")
    assert len(recs) == 4
    assert recs[1]["directional"] is None and abs(recs[1]["image_sim"] - 1) < 1e-12
    assert abs(recs[2]["directional"] - 1) < 1e-6 and abs(recs[3]["directional"] - 1) < 1e-6
    assert abs(recs[0]["directional"] + 1) < 1e-6                       # the sign flips with the walk's sign
    for k, r in enumerate(recs):
        assert abs(r["clip_for"] - cs.cosine(img[k], text["src"])) < 1e-12
        assert abs(r["clip_edit"] - cs.cosine(img[k], text["edit"])) < 1e-12
        assert abs(r["image_sim"] - cs.cosine(img[k], img[1])) < 1e-12
    # an orthogonal image move scores 0
    o = torch.randn(16, generator=g)
    o = o - (o @ d) / (d @ d) * d
    r = _StubScorer(torch.stack([e0, e0 + o]), text).score(None, 0, "src", "edit")
    assert abs(r[1]["directional"]) < 1e-6
    # None cases: an empty prompt
    for fp, ep in (("", "edit"), ("src", ""), ("", "")):
        recs = _StubScorer(img, text).score(None, 1, fp, ep)
        assert all(r["directional"] is None for r in recs)
        assert (recs[0]["clip_for"] is None) == (fp == "") and (recs[0]["clip_edit"] is None) == (ep == "")
        assert abs(recs[0]["image_sim"] - cs.cosine(img[0], img[1])) < 1e-12
    with pytest.raises(ValueError, match="original_index"):
        _StubScorer(img, text).score(None, 4, "src", "edit")
