"""Host tests of the Segment Anything path (loco_edit_amd/mask_segmentation.py) against the fixtures tests/make_golden_sam.py
wrote from the installed `transformers` (tests/golden/sam/):

* `restated_sam_encoder` below -- the image encoder stated in torch as csrc/samenc.hip computes it -- and the torch prompt
  encoder / mask decoder, in fp32 against the float64 outputs of SamModel: rel-L2 <= max(4 e_ref, 2e-5), e_ref being
  transformers' own fp32 run against the same float64 values (2e-5: the bar of the tiny T5 test);
* the automatic mask generator on the synthetic decoder outputs: the same masks, order, scores and boxes as
  SamImageProcessor's filter_masks / post_process_for_mask_generation;
* the preprocessing against recorded pixel_values;
* the loader: key normalisation round trip, a relative position table of the wrong length and missing parameters refused;
* the flag parses, and with it empty the three drivers raise the FileNotFoundError they raised before."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import mask_segmentation as ms  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "sam")


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


def bound(e_ref, floor=2e-5):
    return max(4 * e_ref, floor)


def load_tiny(name):
    g = torch.load(os.path.join(GOLD, f"{name}.pt"))
    parts, k = [], 0
    while os.path.exists(os.path.join(GOLD, f"{name}_masks_{k}.pt")):
        p = torch.load(os.path.join(GOLD, f"{name}_masks_{k}.pt"))
        assert p["first_point"] == sum(x.shape[0] for x in parts)
        parts.append(p["pred_masks"])
        k += 1
    g["pred_masks"] = torch.cat(parts)
    assert list(g["pred_masks"].shape) == g["pred_masks_shape"]
    g["cfg"] = ms.config_from_dict(g["config"])
    g["sd"] = ms.normalize_sam_state_dict(g["state_dict"])
    return g


def restated_sam_encoder(sd, cfg, pixel_values, dtype=torch.float32):
    """SamVisionEncoder as the HIP engine computes it: `sd` in vision naming (mask_segmentation.vision_state_dict),
    pixel_values [3, S, S] -> [1, C_out, G, G]."""
    P = {k: v.to(dtype=dtype, device=pixel_values.device) for k, v in sd.items()}
    D, G, ws, H, hd = cfg.hidden_size, cfg.grid, cfg.window_size, cfg.num_attention_heads, cfg.head_dim
    x = F.conv2d(pixel_values.to(dtype)[None], P["patch_embed.projection.weight"], P["patch_embed.projection.bias"], stride=cfg.patch_size)
    x = x.permute(0, 2, 3, 1) + P["pos_embed"]                                       # [1, G, G, D]
    for i in range(cfg.num_hidden_layers):
        p = f"layers.{i}."
        glob = i in cfg.global_attn_indexes
        size = G if glob else ws
        y = F.layer_norm(x, (D,), P[p + "layer_norm1.weight"], P[p + "layer_norm1.bias"], cfg.layer_norm_eps)
        if not glob:                                                                  # zero-pad the NORMALISED map, partition
            Gp = (G + ws - 1) // ws * ws
            y = F.pad(y, (0, 0, 0, Gp - G, 0, Gp - G))
            n = Gp // ws
            y = y.reshape(1, n, ws, n, ws, D).permute(0, 1, 3, 2, 4, 5).reshape(n * n, ws, ws, D)
        B = y.shape[0]
        qkv = F.linear(y, P[p + "attn.qkv.weight"], P[p + "attn.qkv.bias"]).reshape(B, size * size, 3, H, hd).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]                                              # [B, H, T, hd]
        idx = torch.arange(size)[:, None] - torch.arange(size)[None, :] + size - 1    # [q coordinate, k coordinate]
        Rh, Rw = P[p + "attn.rel_pos_h"][idx], P[p + "attn.rel_pos_w"][idx]          # [size, size, hd]
        q5 = q.reshape(B, H, size, size, hd)
        rel_h = torch.einsum("bnhwc,hkc->bnhwk", q5, Rh)
        rel_w = torch.einsum("bnhwc,wkc->bnhwk", q5, Rw)
        s = (q * hd ** -0.5) @ k.transpose(-2, -1)
        s = s + (rel_h[..., :, None] + rel_w[..., None, :]).reshape(B, H, size * size, size * size)
        o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, size, size, D)
        o = F.linear(o, P[p + "attn.proj.weight"], P[p + "attn.proj.bias"])
        if not glob:
            o = o.reshape(1, n, n, ws, ws, D).permute(0, 1, 3, 2, 4, 5).reshape(1, Gp, Gp, D)[:, :G, :G]
        x = x + o
        y = F.layer_norm(x, (D,), P[p + "layer_norm2.weight"], P[p + "layer_norm2.bias"], cfg.layer_norm_eps)
        x = x + F.linear(F.gelu(F.linear(y, P[p + "mlp.lin1.weight"], P[p + "mlp.lin1.bias"])), P[p + "mlp.lin2.weight"], P[p + "mlp.lin2.bias"])
    x = F.conv2d(x.permute(0, 3, 1, 2), P["neck.conv1.weight"])
    x = ms._channel_ln(x, P["neck.layer_norm1.weight"], P["neck.layer_norm1.bias"])
    x = F.conv2d(x, P["neck.conv2.weight"], padding=1)
    return ms._channel_ln(x, P["neck.layer_norm2.weight"], P["neck.layer_norm2.bias"])


def synthetic_vision_sd(cfg, seed, device="cpu"):
    """Seeded weights of a geometry (the at-size GPU tests): fan-in scaled matrices, every bias and table drawn."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    sd = {}
    for k, shp in ms.vision_param_shapes(cfg).items():
        if "layer_norm" in k:
            t = (1.0 if k.endswith("weight") else 0.0) + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith(("rel_pos_h", "rel_pos_w", "pos_embed")):
            t = 0.5 * torch.randn(shp, generator=g)
        elif k.endswith(".bias"):
            t = 0.1 * torch.randn(shp, generator=g)
        else:
            fan_in = 1
            for d in shp[1:]:
                fan_in *= d
            t = torch.randn(shp, generator=g) / fan_in ** 0.5
        sd[k] = t.to(device)
    return sd


# --------------------------------------------------------------------------------------------------------- numerics
@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_restated_encoder_vs_transformers_float64(name):
    g = load_tiny(name)
    vis = ms.vision_state_dict(g["sd"], g["cfg"].vision)
    out = restated_sam_encoder(vis, g["cfg"].vision, g["pixel_values"][0])
    e, er = rel(out, g["image_embeddings"]), g["e_ref"]["image_embeddings"]
    print(f"{name}: restated fp32 encoder vs float64 {e:.2e}   e_ref {er:.2e}   ratio {e / er:.2f}")
    assert e <= bound(er)
    # the same statement in float64 is transformers' float64 run to rounding: the fixture and the statement agree
    e64 = rel(restated_sam_encoder(vis, g["cfg"].vision, g["pixel_values"][0], torch.float64), g["image_embeddings"])
    print(f"{name}: restated float64 encoder vs float64 {e64:.2e}")
    assert e64 <= 1e-12
    assert g["zeroed_bias_change"] > 1e-3 and g["zeroed_rel_pos_change"] > 1e-3


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_prompt_encoder_and_decoder_vs_transformers_float64(name):
    g = load_tiny(name)
    head = ms.SamHead(g["cfg"], g["sd"])
    masks, iou = head.predict(g["image_embeddings"].float(), g["points"])
    assert tuple(masks.shape) == tuple(g["pred_masks"].shape) and tuple(iou.shape) == (64, 3)
    em, ei = rel(masks, g["pred_masks"]), rel(iou, g["iou_scores"])
    rm, ri = g["e_ref"]["pred_masks_decoder_only"], g["e_ref"]["iou_scores_decoder_only"]
    print(f"{name}: torch decoder fp32 vs float64: pred_masks {em:.2e} (e_ref {rm:.2e}, ratio {em / rm:.2f})   "
          f"iou_scores {ei:.2e} (e_ref {ri:.2e}, ratio {ei / ri:.2f})")
    assert em <= bound(rm) and ei <= bound(ri)
    h64 = ms.SamHead(g["cfg"], g["sd"], dtype=torch.float64)
    m64, i64 = h64.predict(g["image_embeddings"], g["points"])
    assert rel(m64, g["pred_masks"]) <= 1e-11 and rel(i64, g["iou_scores"]) <= 1e-11


# -------------------------------------------------------------------------------------------------------- generator
def test_mask_generator_on_synthetic_decoder_outputs():
    g = torch.load(os.path.join(GOLD, "generator.pt"))
    assert g["margins"]["thresholds"] >= 1e-3 and g["margins"]["nms_iou"] >= 1e-3
    gen = ms.MaskGenerator(**g["thresholds"])
    batches = []
    for grp in g["groups"]:
        m, s, b = gen.filter_batch(grp["low_res"].float(), grp["scores"], grp["original_size"], grp["reshaped_size"], g["image_size"],
                                   crop_box=grp["crop_box"])
        assert m.shape[0] == grp["kept"]
        batches.append((m, s, b))
    masks, scores, boxes = gen.finish(batches)
    exp = g["expected"]
    assert masks.shape[0] == exp["masks"].shape[0] < exp["candidates"]
    assert torch.equal(masks, exp["masks"])
    assert torch.equal(scores, exp["scores"])
    assert torch.equal(boxes.float(), exp["boxes"].float())


def test_grid_points_match_the_pipeline():
    gen = ms.MaskGenerator()
    pts = gen.grid_points((96, 128), 64)
    assert tuple(pts.shape) == (1024, 2) and pts.dtype == torch.float64
    # 32 x 32 cell centres of the 96 x 128 image, scaled to the 48 x 64 resized frame: x fastest
    assert pts[0].tolist() == [128 / 64 * (64 / 128), 96 / 64 * (48 / 96)]
    assert torch.allclose(pts[33], torch.tensor([3.0, 2.25], dtype=torch.float64))


def test_greedy_nms_order_and_threshold():
    boxes = torch.tensor([[0, 0, 10, 10], [0, 0, 10, 9], [20, 20, 30, 30], [0, 0, 10, 5]], dtype=torch.float32)
    scores = torch.tensor([0.5, 0.9, 0.7, 0.6])
    assert ms.greedy_nms(boxes, scores, 0.7).tolist() == [1, 2, 3]       # box 0 (IoU 0.9 with box 1) is suppressed
    assert ms.greedy_nms(boxes, scores, 0.95).tolist() == [1, 2, 3, 0]


# ---------------------------------------------------------------------------------------------------- preprocessing
def test_preprocess_matches_the_image_processor():
    cases = torch.load(os.path.join(GOLD, "preprocess.pt"))
    assert len(cases) >= 4
    for c in cases:
        pv, orig, resh = ms.preprocess(c["image"].numpy(), c["image_size"])
        assert list(orig) == c["original_size"] and list(resh) == c["reshaped_size"]
        assert pv.dtype == torch.float32 and tuple(pv.shape) == tuple(c["pixel_values"].shape)
        assert torch.allclose(pv, c["pixel_values"], rtol=0, atol=2e-6), (pv - c["pixel_values"]).abs().max()
        assert torch.count_nonzero(pv[:, resh[0]:]) == 0 and torch.count_nonzero(pv[:, :, resh[1]:]) == 0


# ----------------------------------------------------------------------------------------------------------- loader
def test_loader_round_trips_keys(tmp_path):
    g = load_tiny("tiny_a")
    raw = g["state_dict"]
    cfg, sd = ms.load_sam(dict(raw))
    assert cfg == ms.infer_config(sd)
    assert cfg.vision == g["cfg"].vision                                  # the geometry read off the tensors alone
    assert not any(k.startswith("prompt_encoder.mask_embed.") for k in sd)
    assert set(sd) == {k for k in raw if not k.startswith("prompt_encoder.mask_embed.")} | {"prompt_encoder.shared_embedding.positional_embedding"}
    # wrapper prefixes, a nested state_dict, one of the two tied names only
    wrapped = {"state_dict": {"model." + k: v for k, v in raw.items() if k != "prompt_encoder.shared_embedding.positional_embedding"}}
    cfg2, sd2 = ms.load_sam(wrapped)
    assert cfg2 == cfg and set(sd2) == set(sd) and all(torch.equal(sd2[k], sd[k]) for k in sd)
    # a folder with config.json + pytorch_model.bin, and a bare file
    import json
    folder = tmp_path / "sam"
    folder.mkdir()
    (folder / "config.json").write_text(json.dumps(g["config"]))
    torch.save(raw, folder / "pytorch_model.bin")
    cfg3, sd3 = ms.load_sam(str(folder))
    assert cfg3 == g["cfg"] and set(sd3) == set(sd)
    cfg4, _ = ms.load_sam(str(folder / "pytorch_model.bin"))
    assert cfg4.vision == cfg.vision
    with pytest.raises(FileNotFoundError):
        ms.load_sam(str(tmp_path / "nowhere"))
    with pytest.raises(ValueError, match="foreign key"):
        ms.load_sam({**raw, "text_model.x": torch.zeros(1)})


def test_loader_refuses_wrong_table_length_and_missing_parameters():
    g = load_tiny("tiny_a")
    cfg = g["cfg"]
    bad = dict(g["sd"])
    k = "vision_encoder.layers.0.attn.rel_pos_h"                         # a windowed layer: 2 * 3 - 1 = 5 rows
    assert bad[k].shape[0] == 5
    bad[k] = torch.zeros(2 * cfg.vision.grid - 1, cfg.vision.head_dim)    # transformers would interpolate this one
    with pytest.raises(ValueError, match="relative position table of 15 rows, the layer needs 5"):
        ms.vision_state_dict(bad, cfg.vision)
    miss = {k: v for k, v in g["sd"].items() if k != "vision_encoder.layers.2.mlp.lin2.bias"}
    with pytest.raises(ValueError, match="missing keys of the SAM image encoder.*layers.2.mlp.lin2.bias"):
        ms.vision_state_dict(miss, cfg.vision)
    raw = {k: v for k, v in g["state_dict"].items() if k != "mask_decoder.iou_prediction_head.proj_out.bias"}
    with pytest.raises(ValueError, match="missing keys of the SAM prompt encoder / mask decoder"):
        ms.load_sam({**raw})


def test_geometries():
    for cfg, (D, depth, heads, hd) in ((ms.VIT_B, (768, 12, 12, 64)), (ms.VIT_L, (1024, 24, 16, 64)), (ms.VIT_H, (1280, 32, 16, 80))):
        assert (cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.head_dim) == (D, depth, heads, hd)
        assert cfg.grid == 64 and len(cfg.global_attn_indexes) == 4
    n = sum(torch.Size(s).numel() for s in ms.vision_param_shapes(ms.VIT_L).values())
    assert 300e6 < n < 315e6                                              # the 308 M parameters of ViT-L


# ------------------------------------------------------------------------------------------------- flag and drivers
def test_flag_parses():
    from loco_edit_amd.define_argparser import build_parser
    p = build_parser()
    assert p.parse_args([]).mask_model_path == ""
    a = p.parse_args(["--mask_model_path", "/models/sam-vit-large"])
    assert a.mask_model_path == "/models/sam-vit-large" and a.mask_model_name == "facebook/sam-vit-large"


class _Solo:
    active, is_main = False, True

    def agree(self, v):
        return v


def _driver_stub(tmp_path, **kw):
    args = SimpleNamespace(mask_model_path="", sampling_mode=False, mask_index=0, sample_idx=0)
    return SimpleNamespace(args=args, result_folder=str(tmp_path), sharder=_Solo(), _exists=lambda p: bool(p) and os.path.exists(p),
                           c_in=3, image_size=8, dtype=torch.float32, device="cpu", sampling_mode=False, **kw)


def test_drivers_without_the_flag_raise_as_before(tmp_path):
    from loco_edit_amd.edit import EditUncondDiffusion
    from loco_edit_amd.tloco import EditDeepFloydIF
    from loco_edit_amd.tloco_sd import EditStableDiffusion
    for name in ("Random", "FFHQ"):
        with pytest.raises(FileNotFoundError, match=r"mask/mask\.pt missing: SAM mask generation is outside the hot path"):
            EditUncondDiffusion._get_xT_and_mask(_driver_stub(tmp_path, dataset_name=name), 0, True)
    stub = _driver_stub(tmp_path)
    with pytest.raises(FileNotFoundError, match=r"mask/mask\.pt missing: stage-II super-resolution \+ SAM"):
        EditDeepFloydIF._masks(stub)
    with pytest.raises(FileNotFoundError, match=r"mask/mask\.pt missing: stage-II super-resolution \+ SAM"):
        EditDeepFloydIF._masks(stub, lambda: None, 8)                    # an image at hand changes nothing without the flag
    assert EditStableDiffusion._masks is EditDeepFloydIF._masks
    # a cached mask.pt still wins, flag or not
    os.makedirs(tmp_path / "mask")
    torch.save(torch.ones(2, 8, 8, dtype=torch.bool), tmp_path / "mask" / "mask.pt")
    stub.args.mask_model_path = "/nowhere"
    stub._load = torch.load
    assert tuple(EditDeepFloydIF._masks(stub, lambda: 1 / 0, 8).shape) == (2, 8, 8)
    xT, mask = EditUncondDiffusion._get_xT_and_mask(_driver_stub(tmp_path, dataset_name="Random"), 0, True)
    assert tuple(mask.shape) == (3, 8, 8)
