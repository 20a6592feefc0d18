"""GPU tests of the Segment Anything path (csrc/samenc.hip through hip.LocoSamEngine, mask_segmentation.SAM):

* tiny fixtures: the HIP image encoder against SamModel's float64 embeddings (tests/golden/sam/tiny_*.pt),
  rel-L2 <= max(4 e_ref, 2e-5), printed next to e_ref (transformers' own fp32 run against the same float64 values);
* bit-identical output on a second call and on a second engine; zeroing the position tensors moves the output;
* encoder -> torch decoder on 64 points against the float64 pred_masks and iou_scores, same bound;
* end to end on the fixture image against the mask-generation pipeline: number, order, every decided pixel, scores, files;
* one driver run: the tiny latent Stable Diffusion setup with --mask_model_path and no mask.pt from outside;
* at size: the ViT-B geometry at 1024^2 with seeded weights against the torch statement of test_sam_host.py in fp32 on the
  host, rel-L2 <= max(4 e_ref_tiny, 1e-4); the ViT-L geometry runs, is finite and is timed (unasserted)."""
import importlib.util
import json
import os
import statistics
import sys
from argparse import Namespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import mask_segmentation as ms  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(ROOT, "tests", "golden", "sam")
_spec = importlib.util.spec_from_file_location("sam_host", os.path.join(ROOT, "tests", "test_sam_host.py"))
_host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_host)
rel, bound, load_tiny = _host.rel, _host.bound, _host.load_tiny


def _engine(cfg, vis):
    from loco_edit_amd.hip import LocoSamEngine
    eng = LocoSamEngine(cfg, device=torch.device(DEV))
    eng.load_state_dict(vis)
    return eng


def _tiny(name):
    g = load_tiny(name)
    vis = ms.vision_state_dict(g["sd"], g["cfg"].vision)
    return g, vis, _engine(g["cfg"].vision, vis)


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_tiny_encoder_vs_transformers_float64(name):
    g, vis, eng = _tiny(name)
    out = eng.encode(g["pixel_values"])
    v = g["cfg"].vision
    assert tuple(out.shape) == (1, v.output_channels, v.grid, v.grid)
    e, er = rel(out, g["image_embeddings"]), g["e_ref"]["image_embeddings"]
    print(f"{name}: HIP encoder vs float64 {e:.2e}   e_ref (transformers fp32 vs float64) {er:.2e}   ratio {e / er:.2f}")
    assert e <= bound(er)


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_encoder_is_bit_identical_across_calls_and_engines(name):
    g, vis, eng = _tiny(name)
    a = eng.encode(g["pixel_values"]).clone()
    other = torch.randn_like(g["pixel_values"])
    eng.encode(other)                                         # another image in between: no state survives a call
    b = eng.encode(g["pixel_values"][0])
    assert torch.equal(a, b)
    c = _engine(g["cfg"].vision, vis).encode(g["pixel_values"])
    assert torch.equal(a, c)
    assert torch.isfinite(a).all()


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_engine_sees_the_position_tensors(name):
    g, vis, eng = _tiny(name)
    base = eng.encode(g["pixel_values"]).clone()
    zero_rel = {k: (torch.zeros_like(v) if k.endswith(("rel_pos_h", "rel_pos_w")) else v) for k, v in vis.items()}
    d_rel = rel(_engine(g["cfg"].vision, zero_rel).encode(g["pixel_values"]), base)
    zero_all = {k: (torch.zeros_like(v) if k.endswith(("rel_pos_h", "rel_pos_w", "pos_embed")) else v) for k, v in vis.items()}
    d_all = rel(_engine(g["cfg"].vision, zero_all).encode(g["pixel_values"]), base)
    print(f"{name}: zeroed rel_pos moves the embedding by {d_rel:.2e} (fixture {g['zeroed_rel_pos_change']:.2e}), "
          f"all position tensors {d_all:.2e} (fixture {g['zeroed_bias_change']:.2e})")
    assert d_rel > 1e-3 and d_all > 1e-3
    assert abs(d_rel - g["zeroed_rel_pos_change"]) <= 1e-3 * g["zeroed_rel_pos_change"]
    assert abs(d_all - g["zeroed_bias_change"]) <= 1e-3 * g["zeroed_bias_change"]


def test_engine_refuses_bad_parameters_and_shapes():
    g, vis, eng = _tiny("tiny_a")
    from loco_edit_amd.hip import LocoSamEngine
    fresh = LocoSamEngine(g["cfg"].vision, device=torch.device(DEV))
    with pytest.raises(RuntimeError, match="parameters missing"):
        fresh.load_state_dict({k: v for k, v in vis.items() if k != "neck.conv2.weight"})
    with pytest.raises(RuntimeError, match="attn.rel_pos_h has shape"):
        fresh.load_params({"layers.0.attn.rel_pos_h": torch.zeros(15, 32)})          # a global table on a windowed layer
    with pytest.raises(RuntimeError, match="unknown parameter"):
        fresh.load_params({"layers.9.attn.rel_pos_h": torch.zeros(5, 32)})
    with pytest.raises(ValueError, match="one image per call"):
        eng.encode(torch.zeros(2, 3, 64, 64))


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_encoder_then_torch_decoder_vs_transformers_float64(name):
    g, vis, eng = _tiny(name)
    head = ms.SamHead(g["cfg"], g["sd"], device=DEV)
    masks, iou = head.predict(eng.encode(g["pixel_values"]), g["points"])
    em, ei = rel(masks, g["pred_masks"]), rel(iou, g["iou_scores"])
    rm, ri = g["e_ref"]["pred_masks"], g["e_ref"]["iou_scores"]
    print(f"{name}: HIP encoder -> torch decoder vs float64: pred_masks {em:.2e} (e_ref {rm:.2e}, ratio {em / rm:.2f})   "
          f"iou_scores {ei:.2e} (e_ref {ri:.2e}, ratio {ei / ri:.2f})")
    assert em <= bound(rm) and ei <= bound(ri)


def _model_folder(tmp_path, m):
    folder = tmp_path / "sam_model"
    folder.mkdir()
    (folder / "config.json").write_text(json.dumps(m["config"]))
    torch.save(m["state_dict"], folder / "pytorch_model.bin")
    return str(folder)


def test_end_to_end_vs_the_mask_generation_pipeline(tmp_path):
    m = torch.load(os.path.join(GOLD, "end_to_end_model.pt"))
    e = torch.load(os.path.join(GOLD, "end_to_end.pt"))
    args = Namespace(mask_model_path=_model_folder(tmp_path, m), device=torch.device(DEV), filter_mask=100)
    sam = ms.SAM(args, str(tmp_path / "run"), **e["thresholds"])
    image = m["image"].numpy()
    masks, scores, boxes = sam.segment(image)
    n = e["masks"].shape[0]
    assert masks.shape[0] == n >= 3 and tuple(masks.shape[1:]) == (96, 128)
    masks, scores = masks.cpu(), scores.cpu().double()
    print("scores", [round(float(s), 5) for s in scores], "fixture", [round(float(s), 5) for s in e["scores"]])
    assert (scores - e["scores"]).abs().max().item() <= 1e-4                       # and so the same order: gaps >= 1e-3
    assert torch.equal(torch.argsort(scores, descending=True), torch.arange(n))
    for i in range(n):
        d = e["decided"][i]
        wrong = int((masks[i][d] != e["masks"][i][d]).sum())
        print(f"mask {i}: {int(masks[i].sum())} pixels, decided {float(d.float().mean()):.4f}, differing decided pixels {wrong}, "
              f"differing pixels {int((masks[i] != e['masks'][i]).sum())}")
        assert wrong == 0
    assert torch.equal(boxes.cpu().float(), e["boxes"])
    out = sam.mask_segmentation(image, resolution=32)
    assert out.dtype == torch.bool and tuple(out.shape) == (n, 32, 32)
    saved = torch.load(os.path.join(sam.log_dir, "mask.pt"))
    assert saved.dtype == torch.bool and tuple(saved.shape) == (n, 32, 32) and torch.equal(saved, out)
    ref = torch.round(torch.nn.functional.interpolate(e["masks"].unsqueeze(1).float(), [32, 32]).squeeze(1)).bool()
    assert (out != ref).sum().item() <= int((~e["decided"]).sum())
    assert os.path.exists(os.path.join(sam.log_dir, "total_mask.png"))
    big = [i for i in range(n) if int(masks[i].sum()) > 100]
    assert big and all(os.path.exists(os.path.join(sam.log_dir, f"mask_{i}.png")) for i in big)
    assert not any(os.path.exists(os.path.join(sam.log_dir, f"mask_{i}.png")) for i in range(n) if i not in big)
    print("timing of the last call (ms):", {k: round(v, 2) for k, v in sam.last_timing.items()})


def test_sd_driver_segments_its_own_sample(golden, tmp_path):
    """run_edit_null_space_projection_zt on the tiny latent setup with --mask_model_path: no mask.pt comes from outside."""
    from loco_edit_amd.config import TINY_DECODER, TINY_LATENT
    from loco_edit_amd.tloco_sd import EditStableDiffusion
    g = golden("tloco_sd_tiny")
    m = torch.load(os.path.join(GOLD, "end_to_end_model.pt"))                   # image size 64 = the decoded sample
    sd = {k: v.clone() for k, v in m["state_dict"].items()}
    # a random SAM passes the default filters nowhere: scores lifted above 0.88, logits steepened (stability -> 1)
    sd["mask_decoder.iou_prediction_head.proj_out.weight"] *= 0.05
    sd["mask_decoder.iou_prediction_head.proj_out.bias"] = sd["mask_decoder.iou_prediction_head.proj_out.bias"] * 0.05 + 0.94
    for i in range(4):
        for k in ("weight", "bias"):
            sd[f"mask_decoder.output_hypernetworks_mlps.{i}.proj_out.{k}"] *= 1000.0
    os.environ.pop("WORLD_SIZE", None)
    args = Namespace(device=torch.device(DEV), dtype=torch.float32, seed=1, unet_config=TINY_LATENT, vae_config=TINY_DECODER,
                     synthetic_weights=0, ckpt_path="", vae_ckpt_path="", max_batch=8, precision="bf16x3", dataset_name="Random",
                     for_steps=100, use_yh_custom_scheduler=True, guidance_scale=g["guidance_scale"],
                     guidance_scale_edit=g["guidance_scale_edit"],
                     prompt_emb={"for": g["for_e"], "edit": g["edit_e"], "null": g["null_e"]}, for_prompt="a man",
                     edit_prompt="a man wearing glasses", edit_t=0.7, sampling_mode=False,
                     tilda_v_score_type="null+(for-null)+(edit-null)", ablation_method="null-space-proj", mask_type="SAM",
                     vT_path="", use_sega=False, x_space_guidance_edit_step=1.0, x_space_guidance_scale=0.5,
                     x_space_guidance_num_step=16, result_folder=str(tmp_path / "run"), filter_mask=100,
                     mask_model_path=_model_folder(tmp_path, {"config": m["config"], "state_dict": sd}))
    ed = EditStableDiffusion(args)
    mpath = os.path.join(ed.result_folder, "mask", "mask.pt")
    assert not os.path.exists(mpath)
    ed._set_edit_prompt(None)
    torch.manual_seed(5)
    assert ed._prepare(0) is not None                                           # samples, decodes, segments, caches
    masks = torch.load(mpath)
    assert masks.dtype == torch.bool and masks.dim() == 3 and tuple(masks.shape[1:]) == (64, 64) and masks.shape[0] >= 1
    assert os.path.exists(os.path.join(ed.result_folder, "original.png"))
    assert os.path.exists(os.path.join(ed.result_folder, "mask", "total_mask.png"))
    area = masks.flatten(1).float().mean(1)
    print("driver masks:", masks.shape[0], "areas", [round(float(a), 3) for a in area])
    ok = [i for i in range(masks.shape[0]) if 0.02 < float(area[i]) < 0.98]
    assert ok, "no mask that leaves both a region and its complement"
    stamp = os.path.getmtime(mpath)
    torch.manual_seed(5)
    lat, x0 = ed.run_edit_null_space_projection_zt(op="mid", block_idx=0, vis_num=2, mask_index=ok[0], vis_num_pc=1, pca_rank=1,
                                                   null_space_projection=True, pca_rank_null=2)
    assert x0.dtype == torch.uint8 and tuple(x0.shape) == (5, 64, 64, 3) and tuple(lat.shape) == (5, 4, 16, 16)
    assert os.path.getmtime(mpath) == stamp                                     # the cached mask.pt won
    bdir = os.path.join(ed.result_folder, "basis", f"local_basis-0.7T-pca-rank-1-select-mask{ok[0]}")
    assert tuple(torch.load(os.path.join(bdir, "u-modify.pt")).shape) == (int(masks[ok[0]].sum()) * 3, 1)


def _timed(eng, pv, runs=3):
    eng.encode(pv)                                            # warm
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = eng.encode(pv)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return out, statistics.median(ts)


def test_vit_b_geometry_at_size_vs_host_statement():
    cfg = ms.VIT_B
    vis = _host.synthetic_vision_sd(cfg, seed=11)
    pv = torch.randn(3, 1024, 1024, generator=torch.Generator().manual_seed(12))
    eng = _engine(cfg, vis)
    out, ms_med = _timed(eng, pv)
    assert tuple(out.shape) == (1, 256, 64, 64) and torch.isfinite(out).all()
    with torch.no_grad():
        ref = _host.restated_sam_encoder(vis, cfg, pv)                         # fp32 on the host
    e = rel(out, ref)
    e_ref_tiny = max(load_tiny(n)["e_ref"]["image_embeddings"] for n in ("tiny_a", "tiny_b"))
    print(f"ViT-B geometry at 1024^2: HIP vs host fp32 statement {e:.2e}   bound {bound(e_ref_tiny, 1e-4):.1e}   "
          f"encode {ms_med:.1f} ms (median of 3 warm runs)")
    assert e <= bound(e_ref_tiny, 1e-4)


def test_vit_l_geometry_runs_and_is_timed():
    cfg = ms.VIT_L
    vis = _host.synthetic_vision_sd(cfg, seed=13)
    pv = torch.randn(3, 1024, 1024, generator=torch.Generator().manual_seed(14))
    eng = _engine(cfg, vis)
    del vis
    out, ms_med = _timed(eng, pv)
    assert tuple(out.shape) == (1, 256, 64, 64) and torch.isfinite(out).all()
    eng.profile(True)
    eng.encode(pv)
    split = eng.profile_read()
    eng.profile(False)
    print(f"ViT-L geometry at 1024^2: encode {ms_med:.1f} ms (median of 3 warm runs); split of a profiled run (ms): "
          + ", ".join(f"{k} {v:.1f}" for k, v in split.items()))
    assert all(v >= 0 for v in split.values()) and split["gemm"] > 0 and split["window_attn"] > 0 and split["global_attn"] > 0
