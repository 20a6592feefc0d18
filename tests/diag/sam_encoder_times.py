"""Diagnostic (by hand): the figures of DESIGN 7.4 / profiles/sam_encoder.md for the Segment Anything path.

* encode time of hip.LocoSamEngine at the ViT-B, ViT-L and ViT-H geometry at 1024 x 1024 with seeded synthetic weights (HIP
  events, warm, median of --runs), the shader clock over the timed runs, and the split of one profiled run between GEMMs,
  windowed attention, global attention and the rest (loco_sam_profile);
* if transformers is importable: its SamVisionEncoder on PyTorch-ROCm in fp32 with the same weights and input, timed the
  same way, and the rel-L2 between the two outputs;
* one SAM.segment call at the ViT-B geometry on a 512 x 512 image with a seeded random prompt encoder / mask decoder of SAM's
  size: the encoder against the 16 decoder batches + generator.  A random decoder passes the default filters nowhere, which is
  the generator's cheapest case; a second run lifts the predicted IoU and steepens the logits so that every candidate passes
  the two score filters, which is its dearest.

One JSON line per figure.

    python tests/diag/sam_encoder_times.py [--runs 7] [--skip-h]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--skip-h", action="store_true")
a = ap.parse_args()
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import mask_segmentation as ms  # noqa: E402
from loco_edit_amd.config import TINY_DDPM  # noqa: E402
from loco_edit_amd.hip import LocoEngine, LocoSamEngine  # noqa: E402

_spec = importlib.util.spec_from_file_location("sam_host", os.path.join(ROOT, "tests", "test_sam_host.py"))
_host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_host)

dev = torch.device("cuda:0")
clock = LocoEngine(TINY_DDPM, max_batch=1, device=dev)          # loco_clock_stamp lives on a denoiser context


def say(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn):
    """Median ms of --runs warm calls (HIP events) and the average shader clock over them."""
    fn()
    fn()
    torch.cuda.synchronize()
    c0 = clock.clock_stamp()
    ts = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    c1 = clock.clock_stamp()
    torch.cuda.synchronize()
    return {"median_ms": round(statistics.median(ts), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2),
            "runs": a.runs, "sclk_mhz": round(clock.sclk_mhz(c0, c1))}


try:
    from transformers import SamVisionConfig
    from transformers.models.sam.modeling_sam import SamVisionEncoder
except Exception as ex:                                          # the comparison cannot be made here
    SamVisionEncoder = None
    say(what="transformers", importable=False, why=repr(ex))

geoms = [("vit_b", ms.VIT_B, 21), ("vit_l", ms.VIT_L, 23)] + ([] if a.skip_h else [("vit_h", ms.VIT_H, 25)])
for name, cfg, seed in geoms:
    vis = _host.synthetic_vision_sd(cfg, seed=seed)
    pv = torch.randn(3, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
    eng = LocoSamEngine(cfg, device=dev)
    eng.load_state_dict(vis)
    out = torch.empty(1, cfg.output_channels, cfg.grid, cfg.grid, device=dev)
    r = timed(lambda: eng.encode(pv, out))
    eng.profile(True)
    eng.encode(pv, out)
    split = eng.profile_read()
    eng.profile(False)
    say(what="hip_encode", geometry=name, finite=bool(torch.isfinite(out).all()), **r,
        split_ms={k: round(v, 2) for k, v in split.items()})
    if SamVisionEncoder is not None:
        tcfg = SamVisionConfig(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                               num_attention_heads=cfg.num_attention_heads, mlp_dim=cfg.mlp_dim, window_size=cfg.window_size,
                               global_attn_indexes=list(cfg.global_attn_indexes), image_size=cfg.image_size,
                               patch_size=cfg.patch_size, output_channels=cfg.output_channels, layer_norm_eps=cfg.layer_norm_eps)
        try:
            ref = SamVisionEncoder(tcfg)
            ref.load_state_dict(vis, strict=True)
            ref = ref.to(dev).eval()
            with torch.no_grad():
                r = timed(lambda: ref(pv[None]))
                got = ref(pv[None])[0]
            say(what="transformers_encode_fp32", geometry=name, **r, rel_l2_hip_vs_transformers=_host.rel(out, got))
            del ref, got
        except Exception as ex:
            say(what="transformers_encode_fp32", geometry=name, failed=repr(ex))
    del eng, vis, out
    torch.cuda.empty_cache()


def head_sd(cfg, seed):
    """Seeded prompt encoder / mask decoder tensors of the shapes SamModel gives them (fan-in scaled matrices)."""
    g = torch.Generator().manual_seed(seed)
    d, C = cfg.decoder, cfg.decoder.hidden_size
    sd = {}
    for k in ms.head_param_names(cfg):
        part, leaf = k.rsplit(".", 2)[-2], k.rsplit(".", 1)[-1]
        cross = "cross_attn" in k or "final_attn_token_to_image" in k
        inner = C // d.attention_downsample_rate if cross else C
        if k.endswith("positional_embedding"):
            shp = (2, C // 2)
        elif "mask_tokens" in k:
            shp = (d.num_multimask_outputs + 1, C)
        elif k.startswith("prompt_encoder.") or "iou_token" in k:
            shp = (1, C)
        elif "layer_norm_final_attn" in k or ".layer_norm" in k and "upscale" not in k:
            shp = (C,)
        elif "upscale_layer_norm" in k:
            shp = (C // 4,)
        elif "upscale_conv1" in k:
            shp = (C, C // 4, 2, 2) if leaf == "weight" else (C // 4,)
        elif "upscale_conv2" in k:
            shp = (C // 4, C // 8, 2, 2) if leaf == "weight" else (C // 8,)
        elif part in ("q_proj", "k_proj", "v_proj"):
            shp = (inner, C) if leaf == "weight" else (inner,)
        elif part == "out_proj":
            shp = (C, inner) if leaf == "weight" else (C,)
        elif part == "lin1":
            shp = (d.mlp_dim, C) if leaf == "weight" else (d.mlp_dim,)
        elif part == "lin2":
            shp = (C, d.mlp_dim) if leaf == "weight" else (C,)
        elif "output_hypernetworks_mlps" in k:
            o = C // 8 if part == "proj_out" else C
            shp = (o, C) if leaf == "weight" else (o,)
        else:                                                    # the IoU head
            hid = d.iou_head_hidden_dim
            o = d.num_multimask_outputs + 1 if part == "proj_out" else hid
            i = C if part == "proj_in" else hid
            shp = (o, i) if leaf == "weight" else (o,)
        if "layer_norm" in k:
            t = (1.0 if leaf == "weight" else 0.0) + 0.1 * torch.randn(shp, generator=g)
        elif leaf == "bias":
            t = 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("positional_embedding"):
            t = torch.randn(shp, generator=g)
        else:
            t = torch.randn(shp, generator=g) / (shp[-1] if len(shp) == 2 else shp[0]) ** 0.5
        sd[k] = t
    return sd


cfg = ms.SamConfig(ms.VIT_B, ms.SamDecoderConfig())
full = {"vision_encoder." + k: v for k, v in _host.synthetic_vision_sd(cfg.vision, seed=21).items()}
full.update(head_sd(cfg, seed=27))
yy, xx = torch.meshgrid(torch.arange(512.0), torch.arange(512.0), indexing="ij")
image = torch.stack([0.5 + 0.5 * torch.sin(xx / 37 + i) * torch.cos(yy / 23 - i) for i in range(3)]).clamp(0, 1)
image = ms.to_uint8_image(image)
tmp = os.path.join(os.environ.get("TMPDIR", "/tmp"), "sam_encoder_times")
for label in ("no_candidate_passes", "every_candidate_passes"):
    sd = dict(full)
    if label == "every_candidate_passes":
        p = "mask_decoder.iou_prediction_head.proj_out."
        sd[p + "weight"] = sd[p + "weight"] * 0.0
        sd[p + "bias"] = torch.full_like(sd[p + "bias"], 0.94)
        for i in range(4):
            for leaf in ("weight", "bias"):
                k = f"mask_decoder.output_hypernetworks_mlps.{i}.proj_out.{leaf}"
                sd[k] = sd[k] * 1000.0
    sam = ms.SAM(Namespace(mask_model_path=sd, device=dev, filter_mask=0), os.path.join(tmp, "run_" + label))   # a bare state dict
    enc, dec, n = [], [], 0
    for i in range(4):                                           # the first call is the warm-up
        masks, _, _ = sam.segment(image)
        n = int(masks.shape[0])
        if i:
            enc.append(sam.last_timing["encoder_ms"])
            dec.append(sam.last_timing["decoder_generator_ms"])
    e, d_ = statistics.median(enc), statistics.median(dec)
    say(what="segment_call", geometry="vit_b", image="512x512", case=label, masks_after_nms=n, encoder_ms=round(e, 1),
        decoder_generator_ms=round(d_, 1), decoder_generator_share=round(d_ / (e + d_), 3), calls=3)
    del sam
    torch.cuda.empty_cache()
