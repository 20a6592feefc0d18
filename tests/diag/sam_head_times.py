"""Diagnostic (by hand): the torch head against the HIP head of Segment Anything (profiles/sam_encoder.md).

The companion of tests/diag/sam_encoder_times.py, whose `segment_call` lines give the share of the 16 decoder batches + generator
in one SAM.segment call with the torch head.  Here, at the ViT-B geometry on the same 512 x 512 image with a seeded random
prompt encoder / mask decoder of SAM's size, in the same two regimes (a random decoder passes the default filters nowhere; with
the predicted IoU lifted and the logits steepened every candidate passes the two score filters):

* the share line of one SAM.segment call (torch head, as the companion prints it);
* the 16 decoder batches + generator alone with head="torch" (mask_segmentation.SamHead + the torch filters) and with
  head="hip" (csrc/samdec.hip: SamHeadHip as head and scorer) on the same engine, embedding and weights: HIP events, warm,
  median of --runs, the shader clock from loco_clock_stamp over the timed runs;
* whether the two heads returned the same masks and scores.

One JSON line per figure.

    python tests/diag/sam_head_times.py [--runs 7]
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
a = ap.parse_args()
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import mask_segmentation as ms  # noqa: E402
from loco_edit_amd.config import TINY_DDPM  # noqa: E402
from loco_edit_amd.hip import LocoEngine  # noqa: E402

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


def head_sd(cfg, seed):
    """Seeded prompt encoder / mask decoder of the shapes SamModel gives them: fan-in scaled matrices, LayerNorm 1 / 0 +- 0.1,
    biases 0.1 N, tokens, embeddings and the positional matrix N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in ms.head_param_shapes(cfg).items():
        if "layer_norm" in k:
            t = (1.0 if k.endswith("weight") else 0.0) + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith(".bias"):
            t = 0.1 * torch.randn(shp, generator=g)
        elif k.endswith(("positional_embedding", "_embed.weight", "point_embed.1.weight", "_token.weight", "_tokens.weight")):
            t = torch.randn(shp, generator=g)
        else:
            fan_in = shp[0] if "upscale_conv" in k else torch.Size(shp[1:]).numel()
            t = torch.randn(shp, generator=g) / fan_in ** 0.5
        sd[k] = t
    sd["prompt_encoder.point_embed.0.weight"] = torch.randn(1, cfg.decoder.hidden_size, generator=g)
    return sd


cfg = ms.SamConfig(ms.VIT_B, ms.SamDecoderConfig())
full = {"vision_encoder." + k: v for k, v in _host.synthetic_vision_sd(cfg.vision, seed=21).items()}
full.update(head_sd(cfg, seed=27))
yy, xx = torch.meshgrid(torch.arange(512.0), torch.arange(512.0), indexing="ij")
image = torch.stack([0.5 + 0.5 * torch.sin(xx / 37 + i) * torch.cos(yy / 23 - i) for i in range(3)]).clamp(0, 1)
image = ms.to_uint8_image(image)
tmp = os.path.join(os.environ.get("TMPDIR", "/tmp"), "sam_head_times")
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
    say(what="segment_call", geometry="vit_b", image="512x512", case=label, head="torch", masks_after_nms=n, encoder_ms=round(e, 1),
        decoder_generator_ms=round(d_, 1), decoder_generator_share=round(d_ / (e + d_), 3), calls=3)
    # the decoder batches + generator alone, both heads on the same engine, embedding and weights
    pv, orig, resh = ms.preprocess(image, cfg.vision.image_size)
    emb = sam.engine.encode(pv)
    hip_head = ms.SamHeadHip(sam.cfg, ms.normalize_sam_state_dict(sd), device=dev, max_prompts=sam.generator.points_per_batch)
    got = {}
    with torch.no_grad():
        for head, fn in (("torch", lambda: sam.generator.generate(sam.head, emb, orig, resh)),
                         ("hip", lambda: sam.generator.generate(hip_head, emb, orig, resh, scorer=hip_head))):
            r = timed(fn)
            out = fn()
            got[head] = out
            say(what="decoder_generator", geometry="vit_b", image="512x512", case=label, head=head, masks_after_nms=int(out[0].shape[0]), **r)
    same = got["torch"][0].shape == got["hip"][0].shape
    say(what="decoder_generator_agreement", case=label, same_count=bool(same),
        differing_pixels=int((got["torch"][0] != got["hip"][0]).sum()) if same else None,
        max_score_diff=float((got["torch"][1] - got["hip"][1]).abs().max()) if same and got["hip"][1].numel() else None)
    del sam, hip_head, got, emb
    torch.cuda.empty_cache()
