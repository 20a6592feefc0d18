"""Diagnostic (by hand): time of text-prompted masks at the real geometry (profiles/clipseg.md).

CLIPSeg rd64 -- ViT-B/16 run at 352 (G = 22, T = 485), taps after layers 3, 6, 9, reduce_dim 64, 4 decoder heads, ffn 2048 --
with seeded random weights, 1 image x 4 prompts, both heads: HIP events around the warm calls of the tower (encode_taps, which
stops after layer 9), the decoder and the mask kernel (352 -> 256), median of --runs, the shader clock from loco_clock_stamp
over the timed runs.  One JSON line per figure.

    python tests/diag/clipseg_times.py [--runs 9]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=9)
a = ap.parse_args()
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import clip_score as cs  # noqa: E402
from loco_edit_amd import prompt_mask as pm  # noqa: E402
from loco_edit_amd.config import TINY_DDPM  # noqa: E402
from loco_edit_amd.hip import LocoClipSegDecoder, LocoClipVisionEngine, LocoEngine  # noqa: E402

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
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    c1 = clock.clock_stamp()
    return statistics.median(ts), min(ts), max(ts), LocoEngine.sclk_mhz(c0, c1)


def seeded(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, s in shapes.items():
        if "norm" in k and k.endswith("weight"):
            out[k] = 1 + 0.1 * torch.randn(s, generator=g)
        elif k.endswith("bias"):
            out[k] = 0.1 * torch.randn(s, generator=g)
        else:
            out[k] = torch.randn(s, generator=g) * (s[-1] if len(s) == 2 else 64) ** -0.5
    return out


vcfg = cs.ClipVisionConfig(image_size=352, patch_size=16, width=768, layers=12, heads=12, mlp_dim=3072, projection_dim=512,
                           image_mean=pm.IMAGENET_MEAN, image_std=pm.IMAGENET_STD)
tower = LocoClipVisionEngine(vcfg, max_images=1, device=dev)
tower.load_state_dict(seeded(cs.vision_param_shapes(vcfg), 0))
frame = torch.randint(0, 256, (1, 512, 512, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
cond = torch.randn(4, 512, generator=torch.Generator().manual_seed(2)).to(dev)
for complex_head in (True, False):
    dcfg = pm.ClipSegDecoderConfig(complex_head=complex_head, max_masks=4)
    dec = LocoClipSegDecoder(dcfg, device=dev)
    dec.load_state_dict(seeded(pm.decoder_param_shapes(dcfg), 3))
    pv = dec.preprocess(frame, 352, 3, pm.IMAGENET_MEAN, pm.IMAGENET_STD)
    taps = tower.encode_taps(pv, pm.DEFAULT_EXTRACT_LAYERS)
    logits = dec.decode(taps, cond, [0] * 4)
    assert bool(torch.isfinite(logits).all()) and tuple(logits.shape) == (4, 352, 352)
    stages = {"preprocess_512_to_352": lambda: dec.preprocess(frame, 352, 3, pm.IMAGENET_MEAN, pm.IMAGENET_STD),
              "tower_taps_3_6_9": lambda: tower.encode_taps(pv, pm.DEFAULT_EXTRACT_LAYERS),
              "decoder_4_masks": lambda: dec.decode(taps, cond, [0] * 4),
              "masks_352_to_256": lambda: dec.masks(logits, 256, 0.0)}
    stages["all"] = lambda: [f() for f in list(stages.values())[:4]]
    for name, fn in stages.items():
        med, lo, hi, mhz = timed(fn)
        say(head="complex" if complex_head else "simple", stage=name, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
            runs=a.runs, sclk_mhz=round(mhz))
