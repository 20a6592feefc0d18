"""Diagnostic (by hand): the two encode times behind profiles/encoder_attn.md, for the library LOCO_HIP_LIB names -- one process per
run, so that an A/B interleaves fresh processes of each library.

* SAM: hip.LocoSamEngine at the ViT-B geometry at 1024 x 1024, seeded synthetic weights -- the geometry, weights and timing of
  sam_encoder_times.py (HIP events, warm, median of --runs);
* CLIP: hip.LocoClipVisionEngine at the ViT-L/14 geometry, `encode` of 8 images, weights seeded on the device as
  test_gpu_clip_vision.py's test_vit_l14_vs_restatement builds them.

One JSON line per figure, each with the sha256 of the output.

    python tests/diag/encoder_attn_times.py [--runs 7]
"""
import argparse
import hashlib
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=7)
a = ap.parse_args()
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import clip_score as cs, mask_segmentation as ms  # noqa: E402
from loco_edit_amd.hip import LocoClipVisionEngine, LocoSamEngine  # noqa: E402


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dev = torch.device("cuda:0")


def timed(fn):
    fn()
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "runs": a.runs}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


lib = os.path.basename(os.environ.get("LOCO_HIP_LIB", "libloco_hip.so"))

cfg = ms.VIT_B
vis = _load("test_sam_host").synthetic_vision_sd(cfg, seed=21)
pv = torch.randn(3, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(22)).to(dev)
eng = LocoSamEngine(cfg, device=dev)
eng.load_state_dict(vis)
out = torch.empty(1, cfg.output_channels, cfg.grid, cfg.grid, device=dev)
r = timed(lambda: eng.encode(pv, out))
print(json.dumps(dict(what="sam_vit_b_1024_encode", lib=lib, **r, sha256=sha(out))), flush=True)
del eng, vis, out
torch.cuda.empty_cache()

cfg = cs.CLIP_VIT_L14
sd = _load("test_gpu_clip_vision")._synth_clip_vision(cfg, 3)
eng = LocoClipVisionEngine(cfg, max_images=8, device=dev)
eng.load_state_dict(sd)
pv = torch.randn(8, 3, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(5)).to(dev)
res = {}
r = timed(lambda: res.__setitem__("emb", eng.encode(pv)))
print(json.dumps(dict(what="clip_vit_l14_encode_8", lib=lib, **r, sha256=sha(res["emb"]))), flush=True)
