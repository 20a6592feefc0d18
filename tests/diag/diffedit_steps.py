"""Diagnostic (by hand): per-step time of the masked sampler (MaskedDDPMforwardsteps, the `diffedit` ablation) next to the
three-way decode (DDPMforwardsteps mode 'null+(for-null)+(edit-null)', the `sega` ablation) at IF_I_M_UNET 64 x 64 with one
frame and with five, and the wall time of mask_diffedit (20 evaluations at B <= 8).  HIP events around single steps, warm-up,
median of STEPS steps, shader clock noted.  One JSON line per figure.

    python tests/diag/diffedit_steps.py [--root CHECKOUT] [--steps 25]

--root: measure another checkout of this repository (with its library built) in the same visit, e.g. the parent commit:
only the figures that checkout can produce are printed (the three-way decode exists on both sides).
"""
import argparse
import json
import os
import statistics
import sys
from argparse import Namespace

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--steps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--label", default="this")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import torch  # noqa: E402
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd.config import IF_I_M_UNET as cfg  # noqa: E402
from loco_edit_amd.tloco import EditDeepFloydIF  # noqa: E402

dev = torch.device("cuda:0")
gen = torch.Generator().manual_seed(31)
pe = {k: torch.randn(1, cfg.context_len, cfg.encoder_dim, generator=gen) for k in ("for", "edit", "null")}
args = Namespace(device=dev, dtype=torch.float32, seed=1, unet_config=cfg, synthetic_weights=0, ckpt_path="", max_batch=8,
                 precision="bf16x3", dataset_name="Random", for_steps=100, use_yh_custom_scheduler=True, guidance_scale=7.5,
                 guidance_scale_edit=7.5, prompt_emb=pe, for_prompt="a", edit_prompt="b", edit_t=0.75, sampling_mode=False,
                 tilda_v_score_type="null+(for-null)+(edit-null)", ablation_method="sega", mask_type="SAM", vT_path="",
                 x_space_guidance_edit_step=1.0, x_space_guidance_scale=10.0, x_space_guidance_num_step=1,
                 result_folder=os.path.join(os.environ.get("TMPDIR", "/tmp"), "diffedit_steps"))
ed = EditDeepFloydIF(args)
F, E, N = pe["for"], pe["edit"], pe["null"]
s = ed.edit_t_idx
mask = torch.zeros(1, 64, 64, dtype=torch.bool)
mask[:, 24:40, 16:36] = True


def per_step(fn, frames):
    """Median ms of one sampler step (t_start_idx = s, t_end_idx = s + 1: one evaluation set and one update)."""
    x = torch.randn(frames, 3, 64, 64, generator=gen).to(dev)
    for _ in range(a.warmup):
        fn(x)
    torch.cuda.synchronize()
    c0 = ed.engine.clock_stamp()
    ms = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(x)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    c1 = ed.engine.clock_stamp()
    torch.cuda.synchronize()
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "steps": a.steps, "sclk_mhz": round(ed.engine.sclk_mhz(c0, c1))}


for frames in (1, 5):
    r = per_step(lambda x: ed.DDPMforwardsteps(x, s, s + 1, F, E, N, mode="null+(for-null)+(edit-null)"), frames)
    print(json.dumps(dict(r, what="threeway_decode_step", frames=frames, commit=a.label)), flush=True)
    if hasattr(ed, "MaskedDDPMforwardsteps"):
        r = per_step(lambda x: ed.MaskedDDPMforwardsteps(x, s, s + 1, F, E, N, mask=mask), frames)
        print(json.dumps(dict(r, what="masked_sampler_step", frames=frames, commit=a.label)), flush=True)
if hasattr(ed, "mask_diffedit"):
    import time
    x0 = torch.randn(1, 3, 64, 64, generator=gen).clamp(-1, 1).to(dev)
    ts = []
    for i in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ed.mask_diffedit(x0, F, E, N)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"what": "mask_diffedit_wall", "median_ms": round(statistics.median(ts[1:]), 2), "first_ms": round(ts[0], 2),
                      "evaluations": 20, "max_batch": 8, "commit": a.label}), flush=True)
