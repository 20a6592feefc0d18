"""Diagnostic (by hand): the figures of DESIGN 7.5 "Measured" for the latent-consistency path.

* per-solve time at size: `config.LCM_DREAMSHAPER_V7_UNET` + `config.SD_VAE_DECODER`, mask on the decoded 3 x 512 x 512 image,
  5 probes, 12 iterations (`EditLatentConsistency.local_encoder_decoder_pullback_zt`), seeded synthetic weights;
* next to it the same solve on `config.SD15_UNET` through `EditStableDiffusion` with `guidance_scale` 1 (one branch of weight
  1): the single-branch solve that existed before this path.  Expected: equal within the +-3 % the README attributes to the
  box -- the added work per solve is one ch x P GEMV and ch adds;
* `lcm_step` (one launch) against `sched_step` + two `lincomb` (three launches, two intermediates) at 5 x 4 x 64 x 64 elements.

HIP events, warm, median of --runs; one JSON line per figure.

    python tests/diag/lcm_steps.py [--runs 7]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=7)
a = ap.parse_args()
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import config as K  # noqa: E402
from loco_edit_amd.tloco_lcm import EditLatentConsistency  # noqa: E402
from loco_edit_amd.tloco_sd import EditStableDiffusion  # noqa: E402

os.environ.pop("WORLD_SIZE", None)
dev = torch.device("cuda:0")


def say(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, inner=1):
    """Median ms per call of --runs warm timings (HIP events), each over `inner` calls."""
    fn()
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "runs": a.runs}


def build(cls, cfg, params, guidance_scale, tmp, **kw):
    args = Namespace(device=dev, dtype=torch.float32, seed=1, unet_config=cfg, vae_config=K.SD_VAE_DECODER, params=params,
                     synthetic_weights=0, ckpt_path="", vae_ckpt_path="", max_batch=8, precision=None, dataset_name="Random",
                     for_steps=100, use_yh_custom_scheduler=True, guidance_scale=guidance_scale, guidance_scale_edit=7.5,
                     prompt_emb=None, prompt_emb_seed=31, for_prompt="a", edit_prompt="b", edit_t=0.5, sampling_mode=False,
                     tilda_v_score_type="null+(for-null)+(edit-null)", ablation_method="null-space-proj", mask_type="SAM",
                     vT_path="", use_sega=False, x_space_guidance_edit_step=1.0, x_space_guidance_scale=0.5,
                     x_space_guidance_num_step=1, result_folder=tmp, **kw)
    return cls(args)


g = torch.Generator().manual_seed(3)
z = torch.randn(1, 4, 64, 64, generator=g).to(dev)
v0 = torch.randn(K.SD15_UNET.n, 5, generator=g).to(dev)
mask = torch.zeros(3, 512, 512, dtype=torch.bool)
mask[:, 160:320, 96:352] = True
ITER = 12

with tempfile.TemporaryDirectory() as tmp:
    # the synthesiser draws every tensor from (seed, name): the LCM set is the SD v1 set plus cond_proj
    sd_params = K.synth_params(K.SD15_UNET, 0)
    lcm_params = dict(sd_params)
    shp = K.param_shapes(K.LCM_DREAMSHAPER_V7_UNET)["time_embed.cond_proj.weight"]
    lcm_params["time_embed.cond_proj.weight"] = K._synth_tensor(K.LCM_DREAMSHAPER_V7_UNET, 0, "time_embed.cond_proj.weight", shp)

    ed = build(EditLatentConsistency, K.LCM_DREAMSHAPER_V7_UNET, lcm_params, 7.5, tmp, num_inference_steps=4, edit_t_idx=2,
               lcm_timesteps="linspace")
    t = ed.scheduler.timesteps[ed.edit_t_idx]
    solve = lambda: ed.local_encoder_decoder_pullback_zt(z, t, ed.edit_t_idx, "a", pca_rank=5, min_iter=ITER, max_iter=ITER,
                                                         mask=mask, v0=v0, verbose=False)
    say(what="lcm_solve", unet="LCM_DREAMSHAPER_V7_UNET", decoder="SD_VAE_DECODER", probes=5, iterations=ITER, t=int(t),
        precision=ed.engine.get_precision(), **timed(solve))
    # the scheduler step against its three-launch composition, 5 x 4 x 64 x 64 elements
    x, eps, nz = (torch.randn(5, 4, 64, 64, generator=g).to(dev) for _ in range(3))
    eng, sch = ed.engine, ed.scheduler
    _, at, at_prev, _ = sch.step_coeffs(t)
    c_skip, c_out = sch.scalings(t)
    s_prev, s1m_prev = float(at_prev) ** 0.5, (1.0 - float(at_prev)) ** 0.5

    def composed():
        _, x0 = eng.sched_step(x, eps, at, at, 0.0, None, want_x0=True)
        den = eng.lincomb([(c_out, x0), (c_skip, x)])
        return eng.lincomb([(s_prev, den), (s1m_prev, nz)]), den
    fused = lambda: eng.lcm_step(x, eps, at, at_prev, c_skip, c_out, nz)
    pf, df = fused()
    pc, dc = composed()
    say(what="lcm_step", elements=x.numel(), launches=1, max_abs_diff_prev=float((pf - pc).abs().max()),
        max_abs_diff_denoised=float((df - dc).abs().max()), **timed(fused, inner=200))
    say(what="sched_step+2xlincomb", elements=x.numel(), launches=3, **timed(composed, inner=200))
    del ed, eng, sch
    torch.cuda.empty_cache()

    sd = build(EditStableDiffusion, K.SD15_UNET, sd_params, 1.0, tmp)
    F, E, N = sd.for_prompt_emb, sd.edit_prompt_emb, sd.null_prompt_emb
    t_sd = sd.scheduler.timesteps[sd.edit_t_idx]
    solve_sd = lambda: sd.local_encoder_decoder_pullback_zt(z, t_sd, sd.edit_t_idx, F, E, N, pca_rank=5, min_iter=ITER, max_iter=ITER,
                                                            mask=mask, mode="null+(for-null)", v0=v0, verbose=False)
    say(what="sd15_single_branch_solve", unet="SD15_UNET", decoder="SD_VAE_DECODER", probes=5, iterations=ITER, t=float(t_sd),
        guidance_scale=1.0, precision=sd.engine.get_precision(), **timed(solve_sd))
