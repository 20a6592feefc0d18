"""By hand: ms per guided step of the Blended Diffusion baseline, split into its three device parts, on the headline
network (CELEBA_DDPM, 256^2, synthetic weights) with a seeded ViT-B/16-geometry CLIP image tower and 8 windows
(profiles/clip_guidance.md).

    python tests/diag/clip_guidance_profile.py [--iters 7] [--precision bf16x3]

Each part is timed on its own between device events around `iters` warm calls, the median is reported; the step as a whole
(blended.guided_step, which adds the scheduler updates and the small torch operations) is timed the same way."""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import blended, clip_score as cs  # noqa: E402
from loco_edit_amd.config import CELEBA_DDPM, synth_params  # noqa: E402
from loco_edit_amd.hip import LocoClipVisionEngine, LocoEngine  # noqa: E402

DEV = torch.device("cuda:0")


def synth_clip_vision(cfg, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)

    def r(*s, std=0.02):
        return torch.randn(*s, generator=g, device=DEV) * std
    D, Fm, ps = cfg.width, cfg.mlp_dim, cfg.patch_size
    T = 1 + (cfg.image_size // ps) ** 2
    sd = {"embeddings.class_embedding": r(D, std=0.5), "embeddings.patch_embedding.weight": r(D, 3, ps, ps, std=(3 * ps * ps) ** -0.5),
          "embeddings.position_embedding.weight": r(T, D, std=0.3)}
    for ln in ("pre_layrnorm", "post_layernorm"):
        sd[ln + ".weight"], sd[ln + ".bias"] = 1 + r(D, std=0.1), r(D, std=0.1)
    for i in range(cfg.layers):
        p = f"encoder.layers.{i}."
        for ln in ("layer_norm1", "layer_norm2"):
            sd[p + ln + ".weight"], sd[p + ln + ".bias"] = 1 + r(D, std=0.1), r(D, std=0.1)
        for m in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[p + f"self_attn.{m}.weight"], sd[p + f"self_attn.{m}.bias"] = r(D, D, std=D ** -0.5), r(D)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = r(Fm, D, std=D ** -0.5), r(Fm)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = r(D, Fm, std=Fm ** -0.5), r(D)
    sd["visual_projection.weight"] = r(cfg.projection_dim, D, std=D ** -0.5)
    return sd


def timed(fn, iters):
    fn()
    fn()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--windows", type=int, default=8)
    args = ap.parse_args()
    cfg = CELEBA_DDPM
    eng = LocoEngine(cfg, max_batch=4, device=DEV)
    eng.load_state_dict(synth_params(cfg, 0))
    eng.set_precision(args.precision)
    vcfg = cs.ClipVisionConfig(image_size=224, patch_size=16, width=768, layers=12, heads=12, mlp_dim=3072, projection_dim=512)
    vis = LocoClipVisionEngine(vcfg, max_images=args.windows, device=DEV, grad=True)
    vis.load_state_dict(synth_clip_vision(vcfg, 3))
    scorer = types.SimpleNamespace(vision=vis, vision_cfg=vcfg, device=DEV)
    scorer.text_guidance = lambda *a, **k: cs.ClipScorer.text_guidance(scorer, *a, **k)
    R = cfg.resolution
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(1, 3, R, R, generator=gen).to(DEV)
    noise = torch.randn(1, 3, R, R, generator=gen).to(DEV)
    text = torch.randn(vcfg.projection_dim, generator=gen)
    boxes = blended.draw_boxes(gen, args.windows, R, R)
    m = torch.zeros(1, 3, R, R, device=DEV)
    m[:, :, 64:192, 48:208] = 1
    t, at, at_next = 595.0, 0.25, 0.27
    eng.pmp_primal(x, t, at, None)
    eps = eng.pmp_primal_eps().view_as(x)
    _, x0 = eng.sched_step(x, eps, at, at, 0.0, None, want_x0=True)
    _, g_x0 = blended.guidance_gradient(scorer, x0, m, text, boxes, 1000.0, 50.0)
    out = {"network": "CELEBA_DDPM 256^2", "precision": args.precision, "tower": "ViT-B/16 geometry, seeded", "windows": args.windows,
           "grad_bytes": vis.grad_bytes}
    out["primal_ms"] = timed(lambda: eng.pmp_primal(x, t, at, None), args.iters)
    out["clip_forward_backward_ms"] = timed(lambda: blended.guidance_gradient(scorer, x0, m, text, boxes, 1000.0, 50.0), args.iters)
    pv = vis.preprocess_float((x0 * m).contiguous(), boxes)
    g_emb = torch.randn(args.windows, vcfg.projection_dim, generator=gen).to(DEV)
    out["clip_preprocess_ms"] = timed(lambda: vis.preprocess_float((x0 * m).contiguous(), boxes), args.iters)
    out["clip_encode_ms"] = timed(lambda: vis.encode(pv), args.iters)
    out["clip_encode_vjp_ms"] = timed(lambda: vis.encode_vjp(g_emb), args.iters)
    gp = vis.encode_vjp(g_emb)
    out["clip_preprocess_vjp_ms"] = timed(lambda: vis.preprocess_float_vjp(gp, boxes, 1, R, R), args.iters)
    eng.pmp_primal(x, t, at, None)
    out["unet_cotangent_ms"] = timed(lambda: eng.pmp_vjp(g_x0.view(1, -1)), args.iters)
    out["guided_step_ms"] = timed(lambda: blended.guided_step(eng, scorer, x, t, at, at_next, text, boxes, m, 1000.0, 50.0, 1.0, noise), args.iters)
    for k, v in out.items():
        if isinstance(v, tuple):
            out[k] = {"median": round(v[0], 3), "min": round(v[1], 3), "max": round(v[2], 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
