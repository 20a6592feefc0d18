"""Diagnostic (by hand, one MI355X): the time of one Asyrp training step on the headline network and of its parts, next to
unet_forward / get_h / forward_dh (profiles/asyrp.md).
    python tests/diag/asyrp_time.py [out.md]
CELEBA_DDPM 256 x 256 with seeded weights, the engine's default conv arithmetic (bf16x3), B = 1; the CLIP towers are the tiny_a
fixture of tests/golden (no CLIP checkpoint is available offline: the CLIP rows are NOT those of a ViT-B/32).  Every figure is the
median of 7 timed calls after 2 untimed ones, by device events around the call."""
import importlib.util
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import asyrp, clip_score as cs  # noqa: E402
from loco_edit_amd.config import CELEBA_DDPM, synth_params  # noqa: E402
from loco_edit_amd.hip import LocoAsyrpBlock, LocoEngine  # noqa: E402
from loco_edit_amd.scheduler import YHCustomScheduler  # noqa: E402
import asyrp_oracle as ao  # noqa: E402

DEV = torch.device("cuda:0")


def ms(fn, reps=7, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main():
    spec = importlib.util.spec_from_file_location("gpu_clip_vision", os.path.join(ROOT, "tests", "test_gpu_clip_vision.py"))
    cv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cv)
    cfg = CELEBA_DDPM
    eng = LocoEngine(cfg, max_batch=2, device=DEV)
    eng.load_state_dict(synth_params(cfg, 0))
    sched = YHCustomScheduler(engine=eng)
    sched.set_timesteps(100)
    root = cv.write_clip_folder(os.path.join(tempfile.mkdtemp(), "tiny_a"), "tiny_a")
    sc = cs.load_clip(root, device=DEV, max_images=2, grad=True)
    text = sc.text_embeds(["a photo of a man", "a photo of a man wearing glasses"])
    Ch, Hh, Wh = eng.h_shape
    blk = LocoAsyrpBlock(Ch, Hh, Wh, cfg.temb_ch, max_batch=1, gn_eps=cfg.gn_eps, seed=None, device=DEV)
    p = ao.random_params(Ch, cfg.temb_ch, seed=1)
    p["W2"] = 0.5 * p["W2"]
    blk.load_state_dict(p)
    tr = asyrp.AsyrpTrainer(eng, sched, sc, blk, text[0], text[1], cfg, lr=1e-3)
    t, t_next = float(sched.timesteps[40]), float(sched.timesteps_next[40])
    at = sched.alpha_at(t)
    x = torch.randn(1, 3, cfg.resolution, cfg.resolution, generator=torch.Generator().manual_seed(1)).to(DEV)
    e = asyrp.time_vector(cfg, t).to(DEV)
    h = eng.get_h(x, t)
    dh = blk.forward(h, e)
    eps = eng.unet_forward(x, t)
    g_h = torch.randn_like(h)
    x0 = torch.randn_like(x).clamp(-1, 1)
    g = torch.randn(1, x.numel(), device=DEV)

    def primal():
        eng.pmp_primal(x, t, at, None, use_et=False, tap="dec", dh=dh.reshape(-1))

    rows = [("unet_forward (B = 1)", lambda: eng.unet_forward(x, t)),
            ("get_h (B = 1)", lambda: eng.get_h(x, t)),
            ("forward_dh (B = 1)", lambda: eng.unet_forward(x, t, dh=dh.reshape(1, -1))),
            ("f_t forward (512 x 8 x 8, E = 512)", lambda: blk.forward(h, e)),
            ("decoder-tap primal at h + dh", primal),
            ("directional CLIP loss + pixel gradient (tiny_a towers)", lambda: asyrp.directional_clip_loss(sc, x0, x0 * 0.9, text[0], text[1])),
            ("h_dec cotangent, k = 1 (pmp_vjp)", lambda: eng.pmp_vjp(g)),
            ("f_t backward (ten parameter gradients)", lambda: blk.backward(g_h)),
            ("Adam step (one launch)", lambda: blk.adam_step(1, 1e-3)),
            ("asymmetric step", lambda: eng.sched_step_asym(x, eps, eps, at, sched.alpha_at(t_next)))]
    lines = ["| part | ms (median of 7) | min - max |", "|---|---|---|"]
    for name, fn in rows:
        if name.startswith("h_dec"):
            primal()
        med, lo, hi = ms(fn)
        lines.append(f"| {name} | {med:.3f} | {lo:.3f} - {hi:.3f} |")
    med, lo, hi = ms(lambda: tr.step(x, t, t_next))
    lines.append(f"| **one AsyrpTrainer.step** | {med:.3f} | {lo:.3f} - {hi:.3f} |")
    text_out = "\n".join(lines)
    print(f"engine: {eng.version()}, conv arithmetic {eng.get_precision()}, t = {t:.1f}")
    print(text_out)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text_out + "\n")


if __name__ == "__main__":
    main()
