"""GPU tests of the Blended Diffusion baseline (loco_edit_amd/blended.py, EditUncondDiffusion.run_edit_blended_diffusion) on
TINY_DDPM (32^2, synthetic weights) with the tiny_a CLIP fixture:

* one guided step against float64: the U-Net of oracle/loco_oracle.py under autograd composed with tests/clip_grad_oracle.py.
  g = J^T g_x0 and x_t' at the bar the unmasked cotangent test of tests/test_gpu_parity.py holds on this network
  (1.5 x TOL[precision]: 3e-5 in f32, 1.5e-4 in bf16x3);
* a whole 4-step run: the result equals the source outside the mask bit for bit; the same seed gives the same bits; scales 0
  give the bits of the unguided blended sampler assembled from unet_forward / sched_step; at a positive scale the whole-frame
  CLIP loss of the result is lower than that of the scale-0 run;
* the CLI: the PNG and the _clip.json exist; the flag without --clip_model_path or --edit_prompt raises in the parser."""
import importlib.util
import json
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loco_edit_amd  # noqa: E402,F401
import loco_oracle as orc  # noqa: E402
from loco_edit_amd import blended, clip_score as cs  # noqa: E402
from loco_edit_amd.config import TINY_DDPM, synth_params  # noqa: E402
import clip_grad_oracle as cgo  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {"f32": 2e-5, "bf16x3": 1e-4}          # tests/test_gpu_parity.py; its unmasked cotangent holds 1.5 x these on TINY_DDPM
_spec = importlib.util.spec_from_file_location("gpu_clip_vision", os.path.join(ROOT, "tests", "test_gpu_clip_vision.py"))
_cv = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cv)
PROMPT = "a photo of a man wearing glasses"


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def engine():
    from loco_edit_amd.hip import LocoEngine
    e = LocoEngine(TINY_DDPM, max_batch=4, device=torch.device(DEV))
    e.load_state_dict(synth_params(TINY_DDPM, 0))
    return e


@pytest.fixture(scope="module")
def scorer(tmp_path_factory):
    root = _cv.write_clip_folder(str(tmp_path_factory.mktemp("clip_blended") / "tiny_a"), "tiny_a")
    sc = cs.load_clip(root, device=torch.device(DEV), max_images=4, grad=True)
    return sc, sc.text_embeds([PROMPT])[0]


def the_mask():
    m = torch.zeros(3, 32, 32, dtype=torch.bool)
    m[:, 6:24, 8:27] = True
    return m


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_one_guided_step_vs_float64(prec, engine, scorer):
    sc, text = scorer
    _, _, vsd, vcfg = _cv.fixture("tiny_a")
    engine.set_precision(prec)
    oed = orc.OracleEdit({k: v.double() for k, v in orc.to_torch(synth_params(TINY_DDPM, 0)).items()}, TINY_DDPM)
    sched = oed.sched
    t, t_next = sched.timesteps[60], sched.timesteps_next[60]
    at, at_next = sched.alpha_at(t), sched.alpha_at(t_next)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(1, 3, 32, 32, generator=gen)
    noise = torch.randn(1, 3, 32, 32, generator=gen)
    boxes = blended.draw_boxes(gen, 4, 32, 32)
    assert boxes[0] == (0, 0, 32, 32) and len(boxes) == 4
    m = the_mask()[None].float()
    cscale, rscale, eta = 1000.0, 50.0, 1.0
    got_next, got_g, got_loss = blended.guided_step(engine, sc, x.to(DEV), float(t), float(at), float(at_next), text, boxes, m.to(DEV),
                                                    cscale, rscale, eta, noise.to(DEV))
    # float64: the same step under autograd
    a, an = at.double(), at_next.double()
    x64 = x.double().clone().requires_grad_(True)
    eps = oed.unet(x64, t)
    x0 = (x64 - eps * (1 - a).sqrt()) / a.sqrt()
    pv = cgo.preprocess_windows(x0 * m.double(), boxes, vcfg.image_size, vcfg.image_mean, vcfg.image_std)
    loss = cscale * cgo.cosine_losses(cgo.clip_vision_embeds(vsd, vcfg, pv), text.double()).mean() \
        + rscale * (x0 - x0.clamp(-1, 1)).abs().mean()
    g, = torch.autograd.grad(loss, x64)
    assert float((x0.detach().abs() > 1).double().mean()) > 0.01          # the range term is live
    eps_hat = eps.detach() + (1 - a).sqrt() * g
    sigma = ((1 - a / an) * (1 - an) / (1 - a)).sqrt()
    p_xt = (x.double() - eps_hat * (1 - a).sqrt()) / a.sqrt()
    want_next = an.sqrt() * p_xt + (1 - an - eta * sigma ** 2).sqrt() * eps_hat + eta * sigma * noise.double()
    eg, ex, el = rel(got_g, g), rel(got_next, want_next), abs(float(got_loss) - float(loss.detach())) / abs(float(loss.detach()))
    print(f"{prec}: g = J^T g_x0 rel-L2 {eg:.2e}, x_t' rel-L2 {ex:.2e} (bar {1.5 * TOL[prec]:.1e}); loss {float(got_loss):.5f} rel err {el:.1e}; "
          f"|sqrt(1 - a) g| / |eps| = {float(((1 - a).sqrt() * g).norm() / eps.detach().norm()):.2e}")
    assert eg < 1.5 * TOL[prec] and ex < 1.5 * TOL[prec]


def sampler_setup(engine, n_steps=9):
    from loco_edit_amd.scheduler import YHCustomScheduler
    sched = YHCustomScheduler(engine=engine)
    sched.set_timesteps(n_steps)
    x_src = (_cv.smooth_noise_image(32, 32, seed=9).permute(2, 0, 1).float() / 127.5 - 1)[None].to(DEV)
    return sched, x_src


def unguided_blended(engine, sched, x_src, mask, seed, start_t, num_aug, eta=1.0):
    """The blended sampler without guidance from calls that existed before the baseline; the draws in blended.run's order."""
    gen = torch.Generator().manual_seed(seed)
    keep = mask.to(DEV).view_as(x_src)
    ts, tn = sched.timesteps, sched.timesteps_next
    i0 = int((ts - start_t * 1000).abs().argmin())
    a0 = sched.alpha_at(ts[i0])
    x = (math.sqrt(a0) * x_src + math.sqrt(1.0 - a0) * torch.randn(x_src.shape, generator=gen).to(DEV)).contiguous()
    for i in range(i0, len(ts)):
        at, an = sched.alpha_at(ts[i]), sched.alpha_at(tn[i])
        blended.draw_boxes(gen, num_aug, 32, 32)
        noise = torch.randn(x_src.shape, generator=gen).to(DEV)
        nxt, _ = engine.sched_step(x, engine.unet_forward(x, float(ts[i])), at, an, eta, noise)
        bg = x_src if i == len(ts) - 1 else math.sqrt(an) * x_src + math.sqrt(1.0 - an) * torch.randn(x_src.shape, generator=gen).to(DEV)
        x = torch.where(keep, nxt, bg).contiguous()
    return x, len(ts) - i0


def test_four_step_run(engine, scorer):
    sc, text = scorer
    engine.set_precision("bf16x3")
    sched, x_src = sampler_setup(engine)
    mask = the_mask()
    kw = dict(seed=3, start_t=0.5, num_aug=4)
    plain, steps = unguided_blended(engine, sched, x_src, mask, 3, 0.5, 4)
    assert steps == 4
    zero = blended.run(engine, sched, sc, x_src, mask, text, clip_guidance_scale=0.0, range_scale=0.0, **kw)
    assert torch.equal(zero, plain)
    out = blended.run(engine, sched, sc, x_src, mask, text, clip_guidance_scale=1000.0, range_scale=50.0, **kw)
    assert torch.equal(out, blended.run(engine, sched, sc, x_src, mask, text, clip_guidance_scale=1000.0, range_scale=50.0, **kw))
    other = blended.run(engine, sched, sc, x_src, mask, text, clip_guidance_scale=1000.0, range_scale=50.0, **dict(kw, seed=4))
    assert not torch.equal(out, other)
    outside = ~mask.to(DEV).view_as(x_src)
    for r in (zero, out, other):
        assert torch.equal(r[outside], x_src[outside]) and bool(torch.isfinite(r).all())
    assert not torch.equal(out, zero)
    l_out, _ = sc.text_guidance(out, text, [(0, 0, 32, 32)])
    l_zero, _ = sc.text_guidance(zero, text, [(0, 0, 32, 32)])
    print(f"whole-frame CLIP loss: guided {float(l_out):.5f}, unguided {float(l_zero):.5f}")
    assert float(l_out) < float(l_zero)


def test_cli(tmp_path, monkeypatch):
    from loco_edit_amd.main import main
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    root = _cv.write_clip_folder(str(tmp_path / "tiny_a"), "tiny_a")
    rdir = tmp_path / "runs" / "CelebA_HQ_HF-Random" / "results" / "sample_seed11"
    os.makedirs(rdir / "mask")
    masks = torch.zeros(2, 32, 32, dtype=torch.bool)
    masks[0, 8:20, 6:18] = True
    torch.save(masks, rdir / "mask" / "mask.pt")
    base = ["--sh_file_name", "main_celeba_hf_null_space_projection.sh", "--sample_idx", "3", "--device", DEV, "--dtype", "fp32",
            "--seed", "11", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Random", "--unet_preset", "tiny_ddpm",
            "--synthetic_weights", "0", "--for_steps", "100", "--inv_steps", "100", "--use_yh_custom_scheduler", "True", "--performance_boosting_t", "0.2", "--mask_index", "0",
            "--run_edit_blended_diffusion", "True", "--blended_num_aug", "3", "--blended_start_t", "0.08", "--quality_metrics", "ssim,mmse"]
    with pytest.raises(ValueError, match="--clip_model_path"):
        main(base + ["--edit_prompt", PROMPT])
    with pytest.raises(ValueError, match="--edit_prompt"):
        main(base + ["--clip_model_path", root])
    out = main(base + ["--clip_model_path", root, "--edit_prompt", PROMPT, "--for_prompt", "a photo of a man"])
    assert tuple(out.shape) == (1, 3, 32, 32) and bool(torch.isfinite(out).all())
    names = os.listdir(rdir)
    png = [n for n in names if n.endswith("_blended.png")]
    assert len(png) == 1
    stem = png[0][:-len("_blended.png")]
    with open(rdir / f"{stem}_clip.json") as f:
        rec = json.load(f)
    assert rec["edit_prompt"] == PROMPT and len(rec["frames"]) == 1 and rec["frames"][0]["clip_edit"] is not None
    assert rec["frames"][0]["directional"] is not None
    assert os.path.exists(rdir / f"{stem}_quality.json")
