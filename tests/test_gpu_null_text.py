"""GPU tests of null-text inversion on the Stable Diffusion path (loco_edit_amd.null_text.NullTextInversion and the
--null_text_inversion route of tloco_sd.EditStableDiffusion).

The optimiser against its float64 restatement on the host (tests/context_grad_oracle.null_text_restatement: oracle forward,
torch.autograd, torch.optim.Adam) on the case of tests/null_text_case.py: losses and final embeddings within 4 x what the same
restatement run in fp32 on the host differs from its float64 run (the project's yardstick rule; both figures printed).  That
the case is in a regime where Adam iterates can be compared at all is checked on the CPU, tests/test_null_text_host.py."""
import json
import os
import sys
from argparse import Namespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loco_edit_amd  # noqa: E402,F401
import null_text_case as case  # noqa: E402
from context_grad_oracle import rel  # noqa: E402
from loco_edit_amd.config import TINY_DECODER, TINY_ENCODER, TINY_LDM  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _edit(c, tmp_path, prec, **kw):
    from loco_edit_amd.tloco_sd import EditStableDiffusion
    os.environ.pop("WORLD_SIZE", None)
    a = dict(device=torch.device(DEV), dtype=torch.float32, seed=1, unet_config=TINY_LDM, vae_config=TINY_DECODER,
             synthetic_weights=0, ckpt_path="", vae_ckpt_path="", max_batch=4, precision=prec, dataset_name="Random",
             for_steps=case.FOR_STEPS, use_yh_custom_scheduler=True, guidance_scale=case.W, guidance_scale_edit=4.0,
             prompt_emb={"for": c["cond"], "edit": c["edit"], "null": c["null"]}, for_prompt="a man",
             edit_prompt="a man wearing glasses", edit_t=0.7, sampling_mode=False,
             tilda_v_score_type="null+(for-null)+(edit-null)", ablation_method="null-space-proj", mask_type="SAM", vT_path="",
             use_sega=False, x_space_guidance_edit_step=1.0, x_space_guidance_scale=0.5, x_space_guidance_num_step=16,
             result_folder=str(tmp_path))
    a.update(kw)
    return EditStableDiffusion(Namespace(**a))


def test_optimiser_vs_float64_restatement(tmp_path):
    from loco_edit_amd.null_text import NullTextInversion
    c = case.build()
    ed = _edit(c, tmp_path, "f32")
    ed.scheduler.set_timesteps(case.FOR_STEPS)
    embs, zbar, losses = NullTextInversion(ed).run(c["traj"], c["timesteps"], c["null"], c["cond"], case.INNER, case.LR,
                                                   case.EARLY_STOP)
    assert tuple(embs.shape) == (case.STEPS, TINY_LDM.context_len, TINY_LDM.context_dim)
    assert [len(li) for li in losses] == [case.INNER] * case.STEPS
    eL, eE, eZ = rel(c["flat"](losses), c["flat"](c["losses64"])), rel(embs, c["embs64"]), rel(zbar, c["zbar64"])
    print(f"null-text vs float64: losses rel-L2 {eL:.3e} (fp32 host {c['yard_losses']:.3e}), embeddings {eE:.3e} "
          f"(fp32 host {c['yard_embs']:.3e}), z_bar {eZ:.3e} (fp32 host {c['yard_zbar']:.3e})")
    for li in losses:
        assert li[-1] <= li[0]
    assert rel(embs[-1], c["null"][0]) > 1e-2                    # the states moved
    assert eL <= 4 * c["yard_losses"] and eE <= 4 * c["yard_embs"]


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_without_inner_steps_it_is_the_plain_guided_decode(prec, tmp_path):
    from loco_edit_amd.null_text import NullTextInversion
    c = case.build()
    ed = _edit(c, tmp_path, prec)
    ed.scheduler.set_timesteps(case.FOR_STEPS)
    embs, zbar, losses = NullTextInversion(ed).run(c["traj"], c["timesteps"], c["null"], c["cond"], 0)
    assert losses == [[]] * case.STEPS and all(torch.equal(e.cpu(), c["null"][0]) for e in embs)
    ref, _, i = ed.DDIMforwardsteps(c["traj"][0].to(DEV), case.T0_IDX, case.T0_IDX + case.STEPS, c["cond"], c["edit"], c["null"])
    assert i == case.T0_IDX + case.STEPS and torch.equal(zbar, ref)
    # ... and with the optimised states the sampler's per-step list reproduces the optimiser's latent
    embs, zbar, _ = NullTextInversion(ed).run(c["traj"], c["timesteps"], c["null"], c["cond"], 2, case.LR, case.EARLY_STOP)
    per_step = [None] * case.T0_IDX + [e[None].contiguous() for e in embs]
    z2, _, _ = ed.DDIMforwardsteps(c["traj"][0].to(DEV), case.T0_IDX, case.T0_IDX + case.STEPS, c["cond"], c["edit"], c["null"],
                                   null_prompt_embs=per_step)
    assert torch.equal(z2, zbar) and not torch.equal(z2, ref)


def test_driver_edits_an_image_of_the_dataset(tmp_path):
    """run_edit_null_space_projection_zt on the tiny networks with an in-memory one-image dataset: the inversion runs once,
    the grid, the report and the cache are written; a second run loads the cache and decodes the same frames."""
    c = case.build()
    g = torch.Generator().manual_seed(9)
    image = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    kw = dict(dataset_name="Synthetic", dataset=[image], vae_encoder_config=TINY_ENCODER, for_steps=12, inv_steps=12,
              null_text_inversion=True, null_text_inner_steps=2, null_text_lr=1e-2, null_text_early_stop=1e-5, sample_idx=0)
    with pytest.raises(ValueError, match="inv_steps == for_steps"):
        _edit(c, tmp_path, "bf16x3", **dict(kw, inv_steps=10))._zT()
    with pytest.raises(ValueError, match="Random"):
        _edit(c, tmp_path, "bf16x3", **dict(kw, null_text_inversion=False))._zT()
    with pytest.raises(ValueError, match="edit step must come after"):
        _edit(c, tmp_path, "bf16x3", **dict(kw, edit_t=0.999))._zT()          # decode step 0: ahead of the inverted latent
    ed = _edit(c, tmp_path, "bf16x3", **kw)
    masks = torch.zeros(2, 1, 64, 64, dtype=torch.bool)
    masks[1, 0, 20:40, 12:44] = True
    os.makedirs(os.path.join(ed.result_folder, "mask"))
    torch.save(masks, os.path.join(ed.result_folder, "mask", "mask.pt"))
    run = lambda e: e.run_edit_null_space_projection_zt(op="mid", block_idx=0, vis_num=1, mask_index=1, vis_num_pc=1, pca_rank=1,
                                                        null_space_projection=True, pca_rank_null=2)
    torch.manual_seed(5)
    lat, x0 = run(ed)
    assert x0.dtype == torch.uint8 and tuple(x0.shape) == (3, 64, 64, 3)
    cache = os.path.join(ed.result_folder, "null_text-0.pt")
    report = os.path.join(ed.result_folder, f"{ed.EXP_NAME}_null_text.json")
    assert os.path.exists(cache) and os.path.exists(report) and os.path.exists(os.path.join(ed.result_folder, f"{ed.EXP_NAME}.png"))
    rep = json.load(open(report))
    assert rep["cached"] is False and rep["steps"] == 10 and len(rep["per_step"]) == 10
    assert all(1 <= s["inner_steps_used"] <= 2 and s["last_loss"] is not None for s in rep["per_step"])
    ps = rep["psnr_vs_autoencoder_round_trip"]
    print(f"driver: PSNR vs the autoencoder's round trip, null-text {ps['null_text']:.2f} dB, plain guided {ps['plain_guided']:.2f} dB, "
          f"{rep['seconds']:.2f} s")
    import math
    assert all(math.isfinite(ps[k]) for k in ("null_text", "plain_guided"))
    ed2 = _edit(c, tmp_path, "bf16x3", **kw)
    ed2.run_DDIMinversion = None                                 # the cache serves: nothing is inverted
    torch.manual_seed(5)
    lat2, x02 = run(ed2)
    assert json.load(open(report))["cached"] is True and torch.equal(x02, x0)
    # the sega branch of the semantic driver decodes with the per-step states too, and says so
    ed3 = _edit(c, tmp_path, "bf16x3", **dict(kw, use_sega=True))
    ls, xs = ed3.run_edit_null_space_projection_zt_semantic(op="mid", block_idx=0, vis_num=1, mask_index=1, vis_num_pc=1, pca_rank=1)
    assert tuple(xs.shape) == (1, 64, 64, 3) and ed3._nt_embs is not None
    assert json.load(open(os.path.join(ed3.result_folder, f"{ed3.EXP_NAME}_null_text.json")))["cached"] is True
    zt, _, _ = ed3._prepare(1)[:3]
    plain = ed3.DDIMforwardsteps(zt, ed3.edit_t_idx, -1, ed3.for_prompt_emb, ed3.edit_prompt_emb, ed3.null_prompt_emb,
                                 mode="null+(for-null)+(edit-null)")[0]
    assert not torch.equal(plain, ls)                            # (the one null prompt decodes another frame)
    # other settings, or another image behind the same index, do not load the cache
    ed4 = _edit(c, tmp_path, "bf16x3", **dict(kw, null_text_lr=2e-2))
    ed4._zT()
    assert ed4._nt_report["cached"] is False and ed4._nt_report["lr"] == 2e-2
    ed5 = _edit(c, tmp_path, "bf16x3", **dict(kw, null_text_lr=2e-2, dataset=[image.flip(-1)]))
    ed5._zT()
    assert ed5._nt_report["cached"] is False
