"""GPU tests of --clip_model_path in the semantic T-LOCO drivers: the IF driver on the tiny stand-in of test_gpu_tloco.py and the
Stable Diffusion driver on tiny_ldm (and the LCM driver on its tiny stand-in), scored by the tiny_a CLIP fixture written to a temp
folder.  The JSON holds one record
per returned frame, the alpha = 0 record is the original, the numbers are ClipScorer.score's on the returned frames, and a
run without the flag writes no JSON and returns bit-equal frames."""
import glob
import importlib.util
import json
import os
import sys
from argparse import Namespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("clip_for", "clip_edit", "image_sim", "directional")


def _module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", f"{name}.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def clip_folder(tmp_path_factory):
    return _module("test_gpu_clip_vision").write_clip_folder(str(tmp_path_factory.mktemp("clip") / "tiny_a"), "tiny_a")


def _check_json(ed, frames, alphas):
    """The JSON of the run `ed` just made against its frames; -> the parsed JSON."""
    path = os.path.join(ed.result_folder, f"{ed.EXP_NAME}_clip.json")
    assert os.path.exists(path), os.listdir(ed.result_folder)
    with open(path) as f:
        js = json.load(f)
    assert js["clip_model_path"] == ed.args.clip_model_path and js["clip_preprocess"] == "device"
    assert js["for_prompt"] == ed.for_prompt and js["edit_prompt"] == ed.edit_prompt
    assert len(js["frames"]) == frames.shape[0]
    assert [r["alpha"] for r in js["frames"]] == alphas
    return js


def _same(a, b):
    return all((a[k] is None and b[k] is None) or abs(a[k] - b[k]) <= 1e-12 for k in KEYS)


def _if_edit(g, root, **kw):
    from loco_edit_amd.config import TINY_ADM
    from loco_edit_amd.tloco import EditDeepFloydIF
    os.environ.pop("WORLD_SIZE", None)
    a = dict(device=torch.device(DEV), dtype=torch.float32, seed=1, unet_config=TINY_ADM, synthetic_weights=0, ckpt_path="", max_batch=8,
             precision="bf16x3", dataset_name="Random", for_steps=100, use_yh_custom_scheduler=True, guidance_scale=g["guidance_scale"],
             guidance_scale_edit=g["guidance_scale_edit"], prompt_emb={"for": g["for_e"], "edit": g["edit_e"], "null": g["null_e"]},
             for_prompt="a photo of a man", edit_prompt="a photo of a man wearing glasses", edit_t=0.6, sampling_mode=False,
             tilda_v_score_type="null+(for-null)+(edit-null)", ablation_method="null-space-proj", mask_type="SAM", vT_path="",
             x_space_guidance_edit_step=1.0, x_space_guidance_scale=0.5, x_space_guidance_num_step=16, result_folder=str(root))
    a.update(kw)
    ed = EditDeepFloydIF(Namespace(**a))
    masks = torch.zeros(2, 1, 32, 32, dtype=torch.bool)
    masks[1, 0, 12:20, 8:18] = True
    os.makedirs(os.path.join(ed.result_folder, "mask"), exist_ok=True)
    torch.save(masks, os.path.join(ed.result_folder, "mask", "mask.pt"))
    return ed


def test_if_semantic_driver_writes_clip_scores(golden, tmp_path, clip_folder):
    g = golden("tloco_tiny")
    run = dict(op="mid", block_idx=0, vis_num=2, mask_index=1, vis_num_pc=1, pca_rank=1, null_space_projection=True, pca_rank_null=2,
               jacobian=True)
    frames = {}
    for flag in (True, False):
        ed = _if_edit(g, tmp_path / ("on" if flag else "off"), clip_model_path=clip_folder if flag else "")
        torch.manual_seed(5)
        frames[flag] = ed.run_edit_null_space_projection_xt_semantic(**run)
        if flag:
            on = ed
        else:
            assert ed._clip is None and not glob.glob(os.path.join(ed.result_folder, "*_clip.json"))
    assert tuple(frames[True].shape) == (5, 32, 32, 3) and torch.equal(frames[True], frames[False])
    js = _check_json(on, frames[True], [-8.0, -4.0, 0.0, 4.0, 8.0])
    assert js["original_frame"] is None
    want = on._clip.score(frames[True], 2, on.for_prompt, on.edit_prompt)
    for got, w in zip(js["frames"], want):
        print({k: got[k] for k in ("alpha",) + KEYS})
        assert _same(got, w)
    zero = js["frames"][2]
    assert abs(zero["image_sim"] - 1) <= 1e-6 and zero["directional"] is None
    assert all(r["directional"] is not None for i, r in enumerate(js["frames"]) if i != 2)
    scorer = on._clip
    # sega returns no unedited frame: xt is decoded once more, only when the scores are on
    xs = {}
    for flag in (True, False):
        ed = _if_edit(g, tmp_path / ("sega_on" if flag else "sega_off"), ablation_method="sega", clip_model_path=clip_folder if flag else "")
        if flag:
            ed._clip = scorer                                            # (one scorer serves the test)
        torch.manual_seed(5)
        xs[flag] = ed.run_edit_null_space_projection_xt_semantic(op="mid", block_idx=0, vis_num=2, mask_index=1, vis_num_pc=1, pca_rank=1)
        pngs = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ed.result_folder, "*.png")))
        if flag:
            js = _check_json(ed, xs[flag], [None])
            assert abs(js["original_frame"]["image_sim"] - 1) <= 1e-6 and js["original_frame"]["directional"] is None
            assert js["frames"][0]["directional"] is not None
            assert any(p.endswith("_clip_original_stage1.png") for p in pngs)
        else:
            assert not glob.glob(os.path.join(ed.result_folder, "*_clip*"))
    assert tuple(xs[True].shape) == (1, 32, 32, 3) and torch.equal(xs[True], xs[False])


def test_sd_semantic_driver_writes_clip_scores(tmp_path, clip_folder):
    from loco_edit_amd.tloco_sd import EditStableDiffusion
    sd_args = _module("test_gpu_text_encoder")._sd_args
    os.environ.pop("WORLD_SIZE", None)
    frames = {}
    for flag in (True, False):
        root = tmp_path / ("on" if flag else "off")
        ed = EditStableDiffusion(sd_args(root, clip_model_path=clip_folder if flag else ""))
        masks = torch.zeros(3, 1, 64, 64, dtype=torch.bool)
        masks[1, 0, 20:40, 12:44] = True
        os.makedirs(os.path.join(ed.result_folder, "mask"), exist_ok=True)
        torch.save(masks, os.path.join(ed.result_folder, "mask", "mask.pt"))
        torch.manual_seed(5)
        _, frames[flag] = ed.run_edit_null_space_projection_zt_semantic(op="mid", block_idx=0, vis_num=1, mask_index=1, vis_num_pc=1,
                                                                        pca_rank=1, null_space_projection=True, pca_rank_null=2)
        if flag:
            on = ed
        else:
            assert ed._clip is None and not glob.glob(os.path.join(ed.result_folder, "*_clip.json"))
    assert tuple(frames[True].shape) == (3, 64, 64, 3) and torch.equal(frames[True], frames[False])
    js = _check_json(on, frames[True], [-8.0, 0.0, 8.0])
    want = on._clip.score(frames[True], 1, on.for_prompt, on.edit_prompt)
    for got, w in zip(js["frames"], want):
        print({k: got[k] for k in ("alpha",) + KEYS})
        assert _same(got, w)
    assert abs(js["frames"][1]["image_sim"] - 1) <= 1e-6 and js["frames"][1]["directional"] is None
    assert js["frames"][0]["directional"] is not None and js["frames"][2]["directional"] is not None


def test_lcm_driver_writes_clip_scores(tmp_path, clip_folder):
    """The LCM driver (semantic direction, then use_sega): its sampler draws noise from the global generator, so the unedited
    latent of the sega run is decoded after the edit and the flagged run's frames stay those of the run without scores."""
    from loco_edit_amd.config import TINY_DECODER, TINY_LCM
    from loco_edit_amd.tloco_lcm import EditLatentConsistency
    os.environ.pop("WORLD_SIZE", None)
    g = torch.Generator().manual_seed(47)
    ctx, ctx2 = (torch.randn(1, TINY_LCM.context_len, TINY_LCM.context_dim, generator=g) for _ in range(2))
    run = dict(op="mid", block_idx=0, vis_num=1, mask_index=1, vis_num_pc=1, pca_rank=1, edit_prompt="a man wearing glasses",
               null_space_projection=True, pca_rank_null=2, non_semantic=False)
    frames, sega = {}, {}
    for flag in (True, False):
        args = Namespace(device=torch.device(DEV), dtype=torch.float32, seed=1, unet_config=TINY_LCM, vae_config=TINY_DECODER,
                         synthetic_weights=0, ckpt_path="", vae_ckpt_path="", max_batch=8, precision="bf16x3", dataset_name="Random",
                         for_steps=100, use_yh_custom_scheduler=False, guidance_scale=7.5, guidance_scale_edit=7.5,
                         prompt_emb={"for": ctx, "edit": ctx2, "null": torch.zeros_like(ctx)}, for_prompt="a man",
                         edit_prompt="a man wearing glasses", edit_t=1.0, sampling_mode=False,
                         tilda_v_score_type="null+(for-null)+(edit-null)", ablation_method=None, mask_type="SAM", vT_path="", use_sega=False,
                         x_space_guidance_edit_step=1.0, x_space_guidance_scale=0.5, x_space_guidance_num_step=2, num_inference_steps=4,
                         edit_t_idx=2, lcm_timesteps="linspace", result_folder=str(tmp_path / ("on" if flag else "off")),
                         clip_model_path=clip_folder if flag else "")
        ed = EditLatentConsistency(args)
        masks = torch.zeros(3, 1, 64, 64, dtype=torch.bool)
        masks[1, 0, 20:40, 12:44] = True
        os.makedirs(os.path.join(ed.result_folder, "mask"))
        torch.save(masks, os.path.join(ed.result_folder, "mask", "mask.pt"))
        torch.manual_seed(5)
        _, frames[flag] = ed.run_edit_null_space_projection_zt(**run)
        if flag:
            js = _check_json(ed, frames[flag], [-1.0, 0.0, 1.0])
            want = ed._clip.score(frames[flag], 1, ed.for_prompt, ed.edit_prompt)
            assert all(_same(a, b) for a, b in zip(js["frames"], want))
            assert abs(js["frames"][1]["image_sim"] - 1) <= 1e-6 and js["frames"][1]["directional"] is None
        ed.use_sega = True
        torch.manual_seed(6)
        _, sega[flag] = ed.run_edit_null_space_projection_zt(**run)
        if flag:
            js = _check_json(ed, sega[flag], [None])
            assert abs(js["original_frame"]["image_sim"] - 1) <= 1e-6 and js["frames"][0]["directional"] is not None
        else:
            assert ed._clip is None and not glob.glob(os.path.join(ed.result_folder, "*_clip*"))
    assert tuple(frames[True].shape) == (3, 64, 64, 3) and torch.equal(frames[True], frames[False])
    assert tuple(sega[True].shape) == (1, 64, 64, 3) and torch.equal(sega[True], sega[False])
