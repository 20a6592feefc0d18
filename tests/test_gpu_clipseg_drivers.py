"""GPU tests of the --mask_prompts branches of the drivers, with a CLIPSeg folder written from the seg_a fixture (tower run at
48, logits 48 x 48): the unconditional driver's two sites and the DeepFloyd IF driver's `_masks` on the stubs of
test_gpu_sam_drivers.py, and one end-to-end run_edit_null_space_projection on the tiny DDPM whose mask comes from a prompt."""
import json
import os
import shutil
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import prompt_mask as pm  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(ROOT, "tests", "golden", "clipseg")
TOK = os.path.join(ROOT, "tests", "golden", "clip_text", "tokenizer_sd1")
PROMPTS = "hair,the eyes,a smiling mouth"


class _Solo:
    active, is_main = False, True

    def agree(self, v):
        return v


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """A CLIPSegForImageSegmentation folder as a user would have it: config, weights, preprocessor, tokenizer files."""
    g = torch.load(os.path.join(GOLD, "seg_a.pt"))
    d = tmp_path_factory.mktemp("clipseg_model")
    (d / "config.json").write_text(json.dumps(g["config"]))
    (d / "preprocessor_config.json").write_text(json.dumps(g["preprocessor"]))
    torch.save({k: (v.float() if v.is_floating_point() else v) for k, v in g["state_dict"].items()}, d / "pytorch_model.bin")
    for f in os.listdir(TOK):
        shutil.copy(os.path.join(TOK, f), d / f)
    return str(d), g["frames"][0, :, :40].contiguous()             # and a uint8 image [40, 40, 3]


@pytest.fixture(scope="module")
def masker(folder):
    return pm.load_prompt_masker(folder[0], device=torch.device(DEV), max_masks=3)


def _stub(tmp_path, folder, run, mask_index=0, **kw):
    args = SimpleNamespace(mask_model_path="", mask_prompt_model_path=folder[0], mask_prompts=PROMPTS, mask_prompt_threshold=0.5,
                           tokenizer_path="", device=torch.device(DEV), filter_mask=10, sampling_mode=False, mask_index=mask_index,
                           sample_idx=0)
    d = tmp_path / run
    d.mkdir()
    return SimpleNamespace(args=args, result_folder=str(d), sharder=_Solo(), _exists=lambda p: bool(p) and os.path.exists(p),
                           _load=torch.load, c_in=3, image_size=40, dtype=torch.float32, device="cpu", sampling_mode=False, **kw)


def _check_cache(stub, mask, masker, image):
    saved = torch.load(os.path.join(stub.result_folder, "mask", "mask.pt"))
    assert saved.dtype == torch.bool and tuple(saved.shape) == (3, 40, 40)                 # N = the number of prompts
    assert torch.equal(saved, masker.masks(image[None], pm.parse_prompts(PROMPTS), 40, 0.5).cpu())
    rec = json.loads(open(os.path.join(stub.result_folder, "mask", "mask_prompts.json")).read())
    assert [r["prompt"] for r in rec] == pm.parse_prompts(PROMPTS)
    assert all(abs(r["area_share"] - float(m.sum()) / 1600) < 1e-12 and r["logit_min"] < r["logit_max"] for r, m in zip(rec, saved))
    assert os.path.exists(os.path.join(stub.result_folder, "mask", "total_mask.png"))
    if mask is not None:
        assert mask.dtype == torch.bool and torch.equal(mask, saved[stub.args.mask_index].repeat(3, 1, 1))
    return saved


def test_unconditional_driver_prompts_the_sample_and_the_dataset_image(tmp_path, folder, masker, monkeypatch):
    from loco_edit_amd.edit import EditUncondDiffusion
    image = folder[1]
    x0 = (image.float() / 127.5 - 1).permute(2, 0, 1)[None]                                # what the sampler returns
    image = ((x0 / 2 + 0.5).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1)[0]        # and what the driver makes of it
    calls = []

    def sampler(xT, t_start_idx, t_end_idx):
        calls.append((t_start_idx, t_end_idx))
        return x0
    rnd = _stub(tmp_path, folder, "random", mask_index=1, dataset_name="Random", DDIMforwardsteps=sampler)
    rnd._segment = lambda fn: EditUncondDiffusion._segment(rnd, fn)
    xT, mask = EditUncondDiffusion._get_xT_and_mask(rnd, 0, True)
    assert calls == [(0, -1)] and rnd.EXP_NAME == "original" and tuple(xT.shape) == (1, 3, 40, 40)
    first = _check_cache(rnd, mask, masker, image)                                         # --mask_index 1 picked the second prompt
    monkeypatch.setattr(pm, "load_prompt_masker", lambda *a, **k: 1 / 0)                  # the cache wins: no model, no second sample
    _, again = EditUncondDiffusion._get_xT_and_mask(rnd, 0, True)
    assert calls == [(0, -1)] and torch.equal(again, mask)
    monkeypatch.undo()
    data = _stub(tmp_path, folder, "dataset", mask_index=2, dataset_name="FFHQ", dataset=[x0], run_DDIMinversion=lambda idx: x0 * 0)
    data._segment = lambda fn: EditUncondDiffusion._segment(data, fn)
    _, mask = EditUncondDiffusion._get_xT_and_mask(data, 0, True)
    assert torch.equal(_check_cache(data, mask, masker, image), first)                     # the same image either way


def test_if_driver_prompts_the_image_it_is_given(tmp_path, folder, masker, monkeypatch):
    from loco_edit_amd.tloco import EditDeepFloydIF
    stub = _stub(tmp_path, folder, "if")
    masks = EditDeepFloydIF._masks(stub, lambda: folder[1].numpy(), 40)
    assert torch.equal(_check_cache(stub, None, masker, folder[1]), masks)
    monkeypatch.setattr(pm, "load_prompt_masker", lambda *a, **k: 1 / 0)
    assert torch.equal(EditDeepFloydIF._masks(stub, lambda: 1 / 0, 40), masks)            # cached: neither image nor model again


def test_null_space_projection_with_a_prompted_mask(tmp_path, folder):
    from argparse import Namespace
    from loco_edit_amd.config import TINY_DDPM
    from loco_edit_amd.edit import EditUncondDiffusion
    os.environ.pop("WORLD_SIZE", None)
    cfg = TINY_DDPM
    args = Namespace(device=torch.device(DEV), dtype=torch.float32, seed=1, model_name="tiny", unet_config=cfg, synthetic_weights=0,
                     ckpt_path="", max_batch=8, image_size=cfg.resolution, c_in=3, dataset_name="Random", dataset_root="", for_steps=100,
                     inv_steps=100, use_yh_custom_scheduler=True, edit_t=0.6, performance_boosting_t=0.2, x_space_guidance_edit_step=1.0,
                     x_space_guidance_scale=0.5, x_space_guidance_num_step=16, result_folder=str(tmp_path), sample_idx=0, vT_path="",
                     vT1_path="", choose_sem="l_eye", mask_index=1, sampling_mode=False, mask_model_path="",
                     mask_prompt_model_path=folder[0], mask_prompts=PROMPTS, mask_prompt_threshold=0.5, tokenizer_path="", filter_mask=10)
    ed = EditUncondDiffusion(args)
    seen = []
    sample = ed.DDIMforwardsteps

    def spy(xT, t_start_idx, t_end_idx, **kw):
        out = sample(xT, t_start_idx=t_start_idx, t_end_idx=t_end_idx, **kw)
        if (t_start_idx, t_end_idx) == (0, -1) and not seen:
            seen.append(out.detach().clone())
        return out
    ed.DDIMforwardsteps = spy
    xt = ed.run_edit_null_space_projection(idx=0, vis_num=2, vis_num_pc=1, pca_rank=1, pca_rank_null=3, null_space_projection=True,
                                           use_mask=True)
    assert xt.shape == (5, 3, cfg.resolution, cfg.resolution) and bool(torch.isfinite(xt).all())
    saved = torch.load(os.path.join(ed.result_folder, "mask", "mask.pt"))
    assert saved.dtype == torch.bool and tuple(saved.shape) == (3, cfg.resolution, cfg.resolution)
    image = ((seen[0] / 2 + 0.5).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).cpu()
    mk = pm.load_prompt_masker(folder[0], device=torch.device(DEV), max_masks=3)
    assert torch.equal(saved, mk.masks(image, pm.parse_prompts(PROMPTS), cfg.resolution, 0.5).cpu())
