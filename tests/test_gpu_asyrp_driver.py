"""MI355X: the Asyrp driver end to end (main.py --run_edit_asyrp True) on TINY_DDPM (32^2, synthetic weights), the Synthetic
dataset and the tiny_a CLIP fixture: the first run trains on two images (20 timesteps each: T down to --edit_t 0.8 of the
100-step schedule), writes the checkpoint, the panel, _asyrp.json, _clip.json and _quality.json; a second run loads the checkpoint,
trains nothing and returns the same image bit for bit; the flag without --clip_model_path or without the prompts is refused."""
import importlib.util
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_spec = importlib.util.spec_from_file_location("gpu_clip_vision", os.path.join(ROOT, "tests", "test_gpu_clip_vision.py"))
_cv = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cv)
SRC, TGT = "a photo of a man", "a photo of a man wearing glasses"


def test_cli(tmp_path, monkeypatch):
    from loco_edit_amd.main import main
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    root = _cv.write_clip_folder(str(tmp_path / "tiny_a"), "tiny_a")
    rdir = tmp_path / "runs" / "CelebA_HQ_HF-Synthetic" / "results" / "sample_idx3"
    ckpt = tmp_path / "blocks" / "glasses.pt"
    base = ["--sh_file_name", "main_celeba_hf_asyrp.sh", "--sample_idx", "3", "--device", DEV, "--dtype", "fp32", "--seed", "11",
            "--model_name", "CelebA_HQ_HF", "--dataset_name", "Synthetic", "--unet_preset", "tiny_ddpm", "--synthetic_weights", "0",
            "--for_steps", "100", "--inv_steps", "100", "--use_yh_custom_scheduler", "True", "--performance_boosting_t", "0.2",
            "--edit_t", "0.8", "--max_batch", "2", "--run_edit_asyrp", "True", "--asyrp_train_idx", "0-1", "--asyrp_ckpt", str(ckpt),
            "--quality_metrics", "ssim"]
    pair = ["--asyrp_src_prompt", SRC, "--asyrp_tgt_prompt", TGT]
    with pytest.raises(ValueError, match="--run_edit_asyrp needs --clip_model_path"):
        main(base + pair)
    with pytest.raises(ValueError, match="--asyrp_src_prompt and --asyrp_tgt_prompt"):
        main(base + ["--clip_model_path", root])
    assert not ckpt.exists()
    out = main(base + pair + ["--clip_model_path", root])
    assert tuple(out.shape) == (1, 3, 32, 32) and bool(torch.isfinite(out).all())
    assert ckpt.exists()
    sd = torch.load(ckpt)
    assert sd["adam_step"] == 2 * 20 and sd["W2"].any() and tuple(sd["W1"].shape) == (64, 64)
    png = [n for n in os.listdir(rdir) if n.endswith("_asyrp.png")]
    assert len(png) == 1
    stem = png[0][:-len("_asyrp.png")]
    with open(rdir / f"{stem}_asyrp.json") as f:
        rec = json.load(f)
    assert rec["trained"] and rec["adam_steps"] == 40 and rec["learning_time_s"] > 0 and rec["transfer_edit_time_s"] > 0
    assert rec["src_prompt"] == SRC and rec["tgt_prompt"] == TGT
    with open(rdir / f"{stem}_clip.json") as f:
        clip = json.load(f)
    assert clip["edit_prompt"] == TGT and len(clip["frames"]) == 1 and clip["frames"][0]["directional"] is not None
    assert os.path.exists(rdir / f"{stem}_quality.json")
    print(f"learning {rec['learning_time_s']:.2f} s for 40 steps, transfer {rec['transfer_edit_time_s']:.2f} s; directional similarity of the edit "
          f"{clip['frames'][0]['directional']:.4f}")
    # the second run loads the block and trains nothing
    before = ckpt.stat().st_mtime_ns
    again = main(base + pair + ["--clip_model_path", root])
    with open(rdir / f"{stem}_asyrp.json") as f:
        rec2 = json.load(f)
    assert not rec2["trained"] and rec2["learning_time_s"] == 0 and rec2["adam_steps"] == 40
    assert ckpt.stat().st_mtime_ns == before
    assert torch.equal(again, out)
