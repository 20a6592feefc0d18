"""The drivers under ``--solver krylov`` / ``LOCO_SOLVER=krylov`` on the tiny configurations: the unconditional
``run_edit_null_space_projection`` through the command line, and the DeepFloyd IF, Stable Diffusion and LCM T-LOCO entry
points on their classes.  Each completes, writes the basis files it writes under the power solver, and next to every
basis it solved for a ``<basis name>_residual.json`` with the Krylov solver's residuals."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_latent import _edit_sd      # noqa: E402
from test_gpu_lcm import _edit_lcm, nets      # noqa: E402,F401  (the stand-in networks of the LCM tests, as a fixture here)
from test_gpu_tloco import _edit      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _residuals(path, k):
    assert os.path.exists(path), path
    d = json.load(open(path))
    assert d["solver"] == "krylov" and len(d["residual"]) == k and d["reason"] in ("invariant", "converged", "full", "max_iter")
    assert all(r == r and 0.0 <= r < 1.0 for r in d["residual"]) and d["rows"] % k == 0
    return d


def test_cli_tiny_config_with_the_krylov_solver(tmp_path, monkeypatch):
    from loco_edit_amd.main import main
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("LOCO_PRECISION", "bf16x3")
    monkeypatch.setenv("LOCO_SOLVER", "power")          # --solver overwrites it; restored when the test ends
    xt = main(["--sh_file_name", "main_celeba_hf_null_space_projection.sh", "--sample_idx", "3", "--device", DEV,
               "--dtype", "fp32", "--seed", "11", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Synthetic",
               "--unet_preset", "tiny_ddpm", "--synthetic_weights", "0", "--for_steps", "100", "--inv_steps", "100",
               "--use_yh_custom_scheduler", "True", "--x_space_guidance_edit_step", "1", "--x_space_guidance_scale", "0.5",
               "--x_space_guidance_num_step", "16", "--edit_t", "0.6", "--performance_boosting_t", "0.2",
               "--choose_sem", "l_eye", "--null_space_projection", "True", "--use_mask", "True", "--pca_rank_null", "2",
               "--pca_rank", "2", "--vis_num", "2", "--run_edit_null_space_projection", "True", "--solver", "krylov"])
    assert os.environ["LOCO_SOLVER"] == "krylov" and xt.shape == (5, 3, 32, 32)
    bdir = tmp_path / "runs" / "CelebA_HQ_HF-Synthetic" / "results" / "sample_idx3" / "basis" / "local_basis-0.6T-select-mask-l_eye"
    vm, vn = (torch.load(bdir / f, map_location="cpu") for f in ("vT-modify-pca-rank-2.pt", "vT-null-2.pt"))
    assert tuple(vm.shape) == tuple(vn.shape) == (2, 3 * 32 * 32)
    for v in (vm, vn):
        assert (v.double() @ v.double().T - torch.eye(2, dtype=torch.float64)).abs().max().item() < 2e-5
    _residuals(str(bdir / "vT-modify-pca-rank-2_residual.json"), 2)
    _residuals(str(bdir / "vT-null-2_residual.json"), 2)


def test_if_driver_with_the_krylov_solver(golden, tmp_path, monkeypatch):
    monkeypatch.setenv("LOCO_SOLVER", "krylov")
    ed = _edit(golden("tloco_tiny"), tmp_path, "bf16x3")
    masks = torch.zeros(2, 1, 32, 32, dtype=torch.bool)
    masks[1, 0, 12:20, 8:18] = True
    os.makedirs(os.path.join(ed.result_folder, "mask"))
    torch.save(masks, os.path.join(ed.result_folder, "mask", "mask.pt"))
    torch.manual_seed(5)
    x0 = ed.run_edit_null_space_projection_xt(op="mid", block_idx=0, vis_num=2, mask_index=1, vis_num_pc=1, pca_rank=1,
                                              null_space_projection=True, pca_rank_null=2)
    assert x0.dtype == torch.uint8 and tuple(x0.shape) == (5, 32, 32, 3)
    bdir = os.path.join(ed.result_folder, "basis", "local_basis-0.6T-pca-rank-1-select-mask1")
    for f in ("u-modify.pt", "vT-modify.pt", "u-null-null_space_rank_2.pt", "vT-null-null_space_rank_2.pt"):
        assert os.path.exists(os.path.join(bdir, f)), f
    _residuals(os.path.join(bdir, "vT-modify_residual.json"), 1)
    _residuals(os.path.join(bdir, "vT-null-null_space_rank_2_residual.json"), 2)


def test_sd_driver_with_the_krylov_solver(golden, tmp_path, monkeypatch):
    monkeypatch.setenv("LOCO_SOLVER", "krylov")
    ed = _edit_sd(golden("tloco_sd_tiny"), tmp_path, "bf16x3")
    masks = torch.zeros(2, 1, 64, 64, dtype=torch.bool)
    masks[1, 0, 20:40, 12:44] = True
    os.makedirs(os.path.join(ed.result_folder, "mask"))
    torch.save(masks, os.path.join(ed.result_folder, "mask", "mask.pt"))
    torch.manual_seed(5)
    lat, x0 = ed.run_edit_null_space_projection_zt(op="mid", block_idx=0, vis_num=2, mask_index=1, vis_num_pc=1, pca_rank=1,
                                                   null_space_projection=True, pca_rank_null=2)
    assert x0.dtype == torch.uint8 and tuple(x0.shape) == (5, 64, 64, 3) and tuple(lat.shape) == (5, 4, 16, 16)
    bdir = os.path.join(ed.result_folder, "basis", "local_basis-0.7T-pca-rank-1-select-mask1")
    for f in ("u-modify.pt", "vT-modify.pt", "u-null-null_space_rank_2.pt", "vT-null-null_space_rank_2.pt"):
        assert os.path.exists(os.path.join(bdir, f)), f
    assert tuple(torch.load(os.path.join(bdir, "u-modify.pt"), map_location="cpu").shape) == (int(masks[1].sum()) * 3, 1)     # rows of J V: the decoded image
    _residuals(os.path.join(bdir, "vT-modify_residual.json"), 1)
    _residuals(os.path.join(bdir, "vT-null-null_space_rank_2_residual.json"), 2)


def test_lcm_driver_with_the_krylov_solver(nets, tmp_path, monkeypatch):      # noqa: F811
    """This driver keeps no basis files (as in the reference), so there is nothing for a residual file to stand next to:
    the solves' residuals are on the object."""
    monkeypatch.setenv("LOCO_SOLVER", "krylov")
    ed = _edit_lcm(nets, tmp_path, "bf16x3")
    os.makedirs(os.path.join(ed.result_folder, "mask"))
    masks = torch.zeros(3, 1, 64, 64, dtype=torch.bool)
    masks[1, 0, 20:40, 12:44] = True
    torch.save(masks, os.path.join(ed.result_folder, "mask", "mask.pt"))
    lat, frames = ed.run_edit_null_space_projection_zt(op="mid", block_idx=0, vis_num=1, mask_index=1, vis_num_pc=1, pca_rank=1,
                                                       edit_prompt="a man wearing glasses", null_space_projection=True,
                                                       pca_rank_null=2, non_semantic=True)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (3, 64, 64, 3)
    assert tuple(ed.last_vT.shape) == (1, nets["cfg"].n) and abs(float(ed.last_vT.norm()) - 1) < 1e-4
    info = ed.last_solver_info
    assert info["solver"] == "krylov" and len(info["residual"]) == 2 and all(0.0 <= r < 1.0 for r in info["residual"])
