"""GPU tests of the --mask_model_path branches that test_gpu_sam.py's Stable Diffusion run does not reach: the unconditional
driver's two sites (the sample of dataset 'Random', a dataset image) and the DeepFloyd IF driver's `_masks`, each on a stub
of the driver that supplies the image, with the tiny SAM of the end-to-end fixture (image size 64).  The rank-0 broadcast of
`segment_for_driver` is checked on stand-in sharders (the last two tests need no GPU work but share the fixtures)."""
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import mask_segmentation as ms  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(ROOT, "tests", "golden", "sam")


class _Solo:
    active, is_main = False, True

    def agree(self, v):
        return v


@pytest.fixture(scope="module")
def model():
    """(state dict, config, uint8 image [64, 64, 3]): the fixture's random SAM with its predicted IoU lifted above 0.88 and its
    logits steepened, so that the default filters pass something (as in test_gpu_sam.py's driver run)."""
    m = torch.load(os.path.join(GOLD, "end_to_end_model.pt"))
    sd = {k: v.clone() for k, v in m["state_dict"].items()}
    p = "mask_decoder.iou_prediction_head.proj_out."
    sd[p + "weight"] *= 0.05
    sd[p + "bias"] = sd[p + "bias"] * 0.05 + 0.94
    for i in range(4):
        for leaf in ("weight", "bias"):
            sd[f"mask_decoder.output_hypernetworks_mlps.{i}.proj_out.{leaf}"] *= 1000.0
    return sd, m["config"], m["image"][:64, 32:96].contiguous()


def _stub(tmp_path, model, **kw):
    sd, config, _ = model
    folder = tmp_path / "sam_model"
    if not folder.exists():
        folder.mkdir()
        (folder / "config.json").write_text(json.dumps(config))
        torch.save(sd, folder / "pytorch_model.bin")
    args = SimpleNamespace(mask_model_path=str(folder), device=torch.device(DEV), filter_mask=100, sampling_mode=False, mask_index=0,
                           sample_idx=0)
    run = tmp_path / kw.pop("run")
    run.mkdir()
    return SimpleNamespace(args=args, result_folder=str(run), sharder=_Solo(), _exists=lambda p: bool(p) and os.path.exists(p),
                           _load=torch.load, c_in=3, image_size=64, dtype=torch.float32, device="cpu", sampling_mode=False, **kw)


def _check_cache(stub, mask):
    saved = torch.load(os.path.join(stub.result_folder, "mask", "mask.pt"))
    assert saved.dtype == torch.bool and saved.dim() == 3 and tuple(saved.shape[1:]) == (64, 64) and saved.shape[0] >= 1
    assert os.path.exists(os.path.join(stub.result_folder, "mask", "total_mask.png"))
    if mask is not None:
        assert mask.dtype == torch.bool and tuple(mask.shape) == (3, 64, 64) and torch.equal(mask, saved[0].repeat(3, 1, 1))
    return saved


def test_unconditional_driver_segments_sample_and_dataset_image(tmp_path, model):
    from loco_edit_amd.edit import EditUncondDiffusion
    x0 = (model[2].float() / 127.5 - 1).permute(2, 0, 1)[None]                 # [1, 3, 64, 64] in [-1, 1], what the sampler returns
    calls = []

    def sampler(xT, t_start_idx, t_end_idx):
        calls.append((t_start_idx, t_end_idx))
        return x0
    rnd = _stub(tmp_path, model, run="random", dataset_name="Random", DDIMforwardsteps=sampler)
    rnd._segment = lambda fn: EditUncondDiffusion._segment(rnd, fn)
    xT, mask = EditUncondDiffusion._get_xT_and_mask(rnd, 0, True)
    assert calls == [(0, -1)] and rnd.EXP_NAME == "original" and tuple(xT.shape) == (1, 3, 64, 64)
    first = _check_cache(rnd, mask)
    EditUncondDiffusion._get_xT_and_mask(rnd, 0, True)                          # the cache wins: no second sample
    assert calls == [(0, -1)]
    data = _stub(tmp_path, model, run="dataset", dataset_name="FFHQ", dataset=[x0], run_DDIMinversion=lambda idx: x0 * 0)
    data._segment = lambda fn: EditUncondDiffusion._segment(data, fn)
    _, mask = EditUncondDiffusion._get_xT_and_mask(data, 0, True)
    assert torch.equal(_check_cache(data, mask), first)                         # the same image either way


def test_if_driver_segments_the_image_it_is_given(tmp_path, model):
    from loco_edit_amd.tloco import EditDeepFloydIF
    stub = _stub(tmp_path, model, run="if")
    masks = EditDeepFloydIF._masks(stub, lambda: model[2].numpy(), 64)
    assert torch.equal(_check_cache(stub, None), masks)
    assert torch.equal(EditDeepFloydIF._masks(stub, lambda: 1 / 0, 64), masks)  # cached now: the image is not produced again


class _Rank:
    """A rank of two: `agree` hands out what rank 0 put in."""
    active = True

    def __init__(self, is_main, wire):
        self.is_main, self.wire = is_main, wire

    def agree(self, v):
        if self.is_main:
            self.wire.append(v)
        return self.wire[0]


def test_rank_0_segments_and_the_others_receive(tmp_path, model):
    stub = _stub(tmp_path, model, run="ranks")
    wire, made = [], []

    def image():
        made.append(1)
        return model[2].numpy()
    m0 = ms.segment_for_driver(stub.args, stub.result_folder, _Rank(True, wire), image, 64)
    seen = os.listdir(os.path.join(stub.result_folder, "mask"))
    other = SimpleNamespace(mask_model_path="/nowhere", device=torch.device(DEV), filter_mask=100)   # rank 1 never loads the model
    m1 = ms.segment_for_driver(other, stub.result_folder, _Rank(False, wire), image, 64)
    assert len(made) == 2 and torch.equal(m0, m1) and m1.dtype == torch.bool
    assert os.listdir(os.path.join(stub.result_folder, "mask")) == seen        # and writes nothing


def test_a_failure_on_rank_0_raises_on_every_rank(tmp_path):
    wire = []
    args = SimpleNamespace(mask_model_path=str(tmp_path / "nowhere"), device=torch.device(DEV), filter_mask=100)
    for is_main in (True, False):
        with pytest.raises(RuntimeError, match="rank 0 could not segment the image: FileNotFoundError"):
            ms.segment_for_driver(args, str(tmp_path), _Rank(is_main, wire), lambda: None, 64)
