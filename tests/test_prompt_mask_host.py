"""Host tests of the text-prompted masks (prompt_mask.py, the --mask_prompts flags, the dispatch of segment_for_driver): no GPU.
The float64 restatements checked here are the yardsticks of tests/test_gpu_clipseg.py."""
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import define_argparser as da  # noqa: E402
from loco_edit_amd import mask_segmentation as ms  # noqa: E402
from loco_edit_amd import prompt_mask as pm  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "clipseg")


def _gold(name):
    g = torch.load(os.path.join(GOLD, f"{name}.pt"))
    ref = os.path.join(GOLD, f"{name}_ref.pt")
    if os.path.exists(ref):
        g.update(torch.load(ref))
    g["state_dict"] = {k: (v.float() if v.is_floating_point() else v) for k, v in g["state_dict"].items()}
    return g


# ------------------------------------------------------------------------------------------------------------------- parser
def test_parser_takes_the_flags_and_their_defaults():
    a = da.parse_args([])
    assert a.mask_prompts == "" and a.mask_prompt_model_path == "" and a.mask_prompt_threshold == 0.5
    a = da.parse_args(["--mask_prompts", "hair, eyes,mouth", "--mask_prompt_model_path", "/models/clipseg", "--mask_index", "2",
                       "--mask_prompt_threshold", "0.4"])
    assert pm.parse_prompts(a.mask_prompts) == ["hair", "eyes", "mouth"] and a.mask_index == 2 and a.mask_prompt_threshold == 0.4
    assert ms.wants_segmentation(a) and not ms.wants_segmentation(da.parse_args([]))
    assert ms.wants_segmentation(da.parse_args(["--mask_model_path", "/models/sam"]))
    # the new flags come last: the order of the earlier ones is untouched
    names = [x.dest for x in da.build_parser()._actions]
    assert names[-3:] == ["mask_prompts", "mask_prompt_model_path", "mask_prompt_threshold"]


@pytest.mark.parametrize("argv, message", [
    (["--mask_prompts", "hair", "--mask_prompt_model_path", "/m", "--mask_model_path", "/sam"], "pass one"),
    (["--mask_prompts", "hair"], "needs --mask_prompt_model_path"),
    (["--mask_prompt_model_path", "/m"], "needs --mask_prompts"),
    (["--mask_prompts", "hair,eyes", "--mask_prompt_model_path", "/m", "--mask_index", "2"], "beyond the 2 prompts"),
    (["--mask_prompts", "hair,eyes", "--mask_prompt_model_path", "/m", "--mask_index", "-1"], "beyond the 2 prompts"),
    (["--mask_prompts", "hair,,eyes", "--mask_prompt_model_path", "/m"], "entry 1 .* is empty"),
    (["--mask_prompts", "hair, ", "--mask_prompt_model_path", "/m"], "entry 1 .* is empty"),
    (["--mask_prompts", "hair", "--mask_prompt_model_path", "/m", "--mask_prompt_threshold", "1.0"], "outside \\(0, 1\\)"),
])
def test_parser_refuses(argv, message):
    with pytest.raises(ValueError, match=message):
        da.parse_args(argv)


def test_prompt_list_parsing():
    assert pm.parse_prompts("hair") == ["hair"]
    assert pm.parse_prompts(" a red car ,the sky") == ["a red car", "the sky"]
    assert pm.parse_prompts(["x ", "y"]) == ["x", "y"]
    for bad in ("", "  ", ",", "a,"):
        with pytest.raises(ValueError):
            pm.parse_prompts(bad)
    assert pm.threshold_logit(0.5) == 0.0 and abs(pm.threshold_logit(0.25) + 1.0986122886681098) < 1e-15


# --------------------------------------------------------------------------------------------------------------- checkpoint
@pytest.mark.parametrize("name", ["seg_a", "seg_b"])
def test_checkpoint_split_and_config_inference(name, tmp_path):
    g = _gold(name)
    c, vc = g["config"], g["config"]["vision_config"]
    parts = pm.parts_from_state_dict(g["state_dict"], c, g["preprocessor"], "tok", max_masks=5)
    S = g["run_size"]
    assert parts.native_size == vc["image_size"] and parts.vision_cfg.image_size == S == parts.preprocess.size
    assert parts.preprocess.resample == g["preprocessor"]["resample"] and parts.preprocess.image_mean == pm.IMAGENET_MEAN
    d = parts.decoder_cfg
    assert (d.width, d.grid, d.patch_size) == (vc["hidden_size"], S // vc["patch_size"], vc["patch_size"])
    assert (d.reduce_dim, d.heads, d.ffn, d.n_taps) == (c["reduce_dim"], c["decoder_num_attention_heads"], c["decoder_intermediate_size"],
                                                        len(c["extract_layers"]))
    assert (d.conditional_layer, d.projection_dim, d.complex_head, d.max_masks) == (c["conditional_layer"], c["projection_dim"],
                                                                                   c["use_complex_transposed_convolution"], 5)
    assert d.logit_size == g["logits64"].shape[-1] and parts.extract_layers == tuple(c["extract_layers"])
    # every key lands in exactly one part
    n_clip = sum(k.startswith("clip.") and not k.endswith(("logit_scale", "position_ids")) for k in g["state_dict"])
    assert len(parts.vision_sd) + len(parts.text_sd) + 1 == n_clip
    assert set(parts.decoder_sd) == set(pm.decoder_param_shapes(d)) == {k[8:] for k in g["state_dict"] if k.startswith("decoder.")}
    assert tuple(parts.text_projection.shape) == (c["projection_dim"], c["text_config"]["hidden_size"])
    # the same from a folder; preprocessor_config.json absent: 352, bicubic, ImageNet
    folder = tmp_path / "model"
    folder.mkdir()
    (folder / "config.json").write_text(json.dumps(c))
    torch.save(g["state_dict"], folder / "pytorch_model.bin")
    bare = pm.read_clipseg_checkpoint(str(folder))
    assert bare.preprocess == pm.Preprocess(352, 3, pm.IMAGENET_MEAN, pm.IMAGENET_STD) and bare.decoder_cfg.grid == 352 // vc["patch_size"]
    (folder / "preprocessor_config.json").write_text(json.dumps(g["preprocessor"]))
    again = pm.read_clipseg_checkpoint(str(folder), max_masks=5)
    assert again.decoder_cfg == d and again.vision_cfg == parts.vision_cfg and again.tokenizer_dir is None
    (folder / "preprocessor_config.json").write_text(json.dumps(dict(g["preprocessor"], resample=0)))
    with pytest.raises(ValueError, match="resample 0 is not supported"):
        pm.read_clipseg_checkpoint(str(folder))
    with pytest.raises(FileNotFoundError, match="nothing is downloaded"):
        pm.read_clipseg_checkpoint("CIDAS/clipseg-rd64-refined")
    with pytest.raises(ValueError, match="foreign keys"):
        pm.parts_from_state_dict(dict(g["state_dict"], **{"head.weight": torch.zeros(1)}), c)
    broken = {k: v for k, v in g["state_dict"].items() if k != "decoder.film_add.bias"}
    with pytest.raises(ValueError, match="missing keys of the CLIPSeg decoder"):
        pm.parts_from_state_dict(broken, c)


@pytest.mark.parametrize("name", ["seg_a", "seg_b"])
def test_position_table_is_the_one_transformers_adds(name):
    g = _gold(name)
    parts = pm.parts_from_state_dict(g["state_dict"], g["config"], g["preprocessor"])
    got = parts.vision_sd["embeddings.position_embedding.weight"]
    assert got.dtype == torch.float32 and torch.equal(got, g["position_table"])
    native = g["state_dict"]["clip.vision_model.embeddings.position_embedding.weight"]
    assert got.shape[0] != native.shape[0] and torch.equal(got[0], native[0])                  # the class row is kept
    same = pm.parts_from_state_dict(g["state_dict"], g["config"], g["preprocessor"], run_size=g["config"]["vision_config"]["image_size"])
    assert torch.equal(same.vision_sd["embeddings.position_embedding.weight"], native)           # native size: unchanged


# ------------------------------------------------------------------------------------------------------------- restatements
@pytest.mark.parametrize("resample, mode", [(2, "bilinear"), (3, "bicubic")])
@pytest.mark.parametrize("n_in, n_out", [(40, 48), (56, 48), (200, 144), (120, 144), (48, 48), (7, 31), (97, 5)])
def test_resize_restatement_is_torch_antialiased_interpolate(resample, mode, n_in, n_out):
    x = torch.rand(2, 3, n_in, 9, dtype=torch.float64, generator=torch.Generator().manual_seed(n_in))
    want = F.interpolate(x, size=(n_out, 9), mode=mode, antialias=True, align_corners=False)
    got = torch.einsum("oh,nchw->ncow", pm.resize_matrix(n_in, n_out, resample), x)
    assert float((got - want).abs().max()) <= 1e-13
    rows = pm.resize_matrix(n_in, n_out, resample).sum(dim=1)
    assert float((rows - 1).abs().max()) <= 1e-14


def test_preprocess_restatement_resizes_each_axis_on_its_own():
    g = _gold("seg_a")
    pre = pm.Preprocess(size=48, resample=2)
    x = g["frames"].permute(0, 3, 1, 2).double()
    want = F.interpolate(x, size=(48, 48), mode="bilinear", antialias=True, align_corners=False)
    assert float((pm.restated_preprocess(g["frames"], pre, normalize=False) - want).abs().max()) <= 1e-10
    as_float = x / 127.5 - 1
    assert float((pm.restated_preprocess(as_float, pre) - pm.restated_preprocess(g["frames"], pre)).abs().max()) <= 1e-12
    assert float((pm.restated_preprocess(g["frames"], pre).float() - g["pixel_values"]).abs().max()) <= 1e-6
    with pytest.raises(ValueError, match="resample 1"):
        pm.resize_matrix(4, 8, 1)


# ------------------------------------------------------------------------------------------------------------------- driver
class _Solo:
    active, is_main = False, True

    def agree(self, v):
        return v


class _Rank:
    active = True

    def __init__(self, is_main, wire):
        self.is_main, self.wire = is_main, wire

    def agree(self, v):
        if self.is_main:
            self.wire.append(v)
        return self.wire[0]


class _StubMasker:
    """Logits 16 x 16 per prompt: a bright square whose place depends on the prompt's index; `dark` prompts stay below 0."""

    def __init__(self):
        self.calls = []

    def logits(self, frames, prompts):
        self.calls.append((tuple(frames.shape), list(prompts)))
        out = torch.full((len(prompts), 16, 16), -3.0)
        for i, p in enumerate(prompts):
            if p != "dark":
                out[i, 2 * i:2 * i + 8, 4:12] = 2.0 + i
        return out

    def masks_from_logits(self, logits, resolution, threshold):
        r, m = pm.restated_masks(logits, resolution, threshold)
        return m, m.flatten(1).sum(dim=1).to(torch.int32)


def _args(**kw):
    base = dict(mask_prompts="hair,eyes", mask_prompt_model_path="/models/clipseg", mask_model_path="", mask_prompt_threshold=0.5,
                mask_index=1, filter_mask=0, device="cpu")
    return SimpleNamespace(**dict(base, **kw))


def test_driver_files_format(tmp_path):
    stub, image = _StubMasker(), torch.randint(0, 255, (24, 32, 3), dtype=torch.uint8).numpy()
    masks = pm.prompt_masks_for_driver(_args(), str(tmp_path), image, 20, masker=stub)
    assert stub.calls == [((1, 24, 32, 3), ["hair", "eyes"])]
    saved = torch.load(tmp_path / "mask" / "mask.pt")
    assert saved.dtype == torch.bool and tuple(saved.shape) == (2, 20, 20) and torch.equal(saved, masks)
    assert bool(saved[0].any()) and bool(saved[1].any()) and not torch.equal(saved[0], saved[1])
    rec = json.loads((tmp_path / "mask" / "mask_prompts.json").read_text())
    assert [r["prompt"] for r in rec] == ["hair", "eyes"] and [r["index"] for r in rec] == [0, 1]
    for r, m in zip(rec, saved):
        assert r["threshold"] == 0.5 and r["logit_min"] == -3.0 and r["logit_max"] == 2.0 + r["index"]
        assert r["area_share"] == float(m.sum()) / 400
    for f in ("mask_0.png", "mask_1.png", "total_mask.png"):
        assert (tmp_path / "mask" / f).exists()


def test_empty_mask_raises_before_anything_is_written(tmp_path):
    with pytest.raises(RuntimeError, match=r"prompt 'dark' gives an empty mask: its largest logit is -3"):
        pm.prompt_masks_for_driver(_args(mask_prompts="hair,dark"), str(tmp_path), torch.zeros(8, 8, 3, dtype=torch.uint8).numpy(), 20,
                                   masker=_StubMasker())
    assert not (tmp_path / "mask" / "mask.pt").exists()
    pm.check_not_empty(["a"], torch.tensor([3]), torch.tensor([1.0]), 0.5)


def test_segment_for_driver_dispatches_to_the_prompt_masker(tmp_path, monkeypatch):
    seen = []

    def fake(args, log_dir, image, resolution, masker=None):
        seen.append((log_dir, resolution))
        return torch.ones(2, resolution, resolution, dtype=torch.bool)
    monkeypatch.setattr(pm, "prompt_masks_for_driver", fake)
    monkeypatch.setattr(ms, "SAM", lambda *a, **k: 1 / 0)                       # Segment Anything is not touched
    m = ms.segment_for_driver(_args(), str(tmp_path), _Solo(), lambda: "image", 12)
    assert seen == [(str(tmp_path), 12)] and tuple(m.shape) == (2, 12, 12)
    # two ranks: rank 0 segments, rank 1 receives
    wire = []
    m0 = ms.segment_for_driver(_args(), str(tmp_path), _Rank(True, wire), lambda: "image", 12)
    m1 = ms.segment_for_driver(_args(), str(tmp_path), _Rank(False, wire), lambda: "image", 12)
    assert len(seen) == 2 and torch.equal(m0, m1)


def test_a_failure_on_rank_0_raises_on_every_rank(tmp_path):
    wire = []
    args = _args(mask_prompt_model_path=str(tmp_path / "nowhere"))
    for is_main in (True, False):
        with pytest.raises(RuntimeError, match="rank 0 could not segment the image: FileNotFoundError"):
            ms.segment_for_driver(args, str(tmp_path), _Rank(is_main, wire), lambda: torch.zeros(8, 8, 3, dtype=torch.uint8).numpy(), 12)
    with pytest.raises(FileNotFoundError, match="nothing is downloaded"):      # single rank: the error itself
        ms.segment_for_driver(args, str(tmp_path), _Solo(), lambda: torch.zeros(8, 8, 3, dtype=torch.uint8).numpy(), 12)
