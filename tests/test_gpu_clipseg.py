"""GPU tests of the text-prompted masks (csrc/clipseg.hip and the taps of csrc/clipvis.hip through hip.LocoClipVisionEngine /
hip.LocoClipSegDecoder / prompt_mask.PromptMasker) on the fixtures of tests/make_golden_clipseg.py:

* taps against transformers, rel-L2 <= 2e-5 per image and tap (the bar test_gpu_clip_vision.py holds for the same GEMM and
  arithmetic); bit-identical alone and at every position of a full batch; `encode` unchanged by a preceding `encode_taps`;
* logits against the float64 goldens per mask, bar max(2e-5, 4 x fp32_err) with fp32_err (what transformers' own fp32 run loses
  on the same model) read from the fixture; bit-identical whatever M, the position, the prompt order, under LOCO_PRECISION=f16;
* the preprocessing against the float64 restatement, max abs <= 1e-3 grey level before the normalisation (the bar
  test_gpu_clip_vision.py derives for the same two-pass fp32 scheme);
* masks at 40 (down) and 200 (up) bit-equal to the float64 goldens outside the band of 1e-3 around the threshold logit (at most
  0.5 % of a mask's pixels), `area` equal to the count of the returned mask;
* refusals are errors.

Measured on MI355X (rel-L2 of the logits per mask | fp32_err of the fixture): see profiles/clipseg.md."""
import os
import sys
from dataclasses import replace

import numpy as np
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
NAMES = ("seg_a", "seg_b")
_cache = {}


def fixture(name):
    """(golden dict, PromptMasker) of a fixture, built once."""
    if name not in _cache:
        g = torch.load(os.path.join(GOLD, f"{name}.pt"))
        ref = os.path.join(GOLD, f"{name}_ref.pt")
        if os.path.exists(ref):
            g.update(torch.load(ref))
        sd = {k: (v.float() if v.is_floating_point() else v) for k, v in g["state_dict"].items()}
        parts = pm.parts_from_state_dict(sd, g["config"], g["preprocessor"], TOK, max_masks=8)
        from loco_edit_amd.text_encoder import CLIPTokenizer
        _cache[name] = (g, pm.PromptMasker(parts, CLIPTokenizer.from_dir(TOK), device=torch.device(DEV), max_images=3))
    return _cache[name]


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _unpack(packed, res):
    bits = np.unpackbits(packed.numpy(), axis=1)[:, :res * res]
    return torch.from_numpy(bits).bool().view(-1, res, res)


@pytest.mark.parametrize("name", NAMES)
def test_taps_against_transformers_and_bit_identity(name):
    g, mk = fixture(name)
    pv, layers = g["pixel_values"], mk.parts.extract_layers
    n = pv.shape[0]
    taps = mk.vision.encode_taps(pv, layers)
    assert tuple(taps.shape) == tuple(g["taps"].shape)
    for j in range(len(layers)):
        for i in range(n):
            err = _rel(taps[j, i], g["taps"][j, i])
            print(f"{name} tap {layers[j]} image {i}: rel-L2 {err:.2e}")
            assert err <= 2e-5
    # the position table the loader interpolated is the one transformers adds
    assert torch.equal(mk.parts.vision_sd["embeddings.position_embedding.weight"], g["position_table"])
    # alone and at every position of a full batch
    mi = mk.vision.max_images
    filler = torch.flip(pv, dims=(2,))
    for i in range(n):
        alone = mk.vision.encode_taps(pv[i:i + 1], layers)
        assert torch.equal(alone[:, 0], taps[:, i])
        for pos in range(mi):
            batch = torch.cat([filler[:1]] * mi).clone()
            batch[pos] = pv[i]
            assert torch.equal(mk.vision.encode_taps(batch, layers)[:, pos], taps[:, i])
    # a shorter tap list stops early and gives the same rows; encode is unchanged by a preceding encode_taps
    assert torch.equal(mk.vision.encode_taps(pv, layers[:1])[0], taps[0])
    from loco_edit_amd.hip import LocoClipVisionEngine
    fresh = LocoClipVisionEngine(mk.parts.vision_cfg, max_images=mi, device=torch.device(DEV))
    fresh.load_state_dict(mk.parts.vision_sd)
    want = fresh.encode(pv, want_hidden=True)
    mk.vision.encode_taps(pv, layers)
    got = mk.vision.encode(pv, want_hidden=True)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("name", NAMES)
def test_logits_against_float64_and_bit_identity(name):
    g, mk = fixture(name)
    iom, pom = g["image_of_mask"], g["prompt_of_mask"]
    cond = mk.conditional_embeddings(g["prompts"])
    assert _rel(cond, g["cond"]) <= 2e-5
    taps = mk.vision.encode_taps(g["pixel_values"], mk.parts.extract_layers)
    logits = mk.decoder.decode(taps, cond[pom], iom)
    assert tuple(logits.shape) == tuple(g["logits64"].shape) and logits.shape[1] == mk.parts.decoder_cfg.logit_size
    for m in range(len(iom)):
        err, bar = _rel(logits[m], g["logits64"][m]), max(2e-5, 4 * g["fp32_err"][m])
        print(f"{name} mask {m}: rel-L2 to float64 {err:.2e}, fp32_err of transformers {g['fp32_err'][m]:.2e}, bar {bar:.2e}")
        assert err <= bar
    # the public path gives the same bits
    assert torch.equal(mk.logits_from_embeddings(g["frames"], cond[pom], iom),
                       mk.decoder.decode(mk.taps(mk.pixel_values(g["frames"])), cond[pom], iom))
    # whatever M, the position and the order
    M = len(iom)
    for m in range(M):
        assert torch.equal(mk.decoder.decode(taps, cond[pom[m]][None], [iom[m]])[0], logits[m])
    rev = list(range(M))[::-1]
    back = mk.decoder.decode(taps, cond[[pom[m] for m in rev]], [iom[m] for m in rev])
    assert torch.equal(torch.flip(back, dims=(0,)), logits)
    full = mk.decoder.cfg.max_masks
    for pos in range(0, full, 3):
        c = cond[[pom[0]] * full].clone()
        im = [iom[0]] * full
        c[pos], im[pos] = cond[pom[-1]], iom[-1]
        assert torch.equal(mk.decoder.decode(taps, c, im)[pos], logits[-1])
    os.environ["LOCO_PRECISION"] = "f16"
    try:
        from loco_edit_amd.hip import LocoClipSegDecoder
        d16 = LocoClipSegDecoder(mk.parts.decoder_cfg, device=torch.device(DEV))
        d16.load_state_dict(mk.parts.decoder_sd)
        assert torch.equal(d16.decode(taps, cond[pom], iom), logits)
    finally:
        os.environ.pop("LOCO_PRECISION")


@pytest.mark.parametrize("name", NAMES)
def test_preprocessing_against_the_float64_restatement(name):
    g, mk = fixture(name)
    p = mk.parts.preprocess
    mean, std = (torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1) for v in (p.image_mean, p.image_std))
    want = pm.restated_preprocess(g["frames"], p, normalize=False)
    as_float = (g["frames"].permute(0, 3, 1, 2).float() / 127.5 - 1)
    for label, frames in (("uint8", g["frames"]), ("float", as_float)):
        got = (mk.pixel_values(frames).double().cpu() * std + mean) * 255
        err = float((got - want).abs().max())
        print(f"{name} {label}: max abs {err:.2e} grey levels")
        assert err <= 1e-3
    assert _rel(mk.pixel_values(g["frames"]), g["pixel_values"]) <= 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_masks_against_the_float64_goldens(name):
    g, mk = fixture(name)
    thr = g["threshold"]
    logits = g["logits64"].float()
    for res, gold in g["resized"].items():
        mask, area = mk.masks_from_logits(logits, res, thr)
        want, near = _unpack(gold["masks"], res), _unpack(gold["near"], res)
        assert mask.dtype == torch.bool and tuple(mask.shape) == tuple(want.shape)
        assert float(near.flatten(1).float().mean(dim=1).max()) <= 0.005
        mask = mask.cpu()
        wrong = (mask != want) & ~near
        print(f"{name} res {res}: {int((mask != want).sum())} pixels differ, {int(wrong.sum())} of them outside the band")
        assert not bool(wrong.any())
        assert area.dtype == torch.int32 and area.cpu().tolist() == mask.flatten(1).sum(dim=1).tolist()
        if "logits" in gold:
            r64, _ = pm.restated_masks(g["logits64"], res, thr)
            assert torch.equal(r64, gold["logits"])


def test_empty_mask_raises_with_the_prompt_and_its_logit_maximum():
    g, mk = fixture("seg_a")
    with pytest.raises(RuntimeError, match=r"prompt 'hair' gives an empty mask: its largest logit is"):
        mk.masks(g["frames"][:1], ["hair"], 40, threshold=1 - 1e-9)
    m = mk.masks(g["frames"][:1], g["prompts"], 40, threshold=0.5)
    assert m.dtype == torch.bool and tuple(m.shape) == (3, 40, 40)
    # end to end from the frame: the golden masks outside a band of fp32-logit width around the threshold
    r64, want = pm.restated_masks(g["logits64"][:3], 40, 0.5)
    assert not bool(((m.cpu() != want) & (r64.abs() > 1e-3)).any())


def test_refusals_are_errors():
    from loco_edit_amd.hip import LocoClipSegDecoder, LocoClipVisionEngine
    g, mk = fixture("seg_a")
    dcfg, dev = mk.parts.decoder_cfg, torch.device(DEV)
    for bad, msg in ((replace(dcfg, heads=16), "head width"), (replace(dcfg, grid=64), "tokens"), (replace(dcfg, max_masks=65), "max_masks"),
                     (replace(dcfg, conditional_layer=3), "conditional_layer"), (replace(dcfg, complex_head=True, patch_size=6), "complex head")):
        with pytest.raises(RuntimeError, match=msg):
            LocoClipSegDecoder(bad, device=dev)
    taps = mk.vision.encode_taps(g["pixel_values"], mk.parts.extract_layers)
    cond = g["cond"]
    with pytest.raises(RuntimeError, match="outside"):
        mk.decoder.decode(taps, cond[[0] * 9], [0] * 9)                       # M > max_masks
    with pytest.raises(RuntimeError, match="image_of_mask"):
        mk.decoder.decode(taps, cond[:1], [2])                                # image out of range
    empty = LocoClipSegDecoder(dcfg, device=dev)
    with pytest.raises(RuntimeError, match="missing parameter"):
        empty.decode(taps, cond[:1], [0])
    with pytest.raises(RuntimeError, match="resample 1"):
        mk.decoder.preprocess(g["frames"], 48, 1, pm.IMAGENET_MEAN, pm.IMAGENET_STD)
    pv = g["pixel_values"]
    for layers, msg in (([1, 1], "strictly increasing"), ([2, 1], "strictly increasing"), ([0, 4], "outside"), ([-1], "outside"), ([], "n_taps")):
        with pytest.raises(RuntimeError, match=msg):
            mk.vision.encode_taps(pv, layers)
    with pytest.raises(RuntimeError, match="outside"):
        mk.vision.encode_taps(torch.cat([pv, pv]), [0])                       # n > max_images
    fresh = LocoClipVisionEngine(mk.parts.vision_cfg, max_images=2, device=dev)
    with pytest.raises(RuntimeError, match="missing parameter"):
        fresh.encode_taps(pv, [0])
