"""GPU tests of the CLIP image encoder and the scores built on it (csrc/clipvis.hip through hip.LocoClipVisionEngine /
clip_score.ClipScorer):

* tiny fixtures (tests/golden/clip_vision/tiny_*.pt, see tests/make_golden_clip_vision.py for why these geometries): HIP against
  transformers' CLIPVisionModelWithProjection outputs, rel-L2 <= 2e-5 per image (the bar the CLIP text test holds for the same
  GEMM and arithmetic); each image bit-identical alone, at every position of a max_images batch and under LOCO_PRECISION=f16;
  refusals are errors;
* the device preprocessing against the float64 restatement of test_clip_score_host.py, max abs <= 1e-3 grey level before the
  normalisation (two passes of at most 12 fp32 FMA taps on values up to about 330 bound the error near 5e-4);
* the text side and the four cosines end to end in both preprocessing modes, abs <= 1e-4 against transformers' embeddings;
* at size: ViT-L/14 with seeded weights against a float64 restatement on the device, rel-L2 <= 1e-4."""
import importlib.util
import json
import os
import shutil
import sys
import time

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import clip_score as cs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(ROOT, "tests", "golden", "clip_vision")
_spec = importlib.util.spec_from_file_location("clip_score_host", os.path.join(ROOT, "tests", "test_clip_score_host.py"))
_host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_host)
restated_preprocess, smooth_noise_image = _host.restated_preprocess, _host.smooth_noise_image

_FIXTURES = {}


def fixture(name):
    """The fixture, its state dict upcast to fp32 (the stored bf16 values are exact), the split parts and the geometry."""
    if name not in _FIXTURES:
        g = torch.load(os.path.join(GOLD, f"{name}.pt"))
        sd = {k: (v.float() if v.is_floating_point() else v) for k, v in g["state_dict"].items()}
        vision, text, vproj, tproj = cs.split_clip_state_dict(sd)
        vcfg = cs.infer_vision_config(vision, vproj, g["config"]["vision_config"])
        _FIXTURES[name] = (g, sd, dict(vision, **{"visual_projection.weight": vproj}), vcfg)
    return _FIXTURES[name]


def rel_rows(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return [((a[i] - b[i]).norm() / b[i].norm()).item() for i in range(a.shape[0])]


def write_clip_folder(root, name):
    """A transformers CLIPModel folder of a fixture: config.json, pytorch_model.bin, the tokenizer files."""
    g, sd, _, _ = fixture(name)
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "clip_text", "tokenizer_sd1"), root)
    with open(os.path.join(root, "config.json"), "w") as f:
        json.dump(g["config"], f)
    torch.save(sd, os.path.join(root, "pytorch_model.bin"))
    return root


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_tiny_encoders_vs_transformers_and_batch_invariance(name):
    from loco_edit_amd.hip import LocoClipVisionEngine
    g, _, vsd, vcfg = fixture(name)
    pv = g["pixel_values"]
    n = pv.shape[0]
    eng = LocoClipVisionEngine(vcfg, max_images=n + 2, device=torch.device(DEV))
    eng.load_state_dict(vsd)
    emb, hid, pool = eng.encode(pv, want_hidden=True)
    for what, got, want in (("last_hidden_state", hid, g["last_hidden_state"]), ("pooler_output", pool, g["pooler_output"]),
                            ("image_embeds", emb, g["image_embeds"])):
        errs = rel_rows(got, want)
        print(name, what, "rel-L2 per image vs transformers:", ["%.1e" % e for e in errs])
        assert tuple(got.shape) == tuple(want.shape) and max(errs) <= 2e-5
    assert torch.equal(eng.encode(pv), emb)
    # bit-identity: alone, and at every position of a full batch of max_images images
    for i in range(n):
        assert torch.equal(eng.encode(pv[i:i + 1])[0], emb[i])
    full = torch.cat([pv, pv[:2]])
    for shift in range(n + 2):
        e2, h2, p2 = eng.encode(torch.roll(full, shift, dims=0), want_hidden=True)
        e2, h2, p2 = (torch.roll(t, -shift, dims=0) for t in (e2, h2, p2))
        assert torch.equal(e2[:n], emb) and torch.equal(e2[n:], emb[:2])
        assert torch.equal(h2[:n], hid) and torch.equal(p2[:n], pool)
    # the encoder's result does not depend on the conv arithmetic switch
    os.environ["LOCO_PRECISION"] = "f16"
    try:
        eng16 = LocoClipVisionEngine(vcfg, max_images=n, device=torch.device(DEV))
        eng16.load_state_dict(vsd)
        assert torch.equal(eng16.encode(pv), emb) and torch.equal(eng.encode(pv), emb)
    finally:
        os.environ.pop("LOCO_PRECISION")


def test_refusals_are_errors():
    from dataclasses import replace
    from loco_edit_amd.hip import LocoClipVisionEngine
    g, _, vsd, vcfg = fixture("tiny_a")
    pv = g["pixel_values"]
    eng = LocoClipVisionEngine(vcfg, max_images=2, device=torch.device(DEV))
    eng.load_state_dict(vsd)
    with pytest.raises(RuntimeError, match="max_images"):
        eng.encode(pv)                                                  # 3 images
    with pytest.raises(ValueError, match="pixel_values must be"):
        eng.encode(pv[:1, :, :24])
    with pytest.raises(ValueError, match="pixel_values must be"):
        eng.encode(pv[0])
    with pytest.raises(ValueError, match="frames must be uint8"):
        eng.preprocess(g["frames"].float())
    with pytest.raises(ValueError, match="frames must be uint8"):
        eng.preprocess(g["frames"][..., :2])
    part = LocoClipVisionEngine(vcfg, max_images=1, device=torch.device(DEV))
    with pytest.raises(RuntimeError, match="missing"):
        part.load_state_dict({k: v for k, v in vsd.items() if k != "pre_layrnorm.bias"})
    with pytest.raises(RuntimeError, match="missing parameter pre_layrnorm.bias"):
        part.encode(pv[:1])
    with pytest.raises(RuntimeError, match="unknown parameter"):
        part.load_state_dict({"encoder.layers.99.mlp.fc1.weight": torch.zeros(2)})
    with pytest.raises(RuntimeError, match="has shape"):
        part.load_state_dict({"visual_projection.weight": torch.zeros(3, 3)})
    with pytest.raises(RuntimeError, match="image_size is not a multiple of patch_size"):
        LocoClipVisionEngine(replace(vcfg, image_size=36), device=torch.device(DEV))
    with pytest.raises(RuntimeError, match="width is not a multiple of heads"):
        LocoClipVisionEngine(replace(vcfg, heads=5), device=torch.device(DEV))
    with pytest.raises(RuntimeError, match="head width"):
        LocoClipVisionEngine(replace(vcfg, width=256, heads=2), device=torch.device(DEV))
    assert torch.equal(eng.encode(pv[:2]), eng.encode(pv[:2]))         # the handle still works


@pytest.fixture(scope="module")
def engine224():
    from loco_edit_amd.hip import LocoClipVisionEngine
    cfg = cs.ClipVisionConfig(image_size=224, patch_size=32, width=64, layers=1, heads=1, mlp_dim=64, projection_dim=8)
    return LocoClipVisionEngine(cfg, max_images=1, device=torch.device(DEV))


@pytest.mark.parametrize("H,W", [(64, 64), (256, 256), (96, 80), (80, 96), (512, 512)])
def test_device_preprocess_vs_float64_restatement(engine224, H, W):
    frames = torch.stack([smooth_noise_image(H, W, seed=H * 1000 + W + i) for i in range(2)])
    got = engine224.preprocess(frames.to(DEV)).double().cpu()
    assert tuple(got.shape) == (2, 3, 224, 224)
    m, s = torch.tensor(cs.CLIP_MEAN, dtype=torch.float64).view(1, 3, 1, 1), torch.tensor(cs.CLIP_STD, dtype=torch.float64).view(1, 3, 1, 1)
    grey = (got * s + m) * 255
    want = restated_preprocess(frames, 224, normalize=False)
    err = float((grey - want).abs().max())
    print(f"{H}x{W}: device preprocess vs float64 restatement, max abs {err:.2e} grey levels")
    assert err <= 1e-3
    assert torch.equal(engine224.preprocess(frames[1])[0].double().cpu(), got[1])       # one frame, from the host


def test_device_preprocess_identity_case(engine224):
    """S x S in: no resize, no crop -- exact up to the roundings of / 255, - mean and / std (three fp32 roundings on values of
    at most 1, 0.6 and 2.7, the first two divided by std >= 0.26: below 5.3e-7)."""
    frames = smooth_noise_image(224, 224, seed=3)[None]
    got = engine224.preprocess(frames).double().cpu()
    err = float((got - restated_preprocess(frames, 224)).abs().max())
    print(f"224x224: device preprocess identity case, max abs {err:.2e}")
    assert err <= 1e-6


@pytest.fixture(scope="module")
def scorers(tmp_path_factory):
    root = write_clip_folder(str(tmp_path_factory.mktemp("clip") / "tiny_a"), "tiny_a")
    return {mode: cs.load_clip(root, device=torch.device(DEV), max_images=2, preprocess=mode) for mode in ("pil", "device")}


def test_text_embeds_vs_transformers(scorers):
    g = fixture("tiny_a")[0]
    sc = scorers["pil"]
    assert torch.equal(sc.tokenizer.batch(g["prompts"]).long(), g["ids"])
    got = sc.text_embeds(g["prompts"])
    errs = rel_rows(got, g["text_embeds"])
    print("text_embeds rel-L2 per prompt vs CLIPTextModelWithProjection:", ["%.1e" % e for e in errs])
    assert max(errs) <= 2e-5


@pytest.mark.parametrize("mode", ["pil", "device"])
def test_scores_end_to_end(scorers, mode):
    """The four cosines per frame against the same cosines in float64 from transformers' embeddings: CLIPImageProcessor's
    pixel values ("pil") or the float64 restatement of the preprocessing ("device") through CLIPVisionModelWithProjection."""
    g = fixture("tiny_a")[0]
    img = g["image_embeds" if mode == "pil" else "image_embeds_device"].double()
    txt = g["text_embeds"].double()
    # the directional similarity is well conditioned on these frames and prompts
    cond = [float((img[i] - img[0]).norm() / img[0].norm()) for i in range(1, img.shape[0])] + [float((txt[1] - txt[0]).norm() / txt[0].norm())]
    assert min(cond) >= 1e-3
    want = cs.score_embeddings(img, 0, txt[0], txt[1])
    got = scorers[mode].score(g["frames"].to(DEV), 0, g["prompts"][0], g["prompts"][1])
    assert len(got) == img.shape[0] and got[0]["directional"] is None and abs(got[0]["image_sim"] - 1) <= 1e-6
    for i, (a, b) in enumerate(zip(got, want)):
        for k in ("clip_for", "clip_edit", "image_sim", "directional"):
            if b[k] is None:
                assert a[k] is None
                continue
            print(f"{mode} frame {i} {k}: {a[k]:+.6f} vs {b[k]:+.6f} (diff {abs(a[k] - b[k]):.1e})")
            assert abs(a[k] - b[k]) <= 1e-4
    if mode == "pil":
        assert torch.equal(scorers[mode].pixel_values(g["frames"]).cpu(), g["pixel_values"])


def test_eval_cli_scores_folders_of_pngs(tmp_path):
    """eval.py --eval_metric clip / clip_dir on folders of PNGs (lossless), default "pil" preprocessing: the numbers of the
    fixture's transformers embeddings, abs <= 1e-4."""
    from PIL import Image
    from loco_edit_amd import eval as ev
    g = fixture("tiny_a")[0]
    root = write_clip_folder(str(tmp_path / "tiny_a"), "tiny_a")
    os.makedirs(tmp_path / "preds"), os.makedirs(tmp_path / "orig")
    for i, name in ((1, "a.png"), (2, "b.png")):
        Image.fromarray(g["frames"][i].numpy()).save(str(tmp_path / "preds" / name))
        Image.fromarray(g["frames"][0].numpy()).save(str(tmp_path / "orig" / name))
    want = cs.score_embeddings(g["image_embeds"], 0, g["text_embeds"][0], g["text_embeds"][1])
    for metric, key in (("clip", "clip_edit"), ("clip_dir", "directional")):
        r = ev.main(["--eval_metric", metric, "--folder_preds", str(tmp_path / "preds"), "--folder_original", str(tmp_path / "orig"),
                     "--clip_model_path", root, "--for_prompt", g["prompts"][0], "--edit_prompt", g["prompts"][1]])
        assert r["n"] == 2 and r["clip_preprocess"] == "pil"
        for v, w in zip(r["values"], want[1:]):
            assert abs(v - w[key]) <= 1e-4
        assert abs(r["mean"] - (want[1][key] + want[2][key]) / 2) <= 1e-4
    with pytest.raises(ValueError, match="edit_prompt"):
        ev.main(["--eval_metric", "clip_dir", "--folder_preds", str(tmp_path / "preds"), "--folder_original", str(tmp_path / "orig"),
                 "--clip_model_path", root, "--edit_prompt", g["prompts"][1]])


# ------------------------------------------------------------------------------------------------------------------ at size
def _synth_clip_vision(cfg, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)

    def r(*s, std=0.02):
        return torch.randn(*s, generator=g, device=DEV) * std
    D, Fm, ps = cfg.width, cfg.mlp_dim, cfg.patch_size
    T = 1 + (cfg.image_size // ps) ** 2
    sd = {"embeddings.class_embedding": r(D, std=0.5), "embeddings.patch_embedding.weight": r(D, 3, ps, ps, std=(3 * ps * ps) ** -0.5),
          "embeddings.position_embedding.weight": r(T, D, std=0.3)}
    for ln in ("pre_layrnorm", "post_layernorm"):
        sd[ln + ".weight"], sd[ln + ".bias"] = 1 + r(D, std=0.1), r(D, std=0.1)
    for i in range(cfg.layers):
        p = f"encoder.layers.{i}."
        for ln in ("layer_norm1", "layer_norm2"):
            sd[p + ln + ".weight"], sd[p + ln + ".bias"] = 1 + r(D, std=0.1), r(D, std=0.1)
        for m in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[p + f"self_attn.{m}.weight"], sd[p + f"self_attn.{m}.bias"] = r(D, D, std=D ** -0.5), r(D)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = r(Fm, D, std=D ** -0.5), r(Fm)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = r(D, Fm, std=Fm ** -0.5), r(D)
    sd["visual_projection.weight"] = r(cfg.projection_dim, D, std=D ** -0.5)
    return sd


def restated_clip_vision(sd, cfg, pixel_values, dtype=torch.float64):
    """CLIPVisionModelWithProjection restated in plain torch: (image_embeds [n, P], last_hidden_state [n, T, D])."""
    w = {k: v.to(dtype) for k, v in sd.items()}
    D, ps, heads = cfg.width, cfg.patch_size, cfg.heads
    x = F.conv2d(pixel_values.to(dtype), w["embeddings.patch_embedding.weight"], stride=ps).flatten(2).transpose(1, 2)
    n = x.shape[0]
    x = torch.cat([w["embeddings.class_embedding"].expand(n, 1, D), x], dim=1) + w["embeddings.position_embedding.weight"]
    ln = lambda v, name: F.layer_norm(v, (D,), w[name + ".weight"], w[name + ".bias"], cfg.ln_eps)      # noqa: E731
    lin = lambda v, name: F.linear(v, w[name + ".weight"], w[name + ".bias"])                              # noqa: E731
    x = ln(x, "pre_layrnorm")
    for i in range(cfg.layers):
        p = f"encoder.layers.{i}."
        y = ln(x, p + "layer_norm1")
        q, k, v = (lin(y, p + f"self_attn.{m}_proj").view(n, -1, heads, D // heads).transpose(1, 2) for m in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) * (D // heads) ** -0.5, dim=-1) @ v
        x = x + lin(a.transpose(1, 2).reshape(n, -1, D), p + "self_attn.out_proj")
        y = lin(ln(x, p + "layer_norm2"), p + "mlp.fc1")
        y = y * torch.sigmoid(1.702 * y) if cfg.act == "quick_gelu" else F.gelu(y)
        x = x + lin(y, p + "mlp.fc2")
    return ln(x[:, 0], "post_layernorm") @ w["visual_projection.weight"].T, x


def test_restatement_agrees_with_transformers_fixture():
    """The float64 restatement that judges the at-size run is itself pinned to transformers on a fixture."""
    g, _, vsd, vcfg = fixture("tiny_b")
    emb, hid = restated_clip_vision(vsd, vcfg, g["pixel_values"])
    assert max(rel_rows(emb, g["image_embeds"])) <= 2e-5 and max(rel_rows(hid, g["last_hidden_state"])) <= 2e-5


def test_vit_l14_vs_restatement():
    from loco_edit_amd.hip import LocoClipVisionEngine
    cfg = cs.CLIP_VIT_L14
    sd = _synth_clip_vision(cfg, 3)
    eng = LocoClipVisionEngine(cfg, max_images=25, device=torch.device(DEV))
    eng.load_state_dict(sd)
    frames = torch.stack([smooth_noise_image(512, 512, seed=40 + i) for i in range(2)]).to(DEV)
    pv = eng.preprocess(frames)
    emb, hid, _ = eng.encode(pv, want_hidden=True)
    with torch.no_grad():
        ref_emb, ref_hid = restated_clip_vision(sd, cfg, pv)
    e1, e2 = rel_rows(emb, ref_emb), rel_rows(hid, ref_hid)
    print("ViT-L/14 rel-L2 per image vs float64 restatement: image_embeds", ["%.1e" % e for e in e1], "last_hidden_state", ["%.1e" % e for e in e2])
    assert max(e1) <= 1e-4 and max(e2) <= 1e-4
    assert torch.equal(eng.encode(pv[1:])[0], emb[1])
    # 25 frames of 512 x 512: preprocess + encode, warm, timed from the host around a device synchronisation
    many = frames[:1].expand(25, -1, -1, -1).contiguous()
    eng.encode(eng.preprocess(many))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = eng.encode(eng.preprocess(many))
    torch.cuda.synchronize()
    print(f"ViT-L/14: warm 25-frame (512 x 512) preprocess + encode {1e3 * (time.perf_counter() - t0):.1f} ms (host-timed, unasserted)")
    assert torch.equal(out[0], emb[0]) and torch.equal(out[24], emb[0])
