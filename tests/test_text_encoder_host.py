"""CPU: the CLIP text encoder's host side (loco_edit_amd.text_encoder) -- tokenizer ids against transformers.CLIPTokenizer
(fixture tests/golden/clip_text/ids.json, and live when transformers imports), the checkpoint layouts and their refusals,
the flag conflict, and this file's own torch restatement of the encoder against transformers' CLIPTextModel outputs
(tests/golden/clip_text/tiny_*.pt), which makes the restatement the yardstick of the GPU tests at full size."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import text_encoder as te  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "clip_text")


def restated_clip_text(sd, cfg, ids, dtype=torch.float64):
    """last_hidden_state of CLIPTextTransformer written out in torch: sd in the normalised naming, ids [n, L]."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    n, L = ids.shape
    D, H = cfg.width, cfg.heads
    hd = D // H
    x = p["embeddings.token_embedding.weight"][ids.long()] + p["embeddings.position_embedding.weight"][:L]
    causal = torch.full((L, L), float("-inf"), dtype=dtype, device=x.device).triu(1)

    def ln(v, pre):
        return torch.nn.functional.layer_norm(v, (D,), p[pre + ".weight"], p[pre + ".bias"], cfg.ln_eps)

    def lin(v, pre):
        return v @ p[pre + ".weight"].T + p[pre + ".bias"]
    for i in range(cfg.layers):
        pre = f"encoder.layers.{i}."
        h = ln(x, pre + "layer_norm1")
        q, k, v = (lin(h, pre + f"self_attn.{m}_proj").view(n, L, H, hd).transpose(1, 2) for m in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5 + causal, dim=-1) @ v
        x = x + lin(a.transpose(1, 2).reshape(n, L, D), pre + "self_attn.out_proj")
        h = lin(ln(x, pre + "layer_norm2"), pre + "mlp.fc1")
        h = h * torch.sigmoid(1.702 * h) if cfg.act == "quick_gelu" else torch.nn.functional.gelu(h)
        x = x + lin(h, pre + "mlp.fc2")
    return ln(x, "final_layer_norm")


def _ids():
    with open(os.path.join(GOLD, "ids.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("conv", ["sd1", "sd2"])
def test_tokenizer_matches_fixture_ids(conv):
    d = _ids()
    tok = te.CLIPTokenizer.from_dir(os.path.join(GOLD, f"tokenizer_{conv}"))
    assert tok.model_max_length == 77
    assert tok.pad_token_id == (0 if conv == "sd2" else tok.eos_token_id)
    for s, want in zip(d["strings"], d[conv]):
        got = tok(s)
        assert len(got) == 77 and got == want, s
    long_ids = tok(d["strings"][18])           # truncated: EOS stays the last token
    assert long_ids[0] == tok.bos_token_id and long_ids[-1] == tok.eos_token_id


@pytest.mark.parametrize("conv", ["sd1", "sd2"])
def test_tokenizer_matches_live_transformers(conv):
    transformers = pytest.importorskip("transformers")
    path = os.path.join(GOLD, f"tokenizer_{conv}")
    ref = transformers.CLIPTokenizer.from_pretrained(path)
    tok = te.CLIPTokenizer.from_dir(path)
    extra = ["!", "a!b", "!!hello!!", "it's IT'S", "x y　z", "İstanbul", "ｆｕｌｌ", "½ ² ①",
             "a photo of a man with glasses , 4k", "tab\tsep  ", "é́ café"]
    for s in _ids()["strings"] + extra:
        want = ref(s, padding="max_length", max_length=ref.model_max_length, truncation=True).input_ids
        assert tok(s) == want, s


def _tiny(name):
    return torch.load(os.path.join(GOLD, f"{name}.pt"))


def test_checkpoint_layouts_normalise_to_one_dict(tmp_path):
    g = _tiny("tiny_quick_gelu")
    sd = g["state_dict"]
    ref = te.normalize_text_state_dict(dict(sd))
    assert "embeddings.position_ids" not in ref and all(not k.startswith("text_model.") for k in ref)
    cfg = te.infer_text_config(ref, g["config"])
    te.check_text_state_dict(ref, cfg)
    # 1. a text_encoder/ folder (config.json + pytorch_model.bin) inside a pipeline root with tokenizer/
    root = tmp_path / "pipe"
    os.makedirs(root / "text_encoder")
    with open(root / "text_encoder" / "config.json", "w") as f:
        json.dump(g["config"], f)
    torch.save(dict(sd, **{"text_projection.weight": torch.zeros(4, 32)}), root / "text_encoder" / "pytorch_model.bin")
    os.symlink(os.path.join(GOLD, "tokenizer_sd1"), root / "tokenizer")
    cfg1, sd1, tok_dir = te.load_text_encoder(str(root))
    assert cfg1 == cfg and tok_dir == str(root / "tokenizer")
    cfg2, sd2, tok2 = te.load_text_encoder(str(root / "text_encoder"))
    assert tok2 is None
    # 2. CompVis single files, both prefixes, next to the other networks of the file
    for pre in ("cond_stage_model.transformer.", "cond_stage_model.transformer.text_model."):
        ck = {pre + k[len("text_model."):]: v for k, v in sd.items()}
        ck["model.diffusion_model.out.0.weight"] = torch.zeros(3)
        path = tmp_path / f"ck{len(pre)}.ckpt"
        torch.save({"state_dict": ck}, path)
        sd3 = te.normalize_text_state_dict(torch.load(path))   # (load_text_encoder: width 32 has no preset, see below)
        assert sd3.keys() == ref.keys() and all(torch.equal(sd3[k], ref[k]) for k in ref)
    for d in (sd1, sd2):
        assert d.keys() == ref.keys() and all(torch.equal(d[k], ref[k]) for k in ref)


def test_checkpoint_geometry_from_presets_and_refusals(tmp_path):
    g = _tiny("tiny_gelu")
    ref = te.normalize_text_state_dict(dict(g["state_dict"]))
    with pytest.raises(ValueError, match="width 48"):       # no config.json and no preset of that width
        te.infer_text_config(ref)
    fake = {"embeddings.token_embedding.weight": torch.zeros(10, 1024), "embeddings.position_embedding.weight": torch.zeros(77, 1024),
            "encoder.layers.22.layer_norm1.weight": torch.zeros(1024)}
    c = te.infer_text_config(fake)
    assert (c.width, c.layers, c.heads, c.ffn, c.act, c.vocab) == (1024, 23, 16, 4096, "gelu", 10)
    fake["embeddings.token_embedding.weight"] = torch.zeros(10, 768)
    fake["embeddings.position_embedding.weight"] = torch.zeros(77, 768)
    c = te.infer_text_config(fake)
    assert (c.width, c.layers, c.heads, c.ffn, c.act) == (768, 23, 12, 3072, "quick_gelu")
    with pytest.raises(ValueError, match="OpenCLIP"):
        te.normalize_text_state_dict({"cond_stage_model.model.transformer.resblocks.0.attn.in_proj_weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="foreign"):
        te.normalize_text_state_dict(dict(g["state_dict"], **{"vision_model.x": torch.zeros(1)}))
    cfg = te.infer_text_config(ref, g["config"])
    part = {k: v for k, v in ref.items() if "layers.2.mlp.fc2" not in k}
    with pytest.raises(ValueError, match="missing"):
        te.check_text_state_dict(part, cfg)
    with pytest.raises(ValueError, match="foreign"):
        te.check_text_state_dict(dict(ref, **{"encoder.layers.3.layer_norm1.weight": torch.zeros(48)}), cfg)
    with pytest.raises(ValueError, match="missing"):         # a file whose text tower is cut short
        p = tmp_path / "x.bin"
        torch.save({k: v for k, v in g["state_dict"].items() if "final_layer_norm" not in k}, p)
        os.makedirs(tmp_path / "te")
        os.replace(p, tmp_path / "te" / "pytorch_model.bin")
        with open(tmp_path / "te" / "config.json", "w") as f:
            json.dump(g["config"], f)
        te.load_text_encoder(str(tmp_path / "te"))


def test_text_encoder_flag_conflicts_with_prompt_emb_path():
    from loco_edit_amd.define_argparser import parse_args
    with pytest.raises(ValueError, match="prompt_emb_path"):
        parse_args(["--text_encoder_path", "a", "--prompt_emb_path", "b"])
    a = parse_args(["--text_encoder_path", "a", "--tokenizer_path", "t"])
    assert (a.text_encoder_path, a.tokenizer_path, a.prompt_emb_path) == ("a", "t", "")
    assert parse_args([]).text_encoder_path == ""


@pytest.mark.parametrize("name", ["tiny_quick_gelu", "tiny_gelu"])
def test_restatement_reproduces_transformers_outputs(name):
    g = _tiny(name)
    sd = te.normalize_text_state_dict(dict(g["state_dict"]))
    cfg = te.infer_text_config(sd, g["config"])
    out = restated_clip_text(sd, cfg, g["ids"])
    ref = g["last_hidden_state"].double()
    for i in range(ref.shape[0]):
        e = ((out[i] - ref[i]).norm() / ref[i].norm()).item()
        assert e < 2e-6, (i, e)
