"""CPU: the T5 text encoder's host side (loco_edit_amd.text_encoder) -- tokenizer ids against transformers.T5Tokenizer
(fixture tests/golden/t5_text/ids.json from tokenizer.json and from spiece.model, and live when transformers imports), the
relative-position buckets against T5Attention._relative_position_bucket, the checkpoint layouts and their refusals, and
this file's own torch restatement of the encoder against T5EncoderModel's float64 outputs (tests/golden/t5_text/tiny_*.pt),
which makes the restatement the yardstick of the GPU tests at full size."""
import json
import os
import shutil
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import text_encoder as te  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "t5_text")


def restated_t5(sd, cfg, ids, lens=None, dtype=torch.float64):
    """last_hidden_state of T5EncoderModel written out in torch: sd in the normalised naming (values on any device, any
    float dtype), ids [n, L], lens [n] or None.  Walks the blocks, converting one block's weights at a time."""
    n, L = ids.shape
    dev = ids.device
    D, H, hd = cfg.d_model, cfg.heads, cfg.d_kv

    def P(k):
        return sd[k].to(device=dev, dtype=dtype)

    def rms(v, w):
        return v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + cfg.ln_eps) * w
    x = P("shared.weight")[ids.long()]
    pos = torch.arange(L, device=dev)
    rel = (pos[None, :] - pos[:, None]).tolist()                       # k - q
    bucket = torch.tensor([[te.t5_relative_bucket(r, cfg.buckets, cfg.max_distance) for r in row] for row in rel], device=dev)
    bias = P("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight")[bucket].permute(2, 0, 1)[None]   # [1,H,q,k]
    if lens is not None:
        keep = pos[None, :] < torch.as_tensor(lens, device=dev).long()[:, None]
        bias = bias.expand(n, H, L, L).masked_fill(~keep[:, None, None, :], float("-inf"))
    for i in range(cfg.layers):
        a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
        h = rms(x, P(a + "layer_norm.weight"))
        q, k, v = ((h @ P(a + f"SelfAttention.{m}.weight").T).view(n, L, H, hd).transpose(1, 2) for m in "qkv")
        o = torch.softmax(q @ k.transpose(-1, -2) + bias, dim=-1) @ v
        x = x + o.transpose(1, 2).reshape(n, L, H * hd) @ P(a + "SelfAttention.o.weight").T
        h = rms(x, P(f + "layer_norm.weight"))
        g = h @ P(f + "DenseReluDense.wi_0.weight").T
        g = 0.5 * g * (1.0 + torch.tanh(0.7978845608028654 * (g + 0.044715 * g.pow(3))))
        x = x + (g * (h @ P(f + "DenseReluDense.wi_1.weight").T)) @ P(f + "DenseReluDense.wo.weight").T
    return rms(x, P("encoder.final_layer_norm.weight"))


def _ids():
    with open(os.path.join(GOLD, "ids.json")) as f:
        return json.load(f)


def _tiny(name):
    g = torch.load(os.path.join(GOLD, f"{name}.pt"))
    sd = te.normalize_t5_state_dict(dict(g["state_dict"]))
    cfg = te.infer_t5_config(sd, g["config"], positions=g["positions"])
    te.check_t5_state_dict(sd, cfg)
    return g, sd, cfg


@pytest.mark.parametrize("source", ["tokenizer.json", "spiece.model"])
def test_t5_tokenizer_matches_fixture_ids(source, tmp_path):
    d = _ids()
    assert len(d["prompts"]) >= 200 and all(p.isascii() for p in d["prompts"])
    shutil.copy(os.path.join(GOLD, "tokenizer", source), str(tmp_path / source))      # a folder with that one file
    for L in (7, 77):
        tok = te.T5Tokenizer.from_dir(str(tmp_path), model_max_length=L)
        assert (tok.pad_token_id, tok.eos_token_id, tok.unk_token_id) == (0, 1, 2)
        want = d[f"L{L}"]
        assert len(want["ids"]) == len(want["lens"]) == len(d["prompts"])
        for p, ids, ln in zip(d["prompts"], want["ids"], want["lens"]):
            got, glen = tok(p)
            assert len(got) == L and got == ids and glen == ln, p
            assert got[glen - 1] == 1 and all(v == 0 for v in got[glen:])             # </s> last, then padding
        bi, bl = tok.batch(d["prompts"][:9])
        assert bi.tolist() == want["ids"][:9] and bl.tolist() == want["lens"][:9]
    assert max(d["L7"]["lens"]) == 7 and max(d["L77"]["lens"]) == 77 and min(d["L77"]["lens"]) == 1


def test_t5_tokenizer_matches_live_transformers():
    transformers = pytest.importorskip("transformers")
    tok = te.T5Tokenizer.from_dir(os.path.join(GOLD, "tokenizer"))
    ref = transformers.T5Tokenizer(vocab=[(p, s) for p, s in tok.pieces], extra_ids=0)
    extra = ["a photo of a man , 4k", "it's IT'S", "tab\tsep  ", "x" * 200, "glasses!glasses", "a . b . c", "0 1 2 3 4 5 6 7 8 9 10"]
    for L in (7, 77):
        tok.model_max_length = L
        for s in _ids()["prompts"] + extra:
            e = ref(s, padding="max_length", max_length=L, truncation=True)
            assert tok(s) == (e.input_ids, sum(e.attention_mask)), s


def test_relative_position_buckets():
    table = _ids()["buckets_L128"]
    assert table == [te.t5_relative_bucket(r, 32, 128) for r in range(-127, 128)]
    try:
        from transformers.models.t5.modeling_t5 import T5Attention
    except Exception:
        return
    for L in (7, 77, 128, 512):
        rel = torch.arange(-(L - 1), L)
        for nb, md in ((32, 128), (32, 64), (16, 128), (64, 256), (32, 256), (64, 128)):
            want = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=nb, max_distance=md).tolist()
            got = [te.t5_relative_bucket(int(r), nb, md) for r in rel]
            assert got == want, (L, nb, md)         # every offset; (32, 128) is the shipped geometry


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_restatement_matches_t5_encoder_model_float64(name):
    g, sd, cfg = _tiny(name)
    L = g["positions"]
    assert cfg.inner != cfg.d_model or name == "tiny_b"
    assert int(g["lens"].min()) == 1 and int(g["lens"].max()) == L
    with torch.no_grad():
        out = restated_t5(sd, cfg, g["ids"], g["lens"], dtype=torch.float64)
    ref = g["last_hidden_state"]
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (g["ids"].shape[0], L, cfg.d_model)
    for i in range(ref.shape[0]):
        e = ((out[i] - ref[i]).norm() / ref[i].norm()).item()
        assert e <= 1e-10, (i, e)
    # the fp32 restatement sits where transformers' fp32 run sits (e_ref), and the mask matters
    with torch.no_grad():
        o32 = restated_t5(sd, cfg, g["ids"], g["lens"], dtype=torch.float32).double()
        nomask = restated_t5(sd, cfg, g["ids"], None, dtype=torch.float64)
    for i, er in enumerate(g["e_ref"]):
        assert ((o32[i] - ref[i]).norm() / ref[i].norm()).item() <= 4 * er + 1e-7
    short = int(g["lens"].argmin())
    assert ((nomask[short] - ref[short]).norm() / ref[short].norm()).item() > 1e-3


def test_t5_state_dict_layouts_and_refusals(tmp_path):
    from safetensors.torch import save_file
    g, sd, cfg = _tiny("tiny_a")
    raw = dict(g["state_dict"])
    assert "shared.weight" in raw and "encoder.embed_tokens.weight" in raw          # the tied pair as transformers saves it
    assert cfg == te.T5Config(vocab=raw["shared.weight"].shape[0], d_model=24, d_kv=8, heads=4, d_ff=40, layers=2, positions=7)
    assert te.infer_t5_config(sd, None, positions=7) == cfg                          # the same geometry from the shapes alone
    assert set(sd) == set(te.t5_param_shapes(cfg))
    # pipeline prefix, either name of the tied embedding, a bare stack, fp16 / bf16 input
    for variant in ({"text_encoder." + k: v for k, v in raw.items()},
                    {k: v for k, v in raw.items() if k != "shared.weight"},
                    {k: v for k, v in raw.items() if k != "encoder.embed_tokens.weight"},
                    {k[len("encoder."):]: v for k, v in raw.items() if k.startswith("encoder.")}):
        n = te.normalize_t5_state_dict(variant)
        assert set(n) == set(sd) and all(torch.equal(n[k], sd[k]) for k in sd)
    for dt in (torch.float16, torch.bfloat16):
        n = te.normalize_t5_state_dict({k: v.to(dt) for k, v in raw.items()})
        assert all(v.dtype == torch.float32 for v in n.values())
        assert torch.equal(n["shared.weight"], raw["shared.weight"].to(dt).float())
    # refusals: unknown, missing, wrong shape, another activation
    with pytest.raises(ValueError, match="foreign"):
        te.normalize_t5_state_dict(dict(raw, **{"text_model.embeddings.token_embedding.weight": torch.zeros(2, 2)}))
    with pytest.raises(ValueError, match="foreign"):
        te.check_t5_state_dict(dict(sd, **{"encoder.block.7.layer.0.layer_norm.weight": torch.zeros(24)}), cfg)
    with pytest.raises(ValueError, match="missing"):
        te.check_t5_state_dict({k: v for k, v in sd.items() if k != "encoder.final_layer_norm.weight"}, cfg)
    with pytest.raises(ValueError, match="shape"):
        te.check_t5_state_dict(dict(sd, **{"encoder.block.1.layer.1.DenseReluDense.wo.weight": torch.zeros(24, 41)}), cfg)
    with pytest.raises(ValueError, match="gated-gelu"):
        te.infer_t5_config(sd, dict(g["config"], feed_forward_proj="relu"))
    # a pipeline root with one file, a bare folder, one state_dict file: all recognised as T5
    root = tmp_path / "pipe"
    os.makedirs(root / "text_encoder")
    shutil.copytree(os.path.join(GOLD, "tokenizer"), str(root / "tokenizer"))
    with open(root / "text_encoder" / "config.json", "w") as f:
        json.dump(g["config"], f)
    save_file({k: v.contiguous() for k, v in raw.items() if k != "encoder.embed_tokens.weight"},
              str(root / "text_encoder" / "model.safetensors"))
    c1, s1, tok_dir = te.load_text_encoder(str(root), positions=7)
    assert isinstance(c1, te.T5Config) and c1 == cfg and tok_dir == str(root / "tokenizer")
    assert set(s1) == set(sd) and all(torch.equal(s1[k], sd[k]) for k in sd)
    c2, s2, t2 = te.load_text_encoder(str(root / "text_encoder"), positions=7)
    assert c2 == cfg and t2 is None
    torch.save(raw, str(tmp_path / "t5.pt"))
    c3, s3, _ = te.load_text_encoder(str(tmp_path / "t5.pt"), positions=7)
    assert c3 == cfg and all(torch.equal(s3[k], sd[k]) for k in sd)
    # a two-shard folder with an index file: read one shard at a time
    sh = tmp_path / "sharded"
    os.makedirs(sh)
    with open(sh / "config.json", "w") as f:
        json.dump(g["config"], f)
    keys = [k for k in raw if k != "encoder.embed_tokens.weight"]
    parts = {"model-00001-of-00002.safetensors": keys[:len(keys) // 2], "model-00002-of-00002.safetensors": keys[len(keys) // 2:]}
    for fn, ks in parts.items():
        save_file({k: raw[k].half().contiguous() for k in ks}, str(sh / fn))
    with open(sh / "model.safetensors.index.json", "w") as f:
        json.dump({"metadata": {}, "weight_map": {k: fn for fn, ks in parts.items() for k in ks}}, f)
    c4, shards, _ = te.load_text_encoder(str(sh), positions=7)
    assert c4 == cfg and isinstance(shards, te.T5Shards) and set(shards.names) == set(sd)
    got, count = {}, 0
    for part in shards:
        assert 0 < len(part) < len(sd)
        got.update(part); count += 1
    assert count == 2 and set(got) == set(sd)
    assert all(torch.equal(v.float(), sd[k].half().float()) for k, v in got.items())    # upcast by the loader, per tensor
    with open(sh / "model.safetensors.index.json", "w") as f:       # a name the index lacks
        json.dump({"weight_map": {k: fn for fn, ks in parts.items() for k in ks if "final_layer_norm" not in k}}, f)
    with pytest.raises(ValueError, match="missing"):
        te.load_text_encoder(str(sh), positions=7)
