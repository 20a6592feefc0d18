"""GPU tests of the CLIP text encoder (csrc/textenc.hip through hip.LocoTextEngine / text_encoder.TextEncoder):

* tiny fixtures: HIP against transformers' CLIPTextModel outputs (tests/golden/clip_text/tiny_*.pt), rel-L2 <= 2e-5 per
  prompt; each row bit-identical alone and at every position of a max_prompts batch; bad ids / n / parameters refused;
* at size: the SD 1.x and SD 2.x geometries with seeded weights against the float64 restatement of
  test_text_encoder_host.py on the device, rel-L2 <= 1e-4 (and against transformers when it imports);
* end to end: EditStableDiffusion on the tiny_ldm stand-in (context 16 x 7) with --text_encoder_path."""
import importlib.util
import json
import os
import shutil
import sys
import time
from argparse import Namespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import text_encoder as te  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(ROOT, "tests", "golden", "clip_text")
_spec = importlib.util.spec_from_file_location("text_encoder_host", os.path.join(ROOT, "tests", "test_text_encoder_host.py"))
_host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_host)
restated_clip_text = _host.restated_clip_text


def rel_rows(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return [((a[i] - b[i]).norm() / b[i].norm()).item() for i in range(a.shape[0])]


@pytest.mark.parametrize("name", ["tiny_quick_gelu", "tiny_gelu"])
def test_tiny_encoders_vs_transformers_and_batch_invariance(name):
    from loco_edit_amd.hip import LocoTextEngine
    g = torch.load(os.path.join(GOLD, f"{name}.pt"))
    sd = te.normalize_text_state_dict(dict(g["state_dict"]))
    cfg = te.infer_text_config(sd, g["config"])
    n = g["ids"].shape[0]
    eng = LocoTextEngine(cfg, max_prompts=n + 2, device=torch.device(DEV))
    eng.load_state_dict(sd)
    out = eng.encode_ids(g["ids"])
    errs = rel_rows(out, g["last_hidden_state"])
    print(name, "rel-L2 per prompt vs transformers:", ["%.1e" % e for e in errs])
    assert max(errs) <= 2e-5
    # bit-identity: alone, and at every position of a full batch of max_prompts rows
    for i in range(n):
        assert torch.equal(eng.encode_ids(g["ids"][i:i + 1])[0], out[i])
    full = eng.encode_ids(torch.cat([g["ids"], g["ids"][:2]]))
    assert torch.equal(full[:n], out) and torch.equal(full[n:], out[:2])
    rolled = eng.encode_ids(torch.roll(g["ids"], 1, dims=0))
    assert torch.equal(torch.roll(rolled, -1, dims=0), out)
    # refusals: out-of-range ids, n > max_prompts, missing parameters (errors, not aborts)
    bad = g["ids"][:1].clone()
    bad[0, 3] = cfg.vocab
    with pytest.raises(RuntimeError, match="outside"):
        eng.encode_ids(bad)
    bad[0, 3] = -1
    with pytest.raises(RuntimeError, match="outside"):
        eng.encode_ids(bad)
    with pytest.raises(RuntimeError, match="max_prompts"):
        eng.encode_ids(g["ids"][:1].repeat(n + 3, 1))
    part = LocoTextEngine(cfg, max_prompts=1, device=torch.device(DEV))
    with pytest.raises(RuntimeError, match="missing"):
        part.load_state_dict({k: v for k, v in sd.items() if k != "final_layer_norm.bias"})
    with pytest.raises(RuntimeError, match="missing parameter final_layer_norm.bias"):
        part.encode_ids(g["ids"][:1])
    with pytest.raises(RuntimeError, match="unknown parameter"):
        part.load_state_dict({"encoder.layers.99.mlp.fc1.weight": torch.zeros(2)})
    # the encoder's result does not depend on the conv arithmetic switch
    os.environ["LOCO_PRECISION"] = "f16"
    try:
        assert torch.equal(eng.encode_ids(g["ids"]), out)
    finally:
        os.environ.pop("LOCO_PRECISION")


def _synth_clip(cfg, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)

    def r(*s, std=0.02):
        return torch.randn(*s, generator=g, device=DEV) * std
    D, F = cfg.width, cfg.ffn
    sd = {"embeddings.token_embedding.weight": r(cfg.vocab, D), "embeddings.position_embedding.weight": r(cfg.positions, D, std=0.01)}
    for i in range(cfg.layers):
        p = f"encoder.layers.{i}."
        for ln in ("layer_norm1", "layer_norm2"):
            sd[p + ln + ".weight"], sd[p + ln + ".bias"] = 1 + r(D, std=0.1), r(D, std=0.1)
        for m in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[p + f"self_attn.{m}.weight"], sd[p + f"self_attn.{m}.bias"] = r(D, D, std=D ** -0.5), r(D)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = r(F, D, std=D ** -0.5), r(F)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = r(D, F, std=F ** -0.5), r(D)
    sd["final_layer_norm.weight"], sd["final_layer_norm.bias"] = 1 + r(D, std=0.1), r(D, std=0.1)
    return sd


@pytest.mark.parametrize("which", ["sd1", "sd2"])
def test_encoder_at_stable_diffusion_size_vs_restatement(which):
    from loco_edit_amd.hip import LocoTextEngine
    cfg = te.SD1_CLIP_TEXT if which == "sd1" else te.SD2_CLIP_TEXT
    sd = _synth_clip(cfg, 3)
    eng = LocoTextEngine(cfg, max_prompts=5, device=torch.device(DEV))
    eng.load_state_dict(sd)
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, cfg.vocab, (5, 77), generator=g)
    ids[:, 0] = cfg.vocab - 2
    ids[1, 10:] = cfg.vocab - 1                       # padded rows: EOS / pad runs
    ids[2, 5:] = 0
    out = eng.encode_ids(ids)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        eng.encode_ids(ids, out=out)
    torch.cuda.synchronize()
    print(f"{which}: warm 5-prompt encode {1e3 * (time.perf_counter() - t0) / 5:.2f} ms (host-timed, unasserted)")
    with torch.no_grad():
        ref = restated_clip_text(sd, cfg, ids.to(DEV), dtype=torch.float64)
    errs = rel_rows(out, ref)
    print(which, "rel-L2 per prompt vs float64 restatement:", ["%.1e" % e for e in errs])
    assert max(errs) <= 1e-4
    try:
        import transformers
    except Exception:
        return
    hcfg = transformers.CLIPTextConfig(vocab_size=cfg.vocab, hidden_size=cfg.width, intermediate_size=cfg.ffn,
                                       num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads, max_position_embeddings=77,
                                       hidden_act=cfg.act, layer_norm_eps=cfg.ln_eps)
    model = transformers.CLIPTextModel(hcfg).eval()
    missing, unexpected = model.load_state_dict({"text_model." + k: v.cpu() for k, v in sd.items()}, strict=False)
    if missing and not all(k.endswith("position_ids") for k in missing):      # transformers' own naming: try without prefix
        model.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=False)
    with torch.no_grad():
        hs = model.to(DEV)(input_ids=ids.to(DEV)).last_hidden_state
    errs = rel_rows(out, hs)
    print(which, "rel-L2 per prompt vs transformers CLIPTextModel:", ["%.1e" % e for e in errs])
    assert max(errs) <= 1e-4


def test_heads_wider_than_a_wave_vs_restatement():
    """hd = 80 > 64: a lane of the attention kernel owns a second output channel (c = lane + 64); L = 70 keeps the second
    key slot live (keys 64..69) and leaves the last round of the 4 waves partly empty (70 = 17 * 4 + 2).  3 prompts: T = 210
    pads to Tp = 224.  Bound: the file's rel-L2 <= 1e-4 against the float64 restatement."""
    from loco_edit_amd.hip import LocoTextEngine
    cfg = te.TextConfig(vocab=50, width=160, layers=1, heads=2, ffn=64, positions=70)
    sd = _synth_clip(cfg, 5)
    eng = LocoTextEngine(cfg, max_prompts=3, device=torch.device(DEV))
    eng.load_state_dict(sd)
    ids = torch.randint(0, cfg.vocab, (3, cfg.positions), generator=torch.Generator().manual_seed(11))
    out = eng.encode_ids(ids)
    with torch.no_grad():
        ref = restated_clip_text(sd, cfg, ids.to(DEV), dtype=torch.float64)
        r32 = restated_clip_text(sd, cfg, ids.to(DEV), dtype=torch.float32)
    errs, eref = rel_rows(out, ref), rel_rows(r32, ref)
    for p in range(3):
        print(f"hd 80 prompt {p}: HIP vs float64 restatement {errs[p]:.2e}   e_ref (torch fp32 restatement vs float64) {eref[p]:.2e}"
              f"   ratio {errs[p] / eref[p]:.2f}")
    assert max(errs) <= 1e-4
    for i in range(3):
        assert torch.equal(eng.encode_ids(ids[i:i + 1])[0], out[i])


# ---------------------------------------------------------------------------------------------------------- end to end
def _write_pipeline(root, seed=0):
    """A diffusers-layout text encoder of the tiny_ldm geometry (context 16 x 7): text_encoder/ + tokenizer/."""
    with open(os.path.join(GOLD, "tokenizer_sd1", "vocab.json")) as f:
        vocab = len(json.load(f))
    config = {"vocab_size": vocab, "hidden_size": 16, "intermediate_size": 32, "num_hidden_layers": 2, "num_attention_heads": 2,
              "max_position_embeddings": 7, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5}
    cfg = te.infer_text_config({"embeddings.token_embedding.weight": torch.zeros(vocab, 16),
                                "embeddings.position_embedding.weight": torch.zeros(7, 16)}, config)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k in te.text_param_names(cfg):
        shape = {"embeddings.token_embedding.weight": (vocab, 16), "embeddings.position_embedding.weight": (7, 16)}.get(k)
        if shape is None:
            base = k.rsplit(".", 1)[0]
            D, F = 16, 32
            shape = ((F, D) if base.endswith("fc1") else (D, F) if base.endswith("fc2") else (D, D)) if k.endswith("weight") and "norm" not in k \
                else ((F,) if base.endswith("fc1") else (D,))
        v = torch.randn(*shape, generator=g) * (0.3 if len(shape) == 2 else 0.1)
        if "norm" in k and k.endswith("weight"):
            v += 1
        sd["text_model." + k] = v
    sd["text_model.embeddings.position_ids"] = torch.arange(7)[None]
    os.makedirs(os.path.join(root, "text_encoder"))
    with open(os.path.join(root, "text_encoder", "config.json"), "w") as f:
        json.dump(config, f)
    torch.save(sd, os.path.join(root, "text_encoder", "pytorch_model.bin"))
    tok = os.path.join(root, "tokenizer")
    shutil.copytree(os.path.join(GOLD, "tokenizer_sd1"), tok)
    with open(os.path.join(tok, "tokenizer_config.json")) as f:
        tc = json.load(f)
    tc["model_max_length"] = 7
    with open(os.path.join(tok, "tokenizer_config.json"), "w") as f:
        json.dump(tc, f)
    return root


def _sd_args(tmp_path, **kw):
    from loco_edit_amd.config import TINY_DECODER, TINY_LDM
    a = dict(device=torch.device(DEV), dtype=torch.float32, seed=1, unet_config=TINY_LDM, vae_config=TINY_DECODER,
             synthetic_weights=0, ckpt_path="", vae_ckpt_path="", max_batch=8, precision="f32", dataset_name="Random",
             for_steps=100, use_yh_custom_scheduler=True, guidance_scale=7.5, guidance_scale_edit=4.0, prompt_emb=None,
             prompt_emb_path="", text_encoder_path="", tokenizer_path="", for_prompt="a photo of a man",
             edit_prompt="a photo of a man wearing glasses", neg_prompt="", inv_prompt="a photo of a man, portrait",
             edit_t=0.7, sampling_mode=False, tilda_v_score_type="null+(for-null)+(edit-null)", ablation_method="null-space-proj",
             mask_type="SAM", vT_path="", use_sega=False, x_space_guidance_edit_step=1.0, x_space_guidance_scale=0.5,
             x_space_guidance_num_step=16, result_folder=str(tmp_path / "res"))
    a.update(kw)
    return Namespace(**a)


def test_stable_diffusion_class_with_text_encoder(tmp_path):
    from loco_edit_amd.tloco import EditDeepFloydIF
    from loco_edit_amd.tloco_sd import EditStableDiffusion
    os.environ.pop("WORLD_SIZE", None)
    root = _write_pipeline(str(tmp_path / "pipe"))
    ed = EditStableDiffusion(_sd_args(tmp_path, text_encoder_path=root))
    enc = ed.text_encoder
    want = enc.encode(["a photo of a man", "a photo of a man wearing glasses", "", "a photo of a man, portrait"])
    for i, e in enumerate((ed.for_prompt_emb, ed.edit_prompt_emb, ed.null_prompt_emb, ed.inv_prompt_emb)):
        assert tuple(e.shape) == (1, 7, 16) and torch.equal(e[0], want[i])
    assert ed.inv_prompt == "a photo of a man"                       # edit.py:524 naming quirk; the embedding encodes all
    assert torch.equal(ed._get_prompt_emb("a cat"), enc.encode(["a cat"]))
    # the same tensors through --prompt_emb_path: bit-identical CFG noise
    pe_file = str(tmp_path / "pe.pt")
    torch.save({"for": ed.for_prompt_emb.cpu(), "edit": ed.edit_prompt_emb.cpu(), "null": ed.null_prompt_emb.cpu()}, pe_file)
    ed2 = EditStableDiffusion(_sd_args(tmp_path, prompt_emb_path=pe_file))
    assert ed2.text_encoder is None
    z = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(3)).to(DEV)
    t = float(ed.scheduler.timesteps[ed.edit_t_idx])
    mode = "null+(for-null)+(edit-null)"
    n1 = ed._classifer_free_guidance(z, t, ed.for_prompt_emb, ed.edit_prompt_emb, ed.null_prompt_emb, mode, True)
    n2 = ed2._classifer_free_guidance(z, t, ed2.for_prompt_emb, ed2.edit_prompt_emb, ed2.null_prompt_emb, mode, True)
    assert torch.equal(n1, n2)
    # another edit prompt: re-encoded (edit.py:929-931) and a different semantic direction
    mask = torch.zeros(3, 64, 64, dtype=torch.bool)
    mask[:, 20:40, 12:44] = True
    z1 = z[:1].contiguous()
    v0 = ed.get_delta_zt_via_grad(z1, t, ed.edit_t_idx, ed.for_prompt_emb, ed.edit_prompt_emb, ed.null_prompt_emb, mask=mask.to(DEV))
    # (7 positions: BOS, five tokens, EOS -- the new prompt must differ within its first five tokens)
    ed._set_edit_prompt("red hair, smiling")
    assert ed.edit_prompt == "red hair, smiling"
    assert torch.equal(ed.edit_prompt_emb, enc.encode(["red hair, smiling"]))
    v1 = ed.get_delta_zt_via_grad(z1, t, ed.edit_t_idx, ed.for_prompt_emb, ed.edit_prompt_emb, ed.null_prompt_emb, mask=mask.to(DEV))
    cos = float((v0 * v1).sum() / (v0.norm() * v1.norm()))
    print("semantic direction cos between the two edit prompts:", cos)
    assert abs(cos) < 0.9999
    # geometry mismatch, and the IF path
    from loco_edit_amd.config import TINY_LATENT_XATTN
    if (TINY_LATENT_XATTN.context_dim, TINY_LATENT_XATTN.context_len) != (16, 7):
        with pytest.raises(ValueError, match="context_len x context_dim"):
            EditStableDiffusion(_sd_args(tmp_path, text_encoder_path=root, unet_config=TINY_LATENT_XATTN))
    with pytest.raises(NotImplementedError, match="T5"):
        EditDeepFloydIF(_sd_args(tmp_path, text_encoder_path=root))


def test_cli_shipped_sd_script_with_text_encoder(tmp_path, monkeypatch):
    from loco_edit_amd.config import TINY_LDM
    from loco_edit_amd.main import main
    argv = json.load(open(os.path.join(ROOT, "tests", "golden", "script_args.json")))["main_T2I_StableDiffusion_null_space_projection.sh"]
    root = _write_pipeline(str(tmp_path / "pipe"), seed=1)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("LOCO_PRECISION", "bf16x3")
    rdir = tmp_path / "runs" / "Stable_Diffusion-Random-with_prompt" / "results" / "for_prompt_a photo of a man_cfg7.5_seed305186554_standin"
    os.makedirs(rdir / "mask")
    masks = torch.zeros(3, 1, 64, 64, dtype=torch.bool)
    masks[1, 0, 20:40, 12:44] = True
    torch.save(masks, str(rdir / "mask" / "mask.pt"))
    lat, x0 = main(argv + ["--device", DEV, "--unet_preset", "tiny_ldm", "--vae_preset", "tiny_decoder", "--synthetic_weights", "0",
                           "--text_encoder_path", root])
    assert x0.dtype == torch.uint8 and tuple(x0.shape) == (3, 64, 64, 3)
    sdir = rdir / "basis" / 'local_basis-0.7T-"a photo of a man wearing glasses"-pca-rank-1-select-mask1'
    v = torch.load(str(sdir / "vT-modify.pt"))
    assert tuple(v.shape) == (1, TINY_LDM.n) and abs(float(v.norm()) - 1.0) < 1e-4
    assert (rdir / "original.png").exists()
