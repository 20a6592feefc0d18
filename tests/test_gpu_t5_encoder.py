"""GPU tests of the T5 text encoder (csrc/t5enc.hip through hip.LocoTextEngine / text_encoder.TextEncoder):

* tiny fixtures: HIP against T5EncoderModel's float64 outputs (tests/golden/t5_text/tiny_*.pt), rel-L2 <= 2e-5 per prompt,
  printed next to e_ref (transformers' own fp32 run against the same float64 states);
* each row bit-identical alone, at every position of a max_prompts batch, and whatever the other prompts' lengths;
* bad ids / lengths / n / parameters and the masked call on a CLIP handle refused as errors;
* at size: the XXL geometry (and the t5-v1.1-small shape, inner != d_model) with weights seeded on the device against the
  float64 restatement of test_t5_host.py on the device, rel-L2 <= 1e-4; the encode time by HIP events, unasserted;
* end to end: EditDeepFloydIF on TINY_IF with --text_encoder_path, and the shipped IF script's arguments through the CLI."""
import importlib.util
import json
import os
import shutil
import statistics
import sys
import zlib
from argparse import Namespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import text_encoder as te  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(ROOT, "tests", "golden", "t5_text")
_spec = importlib.util.spec_from_file_location("t5_host", os.path.join(ROOT, "tests", "test_t5_host.py"))
_host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_host)
restated_t5 = _host.restated_t5


def rel_rows(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return [((a[i] - b[i]).norm() / b[i].norm()).item() for i in range(a.shape[0])]


def _tiny(name, max_prompts):
    from loco_edit_amd.hip import LocoTextEngine
    g = torch.load(os.path.join(GOLD, f"{name}.pt"))
    sd = te.normalize_t5_state_dict(dict(g["state_dict"]))
    cfg = te.infer_t5_config(sd, g["config"], positions=g["positions"])
    eng = LocoTextEngine(cfg, max_prompts=max_prompts, device=torch.device(DEV))
    eng.load_state_dict(sd)
    return g, sd, cfg, eng


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_tiny_t5_vs_transformers_float64(name):
    g, sd, cfg, eng = _tiny(name, 8)
    out = eng.encode_ids(g["ids"], lens=g["lens"])
    assert tuple(out.shape) == (g["ids"].shape[0], cfg.positions, cfg.d_model)
    errs = rel_rows(out, g["last_hidden_state"])
    for i, (e, er) in enumerate(zip(errs, g["e_ref"])):
        print(f"{name} prompt {i} (len {int(g['lens'][i])}): HIP vs float64 {e:.2e}   e_ref (transformers fp32 vs float64) {er:.2e}"
              f"   ratio {e / er:.2f}")
    assert max(errs) <= 2e-5
    # the padded query rows are part of the comparison above; without the mask a short prompt is visibly another result
    short = int(g["lens"].argmin())
    nomask = eng.encode_ids(g["ids"][short:short + 1])
    assert rel_rows(nomask, g["last_hidden_state"][short:short + 1])[0] > 1e-3
    # lens=None means every prompt is L long, through either entry point
    full = int(g["lens"].argmax())
    assert torch.equal(eng.encode_ids(g["ids"][full:full + 1])[0], out[full])


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_t5_rows_are_bit_identical_in_any_batch(name):
    g, sd, cfg, eng = _tiny(name, 8)
    ids, lens = g["ids"], g["lens"]
    n, mp, L = ids.shape[0], 8, cfg.positions
    out = eng.encode_ids(ids, lens=lens)
    for i in range(n):                                     # alone
        assert torch.equal(eng.encode_ids(ids[i:i + 1], lens=lens[i:i + 1])[0], out[i])
    rep = (mp + n - 1) // n
    bi, bl, bo = ids.repeat(rep, 1)[:mp], lens.repeat(rep)[:mp], out.repeat(rep, 1, 1)[:mp]
    for r in range(mp):                                    # every row at every position of a full batch
        got = eng.encode_ids(torch.roll(bi, r, dims=0), lens=torch.roll(bl, r, dims=0))
        assert torch.equal(got, torch.roll(bo, r, dims=0)), r
    for i in range(n):                                     # the neighbours' lengths changed (every row checked)
        for other in (1, max(1, L // 2), L):
            l2 = torch.full((mp,), other, dtype=lens.dtype)
            at = i % mp
            b2 = bi.clone()
            b2[at], l2[at] = ids[i], lens[i]
            assert torch.equal(eng.encode_ids(b2, lens=l2)[at], out[i]), (i, other)
    os.environ["LOCO_PRECISION"] = "f16"                   # the result does not depend on the conv arithmetic switch
    try:
        assert torch.equal(eng.encode_ids(ids, lens=lens), out)
    finally:
        os.environ.pop("LOCO_PRECISION")


def test_t5_refusals_are_errors():
    from loco_edit_amd.hip import LocoTextEngine
    g, sd, cfg, eng = _tiny("tiny_a", 3)
    ids, lens = g["ids"][:2], g["lens"][:2]
    for v in (cfg.vocab, -1):
        bad = ids.clone()
        bad[1, 6] = v                                      # a padded position counts: it is embedded and returned
        with pytest.raises(RuntimeError, match="outside"):
            eng.encode_ids(bad, lens=lens)
    for v in (0, cfg.positions + 1, -3):
        with pytest.raises(RuntimeError, match="length"):
            eng.encode_ids(ids, lens=[int(lens[0]), v])
    with pytest.raises(ValueError, match="lens"):
        eng.encode_ids(ids, lens=[1])
    with pytest.raises(RuntimeError, match="max_prompts"):
        eng.encode_ids(g["ids"][:4], lens=g["lens"][:4])
    ok = eng.encode_ids(ids, lens=lens)                    # the handle works after the refusals
    assert torch.equal(ok, eng.encode_ids(ids, lens=lens))
    part = LocoTextEngine(cfg, max_prompts=1, device=torch.device(DEV))
    with pytest.raises(RuntimeError, match="missing"):
        part.load_state_dict({k: v for k, v in sd.items() if k != "encoder.final_layer_norm.weight"})
    with pytest.raises(RuntimeError, match="missing parameter encoder.final_layer_norm.weight"):
        part.encode_ids(ids[:1], lens=lens[:1])
    with pytest.raises(RuntimeError, match="unknown parameter"):
        part.load_state_dict({"encoder.block.9.layer.0.SelfAttention.q.weight": torch.zeros(2)})
    with pytest.raises(RuntimeError, match="unknown parameter"):       # the bias table exists in block 0 only
        part.load_state_dict({"encoder.block.1.layer.0.SelfAttention.relative_attention_bias.weight": torch.zeros(32, 4)})
    with pytest.raises(RuntimeError, match="shape"):
        part.load_state_dict({"encoder.block.0.layer.0.SelfAttention.q.weight": torch.zeros(24, 32)})
    import dataclasses
    with pytest.raises(RuntimeError, match="positions"):
        LocoTextEngine(dataclasses.replace(cfg, positions=129), max_prompts=1, device=torch.device(DEV))
    clip = LocoTextEngine(te.TextConfig(vocab=50, width=16, layers=1, heads=2, ffn=32, positions=7), max_prompts=2,
                          device=torch.device(DEV))
    with pytest.raises(RuntimeError, match="CLIP"):
        clip.encode_ids(torch.zeros(1, 7, dtype=torch.int32), lens=[3])


# -------------------------------------------------------------------------------------------------------------- at size
class SeededT5:
    """The state_dict of a seeded T5 encoder whose tensors are made on the device when asked for (and made again, bit for
    bit, when asked again): nothing but the engine holds all 19 GB of the XXL geometry."""

    def __init__(self, cfg, seed):
        self.cfg, self.seed, self.shapes = cfg, seed, te.t5_param_shapes(cfg)

    def keys(self):
        return self.shapes.keys()

    def __getitem__(self, k):
        c = self.cfg
        g = torch.Generator(device=DEV).manual_seed(zlib.crc32(f"{self.seed}:{k}".encode()))
        r = torch.randn(*self.shapes[k], generator=g, device=DEV)
        if "layer_norm" in k:
            return 1 + 0.1 * r
        if k == "shared.weight" or "relative_attention_bias" in k:
            return r                                       # unit embedding rows; a bias of the size of the scores
        if ".q." in k:                                     # scores of standard deviation 2: a softmax that is neither flat nor one-hot
            return r * (2.0 / (c.d_kv ** 0.5 * c.d_model ** 0.5))
        fan_in = self.shapes[k][1]
        return r * fan_in ** -0.5


def _time_encode(eng, ids, lens, out, warm=2, reps=7):
    for _ in range(warm):
        eng.encode_ids(ids, out=out, lens=lens)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.encode_ids(ids, out=out, lens=lens)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


@pytest.mark.parametrize("which", ["small", "xxl"])
def test_t5_at_size_vs_float64_restatement(which):
    from loco_edit_amd.hip import LocoTextEngine
    cfg = te.T5_XXL if which == "xxl" else te.T5Config(d_model=512, d_kv=64, heads=6, d_ff=1024, layers=8)
    assert which == "xxl" or cfg.inner != cfg.d_model
    sd = SeededT5(cfg, 3)
    eng = LocoTextEngine(cfg, max_prompts=5, device=torch.device(DEV))
    for k in sd.keys():                                    # one tensor at a time, through device pointers
        eng.load_params({k: sd[k]})
    eng.check_complete()
    nparam = sum(int(torch.tensor(s).prod()) for s in sd.shapes.values())
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(2, cfg.vocab, (5, 77), generator=g)
    lens = torch.tensor([77, 1, 6, 40, 76])
    for p, ln in enumerate(lens.tolist()):
        ids[p, ln - 1] = 1
        ids[p, ln:] = 0
    out = eng.encode_ids(ids, lens=lens)
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = restated_t5(sd, cfg, ids.to(DEV), lens, dtype=torch.float64)
        r32 = restated_t5(sd, cfg, ids.to(DEV), lens, dtype=torch.float32)
    errs, eref = rel_rows(out, ref), rel_rows(r32, ref)
    for p in range(5):
        print(f"{which} prompt {p} (len {int(lens[p])}): HIP vs float64 restatement {errs[p]:.2e}   e_ref (torch fp32 restatement vs "
              f"float64) {eref[p]:.2e}   ratio {errs[p] / eref[p]:.2f}")
    assert max(errs) <= 1e-4
    # encode time (HIP events, medians; a record, no threshold) next to the two bounds of the shape
    gemm_params = nparam - cfg.vocab * cfg.d_model
    for n in (1, 5):
        med, lo, hi = _time_encode(eng, ids[:n].to(DEV), lens[:n], out[:n])
        Tp = (n * 77 + 15) // 16 * 16
        print(f"{which} n={n}: encode {med:.2f} ms median of 7 (min {lo:.2f}, max {hi:.2f}); bounds: weights {4e-9 * nparam:.2f} GB "
              f"at 8.0 TB/s spec / 6.29 TB/s measured copy rate = {4 * nparam / 8e12 * 1e3:.2f} / {4 * nparam / 6.29e12 * 1e3:.2f} ms, "
              f"exact-fp32 MFMA 2 x {gemm_params:.3g} x Tp {Tp} at 157.3 TFLOP/s = {2 * gemm_params * Tp / 157.3e12 * 1e3:.2f} ms")
    print(f"{which}: resident parameters {4e-9 * nparam:.2f} GB, torch allocator peak {torch.cuda.max_memory_allocated() / 1e9:.2f} GB "
          "(the restatement; the engine's own allocations are outside it)")


def test_t5_heads_wider_than_a_wave_vs_restatement():
    """d_kv = 80 > 64: a lane of the attention kernel owns a second output channel (c = lane + 64), inner = 160 != d_model;
    L = 70 keeps the second key slot live for the full-length prompt and leaves the last round of the 4 waves partly empty;
    lens 70 / 1 / 37 are a full, a one-key and a first-slot-only prompt.  Bound: the file's rel-L2 <= 1e-4 against the
    float64 restatement."""
    from loco_edit_amd.hip import LocoTextEngine
    cfg = te.T5Config(d_model=48, d_kv=80, heads=2, d_ff=64, layers=1, positions=70)
    assert cfg.inner != cfg.d_model
    sd = SeededT5(cfg, 5)
    eng = LocoTextEngine(cfg, max_prompts=3, device=torch.device(DEV))
    eng.load_state_dict({k: sd[k] for k in sd.keys()})
    ids = torch.randint(2, cfg.vocab, (3, cfg.positions), generator=torch.Generator().manual_seed(11))
    lens = torch.tensor([70, 1, 37])
    for p, ln in enumerate(lens.tolist()):
        ids[p, ln - 1] = 1
        ids[p, ln:] = 0
    out = eng.encode_ids(ids, lens=lens)
    with torch.no_grad():
        ref = restated_t5(sd, cfg, ids.to(DEV), lens, dtype=torch.float64)
        r32 = restated_t5(sd, cfg, ids.to(DEV), lens, dtype=torch.float32)
    errs, eref = rel_rows(out, ref), rel_rows(r32, ref)
    for p in range(3):
        print(f"d_kv 80 prompt {p} (len {int(lens[p])}): HIP vs float64 restatement {errs[p]:.2e}   e_ref (torch fp32 restatement vs "
              f"float64) {eref[p]:.2e}   ratio {errs[p] / eref[p]:.2f}")
    assert max(errs) <= 1e-4
    for i in range(3):
        assert torch.equal(eng.encode_ids(ids[i:i + 1], lens=lens[i:i + 1])[0], out[i])


# ---------------------------------------------------------------------------------------------------------- end to end
def _write_pipeline(root, name="tiny_a"):
    """A diffusers-layout IF text encoder from a fixture: text_encoder/ (config.json + model.safetensors) + tokenizer/."""
    from safetensors.torch import save_file
    g = torch.load(os.path.join(GOLD, f"{name}.pt"))
    os.makedirs(os.path.join(root, "text_encoder"))
    with open(os.path.join(root, "text_encoder", "config.json"), "w") as f:
        json.dump(g["config"], f)
    save_file({k: v.contiguous() for k, v in g["state_dict"].items() if k != "encoder.embed_tokens.weight"},
              os.path.join(root, "text_encoder", "model.safetensors"))
    shutil.copytree(os.path.join(GOLD, "tokenizer"), os.path.join(root, "tokenizer"))
    return root


def test_text_encoder_from_a_sharded_folder_and_a_tokenizer_path(tmp_path):
    """A two-shard fp16 checkpoint folder (index file + shards, loaded shard by shard) with the tokenizer given on its own."""
    from safetensors.torch import save_file
    g, sd, cfg, eng = _tiny("tiny_a", 4)
    sh = tmp_path / "text_encoder"
    os.makedirs(sh)
    with open(sh / "config.json", "w") as f:
        json.dump(g["config"], f)
    keys = sorted(sd)
    parts = {"model-00001-of-00002.safetensors": keys[::2], "model-00002-of-00002.safetensors": keys[1::2]}
    for fn, ks in parts.items():
        save_file({k: sd[k].half().contiguous() for k in ks}, str(sh / fn))
    with open(sh / "model.safetensors.index.json", "w") as f:
        json.dump({"metadata": {}, "weight_map": {k: fn for fn, ks in parts.items() for k in ks}}, f)
    enc = te.TextEncoder(str(sh), tokenizer_path=os.path.join(GOLD, "tokenizer"), device=torch.device(DEV), max_prompts=4, positions=7)
    assert enc.kind == "t5" and enc.cfg == cfg
    eng.load_state_dict({k: v.half().float() for k, v in sd.items()})
    prompts = ["a photo of a man", "", "red hair, smiling", "A PHOTO", "zebra", "glasses glasses glasses glasses glasses glasses"]
    ids, lens = enc.tokenizer.batch([p.lower().strip() for p in prompts])
    out = enc.encode(prompts)                              # six prompts through max_prompts = 4: two calls
    assert tuple(out.shape) == (6, 7, 24)
    assert torch.equal(out, torch.cat([eng.encode_ids(ids[:4], lens=lens[:4]), eng.encode_ids(ids[4:], lens=lens[4:])]))
    with pytest.raises(ValueError, match="tokenizer_path"):
        te.TextEncoder(str(sh), device=torch.device(DEV), positions=7)


def _if_args(tmp_path, **kw):
    from loco_edit_amd.config import TINY_IF
    a = dict(device=torch.device(DEV), dtype=torch.float32, seed=1, unet_config=TINY_IF, synthetic_weights=0, ckpt_path="",
             max_batch=8, precision="f32", dataset_name="Random", for_steps=100, use_yh_custom_scheduler=True, guidance_scale=7.5,
             guidance_scale_edit=4.0, prompt_emb=None, prompt_emb_path="", text_encoder_path="", tokenizer_path="",
             for_prompt="A photo of a man", edit_prompt=" A photo of a man wearing glasses ", neg_prompt="", edit_t=0.6,
             sampling_mode=False, tilda_v_score_type="null+(for-null)+(edit-null)", ablation_method="null-space-proj",
             mask_type="SAM", vT_path="", x_space_guidance_edit_step=1.0, x_space_guidance_scale=0.5,
             x_space_guidance_num_step=16, result_folder=str(tmp_path / "res"), model_name="DeepFloyd/IF-I-M-v1.0")
    a.update(kw)
    return Namespace(**a)


def test_deepfloyd_if_class_with_t5_text_encoder(tmp_path):
    from loco_edit_amd.config import MID_IF, TINY_DECODER, TINY_LDM
    from loco_edit_amd.tloco import EditDeepFloydIF
    from loco_edit_amd.tloco_sd import EditStableDiffusion
    os.environ.pop("WORLD_SIZE", None)
    root = _write_pipeline(str(tmp_path / "pipe"))
    ed = EditDeepFloydIF(_if_args(tmp_path, text_encoder_path=root))
    enc = ed.text_encoder
    assert enc.kind == "t5" and enc.length == 7 and enc.width == 24
    # the five states of the one batched encode = the encoder on the lower-cased, stripped prompts
    want = enc.encode(["a photo of a man", "a photo of a man wearing glasses", "", "", ""])
    for k, i in (("for", 0), ("edit", 1), ("null", 2), ("neg", 3), ("inv", 4)):
        assert tuple(ed._text_pe[k].shape) == (1, 7, 24) and torch.equal(ed._text_pe[k][0], want[i]), k
    assert torch.equal(ed.for_prompt_emb, ed._text_pe["for"]) and torch.equal(ed.edit_prompt_emb, ed._text_pe["edit"])
    assert torch.equal(ed.null_prompt_emb, ed._text_pe["null"])
    ids, lens = enc.tokenizer.batch(["a photo of a man", ""])
    assert lens.tolist() == [6, 1] and torch.equal(enc.engine.encode_ids(ids, lens=lens), want[[0, 2]])
    assert torch.equal(ed._get_prompt_emb("  A Cat "), enc.encode(["a cat"]))
    # another edit prompt: re-encoded, and a different semantic direction
    x = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(DEV)
    t = ed.scheduler.timesteps[ed.edit_t_idx]
    mask = torch.zeros(3, 32, 32, dtype=torch.bool)
    mask[:, 12:20, 8:18] = True
    v0 = ed.get_delta_xt_via_grad(x, t, ed.edit_t_idx, ed.for_prompt_emb, ed.edit_prompt_emb, ed.null_prompt_emb, mask=mask.to(DEV))
    before = ed.edit_prompt_emb
    ed._set_edit_prompt("red hair, smiling")
    assert ed.edit_prompt == "red hair, smiling" and not torch.equal(ed.edit_prompt_emb, before)
    assert torch.equal(ed.edit_prompt_emb, enc.encode(["red hair, smiling"]))
    v1 = ed.get_delta_xt_via_grad(x, t, ed.edit_t_idx, ed.for_prompt_emb, ed.edit_prompt_emb, ed.null_prompt_emb, mask=mask.to(DEV))
    cos = float((v0 * v1).sum() / (v0.norm() * v1.norm()))
    print("semantic direction cos between the two edit prompts:", cos)
    assert abs(cos) < 0.9999
    # a driver's edit_prompt argument does the same (sampling_mode: the driver returns before it edits)
    os.makedirs(os.path.join(ed.result_folder, "mask"), exist_ok=True)
    masks = torch.zeros(2, 1, 32, 32, dtype=torch.bool)
    masks[1, 0, 12:20, 8:18] = True
    torch.save(masks, os.path.join(ed.result_folder, "mask", "mask.pt"))
    ed.sampling_mode = True
    ed.run_edit_null_space_projection_xt_semantic(op="mid", block_idx=0, vis_num=1, mask_index=1, pca_rank=1,
                                                  edit_prompt="a man with a beard", null_space_projection=True, pca_rank_null=2)
    assert ed.edit_prompt == "a man with a beard" and torch.equal(ed.edit_prompt_emb, enc.encode(["a man with a beard"]))
    # width mismatch names both; the kinds of encoder are told apart before any geometry
    with pytest.raises(ValueError, match="d_model 24.*encoder_dim 128"):
        EditDeepFloydIF(_if_args(tmp_path, text_encoder_path=root, unet_config=MID_IF))
    with pytest.raises(NotImplementedError, match="T5"):
        EditStableDiffusion(_if_args(tmp_path, text_encoder_path=root, unet_config=TINY_LDM, vae_config=TINY_DECODER,
                                     vae_ckpt_path="", inv_prompt="", use_sega=False))


def test_cli_shipped_if_script_with_t5_text_encoder(tmp_path, monkeypatch):
    from loco_edit_amd.config import TINY_IF
    from loco_edit_amd.main import main
    argv = json.load(open(os.path.join(ROOT, "tests", "golden", "script_args.json")))["main_T2I_DeepFloydIF_null_space_projection.sh"]
    assert "--prompt_emb_path" not in argv
    root = _write_pipeline(str(tmp_path / "pipe"))
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("LOCO_PRECISION", "bf16x3")
    rdir = tmp_path / "runs" / "DeepFloyd-IF-Random-with_prompt" / "results" / "for_prompt_A photo of a man_cfg7.5_seed2628577915_M"
    os.makedirs(rdir / "mask")
    masks = torch.zeros(13, 1, 32, 32, dtype=torch.bool)
    masks[12, 0, 12:20, 8:18] = True
    torch.save(masks, str(rdir / "mask" / "mask.pt"))
    x0 = main(argv + ["--device", DEV, "--unet_preset", "tiny_if", "--synthetic_weights", "0", "--text_encoder_path", root])
    assert x0.dtype == torch.uint8 and tuple(x0.shape) == (3, 32, 32, 3)
    pcs = [f for f in os.listdir(rdir / "basis") if f.endswith(".pt")]
    assert pcs, "no direction saved"
    # the same run on seeded states is another picture: the prompts drove this one
    x1 = main(argv + ["--device", DEV, "--unet_preset", "tiny_if", "--synthetic_weights", "0"])
    assert not torch.equal(x0, x1)
    # the two ways to give the states exclude each other, and a tokenizer folder can be given on its own
    with pytest.raises(ValueError, match="pass one of them"):
        main(argv + ["--device", DEV, "--unet_preset", "tiny_if", "--synthetic_weights", "0", "--text_encoder_path", root,
                     "--prompt_emb_path", "x.pt"])
    assert TINY_IF.encoder_dim == 24 and TINY_IF.context_len == 7
