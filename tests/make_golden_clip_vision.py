"""Writes tests/golden/clip_vision/ (run by hand where `transformers` is installed; not collected by pytest): two small
seeded CLIPModels, the smallest geometries at which the kernels of csrc/clipvis.hip can go wrong.

* tiny_a: image 32, patch 8 (T = 17 tokens: fewer than one key chunk of 64, not a multiple of 16), width 64, 4 heads (head
  width 16), 2 layers, quick_gelu, projection 24; 3 images, so n T = 51 needs padding columns.  Frames 48 x 40 (a
  downsampling resize and a crop).
* tiny_b: image 72, patch 8 (T = 82: two key chunks, the second partial), width 160, 2 heads (head width 80 > 64: a lane of
  the attention kernel owns two channels), 2 layers, gelu, projection 32; 2 images.  Frames 40 x 56 (an upsampling resize).

Each file: `config` (the CLIPConfig as a dict), `state_dict` (CLIPModel naming; the values are bf16-representable and stored
as bf16 to halve the file, the models below ran on their fp32 upcast), `frames` (uint8 [n, H, W, 3]), `pixel_values`
(CLIPImageProcessor, PIL backend), `last_hidden_state` / `pooler_output` / `image_embeds` of CLIPVisionModelWithProjection on
them, `image_embeds_device` (the same model on the float64 restatement of the preprocessing, test_clip_score_host.py, rounded
to fp32), `prompts`, `ids`, `text_embeds` of CLIPTextModelWithProjection.  The tokenizer is tests/golden/clip_text/tokenizer_sd1.
frames[0] is the "original" of the score tests: the others and the two prompts are far enough apart for the directional
similarity to be well conditioned (asserted here and in the test).

    python tests/make_golden_clip_vision.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "clip_vision")
TOK = os.path.join(ROOT, "tests", "golden", "clip_text", "tokenizer_sd1")
PROMPTS = ["a photo of a man", "a photo of a man wearing glasses"]

GEOMETRIES = {
    "tiny_a": dict(image_size=32, patch_size=8, width=64, heads=4, layers=2, mlp=128, act="quick_gelu", proj=24, n=3, frame=(48, 40),
                   text_width=32),
    "tiny_b": dict(image_size=72, patch_size=8, width=160, heads=2, layers=2, mlp=32, act="gelu", proj=32, n=2, frame=(40, 56),
                   text_width=48),
}


def main():
    import transformers
    from test_clip_score_host import restated_preprocess, smooth_noise_image
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(TOK, "vocab.json")) as f:
        vocab = json.load(f)
    tok = transformers.CLIPTokenizer.from_pretrained(TOK)
    ids = torch.tensor([tok(s, padding="max_length", max_length=77, truncation=True).input_ids for s in PROMPTS], dtype=torch.int64)
    for seed, (name, g) in enumerate(GEOMETRIES.items()):
        vc = dict(image_size=g["image_size"], patch_size=g["patch_size"], hidden_size=g["width"], num_attention_heads=g["heads"],
                  num_hidden_layers=g["layers"], intermediate_size=g["mlp"], hidden_act=g["act"], layer_norm_eps=1e-5,
                  projection_dim=g["proj"])
        tc = dict(vocab_size=len(vocab), hidden_size=g["text_width"], num_attention_heads=2, num_hidden_layers=2,
                  intermediate_size=2 * g["text_width"], max_position_embeddings=77, hidden_act=g["act"], layer_norm_eps=1e-5,
                  projection_dim=g["proj"], bos_token_id=vocab["<|startoftext|>"], eos_token_id=vocab["<|endoftext|>"],
                  pad_token_id=vocab["<|endoftext|>"])
        cfg = transformers.CLIPConfig(text_config=tc, vision_config=vc, projection_dim=g["proj"])
        torch.manual_seed(21 + seed)
        model = transformers.CLIPModel(cfg).eval()
        with torch.no_grad():
            for k, v in model.named_parameters():
                if "norm" in k or k.endswith("bias"):      # layer norms and biases away from their 1 / 0 initialisation
                    v.add_(0.1 * torch.randn(v.shape))
                elif "projection" in k or k.endswith("proj.weight") or ".fc" in k or "patch_embedding" in k:
                    v.mul_(4.0)                            # the 0.02-scale initialisation leaves the attention flat: sharpen it
                v.copy_(v.to(torch.bfloat16).float())
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        vis = transformers.CLIPVisionModelWithProjection(cfg.vision_config).eval()
        txt = transformers.CLIPTextModelWithProjection(cfg.text_config).eval()
        for part, prefix, head in ((vis, "vision_model.", "visual_projection.weight"), (txt, "text_model.", "text_projection.weight")):
            miss, unexp = part.load_state_dict({k: v for k, v in sd.items() if k.startswith(prefix) or k == head}, strict=False)
            assert not unexp and all(k.endswith("position_ids") for k in miss), (miss, unexp)
        H, W = g["frame"]
        frames = torch.stack([smooth_noise_image(H, W, seed=100 * seed + i, noise=0.15) for i in range(g["n"])])
        S = g["image_size"]
        proc = transformers.CLIPImageProcessor(size={"shortest_edge": S}, crop_size={"height": S, "width": S})
        pv = proc(images=[f.numpy() for f in frames], return_tensors="pt")["pixel_values"]
        with torch.no_grad():
            o = vis(pixel_values=pv)
            pooled = vis.vision_model(pixel_values=pv).pooler_output
            od = vis(pixel_values=restated_preprocess(frames, S).to(torch.float32))
            t = txt(input_ids=ids)
        emb, temb = o.image_embeds.double(), t.text_embeds.double()
        cond = [float((emb[i] - emb[0]).norm() / emb[0].norm()) for i in range(1, g["n"])] + [float((temb[1] - temb[0]).norm() / temb[0].norm())]
        print(name, "difference norms relative to the embedding norm:", ["%.3f" % c for c in cond])
        assert min(cond) > 1e-3
        keep = dict(cfg.to_dict())
        config = {"projection_dim": g["proj"], "vision_config": {k: keep["vision_config"][k] for k in vc},
                  "text_config": {k: keep["text_config"][k] for k in tc}}
        out = {"config": config, "state_dict": {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in sd.items()},
               "frames": frames, "pixel_values": pv, "last_hidden_state": o.last_hidden_state, "pooler_output": pooled,
               "image_embeds": o.image_embeds, "image_embeds_device": od.image_embeds, "prompts": PROMPTS, "ids": ids,
               "text_embeds": t.text_embeds}
        for k, v in sd.items():
            assert not v.is_floating_point() or torch.equal(v.to(torch.bfloat16).float(), v), k
        path = os.path.join(OUT, f"{name}.pt")
        torch.save(out, path)
        print("wrote", path, os.path.getsize(path), "bytes")
    print("transformers", transformers.__version__)


if __name__ == "__main__":
    main()
