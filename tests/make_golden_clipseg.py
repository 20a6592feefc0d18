"""Writes tests/golden/clipseg/ (run by hand where `transformers` is installed; not collected by pytest): two small seeded
CLIPSegForImageSegmentation models, the smallest geometries at which the kernels of csrc/clipseg.hip and the taps of
csrc/clipvis.hip can go wrong.

* seg_a: tower patch 8, native image 32, RUN AT 48 (G = 6, T = 37 tokens: fewer than one key chunk, not a multiple of 16; the
  position table interpolated 4^2 -> 6^2), width 64, 4 heads, 4 layers.  Decoder: extract_layers [0, 1, 3] (not contiguous, the
  last layer included), reduce_dim 16, 2 heads (head width 8), ffn 64, conditional_layer 0, the simple head (logits 48^2).
  2 images of 40 x 56 (both axes resized differently), 3 prompts; masks 0-2 on image 0, mask 3 (prompt 0) on image 1.  resample 2.
* seg_b: tower patch 16, native 64, run at 144 (G = 9, T = 82: two key chunks, the second partial), width 96, 2 heads (head
  width 48), 3 layers, gelu.  Decoder: extract_layers [0, 1, 2], reduce_dim 64 with 4 heads (the real decoder geometry, head
  width 16), ffn 128, conditional_layer 1, the complex head (kernels 4 and 4, logits 144^2).  1 image of 120 x 200, 2 prompts.
  resample 3.

Weights: seeded, layer norms and biases moved off 1 / 0, the towers' matrices x 4 as in make_golden_clip_vision.py, the
decoder's x 2; the LAST layer of the head is then rescaled and its bias shifted so that the float64 logits of every mask have
a standard deviation inside [1, 5] and 20 % .. 80 % of their pixels above the threshold 0.5 (asserted; the x 4 recipe on the
decoder saturates it).  All values bf16-representable, stored as bf16; the models ran on the fp32 upcast.

seg_b is written as two files, seg_b.pt (the model, the prompts and their ids) and seg_b_ref.pt (the frames and everything computed): one file
would pass 1 MiB.  Each fixture: `config` (CLIPSegConfig as a dict), `preprocessor` (the preprocessor_config.json), `state_dict`, `run_size`, `frames`
(uint8 [n, H, W, 3]), `pixel_values` (the float64 restatement prompt_mask.restated_preprocess, rounded to fp32), `prompts`,
`ids`, `image_of_mask`, `prompt_of_mask`, `taps` [n_taps, n, T, D] (hidden_states[l + 1] for l in extract_layers),
`position_table` (what transformers adds at the run size), `cond` (conditional embeddings per prompt), `logits` (fp32 model)
and `logits64` (model.double(), the reference), `fp32_err` (rel-L2 of the two per mask), `threshold`, and per resolution in
`resized` (40: downsampling, 200: upsampling) the `masks` of the float64 bilinear resize of logits64 and `near` (pixels within
1e-3 of the threshold logit; at most 0.5 % per mask, asserted), both bit-packed, and at 40 the resized `logits` themselves (at
200 they would double the file: prompt_mask.restated_masks on `logits64` gives them again).

    python tests/make_golden_clipseg.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "clipseg")
TOK = os.path.join(ROOT, "tests", "golden", "clip_text", "tokenizer_sd1")
THRESHOLD, NEAR, NEAR_CAP = 0.5, 1e-3, 0.005
RESOLUTIONS = (40, 200)
FILM_GAIN, REDUCE_GAIN = 8.0, 0.03

GEOMETRIES = {
    "seg_a": dict(native=32, run=48, patch=8, width=64, heads=4, layers=4, mlp=128, act="quick_gelu", proj=24, text_width=32,
                  extract=[0, 1, 3], rd=16, dheads=2, dffn=64, cond_layer=0, complex=False, n=2, frame=(40, 56), resample=2,
                  prompts=["hair", "the eyes", "a smiling mouth"], image_of_mask=[0, 0, 0, 1], prompt_of_mask=[0, 1, 2, 0]),
    "seg_b": dict(native=64, run=144, patch=16, width=96, heads=2, layers=3, mlp=96, act="gelu", proj=32, text_width=32,
                  extract=[0, 1, 2], rd=64, dheads=4, dffn=128, cond_layer=1, complex=True, n=1, frame=(120, 200), resample=3,
                  prompts=["the sky", "a red car"], image_of_mask=[0, 0], prompt_of_mask=[0, 1]),
}


def pack(bits):
    """bool [M, res, res] -> uint8 [M, ceil(res^2 / 8)] (numpy.packbits; test_gpu_clipseg.py unpacks)"""
    return torch.from_numpy(np.packbits(bits.flatten(1).numpy(), axis=1))


def run(model, pv, ids, g):
    iom, pom = g["image_of_mask"], g["prompt_of_mask"]
    with torch.no_grad():
        return model(pixel_values=pv[iom], input_ids=ids[pom], interpolate_pos_encoding=True, output_hidden_states=True)


def main():
    import transformers
    from test_clip_score_host import smooth_noise_image
    import loco_edit_amd  # noqa: F401
    from loco_edit_amd import prompt_mask as pm
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(TOK, "vocab.json")) as f:
        vocab = json.load(f)
    tok = transformers.CLIPTokenizer.from_pretrained(TOK)
    for seed, (name, g) in enumerate(GEOMETRIES.items()):
        vc = dict(image_size=g["native"], patch_size=g["patch"], hidden_size=g["width"], num_attention_heads=g["heads"],
                  num_hidden_layers=g["layers"], intermediate_size=g["mlp"], hidden_act=g["act"], layer_norm_eps=1e-5)
        tc = dict(vocab_size=len(vocab), hidden_size=g["text_width"], num_attention_heads=2, num_hidden_layers=2,
                  intermediate_size=2 * g["text_width"], max_position_embeddings=77, hidden_act=g["act"], layer_norm_eps=1e-5,
                  bos_token_id=vocab["<|startoftext|>"], eos_token_id=vocab["<|endoftext|>"], pad_token_id=vocab["<|endoftext|>"])
        top = dict(projection_dim=g["proj"], extract_layers=g["extract"], reduce_dim=g["rd"], decoder_num_attention_heads=g["dheads"],
                   decoder_intermediate_size=g["dffn"], conditional_layer=g["cond_layer"],
                   use_complex_transposed_convolution=g["complex"])
        cfg = transformers.CLIPSegConfig(text_config=tc, vision_config=vc, **top)
        torch.manual_seed(41 + seed)
        model = transformers.CLIPSegForImageSegmentation(cfg).eval()
        last = "decoder.transposed_convolution.4." if g["complex"] else "decoder.transposed_convolution."
        with torch.no_grad():
            for k, v in model.named_parameters():
                if "norm" in k or k.endswith("bias"):      # layer norms and biases away from their 1 / 0 initialisation
                    v.add_(0.1 * torch.randn(v.shape))
                elif k.startswith("clip.") and ("projection" in k or k.endswith("proj.weight") or ".fc" in k or "patch_embedding" in k):
                    v.mul_(4.0)                            # the 0.02-scale initialisation leaves the attention flat: sharpen it
                elif k.startswith("decoder.film") and k.endswith("weight"):
                    v.mul_(FILM_GAIN)                      # or the prompt barely moves the state
                elif k.startswith("decoder.reduces") and k.endswith("weight"):
                    v.mul_(REDUCE_GAIN)                    # or the later taps drown the conditioned state
                elif k.startswith("decoder.") and k.endswith("weight"):
                    v.mul_(2.0)
                v.copy_(v.to(torch.bfloat16).float())
        ids = torch.tensor([tok(s, padding="max_length", max_length=77, truncation=True).input_ids for s in g["prompts"]], dtype=torch.int64)
        H, W = g["frame"]
        frames = torch.stack([smooth_noise_image(H, W, seed=300 + 100 * seed + i, noise=0.15) for i in range(g["n"])])
        pre = pm.Preprocess(size=g["run"], resample=g["resample"])
        pv = pm.restated_preprocess(frames, pre).to(torch.float32)
        # the last layer of the head: scale and shift so that the logits are neither flat nor saturated
        model.double()
        with torch.no_grad():
            lg = run(model, pv.double(), ids, g).logits
            w, b = (dict(model.named_parameters())[last + s] for s in ("weight", "bias"))
            a = 2.5 / float(lg.flatten(1).std(dim=1).mean())
            w.mul_(a)
            b.copy_(a * b - a * float(lg.flatten(1).median(dim=1).values.mean()))
            for v in (w, b):
                v.copy_(v.to(torch.bfloat16).double())
        o64 = run(model, pv.double(), ids, g)
        lg64 = o64.logits
        for k, v in model.state_dict().items():
            assert not v.is_floating_point() or torch.equal(v.to(torch.bfloat16).double(), v), k
        sd = {k: v.float().clone() if v.is_floating_point() else v.clone() for k, v in model.state_dict().items()}
        model.float()
        model.load_state_dict(sd)
        o32 = run(model, pv, ids, g)
        with torch.no_grad():
            cond = model.clip.get_text_features(ids).pooler_output
            emb = model.clip.vision_model.embeddings
            pos = emb.interpolate_pos_encoding(torch.zeros(1, 1 + (g["run"] // g["patch"]) ** 2, g["width"]), g["run"], g["run"])[0]
        n = g["n"]
        first = [g["image_of_mask"].index(i) for i in range(n)]         # a mask of every image: its row of the batched hidden states
        taps = torch.stack([o32.vision_model_output.hidden_states[l + 1][first] for l in g["extract"]])
        fp32_err = [float((o32.logits[m].double() - lg64[m]).norm() / lg64[m].norm()) for m in range(lg64.shape[0])]
        std = lg64.flatten(1).std(dim=1)
        share = (lg64 > pm.threshold_logit(THRESHOLD)).flatten(1).double().mean(dim=1)
        print(name, "logit std", [f"{v:.2f}" for v in std.tolist()], "share above threshold", [f"{v:.2f}" for v in share.tolist()],
              "fp32_err", [f"{v:.2e}" for v in fp32_err])
        assert bool(((std >= 1) & (std <= 5)).all()) and bool(((share >= 0.2) & (share <= 0.8)).all())
        differ = [float((lg64[i] > 0).ne(lg64[j] > 0).double().mean()) for i in range(len(lg64)) for j in range(i)]
        print(name, "share of pixels on which two masks differ:", [f"{v:.3f}" for v in differ])
        assert min(differ) > 0.01
        resized = {}
        for res in RESOLUTIONS:
            r, mk = pm.restated_masks(lg64, res, THRESHOLD)
            near = (r - pm.threshold_logit(THRESHOLD)).abs() <= NEAR
            print(name, "res", res, "pixels near the threshold per mask:", near.flatten(1).sum(dim=1).tolist())
            assert float(near.flatten(1).double().mean(dim=1).max()) <= NEAR_CAP
            resized[res] = {"masks": pack(mk), "near": pack(near)}
            if res <= 64:
                resized[res]["logits"] = r
        keep = cfg.to_dict()
        config = dict({k: keep[k] for k in top}, vision_config={k: keep["vision_config"][k] for k in vc},
                      text_config={k: keep["text_config"][k] for k in tc})
        preprocessor = {"size": {"height": g["run"], "width": g["run"]}, "resample": g["resample"], "image_mean": list(pm.IMAGENET_MEAN),
                        "image_std": list(pm.IMAGENET_STD), "do_resize": True, "do_rescale": True, "do_normalize": True}
        out = {"config": config, "preprocessor": preprocessor, "run_size": g["run"],
               "state_dict": {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in sd.items() if "position_ids" not in k},
               "frames": frames, "pixel_values": pv, "prompts": g["prompts"], "ids": ids, "image_of_mask": g["image_of_mask"],
               "prompt_of_mask": g["prompt_of_mask"], "taps": taps, "position_table": pos, "cond": cond, "logits": o32.logits,
               "logits64": lg64, "fp32_err": fp32_err, "threshold": THRESHOLD, "resized": resized}
        # two files where one would pass the size of the CLIP fixtures: the model, and what it computed
        parts = {name: out}
        if g["complex"]:
            model_keys = ("config", "preprocessor", "run_size", "state_dict", "prompts", "ids", "image_of_mask", "prompt_of_mask")
            parts = {name: {k: out[k] for k in model_keys}, name + "_ref": {k: v for k, v in out.items() if k not in model_keys}}
        for stem, part in parts.items():
            path = os.path.join(OUT, f"{stem}.pt")
            torch.save(part, path)
            print("wrote", path, os.path.getsize(path), "bytes")
            assert os.path.getsize(path) < 1 << 20
    print("transformers", transformers.__version__)


if __name__ == "__main__":
    main()
