"""Diagnostic (by hand): bit-for-bit A/B of the encoder units of every library under tests/diag/lib on one box (LOCO_HIP_LIB) --
the check behind a change of the kernels or launch sequences the encoders share (csrc/encoder_kernels.hip, encoder_common.h's
pre_ln_block / add_clip_layer), which must leave every output bit of every encoder alone.

Each library runs in a fresh child process under its own time limit, on the committed fixtures under tests/golden (seeded
inputs where a fixture has none):

* CLIP text (clip_text/tiny_*): n = 1 and n = max_prompts;
* T5 (t5_text/tiny_*): the fixture's prompts with their unequal lengths -- it shares only the transpose;
* CLIP vision (clip_vision/tiny_a, tiny_b: T = 17 and 82, heads of 16 and 80 -- less than one key chunk, a partial second chunk
  and the second output channel): the uint8 preprocessing, `encode` with hidden and pooled outputs at n = 1 and at the full
  batch, `encode_taps`, and with grad enabled `encode` then `encode_vjp` (the kernel that keeps the softmax statistics, and the
  cotangent kernels);
* SAM (sam/tiny_a, tiny_b and the three wide-head geometries of test_gpu_sam_wide_heads.py, heads of 80, 96 and 65): a padded
  window, a window equal to the grid, global layers at exactly one chunk and at several, the bias tables with hd > 64;
* the SAM mask decoder (sam/tiny_a, tiny_b through mask_segmentation.SamHeadHip: both cross-attention kernels in every layer):
  masks and IoU scores for one prompt and for all of the fixture's;
* CLIPSeg (clipseg/seg_*): its preprocessing, the taps of the tower and the decoder's logits.

A child prints one line per output with its sha256.  The parent stops at the first child that does not exit 0 and exits
non-zero if any two libraries differ on any line.

    python tests/diag/enc_bits.py            # ENC_BITS_TIMEOUT=<seconds per library>, default 300
"""
import hashlib
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIBDIR = os.path.join(ROOT, "tests/diag/lib")
GOLD = os.path.join(ROOT, "tests", "golden")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def child():
    sys.path.insert(0, ROOT)
    import torch
    import loco_edit_amd  # noqa: F401
    from loco_edit_amd import clip_score as cs, mask_segmentation as ms, prompt_mask as pm, text_encoder as te
    from loco_edit_amd.hip import LocoClipVisionEngine, LocoSamEngine, LocoTextEngine
    dev = torch.device("cuda:0")

    def put(*what):
        *name, t = what
        print(*name, hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest(), flush=True)

    for name in ("tiny_quick_gelu", "tiny_gelu"):
        g = torch.load(os.path.join(GOLD, "clip_text", f"{name}.pt"))
        sd = te.normalize_text_state_dict(dict(g["state_dict"]))
        n = g["ids"].shape[0]
        eng = LocoTextEngine(te.infer_text_config(sd, g["config"]), max_prompts=n + 2, device=dev)
        eng.load_state_dict(sd)
        put("clip_text", name, "n1", eng.encode_ids(g["ids"][:1]))
        put("clip_text", name, "nmax", eng.encode_ids(torch.cat([g["ids"], g["ids"][:2]])))

    for name in ("tiny_a", "tiny_b"):
        g = torch.load(os.path.join(GOLD, "t5_text", f"{name}.pt"))
        sd = te.normalize_t5_state_dict(dict(g["state_dict"]))
        eng = LocoTextEngine(te.infer_t5_config(sd, g["config"], positions=g["positions"]), max_prompts=8, device=dev)
        eng.load_state_dict(sd)
        assert len(set(g["lens"].tolist())) > 1
        put("t5", name, "lens", eng.encode_ids(g["ids"], lens=g["lens"]))

    for name in ("tiny_a", "tiny_b"):
        g = torch.load(os.path.join(GOLD, "clip_vision", f"{name}.pt"))
        sd = {k: (v.float() if v.is_floating_point() else v) for k, v in g["state_dict"].items()}
        vision, _, vproj, _ = cs.split_clip_state_dict(sd)
        vcfg = cs.infer_vision_config(vision, vproj, g["config"]["vision_config"])
        vsd = dict(vision, **{"visual_projection.weight": vproj})
        pv = g["pixel_values"]
        n = pv.shape[0]
        for grad in (False, True):
            eng = LocoClipVisionEngine(vcfg, max_images=n, device=dev, grad=grad)
            eng.load_state_dict(vsd)
            tag = "grad" if grad else "plain"
            for k, x in (("n1", pv[:1]), ("nfull", pv)):
                for what, t in zip(("embeds", "hidden", "pooled"), eng.encode(x, want_hidden=True)):
                    put("clip_vision", name, tag, k, what, t)
            if grad:
                ge = torch.randn(n, vcfg.projection_dim, generator=torch.Generator().manual_seed(11))
                put("clip_vision", name, "encode_vjp", eng.encode_vjp(ge))
            else:
                put("clip_vision", name, "preprocess", eng.preprocess(g["frames"].to(dev)))
                layers = list(range(vcfg.layers))
                put("clip_vision", name, "taps_all", eng.encode_taps(pv, layers))
                put("clip_vision", name, "taps_first", eng.encode_taps(pv[:1], layers[:1]))

    host = _load("sam_host", "test_sam_host.py")
    cases = []
    for name in ("tiny_a", "tiny_b"):
        g = host.load_tiny(name)
        cases.append((name, g["cfg"].vision, ms.vision_state_dict(g["sd"], g["cfg"].vision), g["pixel_values"]))
    for heads, hd in ((2, 80), (1, 96), (2, 65)):
        cfg = ms.SamVisionConfig(image_size=40, patch_size=4, hidden_size=heads * hd, num_hidden_layers=3, num_attention_heads=heads,
                                 mlp_dim=96, window_size=4, global_attn_indexes=(1,), output_channels=32, num_pos_feats=16)
        cases.append((f"wide{hd}", cfg, host.synthetic_vision_sd(cfg, seed=100 + hd),
                      torch.randn(3, 40, 40, generator=torch.Generator().manual_seed(7))))
    for name, cfg, vis, pv in cases:
        eng = LocoSamEngine(cfg, device=dev)
        eng.load_state_dict(vis)
        put("sam", name, "encode", eng.encode(pv))

    for name in ("tiny_a", "tiny_b"):
        g = host.load_tiny(name)
        head = ms.SamHeadHip(g["cfg"], g["sd"], device=dev)
        emb = g["image_embeddings"].float()
        for k, pts in (("p1", g["points"][:1]), ("pall", g["points"])):
            masks, iou = head.predict(emb, pts)
            put("samdec", name, k, "masks", masks)
            put("samdec", name, k, "iou", iou)

    tok = os.path.join(GOLD, "clip_text", "tokenizer_sd1")
    for name in ("seg_a", "seg_b"):
        g = torch.load(os.path.join(GOLD, "clipseg", f"{name}.pt"))
        ref = os.path.join(GOLD, "clipseg", f"{name}_ref.pt")
        if os.path.exists(ref):
            g.update(torch.load(ref))
        sd = {k: (v.float() if v.is_floating_point() else v) for k, v in g["state_dict"].items()}
        parts = pm.parts_from_state_dict(sd, g["config"], g["preprocessor"], tok, max_masks=8)
        mk = pm.PromptMasker(parts, te.CLIPTokenizer.from_dir(tok), device=dev, max_images=3)
        cond = mk.conditional_embeddings(g["prompts"])
        taps = mk.vision.encode_taps(g["pixel_values"], parts.extract_layers)
        put("clipseg", name, "pixel_values", mk.pixel_values(g["frames"]))
        put("clipseg", name, "cond", cond)
        put("clipseg", name, "taps", taps)
        put("clipseg", name, "logits", mk.decoder.decode(taps, cond[g["prompt_of_mask"]], g["image_of_mask"]))


def main():
    libs = sorted(f for f in os.listdir(LIBDIR) if f.endswith(".so"))
    if len(libs) < 2:
        sys.exit(f"need at least two libraries under {LIBDIR}, found {libs}")
    limit = os.environ.get("ENC_BITS_TIMEOUT", "300")
    lines = {}
    for l in libs:
        env = dict(os.environ, LOCO_HIP_LIB=os.path.join(LIBDIR, l))
        r = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--child"], env=env,
                           capture_output=True, text=True)
        if r.returncode != 0:      # nothing more is started on the GPU after a child that failed
            print(r.stdout[-2000:], r.stderr[-2000:], sep="\n")
            sys.exit(f"{l}: child exited {r.returncode}")
        lines[l] = r.stdout.splitlines()
        print(f"{l}: {len(lines[l])} lines", flush=True)
    ref = libs[0]
    bad = 0
    for l in libs[1:]:
        if len(lines[l]) != len(lines[ref]):
            print(f"{l}: {len(lines[l])} lines, {ref}: {len(lines[ref])}")
            bad += 1
        for a, b in zip(lines[ref], lines[l]):
            if a != b:
                print(f"- {ref}: {a}\n+ {l}: {b}")
                bad += 1
    for a in lines[ref]:
        print(a)
    print(f"{len(libs)} libraries, {len(lines[ref])} lines each: " + ("IDENTICAL" if not bad else f"{bad} DIFFERENCES"))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    child() if sys.argv[1:] == ["--child"] else main()
