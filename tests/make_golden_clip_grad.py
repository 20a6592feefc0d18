"""Writes tests/golden/clip_vision/tiny_{a,b}_grad.pt (run by hand where `transformers` is installed; not collected by
pytest): the pixel gradient of transformers' CLIPVisionModelWithProjection on the fixtures of make_golden_clip_vision.py.

Each file: `g_embeds` (seeded cotangent of image_embeds, [n, P] fp32), `grad64` = (d image_embeds / d pixel_values)^T g_embeds
by autograd with the model and the fixture's pixel_values in float64, `grad32` the same in fp32, `err32` the rel-L2 of grad32
against grad64 per image -- the reference's own fp32 error, which the GPU test's bar is a multiple of -- and `text_embed`
(a seeded [P] vector for the guidance-loss test).

    python tests/make_golden_clip_grad.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "clip_vision")


def main():
    import transformers
    for seed, name in enumerate(("tiny_a", "tiny_b")):
        g = torch.load(os.path.join(OUT, f"{name}.pt"))
        sd = {k: (v.float() if v.is_floating_point() else v) for k, v in g["state_dict"].items()}
        cfg = transformers.CLIPConfig(text_config=g["config"]["text_config"], vision_config=g["config"]["vision_config"],
                                      projection_dim=g["config"]["projection_dim"])
        pv = g["pixel_values"]
        gen = torch.Generator().manual_seed(77 + seed)
        g_emb = torch.randn(pv.shape[0], g["config"]["projection_dim"], generator=gen)
        text_embed = torch.randn(g["config"]["projection_dim"], generator=gen)
        grads = {}
        for dtype in (torch.float64, torch.float32):
            vis = transformers.CLIPVisionModelWithProjection(cfg.vision_config).eval()
            miss, unexp = vis.load_state_dict({k: v for k, v in sd.items() if k.startswith("vision_model.") or k == "visual_projection.weight"},
                                              strict=False)
            assert not unexp and all(k.endswith("position_ids") for k in miss), (miss, unexp)
            vis = vis.to(dtype)
            x = pv.to(dtype).clone().requires_grad_(True)
            emb = vis(pixel_values=x).image_embeds
            if dtype == torch.float32:
                assert torch.allclose(emb.detach(), g["image_embeds"], rtol=0, atol=1e-4 * float(g["image_embeds"].abs().max()))
            (emb * g_emb.to(dtype)).sum().backward()
            grads[dtype] = x.grad.detach().clone()
        g64, g32 = grads[torch.float64], grads[torch.float32]
        err = torch.tensor([float((g32[i].double() - g64[i]).norm() / g64[i].norm()) for i in range(pv.shape[0])], dtype=torch.float64)
        print(name, "fp32 autograd against float64, rel-L2 per image:", ["%.2e" % e for e in err.tolist()])
        path = os.path.join(OUT, f"{name}_grad.pt")
        torch.save({"g_embeds": g_emb, "text_embed": text_embed, "grad64": g64, "grad32": g32, "err32": err}, path)
        print("wrote", path, os.path.getsize(path), "bytes")
    print("transformers", transformers.__version__)


if __name__ == "__main__":
    main()
