"""GPU tests of the Segment Anything head in HIP (csrc/samdec.hip through hip.LocoSamHeadEngine, mask_segmentation.SamHeadHip):

1. the decoder alone on the tiny fixtures against SamModel's float64 pred_masks / iou_scores (tests/golden/sam/tiny_*.pt),
   rel-L2 <= max(4 e_ref, 2e-5) with e_ref transformers' own fp32 decoder on the same float64 embeddings;
2. SAM's own decoder width (C 256, 8 heads, mlp 2048) on small grids with seeded weights against SamHead in float64 on the
   host, e_ref = SamHead in fp32 on the host, same bound; C 64 with 8 heads passes or is refused at create;
3. zeroing single parameters moves the output as it moves the float64 reference;
4. bit identity across calls, engines and batch sizes;
5. refusals;
6. score / binarize against MaskGenerator.upsample + stability_score + mask_to_box in float64;
7. SAM(..., head="hip") end to end against the mask-generation pipeline's fixture, SAM(..., head="torch") unchanged."""
import importlib.util
import os
import sys
from argparse import Namespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import mask_segmentation as ms  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(ROOT, "tests", "golden", "sam")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_host = _load("test_sam_host")
rel, bound, load_tiny = _host.rel, _host.bound, _host.load_tiny


def _engine(cfg, sd, max_prompts=64):
    from loco_edit_amd.hip import LocoSamHeadEngine
    eng = LocoSamHeadEngine(cfg, max_prompts=max_prompts, device=torch.device(DEV))
    eng.load_state_dict(ms.head_state_dict(sd, cfg))
    return eng


# ------------------------------------------------------------------------------------- 1. tiny fixtures vs transformers
@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_tiny_decoder_vs_transformers_float64(name):
    g = load_tiny(name)
    head = ms.SamHeadHip(g["cfg"], g["sd"], device=DEV)
    masks, iou = head.predict(g["image_embeddings"].float(), g["points"])
    assert tuple(masks.shape) == tuple(g["pred_masks"].shape) and tuple(iou.shape) == (64, 3)
    em, ei = rel(masks, g["pred_masks"]), rel(iou, g["iou_scores"])
    rm, ri = g["e_ref"]["pred_masks_decoder_only"], g["e_ref"]["iou_scores_decoder_only"]
    print(f"{name}: HIP decoder vs float64: pred_masks {em:.2e} (e_ref {rm:.2e}, ratio {em / rm:.2f})   "
          f"iou_scores {ei:.2e} (e_ref {ri:.2e}, ratio {ei / ri:.2f})")
    assert em <= bound(rm) and ei <= bound(ri)


# ------------------------------------------------------------------------------------------------ 2. SAM's own width
def _cfg(G, C=256, heads=8, mlp=2048, hid=256):
    return ms.SamConfig(ms.SamVisionConfig(image_size=16 * G, patch_size=16, output_channels=C, num_pos_feats=C // 2),
                        ms.SamDecoderConfig(hidden_size=C, num_attention_heads=heads, mlp_dim=mlp, iou_head_hidden_dim=hid))


def _weights(cfg, seed):
    """Seeded head: matrices ~ N(0, 1 / fan_in), LayerNorm 1 / 0 +- 0.1, biases 0.1 N, tokens, embeddings and the positional
    matrix ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in ms.head_param_shapes(cfg).items():
        if "layer_norm" in k:
            t = (1.0 if k.endswith("weight") else 0.0) + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith(".bias"):
            t = 0.1 * torch.randn(shp, generator=g)
        elif k.endswith(("positional_embedding", "_embed.weight", "point_embed.1.weight", "_token.weight", "_tokens.weight")):
            t = torch.randn(shp, generator=g)
        else:
            fan_in = shp[0] if "upscale_conv" in k else torch.Size(shp[1:]).numel()
            t = torch.randn(shp, generator=g) / fan_in ** 0.5
        sd[k] = t
    sd["prompt_encoder.point_embed.0.weight"] = torch.randn(1, cfg.decoder.hidden_size, generator=g)   # read by no point prompt
    return sd


def _inputs(cfg, P, seed):
    g = torch.Generator().manual_seed(seed)
    G, C, S = cfg.vision.grid, cfg.decoder.hidden_size, cfg.vision.image_size
    emb = torch.randn(1, C, G, G, generator=g)
    pts = torch.rand(P, 2, generator=g, dtype=torch.float64) * (S - 1)
    return emb, pts


_CASES = {}


def _case(G, P, C=256, seed=3):
    """(cfg, sd, emb, pts, float64 reference, e_ref of the fp32 host statement), computed once per geometry."""
    key = (G, P, C)
    if key not in _CASES:
        cfg = _cfg(G, C=C, mlp=8 * C, hid=C)
        sd = _weights(cfg, seed)
        emb, pts = _inputs(cfg, P, seed + 1)
        with torch.no_grad():
            m64, i64 = ms.SamHead(cfg, sd, dtype=torch.float64).predict(emb.double(), pts)
            m32, i32 = ms.SamHead(cfg, sd, dtype=torch.float32).predict(emb, pts)
        _CASES[key] = (cfg, sd, emb, pts, (m64, i64), (rel(m32, m64), rel(i32, i64)))
    return _CASES[key]


def _check(label, masks, iou, ref, e_ref):
    em, ei = rel(masks, ref[0]), rel(iou, ref[1])
    print(f"{label}: HIP vs float64: pred_masks {em:.2e} (e_ref {e_ref[0]:.2e}, ratio {em / e_ref[0]:.2f})   "
          f"iou_scores {ei:.2e} (e_ref {e_ref[1]:.2e}, ratio {ei / e_ref[1]:.2f})")
    assert torch.isfinite(masks).all() and torch.isfinite(iou).all()
    assert em <= bound(e_ref[0]) and ei <= bound(e_ref[1])


@pytest.mark.parametrize("G,P", [(8, 64), (5, 5), (7, 1)])
def test_sam_width_decoder_vs_host_float64(G, P):
    cfg, sd, emb, pts, ref, e_ref = _case(G, P)
    eng = _engine(cfg, sd)
    eng.set_image(emb)
    masks, iou = eng.predict(ms.prompt_coords(pts, cfg.vision.image_size))
    assert tuple(masks.shape) == (P, 3, 4 * G, 4 * G) and tuple(iou.shape) == (P, 3)
    _check(f"C 256, G {G}, P {P}", masks, iou, ref, e_ref)


def test_narrow_heads_pass_or_are_refused_at_create():
    cfg, sd, emb, pts, ref, e_ref = _case(7, 7, C=64)               # 8 heads of 8 (self) and 4 (cross) channels
    try:
        eng = _engine(cfg, sd)
    except RuntimeError as ex:
        print("refused:", ex)
        assert "loco_samdec_create" in str(ex) and len(str(ex)) > len("loco_samdec_create failed (-1): loco_samdec_create: ")
        return
    eng.set_image(emb)
    masks, iou = eng.predict(ms.prompt_coords(pts, cfg.vision.image_size))
    _check("C 64, 8 heads, G 7, P 7", masks, iou, ref, e_ref)


# --------------------------------------------------------------------------------------------------- 3. sensitivity
_ZEROED = [("prompt_encoder.no_mask_embed.weight", 0), ("prompt_encoder.not_a_point_embed.weight", 0),
           ("prompt_encoder.point_embed.1.weight", 0),
           ("mask_decoder.transformer.layers.1.cross_attn_image_to_token.out_proj.bias", 0),
           ("mask_decoder.transformer.layers.1.layer_norm4.bias", 0), ("mask_decoder.upscale_layer_norm.bias", 0),
           ("mask_decoder.output_hypernetworks_mlps.3.proj_out.bias", 0), ("mask_decoder.iou_prediction_head.layers.0.bias", 1)]


@pytest.mark.parametrize("key,which", _ZEROED)
def test_zeroed_parameter_moves_the_output_as_it_moves_the_reference(key, which):
    cfg, sd, emb, pts, ref, e_ref = _case(8, 64)
    coords = ms.prompt_coords(pts, cfg.vision.image_size)
    eng = _engine(cfg, sd)
    eng.set_image(emb)
    base = [t.clone() for t in eng.predict(coords)]
    zsd = {**sd, key: torch.zeros_like(sd[key])}
    eng.load_params({key: zsd[key]})                                # one tensor replaced on the live engine
    eng.set_image(emb)
    moved = eng.predict(coords)
    with torch.no_grad():
        ref0 = ms.SamHead(cfg, zsd, dtype=torch.float64).predict(emb.double(), pts)
    d_hip, d_ref = rel(moved[which], base[which]), rel(ref0[which], ref[which])
    floor = 10 * bound(e_ref[which])
    print(f"{key} zeroed: {'iou_scores' if which else 'pred_masks'} move by {d_hip:.4e} (HIP), {d_ref:.4e} (float64), "
          f"ratio {d_hip / d_ref:.4f}; 10 x bound = {floor:.2e}")
    assert d_hip > floor
    assert abs(d_hip - d_ref) <= 0.01 * d_ref


# --------------------------------------------------------------------------------------------------- 4. determinism
def test_bit_identity_across_calls_engines_and_batch_sizes():
    g = load_tiny("tiny_a")
    cfg, sd = g["cfg"], g["sd"]
    emb = g["image_embeddings"].float().to(DEV)
    coords = ms.prompt_coords(g["points"], cfg.vision.image_size)
    eng = _engine(cfg, sd)
    eng.set_image(emb)
    m0, i0 = [t.clone() for t in eng.predict(coords)]
    assert torch.isfinite(m0).all() and torch.isfinite(i0).all()
    eng.set_image(torch.randn_like(emb))                            # another image in between
    eng.predict(coords[:5])
    eng.set_image(emb)
    m1, i1 = eng.predict(coords)
    assert torch.equal(m0, m1) and torch.equal(i0, i1)
    other = _engine(cfg, sd)
    other.set_image(emb)
    m2, i2 = other.predict(coords)
    assert torch.equal(m0, m2) and torch.equal(i0, i2)
    for p in range(64):                                             # a prompt's rows do not depend on the batch
        mp, ip = other.predict(coords[p: p + 1])
        assert torch.equal(mp[0], m0[p]) and torch.equal(ip[0], i0[p]), p


def test_head_sets_the_image_again_only_for_another_embedding():
    g = load_tiny("tiny_a")
    head = ms.SamHeadHip(g["cfg"], g["sd"], device=DEV)
    calls = []
    real = head.engine.set_image
    head.engine.set_image = lambda e: (calls.append(1), real(e))[1]
    emb = g["image_embeddings"].float().to(DEV)
    a = head.predict(emb, g["points"][:8])[0].clone()
    head.predict(emb, g["points"][8:16])
    assert len(calls) == 1
    other = torch.randn_like(emb)
    head.predict(other, g["points"][:8])
    b = head.predict(emb, g["points"][:8])[0]
    assert len(calls) == 3 and torch.equal(a, b)
    emb.mul_(2.0)                                                   # the same tensor, written to
    head.predict(emb, g["points"][:8])
    assert len(calls) == 4
    assert head.image_pe() is None and head.cfg is g["cfg"]


# ------------------------------------------------------------------------------------------------------ 5. refusals
def test_engine_refuses_bad_parameters_prompts_and_grids():
    from loco_edit_amd.hip import LocoSamHeadEngine
    g = load_tiny("tiny_a")
    cfg = g["cfg"]
    sd = ms.head_state_dict(g["sd"], cfg)
    fresh = LocoSamHeadEngine(cfg, max_prompts=4, device=torch.device(DEV))
    with pytest.raises(RuntimeError, match="parameters missing"):
        fresh.load_state_dict({k: v for k, v in sd.items() if k != "mask_decoder.upscale_conv2.bias"})
    with pytest.raises(RuntimeError, match="parameters missing|missing parameter"):
        fresh.set_image(g["image_embeddings"].float())
    k = "mask_decoder.transformer.layers.0.mlp.lin1.weight"
    with pytest.raises(RuntimeError, match="mlp.lin1.weight has shape"):
        fresh.load_params({k: sd[k].t().contiguous()})
    with pytest.raises(RuntimeError, match="unknown parameter"):
        fresh.load_params({"prompt_encoder.point_embed.0.weight": torch.zeros(1, 32)})
    fresh.load_state_dict(sd)
    coords = ms.prompt_coords(g["points"], cfg.vision.image_size)
    with pytest.raises(RuntimeError, match="no image set"):
        fresh.predict(coords[:4])
    fresh.set_image(g["image_embeddings"].float())
    with pytest.raises(ValueError, match="max_prompts = 4"):
        fresh.predict(coords[:5])
    buf = [coords[:5].to(DEV).contiguous(), torch.empty(5, 3, 32, 32, device=DEV), torch.empty(5, 3, device=DEV)]
    rc = fresh.lib.loco_samdec_predict(fresh._t, buf[0].data_ptr(), 5, buf[1].data_ptr(), buf[2].data_ptr(), None)   # the C call itself
    assert rc != 0 and b"outside [1, max_prompts = 4]" in fresh.lib.loco_samdec_last_error(fresh._t)
    with pytest.raises(ValueError, match=r"must be \[1, 32, 8, 8\]"):
        fresh.set_image(torch.zeros(1, 32, 14, 14))                  # tiny_b's grid
    masks, iou = fresh.predict(coords[:4])                          # the refusals left the engine usable
    assert torch.isfinite(masks).all() and torch.isfinite(iou).all()
    bad = ms.SamConfig(cfg.vision, ms.SamDecoderConfig(hidden_size=48, num_attention_heads=2, mlp_dim=64, iou_head_hidden_dim=32))
    with pytest.raises(RuntimeError, match="loco_samdec_create: hidden must be"):
        LocoSamHeadEngine(bad, device=torch.device(DEV))


# ---------------------------------------------------------------------------------------------- 6. score / binarize
def _score_cases():
    g = torch.load(os.path.join(GOLD, "generator.pt"))
    thr, off = float(g["thresholds"]["mask_threshold"]), float(g["thresholds"]["stability_score_offset"])
    cases = []
    for grp in g["groups"]:
        left, top, right, bottom = grp["crop_box"]
        cases.append((grp["low_res"].float().flatten(0, 1), (bottom - top, right - left), tuple(grp["reshaped_size"]), g["image_size"], thr, off))
    gen = torch.Generator().manual_seed(9)
    low = 3.0 * torch.randn(5, 32, 32, generator=gen)               # 5 candidates: no multiple of anything
    low[3] = -1.0 - torch.rand(32, 32, generator=gen)               # all below threshold - offset ... empty mask
    low[4] = 2.0 + torch.rand(32, 32, generator=gen)                # all above threshold + offset
    cases.append((low, (75, 100), (96, 128), 128, 0.5, 1.0))        # a crop and two different scale factors
    return cases


_SCORE_CASES = _score_cases()


@pytest.mark.parametrize("case", range(len(_SCORE_CASES)))
def test_score_and_binarize_vs_the_generator_in_float64(case):
    from loco_edit_amd.hip import LocoSamHeadEngine
    low, size, resh, S, thr, off = _SCORE_CASES[case]
    N = low.shape[0]
    ref = ms.MaskGenerator.upsample(low.double()[:, None], size, resh, S)[:, 0]           # [N, H, W] float64
    assert tuple(ref.shape) == (N,) + tuple(size)
    tol = 1e-4 * ref.flatten(1).pow(2).mean(1).sqrt()[:, None, None]
    und = {t: (ref - t).abs() <= tol for t in (thr + off, thr - off, thr)}
    for t, u in und.items():
        frac = u.flatten(1).float().mean(1).max().item()
        assert frac < 0.01, (t, frac)
    ref_counts = torch.stack([(ref > thr + off).flatten(1).sum(1), (ref > thr - off).flatten(1).sum(1)], dim=1)
    ref_boxes = ms.mask_to_box(ref > thr)
    eng = LocoSamHeadEngine(load_tiny("tiny_a")["cfg"], device=torch.device(DEV))         # no parameters needed
    counts, boxes = eng.score(low, size, resh, S, thr, off)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (N, 2) and tuple(boxes.shape) == (N, 4)
    counts, boxes = counts.cpu().long(), boxes.cpu().long()
    allow = torch.stack([und[thr + off].flatten(1).sum(1), und[thr - off].flatten(1).sum(1)], dim=1)
    worst = (counts - ref_counts).abs()
    print(f"case {case}: N {N}, count differences up to {int(worst.max())}, undecided pixels up to {int(allow.max())}; "
          f"empty masks {int((ref_counts[:, 1] == 0).sum())}, full masks {int((ref_counts[:, 0] == ref[0].numel()).sum())}")
    assert (worst <= allow).all()
    checked = 0
    for n in range(N):
        x0, y0, x1, y1 = [int(v) for v in ref_boxes[n]]
        u = und[thr][n]
        if not (u[y0].any() or u[y1].any() or u[:, x0].any() or u[:, x1].any()):
            assert boxes[n].tolist() == [x0, y0, x1, y1], n
            checked += 1
    assert checked >= N // 2
    rows = torch.tensor([r for r in range(N) if r % 3 != 1][::-1])                         # a subset, out of order
    masks = eng.binarize(low, rows, size, resh, S, thr).cpu()
    assert masks.dtype == torch.bool and tuple(masks.shape) == (rows.numel(),) + tuple(size)
    want, decided = (ref > thr)[rows], ~und[thr][rows]
    assert torch.equal(masks[decided], want[decided])
    assert tuple(eng.binarize(low, rows[:0], size, resh, S, thr).shape) == (0,) + tuple(size)
    if case == len(_SCORE_CASES) - 1:
        assert boxes[3].tolist() == [0, 0, 0, 0] and counts[3].tolist() == [0, 0]
        assert boxes[4].tolist() == [0, 0, size[1] - 1, size[0] - 1] and counts[4].tolist() == [size[0] * size[1]] * 2


# ---------------------------------------------------------------------------------------------------- 7. end to end
def test_end_to_end_with_the_hip_head_vs_the_mask_generation_pipeline(tmp_path):
    _model_folder = _load("test_gpu_sam")._model_folder
    m = torch.load(os.path.join(GOLD, "end_to_end_model.pt"))
    e = torch.load(os.path.join(GOLD, "end_to_end.pt"))
    args = Namespace(mask_model_path=_model_folder(tmp_path, m), device=torch.device(DEV), filter_mask=100)
    sam = ms.SAM(args, str(tmp_path / "run"), head="hip", **e["thresholds"])
    assert isinstance(sam.head, ms.SamHeadHip) and sam.scorer is sam.head
    image = m["image"].numpy()
    masks, scores, boxes = sam.segment(image)
    n = e["masks"].shape[0]
    assert masks.shape[0] == n >= 3 and tuple(masks.shape[1:]) == (96, 128) and masks.dtype == torch.bool
    masks, scores = masks.cpu(), scores.cpu().double()
    print("scores", [round(float(s), 5) for s in scores], "fixture", [round(float(s), 5) for s in e["scores"]])
    assert (scores - e["scores"]).abs().max().item() <= 1e-4                       # and so the same order: gaps >= 1e-3
    assert torch.equal(torch.argsort(scores, descending=True), torch.arange(n))
    for i in range(n):
        d = e["decided"][i]
        wrong = int((masks[i][d] != e["masks"][i][d]).sum())
        print(f"mask {i}: {int(masks[i].sum())} pixels, decided {float(d.float().mean()):.4f}, differing decided pixels {wrong}, "
              f"differing pixels {int((masks[i] != e['masks'][i]).sum())}")
        assert wrong == 0
    assert torch.equal(boxes.cpu().float(), e["boxes"])
    out = sam.mask_segmentation(image, resolution=32)
    assert out.dtype == torch.bool and tuple(out.shape) == (n, 32, 32)
    saved = torch.load(os.path.join(sam.log_dir, "mask.pt"))
    assert saved.dtype == torch.bool and tuple(saved.shape) == (n, 32, 32) and torch.equal(saved, out)
    ref = torch.round(torch.nn.functional.interpolate(e["masks"].unsqueeze(1).float(), [32, 32]).squeeze(1)).bool()
    assert (out != ref).sum().item() <= int((~e["decided"]).sum())
    assert os.path.exists(os.path.join(sam.log_dir, "total_mask.png"))
    big = [i for i in range(n) if int(masks[i].sum()) > 100]
    assert big and all(os.path.exists(os.path.join(sam.log_dir, f"mask_{i}.png")) for i in big)
    assert not any(os.path.exists(os.path.join(sam.log_dir, f"mask_{i}.png")) for i in range(n) if i not in big)
    assert set(sam.last_timing) == {"encoder_ms", "decoder_generator_ms"}
    print("timing of the last call (ms):", {k: round(v, 2) for k, v in sam.last_timing.items()})
    # the torch head on the same input: what it returns today, and the default
    for kw in ({"head": "torch"}, {}):
        ts = ms.SAM(args, str(tmp_path / "run_torch"), **kw, **e["thresholds"])
        assert type(ts.head) is ms.SamHead and ts.scorer is None
    tm, tsc, tb = ts.segment(image)
    assert tm.shape[0] == n and torch.equal(tb.cpu().float(), e["boxes"]) and (tsc.cpu().double() - e["scores"]).abs().max().item() <= 1e-4
    assert all(int((tm[i].cpu()[e["decided"][i]] != e["masks"][i][e["decided"][i]]).sum()) == 0 for i in range(n))
    args.mask_head = "hip"                                                          # the flag selects the head when none is named
    assert isinstance(ms.SAM(args, str(tmp_path / "run_flag"), **e["thresholds"]).head, ms.SamHeadHip)
