"""Host tests of the edit-quality scores (loco_edit_amd/quality.py, eval.py --backend, define_argparser.py); no GPU.

Also here, for the GPU tests: the seeded LPIPS weights (convolutions N(0, 2 / fan_in), biases 0.05 N(0, 1), heads
U(0, 1) 10 / C: about half of every tap's activations stay live), the smooth-noise image pairs (bicubic upsampling of an
H/8 x W/8 normal field, times 0.5, clamped to [-1, 1]; y = clamp(x + amp smooth)) and ``lpips_restated``, the restatement of
``eval.lpips`` in a chosen dtype that also returns the five taps (the float64 yardstick of csrc/quality.hip)."""
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import define_argparser, quality  # noqa: E402
from loco_edit_amd import eval as ev  # noqa: E402

ALEX_SHAPES = {0: (64, 3, 11, 11), 3: (192, 64, 5, 5), 6: (384, 192, 3, 3), 8: (256, 384, 3, 3), 10: (256, 256, 3, 3)}


def seeded_lpips_weights(seed=0):
    g = torch.Generator().manual_seed(seed)
    w = {}
    for j, (i, sh) in enumerate(ALEX_SHAPES.items()):
        w[f"features.{i}.weight"] = torch.randn(sh, generator=g) * (2.0 / (sh[1] * sh[2] * sh[3])) ** 0.5
        w[f"features.{i}.bias"] = 0.05 * torch.randn(sh[0], generator=g)
        w[f"lin{j}.model.1.weight"] = torch.rand(1, sh[0], 1, 1, generator=g) * 10.0 / sh[0]
    return w


def smooth_noise(n, H, W, generator):
    z = torch.randn(n, 3, -(-H // 8), -(-W // 8), generator=generator)
    return F.interpolate(z, size=(H, W), mode="bicubic", align_corners=False)


def image_pairs(n, H, W, amp, seed):
    """x, y [n,3,H,W] fp32 in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    x = (0.5 * smooth_noise(n, H, W, g)).clamp(-1, 1)
    y = (x + amp * smooth_noise(n, H, W, g)).clamp(-1, 1)
    return x, y


def _conv(x, w, b, stride, pad):
    if not x.is_cuda:
        return F.conv2d(x, w, b, stride=stride, padding=pad)
    # on a device: im2col + matmul (no library convolution in double there)
    n, _, H, W = x.shape
    k = w.shape[-1]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    cols = F.unfold(x, k, padding=pad, stride=stride)
    return (w.reshape(w.shape[0], -1) @ cols + b[None, :, None]).reshape(n, -1, Ho, Wo)


def lpips_restated(x, y, weights, dtype=torch.float64, normalize=False):
    """The formulas of eval.lpips in `dtype` on x's device -> (distance [n], taps [n,5])."""
    n, dev = x.shape[0], x.device
    w = {k: v.to(device=dev, dtype=dtype) for k, v in weights.items()}
    h = torch.cat([x, y]).to(dtype)
    if normalize:
        h = 2 * h - 1
    h = (h - torch.tensor(ev._LPIPS_SHIFT, dtype=dtype, device=dev).view(1, 3, 1, 1)) / \
        torch.tensor(ev._LPIPS_SCALE, dtype=dtype, device=dev).view(1, 3, 1, 1)
    taps = []
    for j, (i, _, _, stride, pad, pool) in enumerate(ev._ALEX):
        if pool:
            h = F.max_pool2d(h, kernel_size=3, stride=2)
        h = F.relu(_conv(h, w[f"features.{i}.weight"], w[f"features.{i}.bias"], stride, pad))
        f = h / (h.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
        d = ((f[:n] - f[n:]) ** 2 * w[f"lin{j}.model.1.weight"]).sum(dim=1)
        taps.append(d.mean(dim=(1, 2)))
    taps = torch.stack(taps, dim=1)
    return taps.sum(dim=1), taps


# ---------------------------------------------------------------------------
def test_restatement_is_eval_lpips():
    """The yardstick of the GPU tests restates eval.lpips: in fp32 the two agree to rounding, pair by pair."""
    w = seeded_lpips_weights()
    x, y = image_pairs(2, 35, 33, 0.3, 5)
    d32, taps = lpips_restated(x, y, w, dtype=torch.float32)
    for i in range(2):
        assert abs(float(ev.lpips(x[i:i + 1], y[i:i + 1], weights=w)) - float(d32[i])) <= 2e-6 * float(d32[i])
    assert tuple(taps.shape) == (2, 5) and bool((taps > 0).all())
    d64, _ = lpips_restated(x, y, w)
    assert 1e-3 < float(d64.min()) and float(d64.max()) < 5e-2          # an edit-sized difference
    xs, ys = image_pairs(1, 64, 64, 1 / 255, 6)
    assert 1e-7 < float(lpips_restated(xs, ys, w)[0]) < 1e-4            # a one-grey-level difference


def test_new_flags_default_off_and_change_no_other_field():
    scripts = json.load(open(os.path.join(ROOT, "tests", "golden", "script_args.json")))
    assert len(scripts) == 12
    for name, argv in scripts.items():
        a = vars(define_argparser.parse_args(argv))
        assert a["quality_metrics"] == "" and a["lpips_weights"] == "", name
        b = vars(define_argparser.parse_args(argv + ["--quality_metrics", "ssim,mmse", "--lpips_weights", "w.pt"]))
        assert (b["quality_metrics"], b["lpips_weights"]) == ("ssim,mmse", "w.pt")
        assert {k: v for k, v in a.items() if k not in ("quality_metrics", "lpips_weights")} == \
               {k: v for k, v in b.items() if k not in ("quality_metrics", "lpips_weights")}, name
        assert quality.scorer_from_args(define_argparser.parse_args(argv), "cpu") is None


def test_lpips_without_weights_raises_at_construction(tmp_path):
    a = define_argparser.parse_args(["--quality_metrics", "lpips"])
    with pytest.raises(ValueError, match="lpips_weights"):
        quality.scorer_from_args(a, "cpu")
    with pytest.raises(ValueError, match="psnr"):
        quality.scorer_from_args(define_argparser.parse_args(["--quality_metrics", "ssim,psnr"]), "cpu")
    with pytest.raises(NotImplementedError):
        quality.QualityScorer("cpu", "lpips", None)
    s = quality.scorer_from_args(define_argparser.parse_args(["--quality_metrics", "mmse, ssim"]), "cpu")
    assert s.metrics == ["ssim", "mmse"] and s.lpips_weights_path == ""
    f = tmp_path / "w.pt"
    torch.save(seeded_lpips_weights(), str(f))
    s = quality.scorer_from_args(define_argparser.parse_args(["--quality_metrics", "lpips", "--lpips_weights", str(f)]), "cpu")
    assert s.metrics == ["lpips"] and s.lpips_weights_path == str(f)


def test_two_file_weights_merge_and_missing_key(tmp_path):
    w = seeded_lpips_weights()
    feats = {("net." + k if "features.0" in k else k): v for k, v in w.items() if k.startswith("features.")}
    feats["classifier.1.weight"] = torch.zeros(2, 2)                    # a torchvision file holds more than the features
    heads = {k: v for k, v in w.items() if k.startswith("lin")}
    ff, hf, af = tmp_path / "alexnet.pth", tmp_path / "alex.pth", tmp_path / "all.pt"
    torch.save(feats, str(ff)); torch.save(heads, str(hf)); torch.save(w, str(af))
    for spec in (f"{ff},{hf}", f"{hf}, {ff}", str(af)):
        got = quality.load_lpips_weights(spec)
        assert list(got) == ev.lpips_weight_names() and all(torch.equal(got[k], w[k]) for k in w)
    with pytest.raises(ValueError, match="lacks lin0"):
        quality.load_lpips_weights(str(ff))
    heads.pop("lin3.model.1.weight")
    torch.save(heads, str(hf))
    with pytest.raises(ValueError, match="lin3"):
        quality.load_lpips_weights(f"{ff},{hf}")
    with pytest.raises(NotImplementedError):
        quality.load_lpips_weights("")


class StubEngine:
    """What QualityScorer asks of hip.LocoQualityEngine, computed on the host from the definitions."""
    max_pairs, max_hw = 64, (512, 512)

    def __init__(self):
        self.calls = []

    def ssim(self, a, b, data_range=None):
        self.calls.append(("ssim", data_range))
        return torch.stack([ev.ssim(a[i:i + 1], b[i:i + 1], data_range=data_range) for i in range(a.shape[0])])

    def lpips(self, a, b, normalize=False):
        self.calls.append(("lpips", normalize))
        return ((a - b) ** 2).mean(dim=(1, 2, 3))

    def masked_mse(self, a, b, mask):
        self.calls.append(("mmse", None))
        return torch.stack([ev.masked_mse(a[i:i + 1], b[i:i + 1], mask) for i in range(a.shape[0])])


def test_score_records_and_json_layout_on_a_stub_engine(tmp_path):
    g = torch.Generator().manual_seed(2)
    frames = torch.rand(5, 3, 16, 20, generator=g)
    mask = torch.zeros(16, 20, dtype=torch.bool)
    mask[3:9, 4:12] = True
    eng = StubEngine()
    s = quality.QualityScorer("cpu", "lpips,ssim,mmse", seeded_lpips_weights(), engine=eng)
    recs = s.score(frames, 2, mask)
    assert [c[0] for c in eng.calls] == ["ssim", "mmse", "mmse", "lpips"] and ("ssim", 1.0) in eng.calls and ("lpips", True) in eng.calls
    assert len(recs) == 5 and all(list(r) == ["ssim", "mmse_in", "mmse_out", "lpips"] for r in recs)
    assert recs[2] == {"ssim": 1.0, "mmse_in": 0.0, "mmse_out": 0.0, "lpips": 0.0}
    m3 = mask[None].expand(3, 16, 20)
    for i in (0, 1, 3, 4):
        a, b = frames[i:i + 1], frames[2:3]
        assert recs[i]["ssim"] == float(ev.ssim(a, b, data_range=1.0)) < 1.0
        assert recs[i]["mmse_in"] == float(ev.masked_mse(a, b, m3[None])) > 0.0
        assert recs[i]["mmse_out"] == float(ev.masked_mse(a, b, ~m3[None])) > 0.0
        assert recs[i]["lpips"] == float(((a - b) ** 2).mean())
    # no mask, or a region without elements: null, never a made-up number
    assert all(r["mmse_in"] is None and r["mmse_out"] is None for r in s.score(frames, 0, None))
    full = s.score(frames, 0, torch.ones(3, 16, 20, dtype=torch.bool))
    assert all(r["mmse_out"] is None and r["mmse_in"] is not None for r in full)
    only = quality.QualityScorer("cpu", ["ssim"], engine=StubEngine()).score(frames, 4)
    assert all(list(r) == ["ssim"] for r in only) and only[4]["ssim"] == 1.0
    with pytest.raises(ValueError):
        s.score(frames, 5, mask)
    with pytest.raises(ValueError):
        s.score(frames[:, :1], 0, mask)
    # the file a driver writes
    alphas = [-8.0, -4.0, 0.0, 4.0, 8.0]
    out = s.write(str(tmp_path / "walk_quality.json"), frames, 2, mask=mask, alphas=alphas, exp_name="walk")
    disk = json.load(open(tmp_path / "walk_quality.json"))
    assert disk == out
    assert disk["metrics"] == ["ssim", "mmse", "lpips"] and disk["lpips_weights"] == "" and disk["alphas"] == alphas
    assert disk["original_index"] == 2 and disk["masked"] is True and disk["exp_name"] == "walk"
    assert [f["alpha"] for f in disk["frames"]] == alphas
    assert all({k: v for k, v in f.items() if k != "alpha"} == r for f, r in zip(disk["frames"], recs))
    with pytest.raises(ValueError):
        s.report(frames, 2, alphas=alphas[:3])


def test_eval_main_backend_torch_is_the_default_path(tmp_path, capsys):
    from loco_edit_amd.utils import save_image
    assert list(ev.METRICS) == ["ssim", "mmse", "lpips"] and ev.METRICS["ssim"] is ev.ssim and ev.METRICS["mmse"] is ev.masked_mse
    p, o = tmp_path / "p", tmp_path / "o"
    os.makedirs(p / "mask"); os.makedirs(o)
    x, y = image_pairs(2, 32, 36, 0.3, 9)
    m = torch.zeros(32, 36, dtype=torch.bool)
    m[5:11, 6:20] = True
    for i in range(2):
        save_image((x[i:i + 1] + 1) / 2, str(o / f"{i}.png"), padding=0)
        save_image((y[i:i + 1] + 1) / 2, str(p / f"{i}.png"), padding=0)
        torch.save(m, str(p / "mask" / f"{i}.pt"))
    wf = tmp_path / "w.pt"
    torch.save(seeded_lpips_weights(), str(wf))
    base = ["--folder_preds", str(p), "--folder_original", str(o), "--lpips_weights", str(wf)]
    for metric in ("ssim", "mmse", "lpips"):
        r0 = ev.main(base + ["--eval_metric", metric])
        r1 = ev.main(base + ["--eval_metric", metric, "--backend", "torch"])
        assert r0 == r1 and r0["n"] == 2 and r0["metric"] == metric
    xs, ys = [ev._load_png(str(p / f"{i}.png")) for i in range(2)], [ev._load_png(str(o / f"{i}.png")) for i in range(2)]
    want = sum(float(ev.ssim(a, b)) for a, b in zip(xs, ys)) / 2
    assert ev.main(base + ["--eval_metric", "ssim", "--backend", "torch"])["mean"] == want
    assert ev.evaluate_folders(str(p), str(o), "mmse", outside_mask=True, backend="torch") == \
           ev.evaluate_folders(str(p), str(o), "mmse", outside_mask=True)
    with pytest.raises(ValueError):
        ev.evaluate_folders(str(p), str(o), "ssim", backend="cuda")
    with pytest.raises(SystemExit):
        ev.main(base + ["--backend", "cuda"])


class _Main:
    is_main = True


def test_driver_hooks_write_the_json_on_a_stub_engine(tmp_path):
    """EditUncondDiffusion._score_quality (float frames in [0, 1]) and EditDeepFloydIF._score_quality (the uint8 frames the
    text-guided samplers return) around a scorer with the stub engine: file name, original frame, mask handling, off switch."""
    from loco_edit_amd.edit import EditUncondDiffusion
    from loco_edit_amd.tloco import EditDeepFloydIF
    g = torch.Generator().manual_seed(4)
    frames = torch.rand(5, 3, 16, 20, generator=g)
    mask = torch.zeros(3, 16, 20, dtype=torch.bool)
    mask[:, 2:7, 3:9] = True
    e = object.__new__(EditUncondDiffusion)
    e.sharder, e.result_folder = _Main(), str(tmp_path)
    e.x_space_guidance_num_step, e.x_space_guidance_scale, e.x_space_guidance_edit_step = 16, 0.5, 1.0
    assert e._score_quality(frames, "off", e._walk_alphas(2), mask) is None and not os.listdir(tmp_path)     # no scorer: nothing
    e.quality = quality.QualityScorer("cpu", "ssim,mmse", engine=StubEngine())
    out = e._score_quality(frames, "walk", e._walk_alphas(2), mask)
    assert json.load(open(tmp_path / "walk_quality.json")) == out and out["original_index"] == 2
    assert out["alphas"] == [-8.0, -4.0, 0.0, 4.0, 8.0] and out["frames"][2]["ssim"] == 1.0 and out["frames"][0]["mmse_in"] > 0.0
    grp = e._score_quality(frames[:3], "group", None, None, original_index=0)           # the composed edit against frame 0, no mask
    assert grp["alphas"] == [None] * 3 and grp["masked"] is False and grp["frames"][0]["ssim"] == 1.0
    assert all(f["mmse_in"] is None and f["mmse_out"] is None for f in grp["frames"])
    with pytest.raises(ValueError):
        e._score_quality(frames, "bad", [1.0, 2.0, 3.0, 4.0, 5.0], mask)
    e.sharder = type("S", (), {"is_main": False})()
    assert e._score_quality(frames, "rank1", e._walk_alphas(2), mask) is None and not (tmp_path / "rank1_quality.json").exists()

    t = object.__new__(EditDeepFloydIF)
    t.sharder, t.result_folder, t.device, t.EXP_NAME = _Main(), str(tmp_path), "cpu", "sem"
    u8 = (frames * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert t._score_quality(u8, [-1.0, -0.5, 0.0, 0.5, 1.0], mask) is None                # class default: off
    t._quality = quality.QualityScorer("cpu", "ssim,mmse", engine=StubEngine())
    out = t._score_quality(u8, [-1.0, -0.5, 0.0, 0.5, 1.0], mask)
    assert json.load(open(tmp_path / "sem_quality.json")) == out and out["exp_name"] == "sem" and out["masked"] is True
    f01 = u8.permute(0, 3, 1, 2).float() / 255.0
    assert out["frames"][4]["mmse_in"] == float(ev.masked_mse(f01[4:5], f01[2:3], mask[None]))
    lat = t._score_quality(u8, [-1.0, -0.5, 0.0, 0.5, 1.0], torch.ones(3, 4, 5, dtype=torch.bool))   # a latent-sized mask: not used
    assert lat["masked"] is False and lat["frames"][1]["mmse_in"] is None
    with pytest.raises(ValueError):
        t._score_quality(u8, [1.0, 2.0, 3.0, 4.0, 5.0], mask)


def test_lcm_walk_scores_quality_without_a_clip_model(tmp_path):
    """EditLatentConsistency.run_edit_null_space_projection_zt with --quality_metrics and no --clip_model_path: the semantic
    walk writes <EXP_NAME>_quality.json (the CLIP scores stay off), the non-semantic one (k rows: no single alpha list) does
    not.  The sampler, the solver and the engine are stubs; the flow between them is the driver's own."""
    from loco_edit_amd.tloco_lcm import EditLatentConsistency
    g = torch.Generator().manual_seed(6)
    H, W = 16, 20
    t = object.__new__(EditLatentConsistency)
    t.args = type("A", (), {"mask_model_path": "", "clip_model_path": ""})()
    t.sharder = type("S", (), {"is_main": True, "agree": staticmethod(lambda v: v)})()
    t.result_folder, t.device, t.sampling_mode, t.use_sega = str(tmp_path), "cpu", False, False
    t.scheduler = type("Sch", (), {"set_timesteps": lambda self, *a, **k: None})()
    t.num_inference_steps, t.edit_t_idx, t.for_prompt, t.edit_prompt = 4, 2, "a", "b"
    t.x_space_guidance_num_step, t.x_space_guidance_scale, t.x_space_guidance_edit_step = 4, 0.5, 1.0
    t.engine = type("E", (), {"null_project": staticmethod(lambda vm, vn: vm)})()
    masks = torch.zeros(2, 1, H, W, dtype=torch.bool)
    masks[1, 0, 3:9, 4:12] = True
    t._set_edit_prompt = lambda p: None
    t._zT = lambda: torch.randn(1, 3, H, W, generator=g)
    t._exists = lambda p: False
    t._masks = lambda fn, res: masks
    t.run_LCMforward = lambda z, prompt: (z, (torch.rand(1, H, W, 3, generator=g) * 255).to(torch.uint8))

    def steps(z, t_start_idx, t_end_idx, prompt):
        if t_end_idx != -1:
            return z, 499, t_end_idx
        return z, ((z / 4 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    t.LCMforwardsteps = steps
    t.get_delta_zt_via_grad = lambda z, *a, **k: torch.randn(1, z[0].numel(), generator=g)
    t.local_encoder_decoder_pullback_zt = lambda z, *a, **k: (None, None, torch.randn(2, z[0].numel(), generator=g))
    t.x_space_guidance_direct = lambda z, t_idx, vk, single_edit_step: z + single_edit_step * vk
    kw = dict(op="mid", block_idx=0, vis_num=2, mask_index=1, pca_rank=2)
    out = t.run_edit_null_space_projection_zt(**kw)                                     # class default: off, nothing written
    assert tuple(out[1].shape) == (5, H, W, 3) and not [f for f in os.listdir(tmp_path) if f.endswith(".json")]
    t._quality = quality.QualityScorer("cpu", "ssim,mmse", engine=StubEngine())
    assert not t.clip_scoring
    out = t.run_edit_null_space_projection_zt(**kw)
    files = [f for f in os.listdir(tmp_path) if f.endswith(".json")]
    assert files == [f"{t.EXP_NAME}_quality.json"]
    q = json.load(open(tmp_path / files[0]))
    assert q["alphas"] == [-2.0, -1.0, 0.0, 1.0, 2.0] and q["original_index"] == 2 and q["masked"] is True
    assert q["frames"][2]["ssim"] == 1.0 and q["frames"][0]["mmse_in"] > 0.0 and len(q["frames"]) == 5
    os.remove(tmp_path / files[0])
    t.run_edit_null_space_projection_zt(non_semantic=True, **kw)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".json")]
