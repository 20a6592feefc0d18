"""GPU tests of the edit-quality scorer (csrc/quality.hip through hip.LocoQualityEngine / quality.QualityScorer):

* LPIPS with seeded weights against the float64 restatement of test_quality_host.py at the smallest sizes at which the layer
  geometry can go wrong (31x31: every late tap is 1x1; 35x33; 67x45: the floors of the stride-4 layer and of both pools differ
  per axis; 64x64 with three pairs), for an edit-sized difference (amp 0.3) and a one-grey-level one (amp 1/255).  The bar is
  not a constant: the project's fp32 host path, eval.lpips, is run on the same pairs, and the HIP distance and each of its five
  taps must stay within 4x the largest relative error of that path in the amplitude class (the factor: another summation
  order over up to 3456 terms in the same arithmetic class).  Both columns are printed;
* the same rule once at size, 26 pairs of 256x256, against the restatement in float64 on the device;
* SSIM within 1e-9 absolute of eval.ssim (both are float64 sums of at most 121 products of the same fp32 inputs), masked MSE
  within 1e-12 relative of eval.masked_mse;
* identities (lpips(x, x) == 0, symmetric bit for bit, ssim(x, x) == 1), bit-identity of a pair alone, at every position of
  a full batch and under LOCO_PRECISION=f16; refusals are errors with a message;
* the unconditional driver with --quality_metrics, and eval.main --backend hip against --backend torch."""
import importlib.util
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import eval as ev  # noqa: E402
from loco_edit_amd import quality  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_spec = importlib.util.spec_from_file_location("quality_host", os.path.join(ROOT, "tests", "test_quality_host.py"))
_host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_host)
seeded_lpips_weights, image_pairs, lpips_restated = _host.seeded_lpips_weights, _host.image_pairs, _host.lpips_restated

LPIPS_SHAPES = [(1, 31, 31), (1, 35, 33), (1, 67, 45), (3, 64, 64)]
AMPS = {"edit": 0.3, "grey": 1 / 255}
_CACHE = {}


def weights():
    if "w" not in _CACHE:
        _CACHE["w"] = seeded_lpips_weights()
    return _CACHE["w"]


def engine(max_pairs=3, max_hw=(67, 64), with_weights=True):
    from loco_edit_amd.hip import LocoQualityEngine
    e = LocoQualityEngine(max_hw=max_hw, max_pairs=max_pairs, device=torch.device(DEV))
    if with_weights:
        e.load_state_dict(weights())
    return e


def shared_engine():
    if "eng" not in _CACHE:
        _CACHE["eng"] = engine()
    return _CACHE["eng"]


def lpips_cases():
    """Per amplitude class: the pairs of every shape with their float64 distance and taps, and the class maximum of the relative
    error of eval.lpips (fp32 on the host) against float64.  Computed once."""
    if "cases" not in _CACHE:
        out = {}
        for cls, amp in AMPS.items():
            rows, worst = [], 0.0
            for k, (n, H, W) in enumerate(LPIPS_SHAPES):
                x, y = image_pairs(n, H, W, amp, 100 + k)
                d64, t64 = lpips_restated(x, y, weights())
                for i in range(n):
                    d32 = float(ev.lpips(x[i:i + 1], y[i:i + 1], weights=weights()))
                    worst = max(worst, abs(d32 - float(d64[i])) / float(d64[i]))
                rows.append((x, y, d64, t64))
            out[cls] = (rows, worst)
        _CACHE["cases"] = out
    return _CACHE["cases"]


def rel(a, ref):
    return ((a.double().cpu() - ref) / ref).abs()


@pytest.mark.parametrize("cls", list(AMPS))
@pytest.mark.parametrize("shape", range(len(LPIPS_SHAPES)))
def test_lpips_vs_float64_within_4x_the_fp32_host_path(cls, shape):
    rows, worst32 = lpips_cases()[cls]
    x, y, d64, t64 = rows[shape]
    d, taps = shared_engine().lpips(x, y, want_taps=True)
    ed, et = rel(d, d64), rel(taps, t64)
    print(f"\nLPIPS {cls} {LPIPS_SHAPES[shape]}: float64 {d64.tolist()}  eval.lpips fp32 class max rel {worst32:.3e}  "
          f"HIP rel distance {ed.max():.3e} taps {et.max(dim=0).values.tolist()}")
    assert torch.isfinite(d).all() and bool((d64 > 0).all())
    assert float(ed.max()) <= 4 * worst32
    assert float(et.max()) <= 4 * worst32


def test_lpips_identities_and_normalize():
    eng = shared_engine()
    _, worst32 = lpips_cases()["edit"]
    x, y, d64, _ = lpips_cases()["edit"][0][3]
    assert torch.equal(eng.lpips(x, x), torch.zeros(3, device=DEV))
    dxy, dyx = eng.lpips(x, y), eng.lpips(y, x)
    assert torch.equal(dxy, dyx)                                       # (fa - fb)^2 from the same two feature maps
    dn = eng.lpips((x + 1) / 2, (y + 1) / 2, normalize=True)
    assert float(rel(dn, d64).max()) <= 4 * worst32


def test_lpips_bit_identical_alone_in_a_full_batch_and_under_f16(monkeypatch):
    eng = shared_engine()
    assert eng.max_pairs == 3
    x, y, _, _ = lpips_cases()["grey"][0][3]
    alone = [eng.lpips(x[i:i + 1], y[i:i + 1], want_taps=True) for i in range(3)]
    for shift in range(3):
        order = [(i + shift) % 3 for i in range(3)]
        d, taps = eng.lpips(x[order], y[order], want_taps=True)
        for pos, i in enumerate(order):
            assert torch.equal(d[pos:pos + 1], alone[i][0]) and torch.equal(taps[pos:pos + 1], alone[i][1])
    # the variable is read when a handle is created: a U-Net context created now runs f16 (and is told so once more), and so
    # would a quality handle created now if it had a precision input
    monkeypatch.setenv("LOCO_PRECISION", "f16")
    from loco_edit_amd.config import TINY_DDPM
    from loco_edit_amd.hip import LocoEngine
    unet = LocoEngine(TINY_DDPM, max_batch=1, device=torch.device(DEV))
    assert unet.get_precision() == "f16"
    unet.set_precision("f16")
    d16, t16 = engine().lpips(x, y, want_taps=True)
    d, taps = eng.lpips(x, y, want_taps=True)
    assert torch.equal(d16, d) and torch.equal(t16, taps)


def test_lpips_refusals():
    eng = shared_engine()
    x, y = image_pairs(4, 31, 31, 0.3, 7)
    with pytest.raises(RuntimeError, match="below 31"):
        eng.lpips(x[:1, :, :30], y[:1, :, :30])
    with pytest.raises(RuntimeError, match="below 31"):
        eng.lpips(x[:1, :, :, :30], y[:1, :, :, :30])
    with pytest.raises(RuntimeError, match="max_pairs = 3"):
        eng.lpips(x, y)
    big = torch.zeros(1, 3, 68, 40)
    with pytest.raises(RuntimeError, match="above the configured"):
        eng.lpips(big, big)
    with pytest.raises(ValueError):
        eng.lpips(x[:1, :2], y[:1, :2])
    part = engine(with_weights=False)
    with pytest.raises(RuntimeError, match="missing parameter"):
        part.lpips(x[:1], y[:1])
    part.load_params({k: v for k, v in weights().items() if k != "lin4.model.1.weight"})
    with pytest.raises(RuntimeError, match="lin4.model.1.weight"):
        part.lpips(x[:1], y[:1])
    with pytest.raises(RuntimeError, match="shape"):
        part.load_params({"lin4.model.1.weight": torch.zeros(256)})
    # SSIM and masked MSE need no parameters
    assert float(part.ssim(x[:1], x[:1])[0]) == 1.0
    from loco_edit_amd.hip import LocoQualityEngine
    with pytest.raises(RuntimeError, match="positive"):
        LocoQualityEngine(max_hw=(0, 64), device=torch.device(DEV))


def test_lpips_at_size_26_frames_of_256():
    x, y = image_pairs(26, 256, 256, AMPS["edit"], 300)
    w = weights()
    d64, t64 = lpips_restated(x.to(DEV), y.to(DEV), w)
    d64, t64 = d64.cpu(), t64.cpu()
    worst32 = max(abs(float(ev.lpips(x[i:i + 1], y[i:i + 1], weights=w)) - float(d64[i])) / float(d64[i]) for i in range(26))
    eng = engine(max_pairs=26, max_hw=(256, 256))
    d, taps = eng.lpips(x, y, want_taps=True)
    ed, et = rel(d, d64), rel(taps, t64)
    print(f"\nLPIPS 26 x 256 x 256: float64 mean {float(d64.mean()):.6e}  eval.lpips fp32 max rel {worst32:.3e}  "
          f"HIP rel distance {ed.max():.3e} taps {et.max(dim=0).values.tolist()}")
    assert float(ed.max()) <= 4 * worst32
    assert float(et.max()) <= 4 * worst32


def test_score_25_frames_of_256_and_print_the_wall_time():
    """The 25 decoded frames of a headline run (5 directions x 5 frames at 256 x 256), all three metrics with a mask, through
    QualityScorer.score; prints the wall time DESIGN 7.7 quotes: host clock around the call, which ends in reading the results
    back, 3 warm-up calls, the median of 10."""
    import statistics
    import time
    x, y = image_pairs(25, 256, 256, AMPS["edit"], 1)
    frames = (x[:1] + (y - x)).clamp(-1, 1)                            # 25 edit-sized departures from one image ...
    frames[12] = x[0]                                                   # ... which is the middle frame
    frames = ((frames + 1) / 2).to(DEV).contiguous()
    mask = torch.zeros(3, 256, 256, dtype=torch.bool)
    mask[:, 100:140, 60:120] = True
    s = quality.QualityScorer(DEV, "ssim,mmse,lpips", weights())

    def timed(fn, reps=10):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)
    orig = frames[12][None].expand_as(frames).contiguous()
    rows = [("score, 25 frames", timed(lambda: s.score(frames, 12, mask))),
            ("score, 5 frames", timed(lambda: s.score(frames[10:15], 2, mask))),
            ("lpips alone, 25 frames", timed(lambda: s.lpips(frames, orig, normalize=True))),
            ("ssim alone, 25 frames", timed(lambda: s.ssim(frames, orig, data_range=1.0)))]
    for name, (med, lo, hi) in rows:
        print(f"\nquality wall time, {name}: median {med:.2f} ms ({lo:.2f} - {hi:.2f}, 10 warm repeats)")
    recs = s.score(frames, 12, mask)
    assert recs[12] == {"ssim": 1.0, "mmse_in": 0.0, "mmse_out": 0.0, "lpips": 0.0}
    assert all(0.0 < r["ssim"] < 1.0 and r["lpips"] > 0.0 and r["mmse_in"] > 0.0 for i, r in enumerate(recs) if i != 12)


SSIM_SHAPES = [(1, 1, 12, 13), (2, 3, 37, 50), (3, 3, 64, 64), (1, 3, 9, 40)]


@pytest.mark.parametrize("scale", [255.0, 1.0])
@pytest.mark.parametrize("shape", SSIM_SHAPES)
def test_ssim_vs_eval_ssim(shape, scale):
    eng = shared_engine()
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.rand(shape, generator=g) * scale
    y = (x + 0.08 * scale * torch.randn(shape, generator=g)).clamp(0, scale)
    x[0, 0, :6, :6] = 0.97 * scale                                      # a flat bright patch: E[x^2] - mu^2 cancels
    for dr in (scale, None):
        got = eng.ssim(x, y, data_range=dr).cpu()
        rng = dr if dr is not None else max(float(x.double().max() - x.double().min()), float(y.double().max() - y.double().min()))
        want = torch.stack([ev.ssim(x[i:i + 1], y[i:i + 1], data_range=rng) for i in range(shape[0])])
        err = float((got - want).abs().max())
        print(f"\nSSIM {shape} scale {scale} data_range {dr}: {want.tolist()}  HIP abs err {err:.3e}")
        assert got.dtype == torch.float64 and err <= 1e-9
        assert abs(float(got.mean()) - float(ev.ssim(x, y, data_range=dr))) <= 1e-9
    assert float((eng.ssim(x, x) - 1.0).abs().max()) <= 1e-12
    assert float((eng.ssim(y, y, data_range=scale) - 1.0).abs().max()) <= 1e-12


def test_ssim_batch_position_and_refusals():
    eng = shared_engine()
    g = torch.Generator().manual_seed(4)
    x = torch.rand(3, 3, 37, 50, generator=g)
    y = (x + 0.1 * torch.randn(3, 3, 37, 50, generator=g)).clamp(0, 1)
    alone = [eng.ssim(x[i:i + 1], y[i:i + 1], data_range=1.0) for i in range(3)]
    for shift in range(3):
        order = [(i + shift) % 3 for i in range(3)]
        got = eng.ssim(x[order], y[order], data_range=1.0)
        for pos, i in enumerate(order):
            assert torch.equal(got[pos:pos + 1], alone[i])
    with pytest.raises(RuntimeError, match="below 6"):
        eng.ssim(x[:, :, :5], y[:, :, :5])
    with pytest.raises(RuntimeError, match="below 6"):
        eng.ssim(x[:, :, :, :5], y[:, :, :, :5])
    with pytest.raises(RuntimeError, match="max_pairs = 3"):
        eng.ssim(torch.cat([x, x]), torch.cat([y, y]))
    with pytest.raises(RuntimeError, match="above the configured"):
        eng.ssim(torch.zeros(1, 1, 68, 8), torch.zeros(1, 1, 68, 8), data_range=1.0)
    with pytest.raises(RuntimeError, match="exceed the workspace"):
        eng.ssim(torch.zeros(3, 40, 67, 64), torch.zeros(3, 40, 67, 64), data_range=1.0)
    # an uncropped strip has more tiles per plane (7) than the cropped map of the largest plane (6): a full batch of it fits
    strip = engine(max_pairs=2, max_hw=(20, 100), with_weights=False)
    xs, ys = x[:2, :, :10].repeat(1, 1, 1, 2).contiguous(), y[:2, :, :10].repeat(1, 1, 1, 2).contiguous()
    want = torch.stack([ev.ssim(xs[i:i + 1], ys[i:i + 1], data_range=1.0) for i in range(2)])
    assert tuple(xs.shape) == (2, 3, 10, 100) and float((strip.ssim(xs, ys, data_range=1.0).cpu() - want).abs().max()) <= 1e-9
    full = torch.rand(2, 3, 20, 100, generator=g)
    assert float((strip.ssim(full, full, data_range=1.0) - 1.0).abs().max()) <= 1e-12


def test_masked_mse_vs_eval():
    eng = shared_engine()
    g = torch.Generator().manual_seed(8)
    x = torch.rand(2, 3, 37, 50, generator=g)
    y = x + 0.2 * torch.randn(2, 3, 37, 50, generator=g)
    rnd = torch.rand(3, 37, 50, generator=g) < 0.3
    one = torch.zeros(3, 37, 50, dtype=torch.bool)
    one[1, 17, 33] = True
    for m in (rnd, ~rnd, one, ~one, rnd[0]):
        got = eng.masked_mse(x, y, m[None] if m.dim() == 3 else m).cpu()
        want = torch.stack([ev.masked_mse(x[i:i + 1], y[i:i + 1], m[None] if m.dim() == 3 else m) for i in range(2)])
        assert got.dtype == torch.float64 and float(((got - want) / want).abs().max()) <= 1e-12
    per = torch.stack([rnd, ~rnd])                                      # a mask per image
    got = eng.masked_mse(x, y, per).cpu()
    want = torch.stack([ev.masked_mse(x[i:i + 1], y[i:i + 1], per[i:i + 1]) for i in range(2)])
    assert float(((got - want) / want).abs().max()) <= 1e-12
    with pytest.raises(ValueError, match="empty mask"):
        eng.masked_mse(x, y, torch.zeros(3, 37, 50, dtype=torch.bool))
    with pytest.raises(ValueError, match="empty mask"):
        eng.masked_mse(x, y, torch.stack([rnd, torch.zeros_like(rnd)]))


def _run_driver(tmp, monkeypatch, extra):
    from loco_edit_amd.main import main
    os.makedirs(tmp)
    monkeypatch.chdir(tmp)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("LOCO_PRECISION", "bf16x3")
    base = ["--sh_file_name", "main_celeba_hf_null_space_projection.sh", "--sample_idx", "3", "--device", DEV,
            "--dtype", "fp32", "--seed", "11", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Synthetic",
            "--unet_preset", "tiny_ddpm", "--synthetic_weights", "0", "--for_steps", "100", "--inv_steps", "100",
            "--use_yh_custom_scheduler", "True", "--x_space_guidance_edit_step", "1", "--x_space_guidance_scale", "0.5",
            "--x_space_guidance_num_step", "16", "--edit_t", "0.6", "--performance_boosting_t", "0.2",
            "--choose_sem", "l_eye", "--null_space_projection", "True", "--use_mask", "True", "--pca_rank_null", "2",
            "--pca_rank", "2", "--vis_num", "2", "--run_edit_null_space_projection", "True"]
    main(base + extra)
    return tmp / "runs" / "CelebA_HQ_HF-Synthetic" / "results" / "sample_idx3"


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.mark.parametrize("batch_decode", ["1", "0"])
def test_driver_writes_quality_json_and_changes_nothing_else(batch_decode, tmp_path, monkeypatch):
    """The tiny unconditional run of test_cli_main_tiny_config (32x32, l_eye mask, two directions of five frames) with and
    without --quality_metrics, in both decode branches."""
    monkeypatch.setenv("LOCO_BATCH_DECODE", batch_decode)
    wf = tmp_path / "lpips.pt"
    torch.save(weights(), str(wf))
    seen = []
    score = quality.QualityScorer.score

    def spy(self, frames, original_index, mask=None):
        recs = score(self, frames, original_index, mask)
        seen.append((frames.detach().clone(), original_index, None if mask is None else torch.as_tensor(mask).clone(), recs))
        return recs
    monkeypatch.setattr(quality.QualityScorer, "score", spy)
    plain = _tree(_run_driver(tmp_path / "plain", monkeypatch, []))
    assert not seen and not [f for f in plain if f.endswith("_quality.json")]
    rdir = _run_driver(tmp_path / "scored", monkeypatch, ["--quality_metrics", "ssim,mmse,lpips", "--lpips_weights", str(wf)])
    scored = _tree(rdir)
    files = sorted(f for f in scored if f.endswith("_quality.json"))
    grids = sorted(f for f in scored if f.startswith("3-Edit-randomFalse_xt-noise-") and f.endswith(".png"))
    assert len(files) == 2 and len(seen) == 2 and [g[:-4] + "_quality.json" for g in grids] == files
    # nothing that existed changes: the grids, the basis files and everything else, byte for byte
    assert {k: v for k, v in scored.items() if k not in files} == plain
    fresh = quality.QualityScorer(DEV, "ssim,mmse,lpips", weights())
    _, worst32 = lpips_cases()["edit"]
    for f, (frames, oi, mask, recs) in zip(files, seen):
        out = json.loads(scored[f])
        assert out["metrics"] == ["ssim", "mmse", "lpips"] and out["lpips_weights"] == str(wf)
        assert out["alphas"] == [-8.0, -4.0, 0.0, 4.0, 8.0] and out["original_index"] == oi == 2 and out["masked"] is True
        assert len(out["frames"]) == 5 and tuple(frames.shape) == (5, 3, 32, 32) and frames.is_cuda
        assert float(frames.min()) >= 0.0 and float(frames.max()) <= 1.0 and tuple(mask.shape) == (3, 32, 32)
        assert out["frames"][2] == {"alpha": 0.0, "ssim": 1.0, "mmse_in": 0.0, "mmse_out": 0.0, "lpips": 0.0}
        again = fresh.score(frames, oi, mask)
        fr, orig = frames.cpu(), frames[oi:oi + 1].cpu()
        d64, _ = lpips_restated(fr, orig.expand_as(fr), weights(), normalize=True)
        for i in (0, 1, 3, 4):
            rec = {k: v for k, v in out["frames"][i].items() if k != "alpha"}
            assert rec == recs[i] == again[i]
            assert abs(rec["ssim"] - float(ev.ssim(fr[i:i + 1], orig, data_range=1.0))) <= 1e-9
            for key, m in (("mmse_in", mask), ("mmse_out", ~mask)):
                want = float(ev.masked_mse(fr[i:i + 1], orig, m[None].cpu()))
                assert abs(rec[key] - want) <= 1e-12 * want
            assert abs(rec["lpips"] - float(d64[i])) <= 4 * worst32 * float(d64[i])


def test_eval_main_backend_hip_matches_backend_torch(tmp_path):
    from loco_edit_amd.utils import save_image
    p, o = tmp_path / "p", tmp_path / "o"
    os.makedirs(p / "mask"); os.makedirs(o)
    x, y = image_pairs(2, 40, 36, AMPS["edit"], 9)
    m = torch.zeros(40, 36, dtype=torch.bool)
    m[5:11, 6:20] = True
    for i in range(2):
        save_image((x[i:i + 1] + 1) / 2, str(o / f"{i}.png"), padding=0)
        save_image((y[i:i + 1] + 1) / 2, str(p / f"{i}.png"), padding=0)
        torch.save(m, str(p / "mask" / f"{i}.pt"))
    wf = tmp_path / "w.pt"
    torch.save(weights(), str(wf))
    base = ["--folder_preds", str(p), "--folder_original", str(o), "--lpips_weights", str(wf)]
    t = {k: ev.main(base + ["--eval_metric", k, "--backend", "torch"]) for k in ("ssim", "mmse", "lpips")}
    h = {k: ev.main(base + ["--eval_metric", k, "--backend", "hip"]) for k in ("ssim", "mmse", "lpips")}
    assert all(h[k]["n"] == 2 and h[k]["metric"] == k for k in h)
    assert max(abs(a - b) for a, b in zip(h["ssim"]["values"], t["ssim"]["values"])) <= 1e-9
    assert max(abs(a - b) / b for a, b in zip(h["mmse"]["values"], t["mmse"]["values"])) <= 1e-12
    out = ev.main(base + ["--eval_metric", "mmse", "--outside_mask", "--backend", "hip"])
    assert abs(out["mean"] - ev.main(base + ["--eval_metric", "mmse", "--outside_mask"])["mean"]) <= 1e-12 * out["mean"]
    # LPIPS: against float64 of the same PNGs, within the bar of the edit-sized class
    xs = torch.cat([ev._load_png(str(p / f"{i}.png")) for i in range(2)]) / 127.5 - 1
    ys = torch.cat([ev._load_png(str(o / f"{i}.png")) for i in range(2)]) / 127.5 - 1
    d64, _ = lpips_restated(xs, ys, weights())
    _, worst32 = lpips_cases()["edit"]
    print(f"\neval.main lpips: float64 {d64.tolist()} torch {t['lpips']['values']} hip {h['lpips']['values']}")
    assert max(abs(v - float(d)) / float(d) for v, d in zip(h["lpips"]["values"], d64)) <= 4 * worst32
