"""GPU tests of the CLIP pixel gradient (csrc/clipvis.hip: loco_clipvis_enable_grad / _encode_vjp / _preprocess_f32 / _preprocess_f32_vjp
through hip.LocoClipVisionEngine and clip_score.ClipScorer.text_guidance).

* ``encode_vjp`` against transformers' float64 autograd gradient (tests/golden/clip_vision/tiny_*_grad.pt), rel-L2 per image.
  The bar is 4 x the error transformers' own fp32 autograd makes on that image (stored in the fixture, checked on the CPU by
  test_clip_grad_host.py): the same unit roundoff, another summation order (64-wide exact-fp32 MFMA chains, fixed key order).
* Head widths 92, 96 and 106, where the attention cotangent streams chunks of 32 tokens instead of 64, against the float64
  restatement of tests/clip_grad_oracle.py at 4 x the error of the same restatement under fp32 autograd.
* Bit identities (torch.equal): a grad-enabled encode against a plain handle's; an image's gradient alone against every position
  of a full max_images batch; call against call; under LOCO_PRECISION=f16.
* ``preprocess_float`` and its transpose against the float64 restatement of tests/clip_grad_oracle.py on 40 x 56 and 48 x 40
  frames with S = 16: forward 1e-3 grey level (1e-3 / 255 * 2 on the [-1, 1] scale before the normalisation, the bar of the
  uint8 preprocessing test); the transpose against the restatement's autograd at RELBAR and against the unit's own forward by
  <R dx, y> = <dx, R^T y> to 1e-5 relative.
* ``text_guidance`` loss and gradient end to end against the float64 oracle at RELBAR.
* Refusals are errors and leave a usable handle.

RELBAR, the relative bar of everything that has no stored error of its own, is 4 x the smallest stored fp32-autograd error."""
import importlib.util
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import clip_score as cs  # noqa: E402
import clip_grad_oracle as cgo  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(ROOT, "tests", "golden", "clip_vision")
_spec = importlib.util.spec_from_file_location("gpu_clip_vision", os.path.join(ROOT, "tests", "test_gpu_clip_vision.py"))
_cv = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cv)
fixture, write_clip_folder, rel_rows = _cv.fixture, _cv.write_clip_folder, _cv.rel_rows

_GRADS = {}


def grads(name):
    if name not in _GRADS:
        _GRADS[name] = torch.load(os.path.join(GOLD, f"{name}_grad.pt"))
    return _GRADS[name]


RELBAR = 4 * min(float(grads(n)["err32"].min()) for n in ("tiny_a", "tiny_b"))


def engine(vcfg, vsd, max_images, grad=True):
    from loco_edit_amd.hip import LocoClipVisionEngine
    eng = LocoClipVisionEngine(vcfg, max_images=max_images, device=torch.device(DEV), grad=grad)
    eng.load_state_dict(vsd)
    return eng


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_encode_vjp_vs_transformers_float64(name):
    g, _, vsd, vcfg = fixture(name)
    gg = grads(name)
    pv = g["pixel_values"]
    eng = engine(vcfg, vsd, pv.shape[0])
    assert eng.grad_bytes > 0
    eng.encode(pv)
    got = eng.encode_vjp(gg["g_embeds"])
    errs, ref = rel_rows(got, gg["grad64"]), gg["err32"].tolist()
    print(name, "encode_vjp rel-L2 per image vs float64 autograd:", ["%.2e" % e for e in errs], "| transformers fp32 autograd:",
          ["%.2e" % e for e in ref], f"| records + workspace {eng.grad_bytes} bytes")
    assert tuple(got.shape) == tuple(pv.shape)
    for e, r in zip(errs, ref):
        assert e <= 4 * r


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_bit_identities(name):
    g, _, vsd, vcfg = fixture(name)
    pv, ge = g["pixel_values"], grads(name)["g_embeds"]
    n = pv.shape[0]
    plain = engine(vcfg, vsd, n + 2, grad=False)
    eng = engine(vcfg, vsd, n + 2)
    assert plain.grad_bytes == 0
    for a, b in zip(plain.encode(pv, want_hidden=True), eng.encode(pv, want_hidden=True)):
        assert torch.equal(a, b)
    grad = eng.encode_vjp(ge)
    assert torch.equal(eng.encode_vjp(ge), grad)                      # the same records, again
    eng.encode(pv)
    assert torch.equal(eng.encode_vjp(ge), grad)                      # a second encode + vjp
    for i in range(n):                                                # alone
        eng.encode(pv[i:i + 1])
        assert torch.equal(eng.encode_vjp(ge[i:i + 1])[0], grad[i])
    full, gfull = torch.cat([pv, pv[:2]]), torch.cat([ge, ge[:2]])
    for shift in range(n + 2):                                        # at every position of a full batch
        e2 = eng.encode(torch.roll(full, shift, dims=0))
        assert torch.equal(torch.roll(e2, -shift, dims=0)[:n], plain.encode(pv))
        g2 = torch.roll(eng.encode_vjp(torch.roll(gfull, shift, dims=0)), -shift, dims=0)
        assert torch.equal(g2[:n], grad) and torch.equal(g2[n:], grad[:2])
    os.environ["LOCO_PRECISION"] = "f16"
    try:
        eng16 = engine(vcfg, vsd, n)
        assert torch.equal(eng16.encode(pv), plain.encode(pv))
        assert torch.equal(eng16.encode_vjp(ge), grad)
    finally:
        os.environ.pop("LOCO_PRECISION")


@pytest.mark.parametrize("hd", [92, 96, 106])
def test_wide_heads_take_the_32_token_chunk(hd):
    """Head widths above 88 (dK / dV) and 95 (dQ) stream chunks of 32 tokens instead of 64 (the 64 KiB of LDS): 92 mixes the two,
    96 and 106 (the widest head the forward accepts) run both kernels at 32.  T = 37: two chunks of 32 with a tail of 5, three
    query blocks.  No transformers fixture has such heads: seeded weights against the float64 restatement of
    tests/clip_grad_oracle.py (pinned to transformers by test_clip_grad_host.py), at 4 x the error the same restatement makes
    under fp32 autograd on the CPU."""
    cfg = cs.ClipVisionConfig(image_size=48, patch_size=8, width=2 * hd, layers=2, heads=2, mlp_dim=64, projection_dim=16, act="gelu")
    # q / k weights of std D^-1/2 on LayerNorm outputs: scores of order 1, a softmax that is neither flat nor one-hot.  (Scores
    # 36 x larger made the problem ill-conditioned: fp32 autograd's own error then ranged over 9e-7 ... 2e-4 from image to image.)
    sd = {k: v.cpu() for k, v in _cv._synth_clip_vision(cfg, 11).items()}
    gen = torch.Generator().manual_seed(hd)
    pv, ge = torch.randn(3, 3, 48, 48, generator=gen), torch.randn(3, 16, generator=gen)
    want = cgo.embeds_vjp(sd, cfg, pv, ge)
    ref = rel_rows(cgo.embeds_vjp(sd, cfg, pv, ge, dtype=torch.float32), want)
    plain, eng = engine(cfg, sd, 4, grad=False), engine(cfg, sd, 4)
    assert torch.equal(eng.encode(pv), plain.encode(pv))
    got = eng.encode_vjp(ge)
    errs = rel_rows(got, want)
    print(f"hd {hd}: encode_vjp rel-L2 per image vs float64:", ["%.2e" % e for e in errs], "| fp32 autograd on the CPU:", ["%.2e" % e for e in ref])
    for e, r in zip(errs, ref):
        assert e <= 4 * r
    eng.encode(torch.cat([pv[2:], pv[:1]]))           # another position, another n
    g2 = eng.encode_vjp(torch.cat([ge[2:], ge[:1]]))
    assert torch.equal(g2[0], got[2]) and torch.equal(g2[1], got[0])


# ------------------------------------------------------------------------------------------------------------ preprocessing
S16 = 16


@pytest.fixture(scope="module")
def engine16():
    from loco_edit_amd.hip import LocoClipVisionEngine
    cfg = cs.ClipVisionConfig(image_size=S16, patch_size=8, width=64, layers=1, heads=1, mlp_dim=64, projection_dim=8)
    return LocoClipVisionEngine(cfg, max_images=1, device=torch.device(DEV))


def float_frames(nf, H, W, seed):
    return torch.stack([_cv.smooth_noise_image(H, W, seed=seed + i).permute(2, 0, 1).float() / 127.5 - 1 for i in range(nf)])


def windows(H, W):
    """name -> (nf, boxes): (top, left, h, w) windows of an H x W frame for S = 16."""
    return {
        "whole frame": (1, [(0, 0, H, W)]),
        "flush with two borders": (1, [(H - 21, W - 23, 21, 23)]),
        "smaller than S (4 taps)": (1, [(3, 5, 10, 12)]),
        "at least 2 S wide": (1, [(2, 1, 2 * S16 + 2, 2 * S16 + 5)]),
        "non-square": (1, [(1, 2, 30, 17)]),
        "one frame, three windows": (1, [(0, 0, H, W), (4, 6, 20, 20), (H - 33, 0, 33, 35)]),
        "a frame per window": (3, [(0, 0, H, W), (4, 6, 9, 9), (H - 33, W - 35, 33, 35)]),
        "centred squares": (2, None),
    }


@pytest.mark.parametrize("H,W", [(40, 56), (48, 40)])
def test_preprocess_float_and_its_transpose(engine16, H, W):
    assert cgo.tap_count(10, S16) == 4 and cgo.tap_count(2 * S16 + 2, S16) > 4
    std = torch.tensor(cs.CLIP_STD, dtype=torch.float64).view(1, 3, 1, 1)
    for k, (what, (nf, boxes)) in enumerate(windows(H, W).items()):
        gen = torch.Generator().manual_seed(1000 * H + k)
        fr = float_frames(nf, H, W, seed=10 * k + H)
        want = cgo.preprocess_windows(fr, boxes, S16, cs.CLIP_MEAN, cs.CLIP_STD)
        got = engine16.preprocess_float(fr.to(DEV), boxes).double().cpu()
        assert tuple(got.shape) == tuple(want.shape)
        ferr = float(((got - want) * std * 2).abs().max())             # on the [-1, 1] scale, before the normalisation
        # the transpose against autograd of the restatement
        n = want.shape[0]
        y = torch.randn(n, 3, S16, S16, generator=gen)
        x64 = fr.double().clone().requires_grad_(True)
        (cgo.preprocess_windows(x64, boxes, S16, cs.CLIP_MEAN, cs.CLIP_STD) * y.double()).sum().backward()
        gt = engine16.preprocess_float_vjp(y.to(DEV), boxes, nf, H, W)
        assert tuple(gt.shape) == (nf, 3, H, W)
        assert torch.equal(engine16.preprocess_float_vjp(y.to(DEV), boxes, nf, H, W), gt)
        verr = float((gt.double().cpu() - x64.grad).norm() / x64.grad.norm())
        # <R dx, y2> = <dx, R^T y2> against the unit's own forward; y2 close to R dx, so that the product is well conditioned
        fr2 = float_frames(nf, H, W, seed=10 * k + H + 500)
        rdx = engine16.preprocess_float(fr.to(DEV), boxes) - engine16.preprocess_float(fr2.to(DEV), boxes)
        y2 = rdx + 0.5 * rdx.std() * torch.randn(rdx.shape, generator=gen).to(DEV)
        lhs = float((rdx.double() * y2.double()).sum())
        rhs = float(((fr - fr2).double().to(DEV) * engine16.preprocess_float_vjp(y2, boxes, nf, H, W).double()).sum())
        aerr = abs(lhs - rhs) / abs(lhs)
        print(f"{H}x{W} {what}: forward max abs {ferr:.2e} (bar {1e-3 / 255 * 2:.2e}), transpose rel-L2 {verr:.2e} (bar {RELBAR:.2e}), "
              f"adjoint identity {aerr:.2e} (bar 1e-5)")
        assert ferr <= 1e-3 / 255 * 2
        assert verr <= RELBAR
        assert aerr <= 1e-5


# ------------------------------------------------------------------------------------------------------------- text guidance
@pytest.fixture(scope="module")
def scorer(tmp_path_factory):
    root = write_clip_folder(str(tmp_path_factory.mktemp("clip_grad") / "tiny_a"), "tiny_a")
    return cs.load_clip(root, device=torch.device(DEV), max_images=2, grad=True)


@pytest.mark.parametrize("case", ["one frame, three windows", "a frame per window, centred squares"])
def test_text_guidance_vs_float64_oracle(scorer, case):
    g, _, vsd, vcfg = fixture("tiny_a")
    text = grads("tiny_a")["text_embed"]
    frames = g["frames"].permute(0, 3, 1, 2).float() / 127.5 - 1       # [3, 3, 48, 40]
    if case.startswith("one"):
        fr, boxes = frames[:1], [(0, 0, 48, 40), (5, 3, 36, 36), (10, 0, 38, 40)]     # 3 windows on max_images = 2: two encodes
    else:
        fr, boxes = frames[:2], None
    want_loss, want_grad = cgo.text_guidance(vsd, vcfg, fr, text, boxes)
    loss, grad = scorer.text_guidance(fr.to(DEV), text, boxes)
    assert tuple(loss.shape) == tuple(want_loss.shape) and tuple(grad.shape) == tuple(fr.shape)
    lerr = float(((loss.double().cpu() - want_loss) / want_loss).abs().max())
    gerr = max(rel_rows(grad, want_grad))
    print(f"text_guidance, {case}: loss {['%.6f' % v for v in loss.tolist()]} rel err {lerr:.2e}, gradient rel-L2 {gerr:.2e} (bar {RELBAR:.2e})")
    assert lerr <= RELBAR and gerr <= RELBAR
    l2, g2 = scorer.text_guidance(fr.to(DEV), text, boxes)
    assert torch.equal(l2, loss) and torch.equal(g2, grad)


def test_text_guidance_needs_grad(tmp_path):
    root = write_clip_folder(str(tmp_path / "tiny_a"), "tiny_a")
    sc = cs.load_clip(root, device=torch.device(DEV), max_images=2)
    with pytest.raises(RuntimeError, match="grad=True"):
        sc.text_guidance(torch.zeros(1, 3, 40, 40), grads("tiny_a")["text_embed"])


def test_refusals_are_errors():
    g, _, vsd, vcfg = fixture("tiny_a")
    pv, ge = g["pixel_values"], grads("tiny_a")["g_embeds"]
    plain = engine(vcfg, vsd, 3, grad=False)
    plain.encode(pv)
    with pytest.raises(RuntimeError, match="keeps no records"):
        plain.encode_vjp(ge)
    assert torch.equal(plain.encode(pv), plain.encode(pv))
    eng = engine(vcfg, vsd, 3)
    with pytest.raises(RuntimeError, match="no kept"):
        eng.encode_vjp(ge)
    eng.encode(pv)
    with pytest.raises(RuntimeError, match="the kept encode carried 3"):
        eng.encode_vjp(ge[:2])
    with pytest.raises(ValueError, match="g_embeds must be"):
        eng.encode_vjp(ge[:, :5])
    grad = eng.encode_vjp(ge)
    fr = float_frames(2, 40, 56, seed=1).to(DEV)
    for box in ((0, 0, 41, 56), (-1, 0, 10, 10), (0, 50, 10, 7), (0, 0, 0, 10)):
        with pytest.raises(RuntimeError, match="leaves the 40 x 56 frame"):
            eng.preprocess_float(fr[:1], [box])
        with pytest.raises(RuntimeError, match="leaves the 40 x 56 frame"):
            eng.preprocess_float_vjp(pv[:1], [box], 1, 40, 56)
    with pytest.raises(RuntimeError, match="must be 1 or n"):
        eng.preprocess_float(fr, [(0, 0, 40, 56)] * 3)                  # nf = 2, n = 3
    with pytest.raises(RuntimeError, match="must be 1 or n"):
        eng.preprocess_float_vjp(pv, [(0, 0, 40, 56)] * 3, 2, 40, 56)
    with pytest.raises(ValueError, match="boxes must be"):
        eng.preprocess_float(fr[:1], [(0.0, 0.0, 40.0, 56.0)])
    with pytest.raises(ValueError, match="frames must be"):
        eng.preprocess_float(torch.zeros(1, 40, 56, 3, dtype=torch.uint8))
    assert torch.equal(eng.encode_vjp(ge), grad)                       # the handle still works
    assert eng.preprocess_float(fr).shape == (2, 3, 32, 32)
