"""MI355X: the Asyrp loss, trainer and asymmetric step (loco_edit_amd/asyrp.py) on TINY_DDPM at 32^2 (seeded weights, exact-fp32
conv arithmetic) with the tiny_a CLIP fixture, 2 synthetic latents and 3 timesteps (t = 749, 624, 499 of a 9-step schedule),
against the chained float64 oracle tests/asyrp_oracle.py:chain_step (tests/hspace_oracle.py -> the losses through
tests/clip_grad_oracle.py -> the block's restatement).  The block starts from seeded non-trivial parameters: with W2 = c2 = 0 the
directional loss sits at its kink (both frames embed alike) where autograd has no gradient to compare with.

* the directional loss and its pixel gradient against float64 at RELBAR, the bar of test_gpu_clip_grad.py (4 x the smallest
  stored fp32-autograd error of the CLIP fixtures);
* one AsyrpTrainer.step from the same seeded parameters at each of the 2 x 3 (latent, timestep) cases: each of the ten parameter
  gradients, max |g - g64| / max |g64|, within 4 x the yardstick = the largest error the fp32 run of the same chain makes on that
  parameter over those cases; the three losses likewise; x_t' at the engine's f32 forward bar (2e-5 rel-L2, test_gpu_hspace.py);
* 6 steps (2 latents x 3 timesteps): the loss sequence follows the float64 run within 4 x the largest relative deviation of
  the fp32 run; the parameters of two runs are bit-identical;
* the asymmetric step against the restatement (bound in the test) and, with one network output for both terms, bit-identical to
  sched_step(eta = 0);
* a checkpoint round-trips bit-exactly; inference with an untrained block reproduces the plain decode of the same x_T bit for bit.

Measured on MI355X (yardstick / HIP):
  directional loss 9.3e-09 and its pixel gradient 2.4e-06 (RELBAR 8.0e-06); gradients of one step g1 6.6e-05 / 7.9e-05,
  b1 7.3e-05 / 6.0e-05, W1 7.4e-05 / 7.2e-05, c1 = Wt = ct 6.7e-05 / 7.9e-05, g2 8.1e-05 / 5.9e-05, b2 8.4e-05 / 7.5e-05,
  W2 8.6e-05 / 5.9e-05, c2 9.2e-05 / 6.6e-05 (E_I(x0_edit) - E_I(x0_src) cancels: both runs inherit the fp32 rounding of the two
  embeddings); the three losses 5.0e-05 / 3.0e-05; x_t' 3.7e-07 - 4.4e-07 rel-L2; loss sequence of 6 steps 5.0e-04 / 6.0e-05;
  asymmetric step 3.05 x 2^-24 of its terms.
"""
import importlib.util
import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loco_edit_amd  # noqa: E402,F401
import loco_oracle as orc  # noqa: E402
from loco_edit_amd import asyrp, clip_score as cs  # noqa: E402
from loco_edit_amd.config import TINY_DDPM, synth_params  # noqa: E402
import asyrp_oracle as ao  # noqa: E402
import clip_grad_oracle as cgo  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_spec = importlib.util.spec_from_file_location("gpu_clip_vision", os.path.join(ROOT, "tests", "test_gpu_clip_vision.py"))
_cv = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cv)
GOLD = os.path.join(ROOT, "tests", "golden", "clip_vision")
RELBAR = 4 * min(float(torch.load(os.path.join(GOLD, f"{n}_grad.pt"))["err32"].min()) for n in ("tiny_a", "tiny_b"))
CFG = TINY_DDPM
SRC, TGT = "a photo of a man", "a photo of a man wearing glasses"
LR, WC, WR = 1e-3, 0.8, 3.0
STEP_IDX = (2, 3, 4)          # of the 9-step schedule


@pytest.fixture(scope="module")
def engine():
    from loco_edit_amd.hip import LocoEngine
    e = LocoEngine(CFG, max_batch=2, device=torch.device(DEV))
    e.load_state_dict(synth_params(CFG, 0))
    e.set_precision("f32")
    return e


@pytest.fixture(scope="module")
def sched(engine):
    from loco_edit_amd.scheduler import YHCustomScheduler
    s = YHCustomScheduler(engine=engine)
    s.set_timesteps(9)
    return s


@pytest.fixture(scope="module")
def scorer(tmp_path_factory):
    root = _cv.write_clip_folder(str(tmp_path_factory.mktemp("clip_asyrp") / "tiny_a"), "tiny_a")
    sc = cs.load_clip(root, device=torch.device(DEV), max_images=2, grad=True)
    return sc, sc.text_embeds([SRC, TGT])


def new_block(params=None, seed=None):
    from loco_edit_amd.hip import LocoAsyrpBlock
    C_, H, W = 64, 8, 8
    blk = LocoAsyrpBlock(C_, H, W, CFG.temb_ch, max_batch=1, gn_eps=CFG.gn_eps, seed=seed, device=torch.device(DEV))
    if params is not None:
        blk.load_state_dict(params)
    return blk


def block_params():
    p = ao.random_params(64, CFG.temb_ch, seed=21)
    p["W2"] = 0.5 * p["W2"]
    return p


def latents():
    g = torch.Generator().manual_seed(17)
    return [torch.randn(1, 3, 32, 32, generator=g) for _ in range(2)]


def schedule(sched):
    ts, tn = sched.timesteps, sched.timesteps_next
    return [(float(ts[i]), float(tn[i]), sched.alpha_at(ts[i]), sched.alpha_at(tn[i])) for i in STEP_IDX]


_ORACLE = {}


def oracle_runs(sched, text):
    """The 6 steps in float64 and in fp32: per step (loss, l_dir, l_rec, grads, x_next), the parameters moving by the restated Adam."""
    if not _ORACLE:
        net = orc.to_torch(synth_params(CFG, 0))
        _, _, vsd, vcfg = _cv.fixture("tiny_a")
        for dt in (torch.float64, torch.float32):
            opt = ao.Adam({k: v.to(dt) for k, v in block_params().items()}, LR)
            steps = []
            for x_T in latents():
                x = x_T.to(dt)
                for t, t_next, at, an in schedule(sched):
                    loss, l_dir, l_rec, grads, x_next, dh = ao.chain_step(net, CFG, vsd, vcfg, opt.p, x, t, at, an, text[0], text[1], WC, WR, dt)
                    opt.step(grads)
                    steps.append(SimpleNamespace(loss=float(loss), l_dir=float(l_dir), l_rec=float(l_rec), grads=grads, x_next=x_next, dh=dh))
                    x = x_next
            _ORACLE[dt] = steps
    return _ORACLE[torch.float64], _ORACLE[torch.float32]


_CASES = {}


def oracle_cases(sched, text):
    """One step from the SAME seeded parameters at each of the 2 latents x 3 timesteps, in float64 and in fp32: the cases the
    gradient yardstick is taken over (no Adam drift between the two runs: both differentiate at the same point)."""
    if not _CASES:
        net = orc.to_torch(synth_params(CFG, 0))
        _, _, vsd, vcfg = _cv.fixture("tiny_a")
        for dt in (torch.float64, torch.float32):
            p = {k: v.to(dt) for k, v in block_params().items()}
            _CASES[dt] = [ao.chain_step(net, CFG, vsd, vcfg, p, x_T.to(dt), t, at, an, text[0], text[1], WC, WR, dt)
                          for x_T in latents() for t, _, at, an in schedule(sched)]
    return _CASES[torch.float64], _CASES[torch.float32]


def hip_run(engine, sched, scorer, n_steps=6):
    sc, text = scorer
    blk = new_block(block_params())
    tr = asyrp.AsyrpTrainer(engine, sched, sc, blk, text[0], text[1], CFG, lr=LR, clip_weight=WC, rec_weight=WR)
    out = []
    for x_T in latents():
        x = x_T.to(DEV)
        for t, t_next, at, an in schedule(sched):
            if len(out) == n_steps:
                break
            x = tr.step(x, t, t_next)
            out.append(SimpleNamespace(x_next=x.cpu(), grads=blk.grads() if len(out) == 0 else None, **tr.last))
    return out, blk


def test_directional_loss_vs_float64(scorer):
    sc, text = scorer
    _, _, vsd, vcfg = _cv.fixture("tiny_a")
    fr = torch.stack([_cv.smooth_noise_image(32, 32, seed=3 + i).permute(2, 0, 1).float() / 127.5 - 1 for i in range(2)])
    x64 = fr[:1].double().clone().requires_grad_(True)
    pv = cgo.preprocess_windows(torch.cat([x64, fr[1:].double()]), None, vcfg.image_size, vcfg.image_mean, vcfg.image_std)
    emb = cgo.clip_vision_embeds(vsd, vcfg, pv)
    want = ao.directional_loss(emb[0], emb[1].detach(), text[0].double(), text[1].double())
    want.backward()
    loss, grad = asyrp.directional_clip_loss(sc, fr[:1].to(DEV), fr[1:].to(DEV), text[0], text[1])
    lerr = abs(float(loss) - float(want.detach())) / abs(float(want.detach()))
    gerr = float((grad.double().cpu() - x64.grad).norm() / x64.grad.norm())
    print(f"directional loss {float(loss):.6f} rel err {lerr:.2e}, pixel gradient rel-L2 {gerr:.2e} (bar {RELBAR:.2e})")
    assert tuple(grad.shape) == (1, 3, 32, 32)
    assert lerr <= RELBAR and gerr <= RELBAR
    l2, g2 = asyrp.directional_clip_loss(sc, fr[:1].to(DEV), fr[1:].to(DEV), text[0], text[1])
    assert torch.equal(l2, loss) and torch.equal(g2, grad)


def test_one_step_gradients_vs_chained_oracle(engine, sched, scorer):
    sc, text = scorer
    c64, c32 = oracle_cases(sched, text)
    yard = {k: max(ao.rel_err(b[3][k], a[3][k]) for a, b in zip(c64, c32)) for k in ao.PARAMS}
    yard_loss = max(abs(float(b[j]) - float(a[j])) / abs(float(a[j])) for a, b in zip(c64, c32) for j in range(3))
    cases = [(x_T, step) for x_T in latents() for step in schedule(sched)]
    bad, worst = [], {k: 0.0 for k in ao.PARAMS}
    for i, (x_T, (t, t_next, at, an)) in enumerate(cases):
        blk = new_block(block_params())
        tr = asyrp.AsyrpTrainer(engine, sched, sc, blk, text[0], text[1], CFG, lr=LR, clip_weight=WC, rec_weight=WR)
        x_next = tr.step(x_T.to(DEV), t, t_next)
        grads = blk.grads()
        want_loss, want_dir, want_rec, want_grads, want_next, _ = c64[i]
        for k in ao.PARAMS:
            err = ao.rel_err(grads[k], want_grads[k])
            worst[k] = max(worst[k], err)
            if not err <= 4 * yard[k]:
                bad.append((i, k, err, yard[k]))
        # the forward half: x_t' at the engine's own bar for an f32 forward (test_gpu_hspace.py FWD); the three losses against the
        # fp32 chain's own error like the gradients (E_I(x0_edit) - E_I(x0_src) cancels: the bar of a loss of GIVEN frames, RELBAR,
        # does not carry over to frames that come with the network's rounding)
        ex = float((x_next.cpu().double() - want_next).norm() / want_next.norm())
        el = max(abs(tr.last[n] - float(w)) / abs(float(w)) for n, w in (("loss", want_loss), ("l_dir", want_dir), ("l_rec", want_rec)))
        print(f"case {i} (t = {t}): loss {tr.last['loss']:.6f}, worst rel err of the three losses {el:.2e} (yardstick {yard_loss:.2e}), "
              f"x_t' rel-L2 {ex:.2e}")
        if not ex < 2e-5:
            bad.append((i, "x_next", ex, 2e-5))
        if not el <= 4 * yard_loss:
            bad.append((i, "loss", el, yard_loss))
    for k in ao.PARAMS:
        print(f"grad:{k}: yardstick {yard[k]:.2e}, worst HIP over the 6 cases {worst[k]:.2e}")
    assert not bad, bad


def test_six_steps_follow_the_float64_run(engine, sched, scorer):
    r64, r32 = oracle_runs(sched, scorer[1])
    got, _ = hip_run(engine, sched, scorer)
    ly = max(abs(b.loss - a.loss) / abs(a.loss) for a, b in zip(r64, r32))
    lerrs = [abs(g.loss - a.loss) / abs(a.loss) for a, g in zip(r64, got)]
    print("loss float64:", ["%.6f" % a.loss for a in r64], "| fp32 chain:", ["%.6f" % b.loss for b in r32], "| HIP:", ["%.6f" % g.loss for g in got])
    print(f"loss sequence: fp32 chain worst {ly:.2e}, HIP per step {['%.2e' % e for e in lerrs]}")
    assert max(lerrs) <= 4 * ly
    assert len({round(a.loss, 9) for a in r64}) == 6            # the parameters and the inputs move: six different losses


def test_two_runs_are_bit_identical(engine, sched, scorer):
    (a, blk_a), (b, blk_b) = hip_run(engine, sched, scorer), hip_run(engine, sched, scorer)
    sa, sb = blk_a.state_dict(), blk_b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in ao.PARAMS)
    assert all(torch.equal(x.x_next, y.x_next) and x.loss == y.loss for x, y in zip(a, b))
    p0 = block_params()
    assert not any(torch.equal(sa[k], p0[k]) for k in ao.PARAMS)


def test_asymmetric_step(engine):
    g = torch.Generator().manual_seed(8)
    x, e1, e2 = (torch.randn(1, 3, 32, 32, generator=g) for _ in range(3))
    at, an = 0.37, 0.52
    nxt, x0 = engine.sched_step_asym(x.to(DEV), e1.to(DEV), e2.to(DEV), at, an, want_x0=True)
    want = ao.asym_step(x.double(), e1.double(), e2.double(), at, an)
    want0 = (x.double() - (1 - at) ** 0.5 * e1.double()) / at ** 0.5
    # fp32 coefficients (a rounding each on a, a', their roots) and four rounded operations: 2^-21 of the terms' magnitudes
    terms = an ** 0.5 / at ** 0.5 * (x.abs() + (1 - at) ** 0.5 * e1.abs()).double() + (1 - an) ** 0.5 * e2.abs().double()
    err = ((nxt.cpu().double() - want).abs() / terms).max()
    print(f"asymmetric step: worst error {float(err) * 2 ** 24:.2f} x 2^-24 of the terms")
    assert float(err) <= 2.0 ** -21
    assert float(((x0.cpu().double() - want0).abs() / (terms / an ** 0.5)).max()) <= 2.0 ** -21
    same, p_same = engine.sched_step_asym(x.to(DEV), e1.to(DEV), e1.to(DEV), at, an, want_x0=True)
    ddim, p_ddim = engine.sched_step(x.to(DEV), e1.to(DEV), at, an, 0.0, None, want_x0=True)
    assert torch.equal(same, ddim) and torch.equal(p_same, p_ddim)
    with pytest.raises(ValueError, match="same number of elements"):
        engine.sched_step_asym(x.to(DEV), e1.to(DEV), e2[:, :2].contiguous().to(DEV), at, an)


def test_checkpoint_round_trip(engine, sched, scorer, tmp_path):
    _, blk = hip_run(engine, sched, scorer, n_steps=2)
    path = str(tmp_path / "ckpt" / "asyrp.pt")
    asyrp.save_checkpoint(path, blk, 2, {"src_prompt": SRC})
    other = new_block(seed=5)
    assert asyrp.load_checkpoint(path, other) == 2
    a, b = blk.state_dict(), other.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in ao.PARAMS)
    h, e = torch.randn(1, 64, 8, 8, device=DEV), asyrp.time_vector(CFG, 499.0).to(DEV)
    assert torch.equal(blk.forward(h, e), other.forward(h, e))
    from loco_edit_amd.hip import LocoAsyrpBlock
    wrong = LocoAsyrpBlock(64, 4, 4, CFG.temb_ch, device=torch.device(DEV))
    with pytest.raises(ValueError, match="geometry"):
        asyrp.load_checkpoint(path, wrong)
    torch.save({"g1": a["g1"]}, str(tmp_path / "part.pt"))
    with pytest.raises(ValueError, match="no Asyrp checkpoint"):
        asyrp.load_checkpoint(str(tmp_path / "part.pt"), other)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_untrained_block_reproduces_the_plain_decode(engine, prec):
    from loco_edit_amd import hspace_pca
    from loco_edit_amd.scheduler import YHCustomScheduler
    engine.set_precision(prec)
    try:
        s = YHCustomScheduler(engine=engine)
        ed = SimpleNamespace(engine=engine, scheduler=s, for_steps=9, device=torch.device(DEV), performance_boosting_t_idx=1000)
        s.set_timesteps(9)
        x_T = latents()[0].to(DEV)
        plain = hspace_pca.decode_with_dh(ed, x_T, 0, None)
        blk = new_block(seed=0)
        x_mid = asyrp.edit(engine, s, blk, CFG, x_T, 5, scale=1.0)
        out = hspace_pca.decode_with_dh(ed, x_mid, 5, None)
        assert torch.equal(out, plain)
        trained = new_block(block_params())
        x_mid2 = asyrp.edit(engine, s, trained, CFG, x_T, 5, scale=1.0)
        assert not torch.equal(x_mid2, x_mid) and bool(torch.isfinite(x_mid2).all())
        assert torch.equal(asyrp.edit(engine, s, trained, CFG, x_T, 5, scale=0.0), x_mid)      # scale 0: the plain steps
    finally:
        engine.set_precision("f32")
