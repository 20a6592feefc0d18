"""MI355X: DiffEdit on the DeepFloyd-IF path -- the two kernels of csrc/diffedit.hip (loco_diffedit_mask,
loco_cfg_masked_step) against float64 / the composition of the existing kernels, EditDeepFloydIF.mask_diffedit and
MaskedDDPMforwardsteps against the fixture the reference's own methods produced (tests/golden/tloco_diffedit.pt,
oracle/make_golden_tloco_diffedit.py), the drivers and the CLI from two prompts and a seed with no mask.pt, and both
methods at the IF stage-I architecture's size."""
import math
import os
from argparse import Namespace

import pytest
import torch

from loco_edit_amd.config import TINY_ADM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {"f32": 2e-5, "bf16x3": 1e-4}       # single guided evaluation, rel-L2 (tests/test_gpu_tloco.py)
U = 2.0 ** -24                            # unit round-off of fp32
BAND = 1e-2                               # test 4: pixels whose reference ||z| - 0.5| is below this may flip


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _edit(g, tmp_path, prec, **kw):
    from loco_edit_amd.tloco import EditDeepFloydIF
    os.environ.pop("WORLD_SIZE", None)
    args = Namespace(device=torch.device(DEV), dtype=torch.float32, seed=1, unet_config=kw.get("cfg", TINY_ADM), synthetic_weights=0,
                     ckpt_path="", max_batch=kw.get("max_batch", 8), precision=prec, dataset_name="Random", for_steps=100,
                     use_yh_custom_scheduler=True, guidance_scale=kw.get("guidance_scale", g["guidance_scale"]),
                     guidance_scale_edit=g["guidance_scale_edit"],
                     prompt_emb={"for": g["for_e"], "edit": g["edit_e"], "null": g["null_e"]}, for_prompt="a cat",
                     edit_prompt="a dog", edit_t=0.6, sampling_mode=kw.get("sampling_mode", False),
                     tilda_v_score_type="null+(for-null)+(edit-null)", ablation_method=kw.get("ablation", "null-space-proj"),
                     mask_type=kw.get("mask_type", "diffedit"), vT_path="", x_space_guidance_edit_step=1.0,
                     x_space_guidance_scale=0.5, x_space_guidance_num_step=16, result_folder=str(tmp_path))
    return EditDeepFloydIF(args)


def _both(golden):
    g = dict(golden("tloco_tiny"))
    g.update(golden("tloco_diffedit"))
    return g


@pytest.fixture(scope="module")
def tiny_ed(golden, tmp_path_factory):
    return _edit(_both(golden), tmp_path_factory.mktemp("kernels"), "f32")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the kernels against torch on random inputs
def _map64(a, b, scale):
    return (scale * (a.double() - b.double())).mean(dim=0).mean(dim=0).reshape(-1)


@pytest.mark.parametrize("B,C,HW", [(1, 3, 32 * 32), (10, 3, 64 * 64), (13, 3, 256 * 256), (10, 4, 64 * 64), (3, 2, 33 * 33)])
def test_diffedit_mask_kernel_vs_float64(B, C, HW, tiny_ed):
    """m within B C 2^-24 max|scale (a - b)| of the float64 value: the mean of n = B C terms computed as an fp32 sum
    (error <= (n - 1) u sum|x_i| <= n^2 u max|x_i|) divided by n.  The mask equals the float64 mask wherever z is further
    from its flip point than that bound eps times the sensitivity of z to m, min and max -- each of the three is a value
    of the map, so each carries an error of at most eps -- plus the fp32 evaluation of z itself:
      reference  z = m - min / R, R = max - min:   |dz| <= eps (1 + 1 / R + 2 |min| / R^2)  +  4 u (1 + |min / R| + max|m|)
      intended   z = (m - min) / R:                |dz| <= eps (2 / R + 2 |m - min| / R^2) <= 4 eps / R  +  4 u
    (33 x 33: a map whose length is no multiple of four, the scalar-load form of the kernel)."""
    eng = tiny_ed.engine
    gen = torch.Generator().manual_seed(100 + B + C)
    a, b = torch.randn(B, C, HW, generator=gen), torch.randn(B, C, HW, generator=gen)
    scale = 7.5
    m64 = _map64(a, b, scale)
    eps = B * C * U * float((scale * (a.double() - b.double())).abs().max())
    mn, mx = float(m64.min()), float(m64.max())
    R = mx - mn
    for rule in ("reference", "intended"):
        mask, m = eng.diffedit_mask(a.to(DEV), b.to(DEV), scale, rule=rule, want_map=True)
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == (HW,) == tuple(m.shape)
        err = float((m.cpu().double() - m64).abs().max())
        print(f"[{B},{C},{HW}] {rule}: max |m - m64| {err:.3e}, bound {eps:.3e}")
        assert err <= eps
        if rule == "reference":
            z = m64 - mn / R
            dist = (z.abs() - 0.5).abs()
            want = z.abs() > 0.5
            dz = eps * (1 + 1 / R + 2 * abs(mn) / R ** 2) + 4 * U * (1 + abs(mn / R) + float(m64.abs().max()))
        else:
            z = (m64 - mn) / R
            dist = (z - 0.5).abs()
            want = z > 0.5
            dz = 4 * eps / R + 4 * U
        sure = dist > dz
        assert float(sure.float().mean()) > 0.99                     # the excluded band is a sliver
        assert torch.equal(mask.cpu().bool()[sure], want[sure])
        assert 0.0 < float(mask.float().mean()) < 1.0
        # without the map: the same mask (the map then lives in the context's reduction workspace)
        assert torch.equal(eng.diffedit_mask(a.to(DEV), b.to(DEV), scale, rule=rule), mask)


def test_diffedit_mask_kernel_ties_constant_map_and_arguments(tiny_ed):
    eng = tiny_ed.engine
    zero = torch.zeros(1, 1, 4, device=DEV)
    # min 1, max 3: c = 0.5, z = 0.5 / 1 / 1.5 / 2.5 -- |z| = 0.5 rounds to 0 (half to even), 1.5 to 2
    m = torch.tensor([1.0, 1.5, 2.0, 3.0], device=DEV).view(1, 1, 4)
    assert eng.diffedit_mask(m, zero, 1.0).tolist() == [0, 1, 1, 1]
    assert eng.diffedit_mask(m, zero, 1.0, rule="intended").tolist() == [0, 0, 0, 1]
    # min -3, max -1: c = -1.5, z = -1.5 / -0.5 / 0.5 / -0.25
    m = torch.tensor([-3.0, -2.0, -1.0, -1.75], device=DEV).view(1, 1, 4)
    mask, mm = eng.diffedit_mask(m, zero, 1.0, want_map=True)
    assert mask.tolist() == [1, 0, 0, 0] and mm.tolist() == [-3.0, -2.0, -1.0, -1.75]
    assert eng.diffedit_mask(m, zero, 1.0, rule="intended").tolist() == [0, 0, 1, 1]
    # batch first, then channels: B = 2, C = 2
    a = torch.tensor([[[1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 0.0, 8.0]], [[3.0, 2.0, 1.0, 0.0], [0.0, 4.0, 0.0, 0.0]]], device=DEV)
    _, mm = eng.diffedit_mask(a, torch.zeros_like(a), 2.0, want_map=True)
    assert mm.tolist() == [2.0, 4.0, 2.0, 6.0]
    # identical predictions: the reference divides by zero and returns an all-True mask out of NaN; here an error
    x = torch.randn(10, 3, 32, 32, device=DEV)
    with pytest.raises(ValueError, match="constant map"):
        eng.diffedit_mask(x, x.clone(), 7.5)
    with pytest.raises(ValueError, match="non-finite"):
        eng.diffedit_mask(x, torch.full_like(x, float("nan")), 7.5)
    with pytest.raises(ValueError):
        eng.diffedit_mask(x, x[:5].contiguous(), 7.5)
    with pytest.raises(ValueError):
        eng.diffedit_mask(x, x.clone(), 7.5, rule="minmax")
    # the engine is usable afterwards
    assert eng.diffedit_mask(m, zero, 1.0).tolist() == [1, 0, 0, 0]


def _step_ulp_bound(x, f, e, nn, g, at, atn):
    """Elementwise bound on the difference of two fp32 evaluations of the guided DDIM update that associate the guided noise
    differently: 8 u M, M = the sum of the magnitudes of the terms either evaluation forms,
    M = sqrt(at'/at) (|x| + sqrt(1 - at) E) + sqrt(1 - at') E with E = g max(|f|, |e|) + |1 - g| |n| >= every intermediate of the
    guided noise.  Each evaluation makes about six roundings, each at most u times an intermediate <= M; 8 covers both."""
    E = g * torch.maximum(f.abs(), e.abs()) + abs(1.0 - g) * nn.abs()
    return 8 * U * (math.sqrt(atn / at) * (x.abs() + math.sqrt(1 - at) * E) + math.sqrt(1 - atn) * E)


@pytest.mark.parametrize("B,n", [(1, 3 * 32 * 32), (5, 3 * 64 * 64), (2, 3 * 33 * 33)])
def test_cfg_masked_step_kernel_vs_composition(B, n, tiny_ed):
    """Against lincomb -> sched_step (twice) -> torch.where.  The two ways associate the guided noise differently
    (n + g (f - n) here, as the reference writes it; g f + (1 - g) n in lincomb), a handful of fp32 roundings apart.
    (a) rtol 1e-5 / atol 1e-6 on predictions as a denoiser gives them for one x_t under three prompts: unit scale, a tenth
        apart, so that the guided noise stays below 8 in magnitude.  An absolute tolerance of 1e-6 presupposes that: one ulp of
        a value of 8 is 9.5e-7, and the update forms sqrt(at'/at) (x - sqrt(1 - at) eps) and sqrt(1 - at') eps separately before
        they nearly cancel, so each carries the ulp of the guided noise into the result.
    (b) independent unit-normal predictions, where g (f - n) reaches 30 and one ulp of an intermediate exceeds 1e-6: the
        elementwise bound of _step_ulp_bound.
    Timesteps: the edit step (600 -> 590), 300 -> 290 and 100 -> 90.  (33 x 33 frames: the scalar-load form.)"""
    eng, sch = tiny_ed.engine, tiny_ed.scheduler
    gen = torch.Generator().manual_seed(7 + B)
    x, nn = (torch.randn(B, n, generator=gen).to(DEV) for _ in range(2))
    near = [(nn + 0.1 * torch.randn(B, n, generator=gen).to(DEV)).contiguous() for _ in range(2)]
    far = [torch.randn(B, n, generator=gen).to(DEV) for _ in range(2)]
    mask = (torch.rand(n, generator=gen) < 0.4).to(DEV)
    m8 = mask.to(torch.uint8)
    g = 7.5
    for t, t_next in ((600.0, 590.0), (300.0, 290.0), (100.0, 90.0)):
        at, atn = sch.alpha_at(t), sch.alpha_at(t_next)
        for regime, (f, e) in (("a", near), ("b", far)):
            eF, eE = eng.lincomb([(g, f), (1.0 - g, nn)]), eng.lincomb([(g, e), (1.0 - g, nn)])
            xF, xE = eng.sched_step(x, eF, at, atn)[0], eng.sched_step(x, eE, at, atn)[0]
            want = torch.where(mask[None], xE, xF)
            got = eng.cfg_masked_step(x, f, e, nn, g, at, atn, m8)
            off, on = eng.cfg_masked_step(x, f, e, nn, g, at, atn, torch.zeros_like(m8)), eng.cfg_masked_step(x, f, e, nn, g, at, atn, torch.ones_like(m8))
            bound = _step_ulp_bound(x, f, e, nn, g, at, atn)
            print(f"[{B},{n}] t {t} ({regime}): max |diff| {float((got - want).abs().max()):.3e}, max guided noise {float(eF.abs().max()):.1f}, "
                  f"largest share of the ulp bound {float(((got - want).abs() / bound).max()):.3f}")
            if regime == "a":
                assert float(torch.maximum(eF.abs(), eE.abs()).max()) < 8.0
                for a_, b_ in ((got, want), (off, xF), (on, xE)):
                    assert torch.allclose(a_, b_, rtol=1e-5, atol=1e-6)
            for a_, b_ in ((got, want), (off, xF), (on, xE)):
                assert bool(((a_ - b_).abs() <= bound).all())
            assert float((xF - xE).abs().mean()) > 1e-2                  # the two halves differ: the select is visible
            assert torch.equal(torch.where(mask[None], on, off), got)    # all-False = the `for` half, all-True = the `edit` half
            xa = x.clone()
            assert eng.cfg_masked_step(xa, f, e, nn, g, at, atn, m8, out=xa) is xa and torch.equal(xa, got)      # out aliasing x
            # a select, not a product with 0 / 1: a non-finite value of the half that is not taken does not reach the frame
            e_bad = torch.where(mask[None], e, torch.full_like(e, float("nan")))
            f_bad = torch.where(mask[None], torch.full_like(f, float("inf")), f)
            assert torch.equal(eng.cfg_masked_step(x, f_bad, e_bad, nn, g, at, atn, m8), got)
    f, e = near
    with pytest.raises(ValueError):
        eng.cfg_masked_step(x, f, e, nn, g, 0.3, 0.35, m8[:-1].contiguous())
    with pytest.raises(ValueError):
        eng.cfg_masked_step(x, f, e, nn, g, 0.3, 0.35, mask)          # bool, not uint8


# ---------------------------------------------------------------------------------------------------------------------
# 4. mask_diffedit against the reference's fixture
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_mask_diffedit_vs_reference_golden(prec, golden, tmp_path):
    """The mask equals the reference's on every pixel whose reference ||z| - 0.5| is at least 1e-2 (about 0.25 % of the map's
    range, tens of times the error 4 TOL[prec] allows a guided noise prediction, of which the map is an average); the excluded
    pixels are at most 3 % of the map (the reference alone excludes 1.9 % for these inputs); the fraction True lies in
    [0.2, 0.8]; the map's rel-L2 against the reference's is below 4 TOL[prec], the bound the project grants
    eps_modes['(for-edit)'], the same quantity before averaging (measured values: DESIGN.md 7.3)."""
    import diffedit_oracle as do
    g = _both(golden)
    ed = _edit(g, tmp_path, prec)
    F, E, N = g["for_e"], g["edit_e"], g["null_e"]
    mask = ed.mask_diffedit(g["x0"].to(DEV), F, E, N, noise=g["noise"].to(DEV))
    assert mask.dtype == torch.bool and tuple(mask.shape) == (1, 32, 32) and mask.is_cuda
    band = do.band_distance(g["m"])
    keep = band >= BAND
    excluded = 1.0 - float(keep.float().mean())
    flips = int((mask.cpu() != g["mask"]).sum())
    r = rel(ed.diffedit_map, g["m"])
    print(f"[{prec}] map rel-L2 {r:.3e} (bound {4 * TOL[prec]:.1e}), band pixels {100 * excluded:.2f} %, flipped {flips}, "
          f"True {100 * float(mask.float().mean()):.1f} %")
    assert excluded <= 0.03
    assert torch.equal(mask.cpu()[keep], g["mask"][keep])
    assert 0.2 <= float(mask.float().mean()) <= 0.8
    assert r < 4 * TOL[prec]
    assert os.path.exists(os.path.join(ed.result_folder, "mask", "mask_diffedit_t_500.png"))
    assert not os.path.exists(os.path.join(ed.result_folder, "mask", "mask.pt"))
    # the draw of its own: a mask of the same kind, and the rule switch reaches the kernel
    torch.manual_seed(3)
    own = ed.mask_diffedit(g["x0"].to(DEV), F, E, N)
    assert 0.2 <= float(own.float().mean()) <= 0.8
    os.environ["LOCO_DIFFEDIT_RULE"] = "intended"
    try:
        intended = ed.mask_diffedit(g["x0"].to(DEV), F, E, N, noise=g["noise"].to(DEV))
    finally:
        del os.environ["LOCO_DIFFEDIT_RULE"]
    want = do.diffedit_threshold(g["m"], "intended")
    sure = do.band_distance(g["m"], "intended") >= BAND
    assert torch.equal(intended.cpu()[sure], want[sure]) and not torch.equal(intended, mask)
    # identical prompts: no mask can be derived
    with pytest.raises(ValueError, match="constant map"):
        ed.mask_diffedit(g["x0"].to(DEV), F, F, N, noise=g["noise"].to(DEV))


# ---------------------------------------------------------------------------------------------------------------------
# 5. MaskedDDPMforwardsteps against the reference's fixture
def _count_forwards(ed):
    calls = {"n": 0}
    for eng in set(ed.branches.values()):
        real = eng.unet_forward

        def counted(*a, _real=real, **k):
            calls["n"] += 1
            return _real(*a, **k)
        eng.unet_forward = counted
    return calls


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_masked_sampler_vs_reference_golden(prec, golden, tmp_path):
    """B = 1 and B = 2 under a rectangular [1, H, W] mask and under the DiffEdit mask: share of pixels more than one grey level
    off below 0.002 (f32) / 0.05 (bf16x3), the bounds test_tloco_sampler_vs_reference_golden uses for the same 60 steps of the
    same network.  The final images of this stand-in are almost everywhere 0 or 255 under guidance 7.5, so the state after ten
    steps is compared in floating point too: PSNR over the reference's range above 60 dB (f32) / 35 dB (bf16x3), the bounds the
    same test uses for the 39 steps before the edit step."""
    g = _both(golden)
    ed = _edit(g, tmp_path, prec)
    F, E, N = g["for_e"], g["edit_e"], g["null_e"]
    bound = 0.002 if prec == "f32" else 0.05
    steps = len(ed.scheduler.timesteps) - ed.edit_t_idx
    for mname, mk in (("rect", g["rect"]), ("diffedit", g["mask"])):
        for B in (1, 2):
            x_in = g["dec_in"][:B].to(DEV)
            keep = x_in.clone()
            ed.EXP_NAME = f"masked_{mname}_{B}"
            calls = _count_forwards(ed)
            img = ed.MaskedDDPMforwardsteps(x_in, ed.edit_t_idx, -1, F, E, N, mask=mk)
            assert calls["n"] == 3 * steps                                 # for, edit, null: once each per step
            assert torch.equal(x_in, keep)                                 # the caller's tensor is not the work buffer
            ref = g["masked"][f"{mname}_b{B}"]
            assert img.dtype == torch.uint8 and tuple(img.shape) == tuple(ref.shape) == (B, 32, 32, 3)
            share = float(((img.cpu().int() - ref.int()).abs() > 1).float().mean())
            print(f"[{prec}] masked sampler {mname} B={B}: share of pixels > 1 grey level off {share:.5f} (bound {bound})")
            assert share < bound
            assert os.path.exists(os.path.join(ed.result_folder, f"masked_{mname}_{B}_stage1.png"))
        end = ed.edit_t_idx + g["mid_steps"]
        xm, t, i = ed.MaskedDDPMforwardsteps(g["dec_in"].to(DEV), ed.edit_t_idx, end, F, E, N, mask=mk)
        ref = g["masked_mid"][mname]
        assert i == end and float(t) == float(ed.scheduler.timesteps[end])
        mse = ((xm.cpu().double() - ref.double()) ** 2).mean().item()
        peak = float(ref.max() - ref.min())
        psnr = 10 * math.log10(peak * peak / max(mse, 1e-30))
        print(f"[{prec}] masked sampler {mname}, {g['mid_steps']} steps: PSNR {psnr:.1f} dB")
        assert psnr > (60 if prec == "f32" else 35)


def test_masked_sampler_properties(golden, tmp_path):
    """An all-False mask reproduces DDPMforwardsteps(mode='null+(for-null)'), an all-True mask mode='null+(edit-null)', to within
    one grey level everywhere; mask shapes [H, W], [1, H, W], [C, H, W]; one step from a unit-scale x_t equals the select of
    the two plain samplers' steps (in floating point, where the two prompts are far apart); guidance_scale <= 1: one
    evaluation per step and the plain update, as the reference's guidance then ignores the mode (edit.py:1315-1317)."""
    g = _both(golden)
    ed = _edit(g, tmp_path, "f32")
    F, E, N = g["for_e"], g["edit_e"], g["null_e"]
    x_in = g["dec_in"].to(DEV)
    s = ed.edit_t_idx
    for value, mode in ((False, "null+(for-null)"), (True, "null+(edit-null)")):
        ed.EXP_NAME = f"prop_{value}"
        img = ed.MaskedDDPMforwardsteps(x_in, s, -1, F, E, N, mask=torch.full((32, 32), value))
        ref = ed.DDPMforwardsteps(x_in, s, -1, F, E, N, mode=mode)
        assert int((img.int() - ref.int()).abs().max()) <= 1
    # one step from x ~ N(0, I): the float state is where(mask, step under edit, step under for)
    x1 = g["x"].to(DEV)
    xf = ed.DDPMforwardsteps(x1, s, s + 1, F, E, N, mode="null+(for-null)")[0]
    xe = ed.DDPMforwardsteps(x1, s, s + 1, F, E, N, mode="null+(edit-null)")[0]
    assert rel(xe, xf) > 1e-2
    rect3 = g["mask"]                                           # tloco_tiny's [C, H, W] rectangle
    want = torch.where(rect3.to(DEV)[None], xe, xf)
    t = ed.scheduler.timesteps[s]
    bound = _step_ulp_bound(x1, *ed._branch_eps(x1, t, ("for", "edit", "null")), ed.guidance_scale, ed.scheduler.alpha_at(t),
                            ed.scheduler.alpha_at(ed.scheduler.timesteps_next[s]))
    for mk in (rect3, rect3[:1], rect3[0]):
        got, t_, i = ed.MaskedDDPMforwardsteps(x1, s, s + 1, F, E, N, mask=mk)
        print(f"one step: max |diff| {float((got - want).abs().max()):.3e}, largest share of the ulp bound {float(((got - want).abs() / bound).max()):.3f}")
        assert i == s + 1 and bool(((got - want).abs() <= bound).all())
    with pytest.raises(ValueError):
        ed.MaskedDDPMforwardsteps(x1, s, s + 1, F, E, N, mask=torch.zeros(2, 32, 32, dtype=torch.bool))
    with pytest.raises(ValueError):
        ed.MaskedDDPMforwardsteps(x1, s, s + 1, F, E, N, mask=torch.zeros(16, 16, dtype=torch.bool))
    # guidance_scale <= 1
    ed1 = _edit(g, tmp_path, "f32", guidance_scale=1.0)
    calls = _count_forwards(ed1)
    ed1.EXP_NAME = "nocfg_masked"
    img = ed1.MaskedDDPMforwardsteps(x_in, 96, -1, F, E, N, mask=g["rect"])
    n_steps = len(ed1.scheduler.timesteps) - 96
    assert calls["n"] == n_steps
    ed1.EXP_NAME = "nocfg_plain"
    assert torch.equal(img, ed1.DDPMforwardsteps(x_in, 96, -1, F, E, N, mode="null+(for-null)"))


# ---------------------------------------------------------------------------------------------------------------------
# 6. drivers end to end, no mask.pt anywhere
def _no_mask_pt(folder):
    return not any("mask.pt" in fs for _, _, fs in os.walk(folder))


def test_diffedit_drivers_end_to_end_without_mask_pt(golden, tmp_path):
    g = _both(golden)
    run = dict(op="mid", block_idx=0, vis_num=2, mask_index=0, vis_num_pc=1, pca_rank=1)
    # null-space projection under the DiffEdit mask (the reference raises IndexError here: its mask stays [1, H, W])
    ed = _edit(g, tmp_path / "a", "bf16x3", mask_type="diffedit", ablation="null-space-proj")
    torch.manual_seed(5)
    x0 = ed.run_edit_null_space_projection_xt_semantic(null_space_projection=True, pca_rank_null=2, jacobian=True, **run)
    assert x0.dtype == torch.uint8 and tuple(x0.shape) == (5, 32, 32, 3)
    assert os.path.exists(os.path.join(ed.result_folder, "original_stage1.png"))
    assert os.path.exists(os.path.join(ed.result_folder, "mask", "mask_diffedit_t_500.png"))
    sdir = os.path.join(ed.result_folder, "basis")
    pcs = [f for f in os.listdir(sdir) if f.startswith("Semantic_Edit_xt-") and f.endswith("-pc_000-vT.pt")]
    assert len(pcs) == 1
    v = torch.load(os.path.join(sdir, pcs[0]))
    assert tuple(v.shape) == (1, TINY_ADM.n) and abs(float(v.norm()) - 1.0) < 1e-4
    # the diffedit ablation: the masked sampler from the edit step
    ed2 = _edit(g, tmp_path / "b", "bf16x3", mask_type="diffedit", ablation="diffedit")
    torch.manual_seed(5)
    x2 = ed2.run_edit_null_space_projection_xt_semantic(**run)
    assert x2.dtype == torch.uint8 and tuple(x2.shape) == (1, 32, 32, 3)
    assert os.path.exists(os.path.join(ed2.result_folder, "diffedit-edit_prompt-a dog-mask_type-diffedit-select_mask0_stage1.png"))
    assert os.path.exists(os.path.join(ed2.result_folder, "mask", "mask_diffedit_t_500.png"))
    # sampling_mode: returns after the mask
    ed3 = _edit(g, tmp_path / "c", "bf16x3", mask_type="diffedit", ablation="diffedit", sampling_mode=True)
    torch.manual_seed(5)
    assert ed3.run_edit_null_space_projection_xt_semantic(**run) is None
    assert os.path.exists(os.path.join(ed3.result_folder, "mask", "mask_diffedit_t_500.png"))
    assert os.listdir(ed3.result_folder).count("original_stage1.png") == 1 and not os.path.exists(os.path.join(ed3.result_folder, "basis"))
    for sub in ("a", "b", "c"):
        assert _no_mask_pt(tmp_path / sub)
    # the diffedit ablation under a SAM mask from mask.pt
    ed4 = _edit(g, tmp_path / "d", "bf16x3", mask_type="SAM", ablation="diffedit")
    masks = torch.zeros(2, 1, 32, 32, dtype=torch.bool)
    masks[1, 0, 12:20, 8:18] = True
    os.makedirs(os.path.join(ed4.result_folder, "mask"))
    torch.save(masks, os.path.join(ed4.result_folder, "mask", "mask.pt"))
    torch.manual_seed(5)
    x4 = ed4.run_edit_null_space_projection_xt_semantic(**dict(run, mask_index=1))
    assert tuple(x4.shape) == (1, 32, 32, 3)
    assert os.path.exists(os.path.join(ed4.result_folder, "diffedit-edit_prompt-a dog-mask_type-SAM-select_mask1_stage1.png"))
    assert not os.path.exists(os.path.join(ed4.result_folder, "mask", "mask_diffedit_t_500.png"))


# ---------------------------------------------------------------------------------------------------------------------
# 7. CLI
@pytest.mark.parametrize("ablation", ["diffedit", "null-space-proj"])
def test_cli_if_script_with_diffedit_mask_on_the_standin(ablation, tmp_path, monkeypatch):
    """`python -m loco_edit_amd.main` with the argument list of scripts/main_T2I_DeepFloydIF_null_space_projection.sh
    (tests/golden/script_args.json), `--mask_type diffedit` and either ablation, in an empty result folder: two prompts'
    embeddings (seeded) and a seed in, PNGs out."""
    import json
    from loco_edit_amd.main import main
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    argv = json.load(open(os.path.join(root, "tests", "golden", "script_args.json")))["main_T2I_DeepFloydIF_null_space_projection.sh"]
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("LOCO_PRECISION", "bf16x3")
    x0 = main(argv + ["--device", DEV, "--unet_preset", "tiny_adm", "--synthetic_weights", "0", "--mask_type", "diffedit",
                      "--ablation_method", ablation])
    rdir = tmp_path / "runs" / "DeepFloyd-IF-Random-with_prompt" / "results" / "for_prompt_A photo of a man_cfg7.5_seed2628577915_standin"
    frames = 1 if ablation == "diffedit" else 3                       # vis_num 1: frames -S, 0, +S
    assert x0.dtype == torch.uint8 and tuple(x0.shape) == (frames, 32, 32, 3)
    assert os.path.exists(rdir / "original_stage1.png") and os.path.exists(rdir / "mask" / "mask_diffedit_t_500.png")
    if ablation == "diffedit":
        assert os.path.exists(rdir / "diffedit-edit_prompt-A photo of a man wearing glasses-mask_type-diffedit-select_mask12_stage1.png")
    else:
        assert len([f for f in os.listdir(rdir / "basis") if f.endswith("-pc_000-vT.pt")]) == 1
    assert _no_mask_pt(tmp_path)


# ---------------------------------------------------------------------------------------------------------------------
# 8. at size: the IF stage-I architecture, 64 x 64
def test_diffedit_at_size_if_stage1(tmp_path):
    """IF_I_M_UNET (64 x 64, synthetic weights): mask_diffedit with ten draws in two chunks (max_batch 8) gives a finite map and
    a mask that is neither empty nor full; the last steps of the masked sampler give an image, three steps a finite state."""
    import loco_edit_amd.config as C
    from loco_edit_amd.tloco import EditDeepFloydIF
    cfg = C.IF_I_M_UNET
    os.environ.pop("WORLD_SIZE", None)
    gen = torch.Generator().manual_seed(31)
    pe = {k: torch.randn(1, cfg.context_len, cfg.encoder_dim, generator=gen) for k in ("for", "edit", "null")}
    args = Namespace(device=torch.device(DEV), dtype=torch.float32, seed=1, unet_config=cfg, synthetic_weights=0, ckpt_path="",
                     max_batch=8, precision="bf16x3", dataset_name="Random", for_steps=100, use_yh_custom_scheduler=True,
                     guidance_scale=7.5, guidance_scale_edit=4.0, prompt_emb=pe, for_prompt="a", edit_prompt="b", edit_t=0.6,
                     sampling_mode=False, tilda_v_score_type="null+(for-null)+(edit-null)", ablation_method="diffedit",
                     mask_type="diffedit", vT_path="", x_space_guidance_edit_step=1.0, x_space_guidance_scale=0.5,
                     x_space_guidance_num_step=16, result_folder=str(tmp_path))
    ed = EditDeepFloydIF(args)
    F, E, N = pe["for"], pe["edit"], pe["null"]
    x0 = torch.randn(1, 3, 64, 64, generator=gen).clamp(-1, 1).to(DEV)
    calls = _count_forwards(ed)
    torch.manual_seed(9)
    mask = ed.mask_diffedit(x0, F, E, N)
    assert calls["n"] == 4                                          # two branches, ten draws in chunks of 8 + 2
    assert tuple(mask.shape) == (1, 64, 64) and bool(torch.isfinite(ed.diffedit_map).all())
    frac = float(mask.float().mean())
    print(f"IF_I_M_UNET 64x64: DiffEdit mask {100 * frac:.1f} % True, map in [{float(ed.diffedit_map.min()):.3f}, {float(ed.diffedit_map.max()):.3f}]")
    assert 0.0 < frac < 1.0
    xt = torch.randn(1, 3, 64, 64, generator=gen).to(DEV)
    ed.EXP_NAME = "at_size"
    img = ed.MaskedDDPMforwardsteps(xt, 97, -1, F, E, N, mask=mask)
    assert img.dtype == torch.uint8 and tuple(img.shape) == (1, 64, 64, 3)
    assert os.path.exists(os.path.join(ed.result_folder, "at_size_stage1.png"))
    xs, t, i = ed.MaskedDDPMforwardsteps(xt, 95, 98, F, E, N, mask=mask)          # three steps, the state in floating point
    assert i == 98 and bool(torch.isfinite(xs).all())
