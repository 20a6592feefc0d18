"""GPU tests of the latent-consistency path (loco_edit_amd.tloco_lcm): the `timestep_cond` input of the engine, the fused
scheduler step (csrc/lcm.hip), the single-branch Jacobian operator of the decoded consistency function, the class
`EditLatentConsistency` and the two shipped LCM argument lists -- against tests/lcm_restatement.py (the published formulas on
the oracle's networks).  `TINY_LCM` (16 x 16 latents, ch 32, time_cond_proj_dim 10) with `TINY_DECODER`; bounds as in
test_gpu_latent.py."""
import json
import os
import sys
from argparse import Namespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loco_edit_amd  # noqa: E402,F401
import loco_oracle as orc  # noqa: E402
import lcm_restatement as R  # noqa: E402
from loco_edit_amd.config import TINY_DECODER, TINY_LCM, TINY_LDM, synth_params  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {"f32": 2e-5, "bf16x3": 2e-4}
ADJ = {"f32": 1e-4, "bf16x3": 5e-4}
W = 6.5                      # guidance_scale 7.5 - 1 (edit.py:118)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def cosrow(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a * b).sum(dim=1) / (a.norm(dim=1) * b.norm(dim=1))).abs()


@pytest.fixture(scope="module")
def nets():
    """Parameters, inputs and the CPU references every test shares (computed once, never modified)."""
    cfg = TINY_LCM
    params, dparams = synth_params(cfg, 0), synth_params(TINY_DECODER, 0)
    p, dp = orc.to_torch(params), orc.to_torch(dparams)
    g = torch.Generator().manual_seed(47)
    z = torch.randn(1, 4, cfg.resolution, cfg.resolution, generator=g)
    ctx = torch.randn(cfg.context_len, cfg.context_dim, generator=g)
    ctx2 = torch.randn(cfg.context_len, cfg.context_dim, generator=g)
    return dict(cfg=cfg, params=params, dparams=dparams, p=p, dp=dp, z=z, ctx=ctx, ctx2=ctx2,
                V=torch.randn(3, cfg.n, generator=g), Uc=torch.randn(3, cfg.n, generator=g),
                Ui=torch.randn(3, TINY_DECODER.n_out, generator=g))


# ------------------------------------------------------------------ 1. timestep_cond on the engine
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_timestep_cond_forward_jvp_vjp_vs_restatement(prec, nets):
    """Forward on a batch of 3, J V and U^T J (k = 3) of eps with the guidance-scale embedding set, against autodiff of the
    restatement (cond folded into time_embed.0.bias).  The cond matters: on the CPU alone, setting it moves eps by 0.137 rel-L2
    at w = 6.5 with the synthesiser's N(0, 1/P) cond_proj (printed; the bar is 100 x TOL = 2e-2), so a missing add cannot hide
    under the 2e-5 / 2e-4 bounds.  Clearing restores the earlier output bit for bit; a fork keeps its own embedding; an
    architecture without the input refuses the call."""
    from loco_edit_amd.hip import LocoEngine
    cfg, p, z, ctx = nets["cfg"], nets["p"], nets["z"], nets["ctx"]
    tol = TOL[prec]
    t = torch.tensor(499.0)
    w_emb = R.guidance_embedding(W, cfg.time_cond_proj_dim)
    pc = R.fold_cond(p, w_emb)
    f = lambda z_: orc.unet_forward_adm(pc, cfg, z_, t, context=ctx)
    zb = torch.cat([z, 0.5 * z.flip(-1), z + 0.2], dim=0)
    with torch.no_grad():
        ref, ref0 = f(zb), orc.unet_forward_adm(p, cfg, zb, t, context=ctx)
    moved = rel(ref, ref0)
    print(f"restatement alone: the cond moves eps by {moved:.3e} rel-L2 (bar {100 * TOL['bf16x3']:.0e})")
    assert moved >= 100 * TOL["bf16x3"]
    eng = LocoEngine(cfg, max_batch=4, device=torch.device(DEV))
    eng.load_state_dict(nets["params"])
    eng.set_precision(prec)
    eng.set_context(ctx.to(DEV).contiguous())
    zd = zb.to(DEV)
    out0 = eng.unet_forward(zd, float(t))
    e0 = rel(out0, ref0)
    eng.set_time_cond(w_emb.to(DEV))
    out1 = eng.unet_forward(zd, float(t))
    e1 = rel(out1, ref)
    print(f"[{prec}] forward rel err without cond {e0:.2e}, with cond {e1:.2e}")
    assert e0 < tol and e1 < tol
    # tangent / cotangent passes with the cond set
    JV = torch.stack([torch.func.jvp(f, (z,), (v.view_as(z),))[1].reshape(-1) for v in nets["V"]])
    eng.pmp_primal(z.to(DEV), float(t), 0.5, None, use_et=True)
    U = eng.pmp_jvp(nets["V"].to(DEV))
    zz = z.clone().requires_grad_(True)
    o = f(zz).reshape(-1)
    Aref = torch.stack([torch.autograd.grad((o * u).sum(), zz, retain_graph=True)[0].reshape(-1) for u in nets["Uc"]])
    A = eng.pmp_vjp(nets["Uc"].to(DEV))
    print(f"[{prec}] J V rel err {rel(U, JV):.2e}, U^T J rel err {rel(A, Aref):.2e}")
    assert rel(U, JV) < 5 * tol and rel(A, Aref) < 5 * tol
    lhs, rhs = (U.double().cpu() * nets["Uc"].double()).sum(), (nets["V"].double() * A.double().cpu()).sum()
    assert abs(lhs - rhs) / abs(lhs) < ADJ[prec]
    # a fork with another w: each context keeps its own result
    w2 = R.guidance_embedding(2.0, cfg.time_cond_proj_dim)
    child = eng.fork()
    child.set_context(ctx.to(DEV).contiguous())
    out_c0 = child.unet_forward(zd, float(t))
    assert torch.equal(out_c0, out0)                  # a fork starts without an embedding
    child.set_time_cond(w2.to(DEV))
    out_c = child.unet_forward(zd, float(t))
    with torch.no_grad():
        ref_c = orc.unet_forward_adm(R.fold_cond(p, w2), cfg, zb, t, context=ctx)
    assert rel(out_c, ref_c) < tol and rel(ref_c, ref) > 100 * tol
    assert torch.equal(eng.unet_forward(zd, float(t)), out1)
    # clearing: bit for bit the output before any cond was set
    eng.set_time_cond(None)
    assert torch.equal(eng.unet_forward(zd, float(t)), out0)
    with pytest.raises(RuntimeError, match="pmp_primal"):
        eng.pmp_jvp(nets["V"].to(DEV))                 # the call invalidated the cached primal
    assert torch.equal(child.unet_forward(zd, float(t)), out_c)
    with pytest.raises(ValueError):
        eng.set_time_cond(torch.zeros(cfg.time_cond_proj_dim + 1, device=DEV))


def test_set_time_cond_is_refused_without_the_input():
    from loco_edit_amd.hip import LocoEngine
    eng = LocoEngine(TINY_LDM, max_batch=1, device=torch.device(DEV))
    with pytest.raises(RuntimeError, match="time_cond_proj_dim"):
        eng.set_time_cond(torch.zeros(10, device=DEV))
    with pytest.raises(RuntimeError, match="time_cond_proj_dim"):
        eng.set_time_cond(None)


# ------------------------------------------------------------------ 2. the scheduler step
@pytest.fixture(scope="module")
def step_engine():
    from loco_edit_amd.hip import LocoEngine
    return LocoEngine(TINY_LDM, max_batch=1, device=torch.device(DEV))


@pytest.mark.parametrize("scaling", [10.0, 0.001])
@pytest.mark.parametrize("shape", [(3, 4, 16, 16), (1023,)])
def test_lcm_step_vs_float64(shape, scaling, step_engine):
    """e = rel-L2 error of the kernel against float64, e_ref = that of torch's own fp32 composition of the same formula;
    e <= 4 e_ref (the project's bound for fused elementwise kernels).  1023 elements: the one-element path."""
    eng = step_engine
    g = torch.Generator().manual_seed(5)
    x, eps, nz = (torch.randn(*shape, generator=g) for _ in range(3))
    ab = R.alphas_cumprod()
    at, at_prev = float(ab[499]), float(ab[259])
    c64 = R.scalings(499, scaling)
    c_skip, c_out = float(torch.tensor(c64[0], dtype=torch.float32)), float(torch.tensor(c64[1], dtype=torch.float32))
    xd, ed, nd = x.to(DEV), eps.to(DEV), nz.to(DEV)
    for noise, noise_d in ((nz, nd), (None, None)):
        p64, d64 = R.lcm_step(x.double(), eps.double(), at, at_prev, c_skip, c_out, None if noise is None else noise.double())
        p32, d32 = R.lcm_step(x, eps, at, at_prev, c_skip, c_out, noise)
        prev, den = eng.lcm_step(xd, ed, at, at_prev, c_skip, c_out, noise_d)
        for name, got, r32, r64 in (("prev", prev, p32, p64), ("denoised", den, d32, d64)):
            e, e_ref = rel(got, r64), rel(r32, r64)
            print(f"{shape} scaling {scaling} noise {noise is not None} {name}: e {e:.3e}, e_ref {e_ref:.3e}")
            assert e <= 4 * e_ref
        if noise is None:
            assert torch.equal(prev, den)
        # only `denoised` requested; then x_prev aliasing x
        none, den_only = eng.lcm_step(xd, ed, at, at_prev, c_skip, c_out, noise_d, want_prev=False)
        assert none is None and torch.equal(den_only, den)
        xa = xd.clone()
        pa, da = eng.lcm_step(xa, ed, at, at_prev, c_skip, c_out, noise_d, want_denoised=False, out=xa)
        assert da is None and pa is xa and torch.equal(xa, prev)
    # the boundary condition at t = 0: (c_skip, c_out) = (1, 0) returns x bit for bit
    _, den = eng.lcm_step(xd, ed, at, at_prev, 1.0, 0.0, nd)
    assert torch.equal(den, xd)
    with pytest.raises(ValueError):
        eng.lcm_step(xd, ed[..., :-1].contiguous(), at, at_prev, c_skip, c_out)


# ------------------------------------------------------------------ 3. the operator
@pytest.mark.parametrize("prec,scaling", [("f32", 0.001), ("bf16x3", 0.001), ("f32", 10.0)])
def test_lcm_operator_vs_autodiff(prec, scaling, nets):
    """J V, U^T J with an image mask and adjointness of `LatentLCMJacobianOperator` against autodiff of the restated x0_hat.
    timestep_scaling 0.001 makes (c_skip, c_out) = (0.501, 0.706) at t = 499: at the default scaling c_skip is 1e-8 and a
    dropped c_skip term would pass unseen."""
    from loco_edit_amd.hip import LocoEngine
    from loco_edit_amd.tloco_lcm import LATENT_SCALE, LatentLCMJacobianOperator, LCMScheduler
    cfg, z, ctx = nets["cfg"], nets["z"], nets["ctx"]
    tol, t = TOL[prec], 499
    rs = R.LCMRestatement(nets["p"], cfg, nets["dp"], TINY_DECODER, W, timestep_scaling=scaling)
    mask = torch.zeros(3, 64, 64, dtype=torch.bool); mask[:, 20:40, 12:44] = True
    eng = LocoEngine(cfg, max_batch=4, device=torch.device(DEV))
    eng.load_state_dict(nets["params"])
    dec = LocoEngine(TINY_DECODER, max_batch=4, device=torch.device(DEV))
    dec.load_state_dict(nets["dparams"])
    for e_ in (eng, dec):
        e_.set_precision(prec)
    eng.set_context(ctx.to(DEV).contiguous())
    eng.set_time_cond(rs.w_emb.to(DEV))
    sched = LCMScheduler(engine=eng, timestep_scaling=scaling)
    sched.set_timesteps(4)
    c_skip, c_out = sched.scalings(t)
    if scaling == 0.001:
        assert (c_skip, c_out) == pytest.approx((0.501, 0.706), abs=1e-3)
    at = sched.alpha_at(t)
    zd = z.to(DEV)
    _, den = eng.lcm_step(zd, eng.unet_forward(zd, float(t)), at, 1.0, c_skip, c_out, None, want_prev=False)
    with torch.no_grad():
        assert rel(den, rs.denoised(z, ctx, t)) < tol
    opj = LatentLCMJacobianOperator(eng, dec, zd, float(t), at, c_skip, c_out, eng.lincomb([(1.0 / LATENT_SCALE, den)]), mask.to(DEV))
    f = lambda z_: rs.x0_hat(z_, ctx, t).reshape(-1)
    m = mask.reshape(1, -1)
    JV = torch.stack([torch.func.jvp(f, (z,), (v.view_as(z),))[1] for v in nets["V"]]) * m
    U = opj.jvp(nets["V"].to(DEV))
    zz = z.clone().requires_grad_(True)
    o = f(zz)
    Aref = torch.stack([torch.autograd.grad((o * (u * m.reshape(-1))).sum(), zz, retain_graph=True)[0].reshape(-1) for u in nets["Ui"]])
    A = opj.vjp(nets["Ui"].to(DEV))
    print(f"[{prec}, scaling {scaling}] operator J V rel err {rel(U, JV):.2e}, U^T J rel err {rel(A, Aref):.2e}")
    assert tuple(U.shape) == (3, dec.n_out) and tuple(A.shape) == (3, eng.n)
    assert rel(U, JV) < 5 * tol and rel(A, Aref) < 5 * tol
    lhs, rhs = (U.double().cpu() * (nets["Ui"].double() * m)).sum(), (nets["V"].double() * A.double().cpu()).sum()
    assert abs(lhs - rhs) / abs(lhs) < ADJ[prec]
    assert opj.gather(U).shape == (3, int(mask.sum()))


# ------------------------------------------------------------------ 4. the class
def _edit_lcm(nets, tmp_path, prec, **kw):
    from loco_edit_amd.tloco_lcm import EditLatentConsistency
    os.environ.pop("WORLD_SIZE", None)
    args = Namespace(device=torch.device(DEV), dtype=torch.float32, seed=1, unet_config=TINY_LCM, vae_config=TINY_DECODER,
                     synthetic_weights=0, ckpt_path="", vae_ckpt_path="", max_batch=8, precision=prec, dataset_name="Random",
                     for_steps=100, use_yh_custom_scheduler=False, guidance_scale=W + 1, guidance_scale_edit=7.5,
                     prompt_emb={"for": nets["ctx"][None], "edit": nets["ctx2"][None], "null": torch.zeros_like(nets["ctx"][None])},
                     for_prompt="a man", edit_prompt="a man wearing glasses", edit_t=1.0, sampling_mode=False,
                     tilda_v_score_type="null+(for-null)+(edit-null)", ablation_method=None, mask_type="SAM", vT_path="",
                     use_sega=False, x_space_guidance_edit_step=1.0, x_space_guidance_scale=0.5, x_space_guidance_num_step=2,
                     num_inference_steps=4, edit_t_idx=2, lcm_timesteps="linspace", result_folder=str(tmp_path))
    for k, v in kw.items():
        setattr(args, k, v)
    return EditLatentConsistency(args)


@pytest.fixture(scope="module")
def class_refs(nets):
    """The restated class pieces at t = 499 (index 2 of the 4-step linspace table), computed once on the CPU."""
    rs = R.LCMRestatement(nets["p"], nets["cfg"], nets["dp"], TINY_DECODER, W)
    g = torch.Generator().manual_seed(9)
    mask = torch.zeros(3, 64, 64, dtype=torch.bool); mask[:, 20:40, 12:44] = True
    v0 = torch.randn(nets["cfg"].n, 2, generator=g)
    noise = torch.randn(4, 2, 4, 16, 16, generator=g)
    zT = torch.randn(2, 4, 16, 16, generator=g)
    z, ctx, ctx2, t = nets["z"], nets["ctx"], nets["ctx2"], 499
    with torch.no_grad():
        x0m = rs.x0_hat(z, ctx, t, mask=mask)
        x0e = rs.x0_hat(z, ctx2, t, flatten=True)
    u, s, vT = rs.pullback(z, ctx, t, 2, v0, 3, mask)
    delta = rs.delta_zt_via_grad(z, ctx, ctx2, t, mask)
    mid = rs.forward_loop(zT, ctx, noise, 0, 2)
    lat, den, img = rs.forward_loop(zT, ctx, noise)
    return dict(rs=rs, mask=mask, v0=v0, noise=noise, zT=zT, x0m=x0m, x0e=x0e, s=s, vT=vT, delta=delta, mid=mid, lat=lat, den=den,
                img=img)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_class_pieces_vs_restatement(prec, nets, class_refs, tmp_path):
    """`get_x0`, `get_delta_zt_via_grad`, `local_encoder_decoder_pullback_zt` (k = 2, 3 iterations, injected v0) at s rtol 1e-3
    and row |cos| > 0.999 (the bound of test_latent_tloco_with_text_cross_attention_vs_restatement); `LCMforwardsteps` over 4
    steps with injected noise against the restated loop: 4 denoiser evaluations, each within TOL and carried through steps
    whose gain is O(1) -- 4 x 5 TOL, the Jacobian-product factor per step."""
    c = class_refs
    ed = _edit_lcm(nets, tmp_path, prec)
    assert sorted(ed.branches) == ["edit", "for"] and ed.scheduler.timesteps.tolist() == [999, 759, 499, 259]
    assert ed.result_folder == os.path.join(str(tmp_path), "for_prompt_a man_cfg7.5_seed1")
    assert ed.DDIMforwardsteps is None and ed.run_DDIMinversion is None and ed.run_edit_null_space_projection_zt_semantic is None
    z, t, mask = nets["z"].to(DEV), ed.scheduler.timesteps[2], c["mask"]
    assert int(t) == 499
    with torch.no_grad():
        assert rel(ed.get_x0(z, "a man", t, 2, mask=mask), c["x0m"]) < 10 * TOL[prec]
        assert rel(ed.get_x0(z, "a man wearing glasses", t, 2, flatten=True), c["x0e"]) < 10 * TOL[prec]
    with pytest.raises(NotImplementedError):
        ed.get_x0(z, "a prompt nobody encoded", t, 2)
    u, s, vT = ed.local_encoder_decoder_pullback_zt(z, t, 2, "a man", pca_rank=2, min_iter=3, max_iter=3, mask=mask,
                                                    v0=c["v0"].to(DEV), verbose=False)
    print(f"[{prec}] s {s.cpu().tolist()} vs {c['s'].tolist()}, row cos {cosrow(vT, c['vT']).tolist()}")
    assert tuple(u.shape) == (int(mask.sum()), 2)
    assert torch.allclose(s.cpu(), c["s"], rtol=1e-3) and cosrow(vT, c["vT"]).min().item() > 0.999
    d = ed.get_delta_zt_via_grad(z, t, 2, "a man", "a man wearing glasses", mask=mask)
    assert tuple(d.shape) == (1, nets["cfg"].n) and abs(float(d.norm()) - 1.0) < 1e-4
    assert cosrow(d, c["delta"]).min().item() > 0.999
    # the sampler: stop at the edit index, then the whole loop
    ed.EXP_NAME = "loop"
    zT, noise = c["zT"].to(DEV), c["noise"].to(DEV)
    lat_mid, t_mid, i_mid = ed.LCMforwardsteps(zT, "a man", t_start_idx=0, t_end_idx=2, noise=noise)
    assert (int(t_mid), i_mid) == (499, 2) == (c["mid"][1], c["mid"][2]) and rel(lat_mid, c["mid"][0]) < 2 * 5 * TOL[prec]
    lat, frames = ed.LCMforwardsteps(zT, "a man", noise=noise)
    print(f"[{prec}] 4-step loop rel err {rel(lat, c['lat']):.2e}")
    assert rel(lat, c["lat"]) < 4 * 5 * TOL[prec]
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (2, 64, 64, 3)
    want = (c["img"] * 255).to(torch.uint8).permute(0, 2, 3, 1)
    # uint8 by truncation: one level either way is inherent; the 1 % allows pixels where the loop's 20 TOL error crosses two
    assert ((frames.cpu().int() - want.int()).abs() <= 1).float().mean().item() >= 0.99
    assert os.path.exists(os.path.join(ed.result_folder, "loop.png"))
    # what is decoded is `denoised`: it differs from the latents on every step but the last
    eps = ed.engine.unet_forward(zT, 999.0)
    prev, den = ed.scheduler.step(eps, 999, zT, noise=noise[0])
    assert rel(prev, den) > 0.1
    prev, den = ed.scheduler.step(eps, 259, zT, noise=noise[3])
    assert torch.equal(prev, den)


def test_driver_semantic_nonsemantic_and_sega(nets, tmp_path):
    """The driver on the class: unit directions, the semantic and the non-semantic direction differ, `use_sega` decodes under the
    edit prompt, `sampling_mode` stops after the sample."""
    ed = _edit_lcm(nets, tmp_path, "bf16x3")
    os.makedirs(os.path.join(ed.result_folder, "mask"))
    masks = torch.zeros(3, 1, 64, 64, dtype=torch.bool); masks[1, 0, 20:40, 12:44] = True
    torch.save(masks, os.path.join(ed.result_folder, "mask", "mask.pt"))
    calls = []
    inner = ed.LCMforwardsteps
    ed.LCMforwardsteps = lambda zt, prompt=None, **kw: (calls.append((prompt, kw.get("t_start_idx", 0), zt.shape[0])), inner(zt, prompt, **kw))[1]
    kw = dict(op="mid", block_idx=0, vis_num=1, mask_index=1, vis_num_pc=1, pca_rank=1, edit_prompt="a man wearing glasses",
              null_space_projection=True, pca_rank_null=2)
    lat, frames = ed.run_edit_null_space_projection_zt(non_semantic=False, **kw)
    v_sem = ed.last_vT.clone()
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (3, 64, 64, 3) and calls[-1] == ("a man", 2, 3)
    assert os.path.exists(os.path.join(ed.result_folder, "original.png"))
    assert os.path.exists(os.path.join(ed.result_folder, "Edit_zt-edit_2T-mid-block_0_pos-edit_prompt-a man wearing glasses_select_mask1"
                                                          "_null_space_projection_True_null_space_rank_2.png"))
    lat, frames = ed.run_edit_null_space_projection_zt(non_semantic=True, **kw)
    v_non = ed.last_vT
    assert tuple(v_sem.shape) == tuple(v_non.shape) == (1, nets["cfg"].n)
    assert abs(float(v_sem.norm()) - 1) < 1e-4 and abs(float(v_non.norm()) - 1) < 1e-4
    assert cosrow(v_sem, v_non).item() < 0.9
    ed.use_sega = True
    lat, frames = ed.run_edit_null_space_projection_zt(non_semantic=False, **kw)
    assert calls[-1] == ("a man wearing glasses", 2, 1) and tuple(frames.shape) == (1, 64, 64, 3)
    assert os.path.exists(os.path.join(ed.result_folder, "sega_2T-mid-block_0_pos-edit_prompt-a man wearing glasses.png"))
    ed.sampling_mode = True
    assert ed.run_edit_null_space_projection_zt(non_semantic=False, **kw) is None


# ------------------------------------------------------------------ 5. the shipped argument lists
@pytest.mark.parametrize("script,extra", [
    ("main_T2I_LCM_null_space_projection.sh", []),
    ("main_T2I_LCM_null_space_projection_nonsemantic.sh", []),                       # as shipped: sampling_mode True
    ("main_T2I_LCM_null_space_projection_nonsemantic.sh", ["--sampling_mode", "False", "--seed", "1308424610"]),
    ("main_T2I_LCM_null_space_projection.sh", ["--use_sega", "True"]),
])
def test_cli_shipped_lcm_scripts_on_the_standins(script, extra, tmp_path, monkeypatch):
    """`python -m loco_edit_amd.main` with the argument lists of scripts/main_T2I_LCM_null_space_projection*.sh
    (tests/golden/script_args.json) plus the timestep rule and the deployment flags that replace what is out of scope
    (architecture presets, synthetic weights; SAM masks come from mask.pt), in the form of
    test_cli_shipped_sd_script_on_the_standins."""
    from loco_edit_amd.main import main
    argv = json.load(open(os.path.join(ROOT, "tests", "golden", "script_args.json")))[script]
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("LOCO_PRECISION", "bf16x3")
    with pytest.raises(NotImplementedError, match="lcm_timesteps"):
        main(argv + ["--device", DEV])                                               # the bare list stays refused
    shipped_sampling = "nonsemantic" in script and not extra
    seed = "1308424610"
    if shipped_sampling:                 # --seed 0 draws one: fix the draw so the folder is known
        monkeypatch.setattr(torch, "randint", lambda *a, **k: torch.tensor(int(seed)))
    rdir = tmp_path / "runs" / "LCM-Random-with_prompt" / "results" / f"for_prompt_A photo of a man_cfg7.5_seed{seed}"
    os.makedirs(rdir / "mask")
    masks = torch.zeros(6, 1, 64, 64, dtype=torch.bool)
    masks[2, 0, 20:40, 12:44] = True
    masks[5, 0, 8:30, 30:60] = True
    torch.save(masks, str(rdir / "mask" / "mask.pt"))
    out = main(argv + extra + ["--device", DEV, "--lcm_timesteps", "linspace", "--unet_preset", "tiny_lcm", "--vae_preset", "tiny_decoder",
                               "--synthetic_weights", "0"])
    assert (rdir / "original.png").exists()
    if shipped_sampling:
        assert out is None
        return
    lat, x0 = out
    if "--use_sega" in extra:
        assert x0.dtype == torch.uint8 and tuple(x0.shape) == (1, 64, 64, 3)
        assert (rdir / "sega_2T-mid-block_0_pos-edit_prompt-A photo of a man wearing glasses.png").exists()
        return
    assert x0.dtype == torch.uint8 and tuple(x0.shape) == (3, 64, 64, 3)             # vis_num 1: frames -S, 0, +S
    assert tuple(lat.shape) == (3, 4, 16, 16)
    edit_prompt = argv[argv.index("--edit_prompt") + 1]
    mi = argv[argv.index("--mask_index") + 1]
    assert (rdir / (f"Edit_zt-edit_2T-mid-block_0_pos-edit_prompt-{edit_prompt}_select_mask{mi}_null_space_projection_True"
                    "_null_space_rank_5.png")).exists()
    assert not torch.equal(x0[0], x0[1]) and not torch.equal(x0[1], x0[2])           # the walk moved the sample
