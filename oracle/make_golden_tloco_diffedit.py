"""Generate tests/golden/tloco_diffedit.pt by running the REFERENCE's ``EditDeepFloydIF.mask_diffedit`` (edit.py:1395-1407)
and ``MaskedDDPMforwardsteps`` (:1486-1563) on the stand-in conditional denoiser of oracle/make_golden_tloco.py, and pin
oracle/diffedit_oracle.py against them.  The reference object is built the way ``make_golden_tloco.main`` builds it (same
``TINY_ADM`` stand-in, weights seed 0, cond_dim 16, guidance 7.5 / 4.0); prompt states, x_T and x_t at the edit step come
from tests/golden/tloco_tiny.pt, so the two fixtures describe one run.  Runs only where the reference is present; the
fixture is data (inputs + expected outputs).

    python oracle/make_golden_tloco_diffedit.py
"""
from __future__ import annotations

import math
import os
import sys
import tempfile
import types
from argparse import Namespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
GOLD = os.path.join(ROOT, "tests", "golden")

import make_golden as mg  # noqa: E402
import make_golden_tloco as mgt  # noqa: E402


MID_STEPS = 10


def ref_object(redit, cfg, tiny, tmpdir):
    """The reference's EditDeepFloydIF without its diffusers / T5 / SAM constructor work, and the restatement next to it."""
    from utils.utils import betas_for_alpha_bar, get_deepfloyd_if_scheduler
    import tloco_oracle as tl
    import loco_oracle as orc
    from loco_edit_amd.config import synth_params
    from loco_edit_amd.tloco import cond_params
    D = tiny["cond_dim"]
    params = synth_params(cfg, seed=tiny["weights_seed"])
    cp = cond_params(cfg, D, seed=tiny["weights_seed"])
    model = mg.ref_model_adm(cfg, params)
    cw, cb = torch.from_numpy(cp["cond_proj.weight"].copy()), torch.from_numpy(cp["cond_proj.bias"].copy())
    ed = object.__new__(redit.EditDeepFloydIF)
    sched = types.SimpleNamespace()
    betas = betas_for_alpha_bar(1000, lambda ts: math.cos((ts + 0.008) / 1.008 * math.pi / 2) ** 2)
    sched.betas = torch.tensor(betas, dtype=torch.float32)
    sched.alphas_cumprod = torch.cumprod(1.0 - sched.betas, dim=0)
    sched.scale_model_input = lambda x, t: x
    sargs = Namespace(use_yh_custom_scheduler=True, device=torch.device("cpu"), dtype=torch.float32)
    ed.scheduler = get_deepfloyd_if_scheduler(sargs, sched)
    ed.unet = mgt.ref_cond_unet(model, cw, cb)
    ed.device, ed.dtype, ed.buffer_device, ed.memory_bound = torch.device("cpu"), torch.float32, "cpu", 50
    ed.for_steps, ed.use_yh_custom_scheduler = 100, True
    ed.guidance_scale, ed.guidance_scale_edit = tiny["guidance_scale"], tiny["guidance_scale_edit"]
    ed.result_folder, ed.EXP_NAME = tmpdir, "golden"
    ed.c_in, ed.image_size = cfg.in_channels, cfg.resolution
    ed.scheduler.set_timesteps(100, device="cpu")
    ed.edit_t = 0.6
    ed.edit_t_idx = (ed.scheduler.timesteps - 0.6 * 1000).abs().argmin()
    assert torch.equal(sched.alphas_cumprod, tiny["alphas_cumprod"]) and int(ed.edit_t_idx) == tiny["edit_t_idx"]
    po = orc.to_torch(params)
    po.update({k: torch.from_numpy(v.copy()) for k, v in cp.items()})
    ot = tl.OracleTLoco(po, cfg, guidance_scale=ed.guidance_scale, guidance_scale_edit=ed.guidance_scale_edit)
    return ed, ot


def ref_mask_diffedit(ed, x0, noise, for_e, edit_e, null_e):
    """ed.mask_diffedit with its ten draws injected and `.cuda()` the identity (edit.py:1396 says torch.tensor(500).cuda())."""
    real_randn, real_cuda = torch.randn, torch.Tensor.cuda

    def fake_randn(*size, **kw):
        if tuple(size) == tuple(noise.shape):
            return noise.clone()
        return real_randn(*size, **kw)
    torch.randn, torch.Tensor.cuda = fake_randn, lambda self, *a, **k: self
    try:
        with torch.no_grad():
            return ed.mask_diffedit(x0, for_e, edit_e, null_e)
    finally:
        torch.randn, torch.Tensor.cuda = real_randn, real_cuda


def main(redit, cfg, out_name):
    import diffedit_oracle as do
    torch.set_num_threads(8)
    tiny = torch.load(os.path.join(GOLD, "tloco_tiny.pt"))
    tmpdir = tempfile.mkdtemp(prefix="loco_golden_diffedit_")
    ed, ot = ref_object(redit, cfg, tiny, tmpdir)
    for_e, edit_e, null_e = tiny["for_e"], tiny["edit_e"], tiny["null_e"]
    R, C = cfg.resolution, cfg.in_channels
    out = {"guidance_scale": ed.guidance_scale, "guidance_scale_edit": ed.guidance_scale_edit, "t": do.T_DIFFEDIT}

    # ---- 1. the mask (edit.py:1395-1407), the ten draws injected
    gx = torch.Generator().manual_seed(11)
    x0 = torch.randn(1, C, R, R, generator=gx).clamp(-1, 1)
    noise = torch.randn(do.N_DRAWS, C, R, R, generator=gx)
    mask = ref_mask_diffedit(ed, x0, noise, for_e, edit_e, null_e)
    assert mask.dtype == torch.bool and tuple(mask.shape) == (1, R, R)
    # the map behind it, through the reference's own guidance on the same x_t
    t = torch.tensor(do.T_DIFFEDIT)
    at = ed.scheduler.alphas_cumprod[do.T_DIFFEDIT]
    xt = at.sqrt() * x0 + (1 - at).sqrt() * noise
    with torch.no_grad():
        e1 = ed._classifer_free_guidance(xt, t, for_e, edit_e, null_e, mode="null+(for-null)", do_classifier_free_guidance=True)
        e2 = ed._classifer_free_guidance(xt, t, for_e, edit_e, null_e, mode="null+(edit-null)", do_classifier_free_guidance=True)
    m = (e1 - e2).mean(dim=0, keepdim=True).mean(dim=1)
    c = m.min() / (m.max() - m.min())
    assert torch.equal(torch.round(m - c).to(torch.bool), mask), "the recorded map does not reproduce the reference's mask"
    omask, om = do.mask_diffedit(ot, x0, noise, for_e, edit_e, null_e)
    mg.check("diffedit/map", om, m, rtol=1e-4, atol=1e-5)
    band = do.band_distance(m)
    flips = omask != mask
    print(f"  mask: {100 * mask.float().mean():.1f} % True ('intended' rule {100 * do.diffedit_threshold(m, 'intended').float().mean():.1f} %), "
          f"m in [{float(m.min()):.3f}, {float(m.max()):.3f}], c = {float(c):.4f}; pixels with ||z| - 0.5| < 1e-3: "
          f"{int((band < 1e-3).sum())}, < 1e-2: {int((band < 1e-2).sum())} of {band.numel()}; restatement flips {int(flips.sum())}")
    assert not bool((flips & (band >= 1e-2)).any()), "restatement's mask differs from the reference's outside the band"
    out.update(x0=x0, noise=noise, mask=mask, m=m, c=float(c))

    # ---- 2. the masked sampler (edit.py:1486-1563) from x_t at the edit step, B = 1 and B = 2, two masks
    xt_e = tiny["xt_edit"]
    xb2 = torch.cat([xt_e, xt_e + 0.25 * tiny["x"]], dim=0)
    rect = mg.rect_mask(cfg, 12 * (R // 32), 20 * (R // 32), 8 * (R // 32), 18 * (R // 32))[:1]        # [1, H, W]
    out.update(dec_in=xb2, rect=rect, masked={})
    for mname, mk in (("rect", rect), ("diffedit", mask)):
        for B, xin in ((1, xt_e), (2, xb2)):
            ed.memory_bound = 50 if B == 1 else 2   # batch 2 with CFG -> chunk(2 // (2 // 2)) (make_golden_tloco.py: the reference's
            #                                         chunking divides by zero for 1 < batch < memory_bound // 2, edit.py:1532)
            with torch.no_grad():
                img = ed.MaskedDDPMforwardsteps(xin.clone(), t_start_idx=ed.edit_t_idx, t_end_idx=-1, for_prompt_emb=for_e,
                                                edit_prompt_emb=edit_e, null_prompt_emb=null_e, mask=mk)
            oimg = do.to_uint8(do.masked_forwardsteps(ot, xin.clone(), ot.edit_t_idx, -1, for_e, edit_e, null_e, mk))
            diff = (oimg.int() - img.int()).abs()
            print(f"  oracle vs reference [masked sampler {mname} B={B}] max |diff| {int(diff.max())}, differing {int((diff > 0).sum())}")
            assert img.dtype == torch.uint8 and tuple(img.shape) == (B, R, R, C) and int(diff.max()) <= 1
            out["masked"][f"{mname}_b{B}"] = img
    # ---- 3. the same sampler stopped after MID_STEPS steps: x_t in floating point.  Under guidance 7.5 the stand-in's final images
    #         are almost everywhere 0 or 255, which says little about the blend; the intermediate state says it all
    ed.memory_bound = 2
    out["mid_steps"], out["masked_mid"] = MID_STEPS, {}
    for mname, mk in (("rect", rect), ("diffedit", mask)):
        with torch.no_grad():
            xm, tm, im = ed.MaskedDDPMforwardsteps(xb2.clone(), t_start_idx=ed.edit_t_idx, t_end_idx=int(ed.edit_t_idx) + MID_STEPS,
                                                   for_prompt_emb=for_e, edit_prompt_emb=edit_e, null_prompt_emb=null_e, mask=mk)
        oxm, otm, oim = do.masked_forwardsteps(ot, xb2.clone(), ot.edit_t_idx, ot.edit_t_idx + MID_STEPS, for_e, edit_e, null_e, mk)
        assert int(im) == oim == int(ed.edit_t_idx) + MID_STEPS and float(tm) == float(otm)
        mg.check(f"diffedit/masked sampler {mname}, {MID_STEPS} steps", oxm, xm, rtol=1e-3, atol=1e-4)
        out["masked_mid"][mname] = xm
    a, b = out["masked_mid"]["rect"], out["masked_mid"]["diffedit"]
    print(f"  x_t after {MID_STEPS} steps: the two masks differ by rel-L2 {float((a - b).norm() / b.norm()):.3f}")
    torch.save(out, os.path.join(GOLD, out_name))
    print("done ->", os.path.join(GOLD, out_name))


if __name__ == "__main__":
    redit_ = mg.import_reference()[0]
    from loco_edit_amd.config import TINY_ADM
    main(redit_, TINY_ADM, "tloco_diffedit.pt")
