"""Reference of the prompt-state gradient (LocoEngine.pmp_vjp(U, context_grad=True)) and of null-text inversion
(loco_edit_amd.null_text.NullTextInversion): autograd of the restatement oracle/loco_oracle.unet_forward_adm with respect
to `context`, run in float64 (the reference) and in fp32 on the CPU (the yardstick: what the same arithmetic costs in the
engine's number format).  A helper of tests/test_gpu_context_grad.py and tests/test_gpu_null_text.py, no test itself."""
import dataclasses
import functools
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import loco_edit_amd  # noqa: E402,F401
import loco_oracle as orc  # noqa: E402
from loco_edit_amd import config as C  # noqa: E402

T_REF, AT_REF = 603.0, 0.5


def case_config(name):
    """The shapes at which the kernels can still go wrong (each a fraction of a second on the host):
    tiny_ldm   SpatialTransformer stages at T = 256 and 64, CH 8 / 16, L = 7 (4 columns per lane, pad columns >= L): several
               token blocks, accumulation over five stages
    xattn      the AttentionBlock + cross-attention stage (OP_ATTN, has_x)
    ldm77      L = 77: the 20-columns-per-lane instantiation, 80 held columns per score row (the 4 LG = 80 that the issue
               calls Lp; the program pads the stored rows of P to ctx_Lp = 128, a multiple of 64, so the kernel reads 80 of 128)
    wide       CH 40, 8 heads, T = 64: one token block, Stable Diffusion's head width
    heads16    CH 2 / 4 (16 heads): heads of 2 channels are no multiple of the contraction kernel's 4-channel tile, so the first
               level takes the strided-GEMM route behind the FUSED row kernel (R is recomputed into the score buffer), the second
               the kernel.  (A level whose T is no multiple of the 64-token block cannot be configured: the coarsest level of a
               denoiser is at least 8 x 8 and every finer one has 4 x the tokens; LOCO_FUSE_XATTN=0 covers that route.)"""
    return {"tiny_ldm": C.TINY_LDM, "xattn": C.TINY_LATENT_XATTN,
            "ldm77": dataclasses.replace(C.TINY_LDM, context_len=77), "wide": C.WIDE_LDM,
            "heads16": dataclasses.replace(C.TINY_LDM, num_heads=16)}[name]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _grads(cfg, params, z, ctx, U, mask, cv, ce, dtype):
    """A [k, n] = U^T d f / d z and G [k, L, D] = U^T d f / d ctx of f = mask . (cv z + ce eps(z, ctx)), in `dtype`."""
    p = {k: v.to(dtype) for k, v in orc.to_torch(params).items()}
    zz = z.to(dtype).clone().requires_grad_(True)
    cc = ctx.to(dtype).clone().requires_grad_(True)
    eps = orc.unet_forward_adm(p, cfg, zz, torch.tensor(T_REF, dtype=dtype), context=cc).reshape(-1)
    f = cv * zz.reshape(-1) + ce * eps
    if mask is not None:
        f = f * mask.reshape(-1).to(dtype)
    A, G = [], []
    for u in U.to(dtype):
        a, g = torch.autograd.grad((f * u).sum(), (zz, cc), retain_graph=True)
        A.append(a.reshape(-1)); G.append(g)
    return torch.stack(A), torch.stack(G)


@functools.lru_cache(maxsize=None)
def reference(name, use_et=True, masked=True, k=3, seed=11, ctx_scale=1.0):
    """Inputs and the float64 / fp32 gradients of one case, computed once per session and shared (treat as read-only)."""
    cfg = case_config(name)
    params = C.synth_params(cfg, 0)
    g = torch.Generator().manual_seed(seed)
    R = cfg.resolution
    z = torch.randn(1, cfg.in_channels, R, R, generator=g)
    ctx = torch.randn(cfg.context_len, cfg.context_dim, generator=g) * ctx_scale
    U = torch.randn(k, cfg.n, generator=g)
    mask = None
    if masked:
        mask = torch.zeros(cfg.in_channels, R, R, dtype=torch.bool)
        mask[:, R // 4: R // 4 + R // 2, 1: R - 2] = True
    cv, ce = (0.0, 1.0) if use_et else (1.0 / math.sqrt(AT_REF), -math.sqrt(1.0 - AT_REF) / math.sqrt(AT_REF))
    A64, G64 = _grads(cfg, params, z, ctx, U, mask, cv, ce, torch.float64)
    A32, G32 = _grads(cfg, params, z, ctx, U, mask, cv, ce, torch.float32)
    return {"cfg": cfg, "params": params, "z": z, "ctx": ctx, "U": U, "mask": mask, "A64": A64, "G64": G64,
            "yardstick": rel(G32, G64), "yardstick_A1": rel(A32[:1], A64[:1])}


# --------------------------------------------------------------------------------------------------------------------------
# null-text inversion (Mokady et al., CVPR 2023) restated on the oracle: the loop of loco_edit_amd.null_text in one dtype
def ddim_prev(z, eps, at, at_prev):
    """The scheduler's eta = 0 step z_prev = sqrt(a') (z - sqrt(1 - a) eps) / sqrt(a) + sqrt(1 - a') eps with every operation,
    the coefficients' included, in the dtype of z (an fp32 run is fp32 throughout, as the engine's scheduler step is)."""
    a, ap = torch.tensor(at, dtype=z.dtype), torch.tensor(at_prev, dtype=z.dtype)
    x0 = (z - torch.sqrt(1.0 - a) * eps) / torch.sqrt(a)
    return torch.sqrt(ap) * x0 + torch.sqrt(1.0 - ap) * eps, None


def null_text_restatement(cfg, params, traj, timesteps, alphas, null_emb, cond_emb, w, inner_steps, lr, early_stop, dtype):
    """-> (embs [S, L, D], z_bar, losses: per outer step the list of inner losses), everything in `dtype` on the host.
    `alphas[i]` = (alpha_bar at timesteps[i], alpha_bar at the step's target)."""
    p = {k: v.to(dtype) for k, v in orc.to_torch(params).items()}
    f = lambda z_, t_, c_: orc.unet_forward_adm(p, cfg, z_, torch.tensor(float(t_), dtype=dtype), context=c_)
    null = null_emb.to(dtype).reshape(cfg.context_len, cfg.context_dim).clone().requires_grad_(True)
    cond = cond_emb.to(dtype).reshape(cfg.context_len, cfg.context_dim)
    zb = traj[0].to(dtype)
    embs, losses, grads = [], [], []
    for i in range(len(timesteps)):
        at, at_prev = alphas[i]
        opt = torch.optim.Adam([null], lr=lr * (1.0 - i / 100.0))
        with torch.no_grad():
            eps_c = f(zb, timesteps[i], cond)
        target = traj[i + 1].to(dtype)
        li = []
        for j in range(inner_steps):
            eps_n = f(zb, timesteps[i], null)
            z_prev, _ = ddim_prev(zb, eps_n + w * (eps_c - eps_n), at, at_prev)
            loss = ((target - z_prev) ** 2).mean()
            opt.zero_grad()
            loss.backward()
            if j == 0:
                grads.append(null.grad.detach().clone())
            opt.step()
            li.append(float(loss.detach()))
            if li[-1] < early_stop + 2e-5 * i:
                break
        losses.append(li)
        embs.append(null.detach().clone())
        with torch.no_grad():
            eps_n = f(zb, timesteps[i], null)
            zb, _ = ddim_prev(zb, eps_n + w * (eps_c - eps_n), at, at_prev)
    return torch.stack(embs), zb, losses, grads
