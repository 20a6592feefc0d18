"""Null-text inversion (Mokady et al., "Null-text Inversion for Editing Real Images using Guided Diffusion Models", CVPR
2023) on the HIP engine, for the Stable Diffusion T-LOCO drivers (``tloco_sd.EditStableDiffusion``).

Under classifier-free guidance a DDIM-inverted latent does not decode back to the source image, so the subspace solve at
``edit_t`` would linearise around a different picture.  The remedy: invert with the conditional branch alone, then, walking
back down, optimise the UNCONDITIONAL prompt states per timestep so that the guided step lands on the inverted trajectory.

The optimiser needs d eps / d (prompt states): ``LocoEngine.pmp_vjp(g, context_grad=True)`` (csrc/xattn_ctx.hip).  Per inner
iteration the network work is one primal and one cotangent pass of the null branch; Adam (``torch.optim.Adam``, the published
arithmetic) and the loss are a few torch operations on [L, D] and [n] device tensors.  Constants as published: learning rate
lr (1 - i / 100) at outer step i, early stop at loss < early_stop + 2e-5 i.
"""
from __future__ import annotations

import hashlib
import json
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch


def step_lr(lr: float, i: int) -> float:
    """Adam's learning rate at outer step i."""
    return lr * (1.0 - i / 100.0)


def stops_early(loss: float, early_stop: float, i: int) -> bool:
    """The published stopping rule of the inner loop at outer step i."""
    return loss < early_stop + 2e-5 * i


def eps_coefficient(at: float, at_next: float) -> float:
    """d z_prev / d eps of the scheduler's eta = 0 step z_prev = sqrt(a') (z - sqrt(1 - a) eps) / sqrt(a) + sqrt(1 - a') eps,
    in the fp32 arithmetic of loco_sched_step."""
    a, an = np.float32(at), np.float32(at_next)
    one = np.float32(1.0)
    return float(np.sqrt(one - an) - np.sqrt(an) * np.sqrt(one - a) / np.sqrt(a))


def cache_path(result_folder: str, idx: int) -> str:
    return os.path.join(result_folder, f"null_text-{idx}.pt")


def save_cache(path: str, embs: torch.Tensor, zT: torch.Tensor, report: dict) -> None:
    torch.save({"embs": embs.detach().cpu(), "zT": zT.detach().cpu(), "report": report}, path)


def image_digest(x0: torch.Tensor) -> str:
    """What identifies the inverted image in the cache: the sha256 of its fp32 values."""
    return hashlib.sha256(x0.detach().to("cpu", torch.float32).contiguous().numpy().tobytes()).hexdigest()


def load_cache(path: str, steps: int, shape: Sequence[int], settings: Optional[dict] = None) -> Optional[dict]:
    """The cached embeddings [steps, L, D] of one sample, or None when the file is absent or was written for another run
    length / context shape, or -- ``settings``: the entries of the cached report that must equal this run's (inner_steps, lr,
    early_stop, guidance_scale, image_sha256) -- under other settings or for another image."""
    if not os.path.exists(path):
        return None
    c = torch.load(path, map_location="cpu")
    if tuple(c["embs"].shape) != (steps,) + tuple(shape):
        return None
    if settings is not None and any(c["report"].get(k) != v for k, v in settings.items()):
        return None
    return c


def write_report(path: str, report: dict) -> None:
    with open(path, "w") as f:
        json.dump(report, f, indent=1)


def check_steps(inv_steps: int, for_steps: int) -> None:
    if inv_steps != for_steps:
        raise ValueError(f"--null_text_inversion walks the inverted trajectory back down step by step: it needs inv_steps == "
                         f"for_steps, got inv_steps {inv_steps} and for_steps {for_steps}")


class NullTextInversion:
    """``NullTextInversion(ed).run(...)``: ``ed`` is an ``EditStableDiffusion`` (its "for" and "null" branch engines, its
    scheduler with the decode timestep table set, its guidance scale)."""

    def __init__(self, ed):
        if not ed.use_context:
            raise ValueError("null-text inversion optimises the prompt states of the cross-attention stages: the denoiser has none "
                             "(context_dim = 0)")
        if "null" not in ed.branches or "for" not in ed.branches:
            raise ValueError("null-text inversion optimises the prompt of the `null` guidance branch beside the `for` branch: this "
                             f"class runs the branches {' / '.join(ed.branches)} (the latent-consistency class has no null branch)")
        if ed.guidance_scale <= 1.0:
            raise ValueError("null-text inversion corrects the guided decode: it needs guidance_scale > 1")
        self.ed = ed
        self.seconds: List[float] = []

    def run(self, traj: Sequence[torch.Tensor], timesteps, null_emb: torch.Tensor, cond_emb: torch.Tensor, inner_steps: int = 10,
            lr: float = 1e-2, early_stop: float = 1e-5) -> Tuple[torch.Tensor, torch.Tensor, List[List[float]]]:
        """``traj[i]`` is the inverted latent at ``timesteps[i]`` in decode order (noisiest first, ``traj[-1]`` = z*_0; one
        more point than timesteps).  -> (embs [S, L, D], z_bar, losses): the optimised unconditional states per step, the
        latent the guided decode reaches with them, and per step the loss before each inner update."""
        ed = self.ed
        S = len(timesteps)
        if len(traj) != S + 1:
            raise ValueError(f"{S} steps need {S + 1} trajectory points, got {len(traj)}")
        dev = ed.device
        eng_c, eng_n = ed.branches["for"], ed.branches["null"]
        w = float(ed.guidance_scale)
        E = ed.edit_prompt_emb
        null = null_emb.to(dev, torch.float32).reshape(null_emb.shape[-2], null_emb.shape[-1]).clone().contiguous()
        null.grad = torch.zeros_like(null)
        zb = traj[0].to(dev, torch.float32).contiguous()
        n = zb.numel()
        embs, losses = [], []
        self.seconds = []
        for i, t in enumerate(timesteps):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            at = ed.scheduler.alpha_at(t)
            at_next = ed.scheduler.alpha_at(ed.scheduler.timesteps_next[ed.scheduler.index_of(t)])
            target = traj[i + 1].to(dev, torch.float32).contiguous()
            li: List[float] = []
            if inner_steps > 0:
                opt = torch.optim.Adam([null], lr=step_lr(lr, i))
                ed._bind("for", cond_emb)
                eps_c = eng_c.unet_forward(zb, float(t))
                gscale = (1.0 - w) * eps_coefficient(at, at_next) * 2.0 / n      # g = (1 - w) d loss / d eps~
                for _ in range(inner_steps):
                    eng_n.set_context(null)
                    ed._cond_of.pop("null", None)          # the branch no longer holds the prompt _bind recorded
                    eng_n.pmp_primal(zb, float(t), at, None, use_et=True)
                    eps_n = eng_n.pmp_primal_eps().view_as(zb)
                    z_prev, _ = eng_c.sched_step(zb, eng_c.lincomb([(w, eps_c), (1.0 - w, eps_n)]), at, at_next)
                    diff = z_prev - target
                    loss = (diff * diff).mean()
                    _, G = eng_n.pmp_vjp((gscale * diff).reshape(1, n).contiguous(), context_grad=True)
                    null.grad.copy_(G[0])
                    opt.step()
                    li.append(float(loss))
                    if stops_early(li[-1], early_stop, i):
                        break
            losses.append(li)
            embs.append(null.detach().clone())
            # z_bar <- the guided step with the final states: the sampler's own calls (DDIMforwardsteps), bit for bit
            eps = ed._classifer_free_guidance(zb, t, cond_emb, E, null[None], mode="null+(for-null)", do_classifier_free_guidance=True)
            zb = ed.scheduler.step(eps, t, zb, eta=0).prev_sample
            ev1.record()
            ev1.synchronize()
            self.seconds.append(ev0.elapsed_time(ev1) * 1e-3)
        return torch.stack(embs), zb, losses
