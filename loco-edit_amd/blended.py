"""Blended Diffusion (Avrahami et al., 2022) on the HIP engine: the text-driven, mask-local edit of an unconditional DDPM,
the baseline column of the paper's comparison table.

One step from t to t' on the run's schedule (``guided_step``):

1. one primal pass at (x_t, t) without a mask (``pmp_primal``); its network output is handed out by ``pmp_primal_eps``, the
   network is not evaluated twice; x0_hat follows from eps by the scheduler's own formula (``sched_step`` at a_t -> a_t);
2. loss = clip_guidance_scale . mean_i (1 - cos(E_I(window_i(x0_hat . m)), e_text)) + range_scale . mean |x0_hat -
   clamp(x0_hat, -1, 1)|; its gradient g_x0 with respect to x0_hat comes from ``ClipScorer.text_guidance`` (the CLIP image
   tower's cotangent pass in HIP) plus the range term;
3. g = J^T g_x0 with J = d x0_hat / d x_t (``pmp_vjp``, one row);
4. eps_hat = eps + sqrt(1 - a_t) g and ``sched_step(x_t, eps_hat, a_t, a_t', eta, noise)``: classifier guidance in its DDIM
   form (Dhariwal & Nichol, Alg. 2);
5. the blend x_t' = m . x_t' + (1 - m) . (sqrt(a_t') x_src + sqrt(1 - a_t') z'); after the last step the background is x_src.

Deviations from the released code, both stated in DESIGN 7.9: the release shifts the mean of the DDPM posterior by the scaled
gradient, this engine's scheduler is the reference's DDIM step, so the guidance enters through eps; and the release's
augmentations are random perspective / affine warps, here they are square windows (the first one the whole frame).
Every random draw (the start noise, the steps' noise, the background noise, the windows) comes from one seeded host generator.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch


def draw_boxes(gen: torch.Generator, num_aug: int, H: int, W: int) -> List[Tuple[int, int, int, int]]:
    """`num_aug` windows (top, left, h, w): the whole frame, then squares of side round(s min(H, W)), s ~ U[0.75, 1], at a
    uniform position."""
    boxes = [(0, 0, H, W)]
    for _ in range(max(int(num_aug), 1) - 1):
        s = 0.75 + 0.25 * float(torch.rand((), generator=gen))
        side = max(1, min(int(round(s * min(H, W))), min(H, W)))
        top = int(torch.randint(0, H - side + 1, (), generator=gen))
        left = int(torch.randint(0, W - side + 1, (), generator=gen))
        boxes.append((top, left, side, side))
    return boxes


def guidance_gradient(scorer, x0: torch.Tensor, m: torch.Tensor, text_embed: torch.Tensor, boxes, clip_guidance_scale: float,
                      range_scale: float):
    """(loss, d loss / d x0_hat) of step 2.  x0 [1, 3, H, W]; m [1, 3, H, W] fp32 of zeros and ones."""
    over = x0 - x0.clamp(-1, 1)
    loss = range_scale * over.abs().mean()
    g = (range_scale / x0.numel()) * torch.sign(over)
    if clip_guidance_scale != 0:
        li, gm = scorer.text_guidance((x0 * m).contiguous(), text_embed, boxes)
        loss = loss + clip_guidance_scale * li.mean()
        g = g + (clip_guidance_scale / li.numel()) * gm * m
    return loss, g.contiguous()


def guided_step(engine, scorer, x: torch.Tensor, t: float, at: float, at_next: float, text_embed, boxes, m: torch.Tensor,
                clip_guidance_scale: float, range_scale: float, eta: float, noise: Optional[torch.Tensor]):
    """Steps 1-4 -> (x_t' before the blend, g = J^T g_x0 [1, 3, H, W], loss or None)."""
    engine.pmp_primal(x, float(t), at, None)
    eps = engine.pmp_primal_eps().view_as(x)
    if clip_guidance_scale == 0 and range_scale == 0:
        nxt, _ = engine.sched_step(x, eps, at, at_next, eta, noise)
        return nxt, None, None
    _, x0 = engine.sched_step(x, eps, at, at, 0.0, None, want_x0=True)
    loss, g_x0 = guidance_gradient(scorer, x0, m, text_embed, boxes, clip_guidance_scale, range_scale)
    g = engine.pmp_vjp(g_x0.view(1, -1)).view_as(x)
    eps_hat = engine.lincomb([(1.0, eps), (math.sqrt(1.0 - at), g)])
    nxt, _ = engine.sched_step(x, eps_hat, at, at_next, eta, noise)
    return nxt, g, loss


def start_index(scheduler, start_t: float) -> int:
    return int((scheduler.timesteps - start_t * 1000).abs().argmin())


@torch.no_grad()
def run(engine, scheduler, scorer, x_src: torch.Tensor, mask: torch.Tensor, text_embed, seed: int, start_t: float,
        clip_guidance_scale: float = 1000.0, range_scale: float = 50.0, num_aug: int = 8, eta: float = 1.0, verbose: bool = False):
    """The whole edit: x_src [1, 3, H, W] in [-1, 1] on the device, mask bool [3, H, W] (True: edited), `scheduler` with
    ``set_timesteps`` already called.  Returns the result [1, 3, H, W]: equal to x_src outside the mask."""
    dev = x_src.device
    x_src = x_src.to(torch.float32).contiguous()
    keep = mask.to(dev).bool().view_as(x_src)
    m = keep.to(torch.float32)
    gen = torch.Generator().manual_seed(int(seed))

    def randn():
        return torch.randn(x_src.shape, generator=gen).to(dev)

    ts, ts_next = scheduler.timesteps, scheduler.timesteps_next
    i0 = start_index(scheduler, start_t)
    a0 = scheduler.alpha_at(ts[i0])
    x = (math.sqrt(a0) * x_src + math.sqrt(1.0 - a0) * randn()).contiguous()
    H, W = x_src.shape[-2:]
    for i in range(i0, len(ts)):
        t, at, at_next = float(ts[i]), scheduler.alpha_at(ts[i]), scheduler.alpha_at(ts_next[i])
        boxes = draw_boxes(gen, num_aug, H, W)
        noise = randn() if eta != 0 else None
        nxt, _, loss = guided_step(engine, scorer, x, t, at, at_next, text_embed, boxes, m, clip_guidance_scale, range_scale, eta, noise)
        if i == len(ts) - 1:
            bg = x_src
        else:
            bg = math.sqrt(at_next) * x_src + math.sqrt(1.0 - at_next) * randn()
        x = torch.where(keep, nxt, bg).contiguous()
        if verbose and loss is not None:
            print(f"blended diffusion: t = {t:.1f}, loss {float(loss):.4f}")
    return x
