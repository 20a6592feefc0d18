"""Asyrp (Kwon et al., ICLR 2023, "Diffusion models already have a semantic latent space") on the HIP engine: the learned
h-space baseline of the paper's comparison table.  A small block f_t (``hip.LocoAsyrpBlock``, csrc/asyrp.hip) maps the U-Net
bottleneck h to an edit dh; it is trained from one text pair with a directional CLIP loss and applied asymmetrically in the
DDIM step.  DESIGN 7.12 holds the definition and the deviations from the released code.

One training step at (x_t, t) with the next timestep t' (``AsyrpTrainer.step``; the order matters: ``unet_forward`` and ``get_h``
invalidate a cached primal):

1. eps = unet_forward(x_t, t), h = get_h(x_t, t), dh = f_t(h, e(t)) with e(t) = ``time_vector``;
2. the decoder-tap primal at the shifted bottleneck (``pmp_primal(tap="dec", dh=dh)``); its network output eps~ is handed out by
   ``pmp_primal_eps``;
3. x0_edit = P_t(eps~), x0_src = P_t(eps); L = w_clip L_dir + w_rec mean |x0_edit - x0_src| with
   L_dir = 1 - cos(E_I(x0_edit) - E_I(x0_src), E_T(tgt) - E_T(src)) (``directional_clip_loss``), and its pixel gradient g;
4. g_h = J^T g with J = d x0_hat / d h at h + dh (``pmp_vjp``, one row), ``f_t.backward(g_h)``, one Adam step;
5. x_t' = sqrt(a') P_t(eps~) + sqrt(1 - a') eps (``sched_step_asym``: the x0 estimate is edited, the direction term is not).

Inference (``edit``) runs the same asymmetric step from T down to ``edit_t`` with both outputs from one batched
``unet_forward(dh=[dh, 0])`` and decodes plainly below it.
"""
from __future__ import annotations

import math
import os
import time
from typing import Dict, Optional, Tuple

import torch

DIR_EPS = 1e-7          # added to |E_I(x0_edit) - E_I(x0_src)| before the division: an untrained block gives a zero difference


def time_vector(cfg, t: float) -> torch.Tensor:
    """The sinusoidal embedding of ``t`` at width ``cfg.temb_ch`` in the convention of the denoiser's own first stage
    ("ddpm": [sin, cos] with divisor half - 1; "adm": [cos, sin] with divisor half), formed in float64 -> fp32 [temb_ch] (host)."""
    dim = int(cfg.temb_ch)
    half = dim // 2
    k = torch.arange(half, dtype=torch.float64)
    if cfg.arch == "ddpm":
        arg = float(t) * torch.exp(k * -(math.log(10000.0) / (half - 1)))
        parts = [torch.sin(arg), torch.cos(arg)]
    elif cfg.arch == "adm":
        arg = float(t) * torch.exp(-math.log(10000.0) * k / half)
        parts = [torch.cos(arg), torch.sin(arg)]
    else:
        raise ValueError(f"Asyrp is built for the denoisers with an h-space tap and a time embedding, not arch {cfg.arch!r}")
    emb = torch.cat(parts)
    if dim % 2:
        emb = torch.cat([emb, emb.new_zeros(1)])
    return emb.to(torch.float32)


def directional_cosine(emb: torch.Tensor, d_text: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(loss, d loss / d emb [2, P]) in float64 for emb [2, P] = (E_I(x0_edit), E_I(x0_src)) and d_text [P] = E_T(tgt) - E_T(src):
    loss = 1 - <d / (|d| + DIR_EPS), d_text / |d_text|> with d = emb[0] - emb[1].  The source row of the gradient is zero: the
    source frame is a constant of the loss (Asyrp detaches it)."""
    emb, d_text = emb.double(), d_text.double().flatten()
    tn = d_text / d_text.norm()
    d = emb[0] - emb[1]
    n = d.norm()
    cos = (d @ tn) / (n + DIR_EPS)
    g = tn / (n + DIR_EPS)
    if float(n) > 0:
        g = g - cos * d / (n * (n + DIR_EPS))
    return 1 - cos, torch.stack([-g, torch.zeros_like(g)])


def directional_clip_loss(scorer, x0_edit: torch.Tensor, x0_src: torch.Tensor, text_src_embed: torch.Tensor,
                          text_tgt_embed: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(L_dir, d L_dir / d x0_edit [1, 3, H, W]) for two frames [1, 3, H, W] in [-1, 1] on the device.  Both frames go through ONE
    ``encode`` of the CLIP image tower; the cosine and its derivative with respect to the embeddings are float64 torch
    operations on [2, P]; the cotangent pass is ``encode_vjp`` with a zero row for the source frame, then
    ``preprocess_float_vjp``."""
    if not getattr(scorer.vision, "grad", False):
        raise RuntimeError("directional_clip_loss needs a scorer built with grad=True (load_clip(..., grad=True))")
    if scorer.vision.max_images < 2:
        raise RuntimeError("directional_clip_loss encodes the edited and the source frame together: the scorer needs max_images >= 2")
    if x0_edit.shape != x0_src.shape or x0_edit.dim() != 4 or x0_edit.shape[0] != 1:
        raise ValueError(f"x0_edit and x0_src must both be [1, 3, H, W], got {tuple(x0_edit.shape)} and {tuple(x0_src.shape)}")
    P = scorer.vision_cfg.projection_dim
    ts, tt = torch.as_tensor(text_src_embed).flatten(), torch.as_tensor(text_tgt_embed).flatten()
    if ts.numel() != P or tt.numel() != P:
        raise ValueError(f"the text embeddings must hold {P} values each, got {tuple(text_src_embed.shape)} and {tuple(text_tgt_embed.shape)}")
    frames = torch.cat([x0_edit, x0_src]).to(torch.float32).contiguous()
    H, W = frames.shape[2:]
    pv = scorer.vision.preprocess_float(frames, None)
    emb = scorer.vision.encode(pv)
    loss, g_emb = directional_cosine(emb, (tt.double() - ts.double()).to(emb.device))
    g_pv = scorer.vision.encode_vjp(g_emb.to(torch.float32).contiguous())
    grad = scorer.vision.preprocess_float_vjp(g_pv, None, 2, H, W)
    return loss.to(torch.float32), grad[:1].contiguous()


def _forward_pair(engine, x: torch.Tensor, t: float, dh: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(eps~, eps) of one frame x [1, C, R, R]: the network output with dh added to the bottleneck, and without.  One batched launch
    of exactly max_batch rows (the frame repeated, dh = [dh, 0, 0, ..]) when the engine holds two rows -- the engine picks its conv
    tiling by the batch size, so this is the arithmetic of ``hspace_pca.decode_with_dh`` -- else two launches."""
    mb = engine.max_batch
    if mb < 2:
        return engine.unet_forward(x, float(t), dh=dh.reshape(1, -1).contiguous()), engine.unet_forward(x, float(t))
    xb = x.expand(mb, -1, -1, -1).contiguous()
    dhb = torch.zeros(mb, engine.n_h, device=x.device, dtype=torch.float32)
    dhb[0] = dh.reshape(-1)
    et = engine.unet_forward(xb, float(t), dh=dhb)
    return et[:1].contiguous(), et[1:2].contiguous()


class AsyrpTrainer:
    """Trains ``block`` (a ``hip.LocoAsyrpBlock`` of the engine's bottleneck geometry) on one text pair."""

    def __init__(self, engine, scheduler, scorer, block, text_src_embed, text_tgt_embed, cfg, lr: float = 1e-3,
                 clip_weight: float = 0.8, rec_weight: float = 3.0, adam_step: int = 0):
        if tuple(engine.h_shape) != (block.C, block.H, block.W):
            raise ValueError(f"the block is built for h {(block.C, block.H, block.W)}, the engine's bottleneck is {tuple(engine.h_shape)}")
        if block.E != cfg.temb_ch:
            raise ValueError(f"the block takes a time vector of width {block.E}, the denoiser's is {cfg.temb_ch}")
        if not lr > 0:
            raise ValueError(f"lr = {lr} must be positive")
        self.engine, self.scheduler, self.scorer, self.block, self.cfg = engine, scheduler, scorer, block, cfg
        self.text_src, self.text_tgt = text_src_embed, text_tgt_embed
        self.lr, self.clip_weight, self.rec_weight = float(lr), float(clip_weight), float(rec_weight)
        self.adam_step = int(adam_step)
        self.last: Dict[str, float] = {}

    def loss_and_gradient(self, x0_edit: torch.Tensor, x0_src: torch.Tensor):
        """(L, L_dir, L_rec, d L / d x0_edit) of step 3."""
        diff = x0_edit - x0_src
        l_rec = diff.abs().mean()
        g = (self.rec_weight / diff.numel()) * torch.sign(diff)
        l_dir = torch.zeros((), device=x0_edit.device)
        if self.clip_weight != 0:
            l_dir, g_dir = directional_clip_loss(self.scorer, x0_edit, x0_src, self.text_src, self.text_tgt)
            g = g + self.clip_weight * g_dir
        return self.clip_weight * l_dir + self.rec_weight * l_rec, l_dir, l_rec, g.contiguous()

    @torch.no_grad()
    def step(self, x_t: torch.Tensor, t: float, t_next: float) -> torch.Tensor:
        """One training step at (x_t [1, C, R, R], t); returns x_t' of the asymmetric step.  ``self.last`` holds the losses."""
        eng, sch = self.engine, self.scheduler
        at, at_next = sch.alpha_at(t), sch.alpha_at(t_next)
        x_t = x_t.to(torch.float32).contiguous()
        eps = eng.unet_forward(x_t, float(t))
        h = eng.get_h(x_t, float(t))
        e = time_vector(self.cfg, t).to(x_t.device)
        dh = self.block.forward(h, e, s=1.0, keep_records=True)
        eng.pmp_primal(x_t, float(t), at, None, use_et=False, tap="dec", dh=dh.reshape(-1))
        eps_edit = eng.pmp_primal_eps().view_as(x_t)
        _, x0_edit = eng.sched_step(x_t, eps_edit, at, at, 0.0, None, want_x0=True)
        _, x0_src = eng.sched_step(x_t, eps, at, at, 0.0, None, want_x0=True)
        loss, l_dir, l_rec, g = self.loss_and_gradient(x0_edit, x0_src)
        g_h = eng.pmp_vjp(g.view(1, -1))                 # J = d x0_hat / d h at h + dh: the tap's factor c is inside
        self.block.zero_grad()
        self.block.backward(g_h.view_as(h).contiguous())
        self.adam_step += 1
        self.block.adam_step(self.adam_step, self.lr)
        self.last = {"loss": float(loss), "l_dir": float(l_dir), "l_rec": float(l_rec)}
        x_next, _ = eng.sched_step_asym(x_t, eps_edit, eps, at, at_next)
        return x_next

    def train_image(self, x_T: torch.Tensor, t_end_idx: int, verbose: bool = False) -> float:
        """The timesteps of the scheduler's current schedule from T down to index ``t_end_idx`` (exclusive) for one inverted
        image; returns the mean loss."""
        ts, tn = self.scheduler.timesteps, self.scheduler.timesteps_next
        x, total = x_T, 0.0
        for i in range(int(t_end_idx)):
            x = self.step(x, float(ts[i]), float(tn[i]))
            total += self.last["loss"]
            if verbose:
                print(f"asyrp: t = {float(ts[i]):.1f}, loss {self.last['loss']:.5f} (directional {self.last['l_dir']:.5f}, "
                      f"reconstruction {self.last['l_rec']:.5f})")
        return total / max(int(t_end_idx), 1)


@torch.no_grad()
def edit(engine, scheduler, block, cfg, x_T: torch.Tensor, t_end_idx: int, scale: float = 1.0) -> torch.Tensor:
    """x_T [1, C, R, R] -> x_t at index ``t_end_idx`` of the scheduler's current schedule through the asymmetric step with
    dh = scale f_t(h, e(t)).  The caller decodes plainly from there."""
    ts, tn = scheduler.timesteps, scheduler.timesteps_next
    x = x_T.to(torch.float32).contiguous()
    for i in range(int(t_end_idx)):
        t, t_next = float(ts[i]), float(tn[i])
        at, at_next = scheduler.alpha_at(ts[i]), scheduler.alpha_at(tn[i])
        h = engine.get_h(x, t)
        dh = block.forward(h, time_vector(cfg, t).to(x.device), s=float(scale), keep_records=False)
        eps_edit, eps = _forward_pair(engine, x, t, dh)
        x, _ = engine.sched_step_asym(x, eps_edit, eps, at, at_next)
    return x


def save_checkpoint(path: str, block, adam_step: int, meta: Optional[dict] = None):
    """A state dict of the ten tensors plus the Adam step count (Adam's moments are not kept: a loaded block is for inference)."""
    sd = dict(block.state_dict())
    sd["adam_step"] = int(adam_step)
    sd["geometry"] = {"C": block.C, "H": block.H, "W": block.W, "E": block.E}
    if meta:
        sd["meta"] = dict(meta)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(sd, path)


def load_checkpoint(path: str, block) -> int:
    """Loads the ten tensors into ``block``; returns the Adam step count."""
    sd = torch.load(path, map_location="cpu")
    geo = sd.get("geometry")
    want = {"C": block.C, "H": block.H, "W": block.W, "E": block.E}
    if geo is not None and dict(geo) != want:
        raise ValueError(f"{path} holds a block of geometry {dict(geo)}, this denoiser's bottleneck asks for {want}")
    missing = [k for k in block.PARAMS if k not in sd]
    if missing:
        raise ValueError(f"{path} is no Asyrp checkpoint: it lacks {missing}")
    block.load_state_dict({k: sd[k] for k in block.PARAMS})
    block.reset_moments()
    return int(sd.get("adam_step", 0))


def parse_index_range(text: str):
    """'0-99' (inclusive), '5' or a comma list of those -> the list of indices."""
    out = []
    for part in str(text).split(","):
        part = part.strip()
        if not part:
            continue
        lo, sep, hi = part.partition("-")
        try:
            a = int(lo)
            b = int(hi) if sep else a
        except ValueError:
            raise ValueError(f"--asyrp_train_idx {text!r}: expected indices such as 0-99 or 3,7,11") from None
        if a < 0 or b < a:
            raise ValueError(f"--asyrp_train_idx {text!r}: ranges run upwards from a non-negative index")
        out.extend(range(a, b + 1))
    if not out:
        raise ValueError("--asyrp_train_idx names no image")
    return out


def timed(fn):
    """(result, seconds) with the device drained on both sides."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0
