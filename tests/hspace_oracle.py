"""Torch restatement of the h-space entry points of the reference's denoiser class (models/ddpm/diffusion.py:145-345:
``get_h``, ``get_h_to_e``, ``forward(x, t, u, op='mid', block_idx=0)``), built from the block functions of oracle/loco_oracle.py
for both module trees (Ho-DDPM and ADM).  The forward pass is cut behind the middle block's last op: ``encode`` runs the ops up
to it and returns (h, skips, embedding), ``decode`` the ops behind it.  Works in float64 (float64 parameters and inputs).

    get_h(p, cfg, x, t)          h [B, C, H, W]
    h_to_e(p, cfg, x, t, h)      eps [k, ...] of k bottleneck tensors h [k, C, H, W] with the skips of ONE x (repeated k times)
    forward_dh(p, cfg, x, t, dh) eps [B, ...] with h[b] + dh[b]; dh None = the plain forward
"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import loco_oracle as orc  # noqa: E402


def _is_adm(cfg):
    return getattr(cfg, "arch", "ddpm") == "adm"


def _attn_adm(p, cfg, name, h, context):
    if getattr(cfg, "transformer_depth", 0) > 0:
        ctx = context if context.dim() == 3 else context[None]
        return orc._ldm_spatial_transformer(p, name, h, ctx.expand(h.shape[0], -1, -1), cfg)
    if getattr(cfg, "added_kv", False):
        ctx = context if context.dim() == 3 else context[None]
        return orc._if_attn(p, name, h, ctx.expand(h.shape[0], -1, -1), cfg)
    h = orc._adm_attn(p, name, h, cfg)
    if getattr(cfg, "context_dim", 0) > 0:
        ctx = context if context.dim() == 3 else context[None]
        h = orc._adm_xattn(p, name + ".xattn", h, ctx.expand(h.shape[0], -1, -1), cfg)
    return h


def encode(p, cfg, x, t, context=None, emb_add=None):
    """-> (h, hs, emb): the bottleneck tensor, the skip stack (bottom first, as the up path pops it) and the time embedding.
    ``context`` / ``emb_add``: the prompt states and the addition to the time embedding of the conditioned ADM networks, as
    ``loco_oracle.unet_forward_adm`` takes them."""
    t = t.reshape(1) if t.dim() == 0 else t
    if _is_adm(cfg):
        dt = orc._up_dtype(p["time_embed.0.weight"])
        emb = orc.timestep_embedding_adm(t.to(dt), cfg.ch, dt)
        emb = F.linear(emb, p["time_embed.0.weight"], p["time_embed.0.bias"])
        emb = F.linear(orc._act(cfg)(emb), p["time_embed.2.weight"], p["time_embed.2.bias"])
        if emb_add is not None:
            emb = emb + emb_add
        h = F.conv2d(x, p["input_blocks.0.0.weight"], p["input_blocks.0.0.bias"], padding=1)
        hs = [h]
        res, ib, nlev = cfg.resolution, 1, len(cfg.ch_mult)
        for lvl in range(nlev):
            for _ in range(cfg.num_res_blocks):
                h = orc._adm_resblock(p, f"input_blocks.{ib}.0", h, emb, cfg)
                if res in cfg.attn_resolutions:
                    h = _attn_adm(p, cfg, f"input_blocks.{ib}.1", h, context)
                hs.append(h); ib += 1
            if lvl != nlev - 1:
                if getattr(cfg, "resblock_updown", True):
                    h = orc._adm_resblock(p, f"input_blocks.{ib}.0", h, emb, cfg, down=True)
                else:
                    h = F.conv2d(h, p[f"input_blocks.{ib}.0.op.weight"], p[f"input_blocks.{ib}.0.op.bias"], stride=2, padding=1)
                hs.append(h); ib += 1
                res //= 2
        h = orc._adm_resblock(p, "middle_block.0", h, emb, cfg)
        h = _attn_adm(p, cfg, "middle_block.1", h, context)
        h = orc._adm_resblock(p, "middle_block.2", h, emb, cfg)
        return h, hs, emb
    dt = orc._up_dtype(p["temb.dense.0.weight"])
    temb = orc.timestep_embedding(t.to(dt), cfg.ch, dt)
    temb = F.linear(temb, p["temb.dense.0.weight"], p["temb.dense.0.bias"])
    temb = F.linear(orc._swish(temb), p["temb.dense.1.weight"], p["temb.dense.1.bias"])
    nres, res = len(cfg.ch_mult), cfg.resolution
    hs = [F.conv2d(x, p["conv_in.weight"], p["conv_in.bias"], padding=1)]
    for lvl in range(nres):
        for b in range(cfg.num_res_blocks):
            h = orc._resblock(p, f"down.{lvl}.block.{b}", hs[-1], temb, cfg)
            if res in cfg.attn_resolutions:
                h = orc._attn(p, f"down.{lvl}.attn.{b}", h, cfg)
            hs.append(h)
        if lvl != nres - 1:
            hs.append(F.conv2d(F.pad(hs[-1], (0, 1, 0, 1)), p[f"down.{lvl}.downsample.conv.weight"],
                               p[f"down.{lvl}.downsample.conv.bias"], stride=2))
            res //= 2
    h = orc._resblock(p, "mid.block_1", hs[-1], temb, cfg)
    h = orc._attn(p, "mid.attn_1", h, cfg)
    h = orc._resblock(p, "mid.block_2", h, temb, cfg)
    return h, hs, temb


def decode(p, cfg, h, hs, emb, context=None):
    """The ops behind the tap; ``hs`` is consumed from the back (a copy is taken)."""
    hs = list(hs)
    nlev = len(cfg.ch_mult)
    res = cfg.resolution >> (nlev - 1)
    if _is_adm(cfg):
        ob = 0
        for lvl in reversed(range(nlev)):
            for i in range(cfg.num_res_blocks + 1):
                h = orc._adm_resblock(p, f"output_blocks.{ob}.0", torch.cat([h, hs.pop()], dim=1), emb, cfg)
                j = 1
                if res in cfg.attn_resolutions:
                    h = _attn_adm(p, cfg, f"output_blocks.{ob}.{j}", h, context); j += 1
                if lvl and i == cfg.num_res_blocks:
                    if getattr(cfg, "resblock_updown", True):
                        h = orc._adm_resblock(p, f"output_blocks.{ob}.{j}", h, emb, cfg, up=True)
                    else:
                        h = F.interpolate(h, scale_factor=2, mode="nearest")
                        h = F.conv2d(h, p[f"output_blocks.{ob}.{j}.conv.weight"], p[f"output_blocks.{ob}.{j}.conv.bias"], padding=1)
                    res *= 2
                ob += 1
        h = orc._act(cfg)(orc._adm_gn(p, "out.0", h, cfg))
        h = F.conv2d(h, p["out.2.weight"], p["out.2.bias"], padding=1)
        if cfg.learn_sigma:
            h = torch.split(h, h.shape[1] // 2, dim=1)[0]
        return h
    for lvl in reversed(range(nlev)):
        for b in range(cfg.num_res_blocks + 1):
            h = orc._resblock(p, f"up.{lvl}.block.{b}", torch.cat([h, hs.pop()], dim=1), emb, cfg)
            if res in cfg.attn_resolutions:
                h = orc._attn(p, f"up.{lvl}.attn.{b}", h, cfg)
        if lvl != 0:
            h = F.interpolate(h, scale_factor=2.0, mode="nearest")
            h = F.conv2d(h, p[f"up.{lvl}.upsample.conv.weight"], p[f"up.{lvl}.upsample.conv.bias"], padding=1)
            res *= 2
    h = orc._swish(orc._gn(p, "norm_out", h, cfg))
    return F.conv2d(h, p["conv_out.weight"], p["conv_out.bias"], padding=1)


def get_h(p, cfg, x, t, context=None, emb_add=None):
    return encode(p, cfg, x, t, context, emb_add)[0]


def h_to_e(p, cfg, x, t, h, context=None, emb_add=None):
    """get_h_to_e (diffusion.py:273-345): the skips of the one sample ``x`` repeated for each of the k rows of ``h``."""
    assert x.shape[0] == 1
    h0, hs, emb = encode(p, cfg, x, t, context, emb_add)
    k = h.shape[0]
    return decode(p, cfg, h.reshape(k, *h0.shape[1:]), [s.expand(k, -1, -1, -1) for s in hs], emb, context)


def forward_dh(p, cfg, x, t, dh=None, context=None, emb_add=None):
    """forward(x, t, u=dh, op='mid', block_idx=0) (diffusion.py:145-200)."""
    h, hs, emb = encode(p, cfg, x, t, context, emb_add)
    if dh is not None:
        h = h + dh.reshape(h.shape)
    return decode(p, cfg, h, hs, emb, context)
