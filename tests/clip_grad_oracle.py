"""Float64 restatements for the CLIP pixel-gradient tests (not collected by pytest): the window preprocessing of
``loco_clipvis_preprocess_f32`` as dense per-axis resize matrices built from the tap rule of csrc/clipvis.hip (``cv_taps``), the
image tower in plain torch, and the guidance loss of ``ClipScorer.text_guidance``.  Everything is differentiable: gradients
come from autograd."""
import math

import torch
import torch.nn.functional as F


def cubic(x: float) -> float:
    x = abs(x)
    if x < 1.0:
        return ((1.5 * x - 2.5) * x) * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5
    return 0.0


def resize_matrix(n_in: int, n_out: int) -> torch.Tensor:
    """[n_out, n_in] float64: row o holds the normalised antialiased bicubic (a = -0.5) weights of output pixel o -- taps
    [lo, hi) with lo = max(int(center - support + 0.5), 0), hi = min(int(center + support + 0.5), n_in), center =
    (o + 0.5) scale, support = 2 max(scale, 1), weight cubic((j - center + 0.5) / max(scale, 1)) / (their sum)."""
    scale = n_in / n_out
    support, inv = 2.0 * max(scale, 1.0), 1.0 / max(scale, 1.0)
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        center = (o + 0.5) * scale
        lo, hi = max(int(center - support + 0.5), 0), min(int(center + support + 0.5), n_in)
        w = [cubic((j - center + 0.5) * inv) for j in range(lo, hi)]
        total = math.fsum(w)
        for j, v in zip(range(lo, hi), w):
            m[o, j] = v / total
    return m


def tap_count(n_in: int, n_out: int) -> int:
    return int((resize_matrix(n_in, n_out) != 0).sum(dim=1).max())


def default_boxes(n: int, H: int, W: int):
    s = min(H, W)
    return [((H - s) // 2, (W - s) // 2, s, s)] * n


def preprocess_windows(frames: torch.Tensor, boxes, S: int, mean, std) -> torch.Tensor:
    """frames [nf, 3, H, W] in [-1, 1] (any float dtype; computed in float64), boxes [(top, left, h, w)] * n or None -> float64
    [n, 3, S, S]: every window resized straight to S x S, one matrix per axis, then (v / 2 + 1 / 2 - mean) / std."""
    x = frames.to(torch.float64)
    nf, _, H, W = x.shape
    boxes = default_boxes(nf, H, W) if boxes is None else [tuple(int(v) for v in b) for b in boxes]
    assert nf in (1, len(boxes))
    m = torch.tensor(mean, dtype=torch.float64).view(3, 1, 1)
    s = torch.tensor(std, dtype=torch.float64).view(3, 1, 1)
    out = []
    for i, (top, left, h, w) in enumerate(boxes):
        assert 0 <= top and 0 <= left and h >= 1 and w >= 1 and top + h <= H and left + w <= W
        win = x[0 if nf == 1 else i, :, top:top + h, left:left + w]
        r = resize_matrix(h, S) @ win @ resize_matrix(w, S).T
        out.append((r * 0.5 + 0.5 - m) / s)
    return torch.stack(out)


def clip_vision_embeds(sd, cfg, pixel_values: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """CLIPVisionModelWithProjection's image_embeds [n, P] in `dtype` (float64) from a state dict without the ``vision_model.``
    prefix (plus ``visual_projection.weight``) and a ``clip_score.ClipVisionConfig``."""
    w = {k: v.to(dtype) for k, v in sd.items()}
    D, ps, heads = cfg.width, cfg.patch_size, cfg.heads
    x = F.conv2d(pixel_values.to(dtype), w["embeddings.patch_embedding.weight"], stride=ps).flatten(2).transpose(1, 2)
    n = x.shape[0]
    x = torch.cat([w["embeddings.class_embedding"].expand(n, 1, D), x], dim=1) + w["embeddings.position_embedding.weight"]

    def ln(v, name):
        return F.layer_norm(v, (D,), w[name + ".weight"], w[name + ".bias"], cfg.ln_eps)

    def lin(v, name):
        return F.linear(v, w[name + ".weight"], w[name + ".bias"])

    x = ln(x, "pre_layrnorm")
    for i in range(cfg.layers):
        p = f"encoder.layers.{i}."
        y = ln(x, p + "layer_norm1")
        q, k, v = (lin(y, p + f"self_attn.{m}_proj").view(n, -1, heads, D // heads).transpose(1, 2) for m in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) * (D // heads) ** -0.5, dim=-1) @ v
        x = x + lin(a.transpose(1, 2).reshape(n, -1, D), p + "self_attn.out_proj")
        y = lin(ln(x, p + "layer_norm2"), p + "mlp.fc1")
        y = y * torch.sigmoid(1.702 * y) if cfg.act == "quick_gelu" else F.gelu(y)
        x = x + lin(y, p + "mlp.fc2")
    return ln(x[:, 0], "post_layernorm") @ w["visual_projection.weight"].T


def embeds_vjp(sd, cfg, pixel_values: torch.Tensor, g_embeds: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """(d image_embeds / d pixel_values)^T g_embeds in `dtype` (float64: the truth; float32: plain autograd's own error)."""
    pv = pixel_values.to(dtype).clone().requires_grad_(True)
    (clip_vision_embeds(sd, cfg, pv, dtype) * g_embeds.to(dtype)).sum().backward()
    return pv.grad


def cosine_losses(embeds: torch.Tensor, text_embed: torch.Tensor) -> torch.Tensor:
    t = text_embed.to(embeds.dtype).flatten()
    return 1 - (embeds @ t) / (embeds.norm(dim=1) * t.norm())


def text_guidance(sd, cfg, frames: torch.Tensor, text_embed: torch.Tensor, boxes=None):
    """-> (loss [n] = 1 - cos(E_I(window_i), text_embed), d sum_i loss_i / d frames [nf, 3, H, W]), float64."""
    fr = frames.to(torch.float64).clone().requires_grad_(True)
    pv = preprocess_windows(fr, boxes, cfg.image_size, cfg.image_mean, cfg.image_std)
    loss = cosine_losses(clip_vision_embeds(sd, cfg, pv), text_embed.to(torch.float64))
    loss.sum().backward()
    return loss.detach(), fr.grad
