"""Segment Anything edit masks (reference src/modules/mask_segmentation.py): what the ``transformers`` ``mask-generation``
pipeline does on a ``SamModel``, without ``transformers`` and without any hub access.

* the image encoder (a ViT, nearly all of the arithmetic) is the HIP engine ``hip.LocoSamEngine`` (csrc/samenc.hip);
* the prompt encoder and the mask decoder (about 4 M parameters) are the plain torch functions below, run on the device,
  or, with ``head="hip"`` / ``--mask_head hip``, the HIP engine ``hip.LocoSamHeadEngine`` (csrc/samdec.hip), which also
  scores and binarises the candidates for the generator's filters;
* ``MaskGenerator`` is the automatic mask generator of the pipeline with its defaults: one crop layer, a 32 x 32 point
  grid in batches of 64, the predicted-IoU and stability filters, boxes with the near-crop-edge filter, greedy box NMS.

``SAM(args, log_dir).mask_segmentation(image, resolution)`` keeps the reference's interface and writes ``mask/mask.pt``.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


# --------------------------------------------------------------------------------------------------------- geometry
@dataclass(frozen=True)
class SamVisionConfig:
    image_size: int = 1024
    patch_size: int = 16
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    mlp_dim: int = 3072
    window_size: int = 14
    global_attn_indexes: Tuple[int, ...] = (2, 5, 8, 11)
    output_channels: int = 256
    layer_norm_eps: float = 1e-6
    num_pos_feats: int = 128
    qkv_bias: bool = True

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads


@dataclass(frozen=True)
class SamDecoderConfig:
    hidden_size: int = 256
    num_hidden_layers: int = 2
    num_attention_heads: int = 8
    mlp_dim: int = 2048
    attention_downsample_rate: int = 2
    num_multimask_outputs: int = 3
    iou_head_depth: int = 3
    iou_head_hidden_dim: int = 256
    layer_norm_eps: float = 1e-6
    hidden_act: str = "relu"


@dataclass(frozen=True)
class SamConfig:
    vision: SamVisionConfig = field(default_factory=SamVisionConfig)
    decoder: SamDecoderConfig = field(default_factory=SamDecoderConfig)


VIT_B = SamVisionConfig()
VIT_L = SamVisionConfig(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, mlp_dim=4096,
                        global_attn_indexes=(5, 11, 17, 23))
VIT_H = SamVisionConfig(hidden_size=1280, num_hidden_layers=32, num_attention_heads=16, mlp_dim=5120,
                        global_attn_indexes=(7, 15, 23, 31))


def config_from_dict(config: dict) -> SamConfig:
    """A ``SamConfig`` from the ``config.json`` of a ``SamModel`` folder (missing entries: the defaults of transformers)."""
    v = dict(config.get("vision_config") or {})
    d = dict(config.get("mask_decoder_config") or {})
    p = dict(config.get("prompt_encoder_config") or {})
    for flag in ("use_abs_pos", "use_rel_pos"):
        if not v.get(flag, True):
            raise ValueError(f"vision_config.{flag} = false: the image encoder builds the SAM form (absolute + relative position)")
    if v.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"vision_config.hidden_act {v['hidden_act']!r}: the image encoder builds the erf gelu only")
    if v.get("num_channels", 3) != 3:
        raise ValueError("vision_config.num_channels must be 3")
    hidden = v.get("hidden_size", 768)
    mlp_dim = v.get("mlp_dim") or int(hidden * v.get("mlp_ratio", 4.0))
    vision = SamVisionConfig(
        image_size=v.get("image_size", 1024), patch_size=v.get("patch_size", 16), hidden_size=hidden,
        num_hidden_layers=v.get("num_hidden_layers", 12), num_attention_heads=v.get("num_attention_heads", 12), mlp_dim=mlp_dim,
        window_size=v.get("window_size", 14), global_attn_indexes=tuple(v.get("global_attn_indexes", (2, 5, 8, 11))),
        output_channels=v.get("output_channels", 256), layer_norm_eps=v.get("layer_norm_eps", 1e-6),
        num_pos_feats=v.get("num_pos_feats", 128), qkv_bias=v.get("qkv_bias", True))
    decoder = SamDecoderConfig(
        hidden_size=d.get("hidden_size", 256), num_hidden_layers=d.get("num_hidden_layers", 2),
        num_attention_heads=d.get("num_attention_heads", 8), mlp_dim=d.get("mlp_dim", 2048),
        attention_downsample_rate=d.get("attention_downsample_rate", 2), num_multimask_outputs=d.get("num_multimask_outputs", 3),
        iou_head_depth=d.get("iou_head_depth", 3), iou_head_hidden_dim=d.get("iou_head_hidden_dim", 256),
        layer_norm_eps=d.get("layer_norm_eps", 1e-6), hidden_act=d.get("hidden_act", "relu"))
    if p.get("hidden_size", decoder.hidden_size) != decoder.hidden_size or vision.output_channels != decoder.hidden_size:
        raise ValueError("prompt encoder hidden_size, mask decoder hidden_size and vision output_channels must agree")
    if 2 * vision.num_pos_feats != decoder.hidden_size:
        raise ValueError("vision_config.num_pos_feats must be half the prompt encoder's hidden_size")
    return SamConfig(vision, decoder)


def infer_config(sd: Dict[str, torch.Tensor]) -> SamConfig:
    """The geometry from a normalised state dict alone (a bare checkpoint without config.json).  Heads, window size and the
    global layers are read off the relative position tables; the decoder keeps the SAM constants its tensors do not fix."""
    V = "vision_encoder."
    pw = sd[V + "patch_embed.projection.weight"]
    hidden, patch = pw.shape[0], pw.shape[2]
    grid = sd[V + "pos_embed"].shape[1]
    depth = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith(V + "layers."))
    rel = [sd[V + f"layers.{i}.attn.rel_pos_h"].shape for i in range(depth)]
    head_dim = rel[0][1]
    glob = tuple(i for i in range(depth) if rel[i][0] == 2 * grid - 1)
    win = [(r[0] + 1) // 2 for i, r in enumerate(rel) if i not in glob]
    out_ch = sd[V + "neck.conv1.weight"].shape[0]
    vision = SamVisionConfig(image_size=grid * patch, patch_size=patch, hidden_size=hidden, num_hidden_layers=depth,
                             num_attention_heads=hidden // head_dim, mlp_dim=sd[V + "layers.0.mlp.lin1.weight"].shape[0],
                             window_size=win[0] if win else grid, global_attn_indexes=glob, output_channels=out_ch,
                             num_pos_feats=sd["shared_image_embedding.positional_embedding"].shape[1],
                             qkv_bias=(V + "layers.0.attn.qkv.bias") in sd)
    M = "mask_decoder."
    dl = 1 + max(int(k.split(".")[3]) for k in sd if k.startswith(M + "transformer.layers."))
    base = SamDecoderConfig()
    iou_depth = 2 + sum(1 for k in sd if k.startswith(M + "iou_prediction_head.layers.") and k.endswith(".weight"))
    decoder = SamDecoderConfig(
        hidden_size=out_ch, num_hidden_layers=dl, num_attention_heads=base.num_attention_heads,
        mlp_dim=sd[M + "transformer.layers.0.mlp.lin1.weight"].shape[0],
        attention_downsample_rate=out_ch // sd[M + "transformer.layers.0.cross_attn_token_to_image.q_proj.weight"].shape[0],
        num_multimask_outputs=sd[M + "mask_tokens.weight"].shape[0] - 1, iou_head_depth=iou_depth,
        iou_head_hidden_dim=sd[M + "iou_prediction_head.proj_in.weight"].shape[0])
    return SamConfig(vision, decoder)


# ----------------------------------------------------------------------------------------------------------- loader
_TOP = ("vision_encoder.", "prompt_encoder.", "mask_decoder.", "shared_image_embedding.")


def normalize_sam_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Keys in ``SamModel`` naming: wrapper prefixes (``model.``, ``sam.``, ``module.``) dropped, the tied positional matrix
    present under both of its names, the mask-prompt embedding (unused: no mask prompts) left out."""
    inner = sd.get("state_dict", sd) if isinstance(sd.get("state_dict", None), dict) else sd
    out = {}
    for k, v in inner.items():
        while not k.startswith(_TOP) and "." in k and k.split(".", 1)[0] in ("model", "sam", "module"):
            k = k.split(".", 1)[1]
        if not k.startswith(_TOP):
            raise ValueError(f"foreign key for a SamModel: {k}")
        if k.startswith("prompt_encoder.mask_embed."):
            continue
        out[k] = v
    a, b = "shared_image_embedding.positional_embedding", "prompt_encoder.shared_embedding.positional_embedding"
    if a not in out and b in out:
        out[a] = out[b]
    if b not in out and a in out:
        out[b] = out[a]
    return out


def vision_param_shapes(cfg: SamVisionConfig) -> Dict[str, Tuple[int, ...]]:
    """Names (without ``vision_encoder.``) and shapes the HIP engine's parameter table holds."""
    D, G, F_, C, hd, ps = cfg.hidden_size, cfg.grid, cfg.mlp_dim, cfg.output_channels, cfg.head_dim, cfg.patch_size
    s = {"patch_embed.projection.weight": (D, 3, ps, ps), "patch_embed.projection.bias": (D,), "pos_embed": (1, G, G, D)}
    for i in range(cfg.num_hidden_layers):
        rel = 2 * (G if i in cfg.global_attn_indexes else cfg.window_size) - 1
        p = f"layers.{i}."
        s.update({p + "layer_norm1.weight": (D,), p + "layer_norm1.bias": (D,), p + "attn.qkv.weight": (3 * D, D),
                  p + "attn.qkv.bias": (3 * D,), p + "attn.rel_pos_h": (rel, hd), p + "attn.rel_pos_w": (rel, hd),
                  p + "attn.proj.weight": (D, D), p + "attn.proj.bias": (D,), p + "layer_norm2.weight": (D,),
                  p + "layer_norm2.bias": (D,), p + "mlp.lin1.weight": (F_, D), p + "mlp.lin1.bias": (F_,),
                  p + "mlp.lin2.weight": (D, F_), p + "mlp.lin2.bias": (D,)})
    s.update({"neck.conv1.weight": (C, D, 1, 1), "neck.layer_norm1.weight": (C,), "neck.layer_norm1.bias": (C,),
              "neck.conv2.weight": (C, C, 3, 3), "neck.layer_norm2.weight": (C,), "neck.layer_norm2.bias": (C,)})
    return s


def vision_state_dict(sd: Dict[str, torch.Tensor], cfg: SamVisionConfig) -> Dict[str, torch.Tensor]:
    """The image encoder's part of a normalised state dict, checked against the geometry.  A relative position table of
    another length than 2 * size - 1 is refused: ``transformers`` would interpolate it, this engine does not."""
    V = "vision_encoder."
    got = {k[len(V):]: v for k, v in sd.items() if k.startswith(V)}
    want = vision_param_shapes(cfg)
    if not cfg.qkv_bias:
        for i in range(cfg.num_hidden_layers):
            got.setdefault(f"layers.{i}.attn.qkv.bias", torch.zeros(3 * cfg.hidden_size))
    missing, foreign = sorted(set(want) - set(got)), sorted(set(got) - set(want))
    if foreign:
        raise ValueError(f"foreign keys for the SAM image encoder: {foreign[:8]}")
    if missing:
        raise ValueError(f"missing keys of the SAM image encoder: {missing[:8]}" + (" ..." if len(missing) > 8 else ""))
    for k, shp in want.items():
        if tuple(got[k].shape) != shp:
            if ".rel_pos_" in k:
                raise ValueError(f"{k}: relative position table of {got[k].shape[0]} rows, the layer needs {shp[0]} "
                                 "(2 * size - 1); interpolating tables is not supported")
            raise ValueError(f"{k}: shape {tuple(got[k].shape)}, expected {shp}")
    return got


def head_param_names(cfg: SamConfig) -> List[str]:
    """Names of the prompt encoder / mask decoder parameters the torch functions read."""
    d = cfg.decoder
    n = ["shared_image_embedding.positional_embedding", "prompt_encoder.no_mask_embed.weight",
         "prompt_encoder.not_a_point_embed.weight", "prompt_encoder.point_embed.0.weight", "prompt_encoder.point_embed.1.weight",
         "mask_decoder.iou_token.weight", "mask_decoder.mask_tokens.weight"]
    M = "mask_decoder."

    def lin(p):
        n.extend([p + ".weight", p + ".bias"])

    def attn(p):
        for q in ("q_proj", "k_proj", "v_proj", "out_proj"):
            lin(p + "." + q)
    for i in range(d.num_hidden_layers):
        p = M + f"transformer.layers.{i}."
        for a in ("self_attn", "cross_attn_token_to_image", "cross_attn_image_to_token"):
            attn(p + a)
        for j in range(1, 5):
            lin(p + f"layer_norm{j}")
        lin(p + "mlp.lin1"); lin(p + "mlp.lin2")
    attn(M + "transformer.final_attn_token_to_image")
    lin(M + "transformer.layer_norm_final_attn")
    lin(M + "upscale_conv1"); lin(M + "upscale_conv2"); lin(M + "upscale_layer_norm")
    for i in range(d.num_multimask_outputs + 1):
        p = M + f"output_hypernetworks_mlps.{i}."
        lin(p + "proj_in"); lin(p + "layers.0"); lin(p + "proj_out")
    p = M + "iou_prediction_head."
    lin(p + "proj_in"); lin(p + "proj_out")
    for j in range(d.iou_head_depth - 2):
        lin(p + f"layers.{j}")
    return n


def head_param_shapes(cfg: SamConfig) -> Dict[str, Tuple[int, ...]]:
    """Names (in SamModel naming) and shapes the HIP head's parameter table holds (hip.LocoSamHeadEngine): what
    ``head_param_names`` lists, less ``point_embed.0`` (the background point, which no prompt here uses)."""
    d, C = cfg.decoder, cfg.decoder.hidden_size
    Ci, nm, hid = C // d.attention_downsample_rate, d.num_multimask_outputs + 1, d.iou_head_hidden_dim
    s: Dict[str, Tuple[int, ...]] = {
        "shared_image_embedding.positional_embedding": (2, C // 2), "prompt_encoder.no_mask_embed.weight": (1, C),
        "prompt_encoder.not_a_point_embed.weight": (1, C), "prompt_encoder.point_embed.1.weight": (1, C),
        "mask_decoder.iou_token.weight": (1, C), "mask_decoder.mask_tokens.weight": (nm, C)}
    M = "mask_decoder."

    def lin(p, o, i):
        s[p + ".weight"], s[p + ".bias"] = (o, i), (o,)

    def attn(p, inner):
        for q in ("q_proj", "k_proj", "v_proj"):
            lin(p + "." + q, inner, C)
        lin(p + ".out_proj", C, inner)
    for i in range(d.num_hidden_layers):
        p = M + f"transformer.layers.{i}."
        attn(p + "self_attn", C)
        attn(p + "cross_attn_token_to_image", Ci)
        attn(p + "cross_attn_image_to_token", Ci)
        for j in range(1, 5):
            s[p + f"layer_norm{j}.weight"], s[p + f"layer_norm{j}.bias"] = (C,), (C,)
        lin(p + "mlp.lin1", d.mlp_dim, C)
        lin(p + "mlp.lin2", C, d.mlp_dim)
    attn(M + "transformer.final_attn_token_to_image", Ci)
    s[M + "transformer.layer_norm_final_attn.weight"], s[M + "transformer.layer_norm_final_attn.bias"] = (C,), (C,)
    s[M + "upscale_conv1.weight"], s[M + "upscale_conv1.bias"] = (C, C // 4, 2, 2), (C // 4,)
    s[M + "upscale_conv2.weight"], s[M + "upscale_conv2.bias"] = (C // 4, C // 8, 2, 2), (C // 8,)
    s[M + "upscale_layer_norm.weight"], s[M + "upscale_layer_norm.bias"] = (C // 4,), (C // 4,)
    for i in range(nm):
        p = M + f"output_hypernetworks_mlps.{i}."
        lin(p + "proj_in", C, C)
        lin(p + "layers.0", C, C)
        lin(p + "proj_out", C // 8, C)
    p = M + "iou_prediction_head."
    lin(p + "proj_in", hid, C)
    for j in range(d.iou_head_depth - 2):
        lin(p + f"layers.{j}", hid, hid)
    lin(p + "proj_out", nm, hid)
    return s


def head_state_dict(sd: Dict[str, torch.Tensor], cfg: SamConfig) -> Dict[str, torch.Tensor]:
    """The HIP head's part of a normalised state dict, checked against the geometry."""
    want = head_param_shapes(cfg)
    missing = sorted(k for k in want if k not in sd)
    if missing:
        raise ValueError(f"missing keys of the SAM prompt encoder / mask decoder: {missing[:8]}" + (" ..." if len(missing) > 8 else ""))
    for k, shp in want.items():
        if tuple(sd[k].shape) != shp:
            raise ValueError(f"{k}: shape {tuple(sd[k].shape)}, expected {shp}")
    return {k: sd[k] for k in want}


def load_sam(path_or_sd) -> Tuple[SamConfig, Dict[str, torch.Tensor]]:
    """-> (geometry, normalised state dict) from a local ``SamModel`` folder (``config.json`` + ``model.safetensors`` or
    ``pytorch_model.bin``), a checkpoint file, or a bare state dict.  Local files only."""
    from .text_encoder import _read_state_dict
    config = None
    if isinstance(path_or_sd, dict):
        sd = path_or_sd
    else:
        path = path_or_sd
        if os.path.isdir(path):
            cj = os.path.join(path, "config.json")
            if os.path.exists(cj):
                with open(cj) as f:
                    config = json.load(f)
            for fn in ("model.safetensors", "pytorch_model.bin"):
                if os.path.exists(os.path.join(path, fn)):
                    sd = _read_state_dict(os.path.join(path, fn))
                    break
            else:
                raise FileNotFoundError(f"{path}: no model.safetensors or pytorch_model.bin")
        elif os.path.isfile(path):
            sd = _read_state_dict(path)
        else:
            raise FileNotFoundError(f"{path}: --mask_model_path must name a local SamModel folder or checkpoint file "
                                    "(nothing is downloaded)")
    sd = normalize_sam_state_dict(sd)
    cfg = config_from_dict(config) if config is not None else infer_config(sd)
    vision_state_dict(sd, cfg.vision)
    missing = [k for k in head_param_names(cfg) if k not in sd]
    if missing:
        raise ValueError(f"missing keys of the SAM prompt encoder / mask decoder: {missing[:8]}" + (" ..." if len(missing) > 8 else ""))
    return cfg, sd


# ---------------------------------------------------------------------------------------------------- preprocessing
def preprocess_shape(old_hw: Tuple[int, int], longest_edge: int) -> Tuple[int, int]:
    h, w = old_hw
    scale = longest_edge * 1.0 / max(h, w)
    return int(h * scale + 0.5), int(w * scale + 0.5)


def to_uint8_image(image) -> np.ndarray:
    """PIL image, uint8 [H, W, 3] array, or a float image tensor [3, H, W] / [1, 3, H, W] in [0, 1] -> uint8 [H, W, 3]."""
    if isinstance(image, torch.Tensor):
        t = image.detach().float().cpu()
        if t.dim() == 4:
            t = t[0]
        if t.shape[0] == 3:
            t = t.permute(1, 2, 0)
        if t.max() <= 1.0 + 1e-6:
            t = t.clamp(0, 1) * 255.0
        return t.round().to(torch.uint8).numpy()
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise ValueError("image arrays must be uint8 [H, W, 3]")
        return image
    return np.asarray(image.convert("RGB"))


def preprocess(image, image_size: int):
    """What ``SamImageProcessor`` does: longest edge to ``image_size`` with PIL bilinear, / 255, ImageNet mean / std,
    zero-pad at the bottom and right.  -> (pixel_values [3, S, S] fp32, original (h, w), resized (h, w))."""
    from PIL import Image
    arr = to_uint8_image(image)
    oh, ow = arr.shape[:2]
    nh, nw = preprocess_shape((oh, ow), image_size)
    res = np.asarray(Image.fromarray(arr).resize((nw, nh), resample=Image.BILINEAR))
    x = res.astype(np.float32) * np.float32(1 / 255)
    x = (x - np.asarray(IMAGENET_MEAN, dtype=np.float32)) / np.asarray(IMAGENET_STD, dtype=np.float32)
    pv = np.zeros((3, image_size, image_size), dtype=np.float32)
    pv[:, :nh, :nw] = x.transpose(2, 0, 1)
    return torch.from_numpy(pv), (oh, ow), (nh, nw)


# -------------------------------------------------------------------------- prompt encoder + mask decoder (torch)
def _channel_ln(x, w, b, eps=1e-6):
    """LayerNorm over the channels of [B, C, H, W] at each pixel (SamLayerNorm channels_first)."""
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), w, b, eps).permute(0, 3, 1, 2)


class SamHead:
    """Prompt encoder and mask decoder of ``SamModel`` as functions of the state dict's tensors (point prompts, no box or
    mask prompts, ``multimask_output=True``), on ``device`` in ``dtype``."""

    def __init__(self, cfg: SamConfig, sd: Dict[str, torch.Tensor], device="cpu", dtype=torch.float32):
        self.cfg, self.device, self.dtype = cfg, torch.device(device), dtype
        self.p = {k: sd[k].detach().to(device=self.device, dtype=dtype) for k in head_param_names(cfg)}
        self.act = {"relu": F.relu, "gelu": F.gelu}[cfg.decoder.hidden_act]

    # random-Fourier features of coordinates in [0, 1]^2 from the shared positional matrix
    def _pe(self, coords01):
        c = (2 * coords01 - 1).to(self.dtype) @ self.p["shared_image_embedding.positional_embedding"]
        c = 2 * np.pi * c
        return torch.cat([torch.sin(c), torch.cos(c)], dim=-1)

    def image_pe(self):
        """[1, C, G, G]: the positional encoding of the embedding grid."""
        G = self.cfg.vision.grid
        ones = torch.ones(G, G, device=self.device, dtype=self.dtype)
        y = (ones.cumsum(0) - 0.5) / G
        x = (ones.cumsum(1) - 0.5) / G
        return self._pe(torch.stack([x, y], dim=-1)).permute(2, 0, 1).unsqueeze(0)

    def embed_points(self, points):
        """points [P, 2] (x, y) in the resized image's pixel frame, one foreground point per prompt -> sparse [P, 2, C]
        (the point + the padding point that stands for "no box")."""
        S = self.cfg.vision.image_size
        pts = points.to(self.device) + 0.5
        pts = torch.stack([pts, torch.zeros_like(pts)], dim=1)                       # [P, 2, 2]
        pts = torch.stack([pts[..., 0] / S, pts[..., 1] / S], dim=-1)
        emb = self._pe(pts)
        fg = emb[:, 0] + self.p["prompt_encoder.point_embed.1.weight"]
        pad = self.p["prompt_encoder.not_a_point_embed.weight"].expand(emb.shape[0], -1)
        return torch.stack([fg, pad], dim=1)

    def _lin(self, x, name):
        return F.linear(x, self.p[name + ".weight"], self.p[name + ".bias"])

    def _ln(self, x, name, eps):
        return F.layer_norm(x, (x.shape[-1],), self.p[name + ".weight"], self.p[name + ".bias"], eps)

    def _attn(self, name, q, k, v):
        H = self.cfg.decoder.num_attention_heads
        q, k, v = self._lin(q, name + ".q_proj"), self._lin(k, name + ".k_proj"), self._lin(v, name + ".v_proj")
        B, _, Ci = q.shape

        def heads(t):
            return t.reshape(B, t.shape[1], H, Ci // H).transpose(1, 2)
        q, k, v = heads(q), heads(k), heads(v)
        w = torch.softmax((q @ k.transpose(2, 3)) * (Ci // H) ** -0.5, dim=-1)
        o = (w @ v).transpose(1, 2).reshape(B, -1, Ci)
        return self._lin(o, name + ".out_proj")

    def _mlp3(self, x, name, depth=3):
        x = F.relu(self._lin(x, name + ".proj_in"))
        for j in range(depth - 2):
            x = F.relu(self._lin(x, f"{name}.layers.{j}"))
        return self._lin(x, name + ".proj_out")

    def decode(self, image_embeddings, sparse, image_pe=None):
        """image_embeddings [1, C, G, G], sparse [P, n, C] -> (pred_masks [P, 3, 4G, 4G], iou_scores [P, 3])."""
        d, p = self.cfg.decoder, self.p
        M = "mask_decoder."
        P = sparse.shape[0]
        _, C, G, _ = image_embeddings.shape
        nm = d.num_multimask_outputs + 1
        out_tok = torch.cat([p[M + "iou_token.weight"], p[M + "mask_tokens.weight"]], dim=0)
        tokens = torch.cat([out_tok.unsqueeze(0).expand(P, -1, -1), sparse], dim=1)
        src = image_embeddings.to(self.dtype) + p["prompt_encoder.no_mask_embed.weight"].reshape(1, -1, 1, 1)
        keys = src.flatten(2).transpose(1, 2).expand(P, -1, -1)
        pos = (self.image_pe() if image_pe is None else image_pe).flatten(2).transpose(1, 2).expand(P, -1, -1)
        queries, eps = tokens, d.layer_norm_eps
        for i in range(d.num_hidden_layers):
            L = M + f"transformer.layers.{i}."
            if i == 0:
                queries = self._attn(L + "self_attn", queries, queries, queries)
            else:
                q = queries + tokens
                queries = queries + self._attn(L + "self_attn", q, q, queries)
            queries = self._ln(queries, L + "layer_norm1", eps)
            queries = queries + self._attn(L + "cross_attn_token_to_image", queries + tokens, keys + pos, keys)
            queries = self._ln(queries, L + "layer_norm2", eps)
            queries = queries + self._lin(self.act(self._lin(queries, L + "mlp.lin1")), L + "mlp.lin2")
            queries = self._ln(queries, L + "layer_norm3", eps)
            keys = keys + self._attn(L + "cross_attn_image_to_token", keys + pos, queries + tokens, queries)
            keys = self._ln(keys, L + "layer_norm4", eps)
        queries = queries + self._attn(M + "transformer.final_attn_token_to_image", queries + tokens, keys + pos, keys)
        queries = self._ln(queries, M + "transformer.layer_norm_final_attn", 1e-5)
        iou_tok, mask_tok = queries[:, 0], queries[:, 1:1 + nm]
        up = keys.transpose(1, 2).reshape(P, C, G, G)
        up = F.conv_transpose2d(up, p[M + "upscale_conv1.weight"], p[M + "upscale_conv1.bias"], stride=2)
        up = F.gelu(_channel_ln(up, p[M + "upscale_layer_norm.weight"], p[M + "upscale_layer_norm.bias"]))
        up = F.gelu(F.conv_transpose2d(up, p[M + "upscale_conv2.weight"], p[M + "upscale_conv2.bias"], stride=2))
        hyper = torch.stack([self._mlp3(mask_tok[:, i], M + f"output_hypernetworks_mlps.{i}") for i in range(nm)], dim=1)
        masks = (hyper @ up.flatten(2)).reshape(P, nm, up.shape[2], up.shape[3])
        iou = self._mlp3(iou_tok, M + "iou_prediction_head", d.iou_head_depth)
        return masks[:, 1:], iou[:, 1:]                       # multimask_output=True drops token 0

    def predict(self, image_embeddings, points, image_pe=None):
        return self.decode(image_embeddings, self.embed_points(points), image_pe)


def prompt_coords(points, image_size: int) -> torch.Tensor:
    """points [P, 2] (x, y) in the resized image's pixel frame -> what ``SamHead.embed_points`` feeds the random-Fourier
    features for the foreground point: 2 (p + 0.5) / S - 1 in the points' own precision, then fp32."""
    pts = torch.as_tensor(points) + 0.5
    pts = torch.stack([pts[..., 0] / image_size, pts[..., 1] / image_size], dim=-1)
    return (2 * pts - 1).to(torch.float32)


class SamHeadHip:
    """``SamHead`` on the HIP engine ``hip.LocoSamHeadEngine`` (csrc/samdec.hip): the same ``cfg`` / ``image_pe`` / ``predict``
    that ``MaskGenerator.generate`` uses, plus ``score`` / ``binarize`` for its filters.  Exact fp32, no torch fallback."""

    def __init__(self, cfg: SamConfig, sd: Dict[str, torch.Tensor], device="cuda:0", max_prompts: int = 64):
        from .hip import LocoSamHeadEngine
        self.cfg = cfg
        self.engine = LocoSamHeadEngine(cfg, max_prompts=max_prompts, device=torch.device(device))
        self.engine.load_state_dict(head_state_dict(sd, cfg))
        self.device = self.engine.device
        self._seen = None

    def image_pe(self):
        """None: the engine computes the grid's positional encoding itself in ``set_image``."""
        return None

    def set_image(self, image_embeddings):
        self.engine.set_image(image_embeddings)
        self._seen = (image_embeddings, getattr(image_embeddings, "_version", None))

    def predict(self, image_embeddings, points, image_pe=None):
        """image_embeddings [1, C, G, G], points [P, 2] -> (pred_masks [P, 3, 4G, 4G], iou_scores [P, 3]).  The image side is
        set up again only when the embedding tensor is not the one last seen (or was written to since)."""
        if self._seen is None or self._seen[0] is not image_embeddings or self._seen[1] != getattr(image_embeddings, "_version", None):
            self.set_image(image_embeddings)
        return self.engine.predict(prompt_coords(points, self.cfg.vision.image_size))

    def score(self, low_res, original_size, reshaped_size, image_size, mask_threshold, offset):
        return self.engine.score(low_res, original_size, reshaped_size, image_size, mask_threshold, offset)

    def binarize(self, low_res, rows, original_size, reshaped_size, image_size, mask_threshold):
        return self.engine.binarize(low_res, rows, original_size, reshaped_size, image_size, mask_threshold)


# ---------------------------------------------------------------------------------------- automatic mask generator
def build_point_grid(n_per_side: int) -> np.ndarray:
    offset = 1 / (2 * n_per_side)
    side = np.linspace(offset, 1 - offset, n_per_side)
    return np.stack([np.tile(side[None, :], (n_per_side, 1)), np.tile(side[:, None], (1, n_per_side))], axis=-1).reshape(-1, 2)


def stability_score(masks, mask_threshold, offset):
    inter = (masks > (mask_threshold + offset)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    union = (masks > (mask_threshold - offset)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    return inter / union


def mask_to_box(masks):
    """bool [N, H, W] -> XYXY boxes [N, 4] (inclusive edges), [0, 0, 0, 0] for an empty mask."""
    if masks.numel() == 0:
        return torch.zeros(*masks.shape[:-2], 4, device=masks.device)
    h, w = masks.shape[-2:]
    in_h, _ = torch.max(masks, dim=-1)
    hc = in_h * torch.arange(h, device=masks.device)[None, :]
    bottom, _ = torch.max(hc, dim=-1)
    top, _ = torch.min(hc + h * (~in_h), dim=-1)
    in_w, _ = torch.max(masks, dim=-2)
    wc = in_w * torch.arange(w, device=masks.device)[None, :]
    right, _ = torch.max(wc, dim=-1)
    left, _ = torch.min(wc + w * (~in_w), dim=-1)
    empty = (right < left) | (bottom < top)
    return torch.stack([left, top, right, bottom], dim=-1) * (~empty).unsqueeze(-1)


def box_near_crop_edge(boxes, crop_box, orig_box, atol=20.0):
    crop = torch.as_tensor(crop_box, dtype=torch.float, device=boxes.device)
    orig = torch.as_tensor(orig_box, dtype=torch.float, device=boxes.device)
    left, top = crop_box[0], crop_box[1]
    b = (boxes + torch.tensor([[left, top, left, top]], device=boxes.device)).float()
    near_crop = torch.isclose(b, crop[None, :], atol=atol, rtol=0)
    near_image = torch.isclose(b, orig[None, :], atol=atol, rtol=0)
    return torch.any(near_crop & ~near_image, dim=1)


def box_iou(a, b):
    """IoU of one XYXY box against [N, 4] boxes (areas (x2 - x1)(y2 - y1), as torchvision)."""
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = (torch.minimum(a[2], b[:, 2]) - torch.maximum(a[0], b[:, 0])).clamp(min=0)
    h = (torch.minimum(a[3], b[:, 3]) - torch.maximum(a[1], b[:, 1])).clamp(min=0)
    inter = w * h
    return inter / (area_a + area_b - inter)


def greedy_nms(boxes, scores, iou_threshold: float) -> torch.Tensor:
    """Indexes kept by greedy box NMS in descending score order (what ``torchvision.ops.nms`` returns)."""
    boxes, scores = boxes.float().cpu(), scores.float().cpu()
    order = torch.sort(scores, descending=True, stable=True).indices.tolist()
    keep: List[int] = []
    dead = [False] * len(order)
    for a, i in enumerate(order):
        if dead[a]:
            continue
        keep.append(i)
        rest = order[a + 1:]
        if rest:
            iou = box_iou(boxes[i], boxes[rest])
            for off in torch.nonzero(iou > iou_threshold).flatten().tolist():
                dead[a + 1 + off] = True
    return torch.tensor(keep, dtype=torch.long)


class MaskGenerator:
    """The automatic mask generator of the ``mask-generation`` pipeline at its defaults (one crop layer = the whole image)."""

    def __init__(self, points_per_side: int = 32, points_per_batch: int = 64, pred_iou_thresh: float = 0.88,
                 stability_score_thresh: float = 0.95, stability_score_offset: float = 1, mask_threshold: float = 0.0,
                 crops_nms_thresh: float = 0.7):
        self.points_per_side, self.points_per_batch = points_per_side, points_per_batch
        self.pred_iou_thresh, self.stability_score_thresh = pred_iou_thresh, stability_score_thresh
        self.stability_score_offset, self.mask_threshold, self.crops_nms_thresh = stability_score_offset, mask_threshold, crops_nms_thresh

    def grid_points(self, original_size, image_size: int) -> torch.Tensor:
        """[n, 2] float64 (x, y) in the resized image's pixel frame."""
        oh, ow = original_size
        nh, nw = preprocess_shape((oh, ow), image_size)
        pts = build_point_grid(self.points_per_side) * np.array([[ow, oh]])
        pts = pts.astype(float)
        pts[..., 0] = pts[..., 0] * (nw / ow)
        pts[..., 1] = pts[..., 1] * (nh / oh)
        return torch.from_numpy(pts)

    @staticmethod
    def upsample(low_res, original_size, reshaped_size, image_size: int):
        """Low-resolution logits [P, 3, h, w] -> [P, 3, H, W] at the original size: bilinear to the padded size, crop, bilinear."""
        m = F.interpolate(low_res, (image_size, image_size), mode="bilinear", align_corners=False)
        m = m[..., : reshaped_size[0], : reshaped_size[1]]
        return F.interpolate(m, tuple(original_size), mode="bilinear", align_corners=False)

    def filter_batch(self, low_res, iou_scores, original_size, reshaped_size, image_size: int, crop_box=None, scorer=None):
        """One decoder batch -> (masks bool [k, H, W], scores [k], boxes [k, 4]) after the score, stability and edge filters.
        crop_box [left, top, right, bottom]: the part of the image the batch saw (None: all of it, the one crop layer of the
        defaults); the masks come back padded to the image, the boxes stay in the crop's frame as in the pipeline.
        scorer (``SamHeadHip`` or anything with its ``score`` / ``binarize``): the filters run on its counts and boxes, taken
        at the original size without storing the upsampled logits, and only the survivors are binarised."""
        oh, ow = original_size
        crop = [0, 0, ow, oh] if crop_box is None else [int(v) for v in crop_box]
        left, top, right, bottom = crop
        if scorer is not None:
            size = (bottom - top, right - left)
            low = low_res.flatten(0, 1)
            counts, boxes = scorer.score(low, size, reshaped_size, image_size, self.mask_threshold, self.stability_score_offset)
            scores = iou_scores.flatten(0, 1).to(counts.device)
            keep = torch.ones(low.shape[0], dtype=torch.bool, device=counts.device)
            if self.pred_iou_thresh > 0.0:
                keep = keep & (scores > self.pred_iou_thresh)
            if self.stability_score_thresh > 0.0:
                keep = keep & ((counts[:, 0] / counts[:, 1]) > self.stability_score_thresh)
            boxes = boxes.to(torch.int64)
            keep = keep & ~box_near_crop_edge(boxes, crop, [0, 0, ow, oh])
            rows = torch.nonzero(keep).flatten()
            masks = scorer.binarize(low, rows, size, reshaped_size, image_size, self.mask_threshold)
            if crop != [0, 0, ow, oh]:
                masks = F.pad(masks, (left, ow - right, top, oh - bottom), value=False)
            return masks, scores[rows], boxes[rows]
        masks = self.upsample(low_res, (bottom - top, right - left), reshaped_size, image_size).flatten(0, 1)
        scores = iou_scores.flatten(0, 1).to(masks.device)
        keep = torch.ones(masks.shape[0], dtype=torch.bool, device=masks.device)
        if self.pred_iou_thresh > 0.0:
            keep = keep & (scores > self.pred_iou_thresh)
        if self.stability_score_thresh > 0.0:
            keep = keep & (stability_score(masks, self.mask_threshold, self.stability_score_offset) > self.stability_score_thresh)
        scores, masks = scores[keep], masks[keep] > self.mask_threshold
        boxes = mask_to_box(masks)
        keep = ~box_near_crop_edge(boxes, crop, [0, 0, ow, oh])
        masks = masks[keep]
        if crop != [0, 0, ow, oh]:
            masks = F.pad(masks, (left, ow - right, top, oh - bottom), value=False)
        return masks, scores[keep], boxes[keep]

    def finish(self, batches):
        """NMS over the filtered batches -> (masks bool [N, H, W], scores [N], boxes [N, 4]) in descending score order."""
        masks = torch.cat([b[0] for b in batches])
        scores = torch.cat([b[1] for b in batches])
        boxes = torch.cat([b[2] for b in batches])
        keep = greedy_nms(boxes, scores, self.crops_nms_thresh).to(masks.device)
        return masks[keep], scores[keep], boxes[keep]

    def generate(self, head, image_embeddings, original_size, reshaped_size, scorer=None):
        S = head.cfg.vision.image_size
        pts = self.grid_points(original_size, S)
        pe = head.image_pe()
        batches = []
        for i in range(0, pts.shape[0], self.points_per_batch):
            low, iou = head.predict(image_embeddings, pts[i: i + self.points_per_batch], pe)
            if scorer is None:
                batches.append(self.filter_batch(low, iou, original_size, reshaped_size, S))
            else:
                batches.append(self.filter_batch(low, iou, original_size, reshaped_size, S, scorer=scorer))
        return self.finish(batches)


# ------------------------------------------------------------------------------------------------------ the driver
class SAM(object):
    """``SAM(args, log_dir).mask_segmentation(image, resolution)`` of the reference: bool masks [N, res, res], written to
    ``<log_dir>/mask/mask.pt`` with the overlay PNGs.  The model comes from ``args.mask_model_path`` (a local folder or file)."""

    HEADS = ("torch", "hip")

    def __init__(self, args, log_dir, head=None, **generator_kwargs):
        """head: "torch" (``SamHead`` and the torch filters, the default) or "hip" (``SamHeadHip``: decoder, scoring and
        binarisation on csrc/samdec.hip); None: ``args.mask_head`` (--mask_head), "torch" without it."""
        from .hip import LocoSamEngine
        head = head if head is not None else (getattr(args, "mask_head", "") or "torch")
        if head not in self.HEADS:
            raise ValueError(f"mask head {head!r}: one of {self.HEADS}")
        path = getattr(args, "mask_model_path", "")
        if not path:
            raise ValueError("--mask_model_path is empty: SAM needs a local SamModel folder or checkpoint")
        self.args = args
        self.device = torch.device(getattr(args, "device", "cuda:0"))
        self.cfg, sd = load_sam(path)
        self.engine = LocoSamEngine(self.cfg.vision, device=self.device)
        self.engine.load_state_dict(vision_state_dict(sd, self.cfg.vision))
        self.head_kind = head
        self.generator = MaskGenerator(**generator_kwargs)
        if head == "hip":
            self.head = SamHeadHip(self.cfg, sd, device=self.engine.device, max_prompts=self.generator.points_per_batch)
            self.scorer = self.head
        else:
            self.head = SamHead(self.cfg, sd, device=self.engine.device)
            self.scorer = None
        self.log_dir = os.path.join(log_dir, "mask")
        self.transparency = 0.4
        os.makedirs(self.log_dir, exist_ok=True)
        self.last_scores = None
        self.last_timing: Dict[str, float] = {}

    @torch.no_grad()
    def segment(self, image):
        """-> (masks bool [N, H, W] on the device, scores [N], boxes [N, 4]) at the image's own size."""
        import time
        S = self.cfg.vision.image_size
        pv, orig, resh = preprocess(image, S)
        torch.cuda.synchronize(self.engine.device)
        t0 = time.perf_counter()
        emb = self.engine.encode(pv)
        torch.cuda.synchronize(self.engine.device)
        t1 = time.perf_counter()
        if self.scorer is None:
            out = self.generator.generate(self.head, emb, orig, resh)
        else:
            out = self.generator.generate(self.head, emb, orig, resh, scorer=self.scorer)
        torch.cuda.synchronize(self.engine.device)
        t2 = time.perf_counter()
        self.last_timing = {"encoder_ms": (t1 - t0) * 1e3, "decoder_generator_ms": (t2 - t1) * 1e3}
        return out

    def mask_segmentation(self, image, resolution=64):
        masks, scores, _ = self.segment(image)
        if masks.shape[0] == 0:
            raise RuntimeError("SAM: no mask passed the predicted-IoU / stability filters")
        self.last_scores = scores.cpu()
        masks = masks.cpu()
        self.show_masks_on_image(image, masks.numpy())
        # the reference's resampling: nearest neighbour (interpolate's default) to the square, then rounded to bool
        small = F.interpolate(masks[:, None].float(), size=(resolution, resolution), mode="nearest")[:, 0]
        masks = small.round().bool()
        torch.save(masks, os.path.join(self.log_dir, "mask.pt"))
        return masks

    def _tint(self, canvas, mask, colour):
        """In place inside `mask`: half of the alpha blend of the canvas with `colour`, truncated to uint8 (the look of
        the reference's overlays, which halve the blend)."""
        a = np.float32(self.transparency)
        inside = canvas[mask].astype(np.float32)
        canvas[mask] = (0.5 * ((1 - a) * inside + a * colour.astype(np.float32))).astype(np.uint8)

    def show_masks_on_image(self, raw_image, masks):
        """mask_{i}.png for every mask of more than --filter_mask pixels, each in a colour of its own, and total_mask.png
        with all of them (PIL; the colours come from a seeded generator, so a rerun writes the same files)."""
        from PIL import Image
        base = to_uint8_image(raw_image)
        total = base.copy()
        rng = np.random.default_rng(0)
        least = getattr(self.args, "filter_mask", 0)
        for i, mask in enumerate(masks):
            if mask.sum() <= least:
                continue
            colour = 255 * rng.random(3)
            single = base.copy()
            self._tint(single, mask, colour)
            self._tint(total, mask, colour)
            Image.fromarray(single).save(os.path.join(self.log_dir, f"mask_{i}.png"))
        Image.fromarray(total).save(os.path.join(self.log_dir, "total_mask.png"))


def wants_segmentation(args) -> bool:
    """Whether a driver is to produce mask/mask.pt itself when it is missing: --mask_model_path (Segment Anything) or
    --mask_prompt_model_path (CLIPSeg, one mask per entry of --mask_prompts)."""
    return bool(getattr(args, "mask_model_path", "") or getattr(args, "mask_prompt_model_path", ""))


def segment_for_driver(args, result_folder, sharder, image_fn, resolution: int):
    """The drivers' segmentation step when mask/mask.pt is missing and a mask model is set (``wants_segmentation``): every rank
    produces the image (the sampler is the same flow on all of them), rank 0 segments it -- Segment Anything with
    --mask_model_path, the prompt masker (prompt_mask.prompt_masks_for_driver) with --mask_prompt_model_path -- and writes the
    cache, every rank receives the masks (bool [N, res, res], on the host); a failure on rank 0 raises on all."""
    image = image_fn()
    masks, err = None, None
    if sharder.is_main:
        try:
            if getattr(args, "mask_prompt_model_path", ""):
                from .prompt_mask import prompt_masks_for_driver
                masks = prompt_masks_for_driver(args, result_folder, image, resolution)
            else:
                masks = SAM(args, result_folder).mask_segmentation(image, resolution=resolution)
        except Exception as ex:
            if not sharder.active:
                raise
            err = repr(ex)
    if sharder.active:
        masks, err = sharder.agree((masks, err))
        if err is not None:
            raise RuntimeError(f"rank 0 could not segment the image: {err}")
    return masks
