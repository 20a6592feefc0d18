"""CLIP scores of the text-guided edits: did an edit do what the edit prompt asked, and what did it preserve.

* ``load_clip(path)``: a ``CLIPModel`` folder of transformers (``config.json`` + ``model.safetensors`` or
  ``pytorch_model.bin``) or one state-dict file -> a ``ClipScorer``: the image tower on the HIP engine
  (``hip.LocoClipVisionEngine``, ``csrc/clipvis.hip``), the text tower on ``hip.LocoTextEngine`` (``csrc/textenc.hip``), the
  tokenizer ``text_encoder.CLIPTokenizer``.  Keys are those of transformers (``vision_model.*``, ``text_model.*``,
  ``visual_projection.weight``, ``text_projection.weight``); OpenCLIP naming is refused.
* ``ClipScorer.image_embeds(frames)``: uint8 frames [n, H, W, 3] -> the un-normalised ``image_embeds`` [n, P] of
  ``CLIPVisionModelWithProjection``.  Two preprocessing modes: ``"device"`` resizes on the GPU in float arithmetic (the
  engine's ``preprocess``; yardstick: torch's antialiased bicubic ``interpolate`` in float64), ``"pil"`` resizes on the host
  with PIL itself, which rounds to uint8 after each pass -- that input equals ``CLIPImageProcessor``'s exactly.  Where a resize
  happens the two differ by rel-L2 0.008-0.009 of the normalised pixel values and at most 1.1 grey levels (the smooth-plus-noise
  images of tests/test_clip_score_host.py at 64^2, 256^2, 512^2 and 96 x 80, measured on the CPU); without a resize they agree
  to 1e-7.
* ``ClipScorer.text_embeds(prompts)``: the ``text_embeds`` of ``CLIPTextModelWithProjection``: the final-LayerNorm state at
  the first EOS position times ``text_projection`` (that small product on the host in float64, rounded to fp32).
* ``ClipScorer.score(frames, original_index, for_prompt, edit_prompt)`` -> per frame ``clip_for`` / ``clip_edit`` (image-text
  cosine with the source / the edit prompt), ``image_sim`` (cosine with the original frame) and ``directional``
  (cos(E(frame) - E(original), E(edit prompt) - E(source prompt))); cosines in float64 from the fp32 embeddings.

No published CLIP weights are available offline: the towers are pinned to transformers with seeded random weights, unpinned
against published weights.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import text_encoder as te

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PREPROCESS_MODES = ("pil", "device")


@dataclass(frozen=True)
class ClipVisionConfig:
    image_size: int = 224
    patch_size: int = 14
    width: int = 1024
    layers: int = 24
    heads: int = 16
    mlp_dim: int = 4096
    projection_dim: int = 768
    act: str = "quick_gelu"         # "quick_gelu" x sigmoid(1.702 x) (the OpenAI checkpoints) | "gelu" exact erf
    ln_eps: float = 1e-5
    image_mean: Tuple[float, float, float] = CLIP_MEAN
    image_std: Tuple[float, float, float] = CLIP_STD


CLIP_VIT_L14 = ClipVisionConfig()
CLIP_VIT_B32 = ClipVisionConfig(patch_size=32, width=768, layers=12, heads=12, mlp_dim=3072, projection_dim=512)

_OPENCLIP_MARKS = ("visual.transformer.resblocks.", "visual.conv1.", "transformer.resblocks.", "visual.class_embedding")
_DROP = ("logit_scale", "logit_bias", "text_model.embeddings.position_ids", "vision_model.embeddings.position_ids")


def vision_param_shapes(cfg: ClipVisionConfig) -> Dict[str, Tuple[int, ...]]:
    """Names (CLIPVisionModelWithProjection without ``vision_model.``) and shapes of the image tower's parameters."""
    D, F, ps = cfg.width, cfg.mlp_dim, cfg.patch_size
    T = 1 + (cfg.image_size // ps) ** 2
    out = {"embeddings.class_embedding": (D,), "embeddings.patch_embedding.weight": (D, 3, ps, ps),
           "embeddings.position_embedding.weight": (T, D), "pre_layrnorm.weight": (D,), "pre_layrnorm.bias": (D,)}
    for i in range(cfg.layers):
        p = f"encoder.layers.{i}."
        for ln in ("layer_norm1", "layer_norm2"):
            out[p + ln + ".weight"], out[p + ln + ".bias"] = (D,), (D,)
        for m in ("q_proj", "k_proj", "v_proj", "out_proj"):
            out[p + f"self_attn.{m}.weight"], out[p + f"self_attn.{m}.bias"] = (D, D), (D,)
        out[p + "mlp.fc1.weight"], out[p + "mlp.fc1.bias"] = (F, D), (F,)
        out[p + "mlp.fc2.weight"], out[p + "mlp.fc2.bias"] = (D, F), (D,)
    out["post_layernorm.weight"], out["post_layernorm.bias"] = (D,), (D,)
    out["visual_projection.weight"] = (cfg.projection_dim, D)
    return out


def split_clip_state_dict(sd: Dict[str, torch.Tensor]):
    """A ``CLIPModel`` state dict -> (vision, text, visual_projection, text_projection): ``vision`` under the names of the
    image tower without ``vision_model.``, ``text`` still under ``text_model.*`` (``text_encoder.normalize_text_state_dict``
    takes it from there), the two projection matrices.  ``logit_scale`` and ``position_ids`` are dropped; every other key
    lands in exactly one part.  OpenCLIP naming, foreign keys and a missing projection are refused."""
    sd = sd.get("state_dict", sd) if isinstance(sd.get("state_dict", None), dict) else sd
    if any(k.startswith(_OPENCLIP_MARKS) for k in sd):
        raise ValueError("OpenCLIP naming (visual.transformer.resblocks.* / transformer.resblocks.*) is not supported; convert the "
                         "checkpoint to the transformers CLIPModel layout (vision_model.*, text_model.*, *_projection.weight)")
    vision, text, foreign = {}, {}, []
    vproj = tproj = None
    for k, v in sd.items():
        if k in _DROP:
            continue
        if k.startswith("vision_model."):
            vision[k[len("vision_model."):]] = v
        elif k.startswith("text_model."):
            text[k] = v
        elif k == "visual_projection.weight":
            vproj = v
        elif k == "text_projection.weight":
            tproj = v
        else:
            foreign.append(k)
    if foreign:
        raise ValueError(f"not a CLIPModel state_dict: foreign keys {sorted(foreign)[:8]}")
    for name, part in (("visual_projection.weight", vproj), ("text_projection.weight", tproj)):
        if part is None:
            raise ValueError(f"missing {name}: the scores need a CLIPModel with both projection heads (a bare CLIPVisionModel or "
                             "CLIPTextModel has none)")
    if not vision or not text:
        raise ValueError("missing vision_model.* or text_model.* keys: the scores need both towers of a CLIPModel")
    return vision, text, vproj, tproj


def infer_vision_config(vision: Dict[str, torch.Tensor], vproj: torch.Tensor, config: Optional[dict] = None,
                        preprocessor: Optional[dict] = None) -> ClipVisionConfig:
    """Geometry from the ``vision_config`` of a transformers ``config.json`` when given, else from the shapes (heads =
    width / 64 and quick_gelu, as every OpenAI CLIP ViT has them)."""
    pw, pos = vision.get("embeddings.patch_embedding.weight"), vision.get("embeddings.position_embedding.weight")
    if pw is None or pos is None:
        raise ValueError("missing embeddings.patch_embedding.weight / embeddings.position_embedding.weight")
    kw = {}
    if preprocessor:
        if preprocessor.get("image_mean") is not None:
            kw["image_mean"] = tuple(float(v) for v in preprocessor["image_mean"])
        if preprocessor.get("image_std") is not None:
            kw["image_std"] = tuple(float(v) for v in preprocessor["image_std"])
    if config is not None:
        act = config.get("hidden_act", "quick_gelu")
        if act not in ("quick_gelu", "gelu"):
            raise ValueError(f"hidden_act {act!r}: the encoder supports quick_gelu and gelu")
        return ClipVisionConfig(image_size=int(config["image_size"]), patch_size=int(config["patch_size"]), width=int(config["hidden_size"]),
                                layers=int(config["num_hidden_layers"]), heads=int(config["num_attention_heads"]),
                                mlp_dim=int(config["intermediate_size"]), projection_dim=int(vproj.shape[0]), act=act,
                                ln_eps=float(config.get("layer_norm_eps", 1e-5)), **kw)
    D, ps = int(pw.shape[0]), int(pw.shape[2])
    G = int(round((int(pos.shape[0]) - 1) ** 0.5))
    if 1 + G * G != int(pos.shape[0]) or D % 64:
        raise ValueError(f"cannot infer the geometry from position_embedding {tuple(pos.shape)} / width {D}: pass a folder with config.json")
    layers = 1 + max((int(k.split(".")[2]) for k in vision if k.startswith("encoder.layers.")), default=-1)
    return ClipVisionConfig(image_size=G * ps, patch_size=ps, width=D, layers=layers, heads=D // 64,
                            mlp_dim=int(vision["encoder.layers.0.mlp.fc1.weight"].shape[0]), projection_dim=int(vproj.shape[0]), **kw)


def check_vision_state_dict(sd: Dict[str, torch.Tensor], cfg: ClipVisionConfig):
    want = vision_param_shapes(cfg)
    missing, foreign = sorted(set(want) - set(sd)), sorted(set(sd) - set(want))
    if foreign:
        raise ValueError(f"foreign keys for a {cfg.layers}-layer CLIP image encoder: {foreign[:8]}")
    if missing:
        raise ValueError(f"missing keys of the CLIP image encoder: {missing[:8]}" + (" ..." if len(missing) > 8 else ""))
    for k, shape in want.items():
        if tuple(sd[k].shape) != shape:
            raise ValueError(f"{k} has shape {tuple(sd[k].shape)}, the geometry asks for {shape}")


def resized_shape(H: int, W: int, S: int) -> Tuple[int, int]:
    """CLIPImageProcessor's resize target: shortest edge -> S, the other edge int(long * S / short)."""
    if H <= W:
        return S, int(W * S / H)
    return int(H * S / W), S


def preprocess_pil(frames: torch.Tensor, cfg: ClipVisionConfig) -> torch.Tensor:
    """``CLIPImageProcessor`` (PIL backend) restated with PIL itself: bicubic resize of the shortest edge to S, centre crop,
    float32(float64(v) / 255), (v - mean) / std in float32.  frames uint8 [n, H, W, 3] -> [n, 3, S, S] float32 (host)."""
    from PIL import Image
    S = cfg.image_size
    mean, std = np.array(cfg.image_mean, dtype=np.float32), np.array(cfg.image_std, dtype=np.float32)
    out = []
    for fr in np.asarray(torch.as_tensor(frames).cpu()):
        H, W = fr.shape[:2]
        Hn, Wn = resized_shape(H, W, S)
        if (Hn, Wn) != (H, W):
            fr = np.asarray(Image.fromarray(fr).resize((Wn, Hn), resample=Image.BICUBIC))
        top, left = (Hn - S) // 2, (Wn - S) // 2
        v = (fr[top:top + S, left:left + S].astype(np.float64) * (1 / 255)).astype(np.float32)
        out.append(torch.from_numpy(np.ascontiguousarray(((v - mean) / std).transpose(2, 0, 1))))
    return torch.stack(out)


def cosine(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().flatten(), b.double().flatten()
    return float((a * b).sum() / (a.norm() * b.norm()))


def score_embeddings(img: torch.Tensor, original_index: int, e_for: Optional[torch.Tensor], e_edit: Optional[torch.Tensor]) -> List[dict]:
    """The four numbers per frame from the embeddings: img [n, P]; e_for / e_edit [P], or None for an empty prompt."""
    img = img.double().cpu()
    n = img.shape[0]
    if not 0 <= original_index < n:
        raise ValueError(f"original_index {original_index} outside [0, {n})")
    e_for = None if e_for is None else e_for.double().cpu().flatten()
    e_edit = None if e_edit is None else e_edit.double().cpu().flatten()
    out = []
    for i in range(n):
        rec = {"clip_for": None if e_for is None else cosine(img[i], e_for),
               "clip_edit": None if e_edit is None else cosine(img[i], e_edit),
               "image_sim": cosine(img[i], img[original_index]), "directional": None}
        if i != original_index and e_for is not None and e_edit is not None:
            rec["directional"] = cosine(img[i] - img[original_index], e_edit - e_for)
        out.append(rec)
    return out


class ClipScorer:
    """Image tower + text tower + tokenizer of one CLIP model; see the module docstring."""

    def __init__(self, vision_cfg: ClipVisionConfig, vision_sd: Dict[str, torch.Tensor], text_cfg: te.TextConfig,
                 text_sd: Dict[str, torch.Tensor], text_projection: torch.Tensor, tokenizer: te.CLIPTokenizer, device=None,
                 max_images: int = 8, preprocess: str = "device", model_path: str = "", grad: bool = False):
        from .hip import LocoClipVisionEngine, LocoTextEngine
        if preprocess not in PREPROCESS_MODES:
            raise ValueError(f"clip_preprocess choice: {', '.join(PREPROCESS_MODES)}")
        if tokenizer.model_max_length != text_cfg.positions:
            raise ValueError(f"tokenizer model_max_length {tokenizer.model_max_length} != the text tower's max_position_embeddings "
                             f"{text_cfg.positions}")
        if tuple(text_projection.shape) != (vision_cfg.projection_dim, text_cfg.width):
            raise ValueError(f"text_projection.weight has shape {tuple(text_projection.shape)}, expected "
                             f"{(vision_cfg.projection_dim, text_cfg.width)}")
        self.vision_cfg, self.text_cfg, self.tokenizer = vision_cfg, text_cfg, tokenizer
        self.preprocess_mode, self.model_path = preprocess, model_path
        self.vision = LocoClipVisionEngine(vision_cfg, max_images=max_images, device=device, grad=grad)
        self.vision.load_state_dict(vision_sd)
        self.text = LocoTextEngine(text_cfg, max_prompts=4, device=device)
        self.text.load_state_dict(text_sd)
        self.text_projection = text_projection.detach().double().cpu()
        self.device = self.vision.device

    def pixel_values(self, frames: torch.Tensor) -> torch.Tensor:
        frames = torch.as_tensor(frames)
        if frames.dim() == 3:
            frames = frames[None]
        if frames.dim() != 4 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
            raise ValueError(f"frames must be uint8 [n, H, W, 3], got {frames.dtype} {tuple(frames.shape)}")
        if self.preprocess_mode == "pil":
            return preprocess_pil(frames, self.vision_cfg).to(self.device)
        return self.vision.preprocess(frames)

    def image_embeds(self, frames: torch.Tensor) -> torch.Tensor:
        """uint8 frames [n, H, W, 3] (host or device) -> un-normalised image_embeds [n, P] fp32 on the device."""
        pv = self.pixel_values(frames)
        mi = self.vision.max_images
        outs = [self.vision.encode(pv[i:i + mi]) for i in range(0, pv.shape[0], mi)]
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def text_guidance(self, frames: torch.Tensor, text_embed: torch.Tensor, boxes=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The text loss of a float frame seen through windows, and its pixel gradient (a ``grad=True`` scorer).

        frames [nf, 3, H, W] fp32 in [-1, 1] (nf = 1: one frame through every window, or one frame per window); text_embed [P];
        boxes integer [n, 4] = (top, left, h, w), or None for the centred largest square of every frame.  Returns
        (loss [n] with loss_i = 1 - cos(E_I(window_i), text_embed), grad [nf, 3, H, W] = d sum_i loss_i / d frames), both on
        the device.  The cosine and its derivative with respect to the embeddings are taken in float64 from the fp32
        embeddings; the towers' forward and cotangent passes are the engine's."""
        if not getattr(self.vision, "grad", False):
            raise RuntimeError("text_guidance needs a scorer built with grad=True (load_clip(..., grad=True))")
        fr = torch.as_tensor(frames)
        if fr.dim() == 3:
            fr = fr[None]
        pv = self.vision.preprocess_float(fr, boxes)
        n, nf, H, W = pv.shape[0], fr.shape[0], fr.shape[2], fr.shape[3]
        tn = torch.as_tensor(text_embed).to(self.device).double().flatten()
        if tn.numel() != self.vision_cfg.projection_dim:
            raise ValueError(f"text_embed must hold {self.vision_cfg.projection_dim} values, got {tuple(text_embed.shape)}")
        tn = tn / tn.norm()
        loss, g_pv = [], []
        mi = self.vision.max_images
        for i in range(0, n, mi):
            emb = self.vision.encode(pv[i:i + mi]).double()
            norm = emb.norm(dim=1, keepdim=True)
            en = emb / norm
            cos = en @ tn
            loss.append(1 - cos)
            g_emb = -(tn[None] - cos[:, None] * en) / norm          # d (1 - cos) / d emb
            g_pv.append(self.vision.encode_vjp(g_emb.to(torch.float32)))
        grad = self.vision.preprocess_float_vjp(torch.cat(g_pv), boxes, nf, H, W)
        return torch.cat(loss).to(torch.float32), grad

    def text_embeds_from_ids(self, ids: torch.Tensor) -> torch.Tensor:
        """ids [n, positions] -> un-normalised text_embeds [n, P] fp32 (host): final state at the first EOS id x text_projection."""
        ids = torch.as_tensor(ids).to(torch.int64).cpu()
        mp = self.text.max_prompts
        states = torch.cat([self.text.encode_ids(ids[i:i + mp]) for i in range(0, ids.shape[0], mp)]).cpu()
        is_eos = ids == self.tokenizer.eos_token_id
        if not bool(is_eos.any(dim=1).all()):
            raise ValueError(f"a prompt's ids hold no EOS token ({self.tokenizer.eos_token_id})")
        at = is_eos.int().argmax(dim=1)
        pooled = states[torch.arange(ids.shape[0]), at].double()
        return (pooled @ self.text_projection.T).to(torch.float32)

    def text_embeds(self, prompts: Sequence[str]) -> torch.Tensor:
        return self.text_embeds_from_ids(self.tokenizer.batch(list(prompts)))

    def score(self, frames: torch.Tensor, original_index: int, for_prompt: str, edit_prompt: str) -> List[dict]:
        """Per frame: clip_for, clip_edit, image_sim, directional (None for the original frame and whenever a prompt is
        empty; an image-text cosine is None when its prompt is empty)."""
        img = self.image_embeds(frames)
        prompts = [p for p in (for_prompt, edit_prompt) if p]
        emb = iter(self.text_embeds(prompts)) if prompts else iter(())
        e_for = next(emb) if for_prompt else None
        e_edit = next(emb) if edit_prompt else None
        return score_embeddings(img, original_index, e_for, e_edit)


def _read_json(path: str) -> Optional[dict]:
    if not os.path.exists(path):
        return None
    with open(path) as f:
        return json.load(f)


def read_clip_checkpoint(path: str):
    """-> (state_dict, config.json or None, preprocessor_config.json or None, tokenizer folder or None)"""
    if os.path.isdir(path):
        config, pre = _read_json(os.path.join(path, "config.json")), _read_json(os.path.join(path, "preprocessor_config.json"))
        for fn in ("model.safetensors", "pytorch_model.bin"):
            if os.path.exists(os.path.join(path, fn)):
                sd = te._read_state_dict(os.path.join(path, fn))
                break
        else:
            raise FileNotFoundError(f"{path}: no model.safetensors or pytorch_model.bin")
        tok = next((d for d in (path, os.path.join(path, "tokenizer")) if os.path.exists(os.path.join(d, "vocab.json"))), None)
        return sd, config, pre, tok
    if os.path.isfile(path):
        return te._read_state_dict(path), None, None, None
    raise FileNotFoundError(path)


def load_clip(path: str, tokenizer_path: Optional[str] = None, device=None, max_images: int = 8, preprocess: str = "device",
              grad: bool = False) -> ClipScorer:
    """A ``CLIPModel`` folder or state-dict file -> a ``ClipScorer`` (both towers on the HIP engine).  ``grad``: the image tower
    keeps the records of its cotangent pass (``ClipScorer.text_guidance``)."""
    if not path:
        raise NotImplementedError("the CLIP scores need a CLIPModel checkpoint, which is not available offline: pass --clip_model_path "
                                  "(a transformers CLIPModel folder or state-dict file)")
    sd, config, pre, tok_dir = read_clip_checkpoint(path)
    vision, text, vproj, tproj = split_clip_state_dict(sd)
    vcfg = infer_vision_config(vision, vproj, None if config is None else config.get("vision_config"), pre)
    vision = dict(vision, **{"visual_projection.weight": vproj})
    check_vision_state_dict(vision, vcfg)
    tsd = te.normalize_text_state_dict(text)
    tcfg = te.infer_text_config(tsd, None if config is None else config.get("text_config"))
    te.check_text_state_dict(tsd, tcfg)
    tok_dir = tok_dir or tokenizer_path        # the model's own tokenizer first: a driver's --tokenizer_path may be its T5 one
    if not tok_dir:
        raise ValueError(f"{path} holds no tokenizer (vocab.json, merges.txt): pass --tokenizer_path")
    return ClipScorer(vcfg, vision, tcfg, tsd, tproj, te.CLIPTokenizer.from_dir(tok_dir), device=device, max_images=max_images,
                      preprocess=preprocess, model_path=path, grad=grad)
