"""Text-prompted edit masks: CLIPSeg (``CLIPSegForImageSegmentation`` of transformers, e.g. ``CIDAS/clipseg-rd64-refined``) on
the HIP engine, so that ``--mask_prompts "hair,eyes,mouth"`` gives one mask per prompt where Segment Anything gives N
unlabelled ones.

* ``read_clipseg_checkpoint(path)``: a local folder (``config.json`` + ``model.safetensors`` / ``pytorch_model.bin``, tokenizer
  files, optional ``preprocessor_config.json``) or a state-dict file -> the parts: the CLIP image tower, the CLIP text tower,
  ``text_projection`` and the decoder, with their geometries.  Nothing is ever downloaded.
* ``PromptMasker``: the image tower at the segmentation size on ``hip.LocoClipVisionEngine`` (``encode_taps``: the residual
  stream after ``extract_layers``; the position table is interpolated once on the host with the call transformers makes), the
  text tower on ``hip.LocoTextEngine``, the decoder, the preprocessing and the mask kernel on ``hip.LocoClipSegDecoder``
  (``csrc/clipseg.hip``).  ``logits`` / ``masks`` / ``conditional_embeddings`` / ``logits_from_embeddings``.
* ``prompt_masks_for_driver``: what ``mask_segmentation.segment_for_driver`` calls on rank 0 when ``--mask_prompt_model_path``
  is set: ``mask/mask.pt`` (bool [N, res, res], one mask per prompt in prompt order: ``--mask_index`` selects a prompt),
  ``mask/mask_prompts.json`` and the overlay PNGs of the SAM path.

No published CLIPSeg weights are available offline: the model is pinned to transformers with seeded random weights
(tests/golden/clipseg), unpinned against the published checkpoint.
"""
from __future__ import annotations

import dataclasses
import json
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import clip_score as cs
from . import text_encoder as te

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
RESAMPLE_NAMES = {2: "bilinear", 3: "bicubic"}      # PIL's Image.BILINEAR / Image.BICUBIC, the two filters csrc/clipseg.hip builds
DEFAULT_SIZE, DEFAULT_RESAMPLE = 352, 3
DEFAULT_EXTRACT_LAYERS = (3, 6, 9)


@dataclass(frozen=True)
class ClipSegDecoderConfig:
    width: int = 768                 # D of the tower
    grid: int = 22                   # G at the run size (352 / 16)
    patch_size: int = 16
    reduce_dim: int = 64
    heads: int = 4                   # decoder_num_attention_heads
    ffn: int = 2048                  # decoder_intermediate_size
    n_taps: int = 3                  # len(extract_layers)
    conditional_layer: int = 0
    projection_dim: int = 512
    complex_head: bool = True        # use_complex_transposed_convolution
    ln_eps: float = 1e-5
    max_masks: int = 8

    @property
    def logit_size(self) -> int:
        """What the head's layers give: G ps, or G (ps / 4)^2 with the complex head (G ps only when ps = 16)."""
        return self.grid * (self.patch_size // 4) ** 2 if self.complex_head else self.grid * self.patch_size


@dataclass(frozen=True)
class Preprocess:
    size: int = DEFAULT_SIZE
    resample: int = DEFAULT_RESAMPLE
    image_mean: Tuple[float, float, float] = IMAGENET_MEAN
    image_std: Tuple[float, float, float] = IMAGENET_STD


def parse_prompts(text) -> List[str]:
    """``"hair, eyes,mouth"`` (or a list) -> ["hair", "eyes", "mouth"]; an empty entry is refused."""
    parts = [p.strip() for p in (text.split(",") if isinstance(text, str) else list(text))]
    if not parts or (len(parts) == 1 and not parts[0]):
        raise ValueError("--mask_prompts is empty: give a comma list of prompts, one mask per entry")
    for i, p in enumerate(parts):
        if not p:
            raise ValueError(f"--mask_prompts: entry {i} of {text!r} is empty")
    return parts


def threshold_logit(threshold: float) -> float:
    """sigmoid(logit) > threshold <=> logit > log(threshold / (1 - threshold))"""
    if not 0.0 < float(threshold) < 1.0:
        raise ValueError(f"--mask_prompt_threshold {threshold} outside (0, 1): it is a probability")
    return math.log(float(threshold) / (1.0 - float(threshold)))


# ------------------------------------------------------------------------------------------- float64 restatements (yardsticks)
def _filter(x: torch.Tensor, resample: int) -> torch.Tensor:
    x = x.abs()
    if resample == 2:
        return (1 - x).clamp(min=0)
    near, far = ((1.5 * x - 2.5) * x) * x + 1, (((x - 5) * x + 8) * x - 4) * -0.5
    return torch.where(x < 1, near, torch.where(x < 2, far, torch.zeros_like(x)))


def resize_matrix(n_in: int, n_out: int, resample: int) -> torch.Tensor:
    """[n_out, n_in] float64: the antialiased resize of one axis as PIL and torch's ``interpolate(antialias=True)`` define it
    -- output o sits at (o + 1 / 2) scale, its taps are the input pixels within support = (1 | 2) max(scale, 1) of it,
    weighted by the triangle (resample 2) or the cubic a = -0.5 (resample 3) filter of (pixel centre - position) / max(scale, 1)
    and normalised to sum 1.  The rule csrc/clipseg.hip's two passes evaluate in fp32."""
    if resample not in RESAMPLE_NAMES:
        raise ValueError(f"resample {resample}: only 2 (bilinear) and 3 (bicubic) are supported")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = (1.0 if resample == 2 else 2.0) * fs
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        center = (o + 0.5) * scale
        lo, hi = max(int(center - support + 0.5), 0), min(int(center + support + 0.5), n_in)
        w = _filter((torch.arange(lo, hi, dtype=torch.float64) - center + 0.5) / fs, resample)
        M[o, lo:hi] = w / w.sum()
    return M


def restated_preprocess(frames, pre: Preprocess, normalize: bool = True) -> torch.Tensor:
    """uint8 [n, H, W, 3] or floating [n, 3, H, W] in [-1, 1] -> float64 [n, 3, S, S]: each axis resized to S on its own (no
    shortest-edge rule, no crop), to [0, 1], (v - mean) / std; ``normalize=False`` stops at grey levels (0 .. 255)."""
    x = torch.as_tensor(frames)
    x = x.permute(0, 3, 1, 2).to(torch.float64) if x.dtype == torch.uint8 else (x.to(torch.float64) / 2 + 0.5) * 255
    S = pre.size
    x = torch.einsum("oh,nchw->ncow", resize_matrix(x.shape[2], S, pre.resample), x)
    x = torch.einsum("pw,ncow->ncop", resize_matrix(x.shape[3], S, pre.resample), x)
    if not normalize:
        return x
    m, s = (torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1) for v in (pre.image_mean, pre.image_std))
    return (x / 255 - m) / s


def restated_masks(logits: torch.Tensor, resolution: int, threshold: float):
    """float64: logits [M, s, s] -> (resized [M, res, res], masks bool): bilinear, align_corners False, no antialias."""
    r = F.interpolate(torch.as_tensor(logits).double()[:, None], size=(resolution, resolution), mode="bilinear", align_corners=False)[:, 0]
    return r, r > threshold_logit(threshold)


# ---------------------------------------------------------------------------------------------------------------- checkpoint
def interpolate_position_table(pos: torch.Tensor, grid: int) -> torch.Tensor:
    """position_embedding.weight [1 + G0^2, D] -> [1 + grid^2, D] with exactly the call of transformers'
    ``CLIPSegVisionEmbeddings.interpolate_pos_encoding``: fp32 bicubic, align_corners False, the class row kept.  Unchanged when
    grid == G0."""
    pos = torch.as_tensor(pos).detach().to(torch.float32).cpu()
    n0, D = int(pos.shape[0]) - 1, int(pos.shape[1])
    g0 = int(n0 ** 0.5)
    if 1 + g0 * g0 != pos.shape[0]:
        raise ValueError(f"position_embedding {tuple(pos.shape)} is not 1 + a square grid")
    if grid == g0:
        return pos
    patch = pos[None, 1:].reshape(1, g0, g0, D).permute(0, 3, 1, 2)
    patch = F.interpolate(patch, size=(grid, grid), mode="bicubic", align_corners=False)
    return torch.cat((pos[None, :1], patch.permute(0, 2, 3, 1).reshape(1, -1, D)), dim=1)[0].contiguous()


def decoder_param_shapes(cfg: ClipSegDecoderConfig) -> Dict[str, Tuple[int, ...]]:
    """Names (transformers' ``decoder.*`` without the prefix) and shapes of the decoder's parameters."""
    R, D, Fd, P, ps = cfg.reduce_dim, cfg.width, cfg.ffn, cfg.projection_dim, cfg.patch_size
    out: Dict[str, Tuple[int, ...]] = {}
    for f in ("film_mul", "film_add"):
        out[f + ".weight"], out[f + ".bias"] = (R, P), (R,)
    for i in range(cfg.n_taps):
        out[f"reduces.{i}.weight"], out[f"reduces.{i}.bias"] = (R, D), (R,)
        p = f"layers.{i}."
        for m in ("q_proj", "k_proj", "v_proj", "out_proj"):
            out[p + f"self_attn.{m}.weight"], out[p + f"self_attn.{m}.bias"] = (R, R), (R,)
        for ln in ("layer_norm1", "layer_norm2"):
            out[p + ln + ".weight"], out[p + ln + ".bias"] = (R,), (R,)
        out[p + "mlp.fc1.weight"], out[p + "mlp.fc1.bias"] = (Fd, R), (Fd,)
        out[p + "mlp.fc2.weight"], out[p + "mlp.fc2.bias"] = (R, Fd), (R,)
    tc = "transposed_convolution."
    if cfg.complex_head:
        k = ps // 4
        out[tc + "0.weight"], out[tc + "0.bias"] = (R, R, 3, 3), (R,)
        out[tc + "2.weight"], out[tc + "2.bias"] = (R, R // 2, k, k), (R // 2,)
        out[tc + "4.weight"], out[tc + "4.bias"] = (R // 2, 1, k, k), (1,)
    else:
        out[tc + "weight"], out[tc + "bias"] = (R, 1, ps, ps), (1,)
    return out


def check_decoder_state_dict(sd: Dict[str, torch.Tensor], cfg: ClipSegDecoderConfig):
    want = decoder_param_shapes(cfg)
    missing, foreign = sorted(set(want) - set(sd)), sorted(set(sd) - set(want))
    if foreign:
        raise ValueError(f"foreign keys for a {cfg.n_taps}-stage CLIPSeg decoder: {foreign[:8]}")
    if missing:
        raise ValueError(f"missing keys of the CLIPSeg decoder: {missing[:8]}" + (" ..." if len(missing) > 8 else ""))
    for k, shape in want.items():
        if tuple(sd[k].shape) != shape:
            raise ValueError(f"decoder.{k} has shape {tuple(sd[k].shape)}, the geometry asks for {shape}")


def read_preprocessor(pre: Optional[dict]) -> Preprocess:
    """``preprocessor_config.json`` -> size, resample, mean, std; absent: 352, bicubic, the ImageNet mean / std."""
    if not pre:
        return Preprocess()
    size = pre.get("size", DEFAULT_SIZE)
    if isinstance(size, dict):
        if "height" in size and size.get("height") != size.get("width"):
            raise ValueError(f"preprocessor size {size}: the token grid must be square")
        size = size.get("height", size.get("shortest_edge", DEFAULT_SIZE))
    resample = int(pre.get("resample", DEFAULT_RESAMPLE))
    if resample not in RESAMPLE_NAMES:
        raise ValueError(f"preprocessor_config.json: resample {resample} is not supported (2 = bilinear and 3 = bicubic are)")
    mean = tuple(float(v) for v in (pre.get("image_mean") or IMAGENET_MEAN))
    std = tuple(float(v) for v in (pre.get("image_std") or IMAGENET_STD))
    return Preprocess(size=int(size), resample=resample, image_mean=mean, image_std=std)


@dataclass
class ClipSegParts:
    vision_cfg: cs.ClipVisionConfig          # at the RUN size (image_size = preprocess.size)
    vision_sd: Dict[str, torch.Tensor]       # names of the image tower without prefix, position table at the run size
    text_cfg: te.TextConfig
    text_sd: Dict[str, torch.Tensor]
    text_projection: torch.Tensor
    decoder_cfg: ClipSegDecoderConfig
    decoder_sd: Dict[str, torch.Tensor]
    extract_layers: Tuple[int, ...]
    preprocess: Preprocess
    native_size: int
    tokenizer_dir: Optional[str]


def split_clipseg_state_dict(sd: Dict[str, torch.Tensor]):
    """-> (CLIPModel state dict with ``clip.`` stripped, decoder state dict with ``decoder.`` stripped); foreign keys refused."""
    sd = sd.get("state_dict", sd) if isinstance(sd.get("state_dict", None), dict) else sd
    clip, dec, foreign = {}, {}, []
    for k, v in sd.items():
        if k.startswith("clip."):
            clip[k[len("clip."):]] = v
        elif k.startswith("decoder."):
            dec[k[len("decoder."):]] = v
        else:
            foreign.append(k)
    if foreign:
        raise ValueError(f"not a CLIPSegForImageSegmentation state_dict: foreign keys {sorted(foreign)[:8]}")
    if not clip or not dec:
        raise ValueError("missing clip.* or decoder.* keys: the prompt masks need a CLIPSegForImageSegmentation checkpoint")
    return clip, dec


def parts_from_state_dict(sd, config: Optional[dict] = None, pre: Optional[dict] = None, tokenizer_dir: Optional[str] = None,
                          max_masks: int = 8, run_size: Optional[int] = None) -> ClipSegParts:
    """The split, the geometries (from ``config`` = config.json where given, else from the shapes with the rd64 defaults), the
    position table brought to the run size."""
    clip, dec = split_clipseg_state_dict(sd)
    vision, text, vproj, tproj = cs.split_clip_state_dict(clip)
    prep = read_preprocessor(pre)
    if run_size is not None:
        prep = dataclasses.replace(prep, size=int(run_size))
    vpre = {"image_mean": prep.image_mean, "image_std": prep.image_std}
    native = cs.infer_vision_config(vision, vproj, None if config is None else config.get("vision_config"), vpre)
    if prep.size % native.patch_size:
        raise ValueError(f"segmentation size {prep.size} is not a multiple of the patch size {native.patch_size}")
    G = prep.size // native.patch_size
    vcfg = dataclasses.replace(native, image_size=prep.size)
    vision = dict(vision, **{"visual_projection.weight": vproj})
    vision["embeddings.position_embedding.weight"] = interpolate_position_table(vision["embeddings.position_embedding.weight"], G)
    cs.check_vision_state_dict(vision, vcfg)
    tsd = te.normalize_text_state_dict(text)
    tcfg = te.infer_text_config(tsd, None if config is None else config.get("text_config"))
    te.check_text_state_dict(tsd, tcfg)
    c = config or {}
    n_taps = 1 + max((int(k.split(".")[1]) for k in dec if k.startswith("reduces.")), default=-1)
    extract = tuple(int(v) for v in c.get("extract_layers", DEFAULT_EXTRACT_LAYERS))
    if len(extract) != n_taps:
        raise ValueError(f"extract_layers {list(extract)} for a decoder of {n_taps} stages")
    if list(extract) != sorted(set(extract)) or extract[0] < 0 or extract[-1] >= vcfg.layers:
        raise ValueError(f"extract_layers {list(extract)} must be strictly increasing inside [0, {vcfg.layers})")
    if "reduces.0.weight" not in dec or "layers.0.mlp.fc1.weight" not in dec:
        raise ValueError("missing decoder.reduces.0.weight / decoder.layers.0.mlp.fc1.weight")
    complex_head = bool(c.get("use_complex_transposed_convolution", "transposed_convolution.0.weight" in dec))
    dcfg = ClipSegDecoderConfig(width=vcfg.width, grid=G, patch_size=vcfg.patch_size, reduce_dim=int(dec["reduces.0.weight"].shape[0]),
                                heads=int(c.get("decoder_num_attention_heads", 4)), ffn=int(dec["layers.0.mlp.fc1.weight"].shape[0]),
                                n_taps=n_taps, conditional_layer=int(c.get("conditional_layer", 0)), projection_dim=int(tproj.shape[0]),
                                complex_head=complex_head, ln_eps=vcfg.ln_eps, max_masks=int(max_masks))
    check_decoder_state_dict(dec, dcfg)
    return ClipSegParts(vcfg, vision, tcfg, tsd, tproj, dcfg, dec, extract, prep, native.image_size, tokenizer_dir)


def read_clipseg_checkpoint(path: str, max_masks: int = 8, run_size: Optional[int] = None) -> ClipSegParts:
    """A local ``CLIPSegForImageSegmentation`` folder or state-dict file -> ``ClipSegParts``.  Never downloads."""
    if not path or not os.path.exists(path):
        raise FileNotFoundError(f"{path}: --mask_prompt_model_path must name a local CLIPSegForImageSegmentation folder (config.json + "
                                "model.safetensors or pytorch_model.bin) or a state-dict file; nothing is downloaded")
    sd, config, pre, tok = cs.read_clip_checkpoint(path)
    return parts_from_state_dict(sd, config, pre, tok, max_masks=max_masks, run_size=run_size)


# ------------------------------------------------------------------------------------------------------------------ the model
class PromptMasker:
    """CLIPSeg on the HIP engine; see the module docstring.  ``frames``: uint8 [n, H, W, 3] (or [H, W, 3]) or floating
    [n, 3, H, W] in [-1, 1]."""

    def __init__(self, parts: ClipSegParts, tokenizer: te.CLIPTokenizer, device=None, max_images: int = 4, model_path: str = ""):
        from .hip import LocoClipSegDecoder, LocoClipVisionEngine, LocoTextEngine
        if tokenizer.model_max_length != parts.text_cfg.positions:
            raise ValueError(f"tokenizer model_max_length {tokenizer.model_max_length} != the text tower's max_position_embeddings "
                             f"{parts.text_cfg.positions}")
        self.parts, self.tokenizer, self.model_path = parts, tokenizer, model_path
        self.vision = LocoClipVisionEngine(parts.vision_cfg, max_images=max_images, device=device)
        self.vision.load_state_dict(parts.vision_sd)
        self.text = LocoTextEngine(parts.text_cfg, max_prompts=4, device=device)
        self.text.load_state_dict(parts.text_sd)
        self.decoder = LocoClipSegDecoder(parts.decoder_cfg, device=device)
        self.decoder.load_state_dict(parts.decoder_sd)
        self.text_projection = parts.text_projection.detach().double().cpu()
        self.device = self.vision.device

    def pixel_values(self, frames) -> torch.Tensor:
        fr = torch.as_tensor(frames)
        if fr.dim() == 3:
            fr = fr[None]
        p = self.parts.preprocess
        return self.decoder.preprocess(fr, p.size, p.resample, p.image_mean, p.image_std)

    def conditional_embeddings_from_ids(self, ids: torch.Tensor) -> torch.Tensor:
        """ids [n, 77] -> [n, P] fp32 (host): the final-LayerNorm state at the first EOS id times ``text_projection``.  The
        prompts are padded to the tower's 77 positions and no attention mask is passed: the tower's causal mask makes the state
        at the EOS position independent of the padding behind it."""
        ids = torch.as_tensor(ids).to(torch.int64).cpu()
        mp = self.text.max_prompts
        states = torch.cat([self.text.encode_ids(ids[i:i + mp]) for i in range(0, ids.shape[0], mp)]).cpu()
        is_eos = ids == self.tokenizer.eos_token_id
        if not bool(is_eos.any(dim=1).all()):
            raise ValueError(f"a prompt's ids hold no EOS token ({self.tokenizer.eos_token_id})")
        at = is_eos.int().argmax(dim=1)
        pooled = states[torch.arange(ids.shape[0]), at].double()
        return (pooled @ self.text_projection.T).to(torch.float32)

    def conditional_embeddings(self, prompts: Sequence[str]) -> torch.Tensor:
        return self.conditional_embeddings_from_ids(self.tokenizer.batch(parse_prompts(list(prompts))))

    def taps(self, pixel_values: torch.Tensor) -> torch.Tensor:
        mi = self.vision.max_images
        outs = [self.vision.encode_taps(pixel_values[i:i + mi], self.parts.extract_layers) for i in range(0, pixel_values.shape[0], mi)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)

    def logits_from_embeddings(self, frames, cond: torch.Tensor, image_of_mask=None) -> torch.Tensor:
        """The ``conditional_embeddings=`` door of transformers: cond [M, P]; image_of_mask: the frame every mask looks at
        (None with one frame: all on it; None otherwise: mask m on frame m) -> logits [M, s, s] on the device.  The tower runs
        once per frame, the decoder in batches of ``max_masks``."""
        pv = self.pixel_values(frames)
        cond = torch.as_tensor(cond)
        M, n = cond.shape[0], pv.shape[0]
        if image_of_mask is None:
            if n != 1 and n != M:
                raise ValueError(f"{M} conditional embeddings for {n} frames: pass image_of_mask")
            image_of_mask = [0] * M if n == 1 else list(range(M))
        image_of_mask = [int(v) for v in image_of_mask]
        taps = self.taps(pv)
        mm = self.decoder.cfg.max_masks
        outs = [self.decoder.decode(taps, cond[i:i + mm], image_of_mask[i:i + mm]) for i in range(0, M, mm)]
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def logits(self, frames, prompts: Sequence[str], image_of_mask=None) -> torch.Tensor:
        return self.logits_from_embeddings(frames, self.conditional_embeddings(prompts), image_of_mask)

    def masks_from_logits(self, logits: torch.Tensor, resolution: int, threshold: float = 0.5):
        """-> (bool [M, res, res], area int32 [M]) on the device"""
        mask, area = self.decoder.masks(logits, resolution, threshold_logit(threshold))
        return mask.bool(), area

    def masks(self, frames, prompts: Sequence[str], resolution: int, threshold: float = 0.5) -> torch.Tensor:
        """One frame, N prompts -> bool [N, res, res] on the device; a prompt whose mask comes out empty raises."""
        prompts = parse_prompts(list(prompts))
        logits = self.logits(frames, prompts)
        mask, area = self.masks_from_logits(logits, resolution, threshold)
        check_not_empty(prompts, area.cpu(), logits.flatten(1).max(dim=1).values.cpu(), threshold)
        return mask


def check_not_empty(prompts: Sequence[str], area, logit_max, threshold: float):
    """An all-false mask must not reach the solver (``JacobianOperator.check_mask`` would only catch it after the solve)."""
    for p, a, mx in zip(prompts, area.tolist(), logit_max.tolist()):
        if int(a) == 0:
            raise RuntimeError(f"prompt {p!r} gives an empty mask: its largest logit is {mx:.4g}, the threshold {threshold} asks for more "
                               f"than {threshold_logit(threshold):.4g}; lower --mask_prompt_threshold or change the prompt")


def load_prompt_masker(path: str, tokenizer_path: Optional[str] = None, device=None, max_masks: int = 8, max_images: int = 4,
                       run_size: Optional[int] = None) -> PromptMasker:
    parts = read_clipseg_checkpoint(path, max_masks=max_masks, run_size=run_size)
    tok_dir = parts.tokenizer_dir or tokenizer_path
    if not tok_dir:
        raise ValueError(f"{path} holds no tokenizer (vocab.json, merges.txt): pass --tokenizer_path")
    return PromptMasker(parts, te.CLIPTokenizer.from_dir(tok_dir), device=device, max_images=max_images, model_path=path)


# ----------------------------------------------------------------------------------------------------------------- the driver
def prompt_masks_for_driver(args, log_dir: str, image, resolution: int, masker=None) -> torch.Tensor:
    """Rank 0's part of ``segment_for_driver`` with ``--mask_prompt_model_path``: `image` uint8 [H, W, 3] -> bool
    [N, res, res] on the host, one mask per entry of ``--mask_prompts``, written to ``<log_dir>/mask/mask.pt`` next to
    ``mask_prompts.json`` (per index: prompt, threshold, area share, logit min / max) and the overlay PNGs of the SAM path.
    `masker`: anything with ``logits(frames, prompts)`` and ``masks_from_logits(logits, resolution, threshold)``."""
    from .mask_segmentation import SAM, to_uint8_image
    prompts = parse_prompts(getattr(args, "mask_prompts", ""))
    threshold = float(getattr(args, "mask_prompt_threshold", 0.5))
    threshold_logit(threshold)
    if masker is None:
        masker = load_prompt_masker(args.mask_prompt_model_path, tokenizer_path=getattr(args, "tokenizer_path", None) or None,
                                    device=getattr(args, "device", None), max_masks=min(max(len(prompts), 1), 64))
    img = to_uint8_image(image)
    logits = masker.logits(torch.from_numpy(np.ascontiguousarray(img))[None], prompts)
    masks, area = masker.masks_from_logits(logits, resolution, threshold)
    flat = logits.flatten(1)
    lmin, lmax = flat.min(dim=1).values.cpu(), flat.max(dim=1).values.cpu()
    check_not_empty(prompts, area.cpu(), lmax, threshold)
    masks = masks.cpu()
    mask_dir = os.path.join(log_dir, "mask")
    os.makedirs(mask_dir, exist_ok=True)
    # the overlays at the image's own size, as the SAM path draws them
    full, _ = masker.masks_from_logits(logits, max(img.shape[0], img.shape[1]), threshold)
    full = F.interpolate(full[:, None].float().cpu(), size=img.shape[:2], mode="nearest")[:, 0].bool().numpy()
    painter = SAM.__new__(SAM)
    painter.args, painter.log_dir, painter.transparency = args, mask_dir, 0.4
    painter.show_masks_on_image(img, full)
    record = [{"index": i, "prompt": p, "threshold": threshold, "area_share": float(a) / float(resolution * resolution),
               "logit_min": float(lo), "logit_max": float(hi)}
              for i, (p, a, lo, hi) in enumerate(zip(prompts, area.cpu().tolist(), lmin.tolist(), lmax.tolist()))]
    with open(os.path.join(mask_dir, "mask_prompts.json"), "w") as f:
        json.dump(record, f, indent=1)
    torch.save(masks, os.path.join(mask_dir, "mask.pt"))
    return masks
