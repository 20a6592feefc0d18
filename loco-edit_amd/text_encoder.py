"""CLIP text encoder of the Stable Diffusion paths: what diffusers' ``StableDiffusionPipeline.encode_prompt`` runs
(reference ``src/modules/edit.py:1187-1194``, called for every prompt at :523-538) -- tokenizer on the host, the
transformer on the HIP engine (``hip.LocoTextEngine``, ``csrc/textenc.hip``).

* ``CLIPTokenizer``: byte-level BPE in pure Python, the ids of ``transformers.CLIPTokenizer`` (NFC, runs of white space
  -> one space, lower case, the CLIP split pattern, ``</w>`` end-of-word, BOS / EOS, truncation to ``model_max_length``
  with EOS kept last, padding with the configured pad token).  No ``transformers`` import.
* ``load_text_encoder``: a diffusers pipeline root (``text_encoder/`` + ``tokenizer/``), a ``text_encoder/`` folder
  (``config.json`` + ``model.safetensors`` or ``pytorch_model.bin``) or one state-dict file (e.g. a CompVis SD 1.x
  ``.ckpt``); keys normalised to the CLIPTextTransformer naming without prefix.
* ``TextEncoder.encode(list[str]) -> [n, L, D]`` on the device.
"""
from __future__ import annotations

import json
import os
import re
import unicodedata
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch


@dataclass(frozen=True)
class TextConfig:
    vocab: int = 49408
    width: int = 768
    layers: int = 12
    heads: int = 12
    ffn: int = 3072
    positions: int = 77
    act: str = "quick_gelu"         # "quick_gelu" x sigmoid(1.702 x) | "gelu" exact erf
    ln_eps: float = 1e-5


# CLIP ViT-L/14 text tower (SD 1.x) and the OpenCLIP-H text tower as diffusers stores it (SD 2.x: 23 of its 24 layers)
SD1_CLIP_TEXT = TextConfig(width=768, layers=12, heads=12, ffn=3072, act="quick_gelu")
SD2_CLIP_TEXT = TextConfig(width=1024, layers=23, heads=16, ffn=4096, act="gelu")
_PRESETS_BY_WIDTH = {768: SD1_CLIP_TEXT, 1024: SD2_CLIP_TEXT}


# ---------------------------------------------------------------------------------------------------------------- tokenizer
def bytes_to_unicode() -> Dict[int, str]:
    """The byte -> printable character table of byte-level BPE (GPT-2 / CLIP)."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


# Unicode White_Space (what the normaliser's \s matches; Python's \s also takes U+001C..U+001F)
_WS = "\t\n\x0b\x0c\r \x85\xa0\u1680" + "".join(map(chr, range(0x2000, 0x200B))) + "\u2028\u2029\u202f\u205f\u3000"
_WS_RUN = re.compile("[" + re.escape(_WS) + "]+")
_SPECIAL = ("<|startoftext|>", "<|endoftext|>")
_CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")


def _is_letter(ch: str) -> bool:
    return unicodedata.category(ch)[0] == "L"


def _is_number(ch: str) -> bool:
    return unicodedata.category(ch)[0] == "N"


def split_words(text: str) -> List[str]:
    """The CLIP pattern ``<|startoftext|>|<|endoftext|>|'s|'t|'re|'ve|'m|'ll|'d|[\\p{L}]+|[\\p{N}]|[^\\s\\p{L}\\p{N}]+``
    applied left to right (matches kept, everything between them dropped)."""
    out, i, n = [], 0, len(text)
    while i < n:
        hit = next((s for s in _SPECIAL + _CONTRACTIONS if text.startswith(s, i)), None)
        if hit is not None:
            out.append(hit); i += len(hit); continue
        ch = text[i]
        if _is_letter(ch):
            j = i + 1
            while j < n and _is_letter(text[j]):
                j += 1
        elif _is_number(ch):
            j = i + 1
        elif ch in _WS:
            i += 1; continue
        else:
            j = i + 1
            while j < n and not (text[j] in _WS or _is_letter(text[j]) or _is_number(text[j])):
                j += 1
        out.append(text[i:j]); i = j
    return out


def _token_name(v) -> Optional[str]:
    return v.get("content") if isinstance(v, dict) else v


class CLIPTokenizer:
    """Byte-level BPE with the vocabulary / merges / special tokens of a CLIP ``tokenizer/`` folder."""

    def __init__(self, vocab: Dict[str, int], merges: List[Tuple[str, str]], model_max_length: int = 77,
                 bos_token: str = "<|startoftext|>", eos_token: str = "<|endoftext|>", pad_token: str = "<|endoftext|>",
                 unk_token: str = "<|endoftext|>"):
        self.encoder = dict(vocab)
        self.bpe_ranks = {m: i for i, m in enumerate(merges)}
        self.model_max_length = int(model_max_length)
        for name, tok in (("bos", bos_token), ("eos", eos_token), ("pad", pad_token), ("unk", unk_token)):
            if tok not in self.encoder:
                raise ValueError(f"{name} token {tok!r} is not in the vocabulary")
        self.bos_token_id, self.eos_token_id = self.encoder[bos_token], self.encoder[eos_token]
        self.pad_token_id, self.unk_token_id = self.encoder[pad_token], self.encoder[unk_token]
        self.byte_encoder = bytes_to_unicode()
        self.cache: Dict[str, List[str]] = {}
        # the special tokens are cut out of the raw text before anything else, as the added tokens of transformers'
        # tokenizer: with the SD 2.x pad token "!" every "!" of a prompt becomes the pad id
        specials = sorted({bos_token, eos_token, pad_token, unk_token}, key=len, reverse=True)
        self._special_re = re.compile("(" + "|".join(re.escape(t) for t in specials) + ")")

    @classmethod
    def from_dir(cls, path: str) -> "CLIPTokenizer":
        with open(os.path.join(path, "vocab.json"), encoding="utf-8") as f:
            vocab = json.load(f)
        merges = []
        with open(os.path.join(path, "merges.txt"), encoding="utf-8") as f:
            for line in f.read().split("\n"):
                if line.startswith("#version") or not line.strip():
                    continue
                parts = line.split()
                if len(parts) == 2:
                    merges.append((parts[0], parts[1]))
        kw = {}
        for fn in ("special_tokens_map.json", "tokenizer_config.json"):     # the config wins where both state a token
            p = os.path.join(path, fn)
            if os.path.exists(p):
                with open(p, encoding="utf-8") as f:
                    d = json.load(f)
                for k in ("bos_token", "eos_token", "pad_token", "unk_token"):
                    if d.get(k) is not None:
                        kw[k] = _token_name(d[k])
                if "model_max_length" in d:
                    kw["model_max_length"] = int(d["model_max_length"])
        return cls(vocab, merges, **kw)

    def bpe(self, word: str) -> List[str]:
        if word in self.cache:
            return self.cache[word]
        parts = list(word[:-1]) + [word[-1] + "</w>"]
        while len(parts) > 1:
            best, rank = None, None
            for pair in zip(parts[:-1], parts[1:]):
                r = self.bpe_ranks.get(pair)
                if r is not None and (rank is None or r < rank):
                    best, rank = pair, r
            if best is None:
                break
            merged, i = [], 0
            while i < len(parts):
                if i + 1 < len(parts) and (parts[i], parts[i + 1]) == best:
                    merged.append(parts[i] + parts[i + 1]); i += 2
                else:
                    merged.append(parts[i]); i += 1
            parts = merged
        self.cache[word] = parts
        return parts

    def tokenize(self, text: str) -> List[int]:
        """Ids of the text without BOS / EOS."""
        ids = []
        for k, seg in enumerate(self._special_re.split(text)):
            if k % 2:
                ids.append(self.encoder[seg])
            elif seg:
                ids.extend(self._tokenize_plain(seg))
        return ids

    def _tokenize_plain(self, text: str) -> List[int]:
        text = _WS_RUN.sub(" ", unicodedata.normalize("NFC", text)).lower()
        ids = []
        for w in split_words(text):
            if w in _SPECIAL:
                ids.append(self.encoder[w]); continue
            w = "".join(self.byte_encoder[b] for b in w.encode("utf-8"))
            ids.extend(self.encoder.get(t, self.unk_token_id) for t in self.bpe(w))
        return ids

    def __call__(self, text: str) -> List[int]:
        """``tokenizer(text, padding="max_length", max_length=model_max_length, truncation=True).input_ids``"""
        L = self.model_max_length
        ids = [self.bos_token_id] + self.tokenize(text)[:L - 2] + [self.eos_token_id]
        return ids + [self.pad_token_id] * (L - len(ids))

    def batch(self, texts: List[str]) -> torch.Tensor:
        return torch.tensor([self(t) for t in texts], dtype=torch.int32)


# ------------------------------------------------------------------------------------------------------------- checkpoints
_DROP = ("embeddings.position_ids",)
_OPENCLIP = "cond_stage_model.model."


def _strip_prefix(k: str) -> str:
    for p in ("cond_stage_model.transformer.text_model.", "cond_stage_model.transformer.", "text_model."):
        if k.startswith(p):
            return k[len(p):]
    return k


def text_param_names(cfg: TextConfig) -> List[str]:
    names = ["embeddings.token_embedding.weight", "embeddings.position_embedding.weight"]
    for i in range(cfg.layers):
        p = f"encoder.layers.{i}."
        names += [p + "layer_norm1.weight", p + "layer_norm1.bias", p + "layer_norm2.weight", p + "layer_norm2.bias"]
        for m in ("q_proj", "k_proj", "v_proj", "out_proj"):
            names += [p + f"self_attn.{m}.weight", p + f"self_attn.{m}.bias"]
        names += [p + "mlp.fc1.weight", p + "mlp.fc1.bias", p + "mlp.fc2.weight", p + "mlp.fc2.bias"]
    return names + ["final_layer_norm.weight", "final_layer_norm.bias"]


def normalize_text_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Keys of a CLIPTextModel (``text_model.*``), of a CompVis SD 1.x file (``cond_stage_model.transformer[.text_model].*``;
    the file's other networks are ignored) or already un-prefixed -> the CLIPTextTransformer naming without prefix.
    ``position_ids`` and ``text_projection.*`` are dropped; OpenCLIP naming and unknown keys are refused."""
    sd = sd.get("state_dict", sd) if isinstance(sd.get("state_dict", None), dict) else sd
    if any(k.startswith(_OPENCLIP) for k in sd):
        raise ValueError("OpenCLIP naming (cond_stage_model.model.transformer.resblocks.*: a CompVis SD 2.x checkpoint) is not "
                         "supported; convert it to the diffusers layout (text_encoder/ of the pipeline)")
    if any(k.startswith("cond_stage_model.") for k in sd):       # a whole CompVis pipeline file: its text encoder only
        sd = {k: v for k, v in sd.items() if k.startswith("cond_stage_model.")}
    out, foreign = {}, []
    for k, v in sd.items():
        n = _strip_prefix(k)
        if n in _DROP or n.startswith("text_projection.") or k.startswith("text_projection."):
            continue
        if not (n.startswith(("embeddings.", "encoder.layers.", "final_layer_norm."))):
            foreign.append(k); continue
        out[n] = v
    if foreign:
        raise ValueError(f"not a CLIP text encoder state_dict: foreign keys {sorted(foreign)[:8]}")
    return out


def infer_text_config(sd: Dict[str, torch.Tensor], config: Optional[dict] = None) -> TextConfig:
    """Geometry from a transformers ``config.json`` when given, else the preset of the width with the layer count of the keys."""
    tok = sd.get("embeddings.token_embedding.weight")
    pos = sd.get("embeddings.position_embedding.weight")
    if tok is None or pos is None:
        raise ValueError("missing embeddings.token_embedding.weight / embeddings.position_embedding.weight")
    if config is not None:
        act = config.get("hidden_act", "quick_gelu")
        if act not in ("quick_gelu", "gelu"):
            raise ValueError(f"hidden_act {act!r}: the encoder supports quick_gelu and gelu")
        return TextConfig(vocab=int(config.get("vocab_size", tok.shape[0])), width=int(config["hidden_size"]),
                          layers=int(config["num_hidden_layers"]), heads=int(config["num_attention_heads"]),
                          ffn=int(config["intermediate_size"]), positions=int(config.get("max_position_embeddings", pos.shape[0])),
                          act=act, ln_eps=float(config.get("layer_norm_eps", 1e-5)))
    width = int(tok.shape[1])
    if width not in _PRESETS_BY_WIDTH:
        raise ValueError(f"width {width} without config.json: only the SD 1.x (768) and SD 2.x (1024) geometries are known")
    layers = 1 + max((int(k.split(".")[2]) for k in sd if k.startswith("encoder.layers.")), default=-1)
    base = _PRESETS_BY_WIDTH[width]
    return TextConfig(vocab=int(tok.shape[0]), width=width, layers=layers, heads=base.heads, ffn=base.ffn,
                      positions=int(pos.shape[0]), act=base.act, ln_eps=base.ln_eps)


def check_text_state_dict(sd: Dict[str, torch.Tensor], cfg: TextConfig):
    want = set(text_param_names(cfg))
    missing, foreign = sorted(want - set(sd)), sorted(set(sd) - want)
    if foreign:
        raise ValueError(f"foreign keys for a {cfg.layers}-layer CLIP text encoder: {foreign[:8]}")
    if missing:
        raise ValueError(f"missing keys of the CLIP text encoder: {missing[:8]}" + (" ..." if len(missing) > 8 else ""))


def _read_state_dict(path: str) -> Dict[str, torch.Tensor]:
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    return torch.load(path, map_location="cpu", weights_only=False)


def load_text_encoder(path: str) -> Tuple[TextConfig, Dict[str, torch.Tensor], Optional[str]]:
    """-> (geometry, normalised state_dict, tokenizer folder of a pipeline root or None)."""
    tok_dir, config = None, None
    if os.path.isdir(path) and os.path.isdir(os.path.join(path, "text_encoder")):      # pipeline root
        if os.path.isdir(os.path.join(path, "tokenizer")):
            tok_dir = os.path.join(path, "tokenizer")
        path = os.path.join(path, "text_encoder")
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
        raise FileNotFoundError(path)
    sd = normalize_text_state_dict(sd)
    cfg = infer_text_config(sd, config)
    check_text_state_dict(sd, cfg)
    return cfg, sd, tok_dir


class TextEncoder:
    """Tokenizer + HIP text transformer: ``encode(prompts) -> [n, L, D]`` fp32 on the device."""

    def __init__(self, path: str, tokenizer_path: Optional[str] = None, device=None, max_prompts: int = 8):
        from .hip import LocoTextEngine
        self.cfg, sd, tok_dir = load_text_encoder(path)
        tok_dir = tokenizer_path or tok_dir
        if not tok_dir:
            raise ValueError(f"{path} is not a pipeline root (text_encoder/ + tokenizer/): pass --tokenizer_path")
        self.tokenizer = CLIPTokenizer.from_dir(tok_dir)
        if self.tokenizer.model_max_length != self.cfg.positions:
            raise ValueError(f"tokenizer model_max_length {self.tokenizer.model_max_length} != the encoder's "
                             f"max_position_embeddings {self.cfg.positions}")
        self.engine = LocoTextEngine(self.cfg, max_prompts=max_prompts, device=device)
        self.engine.load_state_dict(sd)
        self.device = self.engine.device

    @property
    def width(self) -> int:
        return self.cfg.width

    @property
    def length(self) -> int:
        return self.cfg.positions

    def encode(self, prompts: List[str]) -> torch.Tensor:
        ids = self.tokenizer.batch(list(prompts))
        mp = self.engine.max_prompts
        outs = [self.engine.encode_ids(ids[i:i + mp]) for i in range(0, ids.shape[0], mp)]
        return outs[0] if len(outs) == 1 else torch.cat(outs)
