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

The T5 (v1.1) encoder of the DeepFloyd IF path (``IFPipeline.encode_prompt``; reference ``src/modules/edit.py:1274-1284``)
goes through the same calls (``csrc/t5enc.hip``):

* ``T5Tokenizer``: unigram Viterbi segmentation in pure Python, the ids of ``transformers.T5Tokenizer`` built from the
  same (piece, score) list: words split on white space, each prefixed with ``▁``, unknown stretches -> ``<unk>``, ``</s>``
  appended, truncation to L with ``</s>`` kept last, padding with id 0; ids and lengths.  It reads ``tokenizer.json``
  (Unigram model) or ``spiece.model`` (protobuf wire format, piece list only).  The text is NFKC-normalised with
  ``unicodedata``: identical to sentencepiece's ``nmt_nfkc`` map for ASCII, approximate beyond.
* ``load_text_encoder`` recognises a T5 encoder (``model_type`` ``t5`` in ``config.json``, or ``SelfAttention`` keys in a
  bare file) and returns a ``T5Config``; a sharded checkpoint (``*.index.json``) comes back as ``T5Shards`` and is read
  one shard at a time.
* IF's preprocessing (``clean_caption=False``: lower case, strip; 77 tokens, padded, attention mask) is restated from
  the published diffusers pipeline, which is not pinned by a test here.
"""
from __future__ import annotations

import json
import math
import os
import re
import struct
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


# ------------------------------------------------------------------------------------------------------------------- T5
class TextEncoderKindError(NotImplementedError):
    """The checkpoint holds the other kind of text encoder than the path needs."""


@dataclass(frozen=True)
class T5Config:
    vocab: int = 32128
    d_model: int = 4096
    d_kv: int = 64
    heads: int = 64
    d_ff: int = 10240
    layers: int = 24
    positions: int = 77             # L: not a property of the checkpoint (no position embedding); IF pads to 77
    buckets: int = 32
    max_distance: int = 128
    act: str = "gated-gelu"         # wo(gelu_new(wi_0 x) * wi_1 x): T5 v1.1
    ln_eps: float = 1e-6

    @property
    def inner(self) -> int:
        return self.heads * self.d_kv


T5_XXL = T5Config()


def t5_relative_bucket(rel: int, buckets: int = 32, max_distance: int = 128) -> int:
    """``T5Attention._relative_position_bucket(k - q, bidirectional=True)`` for one offset, in double precision (the
    same formula as csrc/t5enc.hip t5_bucket)."""
    nb = buckets // 2
    ret = nb if rel > 0 else 0
    n = abs(rel)
    max_exact = nb // 2
    if n < max_exact:
        return ret + n
    large = max_exact + int(math.log(n / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact))
    return ret + min(large, nb - 1)


def t5_param_shapes(cfg: T5Config) -> Dict[str, Tuple[int, ...]]:
    D, I, F = cfg.d_model, cfg.inner, cfg.d_ff
    out = {"shared.weight": (cfg.vocab, D)}
    for i in range(cfg.layers):
        p = f"encoder.block.{i}.layer."
        out[p + "0.layer_norm.weight"] = (D,)
        for m in "qkv":
            out[p + f"0.SelfAttention.{m}.weight"] = (I, D)
        out[p + "0.SelfAttention.o.weight"] = (D, I)
        if i == 0:
            out[p + "0.SelfAttention.relative_attention_bias.weight"] = (cfg.buckets, cfg.heads)
        out[p + "1.layer_norm.weight"] = (D,)
        out[p + "1.DenseReluDense.wi_0.weight"] = (F, D)
        out[p + "1.DenseReluDense.wi_1.weight"] = (F, D)
        out[p + "1.DenseReluDense.wo.weight"] = (D, F)
    out["encoder.final_layer_norm.weight"] = (D,)
    return out


_T5_EMBED = ("shared.weight", "encoder.embed_tokens.weight")


def _t5_name(k: str) -> Optional[str]:
    """Normalised T5EncoderModel name of a checkpoint key; None for keys that are not the encoder's (decoder, lm_head)."""
    if k.startswith("text_encoder."):
        k = k[len("text_encoder."):]
    if k.startswith(("decoder.", "lm_head.")):
        return None
    if k.startswith(("block.", "final_layer_norm.", "embed_tokens.")):      # a bare T5Stack: the `encoder.` level is missing
        k = "encoder." + k
    return "shared.weight" if k in _T5_EMBED else k


def normalize_t5_state_dict(sd: Dict[str, torch.Tensor], upcast: bool = True) -> Dict[str, torch.Tensor]:
    """Keys of a T5EncoderModel, of a pipeline (``text_encoder.*``) or of a bare encoder stack (``block.*``) -> the
    T5EncoderModel naming; the tied embedding under either of its names -> ``shared.weight``; fp16 / bf16 -> fp32
    (``upcast=False`` leaves that to the engine's loader, which converts one tensor at a time).
    Keys outside an encoder are refused (a full T5's decoder and lm_head are dropped)."""
    sd = sd.get("state_dict", sd) if isinstance(sd.get("state_dict", None), dict) else sd
    out, foreign = {}, []
    for k, v in sd.items():
        n = _t5_name(k)
        if n is None:
            continue
        if not (n == "shared.weight" or n.startswith(("encoder.block.", "encoder.final_layer_norm."))):
            foreign.append(k); continue
        if n == "shared.weight" and n in out and k.endswith("embed_tokens.weight"):
            continue                               # the tied copy
        out[n] = v.to(torch.float32) if upcast and torch.is_tensor(v) and v.is_floating_point() else v
    if foreign:
        raise ValueError(f"not a T5 encoder state_dict: foreign keys {sorted(foreign)[:8]}")
    return out


def infer_t5_config(sd: Dict[str, torch.Tensor], config: Optional[dict] = None, positions: int = 77) -> T5Config:
    """Geometry from a transformers ``config.json`` when given, else from the shapes of the normalised state_dict
    (max_distance 128 and eps 1e-6, which no shape shows)."""
    if config is not None:
        act = config.get("feed_forward_proj", "relu")
        if act != "gated-gelu":
            raise ValueError(f"feed_forward_proj {act!r}: the T5 encoder builds gated-gelu (T5 v1.1) only")
        return T5Config(vocab=int(config["vocab_size"]), d_model=int(config["d_model"]), d_kv=int(config["d_kv"]),
                        heads=int(config["num_heads"]), d_ff=int(config["d_ff"]), layers=int(config["num_layers"]),
                        positions=int(positions), buckets=int(config.get("relative_attention_num_buckets", 32)),
                        max_distance=int(config.get("relative_attention_max_distance", 128)), act=act,
                        ln_eps=float(config.get("layer_norm_epsilon", 1e-6)))
    p0 = "encoder.block.0.layer."
    need = ("shared.weight", p0 + "0.SelfAttention.q.weight", p0 + "0.SelfAttention.relative_attention_bias.weight",
            p0 + "1.DenseReluDense.wi_0.weight")
    missing = [k for k in need if k not in sd]
    if missing:
        raise ValueError(f"missing keys of the T5 encoder: {missing}")
    tok, q, rel, wi = (sd[k] for k in need)
    heads = int(rel.shape[1])
    if q.shape[0] % heads:
        raise ValueError(f"q rows {q.shape[0]} are not a multiple of the {heads} heads of relative_attention_bias")
    layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.block."))
    return T5Config(vocab=int(tok.shape[0]), d_model=int(tok.shape[1]), d_kv=int(q.shape[0]) // heads, heads=heads,
                    d_ff=int(wi.shape[0]), layers=layers, positions=int(positions), buckets=int(rel.shape[0]))


def check_t5_names(names, cfg: T5Config):
    want = set(t5_param_shapes(cfg))
    missing, foreign = sorted(want - set(names)), sorted(set(names) - want)
    if foreign:
        raise ValueError(f"foreign keys for a {cfg.layers}-block T5 encoder: {foreign[:8]}")
    if missing:
        raise ValueError(f"missing keys of the T5 encoder: {missing[:8]}" + (" ..." if len(missing) > 8 else ""))


def check_t5_state_dict(sd: Dict[str, torch.Tensor], cfg: T5Config):
    check_t5_names(sd.keys(), cfg)
    for k, shape in t5_param_shapes(cfg).items():
        if tuple(sd[k].shape) != shape:
            raise ValueError(f"{k} has shape {tuple(sd[k].shape)}, the geometry asks for {shape}")


class T5Shards:
    """The state_dict of a sharded checkpoint folder (``*.index.json`` + its shards): ``names`` from the index, the
    tensors by iterating -- one normalised shard at a time in its stored dtype (the engine's loader upcasts tensor by
    tensor), so the host never holds the whole encoder, let alone twice."""

    def __init__(self, folder: str, index_file: str):
        self.folder = folder
        with open(os.path.join(folder, index_file)) as f:
            wm = json.load(f)["weight_map"]
        self.files = sorted(set(wm.values()))
        self.names = sorted({n for n in map(_t5_name, wm) if n is not None})

    def __iter__(self):
        for fn in self.files:
            yield normalize_t5_state_dict(_read_state_dict(os.path.join(self.folder, fn)), upcast=False)


def read_spiece_model(path: str) -> List[Tuple[str, float]]:
    """(piece, score) of every entry of a sentencepiece ``ModelProto`` file: field 1 (repeated SentencePiece: 1 piece
    string, 2 score float, 3 type), read from the protobuf wire format; everything else is skipped."""
    with open(path, "rb") as f:
        buf = f.read()

    def varint(i):
        v, sh = 0, 0
        while True:
            b = buf[i]; i += 1
            v |= (b & 0x7F) << sh; sh += 7
            if not b & 0x80:
                return v, i

    def fields(i, end):
        while i < end:
            key, i = varint(i)
            fno, wt = key >> 3, key & 7
            if wt == 0:
                v, i = varint(i)
            elif wt == 1:
                v, i = buf[i:i + 8], i + 8
            elif wt == 2:
                n, i = varint(i)
                v, i = (i, i + n), i + n
            elif wt == 5:
                v, i = buf[i:i + 4], i + 4
            else:
                raise ValueError(f"{path}: wire type {wt} is not that of a sentencepiece model")
            yield fno, wt, v
    out = []
    for fno, wt, v in fields(0, len(buf)):
        if fno != 1 or wt != 2:
            continue
        piece, score = "", 0.0
        for g, w, x in fields(*v):
            if g == 1 and w == 2:
                piece = buf[x[0]:x[1]].decode("utf-8")
            elif g == 2 and w == 5:
                score = struct.unpack("<f", x)[0]
        out.append((piece, score))
    if not out:
        raise ValueError(f"{path}: no pieces found")
    return out


class T5Tokenizer:
    """Unigram segmentation with the (piece, score) list of a T5 ``tokenizer/`` folder; ids 0 / 1 / 2 are
    ``<pad>`` / ``</s>`` / ``<unk>`` as in every T5 vocabulary."""
    UNK_PENALTY = 10.0

    def __init__(self, pieces: List[Tuple[str, float]], model_max_length: int = 77, eos_token: str = "</s>",
                 unk_token: str = "<unk>", pad_token: str = "<pad>"):
        self.pieces = [(str(p), float(s)) for p, s in pieces]
        self.encoder: Dict[str, int] = {}
        for i, (p, _) in enumerate(self.pieces):
            self.encoder.setdefault(p, i)
        for name, tok in (("eos", eos_token), ("unk", unk_token), ("pad", pad_token)):
            if tok not in self.encoder:
                raise ValueError(f"{name} token {tok!r} is not in the vocabulary")
        self.eos_token_id, self.unk_token_id, self.pad_token_id = (self.encoder[t] for t in (eos_token, unk_token, pad_token))
        self.score = {p: s for p, s in reversed(self.pieces)}          # first entry of a repeated piece wins
        self.max_len = max(len(p) for p, _ in self.pieces)
        self.unk_score = min(s for _, s in self.pieces) - self.UNK_PENALTY
        self.model_max_length = int(model_max_length)
        self.cache: Dict[str, List[int]] = {}

    @classmethod
    def from_dir(cls, path: str, model_max_length: int = 77) -> "T5Tokenizer":
        tj, sp = os.path.join(path, "tokenizer.json"), os.path.join(path, "spiece.model")
        if os.path.exists(tj):
            with open(tj, encoding="utf-8") as f:
                model = json.load(f)["model"]
            if model.get("type", "Unigram") != "Unigram":
                raise ValueError(f"{tj}: model type {model.get('type')!r}, a Unigram model is needed")
            pieces = [(p, s) for p, s in model["vocab"]]
        elif os.path.exists(sp):
            pieces = read_spiece_model(sp)
        else:
            raise FileNotFoundError(f"{path}: no tokenizer.json or spiece.model")
        return cls(pieces, model_max_length=model_max_length)

    def segment(self, word: str) -> List[int]:
        """Viterbi over the pieces of one word (``▁`` already prefixed): the best-scoring path, a character no piece
        covers costs min_score - 10 and consecutive ones fuse into one ``<unk>`` (tokenizers' Unigram, the first of equal
        candidates is kept)."""
        if word in self.cache:
            return self.cache[word]
        n = len(word)
        best = [0.0] * (n + 1)
        start: List[Optional[int]] = [None] * (n + 1)
        unk = [False] * (n + 1)
        for s0 in range(n):
            if s0 > 0 and start[s0] is None:
                continue
            base, single = best[s0], False
            for e in range(s0 + 1, min(n, s0 + self.max_len) + 1):
                sc = self.score.get(word[s0:e])
                if sc is None:
                    continue
                cand = base + sc
                if start[e] is None or cand > best[e]:
                    best[e], start[e], unk[e] = cand, s0, False
                if e == s0 + 1:
                    single = True
            if not single:
                cand = base + self.unk_score
                if start[s0 + 1] is None or cand > best[s0 + 1]:
                    best[s0 + 1], start[s0 + 1], unk[s0 + 1] = cand, s0, True
        out, e, fused = [], n, False
        while e > 0:
            s0 = start[e]
            if unk[e]:
                if not fused:
                    out.append(self.unk_token_id)
                fused = True
            else:
                out.append(self.encoder.get(word[s0:e], self.unk_token_id))
                fused = False
            e = s0
        out.reverse()
        self.cache[word] = out
        return out

    def tokenize(self, text: str) -> List[int]:
        """Ids of the text without ``</s>``."""
        ids: List[int] = []
        for w in _WS_RUN.split(unicodedata.normalize("NFKC", text)):
            if w:
                ids.extend(self.segment("▁" + w))
        return ids

    def __call__(self, text: str) -> Tuple[List[int], int]:
        """``tokenizer(text, padding="max_length", max_length=L, truncation=True)`` -> (input_ids, sum(attention_mask))"""
        L = self.model_max_length
        ids = self.tokenize(text)[:L - 1] + [self.eos_token_id]
        return ids + [self.pad_token_id] * (L - len(ids)), len(ids)

    def batch(self, texts: List[str]) -> Tuple[torch.Tensor, torch.Tensor]:
        rows = [self(t) for t in texts]
        return torch.tensor([r[0] for r in rows], dtype=torch.int32), torch.tensor([r[1] for r in rows], dtype=torch.int32)


def _is_t5(config: Optional[dict], keys) -> bool:
    if config is not None and (config.get("model_type") == "t5" or any("T5" in a for a in config.get("architectures") or [])):
        return True
    return any(".SelfAttention." in k for k in keys)


def load_text_encoder(path: str, positions: int = 77):
    """-> (geometry, normalised state_dict, tokenizer folder of a pipeline root or None).  The geometry tells the kind:
    a ``TextConfig`` (CLIP) or a ``T5Config`` (then the state_dict of a sharded checkpoint is a ``T5Shards``, and
    ``positions`` is the token count L, which a T5 checkpoint does not fix)."""
    tok_dir, config = None, None
    if os.path.isdir(path) and os.path.isdir(os.path.join(path, "text_encoder")):      # pipeline root
        if os.path.isdir(os.path.join(path, "tokenizer")):
            tok_dir = os.path.join(path, "tokenizer")
        path = os.path.join(path, "text_encoder")
    sd = None
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
            for fn in ("model.safetensors.index.json", "pytorch_model.bin.index.json"):
                if os.path.exists(os.path.join(path, fn)):
                    sd = T5Shards(path, fn)
                    break
            else:
                raise FileNotFoundError(f"{path}: no model.safetensors or pytorch_model.bin (nor a sharded *.index.json)")
    elif os.path.isfile(path):
        sd = _read_state_dict(path)
    else:
        raise FileNotFoundError(path)
    if isinstance(sd, T5Shards):
        if not _is_t5(config, sd.names):
            raise ValueError(f"{path}: sharded checkpoints are read for the T5 encoder only")
        if config is None:
            raise ValueError(f"{path}: a sharded T5 checkpoint needs its config.json")
        cfg = infer_t5_config({}, config, positions=positions)
        check_t5_names(sd.names, cfg)
        return cfg, sd, tok_dir
    inner = sd.get("state_dict", sd) if isinstance(sd.get("state_dict", None), dict) else sd
    if _is_t5(config, inner.keys()):
        sd = normalize_t5_state_dict(inner)
        cfg = infer_t5_config(sd, config, positions=positions)
        check_t5_state_dict(sd, cfg)
        return cfg, sd, tok_dir
    sd = normalize_text_state_dict(sd)
    cfg = infer_text_config(sd, config)
    check_text_state_dict(sd, cfg)
    return cfg, sd, tok_dir


class TextEncoder:
    """Tokenizer + HIP text transformer: ``encode(prompts) -> [n, L, D]`` fp32 on the device.  ``kind`` is ``"clip"`` or
    ``"t5"`` after the checkpoint; ``positions`` is the token count L of a T5 encoder (CLIP fixes its own)."""

    def __init__(self, path: str, tokenizer_path: Optional[str] = None, device=None, max_prompts: int = 8, positions: int = 77,
                 expect: Optional[str] = None):
        from .hip import LocoTextEngine
        self.cfg, sd, tok_dir = load_text_encoder(path, positions=positions)
        self.kind = "t5" if isinstance(self.cfg, T5Config) else "clip"
        if expect is not None and self.kind != expect:
            raise TextEncoderKindError(f"{path} holds a {self.kind.upper()} text encoder, a {expect.upper()} encoder is needed here")
        tok_dir = tokenizer_path or tok_dir
        if not tok_dir:
            raise ValueError(f"{path} is not a pipeline root (text_encoder/ + tokenizer/): pass --tokenizer_path")
        if self.kind == "t5":
            self.tokenizer = T5Tokenizer.from_dir(tok_dir, model_max_length=self.cfg.positions)
            if len(self.tokenizer.pieces) > self.cfg.vocab:
                raise ValueError(f"tokenizer has {len(self.tokenizer.pieces)} pieces, the encoder's embedding {self.cfg.vocab} rows")
        else:
            self.tokenizer = CLIPTokenizer.from_dir(tok_dir)
            if self.tokenizer.model_max_length != self.cfg.positions:
                raise ValueError(f"tokenizer model_max_length {self.tokenizer.model_max_length} != the encoder's "
                                 f"max_position_embeddings {self.cfg.positions}")
        self.engine = LocoTextEngine(self.cfg, max_prompts=max_prompts, device=device)
        if isinstance(sd, T5Shards):
            for part in sd:                      # one shard on the host at a time
                self.engine.load_params(part)
            self.engine.check_complete()
        else:
            self.engine.load_state_dict(sd)
        self.device = self.engine.device

    @property
    def width(self) -> int:
        return self.cfg.d_model if self.kind == "t5" else self.cfg.width

    @property
    def length(self) -> int:
        return self.cfg.positions

    @staticmethod
    def preprocess_if(prompt: str) -> str:
        """IFPipeline._text_preprocessing with clean_caption=False (the default of encode_prompt)."""
        return prompt.lower().strip()

    def encode(self, prompts: List[str]) -> torch.Tensor:
        mp = self.engine.max_prompts
        if self.kind == "t5":
            ids, lens = self.tokenizer.batch([self.preprocess_if(p) for p in prompts])
            outs = [self.engine.encode_ids(ids[i:i + mp], lens=lens[i:i + mp]) for i in range(0, ids.shape[0], mp)]
        else:
            ids = self.tokenizer.batch(list(prompts))
            outs = [self.engine.encode_ids(ids[i:i + mp]) for i in range(0, ids.shape[0], mp)]
        return outs[0] if len(outs) == 1 else torch.cat(outs)
