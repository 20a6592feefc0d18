"""Writes tests/golden/clip_text/ (run by hand where `transformers` is installed; not collected by pytest):

* tokenizer_sd1/, tokenizer_sd2/: a synthetic byte-level vocabulary (the 256 byte symbols with and without </w>, the merges
  learned on a small corpus, the two special tokens), its merges, and the configs of the two pad conventions
  (SD 1.x: pad <|endoftext|>; SD 2.x: pad "!" = id 0), model_max_length 77;
* ids.json: the ids transformers.CLIPTokenizer gives for STRINGS under both conventions;
* tiny_quick_gelu.pt / tiny_gelu.pt: two small CLIPTextModels (width 32 / 2 layers / quick_gelu and width 48 / 3 layers /
  gelu, 77 positions): config, state_dict in `text_model.` naming, a batch of id rows and their last_hidden_state.

    python tests/make_golden_clip_text.py
"""
import collections
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "clip_text")

STRINGS = [
    "", "a photo of a man", "a photo of a man wearing glasses", "A PHOTO OF A MAN", "a   photo\tof\n\na  man  ",
    "  leading and trailing   ", "hello, world! how's it going?", "don't we'll they're i'm you've he'd",
    "digits 0123456789 and 3.14159", "punctuation!!! ...??? (brackets) [square] {curly} #hash @at",
    "café naïve résumé", "Ünïcödé ÄÖÜ straße", "日本語のテキスト", "emoji 😀 test 🚀",
    "mixed123abc 4x4 1st 2nd", "a photo of a cat, oil painting, trending on artstation",
    "tabs\tand non-breaking spaces", "quotes \"double\" 'single' `back`",
    " ".join(["word%d" % i for i in range(60)]) + " a very long prompt that runs past the seventy-seven token limit",
    "the quick brown fox jumps over the lazy dog",
]
CORPUS = ("a photo of a man wearing glasses the quick brown fox jumps over the lazy dog a photo of a cat oil painting "
          "trending on artstation hello world how is it going portrait of a woman with red hair smiling landscape with "
          "mountains and a lake at sunset high quality detailed digital art photograph of people walking in the city ") * 3


def learn_merges(n_merges):
    from loco_edit_amd.text_encoder import bytes_to_unicode, split_words
    be = bytes_to_unicode()
    words = collections.Counter()
    for w in split_words(CORPUS.lower()):
        sym = [be[b] for b in w.encode("utf-8")]
        words[tuple(sym[:-1] + [sym[-1] + "</w>"])] += 1
    merges = []
    for _ in range(n_merges):
        pairs = collections.Counter()
        for w, c in words.items():
            for p in zip(w[:-1], w[1:]):
                pairs[p] += c
        if not pairs:
            break
        best = max(pairs.items(), key=lambda kv: (kv[1], kv[0]))[0]
        merges.append(best)
        nw = collections.Counter()
        for w, c in words.items():
            out, i = [], 0
            while i < len(w):
                if i + 1 < len(w) and (w[i], w[i + 1]) == best:
                    out.append(w[i] + w[i + 1]); i += 2
                else:
                    out.append(w[i]); i += 1
            nw[tuple(out)] += c
        words = nw
    return merges


def write_tokenizer(path, vocab, merges, pad):
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "vocab.json"), "w", encoding="utf-8") as f:
        json.dump(vocab, f, ensure_ascii=False)
    with open(os.path.join(path, "merges.txt"), "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "".join(f"{a} {b}\n" for a, b in merges))
    special = {"bos_token": "<|startoftext|>", "eos_token": "<|endoftext|>", "unk_token": "<|endoftext|>", "pad_token": pad}
    with open(os.path.join(path, "special_tokens_map.json"), "w") as f:
        json.dump(special, f)
    with open(os.path.join(path, "tokenizer_config.json"), "w") as f:
        json.dump(dict(special, model_max_length=77, do_lower_case=True, tokenizer_class="CLIPTokenizer"), f)


def main():
    import transformers
    from loco_edit_amd.text_encoder import bytes_to_unicode
    be = bytes_to_unicode()
    syms = list(be.values())
    merges = learn_merges(300)
    vocab_list = syms + [s + "</w>" for s in syms] + ["".join(m) for m in merges] + ["<|startoftext|>", "<|endoftext|>"]
    vocab = {}
    for t in vocab_list:
        vocab.setdefault(t, len(vocab))
    ids = {"strings": STRINGS}
    for name, pad in (("sd1", "<|endoftext|>"), ("sd2", "!")):
        d = os.path.join(OUT, f"tokenizer_{name}")
        write_tokenizer(d, vocab, merges, pad)
        tok = transformers.CLIPTokenizer.from_pretrained(d)
        ids[name] = [tok(s, padding="max_length", max_length=tok.model_max_length, truncation=True).input_ids for s in STRINGS]
    with open(os.path.join(OUT, "ids.json"), "w") as f:
        json.dump(ids, f)
    rows = torch.tensor(ids["sd1"][:3] + ids["sd2"][3:5], dtype=torch.int64)
    g = torch.Generator().manual_seed(5)
    rows = torch.cat([rows, torch.randint(0, len(vocab), (1, 77), generator=g)])
    for name, width, layers, heads, act in (("tiny_quick_gelu", 32, 2, 2, "quick_gelu"), ("tiny_gelu", 48, 3, 3, "gelu")):
        cfg = transformers.CLIPTextConfig(vocab_size=len(vocab), hidden_size=width, intermediate_size=2 * width,
                                          num_hidden_layers=layers, num_attention_heads=heads, max_position_embeddings=77,
                                          hidden_act=act, layer_norm_eps=1e-5, projection_dim=width,
                                          pad_token_id=1, bos_token_id=vocab["<|startoftext|>"], eos_token_id=vocab["<|endoftext|>"])
        torch.manual_seed(11 + width)
        model = transformers.CLIPTextModel(cfg).eval()
        with torch.no_grad():      # layer norms and biases away from their 1 / 0 initialisation
            for k, v in model.named_parameters():
                if "norm" in k or k.endswith("bias"):
                    v.add_(0.1 * torch.randn(v.shape))
            hs = model(input_ids=rows).last_hidden_state
        # `text_model.` naming (that of transformers 4.x checkpoints and of diffusers' text_encoder/ files)
        sd = {(k if k.startswith("text_model.") else "text_model." + k): v.clone() for k, v in model.state_dict().items()}
        keep = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
                "max_position_embeddings", "hidden_act", "layer_norm_eps")
        torch.save({"config": {k: getattr(cfg, k) for k in keep}, "state_dict": sd, "ids": rows, "last_hidden_state": hs},
                   os.path.join(OUT, f"{name}.pt"))
    print("wrote", OUT, "transformers", transformers.__version__)


if __name__ == "__main__":
    main()
