"""Writes tests/golden/t5_text/ (run by hand where `transformers` and `sentencepiece` are installed; not collected by
pytest, neither package is needed afterwards):

* tokenizer/spiece.model, tokenizer/tokenizer.json: one small unigram vocabulary trained by sentencepiece on CORPUS
  (<pad> 0, </s> 1, <unk> 2 as in every T5 vocabulary), as the sentencepiece file and as the Unigram model of the
  `tokenizers` library;
* ids.json: PROMPTS with the ids and lengths transformers.T5Tokenizer(vocab=pieces, extra_ids=0) gives at L = 7 and
  L = 77 (padding="max_length", truncation=True), and the relative-position buckets of every offset at L = 128 from
  T5Attention._relative_position_bucket;
* tiny_a.pt (d_model 24, d_kv 8, 4 heads, d_ff 40, 2 blocks, L 7, the tokenizer's vocabulary: the TINY_IF geometry) and
  tiny_b.pt (d_model 64, d_kv 16, 4 heads, d_ff 160, 2 blocks, L 77, 16 ids): config, state_dict, ids, lengths,
  last_hidden_state of T5EncoderModel in float64 (its norm's fp32 mean of squares kept in float64 for that run), and e_ref = the per-prompt rel-L2 of the same model in fp32 against it.

    python tests/make_golden_t5_text.py
"""
import io
import json
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "t5_text")

CORPUS = ("a photo of a man wearing glasses . a photo of a man having curly hair . a photo of a woman with red hair smiling . "
          "the quick brown fox jumps over the lazy dog . a painting of a cat , oil on canvas , trending on artstation . "
          "portrait of an old man with a beard and a hat . landscape with mountains and a lake at sunset , high quality , "
          "detailed digital art . photograph of people walking in the city at night under the rain . a small house near "
          "the river in winter , snow on the roof . two dogs playing with a ball on the beach . a young girl reading a book "
          "in the library . a red car parked in front of a blue building . an astronaut riding a horse on the moon . "
          "close up of a face , sharp focus , studio lighting , 4k . eyes nose mouth ears hair glasses smile beard "
          "hello world how is it going today ? numbers 0 1 2 3 4 5 6 7 8 9 10 25 100 2024 . "
          "making taking walking talking reading painting wearing having smiling playing parked riding ").split()

WORDS = ["a", "photo", "of", "man", "woman", "wearing", "glasses", "having", "curly", "hair", "red", "smiling", "the", "quick",
         "brown", "fox", "dog", "cat", "painting", "oil", "portrait", "old", "beard", "hat", "landscape", "mountains", "lake",
         "sunset", "city", "night", "rain", "house", "river", "winter", "snow", "young", "girl", "book", "car", "blue",
         "building", "astronaut", "horse", "moon", "face", "sharp", "focus", "studio", "4k", "zebra", "quartz", "xylophone",
         "jazz", "vivid", "100", "2024", ",", ".", "?", "with", "and", "in", "on", "at"]


def prompts(script_args):
    out = ["", " ", "a", "A", "a photo of a man", "A photo of a man", "A PHOTO OF A MAN WEARING GLASSES",
           "  leading and trailing   ", "a   photo\tof\n\na  man  ", "tabs\tand\nnewlines", "hello, world! how's it going?",
           "under_score #hash @at ~tilde ^caret {curly} [square] (round) <angle> | \\ / * + = % $ & ; : ' \" `",
           "digits 0123456789 and 3.14159", "UPPER lower MiXeD CaSe", "zzzzqqqqxxxx", "x", "?", "...", "a,b,c", "man.", ".man",
           "wearingglasses", "photophotophoto", "a-photo-of-a-man", "e=mc^2", "100%", "Q", "QQQ", "aQa", "QaQ", "a Q a",
           " ".join(["word%d" % i for i in range(60)]) + " a very long prompt that runs past the seventy-seven token limit",
           " ".join(["a photo of a man wearing glasses"] * 14), "the quick brown fox jumps over the lazy dog " * 6,
           "a " * 100, "glasses " * 9, "one two three four five six seven eight nine ten"]
    for argv in script_args.values():                 # the prompts of the shipped scripts, as typed and as IF sees them
        for flag in ("--for_prompt", "--edit_prompt", "--neg_prompt", "--inv_prompt"):
            if flag in argv:
                p = argv[argv.index(flag) + 1]
                out += [p, p.lower().strip()]
    rng = random.Random(7)
    while len(set(out)) < 240:
        n = rng.choice([1, 2, 3, 4, 5, 6, 8, 12, 20, 40, 90])
        ws = [rng.choice(WORDS) for _ in range(n)]
        if rng.random() < 0.2:
            ws = [w.upper() if rng.random() < 0.5 else w for w in ws]
        sep = rng.choice([" ", " ", " ", "  ", ", "])
        out.append(sep.join(ws))
    seen, uniq = set(), []
    for p in out:
        if p not in seen:
            seen.add(p); uniq.append(p)
    return uniq


def train_vocab():
    import sentencepiece as spm
    buf = io.BytesIO()
    spm.SentencePieceTrainer.train(sentence_iterator=iter([" ".join(CORPUS[i:i + 12]) for i in range(0, len(CORPUS), 12)] * 4),
                                   model_writer=buf, model_type="unigram", vocab_size=320, hard_vocab_limit=False,
                                   pad_id=0, eos_id=1, unk_id=2, bos_id=-1, character_coverage=1.0, num_threads=1,
                                   split_digits=False, byte_fallback=False, add_dummy_prefix=True)
    sp = spm.SentencePieceProcessor(model_proto=buf.getvalue())
    return buf.getvalue(), [(sp.id_to_piece(i), float(sp.get_score(i))) for i in range(sp.get_piece_size())]


def tiny(name, vocab, d_model, d_kv, heads, d_ff, L, ids, lens, seed):
    import transformers
    cfg = transformers.T5Config(vocab_size=vocab, d_model=d_model, d_kv=d_kv, num_heads=heads, d_ff=d_ff, num_layers=2,
                                feed_forward_proj="gated-gelu", relative_attention_num_buckets=32,
                                relative_attention_max_distance=128, layer_norm_epsilon=1e-6, tie_word_embeddings=False,
                                is_encoder_decoder=False, use_cache=False)
    torch.manual_seed(seed)
    model = transformers.T5EncoderModel(cfg).eval()          # T5PreTrainedModel._init_weights through post_init
    with torch.no_grad():
        for k, v in model.named_parameters():
            if "layer_norm" in k:                            # no parameter stays an identity
                v.copy_(1 + 0.1 * torch.randn(v.shape))
    mask = (torch.arange(L)[None] < lens[:, None]).long()
    with torch.no_grad():
        h32 = model(input_ids=ids, attention_mask=mask).last_hidden_state
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        # T5LayerNorm.forward takes its mean of squares in fp32 whatever the dtype (a guard for half precision), which would
        # leave an fp32 rounding (6e-8) in the float64 reference: for this run the same forward without the downcast
        from transformers.models.t5.modeling_t5 import T5LayerNorm
        fwd = T5LayerNorm.forward
        T5LayerNorm.forward = lambda m, x: m.weight * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + m.variance_epsilon))
        try:
            h64 = model.double()(input_ids=ids, attention_mask=mask).last_hidden_state
        finally:
            T5LayerNorm.forward = fwd
    assert h64.dtype == torch.float64
    e_ref = [((h32[i].double() - h64[i]).norm() / h64[i].norm()).item() for i in range(ids.shape[0])]
    keep = {"vocab_size": vocab, "d_model": d_model, "d_kv": d_kv, "num_heads": heads, "d_ff": d_ff, "num_layers": 2,
            "feed_forward_proj": "gated-gelu", "relative_attention_num_buckets": 32, "relative_attention_max_distance": 128,
            "layer_norm_epsilon": 1e-6, "model_type": "t5"}
    path = os.path.join(OUT, f"{name}.pt")
    torch.save({"config": keep, "positions": L, "state_dict": sd, "ids": ids, "lens": lens, "last_hidden_state": h64,
                "e_ref": e_ref}, path)
    print(name, "bytes", os.path.getsize(path), "e_ref", ["%.1e" % e for e in e_ref])


def main():
    import transformers
    from transformers.models.t5.modeling_t5 import T5Attention
    os.makedirs(os.path.join(OUT, "tokenizer"), exist_ok=True)
    proto, pieces = train_vocab()
    with open(os.path.join(OUT, "tokenizer", "spiece.model"), "wb") as f:
        f.write(proto)
    tok = transformers.T5Tokenizer(vocab=pieces, extra_ids=0)
    tok.backend_tokenizer.save(os.path.join(OUT, "tokenizer", "tokenizer.json"))
    with open(os.path.join(ROOT, "tests", "golden", "script_args.json")) as f:
        P = prompts(json.load(f))
    d = {"prompts": P}
    for L in (7, 77):
        enc = [tok(p, padding="max_length", max_length=L, truncation=True) for p in P]
        d[f"L{L}"] = {"ids": [e.input_ids for e in enc], "lens": [int(sum(e.attention_mask)) for e in enc]}
    rel = torch.arange(-127, 128)
    d["buckets_L128"] = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=32, max_distance=128).tolist()
    with open(os.path.join(OUT, "ids.json"), "w") as f:
        json.dump(d, f)
    print(len(P), "prompts,", len(pieces), "pieces")
    # tiny_a: prompts through the tokenizer at L = 7 (lengths 1 ... 7)
    pick = ["", "a", "a photo", "a photo of a man", "A photo of a man wearing glasses", "zebra jazz", "red hair, smiling", "glasses"]
    rows = [tok(p, padding="max_length", max_length=7, truncation=True) for p in pick]
    ids = torch.tensor([r.input_ids for r in rows], dtype=torch.int64)
    lens = torch.tensor([sum(r.attention_mask) for r in rows], dtype=torch.int64)
    assert int(lens.min()) == 1 and int(lens.max()) == 7
    tiny("tiny_a", len(pieces), 24, 8, 4, 40, 7, ids, lens, seed=21)
    # tiny_b: L = 77 (offsets reach the logarithmic buckets), random ids; prompts of length 1 and L (two prompts keep the file
    # under 500 KB: the float64 states are 39 KB per prompt next to 385 KB of weights)
    g = torch.Generator().manual_seed(22)
    ids = torch.randint(3, 16, (2, 77), generator=g)
    lens = torch.tensor([1, 77])
    ids[0, 0] = 1
    ids[0, 1:] = 0
    ids[1, 76] = 1
    tiny("tiny_b", 16, 64, 16, 4, 160, 77, ids, lens, seed=23)
    print("wrote", OUT, "transformers", transformers.__version__)


if __name__ == "__main__":
    main()
