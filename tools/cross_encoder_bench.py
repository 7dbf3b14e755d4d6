"""Pairs/s of CrossEncoder.predict at stsb-roberta-large dimensions (24 layers, H 1024, 16 heads, I 4096, vocabulary
50265), seeded random weights, on the reference's workload shape: one query against N corpus captions
(models/evaluators.py:501-508), pair lengths drawn from 20-60 tokens, batch_size 32 (predict's default, which the reference
uses) and 256. Next to it: transformers' RobertaForSequenceClassification run eagerly in bf16 on the same GPU with the same
weights, batched as sentence-transformers 2.2.2 batches it (input order), and the largest score difference between the two.

    python tools/cross_encoder_bench.py [--pairs 4096] [--layers 24] [--out result.json]
    python tools/cross_encoder_bench.py --profile-batch 32     # one predict() batch after a warm-up (for rocprofv3)

Needs a HIP device; there is no CPU path.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def word_list(n_words: int, seed: int):
    rng = np.random.default_rng(seed)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    return sorted({"".join(rng.choice(letters, rng.integers(3, 8))) for _ in range(n_words)})


def make_pairs(n: int, words, seed: int):
    """One query, n captions; query 8 words, caption 8-48 words: with one token per word (the tokenizer below holds every
    word whole) a pair is 20-60 tokens with <s> q </s></s> d </s>."""
    rng = np.random.default_rng(seed)
    q = " ".join(rng.choice(words, 8))
    return [[q, " ".join(rng.choice(words, int(rng.integers(8, 49))))] for _ in range(n)]


def build_checkpoint(d: str, layers: int, seed: int):
    import transformers as T
    from tokenizers import Tokenizer, models, pre_tokenizers, processors
    words = word_list(600, seed)
    vocab = {t: i for i, t in enumerate(["<s>", "<pad>", "</s>", "<unk>", "<mask>"])}
    for w in words:
        vocab[w] = len(vocab)
    # whole words: one token per word, so the pair lengths are what make_pairs draws
    tok = Tokenizer(models.WordLevel(vocab=vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    tok.post_processor = processors.RobertaProcessing(("</s>", 2), ("<s>", 0))
    tok.save(os.path.join(d, "tokenizer.json"))
    json.dump({"tokenizer_class": "PreTrainedTokenizerFast", "bos_token": "<s>", "eos_token": "</s>", "sep_token": "</s>",
               "cls_token": "<s>", "unk_token": "<unk>", "pad_token": "<pad>", "mask_token": "<mask>",
               "model_max_length": 512}, open(os.path.join(d, "tokenizer_config.json"), "w"))
    cfg = T.RobertaConfig(vocab_size=50265, hidden_size=1024, num_hidden_layers=layers, num_attention_heads=16,
                          intermediate_size=4096, max_position_embeddings=514, type_vocab_size=1, pad_token_id=1,
                          bos_token_id=0, eos_token_id=2, layer_norm_eps=1e-5, num_labels=1,
                          architectures=["RobertaForSequenceClassification"])
    torch.manual_seed(seed)
    with torch.device("cuda"):
        model = T.RobertaForSequenceClassification(cfg)
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("LayerNorm.weight"):
                p.copy_(1.0 + 0.05 * torch.randn(p.shape, generator=g, device="cuda"))
            elif name.endswith("bias"):
                p.copy_(0.02 * torch.randn(p.shape, generator=g, device="cuda"))
            else:
                p.copy_(0.02 * torch.randn(p.shape, generator=g, device="cuda"))
    model.eval()
    model.save_pretrained(d, safe_serialization=True)
    return model, words


def hf_predict(model, tok, pairs, batch_size):
    """sentence-transformers 2.2.2 CrossEncoder.predict over a transformers model: input order, Sigmoid."""
    out = []
    with torch.no_grad():
        for s in range(0, len(pairs), batch_size):
            b = pairs[s:s + batch_size]
            f = tok([p[0].strip() for p in b], [p[1].strip() for p in b], padding=True, truncation="longest_first",
                    return_tensors="pt", max_length=512)
            f = {k: v.cuda() for k, v in f.items()}
            out.append(torch.sigmoid(model(**f).logits.float())[:, 0])
    return torch.cat(out)


def timed(fn, repeat):
    torch.cuda.synchronize()
    best, res = None, None
    for _ in range(repeat):
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--batch-sizes", default="32,256")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--profile-batch", type=int, default=0, help="run one predict() batch of this size after a warm-up")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cross_encoder_bench needs a HIP device"
    from transformers import AutoTokenizer
    from quadruplet_sentence_transformer_amd.cross_encoder import CrossEncoder
    d = tempfile.mkdtemp(prefix="ce_bench_")
    try:
        run(a, d)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def run(a, d):
    from transformers import AutoTokenizer
    from quadruplet_sentence_transformer_amd.cross_encoder import CrossEncoder
    model, words = build_checkpoint(d, a.layers, a.seed)
    pairs = make_pairs(a.pairs, words, a.seed + 1)
    ce = CrossEncoder(d)
    if a.profile_batch:
        del model
        torch.cuda.empty_cache()
        ce.predict(pairs[:a.profile_batch], batch_size=a.profile_batch)
        torch.cuda.synchronize()
        ce.predict(pairs[a.profile_batch:2 * a.profile_batch], batch_size=a.profile_batch)
        torch.cuda.synchronize()
        print(json.dumps({"profiled_batch": a.profile_batch}))
        return
    tok = AutoTokenizer.from_pretrained(d, local_files_only=True)
    lens = [len(x) for x in tok([p[0] for p in pairs], [p[1] for p in pairs])["input_ids"]]
    # parity at full depth on a subset: bf16x3 against transformers in fp32
    sub = pairs[:64]
    ref32 = hf_predict(model, tok, sub, 32).cpu().numpy()
    x3 = ce.predict(sub, batch_size=32, precision="bf16x3")
    model = model.to(torch.bfloat16)
    res = {"workload": {"layers": a.layers, "hidden": 1024, "heads": 16, "intermediate": 4096, "pairs": a.pairs,
                        "tokens_min": int(min(lens)), "tokens_mean": float(np.mean(lens)), "tokens_max": int(max(lens)),
                        "gflop_per_pair_at_mean_len": None},
           "bf16x3_vs_hf_fp32_max_abs_diff_64_pairs": float(np.abs(x3 - ref32).max()),
           "device": torch.cuda.get_device_name(0), "runs": []}
    Lm = float(np.mean(lens))
    res["workload"]["gflop_per_pair_at_mean_len"] = a.layers * Lm * (8 * 1024 ** 2 + 4 * 1024 * 4096 + 4 * Lm * 1024) / 1e9
    for bs in [int(x) for x in a.batch_sizes.split(",")]:
        ce.predict(pairs[:2 * bs], batch_size=bs)                      # warm-up: every shape loads its code objects
        hf_predict(model, tok, pairs[:2 * bs], bs)
        t_ours, ours = timed(lambda: ce.predict(pairs, batch_size=bs), a.repeat)
        t_hf, hf = timed(lambda: hf_predict(model, tok, pairs, bs).cpu().numpy(), a.repeat)
        run = {"batch_size": bs, "qst_bf16_pairs_per_s": a.pairs / t_ours, "hf_eager_bf16_pairs_per_s": a.pairs / t_hf,
               "speedup": t_hf / t_ours, "max_abs_score_diff_vs_hf_bf16": float(np.abs(ours - hf).max()),
               "qst_s": t_ours, "hf_s": t_hf}
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=2)


if __name__ == "__main__":
    main()
