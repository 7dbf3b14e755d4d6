"""Tiny seeded *ForSequenceClassification checkpoints written with the installed transformers, for the cross-encoder tests
(test_cross_encoder_host.py, test_gpu_cross_encoder.py). Everything is built offline: BERT over tests/golden/tiny_vocab.txt,
RoBERTa / XLM-R over a byte-level BPE trained here with `tokenizers`."""
import json
import os
import shutil

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROBERTA_VOCAB = 300          # embedding rows of the RoBERTa fixtures (the BPE below has 290 entries)

CORPUS = ["a man rides a horse in the park", "two dogs are playing with a ball", "a woman is slicing an onion",
          "children play near the old bridge", "the cat sleeps on a red sofa", "a group of people walk down the street",
          "someone is playing the guitar", "a boy jumps into the lake", "the train arrives at the station",
          "a chef cooks pasta in a small kitchen"]


def bpe_tokenizer_files(d: str, vocab_size: int = 290) -> None:
    """A byte-level BPE (RoBERTa's scheme) trained on CORPUS with RobertaProcessing: tokenizer.json plus a
    tokenizer_config.json naming RobertaTokenizer, which AutoTokenizer loads offline. <s>=0, <pad>=1, </s>=2. The 256 byte
    symbols and the 5 specials come first: ROBERTA_VOCAB rows hold every id."""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=["<s>", "<pad>", "</s>", "<unk>", "<mask>"],
                                  initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tok.train_from_iterator(CORPUS, trainer)
    tok.post_processor = processors.RobertaProcessing(("</s>", tok.token_to_id("</s>")), ("<s>", tok.token_to_id("<s>")))
    tok.save(os.path.join(d, "tokenizer.json"))
    json.dump({"tokenizer_class": "RobertaTokenizer", "bos_token": "<s>", "eos_token": "</s>", "sep_token": "</s>",
               "cls_token": "<s>", "unk_token": "<unk>", "pad_token": "<pad>", "mask_token": "<mask>",
               "model_max_length": 64}, open(os.path.join(d, "tokenizer_config.json"), "w"))


def _randomise(model, seed: int) -> None:
    """Every weight away from its init (LayerNorm gains and biases included), so a tensor in the wrong place shows."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("LayerNorm.weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.08 * torch.randn(p.shape, generator=g))


def make_checkpoint(d: str, kind: str, num_labels: int = 1, seed: int = 0, hidden: int = 64, heads: int = 2,
                    layers: int = 2, intermediate: int = 256, extra_config: dict = None):
    """Write a tiny `kind` ("bert", "roberta", "xlm-roberta") *ForSequenceClassification to directory d; return the model
    (eval mode, fp32, on the CPU)."""
    import transformers as T
    os.makedirs(d, exist_ok=True)
    common = dict(hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=intermediate,
                  hidden_act="gelu", num_labels=num_labels, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    if kind == "bert":
        shutil.copy(os.path.join(ROOT, "tests", "golden", "tiny_vocab.txt"), os.path.join(d, "vocab.txt"))
        json.dump({"tokenizer_class": "BertTokenizer", "do_lower_case": True, "model_max_length": 64},
                  open(os.path.join(d, "tokenizer_config.json"), "w"))
        cfg = T.BertConfig(vocab_size=128, max_position_embeddings=64, type_vocab_size=2, pad_token_id=0, **common)
        model = T.BertForSequenceClassification(cfg)
    else:
        bpe_tokenizer_files(d)
        C = T.RobertaConfig if kind == "roberta" else T.XLMRobertaConfig
        cfg = C(vocab_size=ROBERTA_VOCAB, max_position_embeddings=66, type_vocab_size=1, pad_token_id=1, bos_token_id=0,
                eos_token_id=2, layer_norm_eps=1e-5, **common)
        model = (T.RobertaForSequenceClassification if kind == "roberta" else T.XLMRobertaForSequenceClassification)(cfg)
    _randomise(model, seed)
    model.eval()
    model.save_pretrained(d, safe_serialization=True)
    if extra_config:
        p = os.path.join(d, "config.json")
        c = json.load(open(p))
        c.update(extra_config)
        json.dump(c, open(p, "w"), indent=2)
    return model
