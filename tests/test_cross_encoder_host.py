"""CPU: cross-encoder checkpoints on the host (QST_ARCH_ROBERTA, the head buffer, sentence-transformers 2.2.2's num_labels
and activation rules, pair tokenisation) and the drop-in CrossEncoder's lazy error when no checkpoint exists."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib  # noqa: E402
from quadruplet_sentence_transformer_amd.config import ARCH_ROBERTA, PRESETS, build_layout, hf_param_views  # noqa: E402
from quadruplet_sentence_transformer_amd.cross_encoder import (CrossEncoder, default_activation,  # noqa: E402
                                                               load_checkpoint)
from cross_encoder_fixtures import make_checkpoint  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["bert", "roberta", "xlm-roberta"]


@pytest.fixture(autouse=True)
def _no_device(monkeypatch):
    # host-side behaviour only: never build the device half here, whatever the machine has
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


@pytest.mark.parametrize("kind", KINDS)
def test_every_tensor_lands_in_the_arena_or_the_head_buffer(tmp_path, kind):
    model = make_checkpoint(str(tmp_path), kind, num_labels=3 if kind == "bert" else 1, seed=1)
    ck = load_checkpoint(str(tmp_path))
    cfg = ck.cfg
    assert cfg.pooling == "cls" and not cfg.normalize
    assert cfg.arch == (0 if kind == "bert" else ARCH_ROBERTA)
    if kind != "bert":
        assert (cfg.type_vocab_size, cfg.pad_token_id, cfg.layer_norm_eps, cfg.max_position) == (1, 1, 1e-5, 66)
    sd = {k: v for k, v in model.state_dict().items()}
    prefix = "bert." if kind == "bert" else "roberta."
    so = {s.name: s for s in build_layout(cfg)[0]}
    used = set()
    for name, seg, off, shape in hf_param_views(cfg):
        s = so[seg]
        got = ck.arena[s.offset + off:s.offset + off + int(np.prod(shape))].reshape(shape)
        np.testing.assert_array_equal(got, sd[prefix + name].numpy())
        used.add(prefix + name)
    dense, outp = ("bert.pooler.dense", "classifier") if kind == "bert" else ("classifier.dense", "classifier.out_proj")
    H, C = cfg.hidden_size, ck.num_labels
    for key, name, shape in (("w1", dense + ".weight", (H, H)), ("b1", dense + ".bias", (H,)),
                             ("w2", outp + ".weight", (C, H)), ("b2", outp + ".bias", (C,))):
        o = ck.head_offsets[key]
        assert o % 64 == 0
        np.testing.assert_array_equal(ck.head[o:o + int(np.prod(shape))].reshape(shape), sd[name].numpy())
        used.add(name)
    # nothing of the model is left out (buffers such as position_ids are not parameters)
    assert {n for n, _ in model.named_parameters()} <= used


def test_num_labels_and_default_activation_follow_st(tmp_path):
    make_checkpoint(str(tmp_path / "one"), "roberta", num_labels=1)
    make_checkpoint(str(tmp_path / "three"), "bert", num_labels=3)
    make_checkpoint(str(tmp_path / "cfg"), "roberta", num_labels=1,
                    extra_config={"sbert_ce_default_activation_function": "torch.nn.modules.activation.Tanh"})
    one = CrossEncoder(str(tmp_path / "one"))
    assert one.num_labels == 1 and isinstance(one.default_activation_function, torch.nn.Sigmoid)
    three = CrossEncoder(str(tmp_path / "three"))
    assert three.num_labels == 3 and isinstance(three.default_activation_function, torch.nn.Identity)
    assert isinstance(CrossEncoder(str(tmp_path / "cfg")).default_activation_function, torch.nn.Tanh)
    # an explicit default_activation_function wins over config.json
    own = CrossEncoder(str(tmp_path / "cfg"), default_activation_function=torch.nn.Identity())
    assert isinstance(own.default_activation_function, torch.nn.Identity)
    assert isinstance(default_activation({}, 2), torch.nn.Identity)
    # num_labels must match the trained classifier (no new head is trained here)
    assert CrossEncoder(str(tmp_path / "three"), num_labels=3).num_labels == 3
    with pytest.raises(ValueError):
        CrossEncoder(str(tmp_path / "three"), num_labels=1)
    with pytest.raises(NotImplementedError):
        one.fit([], epochs=1)


def test_unsupported_checkpoints_fail_at_construction(tmp_path):
    # stsb-TinyBERT-L-4's widths: H = 312 (12 heads of 26) is not a multiple of 64 -> a clear error, no torch fallback
    make_checkpoint(str(tmp_path / "w"), "bert", hidden=312, heads=12, intermediate=1200)
    with pytest.raises(_lib.QstError, match="hidden_size 312"):
        CrossEncoder(str(tmp_path / "w"))
    # a bare encoder is not a cross-encoder
    d = tmp_path / "bare"
    make_checkpoint(str(d), "roberta")
    c = json.load(open(d / "config.json"))
    c["architectures"] = ["RobertaModel"]
    json.dump(c, open(d / "config.json", "w"))
    with pytest.raises(NotImplementedError):
        CrossEncoder(str(d))


def test_missing_model_constructs_and_predict_raises_through_the_dropin(tmp_path, monkeypatch):
    for var in ("SENTENCE_TRANSFORMERS_HOME", "HF_HOME", "TORCH_HOME"):
        monkeypatch.setenv(var, str(tmp_path / var))
    monkeypatch.delenv("HF_HUB_CACHE", raising=False)
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]
        from sentence_transformers import CrossEncoder as CE
        from sentence_transformers.cross_encoder import CrossEncoder as CE2
        assert CE is CE2 is CrossEncoder
        ce = CE("cross-encoder/stsb-roberta-large")            # models/evaluators.py:31, at import time
        with pytest.raises(RuntimeError, match="no checkpoint"):
            ce.predict([["a query", "a caption"]])
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]


def test_arch_roberta_is_accepted_by_the_library():
    lib = _lib.load()
    for name in ("tiny-roberta", "roberta-large-2l"):
        cfg = PRESETS[name]
        c = _lib.make_config(cfg)
        assert c.arch == 2 and lib.qst_arena_elems(c) == build_layout(cfg)[1]
    c.arch = 3
    assert lib.qst_arena_elems(c) < 0
    assert lib.qst_version() >= 102


def test_pair_tokenisation(tmp_path):
    make_checkpoint(str(tmp_path / "b"), "bert")
    make_checkpoint(str(tmp_path / "r"), "roberta")
    vocab = [w.strip() for w in open(os.path.join(ROOT, "tests", "golden", "tiny_vocab.txt"))]
    ix = {w: i for i, w in enumerate(vocab)}
    fb = CrossEncoder(str(tmp_path / "b")).tokenize_pairs([("  a man rides ", "two dogs"), ("zebra", "a horse !")])
    assert fb["input_ids"][0].tolist() == [ix[w] for w in ("[CLS]", "a", "man", "rides", "[SEP]", "two", "dogs", "[SEP]")]
    assert fb["token_type_ids"][0].tolist() == [0] * 5 + [1] * 3          # segment B is type 1
    assert fb["token_type_ids"][1].tolist()[:7] == [0, 0, 0, 1, 1, 1, 1]
    ce = CrossEncoder(str(tmp_path / "r"))
    fr = ce.tokenize_pairs([("a man", "a dog")])
    tok = ce.tokenizer
    want = [0] + tok("a man", add_special_tokens=False)["input_ids"] + [2, 2] + \
        tok("a dog", add_special_tokens=False)["input_ids"] + [2]                    # <s> A </s></s> B </s>
    assert fr["input_ids"][0].tolist() == want and "token_type_ids" not in fr
    assert tok.pad_token_id == 1


def test_roberta_bi_encoder_directory_loads_and_saves_as_roberta(tmp_path):
    import transformers as T
    from quadruplet_sentence_transformer_amd.sentence_transformer import (_MODEL_TYPES, SyntheticTokenizer,
                                                                          _load_model_dir)
    cfg = T.RobertaConfig(vocab_size=128, hidden_size=64, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128,
                          max_position_embeddings=66, type_vocab_size=1, pad_token_id=1, layer_norm_eps=1e-5)
    m = T.RobertaModel(cfg, add_pooling_layer=False)
    m.save_pretrained(str(tmp_path), safe_serialization=True)
    ec, arena, _ = _load_model_dir(str(tmp_path))
    assert (ec.arch, ec.type_vocab_size, ec.pad_token_id, ec.max_seq_length, ec.pooling) == (ARCH_ROBERTA, 1, 1, 64, "mean")
    so = {s.name: s for s in build_layout(ec)[0]}
    pos = so["pos_emb"]
    np.testing.assert_array_equal(arena[pos.offset:pos.offset + pos.numel],
                                  m.embeddings.position_embeddings.weight.detach().numpy().reshape(-1))
    assert _MODEL_TYPES[ARCH_ROBERTA] == "roberta"
    syn = SyntheticTokenizer(PRESETS["tiny-roberta"])
    assert (syn.cls_id, syn.sep_id, syn.pad_id) == (0, 2, 1)
