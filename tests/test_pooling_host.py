"""CPU: the pooling heads of sentence-transformers 2.2.2 (cls, max, mean, mean_sqrt_len, weightedmean and their
concatenations) on the host side -- model directories, the models.* descriptors, EncoderConfig, the C-ABI symbols."""
import json
import os
import re
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch

import quadruplet_sentence_transformer_amd  # noqa: F401
from quadruplet_sentence_transformer_amd import _lib, models
from quadruplet_sentence_transformer_amd.config import POOLING_MODES, PRESETS, EncoderConfig, hf_param_views, pooling_mask
from quadruplet_sentence_transformer_amd.sentence_transformer import _load_model_dir, _load_module_chain
from quadruplet_sentence_transformer_amd.synthetic import synthetic_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ST_KEYS = {"cls": "pooling_mode_cls_token", "max": "pooling_mode_max_tokens", "mean": "pooling_mode_mean_tokens",
           "mean_sqrt_len": "pooling_mode_mean_sqrt_len_tokens", "weightedmean": "pooling_mode_weightedmean_tokens"}


def write_tiny_bert(path, pool=None, normalize=True, st_files=True):
    """A tiny-bert checkpoint directory as sentence-transformers writes one: config.json, model.safetensors and, with
    st_files, modules.json + 1_Pooling/config.json (`pool`: the dict to write there) [+ 2_Normalize]."""
    from safetensors.torch import save_file
    cfg = PRESETS["tiny-bert"]
    os.makedirs(path, exist_ok=True)
    arena = synthetic_params(cfg, seed=3)
    from quadruplet_sentence_transformer_amd.config import build_layout
    so = {s.name: s for s in build_layout(cfg)[0]}
    sd = {}
    for name, seg, off, shape in hf_param_views(cfg):
        n = int(np.prod(shape))
        sd[name] = torch.from_numpy(np.ascontiguousarray(arena[so[seg].offset + off: so[seg].offset + off + n])).view(*shape)
    save_file(sd, os.path.join(path, "model.safetensors"))
    hf = {"model_type": "bert", "vocab_size": cfg.vocab_size, "hidden_size": cfg.hidden_size,
          "num_hidden_layers": cfg.num_layers, "num_attention_heads": cfg.num_heads,
          "intermediate_size": cfg.intermediate_size, "max_position_embeddings": cfg.max_position,
          "type_vocab_size": cfg.type_vocab_size, "layer_norm_eps": cfg.layer_norm_eps, "pad_token_id": 0}
    json.dump(hf, open(os.path.join(path, "config.json"), "w"))
    if st_files:
        mods = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
                {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}]
        if normalize:
            mods.append({"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"})
        json.dump(mods, open(os.path.join(path, "modules.json"), "w"))
        os.makedirs(os.path.join(path, "1_Pooling"), exist_ok=True)
        json.dump(pool, open(os.path.join(path, "1_Pooling", "config.json"), "w"))
    return cfg


def st_pool_config(modes, dim=64, **extra):
    """1_Pooling/config.json as sentence-transformers 2.2.2 writes it for the given modes."""
    out = {"word_embedding_dimension": dim}
    out.update({k: m in modes for m, k in ST_KEYS.items()})
    out["pooling_mode_lasttoken"] = False
    out.update(extra)
    return out


@pytest.mark.parametrize("modes", [("cls",), ("max",), ("mean",), ("mean_sqrt_len",), ("weightedmean",), ("cls", "mean")])
def test_model_directory_with_each_pooling_head_loads(tmp_path, modes):
    write_tiny_bert(str(tmp_path), st_pool_config(modes))
    cfg, arena, _ = _load_model_dir(str(tmp_path))
    assert cfg.pooling == "+".join(modes) and cfg.normalize
    assert cfg.embedding_dim == len(modes) * 64
    assert arena.size > 0


def test_pooling_keys_order_does_not_matter_and_blocks_come_in_the_fixed_order(tmp_path):
    write_tiny_bert(str(tmp_path), st_pool_config(("weightedmean", "max", "cls")), normalize=False)
    cfg, _, _ = _load_model_dir(str(tmp_path))
    assert cfg.pooling == "cls+max+weightedmean" and cfg.embedding_dim == 192 and not cfg.normalize


@pytest.mark.parametrize("pool,msg", [
    (st_pool_config(("mean",), pooling_mode_lasttoken=True), "pooling_mode_lasttoken"),
    (st_pool_config(("cls",), pooling_mode_attention_tokens=True), "pooling_mode_attention_tokens"),
    (st_pool_config(("cls",), dim=32), "word_embedding_dimension"),
    (st_pool_config(()), "no pooling mode"),
])
def test_unsupported_pooling_configs_are_refused_with_a_message(tmp_path, pool, msg):
    write_tiny_bert(str(tmp_path), pool)
    with pytest.raises(NotImplementedError, match=msg):
        _load_model_dir(str(tmp_path))


def test_pooling_descriptor_maps_to_the_mode_strings():
    assert models.Pooling(64).pooling == "mean"                                    # ST's default: mean tokens
    assert models.Pooling(64, pooling_mode="cls").pooling == "cls"
    assert models.Pooling(64, pooling_mode="max").pooling == "max"
    assert models.Pooling(64, pooling_mode="weightedmean").pooling == "weightedmean"
    assert models.Pooling(64, pooling_mode="mean+cls").pooling == "cls+mean"
    assert models.Pooling(64, pooling_mode_cls_token=True).pooling == "cls+mean"   # flags add to ST's mean default
    assert models.Pooling(64, pooling_mode_cls_token=True, pooling_mode_mean_tokens=False).pooling == "cls"
    assert models.Pooling(64, pooling_mode_mean_sqrt_len_tokens=True, pooling_mode_max_tokens=True,
                          pooling_mode_mean_tokens=False).pooling == "max+mean_sqrt_len"
    p = models.Pooling(64, pooling_mode="cls+max")
    assert p.get_sentence_embedding_dimension() == 128
    assert models.pooling_from_config(p.get_config_dict(), 64) == "cls+max"
    assert p.get_config_dict() == st_pool_config(("cls", "max"))
    with pytest.raises(NotImplementedError, match="lasttoken"):
        models.Pooling(64, pooling_mode="lasttoken")
    with pytest.raises(NotImplementedError, match="lasttoken"):
        models.Pooling(64, pooling_mode_lasttoken=True, pooling_mode_mean_tokens=False)
    with pytest.raises(ValueError):
        models.Pooling(64, pooling_mode="sum")


def test_encoder_config_pooling_string():
    cfg = replace(PRESETS["tiny-bert"], pooling="weightedmean+cls")
    assert cfg.pooling == "cls+weightedmean" and cfg.embedding_dim == 128
    assert PRESETS["all-MiniLM-L6-v2"].pooling == "mean" and PRESETS["all-MiniLM-L6-v2"].embedding_dim == 384
    assert pooling_mask("mean") == 4 and pooling_mask("+".join(POOLING_MODES)) == 31 and pooling_mask("cls+max") == 3
    with pytest.raises(ValueError, match="lasttoken"):
        EncoderConfig(pooling="lasttoken")


def test_module_chain_picks_the_head_for_a_plain_checkpoint(tmp_path):
    write_tiny_bert(str(tmp_path), st_files=False)                   # a plain HF directory: no modules.json
    cfg, arena, _, _ = _load_module_chain([models.Transformer(str(tmp_path), max_seq_length=48),
                                           models.Pooling(64, pooling_mode="cls"), models.Normalize()])
    assert (cfg.pooling, cfg.normalize, cfg.max_seq_length, cfg.embedding_dim) == ("cls", True, 48, 64)
    cfg, _, _, _ = _load_module_chain([models.Transformer(str(tmp_path)), models.Pooling(64, pooling_mode="max+mean")])
    assert (cfg.pooling, cfg.normalize, cfg.embedding_dim) == ("max+mean", False, 128)
    with pytest.raises(NotImplementedError, match="word_embedding_dimension"):
        _load_module_chain([models.Transformer(str(tmp_path)), models.Pooling(32)])
    from quadruplet_sentence_transformer_amd.sentence_transformer import SentenceTransformer
    for bad in ([models.Transformer(str(tmp_path)), models.Normalize()],
                [models.Pooling(64), models.Transformer(str(tmp_path))],
                [models.Transformer(str(tmp_path)), models.Pooling(64), models.Normalize(), models.Normalize()]):
        with pytest.raises(NotImplementedError, match="module lists"):
            SentenceTransformer(modules=bad, device="cpu")


def test_pooling_entry_points_are_exported_and_bound():
    lib = _lib.load()
    for name in ("qst_encoder_set_pooling", "qst_encoder_embedding_dim", "qst_pool_fwd", "qst_pool_bwd"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.qst_version() >= 114
    for name in ("qst_pool_norm_fwd", "qst_pool_norm_bwd"):        # version 114: one kernel pair, one pair of entry points
        assert not hasattr(lib, name) and name not in _lib.SIGNATURES
    # argument checks come before any launch: no device needed
    assert lib.qst_encoder_set_pooling(None, 1) == -1 and lib.qst_encoder_embedding_dim(None) == -1
    assert lib.qst_pool_fwd(None, None, 1, 32, 64, 1, 1, None, None, None, None) == -1
    assert lib.qst_pool_bwd(None, None, None, None, 1, 32, 64, 2, 1, None, None) == -1


def test_header_mode_bits_follow_the_block_order():
    for h in ("qst.h", "qst_kernels.h"):
        src = open(os.path.join(ROOT, "include", h)).read()
        bits = dict((k, int(v)) for k, v in re.findall(r"#define (QST_POOL_[A-Z_]+) (\d+)", src))
        assert bits == {"QST_POOL_CLS": 1, "QST_POOL_MAX": 2, "QST_POOL_MEAN": 4, "QST_POOL_MEAN_SQRT": 8,
                        "QST_POOL_WMEAN": 16, "QST_POOL_ALL": 31}, h
    assert [pooling_mask(m) for m in POOLING_MODES] == [1, 2, 4, 8, 16]


def test_dropin_exposes_the_descriptors_as_sentence_transformers_models():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        for m in [k for k in sys.modules if k.startswith("sentence_transformers")]:
            del sys.modules[m]
        from sentence_transformers import models as stm
        assert stm.Transformer is models.Transformer and stm.Pooling is models.Pooling and stm.Normalize is models.Normalize
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
