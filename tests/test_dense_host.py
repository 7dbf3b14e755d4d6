"""CPU: models.Dense on the host side -- the module itself (constructor, config, save / load), model directories and module
lists with a Dense in them, the drop-in namespace, the C-ABI symbols and the argument checks that return before any launch."""
import ctypes
import json
import os
import sys

import pytest
import torch
from torch import nn

import quadruplet_sentence_transformer_amd  # noqa: F401
import dense_head_helpers as H
from quadruplet_sentence_transformer_amd import _lib, models
from quadruplet_sentence_transformer_amd.sentence_transformer import (SentenceTransformer, _load_dense_head, _load_model_dir,
                                                                      _load_model_dir_sd, _load_module_chain,
                                                                      _module_chain_dense)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TANH_NAME, IDENTITY_NAME = "torch.nn.modules.activation.Tanh", "torch.nn.modules.linear.Identity"


# ------------------------------------------------------------------ 1. the module
def test_constructor_is_the_one_of_sentence_transformers():
    torch.manual_seed(0)
    d = models.Dense(64, 24)
    assert isinstance(d, nn.Module) and isinstance(d.linear, nn.Linear) and isinstance(d.activation_function, nn.Tanh)
    assert d.linear.weight.shape == (24, 64) and d.linear.bias.shape == (24,)
    assert [n for n, _ in d.named_parameters()] == ["linear.weight", "linear.bias"]
    assert d.get_sentence_embedding_dimension() == 24
    assert d.get_config_dict() == {"in_features": 64, "out_features": 24, "bias": True, "activation_function": TANH_NAME}
    torch.manual_seed(0)
    assert torch.equal(nn.Linear(64, 24).weight, d.linear.weight)      # the same seed gives upstream's initial weights
    w, b = torch.randn(3, 5), torch.randn(3)
    p = models.Dense(5, 3, bias=True, activation_function=nn.Identity(), init_weight=w, init_bias=b)
    assert torch.equal(p.linear.weight, w) and torch.equal(p.linear.bias, b) and p.linear.weight.requires_grad
    assert p.get_config_dict() == {"in_features": 5, "out_features": 3, "bias": True, "activation_function": IDENTITY_NAME}
    q = models.Dense(5, 3, bias=False, activation_function=nn.Identity(), init_weight=w)
    assert q.linear.bias is None and [n for n, _ in q.named_parameters()] == ["linear.weight"]
    assert q.get_config_dict()["bias"] is False
    with pytest.raises(ValueError, match="init_weight"):
        models.Dense(5, 3, init_weight=torch.zeros(5, 3))


@pytest.mark.parametrize("act", [nn.ReLU(), nn.GELU(), nn.Sigmoid()])
def test_another_activation_is_refused_naming_the_two(act):
    with pytest.raises(NotImplementedError, match=f"{type(act).__name__}.*Tanh.*Identity"):
        models.Dense(8, 4, activation_function=act)


@pytest.mark.parametrize("bias,act", [(True, nn.Tanh()), (False, nn.Identity())])
def test_save_writes_what_sentence_transformers_loads_and_load_reads_it_back(tmp_path, bias, act):
    torch.manual_seed(1)
    d = models.Dense(20, 7, bias=bias, activation_function=act)
    d.save(str(tmp_path / "2_Dense"))
    assert sorted(os.listdir(tmp_path / "2_Dense")) == ["config.json", "pytorch_model.bin"]
    cfg = json.load(open(tmp_path / "2_Dense" / "config.json"))
    assert cfg == d.get_config_dict() and list(cfg) == ["in_features", "out_features", "bias", "activation_function"]
    sd = torch.load(tmp_path / "2_Dense" / "pytorch_model.bin", map_location="cpu", weights_only=True)
    assert sorted(sd) == (["linear.bias", "linear.weight"] if bias else ["linear.weight"])
    assert sd["linear.weight"].shape == (7, 20) and torch.equal(sd["linear.weight"], d.linear.weight)
    # upstream's own load: Dense(**config) with the imported activation, then load_state_dict
    up = nn.Linear(cfg["in_features"], cfg["out_features"], bias=cfg["bias"])
    up.load_state_dict({k[len("linear."):]: v for k, v in sd.items()})
    back = models.Dense.load(str(tmp_path / "2_Dense"))
    assert back.get_config_dict() == d.get_config_dict() and type(back.activation_function) is type(act)
    assert torch.equal(back.linear.weight, d.linear.weight)
    assert (back.linear.bias is None) == (not bias) and (not bias or torch.equal(back.linear.bias, d.linear.bias))


def test_load_reads_a_safetensors_directory_too(tmp_path):
    w, b = H.write_model_dir(str(tmp_path), dense_file="model.safetensors")
    d = models.Dense.load(str(tmp_path / "2_Dense"))
    assert torch.equal(d.linear.weight, w) and torch.equal(d.linear.bias, b)
    os.remove(tmp_path / "2_Dense" / "model.safetensors")
    with pytest.raises(FileNotFoundError, match="pytorch_model.bin"):
        models.Dense.load(str(tmp_path / "2_Dense"))


def test_forward_has_no_cpu_path():
    d = models.Dense(8, 4)
    with pytest.raises(_lib.QstError, match="HIP device"):
        d({"sentence_embedding": torch.zeros(2, 8)})


# ------------------------------------------------------------------ 2. model directories and module lists
@pytest.mark.parametrize("normalize", [True, False])
def test_a_directory_with_a_dense_loads_and_reports_its_settings(tmp_path, normalize):
    kinds = ("Transformer", "Pooling", "Dense") + (("Normalize",) if normalize else ())
    w, b = H.write_model_dir(str(tmp_path), kinds=kinds)
    out = _load_model_dir(str(tmp_path))
    assert len(out) == 3 and len(_load_model_dir_sd(str(tmp_path))) == 4
    cfg, arena, _ = out
    assert cfg.pooling == "mean" and cfg.embedding_dim == 64 and arena.size > 0
    assert cfg.normalize is False                        # the encoder never normalises in front of a Dense
    dense, after = _load_dense_head(str(tmp_path), cfg)
    assert after is normalize
    assert dense.get_config_dict() == {"in_features": 64, "out_features": 24, "bias": True, "activation_function": TANH_NAME}
    assert torch.equal(dense.linear.weight, w) and torch.equal(dense.linear.bias, b)


def test_a_directory_without_a_dense_loads_as_it_always_did(tmp_path):
    H.write_model_dir(str(tmp_path), kinds=("Transformer", "Pooling", "Normalize"))
    out = _load_model_dir(str(tmp_path))
    assert len(out) == 3 and out[0].normalize is True
    assert _load_dense_head(str(tmp_path), out[0]) == (None, False)
    os.remove(tmp_path / "modules.json")                 # a plain HF directory
    assert _load_dense_head(str(tmp_path), _load_model_dir(str(tmp_path))[0]) == (None, False)


@pytest.mark.parametrize("kinds,msg", [
    (("Transformer", "Pooling", "Dense", "Dense"), "2 Dense modules"),
    (("Transformer", "Pooling", "Dense", "Dense", "Normalize"), "2 Dense modules"),
    (("Transformer", "Dense", "Pooling"), "Dense before Pooling"),
    (("Transformer", "Pooling", "Normalize", "Dense"), "Dense after Normalize"),
])
def test_a_misplaced_dense_is_refused_with_a_message(tmp_path, kinds, msg):
    H.write_model_dir(str(tmp_path), kinds=kinds)
    with pytest.raises(NotImplementedError, match=msg):
        _load_model_dir(str(tmp_path))
    with pytest.raises(NotImplementedError, match=msg):
        _load_dense_head(str(tmp_path), None)
    with pytest.raises(NotImplementedError, match=msg):
        SentenceTransformer(str(tmp_path), device="cpu")


def test_a_dense_of_another_width_or_activation_is_refused_with_a_message(tmp_path):
    H.write_model_dir(str(tmp_path / "narrow"), Din=32)
    cfg, _, _ = _load_model_dir(str(tmp_path / "narrow"))
    with pytest.raises(NotImplementedError, match="in_features 32 differs from the pooled width 64"):
        _load_dense_head(str(tmp_path / "narrow"), cfg)
    H.write_model_dir(str(tmp_path / "relu"), activation_name="torch.nn.modules.activation.ReLU")
    with pytest.raises(NotImplementedError, match="torch.nn.modules.activation.ReLU.*Tanh.*Identity"):
        _load_dense_head(str(tmp_path / "relu"), cfg)
    for d in ("narrow", "relu"):
        with pytest.raises(NotImplementedError):
            SentenceTransformer(str(tmp_path / d), device="cpu")


def test_an_unknown_module_is_still_refused(tmp_path):
    H.write_model_dir(str(tmp_path), kinds=("Transformer", "Pooling", "LayerNorm"))
    with pytest.raises(NotImplementedError, match="LayerNorm.*not on the accelerated path"):
        _load_model_dir(str(tmp_path))


def test_module_lists_with_a_dense(tmp_path):
    H.write_model_dir(str(tmp_path), kinds=())
    os.remove(tmp_path / "modules.json")
    tr, pool = models.Transformer(str(tmp_path), max_seq_length=48), models.Pooling(64)
    dense = models.Dense(64, 24)
    for mods, after in (([tr, pool, dense], False), ([tr, pool, dense, models.Normalize()], True)):
        out = _load_module_chain(mods)
        assert len(out) == 4
        cfg = out[0]
        assert (cfg.pooling, cfg.normalize, cfg.max_seq_length, cfg.embedding_dim) == ("mean", False, 48, 64)
        assert _module_chain_dense(mods, cfg) == (dense, after)
    cfg = _load_module_chain([tr, pool, models.Normalize()])[0]
    assert cfg.normalize is True and _module_chain_dense([tr, pool, models.Normalize()], cfg) == (None, False)
    for bad, msg in (([tr, pool, dense, models.Dense(24, 8)], "2 Dense modules"),
                     ([tr, dense, pool], "Dense before Pooling"),
                     ([tr, pool, models.Normalize(), dense], "Dense after Normalize"),
                     ([tr, pool, models.Dense(32, 8)], "in_features 32 differs from the pooled width 64"),
                     ([tr, models.Pooling(64, pooling_mode="cls+mean"), dense],
                      "in_features 64 differs from the pooled width 128")):
        with pytest.raises(NotImplementedError, match=msg):
            SentenceTransformer(modules=bad, device="cpu")


def test_dropin_exposes_dense_as_sentence_transformers_models_dense():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        for m in [k for k in sys.modules if k.startswith("sentence_transformers")]:
            del sys.modules[m]
        from sentence_transformers import models as stm
        assert stm.Dense is models.Dense
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))


# ------------------------------------------------------------------ 3. the library
def test_entry_points_are_exported_declared_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "qst.h")).read()
    for name in ("qst_dense_head_fwd", "qst_dense_head_bwd_workspace_bytes", "qst_dense_head_bwd"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f" {name}(" in header
    assert "QST_DENSE_ACT_IDENTITY = 0" in header and "QST_DENSE_ACT_TANH = 1" in header
    assert (models.DENSE_ACT_IDENTITY, models.DENSE_ACT_TANH) == (H.IDENTITY, H.TANH) == (0, 1)
    assert lib.qst_version() >= 110


def test_argument_checks_come_before_any_launch():
    """No device is needed: every refusal returns before the first HIP call (the pointers are host memory nobody reads)."""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    P = ctypes.addressof(buf)
    B, Din, Dout = 4, 20, 3

    def fwd(x=P, ldx=Din, w=P, b=P, B=B, Din=Din, Dout=Dout, act=H.TANH, normalize=1, y=P, norm=P):
        return lib.qst_dense_head_fwd(x, ldx, w, b, B, Din, Dout, act, normalize, y, norm, None)

    def bwd(x=P, ldx=Din, w=P, y=P, norm=P, dy=P, B=B, Din=Din, Dout=Dout, act=H.TANH, normalize=1, gx=P, gw=P, gb=P, wsp=P,
            nbytes=0):
        return lib.qst_dense_head_bwd(x, ldx, w, y, norm, dy, B, Din, Dout, act, normalize, gx, gw, gb, wsp, nbytes, None)

    for f in (fwd, bwd):
        assert f(Din=0) == H.UNSUPPORTED and f(Din=H.MAX_DIM + 1, ldx=H.MAX_DIM + 1) == H.UNSUPPORTED
        assert f(Dout=0) == H.UNSUPPORTED and f(Dout=H.MAX_DIM + 1) == H.UNSUPPORTED and f(B=0) == H.UNSUPPORTED
        assert f(x=None) == H.BAD_ARG and f(w=None) == H.BAD_ARG and f(y=None) == H.BAD_ARG
        assert f(ldx=Din - 1) == H.BAD_ARG and f(act=2) == H.BAD_ARG and f(normalize=2) == H.BAD_ARG
        assert f(norm=None) == H.BAD_ARG
    assert bwd(dy=None) == H.BAD_ARG and bwd(gx=None) == H.BAD_ARG and bwd(gw=None) == H.BAD_ARG and bwd(wsp=None) == H.BAD_ARG
    need = lib.qst_dense_head_bwd_workspace_bytes(B, Din, Dout)
    assert need == B * 4 * 4 and bwd(nbytes=need - 1) == H.BAD_ARG          # a workspace that is too small
    assert lib.qst_dense_head_bwd_workspace_bytes(257, Din, Dout) == (257 * 4 + 5 * Dout * Din + 5 * 4) * 4
    assert lib.qst_dense_head_bwd_workspace_bytes(0, Din, Dout) == 0
    assert lib.qst_dense_head_bwd_workspace_bytes(B, H.MAX_DIM + 1, Dout) == 0
    assert lib.qst_dense_head_bwd_workspace_bytes(1, H.MAX_DIM, H.MAX_DIM) == (H.MAX_DIM * 4)   # one slice: dz alone
