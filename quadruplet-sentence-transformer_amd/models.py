"""The module descriptors of sentence-transformers 2.2.2 that pick a head for a plain HF checkpoint:

    SentenceTransformer(modules=[models.Transformer("bert-base-uncased", max_seq_length=256),
                                 models.Pooling(768, pooling_mode="cls"), models.Normalize()])

Transformer, Pooling and Normalize hold settings only and compute nothing: SentenceTransformer(modules=...) reads them into
an EncoderConfig and runs the whole chain in libqst.so. `Dense` is the one module with parameters of its own: the trained
projection head after pooling (LaBSE's 2_Dense, the PCA layer of the distillation recipes), an nn.Module whose forward and
backward are csrc/dense_head.hip. The chains Transformer -> Pooling -> [Dense] -> [Normalize] are the ones accepted;
`dropin/` re-exports this module as `sentence_transformers.models`.
"""
from __future__ import annotations

import json
import os
from collections import OrderedDict
from typing import Dict, Optional

import torch
from torch import nn

from . import _lib
from .config import POOLING_MODES, pooling_modes

# ST 2.2.2 Pooling config keys (1_Pooling/config.json, in the order ST writes them) -> mode names of config.POOLING_MODES
POOLING_CONFIG_KEYS = {"pooling_mode_cls_token": "cls", "pooling_mode_mean_tokens": "mean",
                       "pooling_mode_max_tokens": "max", "pooling_mode_mean_sqrt_len_tokens": "mean_sqrt_len",
                       "pooling_mode_weightedmean_tokens": "weightedmean"}


class Transformer:
    """sentence_transformers.models.Transformer: the HF checkpoint (a local directory or a model name resolved offline)
    and its max_seq_length (None: the checkpoint's own, at most 512)."""

    def __init__(self, model_name_or_path: str, max_seq_length: Optional[int] = None, model_args: Optional[dict] = None,
                 cache_dir: Optional[str] = None, tokenizer_args: Optional[dict] = None, do_lower_case: bool = False,
                 tokenizer_name_or_path: Optional[str] = None):
        self.model_name_or_path = model_name_or_path
        self.max_seq_length = max_seq_length
        self.cache_dir = cache_dir
        self.do_lower_case = do_lower_case
        if tokenizer_name_or_path not in (None, model_name_or_path):
            raise NotImplementedError("a tokenizer from another directory than the model's is not supported")


class Pooling:
    """sentence_transformers.models.Pooling: pooling_mode ("cls", "max", "mean", "mean_sqrt_len", "weightedmean" or a
    '+' join of them) or the pooling_mode_*_tokens flags, as in ST 2.2.2 (a pooling_mode string overrides the flags).
    `pooling` is the mode string of config.EncoderConfig, in the fixed block order."""

    def __init__(self, word_embedding_dimension: int, pooling_mode: Optional[str] = None,
                 pooling_mode_cls_token: bool = False, pooling_mode_max_tokens: bool = False,
                 pooling_mode_mean_tokens: bool = True, pooling_mode_mean_sqrt_len_tokens: bool = False,
                 pooling_mode_weightedmean_tokens: bool = False, pooling_mode_lasttoken: bool = False):
        self.word_embedding_dimension = int(word_embedding_dimension)
        if pooling_mode is not None:
            if str(pooling_mode).lower() == "lasttoken":
                raise NotImplementedError("pooling_mode='lasttoken' is not implemented (cls, max, mean, mean_sqrt_len, "
                                          "weightedmean)")
            modes = pooling_modes(str(pooling_mode).lower())
        else:
            if pooling_mode_lasttoken:
                raise NotImplementedError("pooling_mode_lasttoken is not implemented (cls, max, mean, mean_sqrt_len, "
                                          "weightedmean)")
            flags = {"cls": pooling_mode_cls_token, "max": pooling_mode_max_tokens, "mean": pooling_mode_mean_tokens,
                     "mean_sqrt_len": pooling_mode_mean_sqrt_len_tokens, "weightedmean": pooling_mode_weightedmean_tokens}
            modes = tuple(m for m in POOLING_MODES if flags[m])
            if not modes:
                raise ValueError("Pooling: no pooling mode enabled")
        self.pooling = "+".join(modes)

    def get_pooling_mode_str(self) -> str:
        return self.pooling

    def get_sentence_embedding_dimension(self) -> int:
        return len(pooling_modes(self.pooling)) * self.word_embedding_dimension

    def get_config_dict(self) -> dict:
        """1_Pooling/config.json as ST 2.2.2 writes it."""
        on = set(pooling_modes(self.pooling))
        out = {"word_embedding_dimension": self.word_embedding_dimension}
        out.update({k: m in on for k, m in POOLING_CONFIG_KEYS.items()})
        out["pooling_mode_lasttoken"] = False
        return out


class Normalize:
    """sentence_transformers.models.Normalize: L2-normalise the pooled vector (over all of its D columns)."""


def pooling_from_config(pool: dict, hidden_size: int, where: str = "") -> str:
    """The pooling string of a 1_Pooling/config.json. An enabled mode other than the five of POOLING_MODES (lasttoken, or
    any key a later sentence-transformers writes), no enabled mode, or a word_embedding_dimension other than hidden_size
    is refused: the checkpoint would be pooled wrongly."""
    pre = f"{where}: " if where else ""
    bad = sorted(k for k, v in pool.items() if k.startswith("pooling_mode") and v and k not in POOLING_CONFIG_KEYS)
    if bad:
        raise NotImplementedError(f"{pre}pooling {bad} is not implemented (cls, max, mean, mean_sqrt_len, weightedmean); "
                                  "this checkpoint would be pooled wrongly")
    on = set(m for k, m in POOLING_CONFIG_KEYS.items() if pool.get(k))
    if not on:
        raise NotImplementedError(f"{pre}no pooling mode enabled in {sorted(pool)}")
    dim = pool.get("word_embedding_dimension", hidden_size)
    if int(dim) != int(hidden_size):
        raise NotImplementedError(f"{pre}Pooling word_embedding_dimension {dim} differs from the encoder's hidden_size "
                                  f"{hidden_size}")
    return "+".join(m for m in POOLING_MODES if m in on)


# ------------------------------------------------------------------------------------------------ models.Dense
DENSE_ACT_IDENTITY, DENSE_ACT_TANH = 0, 1          # include/qst.h: QST_DENSE_ACT_*
# activation class -> (code, the name sentence-transformers' `fullname` writes into 2_Dense/config.json)
_DENSE_ACTS = {nn.Identity: (DENSE_ACT_IDENTITY, "torch.nn.modules.linear.Identity"),
               nn.Tanh: (DENSE_ACT_TANH, "torch.nn.modules.activation.Tanh")}


def dense_activation(name_or_module):
    """(code, class, config name) of a Dense activation given as a module or as the config's fully qualified class name.
    Anything but nn.Tanh and nn.Identity is refused."""
    for cls, (code, full) in _DENSE_ACTS.items():
        if name_or_module == full or type(name_or_module) is cls:
            return code, cls, full
    what = name_or_module if isinstance(name_or_module, str) else type(name_or_module).__name__
    raise NotImplementedError(f"models.Dense: activation_function {what} is not implemented; the head kernels compute "
                              "torch.nn.Tanh and torch.nn.Identity")


def dense_head_fwd_raw(x, w, b, act: int, normalize: bool):
    """qst_dense_head_fwd on contiguous fp32 HIP tensors x [B, Din], w [Dout, Din] and b [Dout] or
    None: (y [B, Dout], row_norm [B] or None without normalize)."""
    lib = _lib.load()
    (B, Din), Dout = x.shape, w.shape[0]
    y = torch.empty(B, Dout, dtype=torch.float32, device=x.device)
    norm = torch.empty(B, dtype=torch.float32, device=x.device) if normalize else None
    with torch.cuda.device(x.device):
        _lib.check(lib.qst_dense_head_fwd(x.data_ptr(), Din, w.data_ptr(), _lib.ptr(b), B, Din, Dout, int(act),
                                          int(bool(normalize)), y.data_ptr(), _lib.ptr(norm), _lib.current_stream_ptr()),
                   "qst_dense_head_fwd")
    return y, norm


def dense_head_bwd_raw(x, w, y, norm, dy, act: int, normalize: bool, bias: bool = True):
    """qst_dense_head_bwd: (grad_x [B, Din], grad_w [Dout, Din], grad_b [Dout] or None without `bias`) from dy [B, Dout]."""
    lib = _lib.load()
    (B, Din), Dout = x.shape, w.shape[0]
    gx = torch.empty(B, Din, dtype=torch.float32, device=x.device)
    gw = torch.empty_like(w)
    gb = torch.empty(Dout, dtype=torch.float32, device=x.device) if bias else None
    nbytes = int(lib.qst_dense_head_bwd_workspace_bytes(B, Din, Dout))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.qst_dense_head_bwd(x.data_ptr(), Din, w.data_ptr(), y.data_ptr(), _lib.ptr(norm), dy.data_ptr(),
                                          B, Din, Dout, int(act), int(bool(normalize)), gx.data_ptr(), gw.data_ptr(),
                                          _lib.ptr(gb), ws.data_ptr(), nbytes, _lib.current_stream_ptr()),
                   "qst_dense_head_bwd")
    return gx, gw, gb


class _DenseHeadFn(torch.autograd.Function):
    """y = [normalize](act(x W^T + b)): qst_dense_head_fwd, and qst_dense_head_bwd from autograd's dy. What the backward
    needs besides its inputs is y and one norm per row."""

    @staticmethod
    def forward(ctx, x, w, b, act, normalize):
        xs = [t.detach().to(torch.float32).contiguous() for t in (x, w)]
        bb = None if b is None else b.detach().to(torch.float32).contiguous()
        y, norm = dense_head_fwd_raw(xs[0], xs[1], bb, act, normalize)
        ctx.save_for_backward(xs[0], xs[1], y, *([norm] if normalize else []))
        ctx.hp = (act, normalize, b is not None)
        ctx.in_dtypes = (x.dtype, w.dtype, None if b is None else b.dtype)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        act, normalize, bias = ctx.hp
        x, w, y = ctx.saved_tensors[:3]
        norm = ctx.saved_tensors[3] if normalize else None
        gx, gw, gb = dense_head_bwd_raw(x, w, y, norm, grad_y.detach().to(torch.float32).contiguous(), act, normalize, bias)
        dx, dw, db = ctx.in_dtypes
        return gx.to(dx), gw.to(dw), (gb.to(db) if bias else None), None, None


def dense_head(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: int, normalize: bool = False):
    """[F.normalize](act(F.linear(x, weight, bias))) of HIP tensors through the head kernels, with autograd. There is no
    other path: tensors that are not on a HIP device are an error."""
    if not (x.is_cuda and weight.is_cuda and (bias is None or bias.is_cuda)):
        raise _lib.QstError("models.Dense runs on the HIP device only (csrc/dense_head.hip): move the input and the module "
                            "there; this build has no CPU path")
    if x.dim() != 2 or x.shape[1] != weight.shape[1]:
        raise ValueError(f"models.Dense: input {tuple(x.shape)} does not match in_features {weight.shape[1]}")
    return _DenseHeadFn.apply(x, weight, bias, int(act), bool(normalize))


class Dense(nn.Module):
    """sentence_transformers.models.Dense (2.2.2): activation_function(nn.Linear(in_features, out_features, bias)) on the
    sentence embedding. activation_function: nn.Tanh() (the default) or nn.Identity(). init_weight / init_bias overwrite
    the Linear's initial values (the PCA components of the dimensionality-reduction recipe)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True, activation_function=nn.Tanh(),
                 init_weight: Optional[torch.Tensor] = None, init_bias: Optional[torch.Tensor] = None):
        super().__init__()
        self._act_code, _, self._act_name = dense_activation(activation_function)
        self.in_features = int(in_features)
        self.out_features = int(out_features)
        self.bias = bool(bias)
        self.activation_function = activation_function
        self.linear = nn.Linear(self.in_features, self.out_features, bias=self.bias)
        for name, init in (("weight", init_weight), ("bias", init_bias)):
            if init is None:
                continue
            par = getattr(self.linear, name)
            if par is None:
                raise ValueError("models.Dense: init_bias given with bias=False")
            init = torch.as_tensor(init).detach().to(torch.float32)
            if tuple(init.shape) != tuple(par.shape):
                raise ValueError(f"models.Dense: init_{name} has shape {tuple(init.shape)}, the Linear's is {tuple(par.shape)}")
            setattr(self.linear, name, nn.Parameter(init.clone()))

    def forward(self, features: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        features.update({"sentence_embedding": self.project(features["sentence_embedding"])})
        return features

    def project(self, x: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        """The head on an embedding matrix [B, in_features]; normalize: the models.Normalize that follows it, fused."""
        return dense_head(x, self.linear.weight, self.linear.bias, self._act_code, normalize)

    def get_sentence_embedding_dimension(self) -> int:
        return self.out_features

    def get_config_dict(self) -> dict:
        """2_Dense/config.json as ST 2.2.2 writes it."""
        return {"in_features": self.in_features, "out_features": self.out_features, "bias": self.bias,
                "activation_function": self._act_name}

    def save(self, output_path: str) -> None:
        """config.json and pytorch_model.bin (the state dict: linear.weight, linear.bias), the files 2.2.2 loads."""
        os.makedirs(output_path, exist_ok=True)
        with open(os.path.join(output_path, "config.json"), "w") as f:
            json.dump(self.get_config_dict(), f)
        # tensors of their own: the parameters may be views of a flat buffer, and torch.save would write the whole buffer
        # behind each of them
        sd = OrderedDict((k, v.detach().cpu().contiguous().clone()) for k, v in self.state_dict().items())
        torch.save(sd, os.path.join(output_path, "pytorch_model.bin"))

    def __repr__(self):
        return "Dense({})".format(self.get_config_dict())

    @staticmethod
    def load(input_path: str) -> "Dense":
        with open(os.path.join(input_path, "config.json")) as f:
            config = json.load(f)
        _, act_cls, _ = dense_activation(config["activation_function"])
        model = Dense(int(config["in_features"]), int(config["out_features"]), bool(config.get("bias", True)), act_cls())
        bin_path, st_path = os.path.join(input_path, "pytorch_model.bin"), os.path.join(input_path, "model.safetensors")
        if os.path.exists(bin_path):
            sd = torch.load(bin_path, map_location="cpu", weights_only=True)
        elif os.path.exists(st_path):
            from safetensors.torch import load_file
            sd = load_file(st_path)
        else:
            raise FileNotFoundError(f"{input_path} has neither pytorch_model.bin nor model.safetensors")
        model.load_state_dict({k: v.to(torch.float32) for k, v in sd.items()})
        return model

