"""The yardstick of models.Dense's kernels (tests/test_gpu_dense_head.py, tests/test_gpu_dense_model.py,
tests/test_dense_host.py): sentence-transformers 2.2.2's models.Dense.forward followed by models.Normalize, written as
F.linear -> torch.tanh / identity -> F.normalize(p=2, dim=1, eps=1e-12) in fp64 on the CPU with autograd, on the fp32 inputs;
the recipe the test inputs are drawn by, the case list, and the calls through the C ABI. Imported like softmax_head_helpers,
not a conftest.

Error measures (the project's own): a value within rtol = atol = max(1e-5, 1.5e-8 * Din) (softmax_head_helpers.value_error
with K = Din), a gradient within rtol 1e-4 and atol 1e-6 * max(1, max |reference gradient|) (mnrl_helpers.grad_error). Both
are reported as a share of the tolerance and must be <= 1.

Conditions on the data, asserted by the tests (conditions_of): max |z| < 4 where the activation is tanh (not saturated), the
row norms of a above 1e-3 (no row on F.normalize's clamp), and every reference gradient with max |.| > 1e-4. The one
exception is mathematical: with Dout = 1 and normalisation y = sign(a), whose derivative is zero everywhere, so all three
gradients ARE zero; there the kernels are held to the absolute tolerance around zero and the condition is not asked.
"""
import functools

import torch
import torch.nn.functional as F

from mnrl_helpers import grad_error  # noqa: F401  (the gradients' measure, shared)
from softmax_head_helpers import value_error  # noqa: F401  (the values' measure, shared)

IDENTITY, TANH = 0, 1                       # include/qst.h QST_DENSE_ACT_*
BAD_ARG, UNSUPPORTED = -1, -2               # include/qst.h QST_ERR_*
MAX_DIM = 8192
EPS = 1e-12

# B: one row; a partial row tile; exactly one tile; one past it; several weight-gradient slices with an uneven last one.
# Din: below one K panel; no multiple of 16; aligned; ragged and wide; the MiniLM width.
# Dout: edge column tiles (1, 3), one tile, one past it, the row norm across more than one column tile.
BS, DINS, DOUTS = [1, 5, 64, 65, 257], [4, 20, 64, 260, 384], [1, 3, 64, 65, 200]


def _cases():
    """(B, Din, Dout, act, normalize, bias): not the full product. For each of the eight (act, normalize, bias) settings five
    cases that walk all of BS, DINS and DOUTS, each setting pairing the three lists at another shift -- so every listed size
    meets every setting -- and the two named cases."""
    out = []
    settings = [(act, nrm, bias) for act in (TANH, IDENTITY) for nrm in (1, 0) for bias in (1, 0)]
    for s, (act, nrm, bias) in enumerate(settings):
        for i in range(5):
            out.append((BS[i], DINS[(i + s) % 5], DOUTS[(i + 2 * s + s // 5) % 5], act, nrm, bias))
    for named in ((257, 384, 200, TANH, 1, 1), (65, 260, 65, IDENTITY, 0, 0)):
        if named not in out:
            out.append(named)
    return out


CASES = _cases()


def head_ref(x, w, b, act, normalize):
    """(z, a, y) in the dtype and on the device of the inputs."""
    z = F.linear(x, w, b)
    a = torch.tanh(z) if act == TANH else z
    y = F.normalize(a, p=2, dim=1, eps=EPS) if normalize else a
    return z, a, y


def case(B, Din, Dout, bias, seed):
    """fp32 inputs: x with entries of order 1, W scaled by 1 / sqrt(Din) (times 0.6, the bias 0.3: z has a standard deviation
    of 0.7, so that the largest of 50,000 of them stays below 4 and tanh is not saturated), dy of order 1."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Din, generator=g)
    w = torch.randn(Dout, Din, generator=g) * (0.6 / Din ** 0.5)
    b = torch.randn(Dout, generator=g) * 0.3 if bias else None
    dy = torch.randn(B, Dout, generator=g)
    return x, w, b, dy


def reference_of(x, w, b, dy, act, normalize):
    """fp64 CPU autograd on the fp32 inputs: (z, a, y, grad_x, grad_w, grad_b or None)."""
    xs = [t.double().clone().requires_grad_(True) for t in (x, w)]
    bb = None if b is None else b.double().clone().requires_grad_(True)
    z, a, y = head_ref(xs[0], xs[1], bb, act, normalize)
    (y * dy.double()).sum().backward()
    return z.detach(), a.detach(), y.detach(), xs[0].grad, xs[1].grad, (None if bb is None else bb.grad)


@functools.lru_cache(maxsize=None)
def reference(B, Din, Dout, act, normalize, bias):
    """The inputs of a case and their reference, computed once and shared (nobody writes to them)."""
    inputs = case(B, Din, Dout, bias, 9000 + 131 * B + 17 * Din + 3 * Dout + 8 * act + 4 * normalize + 2 * bias)
    return inputs + reference_of(*inputs, act, normalize)


def conditions_of(z, a, grads, act, normalize, Dout):
    """The conditions on a case's data (module docstring) as a list of the ones that do NOT hold."""
    bad = []
    if act == TANH and not z.abs().max().item() < 4.0:
        bad.append(f"max |z| = {z.abs().max().item():.3f} >= 4")
    if normalize and not a.norm(dim=1).min().item() > 1e-3:
        bad.append(f"smallest row norm {a.norm(dim=1).min().item():.3e} <= 1e-3")
    if not (normalize and Dout == 1):
        for name, g in zip(("grad_x", "grad_w", "grad_b"), grads):
            if g is not None and not g.abs().max().item() > 1e-4:
                bad.append(f"max |{name}| = {g.abs().max().item():.3e} <= 1e-4")
    return bad


# ------------------------------------------------------------------ the calls through the C ABI (device tensors)
def _ptr(t):
    return None if t is None else t.data_ptr()


def run_fwd(lib, x, w, b, act, normalize, st, y=None, norm=None):
    """qst_dense_head_fwd on device tensors; x may be a column block of a wider buffer (row stride x.stride(0))."""
    (B, Din), Dout = x.shape, w.shape[0]
    assert x.stride(1) == 1 and w.is_contiguous()
    y = torch.empty(B, Dout, device=x.device) if y is None else y
    norm = (torch.empty(B, device=x.device) if normalize else None) if norm is None else norm
    rc = lib.qst_dense_head_fwd(_ptr(x), x.stride(0), _ptr(w), _ptr(b), B, Din, Dout, act, normalize, _ptr(y), _ptr(norm), st)
    assert rc == 0, rc
    return y, norm


def run_bwd(lib, x, w, y, norm, dy, act, normalize, bias, st, outs=None):
    (B, Din), Dout = x.shape, w.shape[0]
    if outs is None:
        outs = (torch.empty(B, Din, device=x.device), torch.empty(Dout, Din, device=x.device),
                torch.empty(Dout, device=x.device) if bias else None)
    gx, gw, gb = outs
    nbytes = lib.qst_dense_head_bwd_workspace_bytes(B, Din, Dout)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    rc = lib.qst_dense_head_bwd(_ptr(x), x.stride(0), _ptr(w), _ptr(y), _ptr(norm), _ptr(dy), B, Din, Dout, act, normalize,
                                _ptr(gx), _ptr(gw), _ptr(gb), _ptr(ws), nbytes, st)
    assert rc == 0, rc
    return gx, gw, gb


def run_all(lib, x, w, b, dy, act, normalize, st):
    """Forward + backward: [y, row_norm or None, grad_x, grad_w, grad_b or None]."""
    y, norm = run_fwd(lib, x, w, b, act, normalize, st)
    return [y, norm, *run_bwd(lib, x, w, y, norm, dy, act, normalize, b is not None, st)]


# ------------------------------------------------------------------ model directories, written by hand
ACT_NAMES = {TANH: "torch.nn.modules.activation.Tanh", IDENTITY: "torch.nn.modules.linear.Identity"}


def dense_tensors(Din, Dout, bias=True, seed=5):
    """(weight [Dout, Din], bias [Dout] or None) of a Dense by the recipe of case()."""
    _, w, b, _ = case(1, Din, Dout, bias, seed)
    return w, b


def write_model_dir(path, kinds=("Transformer", "Pooling", "Dense", "Normalize"), Dout=24, act=TANH, bias=True, Din=64,
                    activation_name=None, dense_file="pytorch_model.bin", seed=3):
    """A tiny-bert checkpoint directory (hidden 64, mean pooling, no vocabulary: the synthetic tokenizer) as
    sentence-transformers 2.2.2 writes one, with the module chain `kinds` in modules.json (paths '<idx>_<kind>', '' for the
    Transformer) and every Dense directory written here by hand: config.json with 2.2.2's four keys and the state dict
    {linear.weight, linear.bias} in `dense_file`. Returns the Dense's (weight, bias)."""
    import json
    import os

    import numpy as np
    from safetensors.torch import save_file

    from quadruplet_sentence_transformer_amd.config import PRESETS, build_layout, hf_param_views
    from quadruplet_sentence_transformer_amd.synthetic import synthetic_params
    cfg = PRESETS["tiny-bert"]
    os.makedirs(path, exist_ok=True)
    arena = synthetic_params(cfg, seed=seed)
    so = {s.name: s for s in build_layout(cfg)[0]}
    sd = {}
    for name, seg, off, shape in hf_param_views(cfg):
        n = int(np.prod(shape))
        sd[name] = torch.from_numpy(np.ascontiguousarray(arena[so[seg].offset + off: so[seg].offset + off + n])).view(*shape)
    save_file(sd, os.path.join(path, "model.safetensors"))
    hf = {"model_type": "bert", "vocab_size": cfg.vocab_size, "hidden_size": cfg.hidden_size,
          "num_hidden_layers": cfg.num_layers, "num_attention_heads": cfg.num_heads,
          "intermediate_size": cfg.intermediate_size, "max_position_embeddings": cfg.max_position,
          "type_vocab_size": cfg.type_vocab_size, "layer_norm_eps": cfg.layer_norm_eps, "pad_token_id": 0,
          "hidden_dropout_prob": 0.1, "attention_probs_dropout_prob": 0.1}
    json.dump(hf, open(os.path.join(path, "config.json"), "w"))
    mods = []
    w, b = dense_tensors(Din, Dout, bias)
    for idx, kind in enumerate(kinds):
        sub = "" if kind == "Transformer" else f"{idx}_{kind}"
        mods.append({"idx": idx, "name": str(idx), "path": sub, "type": f"sentence_transformers.models.{kind}"})
        if sub:
            os.makedirs(os.path.join(path, sub), exist_ok=True)
        if kind == "Pooling":
            json.dump({"word_embedding_dimension": cfg.hidden_size, "pooling_mode_cls_token": False,
                       "pooling_mode_mean_tokens": True, "pooling_mode_max_tokens": False,
                       "pooling_mode_mean_sqrt_len_tokens": False}, open(os.path.join(path, sub, "config.json"), "w"))
        if kind == "Dense":
            json.dump({"in_features": Din, "out_features": Dout, "bias": bool(bias),
                       "activation_function": activation_name or ACT_NAMES[act]},
                      open(os.path.join(path, sub, "config.json"), "w"))
            state = {"linear.weight": w.clone()}
            if bias:
                state["linear.bias"] = b.clone()
            if dense_file.endswith(".safetensors"):
                save_file(state, os.path.join(path, sub, dense_file))
            else:
                torch.save(state, os.path.join(path, sub, dense_file))
    json.dump(mods, open(os.path.join(path, "modules.json"), "w"))
    return w, b
