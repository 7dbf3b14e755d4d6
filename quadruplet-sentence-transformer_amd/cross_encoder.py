"""`CrossEncoder`: sentence-transformers 2.2.2's cross-encoder surface over the HIP encoder and the classification-head kernel.

The reference builds one at import time (models/evaluators.py:31, "cross-encoder/stsb-roberta-large") and scores every
(query, corpus sentence) pair with `predict` when it builds an IR evaluation set with use_cross_encoder=True
(models/evaluators.py:501-508). Here a pair runs through HipEncoder with pooling "cls" and no normalisation (the encoder's
first-token state), then through qst_cls_head_fwd (include/qst.h): the BERT pooler + classifier or the RoBERTa
classifier.dense + out_proj, and the activation, in fp32 on the device. Nothing of the forward executes in torch.

Checkpoints: config.json with a *ForSequenceClassification architecture and model_type bert, roberta or xlm-roberta,
resolved as SentenceTransformer resolves a name (a local directory, then the sentence-transformers and Hugging Face
caches, offline). A name with no checkpoint on disk still constructs -- the reference constructs one whether or not it
will use it -- and `predict` raises QstError (a RuntimeError) saying where it looked. With `num_labels`, a bare encoder (or a
checkpoint without the head tensors) gets a new head, initialised as transformers initialises one.

Around training: `smart_batching_collate`, `save` / `save_pretrained` (a directory transformers' AutoModelForSequenceClassification
and CrossEncoder both load) and, in cross_encoder_evaluation, the evaluators of 2.2.2. `fit` itself refuses: the library has no
training step for the head.
"""
from __future__ import annotations

import importlib
import json
import os
from dataclasses import dataclass, replace
from typing import Callable, Dict, List, Optional

import numpy as np
import torch
from torch import nn

from . import _lib
from .config import ARCH_BERT, EncoderConfig, build_layout, hf_param_views
from .sentence_transformer import _find_cached_model, _load_model_dir_sd, load_tokenizer

HEAD_ALIGN = 64          # floats: every tensor of the head buffer starts on a 256-byte boundary (W1 is read as float4)
MAX_LABELS = 8           # qst_cls_head_fwd: 1 <= C <= 8

# head tensors of the two checkpoint families (model prefix stripped): (dense [H, H], out [C, H]) weight names
HEAD_NAMES = {
    "bert": ("pooler.dense", "classifier"),                 # BertForSequenceClassification
    "roberta": ("classifier.dense", "classifier.out_proj"),  # RobertaForSequenceClassification (and XLM-R)
}


@dataclass
class CrossEncoderCheckpoint:
    """What a *ForSequenceClassification directory holds, on the host: the encoder (config and fp32 arena, layout of
    config.build_layout), the head as one flat fp32 buffer (W1 | b1 | W2 | b2 at `head_offsets`), and its settings."""
    path: str
    cfg: EncoderConfig
    arena: np.ndarray
    head: np.ndarray
    head_offsets: Dict[str, int]
    num_labels: int
    hf_config: dict


def _align(n: int) -> int:
    return (n + HEAD_ALIGN - 1) // HEAD_ALIGN * HEAD_ALIGN


def check_widths(cfg: EncoderConfig) -> None:
    """The encoder limits of qst_encoder_create, checked without a device so that construction fails early and clearly."""
    H, A, I = cfg.hidden_size, cfg.num_heads, cfg.intermediate_size
    bad = []
    if H % 64 != 0 or H > 1024:
        bad.append(f"hidden_size {H} (a multiple of 64, at most 1024)")
    if H % A != 0 or H // A not in (32, 64):
        bad.append(f"head width {H}/{A} (32 or 64)")
    if I % 64 != 0:
        bad.append(f"intermediate_size {I} (a multiple of 64)")
    if cfg.type_vocab_size > 2:
        bad.append(f"type_vocab_size {cfg.type_vocab_size} (at most 2)")
    if bad:
        raise _lib.QstError("this checkpoint's widths are outside what the HIP encoder is built for: " + "; ".join(bad) +
                            ". There is no torch fallback.")


def _new_linear(out_features: int, in_features: int, std: float):
    """A Linear as transformers' _init_weights leaves it: weight normal(0, initializer_range) drawn from torch's global
    generator (torch.manual_seed makes it reproducible), zero bias."""
    return torch.empty(out_features, in_features, dtype=torch.float32).normal_(mean=0.0, std=std), \
        torch.zeros(out_features, dtype=torch.float32)


def load_checkpoint(path: str, num_labels: Optional[int] = None) -> CrossEncoderCheckpoint:
    """Read a cross-encoder directory on the host (no device needed).

    A *ForSequenceClassification checkpoint brings its head, and `num_labels`, if given, must agree with it. A bare encoder
    (another architecture in config.json) or a checkpoint without the head tensors gets a NEW head of `num_labels` outputs,
    built as transformers builds one; a head tensor pair the checkpoint does hold in the right shape is kept (a BERT
    checkpoint's pooler.dense). Without `num_labels` there is nothing to build, and such a directory is refused."""
    hf = json.load(open(os.path.join(path, "config.json")))
    archs = hf.get("architectures") or []
    trained = any(a.endswith("ForSequenceClassification") for a in archs)
    if not trained and num_labels is None:
        raise NotImplementedError(f"{path}: a cross-encoder checkpoint is a *ForSequenceClassification model; config.json "
                                  f"names {archs or 'no architecture'} (pass num_labels to put a new head on an encoder)")
    mt = hf.get("model_type", "bert")
    if mt not in ("bert", "roberta", "xlm-roberta"):
        raise NotImplementedError(f"{path}: model_type '{mt}' is not on the accelerated path (bert, roberta, xlm-roberta)")
    cfg, arena, _, sd = _load_model_dir_sd(path)
    cfg = replace(cfg, pooling="cls", normalize=False)
    check_widths(cfg)
    dense, outp = HEAD_NAMES["bert" if mt == "bert" else "roberta"]
    H = cfg.hidden_size
    missing = [n for n in (dense + ".weight", dense + ".bias", outp + ".weight", outp + ".bias") if n not in sd]
    if trained and not (missing and num_labels is not None):
        if missing:
            raise KeyError(f"{path}: checkpoint lacks the classification head tensors {missing}")
        w1, b1 = sd[dense + ".weight"].to(torch.float32), sd[dense + ".bias"].to(torch.float32)
        w2, b2 = sd[outp + ".weight"].to(torch.float32), sd[outp + ".bias"].to(torch.float32)
        C = int(w2.shape[0])
        if tuple(w1.shape) != (H, H) or tuple(b1.shape) != (H,) or tuple(w2.shape) != (C, H) or tuple(b2.shape) != (C,):
            raise ValueError(f"{path}: head shapes {tuple(w1.shape)}, {tuple(w2.shape)} do not fit hidden_size {H}")
        if num_labels is not None and int(num_labels) != C:
            raise ValueError(f"{path}: num_labels={num_labels} but the checkpoint's classifier has {C} outputs (a trained "
                             "classifier is not replaced)")
    else:
        C = int(num_labels)
        std = float(hf.get("initializer_range", 0.02))

        def held(name, shape_w):
            w, b = sd.get(name + ".weight"), sd.get(name + ".bias")
            if w is not None and b is not None and tuple(w.shape) == shape_w and tuple(b.shape) == shape_w[:1]:
                return w.to(torch.float32), b.to(torch.float32)
            return None
        w1, b1 = held(dense, (H, H)) or _new_linear(H, H, std)
        w2, b2 = held(outp, (C, H)) or _new_linear(C, H, std)
        hf = dict(hf)
        hf["architectures"] = [{"bert": "BertForSequenceClassification", "roberta": "RobertaForSequenceClassification",
                               "xlm-roberta": "XLMRobertaForSequenceClassification"}[mt]]
    if not 1 <= C <= MAX_LABELS:
        raise _lib.QstError(f"{path}: {C} labels; the head kernel takes 1 to {MAX_LABELS}")
    offs, off = {}, 0
    for name, t in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)):
        offs[name] = off
        off = _align(off + t.numel())
    head = np.zeros(off, np.float32)
    for name, t in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)):
        head[offs[name]:offs[name] + t.numel()] = t.numpy().reshape(-1)
    return CrossEncoderCheckpoint(path, cfg, arena, head, offs, C, hf)


def _import_from_string(dotted: str):
    mod, _, name = dotted.rpartition(".")
    return getattr(importlib.import_module(mod), name)


def default_activation(hf_config: dict, num_labels: int):
    """ST 2.2.2: config.json's sbert_ce_default_activation_function if present, else Sigmoid for one label, else Identity."""
    name = hf_config.get("sbert_ce_default_activation_function")
    if name:
        return _import_from_string(name)()
    return nn.Sigmoid() if num_labels == 1 else nn.Identity()


def _kernel_act(fct) -> Optional[int]:
    """The head kernel's act for an activation the kernel applies itself (None: a callable applied to its logits)."""
    if isinstance(fct, nn.Sigmoid):
        return 1
    if isinstance(fct, nn.Identity):
        return 0
    return None


class CrossEncoder:
    def __init__(self, model_name: str, num_labels: Optional[int] = None, max_length: Optional[int] = None,
                 device: Optional[str] = None, tokenizer_args: Optional[dict] = None,
                 automodel_args: Optional[dict] = None, default_activation_function=None, precision: str = "bf16"):
        """As sentence-transformers 2.2.2. `num_labels`: must agree with a trained classifier; on a bare encoder it builds a
        new head of that many outputs (load_checkpoint). `precision`: the encoder's precision in predict() ("bf16", "bf16x3" -- scores
        within rtol 1e-3 / atol 1e-4 of fp32 --, "f16", "f16w" or "fp8"); the head always runs in fp32.
        tokenizer_args / automodel_args are accepted for the signature and ignored (offline, fp32 weights)."""
        self.model_name = model_name
        self.max_length = max_length
        self.precision = precision
        self._device_name = device
        self._enc = None
        self._head_dev = None
        self._ckpt: Optional[CrossEncoderCheckpoint] = None
        path = str(model_name) if os.path.isdir(str(model_name)) else _find_cached_model(str(model_name))
        if path is None:
            # the reference constructs this object at import whether or not it will score anything: fail on use
            self._missing = (f"CrossEncoder({model_name!r}): no checkpoint on this machine (looked in "
                             "$SENTENCE_TRANSFORMERS_HOME, the torch sentence_transformers cache and the Hugging Face hub "
                             "cache; there is no network access). Pass a local *ForSequenceClassification directory.")
            self.config, self.tokenizer, self.default_activation_function = None, None, None
            return
        self._missing = None
        ckpt = load_checkpoint(path, num_labels)
        self._ckpt = ckpt
        self.config = ckpt.hf_config
        self.num_labels = ckpt.num_labels
        self.tokenizer = load_tokenizer(path, ckpt.cfg)
        if self.tokenizer is None:
            raise FileNotFoundError(f"{path}: a cross-encoder needs its tokenizer files (tokenizer.json / vocab.txt / ...)")
        self.default_activation_function = (default_activation_function if default_activation_function is not None
                                            else default_activation(ckpt.hf_config, ckpt.num_labels))
        if torch.cuda.is_available():
            self._to_device()

    # ---- device state: the encoder arena (HipEncoder) and the head's own small fp32 buffer
    def _to_device(self):
        if self._missing is not None:
            raise _lib.QstError(self._missing)
        if self._enc is not None:
            return
        from .encoder import HipEncoder
        if not torch.cuda.is_available():
            raise _lib.QstError("CrossEncoder needs a HIP device and none is visible: this build has no CPU path")
        dev = torch.device(self._device_name or "cuda")
        if dev.type != "cuda":
            raise _lib.QstError(f"CrossEncoder needs a HIP device (got '{dev}'): this build has no CPU path")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        ck = self._ckpt
        enc = HipEncoder(ck.cfg, device=dev)
        enc.load_arena(ck.arena)
        self._head_dev = torch.from_numpy(ck.head).to(dev)
        self._enc = enc
        self._ckpt = replace(ck, arena=np.zeros(0, np.float32))      # the host copy of the encoder is no longer needed

    @property
    def device(self) -> torch.device:
        self._to_device()
        return self._enc.device

    # ---- what surrounds training (sentence-transformers 2.2.2 CrossEncoder.fit's collate_fn; fit itself refuses, below)
    def smart_batching_collate(self, batch):
        """As 2.2.2: the columns of InputExample.texts, stripped, tokenised together; labels float for one label, long
        otherwise. Everything stays on the host. RoBERTa / XLM-R: no token_type_ids."""
        texts = [[] for _ in range(len(batch[0].texts))]
        labels = []
        for example in batch:
            for idx, text in enumerate(example.texts):
                texts[idx].append(text.strip())
            labels.append(example.label)
        tokenized = self.tokenizer(*texts, padding=True, truncation="longest_first", return_tensors="pt",
                                   max_length=self._max_len())
        tokenized = {k: v for k, v in tokenized.items()}
        if self._ckpt.cfg.arch != ARCH_BERT:
            tokenized.pop("token_type_ids", None)
        labels = torch.tensor(labels, dtype=torch.float if self.num_labels == 1 else torch.long)
        return tokenized, labels

    def fit(self, *args, **kwargs):
        raise NotImplementedError("CrossEncoder.fit: cross-encoder training is not part of this build. What surrounds it is: a "
                                  "new head on a bare encoder (num_labels=...), smart_batching_collate, save() / "
                                  "save_pretrained() and the evaluators of cross_encoder_evaluation; the training step itself "
                                  "(the head's training forward and backward, the loss) is not; the joint optimiser step over "
                                  "encoder and head is HipEncoder.adamw_step(extra=...)")

    # ---- saving: a directory transformers' AutoModelForSequenceClassification and CrossEncoder(path) both load
    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Every tensor under its transformers name (model prefix and head names restored), on the host."""
        if self._missing is not None:
            raise _lib.QstError(self._missing)
        ck = self._ckpt
        cfg = ck.cfg
        bert = cfg.arch == ARCH_BERT
        prefix = "bert." if bert else "roberta."
        out = {}
        if self._enc is not None:
            for name, v in self._enc.named_views().items():
                out[prefix + name] = v.detach().cpu().contiguous().clone()
            head = self._head_dev.detach().cpu()
        else:
            so = {s.name: s for s in build_layout(cfg)[0]}
            for name, seg, off, shape in hf_param_views(cfg):
                o = so[seg].offset + off
                out[prefix + name] = torch.from_numpy(ck.arena[o:o + int(np.prod(shape))].reshape(shape).copy())
            head = torch.from_numpy(ck.head)
        dense, outp = HEAD_NAMES["bert" if bert else "roberta"]
        H, C, off = cfg.hidden_size, ck.num_labels, ck.head_offsets
        for key, name, shape in (("w1", dense + ".weight", (H, H)), ("b1", dense + ".bias", (H,)),
                                 ("w2", outp + ".weight", (C, H)), ("b2", outp + ".bias", (C,))):
            full = prefix + name if name.startswith("pooler.") else name        # BERT's pooler sits inside the base model
            out[full] = head[off[key]:off[key] + int(np.prod(shape))].reshape(shape).clone()
        return out

    def save(self, path: Optional[str]) -> None:
        """model.safetensors under transformers' names, config.json (architectures, id2label / label2id for num_labels, the
        dropout fields and sbert_ce_default_activation_function as loaded) and the tokenizer files. Works from the host
        copy when no device was ever opened."""
        if path is None:
            return
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        save_file(self.state_dict(), os.path.join(path, "model.safetensors"), metadata={"format": "pt"})
        hf = dict(self.config)
        C = self.num_labels
        if len(hf.get("id2label") or {}) != C:
            hf["id2label"] = {str(i): f"LABEL_{i}" for i in range(C)}
            hf["label2id"] = {f"LABEL_{i}": i for i in range(C)}
        hf.pop("num_labels", None)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(hf, f, indent=2)
        self.tokenizer.save_pretrained(path)

    def save_pretrained(self, path: Optional[str]) -> None:
        return self.save(path)

    # ---- tokenisation (ST 2.2.2 smart_batching_collate_text_only)
    def _max_len(self) -> int:
        cfg = self._ckpt.cfg
        limit = min(512, cfg.max_position - (0 if cfg.arch == ARCH_BERT else cfg.pad_token_id + 1))
        m = self.max_length if self.max_length is not None else getattr(self.tokenizer, "model_max_length", limit)
        return int(min(limit, m if m is not None else limit))

    def tokenize_pairs(self, pairs) -> Dict[str, torch.Tensor]:
        a = [str(p[0]).strip() for p in pairs]
        b = [str(p[1]).strip() for p in pairs]
        out = self.tokenizer(a, b, padding=True, truncation="longest_first", return_tensors="pt", max_length=self._max_len())
        out = {k: v for k, v in out.items()}
        if self._ckpt.cfg.arch != ARCH_BERT:
            out.pop("token_type_ids", None)        # RoBERTa / XLM-R: one type row, all ids 0
        return out

    # ---- scoring
    def _logits(self, feats, act: int, softmax: int, precision: str) -> torch.Tensor:
        """[n, C] scores of one tokenised batch: encoder (cls, no normalisation) -> qst_cls_head_fwd."""
        enc, cfg, dev = self._enc, self._ckpt.cfg, self._enc.device
        ids = feats["input_ids"].to(dev, torch.int64)
        mask = feats["attention_mask"].to(dev, torch.int64)
        types = feats.get("token_type_ids")
        types = types.to(dev, torch.int64) if types is not None else None
        ids, mask, types, _ = enc.pad_inputs(ids, mask, types, cfg.pad_token_id)
        n, L = ids.shape
        C = self._ckpt.num_labels
        out = torch.empty(n, C, dtype=torch.float32, device=dev)
        # the encoder's 32-bit buffer offsets: nseq * L * I * 2 < 2^32 (include/qst.h); larger batches go in pieces
        rows = max(1, ((1 << 32) - 1) // (L * cfg.intermediate_size * 2))
        off, hd = self._ckpt.head_offsets, self._head_dev
        for s in range(0, n, rows):
            e = min(n, s + rows)
            emb, _, _ = enc.forward(ids[s:e], mask[s:e], None if types is None else types[s:e], training=False,
                                    precision=precision)
            _lib.check(enc.lib.qst_cls_head_fwd(
                emb.data_ptr(), emb.shape[1], e - s, cfg.hidden_size, hd.data_ptr() + 4 * off["w1"],
                hd.data_ptr() + 4 * off["b1"], hd.data_ptr() + 4 * off["w2"], hd.data_ptr() + 4 * off["b2"], C, act,
                softmax, out[s:e].data_ptr(), _lib.current_stream_ptr()), "qst_cls_head_fwd")
        return out

    def predict(self, sentences, batch_size: int = 32, show_progress_bar: Optional[bool] = None, num_workers: int = 0,
                activation_fct: Optional[Callable] = None, apply_softmax: bool = False, convert_to_numpy: bool = True,
                convert_to_tensor: bool = False, precision: Optional[str] = None):
        """Scores of [text_a, text_b] pairs, as sentence-transformers 2.2.2 CrossEncoder.predict returns them: [n] for one
        label, else [n, C]; one pair -> a scalar / one row; numpy, or a tensor with convert_to_tensor.

        activation_fct (default: the model's default_activation_function): torch.nn.Sigmoid and torch.nn.Identity run in
        the head kernel. Any other callable is applied, in torch, to the raw logits the kernel returns, and the softmax of
        apply_softmax then follows in torch as well. Pairs are scored in batches sorted by length (less padding); the
        result is in input order."""
        self._to_device()
        if len(sentences) == 0:
            return torch.zeros(0) if convert_to_tensor else np.zeros(0, np.float32)
        single = isinstance(sentences[0], str)
        if single:
            sentences = [sentences]
        fct = self.default_activation_function if activation_fct is None else activation_fct
        act = _kernel_act(fct)
        C = self._ckpt.num_labels
        softmax = int(bool(apply_softmax) and C > 1)
        prec = precision or self.precision
        order = np.argsort([-(len(str(p[0])) + len(str(p[1]))) for p in sentences], kind="stable")
        chunks = []
        with torch.no_grad(), torch.cuda.device(self._enc.device):
            for start in range(0, len(order), batch_size):
                batch = [sentences[i] for i in order[start:start + batch_size]]
                feats = self.tokenize_pairs(batch)
                if act is not None:
                    z = self._logits(feats, act, softmax, prec)
                else:
                    z = fct(self._logits(feats, 0, 0, prec))
                    if softmax:
                        z = torch.nn.functional.softmax(z, dim=1)
                chunks.append(z)
        scores = torch.cat(chunks, 0)
        inv = torch.as_tensor(np.argsort(order), device=scores.device)
        scores = scores[inv]
        if C == 1:
            scores = scores[:, 0]
        if not convert_to_tensor and convert_to_numpy:
            scores = scores.detach().cpu().numpy()
        elif not convert_to_tensor:
            scores = list(scores)
        return scores[0] if single else scores
