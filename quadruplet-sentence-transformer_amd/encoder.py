"""HipEncoder: torch tensors as storage, libqst.so as the only executor.

Owns the flat fp32 parameter / gradient / Adam-moment arenas and the bf16
operand shadow on one GPU and drives the C-ABI (include/qst.h). No
torch.nn.Module executes anything here; torch is used for device memory and
streams only (ownership rule).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .config import EncoderConfig, build_layout, hf_param_views, pooling_mask


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


@dataclass(frozen=True)
class _Precision:
    """What HipEncoder knows about one precision of include/qst.h. A further precision is one more row of _PRECISIONS."""
    name: str
    aliases: tuple
    code: int                                  # QST_PREC_*
    shadow_size: Optional[str] = None          # the size call of its operand shadow, on its own config (None: no shadow)
    shadow_dtype: Optional[torch.dtype] = None
    refresh: Optional[str] = None              # the entry point that fills the shadow from the fp32 parameters
    bwd_shadow: str = "bf16"                   # the precision whose shadow its BACKWARD reads
    train_needs_bf16: bool = False             # a training forward / a backward also wants the bf16 shadow fresh
    train_saved: str = "saved"                 # the shared arena a training forward keeps its activations in
    bwd_ws: str = "ws"                         # the shared arena of the backward's workspace


_PRECISIONS = (
    _Precision("bf16", (0, None), 0, "qst_shadow_elems", torch.bfloat16, refresh="qst_refresh_shadow"),
    # the fp32-class parity path over the SAME arenas: no shadow of its own, activation arena / scratch apart from bf16's
    _Precision("bf16x3", (1,), 1, train_saved="saved_x3", bwd_ws="ws_x3"),
    # MXFP8 weights (e4m3 + one E8M0 scale per 32 input features) and activations on the fp8 matrix cores; its backward runs
    # on the bf16 shadows
    _Precision("fp8", (3,), 3, "qst_shadow8_bytes", torch.uint8, refresh="qst_refresh_shadow_mx", train_needs_bf16=True,
               train_saved="saved_x3"),
    # the bf16 kernels compiled on IEEE half: [W | W^T] of every Linear weight as f16
    _Precision("f16", ("fp16", 4), 4, "qst_shadow_elems", torch.float16, refresh="qst_refresh_shadow", bwd_shadow="f16"),
    # f16 with split weights (hi + lo) in the forward: shadow = [f16 arena | low halves]
    _Precision("f16w", (5,), 5, "qst_shadow_elems", torch.float16, refresh="qst_refresh_shadow", bwd_shadow="f16w"),
)
_BY_ALIAS = {a: p for p in _PRECISIONS for a in (p.name, *p.aliases)}


def _precision(precision) -> _Precision:
    try:
        return _BY_ALIAS[precision]
    except (KeyError, TypeError):
        raise ValueError(f"unknown precision {precision!r} (bf16 | f16 | f16w | bf16x3 | fp8)") from None


@dataclass
class _Live:
    """One created precision of one encoder: its handle over the shared arenas, its operand shadow and whether the
    parameters have changed since that shadow was filled."""
    spec: _Precision
    handle: object
    shadow: Optional[torch.Tensor]
    stale: bool = True


def _stale_flag(name: str) -> property:
    """shadow*_stale of precision `name`, readable and assignable whether or not that precision exists yet (it appears stale)."""
    def get(self) -> bool:
        rec = self._live.get(name)
        return True if rec is None else rec.stale

    def put(self, stale) -> None:
        rec = self._live.get(name)
        if rec is not None:
            rec.stale = bool(stale)
    return property(get, put)


class HipEncoder:
    def __init__(self, cfg: EncoderConfig, device: Optional[torch.device] = None, precision: int = 0):
        self.cfg = cfg
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.QstError("HipEncoder needs a HIP device; there is no CPU fallback")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(self.device)
        self.ccfg = _lib.make_config(cfg, precision)
        self.segments, self.total = build_layout(cfg)
        n = self.lib.qst_arena_elems(self.ccfg)
        if n != self.total:
            raise _lib.QstError(f"arena layout mismatch: python {self.total} vs libqst {n}")
        self.pool_mode = pooling_mask(cfg.pooling)     # include/qst.h QST_POOL_*: set on every handle this encoder creates
        self.dropout = None           # (p_hidden, p_attn, seed) once set_dropout() switched it on
        self.dropout_step = 0
        self.drop_state = None
        self.ln_fusion = 0
        self.wgrad_pairs = 0
        self._live: Dict[str, _Live] = {}       # canonical precision name -> what exists of it; created on first use
        self._record("bf16")
        self.emb_dim = self.lib.qst_encoder_embedding_dim(self.handle)
        if self.emb_dim != cfg.embedding_dim:
            raise _lib.QstError(f"embedding width mismatch: python {cfg.embedding_dim} vs libqst {self.emb_dim}")
        self.amp_scaler: Optional[torch.Tensor] = None   # device fp32 [4] {loss scale, growth tracker, last skipped, #skipped}
        self._step2_dev: Optional[torch.Tensor] = None   # device int64 [2] {optimiser steps, scheduler steps} of the amp step
        self.params = torch.zeros(self.total, dtype=torch.float32, device=self.device)
        self.grads: Optional[torch.Tensor] = None
        self.exp_avg: Optional[torch.Tensor] = None
        self.exp_avg_sq: Optional[torch.Tensor] = None
        self._arenas: Dict[str, torch.Tensor] = {}        # shared byte arenas by name (_Precision.train_saved / .bwd_ws)
        self._scratch = torch.zeros(2048, dtype=torch.float32, device=self.device)
        self._step_dev: Optional[torch.Tensor] = None    # device-side optimiser step counter (graph-captured steps)
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.opt_step = 0

    def _create(self, ccfg, what: str):
        """A new encoder handle with this encoder's pooling head, dropout setting (same rates, same device counter) and
        ln_fusion: the one place where a handle created late inherits what the earlier ones were told."""
        h = _lib.vp()
        _lib.check(self.lib.qst_encoder_create(ccfg, h), what)
        try:
            if self.pool_mode != pooling_mask("mean"):
                _lib.check(self.lib.qst_encoder_set_pooling(h, self.pool_mode), "qst_encoder_set_pooling")
            if self.dropout is not None:
                _lib.check(self.lib.qst_encoder_set_dropout(h, self.dropout[0], self.dropout[1], self.drop_state.data_ptr()),
                           "qst_encoder_set_dropout")
            if self.ln_fusion:
                _lib.check(self.lib.qst_encoder_set_ln_fusion(h, self.ln_fusion), "qst_encoder_set_ln_fusion")
            if self.wgrad_pairs:
                _lib.check(self.lib.qst_encoder_set_wgrad_pairs(h, self.wgrad_pairs), "qst_encoder_set_wgrad_pairs")
        except Exception:
            self.lib.qst_encoder_destroy(h)
            raise
        return h

    def _record(self, precision) -> _Live:
        """The live record of `precision` (a name or alias of _PRECISIONS), created on first use: an encoder that never runs
        a precision allocates nothing for it."""
        spec = _precision(precision)
        rec = self._live.get(spec.name)
        if rec is None:
            ccfg = self.ccfg if spec.name == "bf16" else _lib.make_config(self.cfg, spec.code)
            h = self._create(ccfg, f"qst_encoder_create({spec.name})")
            try:
                shadow = None if spec.shadow_size is None else torch.zeros(
                    getattr(self.lib, spec.shadow_size)(ccfg), dtype=spec.shadow_dtype, device=self.device)
            except Exception:
                self.lib.qst_encoder_destroy(h)
                raise
            rec = self._live[spec.name] = _Live(spec, h, shadow)
        return rec

    def _handle_for(self, precision):
        return self._record(precision).handle

    @property
    def handle(self):
        """The bf16 handle: the one the optimiser steps and set_ffn_chain go through."""
        return self._live["bf16"].handle

    shadow_stale = _stale_flag("bf16")
    shadow_mx_stale = _stale_flag("fp8")
    shadow_f16_stale = _stale_flag("f16")
    shadow_f16w_stale = _stale_flag("f16w")

    def __del__(self):
        try:
            while self._live:
                self.lib.qst_encoder_destroy(self._live.popitem()[1].handle)
        except Exception:
            pass

    # ------------------------------------------------------------------ parameters
    def load_arena(self, arena) -> None:
        t = torch.as_tensor(np.asarray(arena), dtype=torch.float32) if not torch.is_tensor(arena) else arena
        if t.numel() != self.total:
            raise ValueError(f"arena has {t.numel()} elements, expected {self.total}")
        self.params.copy_(t.to(self.device))
        self.mark_stale()

    def named_views(self) -> Dict[str, torch.Tensor]:
        """HF-named views into the parameter arena (no copies)."""
        seg = {s.name: s for s in self.segments}
        out = {}
        for name, sname, off, shape in hf_param_views(self.cfg):
            s = seg[sname]
            n = int(np.prod(shape))
            out[name] = self.params[s.offset + off: s.offset + off + n].view(*shape)
        return out

    def grad_views(self) -> Dict[str, torch.Tensor]:
        self.ensure_train_state()
        seg = {s.name: s for s in self.segments}
        out = {}
        for name, sname, off, shape in hf_param_views(self.cfg):
            s = seg[sname]
            n = int(np.prod(shape))
            out[name] = self.grads[s.offset + off: s.offset + off + n].view(*shape)
        return out

    def ensure_train_state(self) -> None:
        if self.grads is None:
            self.grads = torch.zeros_like(self.params)
        if self.exp_avg is None:
            self.exp_avg = torch.zeros_like(self.params)
            self.exp_avg_sq = torch.zeros_like(self.params)

    # ------------------------------------------------------------------ dropout
    def set_dropout(self, p_hidden: float = 0.0, p_attn: float = 0.0, seed: int = 0) -> None:
        """Dropout for training forwards/backwards (HF hidden_dropout_prob / attention_probs_dropout_prob; the reference's
        fit() trains in train() mode with 0.1 / 0.1). Masks are counter-based -- a function of (seed, step, tensor, element)
        recomputed by the backward kernels, never stored; `dropout_step` counts the training forwards run since this call
        (the device-side counter the kernels read). 0 / 0 switches dropout off. Inference forwards never drop."""
        if not (0.0 <= p_hidden < 1.0 and 0.0 <= p_attn < 1.0):
            raise ValueError("dropout probabilities must be in [0, 1)")
        on = p_hidden > 0.0 or p_attn > 0.0
        if on:
            if self.drop_state is None:
                self.drop_state = torch.zeros(4, dtype=torch.int32, device=self.device)
            _lib.check(self.lib.qst_dropout_init(self.drop_state.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                 _lib.current_stream_ptr()), "qst_dropout_init")
        for rec in self._live.values():                 # every precision's training forward drops at the same places
            _lib.check(self.lib.qst_encoder_set_dropout(rec.handle, float(p_hidden), float(p_attn),
                                                        self.drop_state.data_ptr() if on else None), "qst_encoder_set_dropout")
        self.dropout = (float(p_hidden), float(p_attn), int(seed)) if on else None
        self.dropout_step = 0

    def set_ffn_chain(self, mask: int) -> None:
        """Where the feed-forward block runs as one kernel (include/qst.h qst_encoder_set_ffn_chain): bit 0 inference
        forward (default), bit 1 training forward, bit 2 backward."""
        _lib.check(self.lib.qst_encoder_set_ffn_chain(self.handle, int(mask)), "qst_encoder_set_ffn_chain")

    def set_ln_fusion(self, mode: int) -> None:
        """Where a projection + LayerNorm (and a dgrad + LayerNorm backward) run as one kernel (include/qst.h
        qst_encoder_set_ln_fusion): 0 by size (default), 1 wherever such a kernel exists, 2 never. Every precision's handle."""
        for rec in self._live.values():
            _lib.check(self.lib.qst_encoder_set_ln_fusion(rec.handle, int(mode)), "qst_encoder_set_ln_fusion")
        self.ln_fusion = int(mode)

    def set_wgrad_pairs(self, mode: int) -> None:
        """How a backward issues the weight gradients (include/qst.h qst_encoder_set_wgrad_pairs): 0 the library's choice
        (default), 1 one grouped launch per layer, 2 one launch for two neighbouring layers wherever a call covers both.
        Every precision's handle; the backward workspace of a handle that may pair is larger (bwd_workspace_bytes)."""
        for rec in self._live.values():
            _lib.check(self.lib.qst_encoder_set_wgrad_pairs(rec.handle, int(mode)), "qst_encoder_set_wgrad_pairs")
        self.wgrad_pairs = int(mode)

    def set_dropout_step(self, step: int) -> None:
        """Continue the mask stream at `step` training forwards (checkpoint resume)."""
        if self.dropout is not None:
            self.drop_state[2] = int(step)
            self.dropout_step = int(step)

    # ------------------------------------------------------------------ operand shadows
    def refresh_shadow(self, precision="bf16") -> None:
        """Fill the operand shadow of `precision` from the fp32 parameters: [W | W^T] of every Linear weight in bf16 / IEEE
        half (f16w: and, behind it, the low halves of the split weights), or the MXFP8 quantisation (fp8)."""
        rec = self._record(precision)
        if rec.shadow is None:
            raise ValueError(f"precision {rec.spec.name!r} has no operand shadow")
        _lib.check(getattr(self.lib, rec.spec.refresh)(rec.handle, self.params.data_ptr(), rec.shadow.data_ptr(),
                                                       _lib.current_stream_ptr()), f"{rec.spec.refresh}({rec.spec.name})")
        rec.stale = False

    def mark_stale(self, keep=None) -> None:
        """The parameters changed: the shadow of every created precision is stale, except that of `keep`, which was refreshed
        after the change (a replayed graph ends with that refresh)."""
        fresh = None if keep is None else _precision(keep).name
        for name, rec in self._live.items():
            rec.stale = name != fresh

    # ------------------------------------------------------------------ shapes
    @staticmethod
    def pad_inputs(ids: torch.Tensor, mask: torch.Tensor, type_ids: Optional[torch.Tensor], pad_id: int
                   ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], int]:
        """Pad L up to a multiple of 32 with masked positions (outputs do not depend on padded content)."""
        n, L = ids.shape
        Lp = _round_up(L, 32)
        if Lp != L:
            ids = torch.nn.functional.pad(ids, (0, Lp - L), value=pad_id)
            mask = torch.nn.functional.pad(mask, (0, Lp - L), value=0)
            if type_ids is not None:
                type_ids = torch.nn.functional.pad(type_ids, (0, Lp - L), value=0)
        return ids.contiguous(), mask.contiguous(), None if type_ids is None else type_ids.contiguous(), L

    def _arena(self, name: str, nbytes: int) -> torch.Tensor:
        buf = self._arenas.get(name)
        if buf is None or buf.numel() < nbytes:
            buf = self._arenas[name] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return buf

    def saved_bytes(self, precision, n: int, L: int, training: bool) -> int:
        """Bytes of the activation arena a forward of [n, L] at `precision` fills (0: unsupported shape)."""
        return self.lib.qst_encoder_saved_bytes(self._record(precision).handle, n, L, int(training))

    def bwd_workspace_bytes(self, precision, n: int, L: int) -> int:
        return self.lib.qst_encoder_bwd_workspace_bytes(self._record(precision).handle, n, L)

    # ------------------------------------------------------------------ forward / backward
    def forward(self, ids: torch.Tensor, mask: torch.Tensor, type_ids: Optional[torch.Tensor] = None,
                training: bool = False, want_tokens: bool = False, saved: Optional[torch.Tensor] = None,
                precision: str = "bf16"):
        """ids/mask int64 [n, L] on this device, L % 32 == 0. Returns (emb [n,D], tok [n,L,H] or None, saved); D =
        cfg.embedding_dim (H for mean pooling).
        precision="bf16x3" runs the fp32-class parity path, "fp8" the fp8 matrix-core path (MXFP8 weights and
        activations). training=True keeps what the matching backward(precision=...) needs."""
        assert ids.dtype == torch.int64 and mask.dtype == torch.int64 and ids.is_cuda and ids.is_contiguous()
        n, L = ids.shape
        rec = self._record(precision)
        if training and rec.spec.train_needs_bf16 and self.shadow_stale:
            self.refresh_shadow("bf16")          # (an fp8 training forward: its backward runs on the bf16 shadows)
        if rec.shadow is not None and rec.stale:
            self.refresh_shadow(rec.spec.name)
        # bf16x3 has no shadow and reads none: it is handed the bf16 buffer as it is
        shadow = rec.shadow if rec.shadow is not None else self._live["bf16"].shadow
        nbytes = self.saved_bytes(precision, n, L, training)
        if nbytes == 0:
            raise _lib.QstError(f"unsupported shape nseq={n} L={L} for this encoder (L % 32 == 0, L <= 512)")
        if saved is None:
            saved = self._arena(rec.spec.train_saved if training else "saved", nbytes)
        emb = torch.empty(n, self.emb_dim, dtype=torch.float32, device=self.device)
        tok = torch.empty(n, L, self.cfg.hidden_size, dtype=torch.float32, device=self.device) if want_tokens else None
        _lib.check(self.lib.qst_encoder_forward(
            rec.handle, ids.data_ptr(), mask.data_ptr(), _lib.ptr(type_ids), n, L, self.params.data_ptr(),
            shadow.data_ptr(), emb.data_ptr(), _lib.ptr(tok), saved.data_ptr(), saved.numel(), int(training),
            _lib.current_stream_ptr()), "qst_encoder_forward")
        if training and self.dropout is not None:
            self.dropout_step += 1           # mirrors the device counter (tests rebuild this step's masks from it)
        return emb, tok, saved

    def backward_operands(self, precision, n: int, L: int, ws: Optional[torch.Tensor] = None):
        """(handle, shadow, workspace) of a backward of [n, L] at `precision`: the [W | W^T] shadow the table names (IEEE half
        for f16 / f16w, bf16 otherwise; refreshed if an fp8 backward finds it stale) and, unless the caller brings `ws`,
        that precision's shared workspace."""
        rec = self._record(precision)
        if rec.spec.train_needs_bf16 and self.shadow_stale:
            self.refresh_shadow("bf16")
        if ws is None:
            ws = self._arena(rec.spec.bwd_ws, self.bwd_workspace_bytes(precision, n, L))
        return rec.handle, self._live[rec.spec.bwd_shadow].shadow, ws

    def backward(self, ids, mask, type_ids, grad_emb: torch.Tensor, saved: torch.Tensor, precision: str = "bf16") -> None:
        """Accumulate d(loss)/d(params) into self.grads given d(loss)/d(emb). precision="bf16x3": the fp32-class backward
        of a forward(training=True, precision="bf16x3") (the parity path: one call); "fp8": the bf16
        backward over what a forward(training=True, precision="fp8") kept (fp8 forward GEMMs, bf16 dgrad / wgrad)."""
        self.ensure_train_state()
        n, L = ids.shape
        handle, shadow, ws = self.backward_operands(precision, n, L)
        grad_emb = grad_emb.contiguous()
        _lib.check(self.lib.qst_encoder_backward(
            handle, ids.data_ptr(), mask.data_ptr(), _lib.ptr(type_ids), n, L, self.params.data_ptr(),
            shadow.data_ptr(), grad_emb.data_ptr(), self.grads.data_ptr(), saved.data_ptr(), saved.numel(),
            ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()), "qst_encoder_backward")

    def adamw_step(self, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01,
                   max_grad_norm: float = 1.0, grad_scale: float = 1.0, extra=None) -> None:
        """clip_grad_norm_ + AdamW + zero_grad in one pass over the arena; the norm stays on the device. `extra`: a
        loss_params.LossParameters on this device, clipped on the joint norm and stepped with the arena
        (qst_clip_adamw_step_joint); None makes the call it always made."""
        if extra is not None and extra.ensure().device != self.device:
            raise _lib.QstError(f"adamw_step: the extra parameters live on {extra.device}, the encoder on {self.device}")
        self.opt_step += 1
        if extra is None:
            self._clip_adamw("qst_clip_adamw_step", lr, betas, eps, weight_decay, max_grad_norm, grad_scale, self.opt_step)
            return
        extra.ensure_state()
        self._clip_adamw("qst_clip_adamw_step_joint", lr, betas, eps, weight_decay, max_grad_norm, grad_scale, self.opt_step,
                         front=(extra.params.data_ptr(), extra.grads.data_ptr(), extra.exp_avg.data_ptr(),
                                extra.exp_avg_sq.data_ptr(), extra.chunk_decay.data_ptr(), extra.total))

    def _clip_adamw(self, entry: str, lr, betas, eps, weight_decay, max_grad_norm, grad_scale, *own, front=()) -> None:
        """What the four optimiser steps share: the arenas, then what an entry point takes in front of the AdamW arguments
        (`front`: the joint step's extra group), those arguments, the entry point's own (`own`), the norm and scratch
        behind them, and every shadow stale afterwards."""
        self.ensure_train_state()
        _lib.check(getattr(self.lib, entry)(
            self.handle, self.params.data_ptr(), self.grads.data_ptr(), self.exp_avg.data_ptr(),
            self.exp_avg_sq.data_ptr(), *front, lr, betas[0], betas[1], eps, weight_decay, max_grad_norm, grad_scale, *own,
            self.grad_norm.data_ptr(), self._scratch.data_ptr(), _lib.current_stream_ptr()), entry)
        self.mark_stale()

    # ------------------------------------------------------------------ optimiser state (true resume)
    def optimizer_state(self) -> Dict[str, torch.Tensor]:
        """The Adam moments as flat arenas (same layout as the parameters) + the step counter."""
        self.ensure_train_state()
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq,
                "opt_step": torch.tensor([self.opt_step], dtype=torch.int64)}

    def load_optimizer_state(self, state: Dict[str, torch.Tensor]) -> None:
        self.ensure_train_state()
        for k in ("exp_avg", "exp_avg_sq"):
            t = state[k]
            if t.numel() != self.total:
                raise ValueError(f"optimizer state '{k}' has {t.numel()} elements, expected {self.total}")
            getattr(self, k).copy_(t.to(self.device, dtype=torch.float32).view(-1))
        self.opt_step = int(state["opt_step"].view(-1)[0])
        if self._step_dev is not None:
            self._step_dev.fill_(self.opt_step)

    def adamw_step_sched(self, base_lr: float, warmup_steps: int, total_steps: int, betas=(0.9, 0.999),
                         eps: float = 1e-8, weight_decay: float = 0.01, max_grad_norm: float = 1.0,
                         grad_scale: float = 1.0) -> None:
        """adamw_step with the WarmupLinear schedule and the step counter on the device (no per-step host value is a
        kernel argument, so the call can sit inside a captured HIP graph). The counter starts from self.opt_step."""
        if self._step_dev is None:
            self._step_dev = torch.tensor([self.opt_step], dtype=torch.int64, device=self.device)
        self.opt_step += 1               # host mirror (bookkeeping only; the device counter is authoritative)
        self._clip_adamw("qst_clip_adamw_step_sched", base_lr, betas, eps, weight_decay, max_grad_norm, grad_scale,
                         int(warmup_steps), int(total_steps), self._step_dev.data_ptr())

    # ------------------------------------------------------------------ mixed precision (QST_PREC_F16 training)
    def ensure_amp_scaler(self, init_scale: float = 65536.0) -> torch.Tensor:
        """The loss scaler of f16 training on the device (include/qst.h qst_amp_scaler_init): fp32 [4] {scale, growth
        tracker, last step skipped, skipped steps}. torch.cuda.amp.GradScaler's default init_scale, as ST fit(use_amp=True)."""
        if self.amp_scaler is None:
            self.amp_scaler = torch.zeros(4, dtype=torch.float32, device=self.device)
            _lib.check(self.lib.qst_amp_scaler_init(self.amp_scaler.data_ptr(), float(init_scale), _lib.current_stream_ptr()),
                       "qst_amp_scaler_init")
        return self.amp_scaler

    def adamw_step_amp(self, base_lr: float, warmup_steps: int, total_steps: int, betas=(0.9, 0.999), eps: float = 1e-8,
                       weight_decay: float = 0.01, max_grad_norm: float = 1.0, grad_scale: float = 1.0,
                       growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000) -> None:
        """GradScaler.unscale_ + clip_grad_norm_ + GradScaler.step(AdamW) + update + zero_grad on the device
        (qst_clip_adamw_step_amp): the gradients in the arena carry the loss scale; a step whose gradients overflowed is
        skipped and halves the scale. total_steps <= 0: constant base_lr. No host value of the step depends on the outcome,
        so the call can sit inside a captured graph; self.opt_step counts CALLS (skipped steps are in amp_scaler[3])."""
        self.ensure_amp_scaler()
        if self._step2_dev is None:
            self._step2_dev = torch.tensor([self.opt_step, self.opt_step], dtype=torch.int64, device=self.device)
        self.opt_step += 1
        self._clip_adamw("qst_clip_adamw_step_amp", base_lr, betas, eps, weight_decay, max_grad_norm, grad_scale,
                         int(warmup_steps), int(total_steps), self._step2_dev.data_ptr(), self.amp_scaler.data_ptr(),
                         growth_factor, backoff_factor, int(growth_interval))

def quadruplet_loss_raw(xa, xp, xq, xn, gamma, m_pn, m_pq, m_qn, p, swap, reduction: int,
                        grad_out: Optional[torch.Tensor] = None, want_grads: bool = False):
    """Direct call of qst_quadruplet_loss on contiguous fp32 CUDA tensors [B, D]."""
    lib = _lib.load()
    B, D = xa.shape
    dev = xa.device
    out = torch.empty(B if reduction == 0 else 1, dtype=torch.float32, device=dev)
    scratch = torch.empty(B, dtype=torch.float32, device=dev)
    # the four gradients are the slabs of ONE [4, B, D] buffer: viewed as [4B, D] it is the encoder backward's
    # grad_emb for the fused four-column pass, with no concatenation in between
    grads = torch.empty(4, B, D, dtype=torch.float32, device=dev).unbind(0) if want_grads else [None] * 4
    _lib.check(lib.qst_quadruplet_loss(
        xa.data_ptr(), xp.data_ptr(), xq.data_ptr(), xn.data_ptr(), B, D, gamma, m_pn, m_pq, m_qn, p, int(swap),
        reduction, out.data_ptr(), _lib.ptr(grad_out), *[_lib.ptr(g) for g in grads], scratch.data_ptr(),
        _lib.current_stream_ptr()), "qst_quadruplet_loss")
    return out, list(grads)


def stacked(grads) -> torch.Tensor:
    """The [4B, D] view behind the four gradient slabs quadruplet_loss_raw returned (no copy)."""
    base = grads[0]._base
    assert base is not None and base.dim() == 3 and all(g._base is base for g in grads)
    return base.view(-1, base.shape[-1])
