"""Parameters a loss owns, outside the encoder's arena, in a form the fused optimiser step can take.

`LossParameters(module)` rehomes every parameter of `module` (the `nn.Linear` classifier of `losses.SoftmaxLoss`, say) into
one flat fp32 buffer with the arena's conventions, so that qst_clip_adamw_step_joint (include/qst.h) runs optim.hip's
kernels on it unchanged:

  * every tensor starts at a multiple of 256 elements and is padded to one with zeros;
  * one decay flag per 256-element chunk: a tensor whose name ends in `bias` does not decay, every other does --
    sentence-transformers' `no_decay` filter, as the arena applies it;
  * `params`, `grads`, `exp_avg`, `exp_avg_sq` are flat buffers of the same size, the moments created when the first step
    asks for them.

The module's `nn.Parameter`s become views into `params` and their `.grad`s views into `grads` -- what SentenceTransformer
does with the encoder's parameters over the arena -- so autograd accumulates straight into the buffer the step reads, and
`state_dict()` / `load_state_dict()` stay plain `nn.Module` behaviour. `nn.Module._apply` (`.to()`, `.cuda()`, `.float()`)
replaces a parameter's `.data`: `ensure()` finds parameters that no longer live in the flat buffer, moves the buffers to
where they went, copies their values back in and rebuilds the views. The owner calls it at the start of every forward, fit()
before its first step.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import nn

CHUNK = 256


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


class LossParameters:
    def __init__(self, module: nn.Module, device=None):
        self.module = module
        if device is not None:
            module.to(device)
        named = list(module.named_parameters())
        if not named:
            raise ValueError("LossParameters: the module has no parameters")
        self.layout: List[Tuple[str, int, int, Tuple[int, ...], bool]] = []     # (name, offset, numel, shape, decay)
        off = 0
        for name, p in named:
            self.layout.append((name, off, p.numel(), tuple(p.shape), not name.endswith("bias")))
            off += _round_up(p.numel(), CHUNK)
        self.total = off
        dev = named[0][1].device
        self.params = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.exp_avg: Optional[torch.Tensor] = None
        self.exp_avg_sq: Optional[torch.Tensor] = None
        flags = torch.zeros(self.total // CHUNK, dtype=torch.uint8)
        for _, o, n, _, decay in self.layout:
            flags[o // CHUNK:(o + _round_up(n, CHUNK)) // CHUNK] = int(decay)
        self.chunk_decay = flags.to(dev)
        self.ensure()

    @property
    def device(self) -> torch.device:
        return self.params.device

    def _inside(self, t: Optional[torch.Tensor], buf: torch.Tensor, off: int) -> bool:
        return t is not None and t.device == buf.device and t.dtype == torch.float32 and \
            t.data_ptr() == buf.data_ptr() + 4 * off

    def _move(self, dev: torch.device) -> None:
        for k in ("params", "grads", "exp_avg", "exp_avg_sq", "chunk_decay"):
            t = getattr(self, k)
            if t is not None:
                setattr(self, k, t.to(dev))

    def ensure(self) -> "LossParameters":
        """Every parameter a view into `params` and every .grad a view into `grads`, on the device the parameters are on."""
        named = dict(self.module.named_parameters())
        first = named[self.layout[0][0]]
        if first.device != self.params.device:           # the module was moved: the buffers follow it
            self._move(first.device)
        with torch.no_grad():
            for name, off, n, shape, _ in self.layout:
                p = named[name]
                if not self._inside(p.data, self.params, off):
                    view = self.params[off:off + n].view(shape)
                    view.copy_(p.data.to(view.device, torch.float32))
                    p.data = view
                if not self._inside(p.grad, self.grads, off):
                    gview = self.grads[off:off + n].view(shape)
                    if p.grad is not None:
                        gview.copy_(p.grad.to(gview.device, torch.float32))
                    p.grad = gview
        return self

    def ensure_state(self) -> None:
        """The Adam moments, zero until the first step."""
        if self.exp_avg is None:
            self.exp_avg = torch.zeros_like(self.params)
            self.exp_avg_sq = torch.zeros_like(self.params)

    def zero_grad(self) -> None:
        self.grads.zero_()
