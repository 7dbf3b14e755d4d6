#!/usr/bin/env python
"""One SHA-256 per case over the raw bytes of everything an optimiser step writes (csrc/optim.hip behind
qst_clip_adamw_step, _joint, _sched, _amp): parameters, both moments and gradients of the arena and of the extra group,
norm_out, all 2048 floats of the scratch (the partial sums, then the extra group's partials or dyn), the device step
counters and the scaler, absorbed after every step of the case. Seeded inputs. Two builds that print the same file compute
the same bits.

The tool calls the entry points directly on buffers of its own; HipEncoder only provides the handle. So it depends on
nothing but the C ABI: --lib points it at another build of libqst.so (say, one of the parent commit).

Cases: every form on the smallest preset's arena (tiny-bert, inside one trip of every loop) and once on minilm-2l (several
trips). Plain: max_grad_norm 1 and 0, without norm_out, grad_scale 0.25. Joint: x_n 0, 256 and 1,048,576 + 256 (the extra
group's sumsq_kernel takes a second trip), flag-0 and flag-1 chunks. Sched: warmup 2 / total 5 over six steps (warmup, decay,
lr 0 past total) and total 0. Amp: good, inf, nan, then four good steps, with growth_interval 2000 and 2, total 0 and 5.

    python tools/optim_digest.py --out profiles/optim_digest_after.txt
"""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib  # noqa: E402
from quadruplet_sentence_transformer_amd.config import PRESETS  # noqa: E402
from quadruplet_sentence_transformer_amd.encoder import HipEncoder  # noqa: E402

HYPER = (1e-2, 0.9, 0.999, 1e-8, 0.01)          # lr, beta1, beta2, eps, weight_decay
SCALE = 1024.0


class Group:
    """params, grads, exp_avg, exp_avg_sq of n elements (the moments start as after some earlier step: nonzero)."""

    def __init__(self, n, gen):
        self.n = n
        self.p = (torch.randn(n, generator=gen) * 0.05).cuda()
        self.g = torch.zeros(n).cuda()
        self.m = (torch.randn(n, generator=gen) * 1e-3).cuda()
        self.v = (torch.rand(n, generator=gen) * 1e-6).cuda()

    def ptrs(self):
        return [t.data_ptr() for t in (self.p, self.g, self.m, self.v)]

    def tensors(self):
        return [self.p, self.g, self.m, self.v]


class Case:
    def __init__(self, lib, preset, x_n=0):
        self.lib, self.gen = lib, torch.Generator().manual_seed(7)
        self.enc = HipEncoder(PRESETS[preset])
        self.arena = Group(self.enc.total, self.gen)
        self.x = Group(x_n, self.gen) if x_n else None
        self.x_decay = (torch.arange(x_n // 256) % 2).to(torch.uint8).cuda() if x_n else None   # chunk 0 undecayed, 1 decayed ...
        self.norm = torch.full((1,), -1.0).cuda()
        self.scratch = torch.full((2048,), -1.0).cuda()
        self.steps = torch.zeros(2, dtype=torch.int64).cuda()
        self.scaler = torch.zeros(4).cuda()
        self.h = hashlib.sha256()

    def grads(self, std, scale=1.0, poison=None):
        for grp in filter(None, (self.arena, self.x)):
            g = torch.randn(grp.n, generator=self.gen) * (std * scale)
            if poison is not None and grp is self.arena:
                g[(2 * grp.n) // 3] = poison
            grp.g.copy_(g)

    def call(self, entry, front, own, max_norm, grad_scale, norm=True):
        st = getattr(self.lib, entry)(
            self.enc.handle, *self.arena.ptrs(), *front, *HYPER, max_norm, grad_scale, *own,
            self.norm.data_ptr() if norm else None, self.scratch.data_ptr() if norm else None, _lib.current_stream_ptr())
        _lib.check(st, entry)
        torch.cuda.synchronize()
        outs = self.arena.tensors() + (self.x.tensors() if self.x else []) + [self.norm, self.scratch, self.steps, self.scaler]
        for t in outs:
            self.h.update(t.cpu().numpy().tobytes())


def plain(lib, preset, max_norm, grad_scale, norm):
    c = Case(lib, preset)
    for step in (1, 2, 3):
        c.grads(3.0 if step == 1 else 1e-4)                 # the first step is clipped, the others are not
        c.call("qst_clip_adamw_step", (), (step,), max_norm, grad_scale, norm)
    return c


def joint(lib, preset, x_n, max_norm, norm=True):
    c = Case(lib, preset, x_n)
    front = (*c.x.ptrs(), c.x_decay.data_ptr(), x_n) if x_n else (None,) * 5 + (0,)
    for step in (1, 2, 3):
        c.grads(3.0 if step == 1 else 1e-4)
        c.call("qst_clip_adamw_step_joint", front, (step,), max_norm, 0.5, norm)
    return c


def sched(lib, preset, warmup, total, steps):
    c = Case(lib, preset)
    for step in range(steps):
        c.grads(3.0 if step == 0 else 1e-4)
        c.call("qst_clip_adamw_step_sched", (), (warmup, total, c.steps.data_ptr()), 1.0, 1.0)
    return c


def amp(lib, preset, warmup, total, interval, poisons):
    c = Case(lib, preset)
    _lib.check(lib.qst_amp_scaler_init(c.scaler.data_ptr(), SCALE, _lib.current_stream_ptr()), "qst_amp_scaler_init")
    for poison in poisons:
        c.grads(0.01, SCALE, poison)
        c.call("qst_clip_adamw_step_amp", (), (warmup, total, c.steps.data_ptr(), c.scaler.data_ptr(), 2.0, 0.5, interval), 1.0, 1.0)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libqst.so to load instead of the tree's")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    assert torch.cuda.is_available(), "this tool needs a HIP device"
    lib = _lib.load()
    small, large, big_x = "tiny-bert", "minilm-2l", 1_048_576 + 256
    inf, nan = float("inf"), float("nan")
    overflows = [None, inf, nan, None, None, None, None]
    cases = [(f"plain {small} max_norm={mn:g} grad_scale={gs:g} norm_out={int(no)}", lambda mn=mn, gs=gs, no=no: plain(lib, small, mn, gs, no))
             for mn, gs, no in ((1.0, 1.0, True), (0.0, 1.0, False), (0.0, 0.25, True), (1.0, 0.25, True))]
    cases.append((f"plain {large} max_norm=1 grad_scale=0.25 norm_out=1", lambda: plain(lib, large, 1.0, 0.25, True)))
    cases += [(f"joint {small} x_n={n} max_norm=1", lambda n=n: joint(lib, small, n, 1.0)) for n in (0, 256, big_x)]
    cases.append((f"joint {small} x_n=256 max_norm=0 norm_out=0", lambda: joint(lib, small, 256, 0.0, False)))
    cases.append((f"joint {large} x_n={big_x} max_norm=1", lambda: joint(lib, large, big_x, 1.0)))
    cases.append((f"sched {small} warmup=2 total=5 steps=6", lambda: sched(lib, small, 2, 5, 6)))
    cases.append((f"sched {small} warmup=0 total=0 steps=3", lambda: sched(lib, small, 0, 0, 3)))
    cases.append((f"sched {large} warmup=2 total=5 steps=3", lambda: sched(lib, large, 2, 5, 3)))
    for total in (0, 5):
        for interval in (2000, 2):
            cases.append((f"amp {small} warmup=2 total={total} interval={interval} good,inf,nan,good*4",
                          lambda total=total, interval=interval: amp(lib, small, 2, total, interval, overflows)))
    cases.append((f"amp {large} warmup=2 total=5 interval=2 good,inf,good,good", lambda: amp(lib, large, 2, 5, 2, [None, inf, None, None])))
    lines = []
    for name, fn in cases:
        c = fn()
        lines.append(f"{name} | norm {c.norm.item():.9g} steps {c.steps.tolist()} scaler {c.scaler.tolist()} | {c.h.hexdigest()}")
        print(lines[-1], file=sys.stderr, flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
