"""GPU: qst_clip_adamw_step_joint (csrc/optim.hip) -- the optimiser step over the encoder's arena and a second flat buffer a
loss owns (loss_params.LossParameters), clipped on the norm of both.

The reference is torch itself in fp64 on the CPU: torch.nn.utils.clip_grad_norm_ over all parameters, then torch.optim.AdamW
with sentence-transformers' two groups (the arena's decay and no-decay elements, plus the extra group's `weight` with decay
and its `bias` without). Tolerances are those tests/test_gpu_optimizer.py states: parameters rtol 1e-5 / atol 1e-6, exp_avg
rtol 1e-5, exp_avg_sq rtol 2e-5 (each with an atol of 1e-6 of the tensor's largest reference magnitude), norm rtol 1e-4.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from kernel_helpers import lib, ptr, stream  # noqa: E402,F401
from quadruplet_sentence_transformer_amd.config import PRESETS, build_layout  # noqa: E402
from quadruplet_sentence_transformer_amd.encoder import HipEncoder  # noqa: E402
from quadruplet_sentence_transformer_amd.loss_params import LossParameters  # noqa: E402
from quadruplet_sentence_transformer_amd.synthetic import synthetic_params  # noqa: E402


def f32(x):
    return float(np.float32(x))


LR, WD, B1, B2, EPS = f32(1e-2), f32(0.01), f32(0.9), f32(0.999), f32(1e-8)


@pytest.fixture(scope="module")
def w():
    cfg = PRESETS["tiny-bert"]
    segs, total = build_layout(cfg)
    real, decay = torch.zeros(total, dtype=torch.bool), torch.zeros(total, dtype=torch.bool)
    for s in segs:
        real[s.offset:s.offset + s.numel] = True
        decay[s.offset:s.offset + s.numel] = bool(s.decay)
    arena = synthetic_params(cfg, seed=3, std=0.05, bias_std=0.02, ln_jitter=0.05)
    return SimpleNamespace(cfg=cfg, total=total, real=real, decay=decay, arena=torch.from_numpy(np.asarray(arena)).clone())


def fresh(w):
    enc = HipEncoder(w.cfg)
    enc.load_arena(w.arena)
    enc.ensure_train_state()
    return enc


def head(seed=5):
    """The extra group: a 3 x 192 weight and 3 biases, padded to 768 + 256 elements."""
    torch.manual_seed(seed)
    lin = torch.nn.Linear(192, 3)
    op = LossParameters(lin, device="cuda")
    assert op.total == 1024 and [(n, o) for n, o, *_ in op.layout] == [("weight", 0), ("bias", 768)]
    return lin, op


def arena_grads(w, seed, std):
    """Seeded randn on the real elements of the arena; the alignment gaps between segments stay zero, as a backward leaves them."""
    g = torch.randn(w.total, generator=torch.Generator().manual_seed(seed)) * std
    g[~w.real] = 0.0
    return g


def joint(lib, enc, x, step, max_norm=1.0, grad_scale=1.0, x_n=None, lr=LR):
    """The raw call; x = (params, grads, exp_avg, exp_avg_sq, chunk_decay) of the extra group or Nones."""
    n = x_n if x_n is not None else (0 if x[0] is None else x[0].numel())
    return lib.qst_clip_adamw_step_joint(enc.handle, ptr(enc.params), ptr(enc.grads), ptr(enc.exp_avg), ptr(enc.exp_avg_sq),
                                         *[ptr(t) for t in x], n, lr, B1, B2, EPS, WD, max_norm, grad_scale, step,
                                         ptr(enc.grad_norm), ptr(enc._scratch), stream())


# ------------------------------------------------------------------ 1. x_n = 0
@pytest.mark.parametrize("max_norm", [1.0, 0.0])
def test_without_an_extra_group_the_bits_are_those_of_the_plain_step(lib, w, max_norm):
    a, b = fresh(w), fresh(w)
    for step in (1, 2):
        g = arena_grads(w, 30 + step, 3.0 if step == 1 else 1e-4)
        a.grads.copy_(g)
        b.grads.copy_(g)
        a.adamw_step(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, max_grad_norm=max_norm, grad_scale=0.5)
        assert joint(lib, b, [None] * 5, step, max_norm, 0.5) == 0
        for k in ("params", "exp_avg", "exp_avg_sq", "grads", "grad_norm"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert a.grad_norm.item() > 0


# ------------------------------------------------------------------ 2. against torch
def torch_reference(w, lin):
    """fp64 CPU parameters: the arena as two tensors (decay / no decay elements), the head's weight and bias."""
    ps = SimpleNamespace(
        dec=torch.nn.Parameter(w.arena[w.decay].double()), nod=torch.nn.Parameter(w.arena[w.real & ~w.decay].double()),
        weight=torch.nn.Parameter(lin.weight.detach().cpu().double().clone()),
        bias=torch.nn.Parameter(lin.bias.detach().cpu().double().clone()))
    opt = torch.optim.AdamW([{"params": [ps.dec, ps.weight], "weight_decay": WD}, {"params": [ps.nod, ps.bias], "weight_decay": 0.0}],
                            lr=LR, betas=(B1, B2), eps=EPS)
    return ps, opt


def close(what, got, ref, rtol, atol):
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().double().reshape(-1)
    part = ((got - ref).abs() / (atol + rtol * ref.abs())).max().item()
    print(f"  {what}: {part:.3f} of rtol {rtol:.0e} / atol {atol:.1e}")
    assert part <= 1.0, what


def test_three_clipped_steps_match_torch_adamw(lib, w):
    enc = fresh(w)
    lin, op = head()
    ps, opt = torch_reference(w, lin)
    nod = w.real & ~w.decay
    for step in (1, 2, 3):
        g = arena_grads(w, 40 + step, 0.02)
        gx = {"weight": torch.randn(3, 192, generator=torch.Generator().manual_seed(50 + step)) * 0.5,
              "bias": torch.randn(3, generator=torch.Generator().manual_seed(60 + step)) * 0.5}
        enc.grads.copy_(g)
        lin.weight.grad.copy_(gx["weight"])                 # through the views autograd accumulates into
        lin.bias.grad.copy_(gx["bias"])
        enc.adamw_step(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, max_grad_norm=0.25, extra=op)
        ps.dec.grad, ps.nod.grad = g[w.decay].double(), g[nod].double()
        ps.weight.grad, ps.bias.grad = gx["weight"].double(), gx["bias"].double()
        norm = torch.nn.utils.clip_grad_norm_([ps.dec, ps.nod, ps.weight, ps.bias], 0.25).item()
        opt.step()
        assert norm > 0.25                                  # a condition on the test data: every step is clipped
        want = float(np.sqrt(g.double().pow(2).sum().item() + sum(t.double().pow(2).sum().item() for t in gx.values())))
        np.testing.assert_allclose(norm, want, rtol=1e-12)
        assert want > 1.05 * g.double().norm().item()       # ... and the extra group is a visible share of the norm
        print(f"  step {step}: norm {enc.grad_norm.item():.7g}, sqrt(|arena g|^2 + |extra g|^2) = {want:.7g}")
        np.testing.assert_allclose(enc.grad_norm.item(), want, rtol=1e-4)
        st = {k: opt.state[getattr(ps, k)] for k in ("dec", "nod", "weight", "bias")}
        for name, mask in (("dec", w.decay), ("nod", nod)):
            close(f"step {step} arena {name} params", enc.params.cpu()[mask], getattr(ps, name), 1e-5, 1e-6)
            m, v = st[name]["exp_avg"], st[name]["exp_avg_sq"]
            close(f"step {step} arena {name} exp_avg", enc.exp_avg.cpu()[mask], m, 1e-5, 1e-6 * m.abs().max().item())
            close(f"step {step} arena {name} exp_avg_sq", enc.exp_avg_sq.cpu()[mask], v, 2e-5, 1e-6 * v.abs().max().item())
        for name in ("weight", "bias"):
            _, off, n, shape, _ = next(e for e in op.layout if e[0] == name)
            close(f"step {step} extra {name} params", getattr(lin, name), getattr(ps, name), 1e-5, 1e-6)
            m, v = st[name]["exp_avg"], st[name]["exp_avg_sq"]
            close(f"step {step} extra {name} exp_avg", op.exp_avg[off:off + n], m, 1e-5, 1e-6 * m.abs().max().item())
            close(f"step {step} extra {name} exp_avg_sq", op.exp_avg_sq[off:off + n], v, 2e-5, 1e-6 * v.abs().max().item())
        # zero_grad on both buffers, and the padding of the extra group is still zero everywhere
        assert int(torch.count_nonzero(enc.grads)) == 0 and int(torch.count_nonzero(op.grads)) == 0
        for buf in (op.params, op.exp_avg, op.exp_avg_sq):
            assert int(torch.count_nonzero(buf[576:768])) == 0 and int(torch.count_nonzero(buf[771:])) == 0
        # the parameters are still the views: the step wrote where the module reads
        assert lin.weight.data_ptr() == op.params.data_ptr() and lin.bias.data_ptr() == op.params.data_ptr() + 4 * 768
    assert enc.opt_step == 3
    # weight decays, bias does not: with zero gradients and fresh moments a step only shrinks the weight
    lin2, op2 = head(6)
    before_w, before_b = lin2.weight.detach().clone(), lin2.bias.detach().clone()
    enc2 = fresh(w)
    enc2.adamw_step(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, max_grad_norm=1.0, extra=op2)
    torch.testing.assert_close(lin2.weight.detach(), before_w * f32(1.0 - LR * WD), rtol=1e-6, atol=0)
    assert torch.equal(lin2.bias.detach(), before_b)


def test_norm_without_clipping_and_with_grad_scale(lib, w):
    enc = fresh(w)
    lin, op = head()
    op.ensure_state()
    g = arena_grads(w, 70, 0.01)
    enc.grads.copy_(g)
    op.grads[:576].normal_().mul_(3.0)
    gx = op.grads.cpu().double()
    want = 0.25 * float(np.sqrt(g.double().pow(2).sum().item() + gx.pow(2).sum().item()))
    assert joint(lib, enc, [op.params, op.grads, op.exp_avg, op.exp_avg_sq, op.chunk_decay], 1, 0.0, 0.25) == 0
    np.testing.assert_allclose(enc.grad_norm.item(), want, rtol=1e-4)
    assert gx.norm().item() > 10 * g.double().norm().item()          # the extra group dominates this norm
    assert int(torch.count_nonzero(op.grads)) == 0 and int(torch.count_nonzero(enc.grads)) == 0


# ------------------------------------------------------------------ 3. arguments
def test_bad_arguments_are_refused_and_nothing_moves(lib, w):
    enc = fresh(w)
    lin, op = head()
    op.ensure_state()
    enc.grads.fill_(0.5)
    op.grads.fill_(0.5)
    x = [op.params, op.grads, op.exp_avg, op.exp_avg_sq, op.chunk_decay]
    keep = [t.clone() for t in (enc.params, enc.grads, op.params, op.grads)]
    assert joint(lib, enc, x, 1, x_n=1000) == -1                     # not a multiple of 256
    assert joint(lib, enc, x, 1, x_n=-256) == -1
    for i in range(5):
        assert joint(lib, enc, [None if j == i else t for j, t in enumerate(x)], 1, x_n=1024) == -1
    assert joint(lib, enc, x, 0) == -1                               # the step is 1-based
    assert lib.qst_clip_adamw_step_joint(None, ptr(enc.params), ptr(enc.grads), ptr(enc.exp_avg), ptr(enc.exp_avg_sq),
                                         *[ptr(t) for t in x], 1024, LR, B1, B2, EPS, WD, 1.0, 1.0, 1, ptr(enc.grad_norm),
                                         ptr(enc._scratch), stream()) == -1
    torch.cuda.synchronize()
    for t, k in zip((enc.params, enc.grads, op.params, op.grads), keep):
        assert torch.equal(t, k)
    # HipEncoder.adamw_step refuses an extra group on another device
    cpu_op = LossParameters(torch.nn.Linear(4, 2))
    with pytest.raises(Exception, match="live on cpu"):
        enc.adamw_step(lr=LR, extra=cpu_op)
