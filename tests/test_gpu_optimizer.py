"""GPU: the optimiser entry points (csrc/optim.hip: qst_clip_adamw_step, _sched, _amp) on an arena their strided loops
need more than one trip for, against a plain fp64 transcription of clip_grad_norm_ + AdamW + zero_grad.

adamw_kernel is launched as <<<2048, 256>>> over float4 (one pass = 2,097,152 arena elements), sumsq_kernel as
<<<1024, 256>>> (1,048,576). The tiny presets the other optimiser tests use end inside the first pass; `minilm-2l` (about
5.3 M elements) takes adamw_kernel through two full trips and a third, partial one, and sumsq_kernel through five and a
partial sixth. Only the optimiser runs here: no forward, no backward.

The reference starts from the same fp32 inputs: parameters, gradients and the hyper-parameters as the C ABI receives them
(`float`, so 0.9, 0.999, 1e-2 ... rounded to fp32), widened to fp64; every operation after that is fp64. The decay mask
comes from config.build_layout's segments. Nothing in it is read back from the library.

Tolerances: parameters rtol 1e-5 / atol 1e-6 and the norm rtol 1e-4 are test_clip_adamw_matches_torch's. A moment is at
most four fp32 operations (2^-24 relative each) from its inputs, one of which is the clip coefficient, which carries the
norm's own error (a sum of 5.3 M squares in a fixed tree: a few 2^-24): once into exp_avg, squared into exp_avg_sq. That
is below 1e-6 either way; the moments are held to rtol 1e-5 (exp_avg) and 2e-5 (exp_avg_sq), plus an atol of 1e-6 of the
tensor's largest reference magnitude for the elements where gg - m cancels. Only real segment elements are compared; the
alignment gaps between segments must stay finite. Every comparison prints its largest error below and above element
2,097,152, so a pass that stops after the first trip is named as such in the failure message.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd.config import PRESETS, build_layout  # noqa: E402
from quadruplet_sentence_transformer_amd.encoder import HipEncoder  # noqa: E402
from quadruplet_sentence_transformer_amd.synthetic import synthetic_params  # noqa: E402

PASS = 2048 * 256 * 4            # arena elements one trip of adamw_kernel (and of the zeroing loop) covers
NORM_PASS = 1024 * 256 * 4       # ... and one trip of sumsq_kernel


def f32(x):
    """x as the C ABI's `float` parameter holds it, widened back to a Python float (fp64)."""
    return float(np.float32(x))


LR, WD, B1, B2, EPS = f32(1e-2), f32(0.01), f32(0.9), f32(0.999), f32(1e-8)


@pytest.fixture(scope="module")
def w():
    """The arena, its layout masks and the conditions on them, once for the file."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    cfg = PRESETS["minilm-2l"]
    segs, total = build_layout(cfg)
    # conditions on the test data: two full trips of adamw_kernel and a third, partial one
    assert total > 2 * PASS and total % PASS != 0
    assert total > 5 * NORM_PASS and total % NORM_PASS != 0
    real, decay = torch.zeros(total, dtype=torch.bool), torch.zeros(total, dtype=torch.bool)
    for s in segs:
        real[s.offset:s.offset + s.numel] = True
        decay[s.offset:s.offset + s.numel] = bool(s.decay)
    # ... and the decay flag of some real element of the later trips differs from the one a wrapped chunk index would read
    for k in (1, 2):
        n = min(PASS, total - k * PASS)
        assert (real[k * PASS:k * PASS + n] & (decay[k * PASS:k * PASS + n] != decay[:n])).any()
    arena = synthetic_params(cfg, seed=3, std=0.05, bias_std=0.02, ln_jitter=0.05)
    return SimpleNamespace(cfg=cfg, total=total, real=real, decay=decay, arena=torch.from_numpy(np.asarray(arena)).clone())


def fresh(w):
    enc = HipEncoder(w.cfg)
    enc.load_arena(w.arena)
    enc.ensure_train_state()
    return enc


def make_grads(w, seed, std):
    """Seeded randn over the whole arena; the stretch only sumsq_kernel's later trips reach and the tail of adamw_kernel's
    partial third trip are scaled up, so a dropped or repeated trip moves the norm by percents."""
    g = torch.randn(w.total, generator=torch.Generator().manual_seed(seed)) * std
    g[NORM_PASS:PASS] *= 2.0
    g[2 * PASS:] *= 3.0
    return g


class Reference:
    """torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW with ST fit()'s two parameter groups, in fp64."""

    def __init__(self, w):
        self.decay = w.decay
        self.p = w.arena.double()
        self.m = torch.zeros(w.total, dtype=torch.float64)
        self.v = torch.zeros(w.total, dtype=torch.float64)

    def step(self, g32, lr, t, max_norm=1.0, grad_scale=1.0):
        """One step at learning rate lr, 1-based step t; returns the pre-clip norm of grad_scale * g."""
        g = g32.double() * grad_scale
        norm = g.norm().item()
        if max_norm > 0:
            g = g * min(1.0, max_norm / (norm + 1e-6))
        self.p = torch.where(self.decay, self.p * (1.0 - lr * WD), self.p)
        self.m = self.m + (1.0 - B1) * (g - self.m)
        self.v = B2 * self.v + (1.0 - B2) * g * g
        denom = self.v.sqrt() / math.sqrt(1.0 - B2 ** t) + EPS
        self.p = self.p - (lr / (1.0 - B1 ** t)) * (self.m / denom)
        return norm


def compare(what, got, ref, w, rtol, atol):
    got = got.detach().cpu()
    assert torch.isfinite(got).all(), f"{what}: not finite (alignment gaps included)"
    err = (got.double() - ref).abs()
    part = err / (atol + rtol * ref.abs())
    err[~w.real] = 0.0
    part[~w.real] = 0.0
    lo_e, hi_e = err[:PASS].max().item(), err[PASS:].max().item()
    lo_p, hi_p = part[:PASS].max().item(), part[PASS:].max().item()
    msg = (f"{what}: max |d| below element {PASS}: {lo_e:.3e} ({lo_p:.3f} of rtol {rtol:.0e} / atol {atol:.1e}), "
           f"at or above it: {hi_e:.3e} ({hi_p:.3f})")
    print("  " + msg)
    assert max(lo_p, hi_p) <= 1.0, f"{msg}; worst element {int(part.argmax())} of {w.total}"


def check_state(tag, enc, ref, w, norm=None):
    """params, exp_avg, exp_avg_sq (and the norm) against the reference; every gradient zeroed."""
    if norm is not None:
        got = enc.grad_norm.item()
        print(f"  {tag} norm: {got:.7g} (reference {norm:.7g}, relative difference {abs(got - norm) / norm:.2e}, rtol 1e-4)")
        np.testing.assert_allclose(got, norm, rtol=1e-4)
    compare(f"{tag} params", enc.params, ref.p, w, 1e-5, 1e-6)
    compare(f"{tag} exp_avg", enc.exp_avg, ref.m, w, 1e-5, 1e-6 * ref.m[w.real].abs().max().item())
    compare(f"{tag} exp_avg_sq", enc.exp_avg_sq, ref.v, w, 2e-5, 1e-6 * ref.v[w.real].abs().max().item())
    assert int(torch.count_nonzero(enc.grads)) == 0, f"{tag}: gradients not zeroed everywhere"


# ------------------------------------------------------------------ 1. qst_clip_adamw_step
def test_clip_adamw_over_three_trips(w):
    """Three steps of qst_clip_adamw_step: the first with gradients of norm ~ 1e4 (the clip scales them down), the others
    with norm ~ 0.4 (the clip leaves them alone)."""
    enc, ref = fresh(w), Reference(w)
    for step in range(3):
        g = make_grads(w, 10 + step, 3.0 if step == 0 else 1e-4)
        enc.grads.copy_(g)
        enc.adamw_step(lr=LR, weight_decay=WD, max_grad_norm=1.0)
        norm = ref.step(g, LR, step + 1)
        assert (norm > 1.0) == (step == 0)                       # a condition on the test data
        check_state(f"step {step + 1}", enc, ref, w, norm)


def test_grad_scale_without_clipping(w):
    """grad_scale = 0.25 (the 1 / world_size of a data-parallel step) with max_grad_norm = 0: the norm reported is
    0.25 * ||g||, and the update takes 0.25 * g as it is although that norm is in the thousands."""
    enc, ref = fresh(w), Reference(w)
    for step in range(2):
        g = make_grads(w, 20 + step, 3.0 if step == 0 else 0.5)
        enc.grads.copy_(g)
        enc.adamw_step(lr=LR, weight_decay=WD, max_grad_norm=0.0, grad_scale=0.25)
        norm = ref.step(g, LR, step + 1, max_norm=0.0, grad_scale=0.25)
        assert norm > 100.0
        np.testing.assert_allclose(norm, 0.25 * g.double().norm().item(), rtol=1e-12)
        check_state(f"step {step + 1}", enc, ref, w, norm)


# ------------------------------------------------------------------ 2. qst_clip_adamw_step_sched
def header_lr(base_lr, t, warmup, total):
    """include/qst.h, qst_clip_adamw_step_sched: the learning rate of step t is get_linear_schedule_with_warmup at t - 1,
    constant base_lr when total_steps <= 0."""
    if total <= 0:
        return base_lr
    k = t - 1
    if k < warmup:
        return base_lr * (k / max(1, warmup))
    return base_lr * max(0.0, (total - k) / max(1, total - warmup))


@pytest.mark.parametrize("warmup,total,start,factors", [
    pytest.param(0, 0, 0, [1, 1, 1], id="constant"),
    pytest.param(0, 5, 0, [1, 4 / 5, 3 / 5], id="no-warmup"),
    pytest.param(1, 5, 0, [0, 1, 3 / 4], id="warmup-1"),
    pytest.param(3, 5, 0, [0, 1 / 3, 2 / 3, 1, 1 / 2, 0, 0], id="past-total"),
    pytest.param(5, 5, 0, [0, 1 / 5, 2 / 5, 3 / 5, 4 / 5, 0, 0], id="warmup-equals-total"),
    pytest.param(0, 2000, 999, [1001 / 2000, 1000 / 2000], id="resume-at-999"),
])
def test_device_side_schedule(w, warmup, total, start, factors):
    """qst_clip_adamw_step_sched: what thread 0 derives on the device -- the step counter and dyn[0..2] = {lr, 1 - beta1^t,
    sqrt(1 - beta2^t)} in the scratch behind the 1024 partial sums -- against the header's rule in fp64 (lr == 0 exactly
    where the rule gives 0, otherwise fp32 rounding: rtol 1e-6), and the step those values drive against the reference.
    `factors` is lr / base_lr per step, written out by hand. A step at lr == 0 leaves the parameters bit-equal and still
    moves the moments. start = 999: the counter starts from enc.opt_step (resume), so the first step is t = 1000."""
    enc, ref = fresh(w), Reference(w)
    enc.opt_step = start
    for i, factor in enumerate(factors):
        t = start + i + 1
        lr = header_lr(LR, t, warmup, total)
        np.testing.assert_allclose(lr, LR * factor, rtol=1e-12, atol=0)
        g = make_grads(w, 30 + i, 3.0 if i == 0 else 1e-4)
        enc.grads.copy_(g)
        before = [x.clone() for x in (enc.params, enc.exp_avg, enc.exp_avg_sq)]
        enc.adamw_step_sched(LR, warmup, total, weight_decay=WD, max_grad_norm=1.0)
        dyn = enc._scratch[1024:1027].cpu().double().numpy()
        want = [lr, 1.0 - B1 ** t, math.sqrt(1.0 - B2 ** t)]
        print(f"  t = {t}: dyn {dyn.tolist()} (rule {want})")
        assert int(enc._step_dev.item()) == t
        if lr == 0.0:
            assert dyn[0] == 0.0
        np.testing.assert_allclose(dyn, want, rtol=1e-6, atol=0)
        norm = ref.step(g, lr, t)
        if lr == 0.0:
            assert torch.equal(enc.params, before[0])
            assert not torch.equal(enc.exp_avg, before[1]) and not torch.equal(enc.exp_avg_sq, before[2])
        check_state(f"t = {t}", enc, ref, w, norm)


# ------------------------------------------------------------------ 3. qst_clip_adamw_step_amp
def test_amp_step_and_overflow_on_the_large_arena(w):
    """qst_clip_adamw_step_amp: one good step under a loss scale of 1024 against the reference on the unscaled gradients,
    then two overflowed steps: a single inf inside adamw_kernel's last, partial trip (sumsq_kernel's sixth), and a single
    nan between elements 1,048,576 and 2,097,152 (sumsq_kernel's second trip). An overflowed step leaves parameters and
    moments bit-equal, zeroes every gradient, halves the scale, and advances neither counter."""
    enc, ref = fresh(w), Reference(w)
    scale = 1024.0
    enc.ensure_amp_scaler(scale)
    g = make_grads(w, 40, 0.01)
    enc.grads.copy_(g * scale)
    enc.adamw_step_amp(LR, 0, 0, weight_decay=WD, max_grad_norm=1.0)
    norm = ref.step(g, LR, 1)
    check_state("good step", enc, ref, w, norm)
    assert enc.amp_scaler.cpu().tolist() == [scale, 1.0, 0.0, 0.0]
    assert enc._step2_dev.cpu().tolist() == [1, 1]
    bad = [(w.total - 300, float("inf")), (NORM_PASS + 451_424, float("nan"))]
    assert bad[0][0] >= 2 * PASS and NORM_PASS < bad[1][0] < PASS and w.real[bad[0][0]] and w.real[bad[1][0]]
    for n, (idx, value) in enumerate(bad, start=1):
        gs = make_grads(w, 40 + n, 0.01) * scale
        gs[idx] = value
        enc.grads.copy_(gs)
        before = [x.clone() for x in (enc.params, enc.exp_avg, enc.exp_avg_sq)]
        enc.adamw_step_amp(LR, 0, 0, weight_decay=WD, max_grad_norm=1.0)
        for x, b in zip((enc.params, enc.exp_avg, enc.exp_avg_sq), before):
            assert torch.equal(x, b)
        left = torch.nonzero(enc.grads).view(-1)
        assert left.numel() == 0, f"{left.numel()} gradients not zeroed, the first at element {int(left[0])}"
        scale *= 0.5
        assert enc.amp_scaler.cpu().tolist() == [scale, 0.0, 1.0, float(n)]
        assert enc._step2_dev.cpu().tolist() == [1, 1]
    compare("after the overflows: params", enc.params, ref.p, w, 1e-5, 1e-6)
