"""HipEncoder's table of precisions (encoder.py _PRECISIONS, one live record per created precision): what exists when, what a
parameter change makes stale, what a refresh clears, and what a handle created late inherits.

One config and one shape serve the whole file: MiniLM layer dimensions on 2 layers and a 4,096-word vocabulary (all five
precisions run it: H and I are multiples of 128), nseq = 4 sequences of L = 32 tokens with ragged lengths, dropout off unless a
test is about it.

Equality. An inference or training forward has no atomics: test_forwards_repeat_bit_for_bit settles that two forwards of one
encoder are bit-identical in every precision at this shape, and the embedding comparisons below are torch.equal. The BACKWARD
flushes its weight gradients with fp32 atomics (tools/determinism_check.py), so gradients of two runs of one path differ in
summation order: they are compared as tests/test_gpu_fp8mx.py compares the fp8 backward with itself (staged against one call),
relative L2 distance below 1e-5.
"""
from dataclasses import replace

import pytest
import torch

from kernel_helpers import quad_batch
from quadruplet_sentence_transformer_amd.config import PRESETS
from quadruplet_sentence_transformer_amd.encoder import HipEncoder
from quadruplet_sentence_transformer_amd.synthetic import synthetic_params, synthetic_quadruplets
from quadruplet_sentence_transformer_amd.trainer import QuadrupletTrainer

pytestmark = pytest.mark.gpu

CFG = replace(PRESETS["all-MiniLM-L6-v2"], num_layers=2, vocab_size=4096)
NSEQ, L = 4, 32
PRECISIONS = ("bf16", "bf16x3", "fp8", "f16", "f16w")
ALIASES = {"bf16": (0, None), "bf16x3": (1,), "fp8": (3,), "f16": ("fp16", 4), "f16w": (5,)}
WKW = dict(std=0.03, bias_std=0.02, ln_jitter=0.05)
# a step this long moves every weight by a third of its spread (Adam: |update| = lr for the first step): no precision's
# rounding hides it, the fp8 codes (3 mantissa bits) included
LR = 1e-2


@pytest.fixture(scope="module")
def arena():
    return synthetic_params(CFG, seed=14, **WKW)


@pytest.fixture(scope="module")
def quads():
    """ids / mask / type ids [4, 1, L] on the device: the trainer's batch; batch(quads) is the encoder's [4, L] view of it."""
    return [torch.from_numpy(x).cuda() for x in synthetic_quadruplets(CFG, NSEQ // 4, L, seed=14, ragged=True)]


def batch(quads):
    return quad_batch(CFG, *quads, NSEQ // 4, L)


def encoder(params):
    """A new encoder on a copy of `params` (a numpy arena or a device tensor)."""
    enc = HipEncoder(CFG)
    enc.load_arena(params.clone() if torch.is_tensor(params) else params)
    return enc


def created(enc):
    return set(enc._live)


def embed(enc, quads, precisions=PRECISIONS, training=False):
    return {p: enc.forward(*batch(quads), training=training, precision=p)[0] for p in precisions}


def random_grads(enc, scale=1.0):
    enc.ensure_train_state()
    enc.grads.copy_(torch.randn(enc.total, generator=torch.Generator().manual_seed(5)) * scale)


# every way the parameters change: (enc, another arena) -> None
CHANGES = {
    "load_arena": lambda enc, other: enc.load_arena(other),
    "adamw_step": lambda enc, other: (random_grads(enc), enc.adamw_step(LR)),
    "adamw_step_sched": lambda enc, other: (random_grads(enc), enc.adamw_step_sched(LR, 0, 0)),
    # (the gradients of the amp step carry the loss scale)
    "adamw_step_amp": lambda enc, other: (random_grads(enc, 65536.0), enc.adamw_step_amp(LR, 0, 0)),
}


@pytest.fixture(scope="module")
def other(arena):
    return synthetic_params(CFG, seed=15, **WKW)


def test_forwards_repeat_bit_for_bit(arena, quads):
    enc = encoder(arena)
    for training in (False, True):
        a, b = embed(enc, quads, training=training), embed(enc, quads, training=training)
        for p in PRECISIONS:
            assert torch.isfinite(a[p]).all() and torch.equal(a[p], b[p]), (p, training)
    assert quads[1].sum(-1).unique().numel() > 1                  # (ragged lengths)


def test_precisions_are_created_on_first_use(arena, quads):
    enc = encoder(arena)
    assert created(enc) == {"bf16"}
    enc.shadow_mx_stale = True                                    # a flag of a precision that does not exist: nothing appears
    enc.shadow_f16_stale = False
    assert created(enc) == {"bf16"} and enc.shadow_mx_stale and enc.shadow_f16_stale
    for p in PRECISIONS:
        e = encoder(arena)
        e.forward(*batch(quads), precision=p)
        assert created(e) == {"bf16", p}
    for p, aliases in ALIASES.items():
        rec = enc._record(p)
        assert rec.spec.name == p and enc._handle_for(p) is rec.handle
        for a in aliases:
            assert enc._record(a) is rec
    assert created(enc) == set(PRECISIONS) and enc.handle is enc._record("bf16").handle
    for bad in ("fp16w", "bf8", 2, 6, [0]):
        with pytest.raises(ValueError, match="unknown precision"):
            enc._handle_for(bad)
        with pytest.raises(ValueError, match="unknown precision"):
            enc.forward(*batch(quads), precision=bad)


@pytest.mark.parametrize("change", list(CHANGES))
def test_a_parameter_change_makes_every_created_precision_stale(change, arena, other, quads):
    enc = encoder(arena)
    emb0 = embed(enc, quads)
    assert not any((enc.shadow_stale, enc.shadow_mx_stale, enc.shadow_f16_stale, enc.shadow_f16w_stale))
    CHANGES[change](enc, other)
    assert all((enc.shadow_stale, enc.shadow_mx_stale, enc.shadow_f16_stale, enc.shadow_f16w_stale))
    emb, ref = embed(enc, quads), embed(encoder(enc.params), quads)
    for p in PRECISIONS:
        moved = (emb[p] - emb0[p]).abs().max().item()
        print(f"[{change}] {p}: max|emb - emb before| {moved:.3e}, equal to a fresh encoder's: {torch.equal(emb[p], ref[p])}")
        assert torch.equal(emb[p], ref[p]), p
        assert moved > 1e-3, p                                    # (unit-norm embeddings of 384 entries)


def test_a_refresh_clears_its_own_flag_only(arena, other, quads):
    enc = encoder(arena)
    embed(enc, quads)
    enc.load_arena(other)
    embed(enc, quads, ("f16",))
    assert enc.shadow_stale and enc.shadow_mx_stale and enc.shadow_f16w_stale and not enc.shadow_f16_stale
    enc.mark_stale(keep="fp16")
    assert enc.shadow_stale and enc.shadow_mx_stale and enc.shadow_f16w_stale and not enc.shadow_f16_stale
    enc.mark_stale()
    assert enc.shadow_f16_stale


def test_fp8_training_refreshes_the_bf16_shadow_of_its_backward(arena, other, quads):
    def step(enc):
        emb, _, saved = enc.forward(*batch(quads), training=True, precision="fp8")
        enc.ensure_train_state()
        enc.grads.zero_()
        enc.backward(*batch(quads), torch.randn(emb.shape, generator=torch.Generator().manual_seed(3)).cuda(), saved,
                     precision="fp8")
        return emb, enc.grads.clone()
    enc = encoder(arena)
    step(enc)                                                     # both shadows filled from the first arena
    enc.load_arena(other)
    assert enc.shadow_stale and enc.shadow_mx_stale
    emb, grads = step(enc)
    assert not enc.shadow_stale and not enc.shadow_mx_stale
    ref_emb, ref_grads = step(encoder(other))
    d = float((grads - ref_grads).norm() / ref_grads.norm())
    print(f"[fp8 training after a parameter change] gradients: relative L2 distance to a fresh encoder's {d:.3e}")
    assert torch.equal(emb, ref_emb) and d < 1e-5


@pytest.mark.parametrize("train,read", [("bf16", "fp8"), ("f16", "bf16"), ("f16w", "bf16")])
def test_a_replayed_step_leaves_the_other_precisions_stale(train, read, arena, quads):
    """A graph-captured trainer at precision `train` and, between its steps, inference forwards at `read` on the same encoder:
    a forward, two steps (the first captures, the second replays), a forward (which refreshes the shadow of `read`), one more
    replayed step, a forward. The replay changed the parameters, so the last forward equals that of a fresh encoder holding
    them. ("bf16", "fp8") is the case the hand-written flags after a replay forgot: it read an MXFP8 shadow of the weights
    before the last step.)"""
    tr = QuadrupletTrainer(CFG, arena=arena, device="cuda:0", lr=LR, use_graph=True, precision=train)
    enc = tr.enc
    embed(enc, quads, (read,))
    tr.step(*quads)
    tr.step(*quads)
    before = embed(enc, quads, (read,))[read]
    p0 = enc.params.clone()
    tr.step(*quads)
    assert len(tr._graphs) == 1 and not torch.equal(enc.params, p0)          # (a replay, and it trained)
    emb = embed(enc, quads, (read,))[read]
    ref = embed(encoder(enc.params), quads, (read,))[read]
    print(f"[replay {train} -> {read}] max|emb - fresh encoder's| {(emb - ref).abs().max().item():.3e}, "
          f"max|emb - emb before the step| {(emb - before).abs().max().item():.3e}")
    assert torch.equal(emb, ref)
    assert not torch.equal(emb, before)


def test_a_handle_created_late_inherits_dropout_and_ln_fusion(arena, quads):
    enc = encoder(arena)
    enc.set_dropout(0.1, 0.1, 11)
    enc.set_ln_fusion(2)
    assert created(enc) == {"bf16"}
    t1, t2 = [embed(enc, quads, ("f16",), training=True)["f16"] for _ in range(2)]
    i1, i2 = [embed(enc, quads, ("f16",))["f16"] for _ in range(2)]
    assert enc.dropout_step == 2 and not torch.equal(t1, t2) and not torch.equal(t1, i1)      # the f16 handle drops
    assert torch.equal(i1, i2)
    # set_ln_fusion before the f16 handle exists gives what set_ln_fusion on the existing handle gives; forced fusion and
    # none agree as in tests/test_gpu_encoder.py (f16 operands: 1e-4 of the largest embedding entry)
    out = {}
    for mode in (1, 2):
        late, early = encoder(arena), encoder(arena)
        late.set_ln_fusion(mode)
        early._handle_for("f16")
        early.set_ln_fusion(mode)
        out[mode] = embed(late, quads, ("f16",), training=True)["f16"]
        assert torch.equal(out[mode], embed(early, quads, ("f16",), training=True)["f16"]), mode
    sc, de = out[2].abs().max().item(), (out[1] - out[2]).abs().max().item()
    print(f"[ln-fusion before creation] f16: max|d emb| {de:.2e} of {sc:.2e}")
    assert de <= 1e-4 * sc


def test_the_stale_flags_stay_assignable_by_name(arena, quads):
    """What a caller that restores parameters behind the encoder's back writes (bench.py does): three of the four flags. It
    runs whether or not the precisions exist, means each precision alone and leaves the fourth flag as it was."""
    e = encoder(arena)
    e.shadow_stale = e.shadow_mx_stale = e.shadow_f16_stale = True
    assert created(e) == {"bf16"} and e.shadow_stale and e.shadow_f16w_stale
    embed(e, quads)
    assert not any((e.shadow_stale, e.shadow_mx_stale, e.shadow_f16_stale, e.shadow_f16w_stale))
    e.shadow_stale = e.shadow_mx_stale = e.shadow_f16_stale = True
    assert e.shadow_stale and e.shadow_mx_stale and e.shadow_f16_stale and not e.shadow_f16w_stale
    e.shadow_mx_stale = False
    assert e.shadow_stale and not e.shadow_mx_stale and e.shadow_f16_stale and not e.shadow_f16w_stale
