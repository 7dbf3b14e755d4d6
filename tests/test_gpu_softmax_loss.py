"""GPU: losses.SoftmaxLoss and evaluation.LabelAccuracyEvaluator on a real encoder (tiny-bert, D = 64), after the pattern of
tests/test_gpu_mnrl.py sections 4 and 5: the class against torch ops on the same embeddings, its other paths against the
fused one, and fit() training the classifier together with the encoder through the joint optimiser step."""
import csv
import os
import random

import numpy as np
import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import softmax_head_helpers as SH  # noqa: E402
from quadruplet_sentence_transformer_amd import evaluation, st_losses as S  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, SentenceTransformer  # noqa: E402

NOUNS = "cat dog horse bridge river apple street garden window train doctor teacher".split()
VERBS = "sees paints crosses finds leaves follows builds opens".split()


def text(i):
    rng = np.random.RandomState(i)
    return " ".join(f"the {rng.choice(NOUNS)} {rng.choice(VERBS)} a {rng.choice(NOUNS)}" for _ in range(2))


def nli_examples(n, classes=3):
    """Pairs of unrelated sentences with labels 0 .. classes - 1 in turn."""
    return [InputExample(texts=[text(i), text(500 + i)], label=i % classes) for i in range(n)]


def twin_examples(n):
    """Class 0: the second text is the first; class 1: an unrelated second text."""
    return [InputExample(texts=[text(i), text(i) if i % 2 == 0 else text(900 + i)], label=i % 2) for i in range(n)]


class Tap(nn.Module):
    """The model, keeping hold of the sentence embeddings it returns (and of their gradients)."""

    def __init__(self, model):
        super().__init__()
        self.model, self.cfg, self.seen = model, model.cfg, []

    def forward(self, feats):
        out = self.model(feats)
        if out["sentence_embedding"].requires_grad:
            out["sentence_embedding"].retain_grad()
            self.seen.append(out["sentence_embedding"])
        return out


@pytest.fixture(scope="module")
def model():
    return SentenceTransformer("tiny-bert", device="cuda")


def batch_of(model, examples):
    feats, labels = model.smart_batching_collate(examples)
    return [{key: v.cuda() for key, v in f.items()} for f in feats], labels.cuda()


def one_backward(model, lm, feats, labels):
    """(loss, encoder gradients, classifier weight and bias gradients) of one forward + backward from zeroed buffers."""
    enc = model._enc
    enc.ensure_train_state()
    enc.grads.zero_()
    lm.owned_parameters().ensure().zero_grad()
    loss = lm([dict(f) for f in feats], labels)
    loss.backward()
    g = torch.cat([v.reshape(-1) for v in enc.grad_views().values()]).clone()
    gw, gb = lm.classifier.weight.grad.clone(), lm.classifier.bias.grad.clone()
    enc.grads.zero_()
    lm.owned_parameters().zero_grad()
    return loss.detach(), g, gw, gb


def in_buffer(lm):
    op = lm.owned_parameters()
    lo, hi = op.params.data_ptr(), op.params.data_ptr() + 4 * op.total
    return all(lo <= p.data_ptr() < hi for p in lm.classifier.parameters()) and \
        lm.classifier.weight.grad.data_ptr() == op.grads.data_ptr()


# ------------------------------------------------------------------ 1. the class against torch ops
@pytest.mark.parametrize("flags", sorted(SH.ST_FLAGS))
def test_class_equals_torch_ops_on_the_same_embeddings(model, flags):
    rep, diff, mult = SH.ST_FLAGS[flags]
    parts = (SH.REP if rep else 0) | (SH.DIFF if diff else 0) | (SH.MULT if mult else 0)
    feats, labels = batch_of(model, nli_examples(16))
    model.train()
    tap = Tap(model)
    D = model.get_sentence_embedding_dimension()
    torch.manual_seed(3)
    lm = S.SoftmaxLoss(tap, D, 3, rep, diff, mult)
    assert lm.classifier.weight.is_cuda and in_buffer(lm)
    with torch.no_grad():
        lm.classifier.weight.mul_(8.0)                  # logits of order 1: a softmax with something to say
    loss, _, gw, gb = one_backward(model, lm, feats, labels)
    assert len(tap.seen) == 1 and tap.seen[0].shape == (32, D)          # one fused pass
    emb = tap.seen[0]
    u, v = emb.detach()[:16].cpu(), emb.detach()[16:].cpu()
    w, b = lm.classifier.weight.detach().cpu(), lm.classifier.bias.detach().cpu()
    _, ref, (ru, rv, rw, rb) = SH.reference_of(u, v, w, b, labels.cpu(), parts, "mean")
    K = SH.nvec(parts) * D
    ev = SH.value_error(loss, ref, K)
    eg = [SH.grad_error(g.cpu(), r) for g, r in ((emb.grad, torch.cat([ru, rv], 0)), (gw, rw), (gb, rb))]
    print(f"  SoftmaxLoss {flags}: loss {loss.item():.7f} torch ops {ref.item():.7f}; share of the tolerance: value {ev:.3f} "
          f"gradients: embeddings {eg[0]:.3f} weight {eg[1]:.3f} bias {eg[2]:.3f}")
    assert ref.item() > 0.05 and rw.abs().max().item() > 1e-4 and ru.abs().max().item() > 1e-5
    assert ev <= 1.0 and max(eg) <= 1.0
    # labels=None: (reps, logits), as sentence-transformers returns them
    with torch.no_grad():
        reps, logits = lm([dict(f) for f in feats], None)
    assert len(reps) == 2 and reps[0].shape == (16, D) and logits.shape == (16, 3)
    assert SH.value_error(logits, SH.logits_ref(reps[0].cpu().double(), reps[1].cpu().double(), w.double(), b.double(), parts),
                          K) <= 1.0


def test_a_foreign_loss_fct_runs_in_torch_on_the_kernels_logits(model):
    feats, labels = batch_of(model, nli_examples(16))
    model.train()
    D = model.get_sentence_embedding_dimension()
    seen = []

    class Smoothed(nn.CrossEntropyLoss):
        def forward(self, logits, target):
            seen.append((tuple(logits.shape), logits.grad_fn is not None and type(logits.grad_fn).__name__))
            return super().forward(logits, target)

    tap = Tap(model)
    torch.manual_seed(4)
    lm = S.SoftmaxLoss(tap, D, 3, loss_fct=Smoothed(label_smoothing=0.1))
    with torch.no_grad():
        lm.classifier.weight.mul_(8.0)
    loss, _, gw, gb = one_backward(model, lm, feats, labels)
    assert seen == [((16, 3), "_SoftmaxHeadFnBackward")]
    emb = tap.seen[0]
    xs = [t.detach().cpu().double().requires_grad_(True) for t in (emb[:16], emb[16:], lm.classifier.weight, lm.classifier.bias)]
    ref = torch.nn.functional.cross_entropy(SH.logits_ref(*xs, 3), labels.cpu(), label_smoothing=0.1)
    ref.backward()
    assert SH.value_error(loss, ref.detach(), 3 * D) <= 1.0
    for g, r in ((emb.grad, torch.cat([xs[0].grad, xs[1].grad], 0)), (gw, xs[2].grad), (gb, xs[3].grad)):
        assert SH.grad_error(g.cpu(), r) <= 1.0


def test_a_shape_the_kernels_refuse_runs_as_torch_ops_on_the_same_views(model):
    """Nine labels (the kernels take eight): cat -> F.linear -> cross_entropy in torch, gradients into the flat buffer."""
    feats, labels = batch_of(model, nli_examples(18, classes=9))
    model.train()
    D = model.get_sentence_embedding_dimension()
    assert not S.softmax_head_supported(D, 9, 3)
    tap = Tap(model)
    torch.manual_seed(6)
    lm = S.SoftmaxLoss(tap, D, 9)
    with torch.no_grad():
        lm.classifier.weight.mul_(8.0)
    loss, _, gw, gb = one_backward(model, lm, feats, labels)
    assert in_buffer(lm)
    emb = tap.seen[0]
    w, b = lm.classifier.weight.detach().cpu(), lm.classifier.bias.detach().cpu()
    _, ref, (ru, rv, rw, rb) = SH.reference_of(emb.detach()[:18].cpu(), emb.detach()[18:].cpu(), w, b, labels.cpu(), 3, "mean")
    assert SH.value_error(loss, ref, 3 * D) <= 1.0
    for g, r in ((emb.grad, torch.cat([ru, rv], 0)), (gw, rw), (gb, rb)):
        assert SH.grad_error(g.cpu(), r) <= 1.0 and r.abs().max().item() > 1e-5


def test_fused_pass_equals_one_pass_per_column(model):
    feats, labels = batch_of(model, nli_examples(16))
    model.train()
    D = model.get_sentence_embedding_dimension()
    torch.manual_seed(5)
    fused = S.SoftmaxLoss(model, D, 3, fused=True)
    split = S.SoftmaxLoss(model, D, 3, fused=False)
    split.load_state_dict(fused.state_dict())
    assert in_buffer(split)
    l1, g1, w1, b1 = one_backward(model, fused, feats, labels)
    lk, gk, wk, bk = one_backward(model, split, feats, labels)
    assert g1.norm().item() > 0 and w1.norm().item() > 0
    assert abs(lk.item() - l1.item()) < 2e-4
    assert (gk - g1).norm().item() <= 2e-2 * g1.norm().item()
    assert (wk - w1).norm().item() <= 2e-2 * w1.norm().item() and (bk - b1).norm().item() <= 2e-2 * b1.norm().item()


def test_to_and_forward_keep_the_parameters_in_the_flat_buffer(model):
    D = model.get_sentence_embedding_dimension()
    lm = S.SoftmaxLoss(model, D, 3)
    ptrs = [p.data_ptr() for p in lm.classifier.parameters()]
    assert lm.to("cuda") is lm and in_buffer(lm)
    lm.classifier.to(torch.float64)                      # .data is replaced: the parameters leave the buffer ...
    assert not in_buffer(lm)
    feats, labels = batch_of(model, nli_examples(8))
    model.eval()
    with torch.no_grad():
        lm(feats, labels)                                # ... and the next forward brings them back
    assert in_buffer(lm) and [p.data_ptr() for p in lm.classifier.parameters()] == ptrs
    assert lm.classifier.weight.dtype == torch.float32
    assert sorted(k for k in lm.state_dict() if k.startswith("classifier.")) == ["classifier.bias", "classifier.weight"]


# ------------------------------------------------------------------ 2. fit()
def accuracy_in_torch(model, lm, examples):
    model.eval()
    feats, labels = batch_of(model, examples)
    with torch.no_grad():
        _, logits = lm(feats, None)
        loss = lm([dict(f) for f in feats], labels).item()
    return int((logits.argmax(1) == labels).sum()) / len(examples), loss


def test_fit_trains_the_classifier_with_the_encoder(tmp_path):
    """The NLI recipe end to end: SentenceTransformer -> SoftmaxLoss -> fit(evaluator=LabelAccuracyEvaluator, output_path)."""
    random.seed(12)
    torch.manual_seed(12)
    m = SentenceTransformer("tiny-bert", device="cuda")
    pairs = twin_examples(32)
    lm = S.SoftmaxLoss(m, m.get_sentence_embedding_dimension(), 2)
    ev = evaluation.LabelAccuracyEvaluator(DataLoader(pairs, batch_size=12), name="twins", softmax_model=lm)
    w0, b0 = lm.classifier.weight.detach().clone(), lm.classifier.bias.detach().clone()
    p0 = m._enc.params.clone()
    acc_before, loss_before = accuracy_in_torch(m, lm, pairs)
    assert ev(m) == acc_before                           # no output_path: nothing is written
    out = str(tmp_path / "out")
    m.fit([(DataLoader(pairs, shuffle=True, batch_size=8), lm)], evaluator=ev, epochs=5, warmup_steps=0, scheduler="constantlr",
          optimizer_params={"lr": 2e-3}, dropout=0, show_progress_bar=False, output_path=out)
    acc_after, loss_after = accuracy_in_torch(m, lm, pairs)
    print(f"  fit SoftmaxLoss: loss on the 32 pairs {loss_before:.5f} -> {loss_after:.5f}, accuracy {acc_before:.3f} -> {acc_after:.3f}")
    assert np.isfinite(loss_after) and loss_after < loss_before
    w1, b1 = lm.classifier.weight.detach(), lm.classifier.bias.detach()
    assert torch.isfinite(w1).all() and torch.isfinite(b1).all() and torch.isfinite(m._enc.params).all()
    assert (w1 - w0).abs().max().item() > 1e-3 and (b1 - b0).abs().max().item() > 1e-3 and not torch.equal(m._enc.params, p0)
    assert in_buffer(lm) and int(torch.count_nonzero(lm.owned_parameters().grads)) == 0
    assert m._enc.opt_step == 20
    assert acc_after > acc_before
    # the evaluator: one row per epoch, the last one what torch's argmax gives on the same logits
    with open(os.path.join(out, "eval", "accuracy_evaluation_twins_results.csv")) as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["epoch", "steps", "accuracy"] and len(rows) == 6 and [r[0] for r in rows[1:]] == [str(e) for e in range(5)]
    assert float(rows[-1][2]) == acc_after and ev(m) == acc_after
    # save_best_model wrote the encoder; the classifier travels through state_dict()
    assert os.path.isfile(os.path.join(out, "modules.json")) and os.path.isfile(os.path.join(out, "model.safetensors"))
    again = S.SoftmaxLoss(m, m.get_sentence_embedding_dimension(), 2)
    again.load_state_dict(lm.state_dict())
    assert accuracy_in_torch(m, again, pairs)[0] == acc_after


def test_two_objectives_step_the_classifier_only_on_its_own_steps():
    random.seed(13)
    torch.manual_seed(13)
    m = SentenceTransformer("tiny-bert", device="cuda")
    lm = S.SoftmaxLoss(m, m.get_sentence_embedding_dimension(), 2)
    cos = S.CosineSimilarityLoss(m)
    graded = [InputExample(texts=[text(i), text(700 + i)], label=float(i % 5) / 4.0) for i in range(16)]
    steps, plain = [], m._enc.adamw_step

    def spy(*args, **kwargs):
        before = lm.owned_parameters().params.clone()
        arena = m._enc.params.clone()
        plain(*args, **kwargs)
        steps.append((kwargs.get("extra"), not torch.equal(before, lm.owned_parameters().params),
                      not torch.equal(arena, m._enc.params)))

    m._enc.adamw_step = spy
    m.fit([(DataLoader(twin_examples(16), batch_size=8), lm), (DataLoader(graded, batch_size=8), cos)], epochs=1, warmup_steps=0,
          scheduler="constantlr", optimizer_params={"lr": 1e-3}, dropout=0, show_progress_bar=False)
    op = lm.owned_parameters()
    # two steps per objective, in turn: the classifier's with its parameters, the cosine loss's on the call fit() always made
    assert [s[0] for s in steps] == [op, None, op, None]
    assert [s[1] for s in steps] == [True, False, True, False] and all(s[2] for s in steps)
    assert m._enc.opt_step == 4 and torch.isfinite(op.params).all()


@pytest.mark.parametrize("kwargs,why", [({"use_amp": True}, "use_amp"), ({"precision": "f16w"}, "f16w"),
                                        ({"resume_from_checkpoint": "/nonexistent/checkpoint"}, "resume_from_checkpoint"),
                                        ({}, "world of 2")])
def test_what_has_no_joint_step_is_refused_before_anything_changes(model, kwargs, why, monkeypatch):
    if not kwargs:          # a process group of two ranks, as far as fit() asks before it refuses: nothing is exchanged
        import torch.distributed as dist
        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
        monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    lm = S.SoftmaxLoss(model, model.get_sentence_embedding_dimension(), 2)
    p0, x0 = model._enc.params.clone(), lm.owned_parameters().params.clone()
    step0 = model._enc.opt_step
    with pytest.raises(NotImplementedError, match=f"SoftmaxLoss.*{why}"):
        model.fit([(DataLoader(twin_examples(8), batch_size=4), lm)], epochs=1, warmup_steps=0, scheduler="constantlr",
                  dropout=0, show_progress_bar=False, **kwargs)
    assert torch.equal(model._enc.params, p0) and torch.equal(lm.owned_parameters().params, x0)
    assert model._enc.opt_step == step0 and model.training_precision == "bf16" and model._dp is None
    # ... and a loss without parameters of its own still takes these paths (resume: up to the missing directory)
    if "resume_from_checkpoint" in kwargs:
        with pytest.raises(FileNotFoundError):
            model.fit([(DataLoader(twin_examples(8), batch_size=4), S.CosineSimilarityLoss(model))], epochs=1,
                      show_progress_bar=False, **kwargs)
