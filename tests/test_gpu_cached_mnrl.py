"""GPU: CachedMultipleNegativesRankingLoss and its symmetric form (GradCache) on a real encoder -- tiny-bert, 16 examples,
as section 4 of test_gpu_mnrl.py: the three steps give the loss and the arena gradients of the uncached loss, the replay
sees the first pass's embeddings bit for bit (dropout masks and precision included) and leaves the dropout counter where
the first pass left it, and fit() trains through it."""
import random

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import dense_head_helpers as DH  # noqa: E402
import mnrl_helpers as M  # noqa: E402
from quadruplet_sentence_transformer_amd import data, st_losses as S, util  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, SentenceTransformer  # noqa: E402

PAIRS = [(S.CachedMultipleNegativesRankingLoss, S.MultipleNegativesRankingLoss),
         (S.CachedMultipleNegativesSymmetricRankingLoss, S.MultipleNegativesSymmetricRankingLoss)]
IDS = ["plain", "symmetric"]
WORDS = "a man rides red horse two dogs play in park woman eats green apple near old bridge small cat sleeps".split()


def sent(i, n):
    rng = np.random.RandomState(i)
    return " ".join(rng.choice(WORDS, size=n))


def mnrl_examples(n, k):
    """(anchor, positive that shares the anchor's words[, an unrelated hard negative])."""
    return [InputExample(texts=[sent(i, 9), sent(i, 9) + " now", sent(1000 + i, 5 + i % 7)][:k]) for i in range(n)]


class Tap(nn.Module):
    """The model, keeping hold of the sentence embeddings it returns and of whether autograd was on."""

    def __init__(self, model):
        super().__init__()
        self.model, self.cfg, self.seen = model, model.cfg, []

    def forward(self, feats):
        out = self.model(feats)
        self.seen.append((torch.is_grad_enabled(), out["sentence_embedding"].detach().clone()))
        return out


@pytest.fixture(scope="module")
def model():
    return SentenceTransformer("tiny-bert", device="cuda")


def batch_of(model, k):
    feats, labels = model.smart_batching_collate(mnrl_examples(16, k))
    return [{key: v.cuda() for key, v in f.items()} for f in feats], labels.cuda()


def one_backward(model, lm, feats, labels):
    enc = model._enc
    enc.ensure_train_state()
    enc.grads.zero_()
    loss = lm([dict(f) for f in feats], labels)
    loss.backward()
    g = torch.cat([v.reshape(-1) for v in enc.grad_views().values()]).clone()
    enc.grads.zero_()
    return loss.detach(), g


def close(l1, g1, l2, g2, what):
    dl, dg, ng = abs(l1.item() - l2.item()), (g1 - g2).norm().item(), g2.norm().item()
    print(f"  {what}: loss {l1.item():.6f} against {l2.item():.6f} (|diff| {dl:.2e}); gradients |diff| {dg:.3e} of |g| {ng:.3e}")
    assert ng > 0
    assert dl < 2e-4
    assert dg <= 2e-2 * ng


# ------------------------------------------------------------------ 1. the cached loss is the uncached loss
@pytest.mark.parametrize("mini", [4, 5, 16, 64])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("cached,plain", PAIRS, ids=IDS)
def test_equals_the_uncached_loss(model, cached, plain, k, mini):
    """Dropout off: the same rows through differently shaped passes, the bounds of
    test_class_fused_pass_equals_one_pass_per_column."""
    feats, labels = batch_of(model, k)
    model.train()
    assert model._enc.dropout is None
    want_l, want_g = one_backward(model, plain(model), feats, labels)
    got_l, got_g = one_backward(model, cached(model, mini_batch_size=mini), feats, labels)
    close(got_l, got_g, want_l, want_g, f"{cached.__name__} k={k} mini_batch_size={mini}")


@pytest.mark.parametrize("cached,plain", PAIRS, ids=IDS)
def test_one_pass_per_column_and_dot_score(model, cached, plain):
    feats, labels = batch_of(model, 3)
    model.train()
    want_l, want_g = one_backward(model, plain(model, scale=1.0, similarity_fct=util.dot_score), feats, labels)
    got_l, got_g = one_backward(model, cached(model, scale=1.0, similarity_fct=util.dot_score, mini_batch_size=5, fused=False),
                                feats, labels)
    close(got_l, got_g, want_l, want_g, f"{cached.__name__} dot_score, fused=False")


# ------------------------------------------------------------------ 2. the replay
@pytest.mark.parametrize("fused", [True, False])
def test_replay_is_exact_and_leaves_the_counter_where_the_first_pass_left_it(model, fused):
    feats, labels = batch_of(model, 2)
    model.train()
    enc = model._enc
    try:
        enc.set_dropout(0.1, 0.1, 123)
        enc.set_dropout_step(7)
        tap = Tap(model)
        lm = S.CachedMultipleNegativesRankingLoss(tap, mini_batch_size=4, fused=fused)
        enc.ensure_train_state()
        enc.grads.zero_()
        loss = lm([dict(f) for f in feats], labels)
        passes = 4 * (1 if fused else 2)
        assert len(tap.seen) == passes and not any(grad for grad, _ in tap.seen)
        after_first = enc.dropout_step
        assert after_first == 7 + passes
        loss.backward()
        torch.cuda.synchronize()
        assert len(tap.seen) == 2 * passes and all(grad for grad, _ in tap.seen[passes:])
        for (_, first), (_, second) in zip(tap.seen[:passes], tap.seen[passes:]):
            assert first.shape[0] == (8 if fused else 4) and torch.equal(first, second)
        # the masks differ from mini-batch to mini-batch, and dropout is really on
        assert not torch.equal(tap.seen[0][1], tap.seen[1][1])
        assert enc.dropout_step == after_first and int(enc.drop_state[2].item()) == after_first
        assert enc.grads.abs().max().item() > 0
    finally:
        enc.set_dropout(0.0, 0.0)
        enc.grads.zero_()


@pytest.mark.parametrize("cached,plain", PAIRS, ids=IDS)
def test_one_mini_batch_has_the_masks_of_one_pass(model, cached, plain):
    """Dropout on, one mini-batch: plain MNRL started at the same dropout_step drops at the same places. Wrong masks miss by
    O(1)."""
    feats, labels = batch_of(model, 2)
    model.train()
    enc = model._enc
    try:
        enc.set_dropout(0.1, 0.1, 321)
        enc.set_dropout_step(3)
        want_l, want_g = one_backward(model, plain(model), feats, labels)
        enc.set_dropout_step(3)
        got_l, got_g = one_backward(model, cached(model, mini_batch_size=16), feats, labels)
        close(got_l, got_g, want_l, want_g, f"{cached.__name__} with dropout, one mini-batch")
        # the comparison has teeth: another step's masks are far outside the bounds
        enc.set_dropout_step(4)
        other_l, other_g = one_backward(model, plain(model), feats, labels)
        assert (other_g - want_g).norm().item() > 2e-2 * want_g.norm().item()
    finally:
        enc.set_dropout(0.0, 0.0)


def test_first_pass_runs_at_the_training_precision_and_the_switch_is_off_by_default(model):
    feats, labels = batch_of(model, 2)
    model.train()
    enc = model._enc
    try:
        model.training_precision = "f16"
        enc.set_dropout(0.1, 0.1, 55)
        tap = Tap(model)
        lm = S.CachedMultipleNegativesRankingLoss(tap, mini_batch_size=8)
        enc.ensure_train_state()
        lm([dict(f) for f in feats], labels).backward()
        torch.cuda.synchronize()
        assert [g for g, _ in tap.seen] == [False, False, True, True]
        assert torch.equal(tap.seen[0][1], tap.seen[2][1]) and torch.equal(tap.seen[1][1], tap.seen[3][1])
        assert model._no_grad_training_precision is False                 # the switch went back
        # without the switch a no-grad train()-mode call still runs "bf16"
        col = {k: v.clone() for k, v in feats[0].items()}
        enc.set_dropout_step(11)
        with torch.no_grad():
            got = model(dict(col))["sentence_embedding"]
        types = col.get("token_type_ids") if model.cfg.type_vocab_size > 0 else None
        ids, mask, types, _ = enc.pad_inputs(col["input_ids"].to(torch.int64), col["attention_mask"].to(torch.int64),
                                             None if types is None else types.to(torch.int64), model.cfg.pad_token_id)
        enc.set_dropout_step(11)
        bf16, _, _ = enc.forward(ids, mask, types, training=True, precision="bf16")
        enc.set_dropout_step(11)
        f16, _, _ = enc.forward(ids, mask, types, training=True, precision="f16")
        assert torch.equal(got, bf16) and not torch.equal(got, f16)
        # ... and inside the switch it runs "f16"
        enc.set_dropout_step(11)
        with torch.no_grad(), model.no_grad_passes_at_training_precision():
            inside = model(dict(col))["sentence_embedding"]
        assert torch.equal(inside, f16)
    finally:
        model.training_precision = "bf16"
        enc.set_dropout(0.0, 0.0)
        enc.grads.zero_()


# ------------------------------------------------------------------ 3. fit()
@pytest.mark.parametrize("use_amp", [False, True])
@pytest.mark.parametrize("cls", [p[0] for p in PAIRS], ids=IDS)
def test_fit_lowers_the_loss_on_its_pairs(cls, use_amp):
    """The recipe of test_gpu_mnrl.py's test of the same name, with the loader's batch of 16 cut into mini-batches of 4;
    under use_amp the loss scale reaches the replay as grad_output, a device scalar."""
    random.seed(11)
    m = SentenceTransformer("tiny-bert", device="cuda")          # a fresh model: amp schedule counters persist per model
    pairs = mnrl_examples(16, 2)
    lm = cls(m, mini_batch_size=4)
    feats, labels = m.smart_batching_collate(pairs)

    def value():
        m.eval()
        with torch.no_grad():
            return lm([{k: v.cuda() for k, v in f.items()} for f in feats], labels.cuda()).item()

    before = value()
    dl = data.NoDuplicatesDataLoader(list(pairs), 16)
    m.fit([(dl, lm)], epochs=5, warmup_steps=0, scheduler="constantlr", optimizer_params={"lr": 1e-3}, dropout=0,
          use_amp=use_amp, show_progress_bar=False)
    after = value()
    print(f"  fit {cls.__name__} amp={use_amp}: loss on the 16 pairs {before:.5f} -> {after:.5f}")
    assert np.isfinite(after) and after < before
    assert torch.isfinite(m._enc.params).all()


# ------------------------------------------------------------------ 4. smaller checks
def test_a_dense_head_trains_through_it(tmp_path):
    DH.write_model_dir(str(tmp_path / "dense"), Dout=24, act=DH.TANH)
    m = SentenceTransformer(str(tmp_path / "dense"), device="cuda")
    m.train()
    feats, labels = m.smart_batching_collate(mnrl_examples(16, 2))
    feats = [{k: v.cuda() for k, v in f.items()} for f in feats]
    dp = m._dense_params
    dp.ensure().zero_grad()
    m._enc.ensure_train_state()
    m._enc.grads.zero_()
    S.CachedMultipleNegativesRankingLoss(m, mini_batch_size=4)(feats, labels).backward()
    torch.cuda.synchronize()
    assert torch.isfinite(dp.grads).all() and int(torch.count_nonzero(dp.grads)) > 0
    assert torch.isfinite(m._enc.grads).all() and m._enc.grads.abs().max().item() > 0
    # the four mini-batches add up to the head gradients of the uncached loss
    cached = dp.grads.clone()
    dp.zero_grad()
    m._enc.grads.zero_()
    S.MultipleNegativesRankingLoss(m)(feats, labels).backward()
    assert (cached - dp.grads).norm().item() <= 2e-2 * dp.grads.norm().item()


@pytest.mark.parametrize("cls", [p[0] for p in PAIRS], ids=IDS)
def test_no_grad_gives_the_same_value_and_leaves_the_gradients_alone(model, cls):
    feats, labels = batch_of(model, 3)
    model.train()
    enc = model._enc
    lm = cls(model, mini_batch_size=5)
    want, _ = one_backward(model, lm, feats, labels)
    enc.grads.fill_(0.5)
    with torch.no_grad():
        got = lm([dict(f) for f in feats], labels)
    assert not got.requires_grad and torch.equal(got, want)
    model.eval()
    in_eval = lm([dict(f) for f in feats], labels)
    model.train()
    torch.cuda.synchronize()
    assert not in_eval.requires_grad and abs(in_eval.item() - want.item()) < 2e-4
    assert (enc.grads == 0.5).all()
    enc.grads.zero_()


@pytest.mark.parametrize("cached,plain", PAIRS, ids=IDS)
def test_a_foreign_similarity_fct_runs_in_torch(model, cached, plain):
    feats, labels = batch_of(model, 3)
    model.train()
    seen = []

    def foreign(x, y):
        seen.append((tuple(x.shape), tuple(y.shape)))
        return util.cos_sim(x, y)

    D = model.get_sentence_embedding_dimension()
    with torch.no_grad():
        got = cached(model, similarity_fct=foreign, mini_batch_size=4)([dict(f) for f in feats], labels)
        want = cached(model, mini_batch_size=4)([dict(f) for f in feats], labels)
    assert seen == [((16, D), (32, D))]
    assert M.value_error(got.item(), want.item(), D) <= 1.0
    # ... and with a differentiable one (util.cos_sim is a kernel without autograd) its gradients are the kernel path's

    def in_torch(x, y):
        return torch.nn.functional.normalize(x, p=2, dim=1) @ torch.nn.functional.normalize(y, p=2, dim=1).t()

    want_l, want_g = one_backward(model, cached(model, mini_batch_size=4), feats, labels)
    got_l, got_g = one_backward(model, cached(model, similarity_fct=in_torch, mini_batch_size=4), feats, labels)
    close(got_l, got_g, want_l, want_g, f"{cached.__name__} with a foreign similarity_fct")


def test_matryoshka_refuses_to_wrap_it(model):
    for cls, _ in PAIRS:
        with pytest.raises(ValueError):
            S.MatryoshkaLoss(model, cls(model), [32, 16])
