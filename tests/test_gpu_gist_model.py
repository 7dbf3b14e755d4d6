"""GPU: GISTEmbedLoss and CachedGISTEmbedLoss on a real encoder -- tiny-bert, a tiny-bert guide with another seed, the 16
examples of test_gpu_cached_mnrl.py: the loss and the arena gradients are those of sentence-transformers' formula
(gist_helpers.gist_ref) run in torch on the model's own autograd embeddings, the cached form is the uncached one, the replay
is exact, the guide stays frozen and in eval mode, fit() trains through both, and a duplicated text is masked."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import gist_helpers as G  # noqa: E402
from quadruplet_sentence_transformer_amd import data, st_losses as S  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, SentenceTransformer  # noqa: E402
from test_gpu_cached_mnrl import Tap, batch_of, close, mnrl_examples, one_backward, sent  # noqa: E402

GUIDE_SEED = 44
T = 0.01
MIN_MODEL_GAP = 1e-4


@pytest.fixture(scope="module")
def model():
    return SentenceTransformer("tiny-bert", device="cuda")


@pytest.fixture(scope="module")
def guide():
    return SentenceTransformer("tiny-bert", device="cuda", seed=GUIDE_SEED)


def guide_gap(lm, feats, margin_strategy="absolute", margin=0.0):
    """The smallest |guide entry - bound_i| of a batch, from the guide embeddings the loss itself computes."""
    g = lm._embed_guide([dict(f) for f in feats]).double().cpu()
    _, gaps = G.gist_masks(list(g.chunk(len(feats), 0)), margin_strategy, margin)
    return min(float(x.min()) for x in gaps)


class Formula:
    """sentence-transformers' GISTEmbedLoss.forward in torch ops: one autograd pass per column, the guide's embeddings as the
    loss under test computes them."""

    def __init__(self, model, lm):
        self.model, self.lm = model, lm

    def __call__(self, feats, labels):
        guide_cols = list(self.lm._embed_guide([dict(f) for f in feats]).chunk(len(feats), 0))
        cols = [self.model(dict(f))["sentence_embedding"] for f in feats]
        return G.gist_ref(cols, guide_cols, self.lm.temperature, self.lm.margin_strategy, self.lm.margin)


# ------------------------------------------------------------------ 1. the loss is the formula
@pytest.mark.parametrize("k", [2, 3])
def test_the_guide_decides_its_masks_on_these_examples(model, guide, k):
    feats, _ = batch_of(model, k)
    gap = guide_gap(S.GISTEmbedLoss(model, guide), feats)
    print(f"  k={k}: the guide's smallest |entry - threshold| on the 16 examples: {gap:.3e}")
    assert gap >= MIN_MODEL_GAP


@pytest.mark.parametrize("margin_strategy,margin", [("absolute", 0.0), ("relative", 0.02)])
@pytest.mark.parametrize("k", [2, 3])
def test_equals_the_formula_in_torch(model, guide, k, margin_strategy, margin):
    feats, labels = batch_of(model, k)
    model.train()
    assert model._enc.dropout is None
    lm = S.GISTEmbedLoss(model, guide, T, margin_strategy, margin)
    assert guide_gap(lm, feats, margin_strategy, margin) >= MIN_MODEL_GAP
    want_l, want_g = one_backward(model, Formula(model, lm), feats, labels)
    got_l, got_g = one_backward(model, lm, feats, labels)
    close(got_l, got_g, want_l, want_g, f"GISTEmbedLoss k={k} {margin_strategy} {margin}")
    # fused=False: one pass per column
    sep_l, sep_g = one_backward(model, S.GISTEmbedLoss(model, guide, T, margin_strategy, margin, fused=False), feats, labels)
    close(sep_l, sep_g, got_l, got_g, f"fused=False k={k}")


@pytest.mark.parametrize("mini", [4, 5, 16, 64])
@pytest.mark.parametrize("k", [2, 3])
def test_cached_equals_the_uncached_loss(model, guide, k, mini):
    feats, labels = batch_of(model, k)
    model.train()
    assert guide_gap(S.GISTEmbedLoss(model, guide), feats) >= MIN_MODEL_GAP
    want_l, want_g = one_backward(model, S.GISTEmbedLoss(model, guide, T), feats, labels)
    got_l, got_g = one_backward(model, S.CachedGISTEmbedLoss(model, guide, T, mini_batch_size=mini), feats, labels)
    close(got_l, got_g, want_l, want_g, f"CachedGISTEmbedLoss k={k} mini_batch_size={mini}")


def test_no_grad_gives_the_same_value_and_leaves_the_gradients_alone(model, guide):
    feats, labels = batch_of(model, 3)
    model.train()
    enc = model._enc
    lm = S.CachedGISTEmbedLoss(model, guide, T, mini_batch_size=5)
    want, _ = one_backward(model, lm, feats, labels)
    enc.grads.fill_(0.5)
    with torch.no_grad():
        got = lm([dict(f) for f in feats], labels)
    torch.cuda.synchronize()
    assert not got.requires_grad and torch.equal(got, want) and (enc.grads == 0.5).all()
    enc.grads.zero_()


# ------------------------------------------------------------------ 2. the replay
def test_replay_is_exact_and_leaves_the_counter_where_the_first_pass_left_it(model, guide):
    feats, labels = batch_of(model, 2)
    model.train()
    enc = model._enc
    try:
        enc.set_dropout(0.1, 0.1, 123)
        enc.set_dropout_step(7)
        tap = Tap(model)
        lm = S.CachedGISTEmbedLoss(tap, guide, T, mini_batch_size=4)
        enc.ensure_train_state()
        enc.grads.zero_()
        loss = lm([dict(f) for f in feats], labels)
        passes = 4
        assert len(tap.seen) == passes and not any(grad for grad, _ in tap.seen)
        after_first = enc.dropout_step
        assert after_first == 7 + passes
        loss.backward()
        torch.cuda.synchronize()
        assert len(tap.seen) == 2 * passes and all(grad for grad, _ in tap.seen[passes:])
        for (_, first), (_, second) in zip(tap.seen[:passes], tap.seen[passes:]):
            assert first.shape[0] == 8 and torch.equal(first, second)
        assert not torch.equal(tap.seen[0][1], tap.seen[1][1])
        assert enc.dropout_step == after_first and int(enc.drop_state[2].item()) == after_first
        assert enc.grads.abs().max().item() > 0
    finally:
        enc.set_dropout(0.0, 0.0)
        enc.grads.zero_()


# ------------------------------------------------------------------ 3. the guide is frozen
@pytest.mark.parametrize("cls", [S.GISTEmbedLoss, S.CachedGISTEmbedLoss])
def test_the_guide_stays_in_eval_mode_and_sees_no_dropout(model, guide, cls):
    feats, labels = batch_of(model, 2)
    enc = model._enc
    guide.eval()
    with torch.no_grad():
        want = torch.cat([guide(dict(f))["sentence_embedding"] for f in feats], 0)       # eval mode, one pass per column
    seen = []
    hook = guide.register_forward_hook(
        lambda mod, args, out: seen.append((mod.training, torch.is_grad_enabled(), out["sentence_embedding"].clone())))
    try:
        lm = cls(model, guide, T)
        assert guide not in list(lm.modules()) and not any(p is q for p in lm.parameters() for q in guide.parameters())
        guide.train()                                                    # whoever left it so: the loss puts it back
        lm.train()
        model.train()
        enc.set_dropout(0.1, 0.1, 5)
        assert guide._enc.dropout is None
        before = guide._enc.dropout_step
        one_backward(model, lm, feats, labels)
        assert guide.training is False and seen
        assert all(training is False and grad is False for training, grad, _ in seen)
        got = torch.cat([emb for _, _, emb in seen], 0)
        assert got.shape == want.shape and (got - want).abs().max().item() < 2e-3        # another padding length at most
        assert guide._enc.dropout_step == before and guide._enc.dropout is None
        lm.train()
        assert guide.training is False and model.training is True
    finally:
        hook.remove()
        enc.set_dropout(0.0, 0.0)
        enc.grads.zero_()


# ------------------------------------------------------------------ 4. fit()
@pytest.mark.parametrize("cls", [S.GISTEmbedLoss, S.CachedGISTEmbedLoss])
def test_fit_lowers_the_loss_and_leaves_the_guide_alone(cls):
    random.seed(11)
    m = SentenceTransformer("tiny-bert", device="cuda")
    g = SentenceTransformer("tiny-bert", device="cuda", seed=GUIDE_SEED)
    pairs = mnrl_examples(16, 2)
    lm = cls(m, g, T, mini_batch_size=4) if cls is S.CachedGISTEmbedLoss else cls(m, g, T)
    feats, labels = m.smart_batching_collate(pairs)
    arena = g._enc.params.clone()

    def value():
        m.eval()
        with torch.no_grad():
            return lm([{k: v.cuda() for k, v in f.items()} for f in feats], labels.cuda()).item()

    before = value()
    dl = data.NoDuplicatesDataLoader(list(pairs), 16)
    m.fit([(dl, lm)], epochs=24, warmup_steps=0, scheduler="constantlr", optimizer_params={"lr": 1e-3}, dropout=0,
          show_progress_bar=False)
    after = value()
    print(f"  fit {cls.__name__}: loss on the 16 pairs {before:.5f} -> {after:.5f}")
    assert np.isfinite(after) and after < before
    assert torch.isfinite(m._enc.params).all()
    assert torch.equal(g._enc.params, arena) and g.training is False
    assert lm.get_config_dict() == {"guide": "tiny-bert", "temperature": T, "margin_strategy": "absolute", "margin": 0.0}


# ------------------------------------------------------------------ 5. smaller checks
def test_a_duplicated_anchor_is_masked(model, guide):
    """Examples 2 and 5 share their anchor text: the guide's aa[2, 5] and aa[5, 2] are 1, above any threshold, and leave the
    softmax although the student scores them 1 / temperature = 100 too. The loss is that of the formula; with those two
    entries left in it would be far away. (ap[2, 5] goes when the guide finds positive 5 closer to the anchor than positive 2,
    as upstream; the formula decides.)"""
    ex = mnrl_examples(16, 2)
    ex[5] = InputExample(texts=[ex[2].texts[0], sent(77, 9)])
    feats, labels = model.smart_batching_collate(ex)
    feats, labels = [{key: v.cuda() for key, v in f.items()} for f in feats], labels.cuda()
    model.train()
    lm = S.GISTEmbedLoss(model, guide, T)
    assert guide_gap(lm, feats) >= MIN_MODEL_GAP
    g = lm._embed_guide([dict(f) for f in feats])
    masks, _ = G.gist_masks(list(g.chunk(2, 0)))
    assert bool(masks[1][2, 5]) and bool(masks[1][5, 2])
    want_l, want_g = one_backward(model, Formula(model, lm), feats, labels)
    got_l, got_g = one_backward(model, lm, feats, labels)
    assert torch.isfinite(got_l) and torch.isfinite(got_g).all()
    close(got_l, got_g, want_l, want_g, "a duplicated anchor")
    with torch.no_grad():
        cols = [model(dict(f))["sentence_embedding"] for f in feats]
        blocks = G.gist_blocks(cols)
        keep = [m.clone() for m in masks]
        keep[1][2, 5] = keep[1][5, 2] = False
        unmasked = torch.nn.functional.cross_entropy(
            torch.cat([b.masked_fill(m, -torch.inf) for b, m in zip(blocks, keep)], 1) / T, torch.arange(16, device="cuda"))
    # each of the two rows gains an entry at the largest possible logit, 1 / T, among at most 3 * 16 entries none of which
    # is larger: its log-sum-exp grows by at least log(1 + 1 / 48), the mean over 16 rows by 2.6e-3 -- 13 x the bound of close()
    far = 2 * np.log1p(1 / 48) / 16
    print(f"  with aa[2, 5] and aa[5, 2] left in: {unmasked.item():.6f} against {got_l.item():.6f}; at least {far:.2e} apart")
    assert unmasked.item() - got_l.item() >= far


def test_two_columns_at_least_and_a_guide_of_this_package(model, guide):
    feats, labels = batch_of(model, 2)
    for cls in (S.GISTEmbedLoss, S.CachedGISTEmbedLoss):
        with pytest.raises(ValueError, match="2 or more"):
            cls(model, guide)(feats[:1], labels)
        with pytest.raises(TypeError, match="guide"):
            cls(model, torch.nn.Identity())


def test_a_guide_that_cannot_read_the_ids_is_refused(model):
    """Stand-in tokenizers (no vocabulary files) hash words into the embedding table: a guide of another vocabulary size or
    max_seq_length would need the texts back, and ids of a hash cannot be decoded."""
    from dataclasses import replace
    other = SentenceTransformer(config=replace(model.cfg, vocab_size=model.cfg.vocab_size // 2), device="cuda")
    with pytest.raises(ValueError, match="decoded"):
        S.GISTEmbedLoss(model, other)
    same = SentenceTransformer(config=model.cfg, device="cuda", seed=3)
    assert S.GISTEmbedLoss(model, same).must_retokenize is False


def test_matryoshka_wraps_the_plain_form_and_refuses_the_cached_one(model, guide):
    feats, labels = batch_of(model, 2)
    model.train()
    D = model.get_sentence_embedding_dimension()
    full = S.GISTEmbedLoss(model, guide, T)
    want_l, want_g = one_backward(model, full, feats, labels)
    got_l, got_g = one_backward(model, S.MatryoshkaLoss(model, S.GISTEmbedLoss(model, guide, T), [D]), feats, labels)
    close(got_l, got_g, want_l, want_g, "MatryoshkaLoss over GISTEmbedLoss at the full width")
    with pytest.raises(ValueError, match="Cached"):
        S.MatryoshkaLoss(model, S.CachedGISTEmbedLoss(model, guide), [D, D // 2])
