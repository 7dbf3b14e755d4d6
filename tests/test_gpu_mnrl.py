"""GPU: MultipleNegativesRankingLoss and its symmetric form -- qst_mnrl_loss (csrc/mnrl.hip), its autograd and the loss
classes of st_losses.py -- against the yardstick in mnrl_helpers: sentence-transformers 2.2.2's formula in torch ops, fp64
on the CPU with autograd. Tolerances are the project's: the value within rtol = atol = max(1e-5, 1.5e-8 D), gradients
within rtol 1e-4, atol 1e-6 * max(1, max |reference gradient|)."""
import random

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import mnrl_helpers as M  # noqa: E402
from kernel_helpers import lib, ptr, stream  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import data, st_losses as S, util  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, SentenceTransformer  # noqa: E402

SIMS = ("cos", "dot")


def check(out, grads, loss, ga, gc, D, what=""):
    """Prints every figure as a share of its tolerance, then asserts."""
    ev = M.value_error(out.item(), loss, D)
    ea, ec = M.grad_error(grads[0].cpu(), ga), M.grad_error(grads[1].cpu(), gc)
    print(f"  {what}: loss {out.item():.7f} ref {loss.item():.7f}; share of the tolerance: value {ev:.3f} grad_a {ea:.3f} "
          f"grad_c {ec:.3f}")
    assert torch.isfinite(out).all() and torch.isfinite(grads[0]).all() and torch.isfinite(grads[1]).all()
    assert ev <= 1.0 and ea <= 1.0 and ec <= 1.0


# ------------------------------------------------------------------ 1. kernel parity
@pytest.mark.parametrize("trained", [0, 1])
@pytest.mark.parametrize("symmetric", [0, 1], ids=["plain", "symmetric"])
@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("B,N,D", M.SHAPES)
def test_kernel_matches_reference(lib, B, N, D, sim, symmetric, trained):
    a, c, loss, ga, gc = M.reference(B, N, D, sim, symmetric, trained)
    if N > 1:       # the softmax of the reference is not saturated: a wrong gradient has nowhere to hide
        assert loss.item() >= M.MIN_REF_LOSS and ga.abs().max().item() >= M.MIN_REF_GRAD
    out, grads = S.mnrl_loss_raw(a.cuda(), c.cuda(), sim, M.SCALE, symmetric, want_grads=True)
    if (B, N, D) == (1, 1, 1):
        assert loss.item() == 0.0
        assert out.item() == 0.0 and not grads[0].any() and not grads[1].any()
    check(out, grads, loss, ga, gc, D, f"{B}x{N}x{D} {sim} sym={symmetric} trained={trained}")
    # the forward-only call returns the same value
    fwd, none = S.mnrl_loss_raw(a.cuda(), c.cuda(), sim, M.SCALE, symmetric)
    assert none == [None, None] and torch.equal(fwd, out)


@pytest.mark.parametrize("symmetric", [0, 1], ids=["plain", "symmetric"])
def test_zero_rows_follow_the_clamp_of_normalize(lib, symmetric):
    """|x| < 1e-12: the normalised row is 0 and its gradient d_hat / 1e-12 -- entries of 1e8 (the zero candidate, whose
    softmax weights are small) to 1e12 (the zero anchor), which is why the absolute tolerance is taken relative to the
    largest reference entry."""
    a, c = M.case(5, 10, 10, "cos", 0, 5010)
    a, c = a.clone(), c.clone()
    a[2] = 0
    c[7] = 0
    loss, ga, gc = M.reference_of(a, c, "cos", symmetric)
    assert ga[2].abs().max().item() > 1e10 and gc[7].abs().max().item() > 1e6      # the clamp, not a small norm
    out, grads = S.mnrl_loss_raw(a.cuda(), c.cuda(), "cos", M.SCALE, symmetric, want_grads=True)
    check(out, grads, loss, ga, gc, 10, f"zero rows sym={symmetric}")
    # the two clamped rows on their own, at the relative tolerance
    torch.testing.assert_close(grads[0].cpu().double()[2], ga[2], rtol=1e-4, atol=1e-4 * ga[2].abs().max().item())
    torch.testing.assert_close(grads[1].cpu().double()[7], gc[7], rtol=1e-4, atol=1e-4 * gc[7].abs().max().item())


# ------------------------------------------------------------------ 2. the call itself
def raw_call(lib, a, c, sim, symmetric, out, grad_out, ga, gc, ws=None):
    B, D = a.shape
    N = c.shape[0]
    nbytes = lib.qst_mnrl_workspace_bytes(B, N, D)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda") if ws is None else ws
    return lib.qst_mnrl_loss(ptr(a), ptr(c), B, N, D, S._SIM_CODE.get(sim, sim), M.SCALE, symmetric, ptr(out),
                             ptr(grad_out), ptr(ga), ptr(gc), ptr(ws), nbytes, stream())


@pytest.mark.parametrize("sim", SIMS)
def test_forward_only_writes_nothing_else_and_one_null_gradient_is_refused(lib, sim):
    a, c = [t.cuda() for t in M.case(7, 14, 33, sim, 1, 7033)]
    ga, gc = torch.full_like(a, -7.25), torch.full_like(c, -7.25)
    out = torch.zeros(1, device="cuda")
    assert raw_call(lib, a, c, sim, 1, out, None, None, None) == 0
    torch.cuda.synchronize()
    assert (ga == -7.25).all() and (gc == -7.25).all() and out.item() > 0
    assert raw_call(lib, a, c, sim, 1, out, None, ga, None) == -1
    assert raw_call(lib, a, c, sim, 1, out, None, None, gc) == -1
    assert raw_call(lib, a, c, 2, 1, out, None, ga, gc) == -1          # QST_SCORE_EUCLID
    torch.cuda.synchronize()
    assert (ga == -7.25).all() and (gc == -7.25).all()


@pytest.mark.parametrize("symmetric", [0, 1], ids=["plain", "symmetric"])
@pytest.mark.parametrize("sim", SIMS)
def test_grad_out_is_read_on_the_device_and_scales_the_gradients(lib, sim, symmetric):
    """grad_out = 3 gives 3 x the gradients of grad_out = NULL within 1 ulp per element (the upstream gradient multiplies
    the finished gradient), and the loss does not move."""
    a, c = [t.cuda() for t in M.case(65, 195, 384, sim, 1, 65384)]
    o1, g1 = S.mnrl_loss_raw(a, c, sim, M.SCALE, symmetric, want_grads=True)
    o3, g3 = S.mnrl_loss_raw(a, c, sim, M.SCALE, symmetric, grad_out=torch.tensor([3.0], device="cuda"), want_grads=True)
    assert torch.equal(o1, o3)
    for x1, x3 in zip(g1, g3):
        want = 3.0 * x1.double()
        ulp = torch.finfo(torch.float32).eps * want.abs().clamp_min(torch.finfo(torch.float32).tiny)
        assert ((x3.double() - want).abs() <= ulp).all()
        assert x1.abs().max().item() > 0


def test_two_identical_calls_are_bit_identical(lib):
    for (B, N, D) in [(130, 260, 64), (33, 99, 768), (7, 14, 33)]:
        for sim in SIMS:
            for symmetric in (0, 1):
                a, c = [t.cuda() for t in M.case(B, N, D, sim, 1, 1000 * B + D)]
                w = torch.tensor([1.7], device="cuda")
                o1, g1 = S.mnrl_loss_raw(a, c, sim, M.SCALE, symmetric, grad_out=w, want_grads=True)
                o2, g2 = S.mnrl_loss_raw(a, c, sim, M.SCALE, symmetric, grad_out=w, want_grads=True)
                assert torch.equal(o1, o2) and torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])


def test_non_default_stream_gives_the_same_result(lib):
    a, c = [t.cuda() for t in M.case(64, 128, 384, "cos", 1, 64384)]
    o1, g1 = S.mnrl_loss_raw(a, c, "cos", M.SCALE, 1, want_grads=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        o2, g2 = S.mnrl_loss_raw(a, c, "cos", M.SCALE, 1, want_grads=True)
    side.synchronize()
    assert torch.equal(o1, o2) and torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])


def test_the_call_pair_is_capturable_in_a_graph(lib):
    """No host synchronisation, grad_out read on the device: a captured forward + backward call replays on new inputs and a
    new upstream gradient written into the same buffers."""
    (a1, c1), (a2, c2) = [[t.cuda() for t in M.case(7, 14, 33, "cos", tr, 7033)] for tr in (0, 1)]
    a, c, w = a1.clone(), c1.clone(), torch.tensor([1.0], device="cuda")
    S.mnrl_loss_raw(a, c, "cos", M.SCALE, 1, grad_out=w, want_grads=True)      # code objects loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fwd, _ = S.mnrl_loss_raw(a, c, "cos", M.SCALE, 1)
        out, grads = S.mnrl_loss_raw(a, c, "cos", M.SCALE, 1, grad_out=w, want_grads=True)
    a.copy_(a2), c.copy_(c2), w.fill_(2.5)
    graph.replay()
    torch.cuda.synchronize()
    want, want_g = S.mnrl_loss_raw(a2, c2, "cos", M.SCALE, 1, grad_out=torch.tensor([2.5], device="cuda"), want_grads=True)
    assert torch.equal(fwd, want) and torch.equal(out, want)
    assert torch.equal(grads[0], want_g[0]) and torch.equal(grads[1], want_g[1])


# ------------------------------------------------------------------ 3. autograd
@pytest.mark.parametrize("symmetric", [False, True], ids=["plain", "symmetric"])
@pytest.mark.parametrize("sim", SIMS)
def test_autograd_equals_the_raw_call(lib, sim, symmetric):
    a0, c0 = [t.cuda() for t in M.case(33, 99, 768, sim, 1, 33768)]
    a, c = a0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
    loss = S.multiple_negatives_ranking_loss(a, c, M.SCALE, sim, symmetric)
    assert loss.dim() == 0
    (loss * 1.7).backward()
    out, grads = S.mnrl_loss_raw(a0, c0, sim, M.SCALE, symmetric, grad_out=torch.tensor([1.7], device="cuda"), want_grads=True)
    assert torch.equal(loss.detach().reshape(1), out) and torch.equal(a.grad, grads[0]) and torch.equal(c.grad, grads[1])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_autograd_returns_gradients_in_the_input_dtypes(lib, dtype):
    a0, c0 = [t.cuda().to(dtype) for t in M.case(8, 16, 384, "cos", 1, 8384)]
    a, c = a0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
    S.multiple_negatives_ranking_loss(a, c).backward()
    assert a.grad.dtype == dtype and c.grad.dtype == dtype
    _, grads = S.mnrl_loss_raw(a0.float(), c0.float(), "cos", 20.0, False, want_grads=True)
    assert torch.equal(a.grad, grads[0].to(dtype)) and torch.equal(c.grad, grads[1].to(dtype))


# ------------------------------------------------------------------ 4. the classes on a real encoder
WORDS = "a man rides red horse two dogs play in park woman eats green apple near old bridge small cat sleeps".split()


def sent(i, n):
    rng = np.random.RandomState(i)
    return " ".join(rng.choice(WORDS, size=n))


def mnrl_examples(n, k):
    """(anchor, positive that shares the anchor's words[, an unrelated hard negative])."""
    return [InputExample(texts=[sent(i, 9), sent(i, 9) + " now", sent(1000 + i, 5 + i % 7)][:k]) for i in range(n)]


class Tap(nn.Module):
    """The model, keeping hold of the sentence embeddings it returns (and of their gradients)."""

    def __init__(self, model):
        super().__init__()
        self.model, self.cfg, self.seen = model, model.cfg, []

    def forward(self, feats):
        out = self.model(feats)
        out["sentence_embedding"].retain_grad()
        self.seen.append(out["sentence_embedding"])
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


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("cls", [S.MultipleNegativesRankingLoss, S.MultipleNegativesSymmetricRankingLoss],
                         ids=["plain", "symmetric"])
@pytest.mark.parametrize("sim", SIMS)
def test_class_equals_torch_ops_on_the_same_embeddings(model, cls, k, sim):
    feats, labels = batch_of(model, k)
    model.train()
    tap = Tap(model)
    fct = util.cos_sim if sim == "cos" else util.dot_score
    loss, _ = one_backward(model, cls(tap, similarity_fct=fct), feats, labels)
    assert len(tap.seen) == 1 and tap.seen[0].shape[0] == 16 * k         # one fused pass
    emb = tap.seen[0]
    a64, c64 = emb.detach()[:16].double().requires_grad_(True), emb.detach()[16:].double().requires_grad_(True)
    ref = M.mnrl_ref(a64, c64, sim, 20.0, cls._symmetric)
    ref.backward()
    D = emb.shape[1]
    ev = M.value_error(loss.item(), ref.item(), D)
    eg = M.grad_error(emb.grad, torch.cat([a64.grad, c64.grad], 0))
    print(f"  {cls.__name__} k={k} {sim}: loss {loss.item():.7f} torch ops {ref.item():.7f}; share of the tolerance: value "
          f"{ev:.3f} embedding gradients {eg:.3f}")
    assert ref.item() > M.MIN_REF_LOSS and ev <= 1.0 and eg <= 1.0


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("cls", [S.MultipleNegativesRankingLoss, S.MultipleNegativesSymmetricRankingLoss],
                         ids=["plain", "symmetric"])
def test_class_fused_pass_equals_one_pass_per_column(model, cls, k):
    feats, labels = batch_of(model, k)
    model.train()
    lk, gk = one_backward(model, cls(model, fused=False), feats, labels)
    l1, g1 = one_backward(model, cls(model, fused=True), feats, labels)
    assert g1.norm().item() > 0
    assert abs(lk.item() - l1.item()) < 2e-4
    assert (gk - g1).norm().item() <= 2e-2 * g1.norm().item()


@pytest.mark.parametrize("cls", [S.MultipleNegativesRankingLoss, S.MultipleNegativesSymmetricRankingLoss],
                         ids=["plain", "symmetric"])
def test_a_foreign_similarity_fct_runs_in_torch(model, cls):
    feats, labels = batch_of(model, 3)
    model.train()
    seen = []

    def foreign(x, y):
        seen.append((tuple(x.shape), tuple(y.shape)))
        return util.cos_sim(x, y)

    with torch.no_grad():
        got = cls(model, similarity_fct=foreign)([dict(f) for f in feats], labels)
        want = cls(model)([dict(f) for f in feats], labels)
    D = model.get_sentence_embedding_dimension()
    assert seen == [((16, D), (32, D))]
    assert M.value_error(got.item(), want.item(), D) <= 1.0


# ------------------------------------------------------------------ 5. fit()
@pytest.mark.parametrize("use_amp", [False, True])
@pytest.mark.parametrize("cls", [S.MultipleNegativesRankingLoss, S.MultipleNegativesSymmetricRankingLoss],
                         ids=["plain", "symmetric"])
def test_fit_lowers_the_loss_on_its_pairs(cls, use_amp):
    """5 epochs over 16 pairs whose positives share their anchors' words, fed by NoDuplicatesDataLoader; under use_amp
    the loss scale reaches the kernel as grad_out, a device scalar."""
    random.seed(11)
    m = SentenceTransformer("tiny-bert", device="cuda")          # a fresh model: amp schedule counters persist per model
    pairs = mnrl_examples(16, 2)
    lm = cls(m)
    feats, labels = m.smart_batching_collate(pairs)

    def value():
        m.eval()
        with torch.no_grad():
            return lm([{k: v.cuda() for k, v in f.items()} for f in feats], labels.cuda()).item()

    before = value()
    dl = data.NoDuplicatesDataLoader(list(pairs), 8)
    m.fit([(dl, lm)], epochs=5, warmup_steps=0, scheduler="constantlr", optimizer_params={"lr": 1e-3}, dropout=0,
          use_amp=use_amp, show_progress_bar=False)
    after = value()
    print(f"  fit {cls.__name__} amp={use_amp}: loss on the 16 pairs {before:.5f} -> {after:.5f}")
    assert np.isfinite(after) and after < before
    assert torch.isfinite(m._enc.params).all()
