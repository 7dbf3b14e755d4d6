"""GPU: the distillation objectives (csrc/distill.hip: qst_embed_mse, qst_margin_mse_loss), MSELoss and MarginMSELoss on
top of them (st_losses.py), fit() on vector labels, MSEEvaluator and TranslationEvaluator, against the yardstick in
distill_helpers: sentence-transformers 2.2.2's formulas in torch ops, fp64 on the CPU with autograd."""
import csv
import os

import numpy as np
import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import distill_helpers as DH  # noqa: E402
import tuple_loss_helpers as H  # noqa: E402
from distill_helpers import (SIMS, U, margin_bounds, margin_labels, mse_rel_bound, reduced_bound)  # noqa: E402
from tuple_loss_helpers import RED, check_grads, dev, f64, upstream  # noqa: E402
from kernel_helpers import lib, ptr, stream  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import st_losses as S, util  # noqa: E402
from quadruplet_sentence_transformer_amd.data import ParallelSentencesDataset  # noqa: E402
from quadruplet_sentence_transformer_amd.evaluation import MSEEvaluator, TranslationEvaluator, translation_matches  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import (InputExample, SentenceTransformer,  # noqa: E402
                                                                      encode_columns_fused)

BAD_ARG = -1
# B = 1; the element-by-element path (D % 4 != 0); D past 2048, where the rows no longer stay in registers; 2500 rows = three
# trips of the 1024-row second stage, the last one partial, on both load paths
SHAPES = H.SHAPES + [(2500, 33), (2500, 64)]


# ------------------------------------------------------------------ 1. kernel parity
@pytest.mark.parametrize("B,D", SHAPES)
def test_embed_mse_matches_yardstick(lib, B, D):
    x, t = H.rows(B, D, 2, B * 1000 + D + 3)
    for w in (None, torch.tensor([1.7])):
        (xs,) = f64((x,))
        ref = DH.embed_mse_ref(xs, t.double())
        (ref * (1.0 if w is None else w.double())).sum().backward()
        out, grad = S.embed_mse_raw(dev(x), dev(t), grad_out=None if w is None else dev(w), want_grads=True)
        assert out.shape == (1,) and grad.shape == (B, D)
        err, bound = abs(out.cpu().double().item() - ref.item()), mse_rel_bound(D) * ref.item()
        print(f"  embed_mse {B}x{D}: |d| = {err:.3e}, bound {bound:.3e} (value {ref.item():.6f})")
        assert err <= bound
        check_grads([grad], [xs])


@pytest.mark.parametrize("B,D", SHAPES)
@pytest.mark.parametrize("sim", SIMS, ids=lambda m: H.METRIC_NAMES[m])
def test_margin_mse_matches_yardstick(lib, B, D, sim):
    q, p, n = H.rows(B, D, 3, B * 1000 + D + 4)
    y = margin_labels(q, p, n, sim, B + D)
    dm, drow = margin_bounds(q, p, n, y, sim)
    m_ref = DH.margin_ref(q.double(), p.double(), n.double(), sim)
    for red_name, red in RED:
        xs = f64((q, p, n))
        ref = DH.margin_mse_ref(*xs, y, sim, red_name)
        w = upstream(B, red)
        (ref * w.double()).sum().backward()
        out, grads, margin = S.margin_mse_raw(dev(q), dev(p), dev(n), dev(y), sim, red, grad_out=dev(w), want_grads=True,
                                              want_margin=True)
        assert out.shape == ((B,) if red == 0 else (1,)) and margin.shape == (B,)
        err = (out.cpu().double().view(ref.shape) - ref.detach()).abs()
        bound = reduced_bound(drow, ref, red)
        merr = (margin.cpu().double() - m_ref).abs()
        print(f"  margin_mse {H.METRIC_NAMES[sim]} {B}x{D} {red_name}: max |d| / bound = {(err / bound).max().item():.3e}; "
              f"margin {(merr / dm).max().item():.3e}")
        assert (err <= bound).all() and (merr <= dm).all()
        check_grads(grads, xs)


@pytest.mark.parametrize("B,D", [(64, 384), (7, 33), (5, 5120), (2500, 64)])
def test_the_upstream_gradient_multiplies_the_finished_gradient(lib, B, D):
    """grad_out = g gives g x (the gradients without), rounded once: the product of two fp32 numbers is exact in double."""
    q, p, n = [dev(t) for t in H.rows(B, D, 3, 17)]
    y = dev(margin_labels(q.cpu(), p.cpu(), n.cpu(), H.COS_SIM, 1))
    w = dev(torch.tensor([1.7]))
    _, base = S.embed_mse_raw(q, p, want_grads=True)
    _, got = S.embed_mse_raw(q, p, grad_out=w, want_grads=True)
    assert torch.equal(got, (base.double() * w.double()).float())
    for sim in SIMS:
        for red in (0, 1, 2):
            w = dev(upstream(B, red))
            _, base = S.margin_mse_raw(q, p, n, y, sim, red, want_grads=True)
            _, got = S.margin_mse_raw(q, p, n, y, sim, red, grad_out=w, want_grads=True)
            wd = w.double()[:, None] if red == 0 else w.double()
            for g, b in zip(got, base):
                assert torch.equal(g, (b.double() * wd).float())


def test_forward_only_equals_the_value_of_a_gradient_call_and_writes_nothing_else(lib):
    B, D = 9, 96
    q, p, n = [dev(t) for t in H.rows(B, D, 3, 11)]
    y = dev(margin_labels(q.cpu(), p.cpu(), n.cpu(), H.DOT, 2))
    # [guard | out | guard] for the loss, the margins and the scratch rows, and gradient buffers that are not handed over
    canary = [torch.full((B, D), 7.0, device="cuda") for _ in range(3)]
    buf = torch.full((3, B), 7.0, device="cuda")
    sc = torch.full((3, B), 7.0, device="cuda")
    assert lib.qst_embed_mse(ptr(q), ptr(p), B, D, ptr(buf[1]), None, None, ptr(sc[1]), stream()) == 0
    full, _ = S.embed_mse_raw(q, p, want_grads=True)
    assert torch.equal(buf[1, :1], full) and (buf[0] == 7.0).all() and (buf[2] == 7.0).all() and (buf[1, 1:] == 7.0).all()
    assert (sc[0] == 7.0).all() and (sc[2] == 7.0).all()
    for sim in SIMS:
        for red, n_out in ((0, B), (1, 1), (2, 1)):
            buf = torch.full((3, B), 7.0, device="cuda")
            mg = torch.full((3, B), 7.0, device="cuda")
            sc = torch.full((3, B), 7.0, device="cuda")
            rc = lib.qst_margin_mse_loss(ptr(q), ptr(p), ptr(n), ptr(y), B, D, sim, red, ptr(buf[1]), ptr(mg[1]), None,
                                         None, None, None, ptr(sc[1]), stream())
            assert rc == 0
            full, _, margin = S.margin_mse_raw(q, p, n, y, sim, red, want_grads=True, want_margin=True)
            assert torch.equal(buf[1, :n_out], full) and torch.equal(mg[1], margin)
            for t in (buf, mg, sc):
                assert (t[0] == 7.0).all() and (t[2] == 7.0).all()
            assert (buf[1, n_out:] == 7.0).all()
            # without out_margin and, for reduction none, without scratch
            o2 = torch.full((B,), 7.0, device="cuda")
            rc = lib.qst_margin_mse_loss(ptr(q), ptr(p), ptr(n), ptr(y), B, D, sim, red, ptr(o2), None, None,
                                         None, None, None, None if red == 0 else ptr(sc[1]), stream())
            assert rc == 0 and torch.equal(o2[:n_out], full)
    assert all((c == 7.0).all() for c in canary)


def test_two_identical_calls_are_bit_identical(lib):
    for B, D in ((64, 384), (2000, 768), (5, 5120), (7, 33), (2500, 64)):
        q, p, n = [dev(t) for t in H.rows(B, D, 3, 3)]
        y = dev(torch.linspace(-1, 1, B))
        w = dev(torch.tensor([1.3]))
        calls = [lambda: S.embed_mse_raw(q, p, grad_out=w, want_grads=True),
                 lambda: S.margin_mse_raw(q, p, n, y, H.DOT, 2, grad_out=w, want_grads=True),
                 lambda: S.margin_mse_raw(q, p, n, y, H.COS_SIM, 1, grad_out=w, want_grads=True),
                 lambda: S.margin_mse_raw(q, p, n, y, H.COS_SIM, 0, grad_out=dev(upstream(B, 0)), want_grads=True)]
        for call in calls:
            o1, g1 = call()
            o2, g2 = call()
            g1, g2 = (g1, g2) if isinstance(g1, list) else ([g1], [g2])
            assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


# ------------------------------------------------------------------ 2. degenerate rows
@pytest.mark.parametrize("B,D", [(6, 64), (3, 33), (2, 2052), (1100, 64)])
def test_embed_mse_of_equal_inputs_is_exactly_zero(lib, B, D):
    (x,) = H.rows(B, D, 1, D)
    out, grad = S.embed_mse_raw(dev(x), dev(x.clone()), grad_out=dev(torch.tensor([1.7])), want_grads=True)
    assert out.item() == 0.0 and (grad == 0).all()
    # one row differs: only that row has a gradient
    t = x.clone()
    t[B - 1] += 1.0
    out, grad = S.embed_mse_raw(dev(x), dev(t), want_grads=True)
    assert out.item() > 0 and (grad[:B - 1] == 0).all() and (grad[B - 1] != 0).all()


@pytest.mark.parametrize("D", [64, 33, 2052])
def test_margin_mse_cosine_with_zero_rows(lib, D):
    B = 6
    q, p, n = H.rows(B, D, 3, D + 1)
    q[0] = 0                        # a zero query: both cosines 0
    p[1] = 0                        # a zero positive
    n[2] = 0                        # a zero negative
    q[3] = 0; p[3] = 0; n[3] = 0    # all three
    y = torch.linspace(-0.8, 0.9, B)
    xs = f64((q, p, n))
    ref = DH.margin_mse_ref(*xs, y, H.COS_SIM, "none")
    ref.sum().backward()
    out, grads, margin = S.margin_mse_raw(dev(q), dev(p), dev(n), dev(y), H.COS_SIM, 0, want_grads=True, want_margin=True)
    assert margin[0].item() == 0.0 and margin[3].item() == 0.0
    _, drow = margin_bounds(q, p, n, y, H.COS_SIM)
    assert ((out.cpu().double() - ref.detach()).abs() <= drow).all()
    # torch's cosine gradients at a zero row are O(1 / eps): not compared there, only required to be finite
    check_grads(grads, xs, skip_rows=torch.tensor([True, True, True, True, False, False]))
    assert (grads[0][3] == 0).all() and (grads[1][3] == 0).all() and (grads[2][3] == 0).all()


# ------------------------------------------------------------------ 3. arguments
def test_bad_arguments_are_refused_and_nothing_is_written(lib):
    B, D = 4, 8
    x = torch.randn(B, D, device="cuda")
    y = torch.zeros(B, device="cuda")
    o = torch.full((B,), 7.0, device="cuda")
    mg = torch.full((B,), 7.0, device="cuda")
    s = torch.full((B,), 7.0, device="cuda")
    g = torch.full((B, D), 7.0, device="cuda")
    X, Y, O, M, Sc, G, st = x.data_ptr(), y.data_ptr(), o.data_ptr(), mg.data_ptr(), s.data_ptr(), g.data_ptr(), stream()
    em = lambda **k: lib.qst_embed_mse(*[k.get(nm, d) for nm, d in  # noqa: E731
                                         (("x", X), ("t", X), ("B", B), ("D", D), ("out", O), ("go", None), ("gx", G),
                                          ("sc", Sc), ("st", st))])
    mm = lambda **k: lib.qst_margin_mse_loss(*[k.get(nm, d) for nm, d in  # noqa: E731
                                               (("q", X), ("p", X), ("n", X), ("y", Y), ("B", B), ("D", D), ("sim", H.DOT),
                                                ("red", 2), ("out", O), ("mg", M), ("go", None), ("gq", G), ("gp", G),
                                                ("gn", G), ("sc", Sc), ("st", st))])
    for fn in (em, mm):
        assert fn(B=0) == BAD_ARG and fn(B=-3) == BAD_ARG and fn(D=0) == BAD_ARG and fn(D=-1) == BAD_ARG
        assert fn(out=None) == BAD_ARG and fn(sc=None) == BAD_ARG
    assert em(x=None) == BAD_ARG and em(t=None) == BAD_ARG
    assert mm(q=None) == BAD_ARG and mm(p=None) == BAD_ARG and mm(n=None) == BAD_ARG and mm(y=None) == BAD_ARG
    for sim in (-1, H.COS_DIST, H.L2, H.L1, H.L2_PLAIN, H.L1_PLAIN, 7):
        assert mm(sim=sim) == BAD_ARG
    assert mm(red=3) == BAD_ARG and mm(red=-1) == BAD_ARG and mm(red=1, sc=None) == BAD_ARG
    # some gradient pointers but not all
    assert mm(gq=None) == BAD_ARG and mm(gp=None, gn=None) == BAD_ARG and mm(gq=None, gp=None) == BAD_ARG
    torch.cuda.synchronize()
    assert (o == 7.0).all() and (mg == 7.0).all() and (s == 7.0).all() and (g == 7.0).all()
    # the same calls with good arguments go through
    assert em() == 0 and mm() == 0 and mm(sim=H.COS_SIM, red=0, sc=None, mg=None) == 0
    assert mm(gq=None, gp=None, gn=None) == 0 and em(gx=None) == 0


# ------------------------------------------------------------------ 4. the functions with autograd
def test_functions_with_autograd(lib):
    B, D = 12, 64
    q, p, n = [dev(t) for t in H.rows(B, D, 3, 21)]
    y = dev(torch.linspace(-1, 1, B))
    # (the function, the yardstick, the inputs that carry a gradient: the target of embed_mse does not)
    for fn, ref, with_grad in ((lambda a, b, c: S.embed_mse(a, b), lambda a, b, c: DH.embed_mse_ref(a, b), (0,)),
                               (lambda a, b, c: S.margin_mse(a, b, c, y, S.METRIC_COS_SIM, "sum"),
                                lambda a, b, c: DH.margin_mse_ref(a, b, c, y, H.COS_SIM, "sum"), (0, 1, 2)),
                               (lambda a, b, c: (util.pairwise_dot_score(a, b) - util.pairwise_cos_sim(a, c)).sum(),
                                lambda a, b, c: (DH.sim_ref(a, b, H.DOT) - DH.sim_ref(a, c, H.COS_SIM)).sum(), (0, 1, 2))):
        xs = [t.clone().requires_grad_(True) for t in (q, p, n)]
        xr = [t.double().clone().requires_grad_(True) for t in (q, p, n)]
        out, want = fn(*xs) * 1.7, ref(*xr) * 1.7
        out.backward()
        want.backward()
        torch.testing.assert_close(out.double(), want, rtol=1e-5, atol=1e-5)
        for k, (a, b) in enumerate(zip(xs, xr)):
            if k in with_grad:
                torch.testing.assert_close(a.grad.double(), b.grad, rtol=1e-4, atol=1e-6)
            else:
                assert a.grad is None
    assert util.pairwise_dot_score(q, p).shape == (B,) and util.pairwise_cos_sim(q, p).shape == (B,)


# ------------------------------------------------------------------ 5. the classes
WORDS = "a man rides red horse two dogs play in park woman eats green apple near old bridge small cat sleeps".split()


def sent(i, n):
    rng = np.random.RandomState(i)
    return " ".join(rng.choice(WORDS, size=n))


def triplet_texts(n):
    return [[sent(i, 9), sent(i, 9) + " now", sent(1000 + i, 5 + i % 7)] for i in range(n)]


@pytest.fixture(scope="module")
def model():
    return SentenceTransformer("tiny-bert", device="cuda")


@pytest.fixture(scope="module")
def teacher():
    return SentenceTransformer("tiny-bert", device="cuda", seed=15)


def teacher_margins(teacher, rows):
    """The teacher's own dot-score margins of (query, positive, negative) rows, as floats."""
    q, p, n = [np.asarray(teacher.encode([r[k] for r in rows], batch_size=16), dtype=np.float64) for k in range(3)]
    return ((q * p).sum(1) - (q * n).sum(1)).tolist()


class TorchOpLoss(nn.Module):
    """The same objective with the loss written in torch ops on the embeddings (the yardstick functions, fp32 on the GPU):
    what a user had to write before the kernels existed. Shares the encoder pass rule with the class under test."""

    def __init__(self, model, fn):
        super().__init__()
        self.model, self.fn = model, fn

    def forward(self, feats, labels):
        return self.fn(*encode_columns_fused(self.model, list(feats)), labels)


CLASS_CASES = {
    "mse": (lambda m, **k: S.MSELoss(m), lambda x, t: DH.embed_mse_ref(x, t)),
    "margin_dot": (lambda m, **k: S.MarginMSELoss(m, **k), lambda q, p, n, y: DH.margin_mse_ref(q, p, n, y, H.DOT)),
    "margin_cos": (lambda m, **k: S.MarginMSELoss(m, similarity_fct=util.pairwise_cos_sim, **k),
                   lambda q, p, n, y: DH.margin_mse_ref(q, p, n, y, H.COS_SIM)),
}

# Relative L2 difference of the gradient arena, per parameter tensor, between a class and the torch-op path on the same
# model (the bf16 backward re-rounds activations that depend on grad_emb, so no bound can be derived in advance): measured
# on an MI355X over the three classes (profiles/distill_parity.txt) and asserted at x 1.25 (README "Parity"). The key
# biases are set aside: their exact gradient is zero, what the arena holds there is the backward's rounding residue
# (test_gpu_tuple_losses), and the figure would compare two residues.
#   margin_dot 6.103e-4, margin_cos 5.309e-4: the same in four processes, both at encoder.layer.0.attention.self.key.weight
#   mse 7.7e-8 .. 1.3e-7, another figure every run -- and no larger than what the torch-op path differs from ITSELF by
#   between two runs in one process (9e-8 .. 2.3e-7 here; 3e-7 is the largest the project has recorded,
#   test_gpu_tuple_losses): MSELoss hands the backward the same gradient to the last bit or two, and what is left is the
#   backward's run-to-run noise. That noise floor is what its figure is held to.
GRAD_REL_MEASURED_NO_KEY_BIAS = {"mse": 1.343e-7, "margin_dot": 6.103e-4, "margin_cos": 5.309e-4}
GRAD_REL_RUN_TO_RUN = 3e-7          # two runs of the torch-op path itself
GRAD_REL_SANITY = 1.65e-2           # the bf16 path's bound against the oracle: at or above it is a bug, not rounding


def grad_rel(gh, gt):
    """(max over all tensors but the key biases, max over every tensor, name of the worst of the former)."""
    rel = {k: ((gh[k] - gt[k]).norm() / gt[k].norm()).item() for k in gt if gt[k].norm().item() > 0}
    rest = {k: v for k, v in rel.items() if "key.bias" not in k}
    worst = max(rest, key=rest.get)
    return rest[worst], max(rel.values()), worst


def one_backward(model, lm, feats, labels):
    enc = model._enc
    enc.ensure_train_state()
    enc.grads.zero_()
    seen = []
    hook = model.register_forward_hook(lambda mod, args, out: seen.append(out["sentence_embedding"].detach().clone()))
    try:
        loss = lm([dict(f) for f in feats], labels)
    finally:
        hook.remove()
    loss.backward()
    g = {k: v.clone() for k, v in enc.grad_views().items()}
    enc.grads.zero_()
    return loss.detach(), g, seen


def class_batch(model, teacher, name):
    if name == "mse":
        texts = [sent(i, 5 + i % 6) for i in range(16)]
        batch = [InputExample(texts=[s], label=e) for s, e in zip(texts, teacher.encode(texts, batch_size=16))]
    else:
        rows = triplet_texts(16)
        batch = [InputExample(texts=r, label=y) for r, y in zip(rows, teacher_margins(teacher, rows))]
    feats, labels = model.smart_batching_collate(batch)
    return [{k: v.cuda() for k, v in f.items()} for f in feats], labels.cuda()


def class_bound(name, embs, labels, ref):
    """The kernel tests' bound of the class's value, on the embeddings its own encoder pass produced."""
    if name == "mse":
        return mse_rel_bound(embs[0].shape[1]) * ref
    sim = H.DOT if name == "margin_dot" else H.COS_SIM
    _, drow = margin_bounds(*embs, labels, sim)
    return reduced_bound(drow, torch.tensor(ref), 2).item()


@pytest.mark.parametrize("name", sorted(CLASS_CASES))
def test_class_equals_torch_ops_on_the_same_model(model, teacher, name):
    make, fn = CLASS_CASES[name]
    feats, labels = class_batch(model, teacher, name)
    assert labels.shape == ((16, model.get_sentence_embedding_dimension()) if name == "mse" else (16,))
    model.train()
    lt, gt, emb_t = one_backward(model, TorchOpLoss(model, fn), feats, labels)
    _, gt2, _ = one_backward(model, TorchOpLoss(model, fn), feats, labels)
    lh, gh, emb_h = one_backward(model, make(model), feats, labels)
    assert lt.item() != 0.0 and len(emb_h) == 1 and len(emb_t) == 1
    # the value, against the objective in fp64 on the embeddings the class's own encoder pass produced
    embs = [e.cpu() for e in emb_h[0].split(16, 0)]
    ref = fn(*[e.double() for e in embs], labels.cpu().double()).item()
    bound = class_bound(name, embs, labels.cpu(), ref)
    print(f"  {name}: loss hip {lh.item():.9f} torch ops {lt.item():.9f} fp64 {ref:.9f}; |hip - fp64| = "
          f"{abs(lh.item() - ref):.3e}, bound {bound:.3e}")
    assert abs(lh.double().item() - ref) <= bound
    # ... and the torch-op path in fp32 sees the same embeddings and lands as close
    assert torch.equal(emb_h[0], emb_t[0])
    assert abs(lt.double().item() - ref) <= bound
    no_kb, every, worst = grad_rel(gh, gt)
    print(f"  {name}: gradient arena, relative L2 difference per tensor: without the key biases {no_kb:.3e} at {worst}; "
          f"every tensor {every:.3e}; the torch-op path against its own second run {grad_rel(gt2, gt)[0]:.3e}")
    assert no_kb < GRAD_REL_SANITY
    assert no_kb <= 1.25 * max(GRAD_REL_MEASURED_NO_KEY_BIAS[name], GRAD_REL_RUN_TO_RUN)


@pytest.mark.parametrize("name", ["margin_cos", "margin_dot"])
def test_margin_mse_fused_pass_equals_one_pass_per_column(model, teacher, name):
    make = CLASS_CASES[name][0]
    feats, labels = class_batch(model, teacher, name)
    model.train()
    lk, gk, emb_k = one_backward(model, make(model, fused=False), feats, labels)
    l1, g1, emb_1 = one_backward(model, make(model, fused=True), feats, labels)
    assert len(emb_k) == 3 and len(emb_1) == 1
    flat = lambda g: torch.cat([t.reshape(-1) for t in g.values()])  # noqa: E731
    assert abs(lk.item() - l1.item()) < 2e-4
    assert (flat(gk) - flat(g1)).norm().item() <= 2e-2 * flat(g1).norm().item()


def test_mse_loss_refuses_labels_of_another_shape(model, teacher):
    feats, labels = class_batch(model, teacher, "mse")
    D = model.get_sentence_embedding_dimension()
    with torch.no_grad():
        with pytest.raises(ValueError, match=rf"\(16, {D}\).*\(16, {D - 1}\)"):
            S.MSELoss(model)([dict(f) for f in feats], labels[:, :D - 1].contiguous())
        with pytest.raises(ValueError, match=rf"\(16, {D}\).*\(16,\)"):
            S.MSELoss(model)([dict(f) for f in feats], labels[:, 0].contiguous())


def test_a_callable_similarity_fct_runs_in_torch(model, teacher):
    """A similarity that is not one of util's two pairwise functions is called on the embeddings as given."""
    feats, labels = class_batch(model, teacher, "margin_dot")
    model.train()
    seen = []

    def neg_sq_l2(x, y):
        seen.append(x.shape)
        return -(x - y).pow(2).sum(1)

    with torch.no_grad():
        got = S.MarginMSELoss(model, similarity_fct=neg_sq_l2)([dict(f) for f in feats], labels)
        q, p, n = [model(dict(f))["sentence_embedding"] for f in feats]
        ref = ((neg_sq_l2(q, p) - neg_sq_l2(q, n) - labels) ** 2).mean()
        member = S.MarginMSELoss(model, similarity_fct=util.pairwise_dot_score)([dict(f) for f in feats], labels)
        direct = ((util.pairwise_dot_score(q, p) - util.pairwise_dot_score(q, n) - labels) ** 2).mean()
    assert len(seen) == 4
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=2e-4)
    torch.testing.assert_close(member, direct, rtol=1e-4, atol=2e-4)


# ------------------------------------------------------------------ 6. fit
class RecordLoss(nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, []

    def forward(self, feats, labels):
        loss = self.inner(feats, labels)
        self.seen.append(loss.detach())
        return loss


def fit_and_check(m, dl, lm, use_amp, what):
    m.fit([(dl, lm)], epochs=5, warmup_steps=0, scheduler="constantlr", optimizer_params={"lr": 1e-3}, dropout=0,
          use_amp=use_amp, show_progress_bar=False)
    seen = torch.stack(lm.seen).cpu()
    assert len(seen) == 20
    print(f"  fit {what} amp={use_amp}: first 5 {seen[:5].mean().item():.6f} last 5 {seen[-5:].mean().item():.6f}")
    assert torch.isfinite(seen).all() and seen[-5:].mean() < seen[:5].mean()
    assert torch.isfinite(m._enc.params).all()


@pytest.mark.parametrize("use_amp", [False, True])
@pytest.mark.parametrize("source", ["dataset", "prebuilt"])
def test_fit_distils_the_teachers_embeddings(teacher, source, use_amp):
    m = SentenceTransformer("tiny-bert", device="cuda")          # a fresh student: amp schedule counters persist per model
    texts = [sent(i, 4 + i % 8) for i in range(64)]
    assert len(set(texts)) == 64
    if source == "dataset":
        data = ParallelSentencesDataset(m, teacher, batch_size=16)
        data.add_dataset([[s] for s in texts], weight=64)
        assert len(data) == 64
    else:
        # labels as device tensors: they are stacked on the device
        data = [InputExample(texts=[s], label=e) for s, e in zip(texts, teacher.encode(texts, convert_to_tensor=True))]
        assert m.smart_batching_collate(data[:3])[1].is_cuda
    ev = MSEEvaluator(texts, texts, teacher_model=teacher, batch_size=16)
    before = ev(m)
    fit_and_check(m, DataLoader(data, batch_size=16, shuffle=False), RecordLoss(S.MSELoss(m)), use_amp, f"mse {source}")
    after = ev(m)
    print(f"  MSEEvaluator: before {before:.6f} after {after:.6f}")
    assert after > before


@pytest.mark.parametrize("use_amp", [False, True])
def test_fit_lowers_the_margin_mse_loss(teacher, use_amp):
    m = SentenceTransformer("tiny-bert", device="cuda")
    rows = triplet_texts(64)
    data = [InputExample(texts=r, label=y) for r, y in zip(rows, teacher_margins(teacher, rows))]
    fit_and_check(m, DataLoader(data, batch_size=16, shuffle=False), RecordLoss(S.MarginMSELoss(m)), use_amp, "margin mse")


# ------------------------------------------------------------------ 7. the evaluators
def test_mse_evaluator(model, teacher, tmp_path):
    src = [sent(i, 4 + i % 7) for i in range(50)]
    trg = [s + " now" for s in src]
    ev = MSEEvaluator(src, trg, teacher_model=teacher, batch_size=16, name="dev")
    model.eval()
    t64 = np.asarray(teacher.encode(src, batch_size=16), dtype=np.float64)
    s64 = np.asarray(model.encode(trg, batch_size=16), dtype=np.float64)
    ref = ((t64 - s64) ** 2).mean() * 100
    assert ev(model) == -ev.mse(model) and os.listdir(tmp_path) == []      # nothing is written without output_path
    got = ev(model, output_path=str(tmp_path), epoch=2, steps=30)
    print(f"  MSEEvaluator: {-got:.9f} (fp64 {ref:.9f})")
    assert abs(-got - ref) <= mse_rel_bound(s64.shape[1]) * ref            # the factor 100 is applied in double
    assert MSEEvaluator(src, trg, teacher_model=teacher, name="dev", write_csv=False)(model, output_path=str(tmp_path)) == got
    ev(model, output_path=str(tmp_path), epoch=3, steps=-1)
    assert os.listdir(tmp_path) == ["mse_evaluation_dev_results.csv"]
    with open(tmp_path / "mse_evaluation_dev_results.csv") as f:
        table = list(csv.reader(f))
    assert table[0] == ["epoch", "steps", "MSE"] and len(table) == 3
    assert table[1][:2] == ["2", "30"] and table[2][:2] == ["3", "-1"] and float(table[1][2]) == -got


def test_translation_evaluator(model, tmp_path):
    src = [sent(i, 5 + i % 6) for i in range(40)]
    trg = [s + " today" if i % 4 else sent(3000 + i, 6) for i, s in enumerate(src)]     # every fourth is no translation
    assert len(set(src)) == 40 and len(set(trg)) == 40
    model.eval()
    e1, e2 = model.encode(src, batch_size=16), model.encode(trg, batch_size=16)
    cos = DH.cos_matrix(e1, e2)
    # a condition on the test data: the best and the second-best score of every row and column are further apart than five
    # times the error the project accepts on a cosine, so that fp32 and fp64 cannot rank them differently
    for c in (cos, cos.T):
        top2 = np.sort(c, axis=1)[:, -2:]
        assert (top2[:, 1] - top2[:, 0]).min() > 5 * H.value_tol(H.COS_SIM, e1.shape[1])
    want = np.arange(40)
    ref12, ref21 = float(np.mean(cos.argmax(1) == want)), float(np.mean(cos.argmax(0) == want))
    assert 0.0 < ref12 < 1.0 and 0.0 < ref21 < 1.0         # the data holds matches and mismatches
    ev = TranslationEvaluator(src, trg, batch_size=16, name="dev")
    assert ev.accuracies(model) == (ref12, ref21)
    assert ev(model) == (ref12 + ref21) / 2 and os.listdir(tmp_path) == []
    got = ev(model, output_path=str(tmp_path), epoch=1, steps=7)
    assert got == (ref12 + ref21) / 2
    assert TranslationEvaluator(src, trg, write_csv=False)(model, output_path=str(tmp_path)) == got
    assert os.listdir(tmp_path) == ["translation_evaluation_dev_results.csv"]
    with open(tmp_path / "translation_evaluation_dev_results.csv") as f:
        table = list(csv.reader(f))
    assert table[0] == ["epoch", "steps", "src2trg", "trg2src"] and len(table) == 2
    assert table[1][:2] == ["1", "7"] and [float(v) for v in table[1][2:]] == [ref12, ref21]
    s2t, t2s = translation_matches(torch.from_numpy(e1).cuda(), torch.from_numpy(e2).cuda())
    assert np.array_equal(s2t.cpu().numpy(), cos.argmax(1)) and np.array_equal(t2s.cpu().numpy(), cos.argmax(0))


def test_translation_matches_picks_the_lowest_index_among_equal_scores(lib):
    g = torch.Generator().manual_seed(5)
    a = torch.randn(12, 64, generator=g)
    b = a + 0.01 * torch.randn(12, 64, generator=g)      # target i is the translation of source i
    b[7] = b[2]; b[9] = b[2]            # bit-identical target rows: every source scores them equally
    a[5] = a[1]; a[11] = a[1]           # ... and bit-identical source rows
    cos = DH.cos_matrix(a, b)
    # np.argmax, on a matrix in which the scores of bit-identical rows are made bit-identical too (a BLAS may compute the
    # columns of one product along different paths)
    cos[:, 7] = cos[:, 2]; cos[:, 9] = cos[:, 2]
    cos[5] = cos[1]; cos[11] = cos[1]
    s2t, t2s = translation_matches(a.cuda(), b.cuda())
    assert s2t.dtype == torch.int64 and s2t.shape == (12,) and t2s.shape == (12,)
    assert np.array_equal(s2t.cpu().numpy(), cos.argmax(1)) and np.array_equal(t2s.cpu().numpy(), cos.argmax(0))
    assert s2t[2].item() == 2 and t2s[1].item() == 1
    # the duplicates are among the winners, so the rule was exercised: never the later copy
    assert 2 in s2t.tolist() and 7 not in s2t.tolist() and 9 not in s2t.tolist()
    assert 1 in t2s.tolist() and 5 not in t2s.tolist() and 11 not in t2s.tolist()
