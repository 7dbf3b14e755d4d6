"""GPU: the batch-mining triplet losses -- qst_batch_triplet_loss (csrc/batch_triplet.hip), its autograd, the four loss
classes of st_losses.py and SentenceLabelDataset -- against the yardstick in batch_triplet_helpers: sentence-transformers
2.2.2's formulas in torch ops, fp64 on the CPU with autograd, on inputs in which every mining decision is at least 1e-5 from
flipping. Tolerances are the project's: the value within rtol = atol = max(1e-5, 1.5e-8 D), gradients within rtol 1e-4,
atol 1e-6 * max(1, max |reference gradient|); counts exactly."""
import math

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import batch_triplet_helpers as T  # noqa: E402
from kernel_helpers import lib, ptr, stream  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import data, st_losses as S  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, SentenceTransformer  # noqa: E402
from test_gpu_tuple_losses import sent  # noqa: E402  (the word salad the other loss tests train the tiny encoder on)

KM = [(k, m) for k in T.KINDS for m in T.METRICS]
KM_IDS = [f"{T.KIND_NAMES[k]}-{T.METRIC_NAMES[m]}" for k, m in KM]
CLASSES = {T.HARD: S.BatchHardTripletLoss, T.SOFT: S.BatchHardSoftMarginTripletLoss, T.SEMI: S.BatchSemiHardTripletLoss,
           T.ALL: S.BatchAllTripletLoss}
DF = S.BatchHardTripletLossDistanceFunction
DIST = {T.EUCLID: DF.eucledian_distance, T.COS: DF.cosine_distance}


def call(lib, x, labels, kind, metric, margin=None, grad_out=None, want_grads=True):
    """lib.qst_batch_triplet_loss on device tensors: (loss [1], counts int64 [2], grad [B, D] or None)."""
    B, D = x.shape
    margin = T.MARGIN[metric] if margin is None else margin
    out = torch.full((1,), -7.0, device="cuda")
    counts = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    grad = torch.full_like(x, -7.25) if want_grads else None
    nbytes = lib.qst_batch_triplet_workspace_bytes(B, D)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.qst_batch_triplet_loss(ptr(x), ptr(labels), B, D, kind, metric, margin, ptr(out), ptr(counts), ptr(grad_out),
                                    ptr(grad), ptr(ws), nbytes, stream())
    assert rc == 0
    return out, counts, grad


def check(got, want, metric, D, what):
    """Prints every figure as a share of its tolerance, then asserts: value, counts, gradient."""
    (out, counts, grad), (loss, ref_grad, ref_counts) = got, want
    ev = T.value_error(out.item(), loss, metric, D)
    eg = T.grad_error(grad.cpu(), ref_grad)
    print(f"  {what}: loss {out.item():.7f} ref {loss.item():.7f} counts {counts.tolist()} ref {list(ref_counts)}; share of "
          f"the tolerance: value {ev:.3f} grad {eg:.3f}")
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()
    assert counts.tolist() == list(ref_counts)
    assert ev <= 1.0 and eg <= 1.0


# ------------------------------------------------------------------ 1. kernel parity
PARITY = [(k, m, B, D) for k, m in KM for (B, D) in T.shapes_of(k)]


@pytest.mark.parametrize("kind,metric,B,D", PARITY,
                         ids=[f"{T.KIND_NAMES[k]}-{T.METRIC_NAMES[m]}-{B}x{D}" for k, m, B, D in PARITY])
def test_kernel_matches_reference(lib, kind, metric, B, D):
    x, labels, loss, grad, counts, _ = T.reference(B, D, kind, metric)
    xd, ld = x.cuda(), labels.cuda()
    got = call(lib, xd, ld, kind, metric)
    check(got, (loss, grad, counts), metric, D, f"{B}x{D} {T.KIND_NAMES[kind]} {T.METRIC_NAMES[metric]}")
    # the forward-only call writes the same loss and counts
    fwd, fcounts, none = call(lib, xd, ld, kind, metric, want_grads=False)
    assert none is None and torch.equal(fwd, got[0]) and torch.equal(fcounts, got[1])


@pytest.mark.parametrize("metric", T.METRICS, ids=[T.METRIC_NAMES[m] for m in T.METRICS])
@pytest.mark.parametrize("kind", T.BIG_KINDS, ids=[T.KIND_NAMES[k] for k in T.BIG_KINDS])
def test_rows_longer_than_one_staged_chunk(lib, kind, metric):
    """B = 1030: the row of distances goes through LDS in two chunks, positives and selected negatives sit in both, and
    every 256-thread loop and the 1024-thread finish make more than one trip."""
    x, labels, loss, grad, counts = T.big_reference(kind, metric)
    got = call(lib, x.cuda(), labels.cuda(), kind, metric)
    check(got, (loss, grad, counts), metric, T.BIG[1], f"{T.BIG} {T.KIND_NAMES[kind]} {T.METRIC_NAMES[metric]}")


# ------------------------------------------------------------------ 2. the call itself
def test_two_identical_calls_are_bit_identical(lib):
    for (B, D) in [(130, 64), (33, 768), (5, 10)]:
        for kind, metric in KM:
            x, labels = [t.cuda() for t in T.case(B, D, T.seed_of(B, D, 0))]
            w = torch.tensor([1.7], device="cuda")
            a = call(lib, x, labels, kind, metric, grad_out=w)
            b = call(lib, x, labels, kind, metric, grad_out=w)
            assert all(torch.equal(p, q) for p, q in zip(a, b)), (B, D, kind, metric)


@pytest.mark.parametrize("kind,metric", KM, ids=KM_IDS)
def test_grad_out_scales_the_finished_gradient(lib, kind, metric):
    """grad_out = 65536 (the loss scale of use_amp, read on the device) gives 65536 x the gradients of grad_out = NULL bit
    for bit -- a power of two scales exactly -- and the loss does not move."""
    x, labels = [t.cuda() for t in T.case(65, 384, T.seed_of(65, 384, 0))]
    o1, c1, g1 = call(lib, x, labels, kind, metric)
    o2, c2, g2 = call(lib, x, labels, kind, metric, grad_out=torch.tensor([65536.0], device="cuda"))
    assert torch.equal(o1, o2) and torch.equal(c1, c2)
    assert g1.abs().max().item() > 0 and torch.equal(g2, g1 * 65536.0)


@pytest.mark.parametrize("kind,metric", KM, ids=KM_IDS)
def test_edge_batches(lib, kind, metric):
    """(8, 32), value only: a label that occurs once; all labels equal (hard and soft follow the formula, all gives 0, semi
    falls back on the diagonal); all labels distinct (all gives 0, semi NaN); two bit-identical rows of one label (euclid:
    their distance is 0, the loss and every gradient finite)."""
    D = 32
    for name, (x, labels) in T.edge_cases().items():
        loss, _, counts = T.reference_of(x, labels, kind, metric)
        out, got_counts, grad = call(lib, x.cuda(), labels.cuda(), kind, metric)
        print(f"  {name} {T.KIND_NAMES[kind]} {T.METRIC_NAMES[metric]}: loss {out.item():.7f} ref {loss.item():.7f} "
              f"counts {got_counts.tolist()}")
        if math.isnan(loss.item()):
            assert name == "all_distinct" and kind == T.SEMI and torch.isnan(out).all()
        else:
            assert T.value_error(out.item(), loss, metric, D) <= 1.0
        if kind == T.ALL and name in ("all_equal", "all_distinct"):
            assert out.item() == 0.0 and got_counts.tolist() == [0, 0] and not grad.any()
        if name == "all_equal" and kind == T.HARD:
            assert abs(out.item() - T.MARGIN[metric]) <= 2 * T.value_tol(metric, D)
        if name != "duplicate_rows":                    # (a distance of exactly 0 sits on the hinge of `d > 0` decisions)
            assert got_counts.tolist() == list(counts)
        if name == "duplicate_rows" and metric == T.EUCLID:
            assert torch.isfinite(out).all() and torch.isfinite(grad).all()


def test_the_call_pair_is_capturable_in_a_graph(lib):
    """No host synchronisation, grad_out read on the device: a captured forward + backward call pair replays twice with
    equal outputs, and on new inputs written into the same buffers."""
    (x1, l1), (x2, l2) = [[t.cuda() for t in T.case(33, 768, T.seed_of(33, 768, k))] for k in (0, 1)]
    x, labels, w = x1.clone(), l1.clone(), torch.tensor([1.0], device="cuda")
    for kind, metric in KM:                             # code objects loaded before the capture
        S.batch_triplet_loss_raw(x, labels, kind, metric, 0.1, grad_out=w, want_grads=True)
    torch.cuda.synchronize()
    for kind, metric in ((T.SEMI, T.COS), (T.ALL, T.EUCLID)):
        x.copy_(x1), labels.copy_(l1), w.fill_(1.0)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fwd, _, _ = S.batch_triplet_loss_raw(x, labels, kind, metric, 0.1)
            out, grad, counts = S.batch_triplet_loss_raw(x, labels, kind, metric, 0.1, grad_out=w, want_grads=True)
        graph.replay()
        torch.cuda.synchronize()
        first = (fwd.clone(), out.clone(), grad.clone(), counts.clone())
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, (fwd, out, grad, counts)))
        want = S.batch_triplet_loss_raw(x1, l1, kind, metric, 0.1, want_grads=True)
        assert torch.equal(out, want[0]) and torch.equal(grad, want[1]) and torch.equal(counts, want[2])
        x.copy_(x2), labels.copy_(l2), w.fill_(2.5)
        graph.replay()
        torch.cuda.synchronize()
        want = S.batch_triplet_loss_raw(x2, l2, kind, metric, 0.1, grad_out=torch.tensor([2.5], device="cuda"), want_grads=True)
        assert torch.equal(fwd, want[0]) and torch.equal(out, want[0]) and torch.equal(grad, want[1])


# ------------------------------------------------------------------ 3. autograd
@pytest.mark.parametrize("kind,metric", KM, ids=KM_IDS)
def test_functional_autograd_returns_the_raw_gradient_in_the_input_dtype(lib, kind, metric):
    x0, labels = [t.cuda() for t in T.case(8, 384, T.seed_of(8, 384, 0))]
    x0 = x0.to(torch.bfloat16)
    x = x0.clone().requires_grad_(True)
    loss = S.batch_triplet_loss(x, labels, kind, metric, 0.1)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (loss * 1.5).backward()
    assert x.grad.dtype == torch.bfloat16
    out, grad, _ = S.batch_triplet_loss_raw(x0.float(), labels, kind, metric, 0.1, grad_out=torch.tensor([1.5], device="cuda"),
                                            want_grads=True)
    assert torch.equal(loss.detach().reshape(1), out) and torch.equal(x.grad, grad.to(torch.bfloat16))
    assert x.grad.float().abs().max().item() > 0


# ------------------------------------------------------------------ 4. the classes on a real encoder
def labelled_examples(n_labels, per_label):
    """One text and one integer label per example; the texts of a label share their first five words."""
    return [InputExample(texts=[sent(lab, 5) + " " + sent(100 + 10 * lab + i, 2 + i % 3)], label=lab)
            for lab in range(n_labels) for i in range(per_label)]


@pytest.fixture(scope="module")
def model():
    return SentenceTransformer("tiny-bert", device="cuda")


@pytest.mark.parametrize("kind,metric", KM, ids=KM_IDS)
def test_an_untagged_callable_mines_in_torch_and_agrees_with_the_kernels(model, kind, metric):
    feats, labels = model.smart_batching_collate(labelled_examples(4, 4))
    feats, labels = [{k: v.cuda() for k, v in f.items()} for f in feats], labels.cuda()
    model.eval()
    seen = []

    def foreign(e):
        seen.append(tuple(e.shape))
        return DIST[metric](e)

    kw = {} if kind == T.SOFT else {"margin": 0.1}
    with torch.no_grad():
        got = CLASSES[kind](model, distance_metric=foreign, **kw)([dict(f) for f in feats], labels)
        want = CLASSES[kind](model, distance_metric=DIST[metric], **kw)([dict(f) for f in feats], labels)
    D = model.get_sentence_embedding_dimension()
    print(f"  {T.KIND_NAMES[kind]} {T.METRIC_NAMES[metric]}: torch route {got.item():.7f} kernels {want.item():.7f}")
    assert seen == [(16, D)] and want.item() > 0
    assert T.value_error(got.item(), want.item(), metric, D) <= 1.0


@pytest.mark.parametrize("kind,use_amp", [(k, False) for k in T.KINDS] + [(T.SEMI, True)],
                         ids=[T.KIND_NAMES[k] for k in T.KINDS] + ["semi-amp"])
def test_fit_trains_from_sentence_label_dataset(kind, use_amp):
    """6 steps of fit() fed by DataLoader(SentenceLabelDataset(samples_per_label=2), batch_size=8): every loss is finite and
    the parameters move; under use_amp the loss scale reaches the kernels as grad_out, a device scalar."""
    np.random.seed(5)
    m = SentenceTransformer("tiny-bert", device="cuda")          # a fresh model: amp schedule counters persist per model
    lm = CLASSES[kind](m)
    seen = []
    lm.register_forward_hook(lambda mod, args, out: seen.append(out.detach().float().cpu()))
    ds = data.SentenceLabelDataset(labelled_examples(6, 4), samples_per_label=2)
    dl = DataLoader(ds, batch_size=8)
    assert len(dl) == 3
    before = m._enc.params.clone()
    m.fit([(dl, lm)], epochs=2, warmup_steps=0, scheduler="constantlr", optimizer_params={"lr": 1e-3}, dropout=0,
          use_amp=use_amp, show_progress_bar=False)
    losses = torch.stack(seen)
    print(f"  fit {T.KIND_NAMES[kind]} amp={use_amp}: losses {[round(v, 5) for v in losses.tolist()]}")
    assert len(seen) == 6 and torch.isfinite(losses).all() and (losses > 0).all()
    assert torch.isfinite(m._enc.params).all() and (m._enc.params != before).any()
