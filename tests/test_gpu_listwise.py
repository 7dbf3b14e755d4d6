"""GPU: listwise distillation (csrc/listwise.hip: qst_listwise_distill_loss), its autograd function, DistillKLDivLoss and
MarginMSELoss with several negatives on top of it (st_losses.py) and fit() on list labels, against the yardstick and the
a-priori bounds in listwise_helpers: the formulas in torch ops, fp64 on the CPU with autograd. Every element of every output
is held to its own bound; outputs sit between guard bands that must come back untouched."""
import numpy as np
import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import distill_helpers as DH  # noqa: E402
import listwise_helpers as LH  # noqa: E402
import tuple_loss_helpers as H  # noqa: E402
from listwise_helpers import BAD_ARG, CASES, KIND_NAMES, KL, MARGIN, SIMS, TEMPERATURES, UNSUPPORTED, kinds_of, worst  # noqa: E402
from tuple_loss_helpers import dev  # noqa: E402
from kernel_helpers import lib, ptr, stream  # noqa: E402,F401
from test_gpu_distill import GRAD_REL_SANITY, RecordLoss, grad_rel, one_backward, sent  # noqa: E402
from quadruplet_sentence_transformer_amd import st_losses as S, util  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, SentenceTransformer  # noqa: E402

GUARD, SENTINEL = 64, 7.0            # floats on either side of an output (256 bytes: 16-byte alignment is kept)


class Guarded:
    """An output of `n` floats between two guard bands filled with the sentinel, `shift` floats past 16-byte alignment."""

    def __init__(self, n, shift=0):
        self.n, self.lo = n, GUARD + shift
        self.buf = torch.full((self.lo + n + GUARD,), SENTINEL, device="cuda")

    @property
    def view(self):
        return self.buf[self.lo:self.lo + self.n]

    def ptr(self):
        return self.view.data_ptr()

    def written(self, upto=None):
        """The first `upto` floats (all by default) on the CPU, after checking that nothing else changed."""
        upto = self.n if upto is None else upto
        assert (self.buf[:self.lo] == SENTINEL).all() and (self.buf[self.lo + upto:] == SENTINEL).all(), "guard band overwritten"
        return self.view[:upto].cpu()


def shifted(t, shift):
    """t on the device, its first element `shift` floats past 16-byte alignment."""
    if not shift:
        return dev(t)
    buf = torch.empty(t.numel() + shift, device="cuda")
    buf[shift:] = t.reshape(-1).cuda()
    return buf[shift:].view(t.shape)


def run_kernel(lib, q, docs, y, kind, sim, T, red, w=None, grads=True, scores=True, shift=0):
    """One qst_listwise_distill_loss call by name on guarded outputs: dict(loss, scores, grad_q, grad_docs) on the CPU (None
    for what was not asked for). shift = 1 moves every row and gradient pointer one float off 16-byte alignment."""
    K, B, D = docs.shape
    qd, dd, yd = shifted(q, shift), shifted(docs, shift), dev(y)
    wd = None if w is None else dev(w)
    n_out = B if red == 0 else 1
    out, sc = Guarded(B), Guarded(B)
    so = Guarded(B * K) if scores else None
    gq, gd = (Guarded(B * D, shift), Guarded(K * B * D, shift)) if grads else (None, None)
    rc = lib.qst_listwise_distill_loss(ptr(qd), ptr(dd), ptr(yd), B, K, D, kind, sim, T, red, out.ptr(),
                                       so.ptr() if scores else None, ptr(wd), gq.ptr() if grads else None,
                                       gd.ptr() if grads else None, sc.ptr(), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    sc.written(0 if red == 0 else B)                      # the scratch rows are used by 'sum' / 'mean' only
    return {"loss": out.written(n_out).view(B if red == 0 else ()),
            "scores": so.written().view(B, K) if scores else None,
            "grad_q": gq.written().view(B, D) if grads else None,
            "grad_docs": gd.written().view(K, B, D) if grads else None}


def hold(got, ref, bd, what, keys=("loss", "scores", "grad_q", "grad_docs")):
    """Every element of every output within its bound; the gradients of an example with a clamped (zero) row only finite."""
    ok = ~bd["clamped"]
    ratios = {}
    for k in keys:
        g, r, b = got[k].double(), ref[k], bd[k]
        assert g.shape == r.shape == b.shape, (k, g.shape, r.shape, b.shape)
        assert torch.isfinite(g).all(), f"{what}: {k} is not finite"
        if k == "grad_q":
            g, r, b = g[ok], r[ok], b[ok]
        elif k == "grad_docs":
            g, r, b = g[:, ok], r[:, ok], b[:, ok]
        ratios[k] = worst(g, r, b)
    print(f"  {what}: max |d| / bound " + ", ".join(f"{k} {v:.3e}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)


# ------------------------------------------------------------------ 1. kernel parity
@pytest.mark.parametrize("B,K,D", CASES)
@pytest.mark.parametrize("sim", SIMS, ids=lambda m: H.METRIC_NAMES[m])
def test_kernel_matches_yardstick(lib, B, K, D, sim):
    for kind in kinds_of(K):
        for red in (0, 1, 2):
            q, docs, y, w, ref, bd = LH.case(B, K, D, kind, sim, 1.0, red, True)
            if kind == MARGIN:
                assert LH.residuals_hold(q, docs, y, sim)
            got = run_kernel(lib, q, docs, y, kind, sim, 1.0, red, w)
            hold(got, ref, bd, f"{KIND_NAMES[kind]} {H.METRIC_NAMES[sim]} {B}x{K}x{D} red {red}")
        # without grad_out and without out_scores; then forward only: the same value, nothing else written
        q, docs, y, _, ref, bd = LH.case(B, K, D, kind, sim, 1.0, 2, False)
        got = run_kernel(lib, q, docs, y, kind, sim, 1.0, 2, None, scores=False)
        hold(got, ref, bd, f"{KIND_NAMES[kind]} {H.METRIC_NAMES[sim]} {B}x{K}x{D} no grad_out", ("loss", "grad_q", "grad_docs"))
        fwd = run_kernel(lib, q, docs, y, kind, sim, 1.0, 2, None, grads=False)
        assert torch.equal(fwd["loss"], got["loss"])
        hold(fwd, ref, bd, f"{KIND_NAMES[kind]} {H.METRIC_NAMES[sim]} {B}x{K}x{D} forward only", ("loss", "scores"))


@pytest.mark.parametrize("sim", SIMS, ids=lambda m: H.METRIC_NAMES[m])
@pytest.mark.parametrize("T", TEMPERATURES)
def test_kl_temperatures(lib, sim, T):
    for B, K, D in ((4, 7, 384), (5, 63, 768), (3, 64, 2052)):
        q, docs, y, w, ref, bd = LH.case(B, K, D, KL, sim, T, 2, True)
        hold(run_kernel(lib, q, docs, y, KL, sim, T, 2, w), ref, bd, f"kl {H.METRIC_NAMES[sim]} {B}x{K}x{D} T {T}")


@pytest.mark.parametrize("sim", SIMS, ids=lambda m: H.METRIC_NAMES[m])
def test_a_pointer_one_float_off_alignment_takes_the_element_form(lib, sim):
    B, K, D = 5, 7, 384
    for kind in (KL, MARGIN):
        q, docs, y, w, ref, bd = LH.case(B, K, D, kind, sim, 1.0, 2, True)
        got = run_kernel(lib, q, docs, y, kind, sim, 1.0, 2, w, shift=1)
        hold(got, ref, bd, f"{KIND_NAMES[kind]} {H.METRIC_NAMES[sim]} {B}x{K}x{D} unaligned")


def test_margin_with_one_negative_agrees_with_the_pairwise_kernel(lib):
    """K = 2 is qst_margin_mse_loss's objective on the same rows: the two kernels within the sum of their bounds."""
    for B, D in ((3, 6), (67, 768), (3, 2050)):
        for sim in SIMS:
            for red in (0, 2):
                q, docs, y, w, ref, bd = LH.case(B, 2, D, MARGIN, sim, 1.0, red, True)
                got = run_kernel(lib, q, docs, y, MARGIN, sim, 1.0, red, w)
                pair, _, margin = S.margin_mse_raw(dev(q), dev(docs[0]), dev(docs[1]), dev(y[:, 0]), sim, red, grad_out=dev(w),
                                                   want_grads=True, want_margin=True)
                dm, drow = DH.margin_bounds(q, docs[0], docs[1], y[:, 0], sim)
                both = bd["loss"] + DH.reduced_bound(drow, ref["loss"], red)
                err = (got["loss"].double() - pair.cpu().double().view(got["loss"].shape)).abs()
                assert (err <= both).all(), (B, D, sim, red, err, both)
                merr = ((got["scores"][:, 0].double() - got["scores"][:, 1].double()) - margin.cpu().double()).abs()
                assert (merr <= dm + bd["scores"].sum(1)).all()


# ------------------------------------------------------------------ 2. numerically hard rows
@pytest.mark.parametrize("T", TEMPERATURES)
def test_scores_beyond_100_need_the_maximum_subtracted(lib, T):
    B, K, D = 3, 7, 2048
    g = torch.Generator().manual_seed(5)
    q, docs = 3 * torch.randn(B, D, generator=g), 3 * torch.randn(K, B, D, generator=g)
    y = LH.kl_labels(B, K, 6)
    s = LH.sims_ref(q.double(), docs.double(), H.DOT)
    assert (s.abs().max(1).values > 100).all() and (s.max(1).values / T > 89).any()      # exp of these overflows fp32
    w = LH.upstream(B, 2)
    ref, bd = LH.reference_of(q, docs, y, KL, H.DOT, T, 2, w), LH.bounds_of(q, docs, y, KL, H.DOT, T, 2, w)
    assert torch.isfinite(ref["loss"])
    hold(run_kernel(lib, q, docs, y, KL, H.DOT, T, 2, w), ref, bd, f"kl dot scores beyond 100, T {T}")


@pytest.mark.parametrize("sim", SIMS, ids=lambda m: H.METRIC_NAMES[m])
def test_teacher_weights_that_underflow_to_zero_count_zero(lib, sim):
    B, K, D = 5, 7, 384
    q, docs = LH.list_rows(B, K, D, 9)
    y = LH.kl_labels(B, K, 10)
    y[:, 2] -= 200.0                 # exp(-200) is 0 in fp32: xlogy's rule decides the term
    y[1, 0] += 200.0                 # one row whose every other weight underflows
    t32 = torch.softmax(y, 1)
    assert (t32[:, 2] == 0).all() and (t32[1, 1:] == 0).all()
    for red in (0, 2):
        w = LH.upstream(B, red)
        ref, bd = LH.reference_of(q, docs, y, KL, sim, 1.0, red, w), LH.bounds_of(q, docs, y, KL, sim, 1.0, red, w)
        got = run_kernel(lib, q, docs, y, KL, sim, 1.0, red, w)
        assert torch.isfinite(got["loss"]).all() and not torch.isnan(got["grad_q"]).any() and not torch.isnan(got["grad_docs"]).any()
        hold(got, ref, bd, f"kl {H.METRIC_NAMES[sim]} teacher 200 apart red {red}")


@pytest.mark.parametrize("sim", SIMS, ids=lambda m: H.METRIC_NAMES[m])
def test_identical_candidates(lib, sim):
    B, K, D = 5, 7, 768
    q, docs = LH.list_rows(B, K, D, 12)
    docs = docs[:1].repeat(K, 1, 1).contiguous()
    for kind in (KL, MARGIN):
        y = LH.labels_of(q, docs, kind, sim, 13)
        w = LH.upstream(B, 2)
        ref, bd = LH.reference_of(q, docs, y, kind, sim, 1.0, 2, w), LH.bounds_of(q, docs, y, kind, sim, 1.0, 2, w)
        got = run_kernel(lib, q, docs, y, kind, sim, 1.0, 2, w)
        assert (got["scores"] == got["scores"][:, :1]).all()          # the same row gives the same bits in every lane
        hold(got, ref, bd, f"{KIND_NAMES[kind]} {H.METRIC_NAMES[sim]} identical candidates")


@pytest.mark.parametrize("D", [384, 2052])
def test_a_zero_query_row_under_the_cosine(lib, D):
    B, K = 5, 7
    q, docs = LH.list_rows(B, K, D, 14)
    q[1] = 0                         # every cosine of the row is 0: the student's softmax is uniform
    for kind in (KL, MARGIN):
        y = LH.kl_labels(B, K, 15) if kind == KL else torch.linspace(-0.8, 0.9, B * (K - 1)).view(B, K - 1)
        ref, bd = LH.reference_of(q, docs, y, kind, H.COS_SIM, 1.0, 0), LH.bounds_of(q, docs, y, kind, H.COS_SIM, 1.0, 0)
        assert bd["clamped"].tolist() == [False, True, False, False, False]
        got = run_kernel(lib, q, docs, y, kind, H.COS_SIM, 1.0, 0)
        assert (got["scores"][1] == 0).all()
        # torch's cosine gradients at a zero row are O(1 / eps): finite is all that is asked of that example (hold), and the
        # norm passes none: what reaches the candidates through |q| = 0 is exactly 0
        hold(got, ref, bd, f"{KIND_NAMES[kind]} cos zero query D {D}")
        assert (got["grad_docs"][:, 1] == 0).all()


@pytest.mark.parametrize("sim", SIMS, ids=lambda m: H.METRIC_NAMES[m])
@pytest.mark.parametrize("B,D", [(1, 4), (5, 384), (3, 2050)])
def test_kl_of_one_candidate_is_exactly_zero(lib, B, D, sim):
    q, docs = LH.list_rows(B, 1, D, 16)
    y = LH.kl_labels(B, 1, 17)
    for red in (0, 1, 2):
        got = run_kernel(lib, q, docs, y, KL, sim, 0.5, red, LH.upstream(B, red))
        assert (got["loss"] == 0).all() and (got["grad_q"] == 0).all() and (got["grad_docs"] == 0).all()
        assert worst(got["scores"], LH.sims_ref(q.double(), docs.double(), sim), LH.score_bounds(q, docs, sim)) <= 1.0


# ------------------------------------------------------------------ 3. determinism, the upstream factor, arguments
def test_two_identical_calls_are_bit_identical(lib):
    for B, K, D in ((67, 64, 384), (5, 63, 768), (4, 7, 2052), (3, 2, 2050)):
        for kind, sim, red in ((KL, H.DOT, 2), (KL, H.COS_SIM, 0), (MARGIN, H.COS_SIM, 1), (MARGIN, H.DOT, 2)):
            q, docs, y, w, _, _ = LH.case(B, K, D, kind, sim, 1.0, red, True)
            a = run_kernel(lib, q, docs, y, kind, sim, 1.0, red, w)
            b = run_kernel(lib, q, docs, y, kind, sim, 1.0, red, w)
            assert all(torch.equal(a[k], b[k]) for k in a)


def test_the_upstream_gradient_multiplies_the_finished_gradient(lib):
    """grad_out = g gives g x (the gradients without), rounded once: the product of two fp32 numbers is exact in double."""
    for B, K, D in ((4, 7, 384), (5, 7, 2048), (4, 7, 2052), (3, 2, 6)):
        for kind in (KL, MARGIN):
            for sim in SIMS:
                for red in (0, 1, 2):
                    q, docs, y, w, _, _ = LH.case(B, K, D, kind, sim, 1.0, red, True)
                    base = run_kernel(lib, q, docs, y, kind, sim, 1.0, red, None)
                    got = run_kernel(lib, q, docs, y, kind, sim, 1.0, red, w)
                    wd = w.double().expand(B)
                    assert torch.equal(got["loss"], base["loss"])
                    assert torch.equal(got["grad_q"], (base["grad_q"].double() * wd[:, None]).float())
                    assert torch.equal(got["grad_docs"], (base["grad_docs"].double() * wd[None, :, None]).float())


def test_bad_arguments_are_refused_on_the_device_and_nothing_is_written(lib):
    B, K, D = 4, 3, 8
    x, d = torch.randn(B, D, device="cuda"), torch.randn(K, B, D, device="cuda")
    y = torch.zeros(B, K, device="cuda")
    outs = [Guarded(n) for n in (B, B * K, B * D, K * B * D, B)]
    o, so, gq, gd, sc = outs
    defaults = (("q", ptr(x)), ("docs", ptr(d)), ("y", ptr(y)), ("B", B), ("K", K), ("D", D), ("kind", KL), ("sim", H.DOT),
                ("T", 1.0), ("red", 2), ("out", o.ptr()), ("so", so.ptr()), ("go", None), ("gq", gq.ptr()), ("gd", gd.ptr()),
                ("sc", sc.ptr()), ("st", stream()))
    call = lambda **k: lib.qst_listwise_distill_loss(*[k.get(nm, dflt) for nm, dflt in defaults])  # noqa: E731
    for kw in LH.REFUSED_BAD_ARG:
        assert call(**kw) == BAD_ARG, kw
    for kw in LH.REFUSED_UNSUPPORTED:
        assert call(**kw) == UNSUPPORTED, kw
    torch.cuda.synchronize()
    for t in outs:
        t.written(0)
    # the same call with good arguments goes through, and so do the optional pointers left out where they may be
    assert call() == 0 and call(kind=MARGIN, y=ptr(y[:, :K - 1].contiguous()), T=0.0) == 0
    assert call(red=0, sc=None, so=None) == 0 and call(gq=None, gd=None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 4. the function with autograd
def test_functions_with_autograd(lib):
    B, K, D = 6, 5, 64
    q, docs = [dev(t) for t in LH.list_rows(B, K, D, 21)]
    for kind, sim, T, red in (("kl", S.METRIC_DOT, 2.0, "mean"), ("kl", S.METRIC_COS_SIM, 1.0, "sum"),
                              ("margin_mse", S.METRIC_DOT, 1.0, "mean"), ("margin_mse", S.METRIC_COS_SIM, 1.0, "none")):
        code = S._LISTWISE_CODE[kind]
        y = LH.labels_of(q.cpu(), docs.cpu(), code, sim, 22)
        w = LH.upstream(B, S._RED_CODE[red])
        xq, xd = q.clone().requires_grad_(True), docs.clone().requires_grad_(True)
        out = S.listwise_distill(xq, xd, dev(y), kind, sim, T, red)
        assert out.shape == ((B,) if red == "none" else ())
        (out * dev(w)).sum().backward()
        ref = LH.reference_of(q.cpu(), docs.cpu(), y, code, sim, T, S._RED_CODE[red], w)
        bd = LH.bounds_of(q.cpu(), docs.cpu(), y, code, sim, T, S._RED_CODE[red], w)
        hold({"loss": out.detach().cpu(), "grad_q": xq.grad.cpu(), "grad_docs": xd.grad.cpu()}, ref, bd,
             f"listwise_distill {kind} {red}", ("loss", "grad_q", "grad_docs"))
    y = dev(torch.zeros(B, K))
    with pytest.raises(ValueError, match=r"\(6, 5\).*\(6, 4\)"):
        S.listwise_distill(q, docs, y[:, :4].contiguous(), "kl")
    with pytest.raises(ValueError, match=r"\(6, 4\).*\(6, 5\)"):
        S.listwise_distill(q, docs, y, "margin_mse")
    with pytest.raises(ValueError):
        S.listwise_distill(q, docs[:, :5], y, "kl")
    with pytest.raises(ValueError):
        S.listwise_distill(q, docs, y, "kl", temperature=0.0)
    with pytest.raises(ValueError):
        S.listwise_distill(q, docs, y, "kl", sim=S.METRIC_L2)


# ------------------------------------------------------------------ 5. the classes
def list_texts(n, negs):
    return [[sent(i, 9), sent(i, 9) + " now"] + [sent(1000 * (k + 1) + i, 5 + (i + k) % 7) for k in range(negs)] for i in range(n)]


@pytest.fixture(scope="module")
def model():
    return SentenceTransformer("tiny-bert", device="cuda")


@pytest.fixture(scope="module")
def teacher():
    return SentenceTransformer("tiny-bert", device="cuda", seed=15)


def teacher_scores(teacher, rows):
    """The teacher's own dot scores [n, K] of (query, candidates ...) rows."""
    embs = [np.asarray(teacher.encode([r[k] for r in rows], batch_size=16), dtype=np.float64) for k in range(len(rows[0]))]
    return np.stack([(embs[0] * e).sum(1) for e in embs[1:]], 1)


def list_examples(teacher, n, negs, kind):
    rows = list_texts(n, negs)
    s = teacher_scores(teacher, rows)
    labels = s if kind == KL else s[:, :1] - s[:, 1:]
    return [InputExample(texts=r, label=[float(v) for v in y]) for r, y in zip(rows, labels)]


def class_batch(model, teacher, negs, kind):
    feats, labels = model.smart_batching_collate(list_examples(teacher, 16, negs, kind))
    return [{k: v.cuda() for k, v in f.items()} for f in feats], labels.cuda()


def foreign_dot(a, b):
    return (a * b).sum(1)


def foreign_cos(a, b):
    return torch.nn.functional.cosine_similarity(a, b)


CLASS_CASES = {
    "kl_dot": (KL, H.DOT, 2.0, lambda m, **k: S.DistillKLDivLoss(m, temperature=2.0, **k), foreign_dot),
    "kl_cos": (KL, H.COS_SIM, 0.5, lambda m, **k: S.DistillKLDivLoss(m, util.pairwise_cos_sim, 0.5, **k), foreign_cos),
    "margin_dot": (MARGIN, H.DOT, 1.0, lambda m, **k: S.MarginMSELoss(m, **k), foreign_dot),
    "margin_cos": (MARGIN, H.COS_SIM, 1.0, lambda m, **k: S.MarginMSELoss(m, util.pairwise_cos_sim, **k), foreign_cos),
}


def make_foreign(model, name):
    kind, _, T, _, fct = CLASS_CASES[name]
    return S.DistillKLDivLoss(model, fct, T) if kind == KL else S.MarginMSELoss(model, fct)


@pytest.mark.parametrize("name", sorted(CLASS_CASES))
def test_class_matches_the_yardstick_and_the_torch_path(model, teacher, name):
    kind, sim, T, make, _ = CLASS_CASES[name]
    feats, labels = class_batch(model, teacher, 3, kind)
    assert labels.shape == ((16, 4) if kind == KL else (16, 3)) and labels.dtype == torch.float32
    model.train()
    lt, gt, emb_t = one_backward(model, make_foreign(model, name), feats, labels)
    lh, gh, emb_h = one_backward(model, make(model), feats, labels)
    assert lt.item() != 0.0 and len(emb_h) == 1 and len(emb_t) == 1 and torch.equal(emb_h[0], emb_t[0])
    # the value, against the objective in fp64 on the embeddings the class's own encoder pass produced
    emb = emb_h[0].cpu()
    q, docs = emb[:16], emb[16:].view(4, 16, -1)
    ref = LH.loss_ref(q.double(), docs.double(), labels.cpu(), kind, sim, T, 2).item()
    drow, _, _ = LH.row_bounds(q, docs, labels.cpu(), kind, sim, T)
    bound = LH.reduced_bound(drow, torch.tensor(ref), kind, 4, 2).item()
    print(f"  {name}: loss hip {lh.item():.9f} torch ops {lt.item():.9f} fp64 {ref:.9f}; |hip - fp64| = "
          f"{abs(lh.item() - ref):.3e}, bound {bound:.3e}")
    assert abs(lh.double().item() - ref) <= bound
    # the fused and the torch path agree: each within the kernel bound of the same fp64 value
    assert abs(lt.double().item() - ref) <= bound and abs(lt.double().item() - lh.double().item()) <= 2 * bound
    no_kb, every, worst_name = grad_rel(gh, gt)
    print(f"  {name}: gradient arena, relative L2 difference per tensor: without the key biases {no_kb:.3e} at {worst_name}; "
          f"every tensor {every:.3e}")
    assert no_kb < GRAD_REL_SANITY


@pytest.mark.parametrize("name", ["kl_dot", "margin_cos"])
def test_fused_pass_equals_one_pass_per_column(model, teacher, name):
    kind, _, _, make, _ = CLASS_CASES[name]
    feats, labels = class_batch(model, teacher, 3, kind)
    model.train()
    lk, gk, emb_k = one_backward(model, make(model, fused=False), feats, labels)
    l1, g1, emb_1 = one_backward(model, make(model, fused=True), feats, labels)
    assert len(emb_k) == 5 and len(emb_1) == 1
    flat = lambda g: torch.cat([t.reshape(-1) for t in g.values()])  # noqa: E731
    assert abs(lk.item() - l1.item()) < 2e-4 * max(1.0, abs(l1.item()))
    assert (flat(gk) - flat(g1)).norm().item() <= 2e-2 * flat(g1).norm().item()


class Tap(nn.Module):
    """A stand-in model that returns given embeddings: the classes above 64 candidates, without 66 encoder passes."""

    def forward(self, feats):
        return {"sentence_embedding": feats["emb"]}


@pytest.mark.parametrize("name", sorted(CLASS_CASES))
def test_65_candidates_take_the_torch_path_and_match_the_yardstick(lib, name, monkeypatch):
    kind, sim, T, make, _ = CLASS_CASES[name]
    B, K, D = 6, 65, 64
    q, docs = LH.list_rows(B, K, D, 31)
    y = LH.labels_of(q, docs, kind, sim, 32)
    called = []
    monkeypatch.setattr(S, "listwise_distill", lambda *a, **k: called.append(a))
    feats = [{"emb": dev(q).requires_grad_(True)}] + [{"emb": dev(d)} for d in docs]
    loss = make(Tap(), fused=False)(feats, dev(y))
    assert not called
    ref = LH.loss_ref(q.double(), docs.double(), y, kind, sim, T, 2)
    drow, _, _ = LH.row_bounds(q, docs, y, kind, sim, T)
    # the torch composition is another fp32 evaluation of the same formulas from the same fp32 scores
    assert abs(loss.double().item() - ref.item()) <= LH.reduced_bound(drow, ref, kind, K, 2).item()
    loss.backward()
    assert torch.isfinite(feats[0]["emb"].grad).all()
    # ... and 64 candidates are one kernel call
    monkeypatch.undo()
    calls = []
    real = S.listwise_distill_raw
    monkeypatch.setattr(S, "listwise_distill_raw", lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch.no_grad():
        make(Tap(), fused=False)(feats[:65], dev(y[:, :64 if kind == KL else 63].contiguous()))
    assert len(calls) == 1


def test_wrong_label_shapes_are_refused(model, teacher):
    feats, labels = class_batch(model, teacher, 3, KL)
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"\(16, 4\).*\(16, 3\)"):
            S.DistillKLDivLoss(model)([dict(f) for f in feats], labels[:, :3].contiguous())
        with pytest.raises(ValueError, match=r"\(16, 3\).*\(16, 4\)"):
            S.MarginMSELoss(model)([dict(f) for f in feats], labels)
        with pytest.raises(ValueError, match=r"\(16, 3\).*\(16,\)"):
            S.MarginMSELoss(model)([dict(f) for f in feats], labels[:, 0].contiguous())


# ------------------------------------------------------------------ 6. fit
class ShapeRecordLoss(RecordLoss):
    def __init__(self, inner):
        super().__init__(inner)
        self.shapes = []

    def forward(self, feats, labels):
        self.shapes.append(tuple(labels.shape))
        return super().forward(feats, labels)


@pytest.mark.parametrize("use_amp", [False, True])
@pytest.mark.parametrize("kind", [KL, MARGIN], ids=["kl", "margin_mse"])
def test_fit_lowers_the_listwise_loss(teacher, kind, use_amp):
    m = SentenceTransformer("tiny-bert", device="cuda")          # a fresh student: amp schedule counters persist per model
    data = list_examples(teacher, 16, 3, kind)
    lm = ShapeRecordLoss(S.DistillKLDivLoss(m) if kind == KL else S.MarginMSELoss(m))
    m.fit([(DataLoader(data, batch_size=4, shuffle=False), lm)], epochs=5, warmup_steps=0, scheduler="constantlr",
          optimizer_params={"lr": 1e-3}, dropout=0, use_amp=use_amp, show_progress_bar=False)
    seen = torch.stack(lm.seen).cpu()
    assert len(seen) == 20 and set(lm.shapes) == {(4, 4) if kind == KL else (4, 3)}
    print(f"  fit {KIND_NAMES[kind]} amp={use_amp}: first 5 {seen[:5].mean().item():.6f} last 5 {seen[-5:].mean().item():.6f}")
    assert torch.isfinite(seen).all() and seen[-5:].mean() < seen[:5].mean()
    assert torch.isfinite(m._enc.params).all()
