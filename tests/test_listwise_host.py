"""CPU: the host side of the listwise distillation objectives -- the binding, the header and the argument checks of
qst_listwise_distill_loss (made before any launch, so they hold without a device), the constructors and the drop-in export
of DistillKLDivLoss, label shapes, the torch composition on CPU tensors against the yardstick, list labels through
smart_batching_collate and _shard_batch, the conditions on the GPU test's data, and the bounds of listwise_helpers against a
plain fp32 evaluation. No kernel runs here."""
import ctypes as C
import inspect
import math
import os
import sys

import pytest
import torch
from torch import nn

import quadruplet_sentence_transformer_amd  # noqa: F401
import listwise_helpers as LH
import tuple_loss_helpers as H
from listwise_helpers import BAD_ARG, KL, MARGIN, UNSUPPORTED
from test_distill_host import collate, header_signature
from quadruplet_sentence_transformer_amd import _lib, st_losses as S, util
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, _shard_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = inspect.Parameter.empty


# ------------------------------------------------------------------ the library
def test_library_version_header_and_ctypes_table():
    lib = _lib.load()
    assert lib.qst_version() >= 121
    name = "qst_listwise_distill_loss"
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    res, args = header_signature(name)
    assert res is C.c_int and len(args) == 17 and args[3:10] == [C.c_int] * 5 + [C.c_float, C.c_int]
    assert _lib.SIGNATURES[name] == (res, args)
    assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    header = open(os.path.join(ROOT, "include", "qst.h")).read()
    assert "QST_LISTWISE_KL = 0, QST_LISTWISE_MARGIN_MSE = 1" in header
    assert (S.LISTWISE_KL, S.LISTWISE_MARGIN_MSE, S.LISTWISE_MAX_K) == (KL, MARGIN, 64)
    makefile = open(os.path.join(ROOT, "quadruplet-sentence-transformer_amd", "csrc", "Makefile")).read()
    assert " listwise.hip " in makefile


def test_bad_arguments_are_refused_without_a_device():
    """Every refusal of qst_listwise_distill_loss comes back before anything is launched: host memory stands in for the
    device pointers, and must be left as it was."""
    lib = _lib.load()
    B, K, D = 4, 3, 6
    q, docs, y = (C.c_float * (B * D))(), (C.c_float * (K * B * D))(), (C.c_float * (B * K))()
    outs = {"out": (C.c_float * B)(), "so": (C.c_float * (B * K))(), "gq": (C.c_float * (B * D))(),
            "gd": (C.c_float * (K * B * D))(), "sc": (C.c_float * B)()}
    for buf in outs.values():
        for i in range(len(buf)):
            buf[i] = 7.0
    p = lambda x: None if x is None else C.cast(x, C.c_void_p)  # noqa: E731
    defaults = (("q", q), ("docs", docs), ("y", y), ("B", B), ("K", K), ("D", D), ("kind", KL), ("sim", H.DOT), ("T", 1.0),
                ("red", 2), ("out", outs["out"]), ("so", outs["so"]), ("go", None), ("gq", outs["gq"]), ("gd", outs["gd"]),
                ("sc", outs["sc"]), ("st", None))

    def call(**kw):
        vals = [kw.get(nm, dflt) for nm, dflt in defaults]
        return lib.qst_listwise_distill_loss(*[v if isinstance(v, (int, float)) else p(v) for v in vals])

    for kw in LH.REFUSED_BAD_ARG:
        assert call(**kw) == BAD_ARG, kw
    for kw in LH.REFUSED_UNSUPPORTED:
        assert call(**kw) == UNSUPPORTED, kw
    assert all(v == 7.0 for buf in outs.values() for v in buf)
    # every refusal the header lists is in the two tables
    keys = {tuple(sorted(kw)) for kw in LH.REFUSED_BAD_ARG}
    for k in ("B", "D", "q", "docs", "y", "out", "sc", "kind", "sim", "red", "T", "gq", "gd"):
        assert (k,) in keys, k
    assert ("K", "kind") in keys and {kw["K"] for kw in LH.REFUSED_UNSUPPORTED} >= {0, -1, 65}


# ------------------------------------------------------------------ surface
class Wide(nn.Module):
    """A stand-in that returns fixed embeddings."""

    def forward(self, feats):
        return {"sentence_embedding": feats["emb"]}


def defaults(fn, skip=("self",)):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if k not in skip}


def test_constructor_config_dict_and_reduction():
    assert defaults(S.DistillKLDivLoss.__init__) == {"model": EMPTY, "similarity_fct": util.pairwise_dot_score,
                                                     "temperature": 1.0, "fused": True}
    assert list(inspect.signature(S.DistillKLDivLoss.forward).parameters) == ["self", "sentence_features", "labels"]
    lm = S.DistillKLDivLoss(Wide())
    assert isinstance(lm, S._TupleLoss) and lm.reduction == "mean" and lm._kernel_sim() == S.METRIC_DOT
    assert lm.get_config_dict() == {"similarity_fct": "pairwise_dot_score", "temperature": 1.0}
    lc = S.DistillKLDivLoss(Wide(), similarity_fct=util.pairwise_cos_sim, temperature=2.5)
    assert lc._kernel_sim() == S.METRIC_COS_SIM
    assert lc.get_config_dict() == {"similarity_fct": "pairwise_cos_sim", "temperature": 2.5}

    def mine(a, b):
        return (a * b).sum(1)

    lf = S.DistillKLDivLoss(Wide(), mine)
    assert lf._kernel_sim() is None and lf.get_config_dict() == {"similarity_fct": "mine", "temperature": 1.0}
    # MarginMSELoss keeps its surface
    assert defaults(S.MarginMSELoss.__init__) == {"model": EMPTY, "similarity_fct": util.pairwise_dot_score, "fused": True}


def test_dropin_export():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    gone = lambda: [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]  # noqa: E731
    for k in gone():
        del sys.modules[k]
    try:
        import sentence_transformers
        from sentence_transformers import losses, util as st_util
        from sentence_transformers.losses import DistillKLDivLoss
        assert sentence_transformers.losses.DistillKLDivLoss is losses.DistillKLDivLoss is DistillKLDivLoss is S.DistillKLDivLoss
        assert losses.MarginMSELoss is S.MarginMSELoss                      # what was there still is
        # the default similarity of the drop-in class is the drop-in function: the kernel path is taken
        assert losses.DistillKLDivLoss(torch.nn.Identity()).similarity_fct is st_util.pairwise_dot_score
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for k in gone():
            del sys.modules[k]


def cpu_feats(q, docs):
    return [{"emb": q}] + [{"emb": d} for d in docs]


def test_labels_of_the_wrong_shape_are_refused():
    q, docs = LH.list_rows(4, 3, 8, 1)
    feats = cpu_feats(q, docs)
    with pytest.raises(ValueError, match=r"\(4, 3\).*\(4, 2\)"):
        S.DistillKLDivLoss(Wide(), fused=False)(feats, torch.zeros(4, 2))
    with pytest.raises(ValueError, match=r"\(4, 3\).*\(4,\)"):
        S.DistillKLDivLoss(Wide(), fused=False)(feats, torch.zeros(4))
    with pytest.raises(ValueError, match=r"\(4, 3\).*\(3, 4\)"):
        S.DistillKLDivLoss(Wide(), fused=False)(feats, torch.zeros(3, 4))
    with pytest.raises(ValueError, match=r"\(4, 2\).*\(4, 3\)"):
        S.MarginMSELoss(Wide(), fused=False)(feats, torch.zeros(4, 3))
    with pytest.raises(ValueError, match=r"\(4, 2\).*\(8,\)"):
        S.MarginMSELoss(Wide(), fused=False)(feats, torch.zeros(8))
    with pytest.raises(ValueError, match="2 or more"):
        S.DistillKLDivLoss(Wide(), fused=False)(feats[:1], torch.zeros(4, 0))
    # the right shapes get as far as the kernel path, which has no CPU form
    with pytest.raises(_lib.QstError, match="HIP device only"):
        S.DistillKLDivLoss(Wide(), fused=False)(feats, torch.zeros(4, 3))
    with pytest.raises(_lib.QstError, match="HIP device only"):
        S.MarginMSELoss(Wide(), fused=False)(feats, torch.zeros(4, 2))
    with pytest.raises(_lib.QstError, match="HIP device only"):
        S.listwise_distill_raw(q, docs, torch.zeros(4, 3), KL, S.METRIC_DOT, 1.0, 2)


@pytest.mark.parametrize("sim", LH.SIMS, ids=lambda m: H.METRIC_NAMES[m])
@pytest.mark.parametrize("K", [1, 2, 5, 65])
def test_a_foreign_similarity_fct_runs_upstreams_composition_on_cpu_tensors(K, sim):
    """The torch path needs no device: the stand-in's embeddings, a callable of the user's, upstream's composition, equal
    to the yardstick's per-row form."""
    B, D = 7, 34
    q, docs = [t.double() for t in LH.list_rows(B, K, D, 3)]
    fct = lambda a, b: H.metric_ref(a, b, sim)  # noqa: E731
    for T in LH.TEMPERATURES:
        y = LH.kl_labels(B, K, 4).double()
        loss = S.DistillKLDivLoss(Wide(), fct, T, fused=False)(cpu_feats(q, docs), y)
        want = LH.loss_ref(q, docs, y, KL, sim, T, 2)
        assert abs(loss.item() - want.item()) <= 1e-12 * (1 + abs(want.item()))
        assert abs(LH.kl_upstream(q, docs, y, fct, T).item() - want.item()) <= 1e-12 * (1 + abs(want.item()))
    if K >= 3:
        y = LH.margin_list_labels(q.float(), docs.float(), sim, 5).double()
        loss = S.MarginMSELoss(Wide(), fct, fused=False)(cpu_feats(q, docs), y)
        want = LH.loss_ref(q, docs, y, MARGIN, sim, 1.0, 2)
        assert abs(loss.item() - want.item()) <= 1e-12 * (1 + abs(want.item()))
        assert abs(LH.margin_upstream(q, docs, y, fct).item() - want.item()) <= 1e-12 * (1 + abs(want.item()))


def test_three_columns_still_resolve_to_margin_mse(monkeypatch):
    q, docs = LH.list_rows(4, 2, 8, 6)
    y = torch.linspace(-1, 1, 4)
    seen = []
    monkeypatch.setattr(S, "margin_mse", lambda *a: seen.append(a) or torch.zeros(()))
    monkeypatch.setattr(S, "listwise_distill", lambda *a, **k: pytest.fail("three columns took the listwise path"))
    S.MarginMSELoss(Wide(), fused=False)(cpu_feats(q, docs), y.view(4, 1))
    (a,) = seen
    assert a[0] is q and torch.equal(a[1], docs[0]) and torch.equal(a[2], docs[1])
    assert a[3].shape == (4,) and a[4:] == (S.METRIC_DOT, "mean")
    with pytest.raises(ValueError, match="3 text columns"):
        S.MarginMSELoss(Wide(), fused=False)(cpu_feats(q, docs[:1]), y)


def test_the_columns_of_one_fused_pass_are_handed_over_without_a_copy():
    B, K, D = 3, 4, 8
    whole = torch.randn((1 + K) * B, D)
    q, docs = S._list_operands(list(whole.split([B] * (1 + K), 0)))
    assert docs.shape == (K, B, D) and docs.data_ptr() == whole[B:].data_ptr() and q.data_ptr() == whole.data_ptr()
    assert torch.equal(docs, whole[B:].view(K, B, D))
    # columns embedded one by one, or rows of another order, are stacked
    cols = [torch.randn(B, D) for _ in range(1 + K)]
    q, docs = S._list_operands(cols)
    assert q is cols[0] and torch.equal(docs, torch.stack(cols[1:], 0))
    parts = list(whole.split([B] * (1 + K), 0))
    q, docs = S._list_operands([parts[0], parts[2], parts[1], parts[3], parts[4]])
    assert torch.equal(docs[0], parts[2]) and torch.equal(docs[1], parts[1])


# ------------------------------------------------------------------ list labels on their way to the loss
def test_list_labels_collate_and_shard_by_rows():
    """fit() is untouched: [B, K] labels reach the loss on the single-process path (smart_batching_collate stacks them) and
    on the data-parallel one (_shard_batch cuts them by rows)."""
    rows = torch.arange(10 * 4, dtype=torch.float32).view(10, 4)
    batch = [InputExample(texts=[f"q {i}", f"p {i}", f"n {i}", f"m {i}", f"o {i}"], label=[float(v) for v in r])
             for i, r in enumerate(rows)]
    feats, labels = collate(batch)
    assert len(feats) == 5 and labels.dtype == torch.float32 and labels.shape == (10, 4) and torch.equal(labels, rows)
    seen = []
    for rank in range(3):
        f, y, n_total, n_mine = _shard_batch(feats, labels, rank, 3)
        assert n_total == 10 and y.shape == (n_mine, 4) and torch.equal(y, rows[rank::3]) and len(f) == 5
        assert all(c["input_ids"].shape[0] == n_mine for c in f)
        seen.extend(y[:, 0].tolist())
    assert sorted(seen) == rows[:, 0].tolist()


# ------------------------------------------------------------------ the GPU test's data and bounds
@pytest.mark.parametrize("B,K,D", [c for c in LH.CASES if c[1] >= 2])
def test_the_margin_residuals_of_the_gpu_cases_stay_at_half_the_scale(B, K, D):
    for sim in LH.SIMS:
        q, docs, y, _, _, _ = LH.case(B, K, D, MARGIN, sim, 1.0, 0, True)
        assert y.shape == (B, K - 1) and LH.residuals_hold(q, docs, y, sim)


def fp32_evaluation(q, docs, y, kind, sim, T, red, w):
    """The formulas in plain fp32 torch ops with their gradients written out: any fp32 evaluation has to fit the bounds."""
    K, B, D = docs.shape
    dot = (q[None] * docs).sum(2)
    if sim == H.COS_SIM:
        nq, nd = (q * q).sum(1).sqrt().clamp_min(1e-8), (docs * docs).sum(2).sqrt().clamp_min(1e-8)
        kxy = 1 / (nq[None] * nd)
        cs = dot * kxy
        s, kxx, kyy = cs, -cs / (nq * nq)[None], -cs / (nd * nd)
    else:
        s, kxy, kxx, kyy = dot, torch.ones_like(dot), torch.zeros_like(dot), torch.zeros_like(dot)
    s = s.t()
    if kind == KL:
        lp, lt = torch.log_softmax(s / T, 1), torch.log_softmax(y / T, 1)
        t = lt.exp()
        rows = T * T * torch.where(t == 0, torch.zeros_like(t), t * (lt - lp)).sum(1)
        g = T * (lp.exp() - t)
    else:
        e = (s[:, :1] - s[:, 1:]) - y
        rows = (e * e).sum(1)
        g = torch.cat([(2 * e).sum(1, keepdim=True), -2 * e], 1)
    den = LH.divisor(kind, B, K, red)
    c = (g / den).t() * w.expand(B)[None]
    gd = (c * kxy)[:, :, None] * q[None] + (c * kyy)[:, :, None] * docs
    gq = ((c * kxy)[:, :, None] * docs).sum(0) + (c * kxx).sum(0)[:, None] * q
    loss = rows if red == 0 else (rows.double().sum() / den).float()
    return {"loss": loss, "scores": s, "grad_q": gq, "grad_docs": gd}


@pytest.mark.parametrize("B,K,D", [(3, 2, 6), (4, 7, 384), (5, 63, 768), (3, 64, 2052)])
def test_a_plain_fp32_evaluation_fits_the_bounds(B, K, D):
    for sim in LH.SIMS:
        for kind in LH.kinds_of(K):
            for red, T in ((0, 1.0), (2, 0.5), (1, 4.0)):
                q, docs, y, w, ref, bd = LH.case(B, K, D, kind, sim, T, red, True)
                got = fp32_evaluation(q, docs, y, kind, sim, T, red, w)
                for k, v in got.items():
                    assert v.dtype == torch.float32 and LH.worst(v, ref[k], bd[k]) <= 1.0, (k, sim, kind, red)
                # and the bounds are bounds of rounding, not tolerances: the value's is below 1e-3 of the value
                assert (bd["loss"] <= 1e-3 * ref["loss"].abs()).all()


def test_the_yardstick_counts_a_zero_teacher_weight_as_zero():
    q, docs = [t.double() for t in LH.list_rows(2, 3, 8, 7)]
    y = torch.tensor([[0.0, -1e4, 1.0], [5.0, 5.0, -1e4]], dtype=torch.float64)     # exp(-1e4) is 0 in double too
    rows = LH.rows_ref(q, docs, y, KL, H.DOT)
    assert torch.isfinite(rows).all() and (rows >= 0).all()
    assert math.isfinite(LH.kl_upstream(q, docs, y, lambda a, b: H.metric_ref(a, b, H.DOT), 1.0).item())
