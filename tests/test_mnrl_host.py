"""CPU: the host side of MultipleNegativesRankingLoss / MultipleNegativesSymmetricRankingLoss -- constructor surface,
similarity_fct dispatch, drop-in namespaces, the refusal of CPU tensors and bad shapes, the argument checks of
qst_mnrl_loss (made before any launch, so they hold without a device), and NoDuplicatesDataLoader. No kernel runs here."""
import ctypes as C
import inspect
import os
import random
import sys

import pytest
import torch
from torch import nn

import quadruplet_sentence_transformer_amd  # noqa: F401
import mnrl_helpers as M
from quadruplet_sentence_transformer_amd import _lib, data, st_losses as S, util
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = (S.MultipleNegativesRankingLoss, S.MultipleNegativesSymmetricRankingLoss)


def defaults(cls):
    return {k: p.default for k, p in inspect.signature(cls.__init__).parameters.items() if k not in ("self", "model")}


def drop_in():
    """The drop-in `sentence_transformers` package, imported afresh; the caller restores sys.path and sys.modules."""
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
        del sys.modules[m]
    import sentence_transformers
    return sentence_transformers


def drop_out():
    sys.path.remove(os.path.join(ROOT, "dropin"))
    for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
        del sys.modules[m]


def test_constructor_defaults_follow_sentence_transformers():
    for cls in BOTH:
        assert defaults(cls) == {"scale": 20.0, "similarity_fct": util.cos_sim, "fused": True}
        assert list(inspect.signature(cls.forward).parameters)[:3] == ["self", "sentence_features", "labels"]
        assert issubclass(cls, S._TupleLoss) and cls.reduction == "mean"
    assert S.MultipleNegativesRankingLoss._symmetric is False and S.MultipleNegativesSymmetricRankingLoss._symmetric is True


def test_config_dict_names_the_similarity_function():
    for cls in BOTH:
        assert cls(nn.Identity()).get_config_dict() == {"scale": 20.0, "similarity_fct": "cos_sim"}
        assert cls(nn.Identity(), scale=1.0, similarity_fct=util.dot_score).get_config_dict() == {
            "scale": 1.0, "similarity_fct": "dot_score"}


def test_similarity_fct_is_dispatched_by_identity():
    try:
        st = drop_in()
        assert st.util.cos_sim is util.cos_sim and st.util.dot_score is util.dot_score
        for cls in BOTH:
            assert cls(nn.Identity())._kernel_sim() == "cos"
            assert cls(nn.Identity(), similarity_fct=st.util.cos_sim)._kernel_sim() == "cos"
            assert cls(nn.Identity(), similarity_fct=st.util.dot_score)._kernel_sim() == "dot"
            assert cls(nn.Identity(), similarity_fct=lambda a, b: util.cos_sim(a, b))._kernel_sim() is None
    finally:
        drop_out()


def test_dropin_losses_and_datasets_resolve_to_this_build():
    try:
        st = drop_in()
        from sentence_transformers import datasets, losses
        from sentence_transformers.datasets import NoDuplicatesDataLoader
        from sentence_transformers.losses import MultipleNegativesRankingLoss, MultipleNegativesSymmetricRankingLoss
        assert losses.MultipleNegativesRankingLoss is MultipleNegativesRankingLoss is S.MultipleNegativesRankingLoss
        assert MultipleNegativesSymmetricRankingLoss is S.MultipleNegativesSymmetricRankingLoss
        assert datasets.NoDuplicatesDataLoader is NoDuplicatesDataLoader is data.NoDuplicatesDataLoader
        assert st.datasets is datasets
        # the classes that were there before still are
        assert losses.TripletLoss is S.TripletLoss and losses.CosineSimilarityLoss is S.CosineSimilarityLoss
    finally:
        drop_out()


def test_cpu_tensors_and_bad_shapes_are_refused():
    a, c = torch.randn(4, 8), torch.randn(6, 8)
    for symmetric in (False, True):
        with pytest.raises(_lib.QstError):
            S.multiple_negatives_ranking_loss(a, c, symmetric=symmetric)
    with pytest.raises(ValueError):
        S.multiple_negatives_ranking_loss(a, torch.randn(6, 9))         # another D
    with pytest.raises(ValueError):
        S.multiple_negatives_ranking_loss(a, c[:3])                      # N < B
    with pytest.raises(ValueError):
        S.multiple_negatives_ranking_loss(a, c, sim="euclid")
    with pytest.raises(ValueError):
        S.multiple_negatives_ranking_loss(a, c, scale=0.0)
    with pytest.raises(ValueError):
        S.multiple_negatives_ranking_loss(a[0], c)
    with pytest.raises(ValueError):
        S.MultipleNegativesRankingLoss(nn.Identity())([{"input_ids": torch.zeros(2, 3, dtype=torch.long)}], None)


def test_library_version_and_new_symbols():
    lib = _lib.load()
    assert lib.qst_version() >= 105
    for name, nargs in (("qst_mnrl_workspace_bytes", 3), ("qst_mnrl_loss", 15)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SIGNATURES["qst_mnrl_workspace_bytes"][0] is C.c_size_t
    assert (S.SCORE_DOT, S.SCORE_COS) == (0, 1)                          # include/qst.h: QST_SCORE_DOT, QST_SCORE_COS
    # scores [B, ldS] with ldS = N rounded up to 4, plus the per-row scalars
    assert lib.qst_mnrl_workspace_bytes(5, 10, 7) >= 5 * 12 * 4
    assert lib.qst_mnrl_workspace_bytes(512, 1024, 768) >= 512 * 1024 * 4
    assert lib.qst_mnrl_workspace_bytes(0, 4, 8) == 0 and lib.qst_mnrl_workspace_bytes(4, 3, 8) == 0


def test_bad_arguments_are_refused_without_a_device():
    """Every QST_ERR_BAD_ARG of qst_mnrl_loss comes back before anything is launched: host memory stands in for the device
    pointers, and must be left as it was."""
    lib = _lib.load()
    B, N, D = 4, 6, 8
    nbytes = lib.qst_mnrl_workspace_bytes(B, N, D)
    assert nbytes > 0
    a, c = (C.c_float * (B * D))(), (C.c_float * (N * D))()
    ga, gc = (C.c_float * (B * D))(), (C.c_float * (N * D))()
    out = (C.c_float * 1)(7.0)
    ws = (C.c_char * nbytes)()
    for buf in (ga, gc):
        for i in range(len(buf)):
            buf[i] = -3.0

    def call(a=a, c=c, B=B, N=N, D=D, sim=S.SCORE_COS, scale=20.0, symmetric=0, out=out, ga=ga, gc=gc, ws=ws, nb=nbytes):
        p = lambda x: None if x is None else C.cast(x, C.c_void_p)  # noqa: E731
        return lib.qst_mnrl_loss(p(a), p(c), B, N, D, sim, scale, symmetric, p(out), None, p(ga), p(gc), p(ws), nb, None)

    bad = [dict(B=0), dict(B=-1), dict(N=B - 1), dict(D=0), dict(a=None), dict(c=None), dict(out=None), dict(ws=None),
           dict(nb=nbytes - 1), dict(nb=0), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")),
           dict(scale=float("nan")), dict(ga=None), dict(gc=None), dict(sim=2), dict(sim=-1), dict(symmetric=2)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert out[0] == 7.0 and all(v == -3.0 for v in ga) and all(v == -3.0 for v in gc)
    assert all(b == b"\x00" for b in ws)


def examples(n, repeat_every=0):
    out = []
    for i in range(n):
        k = i - 1 if repeat_every and i % repeat_every == repeat_every - 1 else i   # every third pair repeats its neighbour
        out.append(InputExample(texts=[f"question {k}", f"  Answer {k} "]))
    return out


@pytest.mark.parametrize("repeat_every", [0, 3])
def test_no_duplicates_data_loader(repeat_every):
    random.seed(5)
    data_set = examples(50, repeat_every)
    dl = data.NoDuplicatesDataLoader(data_set, 8)
    assert len(dl) == 50 // 8 == 6 and dl.collate_fn is None
    seen_batches = 0
    for _ in range(3):                              # the pointer runs on across epochs and wraps around the list
        for batch in dl:
            assert len(batch) == 8
            texts = [t.strip().lower() for ex in batch for t in ex.texts]
            assert len(set(texts)) == len(texts)
            seen_batches += 1
    assert seen_batches == 18
    # 18 batches of 8 out of 50 examples: the list was walked at least twice
    assert 0 <= dl.data_pointer < 50
    dl.collate_fn = lambda batch: len(batch)        # what fit() sets
    assert list(dl) == [8] * 6


def test_no_duplicates_data_loader_wraps_and_gives_up():
    random.seed(1)
    dl = data.NoDuplicatesDataLoader(examples(10), 4)
    assert len(dl) == 2
    first = [[ex.texts[0] for ex in b] for b in dl]
    assert dl.data_pointer == 8
    second = [[ex.texts[0] for ex in b] for b in dl]     # starts at 8, wraps (and reshuffles) after 10
    assert all(len(b) == 4 and len(set(b)) == 4 for b in first + second) and dl.data_pointer < 10
    # three distinct texts cannot fill a batch of four: sentence-transformers would spin for ever
    same = [InputExample(texts=[f"q{i % 3}", f"a{i % 3}"]) for i in range(12)]
    with pytest.raises(ValueError):
        next(iter(data.NoDuplicatesDataLoader(same, 4)))


def test_helper_recipe_keeps_the_comparison_meaningful():
    """The conditions test_gpu_mnrl asserts on its reference hold on the smallest cases (the GPU test checks every case)."""
    for (B, N, D) in M.SHAPES[1:5]:
        for sim in ("cos", "dot"):
            for symmetric in (0, 1):
                for trained in (0, 1):
                    _, _, loss, ga, gc = M.reference(B, N, D, sim, symmetric, trained)
                    assert loss.item() >= M.MIN_REF_LOSS and ga.abs().max().item() >= M.MIN_REF_GRAD
    a, c, loss, ga, gc = M.reference(1, 1, 1, "cos", 1, 0)
    assert loss.item() == 0.0 and not ga.any() and not gc.any()
