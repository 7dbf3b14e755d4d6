"""CPU: the host side of the distillation objectives -- constructor surface of MSELoss, MarginMSELoss, MSEEvaluator and
TranslationEvaluator, drop-in namespaces, the library's exports against the header, the refusal of CPU tensors, vector labels
through smart_batching_collate and _shard_batch, and ParallelSentencesDataset with a fake teacher. No kernel runs here."""
import ctypes as C
import gzip
import inspect
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

import quadruplet_sentence_transformer_amd  # noqa: F401
import distill_helpers as DH
from quadruplet_sentence_transformer_amd import _lib, data, evaluation, st_losses as S, util
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, SentenceTransformer, _shard_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = inspect.Parameter.empty


def defaults(fn, skip=("self",)):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if k not in skip}


# ------------------------------------------------------------------ surface
def test_constructor_defaults_follow_sentence_transformers():
    assert defaults(S.MSELoss.__init__) == {"model": EMPTY}
    assert defaults(S.MarginMSELoss.__init__) == {"model": EMPTY, "similarity_fct": util.pairwise_dot_score, "fused": True}
    for cls in (S.MSELoss, S.MarginMSELoss):
        assert list(inspect.signature(cls.forward).parameters) == ["self", "sentence_features", "labels"]
        assert cls(torch.nn.Identity()).reduction == "mean"
    assert defaults(evaluation.MSEEvaluator.__init__) == {
        "source_sentences": EMPTY, "target_sentences": EMPTY, "teacher_model": None, "show_progress_bar": False,
        "batch_size": 32, "name": "", "write_csv": True}
    assert defaults(evaluation.TranslationEvaluator.__init__) == {
        "source_sentences": EMPTY, "target_sentences": EMPTY, "show_progress_bar": False, "batch_size": 16, "name": "",
        "print_wrong_matches": False, "write_csv": True}
    for cls in (evaluation.MSEEvaluator, evaluation.TranslationEvaluator):
        assert issubclass(cls, evaluation.SentenceEvaluator)
        assert defaults(cls.__call__) == {"model": EMPTY, "output_path": None, "epoch": -1, "steps": -1}
    assert defaults(data.ParallelSentencesDataset.__init__) == {"student_model": EMPTY, "teacher_model": EMPTY,
                                                                "batch_size": 8, "use_embedding_cache": True}
    for fn in (data.ParallelSentencesDataset.load_data, data.ParallelSentencesDataset.add_dataset):
        assert list(defaults(fn).items())[1:] == [("weight", 100), ("max_sentences", None), ("max_sentence_length", 128)]
    lm = S.MarginMSELoss(torch.nn.Identity())
    assert lm._kernel_sim() == S.METRIC_DOT
    assert S.MarginMSELoss(torch.nn.Identity(), similarity_fct=util.pairwise_cos_sim)._kernel_sim() == S.METRIC_COS_SIM
    assert S.MarginMSELoss(torch.nn.Identity(), similarity_fct=lambda a, b: (a * b).sum(1))._kernel_sim() is None
    ev = evaluation.MSEEvaluator(["a"], ["a"], teacher_model=DH.FakeTeacher(), name="dev")
    assert ev.csv_file == "mse_evaluation_dev_results.csv" and ev.csv_headers == ["epoch", "steps", "MSE"]
    ev = evaluation.TranslationEvaluator(["a"], ["b"], name="dev")
    assert ev.csv_file == "translation_evaluation_dev_results.csv"
    assert ev.csv_headers == ["epoch", "steps", "src2trg", "trg2src"]


def test_mse_evaluator_takes_the_teacher_embeddings_once_in_init():
    teacher = DH.FakeTeacher()
    ev = evaluation.MSEEvaluator(["one", "two", "three"], ["eins", "zwei", "drei"], teacher_model=teacher, batch_size=2)
    assert teacher.calls == 1 and teacher.sentences == ["one", "two", "three"] and teacher.batch_sizes == [2]
    np.testing.assert_array_equal(ev.source_embeddings, np.stack([DH.hash_vector(s) for s in ("one", "two", "three")]))
    assert ev.target_sentences == ["eins", "zwei", "drei"]


def test_dropin_names_resolve_to_this_build():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]
        from sentence_transformers import datasets, evaluation as ev, losses, util as u
        assert losses.MSELoss is S.MSELoss and losses.MarginMSELoss is S.MarginMSELoss
        assert ev.MSEEvaluator is evaluation.MSEEvaluator and ev.TranslationEvaluator is evaluation.TranslationEvaluator
        assert datasets.ParallelSentencesDataset is data.ParallelSentencesDataset
        assert u.pairwise_dot_score is util.pairwise_dot_score and u.pairwise_cos_sim is util.pairwise_cos_sim
        # the default similarity of the drop-in class is the drop-in function: the kernel path is taken
        assert losses.MarginMSELoss(torch.nn.Identity()).similarity_fct is u.pairwise_dot_score
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]


CTYPE = {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t}


def header_signature(name):
    src = open(os.path.join(ROOT, "include", "qst.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    ret, args = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src).groups()
    out = []
    for a in args.split(","):
        a = a.strip()
        out.append(_lib.vp if "*" in a else CTYPE[a.split()[-2]])
    return CTYPE[ret], out


def test_library_version_and_header_match_the_ctypes_table():
    lib = _lib.load()
    assert lib.qst_version() >= 107
    for name, nargs in (("qst_embed_mse", 9), ("qst_margin_mse_loss", 16)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        res, args = header_signature(name)
        assert len(args) == nargs
        assert _lib.SIGNATURES[name] == (res, args)
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    # the parser reads what it should: a neighbour with a float among its arguments
    assert header_signature("qst_triplet_loss") == _lib.SIGNATURES["qst_triplet_loss"]


def test_cpu_tensors_are_refused():
    q, p, n = torch.randn(3, 4, 8).unbind(0)
    y = torch.zeros(4)
    with pytest.raises(_lib.QstError):
        S.embed_mse(q, p)
    with pytest.raises(_lib.QstError):
        S.margin_mse(q, p, n, y)
    with pytest.raises(_lib.QstError):
        S.margin_mse(q, p, n, y, S.METRIC_COS_SIM, "none")
    with pytest.raises(_lib.QstError):
        util.pairwise_dot_score(q, p)
    with pytest.raises(_lib.QstError):
        util.pairwise_cos_sim(q, p)
    with pytest.raises(ValueError, match=r"\(4, 8\).*\(4, 7\)"):
        S.embed_mse(q, p[:, :7])
    with pytest.raises(ValueError):
        S.margin_mse(q, p, n[:2], y)
    with pytest.raises(ValueError):
        S.margin_mse(q, p, n, y[:3])
    with pytest.raises(ValueError):
        S.margin_mse(q, p, n, y, S.METRIC_L2)


# ------------------------------------------------------------------ vector labels through the collate function
class WordTokenizer:
    """smart_batching_collate needs nothing of the model but tokenize(): this stands in where no device exists."""

    def tokenize(self, texts):
        return {"input_ids": torch.zeros(len(texts), 4, dtype=torch.int64),
                "attention_mask": torch.ones(len(texts), 4, dtype=torch.int64)}


def collate(batch):
    return SentenceTransformer.smart_batching_collate(WordTokenizer(), batch)


@pytest.mark.parametrize("labels", [[0, 1, 1, 0], [0.5, 0.25, 1.0, 0.0], [3, 0.5, 1, 2], [True, False, True, True]],
                         ids=["int", "float", "mixed", "bool"])
def test_scalar_labels_collate_as_before(labels):
    feats, got = collate([InputExample(texts=[f"s {i}", f"t {i}"], label=y) for i, y in enumerate(labels)])
    ref = torch.tensor(labels)
    assert got.dtype == ref.dtype and got.shape == ref.shape and torch.equal(got, ref)
    assert len(feats) == 2 and feats[0]["input_ids"].shape[0] == 4
    # InputExample's default label
    _, got = collate([InputExample(texts=["a"]), InputExample(texts=["b"])])
    assert got.dtype == torch.int64 and got.tolist() == [0, 0]


@pytest.mark.parametrize("kind", ["ndarray32", "ndarray64", "tensor", "tensor64", "list", "tuple"])
def test_vector_labels_are_stacked_to_fp32_rows(kind):
    rows = np.random.RandomState(0).randn(5, 7)
    make = {"ndarray32": lambda r: r.astype(np.float32), "ndarray64": lambda r: r.astype(np.float64),
            "tensor": lambda r: torch.tensor(r, dtype=torch.float32), "tensor64": lambda r: torch.tensor(r),
            "list": lambda r: [float(v) for v in r], "tuple": lambda r: tuple(float(v) for v in r)}[kind]
    batch = [InputExample(texts=[f"s {i}"], label=make(r)) for i, r in enumerate(rows)]
    feats, got = collate(batch)
    assert got.dtype == torch.float32 and got.shape == (5, 7) and got.is_contiguous()
    assert torch.equal(got, torch.tensor(rows).to(torch.float32))
    assert len(feats) == 1
    assert "label" in str(batch[0])             # InputExample prints such a label


def test_shard_batch_cuts_vector_labels_by_rows():
    B, D = 10, 6
    labels = torch.arange(B * D, dtype=torch.float32).view(B, D)
    feats = [{"input_ids": torch.arange(B).view(B, 1).repeat(1, 3), "attention_mask": torch.ones(B, 3, dtype=torch.int64)}]
    seen = []
    for rank in range(3):
        f, y, n_total, n_mine = _shard_batch(feats, labels, rank, 3)
        assert n_total == B and n_mine == len(range(rank, B, 3)) and y.shape == (n_mine, D)
        assert torch.equal(y, labels[rank::3]) and torch.equal(f[0]["input_ids"][:, 0], torch.arange(B)[rank::3])
        seen.extend(y[:, 0].tolist())
    assert sorted(seen) == labels[:, 0].tolist()


# ------------------------------------------------------------------ ParallelSentencesDataset
def parallel(n, tag="s", k=2):
    return [[f"{tag} source {i}"] + [f"{tag} translation {i}.{j}" for j in range(k)] for i in range(n)]


def drain(ds, n):
    return [ds[i] for i in range(n)]


def test_every_translation_carries_its_sources_vector():
    random.seed(0)
    teacher = DH.FakeTeacher()
    ds = data.ParallelSentencesDataset(None, teacher, batch_size=4)
    ps = parallel(6)
    ds.add_dataset(ps, weight=6)
    assert len(ds) == 18 and teacher.calls == 0            # nothing is encoded before the first example is asked for
    ex = drain(ds, 18)
    source_of = {s: row[0] for row in ps for s in row}
    assert sorted(e.texts[0] for e in ex) == sorted(source_of)     # the source and every translation, once each
    for e in ex:
        assert len(e.texts) == 1
        np.testing.assert_array_equal(e.label, DH.hash_vector(source_of[e.texts[0]]))
    # only source sentences went to the teacher, in batches of batch_size
    assert set(teacher.sentences) == {row[0] for row in ps} and teacher.batch_sizes == [4]
    # and they collate to what MSELoss takes
    labels = collate(ex[:5])[1]
    assert labels.shape == (5, 8) and labels.dtype == torch.float32


def test_the_embedding_cache_is_used():
    random.seed(1)
    for use_cache in (True, False):
        teacher = DH.FakeTeacher()
        ds = data.ParallelSentencesDataset(None, teacher, batch_size=8, use_embedding_cache=use_cache)
        ds.add_dataset(parallel(4), weight=4)
        drain(ds, 12)                                       # one round: every source once
        assert teacher.calls == 1 and len(teacher.sentences) == 4
        drain(ds, 12)                                       # a second round over the same sources
        if use_cache:
            assert teacher.calls == 1 and len(ds.embedding_cache) == 4
        else:
            assert teacher.calls == 2 and len(teacher.sentences) == 8 and not ds.embedding_cache
    # a source that occurs twice in one round is encoded once
    teacher = DH.FakeTeacher()
    ds = data.ParallelSentencesDataset(None, teacher)
    got = ds.get_embeddings(["a", "b", "a"])
    assert teacher.sentences == ["a", "b"] and np.array_equal(got[0], got[2]) and np.array_equal(got[1], DH.hash_vector("b"))


def test_weights_shape_the_draw():
    random.seed(2)
    ds = data.ParallelSentencesDataset(None, DH.FakeTeacher())
    ds.add_dataset(parallel(50, "x", k=0), weight=30)
    ds.add_dataset(parallel(50, "y", k=0), weight=10)
    assert len(ds) == 100
    ds.generate_data()
    tags = [e.texts[0][0] for e in ds.cache]
    assert tags.count("x") == 30 and tags.count("y") == 10          # one round = `weight` entries of each dataset
    assert tags != sorted(tags)                                     # ... shuffled
    # a dataset smaller than its weight wraps around and is reshuffled
    ds = data.ParallelSentencesDataset(None, DH.FakeTeacher())
    ds.add_dataset(parallel(3, "z", k=0), weight=7)
    ds.generate_data()
    assert len(ds.cache) == 7 and {e.texts[0] for e in ds.cache} == {f"z source {i}" for i in range(3)}


def test_max_sentences_and_max_sentence_length_filter():
    ds = data.ParallelSentencesDataset(None, DH.FakeTeacher())
    ps = [["short a", "kurz a"], ["short b", "x" * 40], ["y" * 40, "kurz c"], ["short d", "kurz d"], ["short e", "kurz e"]]
    ds.add_dataset(ps, weight=1, max_sentence_length=20)
    assert [src for src, _ in ds.datasets[0]] == ["short a", "short d", "short e"] and len(ds) == 6
    ds.add_dataset(ps, weight=1, max_sentences=2, max_sentence_length=20)
    assert [src for src, _ in ds.datasets[1]] == ["short a", "short d"] and len(ds) == 10
    ds.add_dataset(ps, weight=1, max_sentences=None, max_sentence_length=None)
    assert len(ds.datasets[2]) == 5
    # the same source twice: merged, duplicates among the translations dropped
    ds.add_dataset([["s", "t1"], ["s", "t2", "t1"]], weight=1)
    assert ds.datasets[3] == [("s", ["s", "t1", "t2"])]
    # nothing left: no dataset is added
    ds.add_dataset([["z" * 200]], weight=5)
    assert len(ds.datasets) == 4 and ds.dataset_indices == [0, 1, 2, 3]


def test_a_tsv_and_a_tsv_gz_load_the_same(tmp_path):
    ps = parallel(9) + [["w" * 300, "too long"]]
    text = "".join("\t".join(row) + "\n" for row in ps)
    (tmp_path / "p.tsv").write_text(text, encoding="utf8")
    with gzip.open(tmp_path / "p.tsv.gz", "wt", encoding="utf8") as f:
        f.write(text)
    loaded = []
    for name in ("p.tsv", "p.tsv.gz"):
        ds = data.ParallelSentencesDataset(None, DH.FakeTeacher())
        ds.load_data(str(tmp_path / name), weight=3, max_sentences=7)
        loaded.append((ds.datasets, ds.dataset_indices, len(ds)))
    assert loaded[0] == loaded[1]
    assert loaded[0][0] == [[(row[0], row) for row in ps[:7]]] and loaded[0][1] == [0, 0, 0] and loaded[0][2] == 21
