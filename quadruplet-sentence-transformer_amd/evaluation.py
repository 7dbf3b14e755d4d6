"""sentence_transformers.evaluation surface used by the reference's evaluators (models/evaluators.py:9-12,187-216,
572-612; ir_evauation_script.py:107-131): the base class, SimilarityFunction, SequentialEvaluator, an encode()-driven
TripletEvaluator and InformationRetrievalEvaluator, whose scoring + top-k run on the GPU
through libqst (util.topk_scores), EmbeddingSimilarityEvaluator (graded pairs; qst_pair_metric) and
ParaphraseMiningEvaluator (util.paraphrase_mining on the streaming top-k, qst_topk_stream), and the two that go with a
distillation, MSEEvaluator (qst_embed_mse) and TranslationEvaluator (two k = 1 searches of the streaming top-k), and
LabelAccuracyEvaluator, which scores the classifier of losses.SoftmaxLoss (qst_softmax_ce's counts), and
BinaryClassificationEvaluator for the contrastive pair losses (best accuracy and F1 cuts and the average precision of
four pair scores, counted without a sort by qst_binary_eval), and RerankingEvaluator for the ranking losses (MAP, MRR@k
and NDCG@k of every query's own candidate list: qst_rerank_scores and qst_rerank_metrics over ragged groups). The two
evaluators the reference selects its models with, QuadrupletEvaluator (qst_quadruplet_eval) and QuadrupletLossEvaluator, and the chain
get_sequential_evaluator builds of them stand at the end."""
from __future__ import annotations

import csv
import json
import logging
import os
import random
from enum import Enum
from typing import Callable, Dict, Iterable, List, Optional, Set

import numpy as np


class SentenceEvaluator:
    def __call__(self, model, output_path: str = None, epoch: int = -1, steps: int = -1) -> float:
        pass


class SimilarityFunction(Enum):
    COSINE = 0
    EUCLIDEAN = 1
    MANHATTAN = 2
    DOT_PRODUCT = 3


class SequentialEvaluator(SentenceEvaluator):
    """Runs evaluators in order; the main score is main_score_function(scores) (default: the last one)."""

    def __init__(self, evaluators: Iterable[SentenceEvaluator], main_score_function=lambda scores: scores[-1]):
        self.evaluators = list(evaluators)
        self.main_score_function = main_score_function

    def __call__(self, model, output_path: str = None, epoch: int = -1, steps: int = -1) -> float:
        scores = [ev(model, output_path, epoch, steps) for ev in self.evaluators]
        return self.main_score_function(scores)


class TripletEvaluator(SentenceEvaluator):
    """accuracy of d(anchor, positive) < d(anchor, negative) under cosine / manhattan / euclidean distance."""

    def __init__(self, anchors: List[str], positives: List[str], negatives: List[str], main_distance_function=None,
                 name: str = "", batch_size: int = 16, show_progress_bar: bool = False, write_csv: bool = True):
        assert len(anchors) == len(positives) == len(negatives)
        self.anchors, self.positives, self.negatives = anchors, positives, negatives
        self.main_distance_function = main_distance_function
        self.name, self.batch_size, self.show_progress_bar, self.write_csv = name, batch_size, show_progress_bar, write_csv
        self.csv_file = "triplet_evaluation" + ("_" + name if name else "") + "_results.csv"
        self.csv_headers = ["epoch", "steps", "accuracy_cosinus", "accuracy_manhattan", "accuracy_euclidean"]

    def __call__(self, model, output_path: str = None, epoch: int = -1, steps: int = -1) -> float:
        enc = lambda xs: np.asarray(model.encode(xs, batch_size=self.batch_size, show_progress_bar=self.show_progress_bar,
                                                 convert_to_numpy=True), dtype=np.float64)
        a, p, n = enc(self.anchors), enc(self.positives), enc(self.negatives)

        def cosd(x, y):
            return 1.0 - (x * y).sum(1) / (np.linalg.norm(x, axis=1) * np.linalg.norm(y, axis=1) + 1e-30)

        acc_cos = float(np.mean(cosd(a, p) < cosd(a, n)))
        acc_man = float(np.mean(np.abs(a - p).sum(1) < np.abs(a - n).sum(1)))
        acc_euc = float(np.mean(np.linalg.norm(a - p, axis=1) < np.linalg.norm(a - n, axis=1)))
        if output_path is not None and self.write_csv:
            path = os.path.join(output_path, self.csv_file)
            new = not os.path.isfile(path)
            with open(path, "a", newline="", encoding="utf-8") as f:
                w = csv.writer(f)
                if new:
                    w.writerow(self.csv_headers)
                w.writerow([epoch, steps, acc_cos, acc_man, acc_euc])
        if self.main_distance_function == SimilarityFunction.COSINE:
            return acc_cos
        if self.main_distance_function == SimilarityFunction.MANHATTAN:
            return acc_man
        if self.main_distance_function == SimilarityFunction.EUCLIDEAN:
            return acc_euc
        return max(acc_cos, acc_man, acc_euc)


def average_ranks(x) -> np.ndarray:
    """1-based ranks of x in ascending order, ties sharing the mean of the ranks they span (scipy.stats.rankdata)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    order = np.argsort(x, kind="mergesort")
    xs = x[order]
    starts = np.r_[True, xs[1:] != xs[:-1]]
    first = np.flatnonzero(starts)                              # first sorted position of every run of equal values
    last = np.r_[first[1:], len(xs)] - 1
    run = np.cumsum(starts) - 1
    ranks = np.empty(len(x), dtype=np.float64)
    ranks[order] = 0.5 * (first[run] + last[run]) + 1.0
    return ranks


def pearson(x, y) -> float:
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    xc, yc = x - x.mean(), y - y.mean()
    den = np.sqrt((xc * xc).sum() * (yc * yc).sum())
    return float((xc * yc).sum() / den) if den > 0 else float("nan")


def spearman(x, y) -> float:
    """Spearman's rank correlation: Pearson's r of the average ranks."""
    return pearson(average_ranks(x), average_ranks(y))


class EmbeddingSimilarityEvaluator(SentenceEvaluator):
    """The STS evaluator of sentence-transformers 2.2.2: encode both sentence lists, score every pair by cosine
    similarity, dot product and the negated Manhattan and Euclidean distances -- one qst_pair_metric launch per metric on
    the device (st_losses.pair_metric; the distances are sklearn's paired distances, without torch's eps) -- and report
    Pearson's and Spearman's correlation with the gold scores (host numpy; average ranks for ties). The return value is
    the Spearman correlation of `main_similarity`, or the largest of the four when it is None."""

    def __init__(self, sentences1: List[str], sentences2: List[str], scores: List[float], batch_size: int = 16,
                 main_similarity: Optional[SimilarityFunction] = None, name: str = "", show_progress_bar: bool = False,
                 write_csv: bool = True):
        assert len(sentences1) == len(sentences2) == len(scores)
        self.sentences1, self.sentences2, self.scores = sentences1, sentences2, scores
        self.batch_size, self.main_similarity, self.name = batch_size, main_similarity, name
        self.show_progress_bar, self.write_csv = show_progress_bar, write_csv
        self.csv_file = "similarity_evaluation" + ("_" + name if name else "") + "_results.csv"
        self.csv_headers = ["epoch", "steps", "cosine_pearson", "cosine_spearman", "euclidean_pearson", "euclidean_spearman",
                            "manhattan_pearson", "manhattan_spearman", "dot_pearson", "dot_spearman"]

    @classmethod
    def from_input_examples(cls, examples, **kwargs):
        return cls([ex.texts[0] for ex in examples], [ex.texts[1] for ex in examples], [ex.label for ex in examples],
                   **kwargs)

    def pair_scores(self, model) -> Dict[str, np.ndarray]:
        """{'cosine', 'euclidean', 'manhattan', 'dot'} -> the similarity of every pair (distances negated), fp32 from
        the device."""
        import torch
        from . import st_losses as S
        e1 = model.encode(self.sentences1, batch_size=self.batch_size, show_progress_bar=self.show_progress_bar,
                          convert_to_tensor=True)
        e2 = model.encode(self.sentences2, batch_size=self.batch_size, show_progress_bar=self.show_progress_bar,
                          convert_to_tensor=True)
        out = {}
        with torch.no_grad():
            for key, metric, sign in (("cosine", S.METRIC_COS_SIM, 1.0), ("euclidean", S.METRIC_L2_PLAIN, -1.0),
                                      ("manhattan", S.METRIC_L1_PLAIN, -1.0), ("dot", S.METRIC_DOT, 1.0)):
                out[key] = sign * S.pair_metric(e1, e2, metric).cpu().numpy()
        return out

    def __call__(self, model, output_path: str = None, epoch: int = -1, steps: int = -1) -> float:
        sims = self.pair_scores(model)
        res = {k: (pearson(self.scores, v), spearman(self.scores, v)) for k, v in sims.items()}
        if output_path is not None and self.write_csv:
            path = os.path.join(output_path, self.csv_file)
            new = not os.path.isfile(path)
            with open(path, "a", newline="", encoding="utf-8") as f:
                w = csv.writer(f)
                if new:
                    w.writerow(self.csv_headers)
                w.writerow([epoch, steps, *res["cosine"], *res["euclidean"], *res["manhattan"], *res["dot"]])
        by_fn = {SimilarityFunction.COSINE: "cosine", SimilarityFunction.EUCLIDEAN: "euclidean",
                 SimilarityFunction.MANHATTAN: "manhattan", SimilarityFunction.DOT_PRODUCT: "dot"}
        if self.main_similarity is None:
            return max(r[1] for r in res.values())
        if self.main_similarity not in by_fn:
            raise ValueError("Unknown main_similarity value")
        return res[by_fn[self.main_similarity]][1]


def ir_metrics(queries_result_list: List[List[dict]], queries_ids: List[str], relevant_docs: Dict[str, Set[str]],
               mrr_at_k: List[int], ndcg_at_k: List[int], accuracy_at_k: List[int], precision_recall_at_k: List[int],
               map_at_k: List[int]) -> dict:
    """Accuracy@k, Precision@k, Recall@k, MRR@k, NDCG@k (binary gains, log2 discount), MAP@k over ranked hit lists
    [{'corpus_id', 'score'}] (best first), with the definitions InformationRetrievalEvaluator.compute_metrics uses:
    MAP@k divides by min(k, |relevant|); a query with no hit in the top k contributes 0."""
    n = len(queries_ids)
    acc = {k: 0 for k in accuracy_at_k}
    prec = {k: [] for k in precision_recall_at_k}
    rec = {k: [] for k in precision_recall_at_k}
    mrr = {k: 0.0 for k in mrr_at_k}
    ndcg = {k: [] for k in ndcg_at_k}
    ap = {k: [] for k in map_at_k}
    for qi, qid in enumerate(queries_ids):
        hits = sorted(queries_result_list[qi], key=lambda h: h["score"], reverse=True)
        rel = relevant_docs[qid]
        flags = [h["corpus_id"] in rel for h in hits]
        for k in accuracy_at_k:
            acc[k] += int(any(flags[:k]))
        for k in precision_recall_at_k:
            c = sum(flags[:k])
            prec[k].append(c / k)
            rec[k].append(c / len(rel))
        for k in mrr_at_k:
            for rank, f in enumerate(flags[:k]):
                if f:
                    mrr[k] += 1.0 / (rank + 1)
                    break
        for k in ndcg_at_k:
            dcg = sum(1.0 / np.log2(r + 2) for r, f in enumerate(flags[:k]) if f)
            idcg = sum(1.0 / np.log2(r + 2) for r in range(min(k, len(rel))))
            ndcg[k].append(dcg / idcg if idcg > 0 else 0.0)
        for k in map_at_k:
            good, s_prec = 0, 0.0
            for rank, f in enumerate(flags[:k]):
                if f:
                    good += 1
                    s_prec += good / (rank + 1)
            ap[k].append(s_prec / min(k, len(rel)))
    return {"accuracy@k": {k: acc[k] / n for k in acc}, "precision@k": {k: float(np.mean(v)) for k, v in prec.items()},
            "recall@k": {k: float(np.mean(v)) for k, v in rec.items()}, "ndcg@k": {k: float(np.mean(v)) for k, v in ndcg.items()},
            "mrr@k": {k: mrr[k] / n for k in mrr}, "map@k": {k: float(np.mean(v)) for k, v in ap.items()}}


_KNOWN_SCORE_NAMES = {"cos_sim": 1, "dot_score": 0, "euclid_score": 2, "euclidean_score": 2}


def resolve_score_function(name: str, fn: Optional[Callable], device=None):
    """How one `score_functions` entry is evaluated: ("native", mode) = the fused libqst score + top-k kernel,
    ("callable", fn) = call fn(query_emb, corpus_emb) -> [nq, nc] and select with qst_topk_rows.

    Native is chosen by BEHAVIOUR, never by the dictionary key alone: this package's own util.cos_sim / dot_score /
    euclidean_score carry a mode tag; any other callable (e.g. the reference's `euclidean_score`,
    /root/reference/models/evaluators.py:392-405, which arrives as a foreign function object) is run once on a small
    fixed probe and taken over by the native mode whose score matrix it reproduces; a callable that matches none of
    them -- including a custom function registered under the name 'cos_sim' -- is called as given. `None` is accepted
    for the three known names."""
    import torch
    if fn is None:
        if name not in _KNOWN_SCORE_NAMES:
            raise ValueError(f"score function {name!r} is None: give a callable, or one of {sorted(_KNOWN_SCORE_NAMES)}")
        return ("native", _KNOWN_SCORE_NAMES[name])
    if not callable(fn):
        raise ValueError(f"score function {name!r} must be callable (got {type(fn).__name__})")
    mode = getattr(fn, "_qst_mode", None)
    if mode is not None:
        return ("native", int(mode))
    from . import util
    try:
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        g = torch.Generator().manual_seed(20240229)
        q = (torch.randn(6, 32, generator=g) * 1.7 + 0.3).to(dev)
        c = (torch.randn(9, 32, generator=g) * 0.6 - 0.2).to(dev)
        got = torch.as_tensor(fn(q, c)).to(dev, torch.float32)
        if tuple(got.shape) == (6, 9):
            for m in (1, 0, 2):
                ref = util.score_matrix(q, c, m)
                # split-bf16 x3 products are accurate to ~2^-17 of sum |a_k b_k|, i.e. relative to the matrix's scale,
                # not to each (possibly cancelling) entry; the three native modes differ by O(1) on this probe
                if float((got - ref).abs().max()) <= 2e-4 * max(1.0, float(ref.abs().max())):
                    return ("native", m)
    except Exception:          # a callable that cannot take the probe is simply called on the real embeddings later
        pass
    return ("callable", fn)


class InformationRetrievalEvaluator(SentenceEvaluator):
    """Queries against a corpus: encode both, score, keep the top max(k) hits per query across corpus chunks, report
    Accuracy/Precision/Recall/MRR/NDCG/MAP @k. Constructor, CSV layout and return value follow sentence-transformers
    2.2.2 as the reference drives it (models/evaluators.py:572-588, ir_evauation_script.py:107-131): the main score is
    max over score functions of MAP@max(map_at_k) unless main_score_function names one.

    score_functions is any {name: callable} dictionary, as in ST -- the reference always passes
    {'cos_sim': cos_sim, 'dot_score': dot_score, 'euclid_score': euclidean_score} (training/main.py:57,
    ir_evauation_script.py:71). Entries that are, or behave like, cosine / dot / 1/(1+L2) scoring run as ONE fused
    libqst call per corpus chunk (qst_topk_scores); any other callable is called and its matrix goes through
    qst_topk_rows (see resolve_score_function). Per-chunk results are merged by a second top-k over the candidates;
    only the metric arithmetic is host Python. Equal scores (duplicate documents) rank by corpus position, also at the
    max(k) cut and across chunks, and a NaN score of either sign ranks first: the hit lists do not depend on
    corpus_chunk_size."""

    def __init__(self, queries: Dict[str, str], corpus: Dict[str, str], relevant_docs: Dict[str, Set[str]],
                 corpus_chunk_size: int = 50000, mrr_at_k: List[int] = [10], ndcg_at_k: List[int] = [10],
                 accuracy_at_k: List[int] = [1, 3, 5, 10], precision_recall_at_k: List[int] = [1, 3, 5, 10],
                 map_at_k: List[int] = [100], show_progress_bar: bool = False, batch_size: int = 32, name: str = "",
                 write_csv: bool = True, score_functions: Optional[Dict[str, Callable]] = None,
                 main_score_function: Optional[str] = None):
        self.queries_ids = [qid for qid in queries if qid in relevant_docs and len(relevant_docs[qid]) > 0]
        self.queries = [queries[qid] for qid in self.queries_ids]
        self.corpus_ids = list(corpus.keys())
        self.corpus = [corpus[cid] for cid in self.corpus_ids]
        self.relevant_docs = relevant_docs
        self.corpus_chunk_size = corpus_chunk_size
        self.mrr_at_k, self.ndcg_at_k, self.accuracy_at_k = mrr_at_k, ndcg_at_k, accuracy_at_k
        self.precision_recall_at_k, self.map_at_k = precision_recall_at_k, map_at_k
        self.show_progress_bar, self.batch_size, self.name, self.write_csv = show_progress_bar, batch_size, name, write_csv
        if score_functions is None:              # ST's default: {'cos_sim': cos_sim, 'dot_score': dot_score}
            score_functions = {"cos_sim": None, "dot_score": None}
        self.score_functions = dict(score_functions)
        self.score_function_names = sorted(self.score_functions.keys())
        for nm, fn in self.score_functions.items():
            if fn is None and nm not in _KNOWN_SCORE_NAMES:
                raise ValueError(f"score function {nm!r} is None: give a callable, or one of {sorted(_KNOWN_SCORE_NAMES)}")
            if fn is not None and not callable(fn):
                raise ValueError(f"score function {nm!r} must be callable (got {type(fn).__name__})")
        self._resolved = None                    # name -> ("native", mode) | ("callable", fn); needs the device
        self.main_score_function = main_score_function
        self.csv_file = "Information-Retrieval_evaluation" + ("_" + name if name else "") + "_results.csv"
        self.csv_headers = ["epoch", "steps"]
        for nm in self.score_function_names:
            for k in accuracy_at_k:
                self.csv_headers.append(f"{nm}-Accuracy@{k}")
            for k in precision_recall_at_k:
                self.csv_headers.append(f"{nm}-Precision@{k}")
                self.csv_headers.append(f"{nm}-Recall@{k}")
            for k in mrr_at_k:
                self.csv_headers.append(f"{nm}-MRR@{k}")
            for k in ndcg_at_k:
                self.csv_headers.append(f"{nm}-NDCG@{k}")
            for k in map_at_k:
                self.csv_headers.append(f"{nm}-MAP@{k}")

    def __call__(self, model, output_path: str = None, epoch: int = -1, steps: int = -1, *args, **kwargs) -> float:
        scores = self.compute_metrices(model, *args, **kwargs)
        if output_path is not None and self.write_csv:
            path = os.path.join(output_path, self.csv_file)
            new = not os.path.isfile(path)
            with open(path, "a", newline="", encoding="utf-8") as f:
                w = csv.writer(f)
                if new:
                    w.writerow(self.csv_headers)
                row = [epoch, steps]
                for nm in self.score_function_names:
                    for k in self.accuracy_at_k:
                        row.append(scores[nm]["accuracy@k"][k])
                    for k in self.precision_recall_at_k:
                        row.append(scores[nm]["precision@k"][k])
                        row.append(scores[nm]["recall@k"][k])
                    for k in self.mrr_at_k:
                        row.append(scores[nm]["mrr@k"][k])
                    for k in self.ndcg_at_k:
                        row.append(scores[nm]["ndcg@k"][k])
                    for k in self.map_at_k:
                        row.append(scores[nm]["map@k"][k])
                w.writerow(row)
        if self.main_score_function is None:
            return max(scores[nm]["map@k"][max(self.map_at_k)] for nm in self.score_function_names)
        return scores[self.main_score_function]["map@k"][max(self.map_at_k)]

    def _embed(self, model, texts):
        return model.encode(texts, batch_size=self.batch_size, show_progress_bar=self.show_progress_bar,
                            convert_to_tensor=True)

    def compute_metrices(self, model, corpus_model=None, corpus_embeddings=None) -> Dict[str, dict]:
        import torch
        from . import util
        if corpus_model is None:
            corpus_model = model
        max_k = max(max(self.mrr_at_k), max(self.ndcg_at_k), max(self.accuracy_at_k), max(self.precision_recall_at_k),
                    max(self.map_at_k))
        q_emb = self._embed(model, self.queries)
        if self._resolved is None:
            self._resolved = {nm: resolve_score_function(nm, self.score_functions[nm], q_emb.device)
                              for nm in self.score_function_names}
        best = {nm: None for nm in self.score_function_names}        # name -> (scores [nq, <=max_k], corpus rows)
        for start in range(0, len(self.corpus), self.corpus_chunk_size):
            end = min(start + self.corpus_chunk_size, len(self.corpus))
            c_emb = corpus_embeddings[start:end] if corpus_embeddings is not None else \
                self._embed(corpus_model, self.corpus[start:end])
            c_emb = torch.as_tensor(c_emb).to(q_emb.device)
            k = min(max_k, end - start)
            for nm in self.score_function_names:
                kind, how = self._resolved[nm]
                if kind == "native":
                    sc, idx = util.topk_scores(q_emb, c_emb, k, mode=how)
                else:                                                # foreign callable: its matrix, our selection
                    full = torch.as_tensor(how(q_emb, c_emb)).to(q_emb.device, torch.float32)
                    if tuple(full.shape) != (q_emb.shape[0], c_emb.shape[0]):
                        raise ValueError(f"score function {nm!r} returned shape {tuple(full.shape)}, expected "
                                         f"{(q_emb.shape[0], c_emb.shape[0])}")
                    sc, idx = util.topk_rows(full, k)
                idx = idx + start
                if best[nm] is not None:                             # merge with the hits of earlier chunks
                    sc = torch.cat([best[nm][0], sc], dim=1)
                    idx = torch.cat([best[nm][1], idx], dim=1)
                    sc, idx = util.topk_rows(sc, min(max_k, sc.shape[1]), index_map=idx)
                best[nm] = (sc, idx)
        out = {}
        for nm in self.score_function_names:
            sc, idx = best[nm][0].cpu().numpy(), best[nm][1].cpu().numpy()
            # an id < 0 is an empty slot of the top-k (fewer candidates than k): it is no document
            results = [[{"corpus_id": self.corpus_ids[int(c)], "score": float(s)} for s, c in zip(sc[qi], idx[qi]) if c >= 0]
                       for qi in range(len(self.queries_ids))]
            out[nm] = ir_metrics(results, self.queries_ids, self.relevant_docs, self.mrr_at_k, self.ndcg_at_k,
                                 self.accuracy_at_k, self.precision_recall_at_k, self.map_at_k)
        return out


# ------------------------------------------------------------------ the quadruplet evaluators
LOGGER = logging.getLogger(__name__)


def _append_csv(path: str, headers: List[str], row: list) -> None:
    new = not os.path.isfile(path)
    with open(path, "a", newline="", encoding="utf-8") as f:
        w = csv.writer(f)
        if new:
            w.writerow(headers)
        w.writerow(row)


def paraphrase_metrics(pairs, ids, duplicates) -> Dict[str, float]:
    """The metrics of a mined pair list, host arithmetic only. pairs: [score, i, j] best first (util.paraphrase_mining),
    ids[i] the id of row i, duplicates: the set of gold pairs as frozensets of two ids. Walking the list, after the n-th
    pair precision = correct / n, recall = correct / len(duplicates), f1 their harmonic mean (0 where both are 0).
    average_precision sums the precision at the positions that are duplicates and divides by len(duplicates). The best
    f1 (the first, where several positions share it) keeps its precision and recall; its threshold is the mean of that
    pair's score and the next pair's, or the pair's own score at the end of the list. All zero for an empty list or no
    gold pairs."""
    out = {"precision": 0.0, "recall": 0.0, "f1": 0.0, "threshold": 0.0, "average_precision": 0.0}
    total = len(duplicates)
    if total == 0:
        return out
    correct, ap = 0, 0.0
    for n, (score, i, j) in enumerate(pairs, start=1):
        hit = frozenset((ids[i], ids[j])) in duplicates
        correct += int(hit)
        precision, recall = correct / n, correct / total
        f1 = 2 * correct / (n + total)          # = 2 P R / (P + R), in the form that gives equal cuts equal floats
        if hit:
            ap += precision
        if f1 > out["f1"]:
            nxt = pairs[n][0] if n < len(pairs) else score
            out.update(precision=precision, recall=recall, f1=f1, threshold=(score + nxt) / 2)
    out["average_precision"] = ap / total
    return out


def duplicate_closure(pairs) -> Set[frozenset]:
    """Every two members of a connected component of the duplicate graph count as duplicates: the gold pairs with their
    transitive closure, as frozensets of two ids."""
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for p in pairs:
        a, b = tuple(p)
        parent[find(a)] = find(b)
    groups = {}
    for x in list(parent):
        groups.setdefault(find(x), []).append(x)
    return {frozenset((g[a], g[b])) for g in groups.values() for a in range(len(g)) for b in range(a + 1, len(g))}


class ParaphraseMiningEvaluator(SentenceEvaluator):
    """sentence-transformers 2.2.2's ParaphraseMiningEvaluator: mine the most similar sentence pairs of `sentences_map`
    ({id: sentence}) with util.paraphrase_mining -- encode once, then for every sentence its top_k best others by the
    streaming top-k on the device -- and score the ranked pair list against the gold duplicates: precision, recall and
    F1 at the best-F1 cut, the score threshold of that cut, and the average precision, which is returned.

    Duplicates are unordered id pairs, given as duplicates_list [(id1, id2)] and / or duplicates_dict {id1: {id2: bool}};
    pairs that name an id outside sentences_map, or one id twice, are dropped. With add_transitive_closure every two
    members of a connected component count. The mined list does not depend on the chunk sizes (util.paraphrase_mining_
    embeddings says where that differs from ST)."""

    def __init__(self, sentences_map: Dict[str, str], duplicates_list=None, duplicates_dict=None,
                 add_transitive_closure: bool = False, query_chunk_size: int = 5000, corpus_chunk_size: int = 100000,
                 max_pairs: int = 500000, top_k: int = 100, show_progress_bar: bool = False, batch_size: int = 16,
                 name: str = "", write_csv: bool = True):
        if not sentences_map:
            raise ValueError("sentences_map is empty")
        if duplicates_list is None and duplicates_dict is None:
            raise ValueError("give the gold duplicates as duplicates_list and / or duplicates_dict")
        if not 1 <= top_k <= 1024:
            raise ValueError(f"top_k must be between 1 and 1024 (got {top_k})")
        if max_pairs < 1 or query_chunk_size < 1 or corpus_chunk_size < 1 or batch_size < 1:
            raise ValueError("max_pairs, query_chunk_size, corpus_chunk_size and batch_size must be positive")
        self.ids = list(sentences_map.keys())
        self.sentences = [sentences_map[i] for i in self.ids]
        gold = set()
        for a, b in (duplicates_list or []):
            gold.add(frozenset((a, b)))
        for a, others in (duplicates_dict or {}).items():
            for b, flag in others.items():
                if flag:
                    gold.add(frozenset((a, b)))
        gold = {p for p in gold if len(p) == 2 and all(x in sentences_map for x in p)}
        self.duplicates = duplicate_closure(gold) if add_transitive_closure else gold
        self.total_num_duplicates = len(self.duplicates)
        self.query_chunk_size, self.corpus_chunk_size = query_chunk_size, corpus_chunk_size
        self.max_pairs, self.top_k = max_pairs, top_k
        self.show_progress_bar, self.batch_size, self.name, self.write_csv = show_progress_bar, batch_size, name, write_csv
        self.csv_file = "paraphrase_mining_evaluation" + ("_" + name if name else "") + "_results.csv"
        self.csv_headers = ["epoch", "steps", "precision", "recall", "f1", "threshold", "average_precision"]

    def mine(self, model):
        from . import util
        return util.paraphrase_mining(model, self.sentences, self.show_progress_bar, self.batch_size,
                                      self.query_chunk_size, self.corpus_chunk_size, self.max_pairs, self.top_k)

    def __call__(self, model, output_path: str = None, epoch: int = -1, steps: int = -1) -> float:
        m = paraphrase_metrics(self.mine(model), self.ids, self.duplicates)
        LOGGER.info("ParaphraseMiningEvaluator %s: epoch %d, steps %d: AP %.4f, best F1 %.4f (precision %.4f, recall %.4f) "
                    "at threshold %.4f", self.name, epoch, steps, m["average_precision"], m["f1"], m["precision"],
                    m["recall"], m["threshold"])
        if output_path is not None and self.write_csv:
            _append_csv(os.path.join(output_path, self.csv_file), self.csv_headers,
                        [epoch, steps, m["precision"], m["recall"], m["f1"], m["threshold"], m["average_precision"]])
        return m["average_precision"]


class MSEEvaluator(SentenceEvaluator):
    """sentence-transformers 2.2.2's MSEEvaluator: the mean squared error, times 100, between the teacher's embeddings of
    `source_sentences` (taken once, here) and the evaluated model's embeddings of `target_sentences` -- the same sentences
    for a plain distillation, their translations for a multilingual student. One forward-only qst_embed_mse call
    (st_losses.embed_mse) on the device. Returns the negated value, so that higher is better."""

    def __init__(self, source_sentences: List[str], target_sentences: List[str], teacher_model=None,
                 show_progress_bar: bool = False, batch_size: int = 32, name: str = "", write_csv: bool = True):
        assert len(source_sentences) == len(target_sentences)
        self.source_embeddings = teacher_model.encode(source_sentences, show_progress_bar=show_progress_bar,
                                                      batch_size=batch_size, convert_to_numpy=True)
        self.target_sentences = target_sentences
        self.show_progress_bar, self.batch_size, self.name, self.write_csv = show_progress_bar, batch_size, name, write_csv
        self.csv_file = "mse_evaluation_" + name + "_results.csv"
        self.csv_headers = ["epoch", "steps", "MSE"]

    def mse(self, model) -> float:
        """100 * mean((teacher - student)^2) over every element."""
        import torch
        from . import st_losses as S
        target = model.encode(self.target_sentences, show_progress_bar=self.show_progress_bar, batch_size=self.batch_size,
                              convert_to_tensor=True)
        source = torch.as_tensor(np.asarray(self.source_embeddings, dtype=np.float32)).to(target.device)
        with torch.no_grad():
            return 100.0 * float(S.embed_mse(target, source).item())

    def __call__(self, model, output_path: str = None, epoch: int = -1, steps: int = -1) -> float:
        mse = self.mse(model)
        LOGGER.info("MSE evaluation (lower = better) on %s: MSE (*100): %.6f", self.name, mse)
        if output_path is not None and self.write_csv:
            _append_csv(os.path.join(output_path, self.csv_file), self.csv_headers, [epoch, steps, mse])
        return -mse


def translation_matches(source_embeddings, target_embeddings):
    """For every source row the target row with the largest cosine, and for every target row the source row: two int64
    tensors on the device, from two util.topk_stream(k=1, mode="cos") searches -- no [N, N] matrix is built. Among equal
    scores the smallest index wins, as np.argmax does."""
    from . import util
    _, s2t = util.topk_stream(source_embeddings, target_embeddings, 1, mode="cos")
    _, t2s = util.topk_stream(target_embeddings, source_embeddings, 1, mode="cos")
    return s2t[:, 0], t2s[:, 0]


class TranslationEvaluator(SentenceEvaluator):
    """sentence-transformers 2.2.2's TranslationEvaluator: source_sentences[i] and target_sentences[i] are translations of
    each other; the accuracy of finding, by cosine similarity, sentence i of the other language among all of them, in both
    directions (translation_matches). Returns the mean of the two accuracies."""

    def __init__(self, source_sentences: List[str], target_sentences: List[str], show_progress_bar: bool = False,
                 batch_size: int = 16, name: str = "", print_wrong_matches: bool = False, write_csv: bool = True):
        assert len(source_sentences) == len(target_sentences)
        self.source_sentences, self.target_sentences = source_sentences, target_sentences
        self.show_progress_bar, self.batch_size, self.name = show_progress_bar, batch_size, name
        self.print_wrong_matches, self.write_csv = print_wrong_matches, write_csv
        self.csv_file = "translation_evaluation" + ("_" + name if name else "") + "_results.csv"
        self.csv_headers = ["epoch", "steps", "src2trg", "trg2src"]

    def accuracies(self, model):
        """(src2trg, trg2src)"""
        enc = lambda xs: model.encode(xs, show_progress_bar=self.show_progress_bar, batch_size=self.batch_size,  # noqa: E731
                                      convert_to_tensor=True)
        s2t, t2s = (m.cpu().numpy() for m in translation_matches(enc(self.source_sentences), enc(self.target_sentences)))
        want = np.arange(len(self.source_sentences))
        if self.print_wrong_matches:
            for i in np.flatnonzero(s2t != want):
                print("i:", int(i), "j:", int(s2t[i]), "INCORRECT")
                print("Src:", self.source_sentences[i])
                print("Trg:", self.target_sentences[int(s2t[i])])
        return float(np.mean(s2t == want)), float(np.mean(t2s == want))

    def __call__(self, model, output_path: str = None, epoch: int = -1, steps: int = -1) -> float:
        acc_src2trg, acc_trg2src = self.accuracies(model)
        LOGGER.info("Translation evaluation on %s: src2trg %.2f trg2src %.2f", self.name, acc_src2trg * 100, acc_trg2src * 100)
        if output_path is not None and self.write_csv:
            _append_csv(os.path.join(output_path, self.csv_file), self.csv_headers, [epoch, steps, acc_src2trg, acc_trg2src])
        return (acc_src2trg + acc_trg2src) / 2


class LabelAccuracyEvaluator(SentenceEvaluator):
    """sentence-transformers 2.2.2's LabelAccuracyEvaluator: the share of a labelled dataset on which the largest logit of
    `softmax_model` (a losses.SoftmaxLoss; called with labels=None it returns the logits) is the label's. `dataloader` yields
    InputExamples with two texts and an integer label. The hits of every batch are counted by a forward-only qst_softmax_ce
    (st_losses.label_counts), summed on the device and read back once; among equal logits the lowest index is the
    prediction, as torch.argmax returns it."""

    def __init__(self, dataloader, name: str = "", softmax_model=None, write_csv: bool = True):
        self.dataloader = dataloader
        self.name = name
        self.softmax_model = softmax_model
        self.write_csv = write_csv
        self.csv_file = "accuracy_evaluation" + ("_" + name if name else "") + "_results.csv"
        self.csv_headers = ["epoch", "steps", "accuracy"]

    def __call__(self, model, output_path: str = None, epoch: int = -1, steps: int = -1) -> float:
        import torch
        from . import st_losses as S
        from .sentence_transformer import batch_to_device
        model.eval()
        self.dataloader.collate_fn = model.smart_batching_collate
        total, hits = 0, None
        for features, label_ids in self.dataloader:
            features = [batch_to_device(f, model.device) for f in features]
            label_ids = label_ids.to(model.device)
            with torch.no_grad():
                _, prediction = self.softmax_model(features, labels=None)
                counts = S.label_counts(prediction, label_ids)
            total += prediction.size(0)
            hits = counts[1:2].clone() if hits is None else hits + counts[1:2]
        correct = int(hits.item()) if hits is not None else 0
        accuracy = correct / total if total else 0.0
        LOGGER.info("Accuracy on %s: %.4f (%d/%d)", self.name, accuracy, correct, total)
        if output_path is not None and self.write_csv:
            _append_csv(os.path.join(output_path, self.csv_file), self.csv_headers, [epoch, steps, accuracy])
        return accuracy


def _binary_cuts_numpy(scores: np.ndarray, labels: np.ndarray, high_score_more_similar: bool) -> Dict[str, float]:
    """The best accuracy and F1 cuts of BinaryClassificationEvaluator on the host, in the counting form the kernel uses:
    the pairs take their places by a stable argsort, the positives before every cut are one cumulative sum, and both
    searches are a first argmax. The arithmetic is upstream's: the accuracy's count over n, c / e, c / T and
    2 * p * r / (p + r) in double, the thresholds in the scores' own type."""
    n = len(scores)
    res = dict(accuracy=0.0, accuracy_threshold=-1.0, f1=0.0, precision=0.0, recall=0.0, f1_threshold=0.0)
    if n < 2:
        return res
    order = np.argsort(-scores if high_score_more_similar else scores, kind="stable")
    s, y = scores[order], labels[order]
    total = int(y.sum())
    place = np.arange(1, n, dtype=np.int64)                     # pairs taken as positive by the cut behind row i
    hits = np.cumsum(y)[:-1]                                    # ... and the positives among them
    count = hits + (n - total) - (place - hits)
    r = int(np.argmax(count))
    if count[r] > 0:
        res["accuracy"] = float(count[r] / n)
        res["accuracy_threshold"] = float((s[r] + s[r + 1]) / 2)
    cuts = np.flatnonzero(hits > 0)
    if len(cuts):
        c = hits[cuts].astype(np.float64)
        precision, recall = c / place[cuts], c / float(total)
        f1 = 2 * precision * recall / (precision + recall)
        k = int(np.argmax(f1))
        r = int(cuts[k])
        res.update(f1=float(f1[k]), precision=float(precision[k]), recall=float(recall[k]),
                   f1_threshold=float((s[r] + s[r + 1]) / 2))
    return res


class BinaryClassificationEvaluator(SentenceEvaluator):
    """sentence-transformers 2.2.2's BinaryClassificationEvaluator, the one that goes with losses.ContrastiveLoss and
    OnlineContrastiveLoss: sentence pairs labelled 1 (similar) or 0, scored by cosine similarity, Manhattan and Euclidean
    distance and dot product; per score the cut of the sorted pairs with the best accuracy and the one with the best F1
    (with precision, recall and thresholds) and the average precision. The return value is the largest of the four
    average precisions. Every distinct sentence is encoded once, the four scores are one qst_pair_metric launch each and
    stay on the device, where ONE qst_binary_eval call (csrc/binary_eval.hip: an n x n counting pass, no sort) turns them
    into the 4 x 8 numbers that come back to the host; upstream sorts the pairs and walks them in Python twice per score.
    Up to 2^20 pairs."""

    _SCORES = ("cossim", "manhattan", "euclidean", "dot")
    _HIGH_IS_SIMILAR = (True, False, False, True)
    _METRICS = ("accuracy", "accuracy_threshold", "f1", "precision", "recall", "f1_threshold", "ap")

    def __init__(self, sentences1: List[str], sentences2: List[str], labels: List[int], name: str = "", batch_size: int = 32,
                 show_progress_bar: bool = False, write_csv: bool = True):
        self.sentences1, self.sentences2, self.labels = sentences1, sentences2, labels
        assert len(self.sentences1) == len(self.sentences2)
        assert len(self.sentences1) == len(self.labels)
        for label in labels:
            assert label == 0 or label == 1
        self.name, self.batch_size, self.write_csv = name, batch_size, write_csv
        if show_progress_bar is None:
            show_progress_bar = LOGGER.getEffectiveLevel() in (logging.INFO, logging.DEBUG)
        self.show_progress_bar = show_progress_bar
        self.csv_file = "binary_classification_evaluation" + ("_" + name if name else "") + "_results.csv"
        self.csv_headers = ["epoch", "steps"] + [f"{s}_{m}" for s in self._SCORES for m in self._METRICS]

    @classmethod
    def from_input_examples(cls, examples, **kwargs):
        return cls([ex.texts[0] for ex in examples], [ex.texts[1] for ex in examples], [ex.label for ex in examples],
                   **kwargs)

    def _device_scores(self, model):
        """fp32 [4, n] on the device, rows in the order of _SCORES; the distances as they are (a smaller one is more
        similar). The distinct sentences, in first-seen order, go through one encode call."""
        import torch
        from . import st_losses as S
        sentences = list(dict.fromkeys(list(self.sentences1) + list(self.sentences2)))
        emb = model.encode(sentences, batch_size=self.batch_size, show_progress_bar=self.show_progress_bar,
                           convert_to_tensor=True)
        index = {s: i for i, s in enumerate(sentences)}
        with torch.no_grad():
            e1 = emb.index_select(0, torch.tensor([index[s] for s in self.sentences1], dtype=torch.int64, device=emb.device))
            e2 = emb.index_select(0, torch.tensor([index[s] for s in self.sentences2], dtype=torch.int64, device=emb.device))
            rows = [S.pair_metric(e1, e2, m) for m in (S.METRIC_COS_SIM, S.METRIC_L1_PLAIN, S.METRIC_L2_PLAIN, S.METRIC_DOT)]
            return torch.stack(rows).to(torch.float32).contiguous()

    def pair_scores(self, model) -> Dict[str, np.ndarray]:
        """{'cossim', 'manhattan', 'euclidean', 'dot'} -> the score of every pair, fp32 from the device; the two distances
        are not negated."""
        return dict(zip(self._SCORES, self._device_scores(model).cpu().numpy()))

    def compute_metrices(self, model) -> Dict[str, Dict[str, float]]:
        import torch
        from . import _lib, st_losses as S
        n = len(self.sentences1)
        if n > S.BINARY_EVAL_MAX_PAIRS:
            raise _lib.QstError(f"BinaryClassificationEvaluator: {n} pairs; qst_binary_eval takes up to "
                                f"{S.BINARY_EVAL_MAX_PAIRS} (2^20)")
        scores = self._device_scores(model)
        labels = torch.as_tensor(np.asarray(self.labels, dtype=np.int64), device=scores.device)
        with torch.no_grad():
            out = S.binary_eval_raw(scores, labels, self._HIGH_IS_SIMILAR)
            finite = torch.isfinite(scores).all().to(torch.float64).reshape(1)
            host = torch.cat([out.reshape(-1), finite]).cpu().numpy()       # the one copy to the host
        if host[-1] == 0.0:
            raise ValueError("BinaryClassificationEvaluator: a pair's score is NaN or infinite; such scores have no order")
        table = host[:-1].reshape(len(self._SCORES), 8)
        result = {}
        for name, row in zip(self._SCORES, table):
            result[name] = {m: float(v) for m, v in zip(self._METRICS, row)}
            LOGGER.info("%s: accuracy %.2f (threshold %.4f), f1 %.2f (threshold %.4f), precision %.2f, recall %.2f, ap %.2f",
                        name, row[0] * 100, row[1], row[2] * 100, row[5], row[3] * 100, row[4] * 100, row[6] * 100)
        return result

    def __call__(self, model, output_path: str = None, epoch: int = -1, steps: int = -1) -> float:
        LOGGER.info("Binary accuracy evaluation of the model on %s dataset (epoch %s, steps %s)", self.name, epoch, steps)
        scores = self.compute_metrices(model)
        main_score = max(scores[name]["ap"] for name in scores)
        if output_path is not None and self.write_csv:
            row = [epoch, steps] + [scores[s][m] for s in self._SCORES for m in self._METRICS]
            _append_csv(os.path.join(output_path, self.csv_file), self.csv_headers, row)
        return main_score

    @staticmethod
    def _best_cuts(scores, labels, high_score_more_similar: bool) -> Dict[str, float]:
        """Both searches on array-likes (lists, numpy arrays, tensors). float32 scores go through qst_binary_eval when a
        HIP device is visible and the pairs fit it; anything else (no device, or scores of another type, whose thresholds
        upstream forms in that type) through the numpy restatement."""
        import torch
        from . import st_losses as S
        to_numpy = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)  # noqa: E731
        s, y = to_numpy(scores).reshape(-1), to_numpy(labels).reshape(-1)
        if len(s) != len(y):
            raise ValueError(f"{len(s)} scores but {len(y)} labels")
        if not np.issubdtype(s.dtype, np.floating):
            s = s.astype(np.float64)
        if not np.isfinite(s).all():
            raise ValueError("a score is NaN or infinite; such scores have no order")
        if not np.isin(y, (0, 1)).all():
            raise ValueError("the labels must be 0 or 1")
        y = y.astype(np.int64)
        if s.dtype == np.float32 and 1 <= len(s) <= S.BINARY_EVAL_MAX_PAIRS and torch.cuda.is_available():
            out = S.binary_eval_raw(torch.from_numpy(np.ascontiguousarray(s)).cuda().view(1, -1),
                                    torch.from_numpy(np.ascontiguousarray(y)).cuda(), [high_score_more_similar])
            return dict(zip(BinaryClassificationEvaluator._METRICS, out.cpu().numpy()[0, :6].tolist()))
        return _binary_cuts_numpy(s, y, bool(high_score_more_similar))

    @staticmethod
    def find_best_acc_and_threshold(scores, labels, high_score_more_similar: bool):
        """(the best accuracy, its threshold) of upstream's walk over the sorted pairs."""
        r = BinaryClassificationEvaluator._best_cuts(scores, labels, high_score_more_similar)
        return r["accuracy"], r["accuracy_threshold"]

    @staticmethod
    def find_best_f1_and_threshold(scores, labels, high_score_more_similar: bool):
        """(the best F1, its precision, its recall, its threshold) of upstream's walk over the sorted pairs."""
        r = BinaryClassificationEvaluator._best_cuts(scores, labels, high_score_more_similar)
        return r["f1"], r["precision"], r["recall"], r["f1_threshold"]


def cos_sim(a, b):
    """util.cos_sim, bound on the first call (util brings torch in; this module does not): RerankingEvaluator's default
    similarity_fct, with util.cos_sim's mode tag."""
    from . import util
    return util.cos_sim(a, b)


cos_sim._qst_mode = 1


class RerankingEvaluator(SentenceEvaluator):
    """sentence-transformers 2.2.2's RerankingEvaluator, the one the re-ranking and unsupervised recipes select their
    checkpoints with: samples {'query': str, 'positive': [str, ...], 'negative': [str, ...]}; every query's candidates are
    ranked by similarity_fct and the mean average precision (the return value) and MRR@mrr_at_k are reported;
    compute_metrices adds NDCG@mrr_at_k, which upstream gained later. Every distinct text, queries and documents together,
    goes through ONE encode call; the candidates of all queries form one flat array with ragged groups, scored by one
    qst_rerank_scores launch (cosine, dot product or the Euclidean score; any other callable is called once per query, as
    upstream calls it, and its results are concatenated on the device) and turned into the metrics by one
    qst_rerank_metrics call (csrc/rerank.hip: counts per positive, no sort); five numbers come back to the host. Upstream
    runs a cos_sim, an argsort, a Python walk and an sklearn call per query.

    Equal scores: the document that comes first in positive + negative ranks first (a stable descending sort). Upstream's
    torch.argsort(-scores) is not stable, so it gives no rule to reproduce; the average precision does not depend on it.
    Samples without a positive or without a negative are dropped, as upstream drops them. use_batched_encoding is accepted
    for the signature and changes nothing: the texts are always encoded in one batched call."""

    def __init__(self, samples, mrr_at_k: int = 10, name: str = "", write_csv: bool = True, similarity_fct=cos_sim,
                 batch_size: int = 64, show_progress_bar: bool = False, use_batched_encoding: bool = True):
        self.samples = samples
        self.name, self.mrr_at_k, self.similarity_fct = name, mrr_at_k, similarity_fct
        self.batch_size, self.show_progress_bar, self.use_batched_encoding = batch_size, show_progress_bar, use_batched_encoding
        if isinstance(self.samples, dict):
            self.samples = list(self.samples.values())
        self.samples = [s for s in self.samples if len(s["positive"]) > 0 and len(s["negative"]) > 0]
        self.csv_file = "RerankingEvaluator" + ("_" + name if name else "") + "_results.csv"
        self.csv_headers = ["epoch", "steps", "MAP", "MRR@{}".format(mrr_at_k)]
        self.write_csv = write_csv

    def _groups(self):
        """(offsets [nq + 1], num_pos [nq]) of the flat document array: a query's positives, then its negatives."""
        sizes = [len(s["positive"]) + len(s["negative"]) for s in self.samples]
        offsets = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.int64)
        return offsets, np.asarray([len(s["positive"]) for s in self.samples], dtype=np.int32)

    def _device_scores(self, model):
        """(scores fp32 [nd] on the device, offsets, num_pos). The distinct texts, in first-seen order, go through one encode
        call; the flat query and document arrays are index_selects of its result."""
        import torch
        from . import util
        if not self.samples:
            raise ValueError("RerankingEvaluator: no sample has both a positive and a negative document")
        queries = [s["query"] for s in self.samples]
        docs = [t for s in self.samples for t in list(s["positive"]) + list(s["negative"])]
        texts = list(dict.fromkeys(queries + docs))
        emb = model.encode(texts, batch_size=self.batch_size, show_progress_bar=self.show_progress_bar, convert_to_tensor=True)
        index = {t: i for i, t in enumerate(texts)}
        offsets, num_pos = self._groups()
        with torch.no_grad():
            q = emb.index_select(0, torch.tensor([index[t] for t in queries], dtype=torch.int64, device=emb.device))
            d = emb.index_select(0, torch.tensor([index[t] for t in docs], dtype=torch.int64, device=emb.device))
            how, fn = resolve_score_function(getattr(self.similarity_fct, "__name__", "similarity_fct"), self.similarity_fct,
                                             emb.device)
            if how == "native":
                scores = util.rerank_scores(q, d, offsets, fn)
            else:
                rows = []
                for g in range(len(queries)):
                    r = torch.as_tensor(fn(q[g], d[offsets[g]:offsets[g + 1]]))
                    rows.append((r[0] if r.dim() == 2 else r).reshape(-1).to(emb.device, torch.float32))
                scores = torch.cat(rows)
                if scores.numel() != len(docs):
                    raise ValueError(f"RerankingEvaluator: similarity_fct returned {scores.numel()} scores for {len(docs)} documents")
        return scores, offsets, num_pos

    def _metrics(self, model, want_table: bool = False):
        import torch
        from . import _lib, util
        scores, offsets, num_pos = self._device_scores(model)
        with torch.no_grad():
            per_query, out = util.rerank_metrics(scores, offsets, num_pos, self.mrr_at_k)
            host = out.cpu().numpy()                                # the one copy to the host
        if host[3] > 0:
            raise ValueError(f"RerankingEvaluator: {int(host[3])} scores are NaN or infinite; such scores have no rank")
        if host[4] > 0:
            raise _lib.QstError(f"RerankingEvaluator: qst_rerank_metrics could not use {int(host[4])} of {len(self.samples)} groups")
        return host, (per_query.cpu().numpy() if want_table else None)

    def compute_metrices(self, model) -> Dict[str, float]:
        """{'map', 'mrr', 'ndcg'}: the means over the queries; mrr and ndcg within mrr_at_k."""
        host, _ = self._metrics(model)
        return {"map": float(host[1]), "mrr": float(host[0]), "ndcg": float(host[2])}

    def per_query_metrics(self, model) -> np.ndarray:
        """float64 [nq, 3]: {reciprocal rank within mrr_at_k, average precision, NDCG within mrr_at_k} of every query, in
        the order of the samples."""
        return self._metrics(model, want_table=True)[1]

    def __call__(self, model, output_path: str = None, epoch: int = -1, steps: int = -1) -> float:
        if epoch != -1:
            out_txt = " after epoch {}:".format(epoch) if steps == -1 else " in epoch {} after {} steps:".format(epoch, steps)
        else:
            out_txt = ":"
        LOGGER.info("RerankingEvaluator: Evaluating the model on " + self.name + " dataset" + out_txt)
        scores = self.compute_metrices(model)
        mean_ap, mean_mrr = scores["map"], scores["mrr"]
        num_positives = [len(s["positive"]) for s in self.samples]
        num_negatives = [len(s["negative"]) for s in self.samples]
        LOGGER.info("Queries: {} \t Positives: Min {:.1f}, Mean {:.1f}, Max {:.1f} \t Negatives: Min {:.1f}, Mean {:.1f}, "
                    "Max {:.1f}".format(len(self.samples), np.min(num_positives), np.mean(num_positives), np.max(num_positives),
                                        np.min(num_negatives), np.mean(num_negatives), np.max(num_negatives)))
        LOGGER.info("MAP: {:.2f}".format(mean_ap * 100))
        LOGGER.info("MRR@{}: {:.2f}".format(self.mrr_at_k, mean_mrr * 100))
        if output_path is not None and self.write_csv:
            _append_csv(os.path.join(output_path, self.csv_file), self.csv_headers, [epoch, steps, mean_ap, mean_mrr])
        return mean_ap


def _unwrap_example(example):
    """An (example, label) row gives its example."""
    return example[0] if isinstance(example, tuple) else example


def sample_quadruplets(examples):
    """(anchors, positives, partially positives, negatives) of rows that are objects with four `texts`, (example, label)
    tuples, or quadruplet dicts (quadruplet_model's keys); where a dict holds a list, one entry is drawn with `random`
    (positive, then partially positive, then negative: one draw each, in that order)."""
    from .quadruplet_model import NEG_EXAMPLES, PART_POS_EXAMPLES, POS_EXAMPLES, REFERENCE_EXAMPLE
    cols = ([], [], [], [])
    for example in examples:
        example = _unwrap_example(example)
        if hasattr(example, "texts"):
            if len(example.texts) < 4:
                raise ValueError(f"a quadruplet example needs four texts, {len(example.texts)} given")
            for col, text in zip(cols, example.texts[:4]):
                col.append(text)
            continue
        cols[0].append(example[REFERENCE_EXAMPLE])
        for col, key in zip(cols[1:], (POS_EXAMPLES, PART_POS_EXAMPLES, NEG_EXAMPLES)):
            v = example[key]
            col.append(v[random.randint(0, len(v) - 1)] if isinstance(v, list) else v)
    return cols


class QuadrupletEvaluator(SentenceEvaluator):
    """Quadruplets (sentence, positive, partially positive, negative): the accuracies of
        pos_part  d(sentence, positive) < d(sentence, partially positive)
        pos_neg   d(sentence, positive) < d(sentence, negative)
        part_neg  d(sentence, partially positive) < d(sentence, negative)
    each under cosine, Manhattan and Euclidean distance, and the score
        ((1 - gamma) * pos_part + gamma * part_neg + pos_neg) / 2,
    where each of the three is the accuracy `main_distance_function` names, or the largest of its three when that is None
    (TripletEvaluator's rule). Constructor, attributes, CSV files and return value are the reference's, which composes the
    score from three TripletEvaluators: nine encodes of four distinct lists, and nine distances per row in host numpy. Here
    every list is encoded once, the embeddings stay on the device, and ONE qst_quadruplet_eval launch returns the nine
    counts -- all that comes back to the host.

    With `all_examples` (from_input_examples keeps its argument there) the four lists are drawn again on every fifth call."""

    N_EPOCHS_RESET_EXAMPLES = 5
    _TRIPLETS = ("pos_part", "pos_neg", "part_neg")

    def __init__(self, anchors: List[str], positives: List[str], partially_positives: List[str], negatives: List[str],
                 gamma: float = 0.6, main_distance_function: Optional[SimilarityFunction] = None, name: str = "",
                 batch_size: int = 16, show_progress_bar: bool = False, write_csv: bool = True, all_examples=None):
        self.anchors, self.positives = anchors, positives
        self.partially_positives, self.negatives = partially_positives, negatives
        self.name = name
        self._gamma = gamma
        self._all_examples = all_examples
        assert len(self.anchors) == len(self.positives)
        assert len(self.anchors) == len(self.partially_positives)
        assert len(self.anchors) == len(self.negatives)
        self.main_distance_function = main_distance_function
        self.batch_size = batch_size
        if show_progress_bar is None:
            show_progress_bar = LOGGER.getEffectiveLevel() in (logging.INFO, logging.DEBUG)
        self.show_progress_bar = show_progress_bar
        self.write_csv = write_csv
        self.csv_file = "quadruplet_evaluation" + ("_" + name if name else "") + "_results.csv"
        self.csv_headers = ["epoch", "steps", "pos_part_accuracy", "pos_neg_accuracy", "part_neg_accuracy", "global_accuracy"]
        # the per-triplet files the reference's three TripletEvaluators (named pos_part, pos_neg, part_neg) leave
        self.triplet_csv_files = [f"triplet_evaluation_{t}_results.csv" for t in self._TRIPLETS]
        self.triplet_csv_headers = ["epoch", "steps", "accuracy_cosinus", "accuracy_manhattan", "accuracy_euclidean"]
        self._epoch_counter = 0

    @classmethod
    def from_input_examples(cls, examples, **kwargs):
        return cls(*sample_quadruplets(examples), all_examples=examples, **kwargs)

    def _reset_examples(self) -> None:
        self._epoch_counter += 1
        if self._all_examples is not None and self._epoch_counter % self.N_EPOCHS_RESET_EXAMPLES == 0:
            self.anchors, self.positives, self.partially_positives, self.negatives = sample_quadruplets(self._all_examples)

    def quadruplet_counts(self, model):
        """The device step: (counts[9], N) with counts[3 * metric + j] = rows on which comparison j (pos_part, pos_neg,
        part_neg) holds under metric 0 cosine, 1 Manhattan, 2 Euclidean. Four encodes, one launch, nine integers back."""
        import torch
        from . import st_losses as S
        embs = [model.encode(xs, batch_size=self.batch_size, show_progress_bar=self.show_progress_bar, convert_to_tensor=True)
                for xs in (self.anchors, self.positives, self.partially_positives, self.negatives)]
        with torch.no_grad():
            _, _, counts = S.quadruplet_eval(*embs)
        return counts.cpu().numpy().astype(np.int64), len(self.anchors)

    def _main_accuracy(self, acc_cos: float, acc_man: float, acc_euc: float) -> float:
        if self.main_distance_function == SimilarityFunction.COSINE:
            return acc_cos
        if self.main_distance_function == SimilarityFunction.MANHATTAN:
            return acc_man
        if self.main_distance_function == SimilarityFunction.EUCLIDEAN:
            return acc_euc
        return max(acc_cos, acc_man, acc_euc)

    def __call__(self, model, output_path: str = None, epoch: int = -1, steps: int = -1) -> float:
        self._reset_examples()
        LOGGER.info("QuadrupletEvaluator %s: epoch %d, steps %d", self.name, epoch, steps)
        counts, n = self.quadruplet_counts(model)
        counts = np.asarray(counts, dtype=np.float64).reshape(3, 3)      # [metric, comparison]
        write = output_path is not None and self.write_csv
        main = []
        for j, fname in enumerate(self.triplet_csv_files):
            acc = [float(counts[m, j] / n) for m in range(3)]            # cosine, Manhattan, Euclidean: the CSV's columns
            if write:
                _append_csv(os.path.join(output_path, fname), self.triplet_csv_headers, [epoch, steps, *acc])
            main.append(self._main_accuracy(*acc))
        pos_part, pos_neg, part_neg = main
        glob = ((1 - self._gamma) * pos_part + self._gamma * part_neg + pos_neg) / 2
        LOGGER.info("accuracy %%: pos_part %.2f, pos_neg %.2f, part_neg %.2f, global %.2f", pos_part * 100, pos_neg * 100,
                    part_neg * 100, glob * 100)
        if write:
            _append_csv(os.path.join(output_path, self.csv_file), self.csv_headers,
                        [epoch, steps, pos_part, pos_neg, part_neg, glob])
        return glob


class QuadrupletLossEvaluator(SentenceEvaluator):
    """The mean quadruplet loss over a dataset, batch by batch, under torch.no_grad(): the running mean
    avg += (loss - avg) / (i + 1) of QuadrupletSentenceTransformerLossModel(model, quadruplet_loss) (one fused encoder pass
    per batch) over an unshuffled DataLoader. The mean stays a device tensor; the host waits for it once, at the end, to log
    it. Rows are InputExamples with four texts, (example, label) tuples, or quadruplet dicts (to_input_example).

    The model's mode is left as it is: inside fit() the model is in train() mode, so this loss is taken with dropout, as the
    reference takes it (SentenceTransformer.forward supports exactly that pass); call model.eval() first for a
    deterministic figure.

    With output_path, epoch / steps / average_loss are appended to <output_path>/_quadruplet_loss_eval.json. With
    output_path=None nothing is written and the loss is returned (the reference raises there, joining None with the file
    name).

    use_amp is accepted and stored for the reference's signature. There is no autocast on this path: the pass runs at the
    precision the model's forward is using, which inside fit(use_amp=True) already is f16.

    Returns the mean as a 0-d tensor on the model's device (the reference returns its tensor too)."""

    LOG_FILE = "_quadruplet_loss_eval.json"

    def __init__(self, quadruplet_dataset, quadruplet_loss, batch_size: int = 32,
                 additional_model_kwargs: Optional[List[str]] = None, additional_loss_kwargs: Optional[List[str]] = None,
                 use_amp: bool = False):
        self._quadruplet_dataset = quadruplet_dataset
        self._quadruplet_loss = quadruplet_loss
        self._batch_size = batch_size
        self._additional_model_kwargs = additional_model_kwargs
        self._additional_loss_kwargs = additional_loss_kwargs
        self._use_amp = use_amp

    def __call__(self, model, output_path: str = None, epoch: int = -1, steps: int = -1):
        import torch
        from torch.utils.data import DataLoader
        from .quadruplet_model import QuadrupletSentenceTransformerLossModel, to_input_example
        from .sentence_transformer import batch_to_device
        loss_model = QuadrupletSentenceTransformerLossModel(
            st_model=model, quadruplet_loss=self._quadruplet_loss, additional_model_kwargs=self._additional_model_kwargs,
            additional_loss_kwargs=self._additional_loss_kwargs)

        def collate(batch):
            rows = [_unwrap_example(b) for b in batch]
            return model.smart_batching_collate([r if hasattr(r, "texts") else to_input_example(r) for r in rows])

        loader = DataLoader(self._quadruplet_dataset, batch_size=self._batch_size, shuffle=False, collate_fn=collate)
        avg = torch.zeros((), dtype=torch.float32, device=model.device)
        with torch.no_grad():
            for i, (features, labels) in enumerate(loader):
                features = [batch_to_device(f, model.device) for f in features]
                loss_value = loss_model(features, labels.to(model.device))
                avg += (loss_value.detach().to(torch.float32).mean() - avg) / (i + 1)
        if output_path is not None:
            path = os.path.join(output_path, self.LOG_FILE)
            log = {}
            if os.path.exists(path):
                with open(path, "r") as fp:
                    log = json.load(fp)
            for k, v in (("epoch", epoch), ("steps", steps), ("average_loss", avg.item())):
                log.setdefault(k, []).append(v)
            with open(path, "w") as fp:
                json.dump(log, fp, indent=2)
        return avg


def get_sequential_evaluator(dataset, loss, evaluation_queries_path: Optional[str] = None, no_transform_dataset=None,
                             corpus_chunk_size: int = 50000, mrr_at_k: List[int] = [10], ndcg_at_k: List[int] = [10],
                             accuracy_at_k: List[int] = [1, 3, 5, 10], precision_recall_at_k: List[int] = [1, 3, 5, 10],
                             map_at_k: List[int] = [100], show_progress_bar: bool = False, batch_size: int = 32,
                             write_csv: bool = True, score_functions: Optional[Dict[str, Callable]] = None,
                             main_score_function: Optional[str] = None,
                             main_distance_function: Optional[SimilarityFunction] = None, name: str = "",
                             additional_model_kwargs: Optional[List[str]] = None,
                             additional_loss_kwargs: Optional[List[str]] = None, use_amp: bool = False) -> SequentialEvaluator:
    """SequentialEvaluator([InformationRetrievalEvaluator?, QuadrupletEvaluator, QuadrupletLossEvaluator]) over `dataset`
    with `loss` (its gamma weights the accuracy): the loss evaluator is last, so its value is the chain's score.

    The retrieval evaluator is built only from `evaluation_queries_path`, a JSON file {"queries": {qid: text}, "corpus":
    {cid: text}, "relevant": {qid: [cid, ...]}}. score_functions=None stands for {'cos_sim', 'dot_score'}, the two this
    package scores natively. Building the query set from `no_transform_dataset` (the reference's create_ir_evaluation_set:
    a cross-encoder scores a sampled corpus) is not done here: with that argument and no readable file the call raises."""
    evaluation_queries = None
    if evaluation_queries_path is not None:
        try:
            with open(evaluation_queries_path, "r") as fp:
                evaluation_queries = json.load(fp)
            # The evaluator takes a set per query. (The reference converts the whole `relevant` mapping -- its keys, the query
            # ids -- for every query instead of the query's own list; each query gets its own list here.)
            evaluation_queries["relevant"] = {q: set(docs) for q, docs in evaluation_queries["relevant"].items()}
        except IOError as e:
            evaluation_queries = None
            print(f"Error: {evaluation_queries_path} file could not be opened due to error: {e}")
    if evaluation_queries is None and no_transform_dataset is not None:
        raise NotImplementedError("get_sequential_evaluator: no readable evaluation_queries_path, and building the retrieval "
                                  "set from no_transform_dataset (create_ir_evaluation_set: cross-encoder scoring of a "
                                  "sampled corpus) is not implemented; write the queries file first")
    evaluators = []
    if evaluation_queries is not None:
        evaluators.append(InformationRetrievalEvaluator(
            queries=evaluation_queries["queries"], corpus=evaluation_queries["corpus"],
            relevant_docs=evaluation_queries["relevant"], corpus_chunk_size=corpus_chunk_size, mrr_at_k=mrr_at_k,
            ndcg_at_k=ndcg_at_k, accuracy_at_k=accuracy_at_k, precision_recall_at_k=precision_recall_at_k, map_at_k=map_at_k,
            show_progress_bar=show_progress_bar, batch_size=batch_size, name=name, write_csv=write_csv,
            score_functions=score_functions, main_score_function=main_score_function))
    evaluators.append(QuadrupletEvaluator.from_input_examples(
        dataset, gamma=loss.gamma, main_distance_function=main_distance_function, name=name, batch_size=batch_size,
        show_progress_bar=show_progress_bar, write_csv=write_csv))
    evaluators.append(QuadrupletLossEvaluator(
        quadruplet_dataset=dataset, quadruplet_loss=loss, additional_model_kwargs=additional_model_kwargs,
        additional_loss_kwargs=additional_loss_kwargs, use_amp=use_amp, batch_size=batch_size))
    return SequentialEvaluator(evaluators=evaluators)
