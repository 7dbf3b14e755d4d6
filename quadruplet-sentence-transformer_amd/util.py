"""sentence_transformers.util functions the reference imports (training/main.py:6, models/evaluators.py:9-12):
cos_sim, dot_score, batch_to_device -- plus euclidean_score, the reference's own third score function
(models/evaluators.py:392-405). All three score matrices come from libqst (qst_score_matrix: row normalisation, the
split-bf16 x3 GEMM or the direct-difference Euclidean kernel); there is no torch arithmetic and no CPU path here.
semantic_search, paraphrase_mining and paraphrase_mining_embeddings (ST 2.2.2 signatures) stand on the streaming top-k
(qst_topk_stream / qst_topk_merge_rows); of them only merge_mined_pairs, the pair bookkeeping, is host numpy.
community_detection (ST 2.2.2) counts, extracts and claims on the device (qst_community_*), with no n x n matrix; its
candidate order, round planning and the final order inside a community are host numpy. rerank_scores and rerank_metrics
(qst_rerank_*) score and rank every query's own candidate list, ragged groups of one flat array, for RerankingEvaluator."""
from __future__ import annotations

import numpy as np
import torch

from .sentence_transformer import batch_to_device  # noqa: F401

SCORE_DOT, SCORE_COS, SCORE_EUCLID = 0, 1, 2
_MODES = {"dot": SCORE_DOT, "dot_score": SCORE_DOT, "cos": SCORE_COS, "cos_sim": SCORE_COS, "cosine": SCORE_COS,
          "euclid": SCORE_EUCLID, "euclid_score": SCORE_EUCLID, "euclidean_score": SCORE_EUCLID}


def _mode(m) -> int:
    if isinstance(m, str):
        return _MODES[m]
    if isinstance(m, bool):
        return SCORE_COS if m else SCORE_DOT
    return int(m)


def _as_2d(x):
    if not isinstance(x, torch.Tensor):
        x = torch.tensor(np.asarray(x))
    if x.dim() == 1:
        x = x.unsqueeze(0)
    return x


def _device_rows(x, dev=None):
    """fp32 contiguous rows on the HIP device, feature dimension zero-padded to a multiple of 32 (zeros change none of
    the three scores). Host tensors are moved: the arithmetic runs in libqst either way."""
    from . import _lib
    x = _as_2d(x)
    if not x.is_cuda:
        if not torch.cuda.is_available():
            raise _lib.QstError("score functions run on the HIP device and none is visible (there is no CPU path)")
        x = x.to(dev if dev is not None else torch.device("cuda", torch.cuda.current_device()))
    x = x.to(torch.float32)
    pad = (-x.shape[1]) % 32
    if pad:
        x = torch.nn.functional.pad(x, (0, pad))
    return x.contiguous()


def score_matrix(a, b, mode) -> torch.Tensor:
    """[len(a), len(b)] scores: mode 'dot' | 'cos' | 'euclid' (libqst qst_score_matrix). The result lives where `a` did."""
    from . import _lib
    lib = _lib.load()
    a0 = _as_2d(a)
    q = _device_rows(a0)
    c = _device_rows(b, q.device)
    if c.device != q.device:
        c = c.to(q.device)
    if q.shape[1] != c.shape[1]:
        raise ValueError(f"embedding sizes differ: {tuple(_as_2d(a).shape)} vs {tuple(_as_2d(b).shape)}")
    nq, dim = q.shape
    nc = c.shape[0]
    ld = (nc + 3) // 4 * 4
    with torch.cuda.device(q.device):
        out = torch.empty(nq, ld, dtype=torch.float32, device=q.device)
        ws = torch.empty(lib.qst_score_workspace_bytes(nq, nc, dim), dtype=torch.uint8, device=q.device)
        _lib.check(lib.qst_score_matrix(q.data_ptr(), c.data_ptr(), nq, nc, dim, _mode(mode), out.data_ptr(), ld,
                                        ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()), "qst_score_matrix")
    out = out[:, :nc]
    return out if a0.is_cuda else out.cpu()


def cos_sim(a, b) -> torch.Tensor:
    return score_matrix(a, b, SCORE_COS)


pytorch_cos_sim = cos_sim


def dot_score(a, b) -> torch.Tensor:
    return score_matrix(a, b, SCORE_DOT)


def euclidean_score(a, b) -> torch.Tensor:
    """1 / (1 + ||a_i - b_j||_2): /root/reference/models/evaluators.py:392-405."""
    return score_matrix(a, b, SCORE_EUCLID)


def pairwise_dot_score(a, b) -> torch.Tensor:
    """sentence_transformers.util.pairwise_dot_score: the dot product of row i of `a` with row i of `b`, [B]
    (qst_pair_metric with its autograd; HIP tensors only)."""
    from . import st_losses
    return st_losses.pair_metric(a, b, st_losses.METRIC_DOT)


def pairwise_cos_sim(a, b) -> torch.Tensor:
    """sentence_transformers.util.pairwise_cos_sim: the cosine of row i of `a` and row i of `b`, [B] (qst_pair_metric with
    its autograd; HIP tensors only). Each norm is clamped at 1e-8 as in F.cosine_similarity; 2.2.2 normalises the rows with
    eps 1e-12 first, which differs only for rows with a norm below 1e-8."""
    from . import st_losses
    return st_losses.pair_metric(a, b, st_losses.METRIC_COS_SIM)


def pairwise_angle_sim(x, y) -> torch.Tensor:
    """sentence_transformers.util.pairwise_angle_sim: the rows of x and y [B, D], D even, read as D / 2 complex numbers
    (real parts in the first half); the absolute sum of the real and imaginary parts of x / y, each quotient divided by
    |x| / |y| -- which is |x . [c - d, c + d]| / (|x| |y|) for y = [c, d]. Torch ops with torch's autograd on whatever
    device the inputs live; no epsilon, a zero row gives NaN as upstream. `losses.CoSENTLoss` recognises this function by
    identity and runs qst_cosent_loss in its place."""
    if x.dim() != 2 or x.shape != y.shape:
        raise ValueError(f"pairwise_angle_sim: two (B, D) tensors of one shape, {tuple(x.shape)} and {tuple(y.shape)} given")
    if x.shape[1] % 2:
        raise ValueError(f"pairwise_angle_sim splits each row into two halves: the width {x.shape[1]} is odd")
    a, b = torch.chunk(x, 2, dim=1)
    c, d = torch.chunk(y, 2, dim=1)
    z = torch.sum(c ** 2 + d ** 2, dim=1, keepdim=True)
    re = (a * c + b * d) / z
    im = (b * c - a * d) / z
    dz = torch.sum(a ** 2 + b ** 2, dim=1, keepdim=True) ** 0.5
    dw = torch.sum(c ** 2 + d ** 2, dim=1, keepdim=True) ** 0.5
    re = re / (dz / dw)
    im = im / (dz / dw)
    return torch.abs(torch.sum(torch.cat((re, im), dim=1), dim=1))


# marks this package's own score functions: evaluators route them (and callables that behave like them) to the fused
# score + top-k kernel instead of materialising the matrix
cos_sim._qst_mode = SCORE_COS
dot_score._qst_mode = SCORE_DOT
euclidean_score._qst_mode = SCORE_EUCLID


def topk_scores(queries: torch.Tensor, corpus: torch.Tensor, k: int, cosine=True, mode=None):
    """The k best corpus rows for every query row on the GPU (libqst qst_topk_scores: normalise / copy, split-bf16 x3
    matmul or Euclidean kernel, radix-select top-k): what InformationRetrievalEvaluator does per corpus chunk with its
    score function + torch.topk. mode: 'dot' | 'cos' | 'euclid' (`cosine` is the older boolean spelling).
    Returns (scores [nq, k] descending, indices int64 [nq, k]). No CPU fallback."""
    from . import _lib
    lib = _lib.load()
    if not (queries.is_cuda and corpus.is_cuda):
        raise _lib.QstError("topk_scores runs on the HIP device: pass CUDA tensors (there is no CPU fallback)")
    m = _mode(mode if mode is not None else cosine)
    q = _device_rows(queries)
    c = _device_rows(corpus, q.device)
    nq, dim = q.shape
    nc = c.shape[0]
    ws = torch.empty(lib.qst_topk_workspace_bytes(nq, nc, dim), dtype=torch.uint8, device=q.device)
    out_s = torch.empty(nq, k, dtype=torch.float32, device=q.device)
    out_i = torch.empty(nq, k, dtype=torch.int64, device=q.device)
    _lib.check(lib.qst_topk_scores(q.data_ptr(), c.data_ptr(), nq, nc, dim, k, m, out_s.data_ptr(),
                                   out_i.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()),
               "qst_topk_scores")
    return out_s, out_i


def topk_rows(scores: torch.Tensor, k: int, index_map: torch.Tensor = None):
    """k best entries per row of a score matrix (libqst qst_topk_rows); index_map translates columns to ids."""
    from . import _lib
    lib = _lib.load()
    if not scores.is_cuda:
        raise _lib.QstError("topk_rows runs on the HIP device: pass a CUDA tensor (there is no CPU fallback)")
    s = scores.to(torch.float32).contiguous()
    im = None if index_map is None else index_map.to(s.device, torch.int64).contiguous()
    n_rows, n = s.shape
    out_s = torch.empty(n_rows, k, dtype=torch.float32, device=s.device)
    out_i = torch.empty(n_rows, k, dtype=torch.int64, device=s.device)
    _lib.check(lib.qst_topk_rows(s.data_ptr(), n, _lib.ptr(im), n_rows, n, k, out_s.data_ptr(), out_i.data_ptr(),
                                 _lib.current_stream_ptr()), "qst_topk_rows")
    return out_s, out_i


# ------------------------------------------------------------------ re-ranking: ragged groups of one flat document array
RERANK_MAX = (1 << 31) - 1           # queries, and documents, of one qst_rerank_* call


def _on_host(x) -> bool:
    return not (isinstance(x, torch.Tensor) and x.is_cuda)


def _rerank_groups(what: str, offsets, num_pos, nd: int):
    """(offsets int64 [nq + 1], num_pos int32 [nq] or None, nq), not yet moved. Host lists, arrays and tensors are checked
    here, before anything touches the device -- ValueError names the first bad group; device tensors go through as they
    are (the kernel counts the groups it cannot use)."""
    from . import _lib
    if _on_host(offsets):
        o = np.asarray(offsets.numpy() if isinstance(offsets, torch.Tensor) else offsets)
        if o.ndim != 1 or len(o) < 2 or not np.issubdtype(o.dtype, np.integer):
            raise ValueError(f"{what}: offsets must be nq + 1 integers, nq >= 1 (got {o.dtype} of shape {o.shape})")
        o = o.astype(np.int64)
        if o[0] != 0:
            raise ValueError(f"{what}: group 0 starts at offsets[0] = {o[0]}, not 0")
        down = np.flatnonzero(np.diff(o) < 0)
        if len(down):
            g = int(down[0])
            raise ValueError(f"{what}: group {g}: offsets descend, {o[g]} -> {o[g + 1]}")
        if o[-1] != nd:
            raise ValueError(f"{what}: group {len(o) - 2} ends at offsets[nq] = {o[-1]}, but there are {nd} documents")
        sizes = np.diff(o)
        offsets = torch.from_numpy(o)
    else:
        sizes = None
    nq = int(offsets.numel()) - 1
    if num_pos is not None:
        if _on_host(num_pos):
            p = np.asarray(num_pos.numpy() if isinstance(num_pos, torch.Tensor) else num_pos)
            if p.ndim != 1 or len(p) != nq or not np.issubdtype(p.dtype, np.integer):
                raise ValueError(f"{what}: num_pos must be {nq} integers, one per group (got {p.dtype} of shape {p.shape})")
            p = p.astype(np.int64)
            bad = np.flatnonzero(p < 1) if sizes is None else np.flatnonzero((p < 1) | (p >= sizes))
            if len(bad):
                g = int(bad[0])
                size = "" if sizes is None else f" of {sizes[g]} documents"
                raise ValueError(f"{what}: group {g}: {p[g]} positives{size}; a group needs 1 <= num_pos < its size")
            num_pos = torch.from_numpy(p.astype(np.int32))
        elif num_pos.numel() != nq:
            raise ValueError(f"{what}: {num_pos.numel()} entries of num_pos for {nq} groups")
    if nq < 1 or nd < 2:
        raise ValueError(f"{what}: {nq} groups over {nd} documents; at least one group and two documents are needed")
    if nq > RERANK_MAX or nd > RERANK_MAX:
        raise _lib.QstError(f"{what}: {nq} groups over {nd} documents; the kernel takes up to {RERANK_MAX} (2^31 - 1) of each")
    return offsets, num_pos, nq


def rerank_scores(queries: torch.Tensor, docs: torch.Tensor, offsets, mode="cos") -> torch.Tensor:
    """The score of every candidate document against the query of its group (libqst qst_rerank_scores): queries [nq, D],
    docs [nd, D] HIP tensors, query g owning docs[offsets[g] : offsets[g + 1]]; mode 'cos' | 'dot' | 'euclid'. Returns fp32
    [nd] on the device. offsets: nq + 1 ascending integers from 0 to nd -- a host list or array is checked first, a device
    tensor is passed through. Current stream, nothing copied to the host, no CPU fallback."""
    from . import _lib
    queries, docs = torch.as_tensor(queries), torch.as_tensor(docs)
    if queries.dim() != 2 or docs.dim() != 2 or queries.shape[1] != docs.shape[1] or queries.shape[1] < 1:
        raise ValueError(f"rerank_scores: queries {tuple(queries.shape)} and docs {tuple(docs.shape)} must be [nq, D] and [nd, D]")
    nd, dim = docs.shape
    off, _, nq = _rerank_groups("rerank_scores", offsets, None, nd)
    if queries.shape[0] != nq:
        raise ValueError(f"rerank_scores: {queries.shape[0]} queries but offsets describe {nq} groups")
    if not (queries.is_cuda and docs.is_cuda):
        raise _lib.QstError("rerank_scores runs on the HIP device: pass CUDA tensors (there is no CPU fallback)")
    lib = _lib.load()
    q = queries.to(torch.float32).contiguous()
    d = docs.to(q.device, torch.float32).contiguous()
    off = off.to(q.device, torch.int64).contiguous()
    with torch.cuda.device(q.device):
        out = torch.empty(nd, dtype=torch.float32, device=q.device)
        _lib.check(lib.qst_rerank_scores(q.data_ptr(), d.data_ptr(), off.data_ptr(), nq, nd, dim, _mode(mode), out.data_ptr(),
                                         _lib.current_stream_ptr()), "qst_rerank_scores")
    return out


def rerank_metrics(scores: torch.Tensor, offsets, num_pos, k: int = 10):
    """Reciprocal rank within k, average precision and NDCG within k of every group, and their means (libqst
    qst_rerank_metrics; include/qst.h states the counts and the tie rule: among equal scores the earlier document ranks
    first). scores fp32 [nd] on the HIP device, the larger the better; the first num_pos[g] documents of group g are its
    positives. Returns (per_query float64 [nq, 3] = {rr, ap, ndcg}, out float64 [5] = {mean rr, mean ap, mean ndcg,
    non-finite scores, invalid groups}), both on the device. Host offsets / num_pos are checked first (ValueError names the
    first bad group); device tensors are passed through and out[4] counts the groups the kernel could not use. Current
    stream, nothing copied to the host."""
    from . import _lib
    scores = torch.as_tensor(scores)
    if scores.dim() != 1 or int(k) < 1:
        raise ValueError(f"rerank_metrics: scores {tuple(scores.shape)} must be [nd] and k = {k} at least 1")
    nd = scores.numel()
    off, pos, nq = _rerank_groups("rerank_metrics", offsets, num_pos, nd)
    if not scores.is_cuda:
        raise _lib.QstError("rerank_metrics runs on the HIP device: pass a CUDA tensor (there is no CPU fallback)")
    lib = _lib.load()
    s = scores.to(torch.float32).contiguous()
    off = off.to(s.device, torch.int64).contiguous()
    pos = pos.to(s.device, torch.int32).contiguous()
    with torch.cuda.device(s.device):
        per_query = torch.empty(nq, 3, dtype=torch.float64, device=s.device)
        out = torch.empty(5, dtype=torch.float64, device=s.device)
        nbytes = int(lib.qst_rerank_workspace_bytes(nq, nd))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=s.device)
        _lib.check(lib.qst_rerank_metrics(s.data_ptr(), off.data_ptr(), pos.data_ptr(), nq, nd, min(int(k), RERANK_MAX),
                                          per_query.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes,
                                          _lib.current_stream_ptr()), "qst_rerank_metrics")
    return per_query, out


# corpus rows per chunk of the streaming top-k where the caller does not say: the score block is
# [min(nq, 2048), chunk] fp32, 128 MB at most here. The result does not depend on it; of 16,384 / 65,536 / 262,144 it
# was the fastest at 2048 x 262,144 x 384 for k = 10 and k = 100 (profiles/topk_stream_bench.json).
STREAM_CHUNK = 16384
TOPK_MAX = 1024


def _new_state(nq: int, k: int, device):
    return (torch.full((nq, k), float("-inf"), dtype=torch.float32, device=device),
            torch.full((nq, k), -1, dtype=torch.int64, device=device))


def _check_state(state, nq: int, k: int, device):
    s, i = state
    if not (torch.is_tensor(s) and torch.is_tensor(i) and s.dtype == torch.float32 and i.dtype == torch.int64
            and tuple(s.shape) == (nq, k) and tuple(i.shape) == (nq, k) and s.device == device and i.device == device
            and s.is_contiguous() and i.is_contiguous()):
        raise ValueError(f"state must be the (scores f32, indices int64) pair of shape {(nq, k)} an earlier call returned")
    return s, i


def topk_merge_rows(scores: torch.Tensor, k: int, col_base: int = 0, row_base: int = 0, exclude_self: bool = False,
                    max_score: float = float("inf"), state=None):
    """Merge one chunk of a score matrix into a running top-k (libqst qst_topk_merge_rows): column j of `scores` is
    global id col_base + j, row r is query row_base + r. Returns (scores [rows, k], indices int64 [rows, k]) sorted by
    (score descending, id ascending), padded with -inf / -1; pass the pair back as `state` with the next chunk (it is
    updated in place)."""
    from . import _lib
    lib = _lib.load()
    if not scores.is_cuda:
        raise _lib.QstError("topk_merge_rows runs on the HIP device: pass a CUDA tensor (there is no CPU fallback)")
    s = scores.to(torch.float32).contiguous()
    rows, n = s.shape
    rs, ri = _new_state(rows, k, s.device) if state is None else _check_state(state, rows, k, s.device)
    with torch.cuda.device(s.device):
        _lib.check(lib.qst_topk_merge_rows(s.data_ptr(), n, rows, n, int(col_base), int(row_base), int(bool(exclude_self)),
                                           float(max_score), k, rs.data_ptr(), ri.data_ptr(), _lib.current_stream_ptr()),
                   "qst_topk_merge_rows")
    return rs, ri


def topk_stream(queries, corpus, k: int, mode="cos", chunk: int = STREAM_CHUNK, exclude_self: bool = False,
                max_score: float = float("inf"), state=None, query_base: int = 0, corpus_base: int = 0):
    """The k best corpus rows for every query row at any corpus size (libqst qst_topk_stream): the corpus goes through
    in chunks of `chunk` rows -- prepare, score, merge into a running top-k -- so the workspace is bounded by the chunk
    and the result, ties included, is the same for every chunk size. mode: 'dot' | 'cos' | 'euclid'. Query row r has
    global id query_base + r, corpus row c has corpus_base + c; exclude_self drops the corpus row whose id is the
    query's own, max_score those scoring above it. Returns (scores [nq, k] descending, indices int64 [nq, k]), padded
    with -inf / -1 where fewer than k rows qualify. Passing the pair back as `state`, with the next piece of the corpus
    and its corpus_base, continues the search (the pair is updated in place). No CPU fallback."""
    from . import _lib
    lib = _lib.load()
    m = _mode(mode)
    q = _device_rows(queries)
    c = _device_rows(corpus, q.device)
    if c.device != q.device:
        c = c.to(q.device)
    if q.shape[1] != c.shape[1]:
        raise ValueError(f"embedding sizes differ: {tuple(q.shape)} vs {tuple(c.shape)}")
    nq, dim = q.shape
    nc = c.shape[0]
    chunk = max(1, min(int(chunk), nc))
    rs, ri = _new_state(nq, k, q.device) if state is None else _check_state(state, nq, k, q.device)
    with torch.cuda.device(q.device):
        ws = torch.empty(lib.qst_topk_stream_workspace_bytes(nq, chunk, dim), dtype=torch.uint8, device=q.device)
        _lib.check(lib.qst_topk_stream(q.data_ptr(), c.data_ptr(), nq, nc, dim, k, m, chunk, int(query_base),
                                       int(corpus_base), int(bool(exclude_self)), float(max_score), rs.data_ptr(),
                                       ri.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()),
                   "qst_topk_stream")
    return rs, ri


def hamming_topk(queries, corpus, k: int, chunk: int = None, exclude_self: bool = False, state=None, query_base: int = 0,
                 corpus_base: int = 0):
    """topk_stream on packed sign bits ('binary' int8 or 'ubinary' uint8 codes of quantization.quantize_embeddings): the
    score is -(Hamming distance). libqst qst_topk_hamming_stream; see quantization.hamming_topk."""
    from . import quantization
    return quantization.hamming_topk(queries, corpus, k, chunk=chunk, exclude_self=exclude_self, state=state,
                                     query_base=query_base, corpus_base=corpus_base)


def int8_topk(queries, corpus, k: int, chunk: int = None, exclude_self: bool = False, state=None, query_base: int = 0,
              corpus_base: int = 0):
    """topk_stream on int8 codes: the score is the exact integer dot product. libqst qst_topk_int8_stream; see
    quantization.int8_topk."""
    from . import quantization
    return quantization.int8_topk(queries, corpus, k, chunk=chunk, exclude_self=exclude_self, state=state,
                                  query_base=query_base, corpus_base=corpus_base)


def _as_rows(x):
    """A tensor, a numpy array, a list of tensors or a single 1-D embedding -> a 2-D tensor (ST's accepted inputs)."""
    if isinstance(x, (list, tuple)):
        x = torch.stack([torch.as_tensor(t) for t in x])
    return _as_2d(x)


def _search(queries, corpus, top_k: int, score_function, query_chunk_size: int, corpus_chunk_size: int,
            exclude_self: bool):
    """(scores [nq, k], corpus rows int64 [nq, k]) on the device, k = min(top_k, TOPK_MAX checked), over the WHOLE
    corpus. The package's own score functions run qst_topk_stream; any other callable is applied per
    (query chunk, corpus chunk) and its matrix goes through qst_topk_merge_rows."""
    if not 1 <= int(top_k) <= TOPK_MAX:
        raise ValueError(f"top_k must be between 1 and {TOPK_MAX} (got {top_k})")
    if query_chunk_size < 1 or corpus_chunk_size < 1:
        raise ValueError("query_chunk_size and corpus_chunk_size must be positive")
    if not callable(score_function):
        raise ValueError(f"score_function must be callable (got {type(score_function).__name__})")
    top_k = int(top_k)
    mode = getattr(score_function, "_qst_mode", None)
    if mode is not None:
        # the library blocks the queries itself; the chunk sizes only bound memory and do not change the result
        return topk_stream(queries, corpus, top_k, mode=int(mode), chunk=min(int(corpus_chunk_size), STREAM_CHUNK),
                           exclude_self=exclude_self)
    from . import _lib
    q = _as_2d(queries)
    if not q.is_cuda:
        if not torch.cuda.is_available():
            raise _lib.QstError("the search runs on the HIP device and none is visible (there is no CPU path)")
        q = q.to(torch.device("cuda", torch.cuda.current_device()))
    c = _as_2d(corpus).to(q.device)
    rs, ri = _new_state(q.shape[0], top_k, q.device)
    for q0 in range(0, q.shape[0], query_chunk_size):
        q1 = min(q0 + query_chunk_size, q.shape[0])
        state = (rs[q0:q1], ri[q0:q1])                       # row slices of contiguous tensors: contiguous views
        for c0 in range(0, c.shape[0], corpus_chunk_size):
            c1 = min(c0 + corpus_chunk_size, c.shape[0])
            full = torch.as_tensor(score_function(q[q0:q1], c[c0:c1])).to(q.device, torch.float32)
            if tuple(full.shape) != (q1 - q0, c1 - c0):
                raise ValueError(f"score_function returned shape {tuple(full.shape)}, expected {(q1 - q0, c1 - c0)}")
            topk_merge_rows(full, top_k, col_base=c0, row_base=q0, exclude_self=exclude_self, state=state)
    return rs, ri


def semantic_search(query_embeddings, corpus_embeddings, query_chunk_size: int = 100, corpus_chunk_size: int = 500000,
                    top_k: int = 10, score_function=cos_sim):
    """sentence_transformers.util.semantic_search (2.2.2): for every query the top_k corpus entries, one list per query
    of {'corpus_id': int, 'score': float} in descending order (ties: ascending corpus_id); shorter than top_k where the
    corpus is. Inputs: a tensor, a numpy array, a list of tensors, or 1-D for a single one; they are moved to the HIP
    device (there is no CPU path). cos_sim, dot_score and euclidean_score of this package run the streaming top-k
    (qst_topk_stream: scoring and selection in one call, no [nq, nc] matrix); any other callable is applied per
    (query chunk, corpus chunk) and selected by qst_topk_merge_rows. The chunk sizes bound memory only."""
    rs, ri = _search(_as_rows(query_embeddings), _as_rows(corpus_embeddings), top_k, score_function, query_chunk_size,
                     corpus_chunk_size, exclude_self=False)
    sc, idx = rs.cpu().numpy(), ri.cpu().numpy()
    return [[{"corpus_id": int(c), "score": float(s)} for s, c in zip(sc[r], idx[r]) if c >= 0] for r in range(len(sc))]


def merge_mined_pairs(scores, rows, cols, max_pairs: int):
    """The host half of paraphrase mining, pure numpy: candidates (score, i, j) -- row i found row j -- become the
    list of unordered pairs [score, min(i, j), max(i, j)]. The max_pairs best candidates by (score descending, min
    ascending, max ascending) are kept FIRST; then the two directions of a pair merge into one entry with the larger
    score; the list comes back in the same order. Entries with j < 0 (empty top-k slots) or i == j are dropped."""
    s = np.asarray(scores, dtype=np.float64).ravel()
    i = np.asarray(rows, dtype=np.int64).ravel()
    j = np.asarray(cols, dtype=np.int64).ravel()
    if not (len(s) == len(i) == len(j)):
        raise ValueError("scores, rows and cols must have the same length")
    if max_pairs < 1:
        raise ValueError(f"max_pairs must be positive (got {max_pairs})")
    keep = (j >= 0) & (i >= 0) & (i != j)
    s, lo, hi = s[keep], np.minimum(i, j)[keep], np.maximum(i, j)[keep]
    order = np.lexsort((hi, lo, -s))[:max_pairs]
    s, lo, hi = s[order], lo[order], hi[order]
    # the first occurrence of a pair in this order carries its larger score
    _, first = np.unique(np.stack([lo, hi], axis=1), axis=0, return_index=True) if len(s) else (None, np.zeros(0, np.int64))
    first = np.sort(first)
    return [[float(s[t]), int(lo[t]), int(hi[t])] for t in first]


def paraphrase_mining_embeddings(embeddings, query_chunk_size: int = 5000, corpus_chunk_size: int = 100000,
                                 max_pairs: int = 500000, top_k: int = 100, score_function=cos_sim):
    """sentence_transformers.util.paraphrase_mining_embeddings (2.2.2): the most similar pairs among the rows of
    `embeddings`, as a list of [score, i, j] with i < j, each pair once, sorted by (score descending, i, j).

    Device: for every row its top_k best OTHER rows (the streaming top-k with exclude_self; score_function as in
    semantic_search). Host: merge_mined_pairs keeps the max_pairs best candidates and merges the two directions.

    One deliberate difference from ST 2.2.2: ST takes top_k (+1 for the row itself) per corpus chunk, so its candidate
    set, and with it the answer, depends on corpus_chunk_size. Here the top_k are selected over the whole corpus and
    the chunk sizes bound memory only. The two agree whenever the corpus fits one chunk and the scores have no ties."""
    e = _as_rows(embeddings)
    rs, ri = _search(e, e, top_k, score_function, query_chunk_size, corpus_chunk_size, exclude_self=True)
    sc, idx = rs.cpu().numpy(), ri.cpu().numpy()
    rows = np.broadcast_to(np.arange(sc.shape[0], dtype=np.int64)[:, None], sc.shape)
    return merge_mined_pairs(sc, rows, idx, max_pairs)


def paraphrase_mining(model, sentences, show_progress_bar: bool = False, batch_size: int = 32,
                      query_chunk_size: int = 5000, corpus_chunk_size: int = 100000, max_pairs: int = 500000,
                      top_k: int = 100, score_function=cos_sim):
    """sentence_transformers.util.paraphrase_mining (2.2.2): encode the sentences with `model`, then
    paraphrase_mining_embeddings. Returns [score, i, j] with i < j indexing `sentences`."""
    emb = model.encode(list(sentences), show_progress_bar=show_progress_bar, batch_size=batch_size, convert_to_tensor=True)
    return paraphrase_mining_embeddings(emb, query_chunk_size, corpus_chunk_size, max_pairs, top_k, score_function)


# Members (row number + score, 8 bytes each) that one round of community_detection extracts at most, beyond its first
# candidate: 2^26 members = 512 MB. A bound on memory in round numbers, not a tuned value; the result does not depend on it.
COMMUNITY_ROUND_MEMBERS = 1 << 26
_ROW_BLOCK = 2048                    # rows per score panel (csrc/retrieval.hip: kQueryBlock)


def community_order(counts, min_community_size: int):
    """The candidate rows (counts >= min_community_size) in greedy order: larger community first, lower row first among
    equal sizes. Pure numpy."""
    counts = np.asarray(counts, dtype=np.int64)
    idx = np.flatnonzero(counts >= min_community_size)
    return idx[np.lexsort((idx, -counts[idx]))]


def plan_community_round(order, counts, self_member, taken, start: int, budget: int):
    """The next round of community_detection, pure numpy: walking order[start:], the candidates whose members are to be
    extracted, until their counts sum past `budget` (the first one is always taken, so a round makes progress). A
    candidate whose own row is taken is dropped here -- it could only be rejected -- but only where the row is a member of
    its own community (self_member): a zero or NaN row is not, and its community is still to be looked at.
    Returns (rows of the round in greedy order, the position in `order` where the next round starts)."""
    order = np.asarray(order, dtype=np.int64)
    cand = order[start:]
    if len(cand) == 0:
        return cand, len(order)
    live = ~(np.asarray(taken, dtype=bool)[cand] & np.asarray(self_member, dtype=bool)[cand])
    if not live.any():
        return cand[:0], len(order)
    cost = np.cumsum(np.where(live, np.asarray(counts, dtype=np.int64)[cand], 0))
    stop = int(np.searchsorted(cost, budget, side="right"))          # leading candidates whose running sum fits
    stop = max(stop, int(np.argmax(live)) + 1)
    return cand[:stop][live[:stop]], start + stop


def order_community(centre: int, members, scores):
    """One community in the order of ST's "the first element is the central point": the candidate row first when it is a
    member, the rest by (score descending, row ascending). Pure numpy; returns a list of int."""
    members = np.asarray(members, dtype=np.int64)
    order = np.lexsort((members, -np.asarray(scores, dtype=np.float64)))
    out = [int(m) for m in members[order]]
    if centre in out:
        out.remove(centre)
        out.insert(0, int(centre))
    return out


def _community_detection(e: torch.Tensor, threshold: float, min_community_size: int, chunk: int, stats=None):
    """community_detection on prepared device rows e [n, dim % 32 == 0]. stats (a dict, for tools/community_bench.py):
    filled with the seconds of the count pass and, per round, candidates / members / row blocks / seconds."""
    import time
    from . import _lib
    lib = _lib.load()
    n, dim = e.shape
    dev = e.device
    sp = _lib.current_stream_ptr

    def clock():
        if stats is not None:
            torch.cuda.synchronize(dev)
        return time.perf_counter()

    with torch.cuda.device(dev):
        ws = torch.empty(lib.qst_community_workspace_bytes(n, chunk, dim), dtype=torch.uint8, device=dev)
        counts_d = torch.empty(n, dtype=torch.int32, device=dev)
        self_d = torch.empty(n, dtype=torch.uint8, device=dev)
        t0 = clock()
        _lib.check(lib.qst_community_count(e.data_ptr(), n, dim, threshold, chunk, counts_d.data_ptr(), self_d.data_ptr(),
                                           ws.data_ptr(), ws.numel(), sp()), "qst_community_count")
        counts = counts_d.cpu().numpy()
        self_member = self_d.cpu().numpy().astype(bool)
        if stats is not None:
            stats.update(count_s=clock() - t0, rounds=[])
        order = community_order(counts, min_community_size)
        taken = np.zeros(n, dtype=bool)
        taken_d = torch.zeros(n, dtype=torch.uint8, device=dev)
        written_d = torch.empty(n, dtype=torch.int32, device=dev)
        communities, start = [], 0
        while start < len(order):
            picked, start = plan_community_round(order, counts, self_member, taken, start, COMMUNITY_ROUND_MEMBERS)
            if len(picked) == 0:
                break
            t0 = clock()
            lens = counts[picked].astype(np.int64)
            begins = np.cumsum(lens) - lens
            total = int(lens.sum())
            row_begin = np.full(n, -1, dtype=np.int64)
            row_begin[picked] = begins
            begin_d = torch.from_numpy(row_begin).to(dev)
            index_d = torch.empty(total, dtype=torch.int32, device=dev)
            score_d = torch.empty(total, dtype=torch.float32, device=dev)
            blocks = np.unique(picked // _ROW_BLOCK)
            for blk in blocks:
                r0 = int(blk) * _ROW_BLOCK
                _lib.check(lib.qst_community_members(e.data_ptr(), n, dim, threshold, chunk, r0, begin_d.data_ptr() + 8 * r0,
                                                     counts_d.data_ptr() + 4 * r0, index_d.data_ptr(), score_d.data_ptr(),
                                                     written_d.data_ptr() + 4 * r0, ws.data_ptr(), ws.numel(), sp()),
                           "qst_community_members")
            picked_d = torch.from_numpy(picked).to(dev)
            if not torch.equal(written_d[picked_d], counts_d[picked_d]):
                raise _lib.QstError("community_detection: the member pass and the count pass disagree")
            t1 = clock()
            cand_begin = torch.from_numpy(begins).to(dev)
            cand_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
            accepted_d = torch.empty(len(picked), dtype=torch.uint8, device=dev)
            _lib.check(lib.qst_community_claim(cand_begin.data_ptr(), cand_len.data_ptr(), len(picked), index_d.data_ptr(), n,
                                               taken_d.data_ptr(), accepted_d.data_ptr(), sp()), "qst_community_claim")
            won = np.flatnonzero(accepted_d.cpu().numpy())
            if len(won):
                # only the accepted communities come back, with fp64 cosines for the order inside them: equally similar
                # rows must tie exactly, which the x3 scores do not promise in their last bits
                members_d = torch.cat([index_d[int(begins[c]):int(begins[c] + lens[c])] for c in won])
                centres_d = torch.from_numpy(np.repeat(picked[won], lens[won]).astype(np.int32)).to(dev)
                exact_d = torch.empty(members_d.numel(), dtype=torch.float64, device=dev)
                _lib.check(lib.qst_community_rescore(e.data_ptr(), n, dim, centres_d.data_ptr(), members_d.data_ptr(),
                                                     members_d.numel(), exact_d.data_ptr(), sp()), "qst_community_rescore")
                members, exact = members_d.cpu().numpy(), exact_d.cpu().numpy()
                ends = np.cumsum(lens[won])
                for c, b, t in zip(won, ends - lens[won], ends):
                    communities.append(order_community(int(picked[c]), members[b:t], exact[b:t]))
            taken = taken_d.cpu().numpy().astype(bool)
            if stats is not None:
                t2 = clock()
                stats["rounds"].append(dict(candidates=int(len(picked)), members=total, row_blocks=int(len(blocks)),
                                            accepted=int(len(won)), members_s=t1 - t0, claim_s=t2 - t1))
    return communities


def community_detection(embeddings, threshold: float = 0.75, min_community_size: int = 10, init_max_size: int = 1000, *,
                        corpus_chunk_size: int = STREAM_CHUNK):
    """sentence_transformers.util.community_detection (2.2.2), "fast clustering": the communities of rows whose cosine
    similarity to a central row is at least `threshold`, as a list of lists of int, largest first, no row in two of them.

    With S the cosine scores (rows normalised with eps 1e-12, as cos_sim) and N(i) = {j : S[i, j] >= threshold} -- the row
    itself when its own score passes, a NaN score passes nothing -- row i is a candidate when |N(i)| >= min_community_size.
    Candidates are taken by (|N(i)| descending, i ascending); one is accepted when none of its members belongs to a
    community accepted before it, and is then returned whole (a rejected one is dropped whole, not trimmed). Inside a
    community the candidate row comes first, the rest by (score descending, row ascending).

    Device: no [n, n] matrix and no top-k. One pass over the [2048, chunk] score panels counts |N(i)|
    (qst_community_count); then, in rounds that bound memory (COMMUNITY_ROUND_MEMBERS), the members of the next
    candidates in greedy order are compacted out of the same panels (qst_community_members), claimed on the device
    (qst_community_claim) and only the accepted communities are copied back, ordered by fp64 cosines
    (qst_community_rescore). Inputs: a tensor, a numpy array or a list of tensors; they are moved to the HIP device
    (there is no CPU path).

    Deliberate differences from ST 2.2.2: init_max_size is checked (a positive int) but changes nothing -- ST uses it only
    as the width of its top-k shortcut and, in a community larger than it, falls back to index order; here the order is
    always the one above. min_community_size > n returns [] where ST's topk raises. min_community_size < 1 or a NaN
    threshold raises ValueError. corpus_chunk_size (keyword-only) bounds memory only."""
    if isinstance(min_community_size, bool) or int(min_community_size) != min_community_size or min_community_size < 1:
        raise ValueError(f"min_community_size must be a positive int (got {min_community_size!r})")
    if isinstance(init_max_size, bool) or not isinstance(init_max_size, (int, np.integer)) or init_max_size < 1:
        raise ValueError(f"init_max_size must be a positive int (got {init_max_size!r})")
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold must not be NaN")
    if isinstance(corpus_chunk_size, bool) or int(corpus_chunk_size) != corpus_chunk_size or corpus_chunk_size < 1:
        raise ValueError(f"corpus_chunk_size must be a positive int (got {corpus_chunk_size!r})")
    rows = _as_rows(embeddings)
    n = rows.shape[0]
    if rows.dim() != 2:
        raise ValueError(f"embeddings must be rows of one width (got shape {tuple(rows.shape)})")
    if n == 0 or int(min_community_size) > n:
        return []
    e = _device_rows(rows)
    return _community_detection(e, threshold, int(min_community_size), min(int(corpus_chunk_size), n))


def mine_hard_negatives(references, candidates, k: int, threshold: float = 0.2, embedder=None, batch_size: int = 64):
    """Negative selection of the reference's dataset (dataset/quadruplet_dataset.py:185-270) for MANY reference
    captions in one GPU pass: among `candidates`, those whose cosine similarity to a reference is <= threshold
    (NEG_EXAMPLE_SIM_TRESHOLD = 0.2, the "not a paraphrase" filter), and of those the k most similar
    (hard_contrastive_sampling(max_mode=True), :31-47). The reference does this per item with two encode() calls on
    the training thread; here both sides are encoded in batches and scored by libqst (qst_topk_scores_capped).

    references / candidates: lists of str (then `embedder` -- a SentenceTransformer -- encodes them) or CUDA tensors of
    embeddings [R, D] / [C, D]. Returns (index int64 [R, k] into candidates, -1 where fewer than k qualify;
    score f32 [R, k], -inf there)."""
    from . import _lib
    lib = _lib.load()

    def emb(x):
        if torch.is_tensor(x):
            return x
        if embedder is None:
            raise ValueError("pass embeddings, or sentences together with an embedder")
        return embedder.encode(list(x), batch_size=batch_size, convert_to_tensor=True)
    q, c = emb(references), emb(candidates)
    if not (q.is_cuda and c.is_cuda):
        raise _lib.QstError("mine_hard_negatives runs on the HIP device: embeddings must be CUDA tensors")
    q = _device_rows(q)
    c = _device_rows(c, q.device)
    nq, dim = q.shape
    nc = c.shape[0]
    kk = min(k, nc)
    ws = torch.empty(lib.qst_topk_workspace_bytes(nq, nc, dim), dtype=torch.uint8, device=q.device)
    out_s = torch.full((nq, k), float("-inf"), dtype=torch.float32, device=q.device)
    out_i = torch.full((nq, k), -1, dtype=torch.int64, device=q.device)
    ts = torch.empty(nq, kk, dtype=torch.float32, device=q.device)
    ti = torch.empty(nq, kk, dtype=torch.int64, device=q.device)
    _lib.check(lib.qst_topk_scores_capped(q.data_ptr(), c.data_ptr(), nq, nc, dim, kk, 1, float(threshold), ts.data_ptr(),
                                          ti.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()),
               "qst_topk_scores_capped")
    out_s[:, :kk], out_i[:, :kk] = ts, ti
    return out_i, out_s
