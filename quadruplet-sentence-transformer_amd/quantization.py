"""sentence_transformers.quantization (2.6+): quantize_embeddings and a search that retrieves on the small codes and
rescores the shortlist with the float query. Ranges, packing, both first stages and the rescoring run in libqst
(csrc/quantize.hip); sorting a row's candidate ids and gathering the winners' ids is torch indexing on the device. There is
no CPU path."""
from __future__ import annotations

import logging

import numpy as np
import torch

from . import util

logger = logging.getLogger(__name__)

QUANT_INT8, QUANT_UINT8, QUANT_BINARY, QUANT_UBINARY = 0, 1, 2, 3
_KINDS = {"int8": QUANT_INT8, "uint8": QUANT_UINT8, "binary": QUANT_BINARY, "ubinary": QUANT_UBINARY}
PRECISIONS = ("float32", "int8", "uint8", "binary", "ubinary")
# corpus rows per chunk of the two quantized streams where the caller does not say (the result does not depend on it): of
# 16,384 / 65,536 / 262,144 it was the fastest for both at 2048 x 262,144, dim 384 and 1,024, k = 10 and k = 100
# (profiles/quantize_bench.json) -- the float search's value.
STREAM_CHUNK = util.STREAM_CHUNK
INT8_MAX_DIM = 1024
RESCORE_MAX = util.TOPK_MAX
_OUT_DTYPE = {QUANT_INT8: torch.int8, QUANT_UINT8: torch.uint8, QUANT_BINARY: torch.int8, QUANT_UBINARY: torch.uint8}


def _check_precision(precision) -> str:
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {', '.join(PRECISIONS)} (got {precision!r})")
    return precision


def _float_rows(x, what: str = "embeddings") -> torch.Tensor:
    """fp32 contiguous rows on the HIP device from any of ST's accepted inputs; the width is kept as it is."""
    from . import _lib
    x = util._as_rows(x)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{what} must be a non-empty [n, dim] array (got shape {tuple(x.shape)})")
    if not x.is_cuda:
        if not torch.cuda.is_available():
            raise _lib.QstError("quantization runs on the HIP device and none is visible (there is no CPU path)")
        x = x.to(torch.device("cuda", torch.cuda.current_device()))
    return x.to(torch.float32).contiguous()


def column_ranges(embeddings) -> torch.Tensor:
    """f32 [2, dim] on the device: the minimum and the maximum of every column (libqst qst_column_ranges); a NaN in a
    column makes both of its entries NaN, as numpy's min / max do."""
    from . import _lib
    lib = _lib.load()
    x = _float_rows(embeddings)
    n, dim = x.shape
    with torch.cuda.device(x.device):
        out = torch.empty(2, dim, dtype=torch.float32, device=x.device)
        ws = torch.empty(lib.qst_column_ranges_workspace_bytes(n, dim), dtype=torch.uint8, device=x.device)
        _lib.check(lib.qst_column_ranges(x.data_ptr(), n, dim, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _lib.current_stream_ptr()), "qst_column_ranges")
    return out


def _device_ranges(ranges, dim: int, device) -> torch.Tensor:
    r = ranges if torch.is_tensor(ranges) else torch.as_tensor(np.asarray(ranges))
    if tuple(r.shape) != (2, dim):
        raise ValueError(f"ranges must have shape (2, {dim}): the minimum and the maximum of every column (got {tuple(r.shape)})")
    return r.to(device, torch.float32).contiguous()


def _quantize_device(x: torch.Tensor, kind: int, ranges=None) -> torch.Tensor:
    from . import _lib
    lib = _lib.load()
    n, dim = x.shape
    width = (dim + 7) // 8 if kind in (QUANT_BINARY, QUANT_UBINARY) else dim
    with torch.cuda.device(x.device):
        out = torch.empty(n, width, dtype=_OUT_DTYPE[kind], device=x.device)
        _lib.check(lib.qst_quantize_rows(x.data_ptr(), n, dim, kind, _lib.ptr(ranges), out.data_ptr(),
                                         _lib.current_stream_ptr()), "qst_quantize_rows")
    return out


def _resolve_ranges(x: torch.Tensor, ranges, calibration_embeddings, warn: bool) -> torch.Tensor:
    dim = x.shape[1]
    if ranges is not None:
        return _device_ranges(ranges, dim, x.device)
    if calibration_embeddings is not None:
        cal = _float_rows(calibration_embeddings, "calibration_embeddings").to(x.device)
        if cal.shape[1] != dim:
            raise ValueError(f"calibration_embeddings have width {cal.shape[1]}, the embeddings {dim}")
        return column_ranges(cal)
    if warn and x.shape[0] < 100:
        logger.warning(f"Computing int8 quantization buckets based on {x.shape[0]} embedding{'s' if x.shape[0] != 1 else ''}. "
                       "int8 quantization is more stable with `ranges` calculated from more `calibration_embeddings` or a "
                       "`calibration_embeddings` that can be used to calculate the buckets.")
    return column_ranges(x)


def quantize_embeddings(embeddings, precision, ranges=None, calibration_embeddings=None):
    """sentence_transformers.quantization.quantize_embeddings: `precision` is 'float32', 'int8', 'uint8', 'binary' or
    'ubinary'. binary / ubinary are np.packbits(x > 0) as int8 (byte - 128) / uint8, [n, ceil(dim / 8)]; int8 / uint8 are
    ((x - lo) / ((hi - lo) / 255) [- 128]) truncated, with (lo, hi) from `ranges` ([2, dim]), else from the column minimum /
    maximum of `calibration_embeddings`, else of the embeddings themselves (with upstream's warning below 100 rows). Where
    upstream's cast is undefined the code saturates; a NaN or a constant column gives the lowest code. A tensor comes back
    as a device tensor, anything else (numpy, lists) as numpy. The arithmetic is libqst's (qst_quantize_rows)."""
    precision = _check_precision(precision)
    as_tensor = torch.is_tensor(embeddings)
    x = _float_rows(embeddings)
    if precision == "float32":
        out = x
    else:
        kind = _KINDS[precision]
        r = None
        if kind in (QUANT_INT8, QUANT_UINT8):
            r = _resolve_ranges(x, ranges, calibration_embeddings, warn=True)
        out = _quantize_device(x, kind, r)
    return out if as_tensor else out.cpu().numpy()


def _code_rows(x, dtype, what: str) -> torch.Tensor:
    from . import _lib
    x = util._as_rows(x)
    if x.dtype != dtype:
        raise ValueError(f"{what} must be {dtype} codes (got {x.dtype})")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{what} must be a non-empty [n, width] array (got shape {tuple(x.shape)})")
    if not x.is_cuda:
        if not torch.cuda.is_available():
            raise _lib.QstError("the quantized search runs on the HIP device and none is visible (there is no CPU path)")
        x = x.to(torch.device("cuda", torch.cuda.current_device()))
    return x.contiguous()


def _padded(x: torch.Tensor, multiple: int) -> torch.Tensor:
    """Zero columns up to a multiple: a zero byte on both sides adds no differing bit and nothing to a dot product."""
    pad = (-x.shape[1]) % multiple
    return torch.nn.functional.pad(x, (0, pad)).contiguous() if pad else x


def _code_pair(queries, corpus, dtypes, what: str):
    """Both code matrices as 2-D tensors of one of `dtypes`, same type and width -- checked before anything moves."""
    q, c = util._as_rows(queries), util._as_rows(corpus)
    if q.dtype not in dtypes:
        raise ValueError(f"{what} codes are {' or '.join(str(d) for d in dtypes)} (got {q.dtype})")
    if q.dtype != c.dtype:
        raise ValueError(f"query and corpus codes differ in type: {q.dtype} vs {c.dtype}")
    if q.dim() != 2 or c.dim() != 2 or q.shape[0] < 1 or c.shape[0] < 1 or q.shape[1] < 1:
        raise ValueError(f"codes must be non-empty [n, width] arrays (got {tuple(q.shape)} and {tuple(c.shape)})")
    if q.shape[1] != c.shape[1]:
        raise ValueError(f"code widths differ: {tuple(q.shape)} vs {tuple(c.shape)}")
    return q, c


def _stream(entry: str, q: torch.Tensor, c: torch.Tensor, multiple: int, k: int, chunk, exclude_self: bool, state,
            query_base: int, corpus_base: int):
    from . import _lib
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= util.TOPK_MAX:
        raise ValueError(f"k must be an integer between 1 and {util.TOPK_MAX} (got {k!r})")
    chunk = STREAM_CHUNK if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be positive")
    if not q.is_cuda:
        if not torch.cuda.is_available():
            raise _lib.QstError("the quantized search runs on the HIP device and none is visible (there is no CPU path)")
        q = q.to(torch.device("cuda", torch.cuda.current_device()))
    lib = _lib.load()
    q = _padded(q.contiguous(), multiple)
    c = _padded(c.to(q.device).contiguous(), multiple)
    nq, width = q.shape
    nc = c.shape[0]
    chunk = min(chunk, nc)
    rs, ri = util._new_state(nq, k, q.device) if state is None else util._check_state(state, nq, k, q.device)
    with torch.cuda.device(q.device):
        ws = torch.empty(getattr(lib, f"qst_topk_{entry}_workspace_bytes")(nq, chunk, width), dtype=torch.uint8, device=q.device)
        _lib.check(getattr(lib, f"qst_topk_{entry}_stream")(q.data_ptr(), c.data_ptr(), nq, nc, width, int(k), chunk,
                                                            int(query_base), int(corpus_base), int(bool(exclude_self)),
                                                            rs.data_ptr(), ri.data_ptr(), ws.data_ptr(), ws.numel(),
                                                            _lib.current_stream_ptr()), f"qst_topk_{entry}_stream")
    return rs, ri


def hamming_topk(queries, corpus, k: int, chunk: int = None, exclude_self: bool = False, state=None, query_base: int = 0,
                 corpus_base: int = 0):
    """util.topk_stream on packed sign bits (libqst qst_topk_hamming_stream): queries / corpus are 'binary' (int8) or
    'ubinary' (uint8) codes of the same kind and width; the score is -(Hamming distance) as f32. Ids, exclude_self, the
    -inf / -1 padding, the order and the `state=` continuation are topk_stream's. Rows are zero-padded to 4 bytes."""
    q, c = _code_pair(queries, corpus, (torch.int8, torch.uint8), "packed")
    return _stream("hamming", q.view(torch.uint8), c.view(torch.uint8), 4, k, chunk, exclude_self, state, query_base,
                   corpus_base)


def int8_topk(queries, corpus, k: int, chunk: int = None, exclude_self: bool = False, state=None, query_base: int = 0,
              corpus_base: int = 0):
    """util.topk_stream on int8 codes (libqst qst_topk_int8_stream): the score is the exact integer dot product as f32.
    Widths up to 1024 (zero-padded to a multiple of 32); the rest as hamming_topk."""
    q, c = _code_pair(queries, corpus, (torch.int8,), "int8")
    if q.shape[1] > INT8_MAX_DIM:
        raise ValueError(f"the int8 search takes widths up to {INT8_MAX_DIM}: beyond it the int32 score is not exact in f32")
    return _stream("int8", q, c, 32, k, chunk, exclude_self, state, query_base, corpus_base)


def rescore_quantized(queries, corpus, precision: str, candidates: torch.Tensor, dim: int = None,
                      check_ids: bool = True) -> torch.Tensor:
    """f32 [nq, kc]: the float queries against the quantized corpus rows `candidates` (int64 [nq, kc], -1 = none -> -inf)
    names, summed in fp32 (libqst qst_rescore_quantized). For the bit kinds the bit (0 / 1) multiplies the query entry,
    for int8 / uint8 the stored integer: upstream's rescoring products. `dim` is the unpacked width (bits only). The library cannot refuse an id >= the corpus size (the ids
    live on the device), so they are checked here, at the price of one read-back; check_ids=False skips that."""
    from . import _lib
    lib = _lib.load()
    kind = _KINDS[precision]
    q = _float_rows(queries, "queries")
    c = util._as_rows(corpus)
    if c.dtype != _OUT_DTYPE[kind]:
        raise ValueError(f"a {precision!r} corpus is {_OUT_DTYPE[kind]} (got {c.dtype})")
    c = c.to(q.device).contiguous()
    nq, qdim = q.shape
    bits = kind in (QUANT_BINARY, QUANT_UBINARY)
    dim = qdim if dim is None else int(dim)
    if dim != qdim or c.shape[1] != ((dim + 7) // 8 if bits else dim):
        raise ValueError(f"widths differ: queries {tuple(q.shape)}, {precision!r} corpus {tuple(c.shape)}")
    cand = candidates.to(q.device, torch.int64).contiguous()
    if cand.dim() != 2 or cand.shape[0] != nq or cand.shape[1] < 1:
        raise ValueError(f"candidates must be int64 [{nq}, kc] (got {tuple(cand.shape)})")
    if check_ids and int(cand.max()) >= c.shape[0]:
        raise ValueError("a candidate id is not a corpus row")
    kc = cand.shape[1]
    with torch.cuda.device(q.device):
        out = torch.empty(nq, kc, dtype=torch.float32, device=q.device)
        _lib.check(lib.qst_rescore_quantized(q.data_ptr(), c.data_ptr(), kind, c.shape[0], dim, cand.data_ptr(), kc, nq, kc,
                                             out.data_ptr(), _lib.current_stream_ptr()), "qst_rescore_quantized")
    return out


def semantic_search_quantized(query_embeddings, corpus_embeddings, corpus_precision: str = "binary", top_k: int = 10,
                              ranges=None, calibration_embeddings=None, rescore: bool = True, rescore_multiplier: int = 4,
                              corpus_chunk_size: int = None, exclude_self: bool = False):
    """Retrieve on quantized codes, rescore with the float query (sentence_transformers.quantization's search, on the
    device): one list per query of {'corpus_id', 'score'}, as util.semantic_search returns.

    corpus_embeddings are float32 (quantized here) or already codes of `corpus_precision` ('binary', 'ubinary' or 'int8').
    Float queries are quantized like the corpus: bits need no ranges; int8 needs `ranges` or `calibration_embeddings` (a
    query set's own range says nothing about the corpus's buckets). The first stage keeps kc = min(top_k *
    rescore_multiplier, corpus size) candidates by -(Hamming distance) or by the integer dot product. rescore=True scores
    them again as float query x quantized row (qst_rescore_quantized) and cuts to top_k; rescore=False returns the first
    stage's scores. The order is score descending, then corpus id ascending, in both."""
    if corpus_precision == "uint8":
        raise ValueError("corpus_precision='uint8' is not searchable: a uint8 x uint8 dot product does not rank like the "
                         "shifted codes; quantize the corpus as 'int8'")
    if corpus_precision not in ("binary", "ubinary", "int8"):
        raise ValueError(f"corpus_precision must be 'binary', 'ubinary' or 'int8' (got {corpus_precision!r})")
    if isinstance(top_k, bool) or int(top_k) != top_k or top_k < 1:
        raise ValueError(f"top_k must be a positive integer (got {top_k!r})")
    if isinstance(rescore_multiplier, bool) or int(rescore_multiplier) != rescore_multiplier or rescore_multiplier < 1:
        raise ValueError(f"rescore_multiplier must be a positive integer (got {rescore_multiplier!r})")
    top_k, rescore_multiplier = int(top_k), int(rescore_multiplier)
    if top_k * rescore_multiplier > RESCORE_MAX:
        raise ValueError(f"top_k * rescore_multiplier must not exceed {RESCORE_MAX} (got {top_k} * {rescore_multiplier})")
    if corpus_chunk_size is not None and corpus_chunk_size < 1:
        raise ValueError("corpus_chunk_size must be positive")
    kind = _KINDS[corpus_precision]
    bits = kind != QUANT_INT8
    queries = util._as_rows(query_embeddings)
    corpus = util._as_rows(corpus_embeddings)
    if not queries.dtype.is_floating_point:
        raise ValueError(f"query_embeddings must be float embeddings: they rescore the candidates (got {queries.dtype})")
    if corpus.dtype.is_floating_point:
        if corpus.shape[1] != queries.shape[1]:
            raise ValueError(f"embedding sizes differ: {tuple(queries.shape)} vs {tuple(corpus.shape)}")
    else:
        if corpus.dtype != _OUT_DTYPE[kind]:
            raise ValueError(f"a {corpus_precision!r} corpus is {_OUT_DTYPE[kind]} (got {corpus.dtype})")
        want = (queries.shape[1] + 7) // 8 if bits else queries.shape[1]
        if corpus.shape[1] != want:
            raise ValueError(f"widths differ: queries {tuple(queries.shape)} need a {corpus_precision!r} corpus of width "
                             f"{want} (got {tuple(corpus.shape)})")
    if not bits and ranges is None and calibration_embeddings is None:
        raise ValueError("int8 search needs `ranges` or `calibration_embeddings`: the queries must fall into the corpus's "
                         "buckets, and their own range does not give those")

    q = _float_rows(queries, "query_embeddings")
    r = None if bits else _resolve_ranges(q, ranges, calibration_embeddings, warn=False)
    if corpus.dtype.is_floating_point:
        c_codes = _quantize_device(_float_rows(corpus, "corpus_embeddings").to(q.device), kind, r)
    else:
        c_codes = _code_rows(corpus, _OUT_DTYPE[kind], "corpus_embeddings").to(q.device)
    q_codes = _quantize_device(q, kind, r)
    nc = c_codes.shape[0]
    chunk = corpus_chunk_size
    first = hamming_topk if bits else int8_topk
    if not rescore:
        rs, ri = first(q_codes, c_codes, min(top_k, nc), chunk=chunk, exclude_self=exclude_self)
    else:
        kc = min(top_k * rescore_multiplier, nc)
        _, cand = first(q_codes, c_codes, kc, chunk=chunk, exclude_self=exclude_self)
        # ascending ids per row (-1 = no candidate first): the second select breaks ties by column, which is then by id
        cand, _ = torch.sort(cand, dim=1)
        scores = rescore_quantized(q, c_codes, corpus_precision, cand, check_ids=False)     # ids of the first stage
        rs, col = util.topk_merge_rows(scores, min(top_k, kc))
        ri = torch.where(col >= 0, torch.gather(cand, 1, col.clamp(min=0)), col)
        rs = torch.where(ri >= 0, rs, torch.full_like(rs, float("-inf")))
    sc, idx = rs.cpu().numpy(), ri.cpu().numpy()
    return [[{"corpus_id": int(c), "score": float(s)} for s, c in zip(sc[i], idx[i]) if c >= 0] for i in range(len(sc))]
