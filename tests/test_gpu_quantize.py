"""GPU: embedding quantization (csrc/quantize.hip) -- qst_column_ranges, qst_quantize_rows, the two first stages
qst_topk_hamming_stream / qst_topk_int8_stream, qst_rescore_quantized -- and what stands on them: quantize_embeddings,
semantic_search_quantized, util.hamming_topk / int8_topk and encode(precision=<output name>). The yardstick is numpy
(tests/quantize_helpers.py) and the full stable sort of tests/topk_stream_cases.py. Every integer result is compared with
==; the exact integer scores of the int8 stream are also the confirmation of the A/B lane map of v_mfma_i32_32x32x32_i8
that the kernel assumes."""
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import quantize_helpers as Q  # noqa: E402
import topk_stream_cases as T  # noqa: E402
from kernel_helpers import lib, stream  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib, quantization, util  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import SentenceTransformer  # noqa: E402

INF = float("inf")
OUT_DTYPE = {Q.INT8: torch.int8, Q.UINT8: torch.uint8, Q.BINARY: torch.int8, Q.UBINARY: torch.uint8}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


# ------------------------------------------------------------------ 1. qst_column_ranges
def ranges_dev(lib, xd):
    n, dim = xd.shape
    out = torch.full((2, dim), 7.0, device="cuda")
    ws = torch.empty(lib.qst_column_ranges_workspace_bytes(n, dim), dtype=torch.uint8, device="cuda")
    assert lib.qst_column_ranges(xd.data_ptr(), n, dim, out.data_ptr(), ws.data_ptr(), ws.numel(), stream()) == 0
    return out.cpu().numpy()


# 1300 rows: past one pass of the first stage's row loop (128 slices x 4 row lanes = 512 rows a pass)
@pytest.mark.parametrize("dim", [1, 33, 384])
@pytest.mark.parametrize("n", [1, 2, 300, 1300])
def test_column_ranges_equal_numpy_with_a_nan_and_a_constant_column(lib, n, dim):
    x = np.random.RandomState(n + dim).randn(n, dim).astype(np.float32)
    x[:, dim // 2] = 2.5                                  # constant
    np.testing.assert_array_equal(ranges_dev(lib, dev(x)), Q.ranges_ref(x))
    if dim > 1:
        x[n - 1, dim - 1] = np.nan                        # in the last row a slice sees, in the last column
        x[n // 2, 0] = np.nan
        want = Q.ranges_ref(x)
        assert np.isnan(want[:, [0, dim - 1]]).all() and not np.isnan(want[:, 1:dim - 1]).any()
        np.testing.assert_array_equal(ranges_dev(lib, dev(x)), want)
        np.testing.assert_array_equal(quantization.column_ranges(x).cpu().numpy(), want)


# ------------------------------------------------------------------ 2. qst_quantize_rows
def quantize_dev(lib, xd, kind, ranges=None):
    n, dim = xd.shape
    width = (dim + 7) // 8 if kind in (Q.BINARY, Q.UBINARY) else dim
    guard = 64
    flat = torch.full((n * width + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = lib.qst_quantize_rows(xd.data_ptr(), n, dim, kind, _lib.ptr(ranges), flat.data_ptr(), stream())
    assert rc == 0
    assert (flat[n * width:] == 0x5A).all()               # nothing past the last row
    return flat[:n * width].view(n, width).view(OUT_DTYPE[kind]).cpu().numpy()


@pytest.mark.parametrize("kind", [Q.UBINARY, Q.BINARY])
@pytest.mark.parametrize("dim", [8, 13, 32, 40, 72, 384, 1000])
def test_bits_equal_packbits(lib, dim, kind):
    for n in (1, 5, 257):
        x = Q.salted(n, dim, seed=n + dim)
        want = Q.bits_ref(x, kind)
        np.testing.assert_array_equal(quantize_dev(lib, dev(x), kind), want)
        # a row-slice view with an odd element offset: 4-byte aligned only, so the element path
        flat = torch.zeros(n * dim + 3, device="cuda")
        view = flat[3:].view(n, dim)
        view.copy_(dev(x))
        assert view.data_ptr() % 16 != 0
        np.testing.assert_array_equal(quantize_dev(lib, view, kind), want)
    name = "ubinary" if kind == Q.UBINARY else "binary"
    got = quantization.quantize_embeddings(x, name)
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype
    np.testing.assert_array_equal(got, want)


def test_bits_of_the_special_values(lib):
    x = np.array([[0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1.0, -1.0, 3e-39, -np.nan, 2.0, 0.0]], dtype=np.float32)
    assert x.shape[1] == 13
    got = quantize_dev(lib, dev(x), Q.UBINARY)
    np.testing.assert_array_equal(got, [[0b00010101, 0b01010000]])       # pad bits 0
    np.testing.assert_array_equal(quantize_dev(lib, dev(x), Q.BINARY).view(np.uint8), got ^ 0x80)


def calibration(dim, seed):
    return np.random.RandomState(seed).randn(1000, dim).astype(np.float32)


@pytest.mark.parametrize("kind", [Q.UINT8, Q.INT8])
@pytest.mark.parametrize("dim", [384, 13])
def test_codes_equal_the_fp32_formula_at_the_bin_edges_and_outside(lib, dim, kind):
    cal = calibration(dim, seed=dim)
    cal[:, 5] = 0.25                                      # a constant column
    ranges = Q.ranges_ref(cal)
    rd = dev(ranges)
    np.testing.assert_array_equal(ranges_dev(lib, dev(cal)), ranges)
    lo, hi = ranges
    step = (hi - lo) / np.float32(255.0)
    edges = (lo[None, :] + np.arange(256, dtype=np.float32)[:, None] * step[None, :]).astype(np.float32)     # lo + j * step
    outside = np.stack([lo - 1.0, hi + 1.0, lo - 1e30, hi + 1e30, np.full(dim, np.inf), np.full(dim, -np.inf)]).astype(np.float32)
    special = cal[:7].copy()
    special[0, 3] = np.nan
    special[1, :] = np.nan
    x = np.concatenate([edges, np.nextafter(edges, np.float32(np.inf)), np.nextafter(edges, np.float32(-np.inf)), outside,
                        special, cal[:300]]).astype(np.float32)
    want = Q.codes_ref(x, ranges, kind)
    got = quantize_dev(lib, dev(x), kind, rd)
    np.testing.assert_array_equal(got, want)
    assert (want[:, 5] == (0 if kind == Q.UINT8 else -128)).all()
    # the misaligned element path gives the same codes
    flat = torch.zeros(x.size + 1, device="cuda")
    view = flat[1:].view(x.shape)
    view.copy_(dev(x))
    np.testing.assert_array_equal(quantize_dev(lib, view, kind, rd), want)
    name = "uint8" if kind == Q.UINT8 else "int8"
    for via in (dict(ranges=ranges), dict(calibration_embeddings=cal)):
        out = quantization.quantize_embeddings(torch.from_numpy(x), name, **via)
        assert torch.is_tensor(out) and out.is_cuda
        np.testing.assert_array_equal(out.cpu().numpy(), want)
    np.testing.assert_array_equal(quantization.quantize_embeddings(cal, name), Q.codes_ref(cal, ranges, kind))
    f = quantization.quantize_embeddings(cal[:3], "float32")
    assert f.dtype == np.float32
    np.testing.assert_array_equal(f, cal[:3])


# ------------------------------------------------------------------ 3. qst_topk_hamming_stream
def new_state(rows, k):
    return (torch.full((rows, k), -INF, dtype=torch.float32, device="cuda"),
            torch.full((rows, k), -1, dtype=torch.int64, device="cuda"))


def stream_dev(lib, entry, qd, cd, k, chunk, pieces=None, exclude_self=0, query_base=0, corpus_base=0):
    """One call over the whole corpus, or one per (start, stop) piece with the state carried over."""
    fn, size = {"hamming": (lib.qst_topk_hamming_stream, lib.qst_topk_hamming_workspace_bytes),
                "int8": (lib.qst_topk_int8_stream, lib.qst_topk_int8_workspace_bytes)}[entry]
    nq, width = qd.shape
    rs, ri = new_state(nq, k)
    for a, b in pieces or [(0, cd.shape[0])]:
        ch = min(chunk, b - a)
        ws = torch.empty(size(nq, ch, width), dtype=torch.uint8, device="cuda")
        rc = fn(qd.data_ptr(), cd.data_ptr() + a * width, nq, b - a, width, k, ch, query_base, corpus_base + a, exclude_self,
                rs.data_ptr(), ri.data_ptr(), ws.data_ptr(), ws.numel(), stream())
        assert rc == 0, rc
    return rs.cpu().numpy(), ri.cpu().numpy()


def cut(want, k):
    return want[0][:, :k], want[1][:, :k]


def check_stream(lib, entry, q, c, scores, corpus_base=0):
    """Every k, every chunking and a corpus fed in three pieces against the full sort of the exact scores."""
    nq, nc = scores.shape
    qd, cd = dev(q), dev(c)
    kmax = min(nc, 1024)
    want = T.topk_ref(scores, kmax, col_base=corpus_base)
    for k in sorted({1, min(10, nc), kmax}):
        for chunk in sorted({1, 7, 256, nc}):
            if nq > 64 and chunk == 1 and nc > 300:
                chunk = 3                                  # thousands of launches of 2 row blocks otherwise; still ragged
            same(stream_dev(lib, entry, qd, cd, k, chunk, corpus_base=corpus_base), cut(want, k))
        same(stream_dev(lib, entry, qd, cd, k, 256, pieces=T.slices(nc, 3), corpus_base=corpus_base), cut(want, k))


@pytest.mark.parametrize("nbytes", [4, 12, 20, 48, 96, 128])
@pytest.mark.parametrize("nq", [1, 3, 33, 2049])
def test_hamming_stream_equals_the_full_sort_for_every_chunking(lib, nq, nbytes):
    for nc in (1, 5, 257, 1000):
        c = Q.random_codes(nc, nbytes, seed=nc + nbytes)
        q = Q.random_codes(nq, nbytes, seed=nq + 7 * nbytes, duplicates=False)
        scores = Q.hamming_scores(q, c)
        if nbytes == 4 and nc == 1000:
            assert len(np.unique(scores[0])) <= 33          # every cut falls inside ties
        check_stream(lib, "hamming", q, c, scores, corpus_base=1000)


def test_hamming_exclude_self_and_padding(lib):
    c = Q.random_codes(300, 12, seed=5)
    scores = Q.hamming_scores(c, c)
    cd = dev(c)
    for k in (1, 10, 300):
        want = T.topk_ref(scores, k, col_base=40, row_base=40, exclude_self=True)
        assert (want[1][:, -1] == -1).all() if k == 300 else True
        for chunk in (7, 300):
            same(stream_dev(lib, "hamming", cd, cd, k, chunk, exclude_self=1, query_base=40, corpus_base=40), want)
    # without it, the row itself (distance 0) or a duplicate with a smaller id comes first
    got = stream_dev(lib, "hamming", cd, cd, 1, 64)
    assert (got[0] == 0).all() and (got[1][:, 0] <= np.arange(300)).all()


def test_hamming_bases_that_are_4_byte_but_not_16_byte_aligned(lib):
    nq, nc, nbytes = 33, 257, 48                          # nbytes % 16 == 0: only the bases keep it off the 16-byte path
    q, c = Q.random_codes(nq, nbytes, 1, duplicates=False), Q.random_codes(nc, nbytes, 2)
    want = T.topk_ref(Q.hamming_scores(q, c), 10)
    qf = torch.zeros(nq * nbytes + 4, dtype=torch.uint8, device="cuda")
    cf = torch.zeros(nc * nbytes + 12, dtype=torch.uint8, device="cuda")
    qv, cv = qf[4:].view(nq, nbytes), cf[12:].view(nc, nbytes)
    qv.copy_(dev(q)); cv.copy_(dev(c))
    assert qv.data_ptr() % 16 == 4 and cv.data_ptr() % 16 == 12
    same(stream_dev(lib, "hamming", qv, cv, 10, 100), want)
    same(stream_dev(lib, "hamming", dev(q), cv, 10, 100), want)
    same(stream_dev(lib, "hamming", dev(q), dev(c), 10, 100), want)


def test_hamming_topk_wrapper_binary_equals_ubinary_and_pads_odd_widths():
    x = np.random.RandomState(3).randn(120, 72).astype(np.float32)          # 72 bits = 9 bytes: padded to 12
    ub, b = Q.bits_ref(x, Q.UBINARY), Q.bits_ref(x, Q.BINARY)
    want = T.topk_ref(Q.hamming_scores(ub[:7], ub), 10)
    for codes in (ub, b):
        for fn in (util.hamming_topk, quantization.hamming_topk):
            rs, ri = fn(codes[:7], codes, 10, chunk=50)
            same((rs.cpu().numpy(), ri.cpu().numpy()), want)
    state = None
    for a, z in T.slices(120, 3):
        state = util.hamming_topk(ub[:7], ub[a:z], 10, chunk=16, state=state, corpus_base=a)
    same((state[0].cpu().numpy(), state[1].cpu().numpy()), want)


# ------------------------------------------------------------------ 4. qst_topk_int8_stream
def full_range_codes(n, dim, seed):
    return np.random.RandomState(seed).randint(-128, 128, size=(n, dim)).astype(np.int8)


@pytest.mark.parametrize("dim", [32, 64, 96, 384, 1024])
def test_int8_stream_equals_the_integer_product_for_every_chunking(lib, dim):
    for nq in (1, 31, 33, 65):
        for nc in (1, 31, 33, 65):
            q, c = full_range_codes(nq, dim, nq + dim), full_range_codes(nc, dim, 3 * nc + dim)
            check_stream(lib, "int8", q, c, Q.int8_scores(q, c))


def test_int8_largest_score_is_exactly_2_to_the_24(lib):
    q = np.full((33, 1024), -128, dtype=np.int8)
    c = np.full((65, 1024), -128, dtype=np.int8)
    c[::2, 0] = 127                                       # every other row scores 2^24 - 128 * 255
    scores = Q.int8_scores(q, c)
    assert scores.max() == 2.0 ** 24 and scores.min() == 2.0 ** 24 - 128 * 255
    same(stream_dev(lib, "int8", dev(q), dev(c), 65, 16), T.topk_ref(scores, 65))


def test_int8_one_hot_queries_read_the_right_row_and_column(lib):
    """Query r is one-hot at k = r (value 1): its scores are column r of the corpus, rows of distinct small integers --
    asymmetric data, so a swapped row / column or a k offset read from the wrong half of a fragment shows."""
    dim, nc = 96, 65
    q = np.zeros((dim, dim), dtype=np.int8)
    q[np.arange(dim), np.arange(dim)] = 1
    c = ((np.arange(nc)[:, None] * 7 + np.arange(dim)[None, :] * 3) % 251 - 125).astype(np.int8)
    scores = Q.int8_scores(q, c)
    np.testing.assert_array_equal(scores, c.T.astype(np.float32))
    same(stream_dev(lib, "int8", dev(q), dev(c), nc, nc), T.topk_ref(scores, nc))
    same(stream_dev(lib, "int8", dev(c), dev(q), dim, 40), T.topk_ref(scores.T.copy(), dim))


def test_int8_width_1056_is_refused_and_the_wrapper_pads(lib):
    q = dev(full_range_codes(2, 1056, 1))
    rs, ri = new_state(2, 1)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    assert lib.qst_topk_int8_stream(q.data_ptr(), q.data_ptr(), 2, 2, 1056, 1, 2, 0, 0, 0, rs.data_ptr(), ri.data_ptr(),
                                    ws.data_ptr(), ws.numel(), stream()) == -2
    assert (ri == -1).all()
    qc, cc = full_range_codes(5, 40, 2), full_range_codes(70, 40, 3)      # 40 is padded to 64
    want = T.topk_ref(Q.int8_scores(qc, cc), 10)
    for fn in (util.int8_topk, quantization.int8_topk):
        rs, ri = fn(qc, cc, 10, chunk=32)
        same((rs.cpu().numpy(), ri.cpu().numpy()), want)
    state = None
    for a, z in T.slices(70, 3):
        state = util.int8_topk(qc, cc[a:z], 10, state=state, corpus_base=a)
    same((state[0].cpu().numpy(), state[1].cpu().numpy()), want)
    got = util.int8_topk(cc, cc, 3, exclude_self=True)
    same((got[0].cpu().numpy(), got[1].cpu().numpy()), T.topk_ref(Q.int8_scores(cc, cc), 3, exclude_self=True))


# ------------------------------------------------------------------ 5. qst_rescore_quantized
def rescore_dev(lib, qd, codes_d, kind, dim, cand_d, kc):
    nq, ld = cand_d.shape
    out = torch.full((nq, ld), 123.0, device="cuda")
    rc = lib.qst_rescore_quantized(qd.data_ptr(), codes_d.data_ptr(), kind, codes_d.shape[0], dim, cand_d.data_ptr(), ld, nq, kc,
                                   out.data_ptr(), stream())
    assert rc == 0
    assert (out[:, kc:] == 123.0).all()                   # columns kc .. ld are the caller's
    return out[:, :kc].cpu().numpy()


def corpus_codes(kind, nc, dim, seed):
    rng = np.random.RandomState(seed)
    if kind in (Q.BINARY, Q.UBINARY):
        return Q.bits_ref(rng.randn(nc, dim).astype(np.float32), kind)
    if kind == Q.INT8:
        return rng.randint(-128, 128, size=(nc, dim)).astype(np.int8)
    return rng.randint(0, 256, size=(nc, dim)).astype(np.uint8)


@pytest.mark.parametrize("kind", [Q.INT8, Q.UINT8, Q.BINARY, Q.UBINARY])
@pytest.mark.parametrize("dim", [13, 384])
def test_rescore_is_exact_on_integer_queries_and_within_the_fp32_bound_on_gaussian_ones(lib, dim, kind):
    nq, nc = 9, 50
    codes = corpus_codes(kind, nc, dim, seed=dim + kind)
    cd = dev(codes)
    rng = np.random.RandomState(kind)
    for kc in (1, 5, 40):
        cand = rng.randint(0, nc, size=(nq, kc + 2)).astype(np.int64)
        cand[rng.rand(nq, kc + 2) < 0.2] = -1
        cand[0, 0] = -1
        rows = np.arange(nq)[:, None]
        missing = cand[:, :kc] < 0
        # integer queries in [-3, 3]: every partial sum is an integer below 2^24, so any order of summation is exact
        qi = rng.randint(-3, 4, size=(nq, dim)).astype(np.float32)
        full, _ = Q.rescore_ref(qi, codes, kind, dim)
        want = np.where(missing, -np.inf, full[rows, np.maximum(cand[:, :kc], 0)]).astype(np.float32)
        np.testing.assert_array_equal(rescore_dev(lib, dev(qi), cd, kind, dim, dev(cand), kc), want)
        qg = rng.randn(nq, dim).astype(np.float32)
        full, mag = Q.rescore_ref(qg, codes, kind, dim)
        got = rescore_dev(lib, dev(qg), cd, kind, dim, dev(cand), kc)
        assert (got[missing] == -np.inf).all()
        err = np.abs(got.astype(np.float64) - full[rows, np.maximum(cand[:, :kc], 0)])
        bound = Q.rescore_bound(dim, mag[rows, np.maximum(cand[:, :kc], 0)])
        assert (err[~missing] <= bound[~missing]).all(), (err[~missing] / bound[~missing]).max()
    name = {v: k for k, v in Q.KIND.items()}[kind]
    got = quantization.rescore_quantized(qi, codes, name, torch.from_numpy(cand[:, :kc]))
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError, match="corpus row"):
        quantization.rescore_quantized(qi, codes, name, torch.full((nq, 1), nc, dtype=torch.int64))


# ------------------------------------------------------------------ 6. capture
def test_the_whole_chain_is_capturable_in_a_graph():
    """No host synchronisation anywhere and the workspaces are the caller's: ranges -> int8 codes of both sides -> the int8
    first stage -> rescoring, captured once (one branch), replays on new inputs to the bits of plain calls."""
    rng = np.random.RandomState(4)
    c1, c2 = rng.randn(300, 64).astype(np.float32), rng.randn(300, 64).astype(np.float32)
    q1, q2 = c1[:9] + 0.1, c2[:9] - 0.1

    def chain(qd, cd):
        r = quantization.column_ranges(cd)
        cc, qc = quantization._quantize_device(cd, Q.INT8, r), quantization._quantize_device(qd, Q.INT8, r)
        rs, ri = util.int8_topk(qc, cc, 10, chunk=128)
        return rs, ri, quantization.rescore_quantized(qd, cc, "int8", ri, check_ids=False)

    qd, cd = dev(q1), dev(c1)
    chain(qd, cd)                                          # code objects loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = chain(qd, cd)
    qd.copy_(dev(q2)), cd.copy_(dev(c2))
    graph.replay()
    torch.cuda.synchronize()
    want = chain(dev(q2), dev(c2))
    assert all(torch.equal(a, b) for a, b in zip(out, want))
    assert (out[1][:, 0].cpu() == torch.arange(9)).all()


# ------------------------------------------------------------------ 7. end to end
@pytest.fixture(scope="module")
def search_case():
    rng = np.random.RandomState(11)
    corpus = rng.randn(600, 384).astype(np.float32)
    src = rng.choice(600, size=20, replace=False)
    queries = (corpus[src] + 0.1 * rng.randn(20, 384)).astype(np.float32)
    return corpus, queries, src


def numpy_first_stage(corpus, queries, precision, k, ranges=None):
    kind = Q.KIND[precision]
    if kind == Q.INT8:
        cc, qc = Q.codes_ref(corpus, ranges, kind), Q.codes_ref(queries, ranges, kind)
        scores = Q.int8_scores(qc, cc)
    else:
        cc, qc = Q.bits_ref(corpus, kind), Q.bits_ref(queries, kind)
        scores = Q.hamming_scores(qc, cc)
    return cc, T.topk_ref(scores, k)


@pytest.mark.parametrize("precision", ["binary", "int8"])
def test_search_without_rescoring_equals_the_numpy_pipeline(search_case, precision):
    corpus, queries, src = search_case
    ranges = Q.ranges_ref(corpus)
    kw = dict(calibration_embeddings=corpus) if precision == "int8" else {}
    _, (ws, wi) = numpy_first_stage(corpus, queries, precision, 10, ranges)
    want = [[{"corpus_id": int(c), "score": float(s)} for s, c in zip(ws[r], wi[r])] for r in range(20)]
    assert quantization.semantic_search_quantized(queries, corpus, precision, top_k=10, rescore=False, **kw) == want
    assert quantization.semantic_search_quantized(torch.from_numpy(queries), torch.from_numpy(corpus).cuda(), precision,
                                                  top_k=10, rescore=False, corpus_chunk_size=77, **kw) == want
    # a corpus that is already codes, and ranges given as such
    codes = quantization.quantize_embeddings(corpus, precision, ranges=ranges if precision == "int8" else None)
    kw = dict(ranges=ranges) if precision == "int8" else {}
    assert quantization.semantic_search_quantized(queries, codes, precision, top_k=10, rescore=False, **kw) == want
    assert [hit[0]["corpus_id"] for hit in want] == list(src)


@pytest.mark.parametrize("precision", ["binary", "int8"])
def test_search_with_rescoring_ranks_the_candidates_by_the_float_product(search_case, precision):
    corpus, queries, src = search_case
    ranges = Q.ranges_ref(corpus)
    kw = dict(calibration_embeddings=corpus) if precision == "int8" else {}
    top_k, mult = 10, 4
    codes, (_, cand) = numpy_first_stage(corpus, queries, precision, top_k * mult, ranges)
    full, mag = Q.rescore_ref(queries, codes, Q.KIND[precision], 384)
    tol = float(Q.rescore_bound(384, mag.max()))          # the bound of the pair with the largest sum of magnitudes
    masked = np.full_like(full, -np.inf)
    rows = np.arange(20)[:, None]
    masked[rows, cand] = full[rows, cand]                 # only the first stage's candidates take part
    _, want_ids = T.topk_ref(masked, top_k)
    hits = quantization.semantic_search_quantized(queries, corpus, precision, top_k=top_k, rescore_multiplier=mult, **kw)
    assert [len(h) for h in hits] == [top_k] * 20
    got_ids = np.array([[h["corpus_id"] for h in row] for row in hits], dtype=np.int64)
    got_scores = np.array([[h["score"] for h in row] for row in hits], dtype=np.float32)
    assert all(set(got_ids[r]) <= set(cand[r]) for r in range(20))
    n_bad = T.ranking_disagreements(got_scores, got_ids, full, want_ids, lambda s: tol)
    print(f"{precision}: tolerance {tol:.3e}, positions that differ from the fp64 ranking inside it: {n_bad}")
    assert list(got_ids[:, 0]) == list(src)               # every query's own source row is rank 1
    # fewer corpus rows than top_k * multiplier, and self-exclusion: shorter lists, same order rules
    small = quantization.semantic_search_quantized(corpus[:5], corpus[:5], precision, top_k=3, exclude_self=True,
                                                   **(dict(calibration_embeddings=corpus) if precision == "int8" else {}))
    assert [len(h) for h in small] == [3] * 5 and all(h["corpus_id"] != r for r, row in enumerate(small) for h in row)


def test_search_ties_after_rescoring_go_to_the_smaller_id():
    """Two-valued queries against duplicated corpus rows: the rescored products tie exactly, inside and across the cut."""
    rng = np.random.RandomState(2)
    base = rng.randn(6, 64).astype(np.float32)
    corpus = np.concatenate([base, base, base])[rng.permutation(18)]
    queries = np.sign(base[:4]).astype(np.float32)
    hits = quantization.semantic_search_quantized(queries, corpus, "ubinary", top_k=5, rescore_multiplier=3)
    codes = Q.bits_ref(corpus, Q.UBINARY)
    full, _ = Q.rescore_ref(queries, codes, Q.UBINARY, 64)
    _, cand = T.topk_ref(Q.hamming_scores(Q.bits_ref(queries, Q.UBINARY), codes), 15)
    masked = np.full_like(full, -np.inf)
    rows = np.arange(4)[:, None]
    masked[rows, cand] = full[rows, cand]
    ws, wi = T.topk_ref(masked, 5)
    assert hits == [[{"corpus_id": int(c), "score": float(s)} for s, c in zip(ws[r], wi[r])] for r in range(4)]


@pytest.fixture(scope="module")
def vocab_model(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = str(tmp_path_factory.mktemp("quantize") / "tiny-bert-vocab")
    SentenceTransformer("tiny-bert", device="cuda").save(d)
    shutil.copy(os.path.join(root, "tests", "golden", "tiny_vocab.txt"), os.path.join(d, "vocab.txt"))
    return SentenceTransformer(d, device="cuda")


SENTENCES = ["a man rides a horse", "two dogs play in the park", "a woman is cooking", "the horse", "dogs",
             "a man and a woman play with two dogs in the park", "cooking"]


@pytest.mark.parametrize("precision", ["ubinary", "int8", "binary", "uint8", "float32"])
def test_encode_output_precisions_equal_quantizing_the_encoded_rows(vocab_model, precision):
    m = vocab_model
    plain = m.encode(SENTENCES, batch_size=3)
    assert plain.dtype == np.float32
    want = quantization.quantize_embeddings(plain, precision)
    got = m.encode(SENTENCES, batch_size=3, precision=precision)
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype
    np.testing.assert_array_equal(got, want)
    t = m.encode(SENTENCES, batch_size=3, precision=precision, convert_to_tensor=True)
    assert torch.is_tensor(t) and t.is_cuda
    np.testing.assert_array_equal(t.cpu().numpy(), want)
    one = m.encode(SENTENCES[0], precision=precision, normalize_embeddings=True, truncate_dim=16)
    ref = quantization.quantize_embeddings(m.encode(SENTENCES[:1], normalize_embeddings=True, truncate_dim=16), precision)
    np.testing.assert_array_equal(one, ref[0])
    assert m.inference_precision == "bf16"
    with pytest.raises(ValueError, match="token_embeddings"):
        m.encode(SENTENCES, precision=precision, output_value="token_embeddings")


def test_encode_compute_precisions_keep_their_meaning(vocab_model):
    m = vocab_model
    x3 = m.encode(SENTENCES, precision="bf16x3")
    assert x3.dtype == np.float32 and m.inference_precision == "bf16"
    m.inference_precision = "bf16x3"
    try:
        np.testing.assert_array_equal(m.encode(SENTENCES), x3)
        # an output name leaves the forward at inference_precision
        np.testing.assert_array_equal(m.encode(SENTENCES, precision="ubinary"), quantization.quantize_embeddings(x3, "ubinary"))
    finally:
        m.inference_precision = "bf16"
    assert not np.array_equal(m.encode(SENTENCES), x3)
