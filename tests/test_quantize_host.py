"""CPU: embedding quantization without a device -- the numpy yardstick's own bit packing, the library version, every
ValueError of quantization.py that is raised before the device is touched, and the refusals of the new C entries that
return before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import quadruplet_sentence_transformer_amd  # noqa: F401
import quantize_helpers as Q
from quadruplet_sentence_transformer_amd import _lib, quantization, util

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3


def test_helper_packing_is_packbits_and_binary_is_xor_0x80():
    rng = np.random.RandomState(0)
    for dim in (1, 7, 8, 13, 40, 1000):
        bits = rng.randint(0, 2, size=(5, dim))
        np.testing.assert_array_equal(Q.pack_bits(bits), np.packbits(bits.astype(bool), axis=-1))
    x = Q.salted(9, 72, seed=1)
    ub, b = Q.bits_ref(x, Q.UBINARY), Q.bits_ref(x, Q.BINARY)
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(ub, np.packbits(x > 0, axis=-1))
        np.testing.assert_array_equal(b, (np.packbits(x > 0, axis=-1) - 128).astype(np.int8))      # upstream's expression
    np.testing.assert_array_equal(b.view(np.uint8), ub ^ np.uint8(0x80))
    np.testing.assert_array_equal(Q.hamming_scores(ub[:3], ub), Q.hamming_scores(b[:3], b))
    np.testing.assert_array_equal(Q.unpack(b, Q.BINARY, 72), Q.unpack(ub, Q.UBINARY, 72))


def test_helper_codes_follow_the_stated_rules():
    ranges = np.array([[0.0, 1.0, 2.0], [255.0, 1.0, 129.5]], dtype=np.float32)      # steps 1, 0 and 0.5: exact
    x = np.array([[0.0, 1.0, 2.0], [254.9, 5.0, 129.5], [300.0, -5.0, np.nan], [-7.0, np.nan, 900.0]], dtype=np.float32)
    np.testing.assert_array_equal(Q.codes_ref(x, ranges, Q.UINT8), [[0, 0, 0], [254, 0, 255], [255, 0, 0], [0, 0, 255]])
    np.testing.assert_array_equal(Q.codes_ref(x, ranges, Q.INT8),
                                  [[-128, -128, -128], [126, -128, 127], [127, -128, -128], [-128, -128, 127]])
    # trunc, not floor: t - 128 = -0.5 is code 0, where floor would give -1
    np.testing.assert_array_equal(Q.codes_ref(np.array([[127.5]], np.float32), np.array([[0.0], [255.0]], np.float32), Q.INT8),
                                  [[0]])


def test_library_version_and_constants():
    lib = _lib.load()
    assert lib.qst_version() >= 120
    assert (quantization.QUANT_INT8, quantization.QUANT_UINT8, quantization.QUANT_BINARY, quantization.QUANT_UBINARY) == \
           (Q.INT8, Q.UINT8, Q.BINARY, Q.UBINARY) == (0, 1, 2, 3)


def test_workspace_sizes():
    lib = _lib.load()
    assert lib.qst_column_ranges_workspace_bytes(0, 8) == 0 and lib.qst_column_ranges_workspace_bytes(5, 0) == 0
    assert lib.qst_column_ranges_workspace_bytes(1, 384) == lib.qst_column_ranges_workspace_bytes(10 ** 9, 384) > 0
    for fn in (lib.qst_topk_hamming_workspace_bytes, lib.qst_topk_int8_workspace_bytes):
        assert fn(0, 4, 32) == 0 and fn(4, 0, 32) == 0 and fn(4, 4, 0) == 0
        assert fn(5000, 1001, 32) >= 2048 * 1004 * 4                     # one [2048, chunk rounded up to 4] f32 block
        assert fn(3, 1001, 32) >= 3 * 1004 * 4


def _aligned(nbytes=256, align=16, offset=0):
    """(keep-alive buffer, address with address % align == offset) in host memory: never dereferenced by a refusal."""
    buf = C.create_string_buffer(nbytes + 2 * align)
    base = C.addressof(buf)
    return buf, base + (-base) % align + offset


def test_refusals_before_any_launch():
    lib = _lib.load()
    keep, p = _aligned()
    _, p4 = _aligned(offset=4)
    _, p1 = _aligned(offset=1)
    # qst_column_ranges
    assert lib.qst_column_ranges(None, 4, 8, p, p, 1 << 20, None) == BAD_ARG
    assert lib.qst_column_ranges(p, 4, 8, None, p, 1 << 20, None) == BAD_ARG
    assert lib.qst_column_ranges(p, 4, 8, p, None, 1 << 20, None) == BAD_ARG
    assert lib.qst_column_ranges(p, 0, 8, p, p, 1 << 20, None) == BAD_ARG
    assert lib.qst_column_ranges(p, 4, 0, p, p, 1 << 20, None) == BAD_ARG
    assert lib.qst_column_ranges(p1, 4, 8, p, p, 1 << 20, None) == BAD_ARG
    assert lib.qst_column_ranges(p, 4, 8, p, p, lib.qst_column_ranges_workspace_bytes(4, 8) - 1, None) == WORKSPACE
    # qst_quantize_rows
    assert lib.qst_quantize_rows(None, 4, 8, Q.UBINARY, None, p, None) == BAD_ARG
    assert lib.qst_quantize_rows(p, 4, 8, Q.UBINARY, None, None, None) == BAD_ARG
    assert lib.qst_quantize_rows(p, 0, 8, Q.UBINARY, None, p, None) == BAD_ARG
    assert lib.qst_quantize_rows(p, 4, 0, Q.UBINARY, None, p, None) == BAD_ARG
    assert lib.qst_quantize_rows(p, 4, 8, 4, None, p, None) == BAD_ARG and lib.qst_quantize_rows(p, 4, 8, -1, p, p, None) == BAD_ARG
    assert lib.qst_quantize_rows(p, 4, 8, Q.INT8, None, p, None) == BAD_ARG        # 8-bit codes need ranges
    assert lib.qst_quantize_rows(p, 4, 8, Q.UINT8, None, p, None) == BAD_ARG
    assert lib.qst_quantize_rows(p1, 4, 8, Q.BINARY, None, p, None) == BAD_ARG
    # the two streams: (entry, a width it takes, its alignment)
    for fn, width in ((lib.qst_topk_hamming_stream, 8), (lib.qst_topk_int8_stream, 32)):
        ok = [p, p, 2, 3, width, 1, 3, 0, 0, 0, p, p, p, 1 << 20, None]
        for null_at in (0, 1, 10, 11, 12):
            a = list(ok)
            a[null_at] = None
            assert fn(*a) == BAD_ARG
        for at, bad in ((2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (7, -1), (8, -1), (7, 2 ** 63 - 1), (8, 2 ** 63 - 2)):
            a = list(ok)
            a[at] = bad
            assert fn(*a) == BAD_ARG, (at, bad)
        a = list(ok)
        a[5] = 1025
        assert fn(*a) == UNSUPPORTED                                               # k > 1024
        a = list(ok)
        a[13] = 8
        assert fn(*a) == WORKSPACE
    ham = [p, p, 2, 3, 8, 1, 3, 0, 0, 0, p, p, p, 1 << 20, None]
    for nbytes in (1, 2, 6, 13):
        a = list(ham)
        a[4] = nbytes
        assert lib.qst_topk_hamming_stream(*a) == UNSUPPORTED
    a = list(ham)
    a[0] = p1
    assert lib.qst_topk_hamming_stream(*a) == BAD_ARG
    i8 = [p, p, 2, 3, 32, 1, 3, 0, 0, 0, p, p, p, 1 << 20, None]
    for dim in (1, 16, 48, 1056, 2048):
        a = list(i8)
        a[4] = dim
        assert lib.qst_topk_int8_stream(*a) == UNSUPPORTED
    a = list(i8)
    a[1] = p4
    assert lib.qst_topk_int8_stream(*a) == BAD_ARG                                 # 16-byte loads of every fragment
    # qst_rescore_quantized(queries, corpus, kind, nc, dim, cand, ld, nq, kc, out, stream)
    ok = [p, p, Q.INT8, 5, 8, p, 4, 2, 4, p, None]
    for null_at in (0, 1, 5, 9):
        a = list(ok)
        a[null_at] = None
        assert lib.qst_rescore_quantized(*a) == BAD_ARG
    for at, bad in ((2, 4), (2, -1), (3, 0), (4, 0), (7, 0), (8, 0), (6, 3), (5, p4)):
        a = list(ok)
        a[at] = bad
        assert lib.qst_rescore_quantized(*a) == BAD_ARG, (at, bad)
    del keep


def test_value_errors_before_the_device_is_touched():
    rng = np.random.RandomState(0)
    q = rng.randn(3, 64).astype(np.float32)
    c = rng.randn(20, 64).astype(np.float32)
    S = quantization.semantic_search_quantized
    with pytest.raises(ValueError, match="int8"):
        S(q, c, "uint8", ranges=np.zeros((2, 64), np.float32))
    with pytest.raises(ValueError, match="corpus_precision"):
        S(q, c, "float32")
    with pytest.raises(ValueError, match="1024"):
        S(q, c, "binary", top_k=300, rescore_multiplier=4)
    with pytest.raises(ValueError, match="top_k"):
        S(q, c, "binary", top_k=0)
    with pytest.raises(ValueError, match="rescore_multiplier"):
        S(q, c, "binary", rescore_multiplier=0)
    with pytest.raises(ValueError, match="ranges"):
        S(q, c, "int8")
    with pytest.raises(ValueError, match="sizes differ"):
        S(q, c[:, :32], "binary")
    with pytest.raises(ValueError, match="width"):
        S(q, np.zeros((20, 7), np.uint8), "ubinary")                        # 64 bits are 8 bytes
    with pytest.raises(ValueError, match="int8"):
        S(q, np.zeros((20, 8), np.uint8), "binary")                         # 'binary' codes are int8
    with pytest.raises(ValueError, match="float"):
        S(np.zeros((3, 8), np.int8), np.zeros((20, 8), np.int8), "binary")
    with pytest.raises(ValueError, match="precision"):
        quantization.quantize_embeddings(q, "int4")
    for fn in (util.hamming_topk, quantization.hamming_topk):
        with pytest.raises(ValueError, match="differ in type"):
            fn(np.zeros((2, 8), np.uint8), np.zeros((5, 8), np.int8), 1)
        with pytest.raises(ValueError, match="widths differ"):
            fn(np.zeros((2, 8), np.uint8), np.zeros((5, 12), np.uint8), 1)
        with pytest.raises(ValueError, match="packed"):
            fn(q, c, 1)
        with pytest.raises(ValueError, match="k must"):
            fn(np.zeros((2, 8), np.uint8), np.zeros((5, 8), np.uint8), 1025)
    for fn in (util.int8_topk, quantization.int8_topk):
        with pytest.raises(ValueError, match="int8"):
            fn(np.zeros((2, 32), np.uint8), np.zeros((5, 32), np.uint8), 1)
        with pytest.raises(ValueError, match="widths differ"):
            fn(np.zeros((2, 32), np.int8), np.zeros((5, 64), np.int8), 1)
        with pytest.raises(ValueError, match="1024"):
            fn(np.zeros((2, 1056), np.int8), np.zeros((5, 1056), np.int8), 1)


def test_no_cpu_path(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.QstError, match="no CPU path"):
        quantization.quantize_embeddings(np.zeros((2, 8), np.float32), "ubinary")
    with pytest.raises(_lib.QstError, match="no CPU path"):
        util.hamming_topk(np.zeros((2, 8), np.uint8), np.zeros((5, 8), np.uint8), 1)


def test_dropin_exports_the_module():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sentence_transformers as st; from sentence_transformers.quantization import quantize_embeddings, "
            "semantic_search_quantized; assert st.quantization.quantize_embeddings is quantize_embeddings; "
            "from sentence_transformers.util import hamming_topk, int8_topk")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, "dropin"), root]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
