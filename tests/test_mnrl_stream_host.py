"""CPU: the host side of qst_mnrl_stream_loss (csrc/mnrl_stream.hip) and of the cached in-batch-negatives losses -- the
exported symbols, the argument checks (made before any launch, so they hold without a device), a workspace that is linear
in B + N, the shape qst_mnrl_loss gives up on, the mini-batch slicing of collated features, and the constructor surface.
No kernel runs here."""
import ctypes as C
import inspect
import os
import sys

import pytest
import torch
from torch import nn

import quadruplet_sentence_transformer_amd  # noqa: F401
from quadruplet_sentence_transformer_amd import _lib, st_losses as S, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = (S.CachedMultipleNegativesRankingLoss, S.CachedMultipleNegativesSymmetricRankingLoss)


def test_library_version_and_new_symbols():
    lib = _lib.load()
    assert lib.qst_version() >= 118
    for name, nargs in (("qst_mnrl_stream_workspace_bytes", 4), ("qst_mnrl_stream_loss", 16)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SIGNATURES["qst_mnrl_stream_workspace_bytes"][0] is C.c_size_t
    with open(os.path.join(ROOT, "include", "qst.h")) as f:
        header = f.read()
    assert "qst_mnrl_stream_workspace_bytes(int B, int N, int D, int strip_rows)" in header
    assert "int qst_mnrl_stream_loss(" in header


def test_bad_arguments_are_refused_without_a_device():
    """Every QST_ERR_BAD_ARG of qst_mnrl_loss, a strip_rows that is neither 0 nor a positive multiple of 64 and a workspace
    that is too small come back before anything is launched: host memory stands in for the device pointers, and must be left
    as it was."""
    lib = _lib.load()
    B, N, D = 4, 6, 8
    nbytes = lib.qst_mnrl_stream_workspace_bytes(B, N, D, 64)
    assert nbytes > 0 and nbytes == lib.qst_mnrl_stream_workspace_bytes(B, N, D, 0)
    a, c = (C.c_float * (B * D))(), (C.c_float * (N * D))()
    ga, gc = (C.c_float * (B * D))(), (C.c_float * (N * D))()
    out = (C.c_float * 1)(7.0)
    ws = (C.c_char * nbytes)()
    for buf in (ga, gc):
        for i in range(len(buf)):
            buf[i] = -3.0

    def call(a=a, c=c, B=B, N=N, D=D, sim=S.SCORE_COS, scale=20.0, symmetric=0, strip=64, out=out, ga=ga, gc=gc, ws=ws,
             nb=nbytes):
        p = lambda x: None if x is None else C.cast(x, C.c_void_p)  # noqa: E731
        return lib.qst_mnrl_stream_loss(p(a), p(c), B, N, D, sim, scale, symmetric, strip, p(out), None, p(ga), p(gc), p(ws),
                                        nb, None)

    bad = [dict(B=0), dict(B=-1), dict(N=B - 1), dict(D=0), dict(a=None), dict(c=None), dict(out=None), dict(ws=None),
           dict(nb=nbytes - 1), dict(nb=0), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")),
           dict(scale=float("nan")), dict(ga=None), dict(gc=None), dict(sim=2), dict(sim=-1), dict(symmetric=2),
           dict(strip=-64), dict(strip=1), dict(strip=63), dict(strip=65), dict(strip=96), dict(strip=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert out[0] == 7.0 and all(v == -3.0 for v in ga) and all(v == -3.0 for v in gc)
    assert all(b == b"\x00" for b in ws)
    for strip in (-64, 1, 63, 65, 96):
        assert lib.qst_mnrl_stream_workspace_bytes(B, N, D, strip) == 0
    assert lib.qst_mnrl_stream_workspace_bytes(0, 4, 8, 0) == 0 and lib.qst_mnrl_stream_workspace_bytes(4, 3, 8, 0) == 0
    assert lib.qst_mnrl_stream_workspace_bytes(4, 6, 0, 0) == 0


def test_workspace_is_linear_in_b_plus_n():
    """Doubling B and N at a fixed strip doubles the workspace, give or take the fixed part: a B x N term would give 4 x."""
    lib = _lib.load()
    sizes = [lib.qst_mnrl_stream_workspace_bytes(n, n, 64, 64) for n in (2048, 4096, 8192)]
    assert sizes[0] >= 64 * 2048 * 4                                    # the strip itself
    for small, big in zip(sizes, sizes[1:]):
        assert 0 < big <= 2.5 * small, sizes
    # the library's own strip stays below 64 MiB plus the linear arrays
    assert lib.qst_mnrl_stream_workspace_bytes(65536, 65536, 768, 0) < (64 << 20) + (32 << 20)


def test_a_shape_past_the_old_limit_has_a_workspace():
    lib = _lib.load()
    B = N = 46344                                                        # B * ldS = 2^31 + 22,800: qst_mnrl_loss refuses it
    assert B * N > 2 ** 31 - 1
    assert lib.qst_mnrl_stream_workspace_bytes(B, N, 8, 0) > 0
    assert lib.qst_mnrl_stream_workspace_bytes(B, N, 8, 0) < 80 << 20
    # the old entry's call gives up on it before any launch
    a = (C.c_float * 4)()
    p = C.cast(a, C.c_void_p)
    assert lib.qst_mnrl_loss(p, p, B, N, 8, S.SCORE_DOT, 2.0, 0, p, None, None, None, p, 2 ** 40, None) == -2


def test_mini_batch_bounds():
    assert S.mini_batch_bounds(16, 4) == [(0, 4), (4, 8), (8, 12), (12, 16)]
    assert S.mini_batch_bounds(16, 5) == [(0, 5), (5, 10), (10, 15), (15, 16)]           # ragged last mini-batch
    assert S.mini_batch_bounds(16, 16) == [(0, 16)] and S.mini_batch_bounds(16, 64) == [(0, 16)]
    assert S.mini_batch_bounds(3, 1) == [(0, 1), (1, 2), (2, 3)]
    for bad in (0, -1):
        with pytest.raises(ValueError):
            S.mini_batch_bounds(16, bad)
        for cls in BOTH:
            with pytest.raises(ValueError):
                cls(nn.Identity(), mini_batch_size=bad)


@pytest.mark.parametrize("mini", [1, 4, 5, 16, 64])
def test_slicing_collated_features_covers_every_row_once(mini):
    B = 16
    cols = [{"input_ids": torch.arange(B * L).reshape(B, L), "attention_mask": torch.ones(B, L, dtype=torch.long),
             "token_type_ids": torch.zeros(B, L, dtype=torch.long), "note": "kept"} for L in (7, 9, 5)]
    bounds = S.mini_batch_bounds(B, mini)
    assert len(bounds) == -(-B // min(mini, B)) and bounds[0][0] == 0 and bounds[-1][1] == B
    pieces = [S.slice_features(cols, lo, hi) for lo, hi in bounds]
    for j, col in enumerate(cols):
        for key in ("input_ids", "attention_mask", "token_type_ids"):
            assert torch.equal(torch.cat([p[j][key] for p in pieces], 0), col[key])
        assert all(p[j]["note"] == "kept" and p[j]["input_ids"].shape[0] == hi - lo for p, (lo, hi) in zip(pieces, bounds))
    assert all(len(p) == 3 for p in pieces)
    assert cols[0]["input_ids"].shape == (B, 7)                           # the batch itself is left as it was


def test_constructor_surface_follows_sentence_transformers():
    for cls in BOTH:
        d = {k: p.default for k, p in inspect.signature(cls.__init__).parameters.items() if k not in ("self", "model")}
        assert d == {"scale": 20.0, "similarity_fct": util.cos_sim, "mini_batch_size": 32, "show_progress_bar": False,
                     "fused": True}
        assert list(inspect.signature(cls.__init__).parameters)[:6] == ["self", "model", "scale", "similarity_fct",
                                                                        "mini_batch_size", "show_progress_bar"]
        assert cls(nn.Identity()).get_config_dict() == {"scale": 20.0, "similarity_fct": "cos_sim"}
        assert cls(nn.Identity(), similarity_fct=util.dot_score)._kernel_sim() == "dot"
        assert issubclass(cls, S.MultipleNegativesRankingLoss) and cls.reduction == "mean" and cls._replays_mini_batches
    assert S.CachedMultipleNegativesRankingLoss._symmetric is False
    assert S.CachedMultipleNegativesSymmetricRankingLoss._symmetric is True
    assert not getattr(S.MultipleNegativesRankingLoss, "_replays_mini_batches", False)


def test_matryoshka_refuses_the_cached_losses():
    for cls in BOTH:
        with pytest.raises(ValueError, match="Cached"):
            S.MatryoshkaLoss(nn.Identity(), cls(nn.Identity()), [8, 4])
    S.MatryoshkaLoss(nn.Identity(), S.MultipleNegativesRankingLoss(nn.Identity()), [8, 4])       # the plain one still wraps


def test_cpu_tensors_and_bad_arguments_are_refused_by_the_functional_form():
    a, c = torch.randn(4, 8), torch.randn(6, 8)
    with pytest.raises(_lib.QstError):
        S.multiple_negatives_ranking_loss_stream(a, c)
    with pytest.raises(ValueError):
        S.multiple_negatives_ranking_loss_stream(a, c[:3])
    with pytest.raises(ValueError):
        S.multiple_negatives_ranking_loss_stream(a, c, strip_rows=32)
    with pytest.raises(ValueError):
        S.multiple_negatives_ranking_loss_stream(a, c, sim="euclid")


def test_dropin_exports_the_cached_losses():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]
        from sentence_transformers import losses
        assert losses.CachedMultipleNegativesRankingLoss is S.CachedMultipleNegativesRankingLoss
        assert losses.CachedMultipleNegativesSymmetricRankingLoss is S.CachedMultipleNegativesSymmetricRankingLoss
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]
