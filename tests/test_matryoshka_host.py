"""CPU: the host side of MatryoshkaLoss and truncate_dim -- constructor refusals, the config dict, the drop-in export, the
binding and the argument checks of qst_mnrl_nested_loss (made before any launch, so they hold without a device), the
refusal of CPU tensors, and the truncate_dim bookkeeping that needs no device. No kernel runs here."""
import ctypes as C
import inspect
import math
import os
import sys

import pytest
import torch
from torch import nn

import quadruplet_sentence_transformer_amd  # noqa: F401
import matryoshka_helpers as MH
from quadruplet_sentence_transformer_amd import _lib, st_losses as S, util
from quadruplet_sentence_transformer_amd.sentence_transformer import SentenceTransformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Wide(nn.Module):
    """A stand-in that knows its embedding width."""

    def __init__(self, width):
        super().__init__()
        self.width = width

    def get_sentence_embedding_dimension(self):
        return self.width


def test_constructor_follows_sentence_transformers():
    params = inspect.signature(S.MatryoshkaLoss.__init__).parameters
    assert list(params) == ["self", "model", "loss", "matryoshka_dims", "matryoshka_weights", "n_dims_per_step", "fused_dims"]
    assert params["matryoshka_weights"].default is None and params["n_dims_per_step"].default == -1
    assert params["fused_dims"].default in (True, False)
    m = Wide(64)
    lm = S.MatryoshkaLoss(m, S.MultipleNegativesRankingLoss(m), [64, 32, 16])
    assert lm.matryoshka_dims == [64, 32, 16] and lm.matryoshka_weights == [1.0, 1.0, 1.0] and lm.n_dims_per_step == -1
    assert lm.model is m and lm.reduction == "mean"
    assert list(inspect.signature(lm.forward).parameters)[:2] == ["sentence_features", "labels"]
    # the reduction is the base loss's
    assert S.MatryoshkaLoss(m, S.ContrastiveLoss(m, size_average=False), [8]).reduction == "sum"
    assert S.MatryoshkaLoss(m, S.OnlineContrastiveLoss(m), [8]).reduction == "sum"
    assert S.MatryoshkaLoss(m, S.CosineSimilarityLoss(m, loss_fct=nn.MSELoss(reduction="none")), [8]).reduction == "none"
    # a stand-in that cannot say its width is taken at its word until the forward
    assert S.MatryoshkaLoss(nn.Identity(), S.TripletLoss(nn.Identity()), [4096]).matryoshka_dims == [4096]


def test_constructor_refusals_name_their_cause():
    m = Wide(64)
    base = S.MultipleNegativesRankingLoss(m)
    with pytest.raises(ValueError, match="larger than the model's embedding dimension 64"):
        S.MatryoshkaLoss(m, base, [64, 65])
    with pytest.raises(ValueError, match="empty"):
        S.MatryoshkaLoss(m, base, [])
    with pytest.raises(ValueError, match="repeats a width"):
        S.MatryoshkaLoss(m, base, [64, 32, 64])
    with pytest.raises(ValueError, match="positive"):
        S.MatryoshkaLoss(m, base, [64, 0])
    with pytest.raises(ValueError, match="2 entries for 3 matryoshka_dims"):
        S.MatryoshkaLoss(m, base, [64, 32, 16], [1.0, 0.5])
    with pytest.raises(TypeError, match="MSELoss does not derive from _TupleLoss"):
        S.MatryoshkaLoss(m, nn.MSELoss(), [64])
    with pytest.raises(ValueError, match="SoftmaxLoss: its classifier has a fixed input width"):
        S.MatryoshkaLoss(m, S.SoftmaxLoss(m, 64, 3), [64, 32])
    with pytest.raises(ValueError, match="MSELoss: the teacher's vectors have the full width"):
        S.MatryoshkaLoss(m, S.MSELoss(m), [64, 32])


def test_config_dict():
    m = Wide(64)
    lm = S.MatryoshkaLoss(m, S.MultipleNegativesSymmetricRankingLoss(m), [64, 16], [1.0, 0.25], n_dims_per_step=1)
    assert lm.get_config_dict() == {"loss": "MultipleNegativesSymmetricRankingLoss", "matryoshka_dims": [64, 16],
                                    "matryoshka_weights": [1.0, 0.25], "n_dims_per_step": 1}


def test_which_base_losses_take_the_single_call():
    m = Wide(64)
    for cls in (S.MultipleNegativesRankingLoss, S.MultipleNegativesSymmetricRankingLoss):
        for fct in (util.cos_sim, util.dot_score):
            assert S.MatryoshkaLoss(m, cls(m, similarity_fct=fct), [64, 8])._one_call(2)
        assert not S.MatryoshkaLoss(m, cls(m, similarity_fct=lambda a, b: util.cos_sim(a, b)), [64, 8])._one_call(2)
        assert not S.MatryoshkaLoss(m, cls(m), [64, 8], fused_dims=False)._one_call(2)
        assert S.MatryoshkaLoss(m, cls(m), [64, 8])._one_call(8) and not S.MatryoshkaLoss(m, cls(m), [64, 8])._one_call(9)
    assert not S.MatryoshkaLoss(m, S.TripletLoss(m), [64, 8])._one_call(2)
    assert S.NESTED_MAX_DIMS == 8


def test_dropin_exports_the_class():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    gone = lambda: [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]  # noqa: E731
    for k in gone():
        del sys.modules[k]
    try:
        from sentence_transformers import losses
        from sentence_transformers.losses import MatryoshkaLoss
        assert losses.MatryoshkaLoss is MatryoshkaLoss is S.MatryoshkaLoss
        assert losses.MultipleNegativesRankingLoss is S.MultipleNegativesRankingLoss      # what was there still is
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for k in gone():
            del sys.modules[k]


def test_library_version_and_new_symbols():
    lib = _lib.load()
    assert lib.qst_version() >= 116
    for name, nargs in (("qst_mnrl_nested_workspace_bytes", 4), ("qst_mnrl_nested_loss", 18)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SIGNATURES["qst_mnrl_nested_workspace_bytes"][0] is C.c_size_t
    header = open(os.path.join(ROOT, "include", "qst.h")).read()
    assert "qst_mnrl_nested_loss(" in header and "qst_mnrl_nested_workspace_bytes(" in header


def test_workspace_query():
    lib = _lib.load()
    q = lib.qst_mnrl_nested_workspace_bytes
    for (B, N, D, K) in [(5, 10, 7, 1), (5, 10, 7, 8), (64, 128, 384, 5), (512, 1024, 768, 8)]:
        ldS = (N + 3) // 4 * 4
        assert q(B, N, D, K) >= K * B * ldS * 4
        assert q(B, N, D, K) % 4 == 0
    assert q(5, 10, 7, 8) > q(5, 10, 7, 1)
    for bad in [(0, 4, 8, 2), (4, 3, 8, 2), (4, 4, 0, 2), (4, 4, 8, 0), (4, 4, 8, 9), (-1, 4, 8, 2)]:
        assert q(*bad) == 0, bad


def test_bad_arguments_are_refused_without_a_device():
    """Every QST_ERR_BAD_ARG of qst_mnrl_nested_loss comes back before anything is launched: host memory stands in for the
    device pointers, and must be left as it was."""
    lib = _lib.load()
    B, N, D, K = 4, 6, 8, 3
    nbytes = lib.qst_mnrl_nested_workspace_bytes(B, N, D, K)
    assert nbytes > 0
    a, c = (C.c_float * (B * D))(), (C.c_float * (N * D))()
    ga, gc = (C.c_float * (B * D))(), (C.c_float * (N * D))()
    out, terms = (C.c_float * 1)(7.0), (C.c_float * K)(7.0, 7.0, 7.0)
    ws = (C.c_char * (nbytes + 8))()
    for buf in (ga, gc):
        for i in range(len(buf)):
            buf[i] = -3.0

    def call(a=a, c=c, B=B, N=N, D=D, dims=(8, 4, 2), weights=(1.0, 0.5, 0.25), K=K, scale=20.0, symmetric=0, out=out,
             terms=terms, ga=ga, gc=gc, ws=ws, nb=nbytes, ws_offset=0):
        p = lambda x: None if x is None else C.cast(x, C.c_void_p)  # noqa: E731
        hd = None if dims is None else (C.c_int32 * len(dims))(*dims)
        hw = None if weights is None else (C.c_float * len(weights))(*weights)
        wsp = None if ws is None else C.c_void_p(C.addressof(ws) + ws_offset)
        return lib.qst_mnrl_nested_loss(p(a), p(c), B, N, D, hd, hw, K, scale, symmetric, p(out), p(terms), None, p(ga),
                                        p(gc), wsp, nb, None)

    nine = tuple(range(1, 10))
    bad = [dict(K=0), dict(K=-1), dict(K=9, dims=nine[:8] + (8,), weights=(1.0,) * 9),
           dict(dims=(8, 0, 2)), dict(dims=(9, 4, 2)), dict(dims=(8, -4, 2)), dict(dims=(8, 4, 4)), dict(dims=(2, 4, 2)),
           dict(weights=(1.0, math.inf, 0.25)), dict(weights=(1.0, -math.inf, 0.25)), dict(weights=(math.nan, 0.5, 0.25)),
           dict(dims=None), dict(weights=None),
           dict(nb=nbytes - 1), dict(nb=0), dict(ws=None), dict(ws_offset=1), dict(ws_offset=2),
           dict(scale=0.0), dict(scale=-1.0), dict(scale=math.inf), dict(scale=math.nan), dict(symmetric=2),
           dict(symmetric=-1), dict(ga=None), dict(gc=None),
           dict(B=0), dict(B=-1), dict(N=B - 1), dict(D=0), dict(a=None), dict(c=None), dict(out=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert out[0] == 7.0 and all(v == 7.0 for v in terms)
    assert all(v == -3.0 for v in ga) and all(v == -3.0 for v in gc)
    assert all(b == b"\x00" for b in ws)
    # index ranges past 2^31 - 1: refused as unsupported, before the workspace is looked at more closely than its size
    big_b, big_n = 40000, 60000
    need = lib.qst_mnrl_nested_workspace_bytes(big_b, big_n, 8, 1)
    assert need >= big_b * big_n * 4
    assert call(B=big_b, N=big_n, dims=(8,), weights=(1.0,), K=1, nb=need) == -2


def test_cpu_tensors_and_bad_shapes_are_refused():
    a, c = torch.randn(4, 8), torch.randn(6, 8)
    with pytest.raises(_lib.QstError, match="HIP device only"):
        S.matryoshka_mnrl_loss(a, c, [8, 4])
    with pytest.raises(_lib.QstError, match="HIP device only"):
        S.mnrl_nested_loss_raw(a, c, [8, 4], [1.0, 1.0], 20.0, False)
    for kw in (dict(dims=[8, 9]), dict(dims=[8, 0]), dict(dims=[]), dict(dims=[4, 4]), dict(dims=list(range(1, 10))),
               dict(dims=[8, 4], weights=[1.0]), dict(dims=[8], scale=0.0)):
        with pytest.raises(ValueError):
            S.matryoshka_mnrl_loss(a, c, kw["dims"], kw.get("weights"), kw.get("scale", 20.0))
    with pytest.raises(ValueError):
        S.matryoshka_mnrl_loss(a, torch.randn(6, 9), [8])               # another D
    with pytest.raises(ValueError):
        S.matryoshka_mnrl_loss(a, c[:3], [8])                           # N < B
    m = Wide(8)
    with pytest.raises(ValueError, match="2 or more text columns"):
        S.MatryoshkaLoss(m, S.MultipleNegativesRankingLoss(m), [8, 4])([{"input_ids": torch.zeros(2, 3, dtype=torch.long)}], None)


def test_the_per_width_path_on_a_stand_in_model():
    """No kernel: a base loss with a foreign similarity function over a stand-in encoder runs entirely in torch, which
    shows the width handed to the base loss, the weighting, and that `_embed` comes back."""

    class Table(nn.Module):
        def forward(self, feats):
            return {"sentence_embedding": feats["emb"]}

    torch.manual_seed(3)
    u, v = torch.randn(5, 12, dtype=torch.float64), torch.randn(5, 12, dtype=torch.float64)
    m = Table()
    seen = []

    def foreign(x, y):
        seen.append((x.shape[1], float(x.norm(dim=1).mean())))
        return x @ y.t()

    base = S.MultipleNegativesRankingLoss(m, similarity_fct=foreign, fused=False)
    lm = S.MatryoshkaLoss(m, base, [12, 5, 2], [1.0, 0.5, 0.25])
    got = lm([{"emb": u}, {"emb": v}], None)
    want, _ = MH.matryoshka_ref(u, v, [12, 5, 2], [1.0, 0.5, 0.25], False)
    assert [s[0] for s in seen] == [12, 5, 2] and all(abs(s[1] - 1.0) < 1e-12 for s in seen)
    assert abs(got.item() - want.item()) < 1e-12
    assert "_embed" not in base.__dict__
    with pytest.raises(ValueError, match="larger than the embedding width 12"):
        S.MatryoshkaLoss(m, base, [13])([{"emb": u}, {"emb": v}], None)
    assert "_embed" not in base.__dict__


def test_truncate_dim_bookkeeping_without_a_device():
    params = inspect.signature(SentenceTransformer.__init__).parameters
    assert "truncate_dim" in params and params["truncate_dim"].default is None
    enc = inspect.signature(SentenceTransformer.encode).parameters
    assert "truncate_dim" in enc and enc["truncate_dim"].default is None
    assert "not persisted" in SentenceTransformer.save.__doc__

    class Shell(SentenceTransformer):                       # the bookkeeping alone: no encoder behind it
        def __init__(self, truncate_dim=None):
            nn.Module.__init__(self)
            from quadruplet_sentence_transformer_amd.config import PRESETS
            from quadruplet_sentence_transformer_amd.sentence_transformer import _checked_truncate_dim
            self.cfg = PRESETS["tiny-bert"]
            self.truncate_dim = _checked_truncate_dim(truncate_dim)

    m = Shell()
    assert m.truncate_dim is None and m.get_sentence_embedding_dimension() == 64
    m = Shell(truncate_dim=16)
    assert m.truncate_dim == 16 and m.get_sentence_embedding_dimension() == 16
    with m.truncate_sentence_embeddings(8):
        assert m.truncate_dim == 8 and m.get_sentence_embedding_dimension() == 8
        with m.truncate_sentence_embeddings(None):
            assert m.truncate_dim is None and m.get_sentence_embedding_dimension() == 64
        with m.truncate_sentence_embeddings(1000):          # wider than the model: the full width
            assert m.get_sentence_embedding_dimension() == 64
        assert m.truncate_dim == 8
    assert m.truncate_dim == 16
    with pytest.raises(KeyError):
        with m.truncate_sentence_embeddings(4):
            raise KeyError("inside")
    assert m.truncate_dim == 16
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="positive integer or None"):
            with m.truncate_sentence_embeddings(bad):
                pass
        with pytest.raises(ValueError, match="positive integer or None"):
            Shell(truncate_dim=bad)
    assert m.truncate_dim == 16
    # MatryoshkaLoss looks at the full width of a truncated model
    assert S.MatryoshkaLoss(m, S.TripletLoss(m), [64, 16]).matryoshka_dims == [64, 16] and m.truncate_dim == 16
    with pytest.raises(ValueError, match="embedding dimension 64"):
        S.MatryoshkaLoss(m, S.TripletLoss(m), [65])


def test_helper_cases_keep_the_comparison_meaningful():
    """The non-saturation condition test_gpu_matryoshka asserts on its reference, on the smaller cases (the GPU test
    checks every case), and the shape of the case list."""
    assert len(MH.CASES) == 11 and max(len(c[3]) for c in MH.CASES) == 8
    assert all(max(dims) == D and len(set(dims)) == len(dims) for (_, _, D, dims) in MH.CASES)
    assert [c for c in MH.CASES if 1 in c[3]] == [MH.CASES[0]] and MH.CASES[0][1] == 1
    for (B, N, D, dims) in MH.CASES[:5]:
        for symmetric in (0, 1):
            for trained in (0, 1):
                _, _, loss, terms, ga, gc, term_grad = MH.reference(B, N, D, dims, symmetric, trained)
                MH.assert_not_saturated(N, terms, term_grad)
                assert abs(loss.item() - sum(w * t for w, t in zip(MH.weights_of(dims), terms.tolist()))) < 1e-12
                assert ga.shape == (B, D) and gc.shape == (N, D)
