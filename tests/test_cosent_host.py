"""CPU: the host side of CoSENTLoss and AnglELoss -- the binding and the argument checks of qst_cosent_loss (made before any
launch, so they hold without a device), the drop-in exports, util.pairwise_angle_sim against both forms of the yardstick,
the yardstick's own two forms of the loss, the conditions on the test data, and the classes' constructors. No kernel runs
here."""
import ctypes as C
import inspect
import math
import os
import sys

import pytest
import torch
from torch import nn

import quadruplet_sentence_transformer_amd  # noqa: F401
import cosent_helpers as CH
from quadruplet_sentence_transformer_amd import _lib, st_losses as S, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_version_and_new_symbols():
    lib = _lib.load()
    assert lib.qst_version() >= 117
    for name, nargs in (("qst_cosent_workspace_bytes", 2), ("qst_cosent_loss", 15)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SIGNATURES["qst_cosent_workspace_bytes"] == (C.c_size_t, [C.c_int, C.c_int])
    res, args = _lib.SIGNATURES["qst_cosent_loss"]
    assert res is C.c_int and args[3:7] == [C.c_int, C.c_int, C.c_int, C.c_float] and args[13] is C.c_size_t
    header = open(os.path.join(ROOT, "include", "qst.h")).read()
    assert "qst_cosent_loss(" in header and "qst_cosent_workspace_bytes(" in header
    assert "QST_PAIRSIM_COS = 0, QST_PAIRSIM_ANGLE = 1" in header
    assert (S.PAIRSIM_COS, S.PAIRSIM_ANGLE) == (0, 1)


def test_workspace_is_per_row_scalars_only():
    q = _lib.load().qst_cosent_workspace_bytes
    for B in (1, 5, 64, 1030, 4096, 1 << 20):
        assert 4 * B <= q(B, 768) < 64 * B + 64 and q(B, 768) % 16 == 0
        assert q(B, 2) == q(B, 768) == q(B, 5120)           # no row is staged: D does not enter
    assert q(4096, 768) < 64 * 4096
    for bad in [(0, 8), (-1, 8), (8, 0), (8, -1)]:
        assert q(*bad) == 0, bad


def test_bad_arguments_are_refused_without_a_device():
    """Every QST_ERR_BAD_ARG of qst_cosent_loss comes back before anything is launched: host memory stands in for the device
    pointers, and must be left as it was."""
    lib = _lib.load()
    B, D = 4, 6
    nbytes = lib.qst_cosent_workspace_bytes(B, D)
    assert nbytes > 0
    u, v, y = (C.c_float * (B * D))(), (C.c_float * (B * D))(), (C.c_float * B)()
    gu, gv = (C.c_float * (B * D))(), (C.c_float * (B * D))()
    out, scores = (C.c_float * 1)(7.0), (C.c_float * B)(7.0, 7.0, 7.0, 7.0)
    ws = (C.c_char * (nbytes + 32))()
    base = (-C.addressof(ws)) % 16                          # the first 16-byte boundary inside ws
    for buf in (gu, gv):
        for i in range(len(buf)):
            buf[i] = -3.0

    def call(u=u, v=v, y=y, B=B, D=D, sim=S.PAIRSIM_ANGLE, scale=20.0, out=out, gu=gu, gv=gv, ws=ws, nb=nbytes, ws_offset=0):
        p = lambda x: None if x is None else C.cast(x, C.c_void_p)  # noqa: E731
        wsp = None if ws is None else C.c_void_p(C.addressof(ws) + base + ws_offset)
        return lib.qst_cosent_loss(p(u), p(v), p(y), B, D, sim, scale, p(out), p(scores), None, p(gu), p(gv), wsp, nb, None)

    bad = [dict(B=0), dict(B=-1), dict(D=0), dict(D=-1), dict(D=5),
           dict(u=None), dict(v=None), dict(y=None), dict(out=None), dict(ws=None),
           dict(nb=nbytes - 1), dict(nb=0), dict(ws_offset=1), dict(ws_offset=4), dict(ws_offset=8),
           dict(sim=2), dict(sim=-1), dict(sim=7),
           dict(scale=0.0), dict(scale=-1.0), dict(scale=math.inf), dict(scale=math.nan),
           dict(gu=None), dict(gv=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert out[0] == 7.0 and all(s == 7.0 for s in scores)
    assert all(g == -3.0 for g in gu) and all(g == -3.0 for g in gv)
    assert all(b == b"\x00" for b in ws)
    # B * D past 2^31 - 1: refused as unsupported, the workspace being large enough for that B
    big_b, big_d = 4, 1 << 30
    assert call(B=big_b, D=big_d, nb=lib.qst_cosent_workspace_bytes(big_b, big_d)) == -2


def test_dropin_exports():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    gone = lambda: [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]  # noqa: E731
    for k in gone():
        del sys.modules[k]
    try:
        from sentence_transformers import losses, util as st_util
        from sentence_transformers.losses import AnglELoss, CoSENTLoss
        assert losses.CoSENTLoss is CoSENTLoss is S.CoSENTLoss and losses.AnglELoss is AnglELoss is S.AnglELoss
        assert st_util.pairwise_angle_sim is util.pairwise_angle_sim
        assert st_util.pairwise_cos_sim is util.pairwise_cos_sim            # the identities the classes look for
        assert losses.CosineSimilarityLoss is S.CosineSimilarityLoss        # what was there still is
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for k in gone():
            del sys.modules[k]


@pytest.mark.parametrize("B,D", [(B, D) for B, D in CH.SHAPES if D % 2 == 0])
def test_pairwise_angle_sim_equals_the_chunk_form_and_the_closed_form(B, D):
    u, v, _ = CH.case(B, D, "graded")
    got, chunk, closed = [], [], []
    for fn, into in ((util.pairwise_angle_sim, got), (CH.angle_sim_ref, chunk), (CH.angle_sim_closed, closed)):
        x, y = u.double().requires_grad_(True), v.double().requires_grad_(True)
        s = fn(x, y)
        assert s.shape == (B,) and s.dtype == torch.float64
        (s * torch.linspace(0.5, 1.5, B, dtype=torch.float64)).sum().backward()
        into.extend([s.detach(), x.grad, y.grad])
    for g, a, b in zip(got, chunk, closed):
        torch.testing.assert_close(g, a, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(g, b, rtol=1e-10, atol=1e-12)
    assert (got[0] >= 0).all() and (got[0] <= math.sqrt(2) + 1e-12).all()


def test_pairwise_angle_sim_refuses_an_odd_width_and_keeps_upstreams_nan():
    with pytest.raises(ValueError, match="7"):
        util.pairwise_angle_sim(torch.randn(3, 7), torch.randn(3, 7))
    with pytest.raises(ValueError):
        util.pairwise_angle_sim(torch.randn(3, 8), torch.randn(4, 8))
    x, y = torch.randn(3, 8), torch.randn(3, 8)
    y[1] = 0
    s = util.pairwise_angle_sim(x, y)
    assert torch.isnan(s[1]) and torch.isfinite(s[[0, 2]]).all()


@pytest.mark.parametrize("B,D,sim", CH.cases(), ids=lambda x: str(x))
def test_the_test_data_and_the_two_forms_of_the_loss(B, D, sim):
    """The conditions on every case the GPU test compares, and the yardstick's loss with the other pairs left out instead of
    pushed down by 1e12."""
    for kind in CH.LABEL_SETS:
        u, v, y, loss, scores, gu, gv = CH.reference(B, D, sim, kind)
        CH.assert_conditions(B, sim, loss, scores, gu, gv)
        assert torch.isfinite(loss) and torch.isfinite(gu).all() and torch.isfinite(gv).all()
        left_out = CH.cosent_excluded(scores, y.double())
        assert abs(left_out.item() - loss.item()) <= 1e-12 * (1 + abs(loss.item()))
        # st_losses' torch composition (what a foreign similarity_fct goes through) is the same formula
        assert abs(S.cosent_loss_torch(scores, y.double()).item() - loss.item()) <= 1e-12 * (1 + abs(loss.item()))
        if B == 1:
            assert loss.item() == 0.0 and not gu.any() and not gv.any()


def test_the_masked_terms_are_exact_zeros_in_fp32():
    u, v, y = CH.case(64, 384, "ties")
    s = CH.cos_sim_ref(u, v)
    a, b = CH.cosent_ref(s, y), CH.cosent_excluded(s, y)
    assert a.dtype == torch.float32 and abs(a.item() - b.item()) <= 1e-6 * (1 + abs(b.item()))
    # no pair at all: exactly 0, and NaN labels order nothing
    assert CH.cosent_ref(s, torch.full((64,), 0.5)).item() == 0.0
    assert CH.cosent_ref(s, torch.full((64,), float("nan"))).item() == 0.0


class Wide(nn.Module):
    """A stand-in that returns fixed embeddings of a given width."""

    def __init__(self, width):
        super().__init__()
        self.width = width

    def get_sentence_embedding_dimension(self):
        return self.width

    def forward(self, feats):
        return {"sentence_embedding": feats["emb"]}


def test_constructors_and_config_dicts_follow_sentence_transformers():
    params = inspect.signature(S.CoSENTLoss.__init__).parameters
    assert list(params) == ["self", "model", "scale", "similarity_fct", "fused"]
    assert params["scale"].default == 20.0 and params["similarity_fct"].default is util.pairwise_cos_sim
    params = inspect.signature(S.AnglELoss.__init__).parameters
    assert list(params)[:3] == ["self", "model", "scale"] and params["scale"].default == 20.0
    assert "similarity_fct" not in params
    m = Wide(64)
    lm = S.CoSENTLoss(m)
    assert isinstance(lm, S._TupleLoss) and lm.model is m and lm.reduction == "mean" and lm._kernel_sim() == "cos"
    assert lm.get_config_dict() == {"scale": 20.0, "similarity_fct": "pairwise_cos_sim"}
    assert list(inspect.signature(lm.forward).parameters)[:2] == ["sentence_features", "labels"]
    la = S.AnglELoss(m, scale=10.0)
    assert isinstance(la, S.CoSENTLoss) and la.similarity_fct is util.pairwise_angle_sim and la._kernel_sim() == "angle"
    assert la.get_config_dict() == {"scale": 10.0, "similarity_fct": "pairwise_angle_sim"} and la.reduction == "mean"
    assert S.CoSENTLoss(m, similarity_fct=util.pairwise_angle_sim)._kernel_sim() == "angle"

    def mine(a, b):
        return (a * b).sum(1)

    lf = S.CoSENTLoss(m, scale=5.0, similarity_fct=mine)
    assert lf._kernel_sim() is None and lf.get_config_dict() == {"scale": 5.0, "similarity_fct": "mine"}
    # both go inside MatryoshkaLoss, which keeps their reduction
    assert S.MatryoshkaLoss(m, la, [64, 32]).reduction == "mean"
    assert not S.MatryoshkaLoss(m, lm, [64, 32])._one_call(2)


def test_a_foreign_similarity_fct_runs_in_torch_on_cpu_tensors():
    """The torch path needs no device: the stand-in's embeddings, a callable of the user's, upstream's composition."""
    u, v, y = CH.case(7, 34, "graded")
    feats = [{"emb": u.double().requires_grad_(True)}, {"emb": v.double().requires_grad_(True)}]
    for sim in CH.SIMS:
        lm = S.CoSENTLoss(Wide(34), similarity_fct=lambda a, b: CH.SIM_REF[sim](a, b), fused=False)
        loss = lm(feats, y.view(-1, 1))
        want = CH.reference_of(u, v, y, sim)[0]
        assert abs(loss.item() - want.item()) <= 1e-12 * (1 + want.item())


def test_odd_width_and_cpu_tensors_are_refused():
    m = Wide(7)
    feats = [{"emb": torch.randn(4, 7)}, {"emb": torch.randn(4, 7)}]
    with pytest.raises(ValueError, match="7"):
        S.AnglELoss(m, fused=False)(feats, torch.rand(4))
    with pytest.raises(ValueError, match="7"):
        S.cosent_loss(torch.randn(4, 7), torch.randn(4, 7), torch.rand(4), sim="angle")
    u, v, y = torch.randn(4, 8), torch.randn(4, 8), torch.rand(4)
    with pytest.raises(_lib.QstError, match="HIP device only"):
        S.cosent_loss(u, v, y)
    with pytest.raises(_lib.QstError, match="HIP device only"):
        S.cosent_loss_raw(u, v, y, "cos", 20.0)
    with pytest.raises(_lib.QstError, match="HIP device only"):
        S.CoSENTLoss(Wide(8), fused=False)([{"emb": u}, {"emb": v}], y)
    for kw in (dict(sim="dot"), dict(scale=0.0), dict(scale=float("inf")), dict(scale=float("nan"))):
        with pytest.raises(ValueError):
            S.cosent_loss(u, v, y, **kw)
    with pytest.raises(ValueError):
        S.cosent_loss(u, v[:3], y)
    with pytest.raises(ValueError):
        S.cosent_loss(u, v, y[:3])
    with pytest.raises(ValueError):
        S.CoSENTLoss(Wide(8), fused=False)([{"emb": u}], y)                 # two text columns
