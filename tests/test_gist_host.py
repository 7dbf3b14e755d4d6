"""CPU: what GISTEmbedLoss and CachedGISTEmbedLoss need no device for -- the library's version and symbols, the argument
checks and workspace size of qst_gist_loss (csrc/gist.hip), the conditions every test case of gist_helpers must meet, the
yardstick against a plain cross entropy, the classes' argument checks and the drop-in exports."""
import ctypes as C
import inspect
import os
import sys

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import quadruplet_sentence_transformer_amd  # noqa: F401
import gist_helpers as G
from quadruplet_sentence_transformer_amd import _lib
from quadruplet_sentence_transformer_amd import st_losses as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_version_and_new_symbols():
    lib = _lib.load()
    assert lib.qst_version() >= 119
    for name, nargs in (("qst_gist_workspace_bytes", 5), ("qst_gist_loss", 16)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SIGNATURES["qst_gist_workspace_bytes"][0] is C.c_size_t
    header = open(os.path.join(ROOT, "include", "qst.h")).read()
    assert "qst_gist_workspace_bytes(int B, int K, int D, int Dg, int strip_rows)" in header
    assert "csrc/gist.hip" in header and "gist.hip" in open(os.path.join(
        ROOT, "quadruplet-sentence-transformer_amd", "csrc", "Makefile")).read()


def test_workspace_is_zero_for_every_bad_argument():
    lib = _lib.load()
    assert lib.qst_gist_workspace_bytes(4, 2, 8, 6, 64) > 0 and lib.qst_gist_workspace_bytes(4, 2, 8, 6, 0) > 0
    for bad in ((0, 2, 8, 6, 64), (-1, 2, 8, 6, 64), (4, 1, 8, 6, 64), (4, 0, 8, 6, 64), (4, 2, 0, 6, 64), (4, 2, 8, 0, 64),
                (4, 2, 8, 6, -64), (4, 2, 8, 6, 32), (4, 2, 8, 6, 100), (2 ** 30, 2, 8, 6, 64)):
        assert lib.qst_gist_workspace_bytes(*bad) == 0, bad


def test_bad_arguments_are_refused_without_a_device():
    """Every QST_ERR_BAD_ARG comes back before anything is launched: host memory stands in for the device pointers, and must
    be left as it was."""
    lib = _lib.load()
    B, K, D, Dg = 4, 3, 8, 6
    nbytes = lib.qst_gist_workspace_bytes(B, K, D, Dg, 64)
    x, g = torch.randn(K * B, D), torch.randn(K * B, Dg)
    out, gx = torch.full((1,), -7.25), torch.full((K * B, D), -7.25)
    ws = torch.zeros(nbytes + 16, dtype=torch.uint8)
    nan, inf = float("nan"), float("inf")

    def call(x_=x.data_ptr(), g_=g.data_ptr(), B_=B, K_=K, D_=D, Dg_=Dg, t=0.05, strat=0, margin=0.0, strip=64,
             out_=out.data_ptr(), ws_=ws.data_ptr(), n=nbytes):
        return lib.qst_gist_loss(x_, g_, B_, K_, D_, Dg_, t, strat, margin, strip, out_, None, gx.data_ptr(), ws_, n, None)

    bad = [dict(B_=0), dict(K_=1), dict(D_=0), dict(Dg_=0), dict(x_=None), dict(g_=None), dict(out_=None), dict(ws_=None),
           dict(t=0.0), dict(t=-0.01), dict(t=nan), dict(t=inf), dict(margin=nan), dict(margin=inf), dict(margin=-inf),
           dict(strat=2), dict(strat=-1), dict(strip=-64), dict(strip=63), dict(strip=96), dict(n=nbytes - 1),
           dict(ws_=ws.data_ptr() + 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert out.item() == -7.25 and (gx == -7.25).all() and not ws.any()


def test_workspace_is_linear_in_b():
    """Doubling B at a fixed strip doubles the workspace, give or take the fixed part: a retained score matrix would give 4 x.
    Two strips of 64 x 3 B floats are the bulk of it."""
    lib = _lib.load()
    small, big = [lib.qst_gist_workspace_bytes(b, 2, 768, 1024, 64) for b in (4096, 8192)]
    assert small >= 2 * 64 * 3 * 4096 * 4
    assert small < big < 2.1 * small, (small, big)
    assert big < 8192 * 8192 * 4 / 8                                    # nowhere near one B x B block
    # the library's own strip keeps both strips within 64 MiB, whatever B
    assert lib.qst_gist_workspace_bytes(65536, 2, 768, 1024, 0) < (64 << 20) + 65536 * 2 * 4 * 6 + 20 * 64 * 768 * 4 * 33


@pytest.mark.parametrize("B,K,D,Dg", G.SHAPES + G.BIG_SHAPES + [(1400, 3, 24, 256)])
def test_every_case_meets_the_conditions(B, K, D, Dg):
    cols, guide_cols = G.case(B, K, D, Dg)
    for temperature in G.TEMPERATURES:
        gap, shares = G.conditions(cols, guide_cols, temperature)
    print(f"  {B}x{K}x{D}x{Dg}: min gap {gap:.2e}, masked " + " ".join(
        f"{n} {s:.1%}" for n, s in zip(G.block_names(K), shares)))


@pytest.mark.parametrize("margin_strategy,margin", G.MARGINS)
def test_the_margin_case_meets_the_conditions(margin_strategy, margin):
    cols, guide_cols = G.case(*G.MARGIN_SHAPE, G.MARGIN_SEED)
    for temperature in G.TEMPERATURES:
        G.conditions(cols, guide_cols, temperature, margin_strategy, margin)


def test_margins_change_the_masks():
    _, guide_cols = G.case(*G.MARGIN_SHAPE, G.MARGIN_SEED)
    counts = {m: sum(int(x.sum()) for x in G.gist_masks(guide_cols, *m)[0]) for m in G.MARGINS}
    assert counts[("absolute", 0.0)] == counts[("relative", 0.0)]
    assert counts[("absolute", 0.1)] > counts[("absolute", 0.0)] and counts[("relative", 0.1)] > counts[("relative", 0.0)]


def test_reference_without_masks_is_a_plain_cross_entropy():
    """A guide whose examples are orthogonal to each other (thr_i = 0.89, every other score 0 or, on the aa and pp diagonals,
    1) masks those two diagonals and nothing else: the yardstick is then F.cross_entropy over the plain concatenation without
    them."""
    B, K, D = 6, 3, 16
    cols = [c.double() for c in G.student_case(B, K, D, 3)]
    base = torch.eye(B, 12, dtype=torch.float64)
    guide_cols = [base * 2.0, base + 0.5 * base.roll(6, 1), base.roll(6, 1)]
    masks, _ = G.gist_masks(guide_cols)
    eye = torch.eye(B, dtype=torch.bool)
    assert not masks[0].any() and torch.equal(masks[1], eye) and torch.equal(masks[2], eye) and not masks[3].any()
    blocks = G.gist_blocks(cols)
    blocks[1] = blocks[1].masked_fill(eye, -torch.inf)
    blocks[2] = blocks[2].masked_fill(eye, -torch.inf)
    want = F.cross_entropy(torch.cat(blocks, 1) / 0.05, torch.arange(B))
    got = G.gist_ref(cols, guide_cols, 0.05)
    assert torch.equal(got, want)
    # ... and with a guide that finds nothing at all more similar than the positive (thr_i = 1 everywhere, no diagonal above
    # it either: a strict comparison), nothing is masked
    assert not any(m.any() for m in G.gist_masks([base, base, base])[0])


def test_constructor_surface_follows_sentence_transformers():
    d = {k: p.default for k, p in inspect.signature(S.GISTEmbedLoss.__init__).parameters.items() if k not in ("self", "model", "guide")}
    assert d == {"temperature": 0.01, "margin_strategy": "absolute", "margin": 0.0, "fused": True}
    names = list(inspect.signature(S.CachedGISTEmbedLoss.__init__).parameters)
    assert names == ["self", "model", "guide", "temperature", "mini_batch_size", "show_progress_bar", "margin_strategy", "margin"]
    d = {k: p.default for k, p in inspect.signature(S.CachedGISTEmbedLoss.__init__).parameters.items() if k in names[3:]}
    assert d == {"temperature": 0.01, "mini_batch_size": 32, "show_progress_bar": False, "margin_strategy": "absolute",
                 "margin": 0.0}
    assert S.CachedGISTEmbedLoss._replays_mini_batches is True and not getattr(S.GISTEmbedLoss, "_replays_mini_batches", False)


@pytest.mark.parametrize("cls", [S.GISTEmbedLoss, S.CachedGISTEmbedLoss])
def test_class_argument_checks(cls):
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")),
               dict(margin_strategy="ratio"), dict(margin=float("nan"))):
        with pytest.raises(ValueError):
            cls(nn.Identity(), nn.Identity(), **kw)
    with pytest.raises(TypeError, match="guide"):                       # anything but a SentenceTransformer of this package
        cls(nn.Identity(), nn.Identity())
    with pytest.raises(TypeError, match="guide"):
        cls(nn.Identity(), None)


def test_functional_form_checks_its_arguments():
    reps, guide = [torch.randn(4, 8) for _ in range(2)], [torch.randn(4, 6) for _ in range(2)]
    with pytest.raises(ValueError, match="2 or more"):
        S.gist_embed_loss(reps[:1], guide[:1])
    with pytest.raises(ValueError):
        S.gist_embed_loss(reps, guide[:1])
    with pytest.raises(ValueError):
        S.gist_embed_loss(reps, guide, temperature=0.0)
    with pytest.raises(ValueError):
        S.gist_embed_loss(reps, guide, margin_strategy="ratio")
    with pytest.raises(ValueError):
        S.gist_embed_loss(reps, guide, strip_rows=32)
    with pytest.raises(ValueError):
        S.gist_embed_loss(reps, [guide[0], guide[1][:3]])
    with pytest.raises(_lib.QstError):                                  # CPU tensors: no CPU path
        S.gist_embed_loss(reps, guide)


def test_matryoshka_refuses_the_cached_form():
    """The cached form embeds in mini-batches and replays them: the per-width losses are not part of that replay."""
    stub = S.CachedGISTEmbedLoss.__new__(S.CachedGISTEmbedLoss)
    nn.Module.__init__(stub)
    with pytest.raises(ValueError, match="Cached"):
        S.MatryoshkaLoss(nn.Identity(), stub, [8, 4])


def test_dropin_exports_the_gist_losses():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]
        from sentence_transformers import losses
        assert losses.GISTEmbedLoss is S.GISTEmbedLoss and losses.CachedGISTEmbedLoss is S.CachedGISTEmbedLoss
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]
