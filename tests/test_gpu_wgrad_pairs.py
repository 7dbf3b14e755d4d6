"""GPU: the weight gradients of two neighbouring layers in one grouped launch (qst_encoder_set_wgrad_pairs, DESIGN.md finding 48).

Switch 1 issues one launch per layer -- the path every other test file runs -- and is the reference here; switch 2 pairs
wherever a call covers two layers: (1, 0), (3, 2), (5, 4) from the bottom, the top layer of an odd depth alone. The products
are the same; what may differ is the grouping of the fp32 partial sums the launch adds into the gradient arena.

The bound of a paired run against a per-layer run, per parameter tensor T, element-wise:

    |g2 - g1|  <=  d11  +  2 * M * sqrt(M) * 2^-24 * max|g1_T|

  d11   the largest element-wise difference among three switch-1 runs of the same inputs, measured in the test itself: the
        arrival order of the fp32 atomics (two runs share every partial sum and differ in the order they are added).
  2nd   the regrouping term. An element is a sum of M products accumulated in fp32; any grouping of it is off the exact sum
        by at most (M - 1) * u * sum|x_m|, u = 2^-24, so two groupings differ by at most twice that. sum|x_m| is not
        observable from outside; it is taken as sqrt(M) * max|g_T| -- the size a sum of M terms of random sign has when the sum
        itself is max|g_T|. DESIGN.md finding 47 measured such a re-ranged launch at 4.6e-6 of the gradient norm over 3,600 to
        4,600 rows per range; the term here is 6.9e-4 * max|g_T| at M = 320, and a lost or doubled partial sum -- what a wrong
        pointer, a stale dY tensor or a race would give -- moves an element by the size of the partial sum itself.
  Measured (tiny-roberta@5, bf16, (5, 64)): d11 = 3.8e-6 at max|g| = 24.6, |g2 - g1| = 3.8e-6; over every case of this file
  the paired run never differed from the per-layer run by more than 2 x d11 (profiles/r08_ab_wgrad_pairs.txt).

Where a launch is the SAME in both settings -- the top layer of an odd depth, every launch of the staged path -- there is no
regrouping: the bound is twice d11 (three runs sample the arrival order; twice the largest of them is the allowance for a
fourth). The issue asked for the staged arenas to be equal bit for bit; two switch-1 runs of the staged path already differ
(1.8e-7 at max|g| = 1.5, tiny-mpnet@3), so what is asserted bit for bit is that the second set of dY tensors is never touched.
"""
import math
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

import encoder_arena_cases as E  # noqa: E402
from quadruplet_sentence_transformer_amd import _lib  # noqa: E402
from quadruplet_sentence_transformer_amd.config import build_layout  # noqa: E402

U = 2.0 ** -24
DEPTH_MODELS = {1: "tiny-bert@1", 2: "tiny-mpnet", 3: "tiny-roberta@3", 5: "tiny-bert@5", 6: "tiny-mpnet@6"}
SHAPE_OF = {1: E.X, 2: E.Y1, 3: E.Y2, 5: E.X, 6: E.Y1}
FILL = 0xFF


def regroup_term(M, gmax):
    return 2.0 * M * math.sqrt(M) * U * gmax


def runner(model, precision, mode, ln_fusion=None, ffn_chain=None, shape=E.X):
    r = E.Runner(model, precision, ffn_chain=ffn_chain, ln_fusion=ln_fusion)
    r.enc.set_wgrad_pairs(mode)
    r.make_windows(shapes=(shape,), pools=(E.POOL_MEAN,))
    return r


def run_filled(r, shape, fill, **kw):
    """One forward + backward with every window armed and the workspace pre-filled with `fill` bytes."""
    nb = r.sizes(shape, True, E.POOL_MEAN, True)
    for k, v in nb.items():
        r.win[k].arm(v)
    r.win["ws"].view(nb["ws"]).fill_(fill)
    res = r.run(shape, arm=False, **kw)
    assert res.rc == E.QST_OK, res.rc
    assert r.bands_written(res.nbytes) == []
    return res


@lru_cache(maxsize=None)
def grads_of(model, precision, dropout, backward, ln_fusion, ffn_chain, shape):
    """(three switch-1 gradient arenas, one switch-2 arena, the two workspace sizes), computed once per case."""
    one, ws = [], {}
    for mode in (1, 2):
        r = runner(model, precision, mode, ln_fusion, ffn_chain, shape)
        for _ in range(3 if mode == 1 else 1):
            res = run_filled(r, shape, 0, dropout=dropout, backward=backward)
            (one if mode == 1 else ws.setdefault("g2", [])).append(res.grads.cpu())
        ws[mode] = res.nbytes["ws"]
    return one, ws["g2"][0], ws[1], ws[2]


def d11_of(one):
    return max(float((one[i] - one[j]).abs().max()) for i, j in ((0, 1), (0, 2), (1, 2)))


def same_launch_bound(one):
    """Two runs of the SAME launches: twice the largest difference among the three sampled runs, and never less than two
    units in the last place of the largest gradient (three runs of a small model can agree bit for bit; a fourth need not)."""
    return 2 * max(d11_of(one), 2.0 ** -23 * float(one[0].abs().max()))


def check_pair_against_layers(cfg, shape, one, g2, what):
    segs, _ = build_layout(cfg)
    M, d11 = shape[0] * shape[1], d11_of(one)
    assert torch.isfinite(g2).all() and float(one[0].abs().max()) > 0
    worst = 0.0
    for s in segs:
        a, b = one[0][s.offset:s.offset + s.numel], g2[s.offset:s.offset + s.numel]
        d, allow = float((a - b).abs().max()), d11 + regroup_term(M, float(a.abs().max()))
        worst = max(worst, d)
        assert d <= allow, f"{what}: {s.name} differs by {d:.3e}, allowed {allow:.3e} (d11 {d11:.3e})"
    print(f"[wgrad-pairs] {what}: max|g| {float(one[0].abs().max()):.3e}  d11 {d11:.3e}  paired-vs-layer {worst:.3e}")
    return d11, worst


@pytest.mark.parametrize("precision", ["bf16", "f16"])
@pytest.mark.parametrize("dropout", [None, E.DROPOUT], ids=["nodrop", "dropout"])
@pytest.mark.parametrize("layers", [1, 2, 3, 5, 6])
def test_paired_launches_give_the_gradients_of_per_layer_launches(layers, dropout, precision):
    model, shape = DEPTH_MODELS[layers], SHAPE_OF[layers]
    cfg = E.config(model)
    assert cfg.num_layers == layers
    one, g2, ws1, ws2 = grads_of(model, precision, dropout, "one", None, None, shape)
    check_pair_against_layers(cfg, shape, one, g2, f"{model} {precision} {'dropout' if dropout else 'nodrop'}")
    if layers == 1:
        assert ws2 == ws1            # nothing to pair: no second set
    if layers in (3, 5):
        # the top layer keeps its own launch, the same launch as with switch 1: arrival order only
        segs, _ = build_layout(cfg)
        bound = same_launch_bound(one)
        top = [s for s in segs if s.name.startswith(f"layer.{layers - 1}.")]
        assert len(top) >= 8
        for s in top:
            d = float((one[0][s.offset:s.offset + s.numel] - g2[s.offset:s.offset + s.numel]).abs().max())
            assert d <= bound, f"top layer {s.name}: {d:.3e} against {bound:.3e}"


@pytest.mark.parametrize("model,ffn,ln,dropout", [("minilm-2l", 7, 1, None), ("minilm-2l@3", 7, 1, None), ("minilm-2l@3", 0, 1, E.DROPOUT),
                                                  ("minilm-2l@5", 0, 1, None), ("minilm-2l", 0, 2, E.DROPOUT), ("h768-2l", None, 1, None)])
def test_paired_launches_under_the_fused_layernorm_backward(model, ffn, ln, dropout):
    """H = 384 / 768 with the LayerNorm backward inside the dgrad launches: the QKV dgrad of layer l writes the dsb of layer
    l - 1 -- into that layer's set -- and the one-kernel feed-forward backward (ffn 7) writes du and dsb1."""
    one, g2, ws1, ws2 = grads_of(model, "bf16", dropout, "one", ln, ffn, E.X)
    check_pair_against_layers(E.config(model), E.X, one, g2, f"{model} ffn{ffn} ln{ln}")
    assert ws2 > ws1


def test_fp8_training_backward_pairs_too():
    one, g2, ws1, ws2 = grads_of("minilm-2l", "fp8", None, "one", None, None, E.Y2)
    check_pair_against_layers(E.config("minilm-2l"), E.Y2, one, g2, "minilm-2l fp8")
    assert ws2 > ws1


def second_set_bytes(cfg, shape):
    M, H, I = shape[0] * shape[1], cfg.hidden_size, cfg.intermediate_size
    up = lambda n: (n + 255) // 256 * 256      # noqa: E731
    return up(M * H * 2) + up(M * H * 2) + up(M * I * 2) + up(M * 3 * H * 2)


@pytest.mark.parametrize("model,precision", [("tiny-bert", "bf16"), ("tiny-mpnet@3", "f16"), ("tiny-roberta@5", "bf16"), ("minilm-2l", "fp8")])
def test_the_workspace_grows_by_one_set_and_only_with_pairing(model, precision):
    cfg = E.config(model)
    for shape in (E.X, E.Y1, E.Y2):
        size = {}
        for mode in (1, 2, 0):
            r = E.Runner(model, precision)
            base = r.lib.qst_encoder_bwd_workspace_bytes(r.handle, *shape)
            r.enc.set_wgrad_pairs(mode)
            size[mode] = r.lib.qst_encoder_bwd_workspace_bytes(r.handle, *shape)
            assert base == size[mode] if mode != 2 else base < size[mode]      # a new handle: the library's choice
        assert size[2] - size[1] == second_set_bytes(cfg, shape)
        # the library's own choice at these row counts (below 8,192) is one launch per layer
        assert size[0] == size[1] and r.lib.qst_wgrad_pairs_rule(_lib.make_config(cfg), shape[0] * shape[1]) == 0
    r = E.Runner(model, precision)
    assert r.lib.qst_encoder_set_wgrad_pairs(r.handle, 3) != E.QST_OK and r.lib.qst_encoder_set_wgrad_pairs(r.handle, -1) != E.QST_OK
    one = E.Runner("tiny-bert@1", "bf16")
    one.enc.set_wgrad_pairs(2)
    w2 = one.lib.qst_encoder_bwd_workspace_bytes(one.handle, *E.X)
    one.enc.set_wgrad_pairs(1)
    assert w2 == one.lib.qst_encoder_bwd_workspace_bytes(one.handle, *E.X)


@pytest.mark.parametrize("model,precision,ln", [("tiny-mpnet@3", "bf16", None), ("tiny-bert@5", "f16", None), ("minilm-2l@3", "bf16", 1)])
def test_stale_workspace_bytes_guard_bands_and_a_short_workspace(model, precision, ln):
    cfg, shape = E.config(model), E.X
    r = runner(model, precision, 2, ln_fusion=ln)
    zeroed = [run_filled(r, shape, 0, backward="one").grads.cpu() for _ in range(3)]
    stale = run_filled(r, shape, FILL, backward="one").grads.cpu()       # (run_filled checks the bands of every window)
    bound = same_launch_bound(zeroed)
    d = float((stale - zeroed[0]).abs().max())
    assert torch.isfinite(stale).all() and d <= bound, f"0xFF-filled workspace: {d:.3e} against {bound:.3e}"
    for k, v in r.sizes(shape, True, E.POOL_MEAN, True).items():
        r.win[k].arm(v)
    short = r.run(shape, backward="one", short=("ws", 1))
    assert short.rc == E.QST_ERR_WORKSPACE and r.bands_written(short.nbytes) == []
    # a workspace of the per-layer size is one set short of what a pairing handle needs
    r1 = runner(model, precision, 1, ln_fusion=ln)
    n1 = r1.sizes(shape, True, E.POOL_MEAN, True)["ws"]
    n2 = r.sizes(shape, True, E.POOL_MEAN, True)["ws"]
    assert n2 - n1 == second_set_bytes(cfg, shape)
    assert r.run(shape, backward="one", short=("ws", n2 - n1)).rc == E.QST_ERR_WORKSPACE


@pytest.mark.parametrize("model,precision,dropout,ln", [("tiny-bert", "bf16", None, None), ("tiny-mpnet@3", "f16", E.DROPOUT, None),
                                                        ("tiny-roberta@5", "bf16", None, None), ("minilm-2l", "bf16", None, 1)])
def test_the_staged_backward_never_pairs(model, precision, dropout, ln):
    """Per-layer stages with SKIP_WGRAD and WGRAD_ONLY on layer 0 (E.stages: what trainer.staged_backward issues): every call
    covers one layer, so nothing pairs with the switch at 2 -- the second set of dY tensors, the tail of the workspace,
    still holds the bytes it was filled with -- and the gradients are those of switch 1 to the arrival order of the atomics."""
    cfg, shape = E.config(model), E.X
    one, g2, ws1, ws2 = grads_of(model, precision, dropout, "staged", ln, None, shape)
    assert ws2 - ws1 == second_set_bytes(cfg, shape)
    bound, d = same_launch_bound(one), float((g2 - one[0]).abs().max())
    assert d <= bound, f"staged, switch 2 against 1: {d:.3e}, allowed {bound:.3e}"
    r = runner(model, precision, 2, ln_fusion=ln)
    res = run_filled(r, shape, FILL, dropout=dropout, backward="staged")
    tail = r.win["ws"].view(ws2)[ws1:]
    assert tail.numel() == second_set_bytes(cfg, shape) and bool((tail == FILL).all())
    assert float((res.grads.cpu() - one[0]).abs().max()) <= bound
    # ... while the one-call backward of the same handle does use it
    run_filled(r, shape, FILL, dropout=dropout, backward="one")
    assert not bool((r.win["ws"].view(ws2)[ws1:] == FILL).all())


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name,B,dropout", [("tiny-bert", 3, None), ("tiny-mpnet", 3, None), ("tiny-bert", 3, (0.1, 0.1, 2024)),
                                            ("tiny-mpnet", 2, (0.1, 0.1, 2024))])
def test_both_settings_meet_the_oracle_bounds_of_the_backward_parity_tests(name, B, dropout, mode, monkeypatch):
    """tests/test_gpu_encoder.py's run_case, unchanged -- embeddings, loss and every gradient tensor against the CPU oracle at
    GRAD_LIMITS -- on the cases of test_tiny_models_trained_like and test_tiny_encoders_train_with_dropout, with the encoder
    it builds set to `mode`."""
    import kernel_helpers
    import test_gpu_encoder as T
    real = kernel_helpers.HipEncoder

    def enc_with_switch(cfg, *a, **kw):
        enc = real(cfg, *a, **kw)
        enc.set_wgrad_pairs(mode)
        return enc

    monkeypatch.setattr(kernel_helpers, "HipEncoder", enc_with_switch)
    T.run_case(name, B, 64, True, dict(std=0.08, bias_std=0.05, ln_jitter=0.1), emb_atol_vs_bf16_oracle=1.5e-3, dropout=dropout)


def test_a_handle_created_late_inherits_the_switch():
    """HipEncoder.set_wgrad_pairs reaches every precision's handle, also one that is created after the call."""
    from quadruplet_sentence_transformer_amd.encoder import HipEncoder
    cfg = E.config("tiny-bert")
    enc = HipEncoder(cfg)
    per_layer = enc.bwd_workspace_bytes("bf16", *E.X)
    enc.set_wgrad_pairs(2)
    paired = enc.bwd_workspace_bytes("bf16", *E.X)
    assert paired - per_layer == second_set_bytes(cfg, E.X)
    assert "f16" not in enc._live and enc.bwd_workspace_bytes("f16", *E.X) == paired
    enc.set_wgrad_pairs(1)
    assert enc.bwd_workspace_bytes("f16", *E.X) == per_layer == enc.bwd_workspace_bytes("bf16", *E.X)
    with pytest.raises(_lib.QstError):
        enc.set_wgrad_pairs(3)
