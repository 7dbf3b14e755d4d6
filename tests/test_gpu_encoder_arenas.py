"""GPU: the two byte arenas of the encoder drivers (csrc/qst_api.hip) -- sizes, bounds, independence from stale bytes -- and
the inference ping-pong of two layer slots.

Every call goes through the C ABI (encoder_arena_cases.Runner: qst_encoder_forward, qst_encoder_backward,
qst_encoder_backward_stage) with `saved`, `workspace`, `out_emb`, `out_tok` and the gradient arena as windows inside larger
tensors of the test's own (encoder_arena_cases.Window): each starts on a multiple of 256 bytes, is exactly as long as the size
function said (the outputs: their documented shapes) and has 1 MiB of the test's memory on each side. The 1 MiB is a
condition, not a measurement: it is more than one 256-row tile of the widest tensor at these shapes, and a band that came back
intact proves nothing about writes beyond it.

  1. sizes and refusals: the exact size is accepted, one byte less is QST_ERR_WORKSPACE before the first launch (in every
     driver the comparison against the plan's total is the first statement after the plan is built -- read, then run), and
     the size functions refuse what the drivers refuse;
  2. bounds: both bands of every window hold a byte pattern before forward + backward and afterwards;
  3. stale contents: X on zero-filled windows against X after Y1 and Y2 in the same windows, forward outputs bit for bit,
     gradients by the run-to-run line of profiles/r05_determinism.txt (encoder_arena_cases.GRAD_REL_L2). The arenas are
     only ever filled by real earlier batches: they hold integer slots (position ids, the dropout counter, the argmax of
     max pooling) that are read as indices, and stale values of a valid batch are in range -- what production sees;
  4. the inference ping-pong (layer l >= 2 reuses the slot of layer l - 2) against the training forward, which keeps every
     layer's slots, at 3 and 5 layers, and the 5-layer result against the oracle.

Parts 2, 3 and 4 were each shown able to fail on a scratch copy of csrc/qst_api.hip with one line changed, every access still
inside the test's tensors: see the docstrings of the three tests concerned.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import encoder_arena_cases as E  # noqa: E402
from encoder_arena_cases import (CASES, DRIVERS, OTHER, PATTERN, PING_PONG, POOL_ALL, POOL_MEAN, QST_ERR_NO_FORWARD,  # noqa: E402
                                 QST_ERR_WORKSPACE, QST_OK, X, Y1, Y2, Runner, same_results)

TRAINING = [c for c in CASES if c.training]
STAGED = [c for c in CASES if c.backward == "staged"]
ids_of = lambda cases: [c.id for c in cases]  # noqa: E731


def runner_of(case, **kw):
    return Runner(case.model, case.precision, ffn_chain=case.ffn_chain, ln_fusion=case.ln_fusion, **kw)


def settings_of(case):
    return dict(training=case.training, pool=case.pool, dropout=case.dropout, backward=case.backward)


def all_pattern(win):
    return bool((win.whole == PATTERN).all())


# ------------------------------------------------------------------ 1. sizes and refusals
@pytest.mark.parametrize("model,precision,training", DRIVERS, ids=[f"{m}-{p}-{'train' if t else 'infer'}" for m, p, t in DRIVERS])
def test_exact_size_is_accepted_and_one_byte_less_is_refused_before_any_launch(model, precision, training):
    """Every forward driver (16-bit, fp8, bf16x3; inference and training) and, from the training entries, both backward
    drivers, one-call and staged. A refused call must have launched nothing: every window -- outputs, arenas, gradients, bands
    and inside -- holds the byte pattern afterwards, bit for bit. (The pattern may fill the arenas here, and only here: the
    refusal stands before the first launch, so nothing reads it.) A refused training forward leaves no record: the window
    has just held a training forward of Y1, and the backward of X over it is QST_ERR_NO_FORWARD, not a run over Y1's bytes."""
    r = Runner(model, precision)
    win = r.make_windows()
    kw = dict(training=training, pool=POOL_ALL)
    if training:
        assert r.run(Y1, backward="one", **kw).rc == QST_OK
    for w in win.values():
        w.whole.fill_(PATTERN)
    assert r.run(X, short=("saved", 1), **kw).rc == QST_ERR_WORKSPACE
    assert [k for k, w in win.items() if not all_pattern(w)] == []
    if not training:
        assert r.run(X, arm=True, **kw).rc == QST_OK
        return
    for form in ("one", "staged"):
        assert r.run(X, backward=form, forward=False, zero_grads=False, **kw).rc == QST_ERR_NO_FORWARD, form
    assert [k for k, w in win.items() if not all_pattern(w)] == []
    # the backward drivers: a forward of exactly the size asked for, then each arena one byte short
    fwd = r.run(X, arm=True, **kw)
    assert fwd.rc == QST_OK
    saved = win["saved"].whole.clone()
    for k in ("ws", "grads"):
        win[k].whole.fill_(PATTERN)
    # (the backward after an fp8 forward reads the bf16 arena in front of the MXFP8 operand copies, not the copies: `saved`
    #  may end before them, so one byte less than the fp8 forward asked for is still enough)
    for form in ("one", "staged"):
        for which in ("ws",) if precision == "fp8" else ("ws", "saved"):
            assert r.run(X, backward=form, forward=False, zero_grads=False, short=(which, 1), **kw).rc == QST_ERR_WORKSPACE, (form, which)
    assert all_pattern(win["ws"]) and all_pattern(win["grads"]) and torch.equal(win["saved"].whole, saved)
    for form in ("one", "staged"):
        win["ws"].arm(r.sizes(X, True, POOL_ALL, True)["ws"])
        out = r.run(X, backward=form, forward=False, **kw)
        assert out.rc == QST_OK and torch.isfinite(out.grads).all() and float(out.grads.abs().max()) > 0, form


@pytest.mark.parametrize("precision", E.PRECISIONS)
def test_the_size_functions_refuse_what_the_drivers_refuse(precision):
    """0 for L % 32 != 0, L > 512, nseq <= 0, L beyond max_position (BERT) and L + pad_token_id + 1 beyond it (MPNet,
    RoBERTa) -- on the presets as they are: 64 position rows, 66 where positions count from the padding."""
    from quadruplet_sentence_transformer_amd.config import PRESETS
    from quadruplet_sentence_transformer_amd.encoder import HipEncoder
    models = ["minilm-2l", "all-mpnet-base-v2"] if precision == "fp8" else ["tiny-bert", "tiny-mpnet", "tiny-roberta", "minilm-2l"]
    for name in models:
        cfg = PRESETS[name] if name != "all-mpnet-base-v2" else E.config("mpnet-base-2l")
        enc = HipEncoder(cfg)
        sizes = lambda n, L: (enc.saved_bytes(precision, n, L, False), enc.saved_bytes(precision, n, L, True),  # noqa: E731
                              enc.bwd_workspace_bytes(precision, n, L))
        top = cfg.max_position if cfg.arch == 0 else cfg.max_position - cfg.pad_token_id - 1
        top = min(top, 512)
        assert top % 32 == 0 and all(s > 0 for s in sizes(5, top)), (name, top)
        for n, L in ((5, 33), (5, 48), (5, 544), (0, 64), (-1, 64), (5, top + 32), (5, 0)):
            assert sizes(n, L) == (0, 0, 0), (name, n, L)


@pytest.mark.parametrize("model,precision", sorted({(c.model, c.precision) for c in CASES}))
def test_relations_between_the_sizes(model, precision):
    """Training >= inference; no size decreases with nseq; QST_POOL_ALL over QST_POOL_MEAN adds the pre-normalize vector's four
    further blocks and the argmax of max pooling (include/qst.h): at least nseq * 4H * 4 + nseq * H * 4 bytes, less than that
    plus 512 (two buffers, each rounded up to 256)."""
    r = Runner(model, precision)
    H = r.cfg.hidden_size
    for L in (32, 64, 96):
        prev = None
        for nseq in range(1, 10):
            mean_i, mean_t = (r.sizes((nseq, L), t, POOL_MEAN, True) for t in (False, True))
            all_i, all_t = (r.sizes((nseq, L), t, POOL_ALL, True) for t in (False, True))
            assert 0 < mean_i["saved"] <= mean_t["saved"] and 0 < all_i["saved"] <= all_t["saved"]
            add = nseq * 4 * H * 4 + nseq * H * 4
            for a, m in ((all_i, mean_i), (all_t, mean_t)):
                assert add <= a["saved"] - m["saved"] < add + 512, (nseq, L, a["saved"] - m["saved"], add)
                assert a["ws"] == m["ws"] > 0
            now = (mean_i["saved"], mean_t["saved"], all_i["saved"], all_t["saved"], mean_t["ws"])
            assert prev is None or all(b >= a for a, b in zip(prev, now)), (nseq, L)
            prev = now


# ------------------------------------------------------------------ 2. bounds
@pytest.mark.parametrize("case", CASES, ids=ids_of(CASES))
def test_nothing_is_written_outside_the_bytes_asked_for(case):
    """X, Y1 and Y2 (320, 288, 256 rows: partial 64-, 128- and 256-row tiles), forward + backward in the case's form, on
    windows of exactly the queried sizes: both bands of every window hold the pattern afterwards, and the results are those of
    the same call on generous arenas (64 KiB more than asked for, and told so), by the rules of Part 3.

    Able to fail: on a scratch copy with `a.rs2 = take(M * 2)` in plan_acts (the row statistics of the second LayerNorm are
    M * 4 bytes: 512 bytes over the slot, for the last layer over the end of the arena) 51 of the 70 cases failed, 42 of them
    on the band of `saved`, the fp8 training ones -- whose arena goes on behind plan_acts -- on the comparison."""
    r = runner_of(case)
    r.make_windows()
    wide = r.make_windows(slack=1 << 16)
    kw = settings_of(case)
    for shape in (X, Y1, Y2):
        ref = r.run(shape, win=wide, generous=1 << 16, **kw)
        got = r.run(shape, arm=True, **kw)
        assert got.rc == QST_OK, f"{shape}: windows of exactly the queried sizes were refused ({got.rc})"
        assert r.bands_written(got.nbytes) == [], f"{shape}: written outside the window"
        same_results(r.cfg, got, ref, f"{case.id} {shape}: exact windows against generous arenas")


# ------------------------------------------------------------------ 3. stale contents
def stale_sequence(case, between, r=None):
    """R0 = X on zero-filled windows; then, clearing nothing, `between` and X again = R1. Same handle, same windows."""
    r = r or runner_of(case)
    r.make_windows()
    kw = settings_of(case)
    r0 = r.run(X, **kw)
    for shape, other in between:
        assert r.run(shape, **{**kw, **other}).rc == QST_OK, (shape, other)
    r1 = r.run(X, **kw)
    worst = same_results(r.cfg, r1, r0, f"{case.id}: X after {[s for s, _ in between]} against X on zeroed arenas")
    if worst is not None:
        print(f"  {case.id}: largest relative L2 difference of a gradient tensor {worst:.2e} (limit {E.GRAD_REL_L2})")
    return r


@pytest.mark.parametrize("case", CASES, ids=ids_of(CASES))
def test_results_do_not_depend_on_what_earlier_batches_left(case):
    """X, Y1, Y2, X with the case's settings throughout: every offset of both arenas differs between the three shapes.

    Able to fail: on a scratch copy with the `hipMemsetAsync(drel, ...)` of backward_op16 dropped (the relative-position
    gradient then accumulates on what the last batch left in the workspace) every MPNet case with a 16-bit backward failed
    here and in the four tests below, 41 of 187; a zeroed workspace, which is all a fresh encoder per test ever sees, hides it."""
    stale_sequence(case, [(Y1, {}), (Y2, {})])


@pytest.mark.parametrize("case", TRAINING, ids=ids_of(TRAINING))
def test_results_do_not_depend_on_batches_of_another_head_and_dropout_setting(case):
    """The batches in between run another pooling head (the pooled vector and the argmax change size, so does out_emb) and
    another dropout setting (the counter slot is written or not). X runs compare equal (seed, step): the counter is
    initialised again before each call."""
    pool, drop = OTHER[(case.pool, case.dropout)]
    stale_sequence(case, [(Y1, dict(pool=pool, dropout=drop)), (Y2, dict(pool=pool, dropout=drop)),
                          (X, dict(pool=pool, dropout=drop))])


@pytest.mark.parametrize("case", TRAINING, ids=ids_of(TRAINING))
def test_inference_and_training_forwards_alternate_in_one_window(case):
    """Inference lays `saved` out by another plan than training (two layer slots; for fp8 and bf16x3 another planner
    altogether): training X, inference Y1, training Y2, inference X, training X in one window -- and the inference X against
    an inference X on zeroed windows."""
    infer = dict(training=False, backward=None, dropout=None)
    r = runner_of(case)
    r.make_windows()
    i0 = r.run(X, **{**settings_of(case), **infer})
    r = stale_sequence(case, [(Y1, infer), (Y2, {}), (X, infer)], r)
    i1 = r.run(X, **{**settings_of(case), **infer})
    same_results(r.cfg, i1, i0, f"{case.id}: inference X after training runs against inference X on zeroed arenas")


@pytest.mark.parametrize("case", STAGED, ids=ids_of(STAGED))
def test_staged_backward_after_a_one_call_backward_in_the_same_workspace(case):
    """QST_BWD_SKIP_WGRAD leaves layer 0's operands in the workspace for the later QST_BWD_WGRAD_ONLY call, and every stage
    finds the running d(loss)/d(x) there: none of it may be what the one-call backward of another batch left."""
    stale_sequence(case, [(Y1, dict(backward="one")), (Y2, dict(backward="one"))])


@pytest.mark.parametrize("precision", E.PRECISIONS)
def test_the_cached_arenas_of_hipencoder_over_x_y1_y2_x(precision):
    """The public path: HipEncoder.forward / backward on its own cached arenas (which only grow, so X's second run finds Y1's
    and Y2's bytes at every offset) against a fresh encoder that only ever saw X."""
    from quadruplet_sentence_transformer_amd.encoder import HipEncoder
    model = "minilm-2l" if precision == "fp8" else "tiny-mpnet@3"
    cfg = E.config(model)

    def inputs(shape):
        ids, mask, types = [torch.from_numpy(a).cuda() for a in E.batch(cfg, shape)]
        return ids, mask, (types if cfg.type_vocab_size else None)

    def step(enc, shape):
        ids, mask, types = inputs(shape)
        emb, tok, saved = enc.forward(ids, mask, types, training=True, want_tokens=True, precision=precision)
        ge = torch.randn(emb.shape, generator=torch.Generator().manual_seed(3)).cuda()
        enc.grads.zero_()
        enc.backward(ids, mask, types, ge, saved, precision=precision)
        emb_i, tok_i, _ = enc.forward(ids, mask, types, want_tokens=True, precision=precision)
        torch.cuda.synchronize()
        return (E.Result(QST_OK, emb.clone(), tok.clone(), enc.grads.clone()), E.Result(QST_OK, emb_i.clone(), tok_i.clone()))

    def encoder():
        enc = HipEncoder(cfg)
        enc.load_arena(E.weights(model))
        enc.ensure_train_state()
        return enc

    fresh = step(encoder(), X)
    enc = encoder()
    for shape in (X, Y1, Y2):
        step(enc, shape)
    again = step(enc, X)
    same_results(cfg, again[0], fresh[0], f"{precision}: training X on the cached arenas after Y1, Y2 against a fresh encoder")
    same_results(cfg, again[1], fresh[1], f"{precision}: inference X on the cached arenas after Y1, Y2 against a fresh encoder")


# ------------------------------------------------------------------ 4. the inference ping-pong
@pytest.mark.parametrize("model,precision", PING_PONG, ids=[f"{m}-{p}" for m, p in PING_PONG])
def test_inference_ping_pong_gives_the_training_forwards_result(model, precision):
    """3 and 5 layers: the inference forward keeps two layer slots (layer l >= 2 writes over layer l - 2; fp8 and bf16x3
    alternate two residual buffers), the training forward keeps them all. set_ffn_chain(0), set_ln_fusion(2) and no dropout:
    both run the same launches, so out_emb and out_tok agree bit for bit.

    fp8 is by design not bit-identical between the two: the training forward's FFN-1 (QST_EPI_GELU_MX_TRAIN) quantises the
    bf16-ROUNDED h to MXFP8 -- the bf16 copy is what its backward reads -- where inference (QST_EPI_GELU_MX) quantises the
    fp32 gelu; it is held to the bound tests/test_gpu_fp8mx.py already sets on this very pair, 4e-3 of the embedding scale
    (measured there and here: see the printed figure).

    Able to fail: on a scratch copy with the slot assignment `a = p.layers[l - 2]` of plan_acts dropped (layers from the third
    on then run with every buffer at offset 0 of the arena) all ten 16-bit cases and both oracle cases below failed. Taking the
    slot of layer l - 1 instead does NOT fail, and rightly: a layer has consumed its input x / xb (QKV GEMM, out-projection
    residual) before the launch that writes its output, so any slot but one a launch reads and writes at once gives the
    training forward's bits."""
    r = Runner(model, precision, ffn_chain=0, ln_fusion=2)
    r.make_windows(shapes=(X,), pools=(POOL_MEAN,))
    train = r.run(X, training=True)
    infer = r.run(X, training=False)
    assert train.rc == QST_OK and infer.rc == QST_OK
    assert torch.isfinite(train.emb).all() and torch.isfinite(train.tok).all()
    if precision == "fp8":
        sc = float(train.emb.norm(dim=-1).mean())
        d = float((infer.emb - train.emb).abs().max()) / sc
        print(f"  {model} fp8: max |d emb| / scale between the inference and the training forward {d:.2e} (limit 4e-3)")
        assert d < 4e-3
        return
    same_results(r.cfg, infer, train, f"{model} {precision}: inference forward against training forward")


@pytest.mark.parametrize("model", ["tiny-bert@5", "tiny-mpnet@5"])
def test_five_layer_inference_against_the_oracle(model):
    """Two equal wrong answers would pass the comparison above: the 5-layer inference result is also held to the oracle
    comparison of test_gpu_encoder.run_case at its tolerances -- embeddings rtol 1e-3 / atol 1e-4 against the oracle with the
    same operand rounding, atol 2e-3 against the fp32 oracle, the loss within 1e-4 / 1e-3 -- on run_case's own inputs (HF-init
    weights, a ragged quadruplet batch)."""
    from oracle import torch_ref as R
    from quadruplet_sentence_transformer_amd.encoder import quadruplet_loss_raw
    from quadruplet_sentence_transformer_amd.synthetic import synthetic_params, synthetic_quadruplets
    from test_gpu_encoder import LOSS_KW
    cfg = E.config(model)
    B, L = 2, 64
    arena = synthetic_params(cfg, seed=14, std=0.02)
    ids, mask, types = [torch.from_numpy(a) for a in synthetic_quadruplets(cfg, B, L, seed=14, ragged=True)]
    P = R.arena_to_dict(arena, cfg)
    with torch.no_grad():
        loss32, emb32 = R.quadruplet_step(P, cfg, ids, mask, types, LOSS_KW)
        lossb, embb = R.quadruplet_step(P, cfg, ids, mask, types, LOSS_KW, bf16_operands=True)
    r = Runner(model, "bf16", ffn_chain=0, ln_fusion=2, arena=arena)
    shape = (4 * B, L)
    r.set_inputs(shape, ids, mask, types)
    r.make_windows(shapes=(shape,), pools=(POOL_MEAN,))
    train = r.run(shape, training=True)
    infer = r.run(shape, training=False)
    same_results(r.cfg, infer, train, f"{model}: inference forward against training forward")
    e4 = infer.emb.view(4, B, -1)
    loss = quadruplet_loss_raw(e4[0], e4[1], e4[2], e4[3], 0.6, 1.0, 0.5, 0.5, 2.0, False, 2)[0].item()
    emb = e4.cpu()
    print(f"  {model}: max |d emb| {float((emb - embb).abs().max()):.2e} vs the same-rounding oracle, "
          f"{float((emb - emb32).abs().max()):.2e} vs fp32; |d loss| {abs(loss - lossb.item()):.2e} / {abs(loss - loss32.item()):.2e}")
    torch.testing.assert_close(emb, embb, rtol=1e-3, atol=1e-4)
    assert abs(loss - lossb.item()) < 1e-4
    assert abs(loss - loss32.item()) < 1e-3
    torch.testing.assert_close(emb, emb32, rtol=0, atol=2e-3)
