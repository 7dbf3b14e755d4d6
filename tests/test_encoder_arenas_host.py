"""The case table of the encoder-arena tests (encoder_arena_cases.py) covers every planner of csrc/qst_api.hip and every
setting the arena layouts depend on. No encoder is created here (qst_encoder_create needs a device): what is checked is the
table, the way test_the_case_list_covers_every_size_under_every_setting checks the one of tests/test_gpu_dense_head.py.
"""
import os
import re

import encoder_arena_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = os.path.join(ROOT, "quadruplet-sentence-transformer_amd", "csrc", "qst_api.hip")


def cases(**kw):
    return [c for c in E.CASES if all(getattr(c, k) == v for k, v in kw.items())]


def test_the_planner_list_is_the_one_of_the_source():
    """A planner added to csrc/qst_api.hip has to be added to PLANNERS (and to planners_of) before this passes again."""
    with open(API) as f:
        src = f.read()
    found = set(re.findall(r"^\w+ (plan_\w+)\(const qst_config& c", src, re.M))
    assert found == set(E.PLANNERS) and len(E.PLANNERS) == 7


def test_every_planner_meets_every_setting_it_depends_on():
    reached = set().union(*(E.planners_of(c) for c in E.CASES))
    assert reached == set(E.PLANNERS)
    for plan in E.PLANNERS:
        mine = [c for c in E.CASES if plan in E.planners_of(c)]
        # architecture: the relative-position table is part of every plan but the fp8 operand copies
        archs = {E.config(c.model).arch for c in mine}
        assert 1 in archs and len(archs) >= 2, plan
        # depth: 2, 3 and 5 layers wherever the plan has a slot per layer or a ping-pong; the fp8 configurations are the
        # two-layer ones tests/test_gpu_fp8mx.py trains (PING_PONG takes fp8 to 3 and 5 layers)
        assert {E.config(c.model).num_layers for c in mine} >= ({2} if "mx" in plan else {2, 3, 5}), plan
        if plan in ("plan_acts", "plan_mx", "plan_x3", "plan_x3_train"):
            assert {c.pool for c in mine} >= set(E.SETTINGS["pool"]), plan
        if plan in ("plan_acts", "plan_x3_train", "plan_mx_train_operands", "plan_bwd", "plan_x3_bwd"):
            assert {c.dropout for c in mine} >= set(E.SETTINGS["dropout"]), plan
        if plan in ("plan_bwd", "plan_x3_bwd"):
            assert {c.backward for c in mine} >= set(E.SETTINGS["backward"]), plan
            assert (E.DROPOUT, "staged") in {(c.dropout, c.backward) for c in mine}, plan
    assert {E.config(c.model).num_layers for c in cases(precision="bf16", training=False)} >= {2, 3, 5}     # the ping-pong of plan_acts
    assert {E.config(c.model).num_layers for c in cases(precision="bf16", training=True)} >= {2, 3, 5}


def test_every_setting_is_varied_against_the_base_case():
    from dataclasses import replace
    assert E.BASE in E.CASES and len(set(E.CASES)) == len(E.CASES)
    assert replace(E.BASE, training=False, backward=None) in E.CASES
    assert replace(E.BASE, pool=E.POOL_ALL) in E.CASES and replace(E.BASE, dropout=E.DROPOUT) in E.CASES
    assert replace(E.BASE, backward="staged") in E.CASES
    for p in E.PRECISIONS:
        assert cases(precision=p, training=False) and cases(precision=p, backward="one") and cases(precision=p, backward="staged"), p
    assert {c.precision for c in cases(pool=E.POOL_ALL)} >= {"bf16", "fp8", "bf16x3"}
    assert {c.precision for c in cases(dropout=E.DROPOUT)} >= {"bf16", "f16", "fp8", "bf16x3"}
    for key, values in E.SETTINGS.items():
        assert {getattr(c, key) for c in E.CASES} >= set(values), key


def test_the_configurations_are_the_ones_the_suite_already_runs():
    from quadruplet_sentence_transformer_amd.config import PRESETS
    models = {c.model for c in E.CASES}
    for t in E.TINY:
        assert {t, f"{t}@3", f"{t}@5"} <= models
        for name, n in ((t, 2), (f"{t}@3", 3), (f"{t}@5", 5)):
            cfg, pre = E.config(name), PRESETS[t]
            assert cfg.num_layers == n
            assert (cfg.hidden_size, cfg.intermediate_size, cfg.num_heads, cfg.arch, cfg.vocab_size) == \
                   (pre.hidden_size, pre.intermediate_size, pre.num_heads, pre.arch, pre.vocab_size)
    assert {(c.ffn_chain, c.ln_fusion) for c in cases(model="minilm-2l", precision="bf16")} >= {(7, 1), (0, 2)}
    h768 = E.config("h768-2l")
    assert (h768.hidden_size, h768.num_layers) == (768, 2) and all(c.ln_fusion == 1 for c in cases(model="h768-2l"))
    assert {c.model for c in cases(precision="fp8")} == set(E.FP8_MODELS)
    for m in E.FP8_MODELS:                         # fp8 needs H and I in multiples of 128: no tiny configuration has them
        cfg = E.config(m)
        assert cfg.hidden_size % 128 == 0 and cfg.intermediate_size % 128 == 0 and cfg.num_layers == 2
    assert {E.config(c.model).hidden_size for c in E.CASES} == {64, 128, 384, 768}          # no new width
    # every driver of Part 1, and the ping-pong at 3 and 5 layers for every precision
    assert {(p, t) for _, p, t in E.DRIVERS} == {(p, t) for p in E.PRECISIONS for t in (False, True)}
    assert {(E.config(m).num_layers, p) for m, p in E.PING_PONG} == {(n, p) for n in (3, 5) for p in E.PRECISIONS}
    assert {m for m, p in E.PING_PONG if p == "bf16"} == {f"{t}@{n}" for t in E.TINY for n in (3, 5)}


def test_the_shapes_move_every_offset_and_stay_small():
    shapes = list(E.SHAPES.values())
    assert shapes == [(5, 64), (3, 96), (8, 32)]
    for pick in (lambda s: s[0], lambda s: s[1], lambda s: s[0] * s[1]):
        assert len({pick(s) for s in shapes}) == 3
    assert all(L % 32 == 0 and n * L <= 512 for n, L in shapes)
    for m in {c.model for c in E.CASES} | {m for m, _ in E.PING_PONG}:
        cfg = E.config(m)
        room = cfg.max_position - (0 if cfg.arch == 0 else cfg.pad_token_id + 1)
        assert all(L <= room for _, L in shapes), m
    # 256-row tiles (the H = 768 GEMM + LayerNorm panel), 128-row ones (H = 384) and 64-row ones all end inside X and Y1
    assert [s[0] * s[1] % 256 for s in shapes] == [64, 32, 0]


def test_batches_are_ragged_and_in_range():
    for m in ("tiny-bert", "tiny-mpnet", "tiny-roberta@5", "minilm-2l"):
        cfg = E.config(m)
        for shape in E.SHAPES.values():
            ids, mask, types = E.batch(cfg, shape)
            assert ids.shape == mask.shape == types.shape == shape
            lens = mask.sum(1)
            assert lens.max() == shape[1] and lens.min() >= 1 and len(set(lens.tolist())) > 1
            assert (mask[:, :-1] >= mask[:, 1:]).all()                      # right-padded
            assert ((ids >= 0) & (ids < cfg.vocab_size)).all() and (ids[mask == 0] == cfg.pad_token_id).all()
            assert (ids[mask == 1] != cfg.pad_token_id).all()             # positions count from the padding id


def test_the_staged_form_is_the_one_the_trainer_issues():
    H, Em, S, W = E.BWD_HEAD, E.BWD_EMBED, E.BWD_SKIP_WGRAD, E.BWD_WGRAD_ONLY
    from quadruplet_sentence_transformer_amd import trainer
    assert (H, Em, S, W) == (trainer.BWD_HEAD, trainer.BWD_EMBED, trainer.BWD_SKIP_WGRAD, trainer.BWD_WGRAD_ONLY)
    assert E.stages(3, False) == [(H, 3, 2), (0, 2, 1), (S | Em, 1, 0), (W, 1, 0)]
    assert E.stages(1, False) == [(H | S | Em, 1, 0), (W, 1, 0)]
    assert E.stages(3, True) == [(H, 3, 2), (0, 2, 1), (Em, 1, 0)] and E.stages(1, True) == [(H | Em, 1, 0)]

    # ... checked against trainer.staged_backward itself, driven with a recording stand-in for the library
    class Lib:
        def __init__(self):
            self.calls = []

        def qst_encoder_backward_stage(self, *a):
            self.calls.append(tuple(a[-4:-1]))
            return 0

    class T:
        def data_ptr(self):
            return 0

        def numel(self):
            return 0

        def contiguous(self):
            return self

        shape = (5, 64)

        def __getitem__(self, _):
            return self

    class Enc:
        def __init__(self, n):
            from types import SimpleNamespace
            self.lib, self.cfg, self.params, self.grads, self.total = Lib(), SimpleNamespace(num_layers=n), T(), T(), 0

        def backward_operands(self, precision, n, L, ws):
            return 0, T(), T()

    class Group:
        def all_reduce(self, t, async_op=False):
            return None

    import quadruplet_sentence_transformer_amd._lib as L
    stream, L.current_stream_ptr = L.current_stream_ptr, lambda: 0
    try:
        for n in (1, 2, 3, 5):
            for prec in ("bf16", "bf16x3"):
                enc = Enc(n)
                trainer.staged_backward(enc, T(), T(), T(), T(), T(), None, [(0, 0)] * (n + 1), Group(), True, precision=prec)
                assert enc.lib.calls == E.stages(n, prec == "bf16x3"), (n, prec)
    finally:
        L.current_stream_ptr = stream
