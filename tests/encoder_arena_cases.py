"""The cases and helpers of the encoder-arena tests (test_gpu_encoder_arenas.py, test_encoder_arenas_host.py).

The encoder drivers of csrc/qst_api.hip place every activation and every gradient scratch tensor into two byte arenas the
caller owns. Seven planners lay those arenas out -- PLANNERS below -- and the library promises that (1) the size functions
say how much is needed and a shorter arena is refused, (2) nothing outside those bytes is written, (3) no result depends on
what the arenas held before the call. CASES is the table of encoder settings those promises are tested under: each setting
(SETTINGS) is varied against one base case, not crossed with every other.

Importing this module needs neither the library nor a device; `Window` and `Runner` do, when they are constructed.

Configurations: the smallest the suite already runs end to end, no new width. The tiny presets keep H, I and their heads;
their position table grows from 64 to 128 rows (66 to 130 where positions count from the padding id), because the shapes
below reach L = 96 and the presets stop at 64. test_gpu_encoder_arenas.py checks the refusal of L past the position table
on the presets as they are.
"""
from dataclasses import dataclass, replace
from functools import lru_cache
from typing import Optional, Tuple

PLANNERS = ("plan_acts", "plan_x3", "plan_x3_train", "plan_x3_bwd", "plan_mx", "plan_mx_train_operands", "plan_bwd")
PRECISIONS = ("bf16", "f16", "f16w", "fp8", "bf16x3")

# (nseq, L): 320, 288 and 256 token rows; no two share nseq, L or the row count, so every offset inside an arena moves from
# one shape to the next. Nothing above 512 rows.
X, Y1, Y2 = (5, 64), (3, 96), (8, 32)
SHAPES = {"X": X, "Y1": Y1, "Y2": Y2}

POOL_MEAN, POOL_ALL = "mean", "cls+max+mean+mean_sqrt_len+weightedmean"
DROPOUT = (0.1, 0.1)
# every value of every setting; the host test checks that CASES meets each of them under every planner it can reach
SETTINGS = {"precision": PRECISIONS, "training": (False, True), "pool": (POOL_MEAN, POOL_ALL), "dropout": (None, DROPOUT),
            "backward": ("one", "staged")}

QST_OK, QST_ERR_WORKSPACE, QST_ERR_NO_FORWARD = 0, -3, -7
BWD_HEAD, BWD_EMBED, BWD_SKIP_WGRAD, BWD_WGRAD_ONLY = 1, 2, 4, 8      # include/qst.h: QST_BWD_*

TINY = ("tiny-bert", "tiny-mpnet", "tiny-roberta")
DEPTHS = (2, 3, 5)
FP8_MODELS = ("bert-base-2l", "mpnet-base-2l", "minilm-2l")          # what tests/test_gpu_fp8mx.py trains
MODELS = tuple(f"{t}@{n}" if n != 2 else t for t in TINY for n in DEPTHS) + ("minilm-2l", "h768-2l") + FP8_MODELS[:2]


def config(model: str):
    """The EncoderConfig of a model name of this file: a preset, `preset@N` with num_layers replaced by N, or one of the
    two-layer cuts of the published widths that other test files build the same way."""
    from quadruplet_sentence_transformer_amd.config import ARCH_BERT, PRESETS
    base, _, depth = model.partition("@")
    if base in ("h768-2l", "bert-base-2l"):        # test_layernorm_fused_across_the_tiles_of_a_row_h768 / test_gpu_fp8mx.py
        cfg = replace(PRESETS["bert-base-uncased"], num_layers=2, vocab_size=4096)
    elif base == "mpnet-base-2l":
        cfg = replace(PRESETS["all-mpnet-base-v2"], num_layers=2, vocab_size=4096)
    else:
        cfg = PRESETS[base]
    if base in TINY:
        cfg = replace(cfg, max_position=128 if cfg.arch == ARCH_BERT else 130)
    if depth:
        cfg = replace(cfg, num_layers=int(depth))
    return cfg


@dataclass(frozen=True)
class Case:
    model: str = "tiny-bert"
    precision: str = "bf16"
    training: bool = True
    pool: str = POOL_MEAN
    dropout: Optional[Tuple[float, float]] = None
    backward: Optional[str] = "one"          # "one": qst_encoder_backward; "staged": as trainer.staged_backward; None
    ffn_chain: Optional[int] = None          # qst_encoder_set_ffn_chain / qst_encoder_set_ln_fusion; None: the default
    ln_fusion: Optional[int] = None

    def __post_init__(self):
        assert self.precision in PRECISIONS and self.backward in ("one", "staged", None)
        assert self.training or (self.backward is None and self.dropout is None)

    @property
    def id(self) -> str:
        parts = [self.model, self.precision, "train" if self.training else "infer"]
        parts += [] if self.pool == POOL_MEAN else ["pool_all" if self.pool == POOL_ALL else self.pool]
        parts += ["dropout"] if self.dropout else []
        parts += [self.backward] if self.backward else []
        parts += [f"ffn{self.ffn_chain}"] if self.ffn_chain is not None else []
        parts += [f"ln{self.ln_fusion}"] if self.ln_fusion is not None else []
        return "-".join(parts)


def planners_of(case: Case):
    """The planners of csrc/qst_api.hip whose layout a run of `case` depends on."""
    if case.precision == "bf16x3":
        fwd = {"plan_x3_train"} if case.training else {"plan_x3"}
        bwd = {"plan_x3_bwd"}
    elif case.precision == "fp8":
        fwd = {"plan_acts", "plan_mx_train_operands"} if case.training else {"plan_mx"}
        bwd = {"plan_bwd"}
    else:
        fwd, bwd = {"plan_acts"}, {"plan_bwd"}
    return fwd | (bwd if case.backward else set())


BASE = Case()


def _cases():
    out = [BASE]
    # architecture and depth: the relative-position table (MPNet), positions from the padding (RoBERTa), and the layer
    # slots of 3 and 5 layers, each with the inference ping-pong of the same depth
    for m in MODELS[:9]:
        out += [replace(BASE, model=m), replace(BASE, model=m, training=False, backward=None)]
    out += [replace(BASE, model=m, backward="staged") for m in ("tiny-bert", "tiny-mpnet@3", "tiny-roberta@5")]
    # precision, each in inference, training with a one-call backward and training with the staged backward
    for p in PRECISIONS:
        m = "minilm-2l" if p == "fp8" else "tiny-mpnet@3"
        out += [Case(m, p), Case(m, p, backward="staged"), Case(m, p, training=False, backward=None)]
    out += [Case("tiny-mpnet@5", "bf16x3"), Case("tiny-mpnet@5", "bf16x3", training=False, backward=None)]
    out += [Case(m, "fp8", backward=b) for m in FP8_MODELS[:2] for b in ("one", "staged")]
    out += [Case(m, "fp8", training=False, backward=None) for m in FP8_MODELS[:2]]
    # pooling head and dropout, on every planner that places the pooled vector, the argmax or the dropout counter
    for p, m in (("bf16", "tiny-bert"), ("bf16x3", "tiny-bert"), ("fp8", "minilm-2l")):
        out += [Case(m, p, pool=POOL_ALL), Case(m, p, pool=POOL_ALL, training=False, backward=None),
                Case(m, p, dropout=DROPOUT), Case(m, p, dropout=DROPOUT, backward="staged")]
    out += [Case("tiny-mpnet", "f16", pool=POOL_ALL, dropout=DROPOUT, backward="staged")]
    # the fused launches: H = 384 with the one-kernel feed-forward block and the GEMM + LayerNorm epilogues, and without
    # either; H = 768 with the row statistics exchanged between the tiles of a row (320 rows: a partial 256-row panel)
    for ffn, ln in ((7, 1), (0, 2)):
        out += [Case("minilm-2l", "bf16", backward=b, ffn_chain=ffn, ln_fusion=ln) for b in ("one", "staged")]
        out += [Case("minilm-2l", "bf16", training=False, backward=None, ffn_chain=ffn, ln_fusion=ln)]
    out += [Case("minilm-2l", "bf16", dropout=DROPOUT, ffn_chain=7, ln_fusion=1)]
    out += [Case("h768-2l", p, backward=b, ln_fusion=1) for p in ("bf16", "f16") for b in ("one", "staged")]
    out += [Case("h768-2l", "bf16", training=False, backward=None, ln_fusion=1),
            Case("h768-2l", "bf16", dropout=DROPOUT, ln_fusion=1),
            Case("bert-base-2l", "fp8", ln_fusion=1), Case("bert-base-2l", "fp8", dropout=DROPOUT, backward="staged", ln_fusion=1),
            Case("bert-base-2l", "fp8", training=False, backward=None, ln_fusion=1)]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return tuple(uniq)


CASES = _cases()

# The size and refusal tests (Part 1) name the drivers themselves: (model, precision, training) reaches forward_op16,
# forward_fp8, forward_x3 and forward_x3_train in both modes; a training entry also runs backward_op16 or backward_x3.
DRIVERS = tuple((m, p, t) for p, m in (("bf16", "tiny-mpnet@3"), ("f16", "tiny-bert"), ("f16w", "tiny-roberta"),
                                       ("fp8", "minilm-2l"), ("bf16x3", "tiny-mpnet@3")) for t in (False, True))

# The inference ping-pong (Part 4): (model, precision) at 3 and 5 layers, run with set_ffn_chain(0), set_ln_fusion(2) and no
# dropout. fp8 has no tiny configuration (H % 128): MiniLM's widths.
PING_PONG = tuple((f"{m}@{n}", p) for n in (3, 5) for p in PRECISIONS
                  for m in (("minilm-2l",) if p == "fp8" else TINY if p == "bf16" else ("tiny-mpnet",)))

# Part 3: what the batches in between (Y1, Y2) run with, next to an X of the case's own settings: another head and another
# dropout setting, and inference forwards between training ones.
OTHER = {(POOL_MEAN, None): (POOL_ALL, DROPOUT), (POOL_ALL, None): (POOL_MEAN, DROPOUT),
         (POOL_MEAN, DROPOUT): ("cls+max", None), (POOL_ALL, DROPOUT): ("max", None)}


@lru_cache(maxsize=None)
def weights(model: str):
    """Trained-like weights (every bias, every LayerNorm parameter matters), one arena per model for the whole session."""
    from quadruplet_sentence_transformer_amd.synthetic import synthetic_params
    cfg = config(model)
    kw = dict(std=0.08, bias_std=0.05, ln_jitter=0.1) if cfg.hidden_size <= 128 else dict(std=0.03, bias_std=0.02, ln_jitter=0.05)
    return synthetic_params(cfg, seed=14, **kw)


def batch(cfg, shape, seed=14):
    """ids / mask / type ids int64 [nseq, L] (numpy) of a ragged batch: lengths U{L/8 .. L}, right-padded with the padding id."""
    import numpy as np
    from quadruplet_sentence_transformer_amd.synthetic import uniform_int
    nseq, L = shape
    stream = 101 + 17 * nseq + L
    ids = uniform_int(seed, stream, nseq * L, min(1000, cfg.vocab_size // 4), cfg.vocab_size).reshape(nseq, L)
    lens = uniform_int(seed, stream + 1, nseq, max(1, L // 8), L + 1)
    lens[0] = L                                       # one full row: the last key tile of a sequence is used
    mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
    ids = np.where(mask == 1, ids, cfg.pad_token_id)
    return ids, mask, np.zeros_like(ids)


# ------------------------------------------------------------------ device side
BAND = 1 << 20
PATTERN = 0xA5


class Window:
    """A byte range inside a larger uint8 tensor that the test owns: [band | window | band], the window starting on a
    multiple of 256 bytes, at least BAND = 1 MiB of the same tensor on each side. `ptr` is what the library is given, and
    the length it is told is exactly the queried one: what it writes past either end lands in the bands.

    The 1 MiB is a condition, not a measurement: it is larger than one 256-row tile of the widest tensor at the shapes of this
    file, so a planner that is short by a tile, a stride or a pad row writes into memory of the test's own. A band that comes
    back intact proves nothing about writes beyond it -- a write further out than 1 MiB is outside what this can see."""

    def __init__(self, max_bytes: int):
        import torch
        self.whole = torch.zeros(BAND + 256 + max_bytes + BAND, dtype=torch.uint8, device="cuda")
        self.start = BAND + (-(self.whole.data_ptr() + BAND)) % 256
        self.max_bytes = max_bytes
        assert (self.whole.data_ptr() + self.start) % 256 == 0

    @property
    def ptr(self) -> int:
        return self.whole.data_ptr() + self.start

    def view(self, nbytes: int, dtype=None):
        import torch
        assert 0 <= nbytes <= self.max_bytes
        return self.whole[self.start:self.start + nbytes].view(dtype or torch.uint8)

    def arm(self, nbytes: int, inside=0) -> None:
        """Both bands -- everything of the tensor outside the window of `nbytes` -- to the byte pattern, the window itself to
        `inside` (zero: what a fresh allocation holds; the arenas keep integer slots that are read as indices, so the
        pattern goes inside only where the call under test is refused before its first launch)."""
        assert 0 <= nbytes <= self.max_bytes
        self.whole.fill_(PATTERN)
        self.view(nbytes).fill_(inside)

    def bands_intact(self, nbytes: int) -> bool:
        lo, hi = self.whole[:self.start], self.whole[self.start + nbytes:]
        assert lo.numel() >= BAND and hi.numel() >= BAND
        return bool((lo == PATTERN).all()) and bool((hi == PATTERN).all())


@dataclass
class Result:
    rc: int                      # the first status that is not QST_OK, else QST_OK
    emb: object = None           # clones of the output windows / the gradient window
    tok: object = None
    grads: object = None
    nbytes: dict = None          # the exact window lengths of this call, by window name


class Runner:
    """One HipEncoder (its handle of `precision`, shadows and parameters) driven through the C ABI -- qst_encoder_forward,
    qst_encoder_backward, qst_encoder_backward_stage -- with every arena and every output a Window: `saved`, `ws`, `emb`,
    `tok`, `grads`. One Runner keeps one handle and one set of windows for as many runs as the test makes."""

    def __init__(self, model: str, precision: str, ffn_chain=None, ln_fusion=None, cfg=None, arena=None):
        import torch
        from quadruplet_sentence_transformer_amd import _lib
        from quadruplet_sentence_transformer_amd.encoder import HipEncoder
        self.torch, self._lib = torch, _lib
        self.cfg = cfg if cfg is not None else config(model)
        self.precision = precision
        self.enc = HipEncoder(self.cfg)
        self.enc.load_arena(arena if arena is not None else weights(model))
        self.lib = self.enc.lib
        rec = self.enc._record(precision)
        self.handle = rec.handle
        if ln_fusion is not None:
            self.enc.set_ln_fusion(ln_fusion)
        if ffn_chain is not None:
            _lib.check(self.lib.qst_encoder_set_ffn_chain(self.handle, ffn_chain), "qst_encoder_set_ffn_chain")
        for name in {precision, rec.spec.bwd_shadow, "bf16"}:
            if self.enc._record(name).shadow is not None:
                self.enc.refresh_shadow(name)
        self.fwd_shadow = rec.shadow if rec.shadow is not None else self.enc._live["bf16"].shadow
        self.bwd_shadow = self.enc._live[rec.spec.bwd_shadow].shadow
        self.drop_state = torch.zeros(4, dtype=torch.int32, device="cuda")
        self.win = {}
        self._batches = {}

    # -- settings of the handle
    def set_head(self, pool: str, dropout, seed: int = 77) -> int:
        """The pooling head and the dropout of the next call; dropout re-initialises the counter, so that equal calls see equal
        (seed, step). Returns the embedding width D."""
        from quadruplet_sentence_transformer_amd.config import pooling_mask
        lib, st = self.lib, self._lib.current_stream_ptr()
        self._lib.check(lib.qst_encoder_set_pooling(self.handle, pooling_mask(pool)), "qst_encoder_set_pooling")
        if dropout:
            self._lib.check(lib.qst_dropout_init(self.drop_state.data_ptr(), seed, st), "qst_dropout_init")
            self._lib.check(lib.qst_encoder_set_dropout(self.handle, dropout[0], dropout[1], self.drop_state.data_ptr()))
        else:
            self._lib.check(lib.qst_encoder_set_dropout(self.handle, 0.0, 0.0, None))
        return lib.qst_encoder_embedding_dim(self.handle)

    def sizes(self, shape, training: bool, pool: str, backward: bool):
        """The exact length of every window of one call: the two size functions, and the documented output shapes."""
        D = self.set_head(pool, None)
        n, L = shape
        out = {"saved": self.lib.qst_encoder_saved_bytes(self.handle, n, L, int(training)),
               "emb": n * D * 4, "tok": n * L * self.cfg.hidden_size * 4}
        if backward:
            out["ws"] = self.lib.qst_encoder_bwd_workspace_bytes(self.handle, n, L)
            out["grads"] = self.enc.total * 4
        return out

    def make_windows(self, shapes=(X, Y1, Y2), pools=(POOL_MEAN, POOL_ALL), slack=0):
        """One window per arena and output, long enough for every shape and head of the test (+ slack); each call is told its
        own exact length."""
        need = {}
        for s in shapes:
            for p in pools:
                for k, v in self.sizes(s, True, p, True).items():
                    need[k] = max(need.get(k, 0), v)
                need["saved"] = max(need["saved"], self.sizes(s, False, p, False)["saved"])
        win = {k: Window(v + slack) for k, v in need.items()}
        if not slack:
            self.win = win
        return win

    def inputs(self, shape):
        if shape not in self._batches:
            ids, mask, types = [self.torch.from_numpy(a).cuda() for a in batch(self.cfg, shape)]
            self._batches[shape] = (ids, mask, types if self.cfg.type_vocab_size else None)
        return self._batches[shape]

    # -- one call
    def set_inputs(self, shape, ids, mask, types):
        """A batch of the test's own for `shape` (numpy or torch, nseq * L elements each) instead of batch()."""
        t = [self.torch.as_tensor(a).reshape(shape).contiguous().cuda() for a in (ids, mask, types)]
        self._batches[shape] = (t[0], t[1], t[2] if self.cfg.type_vocab_size else None)

    def run(self, shape, training=True, pool=POOL_MEAN, dropout=None, backward=None, arm=False, short=None, forward=True,
            win=None, generous=0, zero_grads=True) -> Result:
        """A forward of `shape` and, with backward = "one" / "staged", its backward into a zeroed gradient window.

        arm: every window is re-armed first (bands to the pattern, inside zero). short = (window name, k): that window's
        length is reported k bytes shorter than the size function asked for. forward=False: the backward alone, over what
        the last forward left. The windows are self.win unless `win` names others; generous = k: both arenas are reported k
        bytes LONGER than asked for (windows made with that slack). zero_grads=False leaves the gradient window as it is."""
        torch, lib, _lib = self.torch, self.lib, self._lib
        win = win or self.win
        n, L = shape
        nb = self.sizes(shape, training, pool, backward is not None)
        assert nb["saved"] > 0 and (backward is None or nb["ws"] > 0), f"unsupported shape {shape}"
        D = self.set_head(pool, dropout)
        if arm:
            for k, v in nb.items():
                win[k].arm(v)
        told = dict(nb)
        if short:
            told[short[0]] -= short[1]
        for k in ("saved", "ws"):
            if generous and k in told:
                assert told[k] + generous <= win[k].max_bytes
                told[k] += generous
        ids, mask, types = self.inputs(shape)
        st = _lib.current_stream_ptr()
        res = Result(QST_OK, nbytes=nb)
        if forward:
            res.rc = lib.qst_encoder_forward(self.handle, ids.data_ptr(), mask.data_ptr(), _lib.ptr(types), n, L,
                                             self.enc.params.data_ptr(), self.fwd_shadow.data_ptr(), win["emb"].ptr, win["tok"].ptr,
                                             win["saved"].ptr, told["saved"], int(training), st)
        if backward is not None and res.rc == QST_OK:
            ge = torch.randn(n, D, generator=torch.Generator().manual_seed(3)).cuda()
            if zero_grads:
                win["grads"].view(nb["grads"]).zero_()
            common = (self.handle, ids.data_ptr(), mask.data_ptr(), _lib.ptr(types), n, L, self.enc.params.data_ptr(),
                      self.bwd_shadow.data_ptr(), ge.data_ptr(), win["grads"].ptr, win["saved"].ptr, told["saved"], win["ws"].ptr,
                      told["ws"])
            if backward == "one":
                res.rc = lib.qst_encoder_backward(*common, st)
            else:
                for flags, hi, lo in stages(self.cfg.num_layers, self.precision == "bf16x3"):
                    res.rc = lib.qst_encoder_backward_stage(*common, flags, hi, lo, st)
                    if res.rc != QST_OK:
                        break
        torch.cuda.synchronize()
        if res.rc == QST_OK:
            if forward:
                res.emb = win["emb"].view(nb["emb"], torch.float32).clone().view(n, D)
                res.tok = win["tok"].view(nb["tok"], torch.float32).clone().view(n, L, -1)
            if backward is not None:
                res.grads = win["grads"].view(nb["grads"], torch.float32).clone()
        return res

    def bands_written(self, nbytes: dict):
        """The windows of the last armed call whose bands no longer hold the pattern (empty: none was written)."""
        return [k for k, v in nbytes.items() if not self.win[k].bands_intact(v)]


def stages(N: int, x3: bool):
    """(flags, layer_hi, layer_lo) of the staged backward, exactly as trainer.staged_backward issues them: top-down layer by
    layer, then {layer 0 | SKIP_WGRAD | EMBED} followed by WGRAD_ONLY; bf16x3 has its own tail (no postponed launch)."""
    out = [(BWD_HEAD if k == 0 else 0, l + 1, l) for k, l in enumerate(range(N - 1, 0, -1))]
    head = BWD_HEAD if N == 1 else 0
    if x3:
        return out + [(head | BWD_EMBED, 1, 0)]
    return out + [(head | BWD_SKIP_WGRAD | BWD_EMBED, 1, 0), (BWD_WGRAD_ONLY, 1, 0)]


# ------------------------------------------------------------------ the comparison rule of Parts 2 and 3
# Gradients of two runs of the same call: relative L2 difference per parameter tensor below 1e-6 -- the project's own line in
# profiles/r05_determinism.txt: the atomics of the weight-gradient and embedding kernels reorder fp32 sums from run to run,
# measured 1.7e-7, and "anything above ~1e-6 would be a race". A tensor whose norm is below 1e-5 of the whole gradient's is
# rounding noise around zero: it is held absolutely against the whole norm, as tests/test_gpu_encoder.py does.
GRAD_REL_L2 = 1e-6        # [largest figure over every case of tests/test_gpu_encoder_arenas.py: 1.35e-7]


def grad_differences(cfg, g1, g0):
    """[(segment name, figure)] of every parameter tensor of build_layout(cfg) whose gradient differs between g1 and g0 by
    GRAD_REL_L2 or more, and the largest figure seen."""
    from quadruplet_sentence_transformer_amd.config import build_layout
    segs, _ = build_layout(cfg)
    a, b = g1.double().cpu(), g0.double().cpu()
    gnorm = float(b.norm())
    bad, worst = [], 0.0
    for s in segs:
        x, y = a[s.offset:s.offset + s.numel], b[s.offset:s.offset + s.numel]
        denom = float(y.norm())
        fig = float((x - y).norm()) / (gnorm if denom <= 1e-5 * gnorm else denom) if gnorm > 0 else float(x.norm())
        worst = max(worst, fig)
        if not fig < GRAD_REL_L2:
            bad.append((s.name, fig))
    return bad, worst


def same_results(cfg, r1: Result, r0: Result, what: str):
    """Forward outputs bit for bit, gradients by the rule above. Returns the largest gradient figure (None without one)."""
    import torch
    assert r1.rc == QST_OK and r0.rc == QST_OK, f"{what}: status {r1.rc} / {r0.rc}"
    assert torch.isfinite(r0.emb).all() and torch.isfinite(r0.tok).all(), what
    assert torch.equal(r1.emb, r0.emb), f"{what}: out_emb differs in {int((r1.emb != r0.emb).sum())} elements, " \
                                        f"max |d| {float((r1.emb - r0.emb).abs().max()):.3e}"
    assert torch.equal(r1.tok, r0.tok), f"{what}: out_tok differs in {int((r1.tok != r0.tok).sum())} elements, " \
                                        f"max |d| {float((r1.tok - r0.tok).abs().max()):.3e}"
    if r0.grads is None:
        assert r1.grads is None
        return None
    assert torch.isfinite(r0.grads).all() and float(r0.grads.abs().max()) > 0, what
    bad, worst = grad_differences(cfg, r1.grads, r0.grads)
    assert not bad, f"{what}: gradients differ by relative L2 >= {GRAD_REL_L2}: {bad[:6]}"
    return worst
