"""GPU: CoSENTLoss and AnglELoss -- qst_cosent_loss (csrc/cosent.hip), its autograd and the loss classes of st_losses.py --
against the yardstick in cosent_helpers: sentence-transformers' two pairwise scores and its B x B logsumexp in torch ops,
fp64 on the CPU with autograd. The tolerances are the project's own: values and scores within rtol = atol =
max(1e-5, 1.5e-8 D), gradients within rtol 1e-4, atol 1e-6 * max(1, max |reference gradient|)."""
import math
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import cosent_helpers as CH  # noqa: E402
from kernel_helpers import lib, ptr, stream  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import st_losses as S, util  # noqa: E402
from quadruplet_sentence_transformer_amd.evaluation import EmbeddingSimilarityEvaluator  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import (InputExample, SentenceTransformer,  # noqa: E402
                                                                       encode_columns_fused)

NAN = float("nan")
UP = 1.7                                                    # the upstream gradient of the parity tests
SIM_CODE = {"cos": S.PAIRSIM_COS, "angle": S.PAIRSIM_ANGLE}


def run(u, v, y, sim, scale=CH.SCALE, up=None, want_grads=True):
    """(loss [1], scores [B], [grad_u, grad_v]) of the kernel on the CPU tensors u, v, y."""
    g = None if up is None else torch.tensor([up], device="cuda")
    return S.cosent_loss_raw(u.cuda().contiguous(), v.cuda().contiguous(), y.cuda().contiguous(), sim, scale, grad_out=g,
                             want_grads=want_grads)


def check(got, ref, D, what, up=1.0, rows=None):
    """Prints every figure as a share of its tolerance, then asserts. ref = (loss, scores, grad_u, grad_v) in fp64; rows
    selects the rows of the kernel's outputs the reference has."""
    out, scores, grads = got
    loss, ref_scores, gu, gv = ref
    sc, ku, kv = scores.cpu(), grads[0].cpu(), grads[1].cpu()
    if rows is not None:
        sc, ku, kv = sc[rows], ku[rows], kv[rows]
    ev = CH.value_error(out.item(), loss, D)
    es = CH.score_error(sc, ref_scores, D)
    eu, ew = CH.grad_error(ku, up * gu), CH.grad_error(kv, up * gv)
    print(f"  {what}: loss {out.item():.7f} ref {loss.item():.7f}; share of the tolerance: value {ev:.3f} scores {es:.3f} "
          f"grad_u {eu:.3f} grad_v {ew:.3f}")
    assert torch.isfinite(out).all() and torch.isfinite(ku).all() and torch.isfinite(kv).all()
    assert ev <= 1.0 and es <= 1.0 and eu <= 1.0 and ew <= 1.0


# ------------------------------------------------------------------ 1. kernel parity
@pytest.mark.parametrize("kind", CH.LABEL_SETS)
@pytest.mark.parametrize("B,D,sim", CH.cases(), ids=lambda x: str(x))
def test_kernel_matches_reference(lib, B, D, sim, kind):
    u, v, y, loss, scores, gu, gv = CH.reference(B, D, sim, kind)
    CH.assert_conditions(B, sim, loss, scores, gu, gv)
    got = run(u, v, y, sim, up=UP)
    check(got, (loss, scores, gu, gv), D, f"{B}x{D} {sim} {kind}", up=UP)
    # the forward-only call returns the same values
    fwd, fscores, none = run(u, v, y, sim, want_grads=False)
    assert none == [None, None] and torch.equal(fwd, got[0]) and torch.equal(fscores, got[1])


@pytest.mark.parametrize("sim", CH.SIMS)
def test_unaligned_pointers_take_the_element_form(lib, sim):
    """Rows that start 4 bytes off a 16-byte boundary: the same values as from aligned rows, by the element-wise form."""
    B, D = 8, 384
    u, v, y, loss, scores, gu, gv = CH.reference(B, D, sim, "graded")
    us, vs = [torch.empty(B * D + 1, device="cuda")[1:].view(B, D).copy_(t) for t in (u, v)]
    assert us.data_ptr() % 16 == 4 and us.is_contiguous()
    got = S.cosent_loss_raw(us, vs, y.cuda(), sim, CH.SCALE, want_grads=True)
    check(got, (loss, scores, gu, gv), D, f"unaligned {sim}")


# ------------------------------------------------------------------ 2. edges
@pytest.mark.parametrize("sim", CH.SIMS)
@pytest.mark.parametrize("B,D", [(1, 2), (5, 10), (64, 384)])
def test_without_a_pair_the_loss_is_exactly_zero(lib, B, D, sim):
    u, v, _ = CH.case(B, D, "graded")
    out, scores, grads = run(u, v, torch.full((B,), 0.5), sim, up=UP)
    assert out.item() == 0.0 and torch.isfinite(scores).all()
    assert (grads[0] == 0).all() and (grads[1] == 0).all()


@pytest.mark.parametrize("sim", CH.SIMS)
def test_a_row_with_a_nan_label_takes_no_part(lib, sim):
    B, D, bad = 7, 34, 3
    u, v, y = CH.case(B, D, "graded")
    y = y.clone()
    y[bad] = NAN
    rows = torch.arange(B) != bad
    ref = CH.reference_of(u[rows], v[rows], y[rows], sim)
    assert ref[0].item() >= CH.MIN_REF_LOSS
    got = run(u, v, y, sim, up=UP)
    check(got, ref, D, f"NaN label {sim}", up=UP, rows=rows)
    assert (got[2][0][bad] == 0).all() and (got[2][1][bad] == 0).all()
    assert torch.isfinite(got[1][bad])                      # its score is still a score


def test_cos_with_a_zero_row_follows_the_clamp_of_normalize(lib):
    """F.normalize divides a zero row by 1e-12 and passes no gradient to its norm: score 0, gradient v_hat / 1e-12."""
    B, D, z = 5, 10, 2
    u, v, y = CH.case(B, D, "graded")
    u = u.clone()
    u[z] = 0
    loss, scores, gu, gv = CH.reference_of(u, v, y, "cos")
    assert gu[z].abs().max().item() > 1e8 and scores[z].item() == 0.0       # the clamp, and the row is in a pair
    out, sc, grads = run(u, v, y, "cos")
    ku, kv = grads[0].cpu().double(), grads[1].cpu().double()
    assert CH.value_error(out.item(), loss, D) <= 1.0 and CH.score_error(sc.cpu(), scores, D) <= 1.0
    torch.testing.assert_close(ku[z], gu[z], rtol=1e-4, atol=1e-4 * gu[z].abs().max().item())
    keep = torch.arange(B) != z                             # everything else without the huge entries in its tolerance
    assert CH.grad_error(ku[keep], gu[keep]) <= 1.0 and CH.grad_error(kv, gv) <= 1.0


@pytest.mark.parametrize("labels", ["smallest", "largest", "equal"])
@pytest.mark.parametrize("sim", CH.SIMS)
def test_a_nan_element_gives_a_nan_loss(lib, sim, labels):
    """Whatever the labels make of the row: first of every pair it is in, second of every pair, or in no pair at all."""
    B, D, bad = 7, 34, 4
    u, v, y = CH.case(B, D, "graded")
    u, y = u.clone(), y.clone()
    u[bad, 5] = NAN
    if labels == "equal":
        y[:] = 0.5
    else:
        y[bad] = -1.0 if labels == "smallest" else 2.0
    assert torch.isnan(CH.loss_ref(u.double(), v.double(), y, sim))         # as torch.logsumexp does
    out, _, _ = run(u, v, y, sim, want_grads=False)
    assert torch.isnan(out).all()


def test_angle_with_a_zero_row_gives_a_nan_loss(lib):
    u, v, y = CH.case(5, 10, "graded")
    v = v.clone()
    v[1] = 0
    assert torch.isnan(CH.loss_ref(u.double(), v.double(), y, "angle"))
    out, _, _ = run(u, v, y, "angle", want_grads=False)
    assert torch.isnan(out).all()


def saturated(sim):
    """Two rows whose scores lie 1.9 (cos) or 1.34 (angle) apart, row 0 the larger, and a scale that puts their difference
    past 88, where exp overflows fp32."""
    if sim == "cos":
        w = math.sqrt(1 - 0.95 ** 2)
        u = torch.tensor([[1.0, 0, 0, 0], [1.0, 0, 0, 0]])
        v = torch.tensor([[0.95, w, 0, 0], [-0.95, w, 0, 0]])
        return u, v, 60.0
    return torch.tensor([[1.0, 1.0], [1.0, -0.9]]), torch.tensor([[1.0, 0.0], [1.0, 0.0]]), 100.0


@pytest.mark.parametrize("sim", CH.SIMS)
def test_saturation(lib, sim):
    u, v, scale = saturated(sim)
    D = u.shape[1]
    # the larger score on the smaller label: d = scale * (s_0 - s_1) > 88, the loss is d and the gradients are +-scale ds/dx
    y = torch.tensor([0.0, 1.0])
    ref = CH.reference_of(u, v, y, sim, scale)
    assert ref[0].item() > 100
    got = run(u, v, y, sim, scale, up=UP)
    check(got, ref, D, f"saturated {sim}", up=UP)
    # the other order: exp(-d) is below fp32's range
    y = torch.tensor([1.0, 0.0])
    ref = CH.reference_of(u, v, y, sim, scale)
    got = run(u, v, y, sim, scale, up=UP)
    assert 0.0 <= got[0].item() < 1e-30
    check(got, ref, D, f"saturated the other way {sim}", up=UP)


# ------------------------------------------------------------------ 3. call discipline
def raw_call(lib, u, v, y, sim, out, scores, grad_out, gu, gv, ws=None, nbytes=None, scale=CH.SCALE, B=None, D=None):
    B = u.shape[0] if B is None else B
    D = u.shape[1] if D is None else D
    if ws is None:
        ws = torch.empty(max(lib.qst_cosent_workspace_bytes(u.shape[0], u.shape[1]), 16), dtype=torch.uint8, device="cuda")
        nbytes = ws.numel() if nbytes is None else nbytes
    return lib.qst_cosent_loss(ptr(u), ptr(v), ptr(y), B, D, SIM_CODE.get(sim, sim), scale, ptr(out), ptr(scores),
                               ptr(grad_out), ptr(gu), ptr(gv), ws if isinstance(ws, int) else ptr(ws), nbytes, stream())


def banded(n, band=64):
    """(whole, view): n floats with `band` NaN floats on either side, all NaN to begin with."""
    whole = torch.full((n + 2 * band,), NAN, device="cuda")
    return whole, whole[band:band + n]


def bands_untouched(whole, n, band=64):
    return bool(torch.isnan(whole[:band]).all() and torch.isnan(whole[band + n:]).all())


@pytest.mark.parametrize("sim", CH.SIMS)
@pytest.mark.parametrize("B,D", [(7, 34), (5, 264), (3, 2056)], ids=["element", "registers", "streamed"])
def test_forward_only_writes_its_outputs_and_nothing_else(lib, B, D, sim):
    u, v, y = [t.cuda() for t in CH.case(B, D, "graded")]
    (wo, out), (ws_, scores), (wu, gu), (wv, gv) = banded(1), banded(B), banded(B * D), banded(B * D)
    assert raw_call(lib, u, v, y, sim, out, scores, None, None, None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(scores).all() and out.item() > 0
    assert bands_untouched(wo, 1) and bands_untouched(ws_, B)
    assert torch.isnan(wu).all() and torch.isnan(wv).all()
    # with gradients: the bands around all four outputs stay
    assert raw_call(lib, u, v, y, sim, out, scores, None, gu, gv) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(gu).all() and torch.isfinite(gv).all()
    assert bands_untouched(wo, 1) and bands_untouched(ws_, B) and bands_untouched(wu, B * D) and bands_untouched(wv, B * D)
    # out_scores may be NULL
    assert raw_call(lib, u, v, y, sim, out, None, None, None, None) == 0


def test_bad_arguments_are_refused_and_write_nothing(lib):
    B, D = 7, 34
    u, v, y = [t.cuda() for t in CH.case(B, D, "graded")]
    out, scores = torch.full((1,), -7.25, device="cuda"), torch.full((B,), -7.25, device="cuda")
    gu, gv = torch.full_like(u, -7.25), torch.full_like(v, -7.25)
    nbytes = lib.qst_cosent_workspace_bytes(B, D)
    ws = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda")

    def call(u=u, v=v, y=y, sim="angle", out=out, gu=gu, gv=gv, ws=ws, nb=nbytes, **kw):
        kw = {**dict(B=B, D=D), **kw}                       # a NULL input has no shape to take them from
        return raw_call(lib, u, v, y, sim, out, scores, None, gu, gv, ws=ws, nbytes=nb, **kw)

    assert call() == 0 and call(sim="cos", D=33) == 0       # the arguments the bad ones are varied from are good
    torch.cuda.synchronize()
    out.fill_(-7.25), scores.fill_(-7.25), gu.fill_(-7.25), gv.fill_(-7.25), ws.zero_()
    bad = [dict(gu=None), dict(gv=None),                                        # exactly one NULL gradient
           dict(B=0), dict(B=-1), dict(D=0), dict(D=-2),
           dict(D=33),                                                          # an odd D with angle
           dict(u=None), dict(v=None), dict(y=None), dict(out=None),
           dict(nb=nbytes - 1), dict(nb=0), dict(ws=ws.data_ptr() + 4), dict(ws=ws.data_ptr() + 8),
           dict(sim=2), dict(sim=-1),
           dict(scale=0.0), dict(scale=-1.0), dict(scale=math.inf), dict(scale=math.nan)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert lib.qst_cosent_loss(ptr(u), ptr(v), ptr(y), B, D, S.PAIRSIM_ANGLE, CH.SCALE, ptr(out), ptr(scores), None, ptr(gu),
                               ptr(gv), None, nbytes, stream()) == -1           # a NULL workspace
    # B * D past 2^31 - 1 is refused as unsupported before anything is read
    assert call(B=65536, D=32768, nb=lib.qst_cosent_workspace_bytes(65536, 32768),
                ws=torch.zeros(lib.qst_cosent_workspace_bytes(65536, 32768), dtype=torch.uint8, device="cuda")) == -2
    torch.cuda.synchronize()
    assert (out == -7.25).all() and (scores == -7.25).all() and (gu == -7.25).all() and (gv == -7.25).all()
    assert not ws.any()
    assert lib.qst_cosent_workspace_bytes(0, 8) == 0 and lib.qst_cosent_workspace_bytes(8, 0) == 0


def test_workspace_of_exactly_the_queried_size_and_no_matrix(lib):
    B, D = 65, 768
    u, v, y = [t.cuda() for t in CH.case(B, D, "graded")]
    nbytes = lib.qst_cosent_workspace_bytes(B, D)
    assert nbytes >= 4 * B
    whole = torch.full((nbytes + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = whole[256:256 + nbytes]
    out, scores, gu, gv = torch.empty(1, device="cuda"), torch.empty(B, device="cuda"), torch.empty_like(u), torch.empty_like(v)
    assert raw_call(lib, u, v, y, "angle", out, scores, None, gu, gv, ws=ws, nbytes=nbytes - 1) == -1
    assert raw_call(lib, u, v, y, "angle", out, scores, None, gu, gv, ws=ws, nbytes=nbytes) == 0
    torch.cuda.synchronize()
    assert (whole[:256] == 0xA5).all() and (whole[256 + nbytes:] == 0xA5).all()         # nothing beyond what was asked for
    want, wsc, wg = S.cosent_loss_raw(u, v, y, "angle", CH.SCALE, want_grads=True)
    assert torch.equal(out, want) and torch.equal(scores, wsc) and torch.equal(gu, wg[0]) and torch.equal(gv, wg[1])
    # per-row scalars only: a B x B fp32 matrix at B = 4096 would be 64 MiB, this is under 64 bytes a row
    assert lib.qst_cosent_workspace_bytes(4096, 768) < 64 * 4096
    assert lib.qst_cosent_workspace_bytes(4096, 8) == lib.qst_cosent_workspace_bytes(4096, 768)
    assert lib.qst_cosent_workspace_bytes(8192, 768) < 2 * lib.qst_cosent_workspace_bytes(4096, 768) + 64


# ------------------------------------------------------------------ 4. device-side behaviour
BIG = (1030, 64)


@pytest.mark.parametrize("sim", CH.SIMS)
def test_two_identical_calls_are_bit_identical(lib, sim):
    for B, D in [BIG, (65, 768), (16, 5120)]:
        u, v, y = [t.cuda() for t in CH.case(B, D, "ties")]
        w = torch.tensor([UP], device="cuda")
        r1 = S.cosent_loss_raw(u, v, y, sim, CH.SCALE, grad_out=w, want_grads=True)
        r2 = S.cosent_loss_raw(u, v, y, sim, CH.SCALE, grad_out=w, want_grads=True)
        assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
        assert torch.equal(r1[2][0], r2[2][0]) and torch.equal(r1[2][1], r2[2][1])


@pytest.mark.parametrize("sim", CH.SIMS)
def test_non_default_stream_gives_the_same_result(lib, sim):
    u, v, y = [t.cuda() for t in CH.case(*BIG, "graded")]
    o1, s1, g1 = S.cosent_loss_raw(u, v, y, sim, CH.SCALE, want_grads=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        o2, s2, g2 = S.cosent_loss_raw(u, v, y, sim, CH.SCALE, want_grads=True)
    side.synchronize()
    assert torch.equal(o1, o2) and torch.equal(s1, s2) and torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])


@pytest.mark.parametrize("sim", CH.SIMS)
def test_grad_out_is_read_on_the_device_and_scales_the_gradients(lib, sim):
    """grad_out = 65536 (the first loss scale of use_amp) gives 65536 x the gradients of grad_out = NULL exactly, as a power
    of two does; 3 gives them within 1 ulp per element. The loss and the scores do not move."""
    u, v, y = [t.cuda() for t in CH.case(65, 768, "graded")]
    o1, s1, g1 = S.cosent_loss_raw(u, v, y, sim, CH.SCALE, want_grads=True)
    for scale in (65536.0, 3.0):
        og, sg, gg = S.cosent_loss_raw(u, v, y, sim, CH.SCALE, grad_out=torch.tensor([scale], device="cuda"), want_grads=True)
        assert torch.equal(o1, og) and torch.equal(s1, sg)
        for x1, xg in zip(g1, gg):
            want = scale * x1.double()
            ulp = torch.finfo(torch.float32).eps * want.abs().clamp_min(torch.finfo(torch.float32).tiny)
            assert ((xg.double() - want).abs() <= ulp).all()
            assert x1.abs().max().item() > 0


@pytest.mark.parametrize("sim", CH.SIMS)
def test_the_call_pair_is_capturable_in_a_graph(lib, sim):
    """No host synchronisation, grad_out read on the device: a captured forward + backward call pair replays on new inputs
    and a new upstream gradient written into the same buffers, with the bits of the eager calls. One stream, no branches."""
    (u1, v1, y1), (u2, v2, y2) = [[t.cuda() for t in CH.case(7, 34, "graded", seed)] for seed in (7034, 7035)]
    u, v, y, w = u1.clone(), v1.clone(), y1.clone(), torch.tensor([1.0], device="cuda")
    S.cosent_loss_raw(u, v, y, sim, CH.SCALE, grad_out=w, want_grads=True)      # code objects loaded first
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fwd, fscores, _ = S.cosent_loss_raw(u, v, y, sim, CH.SCALE)
        out, scores, grads = S.cosent_loss_raw(u, v, y, sim, CH.SCALE, grad_out=w, want_grads=True)
    u.copy_(u2), v.copy_(v2), y.copy_(y2), w.fill_(2.5)
    graph.replay()
    torch.cuda.synchronize()
    want, want_s, want_g = S.cosent_loss_raw(u2, v2, y2, sim, CH.SCALE, grad_out=torch.tensor([2.5], device="cuda"),
                                             want_grads=True)
    assert torch.equal(fwd, want) and torch.equal(out, want) and torch.equal(fscores, want_s) and torch.equal(scores, want_s)
    assert torch.equal(grads[0], want_g[0]) and torch.equal(grads[1], want_g[1])


@pytest.mark.parametrize("sim", CH.SIMS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_autograd_returns_gradients_in_the_input_dtypes(lib, dtype, sim):
    u0, v0, y = CH.case(8, 384, "graded")
    u0, v0, y = u0.cuda().to(dtype), v0.cuda().to(dtype), y.cuda()
    u, v = u0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
    loss = S.cosent_loss(u, v, y, 20.0, sim)
    assert loss.dim() == 0
    (loss * UP).backward()
    assert u.grad.dtype == dtype and v.grad.dtype == dtype
    out, _, grads = S.cosent_loss_raw(u0.float(), v0.float(), y, sim, 20.0, grad_out=torch.tensor([UP], device="cuda"),
                                      want_grads=True)
    assert torch.equal(loss.detach().reshape(1), out)
    assert torch.equal(u.grad, grads[0].to(dtype)) and torch.equal(v.grad, grads[1].to(dtype))


def test_the_function_refuses_what_the_kernel_would(lib):
    u, v, y = [t.cuda() for t in CH.case(5, 10, "graded")]
    with pytest.raises(ValueError, match="9"):
        S.cosent_loss(u[:, :9], v[:, :9], y, sim="angle")
    with pytest.raises(ValueError):
        S.cosent_loss(u, v, y, sim="dot")
    with pytest.raises(ValueError):
        S.cosent_loss(u, v, y, scale=0.0)
    with pytest.raises(ValueError):
        S.cosent_loss(u, v, y[:4])


# ------------------------------------------------------------------ 5. the classes on a real encoder
WORDS = "a man rides red horse two dogs play in park woman eats green apple near old bridge small cat sleeps".split()
CLASSES = [(S.CoSENTLoss, "cos"), (S.AnglELoss, "angle")]
CLASS_IDS = ["cosent", "angle"]


def sent(i, n):
    rng = np.random.RandomState(i)
    return list(rng.choice(WORDS, size=n))


def graded_pairs(n):
    """Pair i shares the first k = i % 10 of its nine words, the rest come from another sentence; the label is k / 9."""
    out = []
    for i in range(n):
        k = i % 10
        a, other = sent(i, 9), sent(1000 + i, 9)
        out.append(InputExample(texts=[" ".join(a), " ".join(a[:k] + other[k:])], label=k / 9))
    return out


class Tap(nn.Module):
    """The model, keeping hold of the sentence embeddings it returns (and of their gradients); `width` cuts them."""

    def __init__(self, model, width=None):
        super().__init__()
        self.model, self.cfg, self.seen, self.width = model, model.cfg, [], width

    def forward(self, feats):
        out = dict(self.model(feats))
        if self.width is not None:
            out["sentence_embedding"] = out["sentence_embedding"][:, :self.width]
        if out["sentence_embedding"].requires_grad:
            out["sentence_embedding"].retain_grad()
        self.seen.append(out["sentence_embedding"])
        return out


@pytest.fixture(scope="module")
def model():
    return SentenceTransformer("tiny-bert", device="cuda")


def batch_of(model, n=16):
    feats, labels = model.smart_batching_collate(graded_pairs(n))
    return [{key: v.cuda() for key, v in f.items()} for f in feats], labels.cuda()


def one_backward(model, lm, feats, labels):
    enc = model._enc
    enc.ensure_train_state()
    enc.grads.zero_()
    loss = lm([dict(f) for f in feats], labels)
    loss.backward()
    g = torch.cat([v.reshape(-1) for v in enc.grad_views().values()]).clone()
    enc.grads.zero_()
    return loss.detach(), g


@pytest.mark.parametrize("cls,sim", CLASSES, ids=CLASS_IDS)
def test_class_equals_torch_ops_on_the_same_embeddings(model, cls, sim):
    feats, labels = batch_of(model)
    model.train()
    tap = Tap(model)
    loss, _ = one_backward(model, cls(tap), feats, labels)
    assert len(tap.seen) == 1 and tap.seen[0].shape[0] == 32             # one fused pass for both columns
    emb = tap.seen[0]
    u64, v64 = emb.detach()[:16].double().requires_grad_(True), emb.detach()[16:].double().requires_grad_(True)
    ref = CH.loss_ref(u64, v64, labels.double(), sim)
    ref.backward()
    D = emb.shape[1]
    ev = CH.value_error(loss.item(), ref.item(), D)
    eg = CH.grad_error(emb.grad, torch.cat([u64.grad, v64.grad], 0))
    print(f"  {cls.__name__}: loss {loss.item():.7f} torch ops {ref.item():.7f}; share of the tolerance: value {ev:.3f} "
          f"embedding gradients {eg:.3f}")
    assert ref.item() > 1.0 and emb.grad.abs().max().item() > 0 and ev <= 1.0 and eg <= 1.0
    if sim == "angle":
        assert CH.angle_sim_ref(u64, v64).min().item() >= CH.MIN_ANGLE_SCORE


@pytest.mark.parametrize("cls,sim", CLASSES, ids=CLASS_IDS)
def test_a_foreign_similarity_fct_takes_the_torch_path_and_agrees(model, cls, sim):
    feats, labels = batch_of(model)
    model.train()
    calls = []

    def foreign(a, b):
        calls.append(tuple(a.shape))
        return CH.SIM_REF[sim](a, b)

    got = {}
    for name, make in (("kernel", lambda m: cls(m)), ("torch", lambda m: S.CoSENTLoss(m, similarity_fct=foreign))):
        tap = Tap(model)
        lm = make(tap)
        assert (lm._kernel_sim() is None) == (name == "torch")
        loss, g = one_backward(model, lm, feats, labels)
        got[name] = (loss, tap.seen[0].detach(), tap.seen[0].grad.clone(), g)
    (lk, ek, dk, gk), (lt, et, dt, gt) = got["kernel"], got["torch"]
    assert calls == [(16, ek.shape[1])] and torch.equal(ek, et)          # called once, on the same embeddings
    ev, eg = CH.value_error(lk.item(), lt.item(), ek.shape[1]), CH.grad_error(dk, dt)
    print(f"  {cls.__name__} kernel {lk.item():.7f} torch path {lt.item():.7f}: value {ev:.3f} embedding gradients {eg:.3f}")
    assert ev <= 1.0 and eg <= 1.0
    assert gk.norm().item() > 0 and (gk - gt).norm().item() <= 2e-2 * gk.norm().item()


def test_angle_loss_on_an_odd_width_raises(model):
    feats, labels = batch_of(model)
    model.eval()
    with pytest.raises(ValueError, match="63"), torch.no_grad():
        S.AnglELoss(Tap(model, width=63))(feats, labels)
    with torch.no_grad():                                    # the cosine does not mind
        assert torch.isfinite(S.CoSENTLoss(Tap(model, width=63))(feats, labels))


@pytest.mark.parametrize("cls,sim", CLASSES, ids=CLASS_IDS)
def test_inside_matryoshka_loss_equals_the_per_width_torch_composition(model, cls, sim):
    feats, labels = batch_of(model)
    model.train()
    tap = Tap(model)
    full = tap.model.get_sentence_embedding_dimension()
    dims, weights = [full, full // 2], [1.0, 0.5]
    loss, _ = one_backward(model, S.MatryoshkaLoss(tap.model, cls(tap), dims, weights), feats, labels)
    assert len(tap.seen) == 1                               # one encoder pass for both widths
    emb = tap.seen[0]
    u64, v64 = emb.detach()[:16].double().requires_grad_(True), emb.detach()[16:].double().requires_grad_(True)
    ref = sum(w * CH.loss_ref(F.normalize(u64[:, :d], p=2, dim=1), F.normalize(v64[:, :d], p=2, dim=1), labels.double(), sim)
              for d, w in zip(dims, weights))
    ref.backward()
    ev = CH.value_error(loss.item(), ref.item(), full)
    eg = CH.grad_error(emb.grad, torch.cat([u64.grad, v64.grad], 0))
    print(f"  Matryoshka({cls.__name__}): loss {loss.item():.7f} torch ops {ref.item():.7f}; share of the tolerance: "
          f"value {ev:.3f} embedding gradients {eg:.3f}")
    assert ref.item() > 1.0 and ev <= 1.0 and eg <= 1.0


@pytest.mark.parametrize("use_amp", [False, True])
@pytest.mark.parametrize("cls,sim", CLASSES, ids=CLASS_IDS)
def test_fit_lowers_the_loss_and_does_not_lower_spearman(cls, sim, use_amp):
    """5 epochs over 32 graded pairs; under use_amp the loss scale reaches the kernel as grad_out, a device scalar."""
    random.seed(11)
    m = SentenceTransformer("tiny-bert", device="cuda")          # a fresh model: amp schedule counters persist per model
    pairs = graded_pairs(32)
    lm = cls(m)
    feats, labels = m.smart_batching_collate(pairs)
    ev = EmbeddingSimilarityEvaluator.from_input_examples(pairs, batch_size=16, write_csv=False)

    def value():
        m.eval()
        with torch.no_grad():
            return lm([{k: v.cuda() for k, v in f.items()} for f in feats], labels.cuda()).item()

    before, rho_before = value(), ev(m)
    m.fit([(DataLoader(pairs, batch_size=8, shuffle=False), lm)], epochs=5, warmup_steps=0, scheduler="constantlr",
          optimizer_params={"lr": 1e-3}, dropout=0, use_amp=use_amp, show_progress_bar=False)
    after, rho_after = value(), ev(m)
    print(f"  fit {cls.__name__} amp={use_amp}: loss on the 32 pairs {before:.5f} -> {after:.5f}, Spearman "
          f"{rho_before:.4f} -> {rho_after:.4f}")
    assert np.isfinite(after) and after < before
    assert rho_after >= rho_before
    assert torch.isfinite(m._enc.params).all()
