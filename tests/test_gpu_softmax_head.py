"""GPU: the classifier kernels of losses.SoftmaxLoss (csrc/softmax_head.hip: qst_softmax_head_fwd, qst_softmax_ce,
qst_softmax_head_bwd) against the fp64 CPU reference of softmax_head_helpers, called through the C ABI.

Shapes: B crosses a partial last workgroup of four rows (1, 3, 5), the 64 rows up to which the weight gradient runs as one
slice (64) and several slices with an uneven last one (257); D takes every register form of row_loss.h's dispatch_form
(up to 256, 512, 768, 1024 and 2048 floats a row), among them widths that are no multiple of 256; C = 1, 2, 3, 8.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import softmax_head_helpers as SH  # noqa: E402
from kernel_helpers import lib, ptr, stream  # noqa: E402,F401

# (B, D, C, parts, reduction): not the full product -- every B, D, C and reduction of the lists above at least once, the
# widest row with the most classes and parts, the largest B on both sides of a wide and a narrow row
CASES = [(1, 4, 1, 7, "mean"), (3, 64, 2, 3, "mean"), (5, 260, 3, 7, "sum"), (64, 384, 3, 3, "mean"), (257, 64, 8, 7, "mean"),
         (5, 1024, 2, 5, "none"), (3, 2048, 8, 7, "mean"), (257, 384, 3, 3, "sum"), (65, 516, 3, 6, "none"),
         (64, 2048, 2, 4, "sum")]
CASES += [(5, 64, 3, p, "mean") for p in SH.ALL_PARTS if (5, 64, 3, p, "mean") not in CASES]


def dev(*ts):
    return [t.cuda().contiguous() for t in ts]


def run_fwd(lib, u, v, w, b, parts, st=None):
    (B, D), C = u.shape, w.shape[0]
    logits = torch.empty(B, C, device="cuda")
    assert lib.qst_softmax_head_fwd(ptr(u), ptr(v), ptr(w), ptr(b), B, D, C, parts, ptr(logits), st or stream()) == 0
    return logits


def run_ce(lib, logits, labels, reduction, ignore_index=-100, grad_out=None, grads=True, counts=False, st=None):
    B, C = logits.shape
    out = torch.empty(B if reduction == "none" else 1, device="cuda")
    dl = torch.empty(B, C, device="cuda") if grads else None
    cnt = torch.empty(2, dtype=torch.int64, device="cuda") if counts else None
    scratch = torch.empty(B + 2, device="cuda")
    assert lib.qst_softmax_ce(ptr(logits), ptr(labels), B, C, ignore_index, SH.RED[reduction], ptr(out), ptr(grad_out), ptr(dl),
                              ptr(cnt), ptr(scratch), st or stream()) == 0
    return out, dl, cnt


def run_bwd(lib, u, v, w, dl, parts, st=None):
    (B, D), C = u.shape, w.shape[0]
    gu, gv, gw, gb = torch.empty_like(u), torch.empty_like(v), torch.empty_like(w), torch.empty(C, device="cuda")
    nbytes = lib.qst_softmax_head_bwd_workspace_bytes(B, D, C, parts)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    assert lib.qst_softmax_head_bwd(ptr(u), ptr(v), ptr(w), ptr(dl), B, D, C, parts, ptr(gu), ptr(gv), ptr(gw), ptr(gb), ptr(ws),
                                    nbytes, st or stream()) == 0
    return gu, gv, gw, gb


def run_all(lib, u, v, w, b, labels, parts, reduction, st=None, **kw):
    logits = run_fwd(lib, u, v, w, b, parts, st)
    out, dl, cnt = run_ce(lib, logits, labels, reduction, st=st, **kw)
    return (logits, out, dl, cnt) + run_bwd(lib, u, v, w, dl, parts, st)


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("B,D,C,parts,reduction", CASES)
def test_kernels_match_the_reference(lib, B, D, C, parts, reduction):
    u, v, w, b, labels, ref_logits, ref_loss, ref_grads = SH.reference(B, D, C, parts, reduction)
    K = SH.nvec(parts) * D
    assert w.shape == (C, K)
    logits, out, dl, _, *grads = run_all(lib, *dev(u, v, w, b, labels), parts, reduction)
    el = SH.value_error(logits, ref_logits, K)
    ev = SH.value_error(out, ref_loss, K)
    eg = [SH.grad_error(g.cpu(), r) for g, r in zip(grads, ref_grads)]
    print(f"  B={B} D={D} C={C} parts={parts} {reduction}: share of the tolerance: logits {el:.3f} loss {ev:.3f} "
          f"grad u {eg[0]:.3f} v {eg[1]:.3f} w {eg[2]:.3f} b {eg[3]:.3f}")
    assert el <= 1.0 and ev <= 1.0 and max(eg) <= 1.0
    if C > 1:       # conditions on the test data: a softmax that is not saturated, gradients a wrong one cannot hide behind
        assert ref_loss.mean().item() > 0.05 and min(r.abs().max().item() for r in ref_grads) > 1e-4


def test_tied_rows_take_the_zero_gradient_of_abs(lib):
    """Rows with u == v exactly: d|u - v| at 0 is 0 (torch's sign), so neither sign of W's difference block may leak in."""
    B, D, C, parts = 6, 64, 3, SH.DIFF | SH.REP
    u, v, w, b, labels = SH.case(B, D, C, parts, 5, tied_rows=(1, 4))
    assert torch.equal(u[1], v[1]) and torch.equal(u[4], v[4])
    _, _, ref_grads = SH.reference_of(u, v, w, b, labels, parts, "mean")
    *_, gu, gv, gw, gb = run_all(lib, *dev(u, v, w, b, labels), parts, "mean")
    for g, r in zip((gu, gv, gw, gb), ref_grads):
        assert SH.grad_error(g.cpu(), r) <= 1.0
    # alone, the difference block gives such rows no gradient at all
    _, _, ref_d = SH.reference_of(u, v, w[:, 2 * D:].contiguous(), b, labels, SH.DIFF, "mean")
    *_, gu, gv, _, _ = run_all(lib, *dev(u, v, w[:, 2 * D:], b, labels), SH.DIFF, "mean")
    assert ref_d[0][1].abs().max().item() == 0.0
    assert gu[[1, 4]].abs().max().item() == 0.0 and gv[[1, 4]].abs().max().item() == 0.0
    assert gu[0].abs().max().item() > 0.0


# ------------------------------------------------------------------ 2. labels
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("ignore_index", [-100, 1])
def test_ignored_rows_contribute_nothing(lib, reduction, ignore_index):
    B, D, C, parts = 9, 64, 3, 3
    u, v, w, b, labels = SH.case(B, D, C, parts, 11)
    labels[[0, 3, 8]] = ignore_index
    assert 0 < int((labels != ignore_index).sum()) < B
    ref_logits, ref_loss, ref_grads = SH.reference_of(u, v, w, b, labels, parts, reduction, ignore_index)
    du, dv, dw, db, dy = dev(u, v, w, b, labels)
    logits = run_fwd(lib, du, dv, dw, db, parts)
    out, dl, cnt = run_ce(lib, logits, dy, reduction, ignore_index, counts=True)
    grads = run_bwd(lib, du, dv, dw, dl, parts)
    assert SH.value_error(out, ref_loss, 2 * D) <= 1.0
    for g, r in zip(grads, ref_grads):
        assert SH.grad_error(g.cpu(), r) <= 1.0
    assert dl[[0, 3, 8]].abs().max().item() == 0.0
    kept = labels != ignore_index
    assert cnt.tolist() == [int(kept.sum()), int((ref_logits.argmax(1) == labels)[kept].sum())]


def test_all_rows_ignored_is_nan_under_mean_and_zero_under_sum(lib):
    logits = torch.randn(5, 3, generator=torch.Generator().manual_seed(2)).cuda()
    labels = torch.full((5,), -100, dtype=torch.int64, device="cuda")
    mean, dl_mean, cnt = run_ce(lib, logits, labels, "mean", counts=True)
    total, dl_sum, _ = run_ce(lib, logits, labels, "sum")
    rows, _, _ = run_ce(lib, logits, labels, "none")
    assert math.isnan(mean.item()) and total.item() == 0.0 and rows.abs().max().item() == 0.0
    assert dl_sum.abs().max().item() == 0.0 and dl_mean.abs().max().item() == 0.0      # torch: zeros there too
    assert cnt.tolist() == [0, 0]
    assert math.isnan(torch.nn.functional.cross_entropy(logits.cpu(), labels.cpu()).item())


@pytest.mark.parametrize("bad", [3, 7, -5, 2 ** 40, -2 ** 40])
def test_an_out_of_range_label_is_nan_for_its_row_alone(lib, bad):
    B, C = 7, 3
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(B, C, generator=g).cuda()
    labels = torch.randint(0, C, (B,), generator=g).cuda()
    good = run_ce(lib, logits, labels, "none", counts=True)
    labels_bad = labels.clone()
    labels_bad[2] = bad
    got = run_ce(lib, logits, labels_bad, "none", counts=True)
    others = [r for r in range(B) if r != 2]
    assert math.isnan(got[0][2].item()) and torch.isnan(got[1][2]).all()
    assert torch.equal(got[0][others], good[0][others]) and torch.equal(got[1][others], good[1][others])
    assert got[2][0].item() == B - 1 and good[2][0].item() == B
    for red in ("sum", "mean"):
        out, dl, _ = run_ce(lib, logits, labels_bad, red)
        assert math.isnan(out.item()) and torch.isnan(dl[2]).all() and torch.isfinite(dl[others]).all()
    ref = torch.nn.functional.cross_entropy(logits.cpu().double(), labels.cpu(), reduction="none")
    assert SH.value_error(good[0], ref, C) <= 1.0


def test_counts_equal_the_argmax_of_the_reference(lib):
    B, D, C, parts = 257, 64, 8, 7
    u, v, w, b, labels, ref_logits, _, _ = SH.reference(B, D, C, parts, "mean")
    top2 = ref_logits.topk(2, dim=1).values
    assert (top2[:, 0] - top2[:, 1]).min().item() > 1e-3         # a condition on the test data: no near-ties
    labels = labels.clone()
    labels[5], labels[9], labels[200] = -100, C, -1
    logits = run_fwd(lib, *dev(u, v, w, b), parts)
    _, _, cnt = run_ce(lib, logits, labels.cuda(), "mean", grads=False, counts=True)
    valid = (labels >= 0) & (labels < C)
    hits = int((ref_logits.argmax(1) == labels)[valid].sum())
    assert 0 < hits < int(valid.sum())
    assert cnt.tolist() == [int(valid.sum()), hits]
    # equal logits: the lowest index is the prediction
    tied = torch.tensor([[1.0, 1.0, 0.5], [0.0, 2.0, 2.0], [3.0, 3.0, 3.0]], device="cuda")
    for y, want in (([0, 1, 0], 3), ([1, 2, 1], 0), ([0, 2, 2], 1)):
        _, _, cnt = run_ce(lib, tied, torch.tensor(y, device="cuda"), "sum", grads=False, counts=True)
        assert cnt.tolist() == [3, want]


# ------------------------------------------------------------------ 3. the calls themselves
@pytest.mark.parametrize("reduction", ["sum", "mean", "none"])
def test_grad_out_is_read_on_the_device_and_scales_every_gradient(lib, reduction):
    B, D, C, parts = 5, 64, 3, 7
    u, v, w, b, labels = dev(*SH.case(B, D, C, parts, 21))
    logits = run_fwd(lib, u, v, w, b, parts)
    _, dl1, _ = run_ce(lib, logits, labels, reduction)
    up = torch.full((B if reduction == "none" else 1,), 0.375, device="cuda")
    if reduction == "none":
        up *= torch.arange(1, B + 1, device="cuda")
    out = torch.empty(B if reduction == "none" else 1, device="cuda")
    dl = torch.empty(B, C, device="cuda")
    scratch = torch.empty(B + 2, device="cuda")
    call = lambda: lib.qst_softmax_ce(ptr(logits), ptr(labels), B, C, -100, SH.RED[reduction], ptr(out), ptr(up), ptr(dl),  # noqa: E731
                                      None, ptr(scratch), stream())
    assert call() == 0
    scale = (up.view(-1, 1) if reduction == "none" else up).clone()
    assert torch.equal(dl, dl1 * scale)                     # the upstream factor multiplies the finished gradient
    up *= 2.0                                               # the same pointer, another value on the device
    assert call() == 0
    assert torch.equal(dl, dl1 * (2.0 * scale))
    g1, g2 = run_bwd(lib, u, v, w, dl1, parts), run_bwd(lib, u, v, w, dl, parts)
    if reduction != "none":
        for a, c in zip(g1, g2):
            torch.testing.assert_close(c, a * 0.75, rtol=1e-5, atol=1e-7)
            assert a.abs().max().item() > 0


def test_a_forward_only_call_writes_nothing_else(lib):
    B, D, C, parts = 5, 64, 3, 7
    u, v, w, b, labels = dev(*SH.case(B, D, C, parts, 22))
    buf = torch.full((B * C + 8,), 7.5, device="cuda")
    assert lib.qst_softmax_head_fwd(ptr(u), ptr(v), ptr(w), ptr(b), B, D, C, parts, ptr(buf), stream()) == 0
    assert (buf[B * C:] == 7.5).all() and not (buf[:B * C] == 7.5).any()
    logits = buf[:B * C].view(B, C).clone()
    keep = [t.clone() for t in (u, v, w, b, labels, logits)]
    for reduction, n in (("mean", 1), ("sum", 1), ("none", B)):
        out = torch.full((n + 4,), 7.5, device="cuda")
        scratch = torch.full((B + 2 + 4,), 7.5, device="cuda")
        assert lib.qst_softmax_ce(ptr(logits), ptr(labels), B, C, -100, SH.RED[reduction], ptr(out), None, None, None,
                                  ptr(scratch), stream()) == 0
        assert (out[n:] == 7.5).all() and (scratch[B + 2:] == 7.5).all() and torch.isfinite(out[:n]).all()
        assert not (out[:n] == 7.5).any()
    # the backward writes its four gradients and nothing behind them
    dl = torch.randn(B, C, device="cuda")
    gs = [torch.full((n + 4,), 7.5, device="cuda") for n in (B * D, B * D, C * SH.nvec(parts) * D, C)]
    ws = torch.empty(16, dtype=torch.uint8, device="cuda")
    assert lib.qst_softmax_head_bwd_workspace_bytes(B, D, C, parts) == 0
    assert lib.qst_softmax_head_bwd(ptr(u), ptr(v), ptr(w), ptr(dl), B, D, C, parts, *[ptr(g) for g in gs], ptr(ws), 0,
                                    stream()) == 0
    for g, n in zip(gs, (B * D, B * D, C * SH.nvec(parts) * D, C)):
        assert (g[n:] == 7.5).all() and not (g[:n] == 7.5).any()
    for t, k in zip((u, v, w, b, labels, logits), keep):
        assert torch.equal(t, k)


def test_unsupported_shapes_and_bad_arguments_are_refused(lib):
    B, D, C, parts = 4, 64, 3, 7
    u, v, w, b, labels = dev(*SH.case(B, D, C, parts, 23))
    big = torch.zeros(16 * 4 * 2052, device="cuda")             # room for every shape asked for below
    sent = torch.full((64,), 7.5, device="cuda")
    fwd = lambda D=D, C=C, parts=parts, u=u, B=B: lib.qst_softmax_head_fwd(  # noqa: E731
        ptr(u), ptr(big), ptr(big), ptr(big), B, D, C, parts, ptr(sent), stream())
    bwd = lambda D=D, C=C, parts=parts: lib.qst_softmax_head_bwd(  # noqa: E731
        ptr(big), ptr(big), ptr(big), ptr(big), B, D, C, parts, ptr(sent), ptr(sent), ptr(sent), ptr(sent), ptr(big), 16, stream())
    for f in (fwd, bwd):
        assert f(C=9) == SH.UNSUPPORTED and f(D=6) == SH.UNSUPPORTED and f(D=2052) == SH.UNSUPPORTED
        assert f(parts=0) == SH.BAD_ARG and f(parts=8) == SH.BAD_ARG and f(C=0) == SH.BAD_ARG and f(D=0) == SH.BAD_ARG
    assert fwd(u=None) == SH.BAD_ARG and fwd(B=0) == SH.BAD_ARG
    assert fwd(u=big[1:]) == SH.BAD_ARG                          # not 16-byte aligned
    # a workspace smaller than the query asks for
    need = lib.qst_softmax_head_bwd_workspace_bytes(65, D, C, parts)
    assert need == 2 * C * (4 * D + 4) * 4 and lib.qst_softmax_head_bwd_workspace_bytes(64, D, C, parts) == 0
    assert lib.qst_softmax_head_bwd(ptr(big), ptr(big), ptr(big), ptr(big), 65, D, C, parts, ptr(sent), ptr(sent), ptr(sent),
                                    ptr(sent), ptr(big), need - 1, stream()) == SH.BAD_ARG
    logits = torch.zeros(B, C, device="cuda")
    ce = lambda B=B, C=C, red=2, out=sent, scratch=big: lib.qst_softmax_ce(  # noqa: E731
        ptr(logits), ptr(labels), B, C, -100, red, ptr(out), None, None, None, ptr(scratch), stream())
    assert ce(B=0) == SH.BAD_ARG and ce(C=0) == SH.BAD_ARG and ce(red=3) == SH.BAD_ARG and ce(red=-1) == SH.BAD_ARG
    assert ce(out=None) == SH.BAD_ARG and ce(scratch=None) == SH.BAD_ARG and ce(scratch=big[1:]) == SH.BAD_ARG
    torch.cuda.synchronize()
    assert (sent == 7.5).all()                                   # nothing was written


def test_two_calls_and_another_stream_give_the_same_bits(lib):
    B, D, C, parts = 257, 384, 3, 7
    xs = dev(*SH.case(B, D, C, parts, 24))
    first = run_all(lib, *xs, parts, "mean", counts=True)
    second = run_all(lib, *xs, parts, "mean", counts=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run_all(lib, *xs, parts, "mean", st=side.cuda_stream, counts=True)
    side.synchronize()
    for a, c, d in zip(first, second, third):
        assert torch.equal(a, c) and torch.equal(a, d)
