"""GPU: the kernels of models.Dense (csrc/dense_head.hip: qst_dense_head_fwd, qst_dense_head_bwd) against the fp64 CPU
reference of dense_head_helpers, called through the C ABI.

Shapes (dense_head_helpers.CASES): B crosses a partial row tile (1, 5), exactly one tile of 64 rows, one past it, and 257 rows:
five weight-gradient slices with an uneven last one; Din is below one K panel of 16 (4), no multiple of 16 (20, 260), aligned
(64, 384); Dout gives edge column tiles (1, 3), one tile, one past it and a row norm that crosses column tiles (200). Every one
of them meets both activations, with and without the normalisation, with and without a bias.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import dense_head_helpers as H  # noqa: E402
from kernel_helpers import lib, ptr, stream  # noqa: E402,F401


def dev(*ts):
    return [None if t is None else t.cuda().contiguous() for t in ts]


def same(a, c):
    return (a is None and c is None) or torch.equal(a, c)


# ------------------------------------------------------------------ 1. parity
def test_the_case_list_covers_every_size_under_every_setting():
    for act in (H.TANH, H.IDENTITY):
        for pick, values in ((0, H.BS), (1, H.DINS), (2, H.DOUTS)):
            for flag in (4, 5):             # normalize, bias
                for on in (0, 1):
                    assert {c[pick] for c in H.CASES if c[3] == act and c[flag] == on} >= set(values)
    assert (257, 384, 200, H.TANH, 1, 1) in H.CASES and (65, 260, 65, H.IDENTITY, 0, 0) in H.CASES


@pytest.mark.parametrize("B,Din,Dout,act,normalize,bias", H.CASES)
def test_kernels_match_the_reference(lib, B, Din, Dout, act, normalize, bias):
    x, w, b, dy, z, a, ref_y, *ref_grads = H.reference(B, Din, Dout, act, normalize, bias)
    assert H.conditions_of(z, a, ref_grads, act, normalize, Dout) == []
    y, norm, gx, gw, gb = H.run_all(lib, *dev(x, w, b, dy), act, normalize, stream())
    ey = H.value_error(y, ref_y, Din)
    en = H.value_error(norm, a.norm(dim=1), Din) if normalize else 0.0
    eg = [H.grad_error(g.cpu(), r) for g, r in zip((gx, gw, gb), ref_grads) if r is not None]
    print(f"  B={B} Din={Din} Dout={Dout} act={act} normalize={normalize} bias={bias}: share of the tolerance: y {ey:.3f} "
          f"norm {en:.3f} grads " + " ".join(f"{e:.3f}" for e in eg))
    assert (gb is None) == (not bias) and len(eg) == 2 + bias
    assert ey <= 1.0 and en <= 1.0 and max(eg) <= 1.0


# ------------------------------------------------------------------ 2. the calls themselves
@pytest.mark.parametrize("offset", [4, 1])      # the block starts on a 16-byte boundary, or not
def test_a_column_block_of_a_wider_buffer_gives_the_bits_of_the_contiguous_input(lib, offset):
    B, Din, Dout, act, normalize = 65, 260, 65, H.TANH, 1
    x, w, b, dy = dev(*H.case(B, Din, Dout, True, 31))
    wide = torch.full((B, Din + 12), float("nan"), device="cuda")
    wide[:, offset:offset + Din] = x
    block = wide[:, offset:offset + Din]
    assert block.stride(0) == Din + 12 and block.data_ptr() == wide.data_ptr() + 4 * offset
    plain = H.run_all(lib, x, w, b, dy, act, normalize, stream())
    strided = H.run_all(lib, block, w, b, dy, act, normalize, stream())
    assert all(torch.isfinite(t).all() for t in plain)
    for p, s in zip(plain, strided):
        assert torch.equal(p, s)


def test_two_runs_nan_filled_outputs_and_another_stream_give_the_same_bits(lib):
    B, Din, Dout, act, normalize = 257, 384, 200, H.TANH, 1
    x, w, b, dy = dev(*H.case(B, Din, Dout, True, 32))
    first = H.run_all(lib, x, w, b, dy, act, normalize, stream())
    second = H.run_all(lib, x, w, b, dy, act, normalize, stream())
    # written, not accumulated: outputs that held NaN come back finite and the same
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")  # noqa: E731
    y, norm = H.run_fwd(lib, x, w, b, act, normalize, stream(), y=nan(B, Dout), norm=nan(B))
    third = [y, norm, *H.run_bwd(lib, x, w, y, norm, dy, act, normalize, True, stream(),
                                 outs=(nan(B, Din), nan(Dout, Din), nan(Dout)))]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fourth = H.run_all(lib, x, w, b, dy, act, normalize, side.cuda_stream)
    side.synchronize()
    for a, c, d, e in zip(first, second, third, fourth):
        assert torch.isfinite(a).all() and a.abs().max().item() > 0
        assert torch.equal(a, c) and torch.equal(a, d) and torch.equal(a, e)


def test_a_zero_row_sits_on_the_clamp_of_normalize_without_a_nan(lib):
    B, Din, Dout = 6, 20, 3
    x, w, _, dy = H.case(B, Din, Dout, False, 33)
    x[2] = 0.0
    others = [r for r in range(B) if r != 2]
    for act in (H.TANH, H.IDENTITY):
        _, _, ref_y, ref_gx, ref_gw, _ = H.reference_of(x, w, None, dy, act, 1)
        assert torch.isfinite(ref_gx).all() and ref_y[2].abs().max().item() == 0.0
        y, norm, gx, gw, gb = H.run_all(lib, *dev(x, w, None, dy), act, 1, stream())
        assert gb is None
        assert y[2].abs().max().item() == 0.0 and norm[2].item() == 0.0
        assert all(torch.isfinite(t).all() for t in (y, norm, gx, gw))
        assert H.value_error(y, ref_y, Din) <= 1.0
        # the clamped row's gradient is dy / 1e-12 through W (torch's clamp_min passes nothing to the norm): its own scale
        assert H.grad_error(gx[others].cpu(), ref_gx[others]) <= 1.0 and H.grad_error(gx[2].cpu(), ref_gx[2]) <= 1.0
        assert ref_gx[2].abs().max().item() > 1e9
        assert H.grad_error(gw.cpu(), ref_gw) <= 1.0                # x = 0: the row adds nothing to the weight gradient


def test_a_backward_writes_its_gradients_and_nothing_behind_them(lib):
    B, Din, Dout = 5, 20, 3
    x, w, b, dy = dev(*H.case(B, Din, Dout, True, 34))
    ybuf, nbuf = torch.full((B * Dout + 8,), 7.5, device="cuda"), torch.full((B + 8,), 7.5, device="cuda")
    y, norm = H.run_fwd(lib, x, w, b, H.TANH, 1, stream(), y=ybuf[:B * Dout].view(B, Dout), norm=nbuf[:B])
    assert (ybuf[B * Dout:] == 7.5).all() and (nbuf[B:] == 7.5).all() and not (ybuf[:B * Dout] == 7.5).any()
    sizes = (B * Din, Dout * Din, Dout)
    bufs = [torch.full((n + 8,), 7.5, device="cuda") for n in sizes]
    keep = [t.clone() for t in (x, w, b, dy, y, norm)]
    H.run_bwd(lib, x, w, y, norm, dy, H.TANH, 1, True, stream(),
              outs=(bufs[0][:sizes[0]].view(B, Din), bufs[1][:sizes[1]].view(Dout, Din), bufs[2][:Dout]))
    for g, n in zip(bufs, sizes):
        assert (g[n:] == 7.5).all() and not (g[:n] == 7.5).any()
    for t, k in zip((x, w, b, dy, y, norm), keep):
        assert torch.equal(t, k)


def test_unsupported_shapes_and_bad_arguments_are_refused(lib):
    B, Din, Dout = 4, 20, 3
    # every buffer has room for the largest shape asked for below (4 x 8193), so a check that let one through would still
    # write inside it
    big = torch.zeros(4 * (H.MAX_DIM + 1) + 64, device="cuda")
    sents = [torch.full((4 * (H.MAX_DIM + 1) + 64,), 7.5, device="cuda") for _ in range(4)]
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    P, (s0, s1, s2, s3) = ptr(big), [ptr(s) for s in sents]

    def fwd(x=P, ldx=Din, w=P, b=P, B=B, Din=Din, Dout=Dout, act=H.TANH, normalize=1, y=s0, norm=s1):
        return lib.qst_dense_head_fwd(x, ldx, w, b, B, Din, Dout, act, normalize, y, norm, stream())

    def bwd(x=P, ldx=Din, w=P, y=P, norm=P, dy=P, B=B, Din=Din, Dout=Dout, act=H.TANH, normalize=1, gx=s0, gw=s1, gb=s2,
            wsp=ptr(ws), nbytes=ws.numel()):
        return lib.qst_dense_head_bwd(x, ldx, w, y, norm, dy, B, Din, Dout, act, normalize, gx, gw, gb, wsp, nbytes, stream())

    for f in (fwd, bwd):
        assert f(Din=0) == H.UNSUPPORTED and f(Din=H.MAX_DIM + 1, ldx=H.MAX_DIM + 1) == H.UNSUPPORTED
        assert f(Dout=0) == H.UNSUPPORTED and f(Dout=H.MAX_DIM + 1) == H.UNSUPPORTED and f(B=0) == H.UNSUPPORTED
        assert f(x=None) == H.BAD_ARG and f(w=None) == H.BAD_ARG and f(y=None) == H.BAD_ARG
        assert f(ldx=Din - 1) == H.BAD_ARG
        assert f(act=2) == H.BAD_ARG and f(act=-1) == H.BAD_ARG
        assert f(normalize=2) == H.BAD_ARG and f(normalize=-1) == H.BAD_ARG
        assert f(norm=None) == H.BAD_ARG                       # required with normalize ...
    assert bwd(dy=None) == H.BAD_ARG and bwd(gx=None) == H.BAD_ARG and bwd(gw=None) == H.BAD_ARG
    need = lib.qst_dense_head_bwd_workspace_bytes(B, Din, Dout)
    assert need == B * 4 * 4                                    # dz alone: one slice up to 64 rows
    assert bwd(wsp=None) == H.BAD_ARG and bwd(nbytes=need - 1) == H.BAD_ARG and bwd(wsp=ptr(ws) + 4) == H.BAD_ARG
    big_need = lib.qst_dense_head_bwd_workspace_bytes(257, Din, Dout)
    assert big_need == (257 * 4 + 5 * Dout * Din + 5 * 4) * 4   # dz, five slices of partial weight and bias sums
    assert bwd(B=257, nbytes=big_need - 1) == H.BAD_ARG
    for bad in ((0, Din, Dout), (B, 0, Dout), (B, Din, 0), (B, H.MAX_DIM + 1, Dout), (B, Din, H.MAX_DIM + 1)):
        assert lib.qst_dense_head_bwd_workspace_bytes(*bad) == 0
    torch.cuda.synchronize()
    assert all((s == 7.5).all() for s in sents)                 # nothing was written
    # ... and the largest widths, a NULL bias and a NULL row_norm without normalize are all accepted
    assert fwd(b=None, normalize=0, norm=None) == 0
    assert bwd(normalize=0, norm=None, gb=None, nbytes=need) == 0
    assert fwd(B=1, Din=H.MAX_DIM, ldx=H.MAX_DIM, Dout=3) == 0 and fwd(B=1, Din=4, ldx=4, Dout=H.MAX_DIM) == 0
    torch.cuda.synchronize()
