"""Row kernels that every forward and backward runs, each against a plain reference of the same operation: the embedding
gather + LayerNorm (all its forms), position ids and the forward prologue, the 16-bit weight shadows and the batched
LayerNorm reduction. Gathers, copies and roundings are compared bit for bit; fp32 arithmetic against fp64."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib  # noqa: E402
from oracle import dropout_ref as D  # noqa: E402
from oracle import torch_ref as R  # noqa: E402
from kernel_helpers import OPDT, drop_desc, drop_state, kf, lib, op, ptr, stage_major, stream  # noqa: E402,F401

BAD_ARG, UNSUPPORTED = -1, -2
ARCH_BERT, ARCH_MPNET, ARCH_ROBERTA = 0, 1, 2
MANT = {"bf16": 7, "f16": 10}                  # explicit significand bits of the operand type
F16_MAX = 65504.0


def bits(t):
    """the raw 16-bit patterns of a bf16 / f16 tensor (compares NaN sentinels and signed zeros exactly)"""
    return t.view(torch.int16)


def to_op(op, x):
    """round-to-nearest-even of fp32 x to the operand type, as the forward kernels store it: f16 saturates at +-65,504
    (DESIGN: forward kernels saturate) where torch's conversion overflows to inf"""
    y = x.to(OPDT[op])
    if op == "f16":
        y = torch.where(torch.isinf(y) & torch.isfinite(x), torch.copysign(torch.full_like(y, F16_MAX), y), y)
    return y


def op_ulp(op, x):
    """spacing of the operand type at |x| (its subnormal spacing below the normal range)"""
    x = x.abs().double()
    e = torch.frexp(x.clamp_min(1e-300)).exponent - 1              # floor(log2 |x|)
    emin = -14 if op == "f16" else -126
    return torch.ldexp(torch.ones_like(x), e.clamp_min(emin) - MANT[op])


# ------------------------------------------------------------------ position ids
def hf_position_ids(ids, arch, pad_id):
    """HF create_position_ids_from_input_ids (MPNet / RoBERTa): cumsum of the non-pad mask times the mask, plus pad_id;
    BERT: arange over every row (padding ignored)."""
    if arch == ARCH_BERT:
        return torch.arange(ids.shape[1]).expand_as(ids).to(torch.int32)
    m = ids.ne(pad_id).int()
    return (torch.cumsum(m, dim=1).type_as(m) * m + pad_id).to(torch.int32)


def padded_ids(nseq, L, pad_id, g, vocab=50):
    """rows of five kinds in turn: right-padded, left-padded, pad tokens mid-row, all padding, no padding. Non-pad tokens
    include the OTHER small id (0 when pad_id = 1), which must not count as padding."""
    ids = torch.randint(0, vocab, (nseq, L), generator=g)
    ids[ids == pad_id] = pad_id + 2
    for s in range(nseq):
        kind = (s + L) % 5
        k = int(torch.randint(1, L + 1, (1,), generator=g))
        keep_one = 1 if (k == L and L > 1) else 0
        if kind == 0:
            ids[s, L - k + keep_one:] = pad_id
        elif kind == 1:
            ids[s, : k - keep_one] = pad_id
        elif kind == 2:
            ids[s, torch.rand(L, generator=g) < 0.3] = pad_id
            if L > 2:
                ids[s, 0] = 1 - pad_id                              # a non-pad token, then pads and tokens mixed
        elif kind == 3:
            ids[s] = pad_id
    return ids


@pytest.mark.parametrize("nseq", [1, 64, 65, 130])
@pytest.mark.parametrize("L", [1, 7, 512])
@pytest.mark.parametrize("pad_id", [0, 1])
def test_position_ids_match_hf(lib, nseq, L, pad_id):
    """qst_position_ids for all three architectures against HF's rule, exactly: rows of every padding kind, more than one
    64-sequence workgroup."""
    g = torch.Generator().manual_seed(nseq * 1000 + L * 2 + pad_id)
    ids = padded_ids(nseq, L, pad_id, g)
    idd = ids.cuda()
    for arch in (ARCH_BERT, ARCH_MPNET, ARCH_ROBERTA):
        pos = torch.full((nseq, L), -7, dtype=torch.int32, device="cuda")
        _lib.check(lib.qst_position_ids(idd.data_ptr(), nseq, L, arch, pad_id, pos.data_ptr(), stream()))
        assert torch.equal(pos.cpu(), hf_position_ids(ids, arch, pad_id)), f"arch {arch}"


@pytest.mark.parametrize("nseq", [1, 64, 65, 130])
def test_forward_prologue_advances_the_dropout_step_once(lib, nseq):
    """qst_forward_prologue: the position ids of qst_position_ids, plus exactly one advance of the step word (word 2, with
    uint32 wrap-around) and a snapshot of the advanced state, whatever the number of workgroups."""
    L, pad_id = 33, 1
    g = torch.Generator().manual_seed(nseq)
    ids = padded_ids(nseq, L, pad_id, g)
    idd = ids.cuda()
    pos = torch.empty(nseq, L, dtype=torch.int32, device="cuda")
    for w2 in (41, -1):                                         # -1 = 0xFFFFFFFF: the advance wraps to 0
        state = torch.tensor([11, 22, w2, 99], dtype=torch.int32, device="cuda")
        snap = torch.full((4,), -5, dtype=torch.int32, device="cuda")
        _lib.check(lib.qst_forward_prologue(idd.data_ptr(), nseq, L, ARCH_ROBERTA, pad_id, pos.data_ptr(), state.data_ptr(),
                                            snap.data_ptr(), stream()))
        want = [11, 22, 42 if w2 == 41 else 0, 99]
        assert state.cpu().tolist() == want
        assert snap.cpu().tolist() == want
        assert torch.equal(pos.cpu(), hf_position_ids(ids, ARCH_ROBERTA, pad_id))
    # one of the two state pointers alone is refused (nothing launched)
    assert lib.qst_forward_prologue(idd.data_ptr(), nseq, L, ARCH_MPNET, pad_id, pos.data_ptr(), state.data_ptr(), None,
                                    stream()) == BAD_ARG
    assert lib.qst_forward_prologue(idd.data_ptr(), nseq, L, ARCH_MPNET, pad_id, pos.data_ptr(), None, snap.data_ptr(),
                                    stream()) == BAD_ARG
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [11, 22, 0, 99]


# ------------------------------------------------------------------ embedding gather + LayerNorm
def embed_inputs(M, H, g, vocab=1000, types="ids", pad_id=1, gamma_big_col=None):
    """ids with vocab - 1 and a heavily repeated id; RoBERTa-style position ids (rows of 13 tokens with padding: they start at
    pad_id + 1 and differ from row to row); types: "ids" (a two-row table and type ids), "null" (the table, type_ids NULL:
    row 0 for every token -- HF's all-zero token_type_ids), "none" (no table: MPNet)."""
    Ls = 13
    rows = padded_ids((M + Ls - 1) // Ls, Ls, pad_id, g, vocab)
    pos = hf_position_ids(rows, ARCH_ROBERTA, pad_id).reshape(-1)[:M].contiguous()
    ids = rows.reshape(-1)[:M].clone()
    ids[M // 2:: 7] = vocab - 1
    ids[: M // 4] = 17
    ids[-1] = vocab - 1
    word = torch.randn(vocab, H, generator=g)
    pe = torch.randn(int(pos.max()) + 1, H, generator=g) * 0.5
    te = torch.randn(2, H, generator=g) * 0.5 if types != "none" else None
    tid = torch.randint(0, 2, (M,), generator=g) if types == "ids" else None
    gamma = 1 + 0.1 * torch.randn(H, generator=g)
    beta = 0.1 * torch.randn(H, generator=g)
    if gamma_big_col is not None:
        gamma[gamma_big_col] = 1e5
    return dict(ids=ids, tid=tid, pos=pos, word=word, pe=pe, te=te, gamma=gamma, beta=beta)


def embed_sum_ref(x):
    """fp32, HF's order: (word + type) + position"""
    s = x["word"][x["ids"]]
    if x["te"] is not None:
        s = s + (x["te"][x["tid"]] if x["tid"] is not None else x["te"][0].expand_as(s))
    return s + x["pe"][x["pos"].long()]


def ln_ref64(s, gamma, beta, eps):
    s64 = s.double()
    mean = s64.mean(-1, keepdim=True)
    var = ((s64 - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (s64 - mean) * rstd
    return xhat * gamma.double() + beta.double(), xhat, rstd.squeeze(-1), mean


class Emb:
    """device copies of embed_inputs, kept alive across the launches"""

    def __init__(self, x):
        self.d = {k: (v.cuda().contiguous() if v is not None else None) for k, v in x.items()}

    def args(self):
        d = self.d
        return (ptr(d["ids"]), ptr(d["tid"]), ptr(d["pos"]), ptr(d["word"]), ptr(d["pe"]), ptr(d["te"]), ptr(d["gamma"]), ptr(d["beta"]))


def outs(M, H, op="bf16"):
    return (torch.full((M, H), float("nan"), device="cuda"), torch.empty(M, H, dtype=OPDT[op], device="cuda"),
            torch.empty(M, H, dtype=OPDT[op], device="cuda"), torch.full((M,), float("nan"), device="cuda"))


def check_ln_outputs(op, y, yb, xh, rs, s, gamma, beta, eps):
    """y within 1e-5 of fp64; rstd within 1e-5 relative; yb = the RNE (saturating) rounding of y itself; xhat within one
    operand ulp of fp64 x-hat. Both y and xhat also carry the error of the fp32 x - mean: a few fp32 ulps of (|x| + |mean|)
    * rstd. It is far below the bounds except in a row whose values nearly agree (|mean| * rstd large: at H = 2, two
    close values), where fp32 LayerNorm is ill-conditioned; that term is added to both bounds."""
    yr, xr, rr, mean = ln_ref64(s, gamma, beta, eps)
    y, yb, xh, rs = y.cpu(), yb.cpu(), xh.cpu(), rs.cpu()
    fp32_term = 8 * 2.0 ** -24 * (s.double().abs() + mean.abs()) * rr[:, None]
    yerr = (y.double() - yr).abs()
    ybound = 1e-5 + 1e-5 * yr.abs() + gamma.double().abs() * fp32_term
    assert bool((yerr <= ybound).all()), f"y off by {float((yerr / ybound).max()):.2f} of its bound"
    torch.testing.assert_close(rs.double(), rr, rtol=1e-5, atol=0)
    assert torch.equal(bits(yb), bits(to_op(op, y))), "16-bit copy of y is not the RNE rounding of y"
    err = (xh.double() - xr).abs()
    bound = op_ulp(op, xr) + fp32_term
    assert bool((err <= bound).all()), f"xhat off by {float((err / bound).max()):.2f} of its bound"


@pytest.mark.parametrize("M", [1, 3, 37, 4099])
@pytest.mark.parametrize("H", [2, 64, 100, 312, 640, 896, 1000, 1024])
def test_embed_ln_fwd_matches_fp64(lib, op, M, H):
    """qst_embed_ln_fwd against the fp32 HF-order sum and an fp64 LayerNorm, with a type table and type ids, with the table
    and NULL type ids (= row 0, bit for bit the same as explicit zeros), and without a table. H = 640 / 896 / 1000 / 100 / 2
    leave lanes idle (640 and 896 run the VPL 6 / VPL 8 kernels with masked tails)."""
    eps = 1e-12
    for types in ("ids", "null", "none"):
        g = torch.Generator().manual_seed(M * 7 + H)
        x = embed_inputs(M, H, g, types=types)
        e = Emb(x)
        y, yb, xh, rs = outs(M, H, op)
        _lib.check(kf(lib, "qst_embed_ln_fwd", op)(*e.args(), eps, M, H, y.data_ptr(), yb.data_ptr(), xh.data_ptr(),
                                                   rs.data_ptr(), stream()))
        check_ln_outputs(op, y, yb, xh, rs, embed_sum_ref(x), x["gamma"], x["beta"], eps)
        if types == "null":
            zeros = torch.zeros(M, dtype=torch.int64, device="cuda")
            y2, yb2, xh2, rs2 = outs(M, H, op)
            a = list(e.args())
            a[1] = zeros.data_ptr()
            _lib.check(kf(lib, "qst_embed_ln_fwd", op)(*a, eps, M, H, y2.data_ptr(), yb2.data_ptr(), xh2.data_ptr(),
                                                       rs2.data_ptr(), stream()))
            assert torch.equal(y2, y) and torch.equal(bits(yb2), bits(yb)) and torch.equal(bits(xh2), bits(xh))
            assert torch.equal(rs2, rs)


def test_embed_ln_fwd_f16_saturates_the_16bit_copy(lib):
    """f16: a gamma column of 1e5 drives the output past 65,504. The 16-bit copy saturates to +-65,504 (forward kernels
    saturate), never inf; y keeps the true value."""
    eps = 1e-12
    for M, H in ((37, 64), (300, 640), (64, 896)):
        g = torch.Generator().manual_seed(M + H)
        x = embed_inputs(M, H, g, gamma_big_col=H // 3)
        e = Emb(x)
        y, yb, xh, rs = outs(M, H, "f16")
        _lib.check(lib.qst_embed_ln_fwd_f16(*e.args(), eps, M, H, y.data_ptr(), yb.data_ptr(), xh.data_ptr(), rs.data_ptr(),
                                            stream()))
        check_ln_outputs("f16", y, yb, xh, rs, embed_sum_ref(x), x["gamma"], x["beta"], eps)
        assert bool(torch.isfinite(yb.float()).all())
        col = yb[:, H // 3].float().cpu()
        big = y[:, H // 3].abs().cpu() > F16_MAX + 16                # past the last value that rounds down to 65,504
        assert bool(big.any()) and bool((col[big].abs() == F16_MAX).all())


@pytest.mark.parametrize("M,H", [(1, 2), (37, 100), (300, 640), (129, 896), (1000, 1024)])
def test_embed_ln_fwd_drop_matches_the_oracle_masks(lib, op, M, H):
    """qst_embed_ln_fwd_drop: y = the undropped output times oracle/dropout_ref's mask, bit for bit (and within 1e-5 of fp64
    times the mask); the 16-bit copy rounds the dropped value; xhat / rstd are those of the undropped row."""
    eps, seed, step, prob = 1e-12, 2024, 3, 0.1
    g = torch.Generator().manual_seed(M + H)
    x = embed_inputs(M, H, g)
    e = Emb(x)
    st = drop_state(lib, seed, step)
    mk = torch.from_numpy(D.multipliers(seed, step, D.SITE_EMBED, M * H, prob).reshape(M, H))
    y0, yb0, xh0, rs0 = outs(M, H, op)
    _lib.check(kf(lib, "qst_embed_ln_fwd", op)(*e.args(), eps, M, H, y0.data_ptr(), yb0.data_ptr(), xh0.data_ptr(),
                                               rs0.data_ptr(), stream()))
    y1, yb1, xh1, rs1 = outs(M, H, op)
    _lib.check(kf(lib, "qst_embed_ln_fwd_drop", op)(*e.args(), eps, M, H, y1.data_ptr(), yb1.data_ptr(), xh1.data_ptr(),
                                                    rs1.data_ptr(), drop_desc(st, D.SITE_EMBED, prob), stream()))
    y0c, y1c = y0.cpu(), y1.cpu()
    assert torch.equal(y1c, y0c * mk)
    assert torch.equal(bits(yb1.cpu()), bits(to_op(op, y1c)))
    assert torch.equal(bits(xh1), bits(xh0)) and torch.equal(rs1, rs0)
    yr = ln_ref64(embed_sum_ref(x), x["gamma"], x["beta"], eps)[0]
    torch.testing.assert_close(y1c.double(), yr * mk.double(), rtol=1e-5, atol=1e-5 * float(mk.max()))


def mx_outs(M, H):
    return (torch.empty(M, H, dtype=torch.uint8, device="cuda"),
            torch.zeros((H + 127) // 128 * M * 4, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("M,H", [(1, 64), (37, 640), (300, 896), (129, 1024), (1000, 384)])
def test_mx_train_layernorms_equal_the_plain_kernels(lib, M, H):
    """qst_embed_ln_fwd_mx_train / qst_ln_fwd_mx_train (fp8 training forward): y, the bf16 copy, xhat and rstd bit for bit those
    of qst_embed_ln_fwd(_drop) / qst_ln_fwd; the MXFP8 copy bit for bit what mx_quant makes of its own bf16 copy (stage-major
    scales) -- without and with dropout."""
    eps, seed, step, prob = 1e-12, 77, 5, 0.1
    g = torch.Generator().manual_seed(M * 3 + H)
    x = embed_inputs(M, H, g)
    e = Emb(x)
    st = drop_state(lib, seed, step)
    for dropping in (False, True):
        d = drop_desc(st, D.SITE_EMBED, prob) if dropping else None
        y0, yb0, xh0, rs0 = outs(M, H)
        if dropping:
            _lib.check(lib.qst_embed_ln_fwd_drop(*e.args(), eps, M, H, y0.data_ptr(), yb0.data_ptr(), xh0.data_ptr(),
                                                 rs0.data_ptr(), d, stream()))
            d = C.byref(d)                                      # (the _mx_train binding takes the descriptor as void*)
        else:
            _lib.check(lib.qst_embed_ln_fwd(*e.args(), eps, M, H, y0.data_ptr(), yb0.data_ptr(), xh0.data_ptr(), rs0.data_ptr(),
                                            stream()))
        y1, yb1, xh1, rs1 = outs(M, H)
        yq, ys = mx_outs(M, H)
        _lib.check(lib.qst_embed_ln_fwd_mx_train(*e.args(), eps, M, H, y1.data_ptr(), yb1.data_ptr(), xh1.data_ptr(),
                                                 rs1.data_ptr(), yq.data_ptr(), ys.data_ptr(), d, stream()))
        assert torch.equal(y1, y0) and torch.equal(bits(yb1), bits(yb0)) and torch.equal(bits(xh1), bits(xh0))
        assert torch.equal(rs1, rs0)
        qr, sr, _ = R.mx_quant(yb1.float().cpu())
        assert torch.equal(yq.cpu(), qr) and torch.equal(ys.cpu(), stage_major(sr)), f"dropout={dropping}"
    # the plain LayerNorm pair
    s = (torch.randn(M, H, generator=g) * 2 + 0.3).cuda()
    gm, bt = e.d["gamma"], e.d["beta"]
    y0, yb0, xh0, rs0 = outs(M, H)
    _lib.check(lib.qst_ln_fwd(s.data_ptr(), gm.data_ptr(), bt.data_ptr(), eps, M, H, y0.data_ptr(), yb0.data_ptr(),
                              xh0.data_ptr(), rs0.data_ptr(), stream()))
    y1, yb1, xh1, rs1 = outs(M, H)
    yq, ys = mx_outs(M, H)
    _lib.check(lib.qst_ln_fwd_mx_train(s.data_ptr(), gm.data_ptr(), bt.data_ptr(), eps, M, H, y1.data_ptr(), yb1.data_ptr(),
                                       xh1.data_ptr(), rs1.data_ptr(), yq.data_ptr(), ys.data_ptr(), stream()))
    assert torch.equal(y1, y0) and torch.equal(bits(yb1), bits(yb0)) and torch.equal(bits(xh1), bits(xh0))
    assert torch.equal(rs1, rs0)
    qr, sr, _ = R.mx_quant(yb1.float().cpu())
    assert torch.equal(yq.cpu(), qr) and torch.equal(ys.cpu(), stage_major(sr))


def test_embed_ln_refuses_shapes_it_is_not_built_for(lib, op):
    """odd H: QST_ERR_BAD_ARG; H > 1024: QST_ERR_UNSUPPORTED; the MXFP8 forms need H % 64 == 0. Nothing is launched."""
    M = 4
    for H, want in ((63, BAD_ARG), (1025, BAD_ARG), (1026, UNSUPPORTED), (2048, UNSUPPORTED)):
        g = torch.Generator().manual_seed(H)
        x = embed_inputs(M, H, g, vocab=20)
        e = Emb(x)
        y, yb, xh, rs = outs(M, H, op)
        assert kf(lib, "qst_embed_ln_fwd", op)(*e.args(), 1e-12, M, H, y.data_ptr(), yb.data_ptr(), xh.data_ptr(),
                                               rs.data_ptr(), stream()) == want, H
        assert kf(lib, "qst_embed_ln_fwd_drop", op)(*e.args(), 1e-12, M, H, y.data_ptr(), yb.data_ptr(), xh.data_ptr(),
                                                    rs.data_ptr(), None, stream()) == want, H
        assert kf(lib, "qst_ln_fwd", op)(ptr(e.d["word"]), ptr(e.d["gamma"]), ptr(e.d["beta"]), 1e-12, M, H, y.data_ptr(),
                                         yb.data_ptr(), xh.data_ptr(), rs.data_ptr(), stream()) == want, H
    if op == "bf16":
        for H in (100, 96, 672):
            g = torch.Generator().manual_seed(H)
            x = embed_inputs(M, H, g, vocab=20)
            e = Emb(x)
            y, yb, xh, rs = outs(M, H)
            yq, ys = mx_outs(M, H)
            assert lib.qst_embed_ln_fwd_mx_train(*e.args(), 1e-12, M, H, y.data_ptr(), yb.data_ptr(), xh.data_ptr(),
                                                 rs.data_ptr(), yq.data_ptr(), ys.data_ptr(), None, stream()) == UNSUPPORTED
            assert lib.qst_ln_fwd_mx_train(ptr(e.d["word"]), ptr(e.d["gamma"]), ptr(e.d["beta"]), 1e-12, M, H, y.data_ptr(),
                                           yb.data_ptr(), xh.data_ptr(), rs.data_ptr(), yq.data_ptr(), ys.data_ptr(),
                                           stream()) == UNSUPPORTED


# ------------------------------------------------------------------ 16-bit weight shadows
SENT = 0x7FC1            # a NaN pattern in both 16-bit formats that no rounding of a finite or infinite fp32 value produces
GUARD = 67


def weights(rows, cols, g, op):
    """randn * 0.05 with rounding ties of the operand type (low 16 bits 0x8000 for bf16, low 13 bits 0x1000 for f16) on
    every 5th element, both signs, exact zeros, an f16-subnormal magnitude and, for f16, values past +-65,504"""
    w = torch.randn(rows, cols, generator=g) * 0.05
    flat = w.view(-1)
    b = flat.view(torch.int32)
    tie = torch.arange(flat.numel()) % 5 == 1
    if op == "bf16":
        b[tie] = (b[tie] & ~0xFFFF) | 0x8000
    else:
        b[tie] = (b[tie] & ~0x1FFF) | 0x1000
    n = flat.numel()
    if n > 8:
        flat[3] = 0.0
        flat[5] = -0.0
        flat[7] = 3e-7                                             # f16 subnormal
        flat[n - 2] = -1e5 if op == "f16" else -3e30
        flat[n // 2] = 70000.0 if op == "f16" else 1e20
        flat[n // 3] = 65519.0                                     # rounds down to 65,504 in f16
    return w


def guarded(n, op):
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int16, device="cuda")
    return buf.view(OPDT[op])


def interior(buf, n):
    return buf[GUARD: GUARD + n]


def guards_intact(buf, n):
    b = bits(buf)
    return bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + n:] == SENT).all())


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 33), (33, 65), (31, 32), (384, 1536), (1000, 3)])
def test_shadow_matrix_is_the_exact_rounding(lib, op, rows, cols):
    """qst_shadow_matrix: dst = RNE(w), dstT = RNE(w)^T bit for bit (f16: saturating), with dst only, dstT only and both;
    the guard bands around each destination keep their sentinel."""
    g = torch.Generator().manual_seed(rows * 100 + cols)
    w = weights(rows, cols, g, op)
    wd = w.cuda()
    n = rows * cols
    want, wantT = bits(to_op(op, w)).reshape(-1), bits(to_op(op, w.t().contiguous())).reshape(-1)
    for which in ("dst", "dstT", "both"):
        dst, dstT = guarded(n, op), guarded(n, op)
        dp = interior(dst, n).data_ptr() if which in ("dst", "both") else None
        dtp = interior(dstT, n).data_ptr() if which in ("dstT", "both") else None
        _lib.check(kf(lib, "qst_shadow_matrix", op)(wd.data_ptr(), rows, cols, dp, dtp, stream()))
        torch.cuda.synchronize()
        assert guards_intact(dst, n) and guards_intact(dstT, n), which
        if dp is not None:
            assert torch.equal(bits(interior(dst, n)).cpu(), want), which
        else:
            assert bool((bits(dst) == SENT).all())
        if dtp is not None:
            assert torch.equal(bits(interior(dstT, n)).cpu(), wantT), which
        else:
            assert bool((bits(dstT) == SENT).all())


SEG_SHAPES = [(1, 1), (5, 7), (32, 32), (33, 65), (31, 32), (64, 3), (1, 100), (100, 1), (7, 300), (384, 96), (2, 2),
              (96, 384), (17, 33), (32, 1), (1, 32), (65, 65), (3, 1000), (40, 40), (30, 31), (128, 130)]


def shadow_table(shapes):
    """segment table {src off, rows, cols, dst off, dstT off, first block} with gaps between segments in the parameter
    arena and in the shadow (the shadow's gaps must keep their sentinel)"""
    tab, src, dst, blk = [], 3, 5, 0
    for r, c in shapes:
        tab.append([src, r, c, dst, dst + r * c + 9, blk])
        src += r * c + 11
        dst += 2 * r * c + 9 + 13
        blk += ((r + 31) // 32) * ((c + 31) // 32)
    return torch.tensor(tab, dtype=torch.int64), src + 7, dst + 3, blk


def shadow_expected(params, tab, nshadow, op, lo=False):
    want = torch.full((nshadow,), SENT, dtype=torch.int16)
    for so, r, c, do, dto, _ in tab.tolist():
        w = params[so: so + r * c].view(r, c)
        hi = to_op(op, w)
        if lo:
            want[do: do + r * c] = bits(to_op(op, w - hi.float())).reshape(-1)
        else:
            want[do: do + r * c] = bits(hi).reshape(-1)
            want[dto: dto + r * c] = bits(hi.t().contiguous()).reshape(-1)
    return want


def shadow_params(tab, nparams, g, op):
    params = torch.randn(nparams, generator=g) * 0.05
    for so, r, c, *_ in tab.tolist():
        params[so: so + r * c] = weights(r, c, g, op).reshape(-1)
    return params


def test_shadow_all_follows_its_segment_table(lib, op):
    """qst_shadow_all over a table of 20 segments (one-block segments, gaps between them, ragged 32 x 32 tiles): every W and
    W^T copy bit for bit, every gap untouched, the last segment checked on its own."""
    g = torch.Generator().manual_seed(3)
    tab, nparams, nshadow, nblocks = shadow_table(SEG_SHAPES)
    params = shadow_params(tab, nparams, g, op)
    pd, td = params.cuda(), tab.cuda()
    shadow = torch.full((nshadow,), SENT, dtype=torch.int16, device="cuda")
    _lib.check(kf(lib, "qst_shadow_all", op)(pd.data_ptr(), shadow.data_ptr(), td.data_ptr(), len(tab), nblocks, stream()))
    got = shadow.cpu()
    assert torch.equal(got, shadow_expected(params, tab, nshadow, op))
    so, r, c, do, dto, _ = tab[-1].tolist()
    w = params[so: so + r * c].view(r, c)
    assert torch.equal(got[do: do + r * c], bits(to_op(op, w)).reshape(-1))
    assert torch.equal(got[dto: dto + r * c], bits(to_op(op, w.t().contiguous())).reshape(-1))
    assert bool((got[dto + r * c:] == SENT).all())


def test_shadow_all_split_f16_hi_and_lo(lib):
    """qst_shadow_all_split_f16 (QST_PREC_F16W): hi = f16(w) as qst_shadow_all_f16; lo = f16(w - hi) at the W offsets only;
    hi + lo reconstructs w to 2^-22 relative -- or, where lo falls below f16's normal range (|lo| < 2^-14, the usual case
    for weights of a few hundredths), to half its subnormal spacing, 2^-25."""
    g = torch.Generator().manual_seed(5)
    tab, nparams, nshadow, nblocks = shadow_table(SEG_SHAPES)
    params = shadow_params(tab, nparams, g, "f16")
    pd, td = params.cuda(), tab.cuda()
    hi = torch.full((nshadow,), SENT, dtype=torch.int16, device="cuda")
    lo = torch.full((nshadow,), SENT, dtype=torch.int16, device="cuda")
    _lib.check(lib.qst_shadow_all_split_f16(pd.data_ptr(), hi.data_ptr(), lo.data_ptr(), td.data_ptr(), len(tab), nblocks,
                                            stream()))
    hi_c, lo_c = hi.cpu(), lo.cpu()
    assert torch.equal(hi_c, shadow_expected(params, tab, nshadow, "f16"))
    assert torch.equal(lo_c, shadow_expected(params, tab, nshadow, "f16", lo=True))
    for so, r, c, do, _, _ in tab.tolist():
        w = params[so: so + r * c].double()
        sl = slice(do, do + r * c)
        rec = hi_c[sl].view(torch.float16).double() + lo_c[sl].view(torch.float16).double()
        normal = w.abs() <= 60000
        err = (rec - w).abs()[normal]
        assert bool((err <= torch.clamp(2.0 ** -22 * w.abs()[normal], min=2.0 ** -25)).all())


# ------------------------------------------------------------------ batched LayerNorm reduction
def test_ln_bwd_reduce_batch_matches_the_immediate_path(lib, op):
    """qst_ln_bwd_reduce_batch over the deferred partials of qst_ln_bwd_drop(dgamma = dbeta = NULL) of LayerNorms of different
    M: per-entry nblocks_each, entries of 0 that fall back to nblocks, a full batch of QST_LN_BATCH_MAX. The outputs start
    non-zero (the kernel adds). Against the immediate path (same partial sums, other order) and fp64 autograd, at the
    tolerances of test_layernorm_fwd_bwd."""
    H, eps = (384 if op == "bf16" else 100), 1e-12
    Ms = [1000, 37, 4099, 5, 300, 4099, 1, 129]
    nbl = {M: lib.qst_ln_bwd_scratch_bytes(M, H) // (2 * H * 4) for M in Ms}
    nmax = max(nbl.values())
    g = torch.Generator().manual_seed(H)
    gamma = 1 + 0.1 * torch.randn(H, generator=g)
    gd = gamma.cuda()
    entries = []
    for i in range(32):
        M = Ms[i % len(Ms)]
        s = torch.randn(M, H, generator=g) * 2 + 0.3
        dy = torch.randn(M, H, generator=g)
        sr = s.double().requires_grad_(True)
        gr = gamma.double().requires_grad_(True)
        br = torch.zeros(H, dtype=torch.float64, requires_grad=True)
        (torch.nn.functional.layer_norm(sr, (H,), gr, br, eps) * dy.double()).sum().backward()
        sd, dyd = s.cuda(), dy.cuda()
        y = torch.empty(M, H, device="cuda")
        xh = torch.empty(M, H, dtype=OPDT[op], device="cuda")
        rs = torch.empty(M, device="cuda")
        _lib.check(kf(lib, "qst_ln_fwd", op)(sd.data_ptr(), gd.data_ptr(), gd.data_ptr(), eps, M, H, y.data_ptr(), None,
                                             xh.data_ptr(), rs.data_ptr(), stream()))
        ds = torch.empty(M, H, device="cuda")
        part = torch.full((nbl[M], 2, H), float("nan"), device="cuda")
        _lib.check(kf(lib, "qst_ln_bwd_drop", op)(dyd.data_ptr(), xh.data_ptr(), rs.data_ptr(), gd.data_ptr(), M, H,
                                                  ds.data_ptr(), None, None, None, part.data_ptr(), None, None, stream()))
        dg0, db0 = torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda")
        scratch = torch.empty(nbl[M] * 2 * H, device="cuda")
        _lib.check(kf(lib, "qst_ln_bwd", op)(dyd.data_ptr(), xh.data_ptr(), rs.data_ptr(), gd.data_ptr(), M, H, ds.data_ptr(),
                                             None, dg0.data_ptr(), db0.data_ptr(), scratch.data_ptr(), stream()))
        start_g, start_b = torch.randn(H, generator=g), torch.randn(H, generator=g)
        entries.append(dict(M=M, part=part, dg=start_g.cuda(), db=start_b.cuda(), sg=start_g, sb=start_b, dg0=dg0, db0=db0,
                            rg=gr.grad, rb=br.grad, keep=(sd, dyd, y, xh, rs, ds, scratch)))
    b = _lib.QstLnReduceBatch()
    b.count, b.H, b.nblocks = 32, H, nmax
    for i, en in enumerate(entries):
        b.partials[i], b.dgamma[i], b.dbeta[i] = en["part"].data_ptr(), en["dg"].data_ptr(), en["db"].data_ptr()
        b.nblocks_each[i] = 0 if nbl[en["M"]] == nmax else nbl[en["M"]]      # 0 = the shared nblocks (the largest M here)
    assert any(b.nblocks_each[i] == 0 for i in range(32)) and any(b.nblocks_each[i] > 0 for i in range(32))
    _lib.check(lib.qst_ln_bwd_reduce_batch(C.byref(b), stream()))
    torch.cuda.synchronize()
    for en in entries:
        M = en["M"]
        dg, db = en["dg"].cpu() - en["sg"], en["db"].cpu() - en["sb"]
        torch.testing.assert_close(dg, en["dg0"].cpu(), rtol=1e-4, atol=1e-4 * math.sqrt(M))
        torch.testing.assert_close(db, en["db0"].cpu(), rtol=1e-4, atol=1e-4 * math.sqrt(M))
        torch.testing.assert_close(db.double(), en["rb"], rtol=1e-4, atol=1e-4 * math.sqrt(M))
        torch.testing.assert_close(dg.double(), en["rg"], rtol=1e-2, atol=1e-2 * math.sqrt(M))
    # a batch of fewer entries adds once more to those only; then the refusals (nothing launched)
    b.count = 3
    before = [en["dg"].clone() for en in entries[:4]]
    _lib.check(lib.qst_ln_bwd_reduce_batch(C.byref(b), stream()))
    torch.cuda.synchronize()
    for i in range(3):
        torch.testing.assert_close(entries[i]["dg"] - before[i], entries[i]["dg0"], rtol=1e-4,
                                   atol=1e-4 * math.sqrt(entries[i]["M"]))
    assert torch.equal(entries[3]["dg"], before[3])
    for count in (0, 33, -1):
        b.count = count
        assert lib.qst_ln_bwd_reduce_batch(C.byref(b), stream()) == BAD_ARG
