"""Irregular attention masks, poisoned padding and the fp64 yardsticks of the attention kernels (tests/test_gpu_attention_masks.py,
tests/test_attention_masks_host.py). Pure torch on the CPU: imported like tuple_loss_helpers, not a conftest, and never imports the
library, so the host test can judge the references and the bounds before any kernel is involved.

  * mask_families / poison_padding / make_case: one sequence per mask family, padding keys made loud;
  * attn_ref, scores_ref, lse_ref, pv_abs, exact: HF attention in fp64 and what the bounds are built from;
  * attn_ref_rounded: the same computation with the kernels' rounding points emulated;
  * fwd_bound, block_norms / bwd_floor, drel_floor: the bounds themselves; K_BLOCK, K_DREL: their measured constants.
"""
import math
from collections import namedtuple

import torch

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
EPS = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}          # spacing of the operand type at 1.0

FAMILIES = "abcdefgh"

# (name, n, L, A, d, position bias): the shapes of tests/test_gpu_attention_masks.py and the backward kernel each one reaches
Case = namedtuple("Case", "name n L A d bias")
CASES = [
    Case("c1_L32_fused", 8, 32, 2, 32, False),            # fused, single key tile
    Case("c2_L128_fused_remap", 8, 128, 2, 32, True),     # fused; forward grid 16: workgroup-id remap
    Case("c3_L128_oddA", 8, 128, 3, 32, False),           # fused; odd A: no remap
    Case("c4_L32_persistent", 130, 32, 4, 32, False),     # fused; 520 items for 512 persistent workgroups
    Case("c5_L160_pair32", 8, 160, 2, 32, True),          # d = 32 pair; two query blocks, last chunk of 32 rows
    Case("c6_L96_one64_nc2", 8, 96, 2, 64, True),         # one64, NC = 2
    Case("c7_L288_one64_nc3", 8, 288, 2, 64, True),       # one64, NC = 3, partial chunk
    Case("c8_L512_one64_nc4", 8, 512, 1, 64, False),      # one64, NC = 4
    Case("c9_L416_pair64_bias", 8, 416, 1, 64, True),     # bias above L = 384: one64 does not fit, the d = 64 pair runs
]
BY_NAME = {c.name: c for c in CASES}
SPLIT = ["c1_L32_fused", "c2_L128_fused_remap", "c6_L96_one64_nc2", "c7_L288_one64_nc3", "c8_L512_one64_nc4"]
# (case, force_split) run with dropout of the probabilities, p = 0.1
DROPPED = [("c2_L128_fused_remap", 0), ("c5_L160_pair32", 0), ("c7_L288_one64_nc3", 0), ("c9_L416_pair64_bias", 0),
           ("c7_L288_one64_nc3", 1)]
# every (case, force_split, dropout) the GPU file runs
RUNS = ([(c.name, 0, False) for c in CASES] + [(name, 1, False) for name in SPLIT] + [(name, fs, True) for name, fs in DROPPED])
DROP_SEED, DROP_STEP, DROP_P, DROP_LAYER = 31337, 4, 0.1, 1
# parity-precision kernels: (L, d, bias), A = 2, one sequence per family
PARITY = [(32, 32, False), (96, 32, True), (288, 64, True)]

# Backward bound per block (sequence, head, part q / k / v): ||got - ref||_2 <= K_BLOCK * eps * ||ref||_2 + floor.
# Measured on the CPU, attn_ref_rounded against exact fp64 over every entry of RUNS, both operand types
# (tests/test_attention_masks_host.py::test_backward_constants_come_from_the_rounded_reference re-measures and prints them):
# largest ||rounded - exact|| / (eps ||exact||) over the blocks with a non-zero gradient: 0.959 (the floor NOT subtracted, so k
# alone carries the rounding of a dense block); 3 x 0.959 = 2.88 -> 4.
K_BLOCK = 4.0
# drel [A, 2L], per head: ||got - ref||_2 <= K_DREL * eps * ||ref||_2 + floor. dS enters the bias gradient unrounded, so the
# emulation differs from fp64 only through delta = dO . round(O): largest ratio 1.370; 3 x 1.370 = 4.11 -> 8.
K_DREL = 8.0


# ------------------------------------------------------------------ masks and inputs
def family_mask(f, L):
    """One mask row. The L >= 96 forms are the table of the module's families; at L = 32 / 64 they shrink so that every family
    keeps a valid key: c pads 7 on the left at L = 32; d pads 16 at L = 32; e has no keys 32..63 to kill at L = 32; h is the
    last 32-key tile at 32 < L <= 128 and the last 16 keys at L = 32."""
    j = torch.arange(L)
    if f == "a":                                   # no padding
        m = j >= 0
    elif f == "b":                                 # right-padded: valid length L - 5 is no multiple of 32
        m = j < L - 5
    elif f == "c":                                 # left-padded by a whole 32-key tile + 8 keys
        m = j >= (40 if L >= 64 else 7)
    elif f == "d":                                 # left-padded by exactly one tile
        m = j >= (32 if L >= 64 else 16)
    elif f == "e":                                 # holes: every third key, and an interior dead tile
        m = (j % 3 != 2) & ~((j >= 32) & (j < 64))
    elif f == "f":                                 # one valid key, the last
        m = j == L - 1
    elif f == "g":                                 # all padding
        m = j < 0
    elif f == "h":                                 # valid keys in the last 128-key chunk only
        m = j >= (((L - 1) // 128) * 128 if L > 128 else (L - 32 if L > 32 else 16))
    else:
        raise ValueError(f)
    return m.long()


def mask_families(n, L):
    """int64 [n, L]: row r is family FAMILIES[r % 8]."""
    return torch.stack([family_mask(FAMILIES[r % len(FAMILIES)], L) for r in range(n)])


def poison_padding(qkv, mask, H, g):
    """qkv [n * L, 3H] with the padding keys of every sequence that has a valid key made loud: K rows x 8, V rows +-1000 (random
    signs; both exact in bf16 and f16). Q rows stay: padded queries attend like any other (HF does not mask them). The
    all-padding sequence stays as it is: its result, the uniform mean of V, is defined. A kernel that gives a masked key any
    weight is then off by orders of magnitude more than rounding; the references are not (finfo.min absorbs every score)."""
    n, L = mask.shape
    out = qkv.clone().view(n, L, 3 * H)
    pad = (mask == 0) & (mask.sum(1, keepdim=True) > 0)                     # [n, L]
    sign = torch.randint(0, 2, (n, L, H), generator=g).to(qkv.dtype) * 2 - 1
    out[:, :, H:2 * H] = torch.where(pad[:, :, None], out[:, :, H:2 * H] * 8, out[:, :, H:2 * H])
    out[:, :, 2 * H:] = torch.where(pad[:, :, None], 1000.0 * sign, out[:, :, 2 * H:])
    return out.view(n * L, 3 * H)


def rel_index(L):
    """[i, j] -> j - i + L: the entry of a relative-position vector [2L] that the pair (query i, key j) reads."""
    return (torch.arange(L)[None, :] - torch.arange(L)[:, None]) + L


Inputs = namedtuple("Inputs", "qkv mask relpos dctx pm")


def make_case(case, op, drop=False, full_bias=False):
    """The inputs of one case, fp32 tensors holding operand-type values (op None: fp32 as drawn, for the parity kernels).
    dctx is zero on the all-padding sequences. relpos: [A, 2L], or [A, L, L] with full_bias. pm: dropout multipliers
    [n, A, L, L] of oracle.dropout_ref.multipliers8 or None."""
    n, L, A, d = case.n, case.L, case.A, case.d
    H = A * d
    g = torch.Generator().manual_seed(1000 * L + 10 * A + d + n)
    mask = mask_families(n, L)
    qkv = poison_padding(torch.randn(n * L, 3 * H, generator=g), mask, H, g)
    dctx = torch.randn(n * L, H, generator=g)
    dctx = (dctx.view(n, L, H) * (mask.sum(1) > 0)[:, None, None]).reshape(n * L, H)
    relpos = None
    if case.bias:
        relpos = 0.5 * torch.randn(*((A, L, L) if full_bias else (A, 2 * L)), generator=g)
    if op is not None:
        qkv, dctx = qkv.to(DT[op]).float(), dctx.to(DT[op]).float()
    pm = None
    if drop:
        from oracle import dropout_ref as D
        pm = torch.from_numpy(D.multipliers8(DROP_SEED, DROP_STEP, D.site_probs(DROP_LAYER), n * A * L * L, DROP_P)
                              .reshape(n, A, L, L))
    return Inputs(qkv, mask, relpos, dctx, pm)


# ------------------------------------------------------------------ fp64 references
def heads(x, n, L, A, d):
    """[n * L, A * d] -> [n, A, L, d]"""
    return x.view(n, L, A, d).transpose(1, 2)


def tokens(x, n, L, A, d):
    """[n, A, L, d] -> [n * L, A * d]"""
    return x.transpose(1, 2).reshape(n * L, A * d)


def scores_ref(qkv, mask, rel, n, L, A, d):
    """Masked, biased scores [n, A, L, L] as HF forms them (modeling_bert.py BertSelfAttention; MPNet adds the position bias
    `rel` [A, L, L] before the mask), in the dtype of qkv."""
    H = A * d
    q, k, _ = [heads(t, n, L, A, d) for t in qkv.view(n * L, 3 * H).split(H, dim=-1)]
    s = q @ k.transpose(-1, -2) / math.sqrt(d)
    if rel is not None:
        s = s + rel[None]
    return s + (1.0 - mask[:, None, None, :].to(qkv.dtype)) * torch.finfo(torch.float32).min


def attn_ref(qkv, mask, rel, n, L, A, d, pm=None):
    """HF attention (modeling_bert.py BertSelfAttention; MPNet adds the position bias `rel` [A, L, L] before the mask) in the
    dtype of qkv, fp32 or fp64; pm [n, A, L, L]: dropout multipliers of the probabilities."""
    H = A * d
    v = heads(qkv.view(n * L, 3 * H)[:, 2 * H:], n, L, A, d)
    p = torch.softmax(scores_ref(qkv, mask, rel, n, L, A, d), -1)
    if pm is not None:
        p = p * pm
    return tokens(p @ v, n, L, A, d)


def lse_ref(qkv, mask, rel, n, L, A, d):
    """Natural-log logsumexp of the masked, biased scores, [n, A, L]."""
    return torch.logsumexp(scores_ref(qkv, mask, rel, n, L, A, d), -1)


def pv_abs(qkv, mask, rel, n, L, A, d, pm=None):
    """P @ |V| in the layout of the context, [n * L, H]: what the rounding of P is relative to."""
    H = A * d
    v = heads(qkv.view(n * L, 3 * H)[:, 2 * H:], n, L, A, d)
    p = torch.softmax(scores_ref(qkv, mask, rel, n, L, A, d), -1)
    if pm is not None:
        p = p * pm
    return tokens(p @ v.abs(), n, L, A, d)


def diag_sums(x, L):
    """x [n, A, L, L] -> [A, 2L]: sums over the sequences and along the diagonals j - i (entry j - i + L; entry 0 stays 0)."""
    A = x.shape[1]
    out = torch.zeros(A, 2 * L, dtype=x.dtype)
    return out.index_add_(1, rel_index(L).reshape(-1), x.sum(0).reshape(A, L * L))


Exact = namedtuple("Exact", "ctx lse pv dqkv drel")


def exact(inp, case, rel_shift=0, mask=None, pm="same"):
    """fp64 forward and autograd backward of the case: ctx [n * L, H], lse [n, A, L], pv_abs, dqkv [n * L, 3H], drel (the shape
    of inp.relpos, or None). rel_shift / mask / pm replace what a mutant gets wrong: the bias entry j - i + L + rel_shift
    (relative-position vectors only), another mask, other dropout multipliers."""
    n, L, A, d = case.n, case.L, case.A, case.d
    mask = inp.mask if mask is None else mask
    pm = inp.pm if isinstance(pm, str) else pm
    pm = None if pm is None else pm.double()
    qr = inp.qkv.double().requires_grad_(True)
    relr = full = None
    if inp.relpos is not None:
        relr = inp.relpos.double().requires_grad_(True)
        full = relr if relr.dim() == 3 else relr[:, (rel_index(L) + rel_shift).clamp(max=2 * L - 1)]
    ctx = attn_ref(qr, mask, full, n, L, A, d, pm)
    (ctx * inp.dctx.double()).sum().backward()
    with torch.no_grad():
        lse = lse_ref(qr, mask, full, n, L, A, d)
        pv = pv_abs(qr, mask, full, n, L, A, d, pm)
    return Exact(ctx.detach(), lse, pv, qr.grad, None if relr is None else relr.grad)


def attn_ref_rounded(op, inp, case):
    """(ctx, dqkv, drel) of the case in fp64 with the 16-bit kernels' rounding points emulated (round to nearest even into the
    operand type `op`); everything else the kernels keep in fp32 is exact here. Read off csrc/attention.hip:

    forward (attn_fwd_kernel)
      * the unnormalised probabilities exp(s - max), after dropout has zeroed some, are rounded to the operand type as the B
        operand of P . V (acc_frag); the row sum l uses the unrounded ones. (The kernel rounds relative to the running maximum
        and rescales in fp32; rounding is relative, so the final maximum gives the same error up to the subnormal range.)
      * the output (P . V) * (dropout scale / l) is rounded once (pack_op2).
    backward (attn_bwd_dq_kernel + attn_bwd_dkv_kernel, attn_bwd_fused_kernel, attn_bwd_one64_kernel)
      * delta = dO . O reads the ROUNDED forward output;
      * P = exp(s - lse) and dP = dO . V^T, dS = P (mask dP - delta) are fp32;
      * dS is rounded to the operand type before dQ = dS . K and dK = dS^T . Q (the pair rounds dS * scale, the one-workgroup
        kernels round dS and scale the fp32 sums: the same relative error; the latter is emulated);
      * the dropped, scaled probabilities P mask are rounded before dV = P^T . dO;
      * dQ, dK, dV are rounded once on the way out;
      * the bias gradient takes the UNROUNDED dS (fp32 diagonal sums), so it differs from fp64 only through delta."""
    n, L, A, d = case.n, case.L, case.A, case.d
    H = A * d

    def rnd(t):
        return t.to(DT[op]).double()

    x = inp.qkv.double()
    q, k, v = [heads(t, n, L, A, d) for t in x.split(H, dim=-1)]
    do = heads(inp.dctx.double(), n, L, A, d)
    full = None
    if inp.relpos is not None:
        full = inp.relpos.double() if inp.relpos.dim() == 3 else inp.relpos.double()[:, rel_index(L)]
    s = scores_ref(x, inp.mask, full, n, L, A, d)
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    l = e.sum(-1, keepdim=True)
    pm = torch.ones_like(e) if inp.pm is None else inp.pm.double()
    dscale = float(pm.max())
    o = rnd((rnd(e) * (pm != 0) @ v) * (dscale / l))
    p = e / l
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * ((do @ v.transpose(-1, -2)) * pm - delta)
    dsr = rnd(ds)
    sc = 1.0 / math.sqrt(d)
    dq, dk, dv = rnd(sc * (dsr @ k)), rnd(sc * (dsr.transpose(-1, -2) @ q)), rnd(rnd(p * pm).transpose(-1, -2) @ do)
    dqkv = torch.cat([tokens(t, n, L, A, d) for t in (dq, dk, dv)], dim=1)
    drel = None
    if inp.relpos is not None:
        drel = ds.sum(0) if inp.relpos.dim() == 3 else diag_sums(ds, L)
    return tokens(o, n, L, A, d), dqkv, drel


# ------------------------------------------------------------------ bounds
def fwd_bound(op, ex):
    """Per element of ctx: the forward rounds P once and the output once, everything else is fp32, so to first order
    |ctx - ref| <= eps (pv_abs + |ref|) / 2 under round-to-nearest and eps (pv_abs + |ref|) under truncation; the factor 2 over
    the latter covers the second-order and fp32 terms. (The emulation reaches 0.35 - 0.67 of eps (pv_abs + |ref|).)"""
    return 2 * EPS[op] * (ex.pv + ex.ctx.abs()) + 1e-6


def block_norms(x, n, L, A, d):
    """dqkv-shaped [n * L, 3 A d] -> L2 norms [n, A, 3] of the blocks (sequence, head, part q / k / v)."""
    return x.view(n, L, 3, A, d).pow(2).sum(dim=(1, 4)).sqrt().transpose(1, 2)


def _p_and_a(inp, case, ex):
    n, L, A, d = case.n, case.L, case.A, case.d
    H = A * d
    x = inp.qkv.double()
    full = None
    if inp.relpos is not None:
        full = inp.relpos.double() if inp.relpos.dim() == 3 else inp.relpos.double()[:, rel_index(L)]
    p = torch.softmax(scores_ref(x, inp.mask, full, n, L, A, d), -1)
    a = heads((inp.dctx.double() * ex.ctx).abs(), n, L, A, d).sum(-1)                # [n, A, L]: sum_dd |dO O| of query i
    q, k, _ = [heads(t, n, L, A, d) for t in x.split(H, dim=-1)]
    return p, a, q.norm(dim=-1), k.norm(dim=-1)


def bwd_floor(op, inp, case, ex):
    """[n, A, 3]: the cancellation term of the block bound. delta_i = dO_i . round(O_i) is off by up to eps a_i, a_i = sum_dd
    |dO_i O_i| (one rounding of the forward output), and dS_ij = P_ij (dP_ij - delta_i) carries P_ij times that even where dP
    - delta cancels to exactly 0 in the reference (a row that sees one key has P = 1, dS = 0: the same effect as the comment on
    the parity kernels' bias gradient in tests/test_gpu_kernels.py). Through dQ_i = scale sum_j dS_ij k_j and dK_j = scale sum_i
    dS_ij q_i that is at most
        dQ row i: eps scale a_i sum_j P_ij |k_j|        dK row j: eps scale sum_i P_ij a_i |q_i|
    (P without dropout: dropout does not touch delta's path); dV does not read delta: 0. Block norm over the rows."""
    p, a, qn, kn = _p_and_a(inp, case, ex)
    sc = EPS[op] / math.sqrt(case.d)
    fq = sc * (a * (p @ kn[..., None])[..., 0]).norm(dim=-1)
    fk = sc * (p.transpose(-1, -2) @ (a * qn)[..., None])[..., 0].norm(dim=-1)
    return torch.stack([fq, fk, torch.zeros_like(fq)], dim=-1)


def drel_floor(op, inp, case, ex):
    """[A]: the same term for the bias gradient: entry t of a head gathers P_ij eps a_i over its diagonal and the sequences."""
    p, a, _, _ = _p_and_a(inp, case, ex)
    w = EPS[op] * p * a[..., None]
    return (w.sum(0) if inp.relpos.dim() == 3 else diag_sums(w, case.L)).flatten(1).norm(dim=-1)
