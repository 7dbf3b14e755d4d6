"""What the tests of the grouped weight-gradient launch (tests/test_gpu_wgrad_phase.py, tests/test_gpu_wgrad_shapes.py and the
host-only tests/test_wgrad_cases_host.py) share; imported like kernel_helpers, not a conftest.

  * problem / padded_problem: the operands of one gradient on the device and its fp32 reference on the CPU, cached;
  * run: one grouped launch (or several into the same C) through the entry point the CALLER names -- the entry-point names stay
    in the tests/test_gpu_*.py files, which tests/test_kernel_coverage_host.py reads -- and the comparison with the reference;
  * decomposition and the case table: how the kernels cut a group into tasks, to LABEL the cases (what a case is there for) and
    for the host test that keeps every class in the table. Nothing a GPU test asserts depends on them.

The module imports neither the library nor kernel_helpers at the top: the host test reads the case table without them.
"""
import ctypes as C
import functools
import math

import torch


# ------------------------------------------------------------------ the case table
def layer(H, I):
    """the four weight gradients of a layer, as (N, K) of C[N, K] = dY[M, N]^T . X[M, K]: dW2, dW1, dWo, dWqkv"""
    return [(H, I), (I, H), (H, H), (3 * H, H)]


MINILM = (384, 1536)                   # the layer the older wgrad files test: 48 tiles of 192 x 192
M_FIVE = 2560 - 17                     # five stages of 64 rows per equal range (of eight), the last one ragged
M_TWO = 1024 - 17                      # two stages per range, for the widths whose CPU reference is large

# A: one layer per width class; H up to 512 at M_FIVE, the wide ones at M_TWO
WIDTHS = [(64, 256), (128, 512), (256, 1024), (320, 1280), (448, 1792), (512, 2048), (768, 3072), (1024, 4096)]


def rows_for(H):
    return M_FIVE if H <= 512 else M_TWO


CASES_A = [(H, I, rows_for(H)) for H, I in WIDTHS]
# B: two and three ranges per XCD (16 and 10 workgroups per range): (splits, (H, I)), all at M_FIVE
CASES_B = [(splits, HI) for splits in (16, 24) for HI in (MINILM, (448, 1792))]
# D: problem counts other than 1 and 4: (M, shapes)
CASES_NPROB = [(M_TWO, layer(64, 256) + layer(128, 512)),
               (M_FIVE, [(64, 64), (1152, 1152)]),                 # a one-tile problem in front of a large one
               (M_FIVE, [(200, 136), (192, 192), (72, 392)])]      # ragged, whole, ragged
# E: few rows -- fewer stages than ranges, one ragged stage, a stage and a row, eight stages and a ragged ninth
FEW_ROWS = [1, 63, 65, 520]
FEW_ROWS_LAYERS = [(64, 256), (320, 1280)]
# F: the library's own skew and order, at 16 stages per range: (shapes, whether a skew is expected)
M_AUTO = 8192 - 17
CASES_AUTO = [([(384, 384)], False), ([(1152, 1152)], True), ([(1536, 1536)], True), (layer(448, 1792), True)]

TILED = (192, 192)                     # gemm_tn_group_kernel's tile of C (rows of dY^T x columns of X)
EIGHT_PHASE = (128, 384)               # gemm_tn8_group_kernel's (the form qst_gemm_tn8_group uses)


def workgroups_per_range(splits):
    """32 workgroups per XCD over the ranges that XCD owns (splits rounded up to a multiple of 8; 0 = 8)"""
    return 32 // (max(8, (splits + 7) // 8 * 8) // 8)


def decomposition(shapes, tile_n, tile_k, W):
    """(T, a, b, pieces, idle): T tiles of tile_n x tile_k over the W workgroups of an M-range are a = T // W whole tiles each
    and b = T % W leftover tiles, each cut into pieces = max(1, W // b) stage pieces; idle workgroups run no piece. Without a
    leftover tile (b = 0) there are no pieces: pieces = idle = 0."""
    T = sum(-(-N // tile_n) * -(-K // tile_k) for N, K in shapes)
    a, b = divmod(T, W)
    pieces = max(1, W // b) if b else 0
    return T, a, b, pieces, (W - b * pieces if b else 0)


def ragged(shapes, tile_n, tile_k):
    """(some N is no multiple of the tile, some K is not): zero fill past the operand's width, masked flush"""
    return any(N % tile_n for N, _ in shapes), any(K % tile_k for _, K in shapes)


# ------------------------------------------------------------------ problems
@functools.lru_cache(maxsize=None)
def host_problem(kind, M, N, K):
    """dY [M, N] and X [M, K] as fp32 on the CPU, dY^T . X and the column sums of dY. kind "ints": drawn from the integers
    -2 .. 2 (the same for both operand types: every one is exact in either); otherwise the operand type Gaussians are rounded to."""
    ints = kind == "ints"
    g = torch.Generator().manual_seed(M * 3 + N + K + (7 if ints else 0))
    if ints:
        A = torch.randint(-2, 3, (M, N), generator=g).float()
        B = torch.randint(-2, 3, (M, K), generator=g).float()
    else:
        from kernel_helpers import opr
        A = opr(kind, torch.randn(M, N, generator=g))
        B = opr(kind, torch.randn(M, K, generator=g))
    return A, B, A.t() @ B, A.sum(0)


@functools.lru_cache(maxsize=None)
def problem(op, M, N, K, ints=False):
    """dY [M, N] and X [M, K] in the operand type on the device, dY^T . X and the column sums of dY (fp32, CPU)"""
    from kernel_helpers import OPDT
    A, B, ref, rcs = host_problem("ints" if ints else op, M, N, K)
    return A.to(OPDT[op]).cuda(), B.to(OPDT[op]).cuda(), ref, rcs


GUARD_ROWS, GUARD_COLS, VIEW_COL = 64, 72, 40      # the padded operand is [M + 64, width + 72]; the view starts at column 40
C_GUARD_ROWS, C_GUARD_COLS, CS_GUARD = 1, 8, 8     # C is [N + 1, K + 8], colsum has N + 8 elements


@functools.lru_cache(maxsize=None)
def padded_problem(op, M, N, K, ints=True):
    """problem(), with each operand a view [:M, 40 : 40 + width] of a matrix [M + 64, width + 72] whose every other element
    is ONE: a read past the view's width or rows -- which a dense operand answers with the next row's own data, or with the
    zero fill at the end of the allocation -- adds to the sums."""
    from kernel_helpers import OPDT
    A, B, ref, rcs = host_problem("ints" if ints else op, M, N, K)
    views = []
    for t in (A, B):
        big = torch.ones(M + GUARD_ROWS, t.shape[1] + GUARD_COLS)
        big[:M, VIEW_COL:VIEW_COL + t.shape[1]] = t
        views.append(big.to(OPDT[op]).cuda()[:M, VIEW_COL:VIEW_COL + t.shape[1]])
    return views[0], views[1], ref, rcs


# ------------------------------------------------------------------ the launch
def run(entry, op, M, shapes, skew=0, order=0, launches=1, preset=0.0, ints=False, splits=0, no_colsum=(), padded=False,
        cs_preset=0.0):
    """`launches` calls of entry(grp, stream) -- kf(lib, "qst_gemm_tn_group", op) or its 8-phase twin, named by the caller --
    on the group of `shapes` [(N, K), ...] over M rows, then C == launches * dY^T . X + preset and colsum == launches * column
    sums + cs_preset: EXACTLY with ints, within rtol 1e-3 / atol launches * 1e-3 * sqrt(M) otherwise.
    no_colsum: the problems launched with colsum == NULL. padded: operands with leading dimensions larger than their width
    inside guard bands of ones (padded_problem), C and colsum with guard rows / columns / elements that must keep the preset.
    Returns the group as it was launched."""
    from kernel_helpers import stream
    from quadruplet_sentence_transformer_amd import _lib
    grp = _lib.QstTnGroup()
    grp.nprob, grp.splits, grp.skew, grp.order = len(shapes), splits, skew, order
    outs = []
    for i, (N, K) in enumerate(shapes):
        Ad, Bd, ref, rcs = (padded_problem if padded else problem)(op, M, N, K, ints)
        gr, gc, gs = (C_GUARD_ROWS, C_GUARD_COLS, CS_GUARD) if padded else (0, 0, 0)
        Cd = torch.full((N + gr, K + gc), preset, device="cuda")   # accumulation semantics: C += A^T . B
        cs = None if i in no_colsum else torch.full((N + gs,), cs_preset, device="cuda")
        q = grp.prob[i]
        q.A, q.B, q.C, q.colsum = Ad.data_ptr(), Bd.data_ptr(), Cd.data_ptr(), cs.data_ptr() if cs is not None else None
        q.M, q.N, q.K, q.lda, q.ldb, q.ldc = M, N, K, Ad.stride(0), Bd.stride(0), Cd.stride(0)
        outs.append((N, K, Cd, cs, launches * ref + preset, launches * rcs + cs_preset))
    for _ in range(launches):
        _lib.check(entry(grp, stream()))
    torch.cuda.synchronize()
    rtol, atol = (0.0, 0.0) if ints else (1e-3, launches * 1e-3 * math.sqrt(M))
    for i, (N, K, Cd, cs, ref, rcs) in enumerate(outs):
        what = f"problem {i} (N = {N}, K = {K})"
        Ch = Cd.cpu()
        torch.testing.assert_close(Ch[:N, :K], ref, rtol=rtol, atol=atol, msg=lambda m: f"C of {what}: {m}")
        if cs is not None:
            ch = cs.cpu()
            torch.testing.assert_close(ch[:N], rcs, rtol=rtol, atol=atol, msg=lambda m: f"colsum of {what}: {m}")
            assert bool((ch[N:] == cs_preset).all()), f"colsum of {what}: written past N"
        assert bool((Ch[N:] == preset).all()) and bool((Ch[:, K:] == preset).all()), f"C of {what}: written outside [N, K]"
    return grp


def effective_skew(ranges, grp):
    """ranges = lib.qst_tn_group_ranges (named by the caller): the skew in effect for grp and the splits + 1 range boundaries"""
    n = max(8, (grp.splits + 7) // 8 * 8)
    begins = (C.c_int32 * (n + 1))()
    eff = ranges(grp, begins)
    return eff, list(begins)
