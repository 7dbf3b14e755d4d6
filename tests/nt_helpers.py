"""What the tests of the NT GEMMs (tests/test_gpu_nt_shapes.py and the host-only tests/test_nt_cases_host.py) share; imported like
wgrad_helpers, not a conftest.

  * host_problem / dev_problem: operands whose every product and partial sum is exact in fp32, so that the kernels' results
    are compared with rtol = atol = 0; dense, or as views of larger matrices inside guard bands;
  * run: every epilogue a form accepts through the entry point the CALLER names -- the entry-point names stay in the
    tests/test_gpu_*.py files, which tests/test_kernel_coverage_host.py reads -- the exact comparison on C[:M, :N] and the check
    that every other element of C, C2 and bias still holds its sentinel;
  * the forms' geometry and the case table: which tile, wave tile and K stage a selector runs on, to LABEL the cases (what a
    case is there for) and for the host test that keeps every class in the table. Nothing a GPU test asserts depends on them.

The module imports neither the library nor kernel_helpers at the top: the host test reads the case table without them.
"""
import collections
import functools
import math

import torch

EPI_BF16, EPI_F32_RESID, EPI_GELU, EPI_GELU_BWD, EPI_F32_RESID_BF16 = range(5)
EPI_NAMES = ["BF16", "F32_RESID", "GELU", "GELU_BWD", "F32_RESID_BF16"]
F32_EPIS = (EPI_F32_RESID, EPI_F32_RESID_BF16)
ERR_BAD_ARG, ERR_UNSUPPORTED = -1, -2
SENTINEL = -777.0                      # exact in bf16, f16 and fp32; no reference contains it (test_nt_cases_host.py)

# ------------------------------------------------------------------ forms
# name, how it is called ("nt": entry(args, epi, stream) with QstGemmArgs.splits = sel; "nt8": entry(args, epi, sel, stream)),
# workgroup tile and wave tile as (rows, columns), depth of a K stage, the epilogues that reach THIS kernel through the selector
# (csrc/gemm.hip qst_gemm_nt: splits 3 is the 128 x 384 kernel for QST_EPI_F32_RESID only and the 128-row kernel otherwise,
# splits 4 the tall wave tile for the 16-bit epilogues only), and whether N % 8 == 4 is taken (the tiled kernels: N % 4 == 0).
Form = collections.namedtuple("Form", "name call sel tile wave stage epis n4")
FORMS = [
    Form("tiles128", "nt", 1, (128, 192), (64, 96), 64, (0, 1, 2, 3, 4), True),
    Form("tiles256", "nt", 2, (256, 192), (64, 96), 64, (0, 1, 2, 3, 4), True),
    Form("wide128x384", "nt", 3, (128, 384), (64, 96), 64, (1,), True),
    Form("tall256", "nt", 4, (256, 192), (128, 96), 32, (0, 2, 3), True),
    Form("eight128x384", "nt8", 0, (128, 384), (64, 96), 64, (0, 1, 2, 3, 4), False),
    Form("eight256x256", "nt8", 1, (256, 256), (128, 64), 64, (0, 1, 2, 3, 4), False),
]
FORM = {f.name: f for f in FORMS}
# the same kernels through qst_gemm_nt's selector bits: 0x20 / 0x40 force the 8-phase tiles (where qst_gemm_nt8_supported
# agrees; the 128-row tiled kernel otherwise), 0x80 forbids them
VIA_NT = {0x20: FORM["eight128x384"]._replace(name="nt-0x20", call="nt", sel=0x20),
          0x40: FORM["eight256x256"]._replace(name="nt-0x40", call="nt", sel=0x40),
          0x80: FORM["tiles128"]._replace(name="nt-0x80", sel=0x80)}
MFMA_ROWS = 32                         # rows of an MFMA block of the tiled kernels; two 16-row blocks of the 8-phase ones


def accepts(form, N, K, lda=None, ldb=None, ldc=None, ldr=None):
    """the rules of qst_gemm_nt / qst_gemm_nt8_supported, restated: whether `form`'s own kernel runs the shape (for the "nt8"
    forms called through qst_gemm_nt this is also whether the selector reaches the 8-phase kernel instead of falling back)"""
    lda, ldb, ldc, ldr = (K if lda is None else lda), (K if ldb is None else ldb), (N if ldc is None else ldc), (N if ldr is None else ldr)
    if K % 64 or lda % 8 or ldb % 8:
        return False
    if form.n4:
        return N % 4 == 0 and ldc % 4 == 0
    return N % 8 == 0 and ldc % 8 == 0 and ldr % 4 == 0


def tile_count(form, M, N):
    return -(-M // form.tile[0]) * -(-N // form.tile[1])


def row_classes(form, M):
    th, wh = form.tile[0], form.wave[0]
    out = set()
    if M == 1: out.add("m1")
    if M == MFMA_ROWS - 1: out.add("below_block")
    if M == MFMA_ROWS + 1: out.add("above_block")
    if M == wh + 1: out.add("above_wave")
    if M == th - 1: out.add("below_tile")
    if M == th + 1: out.add("above_tile")
    if th + MFMA_ROWS < M < 2 * th and M % MFMA_ROWS: out.add("ragged_second")
    return out


def col_classes(form, N):
    """the position of the last vector of a row (8 columns; 4 where N % 8 == 4) in the wave tile and the workgroup tile"""
    tw, ww = form.tile[1], form.wave[1]
    h = "4" if N % 8 == 4 else ""
    out = set()
    if N <= 8: out.add("min" + h)
    if 8 < N % ww < 32: out.add("first_block" + h)            # the tail ends inside the first 32-column block of a wave
    if N % ww == 36: out.add("past_block4")                    # half a vector past that block
    if N % ww == 0 and N % tw: out.add("wave_boundary")
    if N > ww and N % ww in (4, 8): out.add("vec_past_wave" + h)
    if N > tw and N % tw in (4, 8): out.add("vec_past_tile" + h)
    if N % tw == 0: out.add("whole_tiles")
    return out


def k_classes(form, K):
    n = K // form.stage
    return {"one_stage64"} if K == 64 else {"even_stages" if n % 2 == 0 else "odd_stages"}


ROW_CLASSES = {"m1", "below_block", "above_block", "above_wave", "below_tile", "above_tile", "ragged_second"}
COL_CLASSES = {"min", "first_block", "wave_boundary", "vec_past_wave", "vec_past_tile", "whole_tiles"}
COL_CLASSES_N4 = {"min4", "first_block4", "past_block4", "vec_past_wave4", "vec_past_tile4"}
TILE_COUNTS = {1, 2, 3, 5, 9}          # ... and every residue of 8 (xcd_remap: q = count >> 3, r = count & 7, a branch on x < r)

# ------------------------------------------------------------------ the case table: (label, M, N, K), M <= 600, N <= 1200, K <= 512
ROW_N, ROW_K = 200, 128
COL_M, COL_K = 70, 128
RED_M, RED_N = 133, 200
CASES = (
    # rows, at N = 200 (one vector past a 192-column tile and past a 64- and a 96-column wave), two K stages
    [("m1", 1), ("below_block", 31), ("above_block", 33), ("above_wave64", 65), ("below_tile128", 127),
     ("above_tile128_wave128", 129), ("ragged_second128", 200), ("below_tile256", 255), ("above_tile256", 257),
     ("ragged_second256", 300)],
    # columns, at M = 70 (one wave tile of 64 rows and six rows of the next)
    [("min4", 4), ("min", 8), ("past_block4", 36), ("wave_boundary96", 96), ("vec_past_wave4", 100), ("vec_past_wave96", 104),
     ("first_block4", 116), ("whole192_wave_boundary64", 192), ("vec_past_tile192_4", 196), ("vec_past_tile192", 200),
     ("first_block", 216), ("vec_past_tile256", 264), ("wave_boundary96_second_tile", 288), ("whole384", 384),
     ("vec_past_tile384_4", 388), ("vec_past_tile384", 392), ("whole_all", 768)],
    # reduction, at (133, 200): 1, 2, 3, 7 and 8 stages of 64 (the tall form's 32-deep stages: always an even number, K % 64 == 0)
    [("one_stage", 64), ("even_stages", 128), ("odd_stages3", 192), ("odd_stages7", 448), ("even_stages8_s5", 512)],
    # tile counts, one K stage
    [("tiles_9_6", 300, 520), ("tiles_15_9_10", 600, 520), ("tiles_15_10_9_8", 300, 776), ("tiles_5_3", 600, 104),
     ("tiles_5_3_4", 70, 776), ("tiles_7_4_5", 70, 1160), ("tiles_25_15_12", 600, 776), ("tiles_35_21_20_15", 600, 1160),
     ("tiles_3_2", 300, 104), ("tiles_8_4_3", 200, 768), ("tiles_12_8_6", 300, 768), ("tiles_14_7_8_5", 200, 1160)],
)
CASES = ([(f"rows-{l}", M, ROW_N, ROW_K) for l, M in CASES[0]] + [(f"cols-{l}", COL_M, N, COL_K) for l, N in CASES[1]] +
         [(f"k-{l}", RED_M, RED_N, K) for l, K in CASES[2]] + [(f"count-{l}", M, N, 64) for l, M, N in CASES[3]])
# B: ragged in M and N; N % 8 == 4 (192- and 384-column tiles); several tiles in both directions; M = 1
PADDED_CASES = [(200, 200, 128), (70, 196, 128), (70, 388, 128), (300, 776, 64), (1, 200, 128)]
RAGGED = (200, 200, 128)               # C, D: one shape ragged in M and N for every form


def cases_for(form):
    return [c for c in CASES if accepts(form, c[2], c[3])]


def case_id(form, case):
    return f"{form.name}-{case[0]}-{case[1]}x{case[2]}x{case[3]}"


# ------------------------------------------------------------------ problems
def scale_exp(K):
    return math.ceil(math.log2(K) / 2)


@functools.lru_cache(maxsize=None)
def host_problem(M, N, K):
    """A [M, K] from the integers -2 .. 2, B [N, K] from the same times 2^-s (s = ceil(log2(K) / 2)), bias multiples of 1/4 in
    [-1, 1], resid multiples of 1/4 in [-4, 4], aux from {0, +-0.25, 0.5, 1, 1.125}: all exact in bf16 and f16, every product and
    partial sum a multiple of 2^-s below 2^24 * 2^-s, so acc = A.B^T, u = acc + bias, u + resid and acc * aux are exact in fp32
    whatever the order of summation. Returns a dict of fp32 CPU tensors, with the fp64 gelu(u) and gelu'(u)."""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = torch.randint(-2, 3, (M, K), generator=g).float()
    B = torch.randint(-2, 3, (N, K), generator=g).float() * 2.0 ** -scale_exp(K)
    bias = torch.randint(-4, 5, (N,), generator=g).float() / 4
    resid = torch.randint(-16, 17, (M, N), generator=g).float() / 4
    aux = torch.tensor([0.0, 0.25, -0.25, 0.5, 1.0, 1.125])[torch.randint(0, 6, (M, N), generator=g)]
    acc = A @ B.t()
    u = acc + bias
    ud = u.double()
    cdf = 0.5 * (1.0 + torch.special.erf(ud / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * ud * ud) / math.sqrt(2.0 * math.pi)
    return dict(A=A, B=B, bias=bias, resid=resid, aux=aux, acc=acc, u=u, gelu=ud * cdf, dgelu=cdf + ud * pdf)


def expected(p, epi, dt):
    """(C, C2) a kernel must give EXACTLY for the epilogue (None: no such output); QST_EPI_GELU is compared by gelu_check"""
    if epi == EPI_BF16:
        return p["u"].to(dt), None
    if epi == EPI_F32_RESID:
        return p["u"] + p["resid"], None
    if epi == EPI_F32_RESID_BF16:
        return p["u"] + p["resid"], (p["u"] + p["resid"]).to(dt)
    if epi == EPI_GELU_BWD:
        return (p["acc"] * p["aux"]).to(dt), None
    raise ValueError(epi)


GUARD_ROWS, GUARD_COLS, VIEW_COL = 64, 72, 40      # a padded operand is [rows + 64, K + 72]; the view starts at column 40
C_GUARD_ROWS = 264                     # more than the tallest tile (256): a store that loses its row guard lands in the band
BIAS_GUARD = 8


def in_band(t, rows, width, guard_rows, guard_cols, col0, fill, dtype):
    """t as the view [:rows, col0 : col0 + width] of a [rows + guard_rows, width + guard_cols] device matrix of `fill`"""
    big = torch.full((rows + guard_rows, width + guard_cols), fill)
    big[:rows, col0:col0 + width] = t
    return big.to(dtype).cuda()[:rows, col0:col0 + width]


TAIL = 8                               # elements behind a DENSE aux (ones) or output (sentinels): one 16-byte vector of 16-bit ones


def with_tail(t, fill):
    """(a dense [M, N] view, the TAIL elements behind it) of one device buffer of M * N + TAIL elements: what a 16-byte access
    that starts inside the last row's last 8 bytes reaches"""
    flat = torch.full((t.numel() + TAIL,), fill, dtype=t.dtype, device=t.device)
    flat[:t.numel()] = t.reshape(-1)
    return flat[:t.numel()].view(t.shape), flat[t.numel():]


@functools.lru_cache(maxsize=None)
def dev_problem(op, M, N, K, pad=0):
    """host_problem on the device in the operand type. pad = 0: dense (aux with TAIL ones behind it: the 16-bit epilogues read
    whole 16-byte vectors of it). Otherwise A and B are views [:rows, 40 : 40 + K] of
    matrices [rows + 64, K + 72] of ONES (lda = ldb = K + 72: a read past the view's width adds to the sums), resid and aux
    views [:M, :N] of matrices [M + 64, N + pad] of ones, the output's leading dimension. bias has 8 sentinels behind N."""
    from kernel_helpers import OPDT
    p, dt = host_problem(M, N, K), OPDT[op]
    bias = torch.cat([p["bias"], torch.full((BIAS_GUARD,), SENTINEL)]).cuda()
    if not pad:
        return dict(A=p["A"].to(dt).cuda(), B=p["B"].to(dt).cuda(), bias=bias, resid=p["resid"].cuda(),
                    aux=with_tail(p["aux"].to(dt).cuda(), 1.0)[0])
    return dict(A=in_band(p["A"], M, K, GUARD_ROWS, GUARD_COLS, VIEW_COL, 1.0, dt),
                B=in_band(p["B"], N, K, GUARD_ROWS, GUARD_COLS, VIEW_COL, 1.0, dt), bias=bias,
                resid=in_band(p["resid"], M, N, GUARD_ROWS, pad, 0, 1.0, torch.float32),
                aux=in_band(p["aux"], M, N, GUARD_ROWS, pad, 0, 1.0, dt))


# ------------------------------------------------------------------ comparisons
def first_at(mask):
    m, n = [int(x) for x in mask.nonzero()[0]]
    return m, n, int(mask.sum())


def assert_exact(got, want, what):
    bad = got != want
    if bool(bad.any()):
        m, n, cnt = first_at(bad)
        raise AssertionError(f"{what}: {cnt} elements differ, first at (m, n) = ({m}, {n}): got {got[m, n].item()!r}, "
                             f"want {want[m, n].item()!r}")


def assert_band(full, M, N, what, fill=SENTINEL):
    """every element of `full` outside [:M, :N] still holds the sentinel"""
    bad = full != fill
    bad[:M, :N] = False
    if bool(bad.any()):
        m, n, cnt = first_at(bad)
        raise AssertionError(f"{what}: {cnt} elements written outside [{M}, {N}], first at (m, n) = ({m}, {n}): "
                             f"{full[m, n].item()!r}")


def assert_untouched(full, what, fill=SENTINEL):
    assert_band(full, 0, 0, what, fill)


MANT = {"bf16": (7, -126), "f16": (10, -14)}      # explicit mantissa bits, exponent of the smallest normal
# The kernels' erf is Abramowitz-Stegun 7.1.26 (csrc/qst_common.h gelu_parts2: |error| <= 1.5e-7 on erf, half of that on the
# cdf) evaluated in fp32, where 0.5 - 0.5 erf(|u| / sqrt 2) cancels for u < 0: an ABSOLUTE error of the cdf. gelu(u) = u cdf
# carries |u| times it. Far out on the negative side gelu(u) itself is below that error, so an error counted in ulps of the
# reference alone has no bound there; the comparison therefore allows GELU_ABS * max(1, |u|) next to the ulps of the operand type.
GELU_ABS = 1.5e-7
# Measured on gfx950 over every form, case and padded run of tests/test_gpu_nt_shapes.py, largest error beyond that term in
# ulps of the operand type: bf16 0.499 (gelu') / 0.493 (gelu), f16 0.493 / 0.488 -- and without the term, over |want| >= 2^-6:
# 0.499 / 0.495 and 0.498 / 0.488. The kernels round a value that is right to well below an ulp. Bound: the larger of 1 ulp
# and twice the measured maximum, i.e. 1 ulp.
GELU_ULPS = {"bf16": 1.0, "f16": 1.0}
GELU_SEEN = {}                         # (op, output[, "raw"]) -> the largest figure seen in this process, in ulps (for measuring)


def ulp_of(x, op):
    """the spacing of the operand type at |x| (fp64 tensor)"""
    mant, emin = MANT[op]
    e = torch.frexp(x.abs())[1].double() - 1                   # floor(log2 |x|); 0 for x = 0
    e = torch.where(x == 0, torch.full_like(e, emin), e).clamp(min=emin)
    return torch.ldexp(torch.ones_like(x), (e - mant).to(torch.int32))


def gelu_check(got, want, u, op, output, what):
    """got (16-bit, the kernel's) against want (fp64, of the exact u): |got - want| <= GELU_ULPS ulps of the operand type at
    want + GELU_ABS * max(1, |u|), and never more than rtol 8e-3 / atol 2e-2 (the bound of test_gemm_nt_epilogues)."""
    err = (got.double() - want).abs()
    ulps = (err - GELU_ABS * u.double().abs().clamp(min=1.0)).clamp(min=0.0) / ulp_of(want, op)
    GELU_SEEN[(op, output)] = max(GELU_SEEN.get((op, output), 0.0), float(ulps.max()))
    big = want.abs() >= 2.0 ** -6                                # ... and without the absolute term, where want is not tiny
    if bool(big.any()):
        raw = float((err / ulp_of(want, op))[big].max())
        GELU_SEEN[(op, output, "raw")] = max(GELU_SEEN.get((op, output, "raw"), 0.0), raw)
    bad = (ulps > GELU_ULPS[op]) | (err > 8e-3 * want.abs() + 2e-2)
    if bool(bad.any()):
        m, n, cnt = first_at(bad)
        raise AssertionError(f"{what} {output}: {cnt} elements outside {GELU_ULPS[op]} ulp, first at (m, n) = ({m}, {n}): got "
                             f"{got[m, n].item()!r}, want {want[m, n].item()!r} ({ulps[m, n].item():.2f} ulp over)")


# ------------------------------------------------------------------ the launch
def call(entry, form, a, epi):
    """entry -- kf(lib, "qst_gemm_nt", op) or kf(lib, "qst_gemm_nt8", op), named by the caller -- on `a` in `form`; the status"""
    from kernel_helpers import stream
    if form.call == "nt":
        a.splits = form.sel
        return entry(a, epi, stream())
    return entry(a, epi, form.sel, stream())


def run(entry, op, form, M, N, K, padded=False, drop=None, pad=GUARD_COLS, epis=None):
    """Every epilogue `form` accepts (or `epis`), each on sentinel-filled C and C2, compared EXACTLY with the references of
    host_problem on [:M, :N] (QST_EPI_GELU: gelu_check); with `padded`, operands, resid and aux inside bands of ones
    (dev_problem), C and C2 [M + 264, N + pad], and every element outside [:M, :N], the whole C2 of an epilogue without one
    and the 8 elements behind bias must still hold the sentinel. Dense, C and C2 have TAIL sentinels behind the last row, which
    must survive too: all a dense output shows of a 16-byte store where 8 bytes belong to the row (inside, the next row's own
    store lands on top).
    drop: a QstDrop for drop_where 1 -- only the fp32 epilogues run and nothing is compared here but the bands.
    Returns {epi: (C[:M, :N], C2[:M, :N] or None)} on the CPU."""
    from kernel_helpers import OPDT, gemm_args
    from quadruplet_sentence_transformer_amd import _lib
    dt, p = OPDT[op], host_problem(M, N, K)
    d = dev_problem(op, M, N, K, pad if padded else 0)
    rows, ld = (M + C_GUARD_ROWS, N + pad) if padded else (M, N)
    assert accepts(form, N, K, d["A"].stride(0), d["B"].stride(0), ld, d["resid"].stride(0)), (form.name, M, N, K, ld)
    out = {}
    for epi in (form.epis if epis is None else epis):
        if drop is not None and epi not in F32_EPIS:
            continue
        what = f"{form.name} ({op}) QST_EPI_{EPI_NAMES[epi]} at M, N, K = {M}, {N}, {K}, ldc = {ld}"
        Cd = torch.full((rows, ld), SENTINEL, dtype=torch.float32 if epi in F32_EPIS else dt, device="cuda")
        C2d = torch.full((rows, ld), SENTINEL, dtype=dt, device="cuda")
        if not padded:                                             # dense: what lies behind the last row is the tail's sentinels
            (Cd, tail), (C2d, tail2) = with_tail(Cd, SENTINEL), with_tail(C2d, SENTINEL)
        kw = dict(A=d["A"], B=d["B"], C=Cd, C2=C2d, M=M, N=N, K=K, lda=d["A"].stride(0), ldb=d["B"].stride(0), ldc=ld)
        if epi == EPI_GELU_BWD:
            kw.update(aux=d["aux"])
        else:
            kw.update(bias=d["bias"])
        if epi in F32_EPIS:
            kw.update(resid=d["resid"], ldr=d["resid"].stride(0))
        if drop is not None:
            kw.update(drop=drop, drop_where=1)
        _lib.check(call(entry, form, gemm_args(**kw), epi), what)
        C, C2 = Cd.cpu(), C2d.cpu()
        assert_band(C, M, N, what + ", C")
        has_c2 = epi in (EPI_GELU, EPI_F32_RESID_BF16)
        assert_band(C2, M if has_c2 else 0, N if has_c2 else 0, what + ", C2")
        if not padded:
            assert bool((tail == SENTINEL).all()) and bool((tail2 == SENTINEL).all()), f"{what}: written behind the last row"
        got, got2 = C[:M, :N], (C2[:M, :N] if has_c2 else None)
        if drop is None and epi == EPI_GELU:
            gelu_check(got, p["dgelu"], p["u"], op, "C = gelu'(u)", what)
            gelu_check(got2, p["gelu"], p["u"], op, "C2 = gelu(u)", what)
        elif drop is None:
            want, want2 = expected(p, epi, dt)
            assert_exact(got, want, what + ", C")
            if has_c2:
                assert_exact(got2, want2, what + ", C2")
        out[epi] = (got, got2)
    bias = d["bias"].cpu()
    assert bool((bias[N:] == SENTINEL).all()) and torch.equal(bias[:N], p["bias"]), f"{form.name}: bias was written"
    return out
