// dense_head.hip -- sentence-transformers 2.2.2's models.Dense after pooling, with the models.Normalize that may follow it:
//
//   qst_dense_head_fwd  z = x W^T + b;  a = act(z), act identity or tanh;  y = a, or a / max(|a|, 1e-12) per row (F.normalize)
//   qst_dense_head_bwd  dy -> grad_x, grad_w, grad_b, all written (not accumulated)
//
// All fp32, on the caller's stream, no host synchronisation, no atomics, every sum in a fixed order: the same inputs give the
// same bits. The three products (x W^T, dz W, dz^T x) run on the LDS-tiled fp32 FMA loop of fp32_tile.h (64 x 64 outputs per
// 256-thread workgroup, K panels of 16, the next panel prefetched into registers), every tile edge guarded: at a training
// shape (256 rows, 384 -> 384) they are 0.23 GFLOP next to an encoder step of 2.2 TFLOP, the reasoning of cross.hip.
//
// Stages, forward:   1. gemm NT  y = act(x W^T + b)
//                    2. rownorm  normalize only, one wave per row: row_norm = |a|, y = a / max(row_norm, 1e-12) in place
// backward:          1. dz       one wave per row, into the workspace:
//                                  normalize: da = (dy - y <y, dy>) / max(row_norm, 1e-12); a row on the clamp (row_norm <
//                                  1e-12) gets dy / 1e-12, as torch's clamp_min does;  tanh: dz = da * (1 - a^2)
//                                (identity without normalize: dz is dy itself and this stage is skipped)
//                    2. gemm NN  grad_x = dz W
//                    3. gemm TN  grad_w = dz^T x, the rows (the K of this product) in slices of at least 64 whose partial
//                                sums land in the workspace; colsum  grad_b = the column sums of dz, in the same slices
//                    4. combine  more than one slice: the partial sums added in the order of the slices
// What is kept between forward and backward: y and, with normalize, one norm per row. No pre-normalisation copy: a is
// recovered as y * max(row_norm, 1e-12), one rounding (6e-8 relative) away from the forward's a, which enters the gradients
// only through 1 - a^2 -- far inside the 1e-4 relative the gradients are held to.
#include "qst_common.h"

namespace {

#include "fp32_tile.h"

constexpr float kNormEps = 1e-12f;      // F.normalize's eps
constexpr int kMaxDim = 8192;           // Din, Dout
constexpr int kMaxRows = 1 << 29;       // B: rows and tiles (at most 2^23 x 128) are counted in 32 bits
constexpr int kSliceRows = 64;          // rows one slice of the weight gradient walks before another slice takes over ...
constexpr int kMaxSlices = 16;          // ... up to this many slices ...
constexpr int kSliceBlocks = 1024;      // ... and while slices * tiles stays below this (4 workgroups a CU); past either the slices grow

inline int wgrad_slices(int B, int Din, int Dout) {
    const int tiles = ((Dout + kTile - 1) / kTile) * ((Din + kTile - 1) / kTile);
    int s = (B + kSliceRows - 1) / kSliceRows;
    if (s > kMaxSlices) s = kMaxSlices;
    if (s > kSliceBlocks / tiles) s = kSliceBlocks / tiles;
    return s < 1 ? 1 : s;
}

// ---- workspace layout (floats; every segment starts on a multiple of 4)
struct DenseWs {
    size_t dz, pw, pb, total;
    int ldz, slices;
};
inline DenseWs dense_layout(int B, int Din, int Dout) {
    DenseWs w;
    w.ldz = (int)pad4((size_t)Dout);
    w.slices = wgrad_slices(B, Din, Dout);
    size_t o = 0;
    w.dz = o; o += (size_t)B * w.ldz;
    w.pw = o; if (w.slices > 1) o += pad4((size_t)w.slices * Dout * Din);
    w.pb = o; if (w.slices > 1) o += (size_t)w.slices * w.ldz;
    w.total = o;
    return w;
}

__device__ __forceinline__ float act_apply(float z, int act) { return act == QST_DENSE_ACT_TANH ? tanhf(z) : z; }

// ---- C[M, N] = act(sum_k A(m, k) * B(k, n) + bias[n]) over the k of this workgroup's slice (blockIdx.y)
// AK: A(m, k) = A[m * lda + k] (k contiguous), else A[k * lda + m]. BKC: B(k, n) = Bm[n * ldb + k], else Bm[k * ldb + n].
struct GemmP {
    const float* A; const float* Bm; float* C;
    int M, N, K, lda, ldb, ldc;
    const float* bias;                  // per n (null = none)
    int act;
    int k_per_slice;                    // slice s takes k in [s * k_per_slice, min(K, (s + 1) * k_per_slice)) ...
    size_t slice_stride;                // ... and writes C + s * slice_stride
    int vecA, vecB, vecC;               // 16-byte accesses allowed (leading dimension % 4 == 0, pointer aligned)
    int tiles_n;
};

template <bool AK, bool BKC>
__global__ __launch_bounds__(256) void dense_gemm_kernel(GemmP p) {
    __shared__ __attribute__((aligned(16))) float As[kBK][kLdT];
    __shared__ __attribute__((aligned(16))) float Bs[kBK][kLdT];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int m0 = (int)(blockIdx.x / p.tiles_n) * kTile, n0 = (int)(blockIdx.x % p.tiles_n) * kTile;
    const int kb = (int)blockIdx.y * p.k_per_slice;
    const int ke = min(p.K, kb + p.k_per_slice);
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    float ra[4], rb[4];
    panel_load<AK>(p.A, p.lda, p.M, ke, m0, kb, p.vecA != 0, nullptr, ra);
    panel_load<BKC>(p.Bm, p.ldb, p.N, ke, n0, kb, p.vecB != 0, nullptr, rb);
    for (int k0 = kb; k0 < ke; k0 += kBK) {
        panel_store<AK>(As, ra);
        panel_store<BKC>(Bs, rb);
        __syncthreads();
        if (k0 + kBK < ke) {            // the next panel travels while this one is multiplied
            panel_load<AK>(p.A, p.lda, p.M, ke, m0, k0 + kBK, p.vecA != 0, nullptr, ra);
            panel_load<BKC>(p.Bm, p.ldb, p.N, ke, n0, k0 + kBK, p.vecB != 0, nullptr, rb);
        }
#pragma unroll
        for (int k = 0; k < kBK; ++k) {
            const f32x4 av = *(const f32x4*)&As[k][ty * 4];
            const f32x4 bv = *(const f32x4*)&Bs[k][tx * 4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }

    const int n = n0 + tx * 4;
    if (n >= p.N) return;
    float bs[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (n + j < p.N) bs[j] = p.bias[n + j];
    }
    float* C = p.C + (size_t)blockIdx.y * p.slice_stride;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m >= p.M) break;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = act_apply(acc[i][j] + bs[j], p.act);
        float* q = C + (size_t)m * p.ldc + n;
        if (p.vecC && n + 3 < p.N) *(f32x4*)q = f32x4{v[0], v[1], v[2], v[3]};
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (n + j < p.N) q[j] = v[j];
        }
    }
}

template <bool AK, bool BKC>
int launch_gemm(GemmP p, int slices, hipStream_t st) {
    p.vecA = (p.lda % 4 == 0) && al16(p.A);
    p.vecB = (p.ldb % 4 == 0) && al16(p.Bm);
    p.vecC = (p.ldc % 4 == 0) && al16(p.C) && (slices == 1 || p.slice_stride % 4 == 0);
    p.k_per_slice = (p.K + slices - 1) / slices;
    const int64_t tm = ((int64_t)p.M + kTile - 1) / kTile, tn = ((int64_t)p.N + kTile - 1) / kTile;
    p.tiles_n = (int)tn;
    dense_gemm_kernel<AK, BKC><<<dim3((unsigned)(tm * tn), (unsigned)slices), 256, 0, st>>>(p);
    QST_LAUNCH_CHECK();
    return QST_OK;
}

// ---- forward 2: one wave per row, in place: row_norm = |a|, y = a / max(|a|, eps). A lane sums its columns in order, the
// wave tree is fixed.
__global__ __launch_bounds__(256) void dense_rownorm_kernel(float* y, int B, int Dout, float* row_norm) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    float* a = y + (size_t)row * Dout;
    float s = 0.f;
    for (int i = lane; i < Dout; i += 64) s = __builtin_fmaf(a[i], a[i], s);
    s = wave_sum(s);
    const float n = sqrtf(s);
    const float d = fmaxf(n, kNormEps);
    for (int i = lane; i < Dout; i += 64) a[i] = a[i] / d;
    if (lane == 0) row_norm[row] = n;
}

// ---- backward 1: one wave per row: dz [B, ldz] from y, dy and the row's norm
__global__ __launch_bounds__(256) void dense_dz_kernel(const float* y, const float* dy, const float* row_norm, int B, int Dout,
                                                       int act, int normalize, float* dz, int ldz) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const float* yr = y + (size_t)row * Dout;
    const float* gr = dy + (size_t)row * Dout;
    float* zr = dz + (size_t)row * ldz;
    float dot = 0.f, r = 1.f, d = 1.f;
    bool clamped = false;
    if (normalize) {
        for (int i = lane; i < Dout; i += 64) dot = __builtin_fmaf(yr[i], gr[i], dot);
        dot = wave_sum(dot);
        const float n = row_norm[row];
        clamped = n < kNormEps;
        d = fmaxf(n, kNormEps);
        r = 1.f / d;
    }
    for (int i = lane; i < Dout; i += 64) {
        const float yi = yr[i];
        float da = gr[i], a = yi;
        if (normalize) {
            da = (clamped ? da : __builtin_fmaf(-yi, dot, da)) * r;
            a = yi * d;
        }
        zr[i] = act == QST_DENSE_ACT_TANH ? da * __builtin_fmaf(-a, a, 1.f) : da;
    }
}

// ---- backward 3: out[slice][n] = sum of dz[r, n] over the rows of the slice, in order. grid (ceil(Dout / 256), slices)
__global__ __launch_bounds__(256) void dense_colsum_kernel(const float* dz, int ldz, int B, int Dout, int rows_per_slice,
                                                           float* out, int ldo) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= Dout) return;
    const int r0 = (int)blockIdx.y * rows_per_slice;
    const int r1 = min(B, r0 + rows_per_slice);
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += dz[(size_t)r * ldz + n];
    out[(size_t)blockIdx.y * ldo + n] = s;
}

// ---- backward 4: element e of out [n]: the slices' partial sums added in the order of the slices
__global__ __launch_bounds__(256) void dense_combine_kernel(const float* part, int slices, size_t stride, int64_t n, float* out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float s = 0.f;
    for (int i = 0; i < slices; ++i) s += part[(size_t)i * stride + e];
    out[e] = s;
}

inline bool shape_ok(int B, int Din, int Dout) {
    return B >= 1 && B <= kMaxRows && Din >= 1 && Din <= kMaxDim && Dout >= 1 && Dout <= kMaxDim;
}
int dense_check(int B, int Din, int Dout, int act, int normalize) {
    if (act != QST_DENSE_ACT_IDENTITY && act != QST_DENSE_ACT_TANH) return QST_ERR_BAD_ARG;
    if (normalize != 0 && normalize != 1) return QST_ERR_BAD_ARG;
    if (!shape_ok(B, Din, Dout)) return QST_ERR_UNSUPPORTED;
    return QST_OK;
}

}  // namespace

extern "C" int qst_dense_head_fwd(const float* x, int ldx, const float* w, const float* b, int B, int Din, int Dout, int act,
                                  int normalize, float* y, float* row_norm, void* stream) {
    if (!x || !w || !y) return QST_ERR_BAD_ARG;
    const int rc = dense_check(B, Din, Dout, act, normalize);
    if (rc != QST_OK) return rc;
    if (ldx < Din || (normalize && !row_norm)) return QST_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    GemmP p = {};
    p.A = x; p.lda = ldx; p.Bm = w; p.ldb = Din; p.C = y; p.ldc = Dout;
    p.M = B; p.N = Dout; p.K = Din; p.bias = b; p.act = act;
    const int grc = launch_gemm<true, true>(p, 1, st);
    if (grc != QST_OK) return grc;
    if (normalize) {
        dense_rownorm_kernel<<<(unsigned)(((int64_t)B + 3) / 4), 256, 0, st>>>(y, B, Dout, row_norm);
        QST_LAUNCH_CHECK();
    }
    return QST_OK;
}

extern "C" size_t qst_dense_head_bwd_workspace_bytes(int B, int Din, int Dout) {
    if (!shape_ok(B, Din, Dout)) return 0;
    return dense_layout(B, Din, Dout).total * sizeof(float);
}

extern "C" int qst_dense_head_bwd(const float* x, int ldx, const float* w, const float* y, const float* row_norm,
                                  const float* dy, int B, int Din, int Dout, int act, int normalize, float* grad_x,
                                  float* grad_w, float* grad_b, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !w || !y || !dy || !grad_x || !grad_w || !workspace) return QST_ERR_BAD_ARG;
    const int rc = dense_check(B, Din, Dout, act, normalize);
    if (rc != QST_OK) return rc;
    if (ldx < Din || (normalize && !row_norm)) return QST_ERR_BAD_ARG;
    const DenseWs L = dense_layout(B, Din, Dout);
    if (workspace_bytes < L.total * sizeof(float) || !al16(workspace)) return QST_ERR_BAD_ARG;

    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const unsigned row_grid = (unsigned)(((int64_t)B + 3) / 4);
    const float* dz = dy;
    int ldz = Dout;
    if (normalize || act != QST_DENSE_ACT_IDENTITY) {
        dense_dz_kernel<<<row_grid, 256, 0, st>>>(y, dy, row_norm, B, Dout, act, normalize, ws + L.dz, L.ldz);
        QST_LAUNCH_CHECK();
        dz = ws + L.dz; ldz = L.ldz;
    }
    // grad_x [B, Din] = dz [B, Dout] . W [Dout, Din]
    GemmP px = {};
    px.A = dz; px.lda = ldz; px.Bm = w; px.ldb = Din; px.C = grad_x; px.ldc = Din;
    px.M = B; px.N = Din; px.K = Dout; px.act = QST_DENSE_ACT_IDENTITY;
    int grc = launch_gemm<true, false>(px, 1, st);
    if (grc != QST_OK) return grc;
    // grad_w [Dout, Din] = dz^T [Dout, B] . x [B, Din], the rows in slices
    const int slices = L.slices;
    GemmP pw = {};
    pw.A = dz; pw.lda = ldz; pw.Bm = x; pw.ldb = ldx; pw.ldc = Din;
    pw.M = Dout; pw.N = Din; pw.K = B; pw.act = QST_DENSE_ACT_IDENTITY;
    pw.C = slices == 1 ? grad_w : ws + L.pw;
    pw.slice_stride = (size_t)Dout * Din;
    grc = launch_gemm<false, false>(pw, slices, st);
    if (grc != QST_OK) return grc;
    const int rows_per_slice = (B + slices - 1) / slices;      // launch_gemm's k_per_slice
    if (grad_b) {
        dense_colsum_kernel<<<dim3((unsigned)((Dout + 255) / 256), (unsigned)slices), 256, 0, st>>>(
            dz, ldz, B, Dout, rows_per_slice, slices == 1 ? grad_b : ws + L.pb, L.ldz);
        QST_LAUNCH_CHECK();
    }
    if (slices > 1) {
        const int64_t nw = (int64_t)Dout * Din;
        dense_combine_kernel<<<(unsigned)((nw + 255) / 256), 256, 0, st>>>(ws + L.pw, slices, (size_t)nw, nw, grad_w);
        QST_LAUNCH_CHECK();
        if (grad_b) {
            dense_combine_kernel<<<(unsigned)((Dout + 255) / 256), 256, 0, st>>>(ws + L.pb, slices, (size_t)L.ldz, Dout, grad_b);
            QST_LAUNCH_CHECK();
        }
    }
    return QST_OK;
}
