// mnrl.hip -- MultipleNegativesRankingLoss and its symmetric form (sentence-transformers 2.2.2), forward + backward in fp32.
//
// Unlike the row-wise losses of tuple_loss.hip every anchor is scored against every candidate of the batch:
//   S = scale * sim(a, c) [B, N];  loss = mean_i(logsumexp_j S[i, j] - S[i, i])   (+ the same over the columns of S[:, :B], / 2)
// Stages (all on the caller's stream, no host synchronisation, no atomics):
//   1. rnorm    cos only: |x| and 1 / max(|x|, 1e-12) of every row of a and c, one wave per row
//   2. gemm NT  S[i, j] = scale * r_a[i] * r_c[j] * <a_i, c_j> into the workspace, leading dimension N rounded up to 4
//   3. colstat  symmetric only: max and sum of exponentials of every column of the B x B block, 64 columns per workgroup --
//               BEFORE the row pass, which overwrites the scores
//   4. row      one workgroup per anchor: max, sum of exponentials, the row's loss term; with gradients S[i, :] becomes
//               G[i, :] = w * ((softmax_row - onehot) + (softmax_col - onehot)[j < B]) / B, w = 1 or 1/2
//   5. loss     one workgroup: the fixed-order sum of the row (and column) terms
//   6. gemm NN  d_hat_a = scale * G . c_hat        gemm TN  d_hat_c = scale * G^T . a_hat       (into grad_a / grad_c)
//   7. normbwd  cos only, in place: r * (d_hat - x_hat * <x_hat, d_hat>); a row with |x| < 1e-12 gets d_hat / 1e-12 as
//               torch's clamp does
// The upstream gradient *grad_out multiplies the FINISHED gradient (stage 7, or the epilogue of stage 6 for dot): the
// gradients of a call with grad_out = g are the correctly rounded g * (gradients of a call without), and the loss scale of
// use_amp (65536) never enters an intermediate.
//
// The three products run on one LDS-tiled fp32 FMA loop (fp32_tile.h: 64 x 64 outputs per 256-thread workgroup, K panels of 16 through
// LDS, 4 x 4 outputs per thread, the next panel prefetched into registers): the embeddings are fp32, sentence-transformers
// computes this loss in fp32, and at training shapes the products are a few hundred MFLOP next to an encoder step of
// milliseconds. Every tile edge is guarded, every index is 64-bit.
#include "qst_common.h"

namespace {

#include "fp32_tile.h"

constexpr float kNormEps = 1e-12f;      // F.normalize's eps

// ---- workspace layout (floats; every segment starts on a multiple of 4)
struct MnrlWs {
    size_t rinv, nrm, rowterm, colterm, cmax, csum, S, total;
    int ldS;
};
inline MnrlWs mnrl_layout(int B, int N) {
    MnrlWs w;
    w.ldS = (int)pad4((size_t)N);
    size_t o = 0;
    w.rinv = o; o += pad4((size_t)B + N);
    w.nrm = o; o += pad4((size_t)B + N);
    w.rowterm = o; o += pad4((size_t)B);
    w.colterm = o; o += pad4((size_t)B);
    w.cmax = o; o += pad4((size_t)B);
    w.csum = o; o += pad4((size_t)B);
    w.S = o; o += (size_t)B * w.ldS;
    w.total = o;
    return w;
}

// ---- 1. row norms of a (rows 0 .. B-1) and c (rows B .. B+N-1)
template <bool VEC>
__global__ __launch_bounds__(256) void mnrl_rnorm_kernel(const float* a, const float* c, int B, int N, int D,
                                                         float* rinv, float* nrm) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)B + N) return;
    const float* x = row < B ? a + (size_t)row * D : c + (size_t)(row - B) * D;
    float s = 0.f;
    if (VEC) {
        const int nv = D >> 2;
        for (int v = lane; v < nv; v += 64) {
            const f32x4 X = *(const f32x4*)(x + (size_t)v * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) s = __builtin_fmaf(X[j], X[j], s);
        }
    } else {
        for (int i = lane; i < D; i += 64) s = __builtin_fmaf(x[i], x[i], s);
    }
    s = wave_sum(s);
    const float n = sqrtf(s);
    if (lane == 0) { nrm[row] = n; rinv[row] = 1.f / fmaxf(n, kNormEps); }
}

// ---- 2. / 6. C[M, N] = alpha * mscale[m] * nscale[n] * g * sum_k A(m, k) * kscale[k] * B(k, n)
// AK: A(m, k) = A[m * lda + k] (k contiguous), else A[k * lda + m]. BKC: B(k, n) = Bm[n * ldb + k], else Bm[k * ldb + n].
struct GemmP {
    const float* A; const float* Bm; float* C;
    int M, N, K, lda, ldb, ldc;
    const float* kscale;                // per k, applied to an n-contiguous B operand as its panel is loaded (null = 1)
    const float* mscale; const float* nscale;   // null = 1
    const float* gout;                  // device scalar (null = 1)
    float alpha;
    int vecA, vecB, vecC;               // 16-byte accesses allowed (leading dimension % 4 == 0, pointer aligned)
    int tiles_n;
};

template <bool AK, bool BKC>
__global__ __launch_bounds__(256) void mnrl_gemm_kernel(GemmP p) {
    __shared__ __attribute__((aligned(16))) float As[kBK][kLdT];
    __shared__ __attribute__((aligned(16))) float Bs[kBK][kLdT];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int m0 = (int)(blockIdx.x / p.tiles_n) * kTile, n0 = (int)(blockIdx.x % p.tiles_n) * kTile;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    float ra[4], rb[4];
    panel_load<AK>(p.A, p.lda, p.M, p.K, m0, 0, p.vecA != 0, nullptr, ra);
    panel_load<BKC>(p.Bm, p.ldb, p.N, p.K, n0, 0, p.vecB != 0, p.kscale, rb);
    for (int k0 = 0; k0 < p.K; k0 += kBK) {
        panel_store<AK>(As, ra);
        panel_store<BKC>(Bs, rb);
        __syncthreads();
        if (k0 + kBK < p.K) {           // the next panel travels while this one is multiplied
            panel_load<AK>(p.A, p.lda, p.M, p.K, m0, k0 + kBK, p.vecA != 0, nullptr, ra);
            panel_load<BKC>(p.Bm, p.ldb, p.N, p.K, n0, k0 + kBK, p.vecB != 0, p.kscale, rb);
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

    const float g = p.gout ? p.gout[0] : 1.f;
    const int n = n0 + tx * 4;
    if (n >= p.N) return;
    float ns[4] = {1.f, 1.f, 1.f, 1.f};
    if (p.nscale) {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (n + j < p.N) ns[j] = p.nscale[n + j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m >= p.M) break;
        const float ms = p.mscale ? p.mscale[m] : 1.f;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // a chain of single multiplications: the value without grad_out, then times g
            float x = acc[i][j] * p.alpha;
            x = x * ms;
            x = x * ns[j];
            v[j] = x * g;
        }
        float* q = p.C + (size_t)m * p.ldc + n;
        if (p.vecC && n + 3 < p.N) *(f32x4*)q = f32x4{v[0], v[1], v[2], v[3]};
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (n + j < p.N) q[j] = v[j];
        }
    }
}

// ---- 3. column statistics of the B x B block (symmetric loss): 64 columns per workgroup, wave w takes rows w, w + 4, ...
__global__ __launch_bounds__(256) void mnrl_colstat_kernel(const float* S, int ldS, int B, float* cmax, float* csum,
                                                           float* colterm) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane;
    const bool in = j < B;
    float mx = -__builtin_inff();
    if (in) for (int i = w; i < B; i += 4) mx = fmaxf(mx, S[(size_t)i * ldS + j]);
    part[w][lane] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(part[0][lane], part[1][lane]), fmaxf(part[2][lane], part[3][lane]));
    __syncthreads();
    float sm = 0.f;
    if (in) for (int i = w; i < B; i += 4) sm += expf(S[(size_t)i * ldS + j] - mx);
    part[w][lane] = sm;
    __syncthreads();
    if (w == 0 && in) {
        sm = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        cmax[j] = mx;
        csum[j] = sm;
        colterm[j] = (logf(sm) + mx) - S[(size_t)j * ldS + j];
    }
}

// ---- 4. the row pass
__global__ __launch_bounds__(256) void mnrl_row_kernel(float* S, int ldS, int B, int N, int symmetric, const float* cmax,
                                                       const float* csum, float* rowterm, int want_g) {
    __shared__ float part[4];
    const int i = blockIdx.x, t = threadIdx.x;
    float* s = S + (size_t)i * ldS;
    const float sii = s[i];             // every thread, before the first barrier: the write pass below replaces it
    float mx = -__builtin_inff();
    for (int j = t; j < N; j += 256) mx = fmaxf(mx, s[j]);
    mx = block_max<4>(mx, part);
    float sm = 0.f;
    for (int j = t; j < N; j += 256) sm += expf(s[j] - mx);
    sm = block_sum<4>(sm, part);
    if (t == 0) rowterm[i] = (logf(sm) + mx) - sii;
    if (!want_g) return;
    const float coef = (symmetric ? 0.5f : 1.f) / (float)B;
    const float inv = 1.f / sm;
    for (int j = t; j < N; j += 256) {
        const float v = s[j];
        const float hot = j == i ? 1.f : 0.f;
        float pr = expf(v - mx) * inv - hot;
        if (symmetric && j < B) pr += expf(v - cmax[j]) / csum[j] - hot;
        s[j] = coef * pr;
    }
}

// ---- 5. the loss: a fixed tree over the row terms (and the column terms)
__global__ __launch_bounds__(1024) void mnrl_loss_kernel(const float* rowterm, const float* colterm, int B, float* out) {
    __shared__ float part[16];
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += 1024) s += rowterm[i];
    s = block_sum<16>(s, part);
    float w = 1.f;
    if (colterm) {
        float c = 0.f;
        for (int i = threadIdx.x; i < B; i += 1024) c += colterm[i];
        c = block_sum<16>(c, part);
        s += c;
        w = 0.5f;
    }
    if (threadIdx.x == 0) out[0] = s * (w / (float)B);
}

// ---- 7. backward of F.normalize, in place on the rows of grad_a and grad_c (which hold d_hat), times *grad_out
template <bool VEC>
__global__ __launch_bounds__(256) void mnrl_normbwd_kernel(const float* a, const float* c, float* ga, float* gc, int B, int N,
                                                           int D, const float* rinv, const float* nrm, const float* gout) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)B + N) return;
    const float* x = row < B ? a + (size_t)row * D : c + (size_t)(row - B) * D;
    float* d = row < B ? ga + (size_t)row * D : gc + (size_t)(row - B) * D;
    const float r = rinv[row];
    const bool clamped = nrm[row] < kNormEps;   // clamp_min passes no gradient to the norm: d_hat / eps
    const float g = gout ? gout[0] : 1.f;
    float dot = 0.f;
    if (VEC) {
        const int nv = D >> 2;
        for (int v = lane; v < nv; v += 64) {
            const f32x4 X = *(const f32x4*)(x + (size_t)v * 4), G = *(const f32x4*)(d + (size_t)v * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) dot = __builtin_fmaf(X[j] * r, G[j], dot);
        }
    } else {
        for (int i = lane; i < D; i += 64) dot = __builtin_fmaf(x[i] * r, d[i], dot);
    }
    dot = wave_sum(dot);
    // each element is read and then written by the same lane
    if (VEC) {
        const int nv = D >> 2;
        for (int v = lane; v < nv; v += 64) {
            const f32x4 X = *(const f32x4*)(x + (size_t)v * 4), G = *(const f32x4*)(d + (size_t)v * 4);
            f32x4 O;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float tt = clamped ? G[j] : __builtin_fmaf(-(X[j] * r), dot, G[j]);
                const float y = r * tt;
                O[j] = y * g;
            }
            *(f32x4*)(d + (size_t)v * 4) = O;
        }
    } else {
        for (int i = lane; i < D; i += 64) {
            const float tt = clamped ? d[i] : __builtin_fmaf(-(x[i] * r), dot, d[i]);
            const float y = r * tt;
            d[i] = y * g;
        }
    }
}

template <bool AK, bool BKC>
int launch_gemm(GemmP p, hipStream_t st) {
    p.vecA = (p.lda % 4 == 0) && al16(p.A);
    p.vecB = (p.ldb % 4 == 0) && al16(p.Bm);
    p.vecC = (p.ldc % 4 == 0) && al16(p.C);
    const int64_t tm = ((int64_t)p.M + kTile - 1) / kTile, tn = ((int64_t)p.N + kTile - 1) / kTile;
    if (tm * tn > 0x7FFFFFFFLL) return QST_ERR_UNSUPPORTED;
    p.tiles_n = (int)tn;
    mnrl_gemm_kernel<AK, BKC><<<(unsigned)(tm * tn), 256, 0, st>>>(p);
    QST_LAUNCH_CHECK();
    return QST_OK;
}

}  // namespace

extern "C" size_t qst_mnrl_workspace_bytes(int B, int N, int D) {
    if (B < 1 || N < B || D < 1) return 0;
    return mnrl_layout(B, N).total * sizeof(float);
}

extern "C" int qst_mnrl_loss(const float* a, const float* c, int B, int N, int D, int sim, float scale, int symmetric,
                             float* out_loss, const float* grad_out, float* grad_a, float* grad_c,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 1 || N < B || D < 1 || !a || !c || !out_loss || !workspace) return QST_ERR_BAD_ARG;
    if (sim != QST_SCORE_DOT && sim != QST_SCORE_COS) return QST_ERR_BAD_ARG;
    if (symmetric != 0 && symmetric != 1) return QST_ERR_BAD_ARG;
    if (!(scale > 0.f) || !(scale < __builtin_inff())) return QST_ERR_BAD_ARG;   // NaN fails the first comparison
    if ((grad_a == nullptr) != (grad_c == nullptr)) return QST_ERR_BAD_ARG;
    if (((uintptr_t)workspace & 3) != 0) return QST_ERR_BAD_ARG;
    const MnrlWs L = mnrl_layout(B, N);
    if (workspace_bytes < L.total * sizeof(float)) return QST_ERR_BAD_ARG;
    // the kernels index in 64 bits; rows and tiles are counted in 32
    if ((int64_t)B * L.ldS > 0x7FFFFFFFLL || (int64_t)N * D > 0x7FFFFFFFLL) return QST_ERR_UNSUPPORTED;

    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    float* rinv = ws + L.rinv;
    float* nrm = ws + L.nrm;
    float* S = ws + L.S;
    const bool cos = sim == QST_SCORE_COS, want_g = grad_a != nullptr;
    const bool vec_in = (D % 4 == 0) && al16(a) && al16(c);
    const unsigned row_grid = (unsigned)(((int64_t)B + N + 3) / 4);

    if (cos) {
        if (vec_in) mnrl_rnorm_kernel<true><<<row_grid, 256, 0, st>>>(a, c, B, N, D, rinv, nrm);
        else mnrl_rnorm_kernel<false><<<row_grid, 256, 0, st>>>(a, c, B, N, D, rinv, nrm);
        QST_LAUNCH_CHECK();
    }
    GemmP p = {};
    p.A = a; p.lda = D; p.Bm = c; p.ldb = D; p.C = S; p.ldc = L.ldS;
    p.M = B; p.N = N; p.K = D; p.alpha = scale;
    p.mscale = cos ? rinv : nullptr; p.nscale = cos ? rinv + B : nullptr;
    int rc = launch_gemm<true, true>(p, st);
    if (rc != QST_OK) return rc;

    if (symmetric) {
        mnrl_colstat_kernel<<<(unsigned)((B + 63) / 64), 256, 0, st>>>(S, L.ldS, B, ws + L.cmax, ws + L.csum, ws + L.colterm);
        QST_LAUNCH_CHECK();
    }
    mnrl_row_kernel<<<(unsigned)B, 256, 0, st>>>(S, L.ldS, B, N, symmetric, ws + L.cmax, ws + L.csum, ws + L.rowterm,
                                                 want_g ? 1 : 0);
    QST_LAUNCH_CHECK();
    mnrl_loss_kernel<<<1, 1024, 0, st>>>(ws + L.rowterm, symmetric ? ws + L.colterm : nullptr, B, out_loss);
    QST_LAUNCH_CHECK();
    if (!want_g) return QST_OK;

    // d_hat_a [B, D] = scale * G [B, N] . c_hat [N, D]
    GemmP pa = {};
    pa.A = S; pa.lda = L.ldS; pa.Bm = c; pa.ldb = D; pa.C = grad_a; pa.ldc = D;
    pa.M = B; pa.N = D; pa.K = N; pa.alpha = scale;
    pa.kscale = cos ? rinv + B : nullptr;
    pa.gout = cos ? nullptr : grad_out;
    rc = launch_gemm<true, false>(pa, st);
    if (rc != QST_OK) return rc;
    // d_hat_c [N, D] = scale * G^T [N, B] . a_hat [B, D]
    GemmP pc = {};
    pc.A = S; pc.lda = L.ldS; pc.Bm = a; pc.ldb = D; pc.C = grad_c; pc.ldc = D;
    pc.M = N; pc.N = D; pc.K = B; pc.alpha = scale;
    pc.kscale = cos ? rinv : nullptr;
    pc.gout = cos ? nullptr : grad_out;
    rc = launch_gemm<false, false>(pc, st);
    if (rc != QST_OK) return rc;
    if (cos) {
        const bool vec = vec_in && al16(grad_a) && al16(grad_c);
        if (vec) mnrl_normbwd_kernel<true><<<row_grid, 256, 0, st>>>(a, c, grad_a, grad_c, B, N, D, rinv, nrm, grad_out);
        else mnrl_normbwd_kernel<false><<<row_grid, 256, 0, st>>>(a, c, grad_a, grad_c, B, N, D, rinv, nrm, grad_out);
        QST_LAUNCH_CHECK();
    }
    return QST_OK;
}
