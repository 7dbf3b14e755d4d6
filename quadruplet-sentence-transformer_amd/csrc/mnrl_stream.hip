// mnrl_stream.hip -- MultipleNegativesRankingLoss and its symmetric form with no B x N term: the loss of mnrl.hip for the
// batches of GradCache (CachedMultipleNegativesRankingLoss), where B reaches tens of thousands and the score matrix of
// qst_mnrl_loss neither fits nor is cheap next to the encoder any more. Same mathematics, same argument contract.
//
// The anchors are walked in strips of R rows (strip_rows, or the largest multiple of 64 whose R x ldS fp32 strip fits
// 64 MiB). Only one strip of scores exists at a time; beyond it the workspace holds per-row and per-column arrays and the
// split-K partial sums of one strip's grad_a. Per strip [r0, r0 + R), all on the caller's stream:
//   gemm NT  S_strip = scale * a_hat[r0 : r0 + R] . c_hat^T
//   row      one workgroup per anchor: max, sum of exponentials, the row's loss term; with gradients the row becomes
//            G[i, :] exactly as in mnrl.hip
//   gemm NN  grad_a[r0 : r0 + R] = scale * G . c_hat                 complete per strip
//   gemm TN  grad_c (+)= scale * G^T . a_hat[r0 : r0 + R]            the first strip writes, later strips add in the epilogue;
//            launches on one stream run in order, so the sum has a fixed order
// Around the strips: the reciprocal norms first and the backward of F.normalize in place last (cos), the fixed-order
// one-workgroup sum of the row terms, and *grad_out times the finished gradients (in the normalisation backward, or in a
// pass of its own for dot).
//
// The symmetric form needs every column's log-sum-exp before any G can be formed, so it sweeps the strips twice: the first
// sweep computes the row terms and merges each strip's column (max, sum) into running per-column arrays in strip order,
// the second recomputes each score strip and forms G. That is FOUR products instead of three -- the price of not keeping
// B x N scores.
//
// All products run on the exact-fp32 matrix-core GEMM of fp32_mgemm.h (v_mfma_f32_32x32x2_f32; shared with gist.hip): every
// output element is one accumulator walking K in order, so its bits do not depend on the tile, on its place in it, or on the
// strip. One exception by design: grad_a = G . c_hat has K = N and only R x D outputs, far fewer tiles than compute units at large
// N; its K is cut into chunks of kChunkK columns (a function of N alone), the chunks run as grid.y, and a second kernel adds
// the partial tiles in chunk order. Plain form therefore: out_loss and grad_a are bit-identical for every strip_rows;
// grad_c (summed over strips) and everything symmetric (column statistics merged over strips) may differ by rounding.
// Every tile edge is guarded in M, N and K (odd K included: the panels are zero-filled), every index is 64-bit.
#include "qst_common.h"

namespace {

#include "fp32_tile.h"
#include "fp32_mgemm.h"

constexpr size_t kStripBytes = (size_t)64 << 20;        // the score strip the library chooses stays below this

struct StreamWs {
    size_t rinv, nrm, rowterm, cmax, csum, diag, part, S, total;
    int ldS, R, chunks;
};

// strip_rows: 0 or a positive multiple of 64 (checked by the caller)
inline StreamWs stream_layout(int B, int N, int D, int strip_rows) {
    StreamWs w;
    w.ldS = (int)pad4((size_t)N);
    const int64_t b64 = ((int64_t)B + 63) / 64 * 64;
    int64_t R = strip_rows;
    if (R == 0) {
        R = (int64_t)(kStripBytes / sizeof(float) / (size_t)w.ldS) / 64 * 64;
        if (R < 64) R = 64;
    }
    if (R > b64) R = b64;
    w.R = (int)R;
    w.chunks = (N + kChunkK - 1) / kChunkK;
    size_t o = 0;
    w.rinv = o; o += pad4((size_t)B + N);
    w.nrm = o; o += pad4((size_t)B + N);
    w.rowterm = o; o += pad4((size_t)B);
    w.cmax = o; o += pad4((size_t)B);
    w.csum = o; o += pad4((size_t)B);
    w.diag = o; o += pad4((size_t)B);
    w.part = o; o += w.chunks > 1 ? (size_t)w.chunks * (size_t)w.R * pad4((size_t)D) : 0;
    w.S = o; o += (size_t)w.R * w.ldS;
    w.total = o;
    return w;
}

// ---- grad_a rows of one strip: the sum of the chunk partials in chunk order
__global__ __launch_bounds__(256) void mnrls_chunksum_kernel(const float* part, size_t cstride, int chunks, int ldp, int rows,
                                                             int D, float* out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)rows * D) return;
    const int64_t r = idx / D;
    const int d = (int)(idx - r * D);
    const float* q = part + (size_t)r * ldp + d;
    float s = q[0];
    for (int y = 1; y < chunks; ++y) s += q[(size_t)y * cstride];
    out[(size_t)r * D + d] = s;
}

// ---- column statistics of the rows of one strip, merged into the running ones (symmetric loss): 64 columns per workgroup,
// wave w takes the strip's rows w, w + 4, ... The strip that holds row j also records the diagonal score S[j, j].
__global__ __launch_bounds__(256) void mnrls_colstat_kernel(const float* S, int ldS, int B, int r0, int rows, float* cmax,
                                                            float* csum, float* diag) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane;
    const bool in = j < B;
    float mx = -__builtin_inff();
    if (in) for (int i = w; i < rows; i += 4) mx = fmaxf(mx, S[(size_t)i * ldS + j]);
    part[w][lane] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(part[0][lane], part[1][lane]), fmaxf(part[2][lane], part[3][lane]));
    __syncthreads();
    float sm = 0.f;
    if (in) for (int i = w; i < rows; i += 4) sm += expf(S[(size_t)i * ldS + j] - mx);
    part[w][lane] = sm;
    __syncthreads();
    if (w == 0 && in) {
        sm = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        if (r0 > 0) {                   // merge behind the strips before this one
            const float pm = cmax[j], ps = csum[j];
            const float m2 = fmaxf(pm, mx);
            sm = ps * expf(pm - m2) + sm * expf(mx - m2);
            mx = m2;
        }
        cmax[j] = mx;
        csum[j] = sm;
        if (j >= r0 && j < (int64_t)r0 + rows) diag[j] = S[(size_t)(j - r0) * ldS + j];
    }
}

// ---- the row pass over one strip: workgroup b owns anchor r0 + b. As stage 4 of mnrl.hip.
__global__ __launch_bounds__(256) void mnrls_row_kernel(float* S, int ldS, int B, int N, int r0, int symmetric,
                                                        const float* cmax, const float* csum, float* rowterm, int want_g) {
    __shared__ float part[4];
    const int i = r0 + (int)blockIdx.x, t = threadIdx.x;
    float* s = S + (size_t)blockIdx.x * ldS;
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

// ---- the loss: a fixed tree over the row terms (and the column terms log(csum) + cmax - S[j, j])
__global__ __launch_bounds__(1024) void mnrls_loss_kernel(const float* rowterm, const float* cmax, const float* csum,
                                                          const float* diag, int B, float* out) {
    __shared__ float part[16];
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += 1024) s += rowterm[i];
    s = block_sum<16>(s, part);
    float w = 1.f;
    if (cmax) {
        float c = 0.f;
        for (int i = threadIdx.x; i < B; i += 1024) c += (logf(csum[i]) + cmax[i]) - diag[i];
        c = block_sum<16>(c, part);
        s += c;
        w = 0.5f;
    }
    if (threadIdx.x == 0) out[0] = s * (w / (float)B);
}

// ---- dot with an upstream gradient: the finished gradients times *grad_out, in place
__global__ __launch_bounds__(256) void mnrls_gscale_kernel(float* ga, int64_t na, float* gc, int64_t nc, const float* gout) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= na + nc) return;
    float* q = idx < na ? ga + idx : gc + (idx - na);
    q[0] = q[0] * gout[0];
}

}  // namespace

extern "C" size_t qst_mnrl_stream_workspace_bytes(int B, int N, int D, int strip_rows) {
    if (B < 1 || N < B || D < 1 || !strip_rows_ok(strip_rows)) return 0;
    return stream_layout(B, N, D, strip_rows).total * sizeof(float);
}

extern "C" int qst_mnrl_stream_loss(const float* a, const float* c, int B, int N, int D, int sim, float scale, int symmetric,
                                    int strip_rows, float* out_loss, const float* grad_out, float* grad_a, float* grad_c,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 1 || N < B || D < 1 || !a || !c || !out_loss || !workspace) return QST_ERR_BAD_ARG;
    if (sim != QST_SCORE_DOT && sim != QST_SCORE_COS) return QST_ERR_BAD_ARG;
    if (symmetric != 0 && symmetric != 1) return QST_ERR_BAD_ARG;
    if (!(scale > 0.f) || !(scale < __builtin_inff())) return QST_ERR_BAD_ARG;   // NaN fails the first comparison
    if ((grad_a == nullptr) != (grad_c == nullptr)) return QST_ERR_BAD_ARG;
    if (!strip_rows_ok(strip_rows)) return QST_ERR_BAD_ARG;
    if (((uintptr_t)workspace & 3) != 0) return QST_ERR_BAD_ARG;
    const StreamWs L = stream_layout(B, N, D, strip_rows);
    if (workspace_bytes < L.total * sizeof(float)) return QST_ERR_BAD_ARG;
    // the kernels index in 64 bits; rows and tiles are counted in 32
    if ((int64_t)L.R * L.ldS > 0x7FFFFFFFLL || (int64_t)N * D > 0x7FFFFFFFLL) return QST_ERR_UNSUPPORTED;

    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    float* rinv = ws + L.rinv;
    float* nrm = ws + L.nrm;
    float* S = ws + L.S;
    float* cmax = ws + L.cmax;
    float* csum = ws + L.csum;
    const bool cos = sim == QST_SCORE_COS, want_g = grad_a != nullptr;
    const bool vec_in = (D % 4 == 0) && al16(a) && al16(c);
    const unsigned row_grid = (unsigned)(((int64_t)B + N + 3) / 4);
    const int ldp = (int)pad4((size_t)D);
    const size_t cstride = (size_t)L.R * ldp;
    int rc;

    if (cos) {
        if (vec_in) mnrls_rnorm_kernel<true><<<row_grid, 256, 0, st>>>(a, c, B, N, D, rinv, nrm);
        else mnrls_rnorm_kernel<false><<<row_grid, 256, 0, st>>>(a, c, B, N, D, rinv, nrm);
        QST_LAUNCH_CHECK();
    }
    // symmetric with gradients: sweep 0 gathers the row terms and the column statistics, sweep 1 forms G and the gradients
    const int sweeps = (symmetric && want_g) ? 2 : 1;
    for (int sweep = 0; sweep < sweeps; ++sweep) {
        const bool form_g = want_g && sweep == sweeps - 1;
        const bool colstat = symmetric && sweep == 0;
        for (int64_t r0 = 0; r0 < B; r0 += L.R) {
            const int rows = (int)(B - r0 < L.R ? B - r0 : L.R);
            MGemmP p = {};
            p.A = a + (size_t)r0 * D; p.lda = D; p.Bm = c; p.ldb = D; p.C = S; p.ldc = L.ldS;
            p.M = rows; p.N = N; p.K = D; p.alpha = scale; p.kchunk = D;
            p.mscale = cos ? rinv + r0 : nullptr; p.nscale = cos ? rinv + B : nullptr;
            rc = launch_mgemm<true, true, true>(p, 1, st);
            if (rc != QST_OK) return rc;
            if (colstat) {
                mnrls_colstat_kernel<<<(unsigned)((B + 63) / 64), 256, 0, st>>>(S, L.ldS, B, (int)r0, rows, cmax, csum,
                                                                                ws + L.diag);
                QST_LAUNCH_CHECK();
            }
            mnrls_row_kernel<<<(unsigned)rows, 256, 0, st>>>(S, L.ldS, B, N, (int)r0, symmetric, cmax, csum, ws + L.rowterm,
                                                             form_g ? 1 : 0);
            QST_LAUNCH_CHECK();
            if (!form_g) continue;

            // d_hat_a [rows, D] = scale * G [rows, N] . c_hat [N, D]
            MGemmP pa = {};
            pa.A = S; pa.lda = L.ldS; pa.Bm = c; pa.ldb = D;
            pa.M = rows; pa.N = D; pa.K = N; pa.alpha = scale;
            pa.kscale = cos ? rinv + B : nullptr;
            if (L.chunks > 1) {
                pa.C = ws + L.part; pa.ldc = ldp; pa.kchunk = kChunkK; pa.cstride = cstride;
                rc = launch_mgemm<true, false, false>(pa, L.chunks, st);
                if (rc != QST_OK) return rc;
                const int64_t n_out = (int64_t)rows * D;
                mnrls_chunksum_kernel<<<(unsigned)((n_out + 255) / 256), 256, 0, st>>>(ws + L.part, cstride, L.chunks, ldp, rows,
                                                                                       D, grad_a + (size_t)r0 * D);
                QST_LAUNCH_CHECK();
            } else {
                pa.C = grad_a + (size_t)r0 * D; pa.ldc = D; pa.kchunk = N;
                rc = launch_mgemm<true, false, false>(pa, 1, st);
                if (rc != QST_OK) return rc;
            }
            // d_hat_c [N, D] (+)= scale * G^T [N, rows] . a_hat [rows, D]
            MGemmP pc = {};
            pc.A = S; pc.lda = L.ldS; pc.Bm = a + (size_t)r0 * D; pc.ldb = D; pc.C = grad_c; pc.ldc = D;
            pc.M = N; pc.N = D; pc.K = rows; pc.alpha = scale; pc.kchunk = rows;
            pc.kscale = cos ? rinv + r0 : nullptr;
            pc.accumulate = r0 > 0 ? 1 : 0;
            rc = launch_mgemm<false, false, true>(pc, 1, st);
            if (rc != QST_OK) return rc;
        }
        if (sweep == 0) {
            mnrls_loss_kernel<<<1, 1024, 0, st>>>(ws + L.rowterm, symmetric ? cmax : nullptr, csum, ws + L.diag, B, out_loss);
            QST_LAUNCH_CHECK();
        }
    }
    if (!want_g) return QST_OK;
    if (cos) {
        const bool vec = vec_in && al16(grad_a) && al16(grad_c);
        if (vec) mnrls_normbwd_kernel<true><<<row_grid, 256, 0, st>>>(a, c, grad_a, grad_c, B, N, D, rinv, nrm, grad_out);
        else mnrls_normbwd_kernel<false><<<row_grid, 256, 0, st>>>(a, c, grad_a, grad_c, B, N, D, rinv, nrm, grad_out);
        QST_LAUNCH_CHECK();
    } else if (grad_out) {
        const int64_t na = (int64_t)B * D, nc = (int64_t)N * D;
        mnrls_gscale_kernel<<<(unsigned)((na + nc + 255) / 256), 256, 0, st>>>(grad_a, na, grad_c, nc, grad_out);
        QST_LAUNCH_CHECK();
    }
    return QST_OK;
}
