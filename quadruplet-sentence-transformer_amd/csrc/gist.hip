// gist.hip -- GISTEmbedLoss (Solatorio 2024) and, at GradCache batch sizes, CachedGISTEmbedLoss: in-batch negatives that a
// frozen guide model filters. x [K * B, D] holds the student's K text columns stacked (anchors a, positives p, hard negatives
// n_1 ...), g [K * B, Dg] the guide's embeddings of the same texts; a hat is F.normalize(eps = 1e-12). Row i has (K + 1) * B
// logits, kept in this column order (the loss does not depend on it):
//   [0, K * B)            a_hat_i . x_hat_j / temperature: the blocks aa (j < B), ap (B <= j < 2 B), an_k (the rest)
//   [K * B, (K + 1) * B)  p_hat_i . p_hat_j / temperature: the block pp
// and the guide has the same blocks from g (not divided). An entry leaves the softmax when its guide value is strictly above
// bound_i = thr_i - margin (absolute) or thr_i * (1 - margin) (relative), thr_i the guide's ap[i, i]. The target ap[i, i] is
// kept BY INDEX, whatever the guide says about it; thr_i is read from the same guide strip the comparison reads, so an entry
// with the target's own bits compares equal, and a NaN compares false and stays.
//   loss = mean_i(logsumexp(row i) - ap[i, i] / temperature)
//
// The anchors and positives are walked in strips of R rows, as mnrl_stream.hip walks its anchors. Two strips exist at a time
// (student logits, guide scores: R x ldS each, ldS = (K + 1) * B rounded up to 4); beyond them the workspace is linear in B.
// Per strip [r0, r0 + R), all on the caller's stream:
//   gemm NT x 2  guide:   a_g[strip] . g^T (K * B columns) and p_g[strip] . p_g^T (B columns)
//   gemm NT x 2  student: the same two products of x, times 1 / temperature
//   row          one workgroup per row: mask, max, sum of exponentials, the row term; with gradients the row becomes
//                G = (softmax - one-hot) / B in place, exactly 0 where masked
//   gemm TN x 2  column side: grad_x[0 : K * B] (+)= G[:, : K * B]^T . a_hat[strip], grad_x[B : 2 B] += G_pp^T . p_hat[strip];
//                the first strip's first product writes every row of grad_x, everything after it adds in the epilogue
//   gemm NN x 2  row side: grad_x[strip of a] += G[:, : K * B] . x_hat, grad_x[strip of p] += G_pp . p_hat; where K * B (or B)
//                exceeds kChunkK the K range runs in chunks as grid.y and a second kernel adds the partial tiles in chunk order
// Around the strips: the reciprocal norms of x and g first, the fixed-order sum of the row terms, and last the backward of
// F.normalize (clamp included) times *grad_out. Launches on one stream run in order and nothing is atomic, so every sum has a
// fixed order. Forward: 3 + 5 * strips launches; with gradients 4 + 9 * strips (+ 1 per chunked row-side product).
// out_loss is bit-identical for every strip_rows (a logit's bits do not depend on the tiling, a row term on its row alone);
// the gradients, summed over strips, may differ between strip_rows by rounding.
#include "qst_common.h"

namespace {

#include "fp32_tile.h"
#include "fp32_mgemm.h"

constexpr size_t kStripBytes = (size_t)64 << 20;        // the two strips the library chooses stay below this together

struct GistWs {
    size_t rinv_x, nrm_x, rinv_g, nrm_g, rowterm, part, S, G, total;
    int ldS, R, chunks;
};

// B >= 1, K >= 2 and (K + 1) * B within int (checked by the caller); strip_rows: 0 or a positive multiple of 64
inline GistWs gist_layout(int B, int K, int D, int strip_rows) {
    GistWs w;
    const size_t KB = (size_t)K * B;
    w.ldS = (int)pad4(KB + B);
    const int64_t b64 = ((int64_t)B + 63) / 64 * 64;
    int64_t R = strip_rows;
    if (R == 0) {
        R = (int64_t)(kStripBytes / sizeof(float) / 2 / (size_t)w.ldS) / 64 * 64;
        if (R < 64) R = 64;
    }
    if (R > b64) R = b64;
    w.R = (int)R;
    w.chunks = (int)((KB + kChunkK - 1) / kChunkK);
    size_t o = 0;
    w.rinv_x = o; o += pad4(KB);
    w.nrm_x = o; o += pad4(KB);
    w.rinv_g = o; o += pad4(KB);
    w.nrm_g = o; o += pad4(KB);
    w.rowterm = o; o += pad4((size_t)B);
    w.part = o; o += w.chunks > 1 ? (size_t)w.chunks * (size_t)w.R * pad4((size_t)D) : 0;
    w.S = o; o += (size_t)w.R * w.ldS;
    w.G = o; o += (size_t)w.R * w.ldS;
    w.total = o;
    return w;
}

inline bool gist_shape_ok(int B, int K, int D, int Dg) {
    return B >= 1 && K >= 2 && D >= 1 && Dg >= 1 && ((int64_t)K + 1) * B <= 0x7FFFFFFFLL - 3;
}

// ---- the row pass over one strip: workgroup b owns row i = r0 + b. s: the row's student logits, gd: its guide scores.
// N = (K + 1) * B columns; the target is column B + i.
__global__ __launch_bounds__(256) void gist_row_kernel(float* S, const float* Gd, int ldS, int B, int N, int r0, int relative,
                                                       float margin, float* rowterm, int want_g) {
    __shared__ float part[4];
    const int i = r0 + (int)blockIdx.x, t = threadIdx.x;
    const int tgt = B + i;
    float* s = S + (size_t)blockIdx.x * ldS;
    const float* gd = Gd + (size_t)blockIdx.x * ldS;
    const float thr = gd[tgt];
    const float bound = relative ? thr * (1.f - margin) : thr - margin;
    const float sii = s[tgt];           // every thread, before the first barrier: the write pass below replaces it
    float mx = -__builtin_inff();
    for (int j = t; j < N; j += 256) {
        float v = s[j];
        if (j != tgt && gd[j] > bound) { v = -__builtin_inff(); s[j] = v; }    // a NaN compares false and stays
        mx = fmaxf(mx, v);
    }
    mx = block_max<4>(mx, part);
    // each thread reads back its own writes only; exp(-inf - mx) is exactly 0 (mx is at least the target's logit)
    float sm = 0.f;
    for (int j = t; j < N; j += 256) sm += expf(s[j] - mx);
    sm = block_sum<4>(sm, part);
    if (t == 0) rowterm[i] = (logf(sm) + mx) - sii;
    if (!want_g) return;
    const float coef = 1.f / (float)B;
    const float inv = 1.f / sm;
    for (int j = t; j < N; j += 256) {
        const float hot = j == tgt ? 1.f : 0.f;
        s[j] = coef * (expf(s[j] - mx) * inv - hot);
    }
}

// ---- the loss: a fixed tree over the row terms
__global__ __launch_bounds__(1024) void gist_loss_kernel(const float* rowterm, int B, float* out) {
    __shared__ float part[16];
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += 1024) s += rowterm[i];
    s = block_sum<16>(s, part);
    if (threadIdx.x == 0) out[0] = s * (1.f / (float)B);
}

// ---- out[rows, D] += the chunk partials of a row-side product, in chunk order
__global__ __launch_bounds__(256) void gist_chunkadd_kernel(const float* part, size_t cstride, int chunks, int ldp, int rows,
                                                            int D, float* out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)rows * D) return;
    const int64_t r = idx / D;
    const int d = (int)(idx - r * D);
    const float* q = part + (size_t)r * ldp + d;
    float s = q[0];
    for (int y = 1; y < chunks; ++y) s += q[(size_t)y * cstride];
    float* o = out + (size_t)r * D + d;
    o[0] = o[0] + s;
}

// rows [r0, r0 + rows) of `left` against every row of `right` [n, Dx], both scaled by their reciprocal norms, into
// C[:, col0 : col0 + n]
int score_block(const float* left, const float* right, int rows, int n, int Dx, const float* rinv_left, const float* rinv_right,
                float alpha, float* C, int ldS, hipStream_t st) {
    MGemmP p = {};
    p.A = left; p.lda = Dx; p.Bm = right; p.ldb = Dx; p.C = C; p.ldc = ldS;
    p.M = rows; p.N = n; p.K = Dx; p.alpha = alpha; p.kchunk = Dx;
    p.mscale = rinv_left; p.nscale = rinv_right;
    return launch_mgemm<true, true, true>(p, 1, st);
}

// out[rows, D] += alpha * Gs[rows, n] . (rinv * xs)[n, D], split in K chunks where n > kChunkK
int row_side(const float* Gs, int ldS, const float* xs, const float* rinv, int rows, int n, int D, float alpha, float* out,
             float* part, int ldp, size_t cstride, hipStream_t st) {
    MGemmP p = {};
    p.A = Gs; p.lda = ldS; p.Bm = xs; p.ldb = D;
    p.M = rows; p.N = D; p.K = n; p.alpha = alpha; p.kscale = rinv;
    const int chunks = (n + kChunkK - 1) / kChunkK;
    if (chunks == 1) {
        p.C = out; p.ldc = D; p.kchunk = n; p.accumulate = 1;
        return launch_mgemm<true, false, false>(p, 1, st);
    }
    p.C = part; p.ldc = ldp; p.kchunk = kChunkK; p.cstride = cstride;
    const int rc = launch_mgemm<true, false, false>(p, chunks, st);
    if (rc != QST_OK) return rc;
    const int64_t n_out = (int64_t)rows * D;
    gist_chunkadd_kernel<<<(unsigned)((n_out + 255) / 256), 256, 0, st>>>(part, cstride, chunks, ldp, rows, D, out);
    QST_LAUNCH_CHECK();
    return QST_OK;
}

// out[n, D] (+)= alpha * Gs[rows, n]^T . (rinv * xs)[rows, D]
int col_side(const float* Gs, int ldS, const float* xs, const float* rinv, int rows, int n, int D, float alpha, float* out,
             int accumulate, hipStream_t st) {
    MGemmP p = {};
    p.A = Gs; p.lda = ldS; p.Bm = xs; p.ldb = D; p.C = out; p.ldc = D;
    p.M = n; p.N = D; p.K = rows; p.alpha = alpha; p.kchunk = rows; p.kscale = rinv;
    p.accumulate = accumulate;
    return launch_mgemm<false, false, true>(p, 1, st);
}

}  // namespace

extern "C" size_t qst_gist_workspace_bytes(int B, int K, int D, int Dg, int strip_rows) {
    if (!gist_shape_ok(B, K, D, Dg) || !strip_rows_ok(strip_rows)) return 0;
    return gist_layout(B, K, D, strip_rows).total * sizeof(float);
}

extern "C" int qst_gist_loss(const float* x, const float* g, int B, int K, int D, int Dg, float temperature,
                             int margin_strategy, float margin, int strip_rows, float* out_loss, const float* grad_out,
                             float* grad_x, void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 1 || K < 2 || D < 1 || Dg < 1 || !x || !g || !out_loss || !workspace) return QST_ERR_BAD_ARG;
    if (!(temperature > 0.f) || !(temperature < __builtin_inff())) return QST_ERR_BAD_ARG;   // NaN fails the first comparison
    if (!(margin > -__builtin_inff()) || !(margin < __builtin_inff())) return QST_ERR_BAD_ARG;
    if (margin_strategy != QST_GIST_ABSOLUTE && margin_strategy != QST_GIST_RELATIVE) return QST_ERR_BAD_ARG;
    if (!strip_rows_ok(strip_rows)) return QST_ERR_BAD_ARG;
    if (((uintptr_t)workspace & 3) != 0) return QST_ERR_BAD_ARG;
    if (!gist_shape_ok(B, K, D, Dg)) return QST_ERR_UNSUPPORTED;
    const GistWs L = gist_layout(B, K, D, strip_rows);
    if (workspace_bytes < L.total * sizeof(float)) return QST_ERR_BAD_ARG;
    // the kernels index in 64 bits; rows and tiles are counted in 32
    const int64_t KB = (int64_t)K * B;
    if ((int64_t)L.R * L.ldS > 0x7FFFFFFFLL || KB * D > 0x7FFFFFFFLL || KB * Dg > 0x7FFFFFFFLL) return QST_ERR_UNSUPPORTED;

    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    float* rinv_x = ws + L.rinv_x;
    float* rinv_g = ws + L.rinv_g;
    float* S = ws + L.S;
    float* Gd = ws + L.G;
    const bool want_g = grad_x != nullptr;
    const int nkb = (int)KB, N = nkb + B;
    const unsigned row_grid = (unsigned)((KB + 3) / 4);
    const float inv_t = 1.f / temperature;
    const int ldp = (int)pad4((size_t)D);
    const size_t cstride = (size_t)L.R * ldp;
    const float* xp = x + (size_t)B * D;                // the positives
    const float* gp = g + (size_t)B * Dg;
    int rc;

    if (D % 4 == 0 && al16(x)) mnrls_rnorm_kernel<true><<<row_grid, 256, 0, st>>>(x, xp, B, nkb - B, D, rinv_x, ws + L.nrm_x);
    else mnrls_rnorm_kernel<false><<<row_grid, 256, 0, st>>>(x, xp, B, nkb - B, D, rinv_x, ws + L.nrm_x);
    QST_LAUNCH_CHECK();
    if (Dg % 4 == 0 && al16(g)) mnrls_rnorm_kernel<true><<<row_grid, 256, 0, st>>>(g, gp, B, nkb - B, Dg, rinv_g, ws + L.nrm_g);
    else mnrls_rnorm_kernel<false><<<row_grid, 256, 0, st>>>(g, gp, B, nkb - B, Dg, rinv_g, ws + L.nrm_g);
    QST_LAUNCH_CHECK();

    for (int64_t r0 = 0; r0 < B; r0 += L.R) {
        const int rows = (int)(B - r0 < L.R ? B - r0 : L.R);
        // the guide's scores, then the student's logits: anchors of the strip against every text, positives against positives
        rc = score_block(g + (size_t)r0 * Dg, g, rows, nkb, Dg, rinv_g + r0, rinv_g, 1.f, Gd, L.ldS, st);
        if (rc != QST_OK) return rc;
        rc = score_block(gp + (size_t)r0 * Dg, gp, rows, B, Dg, rinv_g + B + r0, rinv_g + B, 1.f, Gd + nkb, L.ldS, st);
        if (rc != QST_OK) return rc;
        rc = score_block(x + (size_t)r0 * D, x, rows, nkb, D, rinv_x + r0, rinv_x, inv_t, S, L.ldS, st);
        if (rc != QST_OK) return rc;
        rc = score_block(xp + (size_t)r0 * D, xp, rows, B, D, rinv_x + B + r0, rinv_x + B, inv_t, S + nkb, L.ldS, st);
        if (rc != QST_OK) return rc;
        gist_row_kernel<<<(unsigned)rows, 256, 0, st>>>(S, Gd, L.ldS, B, N, (int)r0, margin_strategy == QST_GIST_RELATIVE ? 1 : 0,
                                                        margin, ws + L.rowterm, want_g ? 1 : 0);
        QST_LAUNCH_CHECK();
        if (!want_g) continue;

        // column side first: on the first strip it writes every row of grad_x, which everything after it adds to
        rc = col_side(S, L.ldS, x + (size_t)r0 * D, rinv_x + r0, rows, nkb, D, inv_t, grad_x, r0 > 0 ? 1 : 0, st);
        if (rc != QST_OK) return rc;
        rc = col_side(S + nkb, L.ldS, xp + (size_t)r0 * D, rinv_x + B + r0, rows, B, D, inv_t, grad_x + (size_t)B * D, 1, st);
        if (rc != QST_OK) return rc;
        rc = row_side(S, L.ldS, x, rinv_x, rows, nkb, D, inv_t, grad_x + (size_t)r0 * D, ws + L.part, ldp, cstride, st);
        if (rc != QST_OK) return rc;
        rc = row_side(S + nkb, L.ldS, xp, rinv_x + B, rows, B, D, inv_t, grad_x + (size_t)(B + r0) * D, ws + L.part, ldp, cstride,
                      st);
        if (rc != QST_OK) return rc;
    }
    gist_loss_kernel<<<1, 1024, 0, st>>>(ws + L.rowterm, B, out_loss);
    QST_LAUNCH_CHECK();
    if (!want_g) return QST_OK;
    float* gxp = grad_x + (size_t)B * D;
    if (D % 4 == 0 && al16(x) && al16(grad_x))
        mnrls_normbwd_kernel<true><<<row_grid, 256, 0, st>>>(x, xp, grad_x, gxp, B, nkb - B, D, rinv_x, ws + L.nrm_x, grad_out);
    else
        mnrls_normbwd_kernel<false><<<row_grid, 256, 0, st>>>(x, xp, grad_x, gxp, B, nkb - B, D, rinv_x, ws + L.nrm_x, grad_out);
    QST_LAUNCH_CHECK();
    return QST_OK;
}
