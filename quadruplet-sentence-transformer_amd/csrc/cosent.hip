// cosent.hip -- CoSENTLoss and AnglELoss of sentence-transformers: pairwise ranking of graded pairs, forward + backward in fp32.
//
// u, v [B, D] and one graded label y per row. s_i is the pairwise score of row i -- the cosine of F.normalize'd rows
// (util.pairwise_cos_sim, eps 1e-12) or util.pairwise_angle_sim, which for x = [a, b], y = [c, d] (halves of h = D / 2) is
//   s = |t| / (|x| |y|),  t = sum_k a_k (c_k - d_k) + b_k (c_k + d_k)
// -- and with V = {(i, j) : y_i < y_j}, d_ij = scale * (s_i - s_j):
//   L = log(1 + sum_V exp(d_ij)),   dL/ds_i = scale * (sum_{j : (i, j) in V} p_ij - sum_{j : (j, i) in V} p_ji),  p_ij = exp(d_ij - L)
// Everything is a function of B scores and B labels, so the workspace holds per-row scalars only: there is no B x B buffer.
// Stages (all on the caller's stream, no host synchronisation, no atomics, every reduction in a fixed order):
//   1. score   one wave per row (the forms of row_loss.h): the three sums of the row, s_i and what its gradient needs
//   2. pair    one wave per row i, lanes over j: m_i = max_j d_ij and sum_j exp(d_ij - m_i) over the (i, j) in V
//   3. finish  one workgroup: m = max(0, max_i m_i), L = m + log(exp(-m) + sum_i sum_i exp(m_i - m)); a score that is not
//              finite makes L NaN (the maxima drop NaNs, torch.logsumexp does not)
//   4. grad    one wave per row i: the row's loads are issued, the walk over j gives both sums of dL/ds_i (row i as the
//              smaller and as the larger label), then the row's gradients are written (from registers up to D = 2048)
// O(B) work per row in 2 and 4, O(B^2) exps per call. *grad_out multiplies the finished gradient.
#include "row_loss.h"

namespace {

constexpr float kNormEps = 1e-12f;      // F.normalize's eps
constexpr float kInf = __builtin_inff();
constexpr int kMaxAngleVec = 4;         // angle keeps four half rows: 256 * 4 floats each, the same D = 2048 in registers

// ---- workspace layout (floats; every segment starts on a multiple of 4, the workspace on 16 bytes)
struct CsWs { size_t score, acc, nx, ny, rmax, rsum, scal, total; };
inline CsWs cs_layout(int B) {
    const size_t p = ((size_t)B + 3) & ~(size_t)3;
    CsWs w;
    w.score = 0; w.acc = p; w.nx = 2 * p; w.ny = 3 * p; w.rmax = 4 * p; w.rsum = 5 * p; w.scal = 6 * p;
    w.total = 6 * p + 4;
    return w;
}

struct CosentArgs {
    const float* u;
    const float* v;
    const float* labels;
    const float* grad_out;          // [1] on the device, or null = 1
    float* gu;
    float* gv;
    float* score;                   // per row: s, the dot product (cos) or t (angle), |u|, |v|
    float* acc;
    float* nx;
    float* ny;
    float* out_scores;              // [B] or null
    const float* L;                 // the loss, as stage 3 left it
    int B, D;
    float scale;
};

// the element(s) k of a row pair: cos {u_k, v_k}; angle {a_k, b_k, c_k, d_k}. s: the numerator, |u|^2, |v|^2
template <bool ANGLE>
__device__ __forceinline__ void accum(const float (&e)[ANGLE ? 4 : 2], float (&s)[3]) {
    if (ANGLE) {
        s[0] += e[0] * (e[2] - e[3]) + e[1] * (e[2] + e[3]);
        s[1] += e[0] * e[0] + e[1] * e[1];
        s[2] += e[2] * e[2] + e[3] * e[3];
    } else {
        s[0] += e[0] * e[1]; s[1] += e[0] * e[0]; s[2] += e[1] * e[1];
    }
}

// ds/du = kxy * w(v) + kxx * u, ds/dv = kxy * w'(u) + kyy * v; cos: w = w' = the other row. c = dL/ds
struct ScoreGrad { float c, kxy, kxx, kyy; };
template <bool ANGLE>
__device__ __forceinline__ ScoreGrad score_grad(float c, float s, float acc, float nx, float ny) {
    ScoreGrad r;
    r.c = c;
    if (ANGLE) {                        // no epsilon: a zero row is 0 / 0, as upstream
        r.kxy = (acc > 0.f ? 1.f : (acc < 0.f ? -1.f : 0.f)) / (nx * ny);
        r.kxx = -s / (nx * nx);
        r.kyy = -s / (ny * ny);
    } else {                            // a norm below the clamp is the constant 1e-12 and passes no gradient
        const float cx = fmaxf(nx, kNormEps), cy = fmaxf(ny, kNormEps);
        r.kxy = 1.f / (cx * cy);
        r.kxx = nx >= kNormEps ? -s / (cx * cx) : 0.f;
        r.kyy = ny >= kNormEps ? -s / (cy * cy) : 0.f;
    }
    return r;
}
template <bool ANGLE>
__device__ __forceinline__ void emit(const ScoreGrad& k, float up, const float (&e)[ANGLE ? 4 : 2], float (&g)[ANGLE ? 4 : 2]) {
    if (ANGLE) {
        g[0] = (k.c * (k.kxy * (e[2] - e[3]) + k.kxx * e[0])) * up;
        g[1] = (k.c * (k.kxy * (e[2] + e[3]) + k.kxx * e[1])) * up;
        g[2] = (k.c * (k.kxy * (e[0] + e[1]) + k.kyy * e[2])) * up;
        g[3] = (k.c * (k.kxy * (e[1] - e[0]) + k.kyy * e[3])) * up;
    } else {
        g[0] = (k.c * (k.kxy * e[1] + k.kxx * e[0])) * up;
        g[1] = (k.c * (k.kxy * e[0] + k.kyy * e[1])) * up;
    }
}

// dL/ds_i: lanes over j, each pair's one exp goes to the sum its order selects. d_ji = -d_ij exactly.
__device__ __forceinline__ float pair_walk(const CosentArgs& a, int64_t row, int lane) {
    const float si = a.score[row], yi = a.labels[row], L = a.L[0];
    float lo = 0.f, hi = 0.f;
    for (int64_t j = lane; j < a.B; j += 64) {
        const float yj = a.labels[j];
        const float d = a.scale * (si - a.score[j]);
        const bool below = yi < yj, above = yj < yi;    // both false for a NaN label: the row takes no part
        const float p = expf((below ? d : -d) - L);
        lo += below ? p : 0.f;
        hi += above ? p : 0.f;
    }
    return a.scale * (wave_sum(lo) - wave_sum(hi));
}

// ---- 1 and 4. NS row streams of W floats (cos: u, v of D; angle: a, b, c, d of h). NV > 0: W <= 256 * NV, the rows are
// loaded once, 16 bytes a lane, before anything else (in stage 4 they travel under the walk). NV == 0: the rows stream, 16
// bytes a lane (VEC) or element by element.
template <int SIM, int NV, bool VEC, bool GRAD>
__global__ __launch_bounds__(256) void cosent_row_kernel(CosentArgs a) {
    constexpr bool ANGLE = SIM == QST_PAIRSIM_ANGLE;
    constexpr int NS = ANGLE ? 4 : 2;
    constexpr int kVec = NV > 0 ? NV : 1;
    const int lane = threadIdx.x & 63;
    int64_t row;
    if (!wave_row(a.B, row)) return;
    const int W = ANGLE ? a.D >> 1 : a.D;
    const size_t base = row_base(row, a.D);
    const float* x[NS];
    float* g[NS] = {};
    x[0] = a.u + base; x[NS / 2] = a.v + base;
    if (ANGLE) { x[1] = x[0] + W; x[NS - 1] = x[NS / 2] + W; }
    if (GRAD) {
        g[0] = a.gu + base; g[NS / 2] = a.gv + base;
        if (ANGLE) { g[1] = g[0] + W; g[NS - 1] = g[NS / 2] + W; }
    }
    const int nv = W >> 2;

    float xr[NS][kVec * 4];
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            const int v = lane + i * 64;
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                f32x4 X = {0, 0, 0, 0};                 // past the row: zeros, which add nothing
                if (v < nv) X = *(const f32x4*)(x[k] + v * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) xr[k][i * 4 + j] = X[j];
            }
        }
    }

    if (!GRAD) {
        float s[3] = {0.f, 0.f, 0.f};
        if (NV > 0) {
#pragma unroll
            for (int i = 0; i < kVec * 4; ++i) {
                float e[NS];
#pragma unroll
                for (int k = 0; k < NS; ++k) e[k] = xr[k][i];
                accum<ANGLE>(e, s);
            }
        } else if (VEC) {
            for (int v = lane; v < nv; v += 64) {
                f32x4 X[NS];
#pragma unroll
                for (int k = 0; k < NS; ++k) X[k] = *(const f32x4*)(x[k] + v * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float e[NS];
#pragma unroll
                    for (int k = 0; k < NS; ++k) e[k] = X[k][j];
                    accum<ANGLE>(e, s);
                }
            }
        } else {
            for (int i = lane; i < W; i += 64) {
                float e[NS];
#pragma unroll
                for (int k = 0; k < NS; ++k) e[k] = x[k][i];
                accum<ANGLE>(e, s);
            }
        }
        const float acc = wave_sum(s[0]), nx = sqrtf(wave_sum(s[1])), ny = sqrtf(wave_sum(s[2]));
        const float sc = ANGLE ? fabsf(acc) / (nx * ny) : acc / (fmaxf(nx, kNormEps) * fmaxf(ny, kNormEps));
        if (lane == 0) {
            a.score[row] = sc; a.acc[row] = acc; a.nx[row] = nx; a.ny[row] = ny;
            if (a.out_scores) a.out_scores[row] = sc;
        }
        return;
    }

    const float c = pair_walk(a, row, lane);
    const ScoreGrad k = score_grad<ANGLE>(c, a.score[row], a.acc[row], a.nx[row], a.ny[row]);
    const float up = a.grad_out ? a.grad_out[0] : 1.f;
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            const int v = lane + i * 64;
            if (v < nv) {
                f32x4 G[NS];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float e[NS], ge[NS];
#pragma unroll
                    for (int q = 0; q < NS; ++q) e[q] = xr[q][i * 4 + j];
                    emit<ANGLE>(k, up, e, ge);
#pragma unroll
                    for (int q = 0; q < NS; ++q) G[q][j] = ge[q];
                }
#pragma unroll
                for (int q = 0; q < NS; ++q) *(f32x4*)(g[q] + v * 4) = G[q];
            }
        }
    } else if (VEC) {
        for (int v = lane; v < nv; v += 64) {
            f32x4 X[NS], G[NS];
#pragma unroll
            for (int q = 0; q < NS; ++q) X[q] = *(const f32x4*)(x[q] + v * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float e[NS], ge[NS];
#pragma unroll
                for (int q = 0; q < NS; ++q) e[q] = X[q][j];
                emit<ANGLE>(k, up, e, ge);
#pragma unroll
                for (int q = 0; q < NS; ++q) G[q][j] = ge[q];
            }
#pragma unroll
            for (int q = 0; q < NS; ++q) *(f32x4*)(g[q] + v * 4) = G[q];
        }
    } else {
        for (int i = lane; i < W; i += 64) {
            float e[NS], ge[NS];
#pragma unroll
            for (int q = 0; q < NS; ++q) e[q] = x[q][i];
            emit<ANGLE>(k, up, e, ge);
#pragma unroll
            for (int q = 0; q < NS; ++q) g[q][i] = ge[q];
        }
    }
}

// ---- 2. per row i: m_i = max over (i, j) in V of d_ij (-inf without one) and sum exp(d_ij - m_i). The sum runs even where
// the maximum found nothing, so a NaN d_ij that fmaxf dropped still reaches it.
__global__ __launch_bounds__(256) void cosent_pair_kernel(const float* score, const float* labels, int B, float scale,
                                                          float* rmax, float* rsum) {
    const int lane = threadIdx.x & 63;
    int64_t row;
    if (!wave_row(B, row)) return;
    const float si = score[row], yi = labels[row];
    float m = -kInf;
    for (int64_t j = lane; j < B; j += 64)
        if (yi < labels[j]) m = fmaxf(m, scale * (si - score[j]));
    m = wave_max(m);
    float s = 0.f;
    for (int64_t j = lane; j < B; j += 64)
        if (yi < labels[j]) s += expf(scale * (si - score[j]) - m);
    s = wave_sum(s);
    if (lane == 0) { rmax[row] = m; rsum[row] = s; }
}

// ---- 3. the loss from the per-row partials: thread i takes rows i, i + 1024, ... in that order, then block_reduce's tree.
// Without any pair m = 0 and the sum is 0: log1p(0) = 0 exactly.
__global__ __launch_bounds__(1024) void cosent_finish_kernel(const float* score, const float* rmax, const float* rsum, int B,
                                                             float* out_loss, float* scal) {
    __shared__ float part[16];
    float mx = -kInf, bad = 0.f;
    for (int64_t i = threadIdx.x; i < B; i += 1024) {
        mx = fmaxf(mx, rmax[i]);
        if (!(fabsf(score[i]) < kInf)) bad = 1.f;
    }
    mx = block_reduce<OP_MAX>(mx, part);
    bad = block_reduce<OP_MAX>(bad, part);
    const float m = fmaxf(mx, 0.f);
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < B; i += 1024) s += rsum[i] * expf(rmax[i] - m);   // a row without a pair: 0 * exp(-inf)
    s = block_reduce<OP_SUM>(s, part);
    if (threadIdx.x == 0) {
        float L = m > 0.f ? m + logf(expf(-m) + s) : log1pf(s);
        if (bad > 0.f) L = __builtin_nanf("");
        out_loss[0] = L;
        scal[0] = L;
    }
}

template <int SIM, bool GRAD>
void launch_rows(const CosentArgs& a, hipStream_t st) {
    constexpr bool ANGLE = SIM == QST_PAIRSIM_ANGLE;
    const float* x[2] = {a.u, a.v};
    float* g[2] = {a.gu, a.gv};
    // angle reads four half rows of h = D / 2 floats: they start on 16 bytes only where h % 4 == 0
    dispatch_form<true>(ANGLE ? a.D / 2 : a.D, rows_al16(x, 2, g, GRAD ? 2 : 0), [&](auto nv, auto vec) {
        constexpr int NV = (ANGLE && decltype(nv)::value > kMaxAngleVec) ? 0 : decltype(nv)::value;
        cosent_row_kernel<SIM, NV, decltype(vec)::value, GRAD><<<row_grid(a.B), 256, 0, st>>>(a);
    });
}

}  // namespace

extern "C" size_t qst_cosent_workspace_bytes(int B, int D) {
    if (B < 1 || D < 1) return 0;
    return cs_layout(B).total * sizeof(float);
}

extern "C" int qst_cosent_loss(const float* u, const float* v, const float* labels, int B, int D, int sim, float scale,
                               float* out_loss, float* out_scores, const float* grad_out, float* grad_u, float* grad_v,
                               void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 1 || D < 1 || !u || !v || !labels || !out_loss || !workspace) return QST_ERR_BAD_ARG;
    if (sim != QST_PAIRSIM_COS && sim != QST_PAIRSIM_ANGLE) return QST_ERR_BAD_ARG;
    if (sim == QST_PAIRSIM_ANGLE && (D & 1)) return QST_ERR_BAD_ARG;
    if (!(scale > 0.f) || !(scale < kInf)) return QST_ERR_BAD_ARG;               // NaN fails the first comparison
    if ((grad_u != nullptr) != (grad_v != nullptr)) return QST_ERR_BAD_ARG;
    if (((uintptr_t)workspace & 15) != 0) return QST_ERR_BAD_ARG;
    const CsWs L = cs_layout(B);
    if (workspace_bytes < L.total * sizeof(float)) return QST_ERR_BAD_ARG;
    if ((int64_t)B * D > 0x7FFFFFFFLL) return QST_ERR_UNSUPPORTED;               // row_base multiplies in 32 bits

    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    CosentArgs a = {};
    a.u = u; a.v = v; a.labels = labels; a.grad_out = grad_out;
    a.score = ws + L.score; a.acc = ws + L.acc; a.nx = ws + L.nx; a.ny = ws + L.ny;
    a.out_scores = out_scores; a.L = ws + L.scal;
    a.B = B; a.D = D; a.scale = scale;
    float* rmax = ws + L.rmax;
    float* rsum = ws + L.rsum;

    if (sim == QST_PAIRSIM_ANGLE) launch_rows<QST_PAIRSIM_ANGLE, false>(a, st);
    else launch_rows<QST_PAIRSIM_COS, false>(a, st);
    QST_LAUNCH_CHECK();
    cosent_pair_kernel<<<row_grid(B), 256, 0, st>>>(a.score, labels, B, scale, rmax, rsum);
    QST_LAUNCH_CHECK();
    cosent_finish_kernel<<<1, 1024, 0, st>>>(a.score, rmax, rsum, B, out_loss, ws + L.scal);
    QST_LAUNCH_CHECK();
    if (!grad_u) return QST_OK;

    a.gu = grad_u; a.gv = grad_v;
    if (sim == QST_PAIRSIM_ANGLE) launch_rows<QST_PAIRSIM_ANGLE, true>(a, st);
    else launch_rows<QST_PAIRSIM_COS, true>(a, st);
    QST_LAUNCH_CHECK();
    return QST_OK;
}
