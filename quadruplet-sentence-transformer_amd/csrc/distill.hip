// distill.hip -- the two distillation objectives of sentence-transformers 2.2.2, forward + backward (one wave64 per row).
//
//   qst_embed_mse        mean over B*D of (x - t)^2: losses.MSELoss (the student's embedding regressed on the teacher's) and
//                        what evaluation.MSEEvaluator scores with
//   qst_margin_mse_loss  (sim(q, p) - sim(q, n) - label)^2, sim the dot product or the cosine: losses.MarginMSELoss
//
// Both have tuple_loss_kernel's shape: a wave reads its rows once with 16-byte coalesced loads, keeps them in registers up to
// D = 2048 (past that the gradient pass re-reads them, still 16 bytes a lane), reduces with DPP, and writes the gradients from
// the registers. The per-row values go through a one-workgroup second stage that sums in double, in a fixed order: B can be
// a whole evaluation set, and the squared error of every row has the same sign. No atomics anywhere: the same inputs give
// the same bits. HBM-bound: 2 (3) rows read and, with gradients, 1 (3) written. The choice of the form, the second stage and
// the cosine's scalars are row_loss.h's, shared with loss.hip and tuple_loss.hip.
#include "row_loss.h"

namespace {

// ---- qst_embed_mse
struct MseArgs {
    const float* x;
    const float* t;
    float* g;                       // null = forward only
    const float* grad_out;          // [1] on the device, or null = 1
    float* row_out;                 // [B]: sum_d (x - t)^2 of the row
    int B, D;
    float k;                        // 2 / (B * D)
};

// NV > 0: float4 per lane kept in registers (the differences: the gradient needs nothing else). NV == 0: the rows stream
// and the gradient pass reads them again, 16 bytes a lane (VEC) or element by element (D % 4 != 0 or unaligned pointers).
template <int NV, bool VEC>
__global__ __launch_bounds__(256) void embed_mse_kernel(MseArgs a) {
    constexpr int kVec = NV > 0 ? NV : 1;
    const int lane = threadIdx.x & 63;
    int64_t row;
    if (!wave_row(a.B, row)) return;
    const int D = a.D;
    const size_t base = row_base(row, D);
    const float* x = a.x + base;
    const float* t = a.t + base;
    const int nv = D >> 2;

    float dr[kVec * 4];
    float s = 0.f;
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            const int v = lane + i * 64;
            f32x4 X = {0, 0, 0, 0}, T = {0, 0, 0, 0};
            if (v < nv) { X = *(const f32x4*)(x + v * 4); T = *(const f32x4*)(t + v * 4); }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = X[j] - T[j];        // past the row: 0 - 0, adds nothing
                dr[i * 4 + j] = d;
                s += d * d;
            }
        }
    } else if (VEC) {
        for (int v = lane; v < nv; v += 64) {
            const f32x4 X = *(const f32x4*)(x + v * 4), T = *(const f32x4*)(t + v * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float d = X[j] - T[j]; s += d * d; }
        }
    } else {
        for (int i = lane; i < D; i += 64) { const float d = x[i] - t[i]; s += d * d; }
    }
    s = wave_sum(s);
    if (lane == 0) a.row_out[row] = s;
    if (a.g == nullptr) return;

    // the finished gradient (x - t) * 2 / (B D), then the upstream factor: one more rounding and no other
    const float up = a.grad_out ? a.grad_out[0] : 1.f;
    const float k = a.k;
    float* g = a.g + base;
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            const int v = lane + i * 64;
            if (v < nv) {
                f32x4 G;
#pragma unroll
                for (int j = 0; j < 4; ++j) G[j] = (dr[i * 4 + j] * k) * up;
                *(f32x4*)(g + v * 4) = G;
            }
        }
    } else if (VEC) {
        for (int v = lane; v < nv; v += 64) {
            const f32x4 X = *(const f32x4*)(x + v * 4), T = *(const f32x4*)(t + v * 4);
            f32x4 G;
#pragma unroll
            for (int j = 0; j < 4; ++j) G[j] = ((X[j] - T[j]) * k) * up;
            *(f32x4*)(g + v * 4) = G;
        }
    } else {
        for (int i = lane; i < D; i += 64) g[i] = ((x[i] - t[i]) * k) * up;
    }
}

// ---- qst_margin_mse_loss
struct MarginArgs {
    const float* x[3];              // query, positive, negative
    float* g[3];                    // all null = forward only
    const float* labels;            // [B]: the teacher's margin
    const float* grad_out;          // [B] (reduction none) or [1]; null = ones
    float* row_out;                 // [B] per-row value
    float* margin_out;              // [B] or null
    int B, D, reduction;
};

// five sums of a row triple: q.p, q.n and, for the cosine, |q|^2, |p|^2, |n|^2
template <bool COS>
__device__ __forceinline__ void margin_accum(float q, float p, float n, float (&s)[5]) {
    s[0] += q * p; s[1] += q * n;
    if (COS) { s[2] += q * q; s[3] += p * p; s[4] += n * n; }
}

// sim(q, y) and the scalars of its gradient: d sim / dq = kxy * y + kxx * q, d sim / dy = kxy * q + kyy * y -- the formulas
// of qst_pair_metric (tuple_loss.hip): a norm at or below the clamp is a constant and passes no gradient
template <bool COS>
__device__ __forceinline__ CosVal sim_finish(float dot, float nx, float ny) {
    return COS ? cos_finish(dot, nx, ny, false) : CosVal{dot, 1.f, 0.f, 0.f};
}

template <bool COS, int NV, bool VEC>
__global__ __launch_bounds__(256) void margin_mse_kernel(MarginArgs a) {
    constexpr int kVec = NV > 0 ? NV : 1;
    const int lane = threadIdx.x & 63;
    int64_t row;
    if (!wave_row(a.B, row)) return;
    const int D = a.D;
    const size_t base = row_base(row, D);
    const float* xq = a.x[0] + base;
    const float* xp = a.x[1] + base;
    const float* xn = a.x[2] + base;
    const int nv = D >> 2;

    float xr[3][kVec * 4];
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            const int v = lane + i * 64;
            f32x4 Q = {0, 0, 0, 0}, P = {0, 0, 0, 0}, N = {0, 0, 0, 0};
            if (v < nv) { Q = *(const f32x4*)(xq + v * 4); P = *(const f32x4*)(xp + v * 4); N = *(const f32x4*)(xn + v * 4); }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                xr[0][i * 4 + j] = Q[j]; xr[1][i * 4 + j] = P[j]; xr[2][i * 4 + j] = N[j];
                margin_accum<COS>(Q[j], P[j], N[j], s);      // past the row: zeros, which add nothing
            }
        }
    } else if (VEC) {
        for (int v = lane; v < nv; v += 64) {
            const f32x4 Q = *(const f32x4*)(xq + v * 4), P = *(const f32x4*)(xp + v * 4), N = *(const f32x4*)(xn + v * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) margin_accum<COS>(Q[j], P[j], N[j], s);
        }
    } else {
        for (int i = lane; i < D; i += 64) margin_accum<COS>(xq[i], xp[i], xn[i], s);
    }
    const float dqp = wave_sum(s[0]), dqn = wave_sum(s[1]);
    float nq = 0.f, np = 0.f, nn = 0.f;
    if (COS) { nq = sqrtf(wave_sum(s[2])); np = sqrtf(wave_sum(s[3])); nn = sqrtf(wave_sum(s[4])); }
    const CosVal sp = sim_finish<COS>(dqp, nq, np), sn = sim_finish<COS>(dqn, nq, nn);

    const float m = sp.m - sn.m;
    const float e = m - a.labels[row];
    if (lane == 0) {
        a.row_out[row] = e * e;
        if (a.margin_out) a.margin_out[row] = m;
    }
    if (a.g[0] == nullptr) return;

    // the finished gradient c * dm/dx with c = 2 (m - y) [/ B], then the upstream factor: one more rounding and no other
    float c = 2.f * e;
    if (a.reduction == QST_REDUCE_MEAN) c /= (float)a.B;
    float up = 1.f;
    if (a.grad_out) up = (a.reduction == QST_REDUCE_NONE) ? a.grad_out[row] : a.grad_out[0];
    const float kq = sp.kxx - sn.kxx;               // dm/dq = kxy_p * p - kxy_n * n + (kxx_p - kxx_n) * q
    auto emit = [&](float q, float p, float n, float& gq, float& gp, float& gn) {
        gq = (c * (sp.kxy * p - sn.kxy * n + kq * q)) * up;
        gp = (c * (sp.kxy * q + sp.kyy * p)) * up;
        gn = (-c * (sn.kxy * q + sn.kyy * n)) * up;
    };
    float* gq = a.g[0] + base;
    float* gp = a.g[1] + base;
    float* gn = a.g[2] + base;
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            const int v = lane + i * 64;
            if (v < nv) {
                f32x4 GQ, GP, GN;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float g0, g1, g2;
                    emit(xr[0][i * 4 + j], xr[1][i * 4 + j], xr[2][i * 4 + j], g0, g1, g2);
                    GQ[j] = g0; GP[j] = g1; GN[j] = g2;
                }
                *(f32x4*)(gq + v * 4) = GQ; *(f32x4*)(gp + v * 4) = GP; *(f32x4*)(gn + v * 4) = GN;
            }
        }
    } else if (VEC) {
        for (int v = lane; v < nv; v += 64) {
            const f32x4 Q = *(const f32x4*)(xq + v * 4), P = *(const f32x4*)(xp + v * 4), N = *(const f32x4*)(xn + v * 4);
            f32x4 GQ, GP, GN;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float g0, g1, g2;
                emit(Q[j], P[j], N[j], g0, g1, g2);
                GQ[j] = g0; GP[j] = g1; GN[j] = g2;
            }
            *(f32x4*)(gq + v * 4) = GQ; *(f32x4*)(gp + v * 4) = GP; *(f32x4*)(gn + v * 4) = GN;
        }
    } else {
        for (int i = lane; i < D; i += 64) {
            float g0, g1, g2;
            emit(xq[i], xp[i], xn[i], g0, g1, g2);
            gq[i] = g0; gp[i] = g1; gn[i] = g2;
        }
    }
}

void launch_mse(const MseArgs& a, hipStream_t st) {
    const float* x[2] = {a.x, a.t};
    dispatch_form<true>(a.D, rows_al16(x, 2, &a.g, 1), [&](auto nv, auto vec) {
        embed_mse_kernel<decltype(nv)::value, decltype(vec)::value><<<row_grid(a.B), 256, 0, st>>>(a);
    });
}

template <bool COS>
void launch_margin(const MarginArgs& a, hipStream_t st) {
    dispatch_form<true>(a.D, rows_al16(a.x, 3, a.g, 3), [&](auto nv, auto vec) {
        margin_mse_kernel<COS, decltype(nv)::value, decltype(vec)::value><<<row_grid(a.B), 256, 0, st>>>(a);
    });
}

}  // namespace

extern "C" int qst_embed_mse(const float* x, const float* t, int B, int D, float* out_loss,
                             const float* grad_out, float* grad_x, float* scratch, void* stream) {
    if (!x || !t || !out_loss || !scratch || B < 1 || D < 1) return QST_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    MseArgs a = {};
    a.x = x; a.t = t; a.g = grad_x; a.grad_out = grad_out; a.row_out = scratch;
    a.B = B; a.D = D;
    a.k = (float)(2.0 / ((double)B * (double)D));
    launch_mse(a, st);
    QST_LAUNCH_CHECK();
    row_sum_kernel<double><<<1, 1024, 0, st>>>(scratch, B, (double)B * (double)D, out_loss);
    QST_LAUNCH_CHECK();
    return QST_OK;
}

extern "C" int qst_margin_mse_loss(const float* q, const float* p, const float* n, const float* labels, int B, int D, int sim,
                                   int reduction, float* out_loss, float* out_margin, const float* grad_out,
                                   float* grad_q, float* grad_p, float* grad_n, float* scratch, void* stream) {
    if (!q || !p || !n || !labels || !out_loss || B < 1 || D < 1) return QST_ERR_BAD_ARG;
    if (sim != QST_METRIC_DOT && sim != QST_METRIC_COS_SIM) return QST_ERR_BAD_ARG;
    if (reduction < QST_REDUCE_NONE || reduction > QST_REDUCE_MEAN) return QST_ERR_BAD_ARG;
    if (reduction != QST_REDUCE_NONE && !scratch) return QST_ERR_BAD_ARG;
    const int have = (grad_q != nullptr) + (grad_p != nullptr) + (grad_n != nullptr);
    if (have != 0 && have != 3) return QST_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    MarginArgs a = {};
    a.x[0] = q; a.x[1] = p; a.x[2] = n;
    a.g[0] = grad_q; a.g[1] = grad_p; a.g[2] = grad_n;
    a.labels = labels; a.grad_out = grad_out; a.margin_out = out_margin;
    a.row_out = (reduction == QST_REDUCE_NONE) ? out_loss : scratch;
    a.B = B; a.D = D; a.reduction = reduction;
    if (sim == QST_METRIC_COS_SIM) launch_margin<true>(a, st);
    else launch_margin<false>(a, st);
    QST_LAUNCH_CHECK();
    if (reduction != QST_REDUCE_NONE) {
        row_sum_kernel<double><<<1, 1024, 0, st>>>(scratch, B, reduction == QST_REDUCE_MEAN ? (double)B : 1.0, out_loss);
        QST_LAUNCH_CHECK();
    }
    return QST_OK;
}
