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
// the same bits. HBM-bound: 2 (3) rows read and, with gradients, 1 (3) written.
#include "qst_common.h"

namespace {

constexpr float kCosEps = 1e-8f;    // torch cosine_similarity default eps (each norm clamped on its own), as qst_pair_metric
constexpr int kMaxVec = 8;          // float4 per lane and row kept in registers -> D <= 64*4*8 = 2048

// wave_sum (qst_common.h) on a double: the same tree, each half of the value moved by its own DPP / readlane
template <int CTRL> __device__ __forceinline__ double dpp_mov_f64(double v) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)u, CTRL, 0xf, 0xf, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(u >> 32), CTRL, 0xf, 0xf, true);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double lane_bcast_f64(double v, int lane) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), lane);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
    v += dpp_mov_f64<0xB1>(v);
    v += dpp_mov_f64<0x4E>(v);
    v += dpp_mov_f64<0x141>(v);
    v += dpp_mov_f64<0x140>(v);
    return (lane_bcast_f64(v, 0) + lane_bcast_f64(v, 16)) + (lane_bcast_f64(v, 32) + lane_bcast_f64(v, 48));
}

// ---- second stage: one workgroup over the per-row values, summed in double. Thread i takes rows i, i + 1024, ... in that
// order, then the wave tree, then the 16 wave totals through the same tree: a fixed order. div = 1 (sum), B (mean over the
// rows) or B * D (mean over the elements), divided in double and rounded to fp32 once.
__global__ __launch_bounds__(1024) void distill_reduce_kernel(const float* rows, int B, double div, float* out) {
    __shared__ double part[16];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < B; i += 1024) s += (double)rows[i];   // 64-bit: i passes B, and B may be near INT_MAX
    s = wave_sum_f64(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    double r = (threadIdx.x & 63) < 16 ? part[threadIdx.x & 63] : 0.0;
    r = wave_sum_f64(r);
    if (threadIdx.x == 0) out[0] = (float)(r / div);
}

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
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.B) return;
    const int D = a.D;
    const size_t base = (size_t)row * D;
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
struct SimVal { float m, kxy, kxx, kyy; };
template <bool COS>
__device__ __forceinline__ SimVal sim_finish(float dot, float nx, float ny) {
    SimVal r = {dot, 1.f, 0.f, 0.f};
    if (COS) {
        const float cx = fmaxf(nx, kCosEps), cy = fmaxf(ny, kCosEps);
        const float inv = 1.f / (cx * cy);
        const float cs = dot * inv;
        r.m = cs;
        r.kxy = inv;
        r.kxx = nx > kCosEps ? -cs / (cx * cx) : 0.f;
        r.kyy = ny > kCosEps ? -cs / (cy * cy) : 0.f;
    }
    return r;
}

template <bool COS, int NV, bool VEC>
__global__ __launch_bounds__(256) void margin_mse_kernel(MarginArgs a) {
    constexpr int kVec = NV > 0 ? NV : 1;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.B) return;
    const int D = a.D;
    const size_t base = (size_t)row * D;
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
    const SimVal sp = sim_finish<COS>(dqp, nq, np), sn = sim_finish<COS>(dqn, nq, nn);

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

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// which of the three forms a launch takes: NV of the register-resident form (0 = a streaming form) and whether the
// streaming form loads 16 bytes a lane
void pick_form(int D, bool aligned, int& nvreg, bool& vec) {
    vec = (D % 4 == 0) && aligned;
    nvreg = 0;
    if (vec && D <= 64 * 4 * kMaxVec) {
        const int n = (D + 255) / 256;
        nvreg = n <= 4 ? n : kMaxVec;
    }
}

void launch_mse(const MseArgs& a, hipStream_t st) {
    int nvreg; bool vec;
    pick_form(a.D, al16(a.x) && al16(a.t) && (!a.g || al16(a.g)), nvreg, vec);
    const int grid = (int)(((int64_t)a.B + 3) / 4);
    switch (nvreg) {
        case 1: embed_mse_kernel<1, true><<<grid, 256, 0, st>>>(a); break;
        case 2: embed_mse_kernel<2, true><<<grid, 256, 0, st>>>(a); break;
        case 3: embed_mse_kernel<3, true><<<grid, 256, 0, st>>>(a); break;
        case 4: embed_mse_kernel<4, true><<<grid, 256, 0, st>>>(a); break;
        case 8: embed_mse_kernel<8, true><<<grid, 256, 0, st>>>(a); break;
        default:
            if (vec) embed_mse_kernel<0, true><<<grid, 256, 0, st>>>(a);
            else embed_mse_kernel<0, false><<<grid, 256, 0, st>>>(a);
    }
}

template <bool COS>
void launch_margin(const MarginArgs& a, hipStream_t st) {
    bool aligned = true;
    for (int k = 0; k < 3; ++k) aligned = aligned && al16(a.x[k]) && (!a.g[0] || al16(a.g[k]));
    int nvreg; bool vec;
    pick_form(a.D, aligned, nvreg, vec);
    const int grid = (int)(((int64_t)a.B + 3) / 4);
    switch (nvreg) {
        case 1: margin_mse_kernel<COS, 1, true><<<grid, 256, 0, st>>>(a); break;
        case 2: margin_mse_kernel<COS, 2, true><<<grid, 256, 0, st>>>(a); break;
        case 3: margin_mse_kernel<COS, 3, true><<<grid, 256, 0, st>>>(a); break;
        case 4: margin_mse_kernel<COS, 4, true><<<grid, 256, 0, st>>>(a); break;
        case 8: margin_mse_kernel<COS, 8, true><<<grid, 256, 0, st>>>(a); break;
        default:
            if (vec) margin_mse_kernel<COS, 0, true><<<grid, 256, 0, st>>>(a);
            else margin_mse_kernel<COS, 0, false><<<grid, 256, 0, st>>>(a);
    }
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
    distill_reduce_kernel<<<1, 1024, 0, st>>>(scratch, B, (double)B * (double)D, out_loss);
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
        distill_reduce_kernel<<<1, 1024, 0, st>>>(scratch, B, reduction == QST_REDUCE_MEAN ? (double)B : 1.0, out_loss);
        QST_LAUNCH_CHECK();
    }
    return QST_OK;
}
