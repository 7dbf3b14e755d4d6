// listwise.hip -- distillation from a teacher's scores over a LIST of candidates per query (one positive, K - 1 negatives),
// forward + backward in one launch (one wave64 per example):
//
//   qst_listwise_distill_loss   kind QST_LISTWISE_KL          T^2 KL(softmax(labels / T) || softmax(sim(q, d_j) / T)) over the
//                                                             K candidates: losses.DistillKLDivLoss
//                               kind QST_LISTWISE_MARGIN_MSE  sum_{j >= 1} (sim(q, d_0) - sim(q, d_j) - labels_{j-1})^2:
//                                                             losses.MarginMSELoss with several negatives
//
// distill.hip's shape with a list in place of the pair: the wave keeps the query row in registers up to D = 2048 and streams
// each candidate row once, 16 bytes a lane, for its score; lane j then holds score j (K <= 64) with the scalars of its
// gradient, and both softmaxes and the row value are DPP reductions around their maxima. A second pass over the candidates
// writes grad_docs and sums grad_q in registers, so the candidates are read twice and none is kept. Past D = 2048 (or
// unaligned, or D % 4 != 0) the query streams as well, and the second pass walks the row chunk by chunk with the candidates
// inside, which keeps grad_q's partial sums in registers all the same. The per-row values go through row_loss.h's
// one-workgroup second stage in double, in a fixed order. No atomics anywhere: the same inputs give the same bits.
// HBM-bound: (1 + K) rows read for the value and, with gradients, K rows read again and (1 + K) written.
#include "row_loss.h"

namespace {

struct ListArgs {
    const float* q;                 // [B, D]
    const float* docs;              // [K, B, D]: candidate j of example b at (j * B + b) * D
    const float* labels;            // [B, K] (KL) or [B, K - 1] (margin)
    float* gq;                      // [B, D]; gq and gd both null = forward only
    float* gd;                      // [K, B, D]
    const float* grad_out;          // [B] (reduction none) or [1]; null = ones
    float* row_out;                 // [B] per-row value
    float* scores_out;              // [B, K] or null
    int B, K, D, kind, reduction;
    float temperature;
};

// sim(q, d) and the scalars of its gradient, d sim / dq = kxy * d + kxx * q and d sim / dd = kxy * q + kyy * d: the formulas
// of qst_pair_metric, as in distill.hip
template <bool COS>
__device__ __forceinline__ CosVal list_sim(float dot, float nq, float nd) {
    return COS ? cos_finish(dot, nq, nd, false) : CosVal{dot, 1.f, 0.f, 0.f};
}

template <bool COS>
__device__ __forceinline__ void list_accum(float q, float d, float& dot, float& nn) {
    dot += q * d;
    if (COS) nn += d * d;
}

// NV > 0: the query is NV float4 per lane in registers. NV == 0: it streams with the candidates, 16 bytes a lane (VEC) or
// element by element.
template <bool COS, int NV, bool VEC>
__global__ __launch_bounds__(256) void listwise_kernel(ListArgs a) {
    constexpr int kVec = NV > 0 ? NV : 1;
    const int lane = threadIdx.x & 63;
    int64_t row;
    if (!wave_row(a.B, row)) return;
    const int D = a.D, K = a.K;
    const int nv = D >> 2;
    const size_t base = row_base(row, D);
    const size_t cand = (size_t)a.B * (size_t)D;        // from candidate j to j + 1 of the same example
    const float* xq = a.q + base;
    const float* xd = a.docs + base;

    // ---- the query: into the registers, and its norm
    float qr[kVec * 4];
    float sq = 0.f;
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            const int v = lane + i * 64;
            f32x4 Q = {0, 0, 0, 0};
            if (v < nv) Q = *(const f32x4*)(xq + v * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { qr[i * 4 + e] = Q[e]; sq += Q[e] * Q[e]; }     // past the row: zeros, which add nothing
        }
    } else if (COS) {
        if (VEC) {
            for (int v = lane; v < nv; v += 64) {
                const f32x4 Q = *(const f32x4*)(xq + v * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) sq += Q[e] * Q[e];
            }
        } else {
            for (int i = lane; i < D; i += 64) sq += xq[i] * xq[i];
        }
    }
    const float nq = COS ? sqrtf(wave_sum(sq)) : 0.f;

    // ---- first pass: candidate j's similarity and gradient scalars end up in lane j
    CosVal mine = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < K; ++j) {
        const float* d = xd + (size_t)j * cand;
        float dot = 0.f, nn = 0.f;
        if (NV > 0) {
#pragma unroll
            for (int i = 0; i < kVec; ++i) {
                const int v = lane + i * 64;
                f32x4 X = {0, 0, 0, 0};
                if (v < nv) X = *(const f32x4*)(d + v * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) list_accum<COS>(qr[i * 4 + e], X[e], dot, nn);
            }
        } else if (VEC) {
            for (int v = lane; v < nv; v += 64) {
                const f32x4 Q = *(const f32x4*)(xq + v * 4), X = *(const f32x4*)(d + v * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) list_accum<COS>(Q[e], X[e], dot, nn);
            }
        } else {
            for (int i = lane; i < D; i += 64) list_accum<COS>(xq[i], d[i], dot, nn);
        }
        dot = wave_sum(dot);
        const float nd = COS ? sqrtf(wave_sum(nn)) : 0.f;
        const CosVal cv = list_sim<COS>(dot, nq, nd);
        if (lane == j) mine = cv;
    }
    const bool active = lane < K;
    const float sim = mine.m;
    if (a.scores_out && active) a.scores_out[row * K + lane] = sim;

    // ---- the row value and g = d row / d sim_j, lane j's
    float value, g;
    if (a.kind == QST_LISTWISE_KL) {
        // student s = sim / T and teacher l = labels / T, each softmax around its own maximum; lanes past K hold -inf and
        // weigh exp(-inf) = 0. A term whose teacher weight is exactly 0 counts 0 (torch's xlogy), whatever its logarithm is
        const float T = a.temperature;
        const float ninf = -__builtin_inff();
        const float s = active ? sim / T : ninf;
        const float l = active ? a.labels[row * K + lane] / T : ninf;
        const float ms = wave_max(s), ml = wave_max(l);
        const float es = active ? expf(s - ms) : 0.f;
        const float el = active ? expf(l - ml) : 0.f;
        const float zs = wave_sum(es), zl = wave_sum(el);
        const float log_p = (s - ms) - logf(zs);
        const float log_t = (l - ml) - logf(zl);
        const float p = es / zs, t = el / zl;
        const float term = (t == 0.f) ? 0.f : t * (log_t - log_p);
        value = (T * T) * wave_sum(term);
        g = active ? T * (p - t) : 0.f;
    } else {
        const float s0 = lane_bcast(sim, 0);
        const bool neg = active && lane >= 1;
        const float y = neg ? a.labels[row * (K - 1) + (lane - 1)] : 0.f;
        const float e = neg ? (s0 - sim) - y : 0.f;
        value = wave_sum(e * e);
        const float ge = 2.f * e;
        const float g0 = wave_sum(ge);                  // the positive is in every residual
        g = lane == 0 ? g0 : -ge;
    }
    if (lane == 0) a.row_out[row] = value;
    if (a.gq == nullptr) return;

    // ---- second pass. The finished gradient c_j * d sim_j / dx with c = g [/ B or / (B (K - 1))], then the upstream factor:
    // one more rounding and no other
    float c = g;
    if (a.reduction == QST_REDUCE_MEAN)
        c /= (a.kind == QST_LISTWISE_KL) ? (float)a.B : (float)((int64_t)a.B * (K - 1));
    float up = 1.f;
    if (a.grad_out) up = (a.reduction == QST_REDUCE_NONE) ? a.grad_out[row] : a.grad_out[0];
    // grad_d_j = cxy_j * q + cyy_j * d_j; grad_q = sum_j cxy_j * d_j + cq * q
    const float cxy = COS ? c * mine.kxy : c;
    const float cyy = COS ? c * mine.kyy : 0.f;
    const float cq = COS ? wave_sum(c * mine.kxx) : 0.f;
    float* gq = a.gq + base;
    float* gd = a.gd + base;
    if (NV > 0) {
        float acc[kVec * 4];
#pragma unroll
        for (int i = 0; i < kVec * 4; ++i) acc[i] = 0.f;
        for (int j = 0; j < K; ++j) {
            const float wxy = lane_bcast(cxy, j), wyy = lane_bcast(cyy, j);
            const float* d = xd + (size_t)j * cand;
            float* gj = gd + (size_t)j * cand;
#pragma unroll
            for (int i = 0; i < kVec; ++i) {
                const int v = lane + i * 64;
                if (v < nv) {
                    const f32x4 X = *(const f32x4*)(d + v * 4);
                    f32x4 G;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        G[e] = (COS ? wxy * qr[i * 4 + e] + wyy * X[e] : wxy * qr[i * 4 + e]) * up;
                        acc[i * 4 + e] += wxy * X[e];
                    }
                    *(f32x4*)(gj + v * 4) = G;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            const int v = lane + i * 64;
            if (v < nv) {
                f32x4 G;
#pragma unroll
                for (int e = 0; e < 4; ++e) G[e] = (COS ? acc[i * 4 + e] + cq * qr[i * 4 + e] : acc[i * 4 + e]) * up;
                *(f32x4*)(gq + v * 4) = G;
            }
        }
    } else if (VEC) {
        // chunk by chunk with the candidates inside: grad_q's chunk is summed in registers and written once. The trips are
        // the same for every lane (the broadcasts of lane j's scalars run with the whole wave), the accesses are guarded
        for (int v0 = 0; v0 < nv; v0 += 64) {
            const int v = v0 + lane;
            const bool on = v < nv;
            f32x4 Q = {0, 0, 0, 0}, A = {0, 0, 0, 0};
            if (on) Q = *(const f32x4*)(xq + v * 4);
            for (int j = 0; j < K; ++j) {
                const float wxy = lane_bcast(cxy, j), wyy = lane_bcast(cyy, j);
                if (on) {
                    const f32x4 X = *(const f32x4*)(xd + (size_t)j * cand + v * 4);
                    f32x4 G;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        G[e] = (COS ? wxy * Q[e] + wyy * X[e] : wxy * Q[e]) * up;
                        A[e] += wxy * X[e];
                    }
                    *(f32x4*)(gd + (size_t)j * cand + v * 4) = G;
                }
            }
            if (on) {
                f32x4 G;
#pragma unroll
                for (int e = 0; e < 4; ++e) G[e] = (COS ? A[e] + cq * Q[e] : A[e]) * up;
                *(f32x4*)(gq + v * 4) = G;
            }
        }
    } else {
        for (int i0 = 0; i0 < D; i0 += 64) {
            const int i = i0 + lane;
            const bool on = i < D;
            const float Q = on ? xq[i] : 0.f;
            float A = 0.f;
            for (int j = 0; j < K; ++j) {
                const float wxy = lane_bcast(cxy, j), wyy = lane_bcast(cyy, j);
                if (on) {
                    const float X = xd[(size_t)j * cand + i];
                    gd[(size_t)j * cand + i] = (COS ? wxy * Q + wyy * X : wxy * Q) * up;
                    A += wxy * X;
                }
            }
            if (on) gq[i] = (COS ? A + cq * Q : A) * up;
        }
    }
}

template <bool COS>
void launch_listwise(const ListArgs& a, hipStream_t st) {
    const float* x[2] = {a.q, a.docs};
    float* g[2] = {a.gq, a.gd};
    dispatch_form<true>(a.D, rows_al16(x, 2, g, 2), [&](auto nv, auto vec) {
        listwise_kernel<COS, decltype(nv)::value, decltype(vec)::value><<<row_grid(a.B), 256, 0, st>>>(a);
    });
}

}  // namespace

extern "C" int qst_listwise_distill_loss(const float* q, const float* docs, const float* labels, int B, int K, int D, int kind,
                                         int sim, float temperature, int reduction, float* out_loss, float* out_scores,
                                         const float* grad_out, float* grad_q, float* grad_docs, float* scratch,
                                         void* stream) {
    if (!q || !docs || !labels || !out_loss || B < 1 || D < 1) return QST_ERR_BAD_ARG;
    if (kind != QST_LISTWISE_KL && kind != QST_LISTWISE_MARGIN_MSE) return QST_ERR_BAD_ARG;
    if (sim != QST_METRIC_DOT && sim != QST_METRIC_COS_SIM) return QST_ERR_BAD_ARG;
    if (reduction < QST_REDUCE_NONE || reduction > QST_REDUCE_MEAN) return QST_ERR_BAD_ARG;
    if (reduction != QST_REDUCE_NONE && !scratch) return QST_ERR_BAD_ARG;
    if (kind == QST_LISTWISE_KL && !(temperature > 0.f && temperature <= 3.402823466e38f)) return QST_ERR_BAD_ARG;
    if ((grad_q != nullptr) != (grad_docs != nullptr)) return QST_ERR_BAD_ARG;
    if (K < 1 || K > 64) return QST_ERR_UNSUPPORTED;
    if (kind == QST_LISTWISE_MARGIN_MSE && K < 2) return QST_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    ListArgs a = {};
    a.q = q; a.docs = docs; a.labels = labels; a.gq = grad_q; a.gd = grad_docs;
    a.grad_out = grad_out; a.scores_out = out_scores;
    a.row_out = (reduction == QST_REDUCE_NONE) ? out_loss : scratch;
    a.B = B; a.K = K; a.D = D; a.kind = kind; a.reduction = reduction; a.temperature = temperature;
    if (sim == QST_METRIC_COS_SIM) launch_listwise<true>(a, st);
    else launch_listwise<false>(a, st);
    QST_LAUNCH_CHECK();
    if (reduction != QST_REDUCE_NONE) {
        double k = 1.0;
        if (reduction == QST_REDUCE_MEAN) k = (kind == QST_LISTWISE_KL) ? (double)B : (double)B * (double)(K - 1);
        row_sum_kernel<double><<<1, 1024, 0, st>>>(scratch, B, k, out_loss);
        QST_LAUNCH_CHECK();
    }
    return QST_OK;
}
