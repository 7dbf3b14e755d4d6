// tuple_loss.hip -- fused row-wise pair and triplet losses, forward + backward (one wave64 per row).
//
// The neighbours of the gamma-quadruplet loss (loss.hip) that sentence-transformers 2.2.2 trains bi-encoders with:
// CosineSimilarityLoss, ContrastiveLoss, OnlineContrastiveLoss, TripletLoss, and the per-row metric itself (what
// EmbeddingSimilarityEvaluator scores with). Each is a function of one or two pair metrics per row, so every kernel here has
// quad_loss_kernel's shape: the rows are read once with 16-byte coalesced loads, kept in registers, reduced with DPP, and the
// gradient pass runs from the registers. HBM-bound: k*D*4 bytes read per row (+ as many written with gradients). The choice of
// the form, the sum over the rows and the cosine's scalars are row_loss.h's, shared with loss.hip and distill.hip.
//
//   COS_SIM  u.v / (max(|u|, 1e-8) max(|v|, 1e-8))     COS_DIST 1 - COS_SIM     DOT u.v
//   L2 / L1  |u - v + 1e-6|_p (torch pairwise_distance) L2_PLAIN / L1_PLAIN |u - v|_p
//
// The L1 sum runs in fp64. That distance grows with D (73.8 at D = 64), and the contrastive gradient of a negative is
// (margin - d): a row 0.05 inside the margin turns the 0.8 ulp an fp32 sum of 64 terms is off by (6e-6) into 1.2e-4 of its
// gradient, and among a few thousand rows some always lie that close. The L1 hinges take d as a double; what is stored and
// returned stays fp32. L2 (sqrt(2 D) for random rows, 0.3 of the gradient tolerance on the same rows) and the cosine metrics
// (bounded by 2) stay in fp32, bit for bit as before. The kernels stay HBM-bound.
#include "row_loss.h"

namespace {

constexpr float kPairEps = 1e-6f;   // torch pairwise_distance default eps (added to the difference)

enum { MODE_METRIC = 0, MODE_MSE, MODE_CONTRASTIVE, MODE_ONLINE_FWD, MODE_ONLINE_BWD, MODE_TRIPLET };

struct TupleArgs {
    const float* x[3];              // u, v | anchor, positive, negative
    float* g[3];                    // grads (all null = forward only)
    const float* labels;            // [B] (pair losses)
    const float* grad_out;          // upstream (may be null = ones)
    const float* sel;               // MODE_ONLINE_BWD: d[B], then {t_pos, t_neg}
    float* row_out;                 // [B] per-row value
    int B, D, mode, metric, reduction;
    float margin, eps;
};

// metric class: 0 = products (cosine, dot), 1 = L2 of the difference, 2 = L1 of the difference (summed in fp64 into sd)
// EXACT: every product-and-add is an explicit fma, so the compiler has no choice between fused and unfused forms (left to
// itself it packs two pairs of a tuple into v_pk_fma_f32 and gives the third v_mul + v_add: equal inputs, unequal sums).
// The losses keep EXACT = false and with it the bits they have always produced.
template <int MC, bool EXACT = false>
__device__ __forceinline__ void accum(float x, float y, float eps, float (&s)[3], double& sd) {
    if (MC == 0) {
        if (EXACT) { s[0] = __builtin_fmaf(x, y, s[0]); s[1] = __builtin_fmaf(x, x, s[1]); s[2] = __builtin_fmaf(y, y, s[2]); }
        else { s[0] += x * y; s[1] += x * x; s[2] += y * y; }
    } else if (MC == 1) {
        const float t = x - y + eps;
        if (EXACT) s[0] = __builtin_fmaf(t, t, s[0]);
        else s[0] += t * t;
    } else sd += fabs((double)x - (double)y + (double)eps);
}

// value m of a pair and the scalars of its gradient: MC 0: dm/dx = kxy*y + kxx*x, dm/dy = kxy*x + kyy*y;
// MC 1: dm/dx = kxy * (x - y + eps) = -dm/dy (0 where the distance is 0, as torch's norm backward masks);
// MC 2: dm/dx = sign(x - y + eps) = -dm/dy
// md: m before its rounding to fp32 (MC 2), for the hinges
struct PairVal { float m, kxy, kxx, kyy; double md; };

// EXACT (value only, cosine similarity or distance): the same formula with contraction off, one IEEE operation per
// operator, for the reason given at accum
template <int MC, bool EXACT = false>
__device__ __forceinline__ PairVal finish(const float (&s)[3], double sd, int metric) {
    PairVal r = {0.f, 0.f, 0.f, 0.f, 0.0};
    if (MC == 0) {
        const float dot = wave_sum(s[0]);
        if (metric == QST_METRIC_DOT) { r.m = dot; r.kxy = 1.f; r.md = (double)dot; return r; }
        const float nx = sqrtf(wave_sum(s[1])), ny = sqrtf(wave_sum(s[2]));
        if (EXACT) {
#pragma clang fp contract(off)
            const float cx = fmaxf(nx, kCosEps), cy = fmaxf(ny, kCosEps);
            const float den = cx * cy;
            const float inv = 1.f / den;
            const float cs = dot * inv;
            r.m = (metric == QST_METRIC_COS_DIST) ? 1.f - cs : cs;
            r.md = (double)r.m;
            return r;
        }
        const CosVal c = cos_finish(dot, nx, ny, metric == QST_METRIC_COS_DIST);
        r.m = c.m; r.kxy = c.kxy; r.kxx = c.kxx; r.kyy = c.kyy;
        r.md = (double)r.m;
    } else if (MC == 1) {
        r.m = sqrtf(wave_sum(s[0]));
        r.md = (double)r.m;
        r.kxy = r.m > 0.f ? 1.f / r.m : 0.f;
    } else {
        r.md = wave_sum_f64(sd);
        r.m = (float)r.md;
        r.kxy = 1.f;
    }
    return r;
}

// c * dm/dx and c * dm/dy of one element
template <int MC>
__device__ __forceinline__ void pair_grad(const PairVal& v, float c, float x, float y, float eps, float& gx, float& gy) {
    if (MC == 0) {
        gx = c * (v.kxy * y + v.kxx * x);
        gy = c * (v.kxy * x + v.kyy * y);
    } else {
        const float t = x - y + eps;
        const float e = (MC == 1) ? c * v.kxy * t : (t > 0.f ? c : (t < 0.f ? -c : 0.f));
        gx = e; gy = -e;
    }
}

// NX: rows per tuple (2 pair, 3 triplet). NV: float4 per lane kept in registers; 0 = scalar path (D not a multiple of 4,
// D > 2048 or unaligned pointers), which re-reads the rows for the gradient pass.
template <int MC, int NX, int NV>
__global__ __launch_bounds__(256) void tuple_loss_kernel(TupleArgs a) {
    constexpr bool VEC = NV > 0;
    constexpr int kVec = NV > 0 ? NV : 1;
    constexpr int NP = NX - 1;                      // pairs: (x0, x1)[, (x0, x2)]
    const int lane = threadIdx.x & 63;
    int64_t row;
    if (!wave_row(a.B, row)) return;
    const int D = a.D;
    const size_t base = row_base(row, D);
    const float eps = a.eps;

    float xr[NX][VEC ? kVec * 4 : 1];
    float s[NP][3];
    double sd[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) { s[p][0] = 0.f; s[p][1] = 0.f; s[p][2] = 0.f; sd[p] = 0.0; }

    if (VEC) {
        const int nv = D >> 2;
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            const int v = lane + i * 64;
            const bool in = v < nv;
            f32x4 X[NX];
#pragma unroll
            for (int k = 0; k < NX; ++k) {
                X[k] = f32x4{0, 0, 0, 0};
                if (in) X[k] = *(const f32x4*)(a.x[k] + base + v * 4);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int k = 0; k < NX; ++k) xr[k][i * 4 + j] = X[k][j];
                if (in) {
#pragma unroll
                    for (int p = 0; p < NP; ++p) accum<MC>(X[0][j], X[p + 1][j], eps, s[p], sd[p]);
                }
            }
        }
    } else {
        for (int i = lane; i < D; i += 64) {
            const float x0 = a.x[0][base + i];
#pragma unroll
            for (int p = 0; p < NP; ++p) accum<MC>(x0, a.x[p + 1][base + i], eps, s[p], sd[p]);
        }
    }
    PairVal pv[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) pv[p] = finish<MC>(s[p], sd[p], a.metric);

    // row value and d(row value)/d(pair metric)
    float val, c[NP];
    const float m = pv[0].m;
    if (NX == 3) {
        const float h = MC == 2 ? (float)(pv[0].md - pv[NP - 1].md + (double)a.margin) : m - pv[NP - 1].m + a.margin;
        val = fmaxf(h, 0.f);
        c[0] = h > 0.f ? 1.f : 0.f;                 // F.relu passes no gradient at 0
        c[NP - 1] = -c[0];
    } else {
        const float y = a.labels ? a.labels[row] : 0.f;
        switch (a.mode) {
            case MODE_MSE: val = (m - y) * (m - y); c[0] = 2.f * (m - y); break;
            case MODE_CONTRASTIVE: {
                const float r = MC == 2 ? (float)fmax((double)a.margin - pv[0].md, 0.0) : fmaxf(a.margin - m, 0.f);
                val = 0.5f * (y * m * m + (1.f - y) * r * r);
                c[0] = y * m - (1.f - y) * r;
                break;
            }
            case MODE_ONLINE_BWD: {
                // the selection is stage 2's, taken on the distances stage 1 stored; the thresholds carry no gradient
                const float dsel = a.sel[row], t_pos = a.sel[a.B], t_neg = a.sel[a.B + 1];
                val = m; c[0] = 0.f;
                if (y == 1.f && dsel > t_pos) c[0] = 2.f * m;
                else if (y == 0.f && dsel < t_neg)
                    c[0] = -2.f * (MC == 2 ? (float)fmax((double)a.margin - pv[0].md, 0.0) : fmaxf(a.margin - m, 0.f));
                break;
            }
            default: val = m; c[0] = 1.f; break;    // MODE_METRIC, MODE_ONLINE_FWD
        }
    }
    if (a.mode != MODE_ONLINE_BWD) { if (lane == 0) a.row_out[row] = val; }
    if (a.g[0] == nullptr) return;

    float up = 1.f;
    if (a.grad_out) up = (a.reduction == QST_REDUCE_NONE) ? a.grad_out[row] : a.grad_out[0];
    if (a.reduction == QST_REDUCE_MEAN) up /= (float)a.B;
#pragma unroll
    for (int p = 0; p < NP; ++p) c[p] *= up;

    auto emit = [&](const float (&x)[NX], float (&g)[NX]) {
        float g0, g1;
        pair_grad<MC>(pv[0], c[0], x[0], x[1], eps, g0, g1);
        g[0] = g0; g[1] = g1;
        if (NX == 3) {
            pair_grad<MC>(pv[NP - 1], c[NP - 1], x[0], x[NX - 1], eps, g0, g1);
            g[0] += g0; g[NX - 1] = g1;
        }
    };
    if (VEC) {
        const int nv = D >> 2;
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            const int v = lane + i * 64;
            if (v < nv) {
                f32x4 G[NX];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float x[NX], g[NX];
#pragma unroll
                    for (int k = 0; k < NX; ++k) x[k] = xr[k][i * 4 + j];
                    emit(x, g);
#pragma unroll
                    for (int k = 0; k < NX; ++k) G[k][j] = g[k];
                }
#pragma unroll
                for (int k = 0; k < NX; ++k) *(f32x4*)(a.g[k] + base + v * 4) = G[k];
            }
        }
    } else {
        for (int i = lane; i < D; i += 64) {
            float x[NX], g[NX];
#pragma unroll
            for (int k = 0; k < NX; ++k) x[k] = a.x[k][base + i];
            emit(x, g);
#pragma unroll
            for (int k = 0; k < NX; ++k) a.g[k][base + i] = g[k];
        }
    }
}

// ---- one-workgroup second stages: fixed summation trees (row_loss.h: block_reduce), so results are bit-reproducible run to run
// OnlineContrastiveLoss's selection: the thresholds from the other class, then the sum over the selected rows.
// d: distances [B] followed by the two thresholds this kernel writes for the gradient launch.
__global__ __launch_bounds__(1024) void online_select_kernel(float* d, const float* labels, int B, float margin, float* out) {
    __shared__ float part[16];
    float np = 0.f, nn = 0.f, sp = 0.f, sn = 0.f, mx = -__builtin_inff(), mn = __builtin_inff();
    for (int i = threadIdx.x; i < B; i += 1024) {
        const float y = labels[i], v = d[i];
        if (y == 1.f) { np += 1.f; sp += v; mx = fmaxf(mx, v); }
        else if (y == 0.f) { nn += 1.f; sn += v; mn = fminf(mn, v); }
    }
    np = block_reduce<OP_SUM>(np, part); nn = block_reduce<OP_SUM>(nn, part);
    sp = block_reduce<OP_SUM>(sp, part); sn = block_reduce<OP_SUM>(sn, part);
    mx = block_reduce<OP_MAX>(mx, part); mn = block_reduce<OP_MIN>(mn, part);
    // the mean of an empty set is 0/0 = NaN, which compares false with everything: nothing selected, as in torch
    const float t_neg = np > 1.f ? mx : sn / nn;
    const float t_pos = nn > 1.f ? mn : sp / np;
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += 1024) {
        const float y = labels[i], v = d[i];
        if (y == 1.f && v > t_pos) s += v * v;
        else if (y == 0.f && v < t_neg) { const float r = fmaxf(margin - v, 0.f); s += r * r; }
    }
    s = block_reduce<OP_SUM>(s, part);
    if (threadIdx.x == 0) { d[B] = t_pos; d[B + 1] = t_neg; out[0] = s; }
}

template <int NX>
void launch_rows(TupleArgs a, hipStream_t st) {
    a.eps = (a.metric == QST_METRIC_L2 || a.metric == QST_METRIC_L1) ? kPairEps : 0.f;
    dispatch_form<false>(a.D, rows_al16(a.x, NX, a.g, NX), [&](auto nv, auto) {
        constexpr int NV = decltype(nv)::value;
        const int grid = row_grid(a.B);
        switch (a.metric) {
            case QST_METRIC_L2: case QST_METRIC_L2_PLAIN: tuple_loss_kernel<1, NX, NV><<<grid, 256, 0, st>>>(a); break;
            case QST_METRIC_L1: case QST_METRIC_L1_PLAIN: tuple_loss_kernel<2, NX, NV><<<grid, 256, 0, st>>>(a); break;
            default: tuple_loss_kernel<0, NX, NV><<<grid, 256, 0, st>>>(a); break;
        }
    });
}

bool grads_ok(float* const* g, int n, bool& any) {
    int have = 0;
    for (int k = 0; k < n; ++k) have += g[k] != nullptr;
    any = have > 0;
    return have == 0 || have == n;
}

bool distance_metric(int metric) {
    return metric == QST_METRIC_COS_DIST || metric == QST_METRIC_L2 || metric == QST_METRIC_L1;
}

// ---- quadruplet evaluation: the nine distances of a row (cosine, Manhattan, Euclidean of (a, p), (a, q), (a, n)) and the nine
// strict comparisons QuadrupletEvaluator counts, from ONE pass over the four rows. No gradient pass, so nothing is kept in
// registers and D is not bounded: the loops stream. All three metric classes accumulate side by side from the same loads; the
// three pairs of a metric run the same accum / finish sequence in its EXACT form (explicit fma, no contraction left to the
// compiler), so bitwise-equal columns give bitwise-equal distances.
struct QuadEvalArgs {
    const float* x[4];              // anchor, positive, partially positive, negative
    float* dist;                    // [B, 9] or null
    int32_t* flags;                 // [B]
    int B, D;
};

struct QuadAcc {
    float c[3][3], e[3][3];         // per pair: the cosine sums; the squared L2 sum in e[p][0]
    double m[3];                    // per pair: the L1 sum
};

__device__ __forceinline__ void quad_accum(QuadAcc& q, float x0, float x1, float x2, float x3) {
    const float y[3] = {x1, x2, x3};
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        double unused_d = 0.0;
        accum<0, true>(x0, y[p], 0.f, q.c[p], unused_d);
        accum<1, true>(x0, y[p], 0.f, q.e[p], unused_d);
        accum<2, true>(x0, y[p], 0.f, q.e[p], q.m[p]);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void quad_eval_kernel(QuadEvalArgs a) {
    const int lane = threadIdx.x & 63;
    int64_t row;
    if (!wave_row(a.B, row)) return;
    const int D = a.D;
    const size_t base = row_base(row, D);
    const float* xa = a.x[0] + base;
    const float* xp = a.x[1] + base;
    const float* xq = a.x[2] + base;
    const float* xn = a.x[3] + base;

    QuadAcc q;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        q.m[p] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { q.c[p][k] = 0.f; q.e[p][k] = 0.f; }
    }
    if (VEC) {
        const int nv = D >> 2;
        for (int v = lane; v < nv; v += 64) {
            const f32x4 A = *(const f32x4*)(xa + v * 4), P = *(const f32x4*)(xp + v * 4);
            const f32x4 Q = *(const f32x4*)(xq + v * 4), N = *(const f32x4*)(xn + v * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) quad_accum(q, A[j], P[j], Q[j], N[j]);
        }
    } else {
        for (int i = lane; i < D; i += 64) quad_accum(q, xa[i], xp[i], xq[i], xn[i]);
    }

    // d[3 * metric + pair]: what out_dist receives, and what is compared whether or not it is stored
    float d[9];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        d[p] = finish<0, true>(q.c[p], 0.0, QST_METRIC_COS_DIST).m;
        d[3 + p] = finish<2, true>(q.e[p], q.m[p], QST_METRIC_L1_PLAIN).m;
        d[6 + p] = finish<1, true>(q.e[p], 0.0, QST_METRIC_L2_PLAIN).m;
    }
    int32_t f = 0;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        f |= (d[3 * m] < d[3 * m + 1] ? 1 : 0) << (3 * m);          // pos_part
        f |= (d[3 * m] < d[3 * m + 2] ? 1 : 0) << (3 * m + 1);      // pos_neg
        f |= (d[3 * m + 1] < d[3 * m + 2] ? 1 : 0) << (3 * m + 2);  // part_neg
    }
    if (lane == 0) {
        a.flags[row] = f;
        if (a.dist) {
#pragma unroll
            for (int k = 0; k < 9; ++k) a.dist[(size_t)row * 9 + k] = d[k];
        }
    }
}

// counts[k] = number of rows whose bit k is set. One workgroup; integer sums, so the order cannot matter. Every wave walks the
// rows in whole trips of 1024 (its lanes past B hold 0), which keeps the ballots wave-uniform.
__global__ __launch_bounds__(1024) void quad_count_kernel(const int32_t* flags, int B, int32_t* counts) {
    __shared__ int32_t part[16][9];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t c[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) c[k] = 0;
    for (int64_t i0 = 0; i0 < B; i0 += 1024) {  // 64-bit: the last trip's indices pass B, and B may be near INT_MAX
        const int64_t i = i0 + threadIdx.x;
        const int32_t f = (i < B) ? flags[i] : 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) c[k] += (int32_t)__popcll(__ballot((f >> k) & 1));
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) part[wave][k] = c[k];
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        int32_t s = 0;
        for (int w = 0; w < 16; ++w) s += part[w][threadIdx.x];
        counts[threadIdx.x] = s;
    }
}

}  // namespace

extern "C" int qst_pair_metric(const float* u, const float* v, int B, int D, int metric, float* out,
                               const float* grad_out, float* grad_u, float* grad_v, void* stream) {
    if (!u || !v || !out || B <= 0 || D <= 0) return QST_ERR_BAD_ARG;
    if (metric < QST_METRIC_COS_SIM || metric > QST_METRIC_L1_PLAIN) return QST_ERR_BAD_ARG;
    float* g[2] = {grad_u, grad_v};
    bool any_g;
    if (!grads_ok(g, 2, any_g)) return QST_ERR_BAD_ARG;
    TupleArgs a = {};
    a.x[0] = u; a.x[1] = v; a.g[0] = grad_u; a.g[1] = grad_v;
    a.grad_out = grad_out; a.row_out = out;
    a.B = B; a.D = D; a.mode = MODE_METRIC; a.metric = metric; a.reduction = QST_REDUCE_NONE;
    launch_rows<2>(a, (hipStream_t)stream);
    QST_LAUNCH_CHECK();
    return QST_OK;
}

extern "C" int qst_pair_loss(const float* u, const float* v, const float* labels, int B, int D, int kind, int metric,
                             float margin, int reduction, float* out_loss, const float* grad_out,
                             float* grad_u, float* grad_v, float* scratch, void* stream) {
    if (!u || !v || !labels || !out_loss || B <= 0 || D <= 0) return QST_ERR_BAD_ARG;
    if (reduction < QST_REDUCE_NONE || reduction > QST_REDUCE_MEAN) return QST_ERR_BAD_ARG;
    if (kind < QST_PAIR_MSE || kind > QST_PAIR_ONLINE_CONTRASTIVE) return QST_ERR_BAD_ARG;
    if ((kind == QST_PAIR_ONLINE_CONTRASTIVE || reduction != QST_REDUCE_NONE) && !scratch) return QST_ERR_BAD_ARG;
    if (kind == QST_PAIR_MSE ? metric != QST_METRIC_COS_SIM : !distance_metric(metric)) return QST_ERR_BAD_ARG;
    if (!(margin >= 0.f)) return QST_ERR_BAD_ARG;
    float* g[2] = {grad_u, grad_v};
    bool any_g;
    if (!grads_ok(g, 2, any_g)) return QST_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    TupleArgs a = {};
    a.x[0] = u; a.x[1] = v; a.labels = labels; a.grad_out = grad_out;
    a.B = B; a.D = D; a.metric = metric; a.margin = margin;
    if (kind == QST_PAIR_ONLINE_CONTRASTIVE) {
        // stage 1: distances; stage 2: thresholds + sum (one workgroup, fixed order); stage 3 (with gradients): the
        // per-row coefficient applied to the recomputed distance's gradient
        a.mode = MODE_ONLINE_FWD; a.row_out = scratch; a.reduction = QST_REDUCE_SUM;
        launch_rows<2>(a, st);
        QST_LAUNCH_CHECK();
        online_select_kernel<<<1, 1024, 0, st>>>(scratch, labels, B, margin, out_loss);
        QST_LAUNCH_CHECK();
        if (any_g) {
            a.mode = MODE_ONLINE_BWD; a.sel = scratch; a.row_out = nullptr;
            a.g[0] = grad_u; a.g[1] = grad_v;
            launch_rows<2>(a, st);
            QST_LAUNCH_CHECK();
        }
        return QST_OK;
    }
    a.mode = (kind == QST_PAIR_MSE) ? MODE_MSE : MODE_CONTRASTIVE;
    a.g[0] = grad_u; a.g[1] = grad_v;
    a.reduction = reduction;
    a.row_out = (reduction == QST_REDUCE_NONE) ? out_loss : scratch;
    launch_rows<2>(a, st);
    QST_LAUNCH_CHECK();
    if (reduction != QST_REDUCE_NONE) {
        row_sum_kernel<float><<<1, 1024, 0, st>>>(scratch, B, reduction == QST_REDUCE_MEAN ? 1.0f / (float)B : 1.0f, out_loss);
        QST_LAUNCH_CHECK();
    }
    return QST_OK;
}

extern "C" int qst_triplet_loss(const float* xa, const float* xp, const float* xn, int B, int D, int metric, float margin,
                                int reduction, float* out_loss, const float* grad_out,
                                float* grad_a, float* grad_p, float* grad_n, float* scratch, void* stream) {
    if (!xa || !xp || !xn || !out_loss || B <= 0 || D <= 0) return QST_ERR_BAD_ARG;
    if (reduction < QST_REDUCE_NONE || reduction > QST_REDUCE_MEAN) return QST_ERR_BAD_ARG;
    if (reduction != QST_REDUCE_NONE && !scratch) return QST_ERR_BAD_ARG;
    if (!distance_metric(metric) || !(margin >= 0.f)) return QST_ERR_BAD_ARG;
    float* g[3] = {grad_a, grad_p, grad_n};
    bool any_g;
    if (!grads_ok(g, 3, any_g)) return QST_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    TupleArgs a = {};
    a.x[0] = xa; a.x[1] = xp; a.x[2] = xn;
    a.g[0] = grad_a; a.g[1] = grad_p; a.g[2] = grad_n;
    a.grad_out = grad_out;
    a.row_out = (reduction == QST_REDUCE_NONE) ? out_loss : scratch;
    a.B = B; a.D = D; a.mode = MODE_TRIPLET; a.metric = metric; a.reduction = reduction; a.margin = margin;
    launch_rows<3>(a, st);
    QST_LAUNCH_CHECK();
    if (reduction != QST_REDUCE_NONE) {
        row_sum_kernel<float><<<1, 1024, 0, st>>>(scratch, B, reduction == QST_REDUCE_MEAN ? 1.0f / (float)B : 1.0f, out_loss);
        QST_LAUNCH_CHECK();
    }
    return QST_OK;
}

extern "C" int qst_quadruplet_eval(const float* xa, const float* xp, const float* xq, const float* xn, int B, int D,
                                   float* out_dist, int32_t* out_flags, int32_t* out_counts, void* stream) {
    if (!xa || !xp || !xq || !xn || !out_flags || !out_counts || B < 1 || D < 1) return QST_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    QuadEvalArgs a = {};
    a.x[0] = xa; a.x[1] = xp; a.x[2] = xq; a.x[3] = xn;
    a.dist = out_dist; a.flags = out_flags; a.B = B; a.D = D;
    const bool vec = D % 4 == 0 && al16(xa) && al16(xp) && al16(xq) && al16(xn);
    if (vec) quad_eval_kernel<true><<<row_grid(B), 256, 0, st>>>(a);
    else quad_eval_kernel<false><<<row_grid(B), 256, 0, st>>>(a);
    QST_LAUNCH_CHECK();
    // second stage: one workgroup over the flags, in stream order behind the first
    quad_count_kernel<<<1, 1024, 0, st>>>(out_flags, B, out_counts);
    QST_LAUNCH_CHECK();
    return QST_OK;
}
