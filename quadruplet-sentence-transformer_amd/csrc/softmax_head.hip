// softmax_head.hip -- the classifier of sentence-transformers 2.2.2's losses.SoftmaxLoss on a pair of sentence embeddings:
//
//   qst_softmax_head_fwd  logits = [u, v, |u - v|, u * v] W^T + b   (the parts a bit mask selects, in that order)
//   qst_softmax_ce        nn.CrossEntropyLoss(weight=None, label_smoothing=0) on [B, C] logits, its dlogits and the counts
//                         evaluation.LabelAccuracyEvaluator reads
//   qst_softmax_head_bwd  dlogits -> grad_u, grad_v, grad_W, grad_b
//
// All fp32, no atomics, every sum in a fixed order: the same inputs give the same bits. The feature vector [B, K] is never
// built: a wave keeps its row of u and of v in registers (16 bytes a lane, the register form of row_loss.h: D <= 2048,
// D % 4 == 0) and forms |u - v| and u * v where it needs them. C <= 8: the C dot products of a row finish with C wave
// reductions, and the weight gradient runs one class per workgroup row.
#include "row_loss.h"

namespace {

constexpr int kMaxClasses = 8;
constexpr int kWgradRows = 64;      // rows one slice of the weight gradient walks before another slice takes over ...
constexpr int kWgradSlices = 32;    // ... up to this many slices; past it the slices grow instead

inline int part_count(int parts) {
    return ((parts & QST_SOFTMAX_REP) ? 2 : 0) + ((parts & QST_SOFTMAX_DIFF) ? 1 : 0) + ((parts & QST_SOFTMAX_MULT) ? 1 : 0);
}
inline int wgrad_slices(int B) {
    const int s = (B + kWgradRows - 1) / kWgradRows;
    return s < kWgradSlices ? s : kWgradSlices;
}

__device__ __forceinline__ float sign0(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }   // torch's abs': sign(0) = 0

// ---- qst_softmax_head_fwd
struct HeadArgs {
    const float* u;
    const float* v;
    const float* w;                 // [C, K], K = (number of parts) * D
    const float* b;                 // [C]
    const float* dlogits;           // [B, C] (backward)
    float* logits;                  // [B, C] (forward)
    float* gu;
    float* gv;
    int B, D, C, parts;
};

// the row of u and of v of this wave, NV float4 per lane; past the row zeros, which add nothing anywhere
template <int NV>
__device__ __forceinline__ void load_rows(const HeadArgs& a, int64_t row, int lane, f32x4 (&U)[NV], f32x4 (&V)[NV]) {
    const size_t base = row_base(row, a.D);
    const int nv = a.D >> 2;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int q = lane + i * 64;
        U[i] = f32x4{0, 0, 0, 0}; V[i] = f32x4{0, 0, 0, 0};
        if (q < nv) { U[i] = *(const f32x4*)(a.u + base + q * 4); V[i] = *(const f32x4*)(a.v + base + q * 4); }
    }
}

template <int NV>
__global__ __launch_bounds__(256) void head_fwd_kernel(HeadArgs a) {
    const int lane = threadIdx.x & 63;
    int64_t row;
    if (!wave_row(a.B, row)) return;
    const int D = a.D, nv = D >> 2;
    f32x4 U[NV], V[NV];
    load_rows<NV>(a, row, lane, U, V);
    const bool rep = a.parts & QST_SOFTMAX_REP, dif = a.parts & QST_SOFTMAX_DIFF, mul = a.parts & QST_SOFTMAX_MULT;
    const int K = (2 * rep + dif + mul) * D;
    const int o_v = D, o_d = rep ? 2 * D : 0, o_m = o_d + (dif ? D : 0);      // where each part starts in a row of W
    for (int c = 0; c < a.C; ++c) {
        const float* w = a.w + (size_t)c * K;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int q = lane + i * 64;
            if (q < nv) {
                if (rep) {
                    const f32x4 Wu = *(const f32x4*)(w + q * 4), Wv = *(const f32x4*)(w + o_v + q * 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) s += U[i][j] * Wu[j] + V[i][j] * Wv[j];
                }
                if (dif) {
                    const f32x4 Wd = *(const f32x4*)(w + o_d + q * 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) s += fabsf(U[i][j] - V[i][j]) * Wd[j];
                }
                if (mul) {
                    const f32x4 Wm = *(const f32x4*)(w + o_m + q * 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) s += (U[i][j] * V[i][j]) * Wm[j];
                }
            }
        }
        s = wave_sum(s);
        if (lane == 0) a.logits[row * a.C + c] = s + a.b[c];
    }
}

// ---- qst_softmax_head_bwd, the embeddings: d/du = sum_c dl_c (Wu_c + sign(u - v) Wd_c + v Wm_c), d/dv likewise
template <int NV>
__global__ __launch_bounds__(256) void head_bwd_rows_kernel(HeadArgs a) {
    const int lane = threadIdx.x & 63;
    int64_t row;
    if (!wave_row(a.B, row)) return;
    const int D = a.D, nv = D >> 2;
    f32x4 U[NV], V[NV], GU[NV], GV[NV];
    load_rows<NV>(a, row, lane, U, V);
#pragma unroll
    for (int i = 0; i < NV; ++i) { GU[i] = f32x4{0, 0, 0, 0}; GV[i] = f32x4{0, 0, 0, 0}; }
    const bool rep = a.parts & QST_SOFTMAX_REP, dif = a.parts & QST_SOFTMAX_DIFF, mul = a.parts & QST_SOFTMAX_MULT;
    const int K = (2 * rep + dif + mul) * D;
    const int o_v = D, o_d = rep ? 2 * D : 0, o_m = o_d + (dif ? D : 0);
    for (int c = 0; c < a.C; ++c) {                                            // classes in order: a fixed sum
        const float* w = a.w + (size_t)c * K;
        const float dl = a.dlogits[row * a.C + c];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int q = lane + i * 64;
            if (q < nv) {
                if (rep) {
                    const f32x4 Wu = *(const f32x4*)(w + q * 4), Wv = *(const f32x4*)(w + o_v + q * 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { GU[i][j] += dl * Wu[j]; GV[i][j] += dl * Wv[j]; }
                }
                if (dif) {
                    const f32x4 Wd = *(const f32x4*)(w + o_d + q * 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float t = dl * (sign0(U[i][j] - V[i][j]) * Wd[j]);
                        GU[i][j] += t; GV[i][j] -= t;
                    }
                }
                if (mul) {
                    const f32x4 Wm = *(const f32x4*)(w + o_m + q * 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { GU[i][j] += dl * (V[i][j] * Wm[j]); GV[i][j] += dl * (U[i][j] * Wm[j]); }
                }
            }
        }
    }
    const size_t base = row_base(row, D);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int q = lane + i * 64;
        if (q < nv) { *(f32x4*)(a.gu + base + q * 4) = GU[i]; *(f32x4*)(a.gv + base + q * 4) = GV[i]; }
    }
}

// ---- qst_softmax_head_bwd, the classifier: grad_W[c, part, d] = sum_b dl[b, c] * part(u, v)[b, d], grad_b[c] = sum_b dl[b, c].
// grid (ceil(D / 4 / 64), C, slices). A thread owns 4 columns d of every part for one class and walks the rows of its slice
// in order; the thread of column 0 also sums the bias gradient. One slice writes the results, more write partial sums
// [slice][C][K + 4] (the bias gradient behind the row, the row padded to 16 bytes) that wgrad_combine_kernel adds in order.
struct WgradArgs {
    const float* u;
    const float* v;
    const float* dlogits;
    float* gw;                      // [C, K] or the partial sums
    float* gb;                      // [C], or null: behind each partial row
    int B, D, C, parts, rows_per_slice, ld;     // ld: stride of an output row (K, or K + 4 for partial sums)
};

__global__ __launch_bounds__(64) void head_wgrad_kernel(WgradArgs a) {
    const int q = blockIdx.x * 64 + threadIdx.x;        // float4 column
    const int c = blockIdx.y, slice = blockIdx.z;
    const int D = a.D;
    if (q >= (D >> 2)) return;
    const int r0 = slice * a.rows_per_slice;
    const int r1 = min(a.B, r0 + a.rows_per_slice);
    const bool rep = a.parts & QST_SOFTMAX_REP, dif = a.parts & QST_SOFTMAX_DIFF, mul = a.parts & QST_SOFTMAX_MULT;
    f32x4 su = {0, 0, 0, 0}, sv = {0, 0, 0, 0}, sd = {0, 0, 0, 0}, sm = {0, 0, 0, 0};
    float sb = 0.f;
    for (int r = r0; r < r1; ++r) {
        const float dl = a.dlogits[(size_t)r * a.C + c];
        const f32x4 U = *(const f32x4*)(a.u + (size_t)r * D + q * 4), V = *(const f32x4*)(a.v + (size_t)r * D + q * 4);
        sb += dl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            su[j] += dl * U[j]; sv[j] += dl * V[j];
            sd[j] += dl * fabsf(U[j] - V[j]);
            sm[j] += dl * (U[j] * V[j]);
        }
    }
    const int o_d = rep ? 2 * D : 0, o_m = o_d + (dif ? D : 0);
    float* out = a.gw + ((size_t)slice * a.C + c) * a.ld;
    if (rep) { *(f32x4*)(out + q * 4) = su; *(f32x4*)(out + D + q * 4) = sv; }
    if (dif) *(f32x4*)(out + o_d + q * 4) = sd;
    if (mul) *(f32x4*)(out + o_m + q * 4) = sm;
    if (q == 0) {
        if (a.gb) a.gb[c] = sb;
        else out[a.ld - 4] = sb;
    }
}

// element e of [C][K + 4] (the bias gradient at column K): the slices' partial sums added in the order of the slices
__global__ __launch_bounds__(256) void wgrad_combine_kernel(const float* part, int slices, int C, int K, float* gw, float* gb) {
    const int ld = K + 4;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)C * ld) return;
    const int c = (int)(e / ld), k = (int)(e % ld);
    if (k > K) return;                                  // the padding behind the bias gradient
    float s = 0.f;
    for (int i = 0; i < slices; ++i) s += part[(size_t)i * C * ld + e];
    if (k < K) gw[(size_t)c * K + k] = s;
    else gb[c] = s;
}

// ---- qst_softmax_ce
struct CeArgs {
    const float* logits;
    const int64_t* labels;
    const float* grad_out;          // [B] (reduction none) or [1]; null = ones
    float* row_out;                 // [B]
    float* dlogits;                 // [B, C] or null
    int64_t* counts;                // {rows with a label in range, rows whose argmax is the label} or null
    int64_t* kept;                  // device scalar: rows whose label is not ignore_index (the mean's denominator)
    int64_t ignore_index;
    int B, C, reduction;
};

// one workgroup: integer sums, any order gives the same result
__global__ __launch_bounds__(1024) void ce_count_kernel(CeArgs a) {
    __shared__ int64_t red[3][16];
    int64_t n_kept = 0, n_valid = 0, n_hit = 0;
    for (int64_t r = threadIdx.x; r < a.B; r += 1024) {
        const int64_t y = a.labels[r];
        n_kept += y != a.ignore_index;
        if (y >= 0 && y < a.C && y != a.ignore_index) {
            ++n_valid;
            if (a.counts) {
                const float* z = a.logits + r * a.C;
                int best = 0;
                float zb = z[0];
                for (int c = 1; c < a.C; ++c)
                    if (z[c] > zb) { zb = z[c]; best = c; }        // a tie stays with the lowest index
                n_hit += best == y;
            }
        }
    }
    // 53 bits hold any count of rows: the wave tree of the double sums is exact
    const double k = wave_sum_f64((double)n_kept), v = wave_sum_f64((double)n_valid), h = wave_sum_f64((double)n_hit);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = (int64_t)k; red[1][threadIdx.x >> 6] = (int64_t)v; red[2][threadIdx.x >> 6] = (int64_t)h;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t t[3] = {0, 0, 0};
        for (int i = 0; i < 16; ++i) { t[0] += red[0][i]; t[1] += red[1][i]; t[2] += red[2][i]; }
        a.kept[0] = t[0];
        if (a.counts) { a.counts[0] = t[1]; a.counts[1] = t[2]; }
    }
}

// a thread per row: loss = logsumexp(z) - z[y]. y == ignore_index: 0 and zero gradients. Any other y outside [0, C): NaN and
// NaN gradients; y is only ever compared with c, never an index. Under 'mean' a row's value is divided by the number of kept
// rows here (in double, rounded once), so that the second stage is the shared sum; no kept row at all: 0 / 0 = NaN, as torch.
__global__ __launch_bounds__(256) void ce_rows_kernel(CeArgs a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.B) return;
    const int C = a.C;
    const float* z = a.logits + r * C;
    const int64_t y = a.labels[r];
    const bool ignored = y == a.ignore_index;
    const bool bad = !ignored && (y < 0 || y >= C);
    float m = z[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
    float s = 0.f, zy = 0.f;
    for (int c = 0; c < C; ++c) {
        s += expf(z[c] - m);
        if (c == y) zy = z[c];
    }
    const float lse = m + logf(s);
    const float nan = __builtin_nanf("");
    float loss = ignored ? 0.f : (bad ? nan : lse - zy);
    const bool mean = a.reduction == QST_REDUCE_MEAN;
    const double kept = mean ? (double)a.kept[0] : 1.0;
    if (mean) loss = (float)((double)loss / kept);
    a.row_out[r] = loss;
    if (a.dlogits == nullptr) return;
    float up = 1.f;
    if (a.grad_out) up = (a.reduction == QST_REDUCE_NONE) ? a.grad_out[r] : a.grad_out[0];
    const float k = mean ? (float)(1.0 / kept) : 1.f;
    float* d = a.dlogits + r * C;
    for (int c = 0; c < C; ++c) {
        const float p = expf(z[c] - lse) - (c == y ? 1.f : 0.f);
        d[c] = ignored ? 0.f : (bad ? nan : (p * k) * up);
    }
}

template <class F>
void dispatch_nv(int D, F fn) {
    dispatch_form<false>(D, true, [&](auto nv, auto) {
        if constexpr (decltype(nv)::value > 0) fn(nv);
    });
}

int head_check(const float* u, const float* v, const float* w, int B, int D, int C, int parts) {
    if (!u || !v || !w || B < 1 || D < 1 || C < 1 || parts <= 0 || parts > 7) return QST_ERR_BAD_ARG;
    if (!al16(u) || !al16(v) || !al16(w)) return QST_ERR_BAD_ARG;
    if (C > kMaxClasses || (D & 3) || D > 256 * kMaxRowVec) return QST_ERR_UNSUPPORTED;
    return QST_OK;
}

}  // namespace

extern "C" int qst_softmax_head_fwd(const float* u, const float* v, const float* w, const float* b, int B, int D, int C,
                                    int parts, float* logits, void* stream) {
    const int rc = head_check(u, v, w, B, D, C, parts);
    if (rc != QST_OK) return rc;
    if (!b || !logits) return QST_ERR_BAD_ARG;
    HeadArgs a = {};
    a.u = u; a.v = v; a.w = w; a.b = b; a.logits = logits; a.B = B; a.D = D; a.C = C; a.parts = parts;
    dispatch_nv(D, [&](auto nv) { head_fwd_kernel<decltype(nv)::value><<<row_grid(B), 256, 0, (hipStream_t)stream>>>(a); });
    QST_LAUNCH_CHECK();
    return QST_OK;
}

extern "C" size_t qst_softmax_head_bwd_workspace_bytes(int B, int D, int C, int parts) {
    if (B < 1 || D < 1 || C < 1 || parts <= 0 || parts > 7) return 0;
    const int s = wgrad_slices(B);
    return s <= 1 ? 0 : (size_t)s * C * ((size_t)part_count(parts) * D + 4) * sizeof(float);
}

extern "C" int qst_softmax_head_bwd(const float* u, const float* v, const float* w, const float* dlogits, int B, int D, int C,
                                    int parts, float* grad_u, float* grad_v, float* grad_w, float* grad_b, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    const int rc = head_check(u, v, w, B, D, C, parts);
    if (rc != QST_OK) return rc;
    if (!dlogits || !grad_u || !grad_v || !grad_w || !grad_b || !al16(grad_u) || !al16(grad_v) || !al16(grad_w))
        return QST_ERR_BAD_ARG;
    const size_t need = qst_softmax_head_bwd_workspace_bytes(B, D, C, parts);
    if (need && (!workspace || workspace_bytes < need || !al16(workspace))) return QST_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    HeadArgs a = {};
    a.u = u; a.v = v; a.w = w; a.dlogits = dlogits; a.gu = grad_u; a.gv = grad_v; a.B = B; a.D = D; a.C = C; a.parts = parts;
    dispatch_nv(D, [&](auto nv) { head_bwd_rows_kernel<decltype(nv)::value><<<row_grid(B), 256, 0, st>>>(a); });
    QST_LAUNCH_CHECK();

    const int slices = wgrad_slices(B), K = part_count(parts) * D;
    WgradArgs g = {};
    g.u = u; g.v = v; g.dlogits = dlogits; g.B = B; g.D = D; g.C = C; g.parts = parts;
    g.rows_per_slice = (B + slices - 1) / slices;
    if (slices == 1) { g.gw = grad_w; g.gb = grad_b; g.ld = K; }
    else { g.gw = (float*)workspace; g.gb = nullptr; g.ld = K + 4; }
    head_wgrad_kernel<<<dim3(((D >> 2) + 63) / 64, C, slices), 64, 0, st>>>(g);
    QST_LAUNCH_CHECK();
    if (slices > 1) {
        const int64_t n = (int64_t)C * (K + 4);
        wgrad_combine_kernel<<<(int)((n + 255) / 256), 256, 0, st>>>((const float*)workspace, slices, C, K, grad_w, grad_b);
        QST_LAUNCH_CHECK();
    }
    return QST_OK;
}

extern "C" int qst_softmax_ce(const float* logits, const int64_t* labels, int B, int C, int64_t ignore_index, int reduction,
                              float* out_loss, const float* grad_out, float* dlogits, int64_t* counts, float* scratch,
                              void* stream) {
    if (!logits || !labels || !out_loss || !scratch || B < 1 || C < 1) return QST_ERR_BAD_ARG;
    if (reduction < QST_REDUCE_NONE || reduction > QST_REDUCE_MEAN) return QST_ERR_BAD_ARG;
    if ((uintptr_t)scratch & 7) return QST_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    CeArgs a = {};
    a.logits = logits; a.labels = labels; a.grad_out = grad_out; a.dlogits = dlogits; a.counts = counts;
    a.kept = (int64_t*)scratch;                         // scratch: the mean's denominator, then the per-row values
    a.row_out = (reduction == QST_REDUCE_NONE) ? out_loss : scratch + 2;
    a.ignore_index = ignore_index; a.B = B; a.C = C; a.reduction = reduction;
    if (counts || reduction == QST_REDUCE_MEAN) {
        ce_count_kernel<<<1, 1024, 0, st>>>(a);
        QST_LAUNCH_CHECK();
    }
    ce_rows_kernel<<<(int)(((int64_t)B + 255) / 256), 256, 0, st>>>(a);
    QST_LAUNCH_CHECK();
    if (reduction != QST_REDUCE_NONE) {
        row_sum_kernel<double><<<1, 1024, 0, st>>>(scratch + 2, B, 1.0, out_loss);
        QST_LAUNCH_CHECK();
    }
    return QST_OK;
}
