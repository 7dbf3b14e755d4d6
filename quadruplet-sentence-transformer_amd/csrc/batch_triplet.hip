// batch_triplet.hip -- the batch-mining triplet losses of sentence-transformers 2.2.2 (BatchHardTripletLoss,
// BatchHardSoftMarginTripletLoss, BatchSemiHardTripletLoss, BatchAllTripletLoss), forward + backward in fp32.
//
// One embedding x [B, D] and one integer label per row. d [B, B] is the matrix of all distances of the batch; pos[i, j]
// means labels equal and i != j, neg[i, k] means labels differ. The triplets are mined on the device at every step:
//   hard   hp_i = max_j(pos * d), hn_i = min_k(d_ik + rowmax_i * (1 - neg)); mean_i relu(hp_i - hn_i + m)
//   soft   the same hp, hn; mean_i log1p(exp(hp_i - hn_i))
//   all    sum of relu(d_ij - d_ik + m) over pos[i, j] & neg[i, k], / (#{terms > 1e-16} + 1e-16)
//   semi   per positive pair (i, j): n_ij = the closest negative farther than d_ij, else the farthest negative, else the row
//          minimum; sum relu(d_ij - n_ij + m) / #pairs  (no pair at all: 0 / 0 = NaN, as upstream)
// Stages (all on the caller's stream, no host synchronisation, no atomics, every reduction in a fixed order):
//   1. rnorm    cos only: |x| and 1 / max(|x|, 1e-12) per row
//   2. dist     d [B, ldB] (ldB = B rounded up to 4) on the LDS-tiled loop of fp32_tile.h: 1 - <x_hat_i, x_hat_j>, or
//               sqrt(sum_k (x_ik - x_jk)^2) accumulated DIRECTLY -- the Gram form G_ii - 2 G_ij + G_jj cancels for close rows
//   3. mine     one workgroup per anchor i: the row's loss numerator and counts and, with gradients, row i of
//               W_ij = d(numerator) / d(d_ij). The O(B^2)-per-row kinds stage the row through LDS in chunks of kChunk.
//   4. finish   one workgroup: the fixed-order sums, the loss, the counts, 1 / denominator as a device scalar
//   5. sym      M = C + C^T, C = W / d (0 where d = 0) for euclid, W for cos
//   6. grad     euclid: grad_i = sum_j M_ij (x_i - x_j) / den   cos: d_hat_i = -sum_j M_ij x_hat_j / den   (one NN tile loop)
//   7. normbwd  cos only, in place: r * (d_hat - x_hat <x_hat, d_hat>), as mnrl.hip stage 7
// *grad_out multiplies the finished gradient (the epilogue of 6, or 7): the loss scale of use_amp never enters an
// intermediate, and a power of two scales the gradients exactly.
#include <climits>
#include "qst_common.h"

namespace {

#include "fp32_tile.h"

typedef unsigned long long u64;
constexpr float kNormEps = 1e-12f;      // F.normalize's eps
constexpr int kChunk = 1024;            // row entries staged through LDS at a time
constexpr float kInf = __builtin_inff();

// ---- workspace layout (floats; every segment starts on a multiple of 4, the workspace on 16 bytes)
struct BtWs {
    size_t rinv, nrm, rowterm, rowcnt, scal, d, W, M, total;
    int ld;
};
inline BtWs bt_layout(int B) {
    BtWs w;
    w.ld = (int)pad4((size_t)B);
    size_t o = 0;
    w.rinv = o; o += pad4((size_t)B);
    w.nrm = o; o += pad4((size_t)B);
    w.rowterm = o; o += pad4((size_t)B);
    w.rowcnt = o; o += 4 * (size_t)B;              // two 64-bit counts per row
    w.scal = o; o += 4;
    w.d = o; o += (size_t)B * w.ld;
    w.W = o; o += (size_t)B * w.ld;
    w.M = o; o += (size_t)B * w.ld;                // semi-hard keeps its selections here (int32) until stage 5 writes M
    w.total = o;
    return w;
}

// ---- fixed-order block reductions through LDS (blockDim.x a power of two)
// the extreme value and, among equal values, the smallest index
template <bool MAX>
__device__ __forceinline__ void block_arg(float& v, int& i, float* sv, int* si) {
    const int t = threadIdx.x;
    sv[t] = v; si[t] = i;
    __syncthreads();
    for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
        if (t < s) {
            const float ov = sv[t + s], mv = sv[t];
            const int oi = si[t + s];
            if ((MAX ? ov > mv : ov < mv) || (ov == mv && oi < si[t])) { sv[t] = ov; si[t] = oi; }
        }
        __syncthreads();
    }
    v = sv[0]; i = si[0];
    __syncthreads();
}
__device__ __forceinline__ u64 block_sum_u64(u64 v, u64* s) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int k = blockDim.x >> 1; k > 0; k >>= 1) {
        if (t < k) s[t] += s[t + k];
        __syncthreads();
    }
    const u64 r = s[0];
    __syncthreads();
    return r;
}

// ---- 1. row norms
template <bool VEC>
__global__ __launch_bounds__(256) void bt_rnorm_kernel(const float* xs, int B, int D, float* rinv, float* nrm) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const float* x = xs + (size_t)row * D;
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

// ---- 2. the distance matrix: both operands are rows of x
template <bool COS>
__global__ __launch_bounds__(256) void bt_dist_kernel(const float* x, int B, int D, int vec, const float* rinv, float* d,
                                                      int ld, int tiles_n) {
    __shared__ __attribute__((aligned(16))) float As[kBK][kLdT];
    __shared__ __attribute__((aligned(16))) float Bs[kBK][kLdT];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int m0 = (int)(blockIdx.x / tiles_n) * kTile, n0 = (int)(blockIdx.x % tiles_n) * kTile;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    float ra[4], rb[4];
    panel_load<true>(x, D, B, D, m0, 0, vec != 0, nullptr, ra);
    panel_load<true>(x, D, B, D, n0, 0, vec != 0, nullptr, rb);
    for (int k0 = 0; k0 < D; k0 += kBK) {
        panel_store<true>(As, ra);
        panel_store<true>(Bs, rb);
        __syncthreads();
        if (k0 + kBK < D) {             // the next panel travels while this one is used
            panel_load<true>(x, D, B, D, m0, k0 + kBK, vec != 0, nullptr, ra);
            panel_load<true>(x, D, B, D, n0, k0 + kBK, vec != 0, nullptr, rb);
        }
#pragma unroll
        for (int k = 0; k < kBK; ++k) {
            const f32x4 av = *(const f32x4*)&As[k][ty * 4];
            const f32x4 bv = *(const f32x4*)&Bs[k][tx * 4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (COS) {
                        acc[i][j] = __builtin_fmaf(av[i], bv[j], acc[i][j]);
                    } else {
                        const float df = av[i] - bv[j];
                        acc[i][j] = __builtin_fmaf(df, df, acc[i][j]);
                    }
                }
        }
        __syncthreads();
    }

    const int n = n0 + tx * 4;
    if (n >= B) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m >= B) break;
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (n + j >= B) v[j] = 0.f;                                     // the pad columns of the last group
            else if (COS) v[j] = 1.f - acc[i][j] * (rinv[m] * rinv[n + j]);
            else v[j] = sqrtf(acc[i][j]);                                   // bit-identical rows: exactly 0
        }
        *(f32x4*)(d + (size_t)m * ld + n) = v;                              // ld % 4 == 0: n + 3 < ld
    }
}

// ---- 3a. hard / soft margin: three arg-reductions per row, at most three non-zeros of W
__global__ __launch_bounds__(256) void bt_hard_kernel(const float* d, int ld, const int64_t* labels, int B, int soft,
                                                      float margin, float* rowterm, u64* rowcnt, float* W) {
    __shared__ float sv[256];
    __shared__ int si[256];
    const int i = blockIdx.x, t = threadIdx.x;
    const float* dr = d + (size_t)i * ld;
    const int64_t li = labels[i];
    float pv = -kInf, mv = -kInf;
    int pj = INT_MAX, mj = INT_MAX;
    for (int j = t; j < B; j += 256) {
        const float v = dr[j];
        if (v > mv) { mv = v; mj = j; }
        if (j != i && labels[j] == li && v > pv) { pv = v; pj = j; }
    }
    block_arg<true>(pv, pj, sv, si);
    block_arg<true>(mv, mj, sv, si);
    // max_j(pos * d): the zeros of the masked-out entries (the diagonal is one) take part, and carry no gradient
    const float hp = pv > 0.f ? pv : 0.f;
    if (!(pv > 0.f)) pj = -1;
    float nv = kInf;
    int nk = INT_MAX;
    for (int k = t; k < B; k += 256) {
        const float v = labels[k] != li ? dr[k] : dr[k] + mv;
        if (v < nv) { nv = v; nk = k; }
    }
    block_arg<false>(nv, nk, sv, si);
    const float xarg = hp - nv;
    float term, sig;
    if (soft) {
        term = xarg > 0.f ? xarg + log1pf(expf(-xarg)) : log1pf(expf(xarg));
        sig = 1.f / (1.f + expf(-xarg));
    } else {
        const float h = xarg + margin;
        term = h > 0.f ? h : 0.f;
        sig = h > 0.f ? 1.f : 0.f;
    }
    if (t == 0) {
        rowterm[i] = term;
        rowcnt[2 * (size_t)i] = 1;
        rowcnt[2 * (size_t)i + 1] = (soft || sig > 0.f) ? 1 : 0;
    }
    if (!W) return;
    float* wr = W + (size_t)i * ld;
    for (int j = t; j < B; j += 256) wr[j] = 0.f;
    __syncthreads();
    if (t == 0 && (unsigned)nk < (unsigned)B) {
        if (pj >= 0 && pj < B) wr[pj] += sig;
        if (nk != i) wr[nk] -= sig;
        // an anchor without any negative: the selected entry is d_ik + rowmax, and rowmax has a gradient of its own
        if (labels[nk] == li && (unsigned)mj < (unsigned)B && mj != i) wr[mj] -= sig;
    }
}

// ---- 3b. all triplets. Pass A: a thread owns a positive j and walks the negatives staged in LDS; with gradients pass B
// swaps the roles. Element j of the row of W is written by thread j % 256 in both passes.
__global__ __launch_bounds__(256) void bt_all_kernel(const float* d, int ld, const int64_t* labels, int B, float margin,
                                                     float* rowterm, u64* rowcnt, float* W) {
    __shared__ float sd[kChunk];
    __shared__ u64 su[256];
    __shared__ float part[4];
    const int i = blockIdx.x, t = threadIdx.x;
    const float* dr = d + (size_t)i * ld;
    float* wr = W ? W + (size_t)i * ld : nullptr;
    const int64_t li = labels[i];
    const int nq = (B + 255) / 256, nch = (B + kChunk - 1) / kChunk;
    float sum = 0.f;
    u64 n_act = 0, n_pos = 0, n_neg = 0;
    for (int pass = 0; pass < (wr ? 2 : 1); ++pass) {
        for (int q = 0; q < nq; ++q) {
            const int j = q * 256 + t;
            const bool same = j < B && labels[j] == li;
            const bool own = j < B && j != i && (pass == 0 ? same : !same);
            const float dj = own ? dr[j] : 0.f;
            if (pass == 0 && j < B && j != i) { if (same) ++n_pos; else ++n_neg; }
            unsigned cnt = 0;
            for (int c = 0; c < nch; ++c) {
                if (nch > 1 || q == 0) {
                    __syncthreads();
                    for (int e = t; e < kChunk; e += 256) {
                        const int k = c * kChunk + e;
                        // pass A stages the negatives (+inf elsewhere), pass B the positives (-inf elsewhere)
                        const bool oth = k < B && k != i && ((labels[k] == li) == (pass == 1));
                        sd[e] = oth ? dr[k] : (pass == 0 ? kInf : -kInf);
                    }
                    __syncthreads();
                }
                if (!own) continue;
                const int n = min(kChunk, B - c * kChunk);
                if (pass == 0) {
                    for (int e = 0; e < n; ++e) {
                        const float h = dj - sd[e] + margin;
                        if (h > 0.f) { sum += h; ++cnt; }
                        if (h > 1e-16f) ++n_act;
                    }
                } else {
                    for (int e = 0; e < n; ++e) if (sd[e] - dj + margin > 0.f) ++cnt;
                }
            }
            if (wr && j < B) {
                if (pass == 0) wr[j] = own ? (float)cnt : 0.f;
                else if (own) wr[j] = -(float)cnt;
            }
        }
    }
    sum = block_sum<4>(sum, part);
    n_act = block_sum_u64(n_act, su);
    n_pos = block_sum_u64(n_pos, su);
    n_neg = block_sum_u64(n_neg, su);
    if (t == 0) {
        rowterm[i] = sum;
        rowcnt[2 * (size_t)i] = n_pos * n_neg;
        rowcnt[2 * (size_t)i + 1] = n_act;
    }
}

// ---- 3c. semi-hard. Pass A: a thread owns a positive j, finds its negative among those staged in LDS and leaves the
// selection (the negative's index, -1 = no active pair) in sel[j]; with gradients pass B has thread k count the pairs that
// selected k.
__global__ __launch_bounds__(256) void bt_semi_kernel(const float* d, int ld, const int64_t* labels, int B, float margin,
                                                      float* rowterm, u64* rowcnt, float* W, int* sel_all) {
    __shared__ float sd[kChunk];
    __shared__ int ss[kChunk];
    __shared__ float sv[256];
    __shared__ int si[256];
    __shared__ u64 su[256];
    __shared__ float part[4];
    const int i = blockIdx.x, t = threadIdx.x;
    const float* dr = d + (size_t)i * ld;
    const int64_t li = labels[i];
    const int nq = (B + 255) / 256, nch = (B + kChunk - 1) / kChunk;
    // what a pair falls back on: the farthest negative, or without any negative the row minimum
    float xv = -kInf, nv = kInf;
    int xk = INT_MAX, nk = INT_MAX;
    for (int k = t; k < B; k += 256) {
        const float v = dr[k];
        if (labels[k] != li && v > xv) { xv = v; xk = k; }
        if (v < nv) { nv = v; nk = k; }
    }
    block_arg<true>(xv, xk, sv, si);
    block_arg<false>(nv, nk, sv, si);
    const bool has_neg = xk != INT_MAX;
    const float fb_v = has_neg ? xv : nv;
    const int fb_k = has_neg ? xk : nk;

    int* sel = (W && sel_all) ? sel_all + (size_t)i * ld : nullptr;
    float sum = 0.f;
    u64 n_act = 0, n_pair = 0;
    for (int q = 0; q < nq; ++q) {
        const int j = q * 256 + t;
        const bool own = j < B && j != i && labels[j] == li;
        const float dj = own ? dr[j] : 0.f;
        float best = kInf;
        int bk = -1;
        for (int c = 0; c < nch; ++c) {
            if (nch > 1 || q == 0) {
                __syncthreads();
                for (int e = t; e < kChunk; e += 256) {
                    const int k = c * kChunk + e;
                    sd[e] = (k < B && labels[k] != li) ? dr[k] : kInf;
                }
                __syncthreads();
            }
            if (!own) continue;
            const int n = min(kChunk, B - c * kChunk);
            for (int e = 0; e < n; ++e) {
                const float v = sd[e];
                if (v > dj && v < best) { best = v; bk = c * kChunk + e; }
            }
        }
        int chosen = -1;
        if (own) {
            ++n_pair;
            if (bk < 0) { best = fb_v; bk = fb_k; }
            const float h = dj - best + margin;
            if (h > 0.f) { sum += h; ++n_act; chosen = bk; }
        }
        if (sel && j < B) sel[j] = chosen;
    }
    sum = block_sum<4>(sum, part);
    n_act = block_sum_u64(n_act, su);
    n_pair = block_sum_u64(n_pair, su);
    if (t == 0) {
        rowterm[i] = sum;
        rowcnt[2 * (size_t)i] = n_pair;
        rowcnt[2 * (size_t)i + 1] = n_act;
    }
    if (!sel) return;
    float* wr = W + (size_t)i * ld;
    for (int q = 0; q < nq; ++q) {
        const int k = q * 256 + t;
        int cnt = 0;
        for (int c = 0; c < nch; ++c) {
            if (nch > 1 || q == 0) {
                __syncthreads();                    // also orders pass A's writes of sel before these reads
                for (int e = t; e < kChunk; e += 256) {
                    const int j = c * kChunk + e;
                    ss[e] = j < B ? sel[j] : -1;
                }
                __syncthreads();
            }
            if (k >= B) continue;
            const int n = min(kChunk, B - c * kChunk);
            for (int e = 0; e < n; ++e) cnt += ss[e] == k ? 1 : 0;
        }
        // +1 for the active pair (i, k), -1 per pair that selected k; the diagonal (selected only by an anchor without
        // negatives) has no gradient
        if (k < B) wr[k] = k == i ? 0.f : (float)((sel[k] >= 0 ? 1 : 0) - cnt);
    }
}

// ---- 4. the loss, the counts and 1 / denominator
__global__ __launch_bounds__(1024) void bt_finish_kernel(const float* rowterm, const u64* rowcnt, int B, int kind,
                                                         float* out_loss, int64_t* out_counts, float* scal) {
    __shared__ float part[16];
    __shared__ u64 su[1024];
    float s = 0.f;
    u64 c0 = 0, c1 = 0;
    for (int i = threadIdx.x; i < B; i += 1024) {
        s += rowterm[i];
        c0 += rowcnt[2 * (size_t)i];
        c1 += rowcnt[2 * (size_t)i + 1];
    }
    s = block_sum<16>(s, part);
    c0 = block_sum_u64(c0, su);
    c1 = block_sum_u64(c1, su);
    if (threadIdx.x == 0) {
        const float den = kind == QST_BT_ALL ? (float)c1 + 1e-16f : (float)c0;
        out_loss[0] = s / den;
        scal[0] = 1.f / den;
        if (out_counts) { out_counts[0] = (int64_t)c0; out_counts[1] = (int64_t)c1; }
    }
}

// ---- 5. M = C + C^T in 64 x 64 tiles, the transposed tile through LDS
template <bool EUCLID>
__device__ __forceinline__ float coef_of(const float* W, const float* d, size_t idx) {
    const float w = W[idx];
    if (!EUCLID) return w;
    const float dd = d[idx];
    return (w != 0.f && dd > 0.f) ? w / dd : 0.f;   // the gradient through an exactly-zero distance is 0
}
template <bool EUCLID>
__global__ __launch_bounds__(256) void bt_sym_kernel(const float* W, const float* d, int ld, int B, float* M, int tiles) {
    __shared__ float T[kTile][kTile + 1];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int i0 = (int)(blockIdx.x / tiles) * kTile, j0 = (int)(blockIdx.x % tiles) * kTile;
    for (int r = ty; r < kTile; r += 4) {
        const int jj = j0 + r, ii = i0 + tx;
        T[r][tx] = (jj < B && ii < B) ? coef_of<EUCLID>(W, d, (size_t)jj * ld + ii) : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < kTile; r += 4) {
        const int ii = i0 + r, jj = j0 + tx;
        if (ii < B && jj < B) {
            const size_t idx = (size_t)ii * ld + jj;
            M[idx] = coef_of<EUCLID>(W, d, idx) + T[tx][r];
        }
    }
}

// ---- 6. G [B, D]: euclid sum_k M[m, k] (x[m, n] - x[k, n]) / den * g; cos -sum_k M[m, k] x_hat[k, n] / den
template <bool COS>
__global__ __launch_bounds__(256) void bt_grad_kernel(const float* M, int ld, const float* x, int B, int D, int vecM, int vecX,
                                                      int vecG, const float* rinv, const float* scal, const float* gout,
                                                      float* G, int tiles_n) {
    __shared__ __attribute__((aligned(16))) float As[kBK][kLdT];
    __shared__ __attribute__((aligned(16))) float Bs[kBK][kLdT];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int m0 = (int)(blockIdx.x / tiles_n) * kTile, n0 = (int)(blockIdx.x % tiles_n) * kTile;
    float acc[4][4], xm[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[i][j] = 0.f;
            const int m = m0 + ty * 4 + i, n = n0 + tx * 4 + j;
            xm[i][j] = (!COS && m < B && n < D) ? x[(size_t)m * D + n] : 0.f;
        }

    const float* ks = COS ? rinv : nullptr;
    float ra[4], rb[4];
    panel_load<true>(M, ld, B, B, m0, 0, vecM != 0, nullptr, ra);
    panel_load<false>(x, D, D, B, n0, 0, vecX != 0, ks, rb);
    for (int k0 = 0; k0 < B; k0 += kBK) {
        panel_store<true>(As, ra);
        panel_store<false>(Bs, rb);
        __syncthreads();
        if (k0 + kBK < B) {
            panel_load<true>(M, ld, B, B, m0, k0 + kBK, vecM != 0, nullptr, ra);
            panel_load<false>(x, D, D, B, n0, k0 + kBK, vecX != 0, ks, rb);
        }
#pragma unroll
        for (int k = 0; k < kBK; ++k) {
            const f32x4 av = *(const f32x4*)&As[k][ty * 4];
            const f32x4 bv = *(const f32x4*)&Bs[k][tx * 4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_fmaf(av[i], COS ? bv[j] : xm[i][j] - bv[j], acc[i][j]);   // a pad k has av = 0
        }
        __syncthreads();
    }

    const float inv = scal[0];
    const float g = (!COS && gout) ? gout[0] : 1.f;         // cos: stage 7 applies it
    const int n = n0 + tx * 4;
    if (n >= D) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m >= B) break;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float y = acc[i][j] * inv;                 // the value without grad_out, then times g
            v[j] = COS ? -y : y * g;
        }
        float* q = G + (size_t)m * D + n;
        if (vecG && n + 3 < D) *(f32x4*)q = f32x4{v[0], v[1], v[2], v[3]};
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (n + j < D) q[j] = v[j];
        }
    }
}

// ---- 7. backward of F.normalize, in place on the rows of G (which hold d_hat), times *grad_out
__global__ __launch_bounds__(256) void bt_normbwd_kernel(const float* xs, float* G, int B, int D, const float* rinv,
                                                         const float* nrm, const float* gout) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const float* x = xs + (size_t)row * D;
    float* d = G + (size_t)row * D;
    const float r = rinv[row];
    const bool clamped = nrm[row] < kNormEps;       // clamp_min passes no gradient to the norm: d_hat / eps
    const float g = gout ? gout[0] : 1.f;
    float dot = 0.f;
    for (int i = lane; i < D; i += 64) dot = __builtin_fmaf(x[i] * r, d[i], dot);
    dot = wave_sum(dot);
    for (int i = lane; i < D; i += 64) {            // each element is read and then written by the same lane
        const float tt = clamped ? d[i] : __builtin_fmaf(-(x[i] * r), dot, d[i]);
        const float y = r * tt;
        d[i] = y * g;
    }
}

}  // namespace

extern "C" size_t qst_batch_triplet_workspace_bytes(int B, int D) {
    if (B < 1 || D < 1) return 0;
    return bt_layout(B).total * sizeof(float);
}

extern "C" int qst_batch_triplet_loss(const float* x, const int64_t* labels, int B, int D, int kind, int metric, float margin,
                                      float* out_loss, int64_t* out_counts, const float* grad_out, float* grad_x,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 1 || D < 1 || !x || !labels || !out_loss || !workspace) return QST_ERR_BAD_ARG;
    if (kind < QST_BT_HARD || kind > QST_BT_ALL) return QST_ERR_BAD_ARG;
    if (metric != QST_METRIC_L2_PLAIN && metric != QST_METRIC_COS_DIST) return QST_ERR_BAD_ARG;
    if (!(margin >= 0.f) || !(margin < __builtin_inff())) return QST_ERR_BAD_ARG;    // NaN fails the first comparison
    if (((uintptr_t)workspace & 15) != 0) return QST_ERR_BAD_ARG;
    const BtWs L = bt_layout(B);
    if (workspace_bytes < L.total * sizeof(float)) return QST_ERR_BAD_ARG;
    // the kernels index in 64 bits; rows and tiles are counted in 32
    if ((int64_t)B * L.ld > 0x7FFFFFFFLL || (int64_t)B * D > 0x7FFFFFFFLL) return QST_ERR_UNSUPPORTED;

    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    float* rinv = ws + L.rinv;
    float* nrm = ws + L.nrm;
    float* rowterm = ws + L.rowterm;
    u64* rowcnt = (u64*)(ws + L.rowcnt);
    float* scal = ws + L.scal;
    float* d = ws + L.d;
    float* W = grad_x ? ws + L.W : nullptr;
    float* M = ws + L.M;
    const bool cos = metric == QST_METRIC_COS_DIST;
    const bool vec_x = (D % 4 == 0) && al16(x);
    const unsigned row_grid = (unsigned)(((int64_t)B + 3) / 4);
    const int tb = (B + kTile - 1) / kTile, td = (D + kTile - 1) / kTile;
    if ((int64_t)tb * tb > 0x7FFFFFFFLL || (int64_t)tb * td > 0x7FFFFFFFLL) return QST_ERR_UNSUPPORTED;

    if (cos) {
        if (vec_x) bt_rnorm_kernel<true><<<row_grid, 256, 0, st>>>(x, B, D, rinv, nrm);
        else bt_rnorm_kernel<false><<<row_grid, 256, 0, st>>>(x, B, D, rinv, nrm);
        QST_LAUNCH_CHECK();
        bt_dist_kernel<true><<<(unsigned)(tb * tb), 256, 0, st>>>(x, B, D, vec_x, rinv, d, L.ld, tb);
    } else {
        bt_dist_kernel<false><<<(unsigned)(tb * tb), 256, 0, st>>>(x, B, D, vec_x, rinv, d, L.ld, tb);
    }
    QST_LAUNCH_CHECK();

    if (kind == QST_BT_HARD || kind == QST_BT_HARD_SOFT)
        bt_hard_kernel<<<(unsigned)B, 256, 0, st>>>(d, L.ld, labels, B, kind == QST_BT_HARD_SOFT, margin, rowterm, rowcnt, W);
    else if (kind == QST_BT_ALL)
        bt_all_kernel<<<(unsigned)B, 256, 0, st>>>(d, L.ld, labels, B, margin, rowterm, rowcnt, W);
    else
        bt_semi_kernel<<<(unsigned)B, 256, 0, st>>>(d, L.ld, labels, B, margin, rowterm, rowcnt, W, (int*)M);
    QST_LAUNCH_CHECK();
    bt_finish_kernel<<<1, 1024, 0, st>>>(rowterm, rowcnt, B, kind, out_loss, out_counts, scal);
    QST_LAUNCH_CHECK();
    if (!grad_x) return QST_OK;

    if (cos) bt_sym_kernel<false><<<(unsigned)(tb * tb), 256, 0, st>>>(W, d, L.ld, B, M, tb);
    else bt_sym_kernel<true><<<(unsigned)(tb * tb), 256, 0, st>>>(W, d, L.ld, B, M, tb);
    QST_LAUNCH_CHECK();
    const int vecG = (D % 4 == 0) && al16(grad_x);
    if (cos) bt_grad_kernel<true><<<(unsigned)(tb * td), 256, 0, st>>>(M, L.ld, x, B, D, 1, vec_x, vecG, rinv, scal, grad_out, grad_x, td);
    else bt_grad_kernel<false><<<(unsigned)(tb * td), 256, 0, st>>>(M, L.ld, x, B, D, 1, vec_x, vecG, rinv, scal, grad_out, grad_x, td);
    QST_LAUNCH_CHECK();
    if (cos) {
        bt_normbwd_kernel<<<row_grid, 256, 0, st>>>(x, grad_x, B, D, rinv, nrm, grad_out);
        QST_LAUNCH_CHECK();
    }
    return QST_OK;
}
