// mnrl_nested.hip -- MultipleNegativesRankingLoss (plain and symmetric) at K nested prefixes of the embedding in one call:
// the arithmetic of MatryoshkaLoss(MultipleNegativesRankingLoss), forward + backward in fp32.
//
//   x_hat_k = F.normalize(x[:, :d_k], eps = 1e-12);  S_k = scale * a_hat_k c_hat_k^T;  term_k = the MNRL cross entropy of S_k
//   loss = sum_k w_k term_k;  grad_a, grad_c: full width, through truncation and normalisation, zero from max_k d_k on
//
// Scheme: the widths are sorted on the host; segment s is the columns [d_(s-1), d_s) between two consecutive boundaries.
// Neither the number of launches nor the number of passes over a and c grows with K:
//   1. rnorm    one wave per row of a and c walks the row once and emits |x[:d_s]| and 1 / max(., 1e-12) at every boundary
//   2. scores   ONE NT product over the columns in ascending order (fp32_tile.h); at the end of every segment the running
//               accumulator, times scale * r_a,s[i] * r_c,s[j], is stored as S_s and goes on accumulating. Panels start at
//               the segment's first column and are guarded at its last, so a boundary never falls inside a panel
//   3. colstat  symmetric only: mnrl.hip's column statistics with s as the second grid dimension
//   4. row      grid (B, K): max, sum of exponentials, the row's loss term; with gradients G_s (beside S_s, which stays) and
//               t_a,s[i] = sum_j G_s[i, j] S_s[i, j], which is <a_hat_s[i], d_hat_a,s[i]> without touching D
//   5. loss     one workgroup: every term in a fixed tree, out_terms in the caller's order, out_loss = sum_k w_k term_k
//               summed in the caller's order
//   6. colpass  64 columns per workgroup: t_c,s[j] = sum_i G_s[i, j] S_s[i, j], and G_s is replaced in place by
//               H_s[i, j] = sum_{s' >= s} w_s' r_a,s'[i] r_c,s'[j] G_s'[i, j] (a suffix sum from the widest prefix down)
//   7. grads    ONE launch for both gradients: output tiles never straddle a boundary, the tile's segment chooses which H
//               feeds the product,   grad_a[:, s] = g * (scale * H_s . c[:, s] - a[:, s] * sum_{s' >= s} w r_a^2 t_a)
//               and the mirror image for grad_c; a clamped prefix (|x[:d]| < 1e-12) has r = 1e12 and no projection term,
//               as torch's clamp gives; the columns from max_k d_k on are written as zeros by tiles of their own
// A prefix ONE column wide has an identically zero gradient; stages 4 and 6 leave its pairs out of t and H unless a clamp
// makes the gradient differ from zero (see kernel 6).
// A forward + backward call is 6 launches (7 symmetric), a forward-only call 4 (5): what qst_mnrl_loss needs for ONE width
// is 7 (8) and 4 (5). No atomics, no host synchronisation, every reduction in a fixed order; every tile edge is guarded and
// every index is 64-bit. *grad_out multiplies the finished gradient, as in mnrl.hip.
#include "qst_common.h"

namespace {

#include "fp32_tile.h"

constexpr float kNormEps = 1e-12f;      // F.normalize's eps
constexpr int kMaxK = 8;

// the sorted view of the caller's widths (by value into every kernel)
struct NestP {
    int K;
    int hi[kMaxK];                      // ascending: segment s is [s ? hi[s - 1] : 0, hi[s])
    float w[kMaxK];                     // the weight of the prefix that ends segment s
    int order[kMaxK];                   // its index in the caller's arrays
};
__device__ __forceinline__ int seg_lo(const NestP& p, int s) { return s ? p.hi[s - 1] : 0; }

// ---- workspace layout (floats; every segment starts on a multiple of 4)
struct NestWs {
    size_t rinv, nrm, rowterm, colterm, cmax, csum, ta, tc, S, G, total;
    int ldS;
};
inline NestWs nested_layout(int B, int N, int K) {
    NestWs w;
    w.ldS = (int)pad4((size_t)N);
    const size_t k = (size_t)K;
    size_t o = 0;
    w.rinv = o; o += pad4(k * ((size_t)B + N));
    w.nrm = o; o += pad4(k * ((size_t)B + N));
    w.rowterm = o; o += pad4(k * B);
    w.colterm = o; o += pad4(k * B);
    w.cmax = o; o += pad4(k * B);
    w.csum = o; o += pad4(k * B);
    w.ta = o; o += pad4(k * B);
    w.tc = o; o += pad4(k * N);
    w.S = o; o += k * B * w.ldS;
    w.G = o; o += k * B * w.ldS;
    w.total = o;
    return w;
}

// ---- 1. prefix norms of a (rows 0 .. B-1) and c (rows B .. B+N-1): [s][row]
__global__ __launch_bounds__(256) void nested_rnorm_kernel(const float* a, const float* c, int B, int N, int D, NestP p,
                                                           float* rinv, float* nrm) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t rows = (int64_t)B + N;
    if (row >= rows) return;
    const float* x = row < B ? a + (size_t)row * D : c + (size_t)(row - B) * D;
    float run = 0.f;
    for (int s = 0; s < p.K; ++s) {
        float part = 0.f;
        for (int i = seg_lo(p, s) + lane; i < p.hi[s]; i += 64) part = __builtin_fmaf(x[i], x[i], part);
        run += wave_sum(part);
        const float n = sqrtf(run);
        if (lane == 0) { nrm[(size_t)s * rows + row] = n; rinv[(size_t)s * rows + row] = 1.f / fmaxf(n, kNormEps); }
    }
}

// ---- 2. S_s[i, j] = scale * r_a,s[i] * r_c,s[j] * <a[i, :d_s], c[j, :d_s]> for every s from one walk over the columns
__global__ __launch_bounds__(256) void nested_scores_kernel(const float* a, const float* c, int B, int N, int D, NestP p,
                                                            float scale, const float* rinv, float* S, int ldS, int vec_in,
                                                            int vecS, int tiles_n) {
    __shared__ __attribute__((aligned(16))) float As[kBK][kLdT];
    __shared__ __attribute__((aligned(16))) float Bs[kBK][kLdT];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int m0 = (int)(blockIdx.x / tiles_n) * kTile, n0 = (int)(blockIdx.x % tiles_n) * kTile;
    const int64_t rows = (int64_t)B + N;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    float ra[4], rb[4];
    for (int s = 0; s < p.K; ++s) {
        const int lo = seg_lo(p, s), hi = p.hi[s];
        const bool vec = vec_in != 0 && (lo & 3) == 0;      // a panel's first column is lo + a multiple of 16
        panel_load<true>(a, D, B, hi, m0, lo, vec, nullptr, ra);
        panel_load<true>(c, D, N, hi, n0, lo, vec, nullptr, rb);
        for (int k0 = lo; k0 < hi; k0 += kBK) {
            panel_store<true>(As, ra);
            panel_store<true>(Bs, rb);
            __syncthreads();
            if (k0 + kBK < hi) {        // the next panel travels while this one is multiplied
                panel_load<true>(a, D, B, hi, m0, k0 + kBK, vec, nullptr, ra);
                panel_load<true>(c, D, N, hi, n0, k0 + kBK, vec, nullptr, rb);
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

        // the boundary d_s: a snapshot of the running sums
        const int n = n0 + tx * 4;
        if (n >= N) continue;
        const float* rA = rinv + (size_t)s * rows;
        const float* rC = rA + B;
        float ns[4] = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) if (n + j < N) ns[j] = rC[n + j];
        float* Ss = S + (size_t)s * B * ldS;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + ty * 4 + i;
            if (m >= B) break;
            const float ms = rA[m];
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float x = acc[i][j] * scale;
                x = x * ms;
                v[j] = x * ns[j];
            }
            float* q = Ss + (size_t)m * ldS + n;
            if (vecS && n + 3 < N) *(f32x4*)q = f32x4{v[0], v[1], v[2], v[3]};
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (n + j < N) q[j] = v[j];
            }
        }
    }
}

// ---- 3. column statistics of the B x B block of S_s (symmetric loss), s = blockIdx.y
__global__ __launch_bounds__(256) void nested_colstat_kernel(const float* S, int ldS, int B, float* cmax, float* csum,
                                                             float* colterm) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t s = blockIdx.y;
    S += s * B * ldS; cmax += s * B; csum += s * B; colterm += s * B;
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

// ---- 4. the row pass, grid (B, K): S_s stays, G_s is written beside it
__global__ __launch_bounds__(256) void nested_row_kernel(const float* S, float* G, int ldS, int B, int N, int symmetric,
                                                         const float* cmax, const float* csum, float* rowterm, float* ta,
                                                         int want_g, const float* nrm_c1) {
    __shared__ float part[4];
    const int i = blockIdx.x, t = threadIdx.x;
    const size_t s = blockIdx.y;
    const float* sr = S + (s * B + i) * ldS;
    float mx = -__builtin_inff();
    for (int j = t; j < N; j += 256) mx = fmaxf(mx, sr[j]);
    mx = block_max<4>(mx, part);
    float sm = 0.f;
    for (int j = t; j < N; j += 256) sm += expf(sr[j] - mx);
    sm = block_sum<4>(sm, part);
    if (t == 0) rowterm[s * B + i] = (logf(sm) + mx) - sr[i];
    if (!want_g) return;
    float* gr = G + (s * B + i) * ldS;
    cmax += s * B; csum += s * B;
    const float coef = (symmetric ? 0.5f : 1.f) / (float)B;
    const float inv = 1.f / sm;
    const bool one_wide = nrm_c1 != nullptr && s == 0;      // see kernel 6
    float dot = 0.f;
    for (int j = t; j < N; j += 256) {
        const float v = sr[j];
        const float hot = j == i ? 1.f : 0.f;
        float pr = expf(v - mx) * inv - hot;
        if (symmetric && j < B) pr += expf(v - cmax[j]) / csum[j] - hot;
        const float g = coef * pr;
        gr[j] = g;
        if (!(one_wide && nrm_c1[j] >= kNormEps)) dot = __builtin_fmaf(g, v, dot);
    }
    dot = block_sum<4>(dot, part);
    if (t == 0) ta[s * B + i] = dot;
}

// ---- 5. the terms and the loss
__global__ __launch_bounds__(1024) void nested_loss_kernel(const float* rowterm, const float* colterm, int B, NestP p,
                                                           float* out_loss, float* out_terms) {
    __shared__ float part[16];
    __shared__ float term[kMaxK], wk[kMaxK];
    for (int s = 0; s < p.K; ++s) {
        float v = 0.f;
        for (int i = threadIdx.x; i < B; i += 1024) v += rowterm[(size_t)s * B + i];
        v = block_sum<16>(v, part);
        float w = 1.f;
        if (colterm) {
            float c = 0.f;
            for (int i = threadIdx.x; i < B; i += 1024) c += colterm[(size_t)s * B + i];
            c = block_sum<16>(c, part);
            v += c;
            w = 0.5f;
        }
        if (threadIdx.x == 0) { term[p.order[s]] = v * (w / (float)B); wk[p.order[s]] = p.w[s]; }
    }
    if (threadIdx.x == 0) {             // the same thread wrote them
        float loss = 0.f;
        for (int k = 0; k < p.K; ++k) {
            if (out_terms) out_terms[k] = term[k];
            loss = __builtin_fmaf(wk[k], term[k], loss);
        }
        out_loss[0] = loss;
    }
}

// ---- 6. the column pass: t_c and, in place of G, the suffix sums H. 64 columns per workgroup, wave w takes rows w, w + 16, ...
__global__ __launch_bounds__(1024) void nested_colpass_kernel(const float* S, float* G, int ldS, int B, int N, NestP p,
                                                              const float* rinv, const float* nrm, float* tc) {
    __shared__ float part[16][64];
    // A prefix ONE column wide has x_hat = +-1 and an identically zero gradient, which the difference of the product and
    // the projection would only reach to rounding (of terms that grow with 1 / |x[0]|). It is sorted first; a pair (i, j)
    // takes part in its H and its t only where the clamp makes the gradient differ from zero: a_i or c_j below 1e-12.
    const bool one_wide = p.hi[0] == 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane;
    const bool in = j < N;
    const bool c_clamped = one_wide && in && nrm[(size_t)B + j] < kNormEps;
    const int64_t rows = (int64_t)B + N;
    const size_t plane = (size_t)B * ldS;
    float cf[kMaxK], acc[kMaxK];
#pragma unroll
    for (int s = 0; s < kMaxK; ++s) {
        acc[s] = 0.f;
        cf[s] = (s < p.K && in) ? p.w[s] * rinv[(size_t)s * rows + B + j] : 0.f;
    }
    if (in) {
        for (int i = w; i < B; i += 16) {
            const size_t at = (size_t)i * ldS + j;
            const bool a_clamped = one_wide && nrm[i] < kNormEps;
            float g[kMaxK];
#pragma unroll
            for (int s = 0; s < kMaxK; ++s) {
                g[s] = 0.f;
                if (s < p.K) {
                    g[s] = G[s * plane + at];
                    if (s == 0 && one_wide && !a_clamped) continue;
                    acc[s] = __builtin_fmaf(g[s], S[s * plane + at], acc[s]);
                }
            }
            float h = 0.f;
#pragma unroll
            for (int s = kMaxK - 1; s >= 0; --s) {
                if (s < p.K) {
                    if (!(s == 0 && one_wide && !a_clamped && !c_clamped))
                        h = __builtin_fmaf(cf[s] * rinv[(size_t)s * rows + i], g[s], h);
                    G[s * plane + at] = h;
                }
            }
        }
    }
    for (int s = 0; s < p.K; ++s) {
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < kMaxK; ++q) if (q == s) v = acc[q];
        part[w][lane] = v;
        __syncthreads();
        if (w == 0 && in) {
            float r = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) r += part[q][lane];
            tc[(size_t)s * N + j] = r;
        }
        __syncthreads();
    }
}

// ---- 7. both gradients. Column tiles are counted per segment (ctile[s] .. ctile[s + 1]); segment K is the zero columns.
struct GradP {
    const float* a; const float* c; float* ga; float* gc;
    const float* H; const float* rinv; const float* nrm; const float* ta; const float* tc; const float* gout;
    int B, N, D, ldS;
    float scale;
    int ctile[kMaxK + 2];
    int tiles_a;                        // row tiles of grad_a; the row tiles of grad_c follow
    int vec_in, vec_out, vecH;
};

// AK: the rows of the output are the rows of H (grad_a), else its columns (grad_c)
template <bool AK>
__device__ __forceinline__ void nested_grad_tile(const GradP& g, const NestP& p, float (*As)[kLdT], float (*Bs)[kLdT], int m0,
                                                 int s, int col0, int colhi) {
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int M = AK ? g.B : g.N, Kred = AK ? g.N : g.B;
    const float* X = AK ? g.c : g.a;                        // the other side's rows feed the product
    const float* Xs = AK ? g.a : g.c;                       // this side's rows take the projection
    float* out = AK ? g.ga : g.gc;
    const int n = col0 + tx * 4;

    if (s >= p.K) {                                         // past the widest prefix
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + ty * 4 + i;
            if (m >= M) break;
#pragma unroll
            for (int j = 0; j < 4; ++j) if (n + j < colhi) out[(size_t)m * g.D + n + j] = 0.f;
        }
        return;
    }

    const float* Hs = g.H + (size_t)s * g.B * g.ldS;
    const bool vecB = g.vec_in != 0 && (col0 & 3) == 0;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    float ra[4], rb[4];
    panel_load<AK>(Hs, g.ldS, M, Kred, m0, 0, g.vecH != 0, nullptr, ra);
    panel_load<false>(X, g.D, colhi, Kred, col0, 0, vecB, nullptr, rb);
    for (int k0 = 0; k0 < Kred; k0 += kBK) {
        panel_store<AK>(As, ra);
        panel_store<false>(Bs, rb);
        __syncthreads();
        if (k0 + kBK < Kred) {
            panel_load<AK>(Hs, g.ldS, M, Kred, m0, k0 + kBK, g.vecH != 0, nullptr, ra);
            panel_load<false>(X, g.D, colhi, Kred, col0, k0 + kBK, vecB, nullptr, rb);
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

    if (n >= colhi) return;
    const float gs = g.gout ? g.gout[0] : 1.f;
    const int64_t rows = (int64_t)g.B + g.N;
    const float* tt = AK ? g.ta : g.tc;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m >= M) break;
        // sum_{s' >= s} w r^2 t over the prefixes that are not clamped, from the widest down
        float proj = 0.f;
        for (int q = p.K - 1; q >= s; --q) {
            const size_t at = (size_t)q * rows + (AK ? 0 : g.B) + m;
            if (g.nrm[at] < kNormEps) continue;             // clamp_min passes no gradient to the norm
            const float r = g.rinv[at];
            proj = __builtin_fmaf(p.w[q] * (r * r), tt[(size_t)q * M + m], proj);
        }
        const float* xs = Xs + (size_t)m * g.D + n;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x = n + j < colhi ? xs[j] : 0.f;
            // the value without grad_out, then times g
            const float y = __builtin_fmaf(-x, proj, acc[i][j] * g.scale);
            v[j] = y * gs;
        }
        float* q = out + (size_t)m * g.D + n;
        if (g.vec_out && (col0 & 3) == 0 && n + 3 < colhi) *(f32x4*)q = f32x4{v[0], v[1], v[2], v[3]};
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (n + j < colhi) q[j] = v[j];
        }
    }
}

__global__ __launch_bounds__(256) void nested_grads_kernel(GradP g, NestP p) {
    __shared__ __attribute__((aligned(16))) float As[kBK][kLdT];
    __shared__ __attribute__((aligned(16))) float Bs[kBK][kLdT];
    const int ct_all = g.ctile[p.K + 1];
    const int rt = (int)(blockIdx.x / ct_all), ct = (int)(blockIdx.x % ct_all);
    int s = 0;
    while (ct >= g.ctile[s + 1]) ++s;                       // ct < ctile[K + 1]
    const int lo = s < p.K ? seg_lo(p, s) : p.hi[p.K - 1];
    const int colhi = s < p.K ? p.hi[s] : g.D;
    const int col0 = lo + (ct - g.ctile[s]) * kTile;
    if (rt < g.tiles_a) nested_grad_tile<true>(g, p, As, Bs, rt * kTile, s, col0, colhi);
    else nested_grad_tile<false>(g, p, As, Bs, (rt - g.tiles_a) * kTile, s, col0, colhi);
}

bool finite_f(float x) { return x == x && x > -__builtin_inff() && x < __builtin_inff(); }

}  // namespace

extern "C" size_t qst_mnrl_nested_workspace_bytes(int B, int N, int D, int K) {
    if (B < 1 || N < B || D < 1 || K < 1 || K > kMaxK) return 0;
    return nested_layout(B, N, K).total * sizeof(float);
}

extern "C" int qst_mnrl_nested_loss(const float* a, const float* c, int B, int N, int D, const int32_t* dims,
                                    const float* weights, int K, float scale, int symmetric, float* out_loss,
                                    float* out_terms, const float* grad_out, float* grad_a, float* grad_c, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    if (B < 1 || N < B || D < 1 || !a || !c || !out_loss || !workspace) return QST_ERR_BAD_ARG;
    if (K < 1 || K > kMaxK || !dims || !weights) return QST_ERR_BAD_ARG;
    if (symmetric != 0 && symmetric != 1) return QST_ERR_BAD_ARG;
    if (!(scale > 0.f) || !(scale < __builtin_inff())) return QST_ERR_BAD_ARG;   // NaN fails the first comparison
    if ((grad_a == nullptr) != (grad_c == nullptr)) return QST_ERR_BAD_ARG;
    if (((uintptr_t)workspace & 3) != 0) return QST_ERR_BAD_ARG;
    for (int k = 0; k < K; ++k) {
        if (dims[k] < 1 || dims[k] > D || !finite_f(weights[k])) return QST_ERR_BAD_ARG;
        for (int q = 0; q < k; ++q) if (dims[q] == dims[k]) return QST_ERR_BAD_ARG;
    }
    const NestWs L = nested_layout(B, N, K);
    if (workspace_bytes < L.total * sizeof(float)) return QST_ERR_BAD_ARG;
    // the kernels index in 64 bits; rows and tiles are counted in 32
    if ((int64_t)B * L.ldS > 0x7FFFFFFFLL || (int64_t)N * D > 0x7FFFFFFFLL) return QST_ERR_UNSUPPORTED;

    // ascending widths (insertion sort of at most 8)
    NestP p = {};
    p.K = K;
    for (int k = 0; k < K; ++k) {
        int s = k;
        while (s > 0 && p.hi[s - 1] > dims[k]) { p.hi[s] = p.hi[s - 1]; p.w[s] = p.w[s - 1]; p.order[s] = p.order[s - 1]; --s; }
        p.hi[s] = dims[k]; p.w[s] = weights[k]; p.order[s] = k;
    }

    const bool want_g = grad_a != nullptr;
    const int64_t tm = ((int64_t)B + kTile - 1) / kTile, tn = ((int64_t)N + kTile - 1) / kTile;
    GradP g = {};
    if (tm * tn > 0x7FFFFFFFLL) return QST_ERR_UNSUPPORTED;
    if (want_g) {
        int64_t ct = 0;
        for (int s = 0; s <= K; ++s) {
            const int lo = s ? p.hi[s - 1] : 0, hi = s < K ? p.hi[s] : D;
            g.ctile[s] = (int)ct;
            ct += ((int64_t)(hi - lo) + kTile - 1) / kTile;
        }
        g.ctile[K + 1] = (int)ct;
        if ((tm + tn) * ct > 0x7FFFFFFFLL) return QST_ERR_UNSUPPORTED;
    }

    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    float* rinv = ws + L.rinv;
    float* nrm = ws + L.nrm;
    float* S = ws + L.S;
    float* G = ws + L.G;
    const bool vec_in = (D % 4 == 0) && al16(a) && al16(c);
    const unsigned row_grid = (unsigned)(((int64_t)B + N + 3) / 4);

    nested_rnorm_kernel<<<row_grid, 256, 0, st>>>(a, c, B, N, D, p, rinv, nrm);
    QST_LAUNCH_CHECK();
    nested_scores_kernel<<<(unsigned)(tm * tn), 256, 0, st>>>(a, c, B, N, D, p, scale, rinv, S, L.ldS, vec_in ? 1 : 0,
                                                              al16(S) ? 1 : 0, (int)tn);
    QST_LAUNCH_CHECK();
    if (symmetric) {
        nested_colstat_kernel<<<dim3((unsigned)((B + 63) / 64), (unsigned)K), 256, 0, st>>>(S, L.ldS, B, ws + L.cmax,
                                                                                            ws + L.csum, ws + L.colterm);
        QST_LAUNCH_CHECK();
    }
    nested_row_kernel<<<dim3((unsigned)B, (unsigned)K), 256, 0, st>>>(S, G, L.ldS, B, N, symmetric, ws + L.cmax, ws + L.csum,
                                                                      ws + L.rowterm, ws + L.ta, want_g ? 1 : 0,
                                                                      p.hi[0] == 1 ? nrm + B : nullptr);
    QST_LAUNCH_CHECK();
    nested_loss_kernel<<<1, 1024, 0, st>>>(ws + L.rowterm, symmetric ? ws + L.colterm : nullptr, B, p, out_loss, out_terms);
    QST_LAUNCH_CHECK();
    if (!want_g) return QST_OK;

    nested_colpass_kernel<<<(unsigned)tn, 1024, 0, st>>>(S, G, L.ldS, B, N, p, rinv, nrm, ws + L.tc);
    QST_LAUNCH_CHECK();
    g.a = a; g.c = c; g.ga = grad_a; g.gc = grad_c;
    g.H = G; g.rinv = rinv; g.nrm = nrm; g.ta = ws + L.ta; g.tc = ws + L.tc; g.gout = grad_out;
    g.B = B; g.N = N; g.D = D; g.ldS = L.ldS;
    g.scale = scale;
    g.tiles_a = (int)tm;
    g.vec_in = vec_in ? 1 : 0;
    g.vec_out = (D % 4 == 0) && al16(grad_a) && al16(grad_c) ? 1 : 0;
    g.vecH = al16(G) ? 1 : 0;
    nested_grads_kernel<<<(unsigned)((tm + tn) * g.ctile[K + 1]), 256, 0, st>>>(g, p);
    QST_LAUNCH_CHECK();
    return QST_OK;
}
