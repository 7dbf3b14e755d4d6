// fp32_mgemm.h -- what the losses that walk a batch in strips of rows (mnrl_stream.hip, gist.hip) share: the exact-fp32
// matrix-core product of their score and gradient GEMMs, and the two row kernels around the strips (reciprocal norms first,
// the backward of F.normalize last). Included inside the including file's own anonymous namespace, after fp32_tile.h.
//
// All products run on v_mfma_f32_32x32x2_f32 (exact fp32, bitwise a k-ordered fmaf chain): K panels of 16 staged through LDS in
// the [k][row] layout of fp32_tile.h, which is the shape the instruction's operands want (lane l reads A[row l & 31][k l >> 5]
// and B[k l >> 5][col l & 31], one float each). 256 threads = 2 x 2 waves; a workgroup owns 128 x 128 outputs (2 x 2
// accumulators per wave), or 64 x 64 (one per wave) when the larger tile would leave compute units idle. Every output
// element is one accumulator walking K in order, so its bits do not depend on the tile, on its place in it, or on the strip.
// Every tile edge is guarded in M, N and K (odd K included: the panels are zero-filled), every index is 64-bit.
#pragma once

constexpr float kNormEps = 1e-12f;                      // F.normalize's eps
constexpr int kChunkK = 4096;                           // split-K products: K columns per partial product (multiple of kBK)
constexpr int kCUs = 256;

// ---- row norms of a (rows 0 .. B-1) and c (rows B .. B+N-1): as stage 1 of mnrl.hip
template <bool VEC>
__global__ __launch_bounds__(256) void mnrls_rnorm_kernel(const float* a, const float* c, int B, int N, int D,
                                                          float* rinv, float* nrm) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)B + N) return;
    const float* x = row < B ? a + (size_t)row * D : c + (size_t)(row - B) * D;
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

// ---- C[M, N] (+)= alpha * mscale[m] * nscale[n] * sum_k A(m, k) * kscale[k] * B(k, n) on the fp32 matrix cores
// AK: A(m, k) = A[m * lda + k] (k contiguous), else A[k * lda + m]. BKC: B(k, n) = Bm[n * ldb + k], else Bm[k * ldb + n].
// blockIdx.y = y takes k in [y * kchunk, min(K, (y + 1) * kchunk)) and writes the tile at C + y * cstride.
struct MGemmP {
    const float* A; const float* Bm; float* C;
    int M, N, K, lda, ldb, ldc;
    const float* kscale;                // per k, applied to the n-contiguous B operand as its panel is loaded (null = 1)
    const float* mscale; const float* nscale;   // null = 1
    float alpha;
    int accumulate;                     // C += instead of C =
    int vecA, vecB;                     // 16-byte loads allowed (leading dimension % 4 == 0, pointer aligned)
    int tiles_n, kchunk;
    size_t cstride;
};

// One thread's TS / 64 float4 pieces of a TS x kBK panel; R: extent of the row index, K: end of the k range.
template <bool KC, int TS>
__device__ __forceinline__ void mpanel_load(const float* P, int ld, int R, int K, int r0, int k0, bool vec,
                                            const float* kscale, float (&reg)[TS / 64][4]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int h = 0; h < TS / 64; ++h) {
        reg[h][0] = reg[h][1] = reg[h][2] = reg[h][3] = 0.f;
        if (KC) {
            const int r = r0 + (t >> 2) + 64 * h, k = k0 + (t & 3) * 4;
            if (r < R && k < K) {
                const float* q = P + (size_t)r * ld + k;
                if (vec && k + 3 < K) {
                    const f32x4 v = *(const f32x4*)q;
                    reg[h][0] = v[0]; reg[h][1] = v[1]; reg[h][2] = v[2]; reg[h][3] = v[3];
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (k + e < K) reg[h][e] = q[e];
                }
            }
        } else {
            constexpr int per = TS / 4;         // float4 pieces per k row
            const int k = k0 + t / per + h * (256 / per), r = r0 + (t % per) * 4;
            if (k < K && r < R) {
                const float* q = P + (size_t)k * ld + r;
                if (vec && r + 3 < R) {
                    const f32x4 v = *(const f32x4*)q;
                    reg[h][0] = v[0]; reg[h][1] = v[1]; reg[h][2] = v[2]; reg[h][3] = v[3];
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (r + e < R) reg[h][e] = q[e];
                }
                if (kscale) {
                    const float ks = kscale[k];
#pragma unroll
                    for (int e = 0; e < 4; ++e) reg[h][e] *= ks;
                }
            }
        }
    }
}

template <bool KC, int TS>
__device__ __forceinline__ void mpanel_store(float (*T)[TS + 4], const float (&reg)[TS / 64][4]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int h = 0; h < TS / 64; ++h) {
        if (KC) {
            const int r = (t >> 2) + 64 * h, k = (t & 3) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) T[k + e][r] = reg[h][e];
        } else {
            constexpr int per = TS / 4;
            const int k = t / per + h * (256 / per), r = (t % per) * 4;
            *(f32x4*)&T[k][r] = f32x4{reg[h][0], reg[h][1], reg[h][2], reg[h][3]};
        }
    }
}

template <bool AK, bool BKC, int TS>
__global__ __launch_bounds__(256) void mnrls_gemm_kernel(MGemmP p) {
    constexpr int FR = TS / 64;         // 32 x 32 accumulators per wave: FR x FR
    constexpr int WT = TS / 2;          // a wave's outputs: WT x WT
    __shared__ __attribute__((aligned(16))) float As[kBK][TS + 4];
    __shared__ __attribute__((aligned(16))) float Bs[kBK][TS + 4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = wave >> 1, wc = wave & 1, l31 = lane & 31, lh = lane >> 5;
    const int m0 = (int)(blockIdx.x / p.tiles_n) * TS, n0 = (int)(blockIdx.x % p.tiles_n) * TS;
    const int kb = (int)blockIdx.y * p.kchunk;
    const int ke = (p.K - kb) < p.kchunk ? p.K : kb + p.kchunk;
    float* C = p.C + (size_t)blockIdx.y * p.cstride;

    f32x16 acc[FR][FR];
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int j = 0; j < FR; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    float ra[FR][4], rb[FR][4];
    mpanel_load<AK, TS>(p.A, p.lda, p.M, ke, m0, kb, p.vecA != 0, nullptr, ra);
    mpanel_load<BKC, TS>(p.Bm, p.ldb, p.N, ke, n0, kb, p.vecB != 0, p.kscale, rb);
    for (int k0 = kb; k0 < ke; k0 += kBK) {
        mpanel_store<AK, TS>(As, ra);
        mpanel_store<BKC, TS>(Bs, rb);
        __syncthreads();
        if (k0 + kBK < ke) {            // the next panel travels while this one is multiplied
            mpanel_load<AK, TS>(p.A, p.lda, p.M, ke, m0, k0 + kBK, p.vecA != 0, nullptr, ra);
            mpanel_load<BKC, TS>(p.Bm, p.ldb, p.N, ke, n0, k0 + kBK, p.vecB != 0, p.kscale, rb);
        }
#pragma unroll
        for (int kk = 0; kk < kBK; kk += 2) {
            float av[FR], bv[FR];
#pragma unroll
            for (int i = 0; i < FR; ++i) av[i] = As[kk + lh][wr * WT + i * 32 + l31];
#pragma unroll
            for (int j = 0; j < FR; ++j) bv[j] = Bs[kk + lh][wc * WT + j * 32 + l31];
#pragma unroll
            for (int i = 0; i < FR; ++i)
#pragma unroll
                for (int j = 0; j < FR; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // accumulator element e of lane l: row (e & 3) + 8 * (e >> 2) + 4 * (l >> 5), column l & 31
#pragma unroll
    for (int j = 0; j < FR; ++j) {
        const int n = n0 + wc * WT + j * 32 + l31;
        if (n >= p.N) continue;
        const float ns = p.nscale ? p.nscale[n] : 1.f;
#pragma unroll
        for (int i = 0; i < FR; ++i) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wr * WT + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (m >= p.M) continue;
                const float ms = p.mscale ? p.mscale[m] : 1.f;
                float x = acc[i][j][e] * p.alpha;   // a chain of single multiplications, as in mnrl.hip
                x = x * ms;
                x = x * ns;
                float* q = C + (size_t)m * p.ldc + n;
                if (p.accumulate) x = q[0] + x;
                q[0] = x;
            }
        }
    }
}

// ---- backward of F.normalize, in place on the rows of grad_a and grad_c (which hold d_hat), times *grad_out: as stage 7
// of mnrl.hip
template <bool VEC>
__global__ __launch_bounds__(256) void mnrls_normbwd_kernel(const float* a, const float* c, float* ga, float* gc, int B, int N,
                                                            int D, const float* rinv, const float* nrm, const float* gout) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)B + N) return;
    const float* x = row < B ? a + (size_t)row * D : c + (size_t)(row - B) * D;
    float* d = row < B ? ga + (size_t)row * D : gc + (size_t)(row - B) * D;
    const float r = rinv[row];
    const bool clamped = nrm[row] < kNormEps;   // clamp_min passes no gradient to the norm: d_hat / eps
    const float g = gout ? gout[0] : 1.f;
    float dot = 0.f;
    if (VEC) {
        const int nv = D >> 2;
        for (int v = lane; v < nv; v += 64) {
            const f32x4 X = *(const f32x4*)(x + (size_t)v * 4), G = *(const f32x4*)(d + (size_t)v * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) dot = __builtin_fmaf(X[j] * r, G[j], dot);
        }
    } else {
        for (int i = lane; i < D; i += 64) dot = __builtin_fmaf(x[i] * r, d[i], dot);
    }
    dot = wave_sum(dot);
    // each element is read and then written by the same lane
    if (VEC) {
        const int nv = D >> 2;
        for (int v = lane; v < nv; v += 64) {
            const f32x4 X = *(const f32x4*)(x + (size_t)v * 4), G = *(const f32x4*)(d + (size_t)v * 4);
            f32x4 O;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float tt = clamped ? G[j] : __builtin_fmaf(-(X[j] * r), dot, G[j]);
                const float y = r * tt;
                O[j] = y * g;
            }
            *(f32x4*)(d + (size_t)v * 4) = O;
        }
    } else {
        for (int i = lane; i < D; i += 64) {
            const float tt = clamped ? d[i] : __builtin_fmaf(-(x[i] * r), dot, d[i]);
            const float y = r * tt;
            d[i] = y * g;
        }
    }
}

// BIG: the 128 x 128 tile may be chosen. A product with few output rows never has the tiles for it before its K chunks
// fill the device.
template <bool AK, bool BKC, bool BIG>
int launch_mgemm(MGemmP p, int chunks, hipStream_t st) {
    p.vecA = (p.lda % 4 == 0) && al16(p.A);
    p.vecB = (p.ldb % 4 == 0) && al16(p.Bm);
    const int64_t big = (((int64_t)p.M + 127) / 128) * (((int64_t)p.N + 127) / 128) * chunks;
    const int ts = (BIG && big >= kCUs) ? 128 : 64;     // a speed choice only: an output element's bits do not depend on it
    const int64_t tm = ((int64_t)p.M + ts - 1) / ts, tn = ((int64_t)p.N + ts - 1) / ts;
    if (tm * tn > 0x7FFFFFFFLL) return QST_ERR_UNSUPPORTED;
    p.tiles_n = (int)tn;
    const dim3 grid((unsigned)(tm * tn), (unsigned)chunks);
    if constexpr (BIG) {
        if (ts == 128) mnrls_gemm_kernel<AK, BKC, 128><<<grid, 256, 0, st>>>(p);
        else mnrls_gemm_kernel<AK, BKC, 64><<<grid, 256, 0, st>>>(p);
    } else {
        mnrls_gemm_kernel<AK, BKC, 64><<<grid, 256, 0, st>>>(p);
    }
    QST_LAUNCH_CHECK();
    return QST_OK;
}

inline bool strip_rows_ok(int strip_rows) { return strip_rows == 0 || (strip_rows > 0 && strip_rows % 64 == 0); }
