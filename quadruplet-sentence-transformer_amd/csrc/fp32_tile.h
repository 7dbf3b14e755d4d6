// fp32_tile.h -- what the losses that score a whole batch against itself (mnrl.hip, batch_triplet.hip) share: the operand
// panels of their LDS-tiled fp32 loop (64 x 64 outputs per 256-thread workgroup, K panels of 16 through LDS, 4 x 4 outputs
// per thread) and the fixed-order block reductions. Every tile edge is guarded, every index is 64-bit. Included inside the
// including file's own anonymous namespace.
#pragma once

constexpr int kTile = 64;               // outputs per workgroup: kTile x kTile
constexpr int kBK = 16;                 // K panel
constexpr int kLdT = kTile + 4;         // LDS row pitch in floats (16-byte multiple)

inline size_t pad4(size_t n) { return (n + 3) & ~(size_t)3; }

// ---- fixed-order block reductions over `NW` waves
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* part) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) r += part[w];
    __syncthreads();
    return r;
}
template <int NW>
__device__ __forceinline__ float block_max(float v, float* part) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = part[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) r = fmaxf(r, part[w]);
    __syncthreads();
    return r;
}

// One thread's four elements of a kTile x kBK panel. R: extent of the row index (M or N), r0 / k0: the panel's origin.
// KC: P(r, k) = P[r * ld + k] (k contiguous), else P[k * ld + r]. kscale (per k) is looked at in the row-contiguous form
// only.
template <bool KC>
__device__ __forceinline__ void panel_load(const float* P, int ld, int R, int K, int r0, int k0, bool vec,
                                           const float* kscale, float (&reg)[4]) {
    const int t = threadIdx.x;
    reg[0] = reg[1] = reg[2] = reg[3] = 0.f;
    if (KC) {
        const int r = r0 + (t >> 2), k = k0 + (t & 3) * 4;
        if (r < R && k < K) {
            const float* q = P + (size_t)r * ld + k;
            if (vec && k + 3 < K) {
                const f32x4 v = *(const f32x4*)q;
                reg[0] = v[0]; reg[1] = v[1]; reg[2] = v[2]; reg[3] = v[3];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (k + e < K) reg[e] = q[e];
            }
        }
    } else {
        const int k = k0 + (t >> 4), r = r0 + (t & 15) * 4;
        if (k < K && r < R) {
            const float* q = P + (size_t)k * ld + r;
            if (vec && r + 3 < R) {
                const f32x4 v = *(const f32x4*)q;
                reg[0] = v[0]; reg[1] = v[1]; reg[2] = v[2]; reg[3] = v[3];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (r + e < R) reg[e] = q[e];
            }
            if (kscale) {
                const float ks = kscale[k];
#pragma unroll
                for (int e = 0; e < 4; ++e) reg[e] *= ks;
            }
        }
    }
}

template <bool KC>
__device__ __forceinline__ void panel_store(float (*T)[kLdT], const float (&reg)[4]) {
    const int t = threadIdx.x;
    if (KC) {
        const int r = t >> 2, k = (t & 3) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) T[k + e][r] = reg[e];
    } else {
        const int k = t >> 4, r = (t & 15) * 4;
        *(f32x4*)&T[k][r] = f32x4{reg[0], reg[1], reg[2], reg[3]};
    }
}
