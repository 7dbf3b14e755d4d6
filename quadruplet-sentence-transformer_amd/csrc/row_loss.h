// row_loss.h -- what the row-wise loss kernels (loss.hip, tuple_loss.hip, distill.hip, cosent.hip) share around their loops:
// the row of a wave, the choice of the form a launch takes, the one-workgroup second stage and its block reductions, and the
// cosine's value and gradient scalars.
// Row indices, the grid size and the second stage's loop are 64-bit: B may be near INT_MAX.
#pragma once
#include <type_traits>
#include "qst_common.h"

namespace {

constexpr float kCosEps = 1e-8f;    // torch cosine_similarity default eps (each norm clamped on its own)
constexpr int kMaxRowVec = 8;       // float4 per lane and row kept in registers -> D <= 64*4*8 = 2048

// four waves to a 256-thread workgroup, one row tuple to a wave: the wave's row, false past the last one. The last workgroup's
// rows reach B + 2, which an int cannot hold at B near INT_MAX; 32 unsigned bits can, and from there on the row is a 64-bit index
__device__ __forceinline__ bool wave_row(int B, int64_t& row) {
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
    row = r;
    return r < (uint32_t)B;
}
inline int row_grid(int B) { return (int)(((int64_t)B + 3) / 4); }
// offset of a row's first element (row < B and D fit an int: one 32 x 32 -> 64-bit multiply)
__device__ __forceinline__ size_t row_base(int64_t row, int D) { return (size_t)((int64_t)(int)row * D); }

// ---- the form of a launch. The kernels have up to three: NV > 0, the rows are read once, 16 bytes a lane, and stay in
// registers (NV float4 per lane and row: rows of up to 256 * NV floats) for the gradient pass; NV == 0 and VEC, the rows
// stream 16 bytes a lane and the gradient pass reads them again; NV == 0 and not VEC, element by element (D not a multiple
// of 4 or unaligned pointers), read again likewise.
// every row and, where gradients are asked for, every gradient row may be accessed 16 bytes a lane
inline bool rows_al16(const float* const* x, int nx, float* const* g, int ng) {
    bool ok = true;
    for (int k = 0; k < nx; ++k) ok = ok && al16(x[k]);
    for (int k = 0; k < ng; ++k) ok = ok && (!g[0] || al16(g[k]));      // the gradients are all given or all null
    return ok;
}
// fn(integral_constant<int, NV>, bool_constant<VEC>). STREAM16: the kernel has the streaming 16-byte form; one without it
// goes element by element wherever the rows do not fit the registers, and may ignore VEC: it is then NV > 0.
template <bool STREAM16, class F>
void dispatch_form(int D, bool aligned, F fn) {
    const bool vec = (D % 4 == 0) && aligned;
    const int n = (D + 255) / 256;
    using T = std::true_type;
    if (vec && n <= kMaxRowVec) {
        if (n <= 1) fn(std::integral_constant<int, 1>{}, T{});
        else if (n <= 2) fn(std::integral_constant<int, 2>{}, T{});
        else if (n <= 3) fn(std::integral_constant<int, 3>{}, T{});
        else if (n <= 4) fn(std::integral_constant<int, 4>{}, T{});
        else fn(std::integral_constant<int, kMaxRowVec>{}, T{});
        return;
    }
    if constexpr (STREAM16) {
        if (vec) { fn(std::integral_constant<int, 0>{}, T{}); return; }
    }
    fn(std::integral_constant<int, 0>{}, std::false_type{});
}

// ---- second stage for 'sum' / 'mean': one workgroup over the per-row values. Thread i takes rows i, i + 1024, ... in that
// order, then the wave tree, then the 16 wave totals through the same tree: a fixed order, so the same inputs give the same
// bits. T = float: out = sum * k (k = 1 or 1 / B). T = double: the sum runs in double and out = sum / k, divided in double
// and rounded to fp32 once (k = 1, B or B * D).
template <typename T>
__global__ __launch_bounds__(1024) void row_sum_kernel(const float* rows, int B, T k, float* out) {
    __shared__ T part[16];
    auto total = [](T v) {
        if constexpr (std::is_same<T, double>::value) return wave_sum_f64(v);
        else return wave_sum(v);
    };
    T s = 0;
    for (int64_t i = threadIdx.x; i < B; i += 1024) s += (T)rows[i];
    s = total(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    T r = (threadIdx.x & 63) < 16 ? part[threadIdx.x & 63] : (T)0;
    r = total(r);
    if (threadIdx.x == 0) {
        if constexpr (std::is_same<T, double>::value) out[0] = (float)(r / k);
        else out[0] = r * k;
    }
}

// ---- what a one-workgroup second stage of 1024 threads reduces with: the wave tree, then the 16 wave totals through the same
// tree (part: 16 floats of LDS). A max or min drops NaNs, as fmaxf does.
enum { OP_SUM = 0, OP_MAX = 1, OP_MIN = 2 };
template <int OP>
__device__ __forceinline__ float block_reduce(float v, float* part) {
    const float id = OP == OP_SUM ? 0.f : (OP == OP_MAX ? -__builtin_inff() : __builtin_inff());
    v = OP == OP_SUM ? wave_sum(v) : (OP == OP_MAX ? wave_max(v) : -wave_max(-v));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = (threadIdx.x & 63) < 16 ? part[threadIdx.x & 63] : id;
    r = OP == OP_SUM ? wave_sum(r) : (OP == OP_MAX ? wave_max(r) : -wave_max(-r));
    __syncthreads();
    return r;
}

// ---- cosine of a pair from its dot product and the two norms, and the scalars of its gradient:
// dm/dx = kxy * y + kxx * x, dm/dy = kxy * x + kyy * y. A norm at or below the clamp is a constant and passes no gradient.
// dist: the distance 1 - cos and its gradient.
struct CosVal { float m, kxy, kxx, kyy; };
__device__ __forceinline__ CosVal cos_finish(float dot, float nx, float ny, bool dist) {
    const float cx = fmaxf(nx, kCosEps), cy = fmaxf(ny, kCosEps);
    const float inv = 1.f / (cx * cy);
    const float cs = dot * inv;
    const float sg = dist ? -1.f : 1.f;
    CosVal r;
    r.m = dist ? 1.f - cs : cs;
    r.kxy = sg * inv;
    r.kxx = nx > kCosEps ? -sg * cs / (cx * cx) : 0.f;
    r.kyy = ny > kCosEps ? -sg * cs / (cy * cy) : 0.f;
    return r;
}

}  // namespace
