// cross.hip -- the classification head of a cross-encoder (include/qst.h: qst_cls_head_fwd).
//
// Replaces what sits on top of the encoder in transformers' BertForSequenceClassification (pooler: dense + tanh over the
// [CLS] row, then classifier) and RobertaForSequenceClassification (classifier.dense + tanh over <s>, then
// classifier.out_proj), and sentence-transformers 2.2.2 CrossEncoder.predict's activation (Sigmoid for one label, Identity
// otherwise) and optional softmax over the labels:
//     h = tanh(W1 x + b1)    [H]      W1 [H, H]
//     z = W2 h + b2          [C]      W2 [C, H], C <= 8
//     out = act(z), then softmax over C when asked for and C > 1
// All in fp32: the head is ~5e-5 of a pair's FLOPs at stsb-roberta-large widths, and fp32 keeps it out of the error budget.
//
// One workgroup per tile of CH_ROWS rows: the tile's inputs are staged in LDS and W1 is streamed once per tile (not once per
// row). Each wave owns CH_J output features at a time: its lanes read the CH_J rows of W1 as coalesced float4 runs over k,
// the NEXT CH_J rows are in flight while the current ones are multiplied against every row of the tile, and the CH_J x
// CH_ROWS partial dots are reduced across the wave on the DPP path (wave_sum). h stays in LDS; the C logits of each row are
// reduced in the same launch, and one thread per row applies the activation.
#include "qst_common.h"
#include "qst_kernels.h"

namespace {

constexpr int CH_ROWS = 8;       // rows per workgroup tile
constexpr int CH_WAVES = 8;      // 512 threads
constexpr int CH_J = 4;          // output features per wave step
constexpr int CH_KV = 4;         // float4 runs of 256 features: H <= 1024
constexpr int CH_MAX_C = 8;

__global__ __launch_bounds__(64 * CH_WAVES) void cls_head_kernel(const float* __restrict__ x, int64_t ldx, int n, int H,
                                                                 const float* __restrict__ w1, const float* __restrict__ b1,
                                                                 const float* __restrict__ w2, const float* __restrict__ b2,
                                                                 int C, int act, int softmax, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* xs = (float*)smem;                       // [CH_ROWS][H]
    float* hs = xs + CH_ROWS * H;                   // [CH_ROWS][H]
    __shared__ float zs[CH_ROWS][CH_MAX_C];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.x * CH_ROWS;
    const int rows = min(CH_ROWS, n - r0);
    for (int i = tid; i < CH_ROWS * H; i += 64 * CH_WAVES) {
        const int r = i / H, k = i - r * H;
        xs[i] = r < rows ? x[(size_t)(r0 + r) * ldx + k] : 0.f;
    }
    __syncthreads();

    // ---- h = tanh(W1 x + b1): wave w takes features j0 = CH_J * (w + CH_WAVES * step), ..., + CH_J - 1
    auto load = [&](int j0, float4 (&w)[CH_J][CH_KV]) {
#pragma unroll
        for (int jj = 0; jj < CH_J; ++jj)
#pragma unroll
            for (int v = 0; v < CH_KV; ++v) {
                const int k = 256 * v + 4 * lane;
                w[jj][v] = (j0 + jj < H && k < H) ? *(const float4*)(w1 + (size_t)(j0 + jj) * H + k)
                                                  : make_float4(0.f, 0.f, 0.f, 0.f);
            }
    };
    const int jstep = CH_J * CH_WAVES;
    float4 wc[CH_J][CH_KV], wn[CH_J][CH_KV];
    int j0 = CH_J * wave;
    if (j0 < H) load(j0, wc);
    for (; j0 < H; j0 += jstep) {
        if (j0 + jstep < H) load(j0 + jstep, wn);
        float acc[CH_J][CH_ROWS];
#pragma unroll
        for (int jj = 0; jj < CH_J; ++jj)
#pragma unroll
            for (int r = 0; r < CH_ROWS; ++r) acc[jj][r] = 0.f;
#pragma unroll
        for (int v = 0; v < CH_KV; ++v) {
            const int k = 256 * v + 4 * lane;
            if (k >= H) continue;
#pragma unroll
            for (int r = 0; r < CH_ROWS; ++r) {
                const float4 xv = *(const float4*)(xs + r * H + k);
#pragma unroll
                for (int jj = 0; jj < CH_J; ++jj)
                    acc[jj][r] += (wc[jj][v].x * xv.x + wc[jj][v].y * xv.y) + (wc[jj][v].z * xv.z + wc[jj][v].w * xv.w);
            }
        }
#pragma unroll
        for (int jj = 0; jj < CH_J; ++jj) {
            const int j = j0 + jj;
            const float bj = j < H ? b1[j] : 0.f;
#pragma unroll
            for (int r = 0; r < CH_ROWS; ++r) {
                const float s = wave_sum(acc[jj][r]);
                if (lane == r && j < H) hs[r * H + j] = tanhf(s + bj);
            }
        }
#pragma unroll
        for (int jj = 0; jj < CH_J; ++jj)
#pragma unroll
            for (int v = 0; v < CH_KV; ++v) wc[jj][v] = wn[jj][v];
    }
    __syncthreads();

    // ---- z = W2 h + b2: the CH_ROWS x C dots, one per wave at a time, lanes over the features
    for (int p = wave; p < CH_ROWS * C; p += CH_WAVES) {
        const int r = p / C, c = p - r * C;
        float s = 0.f;
        for (int k = lane; k < H; k += 64) s += w2[(size_t)c * H + k] * hs[r * H + k];
        s = wave_sum(s);
        if (lane == 0) zs[r][c] = s + b2[c];
    }
    __syncthreads();

    // ---- activation (ST CrossEncoder.predict: activation_fct, then softmax over the labels when there is more than one)
    if (tid < rows) {
        float z[CH_MAX_C];
#pragma unroll
        for (int c = 0; c < CH_MAX_C; ++c) {
            z[c] = c < C ? zs[tid][c] : 0.f;
            if (act == QST_HEAD_ACT_SIGMOID) z[c] = 1.f / (1.f + expf(-z[c]));
        }
        if (softmax && C > 1) {
            float m = -INFINITY, sum = 0.f;
#pragma unroll
            for (int c = 0; c < CH_MAX_C; ++c) if (c < C) m = fmaxf(m, z[c]);
#pragma unroll
            for (int c = 0; c < CH_MAX_C; ++c) if (c < C) { z[c] = expf(z[c] - m); sum += z[c]; }
#pragma unroll
            for (int c = 0; c < CH_MAX_C; ++c) z[c] /= sum;
        }
        for (int c = 0; c < C; ++c) out[(size_t)(r0 + tid) * C + c] = z[c];
    }
}

QstLdsAttr g_cls_head_lds;

}  // namespace

extern "C" int qst_cls_head_fwd(const float* x, int64_t ldx, int n, int H, const float* w1, const float* b1, const float* w2,
                                const float* b2, int C, int act, int softmax, float* out, void* stream) {
    if (!x || !w1 || !b1 || !w2 || !b2 || !out || n <= 0 || H <= 0 || ldx < H) return QST_ERR_BAD_ARG;
    if (C < 1 || C > CH_MAX_C || (act != QST_HEAD_ACT_NONE && act != QST_HEAD_ACT_SIGMOID) || (softmax != 0 && softmax != 1))
        return QST_ERR_BAD_ARG;
    if (H > 256 * CH_KV || H % 4 != 0) return QST_ERR_UNSUPPORTED;
    if (((uintptr_t)w1 & 15) != 0) return QST_ERR_BAD_ARG;          // float4 runs of W1's rows
    const int lds = 2 * CH_ROWS * H * (int)sizeof(float);
    if (int rc = qst_ensure_lds(g_cls_head_lds, (const void*)cls_head_kernel, 2 * CH_ROWS * 1024 * (int)sizeof(float))) return rc;
    const int grid = (n + CH_ROWS - 1) / CH_ROWS;
    cls_head_kernel<<<grid, 64 * CH_WAVES, lds, (hipStream_t)stream>>>(x, ldx, n, H, w1, b1, w2, b2, C, act, softmax, out);
    QST_LAUNCH_CHECK();
    return QST_OK;
}
