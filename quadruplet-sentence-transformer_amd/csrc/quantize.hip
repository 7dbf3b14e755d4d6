// quantize.hip -- embedding quantization and the searches that run on the small codes (sentence_transformers.quantization,
// 2.6+: quantize_embeddings, semantic_search_faiss / _usearch's "retrieve on the codes, rescore with the float query").
//
//   qst_column_ranges        per-column minimum / maximum of a calibration set (upstream's `ranges`), NaN-propagating
//   qst_quantize_rows        f32 rows -> packed sign bits (ubinary / binary) or 8-bit codes (uint8 / int8)
//   qst_topk_hamming_stream  streaming top-k by -(Hamming distance) of packed codes: xor + popcount on the VALU
//   qst_topk_int8_stream     streaming top-k by the exact int32 dot product: v_mfma_i32_32x32x32_i8
//   qst_rescore_quantized    float query x quantized candidate row, for the shortlist of a first stage
//
// Both streams keep qst_topk_stream's contract (retrieval.hip): a [<= 2048 queries, chunk] f32 score block per step, merged
// into the running [nq, k] result by qst_topk_merge_rows, so ordering and tie rules are the float search's. Every score here
// is an integer of magnitude <= 2^24, exact in f32. Vector stores only, no atomics, no host synchronisation.
#include "qst_common.h"
#include "qst_kernels.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;

constexpr int kQueryBlock = 2048;        // score block rows, as in retrieval.hip
constexpr int kTopkMax = 1024;
constexpr int kRangeParts = 128;         // row slices of the first stage of qst_column_ranges (fixed: n does not change it)

inline size_t pad4(size_t n) { return (n + 3) / 4 * 4; }
inline bool al4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// ---------------------------------------------------------------- column ranges
// NaN-propagating running minimum / maximum: a NaN fails every comparison, so it is carried as a flag.
struct MinMax {
    float lo, hi;
    bool nan;
    __device__ __forceinline__ void init() { lo = INFINITY; hi = -INFINITY; nan = false; }
    __device__ __forceinline__ void take(float v) {
        nan |= v != v;
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
};

// Stage 1: grid (ceil(dim / 64), kRangeParts); 64 columns x 4 row lanes per workgroup. Row lane ty of slice p walks rows
// 4 p + ty, + 4 kRangeParts, ...; a wave reads 64 consecutive columns of one row. The four row lanes meet in LDS and the
// slice's result goes to part[p][0 / 1][col] (NaN where the slice saw one; +inf / -inf where it had no row).
__global__ __launch_bounds__(256) void ranges_part_kernel(const float* x, int64_t n, int dim, float* part) {
    __shared__ float slo[4][64], shi[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + tx;
    MinMax m;
    m.init();
    if (col < dim)
        for (int64_t r = (int64_t)blockIdx.y * 4 + ty; r < n; r += 4 * kRangeParts) m.take(x[(size_t)r * dim + col]);
    slo[ty][tx] = m.nan ? NAN : m.lo;
    shi[ty][tx] = m.nan ? NAN : m.hi;
    __syncthreads();
    if (ty == 0 && col < dim) {
        MinMax a, b;
        a.init(); b.init();
#pragma unroll
        for (int i = 0; i < 4; ++i) { a.take(slo[i][tx]); b.take(shi[i][tx]); }
        part[((size_t)blockIdx.y * 2 + 0) * dim + col] = a.nan ? NAN : a.lo;
        part[((size_t)blockIdx.y * 2 + 1) * dim + col] = b.nan ? NAN : b.hi;
    }
}

// Stage 2: one thread per column folds the kRangeParts slices in slice order.
__global__ __launch_bounds__(256) void ranges_finish_kernel(const float* part, int dim, float* out) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= dim) return;
    MinMax a, b;
    a.init(); b.init();
    for (int p = 0; p < kRangeParts; ++p) {
        a.take(part[((size_t)p * 2 + 0) * dim + col]);
        b.take(part[((size_t)p * 2 + 1) * dim + col]);
    }
    out[col] = a.nan ? NAN : a.lo;
    out[(size_t)dim + col] = b.nan ? NAN : b.hi;
}

// ---------------------------------------------------------------- sign bits
// np.packbits(x > 0, axis=-1): bit 7 - (j % 8) of byte j / 8. NaN > 0, 0 > 0 and -0 > 0 are false; a denormal is compared
// as the integer pattern would be (sign clear, not zero), so a flushed comparison cannot lose it.
__device__ __forceinline__ uint32_t positive(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    return (u - 1u) < 0x7F800000u ? 1u : 0u;             // 0 < u <= +inf: positive finite, denormal or +inf
}

// One wave per row, 16 bytes (4 elements) a lane, 256 elements = 32 output bytes a trip. A lane's four bits are a nibble;
// the even lane takes its neighbour's nibble (quad DPP, no LDS) and stores the byte. dim % 4 == 0 and x 16-byte aligned.
__global__ __launch_bounds__(256) void bits_rows_vec_kernel(const float* x, int64_t n, int dim, int nbytes, uint8_t flip,
                                                            uint8_t* out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* src = x + (size_t)row * dim;
    uint8_t* dst = out + (size_t)row * nbytes;
    for (int c0 = 0; c0 < dim; c0 += 256) {
        const int c = c0 + 4 * lane;
        uint32_t nib = 0;
        if (c < dim) {
            const f32x4 v = *(const f32x4*)(src + c);
            nib = (positive(v[0]) << 3) | (positive(v[1]) << 2) | (positive(v[2]) << 1) | positive(v[3]);
        }
        // quad_perm [1, 1, 3, 3]: lanes 0 and 2 of a quad read lanes 1 and 3
        const uint32_t next = (uint32_t)__builtin_amdgcn_mov_dpp((int)nib, 0xF5, 0xf, 0xf, true);
        const int b = c >> 3;
        if (!(lane & 1) && b < nbytes) dst[b] = (uint8_t)(((nib << 4) | next) ^ flip);
    }
}

// Any dim and any 4-byte aligned x: one element a lane, the wave's 64 comparisons by ballot. Bit i of the ballot is
// element c0 + i; reversing all 64 bits puts element c0 + 8 b + e at bit 63 - 8 b - e, i.e. bit 7 - e of byte 7 - b.
__global__ __launch_bounds__(256) void bits_rows_kernel(const float* x, int64_t n, int dim, int nbytes, uint8_t flip,
                                                        uint8_t* out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;                                  // (uniform per wave)
    const float* src = x + (size_t)row * dim;
    uint8_t* dst = out + (size_t)row * nbytes;
    for (int c0 = 0; c0 < dim; c0 += 64) {
        const int c = c0 + lane;
        const bool p = c < dim && positive(src[c]);
        const unsigned long long rev = __brevll(__ballot(p));
        const int b = (c0 >> 3) + lane;
        if (lane < 8 && b < nbytes) dst[b] = (uint8_t)((uint32_t)(rev >> (8 * (7 - (lane & 7)))) ^ flip);
    }
}

// ---------------------------------------------------------------- 8-bit codes
// upstream: ((emb - starts) / steps [- 128]).astype(uint8 / int8) on float32 arrays, steps = (ends - starts) / 255. Each
// operation is one correctly rounded fp32 operation (a division stays a division); out of range saturates, NaN and a
// constant column (hi == lo) give the lowest code.
__device__ __forceinline__ uint32_t code8(float x, float lo, float hi, bool is_signed) {
    const float step = (hi - lo) / 255.0f;
    float t = (x - lo) / step;
    if (hi == lo) t = NAN;
    if (is_signed) {
        const float u = t - 128.0f;
        const int c = u >= 127.0f ? 127 : (u > -128.0f ? (int)u : -128);       // (int): toward zero; NaN fails both
        return (uint32_t)c & 0xFFu;
    }
    const int c = t >= 255.0f ? 255 : (t > 0.0f ? (int)t : 0);
    return (uint32_t)c;
}

// 4 elements a thread: 16-byte reads of x and of both range rows, one 4-byte store. dim % 4 == 0, x and ranges 16-byte
// aligned, out 4-byte aligned. total4 = n * dim / 4.
__global__ __launch_bounds__(256) void code_rows_vec_kernel(const float* x, int64_t total4, int dim, const float* ranges,
                                                            int is_signed, uint32_t* out) {
    const int dim4 = dim >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % dim4) * 4;
        const f32x4 v = *(const f32x4*)(x + 4 * (size_t)i);
        const f32x4 lo = *(const f32x4*)(ranges + c);
        const f32x4 hi = *(const f32x4*)(ranges + (size_t)dim + c);
        uint32_t w = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) w |= code8(v[e], lo[e], hi[e], is_signed) << (8 * e);
        out[i] = w;
    }
}

__global__ __launch_bounds__(256) void code_rows_kernel(const float* x, int64_t total, int dim, const float* ranges,
                                                        int is_signed, uint8_t* out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % dim);
        out[i] = (uint8_t)code8(x[i], ranges[c], ranges[(size_t)dim + c], is_signed);
    }
}

// ---------------------------------------------------------------- Hamming scores
// out[q][c] = -(popcount(query q xor corpus c)) for a [rows, cols] block. A thread owns one corpus row and keeps 8 of its
// words in registers at a time; a workgroup covers 256 corpus rows x 32 queries. The query words are the same for every
// lane (their address depends on blockIdx and loop counters only), so they arrive through the scalar cache and enter the
// xor as a scalar operand: per pair and word one v_xor and one v_bcnt (which adds into the count). Integers throughout.
// VEC: nbytes % 16 == 0 and both bases 16-byte aligned -> 16-byte corpus loads; otherwise dword loads. Query and corpus
// rows past the edge are clamped for the loads and never stored.
constexpr int kHamQ = 32, kHamW = 8;

// words w0 .. w0 + W - 1 of the corpus row against the same words of 32 queries. FULL: all W words exist, nothing is
// guarded and a query's W words are one scalar load; otherwise words at or past nw count as zero on both sides.
template <bool VEC, int W, bool FULL>
__device__ __forceinline__ void hamming_segment(const uint32_t* __restrict__ q, const uint32_t* __restrict__ crow, int q0,
                                                int rows, int nw, int w0, int (&acc)[kHamQ]) {
    uint32_t cw[W];
    if (VEC) {
#pragma unroll
        for (int g = 0; g < W / 4; ++g) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (FULL || w0 + 4 * g < nw) v = *(const u32x4*)(crow + w0 + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) cw[4 * g + e] = v[e];
        }
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) cw[j] = (FULL || w0 + j < nw) ? crow[w0 + j] : 0u;
    }
#pragma unroll
    for (int i = 0; i < kHamQ; ++i) {
        const int qi = q0 + i < rows ? q0 + i : rows - 1;
        const uint32_t* qrow = q + (size_t)qi * nw + w0;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const uint32_t qw = (FULL || w0 + j < nw) ? qrow[j] : 0u;
            acc[i] += __popc(qw ^ cw[j]);
        }
    }
}

// the row in segments of 8 words, then one of 4 where 4 more are whole (dim 384 is 8 + 4), then the guarded rest (< 4 words:
// only where nbytes % 16 != 0)
template <bool VEC>
__global__ __launch_bounds__(256) void hamming_scores_kernel(const uint32_t* __restrict__ q, const uint32_t* __restrict__ c,
                                                             int rows, int cols, int nw, float* __restrict__ out,
                                                             int64_t ld) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    const int q0 = blockIdx.y * kHamQ;
    const uint32_t* crow = c + (size_t)(col < cols ? col : cols - 1) * nw;
    int acc[kHamQ];
#pragma unroll
    for (int i = 0; i < kHamQ; ++i) acc[i] = 0;
    int w0 = 0;
    for (; w0 + kHamW <= nw; w0 += kHamW) hamming_segment<VEC, kHamW, true>(q, crow, q0, rows, nw, w0, acc);
    if (w0 + 4 <= nw) {
        hamming_segment<VEC, 4, true>(q, crow, q0, rows, nw, w0, acc);
        w0 += 4;
    }
    if (w0 < nw) hamming_segment<VEC, 4, false>(q, crow, q0, rows, nw, w0, acc);
    if (col >= cols) return;
#pragma unroll
    for (int i = 0; i < kHamQ; ++i)
        if (q0 + i < rows) out[(size_t)(q0 + i) * ld + col] = (float)(-acc[i]);
}

// ---------------------------------------------------------------- int8 dot-product scores
// out[q][c] = sum_j q[j] * c[j] in int32 for a [rows, cols] block on v_mfma_i32_32x32x32_i8. A wave owns 64 queries x 64
// corpus rows as 2 x 2 tiles of 32 x 32, so every fragment it loads feeds two instructions; four waves = 64 queries x 256
// corpus rows per workgroup. An NT product straight from global memory: lane l's A fragment of k-step s is the 16 bytes at
// k = 32 s + 16 (l >> 5) of query row l & 31 of the tile, its B fragment the same bytes of corpus row l & 31 -- whatever
// order the instruction gives the 16 bytes of a fragment, both operands have the same one, and the sum over k does not care.
// The next step's four fragments are requested before the current step's instructions. C/D: column = lane & 31 (corpus),
// row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (query). Rows past the edge are clamped for the loads and skipped by the
// stores. dim % 32 == 0, both bases 16-byte aligned.
constexpr int kI8Q = 64, kI8C = 256;      // queries x corpus rows of a workgroup

__global__ __launch_bounds__(256) void int8_scores_kernel(const int8_t* __restrict__ q, const int8_t* __restrict__ c, int rows,
                                                          int cols, int dim, float* __restrict__ out, int64_t ld) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.y * kI8Q, c0 = blockIdx.x * kI8C + wave * 64;
    if (c0 >= cols) return;                                // (uniform per wave; no barrier in this kernel)
    const i32x4* ap[2];
    const i32x4* bp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int qi = q0 + 32 * t + r < rows ? q0 + 32 * t + r : rows - 1;
        const int ci = c0 + 32 * t + r < cols ? c0 + 32 * t + r : cols - 1;
        ap[t] = (const i32x4*)(q + (size_t)qi * dim + 16 * h);
        bp[t] = (const i32x4*)(c + (size_t)ci * dim + 16 * h);
    }
    i32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;
    const int steps = dim >> 5;
    i32x4 a[2] = {ap[0][0], ap[1][0]}, b[2] = {bp[0][0], bp[1][0]};
    for (int s = 0; s < steps; ++s) {
        i32x4 an[2] = {a[0], a[1]}, bn[2] = {b[0], b[1]};
        if (s + 1 < steps) {
#pragma unroll
            for (int t = 0; t < 2; ++t) { an[t] = ap[t][2 * (s + 1)]; bn[t] = bp[t][2 * (s + 1)]; }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 2; ++t) { a[t] = an[t]; b[t] = bn[t]; }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = c0 + 32 * j + r;
        if (col >= cols) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = q0 + 32 * i + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                if (row < rows) out[(size_t)row * ld + col] = (float)acc[i][j][reg];
            }
    }
}

// ---------------------------------------------------------------- rescoring
// out[r][p] = sum_j q[r][j] * v(corpus[cand[r][p]][j]) in fp32: one wave per (query, candidate), lanes across dim, partial
// sums by fmaf, then the wave tree. A negative id gives -inf; an id >= nc (the caller's error) reads nothing and gives NaN.
__global__ __launch_bounds__(256) void rescore_kernel(const float* q, const uint8_t* corpus, int kind, int64_t nc, int dim,
                                                      int row_bytes, const int64_t* cand, int64_t ld, int kc, int64_t pairs,
                                                      float* out) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= pairs) return;                             // (uniform per wave)
    const int64_t r = pair / kc;
    const int p = (int)(pair % kc);
    const int64_t id = cand[(size_t)r * ld + p];
    float* dst = out + (size_t)r * ld + p;
    if (id < 0 || id >= nc) {
        if (lane == 0) *dst = id < 0 ? -INFINITY : NAN;
        return;
    }
    const float* qr = q + (size_t)r * dim;
    const uint8_t* cr = corpus + (size_t)id * row_bytes;
    float s = 0.f;
    if (kind == QST_QUANT_INT8) {
        for (int j = lane; j < dim; j += 64) s = fmaf(qr[j], (float)(int8_t)cr[j], s);
    } else if (kind == QST_QUANT_UINT8) {
        for (int j = lane; j < dim; j += 64) s = fmaf(qr[j], (float)cr[j], s);
    } else {
        const uint32_t flip = kind == QST_QUANT_BINARY ? 0x80u : 0u;
        for (int j = lane; j < dim; j += 64) {
            const uint32_t byte = (uint32_t)cr[j >> 3] ^ flip;
            s += ((byte >> (7 - (j & 7))) & 1u) ? qr[j] : 0.f;
        }
    }
    s = wave_sum(s);
    if (lane == 0) *dst = s;
}

inline bool kind_ok(int kind) { return kind >= QST_QUANT_INT8 && kind <= QST_QUANT_UBINARY; }
inline bool kind_bits(int kind) { return kind == QST_QUANT_BINARY || kind == QST_QUANT_UBINARY; }

// the argument checks the two streams share; `chunk` comes back clamped to nc
int stream_check(const void* queries, const void* corpus, int nq, int nc, int width, int k, int& chunk, int64_t query_base,
                 int64_t corpus_base, const float* run_scores, const int64_t* run_index, const void* ws) {
    if (!queries || !corpus || !run_scores || !run_index || !ws || nq <= 0 || nc <= 0 || width <= 0 || k <= 0 || chunk <= 0)
        return QST_ERR_BAD_ARG;
    if (query_base < 0 || corpus_base < 0 || query_base > INT64_MAX - nq || corpus_base > INT64_MAX - nc)
        return QST_ERR_BAD_ARG;
    if (k > kTopkMax) return QST_ERR_UNSUPPORTED;
    if (chunk > nc) chunk = nc;
    return QST_OK;
}

size_t block_bytes(int nq, int chunk) {
    const size_t qrows = (size_t)(nq < kQueryBlock ? nq : kQueryBlock);
    return qrows * pad4((size_t)chunk) * sizeof(float) + 1024;
}

// chunk by chunk, query block by query block: score(q rows, corpus rows, rows, cols, out, ld), then the merge
template <typename Score>
int stream_run(const uint8_t* queries, const uint8_t* corpus, int nq, int nc, int row_bytes, int k, int chunk,
               int64_t query_base, int64_t corpus_base, int exclude_self, float* run_scores, int64_t* run_index, float* sc,
               hipStream_t st, Score score) {
    for (int c0 = 0; c0 < nc; c0 += chunk) {
        const int cols = nc - c0 < chunk ? nc - c0 : chunk;
        const int64_t ld = (int64_t)pad4(cols);
        for (int q0 = 0; q0 < nq; q0 += kQueryBlock) {
            const int rows = nq - q0 < kQueryBlock ? nq - q0 : kQueryBlock;
            int rc = score(queries + (size_t)q0 * row_bytes, corpus + (size_t)c0 * row_bytes, rows, cols, sc, ld);
            if (rc != QST_OK) return rc;
            rc = qst_topk_merge_rows(sc, ld, rows, cols, corpus_base + c0, query_base + q0, exclude_self, INFINITY, k,
                                     run_scores + (size_t)q0 * k, run_index + (size_t)q0 * k, st);
            if (rc != QST_OK) return rc;
        }
    }
    return QST_OK;
}

}  // namespace

extern "C" size_t qst_column_ranges_workspace_bytes(int64_t n, int dim) {
    if (n <= 0 || dim <= 0) return 0;
    return (size_t)kRangeParts * 2 * dim * sizeof(float);
}

extern "C" int qst_column_ranges(const float* x, int64_t n, int dim, float* out, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    if (!x || !out || !workspace || n <= 0 || dim <= 0 || !al4(x) || !al4(out) || !al4(workspace)) return QST_ERR_BAD_ARG;
    if (workspace_bytes < qst_column_ranges_workspace_bytes(n, dim)) return QST_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    ranges_part_kernel<<<dim3((dim + 63) / 64, kRangeParts), 256, 0, st>>>(x, n, dim, part);
    QST_LAUNCH_CHECK();
    ranges_finish_kernel<<<(dim + 255) / 256, 256, 0, st>>>(part, dim, out);
    QST_LAUNCH_CHECK();
    return QST_OK;
}

extern "C" int qst_quantize_rows(const float* x, int64_t n, int dim, int kind, const float* ranges, void* out, void* stream) {
    if (!x || !out || n <= 0 || dim <= 0 || !kind_ok(kind) || !al4(x)) return QST_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (kind_bits(kind)) {
        const int64_t blocks = (n + 3) / 4;
        if (blocks > 0x7FFFFFFFLL) return QST_ERR_UNSUPPORTED;
        const int nbytes = (dim + 7) / 8;
        const uint8_t flip = kind == QST_QUANT_BINARY ? 0x80 : 0;
        if (dim % 4 == 0 && al16(x))
            bits_rows_vec_kernel<<<(unsigned)blocks, 256, 0, st>>>(x, n, dim, nbytes, flip, (uint8_t*)out);
        else
            bits_rows_kernel<<<(unsigned)blocks, 256, 0, st>>>(x, n, dim, nbytes, flip, (uint8_t*)out);
        QST_LAUNCH_CHECK();
        return QST_OK;
    }
    if (!ranges || !al4(ranges)) return QST_ERR_BAD_ARG;
    if (n > INT64_MAX / dim) return QST_ERR_UNSUPPORTED;
    const int64_t total = n * dim;
    const int is_signed = kind == QST_QUANT_INT8;
    const bool vec = dim % 4 == 0 && al16(x) && al16(ranges) && al4(out);
    const int64_t work = vec ? total / 4 : total;
    const int64_t want = (work + 255) / 256;
    const unsigned blocks = (unsigned)(want < 65536 ? want : 65536);
    if (vec)
        code_rows_vec_kernel<<<blocks, 256, 0, st>>>(x, work, dim, ranges, is_signed, (uint32_t*)out);
    else
        code_rows_kernel<<<blocks, 256, 0, st>>>(x, work, dim, ranges, is_signed, (uint8_t*)out);
    QST_LAUNCH_CHECK();
    return QST_OK;
}

extern "C" size_t qst_topk_hamming_workspace_bytes(int nq, int chunk, int nbytes) {
    if (nq <= 0 || chunk <= 0 || nbytes <= 0) return 0;
    return block_bytes(nq, chunk);
}

extern "C" int qst_topk_hamming_stream(const uint8_t* queries, const uint8_t* corpus, int nq, int nc, int nbytes, int k,
                                       int chunk, int64_t query_base, int64_t corpus_base, int exclude_self,
                                       float* run_scores, int64_t* run_index, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    int rc = stream_check(queries, corpus, nq, nc, nbytes, k, chunk, query_base, corpus_base, run_scores, run_index, workspace);
    if (rc != QST_OK) return rc;
    if (!al4(queries) || !al4(corpus) || !al4(workspace)) return QST_ERR_BAD_ARG;
    if (nbytes % 4 != 0) return QST_ERR_UNSUPPORTED;
    if (workspace_bytes < qst_topk_hamming_workspace_bytes(nq, chunk, nbytes)) return QST_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int nw = nbytes / 4;
    const bool vec = nbytes % 16 == 0 && al16(queries) && al16(corpus);
    auto score = [=](const uint8_t* q, const uint8_t* c, int rows, int cols, float* sc, int64_t ld) -> int {
        const dim3 grid((cols + 255) / 256, (rows + kHamQ - 1) / kHamQ);
        if (vec)
            hamming_scores_kernel<true><<<grid, 256, 0, st>>>((const uint32_t*)q, (const uint32_t*)c, rows, cols, nw, sc, ld);
        else
            hamming_scores_kernel<false><<<grid, 256, 0, st>>>((const uint32_t*)q, (const uint32_t*)c, rows, cols, nw, sc, ld);
        QST_LAUNCH_CHECK();
        return QST_OK;
    };
    return stream_run(queries, corpus, nq, nc, nbytes, k, chunk, query_base, corpus_base, exclude_self, run_scores, run_index,
                      (float*)workspace, st, score);
}

extern "C" size_t qst_topk_int8_workspace_bytes(int nq, int chunk, int dim) {
    if (nq <= 0 || chunk <= 0 || dim <= 0) return 0;
    return block_bytes(nq, chunk);
}

extern "C" int qst_topk_int8_stream(const int8_t* queries, const int8_t* corpus, int nq, int nc, int dim, int k, int chunk,
                                    int64_t query_base, int64_t corpus_base, int exclude_self, float* run_scores,
                                    int64_t* run_index, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = stream_check(queries, corpus, nq, nc, dim, k, chunk, query_base, corpus_base, run_scores, run_index, workspace);
    if (rc != QST_OK) return rc;
    if (!al16(queries) || !al16(corpus) || !al4(workspace)) return QST_ERR_BAD_ARG;
    if (dim % 32 != 0 || dim > 1024) return QST_ERR_UNSUPPORTED;
    if (workspace_bytes < qst_topk_int8_workspace_bytes(nq, chunk, dim)) return QST_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    auto score = [=](const uint8_t* q, const uint8_t* c, int rows, int cols, float* sc, int64_t ld) -> int {
        const dim3 grid((cols + kI8C - 1) / kI8C, (rows + kI8Q - 1) / kI8Q);
        int8_scores_kernel<<<grid, 256, 0, st>>>((const int8_t*)q, (const int8_t*)c, rows, cols, dim, sc, ld);
        QST_LAUNCH_CHECK();
        return QST_OK;
    };
    return stream_run((const uint8_t*)queries, (const uint8_t*)corpus, nq, nc, dim, k, chunk, query_base, corpus_base,
                      exclude_self, run_scores, run_index, (float*)workspace, st, score);
}

extern "C" int qst_rescore_quantized(const float* queries, const void* corpus, int kind, int64_t nc, int dim,
                                     const int64_t* cand, int64_t ld, int nq, int kc, float* out, void* stream) {
    if (!queries || !corpus || !cand || !out || nq <= 0 || nc <= 0 || dim <= 0 || kc <= 0 || ld < kc || !kind_ok(kind) ||
        !al4(queries) || !al4(out) || ((uintptr_t)cand & 7) != 0)
        return QST_ERR_BAD_ARG;
    const int64_t pairs = (int64_t)nq * kc;
    if ((pairs + 3) / 4 > 0x7FFFFFFFLL) return QST_ERR_UNSUPPORTED;
    const int row_bytes = kind_bits(kind) ? (dim + 7) / 8 : dim;
    rescore_kernel<<<(unsigned)((pairs + 3) / 4), 256, 0, (hipStream_t)stream>>>(queries, (const uint8_t*)corpus, kind, nc, dim,
                                                                                row_bytes, cand, ld, kc, pairs, out);
    QST_LAUNCH_CHECK();
    return QST_OK;
}
