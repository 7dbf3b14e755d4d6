// binary_eval.hip -- what sentence-transformers 2.2.2's evaluation.BinaryClassificationEvaluator computes from the scores
// and the 0 / 1 labels of n sentence pairs: the cut of the sorted pairs with the best accuracy and the one with the best F1
// (each with its threshold, the mean of the two scores around the cut) and the average precision. Upstream sorts the pairs
// on the host and walks them in Python; here nothing is sorted. Every quantity is a count per pair:
//
//   before(i) = { j : k_j > k_i, or k_j == k_i and j <= i }     its place in the stable sort, itself included
//   ge(i)     = { j : k_j >= k_i }                               the pairs at least as similar
//
// with k the score's bits made monotone ("more similar" is always "larger": negated first for a distance; both zeros one
// key). Three launches on the caller's stream, no atomics, all counts integers, the one floating-point sum in a fixed order:
//   1. pack    one 64-bit word per pair: key << 21 | (2^20 - 1 - j) << 1 | label. Words compare as the sort orders the pairs.
//   2. count   N x N: a workgroup per 1024 pairs i (4 to a lane), all pairs j walked through LDS tiles, every lane reading
//              the same word per step. |before(i)| is a permutation of 1 .. n, so pair i stores its record {score,
//              positives in before(i), |ge(i)| and its label, positives in ge(i)} at that place: the records lie in sorted
//              order without a sort.
//   3. finish  a workgroup per set walks the records: integer argmax for the accuracy, upstream's expression in double for
//              F1, ties to the earliest cut; the sum of the average precision as row_loss.h's second stage takes its sums.
#include "qst_common.h"

namespace {

constexpr int64_t kMaxPairs = (int64_t)1 << 20;
constexpr int kMaxSets = 8;
constexpr int kIdxBits = 20;                // an index below kMaxPairs
constexpr int kTileI = 1024;                // pairs i of a workgroup of the counting pass: 256 lanes x kPerLane
constexpr int kPerLane = 4;
constexpr int kTileJ = 1024;                // words of an LDS tile (8 KiB)
constexpr uint32_t kLabelBit = 0x80000000u; // in a record's |ge| word
static_assert(kTileI == 256 * kPerLane && kTileJ % 256 == 0 && kTileJ < (1 << 16), "tiles of the counting pass");

struct SetFlags { int32_t high[kMaxSets]; };

inline size_t words_bytes(int64_t n, int nsets) { return (((size_t)n * nsets * sizeof(uint64_t)) + 15) & ~(size_t)15; }

// ---- 1. the order words
__global__ __launch_bounds__(256) void be_pack_kernel(const float* scores, const int64_t* labels, int n, SetFlags flags,
                                                      uint64_t* words) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int set = blockIdx.y;
    if (j >= n) return;
    uint32_t u = __builtin_bit_cast(uint32_t, scores[(size_t)set * n + j]);
    if (!flags.high[set]) u ^= 0x80000000u;                     // a distance: the smaller, the more similar
    if ((u << 1) == 0) u = 0;                                   // -0.0 == +0.0
    uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // unsigned order of the keys = order of the floats
    key = key < 1u ? 1u : key;                                  // 0 is left to the padding of the last LDS tile
    const uint64_t lab = labels[j] != 0;
    words[(size_t)set * n + j] = ((uint64_t)key << (kIdxBits + 1)) | ((uint64_t)((kMaxPairs - 1) - j) << 1) | lab;
}

// ---- 2. the counts of every pair, stored at the pair's place in the sorted order
__global__ __launch_bounds__(256) void be_count_kernel(const float* scores, const uint64_t* words, int n, uint4* records) {
    __shared__ uint64_t tile[kTileJ];
    const int set = blockIdx.y;
    const uint64_t* w = words + (size_t)set * n;
    const int i0 = blockIdx.x * kTileI + threadIdx.x;
    uint64_t q[kPerLane], g[kPerLane];      // j is in before(i) when word_j >= q_i, in ge(i) when word_j >= g_i
    uint32_t nb[kPerLane], tb[kPerLane], ng[kPerLane], tg[kPerLane];
#pragma unroll
    for (int m = 0; m < kPerLane; ++m) {
        const int i = i0 + m * 256;
        const uint64_t wi = i < n ? w[i] : ~(uint64_t)0;        // past the end: above every word, counts nothing
        q[m] = wi & ~(uint64_t)1;
        g[m] = wi & ~(((uint64_t)1 << (kIdxBits + 1)) - 1);
        nb[m] = tb[m] = ng[m] = tg[m] = 0;
    }
    for (int j0 = 0; j0 < n; j0 += kTileJ) {
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kTileJ / 256; ++t) {
            const int j = j0 + t * 256 + threadIdx.x;
            tile[t * 256 + threadIdx.x] = j < n ? w[j] : 0;     // 0 is below every q and g
        }
        __syncthreads();
        // within a tile a count stays below 2^16: the pairs in the low half of a word, the positives among them in the high
        uint32_t pb[kPerLane] = {}, pg[kPerLane] = {};
#pragma unroll 8
        for (int jj = 0; jj < kTileJ; ++jj) {
            const uint64_t wj = tile[jj];
            const uint32_t one = 1u | (((uint32_t)wj & 1u) << 16);
#pragma unroll
            for (int m = 0; m < kPerLane; ++m) {
                pb[m] += wj >= q[m] ? one : 0u;
                pg[m] += wj >= g[m] ? one : 0u;
            }
        }
#pragma unroll
        for (int m = 0; m < kPerLane; ++m) {
            nb[m] += pb[m] & 0xFFFFu; tb[m] += pb[m] >> 16;
            ng[m] += pg[m] & 0xFFFFu; tg[m] += pg[m] >> 16;
        }
    }
    uint4* rec = records + (size_t)set * n;
#pragma unroll
    for (int m = 0; m < kPerLane; ++m) {
        const int i = i0 + m * 256;
        const uint32_t place = nb[m] - 1u;
        if (i < n && place < (uint32_t)n) {
            const uint32_t lab = (uint32_t)w[i] & 1u;
            rec[place] = make_uint4(__builtin_bit_cast(uint32_t, scores[(size_t)set * n + i]), tb[m],
                                    ng[m] | (lab ? kLabelBit : 0u), tg[m]);
        }
    }
}

// ---- 3. the cuts and the average precision of a set
struct BestAcc { int32_t v; uint32_t r; };      // v = 2 * positives before - place: the accuracy's count less n - T
struct BestF1 { double f1; uint32_t r; };
__device__ __forceinline__ bool better(const BestAcc& a, const BestAcc& b) { return a.v > b.v || (a.v == b.v && a.r < b.r); }
__device__ __forceinline__ bool better(const BestF1& a, const BestF1& b) { return a.f1 > b.f1 || (a.f1 == b.f1 && a.r < b.r); }

// upstream's expression, one rounding per operation in its order: precision = c / e, recall = c / T, 2 * p * r / (p + r)
__device__ __forceinline__ double f1_of(uint32_t c, uint32_t e, uint32_t T, double* p_out, double* r_out) {
#pragma clang fp contract(off)
    const double p = (double)c / (double)e;
    const double r = (double)c / (double)T;
    const double num = (2.0 * p) * r;
    const double den = p + r;
    if (p_out) { *p_out = p; *r_out = r; }
    return num / den;
}

__device__ __forceinline__ float score_of(const uint4& rec) { return __builtin_bit_cast(float, rec.x); }

__global__ __launch_bounds__(1024) void be_finish_kernel(const uint4* records, int n, double* out) {
    __shared__ BestAcc s_acc[1024];
    __shared__ BestF1 s_f1[1024];
    __shared__ double s_part[16];
    const int set = blockIdx.x;
    const uint4* rec = records + (size_t)set * n;
    const uint32_t T = rec[n - 1].w;                            // ge(the last pair) is every pair
    BestAcc acc = {INT32_MIN, 0xFFFFFFFFu};
    BestF1 f1 = {0.0, 0xFFFFFFFFu};
    double ap = 0.0;
    for (int64_t r = threadIdx.x; r < n; r += 1024) {           // thread i: places i, i + 1024, ... in that order
        const uint4 R = rec[r];
        if (R.z & kLabelBit) ap += (double)R.w / (double)(R.z & ~kLabelBit);
        if (r == n - 1) continue;                               // the last pair is no cut
        const BestAcc a = {2 * (int32_t)R.y - (int32_t)(r + 1), (uint32_t)r};
        if (better(a, acc)) acc = a;
        if (R.y > 0) {
            const BestF1 f = {f1_of(R.y, (uint32_t)(r + 1), T, nullptr, nullptr), (uint32_t)r};
            if (better(f, f1)) f1 = f;
        }
    }
    ap = wave_sum_f64(ap);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = ap;
    s_acc[threadIdx.x] = acc;
    s_f1[threadIdx.x] = f1;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {                         // (value, place) is a total order: any tree gives the same
        if ((int)threadIdx.x < s) {
            if (better(s_acc[threadIdx.x + s], s_acc[threadIdx.x])) s_acc[threadIdx.x] = s_acc[threadIdx.x + s];
            if (better(s_f1[threadIdx.x + s], s_f1[threadIdx.x])) s_f1[threadIdx.x] = s_f1[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x >= 64) return;
    double total = threadIdx.x < 16 ? s_part[threadIdx.x] : 0.0;
    total = wave_sum_f64(total);
    if (threadIdx.x != 0) return;
    double* o = out + (size_t)set * 8;
    // upstream's start values hold where no cut beats them: accuracy 0 at threshold -1, the F1 block 0
    double res[8] = {0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, (double)T};
    const BestAcc A = s_acc[0];
    if (A.r != 0xFFFFFFFFu) {
        const int64_t count = (int64_t)A.v + (int64_t)n - (int64_t)T;
        if (count > 0) {
            res[0] = (double)count / (double)n;
            res[1] = (double)((score_of(rec[A.r]) + score_of(rec[A.r + 1])) * 0.5f);
        }
    }
    const BestF1 F = s_f1[0];
    if (F.r != 0xFFFFFFFFu) {
        res[2] = f1_of(rec[F.r].y, F.r + 1, T, &res[3], &res[4]);
        res[5] = (double)((score_of(rec[F.r]) + score_of(rec[F.r + 1])) * 0.5f);
    }
    if (T > 0) res[6] = total / (double)T;
    for (int k = 0; k < 8; ++k) o[k] = res[k];
}

}  // namespace

extern "C" size_t qst_binary_eval_workspace_bytes(int64_t n, int nsets) {
    if (n < 1 || n > kMaxPairs || nsets < 1 || nsets > kMaxSets) return 0;
    return words_bytes(n, nsets) + (size_t)n * nsets * sizeof(uint4);
}

extern "C" int qst_binary_eval(const float* scores, const int64_t* labels, int64_t n, int nsets, const int32_t* high_is_similar,
                               double* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!scores || !labels || !high_is_similar || !out || !workspace || n < 1 || nsets < 1) return QST_ERR_BAD_ARG;
    if (((uintptr_t)scores & 3) || ((uintptr_t)labels & 7) || ((uintptr_t)out & 7) || !al16(workspace)) return QST_ERR_BAD_ARG;
    if (n > kMaxPairs || nsets > kMaxSets) return QST_ERR_UNSUPPORTED;
    if (workspace_bytes < qst_binary_eval_workspace_bytes(n, nsets)) return QST_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    SetFlags flags = {};
    for (int s = 0; s < nsets; ++s) flags.high[s] = high_is_similar[s] != 0;
    uint64_t* words = (uint64_t*)workspace;
    uint4* records = (uint4*)((char*)workspace + words_bytes(n, nsets));
    const int N = (int)n;
    be_pack_kernel<<<dim3((N + 255) / 256, nsets), 256, 0, st>>>(scores, labels, N, flags, words);
    QST_LAUNCH_CHECK();
    be_count_kernel<<<dim3((N + kTileI - 1) / kTileI, nsets), 256, 0, st>>>(scores, words, N, records);
    QST_LAUNCH_CHECK();
    be_finish_kernel<<<nsets, 1024, 0, st>>>(records, N, out);
    QST_LAUNCH_CHECK();
    return QST_OK;
}
