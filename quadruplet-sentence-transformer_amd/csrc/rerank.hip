// rerank.hip -- what sentence-transformers 2.2.2's evaluation.RerankingEvaluator computes for nq queries, each with its own
// list of candidate documents (ragged groups of one flat array): the score of every document against the query of its
// group, and from the scores the reciprocal rank within k, the average precision and the NDCG within k of every group and
// their means. Upstream scores, sorts and walks one query at a time on the host; here nothing is sorted. With s the scores of
// a group (the larger the better, floats compared as floats, -0.0 == +0.0), every quantity is a count per positive p:
//
//   rank(p)   = 1 + |{ d : s_d > s_p, or s_d == s_p and d < p }|     its place in a stable descending sort
//   ge_all(p) = |{ d : s_d >= s_p }|,  ge_pos(p) = |{ positives d : s_d >= s_p }|
//
//   rr = 1 / min_p rank(p) where that is <= k, ap = (1 / P) sum_p ge_pos(p) / ge_all(p),
//   ndcg = sum_{p : rank(p) <= k} 1 / log2(1 + rank(p)) over sum_{i = 1 .. min(P, k)} 1 / log2(1 + i)
//
// The grids depend on nq and nd alone (the host never sees a group's size); the group of a document is found by a binary
// search in offsets that stays inside offsets[1 .. nq - 1], whatever they hold. Launches, all on the caller's stream,
// without atomics:
//   scores   flat over the documents, four consecutive ones to a wave with their rows in flight together: the lanes stride
//            the rows, 16 bytes a lane where every row is 16-byte aligned and element by element otherwise, then the wave tree.
//   count    flat over the documents, 64 consecutive ones to a wave: every lane looks its own up, and for each that is a
//            positive of a valid group the lanes stride the scores of that group and the wave writes the record {rank,
//            ge_pos, ge_all, non-finite scores of the group} at the document's index.
//   finish   a workgroup per query: the terms of 256 positives at a time in parallel, added by one thread in document order.
//   means    one workgroup, the sums taken as row_loss.h's second stage takes its sums.
#include <math.h>
#include "qst_common.h"

namespace {

constexpr int64_t kMaxCount = (int64_t)1 << 31;     // nq and nd stay below it: every count and index fits 32 unsigned bits
constexpr uint32_t kInvalid = 0x80000000u;          // in a query's info word; the other bits count its non-finite scores

inline size_t records_bytes(int64_t nd) { return (size_t)nd * sizeof(uint4); }
inline size_t info_bytes(int64_t nq) { return (((size_t)nq * sizeof(uint32_t)) + 15) & ~(size_t)15; }

template <int CTRL> __device__ __forceinline__ uint32_t dpp_mov_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t lane_u32(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
// wave_sum's tree (qst_common.h) on a count
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    v += dpp_mov_u32<0xB1>(v);
    v += dpp_mov_u32<0x4E>(v);
    v += dpp_mov_u32<0x141>(v);
    v += dpp_mov_u32<0x140>(v);
    return (lane_u32(v, 0) + lane_u32(v, 16)) + (lane_u32(v, 32) + lane_u32(v, 48));
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    v = min(v, dpp_mov_u32<0xB1>(v));
    v = min(v, dpp_mov_u32<0x4E>(v));
    v = min(v, dpp_mov_u32<0x141>(v));
    v = min(v, dpp_mov_u32<0x140>(v));
    return min(min(lane_u32(v, 0), lane_u32(v, 16)), min(lane_u32(v, 32), lane_u32(v, 48)));
}

// the last group g of 0 .. nq - 1 with offsets[g] <= j (offsets[0] is taken as 0 and never read); reads offsets[1 .. nq - 1] only
__device__ __forceinline__ uint32_t group_of(const int64_t* offsets, uint32_t nq, uint32_t j) {
    uint32_t lo = 0, hi = nq - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= (int64_t)j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the documents lo .. hi - 1 and the P positives of group g; false for a group that takes no part. Reads no score.
__device__ __forceinline__ bool group_range(const int64_t* offsets, const int32_t* num_pos, uint32_t g, uint32_t nd,
                                            uint32_t& lo, uint32_t& hi, uint32_t& P) {
    const int64_t a = offsets[g], b = offsets[g + 1];
    const int64_t p = num_pos[g];
    if (!(a >= 0 && a < b && b <= (int64_t)nd && p >= 1 && p < b - a)) return false;
    lo = (uint32_t)a; hi = (uint32_t)b; P = (uint32_t)p;
    return true;
}

// ---- scores
// A wave takes kRows consecutive documents and keeps their rows in flight together: the loads of all of them are issued
// before the first product. Every document's sums are its own and in the order of a one-document walk.
constexpr int kRows = 4;

template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void rr_scores_kernel(const float* queries, const float* docs, const int64_t* offsets,
                                                        uint32_t nq, uint32_t nd, int dim, float* scores) {
    const uint32_t j0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * 4u + (threadIdx.x >> 6)) * kRows));
    if (j0 >= nd) return;
    const int lane = threadIdx.x & 63;
    const float* q[kRows];
    const float* d[kRows];
    uint32_t g = group_of(offsets, nq, j0);
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const uint32_t j = min(j0 + r, nd - 1);                 // past the end: the last document again, never stored
        if (r > 0 && g + 1 < nq && offsets[g + 1] <= (int64_t)j) g = group_of(offsets, nq, j);      // the next group begins
        q[r] = queries + (size_t)g * dim;
        d[r] = docs + (size_t)j * dim;
    }
    float dot[kRows] = {}, qq[kRows] = {}, dd[kRows] = {};      // euclid: dot holds the sum of the squared differences
    auto step = [&](int r, float x, float y) {
        if (MODE == QST_SCORE_EUCLID) {
            const float t = x - y;
            dot[r] = fmaf(t, t, dot[r]);
        } else {
            dot[r] = fmaf(x, y, dot[r]);
            if (MODE == QST_SCORE_COS) { qq[r] = fmaf(x, x, qq[r]); dd[r] = fmaf(y, y, dd[r]); }
        }
    };
    if (VEC) {
        for (int i = lane; i < dim / 4; i += 64) {
            float4 x[kRows], y[kRows];
#pragma unroll
            for (int r = 0; r < kRows; ++r) { x[r] = ((const float4*)q[r])[i]; y[r] = ((const float4*)d[r])[i]; }
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                step(r, x[r].x, y[r].x); step(r, x[r].y, y[r].y); step(r, x[r].z, y[r].z); step(r, x[r].w, y[r].w);
            }
        }
    } else {
        for (int i = lane; i < dim; i += 64) {
            float x[kRows], y[kRows];
#pragma unroll
            for (int r = 0; r < kRows; ++r) { x[r] = q[r][i]; y[r] = d[r][i]; }
#pragma unroll
            for (int r = 0; r < kRows; ++r) step(r, x[r], y[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        float v = wave_sum(dot[r]);
        if (MODE == QST_SCORE_COS) v = v / (fmaxf(sqrtf(wave_sum(qq[r])), 1e-12f) * fmaxf(sqrtf(wave_sum(dd[r])), 1e-12f));
        else if (MODE == QST_SCORE_EUCLID) v = 1.f / (1.f + sqrtf(v));
        if (lane == 0 && j0 + r < nd) scores[j0 + r] = v;
    }
}

template <int MODE>
void launch_scores(bool vec, const float* queries, const float* docs, const int64_t* offsets, uint32_t nq, uint32_t nd, int dim,
                   float* scores, hipStream_t st) {
    const uint32_t grid = (uint32_t)(((int64_t)nd + 4 * kRows - 1) / (4 * kRows));
    if (vec) rr_scores_kernel<MODE, true><<<grid, 256, 0, st>>>(queries, docs, offsets, nq, nd, dim, scores);
    else rr_scores_kernel<MODE, false><<<grid, 256, 0, st>>>(queries, docs, offsets, nq, nd, dim, scores);
}

// ---- count: the record of every positive of a valid group, at the document's own index
// A wave takes 64 consecutive documents: every lane finds the group of its own and whether it is a positive of a valid group
// (most are not, and cost one search), then the whole wave walks the scores of each positive's group in turn.
__global__ __launch_bounds__(256) void rr_count_kernel(const float* scores, const int64_t* offsets, const int32_t* num_pos,
                                                       uint32_t nq, uint32_t nd, uint4* records) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t j0 = blockIdx.x * 256u + (threadIdx.x & ~63u);
    if (j0 >= nd) return;                       // the whole wave
    const uint32_t mine = j0 + lane;
    uint32_t lo = 0, hi = 0, P = 0;
    bool positive = false;
    if (mine < nd && group_range(offsets, num_pos, group_of(offsets, nq, mine), nd, lo, hi, P))
        positive = mine >= lo && mine - lo < P; // not a negative (or, with offsets out of order, another group's document)
    for (uint64_t todo = __ballot(positive); todo != 0; todo &= todo - 1) {
        const int src = __ffsll((unsigned long long)todo) - 1;
        const uint32_t j = j0 + (uint32_t)src;
        const uint32_t glo = __shfl(lo, src), ghi = __shfl(hi, src), gP = __shfl(P, src);
        const float sp = scores[j];
        const bool first = j == glo;            // the group's first positive also counts its non-finite scores
        uint32_t before = 0, ge_all = 0, ge_pos = 0, bad = 0;
        for (uint32_t d = glo + lane; d < ghi; d += 64) {
            const float sd = scores[d];
            before += (sd > sp || (sd == sp && d < j)) ? 1u : 0u;
            const bool ge = sd >= sp;
            ge_all += ge ? 1u : 0u;
            ge_pos += (ge && d - glo < gP) ? 1u : 0u;
            if (first) bad += (fabsf(sd) <= 3.402823466e+38f) ? 0u : 1u;
        }
        before = wave_sum_u32(before);
        ge_all = wave_sum_u32(ge_all);
        ge_pos = wave_sum_u32(ge_pos);
        bad = wave_sum_u32(bad);
        if (lane == 0) records[j] = make_uint4(before + 1u, ge_pos, ge_all, bad);
    }
}

// ---- finish: {rr, ap, ndcg} of a query from the records of its positives
__global__ __launch_bounds__(256) void rr_finish_kernel(const uint4* records, const int64_t* offsets, const int32_t* num_pos,
                                                        uint32_t nd, uint32_t k, double* per_query, uint32_t* info) {
    __shared__ double s_ap[256], s_dcg[256];
    __shared__ uint32_t s_min[4];
    const uint32_t g = blockIdx.x;
    const int t = threadIdx.x;
    uint32_t lo, hi, P;
    if (!group_range(offsets, num_pos, g, nd, lo, hi, P)) {     // uniform over the workgroup
        if (t < 3) per_query[(size_t)g * 3 + t] = 0.0;
        if (t == 0) info[g] = kInvalid;
        return;
    }
    uint32_t best = 0xFFFFFFFFu;
    double ap = 0.0, dcg = 0.0, ideal = 0.0;    // thread 0's
    for (uint32_t p0 = 0; p0 < P; p0 += 256) {
        const uint32_t p = p0 + t;
        double a = 0.0, c = 0.0;
        if (p < P) {
            const uint4 R = records[lo + p];
            best = min(best, R.x);
            a = (double)R.y / (double)R.z;
            if (R.x <= k) c = 1.0 / log2(1.0 + (double)R.x);
        }
        __syncthreads();
        s_ap[t] = a; s_dcg[t] = c;
        __syncthreads();
        if (t == 0) {
            const int m = (int)min(256u, P - p0);
            for (int i = 0; i < m; ++i) { ap += s_ap[i]; dcg += s_dcg[i]; }
        }
    }
    const uint32_t top = min(P, k);
    for (uint32_t i0 = 0; i0 < top; i0 += 256) {                // the best a ranking can do: the positives at places 1 .. top
        const uint32_t i = i0 + t;
        __syncthreads();
        s_dcg[t] = i < top ? 1.0 / log2(2.0 + (double)i) : 0.0;
        __syncthreads();
        if (t == 0) {
            const int m = (int)min(256u, top - i0);
            for (int n = 0; n < m; ++n) ideal += s_dcg[n];
        }
    }
    best = wave_min_u32(best);
    if ((t & 63) == 0) s_min[t >> 6] = best;
    __syncthreads();
    if (t != 0) return;
    best = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
    double* o = per_query + (size_t)g * 3;
    o[0] = best <= k ? 1.0 / (double)best : 0.0;
    o[1] = ap / (double)P;
    o[2] = dcg / ideal;
    info[g] = records[lo].w;
}

// ---- means over the valid groups, and the two counts
__global__ __launch_bounds__(1024) void rr_means_kernel(const double* per_query, const uint32_t* info, uint32_t nq, double* out) {
    __shared__ double part[5][16];
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // sums of rr, ap, ndcg; non-finite scores; invalid groups
    for (int64_t g = threadIdx.x; g < nq; g += 1024) {
        const uint32_t w = info[g];
        if (w & kInvalid) { v[4] += 1.0; continue; }
        v[0] += per_query[g * 3]; v[1] += per_query[g * 3 + 1]; v[2] += per_query[g * 3 + 2];
        v[3] += (double)w;
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        v[c] = wave_sum_f64(v[c]);
        if ((threadIdx.x & 63) == 0) part[c][threadIdx.x >> 6] = v[c];
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
#pragma unroll
    for (int c = 0; c < 5; ++c) v[c] = wave_sum_f64(threadIdx.x < 16 ? part[c][threadIdx.x] : 0.0);
    if (threadIdx.x != 0) return;
    const double valid = (double)nq - v[4];
    for (int c = 0; c < 3; ++c) out[c] = valid > 0.0 ? v[c] / valid : 0.0;
    out[3] = v[3];
    out[4] = v[4];
}

}  // namespace

extern "C" int qst_rerank_scores(const float* queries, const float* docs, const int64_t* offsets, int64_t nq, int64_t nd,
                                 int dim, int mode, float* scores, void* stream) {
    if (!queries || !docs || !offsets || !scores || nq < 1 || nd < 2 || dim < 1) return QST_ERR_BAD_ARG;
    if (mode != QST_SCORE_DOT && mode != QST_SCORE_COS && mode != QST_SCORE_EUCLID) return QST_ERR_BAD_ARG;
    if (((uintptr_t)queries & 3) || ((uintptr_t)docs & 3) || ((uintptr_t)scores & 3) || ((uintptr_t)offsets & 7)) return QST_ERR_BAD_ARG;
    if (nd >= kMaxCount || nq >= kMaxCount) return QST_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = dim % 4 == 0 && al16(queries) && al16(docs);       // then every row starts on 16 bytes
    const uint32_t NQ = (uint32_t)nq, ND = (uint32_t)nd;
    if (mode == QST_SCORE_COS) launch_scores<QST_SCORE_COS>(vec, queries, docs, offsets, NQ, ND, dim, scores, st);
    else if (mode == QST_SCORE_DOT) launch_scores<QST_SCORE_DOT>(vec, queries, docs, offsets, NQ, ND, dim, scores, st);
    else launch_scores<QST_SCORE_EUCLID>(vec, queries, docs, offsets, NQ, ND, dim, scores, st);
    QST_LAUNCH_CHECK();
    return QST_OK;
}

extern "C" size_t qst_rerank_workspace_bytes(int64_t nq, int64_t nd) {
    if (nq < 1 || nd < 2 || nq >= kMaxCount || nd >= kMaxCount) return 0;
    return records_bytes(nd) + info_bytes(nq);
}

extern "C" int qst_rerank_metrics(const float* scores, const int64_t* offsets, const int32_t* num_pos, int64_t nq, int64_t nd,
                                  int k, double* per_query, double* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!scores || !offsets || !num_pos || !per_query || !out || !workspace || nq < 1 || nd < 2 || k < 1) return QST_ERR_BAD_ARG;
    if (((uintptr_t)scores & 3) || ((uintptr_t)offsets & 7) || ((uintptr_t)num_pos & 3) || ((uintptr_t)per_query & 7) ||
        ((uintptr_t)out & 7) || !al16(workspace))
        return QST_ERR_BAD_ARG;
    if (nd >= kMaxCount || nq >= kMaxCount) return QST_ERR_UNSUPPORTED;
    if (workspace_bytes < qst_rerank_workspace_bytes(nq, nd)) return QST_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    uint4* records = (uint4*)workspace;
    uint32_t* info = (uint32_t*)((char*)workspace + records_bytes(nd));
    const uint32_t NQ = (uint32_t)nq, ND = (uint32_t)nd;
    rr_count_kernel<<<(uint32_t)((nd + 255) / 256), 256, 0, st>>>(scores, offsets, num_pos, NQ, ND, records);
    QST_LAUNCH_CHECK();
    rr_finish_kernel<<<NQ, 256, 0, st>>>(records, offsets, num_pos, ND, (uint32_t)k, per_query, info);
    QST_LAUNCH_CHECK();
    rr_means_kernel<<<1, 1024, 0, st>>>(per_query, info, NQ, out);
    QST_LAUNCH_CHECK();
    return QST_OK;
}
