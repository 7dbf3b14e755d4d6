// retrieval.hip -- similarity scoring + top-k for the encode()-driven evaluators.
//
// Replaces the device part of sentence-transformers' InformationRetrievalEvaluator.compute_metrices (2.2.2,
// third-party; reference call sites /root/reference/models/evaluators.py:572-588 and
// /root/reference/ir_evauation_script.py:107-131): for every corpus chunk, score_function(query_emb, chunk_emb)
// (util.cos_sim = normalise both sides, then a matmul; util.dot_score = matmul) followed by torch.topk(k, dim=1,
// largest=True, sorted=False) and a host-side merge of the per-chunk results.
//
// Here: rows are normalised (cosine) or copied into a 4-row-padded workspace, the [nq, nc] score matrix comes from the
// split-bf16 x3 GEMM (fp32-class products: near-ties keep the order an fp32 matmul would give them), and one
// workgroup per query selects the k best by a radix select on integer keys, then sorts them on those keys.
//
// qst_topk_stream does the same chunk by chunk for a corpus of any size: each chunk's score block is merged into a
// running [nq, k] result by topk_merge_kernel. Both kernels share one selection (topk_select_sort_store) and one order:
// a NaN of either sign first, then score descending with -0.0 = +0.0, then id ascending -- also among the entries tied
// at the k-th place, so neither wave scheduling nor the chunking shows in a result.
//
// qst_community_* (at the end of the file) are sentence-transformers 2.2.2's util.community_detection on the same panels:
// a count per row, the members of the rows that are asked for, and the greedy claim -- no n x n matrix, no top-k.
#include "qst_common.h"
#include "qst_kernels.h"

namespace {

// L2-normalise rows (torch.nn.functional.normalize(p=2, dim=1, eps=1e-12)) or copy them; rows >= n are zero-filled.
__global__ __launch_bounds__(256) void prep_rows_kernel(const float* x, int n, int n_pad, int dim, int normalize, float* y) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_pad) return;
    float* dst = y + (size_t)row * dim;
    if (row >= n) {
        for (int c = lane; c < dim; c += 64) dst[c] = 0.f;
        return;
    }
    const float* src = x + (size_t)row * dim;
    float inv = 1.f;
    if (normalize) {
        float s = 0.f;
        for (int c = lane; c < dim; c += 64) { const float v = src[c]; s += v * v; }
        inv = 1.f / fmaxf(sqrtf(wave_sum(s)), 1e-12f);
    }
    for (int c = lane; c < dim; c += 64) dst[c] = src[c] * inv;
}

// The one order of every top-k here, as an integer key (larger key ranks first): every NaN, of either sign and any
// payload, is the top key 0xFFFFFFFF (above +inf, where torch.topk ranks it); -0.0 and +0.0 share the key of +0.0; the
// rest is numeric. A negative float is the two's complement of its bits (0x80000000 - magnitude), which puts -0.0 on
// +0.0's key at no cost; the keys run from 0x00800000 (-inf) to 0xFF800000 (+inf). This sits in the inner loop of every
// pass of both kernels: a handful of VALU instructions per element, and the time shows each one. No float is compared
// after this point.
__device__ __forceinline__ uint32_t fkey(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    const uint32_t key = (u & 0x80000000u) ? 0u - u : (u | 0x80000000u);
    return v != v ? 0xFFFFFFFFu : key;
}

// the score of a key: a NaN (0x7FFFFFFF) for the top key, +0.0 for the zeros' key, otherwise the bits that went in
__device__ __forceinline__ float fkey_inv(uint32_t key) {
    return __builtin_bit_cast(float, (key & 0x80000000u) ? (key ^ 0x80000000u) : 0u - key);
}

constexpr int TOPK_MAX = 1024;

// What both top-k kernels do once they can enumerate a row's candidates: select the k best by the composite key
// (fkey(score), id ascending), sort them, store them. `visit(f)` calls f(key, id) for every candidate of this thread
// and must enumerate the same candidates each time it is called. An id is ranked by its offset from idbase, which is
// at most id_passes bytes wide; INT64_MAX is not an id (it marks an empty slot).
//
// The radix select runs over all of the composite key: four 8-bit passes over the score key, then passes over the id
// offset's bytes from the top one down, with the digit inverted so that the smaller id is the larger digit. It stops at
// the first pass whose chosen bin holds exactly what is still needed -- for distinct scores at the cut that is pass 4 at
// the latest, so the id passes run only when equal scores straddle the cut, and then they decide it by id however many
// the ties are. The chosen set therefore does not depend on atomic arrival order; the bitonic sort, on the integer keys
// (descending key, ascending id, empty slots last), orders it. Fewer than k candidates leave a tail of -inf / -1.
//
// LDS: 4 KB keys + 8 KB ids + the 1 KB histogram. out_* are written only after the sort.
template <class Visit>
__device__ __forceinline__ void topk_select_sort_store(Visit&& visit, uint64_t idbase, int id_passes, int k, float* rs,
                                                       int64_t* rx) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sh_digit, sh_need, sh_state, sh_cnt;
    __shared__ uint32_t sk[TOPK_MAX];
    __shared__ int64_t si[TOPK_MAX];
    const int tid = threadIdx.x;

    // after the passes: a candidate is taken iff (key & kmask) > kprefix, or equal with (offset & imask) <= iprefix
    uint32_t kprefix = 0, kmask = 0, need = (uint32_t)k;
    uint64_t iprefix = 0, imask = 0;
    for (int pass = 0; pass < 4 + id_passes; ++pass) {
        const bool on_key = pass < 4;
        const int shift = on_key ? 24 - 8 * pass : 8 * (id_passes - 1 - (pass - 4));
        hist[tid] = 0;
        __syncthreads();
        visit([&](uint32_t key, int64_t id) {
            const uint64_t off = (uint64_t)id - idbase;
            if ((key & kmask) != kprefix || (off & imask) != iprefix) return;
            const uint32_t d = on_key ? (key >> shift) & 255u : 255u - (uint32_t)((off >> shift) & 255u);
            atomicAdd(&hist[d], 1u);
        });
        __syncthreads();
        if (tid == 0) {
            uint32_t acc = 0;
            int d = 255;
            for (; d >= 0; --d) {
                if (acc + hist[d] >= need) break;
                acc += hist[d];
            }
            // d < 0: fewer than `need` candidates in all (only on pass 0): every one is taken
            sh_state = d < 0 ? 2u : (acc + hist[d] == need ? 1u : 0u);
            sh_digit = (uint32_t)(d < 0 ? 0 : d);
            sh_need = need - acc;
        }
        __syncthreads();
        const uint32_t state = sh_state, d = sh_digit;
        need = sh_need;
        if (state == 2u) break;                            // masks still zero: the rule above takes everything
        if (on_key) { kprefix |= d << shift; kmask |= 255u << shift; }
        else { iprefix |= (uint64_t)(255u - d) << shift; imask |= (uint64_t)255u << shift; }
        if (state == 1u) break;                            // the bin is taken whole: nothing left to decide
    }

    const int kp = k <= 1 ? 1 : 1 << (32 - __builtin_clz((unsigned)(k - 1)));     // next power of two
    if (tid == 0) sh_cnt = 0;
    for (int i = tid; i < kp; i += 256) { sk[i] = 0u; si[i] = INT64_MAX; }
    __syncthreads();
    visit([&](uint32_t key, int64_t id) {
        const uint32_t hi = key & kmask;
        if (hi > kprefix || (hi == kprefix && (((uint64_t)id - idbase) & imask) <= iprefix)) {
            const uint32_t pos = atomicAdd(&sh_cnt, 1u);
            if (pos < (uint32_t)k) { sk[pos] = key; si[pos] = id; }     // more than k only if an id came in twice
        }
    });
    __syncthreads();
    // bitonic sort of kp entries: descending key, ascending id among equal keys; empty slots (id INT64_MAX) go last
    for (int size = 2; size <= kp; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (kp >> 1); t += 256) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                const uint32_t a = sk[lo], b = sk[hi];
                const int64_t ia = si[lo], ib = si[hi];
                const bool ea = ia == INT64_MAX, eb = ib == INT64_MAX;
                const bool a_first = ea != eb ? eb : (a > b) || (a == b && ia < ib);       // a ranks before b
                if (desc ? !a_first : a_first) { sk[lo] = b; sk[hi] = a; si[lo] = ib; si[hi] = ia; }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < k; i += 256) {
        const bool empty = si[i] == INT64_MAX;
        rs[i] = empty ? -INFINITY : fkey_inv(sk[i]);
        rx[i] = empty ? -1 : si[i];
    }
}

// k best of every row of a score matrix: one workgroup per row. The candidates are the row's n scores that are not above
// cap (the "not too similar" filter of negative mining; +inf = plain top-k; a NaN is not above anything), each with its
// column or its index_map entry as id. Ids are ranked by their offset from the row's smallest one, so any int64 below
// INT64_MAX may be an id; without an index_map the span is n - 1 and nothing is scanned for it.
__global__ __launch_bounds__(256) void topk_rows_kernel(const float* scores, int64_t ld, const int64_t* index_map, int n,
                                                        int k, float cap, float* out_scores, int64_t* out_index) {
    __shared__ unsigned long long sh_ext;
    const int tid = threadIdx.x;
    const float* row = scores + (size_t)blockIdx.x * ld;
    const int64_t* imap = index_map ? index_map + (size_t)blockIdx.x * ld : nullptr;

    uint64_t idbase = 0, span = (uint64_t)(n - 1);
    if (imap) {                                             // (uniform)
        constexpr uint64_t kBias = 1ull << 63;              // signed order as unsigned order
        uint64_t lo = ~0ull, hi = 0ull;
        for (int i = tid; i < n; i += 256) {
            const uint64_t u = (uint64_t)imap[i] ^ kBias;
            lo = u < lo ? u : lo;
            hi = u > hi ? u : hi;
        }
        // one LDS word serves both reductions (the minimum as the maximum of the complement): no more LDS than the merge
        if (tid == 0) sh_ext = 0ull;
        __syncthreads();
        if (tid < n) atomicMax(&sh_ext, (unsigned long long)hi);
        __syncthreads();
        hi = sh_ext;
        __syncthreads();
        if (tid == 0) sh_ext = 0ull;
        __syncthreads();
        if (tid < n) atomicMax(&sh_ext, (unsigned long long)~lo);
        __syncthreads();
        lo = ~(uint64_t)sh_ext;
        idbase = lo ^ kBias;
        span = hi - lo;
    }
    const int id_passes = (64 - __builtin_clzll(span | 1ull) + 7) / 8;

    auto visit = [&](auto&& f) {
        for (int i = tid; i < n; i += 256) {
            const float v = row[i];
            if (!(v > cap)) f(fkey(v), imap ? imap[i] : (int64_t)i);
        }
    };
    topk_select_sort_store(visit, idbase, id_passes, k, out_scores + (size_t)blockIdx.x * k,
                           out_index + (size_t)blockIdx.x * k);
}

// Merge one chunk's scores into a running top-k: one workgroup per row. The candidates are the n scores of the row (global
// id col_base + column) and the k entries of run_* (index -1 = empty). A candidate takes part unless its id is negative,
// is the row's own (exclude_self) or its score is above cap. The k best by (score descending, id ascending) go back to
// run_*, real entries first, then -inf / -1.
//
// Selection and sort are topk_select_sort_store's, over ids counted from 0 (the id passes start at the top non-zero byte
// of the largest id): the chosen set does not depend on atomic arrival order or on how the columns were cut into chunks.
//
// The old running row lives in registers (k <= 1024 = 4 per thread) from before the first barrier; run_* is written only
// after the sort.
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* scores, int64_t ld, int n, int64_t col_base,
                                                         int64_t row_base, int exclude_self, float cap, int k,
                                                         float* run_scores, int64_t* run_index) {
    __shared__ unsigned long long sh_idmax;
    const int tid = threadIdx.x;
    const float* row = scores + (size_t)blockIdx.x * ld;
    float* rs = run_scores + (size_t)blockIdx.x * k;
    int64_t* rx = run_index + (size_t)blockIdx.x * k;
    const int64_t self = exclude_self ? row_base + blockIdx.x : -1;     // -1: no id equals it (negative ids are empty)

    float rv[4];
    int64_t ri[4];
    int64_t idmax = col_base + n - 1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = tid + 256 * e;
        rv[e] = j < k ? rs[j] : -INFINITY;
        ri[e] = j < k ? rx[j] : -1;
        idmax = ri[e] > idmax ? ri[e] : idmax;
    }
    if (tid == 0) sh_idmax = 0;
    __syncthreads();
    atomicMax(&sh_idmax, (unsigned long long)idmax);
    __syncthreads();
    const int id_passes = (64 - __builtin_clzll(sh_idmax | 1ull) + 7) / 8;

    // f(key, id) for every candidate of this thread that takes part
    auto visit = [&](auto&& f) {
        for (int i = tid; i < n; i += 256) {
            const float v = row[i];
            const int64_t id = col_base + i;
            if (id != self && !(v > cap)) f(fkey(v), id);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (ri[e] >= 0 && ri[e] != self && !(rv[e] > cap)) f(fkey(rv[e]), ri[e]);
    };
    topk_select_sort_store(visit, 0ull, id_passes, k, rs, rx);
}

// Euclidean score 1 / (1 + ||q - c||_2): the reference's own third score function (models/evaluators.py:392-405,
// `1 / (1 + torch.cdist(a, b, p=2))`, passed as score_functions['euclid_score'] by training/main.py:57 and
// ir_evauation_script.py:71). Distances are summed from the differences themselves (an fp32 FMA chain per pair): the
// |q|^2 + |c|^2 - 2 q.c form loses the distance of near-duplicates to cancellation, and those are the pairs that decide
// a ranking. 64 x 64 pairs per workgroup, 4 x 4 per thread, 32-dimension slabs staged transposed ([dim][row]) so that a
// thread's four rows are one 16-byte LDS read. VALU-bound: 2 instructions per pair and dimension.
__global__ __launch_bounds__(256) void euclid_scores_kernel(const float* q, const float* c, int nq, int nc, int dim,
                                                            float* out, int ldo) {
    __shared__ __attribute__((aligned(16))) float qs[32][68];
    __shared__ __attribute__((aligned(16))) float cs[32][68];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int q0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int lrow = tid >> 2, lk = (tid & 3) * 8;          // staging: row lrow, dims lk .. lk+7 of the slab
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int k0 = 0; k0 < dim; k0 += 32) {
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, b0 = a0, b1 = a0;
        if (q0 + lrow < nq) {
            a0 = *(const f32x4*)(q + (size_t)(q0 + lrow) * dim + k0 + lk);
            a1 = *(const f32x4*)(q + (size_t)(q0 + lrow) * dim + k0 + lk + 4);
        }
        if (c0 + lrow < nc) {
            b0 = *(const f32x4*)(c + (size_t)(c0 + lrow) * dim + k0 + lk);
            b1 = *(const f32x4*)(c + (size_t)(c0 + lrow) * dim + k0 + lk + 4);
        }
        __syncthreads();                                    // the previous slab's readers are done
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            qs[lk + e][lrow] = a0[e]; qs[lk + 4 + e][lrow] = a1[e];
            cs[lk + e][lrow] = b0[e]; cs[lk + 4 + e][lrow] = b1[e];
        }
        __syncthreads();
#pragma unroll 8
        for (int d = 0; d < 32; ++d) {
            const f32x4 a = *(const f32x4*)(&qs[d][ty * 4]);
            const f32x4 b = *(const f32x4*)(&cs[d][tx * 4]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float df = a[i] - b[j];
                    acc[i][j] = fmaf(df, df, acc[i][j]);
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int qi = q0 + ty * 4 + i;
        if (qi >= nq) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cj = c0 + tx * 4 + j;
            if (cj < ldo) out[(size_t)qi * ldo + cj] = cj < nc ? 1.f / (1.f + sqrtf(acc[i][j])) : 0.f;
        }
    }
}

constexpr int kQueryBlock = 2048;        // score matrix rows per GEMM launch (keeps byte offsets inside 32 bits)

inline size_t pad4(size_t n) { return (n + 3) / 4 * 4; }

}  // namespace

extern "C" int qst_topk_rows(const float* scores, int64_t ld, const int64_t* index_map, int nrows, int n, int k,
                             float* out_scores, int64_t* out_index, void* stream) {
    if (!scores || !out_scores || !out_index || nrows <= 0 || n <= 0 || k <= 0 || ld < n) return QST_ERR_BAD_ARG;
    if (k > n || k > TOPK_MAX) return QST_ERR_UNSUPPORTED;
    topk_rows_kernel<<<nrows, 256, 0, (hipStream_t)stream>>>(scores, ld, index_map, n, k, INFINITY, out_scores, out_index);
    QST_LAUNCH_CHECK();
    return QST_OK;
}

extern "C" size_t qst_topk_workspace_bytes(int nq, int nc, int dim) {
    if (nq <= 0 || nc <= 0 || dim <= 0) return 0;
    const size_t qrows = pad4((size_t)(nq < kQueryBlock ? nq : kQueryBlock));
    return (pad4((size_t)nq) + pad4((size_t)nc)) * dim * sizeof(float) + qrows * pad4((size_t)nc) * sizeof(float) + 1024;
}

static int topk_scores_impl(const float* queries, const float* corpus, int nq, int nc, int dim, int k, int mode, float cap,
                            float* out_scores, int64_t* out_index, void* workspace, size_t workspace_bytes, void* stream);

extern "C" int qst_topk_scores(const float* queries, const float* corpus, int nq, int nc, int dim, int k, int mode,
                               float* out_scores, int64_t* out_index, void* workspace, size_t workspace_bytes,
                               void* stream) {
    return topk_scores_impl(queries, corpus, nq, nc, dim, k, mode, INFINITY, out_scores, out_index, workspace,
                            workspace_bytes, stream);
}

extern "C" int qst_topk_scores_capped(const float* queries, const float* corpus, int nq, int nc, int dim, int k, int mode,
                                      float max_score, float* out_scores, int64_t* out_index, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    if (max_score != max_score) return QST_ERR_BAD_ARG;
    return topk_scores_impl(queries, corpus, nq, nc, dim, k, mode, max_score, out_scores, out_index, workspace,
                            workspace_bytes, stream);
}

// scores of query rows [q0, q0 + rows) against the whole corpus into sc [rows, ncp]; qn / cn = prepared operands
static int score_block(const float* qn, const float* cn, int rows, int nc, int ncp, int dim, int mode, float* sc,
                       hipStream_t st) {
    if (mode == QST_SCORE_EUCLID) {
        euclid_scores_kernel<<<dim3((ncp + 63) / 64, (rows + 63) / 64), 256, 0, st>>>(qn, cn, rows, nc, dim, sc, ncp);
        QST_LAUNCH_CHECK();
        return QST_OK;
    }
    QstGemmArgs g{};
    g.A = qn; g.B = cn; g.C = sc;
    g.M = rows; g.N = ncp; g.K = dim; g.lda = dim; g.ldb = dim; g.ldc = ncp;
    return qst_gemm_nt_x3(&g, 0, st);
}

// a null side is left alone (the streaming path prepares the queries once and then one corpus chunk at a time)
static int prep_operands(const float* queries, const float* corpus, int nq, int nc, int dim, int mode, float* qn, float* cn,
                         hipStream_t st) {
    const int nqp = (int)pad4(nq), ncp = (int)pad4(nc);
    if (queries) {
        prep_rows_kernel<<<(nqp + 3) / 4, 256, 0, st>>>(queries, nq, nqp, dim, mode == QST_SCORE_COS, qn);
        QST_LAUNCH_CHECK();
    }
    if (corpus) {
        prep_rows_kernel<<<(ncp + 3) / 4, 256, 0, st>>>(corpus, nc, ncp, dim, mode == QST_SCORE_COS, cn);
        QST_LAUNCH_CHECK();
    }
    return QST_OK;
}

static int topk_scores_impl(const float* queries, const float* corpus, int nq, int nc, int dim, int k, int mode, float cap,
                            float* out_scores, int64_t* out_index, void* workspace, size_t workspace_bytes, void* stream) {
    if (!queries || !corpus || !out_scores || !out_index || !workspace || nq <= 0 || nc <= 0 || dim <= 0 || k <= 0)
        return QST_ERR_BAD_ARG;
    if (mode != QST_SCORE_DOT && mode != QST_SCORE_COS && mode != QST_SCORE_EUCLID) return QST_ERR_BAD_ARG;
    if (k > nc || k > TOPK_MAX || dim % 32 != 0) return QST_ERR_UNSUPPORTED;
    if (workspace_bytes < qst_topk_workspace_bytes(nq, nc, dim)) return QST_ERR_WORKSPACE;
    if ((int64_t)pad4(nc) * dim * 4 >= 0x7FFFFF00LL) return QST_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int nqp = (int)pad4(nq), ncp = (int)pad4(nc);
    float* qn = (float*)workspace;
    float* cn = qn + (size_t)nqp * dim;
    float* sc = cn + (size_t)ncp * dim;
    int rc = prep_operands(queries, corpus, nq, nc, dim, mode, qn, cn, st);
    if (rc != QST_OK) return rc;
    for (int q0 = 0; q0 < nq; q0 += kQueryBlock) {
        const int rows = nq - q0 < kQueryBlock ? nq - q0 : kQueryBlock;
        rc = score_block(qn + (size_t)q0 * dim, cn, rows, nc, ncp, dim, mode, sc, st);
        if (rc != QST_OK) return rc;
        topk_rows_kernel<<<rows, 256, 0, st>>>(sc, ncp, nullptr, nc, k, cap, out_scores + (size_t)q0 * k,
                                               out_index + (size_t)q0 * k);
        QST_LAUNCH_CHECK();
    }
    return QST_OK;
}

extern "C" int qst_topk_merge_rows(const float* scores, int64_t ld, int nrows, int n, int64_t col_base, int64_t row_base,
                                   int exclude_self, float max_score, int k, float* run_scores, int64_t* run_index,
                                   void* stream) {
    if (!scores || !run_scores || !run_index || nrows <= 0 || n <= 0 || k <= 0 || ld < n) return QST_ERR_BAD_ARG;
    if (col_base < 0 || row_base < 0 || col_base > INT64_MAX - n || row_base > INT64_MAX - nrows) return QST_ERR_BAD_ARG;
    if (max_score != max_score) return QST_ERR_BAD_ARG;
    if (k > TOPK_MAX) return QST_ERR_UNSUPPORTED;
    topk_merge_kernel<<<nrows, 256, 0, (hipStream_t)stream>>>(scores, ld, n, col_base, row_base, exclude_self, max_score, k,
                                                              run_scores, run_index);
    QST_LAUNCH_CHECK();
    return QST_OK;
}

extern "C" size_t qst_topk_stream_workspace_bytes(int nq, int chunk, int dim) {
    return qst_topk_workspace_bytes(nq, chunk, dim);        // the same three parts, with one chunk in the corpus's place
}

extern "C" int qst_topk_stream(const float* queries, const float* corpus, int nq, int nc, int dim, int k, int mode, int chunk,
                               int64_t query_base, int64_t corpus_base, int exclude_self, float max_score,
                               float* run_scores, int64_t* run_index, void* workspace, size_t workspace_bytes,
                               void* stream) {
    if (!queries || !corpus || !run_scores || !run_index || !workspace || nq <= 0 || nc <= 0 || dim <= 0 || k <= 0 ||
        chunk <= 0)
        return QST_ERR_BAD_ARG;
    if (mode != QST_SCORE_DOT && mode != QST_SCORE_COS && mode != QST_SCORE_EUCLID) return QST_ERR_BAD_ARG;
    if (query_base < 0 || corpus_base < 0 || query_base > INT64_MAX - nq || corpus_base > INT64_MAX - nc)
        return QST_ERR_BAD_ARG;
    if (max_score != max_score) return QST_ERR_BAD_ARG;
    if (k > TOPK_MAX || dim % 32 != 0) return QST_ERR_UNSUPPORTED;
    if (chunk > nc) chunk = nc;
    if (workspace_bytes < qst_topk_stream_workspace_bytes(nq, chunk, dim)) return QST_ERR_WORKSPACE;
    if ((int64_t)pad4(chunk) * dim * 4 >= 0x7FFFFF00LL) return QST_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int nqp = (int)pad4(nq);
    float* qn = (float*)workspace;
    float* cn = qn + (size_t)nqp * dim;
    float* sc = cn + pad4(chunk) * dim;
    int rc = prep_operands(queries, nullptr, nq, 0, dim, mode, qn, nullptr, st);
    if (rc != QST_OK) return rc;
    for (int c0 = 0; c0 < nc; c0 += chunk) {
        const int cols = nc - c0 < chunk ? nc - c0 : chunk;
        const int colsp = (int)pad4(cols);
        rc = prep_operands(nullptr, corpus + (size_t)c0 * dim, 0, cols, dim, mode, nullptr, cn, st);
        if (rc != QST_OK) return rc;
        for (int q0 = 0; q0 < nq; q0 += kQueryBlock) {
            const int rows = nq - q0 < kQueryBlock ? nq - q0 : kQueryBlock;
            rc = score_block(qn + (size_t)q0 * dim, cn, rows, cols, colsp, dim, mode, sc, st);
            if (rc != QST_OK) return rc;
            topk_merge_kernel<<<rows, 256, 0, st>>>(sc, colsp, cols, corpus_base + c0, query_base + q0, exclude_self,
                                                    max_score, k, run_scores + (size_t)q0 * k, run_index + (size_t)q0 * k);
            QST_LAUNCH_CHECK();
        }
    }
    return QST_OK;
}

// The whole score matrix (sentence_transformers.util.cos_sim / dot_score and the reference's euclidean_score as
// functions): out f32 [nq, ld_out], ld_out = nc rounded up to a multiple of 4 (the pad columns are written too).
extern "C" size_t qst_score_workspace_bytes(int nq, int nc, int dim) {
    if (nq <= 0 || nc <= 0 || dim <= 0) return 0;
    return (pad4((size_t)nq) + pad4((size_t)nc)) * dim * sizeof(float) + 1024;
}
extern "C" int qst_score_matrix(const float* queries, const float* corpus, int nq, int nc, int dim, int mode, float* out,
                                int64_t ld_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!queries || !corpus || !out || !workspace || nq <= 0 || nc <= 0 || dim <= 0) return QST_ERR_BAD_ARG;
    if (mode != QST_SCORE_DOT && mode != QST_SCORE_COS && mode != QST_SCORE_EUCLID) return QST_ERR_BAD_ARG;
    if (dim % 32 != 0 || ld_out != (int64_t)pad4(nc)) return QST_ERR_UNSUPPORTED;
    if (workspace_bytes < qst_score_workspace_bytes(nq, nc, dim)) return QST_ERR_WORKSPACE;
    if ((int64_t)pad4(nc) * dim * 4 >= 0x7FFFFF00LL) return QST_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int nqp = (int)pad4(nq), ncp = (int)pad4(nc);
    float* qn = (float*)workspace;
    float* cn = qn + (size_t)nqp * dim;
    int rc = prep_operands(queries, corpus, nq, nc, dim, mode, qn, cn, st);
    if (rc != QST_OK) return rc;
    for (int q0 = 0; q0 < nq; q0 += kQueryBlock) {
        const int rows = nq - q0 < kQueryBlock ? nq - q0 : kQueryBlock;
        rc = score_block(qn + (size_t)q0 * dim, cn, rows, nc, ncp, dim, mode, out + (size_t)q0 * ncp, st);
        if (rc != QST_OK) return rc;
    }
    return QST_OK;
}

extern "C" int qst_normalize_rows(const float* x, int n, int dim, float* out, void* stream) {
    if (!x || !out || n <= 0 || dim <= 0) return QST_ERR_BAD_ARG;
    prep_rows_kernel<<<(n + 3) / 4, 256, 0, (hipStream_t)stream>>>(x, n, n, dim, 1, out);
    QST_LAUNCH_CHECK();
    return QST_OK;
}

// ---------------------------------------------------------------- community detection (ST 2.2.2 util.community_detection)
// What the clustering needs from the n x n cosine scores is a count per row and, for a few rows, the columns at or above
// the threshold: neither needs the matrix or a top-k. Both passes walk the same [2048 row block] x [chunk] panels through
// the same call (community_panel), so a score has the same bits in both and the member pass finds exactly what the count
// pass counted. The rows are their own corpus: a chunk's operand is a slice of the prepared rows, not a second copy.
namespace {

__device__ __forceinline__ int wave_sum_i32(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// counts[row] += number of the row's first `cols` scores that are >= thr (a NaN is not). One workgroup per row, 16-byte
// loads (the panel's rows are 16-byte aligned: ld % 4 == 0), one writer per row: launches on one stream need no atomics.
// self_member (nullable): the row's own column, when this panel holds it, leaves whether it passed.
__global__ __launch_bounds__(256) void count_ge_kernel(const float* sc, int64_t ld, int cols, float thr, int64_t row_base,
                                                       int64_t col_base, int32_t* counts, uint8_t* self_member) {
    __shared__ int part[4];
    const int tid = threadIdx.x;
    const float* row = sc + (size_t)blockIdx.x * ld;
    const int c4 = cols >> 2;
    int c = 0;
    for (int i = tid; i < c4; i += 256) {
        const f32x4 v = *(const f32x4*)(row + 4 * (size_t)i);
        c += (v[0] >= thr) + (v[1] >= thr) + (v[2] >= thr) + (v[3] >= thr);
    }
    for (int i = 4 * c4 + tid; i < cols; i += 256) c += row[i] >= thr;
    c = wave_sum_i32(c);
    if ((tid & 63) == 0) part[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        counts[blockIdx.x] += part[0] + part[1] + part[2] + part[3];
        const int64_t own = row_base + blockIdx.x - col_base;
        if (self_member && own >= 0 && own < cols) self_member[blockIdx.x] = row[own] >= thr ? 1 : 0;
    }
}

// The columns of one chunk that pass, appended to the row's slot in ascending column order: one workgroup per wanted row
// (begin >= 0), 256 columns a trip. Each wave ballots its 64 columns; a lane's place is the row's cursor + the counts of
// the waves before it (fixed wave order, through LDS) + the set bits below it. The cursor lives in written[row] between
// chunks. No atomics; nothing is stored at or past begin + capacity, but the cursor counts everything that passed.
__global__ __launch_bounds__(256) void compact_ge_kernel(const float* sc, int64_t ld, int cols, float thr, int32_t col_base,
                                                         const int64_t* begin, const int32_t* capacity, int32_t* out_index,
                                                         float* out_score, int32_t* written) {
    __shared__ int wc[2][4];                                // two sets: one barrier a trip is enough
    const int64_t b = begin[blockIdx.x];
    if (b < 0) return;                                      // (uniform)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = sc + (size_t)blockIdx.x * ld;
    const int cap = capacity[blockIdx.x];
    int cursor = written[blockIdx.x];
    int set = 0;
    for (int t0 = 0; t0 < cols; t0 += 256, set ^= 1) {
        const int col = t0 + tid;
        const float v = col < cols ? row[col] : 0.f;
        const bool ok = col < cols && v >= thr;
        const unsigned long long m = __ballot(ok);
        if (lane == 0) wc[set][wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int x = wc[set][w];
            total += x;
            before += w < wave ? x : 0;
        }
        if (ok) {
            const int pos = cursor + before + __popcll(m & ((1ull << lane) - 1ull));
            if (pos < cap) {
                out_index[b + pos] = col_base + col;
                out_score[b + pos] = v;
            }
        }
        cursor += total;
    }
    if (tid == 0) written[blockIdx.x] = cursor;            // every thread read it before the first barrier
}

// Greedy claim, in the given order, by ONE workgroup: candidate c is accepted when none of its members is taken, and then
// takes them all; the barrier between candidates makes its marks visible to the next one's reads.
__global__ __launch_bounds__(256) void claim_kernel(const int64_t* begin, const int32_t* len, int ncand, const int32_t* members,
                                                    int n, uint8_t* taken, uint8_t* accepted) {
    const int tid = threadIdx.x;
    for (int c = 0; c < ncand; ++c) {
        const int64_t b = begin[c];
        const int L = len[c];
        int clash = (b < 0 || L <= 0) ? 1 : 0;
        if (!clash)
            for (int i = tid; i < L; i += 256) {
                const int j = members[b + i];
                clash |= (j < 0 || j >= n) ? 1 : (int)taken[j];
            }
        clash = __syncthreads_or(clash);
        if (!clash)
            for (int i = tid; i < L; i += 256) taken[members[b + i]] = 1;
        if (tid == 0) accepted[c] = clash ? 0 : 1;
        __syncthreads();
    }
}

// out[p] = cosine of rows a[p] and b[p] in fp64 from the rows as given (norms clamped at 1e-12): one wave per pair.
__global__ __launch_bounds__(256) void pair_cos_f64_kernel(const float* x, int n, int dim, const int32_t* a, const int32_t* b,
                                                           int64_t count, double* out) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= count) return;
    const int ia = a[p], ib = b[p];
    if (ia < 0 || ia >= n || ib < 0 || ib >= n) {
        if (lane == 0) out[p] = __builtin_nan("");
        return;
    }
    const float* xa = x + (size_t)ia * dim;
    const float* xb = x + (size_t)ib * dim;
    double ab = 0.0, aa = 0.0, bb = 0.0;
    for (int c = lane; c < dim; c += 64) {
        const double u = xa[c], v = xb[c];
        ab += u * v; aa += u * u; bb += v * v;
    }
    ab = wave_sum_f64(ab); aa = wave_sum_f64(aa); bb = wave_sum_f64(bb);
    if (lane == 0) out[p] = ab / (fmax(sqrt(aa), 1e-12) * fmax(sqrt(bb), 1e-12));
}

// prepared rows: n rounded up to 4, plus 4 -- the last chunk's operand is read to 4 rows past its start + cols rounded up
inline size_t community_rows(int n) { return pad4((size_t)n) + 4; }

// argument checks shared by the two passes; `chunk` comes back clamped to n
int community_check(const float* emb, int n, int dim, float threshold, int& chunk, const void* ws, size_t ws_bytes) {
    if (!emb || !ws || n <= 0 || dim <= 0 || chunk <= 0 || threshold != threshold) return QST_ERR_BAD_ARG;
    if (dim % 32 != 0) return QST_ERR_UNSUPPORTED;
    if (chunk > n) chunk = n;
    if (ws_bytes < qst_community_workspace_bytes(n, chunk, dim)) return QST_ERR_WORKSPACE;
    if ((int64_t)pad4(chunk) * dim * 4 >= 0x7FFFFF00LL) return QST_ERR_UNSUPPORTED;
    return QST_OK;
}

// the one way either pass gets a panel: rows [r0, r0 + rows) against rows [c0, c0 + cols) of the prepared rows `en`
int community_panel(const float* en, int dim, int r0, int rows, int c0, int cols, float* sc, hipStream_t st) {
    return score_block(en + (size_t)r0 * dim, en + (size_t)c0 * dim, rows, cols, (int)pad4(cols), dim, QST_SCORE_COS, sc, st);
}

int community_prepare(const float* emb, int n, int dim, float* en, hipStream_t st) {
    const int np = (int)community_rows(n);
    prep_rows_kernel<<<(np + 3) / 4, 256, 0, st>>>(emb, n, np, dim, 1, en);
    QST_LAUNCH_CHECK();
    return QST_OK;
}

}  // namespace

extern "C" size_t qst_community_workspace_bytes(int n, int chunk, int dim) {
    if (n <= 0 || chunk <= 0 || dim <= 0) return 0;
    if (chunk > n) chunk = n;
    const size_t rows = (size_t)(n < kQueryBlock ? n : kQueryBlock);
    return (community_rows(n) * dim + rows * pad4((size_t)chunk)) * sizeof(float) + 1024;
}

extern "C" int qst_community_count(const float* emb, int n, int dim, float threshold, int chunk, int32_t* counts,
                                   uint8_t* self_member, void* workspace, size_t workspace_bytes, void* stream) {
    if (!counts) return QST_ERR_BAD_ARG;
    int rc = community_check(emb, n, dim, threshold, chunk, workspace, workspace_bytes);
    if (rc != QST_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* en = (float*)workspace;
    float* sc = en + community_rows(n) * dim;
    rc = community_prepare(emb, n, dim, en, st);
    if (rc != QST_OK) return rc;
    QST_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)n * sizeof(int32_t), st));
    if (self_member) QST_HIP_CHECK(hipMemsetAsync(self_member, 0, (size_t)n, st));
    for (int r0 = 0; r0 < n; r0 += kQueryBlock) {
        const int rows = n - r0 < kQueryBlock ? n - r0 : kQueryBlock;
        for (int c0 = 0; c0 < n; c0 += chunk) {
            const int cols = n - c0 < chunk ? n - c0 : chunk;
            rc = community_panel(en, dim, r0, rows, c0, cols, sc, st);
            if (rc != QST_OK) return rc;
            count_ge_kernel<<<rows, 256, 0, st>>>(sc, (int64_t)pad4(cols), cols, threshold, r0, c0, counts + r0,
                                                  self_member ? self_member + r0 : nullptr);
            QST_LAUNCH_CHECK();
        }
    }
    return QST_OK;
}

extern "C" int qst_community_members(const float* emb, int n, int dim, float threshold, int chunk, int row0,
                                     const int64_t* begin, const int32_t* capacity, int32_t* out_index, float* out_score,
                                     int32_t* written, void* workspace, size_t workspace_bytes, void* stream) {
    if (!begin || !capacity || !out_index || !out_score || !written) return QST_ERR_BAD_ARG;
    int rc = community_check(emb, n, dim, threshold, chunk, workspace, workspace_bytes);
    if (rc != QST_OK) return rc;
    if (row0 < 0 || row0 >= n || row0 % kQueryBlock != 0) return QST_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    float* en = (float*)workspace;
    float* sc = en + community_rows(n) * dim;
    rc = community_prepare(emb, n, dim, en, st);
    if (rc != QST_OK) return rc;
    const int rows = n - row0 < kQueryBlock ? n - row0 : kQueryBlock;
    QST_HIP_CHECK(hipMemsetAsync(written, 0, (size_t)rows * sizeof(int32_t), st));
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int cols = n - c0 < chunk ? n - c0 : chunk;
        rc = community_panel(en, dim, row0, rows, c0, cols, sc, st);
        if (rc != QST_OK) return rc;
        compact_ge_kernel<<<rows, 256, 0, st>>>(sc, (int64_t)pad4(cols), cols, threshold, c0, begin, capacity, out_index,
                                                out_score, written);
        QST_LAUNCH_CHECK();
    }
    return QST_OK;
}

extern "C" int qst_community_claim(const int64_t* begin, const int32_t* len, int ncand, const int32_t* members, int n,
                                   uint8_t* taken, uint8_t* accepted, void* stream) {
    if (ncand < 0 || n <= 0 || !taken) return QST_ERR_BAD_ARG;
    if (ncand == 0) return QST_OK;
    if (!begin || !len || !members || !accepted) return QST_ERR_BAD_ARG;
    claim_kernel<<<1, 256, 0, (hipStream_t)stream>>>(begin, len, ncand, members, n, taken, accepted);
    QST_LAUNCH_CHECK();
    return QST_OK;
}

extern "C" int qst_community_rescore(const float* emb, int n, int dim, const int32_t* rows_a, const int32_t* rows_b,
                                     int64_t count, double* out, void* stream) {
    if (!emb || n <= 0 || dim <= 0 || count < 0) return QST_ERR_BAD_ARG;
    if (count == 0) return QST_OK;
    if (!rows_a || !rows_b || !out) return QST_ERR_BAD_ARG;
    if ((count + 3) / 4 > 0x7FFFFFFFLL) return QST_ERR_UNSUPPORTED;
    pair_cos_f64_kernel<<<(unsigned)((count + 3) / 4), 256, 0, (hipStream_t)stream>>>(emb, n, dim, rows_a, rows_b, count, out);
    QST_LAUNCH_CHECK();
    return QST_OK;
}
