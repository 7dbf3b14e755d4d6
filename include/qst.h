/*
 * qst.h -- C-ABI of libqst.so: the MI355X (gfx950) quadruplet fine-tuning hot path.
 *
 * This is the drop-in boundary. The reference is pure
 * Python with no FFI of its own, so each entry point names the reference
 * interface whose arithmetic it replaces. All pointers are DEVICE pointers
 * unless the parameter name ends in _host; the library never allocates, frees
 * or retains caller memory (handles own only small device tables that depend
 * on the config). Every call enqueues on `stream` (a hipStream_t passed as
 * void*) and returns without a host sync. Return value: 0 = OK, negative =
 * qst_status (see qst_strerror). Nothing throws or aborts.
 *
 * Numeric contract: fp32 parameters, fp32 residual stream / LayerNorm /
 * softmax / pooling / loss; GEMM and attention contractions take bf16 MFMA
 * operands with fp32 accumulation. precision = QST_PREC_BF16X3 splits every
 * fp32 operand into hi+lo bf16 and issues three MFMAs (fp32-class accuracy,
 * the parity mode); QST_PREC_BF16 rounds operands once (the throughput mode);
 * QST_PREC_FP8 (BASELINE configs[4] "fp8 weights ... CDNA4 fp8 MFMA GEMMs"; inference, and with training != 0 the forward
 * of a training step whose backward is the bf16 one: qst_encoder_backward* on this handle with the bf16 shadows) runs every Linear on the fp8 matrix
 * cores: weights AND activations as OCP MXFP8 (e4m3 elements, one E8M0 scale per 32 input features;
 * v_mfma_scale_f32_32x32x64_f8f6f4, fp32 accumulation), attention in bf16, residual stream / LayerNorm in fp32.
 * QST_PREC_F16 (round 5) is QST_PREC_BF16 with IEEE half in bf16's place: the same kernels compiled on the other 16-bit
 * operand type (v_mfma_f32_32x32x16_f16: same issue rate, same bytes), 11 significand bits instead of 8 -- embeddings
 * within the north-star tolerance (rtol 1e-3 / atol 1e-4) of the fp32 reference for the six-layer models, where bf16's
 * are not -- and a 5-bit exponent: forward kernels saturate at +-65,504, and a training step runs under a loss scale
 * (qst_amp_scaler_init / qst_clip_adamw_step_amp), which is what the reference's own reduced precision does:
 * torch.cuda.amp.autocast + GradScaler, /root/reference/training/main.py:142 (`use_amp`), models/evaluators.py:92-94.
 * QST_PREC_F16W is QST_PREC_F16 with SPLIT WEIGHTS in the forward: every Linear multiplies its f16 activations by hi + lo
 * of the weight (two f16 values, W to ~2^-22), as a second pass over K in the same kernel -- the rounding of the weights is
 * the same for every token of a sequence and does not average out in the pooled embedding, the rounding of the activations
 * does: measured, it is 85-95% of plain f16's embedding error. With it the twelve-layer mpnet-base case is inside the
 * north-star tolerance too. Backward as QST_PREC_F16 (gradients need no more). Its shadow is qst_shadow_elems() long: the f16
 * arena and behind it a second one with the low halves.
 * The shadow of a QST_PREC_F16 handle holds IEEE half (qst_refresh_shadow on that handle), its activation arena f16
 * tensors of the bf16 arena's sizes; its backward is refused on another precision's arena and vice versa.
 */
#ifndef QST_H
#define QST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    QST_OK = 0,
    QST_ERR_BAD_ARG = -1,      /* null pointer, non-positive size, bad enum           */
    QST_ERR_UNSUPPORTED = -2,  /* dims the kernels are not built for (see qst_encoder_create) */
    QST_ERR_WORKSPACE = -3,    /* workspace/saved arena smaller than qst_*_bytes() says */
    QST_ERR_HIP = -4,          /* a HIP runtime call failed; qst_last_hip_error() has the code */
    QST_ERR_NO_DEVICE = -5,
    QST_ERR_COMM = -6,         /* RCCL could not be loaded, or one of its calls failed; qst_comm_last_error() has the text */
    QST_ERR_NO_FORWARD = -7    /* backward over an arena that no training forward of this precision and shape has filled */
} qst_status;

/* QST_ARCH_ROBERTA (RoBERTa / XLM-R): BERT's post-LN layer stack and parameter layout, no relative-attention bias,
 * position ids from the padding as MPNet's (pad_token_id + cumsum(ids != pad_token_id), pad 1), a token-type table of
 * type_vocab_size rows (1 in real checkpoints; the ids are all 0). */
enum { QST_ARCH_BERT = 0, QST_ARCH_MPNET = 1, QST_ARCH_ROBERTA = 2 };
enum { QST_PREC_BF16 = 0, QST_PREC_BF16X3 = 1, QST_PREC_FP8 = 3, QST_PREC_F16 = 4, QST_PREC_F16W = 5 };   /* 2 was an fp8-weights-only mode (removed) */
enum { QST_REDUCE_NONE = 0, QST_REDUCE_SUM = 1, QST_REDUCE_MEAN = 2 };

/* Encoder architecture. Mirrors HF BertConfig / MPNetConfig fields that the
 * reference selects by model name (training/main.py:114,242). */
typedef struct {
    int32_t arch;              /* QST_ARCH_*                                           */
    int32_t vocab_size;
    int32_t hidden_size;       /* H; multiple of 64                                    */
    int32_t num_layers;
    int32_t num_heads;         /* H / num_heads must be 32 or 64                       */
    int32_t intermediate_size; /* I; multiple of 64                                    */
    int32_t max_position;
    int32_t type_vocab_size;   /* 0 for MPNet, 1 for RoBERTa                           */
    float   layer_norm_eps;
    int32_t normalize;         /* ST Normalize module present                          */
    int32_t rel_buckets;       /* MPNet relative_attention_num_buckets (32)            */
    int32_t rel_max_distance;  /* MPNet (128)                                          */
    int32_t pad_token_id;      /* MPNet / RoBERTa position ids (1)                     */
    int32_t precision;         /* QST_PREC_*                                           */
} qst_config;

typedef struct qst_encoder qst_encoder;

const char* qst_strerror(int status);
int  qst_last_hip_error(void);
int  qst_version(void);

/* ---- parameter arena layout (contract with config.build_layout on the Python side) ---- */
/* Total elements of the flat fp32 arena (params, grads, exp_avg, exp_avg_sq all share it). */
int64_t qst_arena_elems(const qst_config* cfg);
/* Number of segments and per-segment description. name_out receives a static string. */
int     qst_arena_num_segments(const qst_config* cfg);
int     qst_arena_segment(const qst_config* cfg, int idx, const char** name_out, int64_t* offset_out,
                          int64_t* numel_out, int32_t* decay_out, int32_t* gemm_out);
/* Elements of the bf16 shadow arena: [W | W^T] copies of every GEMM weight. */
int64_t qst_shadow_elems(const qst_config* cfg);

/* Bytes of the MXFP8 weight shadow of QST_PREC_FP8: per GEMM weight the e4m3 matrix and its E8M0 block scales. */
int64_t qst_shadow8_bytes(const qst_config* cfg);

/* ---- encoder handle ---- */
int  qst_encoder_create(const qst_config* cfg, qst_encoder** out);
void qst_encoder_destroy(qst_encoder* enc);

/* Bytes of the activation arena `saved` for nseq sequences of length L.
 * training != 0 also reserves what backward needs. */
size_t qst_encoder_saved_bytes(const qst_encoder* enc, int nseq, int L, int training);
/* Bytes of scratch for backward (gradient activations). */
size_t qst_encoder_bwd_workspace_bytes(const qst_encoder* enc, int nseq, int L);

/* Refresh the bf16 shadows (W and W^T of every GEMM weight) from the fp32 arena.
 * Must be called after any parameter update and before forward/backward. */
int qst_refresh_shadow(const qst_encoder* enc, const float* params, void* shadow_bf16, void* stream);
/* QST_PREC_FP8: a buffer of qst_shadow8_bytes holds every GEMM weight as MXFP8: e4m3 bytes, then one E8M0
 * scale per 32 input features of each output row (qst_quant_mx). qst_encoder_forward on a QST_PREC_FP8 handle takes it
 * as its `shadow` argument. */
int qst_refresh_shadow_mx(const qst_encoder* enc, const float* params, void* shadow_mx, void* stream);

/*
 * Replaces SentenceTransformer.forward = Sequential(Transformer, Pooling(mean)[, Normalize])
 * (sentence-transformers 2.2.2; call site /root/reference/models/quadruplet_sentence_transformer.py:42-60)
 * over BertModel / MPNetModel.forward (transformers).
 *   ids, mask, type_ids : int64 [nseq, L] (type_ids may be NULL = all zero); L multiple of 32, <= 512
 *   params              : fp32 arena; shadow: bf16 arena from qst_refresh_shadow
 *   out_emb             : fp32 [nseq, D]  ('sentence_embedding'; D = qst_encoder_embedding_dim, H for mean pooling)
 *   out_tok             : fp32 [nseq, L, H] token embeddings, or NULL
 *   saved               : activation arena (qst_encoder_saved_bytes)
 */
int qst_encoder_forward(qst_encoder* enc, const int64_t* ids, const int64_t* mask, const int64_t* type_ids,
                        int nseq, int L, const float* params, const void* shadow_bf16,
                        float* out_emb, float* out_tok, void* saved, size_t saved_bytes, int training,
                        void* stream);

/* Dropout for training forwards/backwards of this handle (HF hidden_dropout_prob on the embeddings and on both
 * projection outputs of every layer, attention_probs_dropout_prob on the softmax probabilities; the reference trains
 * in train() mode with HF's defaults 0.1 / 0.1: /root/reference/training/main.py:128). p_* in [0, 1); 0 / 0 turns it off
 * (the state of a new handle). state_dev: device uint32[4] owned by the caller, initialised with qst_dropout_init; every
 * qst_encoder_forward(training != 0) of a handle with dropout on first advances its step counter (on the stream, so the
 * step can sit inside a captured graph), and the backward of that forward recomputes the same masks from it -- no mask
 * is ever stored (include/qst_kernels.h: QstDrop). Inference forwards never drop. Every precision: the fp8 training forward
 * and the parity path (QST_PREC_BF16X3) drop at the same places with the same masks. */
int qst_encoder_set_dropout(qst_encoder* enc, float p_hidden, float p_attn, uint32_t* state_dev);
int qst_dropout_init(uint32_t* state_dev, uint64_t seed, void* stream);
/* Where this handle runs the feed-forward block (dense + GELU + dense + residual + LayerNorm) as ONE kernel instead of two
 * GEMM launches (H = 384 only, no dropout): bit 0 = inference forward (default), bit 1 = training forward, bit 2 = backward.
 * Same results to fp32 summation order; the training variants are slower than the two-kernel path. */
int qst_encoder_set_ffn_chain(qst_encoder* enc, int mask);
/* Where this handle runs a projection and the LayerNorm behind it (forward), or a dgrad and the LayerNorm backward behind
 * it, as ONE kernel (H = 384: full-row tiles; H = 512 / 768 / 1024: the workgroups of a row panel exchange row statistics
 * inside the launch): 0 = by size (default: from 16,384 token rows at H = 384; above, from two tiles per CU -- 256 x 256, or
 * 128 x 384 where only that gives two: H = 768 from 32,768 token rows),
 * 1 = wherever such a kernel exists, 2 = never. Same results to fp32 summation order. */
int qst_encoder_set_ln_fusion(qst_encoder* enc, int mode);
/* How the 16-bit backward (every precision but QST_PREC_BF16X3) issues the weight gradients: 0 = the library's choice
 * (qst_wgrad_pairs_rule), 1 = one grouped launch per layer, 2 = one launch for two neighbouring layers wherever a call allows
 * it. A call pairs when it covers at least two layers and carries neither QST_BWD_SKIP_WGRAD nor QST_BWD_WGRAD_ONLY: pairs are
 * formed from the call's lowest layer up -- (1, 0), (3, 2), (5, 4); with an odd count the top layer keeps its own launch --
 * and a pair's launch is issued where the lower layer's was. Calls of one layer run as with 1. Where the handle may pair,
 * qst_encoder_bwd_workspace_bytes grows by a second set of the four tensors a launch reads (bf16 [M, H], [M, H], [M, I] and
 * [M, 3H]): set the mode BEFORE sizing the workspace. Same products; the fp32 partial sums are grouped differently. */
int qst_encoder_set_wgrad_pairs(qst_encoder* enc, int mode);
/* Host only, no device needed. The library's choice for cfg at M token rows (1 = pairs): at least two layers, M >= 8,192,
 * and at least one but fewer than two 192 x 192 tiles per workgroup in a layer's own launch (32 <= qst_wgrad_tiles(cfg, M, 1)
 * < 64: MiniLM's 48). DESIGN.md finding 48. */
int qst_wgrad_pairs_rule(const qst_config* cfg, int M);
/* Host only: the output tiles of the weight-gradient launch of `layers` (1 or 2) layers of cfg. */
int qst_wgrad_tiles(const qst_config* cfg, int M, int layers);
/* The pooling head of this handle (ST models.Pooling): an OR of the QST_POOL_* bits below, concatenated in the fixed order
 * cls, max, mean, mean_sqrt_len, weightedmean (include/qst_kernels.h: qst_pool_fwd has the exact semantics). 0 or
 * QST_POOL_MEAN = mean pooling, the state of a new handle. Every mode runs qst_pool_fwd/bwd, the only pooling entry
 * points since version 114. out_emb / grad_emb of qst_encoder_forward / _backward* are [nseq, D] with
 * D = qst_encoder_embedding_dim(); qst_encoder_saved_bytes grows by the pre-normalize D-vector and, with max, an int32
 * [nseq, H] argmax. A training forward records its mode with the arena: a backward of a handle set to
 * another mode is refused (QST_ERR_BAD_ARG). */
#define QST_POOL_CLS 1
#define QST_POOL_MAX 2
#define QST_POOL_MEAN 4
#define QST_POOL_MEAN_SQRT 8
#define QST_POOL_WMEAN 16
#define QST_POOL_ALL 31
int qst_encoder_set_pooling(qst_encoder* enc, int mode);
/* D: the width of this handle's sentence embedding (hidden_size x number of pooling blocks). */
int qst_encoder_embedding_dim(const qst_encoder* enc);
int qst_dropout_advance(uint32_t* state_dev, void* stream);

/*
 * Backward of the call above (replaces autograd through the same modules;
 * reference call site: `loss.backward()` inside SentenceTransformer.fit).
 *   grad_emb   : fp32 [nseq, D]
 *   grads      : fp32 arena; gradients are ACCUMULATED into it (zero it for a fresh step)
 *   workspace  : qst_encoder_bwd_workspace_bytes
 *   saved      : the arena a TRAINING forward of this process filled (any handle of the same model and arena kind: the
 *                dropout rates that forward ran under are remembered per arena, so the masks rebuilt here are its masks
 *                whatever qst_encoder_set_dropout has been told since); an arena without such a forward, one filled for another
 *                (nseq, L), or an arena of another kind -- the fp32 one of QST_PREC_BF16X3, the f16 one of QST_PREC_F16 / F16W,
 *                the bf16 one of QST_PREC_BF16 / FP8 -- is refused with QST_ERR_NO_FORWARD.
 */
int qst_encoder_backward(qst_encoder* enc, const int64_t* ids, const int64_t* mask, const int64_t* type_ids,
                         int nseq, int L, const float* params, const void* shadow_bf16,
                         const float* grad_emb, float* grads, void* saved, size_t saved_bytes,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Same backward pass in stages (head -> layers [layer_lo, layer_hi) top-down -> embeddings) so the caller can start
 * the RCCL all-reduce of a finished layer's gradients while lower layers are still running.
 * Calls must cover head first, then contiguous descending layer ranges, then embeddings, on one stream.
 * Per-layer gradient ranges of the arena: qst_arena_segment(). */
int qst_encoder_backward_partial(qst_encoder* enc, const int64_t* ids, const int64_t* mask, const int64_t* type_ids,
                                 int nseq, int L, const float* params, const void* shadow_bf16,
                                 const float* grad_emb, float* grads, void* saved, size_t saved_bytes,
                                 void* workspace, size_t workspace_bytes,
                                 int do_head, int layer_hi, int layer_lo, int do_embed, void* stream);

/* The staged backward with flags. QST_BWD_HEAD / QST_BWD_EMBED = do_head / do_embed above. For LAYER 0 ALONE
 * (layer_lo == 0, layer_hi == 1): QST_BWD_SKIP_WGRAD leaves out that layer's weight-gradient launch (its operands stay in
 * the workspace) and a later call with QST_BWD_WGRAD_ONLY for the same layer runs just that launch -- a data-parallel
 * step does {layer 0 | SKIP_WGRAD | EMBED}, starts the all-reduce of the embedding gradients (the largest bucket),
 * and runs layer 0's weight gradients underneath it. No other stage may run between the two calls. Any other layer range
 * with either flag is QST_ERR_BAD_ARG: below a layer l > 0 the next stage overwrites the gradients its postponed launch
 * would read. */
enum { QST_BWD_HEAD = 1, QST_BWD_EMBED = 2, QST_BWD_SKIP_WGRAD = 4, QST_BWD_WGRAD_ONLY = 8 };
int qst_encoder_backward_stage(qst_encoder* enc, const int64_t* ids, const int64_t* mask, const int64_t* type_ids,
                               int nseq, int L, const float* params, const void* shadow_bf16,
                               const float* grad_emb, float* grads, void* saved, size_t saved_bytes,
                               void* workspace, size_t workspace_bytes,
                               int flags, int layer_hi, int layer_lo, void* stream);

/*
 * Replaces gamma_quadruplet_loss (/root/reference/models/losses/losses.py:9-69) and its autograd:
 * three triplet_margin_loss terms with pairwise_distance eps=1e-6 inside the norm.
 *   xa,xp,xq,xn : fp32 [B, D] anchor / positive / partially-positive / negative (row stride = D)
 *   out_loss    : fp32 [B] (reduction none) or [1]
 *   grad_*      : fp32 [B, D] d(loss)/dx, or all NULL for forward only. For reduction none the
 *                 upstream gradient is grad_out [B] (NULL = ones); for sum/mean grad_out is [1] or NULL.
 *   scratch     : fp32 [B] used for deterministic two-stage reduction when reduction != none
 */
int qst_quadruplet_loss(const float* xa, const float* xp, const float* xq, const float* xn,
                        int B, int D, float gamma, float margin_pos_neg, float margin_pos_part,
                        float margin_part_neg, float p, int swap, int reduction,
                        float* out_loss, const float* grad_out,
                        float* grad_a, float* grad_p, float* grad_q, float* grad_n,
                        float* scratch, void* stream);

/*
 * The row-wise pair and triplet objectives of sentence-transformers 2.2.2 (version 103; csrc/tuple_loss.hip): what
 * losses.CosineSimilarityLoss, ContrastiveLoss, OnlineContrastiveLoss and TripletLoss compute on the embeddings, and the
 * per-row metric evaluation.EmbeddingSimilarityEvaluator scores with, each value and its autograd in one launch per stage.
 * All tensors fp32, rows contiguous (stride D); any B >= 1, D >= 1. Metrics follow torch:
 *   COS_SIM   u.v / (max(|u|_2, 1e-8) * max(|v|_2, 1e-8))     (F.cosine_similarity: each norm clamped on its own)
 *   COS_DIST  1 - COS_SIM
 *   L2, L1    |u - v + 1e-6|_p                                 (F.pairwise_distance: eps added to the difference)
 *   DOT       u.v
 *   L2_PLAIN, L1_PLAIN   |u - v|_p                             (sklearn's paired distances; gradient 0 where u == v)
 * grad_* all NULL = forward only (nothing else is written); some but not all NULL is QST_ERR_BAD_ARG. reduction and
 * grad_out as qst_quadruplet_loss: out [B] and grad_out [B] (NULL = ones) for QST_REDUCE_NONE, out [1] and grad_out [1]
 * or NULL otherwise; sum / mean go through a fixed-order second stage (no atomics: results are bit-reproducible).
 */
enum { QST_METRIC_COS_SIM = 0, QST_METRIC_COS_DIST = 1, QST_METRIC_L2 = 2, QST_METRIC_L1 = 3, QST_METRIC_DOT = 4,
       QST_METRIC_L2_PLAIN = 5, QST_METRIC_L1_PLAIN = 6 };
enum { QST_PAIR_MSE = 0, QST_PAIR_CONTRASTIVE = 1, QST_PAIR_ONLINE_CONTRASTIVE = 2 };
/* out[b] = metric(u[b], v[b]); with grad_u / grad_v: grad_out[b] * d(out[b]) / d(u[b]), d(v[b]). Any metric. */
int qst_pair_metric(const float* u, const float* v, int B, int D, int metric, float* out,
                    const float* grad_out, float* grad_u, float* grad_v, void* stream);
/* labels fp32 [B]; m = metric(u, v) per row:
 *   QST_PAIR_MSE                 (m - label)^2, metric = QST_METRIC_COS_SIM            (CosineSimilarityLoss, MSELoss)
 *   QST_PAIR_CONTRASTIVE         0.5 * (label * m^2 + (1 - label) * relu(margin - m)^2)
 *   QST_PAIR_ONLINE_CONTRASTIVE  with poss = m[label == 1], negs = m[label == 0],
 *                                t_neg = max(poss) if |poss| > 1 else mean(negs), t_pos = min(negs) if |negs| > 1 else mean(poss):
 *                                sum(poss[poss > t_pos]^2) + sum(relu(margin - negs[negs < t_neg])^2). ALWAYS a sum: out [1],
 *                                grad_out [1] or NULL, `reduction` is not looked at beyond its range. The thresholds carry
 *                                no gradient; rows with any other label take no part; the mean of an empty set is NaN
 *                                and selects nothing.
 * The two contrastive kinds take metric QST_METRIC_COS_DIST, QST_METRIC_L2 or QST_METRIC_L1; margin >= 0.
 * scratch: fp32 [B + 2] (row values; for the online kind the distances and the two thresholds). May be NULL for
 * QST_REDUCE_NONE of the first two kinds. */
int qst_pair_loss(const float* u, const float* v, const float* labels, int B, int D, int kind, int metric,
                  float margin, int reduction, float* out_loss, const float* grad_out,
                  float* grad_u, float* grad_v, float* scratch, void* stream);
/* relu(metric(a, p) - metric(a, n) + margin), metric QST_METRIC_COS_DIST, QST_METRIC_L2 or QST_METRIC_L1; margin >= 0.
 * scratch: fp32 [B] (may be NULL for QST_REDUCE_NONE). */
int qst_triplet_loss(const float* xa, const float* xp, const float* xn, int B, int D, int metric, float margin,
                     int reduction, float* out_loss, const float* grad_out,
                     float* grad_a, float* grad_p, float* grad_n, float* scratch, void* stream);
/* What QuadrupletEvaluator scores with: per row the distances of (a, p), (a, q), (a, n) under three metrics and the three
 * strict comparisons of each, from one pass over the four rows. Index k = 3 * metric + j with metric 0 = cosine distance
 * (QST_METRIC_COS_DIST), 1 = Manhattan (QST_METRIC_L1_PLAIN), 2 = Euclidean (QST_METRIC_L2_PLAIN).
 *   out_dist   fp32 [B, 9] or NULL: j = the pair, 0 (a, p), 1 (a, q), 2 (a, n)
 *   out_flags  int32 [B]: bit k set = comparison j of the metric holds, j = 0 pos_part d(a, p) < d(a, q),
 *              1 pos_neg d(a, p) < d(a, n), 2 part_neg d(a, q) < d(a, n)
 *   out_counts int32 [9]: rows with bit k set; written, not accumulated (a fixed one-workgroup second stage over out_flags)
 * The comparisons are made on the fp32 values out_dist receives, with or without out_dist. The three pairs of a metric go
 * through one instruction sequence: bitwise-equal columns give bitwise-equal distances and a clear bit. Inputs fp32 [B, D],
 * rows contiguous; any B >= 1 and D >= 1 (16-byte loads when D % 4 == 0 and the four pointers are 16-byte aligned).
 * B < 1, D < 1 or a NULL input, out_flags or out_counts: QST_ERR_BAD_ARG, nothing written. */
int qst_quadruplet_eval(const float* xa, const float* xp, const float* xq, const float* xn, int B, int D,
                        float* out_dist, int32_t* out_flags, int32_t* out_counts, void* stream);

/*
 * MultipleNegativesRankingLoss and MultipleNegativesSymmetricRankingLoss of sentence-transformers 2.2.2 (version 105;
 * csrc/mnrl.hip): in-batch negatives. a fp32 [B, D] anchors, c fp32 [N, D] candidates, N >= B, rows contiguous; candidate i
 * (i < B) is the positive of anchor i, rows B .. N-1 are further negatives (the text columns after the second, stacked).
 *   S = scale * sim(a, c) [B, N], sim = QST_SCORE_COS (util.cos_sim: both sides through F.normalize(p=2, dim=1, eps=1e-12))
 *       or QST_SCORE_DOT (util.dot_score); QST_SCORE_EUCLID is refused
 *   symmetric = 0: out_loss[0] = mean_i(logsumexp_j S[i, j] - S[i, i])             = F.cross_entropy(S, arange(B))
 *   symmetric = 1: (that + F.cross_entropy(S[:, :B].T, arange(B))) / 2
 * grad_a [B, D] and grad_c [N, D] both NULL = forward only (nothing else is written); exactly one NULL is
 * QST_ERR_BAD_ARG. For cos the gradients pass through the normalisation as torch's autograd does: a row with |x| < 1e-12
 * has the normalised row 0 and the gradient d_hat / 1e-12. grad_out: fp32 [1] on the DEVICE (NULL = 1), read by the
 * kernels -- no host synchronisation, capturable in a HIP graph; it multiplies the finished gradients, so a call with
 * grad_out = g returns the correctly rounded g * (the gradients without).
 * B < 1, N < B, D < 1, a NULL input, out_loss or workspace, a workspace smaller than qst_mnrl_workspace_bytes(B, N, D) or not
 * 4-byte aligned, a scale that is not finite and positive, another sim or symmetric: QST_ERR_BAD_ARG before any launch,
 * nothing written. B * ldS (ldS = N rounded up to 4) or N * D past 2^31 - 1: QST_ERR_UNSUPPORTED. Any other B, N, D is
 * accepted (16-byte accesses when D % 4 == 0 and the pointers are 16-byte aligned). All reductions run in a fixed order
 * without atomics: the same inputs give bit-identical outputs from call to call.
 */
size_t qst_mnrl_workspace_bytes(int B, int N, int D);
int qst_mnrl_loss(const float* a, const float* c, int B, int N, int D, int sim, float scale, int symmetric,
                  float* out_loss, const float* grad_out, float* grad_a, float* grad_c,
                  void* workspace, size_t workspace_bytes, void* stream);

/*
 * qst_mnrl_loss with no B x N term (version 118; csrc/mnrl_stream.hip): the loss of the large batches of
 * CachedMultipleNegativesRankingLoss (GradCache). Same mathematics and the same argument contract as qst_mnrl_loss -- cos or
 * dot, plain or symmetric, the clamp of F.normalize, both gradients NULL = forward only (nothing else is written), exactly one
 * NULL is QST_ERR_BAD_ARG, grad_out a DEVICE scalar (NULL = 1) that multiplies the finished gradients, every bad argument
 * refused before any launch with nothing written, no atomics, no host synchronisation, capturable in a HIP graph,
 * bit-identical from call to call.
 * The anchors are walked in strips of strip_rows rows: 0 = the library's choice (the largest multiple of 64 whose fp32 score
 * strip strip_rows x ldS, ldS = N rounded up to 4, fits 64 MiB, at least 64, at most B rounded up to 64), otherwise a positive
 * multiple of 64; anything else is QST_ERR_BAD_ARG (and a workspace size of 0). Only one strip of scores exists at a time: the
 * workspace holds strip_rows x ldS floats, per-row and per-column arrays, and the partial sums of one strip's grad_a
 * (ceil(N / 4096) x strip_rows x D floats when N > 4096) -- linear in B + N at fixed D and strip_rows. The symmetric form
 * sweeps the strips twice (column statistics first), four products instead of three. All products run on the fp32 matrix
 * cores (v_mfma_f32_32x32x2_f32: exact fp32).
 * strip_rows x ldS or N * D past 2^31 - 1: QST_ERR_UNSUPPORTED; B itself has no limit short of int.
 * Plain form: out_loss and grad_a are bit-identical for every strip_rows; grad_c (summed over the strips) and everything in
 * the symmetric form (column statistics merged over the strips) may differ between strip_rows by rounding.
 */
size_t qst_mnrl_stream_workspace_bytes(int B, int N, int D, int strip_rows);
int qst_mnrl_stream_loss(const float* a, const float* c, int B, int N, int D, int sim, float scale, int symmetric,
                         int strip_rows, float* out_loss, const float* grad_out, float* grad_a, float* grad_c,
                         void* workspace, size_t workspace_bytes, void* stream);

/*
 * GISTEmbedLoss and CachedGISTEmbedLoss of sentence-transformers 2.3 / 3.x (version 119; csrc/gist.hip): in-batch negatives
 * that a frozen guide model filters. x fp32 [K * B, D]: the student's K >= 2 text columns stacked in column order (anchors a,
 * positives p, hard negatives n_1 ...); g fp32 [K * B, Dg]: the guide's embeddings of the same texts, Dg independent of D;
 * rows contiguous. With a hat = F.normalize(p=2, dim=1, eps=1e-12), row i has (K + 1) * B logits
 *   ap[i, j] = a_hat_i . p_hat_j, aa[i, j] = a_hat_i . a_hat_j, pp[i, j] = p_hat_i . p_hat_j, an_k[i, j] = a_hat_i . n_hat_k,j,
 * each divided by temperature; the guide has the same blocks from g, undivided, and thr_i = its ap[i, i]. An entry is removed
 * (probability and gradient exactly 0) when guide entry > bound_i, a strict comparison:
 *   QST_GIST_ABSOLUTE bound_i = thr_i - margin        QST_GIST_RELATIVE bound_i = thr_i * (1 - margin)
 * (margin = 0 is bound_i = thr_i under both: the original rule). The target ap[i, i] is kept by index, whatever the margin and
 * whatever the guide's value there; a NaN guide entry compares false and stays.
 *   out_loss[0] = mean_i(logsumexp(row i) - ap[i, i] / temperature)
 * grad_x [K * B, D] or NULL = forward only (nothing but out_loss is written): the gradient with respect to every student
 * column, through both sides of aa and pp and through the normalisation (a row with |x| < 1e-12 as in qst_mnrl_loss); the guide
 * gets none. grad_out: fp32 [1] on the DEVICE (NULL = 1), it multiplies the finished gradients.
 * Anchors and positives are walked in strips of strip_rows rows: 0 = the library's choice (the largest multiple of 64 whose
 * two fp32 strips strip_rows x ldS, ldS = (K + 1) * B rounded up to 4 -- student logits and guide scores -- fit 64 MiB together,
 * at least 64, at most B rounded up to 64), otherwise a positive multiple of 64. No B x B tensor exists outside the strips:
 * beyond them the workspace holds four arrays of K * B floats, one of B, and the partial sums of a strip's row-side products
 * (ceil(K * B / 4096) x strip_rows x D floats when K * B > 4096) -- linear in B at fixed K, D, Dg and strip_rows.
 * Contract as qst_mnrl_stream_loss: B < 1, K < 2, D < 1, Dg < 1, a NULL x, g, out_loss or workspace, a temperature that is not
 * finite and positive, a margin that is not finite, another margin_strategy, a strip_rows that is neither 0 nor a positive
 * multiple of 64 (workspace size 0 too), a workspace smaller than qst_gist_workspace_bytes or not 4-byte aligned:
 * QST_ERR_BAD_ARG before any launch, nothing written. (K + 1) * B, strip_rows x ldS, K * B * D or K * B * Dg past 2^31 - 1:
 * QST_ERR_UNSUPPORTED. All products run on the fp32 matrix cores (csrc/fp32_mgemm.h, shared with mnrl_stream.hip). No
 * atomics, no host synchronisation, capturable in a HIP graph, bit-identical from call to call. 3 + 5 s launches forward and
 * 4 + 9 s with gradients over s strips (one more per strip and row-side product whose K is chunked). out_loss is bit-identical
 * for every strip_rows; the gradients, summed over the strips, may differ between strip_rows by rounding.
 */
enum { QST_GIST_ABSOLUTE = 0, QST_GIST_RELATIVE = 1 };
size_t qst_gist_workspace_bytes(int B, int K, int D, int Dg, int strip_rows);
int qst_gist_loss(const float* x, const float* g, int B, int K, int D, int Dg, float temperature, int margin_strategy,
                  float margin, int strip_rows, float* out_loss, const float* grad_out, float* grad_x,
                  void* workspace, size_t workspace_bytes, void* stream);

/*
 * MatryoshkaLoss over (Symmetric)MultipleNegativesRankingLoss (version 116; csrc/mnrl_nested.hip): the loss above at K nested
 * prefixes of the embedding in one call. a, c, B, N, D, scale, symmetric as for qst_mnrl_loss. dims and weights are HOST
 * arrays of K entries: K distinct widths 1 <= d_k <= D in any order, 1 <= K <= 8, and finite weights. For each k
 *   x_hat_k = F.normalize(x[:, :d_k], p=2, dim=1, eps=1e-12), S_k = scale * a_hat_k c_hat_k^T,
 *   term_k = the plain or symmetric cross entropy of S_k as qst_mnrl_loss defines it for QST_SCORE_COS
 * (normalising after truncating makes util.cos_sim and util.dot_score the same scores: there is no sim argument).
 * out_terms fp32 [K] or NULL receives term_k in the caller's order; out_loss[0] = sum_k w_k term_k, summed in that order.
 * grad_a [B, D] and grad_c [N, D] are full width: the sum over k of w_k times the gradient through truncation and
 * normalisation, times *grad_out (device scalar, NULL = 1; it multiplies the finished gradient); the columns from max_k d_k on
 * are written as exact zeros; a prefix with |x[:d_k]| < 1e-12 follows torch's clamp as in qst_mnrl_loss. Both NULL = forward
 * only (nothing else is written); exactly one NULL is QST_ERR_BAD_ARG.
 * K outside 1 .. 8, a width outside 1 .. D or repeated, a weight that is not finite, NULL dims or weights, a workspace smaller
 * than qst_mnrl_nested_workspace_bytes(B, N, D, K) (0 for a bad shape or K) or not 4-byte aligned, and every bad argument of
 * qst_mnrl_loss: QST_ERR_BAD_ARG before any launch, nothing written. B * ldS or N * D past 2^31 - 1: QST_ERR_UNSUPPORTED. Any
 * other shape and any widths are accepted. The number of launches (6 with gradients, 7 symmetric) and of passes over a and c
 * does not depend on K. No atomics, no host synchronisation, capturable; the same inputs give bit-identical outputs.
 */
size_t qst_mnrl_nested_workspace_bytes(int B, int N, int D, int K);
int qst_mnrl_nested_loss(const float* a, const float* c, int B, int N, int D,
                         const int32_t* dims, const float* weights, int K,
                         float scale, int symmetric, float* out_loss, float* out_terms,
                         const float* grad_out, float* grad_a, float* grad_c,
                         void* workspace, size_t workspace_bytes, void* stream);

/*
 * The batch-mining triplet losses of sentence-transformers 2.2.2 (version 106; csrc/batch_triplet.hip): BatchHardTripletLoss,
 * BatchHardSoftMarginTripletLoss, BatchSemiHardTripletLoss, BatchAllTripletLoss. x fp32 [B, D], rows contiguous; labels
 * int64 [B]. d [B, B] is the distance of every pair of rows: metric QST_METRIC_L2_PLAIN (sqrt(sum_k (x_ik - x_jk)^2); bit-identical
 * rows give 0, and an exactly-zero distance passes no gradient) or QST_METRIC_COS_DIST (1 - <x_hat_i, x_hat_j>, x_hat =
 * F.normalize(x, p=2, dim=1, eps=1e-12), the gradient through the normalisation as qst_mnrl_loss). pos[i, j]: labels equal
 * and i != j; neg[i, k]: labels differ. With m = margin:
 *   QST_BT_HARD       hp_i = max_j(pos[i, j] * d_ij) (0 without a positive), hn_i = min_k(d_ik + max_k'(d_ik') * (1 - neg[i, k]));
 *                     mean_i relu(hp_i - hn_i + m)
 *   QST_BT_HARD_SOFT  the same hp, hn; mean_i log1p(exp(hp_i - hn_i)); margin is checked and not used
 *   QST_BT_ALL        sum over pos[i, j] & neg[i, k] of t = relu(d_ij - d_ik + m), / (#{t > 1e-16} + 1e-16)
 *   QST_BT_SEMIHARD   per pair pos[i, j]: n_ij = min{d_ik : neg[i, k], d_ik > d_ij}; if that set is empty the largest d_ik
 *                     over neg[i, k]; if anchor i has no negative the smallest entry of row i (its diagonal).
 *                     sum relu(d_ij - n_ij + m) / #pairs; a batch without any pair gives 0 / 0 = NaN, as upstream does
 * A max or min passes its gradient to the selected element only (the smallest index among equal values).
 * out_loss fp32 [1]. out_counts int64 [2] or NULL: {terms of the denominator's population, terms > 0} -- hard {B, anchors
 * with a positive hinge}, soft {B, B}, all {valid triplets, triplets > 1e-16}, semi {pairs, pairs with a positive hinge}.
 * grad_x fp32 [B, D] or NULL = forward only. grad_out: fp32 [1] on the DEVICE (NULL = 1), read by the kernels -- no host
 * synchronisation, capturable in a HIP graph; it multiplies the finished gradient. No atomics, every reduction in a fixed
 * order: the same inputs give bit-identical outputs from call to call.
 * B < 1, D < 1, a NULL x, labels, out_loss or workspace, a workspace smaller than qst_batch_triplet_workspace_bytes(B, D) or
 * not 16-byte aligned, another kind or metric, a margin that is negative or not finite: QST_ERR_BAD_ARG before any launch,
 * nothing written. B * ldB (ldB = B rounded up to 4) or B * D past 2^31 - 1: QST_ERR_UNSUPPORTED.
 */
enum { QST_BT_HARD = 0, QST_BT_HARD_SOFT = 1, QST_BT_SEMIHARD = 2, QST_BT_ALL = 3 };
size_t qst_batch_triplet_workspace_bytes(int B, int D);
int qst_batch_triplet_loss(const float* x, const int64_t* labels, int B, int D, int kind, int metric, float margin,
                           float* out_loss, int64_t* out_counts /* [2] or NULL */, const float* grad_out,
                           float* grad_x /* NULL = forward only */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * CoSENTLoss and AnglELoss of sentence-transformers (version 117; csrc/cosent.hip): pairwise ranking of graded pairs. u, v
 * fp32 [B, D], rows contiguous; labels fp32 [B], the grade of each pair. s_i is the pairwise score of row i:
 *   QST_PAIRSIM_COS    util.pairwise_cos_sim: sum(u_hat * v_hat), x_hat = F.normalize(x, p=2, dim=1, eps=1e-12); the gradient
 *                      passes through the normalisation as torch's autograd does (a row with |x| < 1e-12 is x / 1e-12 and
 *                      its norm passes no gradient, as in qst_mnrl_loss)
 *   QST_PAIRSIM_ANGLE  util.pairwise_angle_sim, D even: with u = [a, b], v = [c, d] (halves of D / 2)
 *                      s = |t| / (|u| |v|), t = sum_k a_k (c_k - d_k) + b_k (c_k + d_k); sgn(0) = 0 in the gradient, and
 *                      there is no epsilon: a zero row gives 0 / 0 = NaN, as upstream
 * With V = {(i, j) : labels_i < labels_j} and d_ij = scale * (s_i - s_j)
 *   out_loss[0] = log(1 + sum_V exp(d_ij)),
 * upstream's logsumexp over the masked B x B differences and a zero, computed around max(0, max_V d_ij). A row whose label
 * is NaN is in no pair. Without any pair (B = 1, all labels equal) the loss is exactly 0 and the gradients are zeros. A
 * score that is not finite makes the loss NaN. out_scores fp32 [B] or NULL receives the unscaled s.
 * grad_u and grad_v [B, D] both NULL = forward only (nothing else is written); exactly one NULL is QST_ERR_BAD_ARG.
 * grad_out: fp32 [1] on the DEVICE (NULL = 1), read by the kernels -- no host synchronisation, capturable in a HIP graph; it
 * multiplies the finished gradient. The workspace holds per-row scalars only (six floats a row: there is no B x B buffer);
 * 3 launches forward, 4 with gradients, whatever B and D are; O(B^2) exps, O(B) per row. No atomics, every reduction in a
 * fixed order: the same inputs give bit-identical outputs from call to call.
 * B < 1, D < 1, an odd D with QST_PAIRSIM_ANGLE, a NULL u, v, labels, out_loss or workspace, a workspace smaller than
 * qst_cosent_workspace_bytes(B, D) or not 16-byte aligned, another sim, a scale that is not finite and positive:
 * QST_ERR_BAD_ARG before any launch, nothing written. B * D past 2^31 - 1: QST_ERR_UNSUPPORTED. Any other B and D is
 * accepted (rows in registers up to D = 2048 and streamed beyond, 16 bytes a lane where D % 4 == 0 -- D % 8 == 0 for
 * QST_PAIRSIM_ANGLE, whose half rows start D / 2 floats apart -- and the pointers are 16-byte aligned, else by element).
 */
enum { QST_PAIRSIM_COS = 0, QST_PAIRSIM_ANGLE = 1 };
size_t qst_cosent_workspace_bytes(int B, int D);
int qst_cosent_loss(const float* u, const float* v, const float* labels, int B, int D, int sim, float scale,
                    float* out_loss /* [1] */, float* out_scores /* [B] or NULL */,
                    const float* grad_out /* device [1], NULL = 1 */, float* grad_u, float* grad_v,
                    void* workspace, size_t workspace_bytes, void* stream);

/*
 * Distillation from a teacher, sentence-transformers 2.2.2 (version 107; csrc/distill.hip): losses.MSELoss and what
 * evaluation.MSEEvaluator scores with, and losses.MarginMSELoss. All tensors fp32, rows contiguous (stride D); any B >= 1 and
 * D >= 1 (16-byte accesses when D % 4 == 0 and the pointers are 16-byte aligned, element by element otherwise; rows are kept
 * in registers up to D = 2048 and read a second time by the gradient pass beyond). Both run on the caller's stream without
 * host synchronisation (capturable in a HIP graph), grad_out is read on the device, and it multiplies the finished
 * gradient: a call with grad_out = g returns the correctly rounded g * (the gradients without). No atomics: the per-row
 * values go through a one-workgroup second stage that sums them in double in a fixed order, so the same inputs give
 * bit-identical outputs from call to call.
 * B < 1, D < 1, a NULL input or out_loss, a NULL scratch where one is needed, another sim or reduction: QST_ERR_BAD_ARG before
 * any launch, nothing written.
 */
/* mean over all B*D elements of (x - t)^2   (torch.nn.MSELoss() on [B, D]; MSELoss, MSEEvaluator)
 * out_loss fp32 [1]. grad_x fp32 [B, D] or NULL = forward only (nothing else is written):
 *   grad_out * 2 * (x - t) / (B * D), grad_out fp32 [1] on the DEVICE (NULL = 1), multiplying the finished gradient.
 * scratch fp32 [B]. */
int qst_embed_mse(const float* x, const float* t, int B, int D, float* out_loss,
                  const float* grad_out, float* grad_x, float* scratch, void* stream);
/* m_b = sim(q_b, p_b) - sim(q_b, n_b); row_b = (m_b - labels_b)^2; reduction QST_REDUCE_NONE / SUM / MEAN as qst_triplet_loss
 * (grad_out [B] for NONE, [1] otherwise, NULL = ones). sim: QST_METRIC_DOT or QST_METRIC_COS_SIM, the latter with exactly
 * the semantics qst_pair_metric documents (each norm clamped at 1e-8) so that the fused and the unfused path agree.
 * util.pairwise_cos_sim of 2.2.2 normalises each row with F.normalize (x / max(|x|_2, 1e-12)) before the dot product
 * instead: the two differ only for rows whose norm is below 1e-8 -- here such a row is divided by 1e-8 and its norm
 * passes no gradient, in 2.2.2 it is divided by its own norm down to 1e-12. A zero row gives 0 in both.
 * out_margin fp32 [B] or NULL receives m. grad_q/p/n all NULL = forward only; some but not all NULL: QST_ERR_BAD_ARG.
 * scratch fp32 [B] (may be NULL for QST_REDUCE_NONE). */
int qst_margin_mse_loss(const float* q, const float* p, const float* n, const float* labels, int B, int D, int sim,
                        int reduction, float* out_loss, float* out_margin, const float* grad_out,
                        float* grad_q, float* grad_p, float* grad_n, float* scratch, void* stream);

/*
 * Distillation from a teacher's scores over a list of K candidates per query, candidate 0 the positive (version 121;
 * csrc/listwise.hip): losses.DistillKLDivLoss (sentence-transformers 3.4) and losses.MarginMSELoss with several negatives
 * (3.x). All tensors fp32. q [B, D]; docs [K, B, D] contiguous, candidate j of example b at (j * B + b) * D -- the text
 * columns of one encoder pass stacked, as they come out of it. sim: QST_METRIC_DOT or QST_METRIC_COS_SIM, the latter with
 * exactly qst_pair_metric's semantics (each norm clamped at 1e-8, a clamped norm passes no gradient), as qst_margin_mse_loss.
 *   QST_LISTWISE_KL          labels [B, K], the teacher's scores. With s_j = sim(q, d_j) / T and t = softmax(labels / T)
 *                            row_b = T^2 * sum_j t_j (log t_j - log_softmax(s)_j); a term with t_j == 0 is exactly 0 (torch's
 *                            xlogy in nn.KLDivLoss). QST_REDUCE_MEAN divides by B (reduction="batchmean").
 *                            d row / d sim_j = T (softmax(s)_j - t_j). Both softmaxes are taken around their maxima.
 *   QST_LISTWISE_MARGIN_MSE  labels [B, K - 1], the teacher's margin per negative; K >= 2.
 *                            row_b = sum_{j >= 1} (sim(q, d_0) - sim(q, d_j) - labels_{j-1})^2. QST_REDUCE_MEAN divides by
 *                            B (K - 1) (nn.MSELoss() on [B, K - 1]). temperature is ignored.
 * reduction QST_REDUCE_NONE / SUM / MEAN as qst_margin_mse_loss: out_loss [B] and grad_out [B] for NONE, [1] and [1]
 * otherwise; grad_out lives on the DEVICE (NULL = ones) and multiplies the finished gradient. out_scores fp32 [B, K] or NULL
 * receives the similarities (not divided by T). grad_q [B, D] and grad_docs [K, B, D] both NULL = forward only (nothing else
 * is written); exactly one NULL is QST_ERR_BAD_ARG. Gradients are written, not accumulated. scratch fp32 [B] (may be NULL
 * for QST_REDUCE_NONE).
 * One wave per example: the query row stays in registers up to D = 2048, every candidate row is read once for its score and
 * once more for the gradients (16-byte accesses when D % 4 == 0 and the pointers are 16-byte aligned, element by element
 * otherwise; past D = 2048 the query streams too). Runs on the caller's stream without host synchronisation (capturable in
 * a HIP graph). No atomics: the per-row values go through the one-workgroup second stage that sums them in double in a
 * fixed order, so the same inputs give bit-identical outputs from call to call.
 * B < 1, D < 1, a NULL q, docs, labels or out_loss, a NULL scratch where one is needed, another kind, sim or reduction, a
 * temperature that is not finite and positive with QST_LISTWISE_KL, K == 1 with QST_LISTWISE_MARGIN_MSE: QST_ERR_BAD_ARG.
 * K < 1 or K > 64 (lane j of the wave holds score j): QST_ERR_UNSUPPORTED. Both before any launch, nothing written.
 */
enum { QST_LISTWISE_KL = 0, QST_LISTWISE_MARGIN_MSE = 1 };
int qst_listwise_distill_loss(const float* q, const float* docs, const float* labels, int B, int K, int D, int kind, int sim,
                              float temperature, int reduction, float* out_loss, float* out_scores, const float* grad_out,
                              float* grad_q, float* grad_docs, float* scratch, void* stream);

/*
 * Replaces torch.nn.utils.clip_grad_norm_(params, max_grad_norm) + torch.optim.AdamW.step()
 * with ST fit()'s two parameter groups (/root/reference/training/main.py:128-148).
 *   n            : arena elements; decay is applied per segment as the layout says
 *   grad_scale   : multiplies every gradient first (1/world_size after an all-reduce sum)
 *   max_grad_norm: <= 0 disables clipping. norm_out (fp32 [1], device) receives the pre-clip global L2 norm.
 *   step         : 1-based optimiser step for bias correction
 *   scratch      : fp32 [1024] partial sums
 */
int qst_clip_adamw_step(const qst_encoder* enc, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                        float lr, float beta1, float beta2, float eps, float weight_decay,
                        float max_grad_norm, float grad_scale, int64_t step,
                        float* norm_out, float* scratch, void* stream);

/* The same step with the schedule on the device, so that a whole training step can be captured in a HIP graph and
 * replayed: no per-step host value is a kernel argument. step_dev (int64 [1], device) holds the number of optimiser
 * steps taken so far and is incremented by the call; the learning rate of step t is
 * transformers.get_linear_schedule_with_warmup(base_lr, warmup_steps, total_steps) at t-1 (constant base_lr when
 * total_steps <= 0), as SentenceTransformer.fit's 'WarmupLinear' (reference call site training/main.py:133-134).
 * scratch: fp32 [1024 + 3]. */
int qst_clip_adamw_step_sched(const qst_encoder* enc, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                              float base_lr, float beta1, float beta2, float eps, float weight_decay,
                              float max_grad_norm, float grad_scale, int64_t warmup_steps, int64_t total_steps,
                              int64_t* step_dev, float* norm_out, float* scratch, void* stream);

/* Mixed-precision optimiser step: what SentenceTransformer.fit(use_amp=True) wraps around AdamW -- scaler.scale(loss)
 * .backward(); scaler.unscale_(optimizer); clip_grad_norm_; scaler.step(optimizer); scaler.update(); and the scheduler
 * step skipped whenever the scale changed (sentence-transformers 2.2.2 fit(); reference call site
 * /root/reference/training/main.py:128-148 with use_amp = True) -- with torch.cuda.amp.GradScaler's defaults as ST builds it
 * (init_scale 65536, growth_factor 2, backoff_factor 0.5, growth_interval 2000), all on the device:
 *   scaler_dev : fp32 [4] {scale, growth tracker, 1.0 if the LAST step was skipped, number of skipped steps so far};
 *                qst_amp_scaler_init writes {init_scale, 0, 0, 0}. scaler_dev[0] is what the backward multiplies the loss
 *                gradient by: pass scaler_dev as qst_quadruplet_loss's grad_out (reduction sum / mean).
 *   step_dev   : int64 [2] {optimiser steps taken, scheduler steps taken}. Bias correction uses the first, the learning rate
 *                (WarmupLinear as qst_clip_adamw_step_sched) the second.
 * The call unscales by 1 / scale (times grad_scale, the 1 / world_size of a data-parallel step), takes the global norm of
 * the unscaled gradients (norm_out), and: if the norm is not finite (an inf / nan anywhere in `grads`: an f16 gradient
 * overflowed) the parameters, the moments and the optimiser step count stay as they are, the gradients are zeroed, scale *=
 * backoff and the tracker restarts; otherwise clip + AdamW + zero_grad as qst_clip_adamw_step, tracker += 1, and at
 * growth_interval scale *= growth. The scheduler count advances only when the scale did not change (ST's rule).
 * growth_interval <= 0: a STATIC scale (no growth; an overflow still skips the step, without backoff).
 * scratch: fp32 [1024 + 8]. Every rank of a data-parallel job sees the same reduced gradients, so the same decisions. */
int qst_amp_scaler_init(float* scaler_dev, float init_scale, void* stream);
int qst_clip_adamw_step_amp(const qst_encoder* enc, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                            float base_lr, float beta1, float beta2, float eps, float weight_decay,
                            float max_grad_norm, float grad_scale, int64_t warmup_steps, int64_t total_steps,
                            int64_t* step_dev, float* scaler_dev, float growth_factor, float backoff_factor,
                            int32_t growth_interval, float* norm_out, float* scratch, void* stream);

/* qst_clip_adamw_step over the arena AND a second flat fp32 buffer that lives outside it (version 108): parameters a loss
 * owns, such as the classifier of losses.SoftmaxLoss (loss_params.py). The extra group has the arena's conventions: x_n
 * elements, a multiple of 256; every tensor padded with zeros to a multiple of 256; x_chunk_decay one flag per 256-element
 * chunk (device). norm_out is the L2 norm over both buffers together -- what clip_grad_norm_(loss_model.parameters()) sees --
 * and one clip coefficient, lr and step apply to both; AdamW and zero_grad run on both. x_n == 0 (the x_ pointers are then
 * not looked at) gives the bits of qst_clip_adamw_step. x_n % 256 != 0, x_n < 0 or a NULL x_ pointer with x_n > 0:
 * QST_ERR_BAD_ARG before any launch. scratch: fp32 [2048]. */
int qst_clip_adamw_step_joint(const qst_encoder* enc, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                              float* x_params, float* x_grads, float* x_exp_avg, float* x_exp_avg_sq,
                              const uint8_t* x_chunk_decay, int64_t x_n,
                              float lr, float beta1, float beta2, float eps, float weight_decay,
                              float max_grad_norm, float grad_scale, int64_t step,
                              float* norm_out, float* scratch, void* stream);

/*
 * The classifier of sentence-transformers 2.2.2's losses.SoftmaxLoss (version 108; csrc/softmax_head.hip): a Linear on the
 * concatenation [u, v, |u - v|, u * v] of two sentence embeddings, its cross entropy, and their backward. All fp32, no
 * atomics, every sum in a fixed order (the same inputs give the same bits), on the caller's stream without host
 * synchronisation.
 *   u, v   : f32 [B, D], contiguous, 16-byte aligned
 *   parts  : which parts are concatenated, a mask of QST_SOFTMAX_*; their order is always u, v, |u - v|, u * v
 *   w      : f32 [C, K], K = (2 with REP + 1 with DIFF + 1 with MULT) * D, torch.nn.Linear layout, 16-byte aligned; b f32 [C]
 * 1 <= C <= 8, D % 4 == 0, D <= 2048: anything else QST_ERR_UNSUPPORTED. parts outside 1 .. 7, B < 1, a NULL or unaligned
 * pointer: QST_ERR_BAD_ARG. Both before any launch, nothing written. The feature vector [B, K] is never materialised.
 */
enum { QST_SOFTMAX_REP = 1, QST_SOFTMAX_DIFF = 2, QST_SOFTMAX_MULT = 4 };
/* logits f32 [B, C] = features W^T + b. One wave per row; the rows of u and v stay in registers. */
int qst_softmax_head_fwd(const float* u, const float* v, const float* w, const float* b, int B, int D, int C, int parts,
                         float* logits, void* stream);
/* From dlogits f32 [B, C]: grad_u, grad_v f32 [B, D], grad_w f32 [C, K], grad_b f32 [C], all written (not accumulated).
 * d|u - v| uses sign(u - v) with sign(0) = 0, torch's abs gradient. The weight gradient walks the rows in order, in up to 32
 * slices of at least 64 rows whose partial sums (in `workspace`, 16-byte aligned, qst_softmax_head_bwd_workspace_bytes; 0
 * bytes up to B = 64) are added in the order of the slices. */
size_t qst_softmax_head_bwd_workspace_bytes(int B, int D, int C, int parts);
int qst_softmax_head_bwd(const float* u, const float* v, const float* w, const float* dlogits, int B, int D, int C, int parts,
                         float* grad_u, float* grad_v, float* grad_w, float* grad_b, void* workspace,
                         size_t workspace_bytes, void* stream);
/* torch.nn.CrossEntropyLoss(weight=None, label_smoothing=0, ignore_index, reduction) on logits f32 [B, C] (any C >= 1) and
 * labels int64 [B]. A row whose label equals ignore_index contributes 0, has zero gradients and is left out of the mean's
 * denominator (no row left: the mean is NaN, as in torch). Any other label outside [0, C) gives NaN for its row's loss and
 * gradients -- where torch asserts on the device -- and counts in the mean's denominator; a label is compared, never used
 * as an index.
 *   out_loss : f32 [B] (QST_REDUCE_NONE) or [1]
 *   dlogits  : f32 [B, C] or NULL = forward only: (softmax - onehot) [/ kept rows], times grad_out (device; [B] for
 *              QST_REDUCE_NONE, [1] otherwise; NULL = ones)
 *   counts   : int64 [2] or NULL: {rows with a label in range, rows among them whose largest logit is the label's}; among
 *              equal logits the lowest index is the argmax
 *   scratch  : f32 [B + 2], 8-byte aligned
 * Under QST_REDUCE_MEAN each row's value is divided by the number of kept rows (in double, rounded to fp32) before the
 * shared second stage sums the rows in double. */
int qst_softmax_ce(const float* logits, const int64_t* labels, int B, int C, int64_t ignore_index, int reduction,
                   float* out_loss, const float* grad_out, float* dlogits, int64_t* counts, float* scratch, void* stream);

/*
 * sentence-transformers 2.2.2's models.Dense on pooled sentence embeddings, with the models.Normalize that may follow it
 * (version 110; csrc/dense_head.hip):
 *   z = x W^T + b;  a = act(z);  y = a, or a / max(|a|_2, 1e-12) per row with `normalize` (F.normalize, eps 1e-12)
 * All fp32, no atomics, every sum in a fixed order (the same inputs give the same bits), on the caller's stream without host
 * synchronisation; the products run on the LDS-tiled fp32 FMA loop of the batch losses, every edge guarded.
 *   x        : f32 [B, Din] with row stride ldx >= Din (a column block of a wider buffer is fine)
 *   w        : f32 [Dout, Din], torch.nn.Linear layout; b f32 [Dout] or NULL = no bias
 *   act      : QST_DENSE_ACT_*; normalize: 0 or 1
 *   y        : f32 [B, Dout]; row_norm f32 [B] = |a| of every row, written with normalize only (may be NULL without)
 * B >= 1 (up to 2^29), 1 <= Din, Dout <= 8192, no multiple-of-anything requirement: anything else QST_ERR_UNSUPPORTED. A NULL
 * required pointer, ldx < Din, another act, a normalize other than 0 or 1, a workspace that is too small or not 16-byte
 * aligned: QST_ERR_BAD_ARG. Both before any launch, nothing written.
 */
enum { QST_DENSE_ACT_IDENTITY = 0, QST_DENSE_ACT_TANH = 1 };
int qst_dense_head_fwd(const float* x, int ldx, const float* w, const float* b, int B, int Din, int Dout, int act,
                       int normalize, float* y, float* row_norm, void* stream);
/* From dy f32 [B, Dout], the forward's y and (with normalize) row_norm: grad_x f32 [B, Din], grad_w f32 [Dout, Din] and
 * grad_b f32 [Dout] (NULL = skipped), all written (not accumulated). Through the normalisation da = (dy - y <y, dy>) /
 * max(|a|, 1e-12) -- a row with |a| < 1e-12 gets dy / 1e-12, as torch's clamp does -- and through tanh dz = da (1 - a^2)
 * with a = y * max(|a|, 1e-12): nothing but y and row_norm is kept from the forward. The weight and bias gradients walk the
 * rows in order, in up to 16 slices of at least 64 rows whose partial sums are added in the order of the slices. workspace:
 * qst_dense_head_bwd_workspace_bytes (dz and the partial sums; 0 for sizes outside the limits), always required. */
size_t qst_dense_head_bwd_workspace_bytes(int B, int Din, int Dout);
int qst_dense_head_bwd(const float* x, int ldx, const float* w, const float* y, const float* row_norm, const float* dy,
                       int B, int Din, int Dout, int act, int normalize, float* grad_x, float* grad_w, float* grad_b,
                       void* workspace, size_t workspace_bytes, void* stream);

/*
 * What sentence-transformers 2.2.2's evaluation.BinaryClassificationEvaluator computes from the scores of n sentence pairs
 * and their labels in {0, 1} (version 109; csrc/binary_eval.hip), for nsets score rows over the same labels in one call.
 * With `rows` the stable sort of (score, label) by score -- descending where high_is_similar[set] != 0 (cosine, dot),
 * ascending otherwise (distances); -0.0 == +0.0 -- and a cut after row i, i = 0 .. n - 2, taking rows[0 .. i] as positive:
 *   accuracy, accuracy_threshold : the largest (positives before the cut + negatives after it) / n and the mean of the
 *                                  two scores around that cut (in fp32); no cut above 0 (n == 1 among them): 0 and -1
 *   f1, precision, recall, f1_threshold : the largest 2 p r / (p + r), p = c / (i + 1), r = c / T (c the positives before
 *                                  the cut, c > 0; T all positives), evaluated in double in exactly that order; none: all 0
 *   ap                           : the average precision, (1 / T) * sum over the positive pairs of (positives at least as
 *                                  similar) / (pairs at least as similar), equal scores included; T == 0: 0
 * Among equal maxima the first cut in sorted order wins; rows inside a run of equal scores are cuts like any other.
 *   scores : f32 [nsets, n] (device), labels : int64 [n] (device), high_is_similar : int32 [nsets] (HOST)
 *   out    : f64 [nsets, 8] (device) = {accuracy, accuracy_threshold, f1, precision, recall, f1_threshold, ap, T}
 * Nothing is sorted: an n x n counting pass gives every pair its place in `rows` and the counts above, and a pass of one
 * workgroup per set picks the cuts. No atomics, integer counts, the sum of ap in a fixed order (the same inputs give the
 * same bits), on the caller's stream without host synchronisation. A NaN score has no defined place.
 * 1 <= n <= 2^20 and 1 <= nsets <= 8: anything larger QST_ERR_UNSUPPORTED. A NULL pointer, n < 1, nsets < 1, a workspace
 * that is not 16-byte aligned or shorter than qst_binary_eval_workspace_bytes (24 bytes per pair and set; 0 for sizes
 * outside the limits): QST_ERR_BAD_ARG. Both before any launch, nothing written.
 */
size_t qst_binary_eval_workspace_bytes(int64_t n, int nsets);
int qst_binary_eval(const float* scores, const int64_t* labels, int64_t n, int nsets, const int32_t* high_is_similar,
                    double* out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * What sentence-transformers 2.2.2's evaluation.RerankingEvaluator computes for nq queries, each with its own candidate
 * documents (version 113; csrc/rerank.hip). The groups are ragged and shared by both entry points: query g owns the
 * documents offsets[g] .. offsets[g + 1] - 1 of the flat arrays (offsets[0] == 0, offsets[nq] == nd), the first num_pos[g]
 * of them its positives and the rest its negatives (upstream's [True] * num_pos + [False] * num_neg).
 *   offsets : int64 [nq + 1] (device), num_pos : int32 [nq] (device)
 * qst_rerank_scores: scores[j] f32 [nd] = the score of document j against the query of its group. queries f32 [nq, dim],
 * docs f32 [nd, dim] (device, contiguous), any dim >= 1 (rows are read 16 bytes a lane where dim % 4 == 0 and both arrays
 * are 16-byte aligned, element by element otherwise). mode: QST_SCORE_COS (util.cos_sim: each side divided by
 * max(|x|, 1e-12); a zero row scores 0), QST_SCORE_DOT or QST_SCORE_EUCLID (1 / (1 + |q - d|_2)); products and sums in
 * fp32. Four consecutive documents to a wave; a group is found by a binary search that reads offsets[1 .. nq - 1] only.
 * qst_rerank_metrics works from scores alone (any similarity may have made them; the larger the better, floats compared
 * as floats, -0.0 == +0.0). For every positive p of a group, over the documents d of that group:
 *   rank(p)   = 1 + |{ d : s_d > s_p, or s_d == s_p and d < p }|    its place in a stable descending sort
 *                                                                    (numpy.argsort(-s, kind="stable")): among equal
 *                                                                    scores the earlier document comes first
 *   ge_all(p) = |{ d : s_d >= s_p }|,  ge_pos(p) = |{ positives d : s_d >= s_p }|
 *   per_query : f64 [nq, 3] (device) = {rr, ap, ndcg} with P = num_pos[g]:
 *     rr   = 1 / min_p rank(p) where that minimum is <= k, else 0                       (upstream's MRR@k term)
 *     ap   = (1 / P) sum_p ge_pos(p) / ge_all(p)                                        (sklearn's average_precision_score)
 *     ndcg = sum_{p : rank(p) <= k} 1 / log2(1 + rank(p)) / sum_{i = 1 .. min(P, k)} 1 / log2(1 + i)
 *   out       : f64 [5] (device) = {mean rr, mean ap, mean ndcg, non-finite scores inside valid groups, invalid groups};
 *               the means run over the valid groups (none: 0)
 * A group is valid when 0 <= lo < hi <= nd and 1 <= num_pos < hi - lo. An invalid one is counted in out[4], its per_query
 * row is 0, it contributes nothing, and none of its scores is read: the check comes before any read of scores, so offsets
 * and num_pos of any content cause no access outside the arrays (offsets that are not ascending give valid-looking groups
 * unspecified numbers). A NaN or infinite score has no rank: it is counted in out[3] and the numbers of its group mean
 * nothing. Nothing is sorted and a group may have any size: a counting pass, the wave of a positive document striding its group, writes
 * {rank, ge_pos, ge_all}; a pass of one workgroup per query adds the terms in double, in document order; one workgroup
 * takes the means in a fixed order. No atomics, integer counts, the same inputs give the same bits, on the caller's
 * stream without host synchronisation.
 * A NULL pointer, nq < 1, nd < 2, k < 1, dim < 1, another mode, a workspace that is not 16-byte aligned or shorter than
 * qst_rerank_workspace_bytes (16 bytes per document and 4 per query, rounded up to 16; 0 for sizes outside the limits):
 * QST_ERR_BAD_ARG. nd >= 2^31 or nq >= 2^31: QST_ERR_UNSUPPORTED. Both before any launch, nothing written.
 */
int qst_rerank_scores(const float* queries, const float* docs, const int64_t* offsets, int64_t nq, int64_t nd, int dim,
                      int mode, float* scores, void* stream);
size_t qst_rerank_workspace_bytes(int64_t nq, int64_t nd);
int qst_rerank_metrics(const float* scores, const int64_t* offsets, const int32_t* num_pos, int64_t nq, int64_t nd, int k,
                       double* per_query, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* Retrieval scoring for the encode()-driven evaluators: what sentence-transformers'
 * InformationRetrievalEvaluator does per corpus chunk -- util.cos_sim / util.dot_score of the query embeddings
 * against the chunk, then torch.topk(k) (reference call sites models/evaluators.py:572-588,
 * ir_evauation_script.py:107-131). queries f32 [nq, dim], corpus f32 [nc, dim] (device, contiguous), dim % 32 == 0,
 * k <= min(nc, 1024). mode: QST_SCORE_DOT (util.dot_score), QST_SCORE_COS (util.cos_sim: both sides normalised first,
 * eps 1e-12) or QST_SCORE_EUCLID (the reference's own euclidean_score, models/evaluators.py:392-405:
 * 1 / (1 + ||q - c||_2), which training/main.py:57 and ir_evauation_script.py:71 pass as 'euclid_score'). Outputs: the
 * k best per query: out_scores f32 [nq, k], out_index int64 [nq, k], in the order qst_kernels.h states at qst_topk_rows:
 * a NaN score of either sign first, then descending score with -0.0 = +0.0, then ascending corpus index -- also among
 * the rows tied at the k-th place. The zero columns that pad the score block are no candidates. */
enum { QST_SCORE_DOT = 0, QST_SCORE_COS = 1, QST_SCORE_EUCLID = 2 };
size_t qst_topk_workspace_bytes(int nq, int nc, int dim);
int qst_topk_scores(const float* queries, const float* corpus, int nq, int nc, int dim, int k, int mode,
                    float* out_scores, int64_t* out_index, void* workspace, size_t workspace_bytes, void* stream);

/* The full score matrix of one of those functions (what util.cos_sim / util.dot_score / euclidean_score return):
 * out f32 [nq, ld_out] with ld_out = nc rounded up to a multiple of 4; columns nc .. ld_out-1 are written with 0.0.
 * dim % 32 == 0, and any other ld_out is refused (QST_ERR_UNSUPPORTED). */
size_t qst_score_workspace_bytes(int nq, int nc, int dim);
int qst_score_matrix(const float* queries, const float* corpus, int nq, int nc, int dim, int mode, float* out,
                     int64_t ld_out, void* workspace, size_t workspace_bytes, void* stream);
/* torch.nn.functional.normalize(x, p=2, dim=1, eps=1e-12) over the rows of x f32 [n, dim] (contiguous): what
 * SentenceTransformer.encode(normalize_embeddings=True) applies. out may alias x. */
int qst_normalize_rows(const float* x, int n, int dim, float* out, void* stream);

/* The classification head of a cross-encoder (version 102): what transformers' BertForSequenceClassification (pooler +
 * classifier) and RobertaForSequenceClassification (classifier.dense + out_proj) put on the encoder's first token, and
 * sentence-transformers 2.2.2 CrossEncoder.predict's activation, in one launch, all in fp32:
 *   h = tanh(W1 x + b1), z = W2 h + b2, out = act(z), then softmax over the C labels when softmax != 0 and C > 1.
 *   x   : f32 [n, H] rows with stride ldx >= H (qst_encoder_forward's out_emb with QST_POOL_CLS and normalize = 0)
 *   w1  : f32 [H, H] (16-byte aligned), b1 f32 [H]; w2 f32 [C, H], b2 f32 [C]   (torch.nn.Linear layout: [out, in])
 *   act : QST_HEAD_ACT_NONE (identity) or QST_HEAD_ACT_SIGMOID;  out: f32 [n, C]
 * H <= 1024 and a multiple of 4, 1 <= C <= 8; anything else is refused (QST_ERR_BAD_ARG / QST_ERR_UNSUPPORTED). */
enum { QST_HEAD_ACT_NONE = 0, QST_HEAD_ACT_SIGMOID = 1 };
int qst_cls_head_fwd(const float* x, int64_t ldx, int n, int H, const float* w1, const float* b1, const float* w2,
                     const float* b2, int C, int act, int softmax, float* out, void* stream);


/* The same with a ceiling: corpus rows scoring above max_score do not take part. This is the reference's negative
 * selection (dataset/quadruplet_dataset.py:185-270: candidates with SBERT cosine <= 0.2 to the reference caption, then
 * hard_contrastive_sampling = the k highest remaining scores, :31-47), for all reference captions at once
 * (SURVEY.md 8f rank 4). Where fewer than k rows qualify the tail of a result row is score -inf, index -1. A row with a
 * NaN score is not above any ceiling and takes part; a NaN max_score is refused (QST_ERR_BAD_ARG) before any launch. */
int qst_topk_scores_capped(const float* queries, const float* corpus, int nq, int nc, int dim, int k, int mode,
                           float max_score, float* out_scores, int64_t* out_index, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- data parallelism (the reference itself is single-process, training/main.py:113) ----
 * The exchange step of the data-parallel path is a sum of slices of the contiguous fp32 gradient arena between
 * qst_encoder_backward_stage calls; qst_clip_adamw_step's grad_scale applies the 1/world_size. The Python side of this
 * build drives it through torch.distributed (backend "nccl" = RCCL over xGMI). A caller without torch uses these: one
 * process per GPU; rank 0 obtains the id and ships its QST_COMM_ID_BYTES to the other ranks by its own means; every rank
 * calls qst_comm_init with the HIP device it will use current. RCCL is loaded at run time (the copy already in the
 * process if there is one), libqst.so has no link dependency on it.
 *   qst_allreduce_bucket : in-place SUM over all ranks of `count` elements at `ptr` (device), enqueued on `stream` --
 *                          pass a stream other than the compute stream and order the two with events to overlap the
 *                          exchange with the next backward stage. dtype: QST_COMM_F32 (the gradient arena) or QST_COMM_BF16.
 * Status QST_ERR_COMM: qst_comm_last_error() returns RCCL's text. */
typedef struct qst_comm qst_comm;
#define QST_COMM_ID_BYTES 128
enum { QST_COMM_F32 = 0, QST_COMM_BF16 = 1 };
int qst_comm_unique_id(void* id_out /* QST_COMM_ID_BYTES, host */);
int qst_comm_init(int rank, int world, const void* unique_id, qst_comm** out);
int qst_allreduce_bucket(qst_comm* comm, void* ptr, int64_t count, int dtype, void* stream);
int qst_comm_rank(const qst_comm* comm);
int qst_comm_world(const qst_comm* comm);
void qst_comm_destroy(qst_comm* comm);
const char* qst_comm_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* QST_H */
