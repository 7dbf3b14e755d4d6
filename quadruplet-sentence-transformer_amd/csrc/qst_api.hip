// qst_api.hip -- C-ABI entry points of libqst.so: arena layout, encoder handle, forward/backward
// orchestration (which kernels run, in which order, on which buffers). See include/qst.h.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include <mutex>
#include <unordered_map>
#include <algorithm>

#include "qst_common.h"
#include "qst_kernels.h"

static thread_local int g_last_hip_error = 0;
extern "C" int qst_set_hip_error(int code) { g_last_hip_error = code; return code; }
extern "C" int qst_last_hip_error(void) { return g_last_hip_error; }
extern "C" int qst_version(void) { return 121; }

extern "C" const char* qst_strerror(int s) {
    switch (s) {
        case QST_OK: return "ok";
        case QST_ERR_BAD_ARG: return "bad argument (null pointer, non-positive size or bad enum)";
        case QST_ERR_UNSUPPORTED: return "unsupported dimensions for the gfx950 kernels";
        case QST_ERR_WORKSPACE: return "workspace or saved-activation arena too small";
        case QST_ERR_HIP: return "HIP runtime error (see qst_last_hip_error)";
        case QST_ERR_NO_DEVICE: return "no HIP device";
        case QST_ERR_COMM: return "RCCL error (see qst_comm_last_error)";
        case QST_ERR_NO_FORWARD: return "no matching training forward: `saved` is not an activation arena that a training forward of this "
                                        "precision and shape (nseq, L) has filled in this process";
        default: return "unknown qst status";
    }
}

// ------------------------------------------------------------------ layout
namespace {

constexpr int64_t kAlign = 256;

struct Seg {
    std::string name;
    int64_t off, numel;
    int rows, cols;     // 2-D view (cols = 1 rows = numel for vectors)
    int decay, gemm;
    int64_t shadow_off; // bf16 shadow arena offset of W (W^T follows at shadow_off + align(numel)); -1 if none
};

struct Layout {
    std::vector<Seg> segs;
    int64_t total = 0, shadow_total = 0;
    // indices
    int word = -1, pos = -1, type = -1, eg = -1, eb = -1, rel = -1;
    std::vector<int> layer0;   // index of w_qkv per layer; following 11 entries are fixed order
};

bool cfg_ok(const qst_config* c) {
    if (!c) return false;
    if (c->arch != QST_ARCH_BERT && c->arch != QST_ARCH_MPNET && c->arch != QST_ARCH_ROBERTA) return false;
    if (c->hidden_size <= 0 || c->num_layers <= 0 || c->num_heads <= 0 || c->intermediate_size <= 0) return false;
    if (c->vocab_size <= 0 || c->max_position <= 0 || c->type_vocab_size < 0) return false;
    return true;
}

Layout build_layout(const qst_config* c) {
    Layout L;
    const int H = c->hidden_size, I = c->intermediate_size;
    int64_t off = 0, soff = 0;
    auto add = [&](const std::string& nm, int rows, int cols, int decay, int gemm) {
        Seg s;
        s.name = nm; s.off = off; s.rows = rows; s.cols = cols; s.numel = (int64_t)rows * cols;
        s.decay = decay; s.gemm = gemm; s.shadow_off = -1;
        if (gemm) { s.shadow_off = soff; soff += 2 * qst_align_up(s.numel, kAlign); }
        off = qst_align_up(off + s.numel, kAlign);
        L.segs.push_back(s);
        return (int)L.segs.size() - 1;
    };
    L.word = add("word_emb", c->vocab_size, H, 1, 0);
    L.pos = add("pos_emb", c->max_position, H, 1, 0);
    if (c->type_vocab_size > 0) L.type = add("type_emb", c->type_vocab_size, H, 1, 0);
    L.eg = add("emb_ln_g", H, 1, 0, 0);
    L.eb = add("emb_ln_b", H, 1, 0, 0);
    if (c->arch == QST_ARCH_MPNET) L.rel = add("rel_bias", c->rel_buckets, c->num_heads, 1, 0);
    for (int l = 0; l < c->num_layers; ++l) {
        const std::string p = "layer." + std::to_string(l) + ".";
        L.layer0.push_back(add(p + "w_qkv", 3 * H, H, 1, 1));
        add(p + "b_qkv", 3 * H, 1, 0, 0);
        add(p + "w_o", H, H, 1, 1);
        add(p + "b_o", H, 1, 0, 0);
        add(p + "ln1_g", H, 1, 0, 0);
        add(p + "ln1_b", H, 1, 0, 0);
        add(p + "w_1", I, H, 1, 1);
        add(p + "b_1", I, 1, 0, 0);
        add(p + "w_2", H, I, 1, 1);
        add(p + "b_2", H, 1, 0, 0);
        add(p + "ln2_g", H, 1, 0, 0);
        add(p + "ln2_b", H, 1, 0, 0);
    }
    L.total = off;
    L.shadow_total = soff;
    return L;
}
enum { W_QKV = 0, B_QKV, W_O, B_O, LN1_G, LN1_B, W_1, B_1, W_2, B_2, LN2_G, LN2_B };

}  // namespace

// What the training forward that FILLED an activation arena did with dropout, and which kind of arena it left: a backward
// regenerates the masks of that forward -- with ITS thresholds, whatever qst_encoder_set_dropout has been told since (fit()
// and bench.py switch dropout on live encoders; several forwards may be alive before their backwards run) and whichever
// handle runs the backward. Process-wide, keyed by the arena's device address; a backward over an arena no training forward
// of this process has filled, or over the other kind of arena, is refused (QST_ERR_BAD_ARG) instead of guessing the rates.
// (Rounds 2-3 kept a 16-entry ring per handle and fell back on the handle's current rates when it had no entry: wrong
// gradients without an error once the ring wrapped or a backward ran on another handle -- ADVICE r03.)
namespace {
enum { ARENA_BF16 = 0, ARENA_X3 = 1, ARENA_F16 = 2 };   // the bf16 activation arena (bf16 and fp8 forwards) / the fp32 one of bf16x3 / the f16 one
// A record also holds the shape of its forward: an arena whose address was reused by a later allocation of another shape (or a
// backward called with another nseq / L than its forward) is refused instead of read with the wrong plan.
// ... and its pooling head (qst_encoder_set_pooling): the saved pre-normalize vector and argmax are laid out for that mode.
struct FwdRec { uint32_t hidden = 0, attn = 0; int kind = ARENA_BF16; uint64_t seq = 0; int nseq = 0, L = 0, pool = QST_POOL_MEAN; };
std::mutex g_rec_mu;
std::unordered_map<const void*, FwdRec> g_recs;
uint64_t g_rec_seq = 0;
void rec_put(const void* saved, uint32_t hidden, uint32_t attn, int kind, int nseq, int L, int pool) {
    std::lock_guard<std::mutex> lk(g_rec_mu);
    g_recs[saved] = FwdRec{hidden, attn, kind, ++g_rec_seq, nseq, L, pool};
    if (g_recs.size() > 4096) {
        // arenas that were freed long ago: keep the 2048 most recently WRITTEN records (by count -- a cut at "sequence number -
        // 2048" dropped live arenas once hot ones had been re-put often enough)
        std::vector<uint64_t> seqs;
        seqs.reserve(g_recs.size());
        for (const auto& kv : g_recs) seqs.push_back(kv.second.seq);
        std::nth_element(seqs.begin(), seqs.end() - 2048, seqs.end());
        const uint64_t cut = *(seqs.end() - 2048);
        for (auto it = g_recs.begin(); it != g_recs.end();) it = it->second.seq < cut ? g_recs.erase(it) : std::next(it);
    }
}
bool rec_get(const void* saved, int kind, int nseq, int L, FwdRec* out) {
    std::lock_guard<std::mutex> lk(g_rec_mu);
    const auto it = g_recs.find(saved);
    if (it == g_recs.end() || it->second.kind != kind || it->second.nseq != nseq || it->second.L != L) return false;
    *out = it->second;
    return true;
}
}  // namespace

struct qst_encoder {
    qst_config cfg;
    Layout lay;
    uint8_t* chunk_decay = nullptr;   // device: decay flag per 256-element chunk
    int32_t* rel_lut = nullptr;       // device: MPNet bucket of (j - i), index (j - i) + 511
    int64_t* shadow_tab = nullptr;    // device: one row per GEMM weight for qst_shadow_all
    int shadow_nseg = 0, shadow_blocks = 0;
    // dropout (qst_encoder_set_dropout): 16-bit thresholds of the hidden-state and attention-probability masks, and the
    // caller's device counter {seed lo, seed hi, step, 0} that every training forward advances
    uint32_t drop_hidden = 0, drop_attn = 0;
    uint32_t* drop_state = nullptr;
    // Where the one-kernel feed-forward block (csrc/ffn.hip) is used (qst_encoder_set_ffn_chain): bit 0 = inference forward
    // (default: the [M, I] tensor never leaves the chip, 121 vs 144 us per layer at M = 32768), bit 1 = training forward,
    // bit 2 = backward. The training variants are correct and tested but measured SLOWER than the two-kernel path (178 vs
    // 144 us and 157 vs 125 us): their side outputs (gelu'(u), h / du: 100-200 MB per call) are stored by the same waves
    // that wait on the LDS-DMA stream, and stores and DMAs retire through one in-order counter.
    int ffn_chain = 1;
    int ln_fusion = 0;      // qst_encoder_set_ln_fusion: 0 = by size, 1 = wherever a fused kernel exists, 2 = never
    int wgrad_pairs = 0;    // qst_encoder_set_wgrad_pairs: 0 = by shape (wgrad_pair_rule), 1 = one launch per layer, 2 = pairs
    int pool = QST_POOL_MEAN;   // qst_encoder_set_pooling: QST_POOL_* bits
};

extern "C" int64_t qst_arena_elems(const qst_config* cfg) { return cfg_ok(cfg) ? build_layout(cfg).total : QST_ERR_BAD_ARG; }
// (QST_PREC_F16W: a second arena of the same layout behind the first holds the low halves of the split weights)
extern "C" int64_t qst_shadow_elems(const qst_config* cfg) {
    if (!cfg_ok(cfg)) return QST_ERR_BAD_ARG;
    const int64_t n = build_layout(cfg).shadow_total;
    return cfg->precision == QST_PREC_F16W ? 2 * n : n;
}
// fp8 shadow: the weight bytes of segment s sit at byte offset s.shadow_off (inside the first half of what is the [W | W^T]
// region in bf16-element units), its fp32 row scales at byte offset s.shadow_off + align(numel): same total, in bytes.
extern "C" int64_t qst_shadow8_bytes(const qst_config* cfg) { return cfg_ok(cfg) ? build_layout(cfg).shadow_total : QST_ERR_BAD_ARG; }
extern "C" int qst_arena_num_segments(const qst_config* cfg) { return cfg_ok(cfg) ? (int)build_layout(cfg).segs.size() : QST_ERR_BAD_ARG; }
extern "C" int qst_arena_segment(const qst_config* cfg, int idx, const char** name_out, int64_t* offset_out,
                                 int64_t* numel_out, int32_t* decay_out, int32_t* gemm_out) {
    if (!cfg_ok(cfg)) return QST_ERR_BAD_ARG;
    static thread_local Layout L;      // keeps name storage alive for the caller
    L = build_layout(cfg);
    if (idx < 0 || idx >= (int)L.segs.size()) return QST_ERR_BAD_ARG;
    const Seg& s = L.segs[idx];
    if (name_out) *name_out = s.name.c_str();
    if (offset_out) *offset_out = s.off;
    if (numel_out) *numel_out = s.numel;
    if (decay_out) *decay_out = s.decay;
    if (gemm_out) *gemm_out = s.gemm;
    return QST_OK;
}

// MPNet relative_position_bucket (modeling_mpnet.py:329-348) evaluated on the host in the same float32
// steps torch takes: log(n.float()/max_exact) / math.log(max_distance/max_exact) * (nb - max_exact) -> trunc.
extern "C" int qst_rel_bucket_host(int rel /* j - i */, int num_buckets, int max_distance) {
    int n = -rel;
    const int nb = num_buckets / 2;
    int ret = (n < 0) ? nb : 0;
    n = n < 0 ? -n : n;
    const int max_exact = nb / 2;
    if (n < max_exact) return ret + n;
    const float ratio = (float)n / (float)max_exact;
    const float denom = (float)log((double)max_distance / (double)max_exact);
    float v = logf(ratio) / denom;
    v = v * (float)(nb - max_exact);
    int large = max_exact + (int)v;
    if (large > nb - 1) large = nb - 1;
    return ret + large;
}

extern "C" void qst_encoder_destroy(qst_encoder* e);
extern "C" int qst_encoder_create(const qst_config* cfg, qst_encoder** out) {
    if (!cfg_ok(cfg) || !out) return QST_ERR_BAD_ARG;
    const int d = cfg->hidden_size / cfg->num_heads;
    if (cfg->hidden_size % cfg->num_heads != 0 || (d != 32 && d != 64)) return QST_ERR_UNSUPPORTED;
    if (cfg->hidden_size % 64 != 0 || cfg->intermediate_size % 64 != 0 || cfg->hidden_size > 1024) return QST_ERR_UNSUPPORTED;
    if (cfg->type_vocab_size > 2) return QST_ERR_UNSUPPORTED;
    if (cfg->precision != QST_PREC_BF16 && cfg->precision != QST_PREC_BF16X3 && cfg->precision != QST_PREC_FP8 &&
        cfg->precision != QST_PREC_F16 && cfg->precision != QST_PREC_F16W)
        return QST_ERR_UNSUPPORTED;
    if (cfg->precision == QST_PREC_FP8 && (cfg->hidden_size % 128 != 0 || cfg->intermediate_size % 128 != 0))
        return QST_ERR_UNSUPPORTED;                      // the fp8 K loop takes 128-deep stages
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return QST_ERR_NO_DEVICE;
    qst_encoder* e = new qst_encoder();
    e->cfg = *cfg;
    e->lay = build_layout(cfg);
    const int64_t nchunks = e->lay.total / kAlign;
    std::vector<uint8_t> flags((size_t)nchunks, 0);
    for (const Seg& s : e->lay.segs)
        if (s.decay)
            for (int64_t ch = s.off / kAlign; ch < qst_align_up(s.off + s.numel, kAlign) / kAlign; ++ch) flags[(size_t)ch] = 1;
    if (hipMalloc((void**)&e->chunk_decay, (size_t)nchunks) != hipSuccess) { delete e; return QST_ERR_HIP; }
    if (hipMemcpy(e->chunk_decay, flags.data(), (size_t)nchunks, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(e->chunk_decay); delete e; return QST_ERR_HIP;
    }
    if (cfg->arch == QST_ARCH_MPNET) {
        std::vector<int32_t> lut(1023);
        for (int r = -511; r <= 511; ++r) lut[(size_t)(r + 511)] = qst_rel_bucket_host(r, cfg->rel_buckets, cfg->rel_max_distance);
        if (hipMalloc((void**)&e->rel_lut, 1023 * sizeof(int32_t)) != hipSuccess ||
            hipMemcpy(e->rel_lut, lut.data(), 1023 * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(e->chunk_decay); if (e->rel_lut) (void)hipFree(e->rel_lut); delete e; return QST_ERR_HIP;
        }
    }
    {
        std::vector<int64_t> tab;
        int64_t blocks = 0;
        for (const Seg& s : e->lay.segs) {
            if (!s.gemm) continue;
            tab.insert(tab.end(), {s.off, (int64_t)s.rows, (int64_t)s.cols, s.shadow_off,
                                   s.shadow_off + qst_align_up(s.numel, kAlign), blocks});
            blocks += (int64_t)((s.cols + 31) / 32) * ((s.rows + 31) / 32);
        }
        e->shadow_nseg = (int)(tab.size() / 6);
        e->shadow_blocks = (int)blocks;
        if (hipMalloc((void**)&e->shadow_tab, tab.size() * sizeof(int64_t)) != hipSuccess ||
            hipMemcpy(e->shadow_tab, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess) {
            qst_encoder_destroy(e);
            return QST_ERR_HIP;
        }
    }
    *out = e;
    return QST_OK;
}

extern "C" void qst_encoder_destroy(qst_encoder* e) {
    if (!e) return;
    if (e->chunk_decay) (void)hipFree(e->chunk_decay);
    if (e->rel_lut) (void)hipFree(e->rel_lut);
    if (e->shadow_tab) (void)hipFree(e->shadow_tab);
    delete e;
}

// ------------------------------------------------------------------ activation arena
namespace {

// The arena planners' bump allocator: every buffer starts on a 256-byte boundary.
struct Bump {
    size_t off = 0;
    size_t operator()(size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; }
};

struct LayerAct {
    size_t qkv, lse, ctx, y1, y1b, xh1, rs1, u, hact, x, xb, xh2, rs2;   // x/xb/xh2/rs2 = layer OUTPUT
};
struct ActPlan {
    size_t pos_ids, x0, x0b, xh0, rs0, s_scratch, pooled, rel, argmax;
    size_t dropst;          // uint32[4]: the dropout counter as THIS forward used it (backward rebuilds the masks from it)
    std::vector<LayerAct> layers;
    size_t total;
};

// The pooling head's part of an activation arena: the pre-normalize [nseq, D] vector (D = H for mean pooling, where the
// arena is what it always was) and, for a head with max, the int32 [nseq, H] argmax -- placed last, so that every other
// offset is the same for every head.
size_t pool_dim(const qst_config& c, int pool) { return (size_t)__builtin_popcount((unsigned)pool) * c.hidden_size; }
size_t take_argmax(Bump& take, const qst_config& c, int nseq, int pool) {
    return (pool & QST_POOL_MAX) ? take((size_t)nseq * c.hidden_size * 4) : 0;
}

ActPlan plan_acts(const qst_config& c, int nseq, int L, bool training, int pool) {
    ActPlan p;
    const size_t M = (size_t)nseq * L, H = c.hidden_size, I = c.intermediate_size, A = c.num_heads;
    Bump take;
    p.pos_ids = take(M * 4);
    p.dropst = take(16);
    p.x0 = take(M * H * 4); p.x0b = take(M * H * 2); p.xh0 = take(M * H * 2); p.rs0 = take(M * 4);
    p.s_scratch = take(M * H * 4);
    p.pooled = take((size_t)nseq * pool_dim(c, pool) * 4);
    p.rel = (c.arch == QST_ARCH_MPNET) ? take(A * (size_t)2 * L * 4) : 0;      // relative-position vectors [A][2L]
    p.layers.resize(c.num_layers);
    for (int l = 0; l < c.num_layers; ++l) {
        LayerAct& a = p.layers[l];
        if (training || l < 2) {
            a.qkv = take(M * 3 * H * 2); a.lse = take((size_t)nseq * A * L * 4); a.ctx = take(M * H * 2);
            a.y1 = take(M * H * 4); a.y1b = take(M * H * 2); a.xh1 = take(M * H * 2); a.rs1 = take(M * 4);
            a.u = take(M * I * 2); a.hact = take(M * I * 2);
            a.x = take(M * H * 4); a.xb = take(M * H * 2); a.xh2 = take(M * H * 2); a.rs2 = take(M * 4);
        } else {
            a = p.layers[l - 2];      // inference: ping-pong two layer slots (a layer reads the previous slot's x)
        }
    }
    p.argmax = take_argmax(take, c, nseq, pool);
    p.total = take.off;
    return p;
}

// QST_PREC_BF16X3 forward: fp32 activations, inference only (two residual slots ping-pong)
struct X3Plan { size_t pos_ids, x[2], qkv, ctx, s, y1, h, pooled, rel, argmax, total; };
X3Plan plan_x3(const qst_config& c, int nseq, int L, int pool) {
    X3Plan p;
    const size_t M = (size_t)nseq * L, H = c.hidden_size, I = c.intermediate_size, A = c.num_heads;
    Bump take;
    p.pos_ids = take(M * 4);
    p.x[0] = take(M * H * 4); p.x[1] = take(M * H * 4);
    p.qkv = take(M * 3 * H * 4); p.ctx = take(M * H * 4); p.s = take(M * H * 4); p.y1 = take(M * H * 4);
    p.h = take(M * I * 4);
    p.pooled = take((size_t)nseq * pool_dim(c, pool) * 4);
    p.rel = (c.arch == QST_ARCH_MPNET) ? take(A * (size_t)L * L * 4) : 0;
    p.argmax = take_argmax(take, c, nseq, pool);
    p.total = take.off;
    return p;
}

// QST_PREC_BF16X3 TRAINING: every tensor the fp32-class backward needs, kept in fp32 (the parity path: sized for parity
// runs, 4x the bf16 path's activation bytes). s0 / s1 / s2 are the PRE-norm inputs of the three LayerNorms (the backward
// recomputes mean and rstd from them), u the pre-GELU tensor.
struct X3Layer { size_t qkv, ctx, s1, y1, u, h, s2, x; };
struct X3TrainPlan { size_t pos_ids, dropst, s0, x0, pooled, rel, argmax, total; std::vector<X3Layer> layers; };
X3TrainPlan plan_x3_train(const qst_config& c, int nseq, int L, int pool) {
    X3TrainPlan p;
    const size_t M = (size_t)nseq * L, H = c.hidden_size, I = c.intermediate_size, A = c.num_heads;
    Bump take;
    p.pos_ids = take(M * 4);
    p.dropst = take(16);                               // the dropout state {seed, step} this forward ran under
    p.s0 = take(M * H * 4); p.x0 = take(M * H * 4);
    p.pooled = take((size_t)nseq * pool_dim(c, pool) * 4);
    p.rel = (c.arch == QST_ARCH_MPNET) ? take(A * (size_t)L * L * 4) : 0;
    p.layers.resize(c.num_layers);
    for (auto& a : p.layers) {
        a.qkv = take(M * 3 * H * 4); a.ctx = take(M * H * 4); a.s1 = take(M * H * 4); a.y1 = take(M * H * 4);
        a.u = take(M * I * 4); a.h = take(M * I * 4); a.s2 = take(M * H * 4); a.x = take(M * H * 4);
    }
    p.argmax = take_argmax(take, c, nseq, pool);
    p.total = take.off;
    return p;
}
// its backward's scratch: gradient activations, one transposed weight (the dgrad's B operand) and the attention backward's
// per-query statistics
struct X3BwdPlan { size_t dx, dy, ds, dbig, dctx, dqkv, wT, drel, astats, total; };
X3BwdPlan plan_x3_bwd(const qst_config& c, int nseq, int L) {
    X3BwdPlan p;
    const size_t M = (size_t)nseq * L, H = c.hidden_size, I = c.intermediate_size, A = c.num_heads;
    Bump take;
    p.dx = take(M * H * 4); p.dy = take(M * H * 4); p.ds = take(M * H * 4); p.dbig = take(M * I * 4);
    p.dctx = take(M * H * 4); p.dqkv = take(M * 3 * H * 4);
    p.wT = take((H * I > 3 * H * H ? H * I : 3 * H * H) * 4);
    p.drel = (c.arch == QST_ARCH_MPNET) ? take(A * (size_t)L * L * 4) : 0;
    p.astats = take(qst_attention_bwd_x3_scratch_bytes(nseq, L, (int)A));
    p.total = take.off;
    return p;
}

// QST_PREC_FP8 forward (inference): MXFP8 operands for every Linear, bf16 attention, fp32 residual stream / LayerNorm
struct MxPlan { size_t pos_ids, x[2], xb, xq, xs, qkv, ctx, cq, cs, s, y1, y1b, yq, ys, hq, hs, pooled, rel, argmax, total; };
MxPlan plan_mx(const qst_config& c, int nseq, int L, int pool) {
    MxPlan p;
    const size_t M = (size_t)nseq * L, H = c.hidden_size, I = c.intermediate_size, A = c.num_heads;
    Bump take;
    p.pos_ids = take(M * 4);
    p.x[0] = take(M * H * 4); p.x[1] = take(M * H * 4);
    p.xb = take(M * H * 2); p.xq = take(M * H); p.xs = take(M * H / 32);
    p.qkv = take(M * 3 * H * 2); p.ctx = take(M * H * 2); p.cq = take(M * H); p.cs = take(M * H / 32);
    p.s = take(M * H * 4); p.y1 = take(M * H * 4); p.y1b = take(M * H * 2); p.yq = take(M * H); p.ys = take(M * H / 32);
    p.hq = take(M * I); p.hs = take(M * I / 32);
    p.pooled = take((size_t)nseq * pool_dim(c, pool) * 4);
    p.rel = (c.arch == QST_ARCH_MPNET) ? take(A * (size_t)2 * L * 4) : 0;
    p.argmax = take_argmax(take, c, nseq, pool);
    p.total = take.off;
    return p;
}
// The MXFP8 operand copies (e4m3 elements q, E8M0 scales s) of the fp8 forward's GEMM inputs: x, ctx, y1 and h. Inference
// finds them in its MxPlan; a TRAINING forward places them behind the bf16 activation arena (ActPlan) it fills.
struct MxOperands { size_t xq, xs, cq, cs, yq, ys, hq, hs, total; };
MxOperands plan_mx_train_operands(const qst_config& c, int nseq, int L, size_t base) {
    MxOperands t;
    const size_t M = (size_t)nseq * L, H = c.hidden_size, I = c.intermediate_size;
    Bump take{base};
    // scales: stage-major [K / 128][M][4] bytes = M * K / 32 exactly (K % 128 == 0), as plan_mx sizes them. Every writer
    // (ln_row_finish, the GELU_MX_TRAIN and GEMM + LayerNorm epilogues, qst_quant_mx) and every reader (the fp8 GEMMs' scale
    // loads) stops at row M - 1: the same kernels run on plan_mx's unpadded arrays. (Until version 112 each array carried
    // 1024 further bytes that nothing wrote or read; tests/test_gpu_encoder_arenas.py holds the last one against its band.)
    t.xq = take(M * H); t.xs = take(M * H / 32);
    t.cq = take(M * H); t.cs = take(M * H / 32);
    t.yq = take(M * H); t.ys = take(M * H / 32);
    t.hq = take(M * I); t.hs = take(M * I / 32);
    t.total = take.off;
    return t;
}

// dsb / dsb1 / du / dqkv are the dY operands of a layer's weight-gradient launch. pair: a second set of the four behind
// everything else (no other offset moves), so that two neighbouring layers' operands are alive at once and one launch can
// take both layers (Pass::backward_op16); without it [1] is [0].
struct BwdPlan { size_t dxa, dxb, ds, dsb[2], dsb1[2], du[2], dctx, dqkv[2], drel, lnred, lnred_stride, delta, total; };
BwdPlan plan_bwd(const qst_config& c, int nseq, int L, bool pair) {
    BwdPlan p;
    const size_t M = (size_t)nseq * L, H = c.hidden_size, I = c.intermediate_size, A = c.num_heads;
    Bump take;
    p.dxa = take(M * H * 4); p.dxb = take(M * H * 4); p.ds = take(M * H * 4); p.dsb[0] = take(M * H * 2);
    p.dsb1[0] = take(M * H * 2);
    p.du[0] = take(M * I * 2); p.dctx = take(M * H * 2); p.dqkv[0] = take(M * 3 * H * 2);
    p.drel = (c.arch == QST_ARCH_MPNET) ? take(A * (size_t)2 * L * 4) : 0;
    p.lnred_stride = (qst_ln_bwd_scratch_bytes((int)M, (int)H) + 255) / 256 * 256;
    p.lnred = take(p.lnred_stride * (size_t)(2 * c.num_layers + 1));
    p.delta = take((size_t)nseq * A * L * 4);
    p.dsb[1] = pair ? take(M * H * 2) : p.dsb[0];
    p.dsb1[1] = pair ? take(M * H * 2) : p.dsb1[0];
    p.du[1] = pair ? take(M * I * 2) : p.du[0];
    p.dqkv[1] = pair ? take(M * 3 * H * 2) : p.dqkv[0];
    p.total = take.off;
    return p;
}

// The shapes of a layer's four weight-gradient products -- dW2 [H, I], dW1 [I, H], dWo [H, H], dWqkv [3H, H], each the
// reduction of dY[M, N]^T . X[M, K] over the M token rows -- as problems at .. at + 3 of a grouped launch.
void wgrad_shapes(QstTnGroup& g, int at, int M, int H, int I) {
    const int nk[4][2] = {{H, I}, {I, H}, {H, H}, {3 * H, H}};
    for (int i = 0; i < 4; ++i) {
        QstGemmArgs& q = g.prob[at + i];
        q.M = M; q.N = nk[i][0]; q.K = nk[i][1];
        q.lda = q.N; q.ldb = q.K; q.ldc = q.K;
    }
}
// ... and the output tiles of such a launch: what the 32 workgroups of an M-range share out
constexpr int kTnTile = 192;        // the tile of gemm_tn_group_kernel (csrc/gemm.hip: TT)
int wgrad_tiles(const qst_config& c, int M, int layers) {
    QstTnGroup g{};
    g.nprob = 4 * layers;
    for (int k = 0; k < layers; ++k) wgrad_shapes(g, 4 * k, M, c.hidden_size, c.intermediate_size);
    int tiles = 0;
    for (int i = 0; i < g.nprob; ++i)
        tiles += ((g.prob[i].N + kTnTile - 1) / kTnTile) * ((g.prob[i].K + kTnTile - 1) / kTnTile);
    return tiles;
}
static_assert(QST_TN_MAX_PROB >= 8, "a launch takes the weight gradients of two layers");

// The library's choice of qst_encoder_set_wgrad_pairs (mode 0). The weight gradients of two neighbouring layers go into ONE
// launch where a layer alone hands the 32 workgroups of an M-range one to two 192 x 192 tiles each (MiniLM: 48 tiles, one
// whole tile and half of a leftover one per workgroup; the pair: 96 = three whole tiles, no leftover piece, a quarter fewer
// flushes, one start-up): measured in the step at M = 8,192 / 16,384 / 32,768, -3.8% / -1.4% / -0.6% (DESIGN.md finding 48).
// From two tiles per workgroup on (H = 768: 192 tiles) a layer keeps its own launch -- the pair gains 1% per launch there and
// loses 0.4% in the step, where the QKV dgrad no longer follows a launch that has just read its operand. Fewer than 8,192
// rows, and layers of fewer tiles than workgroups, were not measured and stay as they were.
constexpr int kWgradPairMinRows = 8192;
bool wgrad_pair_rule(const qst_config& c, int M) {
    const int tiles = wgrad_tiles(c, M, 1);
    return c.num_layers >= 2 && M >= kWgradPairMinRows && tiles >= 32 && tiles < 2 * 32;
}
bool wgrad_pairing(const qst_config& c, int M, int mode) {
    return c.num_layers >= 2 && (mode == 2 || (mode == 0 && wgrad_pair_rule(c, M)));
}

int shape_ok(const qst_encoder* e, int nseq, int L) {
    if (!e || nseq <= 0 || L <= 0) return QST_ERR_BAD_ARG;
    if (L % 32 != 0 || L > 512) return QST_ERR_UNSUPPORTED;
    if ((int64_t)nseq * L * e->cfg.intermediate_size * 2 >= ((int64_t)1 << 32)) return QST_ERR_UNSUPPORTED;  // 32-bit buffer offsets
    if (e->cfg.arch == QST_ARCH_BERT && L > e->cfg.max_position) return QST_ERR_UNSUPPORTED;
    // MPNet and RoBERTa count positions from pad_token_id + 1
    if (e->cfg.arch != QST_ARCH_BERT && L + e->cfg.pad_token_id + 1 > e->cfg.max_position) return QST_ERR_UNSUPPORTED;
    return QST_OK;
}

}  // namespace

extern "C" int qst_encoder_set_ffn_chain(qst_encoder* e, int mask) {
    if (!e || mask < 0 || mask > 7) return QST_ERR_BAD_ARG;
    e->ffn_chain = mask;
    return QST_OK;
}
extern "C" int qst_encoder_set_ln_fusion(qst_encoder* e, int mode) {
    if (!e || mode < 0 || mode > 2) return QST_ERR_BAD_ARG;
    e->ln_fusion = mode;
    return QST_OK;
}
extern "C" int qst_encoder_set_wgrad_pairs(qst_encoder* e, int mode) {
    if (!e || mode < 0 || mode > 2) return QST_ERR_BAD_ARG;
    e->wgrad_pairs = mode;
    return QST_OK;
}
extern "C" int qst_wgrad_pairs_rule(const qst_config* cfg, int M) {
    if (!cfg_ok(cfg) || M <= 0) return QST_ERR_BAD_ARG;
    return wgrad_pair_rule(*cfg, M) ? 1 : 0;
}
extern "C" int qst_wgrad_tiles(const qst_config* cfg, int M, int layers) {
    if (!cfg_ok(cfg) || M <= 0 || layers < 1 || layers > 2) return QST_ERR_BAD_ARG;
    return wgrad_tiles(*cfg, M, layers);
}
extern "C" int qst_encoder_set_pooling(qst_encoder* e, int mode) {
    if (!e || mode < 0 || mode > QST_POOL_ALL) return QST_ERR_BAD_ARG;
    e->pool = mode ? mode : QST_POOL_MEAN;
    return QST_OK;
}
extern "C" int qst_encoder_embedding_dim(const qst_encoder* e) {
    return e ? (int)pool_dim(e->cfg, e->pool) : QST_ERR_BAD_ARG;
}
extern "C" int qst_encoder_set_dropout(qst_encoder* e, float p_hidden, float p_attn, uint32_t* state_dev) {
    if (!e || !(p_hidden >= 0.f && p_hidden < 1.f) || !(p_attn >= 0.f && p_attn < 1.f)) return QST_ERR_BAD_ARG;
    if ((p_hidden > 0.f || p_attn > 0.f) && !state_dev) return QST_ERR_BAD_ARG;
    auto thr = [](float p) { const long t = lroundf(p * 65536.f); return (uint32_t)(t > 65535 ? 65535 : t); };
    e->drop_hidden = thr(p_hidden); e->drop_attn = thr(p_attn);
    e->drop_state = (e->drop_hidden || e->drop_attn) ? state_dev : nullptr;
    return QST_OK;
}

extern "C" size_t qst_encoder_saved_bytes(const qst_encoder* e, int nseq, int L, int training) {
    if (shape_ok(e, nseq, L) != QST_OK) return 0;
    const int pool = e->pool;
    if (e->cfg.precision == QST_PREC_BF16X3)
        return training ? plan_x3_train(e->cfg, nseq, L, pool).total : plan_x3(e->cfg, nseq, L, pool).total;
    if (e->cfg.precision == QST_PREC_FP8)
        return training ? plan_mx_train_operands(e->cfg, nseq, L, plan_acts(e->cfg, nseq, L, true, pool).total).total
                        : plan_mx(e->cfg, nseq, L, pool).total;
    return plan_acts(e->cfg, nseq, L, training != 0, pool).total;
}
extern "C" size_t qst_encoder_bwd_workspace_bytes(const qst_encoder* e, int nseq, int L) {
    if (shape_ok(e, nseq, L) != QST_OK) return 0;
    if (e->cfg.precision == QST_PREC_BF16X3) return plan_x3_bwd(e->cfg, nseq, L).total;
    return plan_bwd(e->cfg, nseq, L, wgrad_pairing(e->cfg, nseq * L, e->wgrad_pairs)).total;
}

namespace {

// The kernels whose operands / 16-bit outputs are bf16 (QST_PREC_BF16, and the backward of QST_PREC_FP8) or IEEE half
// (QST_PREC_F16): the same sources compiled on either type (qst_common.h: op16), entry points qst_* and qst_*_f16. The bf16
// forward / backward below are written once against this table.
struct OpKernels {
    decltype(&qst_gemm_nt) gemm_nt;
    decltype(&qst_gemm_nt_ln) gemm_nt_ln;
    decltype(&qst_ffn_chain) ffn_chain;
    decltype(&qst_gemm_tn_group) gemm_tn_group;
    decltype(&qst_embed_ln_fwd_drop) embed_ln_fwd_drop;
    decltype(&qst_ln_fwd) ln_fwd;
    decltype(&qst_ln_bwd_drop) ln_bwd_drop;
    decltype(&qst_attention_fwd_ex) attention_fwd_ex;
    decltype(&qst_attention_bwd_ex) attention_bwd_ex;
    decltype(&qst_shadow_all) shadow_all;
    int arena_kind;            // what a training forward through these kernels leaves behind (FwdRec.kind)
};
const OpKernels kOpBf16 = {qst_gemm_nt, qst_gemm_nt_ln, qst_ffn_chain, qst_gemm_tn_group, qst_embed_ln_fwd_drop, qst_ln_fwd,
                           qst_ln_bwd_drop, qst_attention_fwd_ex, qst_attention_bwd_ex, qst_shadow_all, ARENA_BF16};
const OpKernels kOpF16 = {qst_gemm_nt_f16, qst_gemm_nt_ln_f16, qst_ffn_chain_f16, qst_gemm_tn_group_f16,
                          qst_embed_ln_fwd_drop_f16, qst_ln_fwd_f16, qst_ln_bwd_drop_f16, qst_attention_fwd_ex_f16,
                          qst_attention_bwd_ex_f16, qst_shadow_all_f16, ARENA_F16};
const OpKernels& op_kernels(const qst_config& c) {
    return (c.precision == QST_PREC_F16 || c.precision == QST_PREC_F16W) ? kOpF16 : kOpBf16;
}

constexpr int kFuseLnMinRows = 16384;      // token rows from which the fused GEMM+LayerNorm kernels win (see forward)
// ... and for H = 512 / 768 / 1024, where a row spans several 256-column tiles whose workgroups exchange the row statistics
// (gemm8.hip): from two tiles per CU on (256 x 256, or 128 x 384 where only that gives two). Measured at H = 768 (tools/ln8_bench.py, fused against the GEMM + row-kernel pair):
// M = 49,152: forward -6 ... -10%, backward -8 ... -9%; M = 196,608: forward -6 ... -10%, backward -13 ... -19%.
static bool fuse_ln_rows(int H, int M, int mode) {
    if (!qst_gemm_nt_ln_supported(H) || mode == 2) return false;
    if (mode == 1) return true;
    if (qst_gemm_nt_ln_block_rows(H) == 128) return M >= kFuseLnMinRows;
    return (int64_t)((M + 255) / 256) * (H / 256) >= 512 || (H % 384 == 0 && (int64_t)((M + 127) / 128) * (H / 384) >= 512);
}

#define QST_TRY(expr) do { int _rc = (expr); if (_rc != QST_OK) return _rc; } while (0)

// a mask for the kernels that take one by pointer: none when it is off
const QstDrop* active(const QstDrop& d) { return d.state ? &d : nullptr; }

// One call of the encoder, built once by each entry point: dimensions, parameters, activation arena (and backward
// workspace), stream, and the dropout of this pass. The drivers below are its member functions.
struct Pass {
    const qst_encoder* e;
    const qst_config& c;
    const Layout& lay;
    const OpKernels& ops;      // the 16-bit kernels: bf16 or IEEE half (QST_PREC_F16 / F16W)
    const int64_t *ids, *mask, *type_ids;
    int nseq, L, M, H, I, A, d;
    const float* params;
    char* sv;                  // activation arena
    hipStream_t st;
    bool sat;                  // forward: the f16 build's GEMMs saturate their 16-bit outputs (QstGemmArgs.sat16); bf16 ignores it
    char* ws = nullptr;        // backward: workspace
    float* grads = nullptr;    // backward: gradients (accumulated)
    const int32_t* pos_ids = nullptr;
    const float* rel = nullptr;          // MPNet: this pass's relative-position table
    // Dropout of this pass: the thresholds in force -- the handle's current ones (forward) or the recorded ones of the
    // forward a backward undoes -- and the counter copy inside the activation arena of the forward at hand: several training
    // forwards may be live before their backwards run (fit() encodes the four columns one after the other), each with its
    // own step value.
    bool dropping = false;
    uint32_t thr_hidden = 0, thr_attn = 0;
    uint32_t* drop_state = nullptr;

    Pass(const qst_encoder* e_, const int64_t* ids_, const int64_t* mask_, const int64_t* type_ids_, int nseq_, int L_,
         const float* params_, void* saved, void* stream, bool forward)
        : e(e_), c(e_->cfg), lay(e_->lay), ops(op_kernels(e_->cfg)), ids(ids_), mask(mask_), type_ids(type_ids_), nseq(nseq_),
          L(L_), M(nseq_ * L_), H(c.hidden_size), I(c.intermediate_size), A(c.num_heads), d(H / A), params(params_),
          sv((char*)saved), st((hipStream_t)stream), sat(forward) {}

    const float* P(int seg) const { return seg < 0 ? nullptr : params + lay.segs[seg].off; }
    float* G(int seg) const { return seg < 0 ? nullptr : grads + lay.segs[seg].off; }
    float* F(size_t off) const { return (float*)(sv + off); }

    // dropout of a forward: a training forward of a handle that has it on
    void forward_dropout(bool training, size_t snapshot) {
        dropping = training && e->drop_state != nullptr;
        if (!dropping) return;
        thr_hidden = e->drop_hidden; thr_attn = e->drop_attn;
        drop_state = (uint32_t*)(sv + snapshot);
    }
    // ... of a backward: that of the training forward which filled the arena, as it recorded it
    int backward_dropout(int kind, size_t snapshot) {
        FwdRec fr;
        if (!rec_get(sv, kind, nseq, L, &fr)) return QST_ERR_NO_FORWARD;
        thr_hidden = fr.hidden; thr_attn = fr.attn;
        dropping = thr_hidden != 0 || thr_attn != 0;
        drop_state = (uint32_t*)(sv + snapshot);
        return QST_OK;
    }
    // the mask of a hidden-state site / of a layer's attention probabilities: all zero when the pass drops nothing, state
    // null and thr16 0 when it drops only the other kind
    QstDrop hidden(uint32_t site) const { return drop_at(thr_hidden, site); }
    QstDrop probs(uint32_t site) const { return drop_at(thr_attn, site); }
    QstDrop drop_at(uint32_t thr16, uint32_t site) const {
        if (!dropping) return QstDrop{nullptr, 0u, 0u};
        return QstDrop{thr16 ? drop_state : nullptr, site, thr16};
    }

    // The first launch of a forward: position ids and, when dropping, the step of the dropout counter (which it also copies
    // beside the activations for the backward). A training forward then records what it did, for the backward over the
    // same arena.
    int prologue(size_t pos_off, bool training, int kind) {
        pos_ids = (const int32_t*)(sv + pos_off);
        QST_TRY(qst_forward_prologue(ids, nseq, L, c.arch, c.pad_token_id, (int32_t*)(sv + pos_off),
                                     dropping ? e->drop_state : nullptr, drop_state, st));
        if (training) rec_put(sv, thr_hidden, thr_attn, kind, nseq, L, e->pool);
        return QST_OK;
    }
    // MPNet: the relative-position table (qst_rel_pos_fwd for the bf16 attention, qst_rel_bias_fwd for bf16x3)
    int rel_table(decltype(&qst_rel_pos_fwd) fn, size_t off) {
        if (c.arch != QST_ARCH_MPNET) return QST_OK;
        rel = F(off);
        return fn(P(lay.rel), e->rel_lut, A, L, F(off), st);
    }
    QstAttnDesc attn(int l, const void* qkv, void* ctx, float* lse) const {
        QstAttnDesc q{};
        q.qkv = qkv; q.mask = mask; q.rel_pos = rel; q.nseq = nseq; q.L = L; q.A = A; q.d = d; q.ctx = ctx; q.lse = lse;
        q.drop = probs(QST_DROP_SITE_PROBS(l));
        return q;
    }
    // pooling (+ normalisation) into out_emb, and the token states into out_tok when asked for
    int tail(const float* x, size_t pooled, size_t argmax, float* out_emb, float* out_tok) const {
        QST_TRY(qst_pool_fwd(x, mask, nseq, L, H, e->pool, c.normalize, out_emb, F(pooled), argmax_at(argmax), st));
        if (out_tok) QST_HIP_CHECK(hipMemcpyAsync(out_tok, x, (size_t)M * H * 4, hipMemcpyDeviceToDevice, st));
        return QST_OK;
    }

    int32_t* argmax_at(size_t off) const { return (e->pool & QST_POOL_MAX) ? (int32_t*)(sv + off) : nullptr; }
    int head_bwd(const float* grad_emb, size_t pooled, size_t argmax, float* dtok) const {
        return qst_pool_bwd(grad_emb, F(pooled), argmax_at(argmax), mask, nseq, L, H, e->pool, c.normalize, dtok, st);
    }
    // a backward over an arena that a training forward of ANOTHER pooling head filled is refused (its saved vector and
    // argmax are laid out for that head); an arena no forward has filled is left to backward_dropout (QST_ERR_NO_FORWARD)
    int check_pool(int kind) const {
        FwdRec fr;
        if (rec_get(sv, kind, nseq, L, &fr) && fr.pool != e->pool) return QST_ERR_BAD_ARG;
        return QST_OK;
    }

    // C[M, N] = A[M, K] . B[N, K]^T over the pass's token rows, operands contiguous. `o` names the optional operands at the
    // call site (designated initialisers); a dropout mask that is off goes in as none.
    QstGemmArgs gemm(const void* A_, const void* B, void* C, int N, int K, QstGemmArgs o) const {
        o.A = A_; o.B = B; o.C = C; o.M = M; o.N = N; o.K = K; o.lda = K; o.ldb = K; o.ldc = N; o.ldr = N;
        if (!o.drop.state) { o.drop = QstDrop{nullptr, 0u, 0u}; o.drop_where = 0; }
        return o;
    }
    int nt(const void* A_, const void* B, void* C, int N, int K, int epi, const QstGemmArgs& o = {}) const {
        QstGemmArgs g = gemm(A_, B, C, N, K, o);
        g.sat16 = sat ? 1 : 0;
        return ops.gemm_nt(&g, epi, st);
    }
    // GEMM with the following LayerNorm (mode 0) / LayerNorm backward (mode 1) fused into its epilogue (N = H)
    int nt_ln(const void* A_, const void* B, float* C, int K, int mode, const QstGemmArgs& o, const QstLnEpi& ln) const {
        const QstGemmArgs g = gemm(A_, B, C, H, K, o);
        return ops.gemm_nt_ln(&g, &ln, mode, st);
    }
    // the feed-forward block as one kernel (csrc/ffn.hip): mode 0 forward, mode 1 backward
    int ffn(QstFfnArgs g, int mode, const QstLnEpi& ln) const {
        g.M = M; g.H = H; g.I = I;
        return ops.ffn_chain(&g, &ln, mode, st);
    }
    int nt3(const float* A_, const float* B, float* C, int N, int K, int epi, const QstGemmArgs& o = {}) const {
        const QstGemmArgs g = gemm(A_, B, C, N, K, o);
        return qst_gemm_nt_x3(&g, epi, st);
    }

    int forward_op16(const void* shadow, float* out_emb, float* out_tok, size_t saved_bytes, bool training);
    int forward_fp8(const void* shadow, float* out_emb, float* out_tok, size_t saved_bytes, bool training);
    int forward_x3(float* out_emb, float* out_tok, size_t saved_bytes);
    int forward_x3_train(float* out_emb, float* out_tok, size_t saved_bytes);
    int backward_op16(const void* shadow, const float* grad_emb, size_t saved_bytes, size_t workspace_bytes, int flags,
                      int layer_hi, int layer_lo);
    int backward_x3(const float* grad_emb, size_t saved_bytes, size_t workspace_bytes, int flags, int layer_hi, int layer_lo);
};

// The 16-bit forward (QST_PREC_BF16 / F16 / F16W)
int Pass::forward_op16(const void* shadow, float* out_emb, float* out_tok, size_t saved_bytes, bool training) {
    const ActPlan p = plan_acts(c, nseq, L, training, e->pool);
    if (saved_bytes < p.total) return QST_ERR_WORKSPACE;
    const uint16_t* sh = (const uint16_t*)shadow;          // bf16, or IEEE half on a QST_PREC_F16 handle
    auto W = [&](int seg) { return sh + lay.segs[seg].shadow_off; };
    // QST_PREC_F16W: every forward Linear multiplies by hi + lo of the weight (a second pass over K: QstGemmArgs.B2)
    const bool splitw = c.precision == QST_PREC_F16W;
    auto WL = [&](int seg) -> const void* { return splitw ? sh + lay.shadow_total + lay.segs[seg].shadow_off : nullptr; };
    const float eps = c.layer_norm_eps;

    // dropout: training forwards of a handle that has it on; the step counter moves first (in the prologue launch, which
    // also leaves its snapshot beside the activations), backward reuses its value
    forward_dropout(training, p.dropst);
    QST_TRY(prologue(p.pos_ids, training, ops.arena_kind));
    const QstDrop de = hidden(QST_DROP_SITE_EMBED);
    QST_TRY(ops.embed_ln_fwd_drop(ids, type_ids, pos_ids, P(lay.word), P(lay.pos), P(lay.type), P(lay.eg), P(lay.eb), eps, M, H,
                                  F(p.x0), sv + p.x0b, sv + p.xh0, F(p.rs0), &de, st));
    QST_TRY(rel_table(qst_rel_pos_fwd, p.rel));
    const float* x = F(p.x0);
    const void* xb = sv + p.x0b;
    float* s = F(p.s_scratch);
    // H = 384: the LayerNorm after each projection runs inside that GEMM's epilogue (full-row tiles) -- from M = 16384
    // token rows on: one 128-row tile per workgroup gives a small batch too few workgroups (measured: the unfused pair
    // is 5-25% faster up to M = 8192, equal at 16384, 25% slower at 32768)
    const bool fuse_ln = fuse_ln_rows(H, M, e->ln_fusion) && !(splitw && qst_gemm_nt_ln_block_rows(H) != 128);   // (no split weights on the 8-phase loop)
    // ... and the whole feed-forward block (FFN-1, GELU, FFN-2, LayerNorm) is ONE kernel: h never returns from HBM, and
    // an inference forward does not write it at all
    const bool fuse_ffn = fuse_ln && !dropping && !splitw && (e->ffn_chain & (training ? 2 : 1)) && qst_ffn_chain_supported(H, I) != 0;
    for (int l = 0; l < c.num_layers; ++l) {
        const LayerAct& a = p.layers[l];
        const int b = lay.layer0[l];
        // (split weights: the value third of the fused QKV product only -- the rounding of the query / key weights perturbs
        //  logits that the softmax and the pooling average out: all-split and v-only measure the same, DESIGN.md finding 34)
        QST_TRY(nt(xb, W(b + W_QKV), sv + a.qkv, 3 * H, H, QST_EPI_BF16, {.bias = P(b + B_QKV), .B2 = WL(b + W_QKV), .b2_n0 = 2 * H}));
        const QstAttnDesc q = attn(l, sv + a.qkv, sv + a.ctx, F(a.lse));
        QST_TRY(ops.attention_fwd_ex(&q, st));
        QstGemmArgs o = {.bias = P(b + B_O), .resid = x, .drop = hidden(QST_DROP_SITE_ATTN_OUT(l)), .drop_where = 1, .B2 = WL(b + W_O)};
        if (fuse_ln) {
            o.C2 = sv + a.y1b;
            QST_TRY(nt_ln(sv + a.ctx, W(b + W_O), F(a.y1), H, 0, o,
                          {.gamma = P(b + LN1_G), .beta = P(b + LN1_B), .eps = eps, .xhat = sv + a.xh1, .rstd = F(a.rs1)}));
        } else {
            QST_TRY(nt(sv + a.ctx, W(b + W_O), s, H, H, QST_EPI_F32_RESID, o));
            QST_TRY(ops.ln_fwd(s, P(b + LN1_G), P(b + LN1_B), eps, M, H, F(a.y1), sv + a.y1b, sv + a.xh1, F(a.rs1), st));
        }
        const QstLnEpi ln2 = {.gamma = P(b + LN2_G), .beta = P(b + LN2_B), .eps = eps, .xhat = sv + a.xh2, .rstd = F(a.rs2)};
        if (fuse_ffn) {
            QST_TRY(ffn({.A = sv + a.y1b, .B1 = W(b + W_1), .B2 = W(b + W_2), .bias1 = P(b + B_1), .bias2 = P(b + B_2),
                         .resid = F(a.y1), .save_gp = training ? sv + a.u : nullptr, .save_h = training ? sv + a.hact : nullptr,
                         .C = F(a.x), .C2 = sv + a.xb},
                        0, ln2));
        } else {
            QST_TRY(nt(sv + a.y1b, W(b + W_1), sv + a.u, I, H, QST_EPI_GELU, {.C2 = sv + a.hact, .bias = P(b + B_1), .B2 = WL(b + W_1)}));
            o = {.bias = P(b + B_2), .resid = F(a.y1), .drop = hidden(QST_DROP_SITE_FFN_OUT(l)), .drop_where = 1, .B2 = WL(b + W_2)};
            if (fuse_ln) {
                o.C2 = sv + a.xb;
                QST_TRY(nt_ln(sv + a.hact, W(b + W_2), F(a.x), I, 0, o, ln2));
            } else {
                QST_TRY(nt(sv + a.hact, W(b + W_2), s, H, I, QST_EPI_F32_RESID, o));
                QST_TRY(ops.ln_fwd(s, P(b + LN2_G), P(b + LN2_B), eps, M, H, F(a.x), sv + a.xb, sv + a.xh2, F(a.rs2), st));
            }
        }
        x = F(a.x);
        xb = sv + a.xb;
    }
    return tail(x, p.pooled, p.argmax, out_emb, out_tok);
}

// fp8 matrix-core forward (QST_PREC_FP8; BASELINE configs[4]): the operator sequence of the bf16 forward with every
// Linear on MXFP8 operands (qst_gemm_nt_f8). Activations are quantised where they are produced when the producer is a
// GEMM (gelu(u) never exists in another format) or a LayerNorm (qst_ln_fwd_mx*), and by qst_quant_mx from the bf16 tensor
// the attention kernel writes.
// Inference keeps what the next launch reads (MxPlan). TRAINING (BASELINE configs[4] as a fine-tuning configuration) leaves,
// in the bf16 path's activation arena (ActPlan), exactly what the bf16 backward reads -- bf16 copies of every GEMM input,
// xhat / rstd of every LayerNorm, the attention statistics, gelu'(u) and h -- and drops out at the sites of the bf16
// training forward. The backward is then qst_encoder_backward_stage as it is, on the bf16 shadows: fp8 forward GEMMs, bf16
// dgrad / wgrad from fp32 master weights. The MXFP8 operand copies live behind the arena.
int Pass::forward_fp8(const void* shadow, float* out_emb, float* out_tok, size_t saved_bytes, bool training) {
    const ActPlan p = training ? plan_acts(c, nseq, L, true, e->pool) : ActPlan{};
    const MxPlan pm = training ? MxPlan{} : plan_mx(c, nseq, L, e->pool);
    const MxOperands mq = training ? plan_mx_train_operands(c, nseq, L, p.total)
                                   : MxOperands{pm.xq, pm.xs, pm.cq, pm.cs, pm.yq, pm.ys, pm.hq, pm.hs, pm.total};
    if (saved_bytes < mq.total) return QST_ERR_WORKSPACE;
    auto WQ = [&](int seg) { return (const uint8_t*)shadow + lay.segs[seg].shadow_off; };
    auto WS = [&](int seg) { return (const float*)(WQ(seg) + qst_align_up(lay.segs[seg].numel, kAlign)); };
    // the arguments of an MXFP8 product: A = e4m3 at aq with its scales at as, the weight of segment wseg
    auto mx = [&](size_t aq, size_t as, int K, int wseg, void* C, int N, QstGemmArgs o) {
        o.aux = sv + as; o.bscale = WS(wseg);
        return gemm(sv + aq, WQ(wseg), C, N, K, o);
    };
    auto f8 = [&](size_t aq, size_t as, int K, int wseg, void* C, int N, int epi, const QstGemmArgs& o) {
        const QstGemmArgs g = mx(aq, as, K, wseg, C, N, o);
        return qst_gemm_nt_f8(&g, epi, st);
    };
    // fp8 GEMM + LayerNorm in one launch (csrc/gemm8.hip gemm_nt8_ln_kernel<0, *, true>): y fp32, y 16-bit / xhat / rstd
    // (nullable) and y as MXFP8 (C3 / C4) for the next fp8 GEMM
    auto f8_ln = [&](size_t aq, size_t as, int K, int wseg, float* y, const QstGemmArgs& o, const QstLnEpi& ln) {
        const QstGemmArgs g = mx(aq, as, K, wseg, y, H, o);
        return qst_gemm_nt8_f8_ln(&g, &ln, st);
    };
    const float eps = c.layer_norm_eps;

    forward_dropout(training, p.dropst);
    QST_TRY(prologue(training ? p.pos_ids : pm.pos_ids, training, ARENA_BF16));
    float* x = F(training ? p.x0 : pm.x[0]);
    if (training) {
        const QstDrop de = hidden(QST_DROP_SITE_EMBED);
        QST_TRY(qst_embed_ln_fwd_mx_train(ids, type_ids, pos_ids, P(lay.word), P(lay.pos), P(lay.type), P(lay.eg), P(lay.eb), eps,
                                          M, H, x, sv + p.x0b, sv + p.xh0, F(p.rs0), sv + mq.xq, sv + mq.xs, &de, st));
    } else {
        QST_TRY(qst_embed_ln_fwd_mx(ids, type_ids, pos_ids, P(lay.word), P(lay.pos), P(lay.type), P(lay.eg), P(lay.eb), eps, M, H,
                                    x, nullptr, sv + mq.xq, sv + mq.xs, st));
    }
    QST_TRY(rel_table(qst_rel_pos_fwd, training ? p.rel : pm.rel));
    float* s = F(training ? p.s_scratch : pm.s);
    // H = 512 / 768 / 1024, two tiles per CU or more: projection + LayerNorm (+ MX emission) as one launch (gemm8.hip)
    const bool fuse_ln = qst_gemm_nt8_ln_supported(H) != 0 && fuse_ln_rows(H, M, e->ln_fusion) && H % 128 == 0 && I % 128 == 0;
    for (int l = 0; l < c.num_layers; ++l) {
        const int b = lay.layer0[l];
        // training: the layer's ActPlan slots; inference: the MxPlan buffers, the output in the other residual slot
        const LayerAct* a = training ? &p.layers[l] : nullptr;
        void* qkv = sv + (a ? a->qkv : pm.qkv);
        void* ctx = sv + (a ? a->ctx : pm.ctx);
        float* y1 = F(a ? a->y1 : pm.y1);
        float* xn = F(a ? a->x : pm.x[(l + 1) & 1]);
        QST_TRY(f8(mq.xq, mq.xs, H, b + W_QKV, qkv, 3 * H, QST_EPI_BF16, {.bias = P(b + B_QKV)}));
        const QstAttnDesc q = attn(l, qkv, ctx, a ? F(a->lse) : nullptr);
        QST_TRY(qst_attention_fwd_ex(&q, st));
        QST_TRY(qst_quant_mx(ctx, 1, M, H, sv + mq.cq, sv + mq.cs, st));
        const QstDrop d1 = hidden(QST_DROP_SITE_ATTN_OUT(l));
        if (fuse_ln) {
            QST_TRY(f8_ln(mq.cq, mq.cs, H, b + W_O, y1,
                          {.C2 = a ? sv + a->y1b : nullptr, .bias = P(b + B_O), .resid = x, .drop = d1, .drop_where = 1,
                           .C3 = sv + mq.yq, .C4 = sv + mq.ys},
                          {.gamma = P(b + LN1_G), .beta = P(b + LN1_B), .eps = eps, .xhat = a ? sv + a->xh1 : nullptr,
                           .rstd = a ? F(a->rs1) : nullptr}));
        } else {
            QST_TRY(f8(mq.cq, mq.cs, H, b + W_O, s, H, QST_EPI_F32_RESID, {.bias = P(b + B_O), .resid = x, .drop = d1, .drop_where = 1}));
            if (a)
                QST_TRY(qst_ln_fwd_mx_train(s, P(b + LN1_G), P(b + LN1_B), eps, M, H, y1, sv + a->y1b, sv + a->xh1, F(a->rs1),
                                            sv + mq.yq, sv + mq.ys, st));
            else
                QST_TRY(qst_ln_fwd_mx(s, P(b + LN1_G), P(b + LN1_B), eps, M, H, y1, nullptr, sv + mq.yq, sv + mq.ys, st));
        }
        if (a) {
            // FFN-1: gelu'(u) and h leave as bf16 (the backward's operands) and, from the same epilogue, the bf16-rounded h as
            // MXFP8 for FFN-2
            QST_TRY(f8(mq.yq, mq.ys, H, b + W_1, sv + a->u, I, QST_EPI_GELU_MX_TRAIN,
                       {.C2 = sv + a->hact, .bias = P(b + B_1), .C3 = sv + mq.hq, .C4 = sv + mq.hs}));
        } else {
            QST_TRY(f8(mq.yq, mq.ys, H, b + W_1, sv + mq.hq, I, QST_EPI_GELU_MX, {.C2 = sv + mq.hs, .bias = P(b + B_1)}));
        }
        const QstDrop d2 = hidden(QST_DROP_SITE_FFN_OUT(l));
        if (fuse_ln) {
            QST_TRY(f8_ln(mq.hq, mq.hs, I, b + W_2, xn,
                          {.C2 = a ? sv + a->xb : nullptr, .bias = P(b + B_2), .resid = y1, .drop = d2, .drop_where = 1,
                           .C3 = sv + mq.xq, .C4 = sv + mq.xs},
                          {.gamma = P(b + LN2_G), .beta = P(b + LN2_B), .eps = eps, .xhat = a ? sv + a->xh2 : nullptr,
                           .rstd = a ? F(a->rs2) : nullptr}));
        } else {
            QST_TRY(f8(mq.hq, mq.hs, I, b + W_2, s, H, QST_EPI_F32_RESID, {.bias = P(b + B_2), .resid = y1, .drop = d2, .drop_where = 1}));
            if (a)
                QST_TRY(qst_ln_fwd_mx_train(s, P(b + LN2_G), P(b + LN2_B), eps, M, H, xn, sv + a->xb, sv + a->xh2, F(a->rs2),
                                            sv + mq.xq, sv + mq.xs, st));
            else
                QST_TRY(qst_ln_fwd_mx(s, P(b + LN2_G), P(b + LN2_B), eps, M, H, xn, nullptr, sv + mq.xq, sv + mq.xs, st));
        }
        x = xn;
    }
    return tail(x, training ? p.pooled : pm.pooled, training ? p.argmax : pm.argmax, out_emb, out_tok);
}

// Parity-precision forward (QST_PREC_BF16X3): same operator sequence as the bf16 forward on fp32 activations and the fp32
// master weights, contractions through split-bf16 x3 MFMA kernels (csrc/x3.hip).
int Pass::forward_x3(float* out_emb, float* out_tok, size_t saved_bytes) {
    const X3Plan p = plan_x3(c, nseq, L, e->pool);
    if (saved_bytes < p.total) return QST_ERR_WORKSPACE;
    const float eps = c.layer_norm_eps;
    QST_TRY(prologue(p.pos_ids, false, ARENA_X3));
    float* x = F(p.x[0]);
    QST_TRY(qst_embed_ln_fwd(ids, type_ids, pos_ids, P(lay.word), P(lay.pos), P(lay.type), P(lay.eg), P(lay.eb), eps, M, H, x,
                             nullptr, nullptr, nullptr, st));
    QST_TRY(rel_table(qst_rel_bias_fwd, p.rel));
    float* qkv = F(p.qkv); float* ctx = F(p.ctx); float* s = F(p.s); float* y1 = F(p.y1); float* h = F(p.h);
    for (int l = 0; l < c.num_layers; ++l) {
        const int b = lay.layer0[l];
        float* xn = F(p.x[(l + 1) & 1]);
        QST_TRY(nt3(x, P(b + W_QKV), qkv, 3 * H, H, 0, {.bias = P(b + B_QKV)}));
        QST_TRY(qst_attention_fwd_x3(qkv, mask, rel, nseq, L, A, d, ctx, st));
        QST_TRY(nt3(ctx, P(b + W_O), s, H, H, 1, {.bias = P(b + B_O), .resid = x}));
        QST_TRY(qst_ln_fwd(s, P(b + LN1_G), P(b + LN1_B), eps, M, H, y1, nullptr, nullptr, nullptr, st));
        QST_TRY(nt3(y1, P(b + W_1), h, I, H, 2, {.bias = P(b + B_1)}));
        QST_TRY(nt3(h, P(b + W_2), s, H, I, 1, {.bias = P(b + B_2), .resid = y1}));
        QST_TRY(qst_ln_fwd(s, P(b + LN2_G), P(b + LN2_B), eps, M, H, xn, nullptr, nullptr, nullptr, st));
        x = xn;
    }
    return tail(x, p.pooled, p.argmax, out_emb, out_tok);
}

// QST_PREC_BF16X3 training forward: the same arithmetic as forward_x3, every intermediate kept (X3TrainPlan)
int Pass::forward_x3_train(float* out_emb, float* out_tok, size_t saved_bytes) {
    const X3TrainPlan p = plan_x3_train(c, nseq, L, e->pool);
    if (saved_bytes < p.total) return QST_ERR_WORKSPACE;
    const float eps = c.layer_norm_eps;
    // dropout as the bf16 training forward has it (same sites, same counter-based masks, the snapshot beside the activations);
    // the hidden-state masks are applied by a pass of their own (qst_dropout_apply_f32): speed is not what this path is for
    forward_dropout(true, p.dropst);
    QST_TRY(prologue(p.pos_ids, true, ARENA_X3));
    // out = (A . W^T + bias) * mask(site) + resid   (BertSelfOutput / BertOutput: LayerNorm(dropout(dense(x)) + input))
    auto proj = [&](const float* Ain, int K, int wseg, int bseg, const float* resid, float* out, uint32_t site) -> int {
        const QstDrop dd = hidden(site);
        if (!dd.state) return nt3(Ain, P(wseg), out, H, K, 1, {.bias = P(bseg), .resid = resid});
        QST_TRY(nt3(Ain, P(wseg), out, H, K, 0, {.bias = P(bseg)}));
        return qst_dropout_apply_f32(&dd, out, resid, (int64_t)M * H, out, st);
    };
    QST_TRY(qst_embed_sum_f32(ids, type_ids, pos_ids, P(lay.word), P(lay.pos), P(lay.type), M, H, F(p.s0), st));
    QST_TRY(qst_ln_fwd(F(p.s0), P(lay.eg), P(lay.eb), eps, M, H, F(p.x0), nullptr, nullptr, nullptr, st));
    const QstDrop de = hidden(QST_DROP_SITE_EMBED);
    if (de.state) QST_TRY(qst_dropout_apply_f32(&de, F(p.x0), nullptr, (int64_t)M * H, F(p.x0), st));
    QST_TRY(rel_table(qst_rel_bias_fwd, p.rel));
    const float* x = F(p.x0);
    for (int l = 0; l < c.num_layers; ++l) {
        const int b = lay.layer0[l];
        const X3Layer& a = p.layers[l];
        QST_TRY(nt3(x, P(b + W_QKV), F(a.qkv), 3 * H, H, 0, {.bias = P(b + B_QKV)}));
        const QstDrop dp = probs(QST_DROP_SITE_PROBS(l));
        QST_TRY(qst_attention_fwd_x3_drop(F(a.qkv), mask, rel, nseq, L, A, d, F(a.ctx), &dp, st));
        QST_TRY(proj(F(a.ctx), H, b + W_O, b + B_O, x, F(a.s1), QST_DROP_SITE_ATTN_OUT(l)));
        QST_TRY(qst_ln_fwd(F(a.s1), P(b + LN1_G), P(b + LN1_B), eps, M, H, F(a.y1), nullptr, nullptr, nullptr, st));
        // u = y1 W1^T + b1 and h = gelu(u) from one launch
        QST_TRY(nt3(F(a.y1), P(b + W_1), F(a.u), I, H, 4, {.C2 = F(a.h), .bias = P(b + B_1)}));
        QST_TRY(proj(F(a.h), I, b + W_2, b + B_2, F(a.y1), F(a.s2), QST_DROP_SITE_FFN_OUT(l)));
        QST_TRY(qst_ln_fwd(F(a.s2), P(b + LN2_G), P(b + LN2_B), eps, M, H, F(a.x), nullptr, nullptr, nullptr, st));
        x = F(a.x);
    }
    return tail(x, p.pooled, p.argmax, out_emb, out_tok);
}

// ... and its backward: fp32-class gradients ACCUMULATED into `grads`. Every contraction runs on split-bf16 x3 products: a
// dgrad is gemm_nt_x3 against the transposed weight, a wgrad (+ bias gradient) one gemm_tn_x3 launch over the token rows.
// Stages as the bf16 backward has them (head -> layers [layer_lo, layer_hi) top-down -> embeddings; the running d(loss)/d(x)
// lives in the workspace between calls), so that a data-parallel step can hand a finished layer's gradients to the all-reduce
// while the layers below are still running (round 5; rounds 3-4 ran it as one call and reduced afterwards).
int Pass::backward_x3(const float* grad_emb, size_t saved_bytes, size_t workspace_bytes, int flags, int layer_hi, int layer_lo) {
    const X3TrainPlan p = plan_x3_train(c, nseq, L, e->pool);
    const X3BwdPlan w = plan_x3_bwd(c, nseq, L);
    if (saved_bytes < p.total || workspace_bytes < w.total) return QST_ERR_WORKSPACE;
    // dropout: the masks of the forward that filled `saved` (its thresholds from its record, its (seed, step) from the
    // snapshot in the arena). ds = d(loss)/d(LayerNorm input) continues down the residual path as it is; the projection
    // that was dropped sees ds * mask (dsm, in a buffer that is free at that point).
    QST_TRY(backward_dropout(ARENA_X3, p.dropst));
    const float eps = c.layer_norm_eps;
    auto Wk = [&](size_t o) { return (float*)(ws + o); };
    float* dx = Wk(w.dx); float* dy = Wk(w.dy); float* ds = Wk(w.ds); float* dbig = Wk(w.dbig);
    float* dctx = Wk(w.dctx); float* dqkv = Wk(w.dqkv); float* wT = Wk(w.wT);
    // dX[M, in] = dY[M, out] . W[out, in] (+ resid)
    auto dgrad = [&](const float* dY, int out, int wseg, int in, float* dX, const float* resid) -> int {
        QST_TRY(qst_transpose_f32(P(wseg), out, in, in, wT, out, st));
        return nt3(dY, wT, dX, in, out, resid ? 1 : 0, {.resid = resid});
    };
    // dW[out, in] += dY^T . X ; db[out] += column sums of dY: one launch, straight from the row-major activations
    auto wgrad = [&](const float* dY, int out, const float* X, int in, int wseg, int bseg) -> int {
        QstGemmArgs g{};
        g.A = dY; g.B = X; g.C = G(wseg); g.colsum = G(bseg);
        g.M = M; g.N = out; g.K = in; g.lda = out; g.ldb = in; g.ldc = in;
        return qst_gemm_tn_x3(&g, st);
    };
    auto masked = [&](const float* g, uint32_t site, float* tmp, const float** out) -> int {
        const QstDrop dd = hidden(site);
        *out = g;
        if (!dd.state) return QST_OK;
        *out = tmp;
        return qst_dropout_apply_f32(&dd, g, nullptr, (int64_t)M * H, tmp, st);
    };
    float* drel = nullptr;
    if (c.arch == QST_ARCH_MPNET) {
        rel = F(p.rel);
        drel = Wk(w.drel);
        if (flags & QST_BWD_HEAD) QST_HIP_CHECK(hipMemsetAsync(drel, 0, (size_t)A * L * L * 4, st));
    }
    if (flags & QST_BWD_HEAD) QST_TRY(head_bwd(grad_emb, p.pooled, p.argmax, dx));
    for (int l = layer_hi - 1; l >= layer_lo; --l) {
        const int b = lay.layer0[l];
        const X3Layer& a = p.layers[l];
        const float* xin = l == 0 ? F(p.x0) : F(p.layers[l - 1].x);
        QST_TRY(qst_ln_bwd_f32(dx, F(a.s2), P(b + LN2_G), eps, M, H, ds, G(b + LN2_G), G(b + LN2_B), st));
        const float* dsm = ds;
        QST_TRY(masked(ds, QST_DROP_SITE_FFN_OUT(l), dctx, &dsm));                   // (dctx is free until the attention part)
        QST_TRY(qst_transpose_f32(P(b + W_2), H, I, I, wT, H, st));                  // du = (dsm . W2) * gelu'(u)
        QST_TRY(nt3(dsm, wT, dbig, I, H, 5, {.aux = F(a.u)}));
        QST_TRY(wgrad(dsm, H, F(a.h), I, b + W_2, b + B_2));
        QST_TRY(dgrad(dbig, I, b + W_1, H, dy, ds));                                 // dy1 = du . W1 + ds2
        QST_TRY(wgrad(dbig, I, F(a.y1), H, b + W_1, b + B_1));
        QST_TRY(qst_ln_bwd_f32(dy, F(a.s1), P(b + LN1_G), eps, M, H, ds, G(b + LN1_G), G(b + LN1_B), st));
        QST_TRY(masked(ds, QST_DROP_SITE_ATTN_OUT(l), dy, &dsm));                    // (dy has been consumed)
        QST_TRY(dgrad(dsm, H, b + W_O, H, dctx, nullptr));
        QST_TRY(wgrad(dsm, H, F(a.ctx), H, b + W_O, b + B_O));
        const QstDrop dp = probs(QST_DROP_SITE_PROBS(l));
        QST_TRY(qst_attention_bwd_x3(F(a.qkv), F(a.ctx), dctx, mask, rel, nseq, L, A, d, dqkv, drel, ws + w.astats, &dp, st));
        QST_TRY(dgrad(dqkv, 3 * H, b + W_QKV, H, dx, ds));                           // dx_in = dqkv . Wqkv + ds1
        QST_TRY(wgrad(dqkv, 3 * H, xin, H, b + W_QKV, b + B_QKV));
    }
    if (!(flags & QST_BWD_EMBED)) return QST_OK;
    const QstDrop de = hidden(QST_DROP_SITE_EMBED);              // the embedding dropout sits AFTER its LayerNorm
    if (de.state) QST_TRY(qst_dropout_apply_f32(&de, dx, nullptr, (int64_t)M * H, dx, st));
    QST_TRY(qst_ln_bwd_f32(dx, F(p.s0), P(lay.eg), eps, M, H, ds, G(lay.eg), G(lay.eb), st));
    QST_TRY(qst_embed_bwd(ds, ids, type_ids, (const int32_t*)(sv + p.pos_ids), nseq, L, H, c.type_vocab_size,
                          G(lay.word), G(lay.pos), G(lay.type), st));
    if (c.arch == QST_ARCH_MPNET) QST_TRY(qst_rel_bias_bwd(drel, e->rel_lut, c.rel_buckets, A, L, G(lay.rel), st));
    return QST_OK;
}

// The 16-bit backward (QST_PREC_BF16 / F16 / F16W, and QST_PREC_FP8 over the arena its training forward filled, `shadow`
// = the bf16 shadows)
int Pass::backward_op16(const void* shadow, const float* grad_emb, size_t saved_bytes, size_t workspace_bytes, int flags,
                        int layer_hi, int layer_lo) {
    const ActPlan p = plan_acts(c, nseq, L, true, e->pool);
    // Two neighbouring layers' weight gradients in one launch (wgrad_pair_rule): only a call that covers both layers and
    // issues its launches itself can do that; the staged calls of the data-parallel path (one layer each, layer 0's launch
    // postponed) run as before, inside the first set of dY tensors. The workspace is sized by the handle alone.
    const BwdPlan w = plan_bwd(c, nseq, L, wgrad_pairing(c, M, e->wgrad_pairs));
    if (saved_bytes < p.total || workspace_bytes < w.total) return QST_ERR_WORKSPACE;
    const bool pairing = w.dsb[1] != w.dsb[0] && layer_hi - layer_lo >= 2 && !(flags & (QST_BWD_SKIP_WGRAD | QST_BWD_WGRAD_ONLY));
    const uint16_t* sh = (const uint16_t*)shadow;
    auto WT = [&](int seg) { return sh + lay.segs[seg].shadow_off + qst_align_up(lay.segs[seg].numel, kAlign); };

    float* dxa = (float*)(ws + w.dxa);
    float* dxb = (float*)(ws + w.dxb);
    float* ds = (float*)(ws + w.ds);
    void* dctx = ws + w.dctx;
    // The dY set of layer l. A pairing call alternates from its top layer down, so that a layer's tensors outlive the layer
    // below it; the top layer of every call -- whose dsb the QKV dgrad of the call above has written in fused mode -- and
    // every layer of a call that does not pair use set 0.
    auto set_of = [&](int l) { return pairing && l >= layer_lo ? (layer_hi - 1 - l) & 1 : 0; };
    // LayerNorm gamma/beta gradients: every ln_bwd of this call writes per-block partials into its own slot; one
    // batched launch at the end reduces them all (13 small launches per step -> 1-7)
    QstLnReduceBatch lnb{};
    lnb.H = H;
    lnb.nblocks = (int)(qst_ln_bwd_scratch_bytes(M, H) / ((size_t)2 * H * sizeof(float)));
    // H = 384: every LayerNorm backward except the top one (whose input comes from the pooling head, not from a GEMM)
    // runs inside the epilogue of the dgrad GEMM that produces its input; those write one partial row per 128-row tile
    const bool fuse_ln = fuse_ln_rows(H, M, e->ln_fusion);
    // dropout: the masks of the forward that filled `saved` are recomputed from its (seed, step) snapshot in the arena and
    // ITS thresholds (recorded by that forward, process-wide: any handle of the same model may run the backward)
    QST_TRY(backward_dropout(ops.arena_kind, p.dropst));
    const bool fuse_ffn = fuse_ln && !dropping && (e->ffn_chain & 4) && qst_ffn_chain_supported(H, I) != 0;
    const int fused_rows = (M + qst_gemm_nt_ln_block_rows_m(H, M) - 1) / qst_gemm_nt_ln_block_rows_m(H, M);
    auto ln_slot = [&](int slot, float* dg, float* db, int nrows = 0) {
        float* sp = (float*)(ws + w.lnred + (size_t)slot * w.lnred_stride);
        lnb.partials[lnb.count] = sp; lnb.dgamma[lnb.count] = dg; lnb.dbeta[lnb.count] = db;
        lnb.nblocks_each[lnb.count] = nrows;
        ++lnb.count;
        return sp;
    };
    float* drel = nullptr;
    if (c.arch == QST_ARCH_MPNET) {
        drel = (float*)(ws + w.drel);
        rel = F(p.rel);
        if (flags & QST_BWD_HEAD) QST_HIP_CHECK(hipMemsetAsync(drel, 0, (size_t)A * 2 * L * 4, st));
    }
    if (flags & QST_BWD_HEAD) QST_TRY(head_bwd(grad_emb, p.pooled, p.argmax, dxa));
    // all four weight gradients (+ bias gradients) of a layer in one grouped launch, or those of layers l_up and l_up - 1
    auto wgrad = [&](int l_up, int layers) -> int {
        QstTnGroup grp{};
        grp.nprob = 4 * layers;
        grp.splits = 0;
        for (int k = 0; k < layers; ++k) {
            const int l = l_up - k, s = set_of(l);
            const LayerAct& a = p.layers[l];
            const int b = lay.layer0[l];
            const void* xin_b = (l == 0) ? (const void*)(sv + p.x0b) : (const void*)(sv + p.layers[l - 1].xb);
            wgrad_shapes(grp, 4 * k, M, H, I);
            auto set = [&](int i, const void* dY, const void* X, int wseg, int bseg) {
                QstGemmArgs& q = grp.prob[4 * k + i];
                q.A = dY; q.B = X; q.C = G(wseg); q.colsum = G(bseg);
            };
            set(0, ws + w.dsb[s], sv + a.hact, b + W_2, b + B_2);          // dW2 [H, I]
            set(1, ws + w.du[s], sv + a.y1b, b + W_1, b + B_1);            // dW1 [I, H]
            set(2, ws + w.dsb1[s], sv + a.ctx, b + W_O, b + B_O);          // dWo [H, H]
            set(3, ws + w.dqkv[s], xin_b, b + W_QKV, b + B_QKV);           // dWqkv [3H, H]
        }
        return ops.gemm_tn_group(&grp, st);
    };
    // the dY tensors of exactly one layer live in the workspace: the one whose stage ran with QST_BWD_SKIP_WGRAD
    if (flags & QST_BWD_WGRAD_ONLY) return wgrad(layer_lo, 1);
    for (int l = layer_hi - 1; l >= layer_lo; --l) {
        const LayerAct& a = p.layers[l];
        const int b = lay.layer0[l];
        const int s = set_of(l);
        void *dsb = ws + w.dsb[s], *dsb1 = ws + w.dsb1[s], *du = ws + w.du[s], *dqkv = ws + w.dqkv[s];
        // LN2 -> ds2 (fp32 for the residual path, bf16 for the GEMMs). Fused mode: only the top layer runs it as a
        // row kernel; below, (ds, dsb) were written by the QKV dgrad of layer l+1.
        if (!fuse_ln || l == c.num_layers - 1)
            QST_TRY(ops.ln_bwd_drop(dxa, sv + a.xh2, F(a.rs2), P(b + LN2_G), M, H, ds, dsb, nullptr, nullptr,
                                    ln_slot(2 * l + 1, G(b + LN2_G), G(b + LN2_B)), nullptr,
                                    active(hidden(QST_DROP_SITE_FFN_OUT(l))), st));
        // FFN2 dgrad through GELU: du = (ds2 . W2) * gelu'(u)   (a.u holds gelu'(u), written by the forward epilogue)
        if (!fuse_ffn) QST_TRY(nt(dsb, WT(b + W_2), du, I, H, QST_EPI_GELU_BWD, {.aux = sv + a.u}));
        // FFN1 dgrad + residual: dy1 = du . W1 + ds2 ; LN1 backward -> ds1 (fp32 in `ds1`, bf16 in dsb1)
        const float* ds1 = ds;
        const QstDrop d1 = hidden(QST_DROP_SITE_ATTN_OUT(l));
        if (fuse_ffn) {
            // both dgrads of the feed-forward block and the LayerNorm-1 backward in one kernel; du is written once
            // (the weight gradients need it) and never read back by this chain
            QST_TRY(ffn({.A = dsb, .B1 = WT(b + W_2), .B2 = WT(b + W_1), .resid = ds, .aux = sv + a.u, .save_h = du, .C = dxb,
                         .C2 = dsb1},
                        1, {.gamma = P(b + LN1_G), .xhat = sv + a.xh1, .rstd = F(a.rs1),
                            .partials = ln_slot(2 * l, G(b + LN1_G), G(b + LN1_B), fused_rows)}));
            ds1 = dxb;
        } else if (fuse_ln) {
            QST_TRY(nt_ln(du, WT(b + W_1), dxb, I, 1, {.C2 = dsb1, .resid = ds, .drop = d1, .drop_where = 2},
                          {.gamma = P(b + LN1_G), .xhat = sv + a.xh1, .rstd = F(a.rs1),
                           .partials = ln_slot(2 * l, G(b + LN1_G), G(b + LN1_B), fused_rows)}));
            ds1 = dxb;
        } else {
            QST_TRY(nt(du, WT(b + W_1), dxb, H, I, QST_EPI_F32_RESID, {.resid = ds}));
            QST_TRY(ops.ln_bwd_drop(dxb, sv + a.xh1, F(a.rs1), P(b + LN1_G), M, H, ds, dsb1, nullptr, nullptr,
                                    ln_slot(2 * l, G(b + LN1_G), G(b + LN1_B)), nullptr, active(d1), st));
        }
        // attention output projection dgrad, attention core
        QST_TRY(nt(dsb1, WT(b + W_O), dctx, H, H, QST_EPI_BF16));
        QstAttnDesc q = attn(l, sv + a.qkv, sv + a.ctx, F(a.lse));
        q.dctx = dctx; q.dqkv = dqkv; q.drel = drel; q.delta_scratch = (float*)(ws + w.delta);
        QST_TRY(ops.attention_bwd_ex(&q, st));
        // pairs from the bottom of the call: (lo + 1, lo), (lo + 3, lo + 2), ...; with an odd count the top layer is alone.
        // A pair's launch sits where the lower layer's did; the upper layer's operands wait in their own set.
        if (!pairing) {
            if (!(flags & QST_BWD_SKIP_WGRAD)) QST_TRY(wgrad(l, 1));
        } else if (((l - layer_lo) & 1) == 0) {
            QST_TRY(wgrad(l + 1 < layer_hi ? l + 1 : l, l + 1 < layer_hi ? 2 : 1));
        }
        // QKV projection dgrad + residual: dx_in = dqkv . Wqkv + ds1. Fused mode: followed in the same kernel by the
        // backward of the LayerNorm that produced this layer's input (LN2 of layer l-1, or the embedding LayerNorm)
        if (fuse_ln && l > 0) {
            const LayerAct& lo = p.layers[l - 1];
            const int bl = lay.layer0[l - 1];
            // dsb of layer l - 1 = d(FFN-2 output of layer l-1)
            QST_TRY(nt_ln(dqkv, WT(b + W_QKV), ds, 3 * H, 1,
                          {.C2 = ws + w.dsb[set_of(l - 1)], .resid = ds1, .drop = hidden(QST_DROP_SITE_FFN_OUT(l - 1)), .drop_where = 2},
                          {.gamma = P(bl + LN2_G), .xhat = sv + lo.xh2, .rstd = F(lo.rs2),
                           .partials = ln_slot(2 * (l - 1) + 1, G(bl + LN2_G), G(bl + LN2_B), fused_rows)}));
        } else if (fuse_ln) {
            // the embedding dropout follows its LayerNorm
            QST_TRY(nt_ln(dqkv, WT(b + W_QKV), ds, 3 * H, 1, {.resid = ds1, .drop = hidden(QST_DROP_SITE_EMBED), .drop_where = 3},
                          {.gamma = P(lay.eg), .xhat = sv + p.xh0, .rstd = F(p.rs0),
                           .partials = ln_slot(2 * c.num_layers, G(lay.eg), G(lay.eb), fused_rows)}));
        } else {
            QST_TRY(nt(dqkv, WT(b + W_QKV), dxa, H, 3 * H, QST_EPI_F32_RESID, {.resid = ds1}));
        }
    }
    const bool do_embed = (flags & QST_BWD_EMBED) != 0;
    if (do_embed && !fuse_ln)
        QST_TRY(ops.ln_bwd_drop(dxa, sv + p.xh0, F(p.rs0), P(lay.eg), M, H, ds, nullptr, nullptr, nullptr,
                                ln_slot(2 * c.num_layers, G(lay.eg), G(lay.eb)), active(hidden(QST_DROP_SITE_EMBED)), nullptr, st));
    if (lnb.count > 0) {
        if (lnb.count > QST_LN_BATCH_MAX) return QST_ERR_UNSUPPORTED;
        QST_TRY(qst_ln_bwd_reduce_batch(&lnb, st));
    }
    if (!do_embed) return QST_OK;
    // embeddings
    QST_TRY(qst_embed_bwd(ds, ids, type_ids, (const int32_t*)(sv + p.pos_ids), nseq, L, H, c.type_vocab_size,
                          G(lay.word), G(lay.pos), G(lay.type), st));
    if (c.arch == QST_ARCH_MPNET) QST_TRY(qst_rel_pos_bwd(drel, e->rel_lut, c.rel_buckets, A, L, G(lay.rel), st));
    return QST_OK;
}

}  // namespace

extern "C" int qst_refresh_shadow(const qst_encoder* e, const float* params, void* shadow, void* stream) {
    if (!e || !params || !shadow) return QST_ERR_BAD_ARG;
    // (a QST_PREC_F16 / F16W handle fills the same layout with IEEE half; every other handle with bf16)
    if (e->cfg.precision == QST_PREC_F16W)
        return qst_shadow_all_split_f16(params, shadow, (uint16_t*)shadow + e->lay.shadow_total, e->shadow_tab, e->shadow_nseg,
                                        e->shadow_blocks, stream);
    return op_kernels(e->cfg).shadow_all(params, shadow, e->shadow_tab, e->shadow_nseg, e->shadow_blocks, stream);
}

// QST_PREC_FP8: every GEMM weight as MXFP8 -- e4m3 bytes at the segment's shadow offset, E8M0 block scales (one per 32
// input features of an output row) behind them at shadow_off + align(numel); the buffer is qst_shadow8_bytes() long.
extern "C" int qst_refresh_shadow_mx(const qst_encoder* e, const float* params, void* shadow_mx, void* stream) {
    if (!e || !params || !shadow_mx) return QST_ERR_BAD_ARG;
    for (const Seg& s : e->lay.segs) {
        if (!s.gemm) continue;
        if (s.cols % 32 != 0) return QST_ERR_UNSUPPORTED;
        uint8_t* q = (uint8_t*)shadow_mx + s.shadow_off;
        uint8_t* sc = q + qst_align_up(s.numel, kAlign);
        int rc = qst_quant_mx(params + s.off, 0, s.rows, s.cols, q, sc, stream);
        if (rc != QST_OK) return rc;
    }
    return QST_OK;
}

extern "C" int qst_encoder_forward(qst_encoder* e, const int64_t* ids, const int64_t* mask, const int64_t* type_ids,
                                   int nseq, int L, const float* params, const void* shadow, float* out_emb,
                                   float* out_tok, void* saved, size_t saved_bytes, int training, void* stream) {
    if (!e || !ids || !mask || !params || !out_emb || !saved) return QST_ERR_BAD_ARG;
    QST_TRY(shape_ok(e, nseq, L));
    const int prec = e->cfg.precision;
    if (prec != QST_PREC_BF16X3 && !shadow) return QST_ERR_BAD_ARG;
    Pass ps(e, ids, mask, type_ids, nseq, L, params, saved, stream, true);
    if (prec == QST_PREC_BF16X3)
        return training ? ps.forward_x3_train(out_emb, out_tok, saved_bytes) : ps.forward_x3(out_emb, out_tok, saved_bytes);
    if (prec == QST_PREC_FP8) return ps.forward_fp8(shadow, out_emb, out_tok, saved_bytes, training != 0);
    return ps.forward_op16(shadow, out_emb, out_tok, saved_bytes, training != 0);
}

// Stages of one backward pass, top to bottom: head (pool/normalise), layers N-1..0, embeddings. A caller may run
// them in several calls (layer_hi > layer_lo) to launch the gradient all-reduce of finished layers in between;
// the running d(loss)/d(x) lives in the workspace between calls.
//
// qst_encoder_backward_stage adds two flags for the LAST layer range of a data-parallel step: with
// QST_BWD_SKIP_WGRAD the range's weight-gradient launch is left out (its operands stay in the workspace), so the
// caller can finish the embedding stage first, start the all-reduce of the embedding gradients -- half of a MiniLM
// arena, and otherwise the one bucket with nothing left to hide behind -- and then run the postponed launch with
// QST_BWD_WGRAD_ONLY underneath it.
extern "C" int qst_encoder_backward_stage(qst_encoder* e, const int64_t* ids, const int64_t* mask,
                                          const int64_t* type_ids, int nseq, int L, const float* params,
                                          const void* shadow, const float* grad_emb, float* grads, void* saved,
                                          size_t saved_bytes, void* workspace, size_t workspace_bytes,
                                          int flags, int layer_hi, int layer_lo, void* stream) {
    const int do_head = (flags & QST_BWD_HEAD) != 0, do_embed = (flags & QST_BWD_EMBED) != 0;
    const bool skip_wgrad = (flags & QST_BWD_SKIP_WGRAD) != 0, wgrad_only = (flags & QST_BWD_WGRAD_ONLY) != 0;
    if (wgrad_only && (skip_wgrad || do_head || do_embed)) return QST_ERR_BAD_ARG;
    // postponing a layer's weight gradients is sound for layer 0 only: the stage of layer l - 1 overwrites the gradients
    // (ds / dsb / du / dqkv in the workspace) that layer l's launch reads
    if ((skip_wgrad || wgrad_only) && (layer_lo != 0 || layer_hi != 1)) return QST_ERR_BAD_ARG;
    if (!e || !ids || !mask || !params || !grads || !saved || !workspace) return QST_ERR_BAD_ARG;
    // the parity path (no shadow) is staged like the bf16 one, without the postponed weight-gradient launch of layer 0
    const bool x3 = e->cfg.precision == QST_PREC_BF16X3;
    if (x3 && (skip_wgrad || wgrad_only)) return QST_ERR_UNSUPPORTED;
    if (!x3 && !shadow) return QST_ERR_BAD_ARG;
    if (do_head && !grad_emb) return QST_ERR_BAD_ARG;
    if (layer_lo < 0 || layer_hi > e->cfg.num_layers || layer_lo > layer_hi) return QST_ERR_BAD_ARG;
    QST_TRY(shape_ok(e, nseq, L));
    Pass ps(e, ids, mask, type_ids, nseq, L, params, saved, stream, false);
    ps.ws = (char*)workspace;
    ps.grads = grads;
    QST_TRY(ps.check_pool(x3 ? ARENA_X3 : ps.ops.arena_kind));
    if (x3) return ps.backward_x3(grad_emb, saved_bytes, workspace_bytes, flags, layer_hi, layer_lo);
    return ps.backward_op16(shadow, grad_emb, saved_bytes, workspace_bytes, flags, layer_hi, layer_lo);
}

extern "C" int qst_encoder_backward_partial(qst_encoder* e, const int64_t* ids, const int64_t* mask,
                                            const int64_t* type_ids, int nseq, int L, const float* params,
                                            const void* shadow, const float* grad_emb, float* grads, void* saved,
                                            size_t saved_bytes, void* workspace, size_t workspace_bytes,
                                            int do_head, int layer_hi, int layer_lo, int do_embed, void* stream) {
    return qst_encoder_backward_stage(e, ids, mask, type_ids, nseq, L, params, shadow, grad_emb, grads, saved, saved_bytes,
                                      workspace, workspace_bytes, (do_head ? QST_BWD_HEAD : 0) | (do_embed ? QST_BWD_EMBED : 0),
                                      layer_hi, layer_lo, stream);
}

extern "C" int qst_encoder_backward(qst_encoder* e, const int64_t* ids, const int64_t* mask, const int64_t* type_ids,
                                    int nseq, int L, const float* params, const void* shadow, const float* grad_emb,
                                    float* grads, void* saved, size_t saved_bytes, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    if (!e) return QST_ERR_BAD_ARG;
    return qst_encoder_backward_partial(e, ids, mask, type_ids, nseq, L, params, shadow, grad_emb, grads, saved,
                                        saved_bytes, workspace, workspace_bytes, 1, e->cfg.num_layers, 0, 1, stream);
}

// The arena group and the hyper-parameters every optimiser entry point takes; each entry adds its own fields (optim.hip).
static AdamStep adam_step(const qst_encoder* e, float* params, float* grads, float* exp_avg, float* exp_avg_sq, float lr,
                          float beta1, float beta2, float eps, float weight_decay, float max_grad_norm, float grad_scale,
                          float* norm_out, float* scratch) {
    AdamStep s = {};
    s.arena = {params, grads, exp_avg, exp_avg_sq, e->chunk_decay, e->lay.total};
    s.lr = lr; s.beta1 = beta1; s.beta2 = beta2; s.eps = eps; s.wd = weight_decay; s.max_norm = max_grad_norm;
    s.grad_scale = grad_scale; s.norm_out = norm_out; s.scratch = scratch;
    return s;
}

extern "C" int qst_clip_adamw_step_sched(const qst_encoder* e, float* params, float* grads, float* exp_avg,
                                         float* exp_avg_sq, float base_lr, float beta1, float beta2, float eps,
                                         float weight_decay, float max_grad_norm, float grad_scale,
                                         int64_t warmup_steps, int64_t total_steps, int64_t* step_dev,
                                         float* norm_out, float* scratch, void* stream) {
    if (!e) return QST_ERR_BAD_ARG;
    AdamStep s = adam_step(e, params, grads, exp_avg, exp_avg_sq, base_lr, beta1, beta2, eps, weight_decay, max_grad_norm,
                           grad_scale, norm_out, scratch);
    s.step_dev = step_dev; s.warmup = warmup_steps; s.total = total_steps;
    return qst_adamw_run(s, (hipStream_t)stream);
}

extern "C" int qst_clip_adamw_step_amp(const qst_encoder* e, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                                       float base_lr, float beta1, float beta2, float eps, float weight_decay,
                                       float max_grad_norm, float grad_scale, int64_t warmup_steps, int64_t total_steps,
                                       int64_t* step_dev, float* scaler_dev, float growth_factor, float backoff_factor,
                                       int32_t growth_interval, float* norm_out, float* scratch, void* stream) {
    if (!e || !scaler_dev) return QST_ERR_BAD_ARG;          // (without a scaler the descriptor would be the _sched step)
    AdamStep s = adam_step(e, params, grads, exp_avg, exp_avg_sq, base_lr, beta1, beta2, eps, weight_decay, max_grad_norm,
                           grad_scale, norm_out, scratch);
    s.step_dev = step_dev; s.warmup = warmup_steps; s.total = total_steps;
    s.scaler = scaler_dev; s.growth = growth_factor; s.backoff = backoff_factor; s.interval = growth_interval;
    return qst_adamw_run(s, (hipStream_t)stream);
}

extern "C" int qst_clip_adamw_step(const qst_encoder* e, float* params, float* grads, float* exp_avg,
                                   float* exp_avg_sq, float lr, float beta1, float beta2, float eps,
                                   float weight_decay, float max_grad_norm, float grad_scale, int64_t step,
                                   float* norm_out, float* scratch, void* stream) {
    if (!e) return QST_ERR_BAD_ARG;
    AdamStep s = adam_step(e, params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, max_grad_norm,
                           grad_scale, norm_out, scratch);
    s.step = step;
    return qst_adamw_run(s, (hipStream_t)stream);
}

extern "C" int qst_clip_adamw_step_joint(const qst_encoder* e, float* params, float* grads, float* exp_avg,
                                         float* exp_avg_sq, float* x_params, float* x_grads, float* x_exp_avg,
                                         float* x_exp_avg_sq, const uint8_t* x_chunk_decay, int64_t x_n, float lr,
                                         float beta1, float beta2, float eps, float weight_decay, float max_grad_norm,
                                         float grad_scale, int64_t step, float* norm_out, float* scratch, void* stream) {
    if (!e) return QST_ERR_BAD_ARG;
    AdamStep s = adam_step(e, params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, max_grad_norm,
                           grad_scale, norm_out, scratch);
    s.extra = {x_params, x_grads, x_exp_avg, x_exp_avg_sq, x_chunk_decay, x_n};
    s.step = step;
    return qst_adamw_run(s, (hipStream_t)stream);
}

extern "C" int64_t qst_abi_sizeof(int which) {
    switch (which) {
        case 0: return sizeof(QstGemmArgs);
        case 1: return sizeof(QstLnEpi);
        case 2: return sizeof(QstFfnArgs);
        case 3: return sizeof(QstTnGroup);
        case 4: return sizeof(QstLnReduceBatch);
        case 5: return sizeof(QstDrop);
        case 6: return sizeof(QstAttnDesc);
        default: return QST_ERR_BAD_ARG;
    }
}
