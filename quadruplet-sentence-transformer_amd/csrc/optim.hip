// optim.hip -- global-norm gradient clipping + AdamW over the flat parameter arena (HBM-bound, 28 B/param).
//
// Replaces torch.nn.utils.clip_grad_norm_(loss_model.parameters(), max_grad_norm) followed by
// torch.optim.AdamW(lr, betas=(0.9,0.999), eps=1e-8, weight_decay on all but bias/LayerNorm).step()
// and optimizer.zero_grad() as SentenceTransformer.fit runs them (sentence-transformers 2.2.2;
// reference call site training/main.py:128-148).
// The clip coefficient is computed on the device from the reduced norm: no host sync in the step.
//
// There is one step (qst_adamw_run over an AdamStep, qst_common.h) with three options, which the four
// qst_clip_adamw_step* entry points of qst_api.hip select by what they fill in:
//   extra group      a second flat buffer with the arena's conventions, clipped on the joint norm     (_joint)
//   device schedule  step counter, WarmupLinear lr and bias corrections derived on the device          (_sched, _amp)
//   GradScaler       unscale / skip / grow / back off, decided on the device from the scaled norm      (_amp)
// Launches: sumsq_kernel <<<1024, 256>>> [+ one over the extra group] -> norm_finish_kernel <<<1, 1024>>> ->
// adamw_kernel <<<2048, 256>>> [+ one over the extra group]. Without the schedule the norm launches run only when the
// step clips or reports the norm. Nothing else goes onto the stream, so every form can be captured into a graph.
#include "qst_common.h"
#include "qst_kernels.h"

namespace {

constexpr int kNormBlocks = 1024;

__global__ __launch_bounds__(256) void sumsq_kernel(const float* g, int64_t n4, float* partial) {
    float s = 0.f;
    const f32x4* g4 = (const f32x4*)g;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const f32x4 v = g4[i];
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    __shared__ float red[4];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// Device-side schedule (graph-capturable step: no per-step host value reaches a kernel argument), active when `step` is not
// null: one thread advances the step counter and derives this step's learning rate and Adam bias corrections into
// dyn[0..2] = {lr, 1-beta1^t, sqrt(1-beta2^t)}.
struct SchedArgs { int64_t* step; float base_lr, beta1, beta2; int64_t warmup, total; float* dyn; };

// Mixed precision (qst_clip_adamw_step_amp, include/qst.h), active when `scaler` is not null (then the schedule is too):
// torch.cuda.amp.GradScaler's unscale_ / step / update and ST fit()'s "skip the scheduler when the scale changed", decided by
// one thread from the reduced norm of the SCALED gradients. It adds dyn[3..4] = {unscale factor (grad_scale / scale),
// 1.0 if this step is skipped}.
struct AmpArgs { float* scaler; float growth, backoff; int interval; };

// transformers.get_linear_schedule_with_warmup (as trainer.warmup_linear_lr) after k scheduler steps; total <= 0: constant
__device__ float sched_lr(const SchedArgs& sc, int64_t k) {
    if (sc.total <= 0) return sc.base_lr;
    if (k < sc.warmup) return sc.base_lr * (float)((double)k / (double)(sc.warmup > 1 ? sc.warmup : 1));
    const int64_t den = sc.total - sc.warmup > 1 ? sc.total - sc.warmup : 1;
    const double f = (double)(sc.total - k) / (double)den;
    return sc.base_lr * (float)(f > 0.0 ? f : 0.0);
}

// The second stage of the norm, and everything one thread decides from it. Thread i adds partial i of the extra group
// (nx == 0: no such group, nothing is added) to partial i of the arena; one tree over the 1024 sums.
__global__ __launch_bounds__(1024) void norm_finish_kernel(const float* partial, int n, const float* xpartial, int nx,
                                                           float grad_scale, float* norm_out, SchedArgs sc, AmpArgs am) {
    __shared__ float red[16];
    float s = threadIdx.x < n ? partial[threadIdx.x] : 0.f;
    if (threadIdx.x < nx) s += xpartial[threadIdx.x];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();                                        // (every xpartial is read by here: dyn may lie over them)
    if (threadIdx.x >= 64) return;
    float v = threadIdx.x < 16 ? red[threadIdx.x] : 0.f;
    v = wave_sum(v);
    if (threadIdx.x != 0) return;
    float unscale = fabsf(grad_scale), scale = 0.f;
    if (am.scaler) { scale = am.scaler[0]; unscale = unscale / scale; }
    const float norm = sqrtf(v) * unscale;                  // amp: inf / nan in any gradient -> not finite
    norm_out[0] = norm;
    if (!sc.step) return;
    bool ok = true;
    int64_t k = sc.step[0];                                 // scheduler steps already taken: the optimiser's, without amp
    if (am.scaler) {
        ok = fabsf(norm) < 3.0e38f;                         // (false for inf and for nan)
        float new_scale = scale, tracker = am.scaler[1];
        if (!ok) {
            if (am.interval > 0) new_scale = scale * am.backoff;
            tracker = 0.f;
        } else {
            tracker += 1.f;
            if (am.interval > 0 && tracker >= (float)am.interval) { new_scale = scale * am.growth; tracker = 0.f; }
        }
        am.scaler[0] = new_scale; am.scaler[1] = tracker;
        am.scaler[2] = ok ? 0.f : 1.f;
        if (!ok) am.scaler[3] += 1.f;
        k = sc.step[1];                                     // ... with amp a counter of its own:
        if (new_scale == scale) sc.step[1] = k + 1;         // ST fit(): skip_scheduler = scaler.get_scale() != scale_before_step
        sc.dyn[3] = unscale;
        sc.dyn[4] = ok ? 0.f : 1.f;
    }
    const int64_t t = sc.step[0] + (ok ? 1 : 0);            // 1-based optimiser step; a skipped step does not count
    sc.step[0] = t;
    const int64_t tt = t > 0 ? t : 1;                       // (only a skipped first step has t == 0)
    sc.dyn[0] = sched_lr(sc, k);
    sc.dyn[1] = (float)(1.0 - pow((double)sc.beta1, (double)tt));
    sc.dyn[2] = (float)sqrt(1.0 - pow((double)sc.beta2, (double)tt));
}

__global__ void amp_scaler_init_kernel(float* sc, float init_scale) { sc[0] = init_scale; sc[1] = 0.f; sc[2] = 0.f; sc[3] = 0.f; }

struct AdamArgs {
    float* p; float* g; float* m; float* v;
    const uint8_t* chunk_decay;     // one flag per 256-element chunk of the arena
    const float* norm;              // device scalar (pre-clip global norm), or null
    const float* dyn;               // device {lr, bc1, bc2_sqrt} (device-side schedule), or null: the by-value fields
    int64_t n4;
    float lr, beta1, beta2, eps, wd, max_norm, grad_scale, bc1, bc2_sqrt;
    int amp;                        // dyn[3] = the gradient factor (grad_scale / loss scale), dyn[4] != 0: skip this step
};

__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs a) {
    if (a.dyn) { a.lr = a.dyn[0]; a.bc1 = a.dyn[1]; a.bc2_sqrt = a.dyn[2]; }
    float coef = a.grad_scale;
    if (a.amp) {
        coef = a.dyn[3];
        if (a.dyn[4] != 0.f) {      // an overflowed step (GradScaler.step skips optimizer.step()): only optimizer.zero_grad()
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            f32x4* g4 = (f32x4*)a.g;
            for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n4; i += (int64_t)gridDim.x * 256) st_stream(g4 + i, z);
            return;
        }
    }
    if (a.norm && a.max_norm > 0.f) {
        const float c = a.max_norm / (a.norm[0] + 1e-6f);      // clip_grad_norm_: clamp(max_norm/(norm+1e-6), max=1)
        coef *= fminf(c, 1.0f);
    }
    const float step = a.lr / a.bc1;
    f32x4* p4 = (f32x4*)a.p; f32x4* g4 = (f32x4*)a.g; f32x4* m4 = (f32x4*)a.m; f32x4* v4 = (f32x4*)a.v;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n4; i += (int64_t)gridDim.x * 256) {
        const float decay = a.chunk_decay[i >> 6] ? (1.0f - a.lr * a.wd) : 1.0f;   // 64 float4 per 256-element chunk
        // the moments and the (zeroed) gradients are not touched again before the next step: streamed past the caches (step 4.575 ->
        // 4.543 ms, three alternations); the parameters are read next by the bf16 refresh and stay plain (streamed: 4.600 -> 4.627)
        f32x4 p = p4[i], g = ld_stream(g4 + i), m = ld_stream(m4 + i), v = ld_stream(v4 + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gg = g[k] * coef;
            p[k] *= decay;
            m[k] = m[k] + (1.0f - a.beta1) * (gg - m[k]);                // exp_avg.lerp_(grad, 1-beta1)
            v[k] = a.beta2 * v[k] + (1.0f - a.beta2) * gg * gg;
            const float denom = sqrtf(v[k]) / a.bc2_sqrt + a.eps;
            p[k] -= step * (m[k] / denom);
            g[k] = 0.f;                                                  // optimizer.zero_grad()
        }
        p4[i] = p; st_stream(m4 + i, m); st_stream(v4 + i, v); st_stream(g4 + i, g);
    }
}

}  // namespace

extern "C" int qst_amp_scaler_init(float* scaler_dev, float init_scale, void* stream) {
    if (!scaler_dev || !(init_scale > 0.f) || !(init_scale < 3.0e38f)) return QST_ERR_BAD_ARG;
    amp_scaler_init_kernel<<<1, 1, 0, (hipStream_t)stream>>>(scaler_dev, init_scale);
    QST_LAUNCH_CHECK();
    return QST_OK;
}

// The one step behind the qst_clip_adamw_step* entry points (AdamStep, qst_common.h). Every refusal comes before the first
// launch. A step counts from the device counter or from the host's 1-based `step`: a descriptor with neither (a scheduled
// entry point that was handed no step_dev leaves step at 0) is refused.
int qst_adamw_run(const AdamStep& s, hipStream_t st) {
    const AdamGroup& A = s.arena;
    const AdamGroup& X = s.extra;
    const bool sched = s.step_dev != nullptr;
    if (!A.p || !A.g || !A.m || !A.v || !A.chunk_decay || A.n <= 0 || (A.n & 255)) return QST_ERR_BAD_ARG;
    if (!sched && s.step < 1) return QST_ERR_BAD_ARG;
    if (X.n < 0 || (X.n & 255)) return QST_ERR_BAD_ARG;
    if (X.n > 0 && (!X.p || !X.g || !X.m || !X.v || !X.chunk_decay)) return QST_ERR_BAD_ARG;
    if (s.scaler && (!sched || !(s.growth >= 1.f) || !(s.backoff > 0.f && s.backoff <= 1.f))) return QST_ERR_BAD_ARG;
    const bool want_norm = sched || s.max_norm > 0.f || s.norm_out;
    if (want_norm && (!s.norm_out || !s.scratch)) return QST_ERR_BAD_ARG;
    const int64_t xn4 = X.n / 4;
    // scratch: the arena's partial sums, then the extra group's; dyn lies over the latter, which norm_finish_kernel has
    // read by the time it writes dyn and which the next step's sumsq_kernel writes afresh
    float* dyn = sched ? s.scratch + kNormBlocks : nullptr;
    if (want_norm) {
        sumsq_kernel<<<kNormBlocks, 256, 0, st>>>(A.g, A.n / 4, s.scratch);
        QST_LAUNCH_CHECK();
        const int xblocks = (int)(xn4 < (int64_t)kNormBlocks * 256 ? (xn4 + 255) / 256 : kNormBlocks);
        if (xblocks > 0) {
            sumsq_kernel<<<xblocks, 256, 0, st>>>(X.g, xn4, s.scratch + kNormBlocks);
            QST_LAUNCH_CHECK();
        }
        SchedArgs sc;
        sc.step = s.step_dev; sc.base_lr = s.lr; sc.beta1 = s.beta1; sc.beta2 = s.beta2; sc.warmup = s.warmup;
        sc.total = s.total; sc.dyn = dyn;
        AmpArgs am;
        am.scaler = s.scaler; am.growth = s.growth; am.backoff = s.backoff; am.interval = s.interval;
        norm_finish_kernel<<<1, 1024, 0, st>>>(s.scratch, kNormBlocks, s.scratch + kNormBlocks, xblocks, s.grad_scale,
                                               s.norm_out, sc, am);
        QST_LAUNCH_CHECK();
    }
    AdamArgs a;
    a.p = A.p; a.g = A.g; a.m = A.m; a.v = A.v; a.chunk_decay = A.chunk_decay;
    a.dyn = dyn; a.amp = s.scaler != nullptr;
    a.norm = (s.max_norm > 0.f) ? s.norm_out : nullptr;
    a.n4 = A.n / 4;
    a.lr = s.lr; a.beta1 = s.beta1; a.beta2 = s.beta2; a.eps = s.eps; a.wd = s.wd; a.max_norm = s.max_norm;
    a.grad_scale = s.grad_scale;
    a.bc1 = a.bc2_sqrt = 1.f;       // (with dyn, adamw_kernel takes lr and both corrections from there)
    if (!sched) {                   // on the host in double: a device pow need not round as this one does
        a.bc1 = (float)(1.0 - pow((double)s.beta1, (double)s.step));
        a.bc2_sqrt = (float)sqrt(1.0 - pow((double)s.beta2, (double)s.step));
    }
    adamw_kernel<<<2048, 256, 0, st>>>(a);
    QST_LAUNCH_CHECK();
    if (X.n > 0) {                  // the same coefficient, learning rate and step on the extra group
        a.p = X.p; a.g = X.g; a.m = X.m; a.v = X.v; a.chunk_decay = X.chunk_decay;
        a.n4 = xn4;
        adamw_kernel<<<(int)(xn4 < 2048 * 256 ? (xn4 + 255) / 256 : 2048), 256, 0, st>>>(a);
        QST_LAUNCH_CHECK();
    }
    return QST_OK;
}
