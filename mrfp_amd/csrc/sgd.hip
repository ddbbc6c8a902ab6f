// sgd.hip -- fused SGD(momentum, weight decay) step over a flat fp32 arena: one launch for all
// 192 trainable tensors (40.35 M elements), 16-byte loads, HBM-bound (reads p, g, m; writes p, m).
//
// Replaces (reference): torch.optim.SGD(lr=1e-2, momentum=0.9, weight_decay=5e-4).step() with the
// LambdaLR poly factor folded into `lr` (main.py:826-839, 863-864).  Update rule of torch.optim.SGD:
//   g' = g*gscale + wd*p ;  m = g' (first step) | mu*m + g' ;  p -= lr*m
// gscale = 1/world_size folds the gradient averaging of the data-parallel all-reduce in.
//
// Checked form (no reference counterpart: the reference trains in fp32; yardstick torch.amp.GradScaler + clip_grad_norm_):
// mrfp_grad_check reads the gradient arena once more and leaves {found_inf, grad_norm, gmul, new loss scale} in a device step
// state, mrfp_sgd_step_checked applies the same update with gmul in place of gscale, or nothing at all.
//
// Averaged forms (no reference counterpart; yardstick torch.optim.swa_utils.AveragedModel): mrfp_sgd_step_avg and
// mrfp_sgd_step_checked_avg make the same update and, while the fresh p is still in registers, fold it into a fourth arena e, an
// exponential moving average or the running mean of the applied steps (include/mrfp_hip.h: the averaging rule).
#include "common.hpp"

namespace mrfp {

struct StepState {            // the device step state of include/mrfp_hip.h, word by word
    float scale;
    int growth_tracker;
    int found_inf;
    float grad_norm;
    float gmul;
    int taken;
    int skipped;
    int reserved;
};
static_assert(sizeof(StepState) == 32, "step state: eight 32-bit words");

constexpr int kArenaCap = 4096;            // workgroups of the streaming arena kernels (step, checked step, accumulate): 16 per CU

// The update of one 16-byte vector in its three parts, shared by the four step kernels so that p and m leave all of them with the
// same bits:  g' = g*gscale + wd*p ;  m = g' (first step) | mu*m + g' ;  p -= lr*m.
__device__ __forceinline__ void sgd_grad(float4& gv, const float4& pv, float gscale, float wd) {
    gv.x = gv.x * gscale + wd * pv.x; gv.y = gv.y * gscale + wd * pv.y;
    gv.z = gv.z * gscale + wd * pv.z; gv.w = gv.w * gscale + wd * pv.w;
}
__device__ __forceinline__ void sgd_momentum(float4& mv, const float4& gv, float mu) {
    mv.x = mu * mv.x + gv.x; mv.y = mu * mv.y + gv.y; mv.z = mu * mv.z + gv.z; mv.w = mu * mv.w + gv.w;
}
__device__ __forceinline__ void sgd_apply(float4& pv, const float4& mv, float lr) {
    pv.x -= lr * mv.x; pv.y -= lr * mv.y; pv.z -= lr * mv.z; pv.w -= lr * mv.w;
}

__global__ __launch_bounds__(256) void sgd_kernel(float4* __restrict__ p, const float4* __restrict__ g,
                                                  float4* __restrict__ m, int64_t n4, float lr, float mu, float wd,
                                                  float gscale, int first) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 pv = p[i], gv = g[i], mv;
        sgd_grad(gv, pv, gscale, wd);
        if (first) {
            mv = gv;
        } else {
            mv = m[i];
            sgd_momentum(mv, gv, mu);
        }
        sgd_apply(pv, mv, lr);
        m[i] = mv;
        p[i] = pv;
    }
}

// Gradient accumulation over micro-batches: acc = g (first: a bit copy, acc is not read) | acc = acc + g, one fp32 addition per
// element in this operand order, nothing to contract with.  Streams 12 bytes per element (8 when first) against sgd_kernel's 20.
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float4* __restrict__ acc, const float4* __restrict__ g, int64_t n4,
                                                              int first) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 gv = g[i];
        if (!first) {
            const float4 av = acc[i];
            gv.x = av.x + gv.x; gv.y = av.y + gv.y; gv.z = av.z + gv.z; gv.w = av.w + gv.w;
        }
        acc[i] = gv;
    }
}

// ---- checked step: non-finite check + gradient norm + dynamic loss scale, all on the device ------------------------------------
// Semantics of torch.amp.GradScaler (unscale_ -> step -> update) + torch.nn.utils.clip_grad_norm_ without the host read of the
// overflow flag: a partials kernel and a one-workgroup finalize decide, mrfp_sgd_step_checked obeys (include/mrfp_hip.h: StepState).
constexpr int kGradCheckCap = 2048;        // workgroups of the partials kernel (8 per CU: one 16-byte load per lane, 8 waves per SIMD)

struct GradPartial {                       // what one workgroup of grad_check_kernel leaves behind (16 bytes)
    double sumsq;                          // sum of (g * gscale / scale)^2 over its elements
    uint32_t nonfinite;                    // 1 if any RAW element is inf / NaN
    uint32_t pad;
};

__device__ __forceinline__ uint32_t nonfinite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// One pass over g[0..4*n4): per-thread accumulation in double (the chain of a thread is n4 / (grid * 256) vectors long, ~20 at the
// 40 M-element arena), workgroup sum in a fixed order; no float atomics.  The flag looks at the exponent bits of the raw element:
// a large finite gradient whose square overflows is not an overflow.
__global__ __launch_bounds__(256) void grad_check_kernel(const float4* __restrict__ g, int64_t n4, float gscale,
                                                         const StepState* __restrict__ st, GradPartial* __restrict__ part) {
    const double mul = (double)gscale / (double)st->scale;
    double acc = 0.0;
    uint32_t bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 v = g[i];
        bad |= nonfinite_bits(v.x) | nonfinite_bits(v.y) | nonfinite_bits(v.z) | nonfinite_bits(v.w);
        const double x = (double)v.x * mul, y = (double)v.y * mul, z = (double)v.z * mul, w = (double)v.w * mul;
        acc += x * x; acc += y * y; acc += z * z; acc += w * w;
    }
    __shared__ double s_sum[4];
    __shared__ uint32_t s_bad[4];
    acc = wave_sum(acc);
    bad = __any((int)bad) ? 1u : 0u;
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = acc; s_bad[threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        GradPartial p;
        p.sumsq = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        p.nonfinite = s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3];
        p.pad = 0;
        part[blockIdx.x] = p;
    }
}

// One workgroup: the partials in a fixed order and in double, then thread 0 decides (torch._amp_update_scale_, clip_grad_norm_).
__global__ __launch_bounds__(256) void grad_check_finalize_kernel(const GradPartial* __restrict__ part, int nblk, float gscale,
                                                                  StepState* __restrict__ st, int dynamic, float growth,
                                                                  float backoff, int growth_interval, float max_norm) {
    double acc = 0.0;
    uint32_t bad = 0;
    for (int i = threadIdx.x; i < nblk; i += 256) { acc += part[i].sumsq; bad |= part[i].nonfinite; }
    __shared__ double s_sum[4];
    __shared__ uint32_t s_bad[4];
    acc = wave_sum(acc);
    bad = __any((int)bad) ? 1u : 0u;
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = acc; s_bad[threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double norm = sqrt(((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3]);
    const int found = (int)(s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]);
    const float scale = st->scale;
    st->found_inf = found;
    st->grad_norm = (float)norm;
    if (found) {
        st->gmul = 0.f;                                 // (not read: the checked step writes nothing)
        st->skipped += 1;
        if (dynamic) { st->scale = scale * backoff; st->growth_tracker = 0; }
        return;
    }
    double c = (double)max_norm / (norm + 1e-6);        // clip_grad_norm_; max_norm = +inf: no clipping
    if (!(c < 1.0)) c = 1.0;
    st->gmul = (float)((double)gscale / (double)scale * c);
    st->taken += 1;
    if (dynamic) {
        const int ok = st->growth_tracker + 1;
        if (ok == growth_interval) {
            const float grown = scale * growth;
            if (!nonfinite_bits(grown)) st->scale = grown;      // (torch keeps the scale when growing it would overflow)
            st->growth_tracker = 0;
        } else {
            st->growth_tracker = ok;
        }
    }
}

// sgd_kernel with the gradient factor and the go / no-go read from the step state.  found_inf: nothing is written, p and m stay
// bit for bit.  There is no first-step flag -- the host cannot know whether the first step was skipped: the momentum arena is ZERO
// wherever no momentum exists (FlatSGD: zeros_like at construction, zero_() in load_state_dict), and mu*0 + g' == g' is the copy
// torch.optim.SGD's first step makes.
__global__ __launch_bounds__(256) void sgd_checked_kernel(float4* __restrict__ p, const float4* __restrict__ g,
                                                          float4* __restrict__ m, int64_t n4, float lr, float mu, float wd,
                                                          const StepState* __restrict__ st) {
    if (st->found_inf) return;
    const float gscale = st->gmul;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 pv = p[i], gv = g[i], mv = m[i];
        sgd_grad(gv, pv, gscale, wd);
        sgd_momentum(mv, gv, mu);
        sgd_apply(pv, mv, lr);
        m[i] = mv;
        p[i] = pv;
    }
}

// ---- weight averaging inside the step --------------------------------------------------------------------------------------------
// The averaging rule of include/mrfp_hip.h.  t = 1-based count of applied steps; an update happens after step t iff t >= start and
// (t - start) % every == 0, its index is n = (t - start) / every.
struct AvgRule {
    double decay;
    int kind;                              // kAvgEma | kAvgSwa
    int warmup;
    int start;
    int every;
};
constexpr int kAvgEma = 0, kAvgSwa = 1;
constexpr int kAvgNone = 0, kAvgCopy = 1, kAvgLerp = 2;       // what step t does to e

// THE definition of the schedule and of the coefficient on the device (harness.average_coefficient is the one in Python): every
// thread evaluates it once, before its loop, from by-value arguments -- the branch on the result is uniform.  c in double with IEEE
// operations, rounded to float once.
__device__ __forceinline__ int average_rule(const AvgRule& r, int t, float* c) {
    *c = 0.f;
    if (t < r.start || (t - r.start) % r.every != 0) return kAvgNone;
    const int n = (t - r.start) / r.every;
    if (n == 0) return kAvgCopy;
    double cd;
    if (r.kind == kAvgSwa) {
        cd = 1.0 / ((double)n + 1.0);                       // the running arithmetic mean
    } else {
        double d = r.decay;
        if (r.warmup) {
            const double w = (1.0 + (double)n) / (10.0 + (double)n);
            d = w < d ? w : d;
        }
        cd = 1.0 - d;
    }
    *c = (float)cd;
    return kAvgLerp;
}

// e + c*(p - e) as three separately rounded fp32 operations: what torch's `e + c * (p - e)` computes, bit for bit.
__device__ __forceinline__ float avg_lerp(float e, float p, float c) { return __fadd_rn(e, __fmul_rn(c, __fsub_rn(p, e))); }

template <int MODE>
__device__ __forceinline__ void sgd_avg_loop(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                             float4* __restrict__ e, int64_t n4, float lr, float mu, float wd, float gscale,
                                             int first, float c) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 pv = p[i], gv = g[i], mv, ev;
        if (MODE == kAvgLerp) ev = e[i];
        sgd_grad(gv, pv, gscale, wd);
        if (first) {
            mv = gv;
        } else {
            mv = m[i];
            sgd_momentum(mv, gv, mu);
        }
        sgd_apply(pv, mv, lr);
        m[i] = mv;
        p[i] = pv;
        if (MODE == kAvgLerp) {
            ev.x = avg_lerp(ev.x, pv.x, c); ev.y = avg_lerp(ev.y, pv.y, c);
            ev.z = avg_lerp(ev.z, pv.z, c); ev.w = avg_lerp(ev.w, pv.w, c);
            e[i] = ev;
        } else if (MODE == kAvgCopy) {
            e[i] = pv;                                      // n == 0: a bit copy of the new parameters, e is not read
        }
    }
}

__device__ __forceinline__ void sgd_avg_body(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                             float4* __restrict__ e, int64_t n4, float lr, float mu, float wd, float gscale,
                                             int first, const AvgRule& rule, int t) {
    float c;
    const int mode = average_rule(rule, t, &c);
    if (mode == kAvgNone) sgd_avg_loop<kAvgNone>(p, g, m, e, n4, lr, mu, wd, gscale, first, c);       // e neither read nor written
    else if (mode == kAvgCopy) sgd_avg_loop<kAvgCopy>(p, g, m, e, n4, lr, mu, wd, gscale, first, c);
    else sgd_avg_loop<kAvgLerp>(p, g, m, e, n4, lr, mu, wd, gscale, first, c);
}

// sgd_kernel + the averaging rule on the fresh p, in the same trip: 28 bytes per element against 20 when step t updates with
// n >= 1 (reads p, g, m, e; writes p, m, e), 24 when n == 0, 20 when it does not update.
__global__ __launch_bounds__(256) void sgd_avg_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                                      float4* __restrict__ e, int64_t n4, float lr, float mu, float wd,
                                                      float gscale, int first, AvgRule rule, int t) {
    sgd_avg_body(p, g, m, e, n4, lr, mu, wd, gscale, first, rule, t);
}

// sgd_checked_kernel + the averaging rule with t = taken + taken_base read on the device (grad_check_finalize_kernel has counted
// this step already).  found_inf: nothing is written, e included.
__global__ __launch_bounds__(256) void sgd_checked_avg_kernel(float4* __restrict__ p, const float4* __restrict__ g,
                                                              float4* __restrict__ m, float4* __restrict__ e, int64_t n4, float lr,
                                                              float mu, float wd, const StepState* __restrict__ st, int taken_base,
                                                              AvgRule rule) {
    if (st->found_inf) return;
    sgd_avg_body(p, g, m, e, n4, lr, mu, wd, st->gmul, 0, rule, st->taken + taken_base);
}

// Exchanges two disjoint fp32 ranges bit for bit (16-byte loads and stores move bits: NaN payloads survive).
__global__ __launch_bounds__(256) void arena_swap_kernel(float4* __restrict__ a, float4* __restrict__ b, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 av = a[i], bv = b[i];
        a[i] = bv;
        b[i] = av;
    }
}

inline int64_t arena_blocks(int64_t n) {
    const int64_t blocks = (n / 4 + 255) / 256;
    return blocks > kArenaCap ? kArenaCap : blocks;
}

inline int64_t grad_check_blocks(int64_t n) {
    int64_t blocks = (n / 4 + 255) / 256;
    return blocks < 1 ? 1 : (blocks > kGradCheckCap ? kGradCheckCap : blocks);
}

}  // namespace mrfp

extern "C" int mrfp_sgd_step(float* p, const float* g, float* m, int64_t n, float lr, float momentum, float weight_decay,
                             float gscale, int first, void* stream) {
    MRFP_CHECK(p && g && m && n > 0 && n % 4 == 0, "sgd_step: bad arguments (n must be a multiple of 4)");
    MRFP_CHECK(mrfp::aligned16(p) && mrfp::aligned16(g) && mrfp::aligned16(m), "sgd_step: arenas must be 16-byte aligned");
    int64_t blocks = (n / 4 + 255) / 256;
    if (blocks > mrfp::kArenaCap) blocks = mrfp::kArenaCap;
    hipLaunchKernelGGL(mrfp::sgd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (float4*)p,
                       (const float4*)g, (float4*)m, n / 4, lr, momentum, weight_decay, gscale, first);
    MRFP_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrfp_grad_accumulate(float* acc, const float* g, int64_t n, int first, void* stream) {
    MRFP_CHECK(acc && g && n > 0 && n % 4 == 0, "grad_accumulate: bad arguments (n must be a positive multiple of 4)");
    MRFP_CHECK(mrfp::aligned16(acc) && mrfp::aligned16(g), "grad_accumulate: acc and g must be 16-byte aligned");
    int64_t blocks = (n / 4 + 255) / 256;
    if (blocks > mrfp::kArenaCap) blocks = mrfp::kArenaCap;
    hipLaunchKernelGGL(mrfp::grad_accumulate_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (float4*)acc,
                       (const float4*)g, n / 4, first);
    MRFP_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t mrfp_grad_check_nblocks(int64_t n) { return mrfp::grad_check_blocks(n); }

extern "C" int mrfp_grad_check(const float* g, int64_t n, float gscale, void* ws, void* state, int dynamic, float growth,
                               float backoff, int growth_interval, float max_norm, void* stream) {
    MRFP_CHECK(g && ws && state && n > 0 && n % 4 == 0, "grad_check: bad arguments (n must be a multiple of 4)");
    MRFP_CHECK(mrfp::aligned16(g) && mrfp::aligned16(ws) && mrfp::aligned16(state),
               "grad_check: arena, workspace and state must be 16-byte aligned");
    MRFP_CHECK(growth > 1.f, "grad_check: growth must be > 1 (got %g)", (double)growth);
    MRFP_CHECK(backoff > 0.f && backoff < 1.f, "grad_check: backoff must be in (0, 1) (got %g)", (double)backoff);
    MRFP_CHECK(growth_interval >= 1, "grad_check: growth_interval must be >= 1 (got %d)", growth_interval);
    MRFP_CHECK(max_norm > 0.f, "grad_check: max_norm must be > 0, +inf for no clipping (got %g)", (double)max_norm);
    const int64_t blocks = mrfp::grad_check_blocks(n);
    hipLaunchKernelGGL(mrfp::grad_check_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)g, n / 4,
                       gscale, (const mrfp::StepState*)state, (mrfp::GradPartial*)ws);
    MRFP_LAUNCH_CHECK();
    hipLaunchKernelGGL(mrfp::grad_check_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const mrfp::GradPartial*)ws,
                       (int)blocks, gscale, (mrfp::StepState*)state, dynamic, growth, backoff, growth_interval, max_norm);
    MRFP_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrfp_sgd_step_checked(float* p, const float* g, float* m, int64_t n, float lr, float momentum, float weight_decay,
                                     const void* state, void* stream) {
    MRFP_CHECK(p && g && m && state && n > 0 && n % 4 == 0, "sgd_step_checked: bad arguments (n must be a multiple of 4)");
    MRFP_CHECK(mrfp::aligned16(p) && mrfp::aligned16(g) && mrfp::aligned16(m) && mrfp::aligned16(state),
               "sgd_step_checked: arenas and state must be 16-byte aligned");
    int64_t blocks = (n / 4 + 255) / 256;
    if (blocks > mrfp::kArenaCap) blocks = mrfp::kArenaCap;
    hipLaunchKernelGGL(mrfp::sgd_checked_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (float4*)p,
                       (const float4*)g, (float4*)m, n / 4, lr, momentum, weight_decay, (const mrfp::StepState*)state);
    MRFP_LAUNCH_CHECK();
    return 0;
}

// The averaging arguments of the two averaged entry points, refused before any launch with the entry point's name in front.
static int avg_rule_check(const char* who, int kind, double decay, int warmup, int start, int every, mrfp::AvgRule* rule) {
    MRFP_CHECK(kind == mrfp::kAvgEma || kind == mrfp::kAvgSwa, "%s: unknown kind %d (0 = ema, 1 = swa)", who, kind);
    MRFP_CHECK(decay > 0.0 && decay < 1.0, "%s: decay must be in (0, 1) (got %g)", who, decay);
    MRFP_CHECK(start >= 1, "%s: start must be >= 1 (got %d)", who, start);
    MRFP_CHECK(every >= 1, "%s: every must be >= 1 (got %d)", who, every);
    rule->decay = decay;
    rule->kind = kind;
    rule->warmup = warmup != 0;
    rule->start = start;
    rule->every = every;
    return 0;
}

extern "C" int mrfp_sgd_step_avg(float* p, const float* g, float* m, float* e, int64_t n, float lr, float momentum,
                                 float weight_decay, float gscale, int first, int kind, double decay, int warmup, int start,
                                 int every, int t, void* stream) {
    MRFP_CHECK(p && g && m && e && n > 0 && n % 4 == 0, "sgd_step_avg: bad arguments (n must be a multiple of 4)");
    MRFP_CHECK(mrfp::aligned16(p) && mrfp::aligned16(g) && mrfp::aligned16(m) && mrfp::aligned16(e),
               "sgd_step_avg: arenas must be 16-byte aligned");
    mrfp::AvgRule rule;
    if (avg_rule_check("sgd_step_avg", kind, decay, warmup, start, every, &rule) != 0) return -1;
    hipLaunchKernelGGL(mrfp::sgd_avg_kernel, dim3((unsigned)mrfp::arena_blocks(n)), dim3(256), 0, (hipStream_t)stream, (float4*)p,
                       (const float4*)g, (float4*)m, (float4*)e, n / 4, lr, momentum, weight_decay, gscale, first, rule, t);
    MRFP_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrfp_sgd_step_checked_avg(float* p, const float* g, float* m, float* e, int64_t n, float lr, float momentum,
                                         float weight_decay, const void* state, int taken_base, int kind, double decay, int warmup,
                                         int start, int every, void* stream) {
    MRFP_CHECK(p && g && m && e && state && n > 0 && n % 4 == 0, "sgd_step_checked_avg: bad arguments (n must be a multiple of 4)");
    MRFP_CHECK(mrfp::aligned16(p) && mrfp::aligned16(g) && mrfp::aligned16(m) && mrfp::aligned16(e) && mrfp::aligned16(state),
               "sgd_step_checked_avg: arenas and state must be 16-byte aligned");
    mrfp::AvgRule rule;
    if (avg_rule_check("sgd_step_checked_avg", kind, decay, warmup, start, every, &rule) != 0) return -1;
    hipLaunchKernelGGL(mrfp::sgd_checked_avg_kernel, dim3((unsigned)mrfp::arena_blocks(n)), dim3(256), 0, (hipStream_t)stream,
                       (float4*)p, (const float4*)g, (float4*)m, (float4*)e, n / 4, lr, momentum, weight_decay,
                       (const mrfp::StepState*)state, taken_base, rule);
    MRFP_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrfp_arena_swap(float* a, float* b, int64_t n, void* stream) {
    MRFP_CHECK(a && b && n > 0 && n % 4 == 0, "arena_swap: bad arguments (n must be a positive multiple of 4)");
    MRFP_CHECK(mrfp::aligned16(a) && mrfp::aligned16(b), "arena_swap: a and b must be 16-byte aligned");
    MRFP_CHECK(a + n <= b || b + n <= a, "arena_swap: the ranges overlap");
    hipLaunchKernelGGL(mrfp::arena_swap_kernel, dim3((unsigned)mrfp::arena_blocks(n)), dim3(256), 0, (hipStream_t)stream, (float4*)a,
                       (float4*)b, n / 4);
    MRFP_LAUNCH_CHECK();
    return 0;
}
