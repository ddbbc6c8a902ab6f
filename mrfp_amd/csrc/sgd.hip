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

__global__ __launch_bounds__(256) void sgd_kernel(float4* __restrict__ p, const float4* __restrict__ g,
                                                  float4* __restrict__ m, int64_t n4, float lr, float mu, float wd,
                                                  float gscale, int first) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 pv = p[i], gv = g[i], mv;
        gv.x = gv.x * gscale + wd * pv.x; gv.y = gv.y * gscale + wd * pv.y;
        gv.z = gv.z * gscale + wd * pv.z; gv.w = gv.w * gscale + wd * pv.w;
        if (first) {
            mv = gv;
        } else {
            mv = m[i];
            mv.x = mu * mv.x + gv.x; mv.y = mu * mv.y + gv.y; mv.z = mu * mv.z + gv.z; mv.w = mu * mv.w + gv.w;
        }
        pv.x -= lr * mv.x; pv.y -= lr * mv.y; pv.z -= lr * mv.z; pv.w -= lr * mv.w;
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
        gv.x = gv.x * gscale + wd * pv.x; gv.y = gv.y * gscale + wd * pv.y;
        gv.z = gv.z * gscale + wd * pv.z; gv.w = gv.w * gscale + wd * pv.w;
        mv.x = mu * mv.x + gv.x; mv.y = mu * mv.y + gv.y; mv.z = mu * mv.z + gv.z; mv.w = mu * mv.w + gv.w;
        pv.x -= lr * mv.x; pv.y -= lr * mv.y; pv.z -= lr * mv.z; pv.w -= lr * mv.w;
        m[i] = mv;
        p[i] = pv;
    }
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
