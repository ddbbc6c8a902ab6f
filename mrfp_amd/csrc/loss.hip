// loss.hip -- CrossEntropyLoss(ignore_index) fwd/bwd over NHWC logits, and the eval-side
// arg-max + confusion histogram.  HBM-bound: logits are read once per pass.
//
// Replaces (reference): nn.CrossEntropyLoss(ignore_index=255) (main.py:822, deepv3.py:363) and the
// host-side np.argmax + np.bincount of the eval loop (main.py:898-909, metrics.py:122-126).
#include "loss_common.hpp"

namespace mrfp {

template <typename T>
__global__ __launch_bounds__(kCeThreads) void ce_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                            int64_t npix, int C, int64_t ignore, float* __restrict__ ws) {
    float nll = 0.f, cnt = 0.f;
    for (int64_t p = (int64_t)blockIdx.x * kCeThreads + threadIdx.x; p < npix; p += (int64_t)gridDim.x * kCeThreads) {
        const int64_t tg = target[p];
        if (tg == ignore || tg < 0 || tg >= C) continue;
        const T* l = logits + p * C;
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) m = fmaxf(m, to_f(l[c]));
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += __expf(to_f(l[c]) - m);
        nll += (m + __logf(s)) - to_f(l[tg]);
        cnt += 1.f;
    }
    ce_store_partial(nll, cnt, ws + 2 * blockIdx.x);
}

__global__ void ce_finalize_kernel(const float* ws, int nblk, float* loss) {
    double a, d;
    ce_reduce_partials(ws, nblk, a, d);
    if (threadIdx.x == 0) {
        loss[0] = (float)(a / d);   // 0/0 -> NaN, as torch does for an all-ignored batch
        loss[1] = (float)d;
    }
}

template <typename T>
__global__ __launch_bounds__(kCeThreads) void ce_bwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                            const float* __restrict__ loss, const float* __restrict__ gscale,
                                                            T* __restrict__ dlogits, int64_t npix, int C, int64_t ignore) {
    const float k = (gscale ? gscale[0] : 1.f) / loss[1];
    for (int64_t p = (int64_t)blockIdx.x * kCeThreads + threadIdx.x; p < npix; p += (int64_t)gridDim.x * kCeThreads) {
        const int64_t tg = target[p];
        const T* l = logits + p * C;
        T* d = dlogits + p * C;
        if (tg == ignore || tg < 0 || tg >= C) {
            for (int c = 0; c < C; ++c) d[c] = from_f<T>(0.f);
            continue;
        }
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) m = fmaxf(m, to_f(l[c]));
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += __expf(to_f(l[c]) - m);
        const float inv = 1.f / s;
        for (int c = 0; c < C; ++c) {
            const float pr = __expf(to_f(l[c]) - m) * inv;
            d[c] = from_f<T>((pr - (c == tg ? 1.f : 0.f)) * k);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kCeThreads) void argmax_hist_kernel(const T* __restrict__ logits,
                                                                 const int64_t* __restrict__ target, int64_t npix, int C,
                                                                 unsigned long long* __restrict__ hist,
                                                                 uint8_t* __restrict__ pred) {
    __shared__ unsigned int lh[kMaxClasses * kMaxClasses];
    for (int i = threadIdx.x; i < C * C; i += kCeThreads) lh[i] = 0;
    __syncthreads();
    for (int64_t p = (int64_t)blockIdx.x * kCeThreads + threadIdx.x; p < npix; p += (int64_t)gridDim.x * kCeThreads) {
        const T* l = logits + p * C;
        float m = to_f(l[0]);
        int am = 0;
        for (int c = 1; c < C; ++c) {
            const float v = to_f(l[c]);
            if (v > m) { m = v; am = c; }   // first maximum, as np.argmax
        }
        if (pred) pred[p] = (uint8_t)am;
        if (target) {
            const int64_t tg = target[p];
            if (tg >= 0 && tg < C) atomicAdd(&lh[(int)tg * C + am], 1u);
        }
    }
    __syncthreads();
    if (target)
        for (int i = threadIdx.x; i < C * C; i += kCeThreads)
            if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
}

static int ce_blocks(int64_t npix) {
    int64_t b = (npix + kCeThreads - 1) / kCeThreads;
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace mrfp

using namespace mrfp;

extern "C" {

int64_t mrfp_ce_nblocks(int64_t npix) { return ce_blocks(npix); }

int mrfp_ce_fwd(const void* logits, const int64_t* target, int dtype, int64_t npix, int64_t C, int64_t ignore_index,
                float* ws, float* loss, void* stream) {
    MRFP_CHECK(logits && target && ws && loss && npix > 0 && C > 0, "ce_fwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int nb = ce_blocks(npix);
    return by_dtype(dtype, "ce_fwd", [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((ce_fwd_kernel<T>), dim3(nb), dim3(kCeThreads), 0, st, (const T*)logits, target, npix, (int)C, ignore_index, ws);
        MRFP_LAUNCH_CHECK();
        hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, st, ws, nb, loss);
        MRFP_LAUNCH_CHECK();
        return 0;
    });
}

int mrfp_ce_bwd(const void* logits, const int64_t* target, const float* loss, const float* gscale, void* dlogits,
                int dtype, int64_t npix, int64_t C, int64_t ignore_index, void* stream) {
    MRFP_CHECK(logits && target && loss && dlogits && npix > 0 && C > 0, "ce_bwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int nb = ce_blocks(npix);
    return by_dtype(dtype, "ce_bwd", [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((ce_bwd_kernel<T>), dim3(nb), dim3(kCeThreads), 0, st, (const T*)logits, target, loss, gscale, (T*)dlogits, npix,
                           (int)C, ignore_index);
        MRFP_LAUNCH_CHECK();
        return 0;
    });
}

int mrfp_argmax_hist(const void* logits, const int64_t* target, int dtype, int64_t npix, int64_t C, int64_t* hist,
                     uint8_t* pred, void* stream) {
    MRFP_CHECK(logits && npix > 0 && C > 0 && C <= kMaxClasses, "argmax_hist: bad arguments (C <= %d)", kMaxClasses);
    MRFP_CHECK(!target || hist, "argmax_hist: target given without hist");
    hipStream_t st = (hipStream_t)stream;
    const int nb = ce_blocks(npix);
    return by_dtype(dtype, "argmax_hist", [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((argmax_hist_kernel<T>), dim3(nb), dim3(kCeThreads), 0, st, (const T*)logits, target, npix, (int)C,
                           (unsigned long long*)hist, pred);
        MRFP_LAUNCH_CHECK();
        return 0;
    });
}

}  // extern "C"

// =============================================================================================
// Fused  bilinear upsample (align_corners) of the low-resolution class scores  +  cross entropy.
// In training the reference only needs the scalar loss (deepv3.py:361-365): the full-resolution
// [B,19,H,W] logits are never written; every thread re-interpolates the 4 taps of its pixel from the
// (L2-resident) low-resolution scores.  Backward writes d(logits) once, channel-padded to a 16-byte
// multiple, for the gather-form bilinear backward.
// =============================================================================================
namespace mrfp {

// (up_scale / up_logits, the interpolation every fused kernel shares: loss_common.hpp)

template <typename T, int CP>
__global__ __launch_bounds__(kCeThreads) void upsample_ce_fwd_kernel(const T* __restrict__ P, int ld, const int64_t* __restrict__ target,
                                                                     int B, int Hi, int Wi, int H, int W, int C, int64_t ignore,
                                                                     float* __restrict__ ws) {
    const int64_t npix = (int64_t)B * H * W;
    float nll = 0.f, cnt = 0.f;
    for (int64_t p = (int64_t)blockIdx.x * kCeThreads + threadIdx.x; p < npix; p += (int64_t)gridDim.x * kCeThreads) {
        const int64_t tg = target[p];
        if (tg == ignore || tg < 0 || tg >= C) continue;
        const int b = (int)(p / ((int64_t)H * W)), rem = (int)(p - (int64_t)b * H * W);
        const int oh = rem / W, ow = rem - oh * W;
        float z[CP];
        up_logits<T, CP>(P, ld, Hi, Wi, H, W, C, b, oh, ow, z);
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < CP; ++c) if (c < C) m = fmaxf(m, z[c]);
        float s = 0.f, zt = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) { s += __expf(z[c] - m); zt = (c == (int)tg) ? z[c] : zt; }
        nll += (m + __logf(s)) - zt;
        cnt += 1.f;
    }
    ce_store_partial(nll, cnt, ws + 2 * blockIdx.x);
}

template <typename T, int CP>
__global__ __launch_bounds__(kCeThreads) void upsample_ce_bwd_kernel(const T* __restrict__ P, int ld, const int64_t* __restrict__ target,
                                                                     const float* __restrict__ loss, const float* __restrict__ gscale,
                                                                     T* __restrict__ dlogits, int Cd, int B, int Hi, int Wi, int H,
                                                                     int W, int C, int64_t ignore) {
    const int64_t npix = (int64_t)B * H * W;
    const float k = (gscale ? gscale[0] : 1.f) / loss[1];
    for (int64_t p = (int64_t)blockIdx.x * kCeThreads + threadIdx.x; p < npix; p += (int64_t)gridDim.x * kCeThreads) {
        const int64_t tg = target[p];
        T* d = dlogits + p * Cd;
        float g[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) g[c] = 0.f;
        const bool valid = !(tg == ignore || tg < 0 || tg >= C);
        if (valid) {
            const int b = (int)(p / ((int64_t)H * W)), rem = (int)(p - (int64_t)b * H * W);
            const int oh = rem / W, ow = rem - oh * W;
            up_logits<T, CP>(P, ld, Hi, Wi, H, W, C, b, oh, ow, g);
            float m = -INFINITY;
#pragma unroll
            for (int c = 0; c < CP; ++c) if (c < C) m = fmaxf(m, g[c]);
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < CP; ++c) { g[c] = c < C ? __expf(g[c] - m) : 0.f; s += g[c]; }
            const float inv = 1.f / s;
#pragma unroll
            for (int c = 0; c < CP; ++c) g[c] = c < C ? (g[c] * inv - (c == (int)tg ? 1.f : 0.f)) * k : 0.f;
        }
        store_class_row<T, CP>(d, Cd, g);
    }
}

// (A backward in gather form over the LOW-resolution pixels -- the full-resolution gradient never written -- was built and
// measured in round 2: 818 us against 276 + 255 us for the two passes at 16 x 768 x 768 x 19; removed, profiles/r02_experiments.md.)

}  // namespace mrfp

extern "C" {

int mrfp_upsample_ce_fwd(const void* P, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi,
                         int64_t H, int64_t W, int64_t C, int64_t ignore_index, float* ws, float* loss, void* stream) {
    MRFP_CHECK(P && target && ws && loss && B > 0 && Hi > 0 && Wi > 0 && H > 0 && W > 0 && C > 0 && C <= mrfp::kMaxClasses,
               "upsample_ce_fwd: bad arguments");
    if (int rc = mrfp::class_pitch_check("upsample_ce_fwd", P, ld, nullptr, 0, false, dtype, C)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nb = mrfp::ce_blocks(B * H * W);
    if (int rc = mrfp::by_dtype_class_pad<mrfp::kMaxClasses>(dtype, "upsample_ce_fwd", (int)C, [&](auto t, auto cp) {
            using T = typename decltype(t)::type;
            hipLaunchKernelGGL((mrfp::upsample_ce_fwd_kernel<T, decltype(cp)::value>), dim3(nb), dim3(mrfp::kCeThreads), 0, st, (const T*)P,
                               (int)ld, target, (int)B, (int)Hi, (int)Wi, (int)H, (int)W, (int)C, ignore_index, ws);
        }))
        return rc;
    hipLaunchKernelGGL(mrfp::ce_finalize_kernel, dim3(1), dim3(256), 0, st, ws, nb, loss);
    MRFP_LAUNCH_CHECK();
    return 0;
}

int mrfp_upsample_ce_bwd(const void* P, int64_t ld, const int64_t* target, const float* loss, const float* gscale,
                         void* dlogits, int64_t Cd, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H, int64_t W,
                         int64_t C, int64_t ignore_index, void* stream) {
    MRFP_CHECK(P && target && loss && dlogits && B > 0 && Hi > 0 && Wi > 0 && H > 0 && W > 0 && C > 0 && C <= mrfp::kMaxClasses,
               "upsample_ce_bwd: bad arguments");
    if (int rc = mrfp::class_pitch_check("upsample_ce_bwd", P, ld, dlogits, Cd, false, dtype, C)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nb = mrfp::ce_blocks(B * H * W);
    return mrfp::by_dtype_class_pad<mrfp::kMaxClasses>(dtype, "upsample_ce_bwd", (int)C, [&](auto t, auto cp) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((mrfp::upsample_ce_bwd_kernel<T, decltype(cp)::value>), dim3(nb), dim3(mrfp::kCeThreads), 0, st, (const T*)P,
                           (int)ld, target, loss, gscale, (T*)dlogits, (int)Cd, (int)B, (int)Hi, (int)Wi, (int)H, (int)W, (int)C,
                           ignore_index);
    });
}

}  // extern "C"

// =============================================================================================
// Class weights, label smoothing and per-image means (include/mrfp_hip.h: mrfp_ce_w_*, mrfp_upsample_ce_w_*): the criteria a
// caller hands to the reference's DeepV3Plus (network/deepv3.py:111 `criterion`, `criterion_aux`) instead of the plain one of
// main.py:822.  The plain kernels above keep their flat grid: they are the default step's path.  Here
//   * the fused forward is the pixel-loop skeleton of loss_common.hpp (pixel_loss_fwd_kernel over BilinearRows) with the
//     WeightedCe criterion below: grid (nbx, B), the image's weight row and its sum staged in LDS; the fused backward
//     (upsample_ce_w_bwd_kernel) is that skeleton written out, for the registers it would otherwise lose;
//   * the dense form (ce_w_fwd/bwd_kernel) walks a run-time C up to kCeDenseMaxC with the weight row in dynamic LDS: it has no
//     register class vector, so it stays outside the skeleton and shares its grid, staging, partial and finalize;
//   * ce_w_finalize_kernel (loss_common.hpp) leaves the denominators the backward divides by behind the loss.
// =============================================================================================
namespace mrfp {

constexpr int kCeDenseMaxC = 8192;        // dense form: the weight row lives in dynamic LDS, (C + 1) floats

// sw[0..C) = weight row of image b (ones for a null pointer), sw[C] = its sum
__device__ __forceinline__ void ce_stage_weights(float* sw, const float* __restrict__ weight, int64_t wstride, int b, int C) {
    const float* w = weight ? weight + (int64_t)b * wstride : nullptr;
    for (int c = threadIdx.x; c < C; c += kCeThreads) sw[c] = w ? w[c] : 1.f;
    __syncthreads();
    if (threadIdx.x < 64) {
        float s = 0.f;
        for (int c = threadIdx.x; c < C; c += 64) s += sw[c];
        s = wave_sum(s);
        if (threadIdx.x == 0) sw[C] = s;
    }
    __syncthreads();
}

// the factor of one image's gradients: gscale / den (MEAN), gscale (SUM), gscale / den_b (IMAGE_MEAN)
__device__ __forceinline__ float ce_w_bwd_factor(const float* __restrict__ loss, const float* __restrict__ gscale, int mode, int b) {
    const float g = gscale ? gscale[0] : 1.f;
    if (mode == MRFP_CE_SUM) return g;
    return g / loss[mode == MRFP_CE_IMAGE_MEAN ? 1 + b : 1];
}

template <typename T>
__global__ __launch_bounds__(kCeThreads) void ce_w_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                              int64_t HW, int C, int64_t ignore, const float* __restrict__ weight,
                                                              int64_t wstride, float eps, float* __restrict__ ws) {
    extern __shared__ float sw[];
    const int b = blockIdx.y;
    ce_stage_weights(sw, weight, wstride, b, C);
    const float om = 1.f - eps, ec = eps / (float)C;
    const T* lb = logits + (int64_t)b * HW * C;
    const int64_t* tb = target + (int64_t)b * HW;
    float num = 0.f, den = 0.f;
    for (int64_t p = (int64_t)blockIdx.x * kCeThreads + threadIdx.x; p < HW; p += (int64_t)gridDim.x * kCeThreads) {
        const int64_t tg = tb[p];
        if (tg == ignore || tg < 0 || tg >= C) continue;
        const T* l = lb + p * C;
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) m = fmaxf(m, to_f(l[c]));
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += __expf(to_f(l[c]) - m);
        const float lse = m + __logf(s), wt = sw[(int)tg];
        float v = om * wt * (lse - to_f(l[tg]));
        if (eps > 0.f) {
            float a = 0.f;
            for (int c = 0; c < C; ++c) a += sw[c] * (lse - to_f(l[c]));
            v += ec * a;
        }
        num += v;
        den += wt;
    }
    ce_w_store_partial(num, den, ws);
}

template <typename T>
__global__ __launch_bounds__(kCeThreads) void ce_w_bwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                              const float* __restrict__ loss, const float* __restrict__ gscale,
                                                              T* __restrict__ dlogits, int64_t HW, int C, int64_t ignore,
                                                              const float* __restrict__ weight, int64_t wstride, float eps, int mode) {
    extern __shared__ float sw[];
    const int b = blockIdx.y;
    ce_stage_weights(sw, weight, wstride, b, C);
    const float om = 1.f - eps, ec = eps / (float)C, wsum = sw[C];
    const float k = ce_w_bwd_factor(loss, gscale, mode, b);
    const T* lb = logits + (int64_t)b * HW * C;
    T* db = dlogits + (int64_t)b * HW * C;
    const int64_t* tb = target + (int64_t)b * HW;
    for (int64_t p = (int64_t)blockIdx.x * kCeThreads + threadIdx.x; p < HW; p += (int64_t)gridDim.x * kCeThreads) {
        const int64_t tg = tb[p];
        const T* l = lb + p * C;
        T* d = db + p * C;
        if (tg == ignore || tg < 0 || tg >= C) {
            for (int c = 0; c < C; ++c) d[c] = from_f<T>(0.f);
            continue;
        }
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) m = fmaxf(m, to_f(l[c]));
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += __expf(to_f(l[c]) - m);
        const float inv = 1.f / s, wt = om * sw[(int)tg], A = wt + ec * wsum;
        for (int c = 0; c < C; ++c) {
            const float pr = __expf(to_f(l[c]) - m) * inv;
            d[c] = from_f<T>((pr * A - (c == tg ? wt : 0.f) - ec * sw[c]) * k);
        }
    }
}

// The criterion of the skeleton's forward: cross entropy of an int64 label (ignore, or outside 0..C-1: the pixel does not count)
// with class weights and label smoothing eps.  sw: ce_stage_weights.
struct WeightedCe {
    static constexpr int kLdsFloats = kMaxClasses + 1, kMaxClassPad = kMaxClasses;
    static constexpr double kDenBias = 0.0;
    const int64_t* target; int64_t ignore; const float* weight; int64_t wstride; float eps; int mode;

    __device__ __forceinline__ void stage(float* sw, int b, int C) const { ce_stage_weights(sw, weight, wstride, b, C); }
    __device__ __forceinline__ int64_t label(int64_t tg, int) const { return tg; }
    __device__ __forceinline__ bool valid(int64_t tg, int C) const { return !(tg == ignore || tg < 0 || tg >= C); }

    template <int CP>
    __device__ __forceinline__ void add_loss(const float (&z)[CP], int C, int64_t tg, const float* sw, float& num, float& den) const {
        const float om = 1.f - eps, ec = eps / (float)C;
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < CP; ++c) if (c < C) m = fmaxf(m, z[c]);
        float s = 0.f, zt = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) { s += __expf(z[c] - m); zt = (c == (int)tg) ? z[c] : zt; }
        const float lse = m + __logf(s), wt = sw[(int)tg];
        float v = om * wt * (lse - zt);
        if (eps > 0.f) {
            float a = 0.f;
#pragma unroll
            for (int c = 0; c < CP; ++c) if (c < C) a += sw[c] * (lse - z[c]);
            v += ec * a;
        }
        num += v;
        den += wt;
    }
};

// The fused backward keeps its own kernel, the skeleton's backward with this criterion's gradient written out: with the gradient
// in a member function the compiler holds every `c < C` mask in scalar registers across the trip and three families of
// instances lose an occupancy step (bf16 / fp16 CP 16: 95 -> 98 VGPRs, 5 -> 4 waves; CP 48: 253 -> 256 + 1 AGPR, 2 -> 1; fp32 CP 8:
// 72 -> 78, 7 -> 6; profiles/loss_skeleton.md).
template <typename T, int CP>
__global__ __launch_bounds__(kCeThreads) void upsample_ce_w_bwd_kernel(const T* __restrict__ P, int ld, const int64_t* __restrict__ target,
                                                                       const float* __restrict__ loss, const float* __restrict__ gscale,
                                                                       T* __restrict__ dlogits, int Cd, int Hi, int Wi, int H, int W,
                                                                       int C, int64_t ignore, const float* __restrict__ weight,
                                                                       int64_t wstride, float eps, int mode) {
    __shared__ float sw[kMaxClasses + 1];
    const int b = blockIdx.y;
    ce_stage_weights(sw, weight, wstride, b, C);
    const float om = 1.f - eps, ec = eps / (float)C, wsum = sw[C];
    const float k = ce_w_bwd_factor(loss, gscale, mode, b);
    const int HW = H * W;
    const int64_t* tb = target + (int64_t)b * HW;
    T* db = dlogits + (int64_t)b * HW * Cd;
    for (int p = blockIdx.x * kCeThreads + threadIdx.x; p < HW; p += gridDim.x * kCeThreads) {
        const int64_t tg = tb[p];
        T* d = db + (int64_t)p * Cd;
        float g[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) g[c] = 0.f;
        if (!(tg == ignore || tg < 0 || tg >= C)) {
            const int oh = p / W, ow = p - oh * W;
            up_logits<T, CP>(P, ld, Hi, Wi, H, W, C, b, oh, ow, g);
            float m = -INFINITY;
#pragma unroll
            for (int c = 0; c < CP; ++c) if (c < C) m = fmaxf(m, g[c]);
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < CP; ++c) { g[c] = c < C ? __expf(g[c] - m) : 0.f; s += g[c]; }
            const float wt = om * sw[(int)tg], A = (wt + ec * wsum) / s;
            if (eps > 0.f) {
#pragma unroll
                for (int c = 0; c < CP; ++c) g[c] = c < C ? (g[c] * A - (c == (int)tg ? wt : 0.f) - ec * sw[c]) * k : 0.f;
            } else {
#pragma unroll
                for (int c = 0; c < CP; ++c) g[c] = c < C ? (g[c] * A - (c == (int)tg ? wt : 0.f)) * k : 0.f;
            }
        }
        store_class_row<T, CP>(d, Cd, g);
    }
}

// what the four entries refuse alike, each under its own name
static int ce_w_check(const char* who, int64_t B, int64_t C, int64_t wstride, float eps, int mode) {
    MRFP_CHECK(B <= 65535, "%s: at most 65535 images (B=%lld)", who, (long long)B);
    if (int rc = wstride_check(who, wstride, C)) return rc;
    MRFP_CHECK(eps >= 0.f && eps < 1.f, "%s: label smoothing must be in [0, 1) (got %g)", who, (double)eps);
    MRFP_CHECK(mode == MRFP_CE_MEAN || mode == MRFP_CE_SUM || mode == MRFP_CE_IMAGE_MEAN, "%s: unknown mode %d", who, mode);
    return 0;
}

// ---- focal loss (include/mrfp_hip.h: mrfp_focal_*, mrfp_upsample_focal_*) -----------------------------------------------------
// The weighted cross entropy of a pixel times (1 - p_t)^gamma: a criterion of the skeleton, forward and backward, over both
// sources, with WeightedCe's labels, staging, partials, finalize and modes.  q = 1 - p_t is sum_{c != t} e_c / sum_c e_c, a sum and
// never a difference: a pixel whose p_t rounds to 1 has q == 0 exactly, and its loss and gradient are zeros for every gamma.
// gamma == 0 takes the branch in which the modulation is the constant 1: the forward is then WeightedCe's arithmetic, term for term.
struct Focal {
    static constexpr int kLdsFloats = kMaxClasses + 1, kMaxClassPad = kMaxClasses;
    static constexpr double kDenBias = 0.0;
    const int64_t* target; int64_t ignore; const float* weight; int64_t wstride; float gamma; int mode;

    __device__ __forceinline__ void stage(float* sw, int b, int C) const { ce_stage_weights(sw, weight, wstride, b, C); }
    __device__ __forceinline__ int64_t label(int64_t tg, int) const { return tg; }
    __device__ __forceinline__ bool valid(int64_t tg, int C) const { return !(tg == ignore || tg < 0 || tg >= C); }
    __device__ __forceinline__ float bwd_factor(const float* __restrict__ loss, const float* __restrict__ gscale, int b) const {
        return ce_w_bwd_factor(loss, gscale, mode, b);
    }
    // q^gamma for q in [0, 1], gamma > 0: 0 at q == 0
    __device__ __forceinline__ float qpow(float q) const { return q > 0.f ? __expf(gamma * __logf(q)) : 0.f; }

    template <int CP>
    __device__ __forceinline__ void add_loss(const float (&z)[CP], int C, int64_t tg, const float* sw, float& num, float& den) const {
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < CP; ++c) if (c < C) m = fmaxf(m, z[c]);
        float s = 0.f, so = 0.f, zt = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) {
                const float e = __expf(z[c] - m);
                s += e;
                so += (c == (int)tg) ? 0.f : e;
                zt = (c == (int)tg) ? z[c] : zt;
            }
        const float lse = m + __logf(s), wt = sw[(int)tg];
        float v = wt * (lse - zt);
        if (gamma != 0.f) v *= qpow(so / s);
        num += v;
        den += wt;
    }

    // g: the class vector in, its gradient out.  F = q^gamma + gamma p_t q^(gamma-1) (-log p_t), q^(gamma-1) as q^gamma / q; at
    // q == 0 the factor is 0 (its limit for every gamma > 0, and every p_j - [j == t] is 0 there as well).
    template <int CP>
    __device__ __forceinline__ void grad(float (&g)[CP], int C, int64_t tg, const float* sw, float k) const {
        float m = -INFINITY, zt = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) { m = fmaxf(m, g[c]); zt = (c == (int)tg) ? g[c] : zt; }
        float s = 0.f, so = 0.f, et = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            g[c] = c < C ? __expf(g[c] - m) : 0.f;
            s += g[c];
            so += (c == (int)tg) ? 0.f : g[c];
            et = (c == (int)tg) ? g[c] : et;
        }
        float F = 1.f;
        if (gamma != 0.f) {
            const float q = so / s, qg = qpow(q), nlp = __logf(s) - (zt - m);       // -log p_t, the difference first
            F = q > 0.f ? qg + gamma * (et / s) * (qg / q) * nlp : 0.f;
        }
        const float wt = sw[(int)tg] * F, A = wt / s;
#pragma unroll
        for (int c = 0; c < CP; ++c) g[c] = c < C ? (g[c] * A - (c == (int)tg ? wt : 0.f)) * k : 0.f;
    }
};

static int focal_check(const char* who, int64_t B, int64_t C, int64_t wstride, float gamma, int mode) {
    MRFP_CHECK(C >= 1 && C <= kMaxClasses, "%s: 1 <= C <= %d (C=%lld)", who, kMaxClasses, (long long)C);
    MRFP_CHECK(gamma >= 0.f && gamma <= 3.0e38f, "%s: gamma must be a finite number >= 0 (got %g)", who, (double)gamma);
    return ce_w_check(who, B, C, wstride, 0.f, mode);
}

// ---- per-image class weights from the label map ------------------------------------------------------------------------------
constexpr int kHistMaxClasses = 1024;

__global__ void label_counts_clear_kernel(unsigned long long* __restrict__ counts, int n) {
    const int i = blockIdx.x * kCeThreads + threadIdx.x;
    if (i < n) counts[i] = 0ull;
}

// integer histogram of one image's labels in [0,C): LDS atomics, then one integer add per class per workgroup (as argmax_hist_kernel)
__global__ __launch_bounds__(kCeThreads) void label_counts_kernel(const int64_t* __restrict__ target, int64_t HW, int C, int pooled,
                                                                  unsigned long long* __restrict__ counts) {
    __shared__ unsigned int lh[kHistMaxClasses];
    for (int i = threadIdx.x; i < C; i += kCeThreads) lh[i] = 0;
    __syncthreads();
    const int64_t* tb = target + (int64_t)blockIdx.y * HW;
    for (int64_t p = (int64_t)blockIdx.x * kCeThreads + threadIdx.x; p < HW; p += (int64_t)gridDim.x * kCeThreads) {
        const int64_t tg = tb[p];
        if (tg >= 0 && tg < C) atomicAdd(&lh[(int)tg], 1u);
    }
    __syncthreads();
    unsigned long long* row = counts + (pooled ? 0 : (int64_t)blockIdx.y * C);
    for (int i = threadIdx.x; i < C; i += kCeThreads)
        if (lh[i]) atomicAdd(&row[i], (unsigned long long)lh[i]);
}

// f_c and w_c in double, one rounding to float (the translation unit is built with -ffp-contract=off: no fused multiply-add)
__global__ void label_weights_kernel(const unsigned long long* __restrict__ counts, int rows, int C, double ub, int norm,
                                     float* __restrict__ out) {
    const int i = blockIdx.x * kCeThreads + threadIdx.x;
    if (i >= rows * C) return;
    const unsigned long long* row = counts + (int64_t)(i / C) * C;
    unsigned long long total = 0ull;
    for (int c = 0; c < C; ++c) total += row[c];
    const unsigned long long n = row[i % C];
    double w = 1.0;
    if (n > 0ull) {
        const double f = (double)n / (double)total;
        w = norm ? 1.0 + ub / f : 1.0 + ub * (1.0 - f);
    }
    out[i] = (float)w;
}

}  // namespace mrfp

extern "C" {

int64_t mrfp_ce_w_nblocks(int64_t B, int64_t HW) { return (int64_t)mrfp::ce_w_blocks_x(B, HW) * (B > 0 ? B : 1); }

int64_t mrfp_ce_w_loss_floats(int64_t B, int mode) { return 1 + (mode == MRFP_CE_IMAGE_MEAN ? B : 1); }

int mrfp_ce_w_fwd(const void* logits, const int64_t* target, int dtype, int64_t B, int64_t HW, int64_t C, int64_t ignore_index,
                  const float* weight, int64_t wstride, float smoothing, int mode, float* ws, float* loss, void* stream) {
    MRFP_CHECK(logits && target && ws && loss && B > 0 && HW > 0 && C > 0 && C <= mrfp::kCeDenseMaxC,
               "ce_w_fwd: bad arguments (C <= %d)", mrfp::kCeDenseMaxC);
    if (int rc = mrfp::ce_w_check("ce_w_fwd", B, C, wstride, smoothing, mode)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nbx = mrfp::ce_w_blocks_x(B, HW);
    const size_t lds = (size_t)(C + 1) * sizeof(float);
    return mrfp::by_dtype(dtype, "ce_w_fwd", [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((mrfp::ce_w_fwd_kernel<T>), dim3(nbx, (unsigned)B), dim3(mrfp::kCeThreads), lds, st, (const T*)logits, target, HW,
                           (int)C, ignore_index, weight, wstride, smoothing, ws);
        MRFP_LAUNCH_CHECK();
        hipLaunchKernelGGL(mrfp::ce_w_finalize_kernel<mrfp::WeightedCe>, dim3(1), dim3(256), 0, st, ws, nbx, (int)B, mode, loss);
        MRFP_LAUNCH_CHECK();
        return 0;
    });
}

int mrfp_ce_w_bwd(const void* logits, const int64_t* target, const float* loss, const float* gscale, void* dlogits, int dtype,
                  int64_t B, int64_t HW, int64_t C, int64_t ignore_index, const float* weight, int64_t wstride, float smoothing,
                  int mode, void* stream) {
    MRFP_CHECK(logits && target && loss && dlogits && B > 0 && HW > 0 && C > 0 && C <= mrfp::kCeDenseMaxC,
               "ce_w_bwd: bad arguments (C <= %d)", mrfp::kCeDenseMaxC);
    if (int rc = mrfp::ce_w_check("ce_w_bwd", B, C, wstride, smoothing, mode)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nbx = mrfp::ce_w_blocks_x(B, HW);
    const size_t lds = (size_t)(C + 1) * sizeof(float);
    return mrfp::by_dtype(dtype, "ce_w_bwd", [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((mrfp::ce_w_bwd_kernel<T>), dim3(nbx, (unsigned)B), dim3(mrfp::kCeThreads), lds, st, (const T*)logits, target, loss,
                           gscale, (T*)dlogits, HW, (int)C, ignore_index, weight, wstride, smoothing, mode);
        MRFP_LAUNCH_CHECK();
        return 0;
    });
}

int mrfp_upsample_ce_w_fwd(const void* P, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H,
                           int64_t W, int64_t C, int64_t ignore_index, const float* weight, int64_t wstride, float smoothing, int mode,
                           float* ws, float* loss, void* stream) {
    const char* who = "upsample_ce_w_fwd";
    MRFP_CHECK(P && target && ws && loss && B > 0, "%s: bad arguments", who);
    MRFP_CHECK(C >= 1 && C <= mrfp::kMaxClasses, "%s: 1 <= C <= %d (C=%lld)", who, mrfp::kMaxClasses, (long long)C);
    if (int rc = mrfp::ce_w_check(who, B, C, wstride, smoothing, mode)) return rc;
    mrfp::BilinearRows src;
    if (int rc = mrfp::bilinear_rows(who, P, ld, nullptr, 0, false, dtype, Hi, Wi, H, W, C, src)) return rc;
    return mrfp::launch_pixel_loss_fwd(who, dtype, B, src, mrfp::WeightedCe{target, ignore_index, weight, wstride, smoothing, mode}, ws, loss,
                                       (hipStream_t)stream);
}

int mrfp_upsample_ce_w_bwd(const void* P, int64_t ld, const int64_t* target, const float* loss, const float* gscale, void* dlogits,
                           int64_t Cd, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H, int64_t W, int64_t C,
                           int64_t ignore_index, const float* weight, int64_t wstride, float smoothing, int mode, void* stream) {
    const char* who = "upsample_ce_w_bwd";
    MRFP_CHECK(P && target && loss && dlogits && B > 0, "%s: bad arguments", who);
    MRFP_CHECK(C >= 1 && C <= mrfp::kMaxClasses, "%s: 1 <= C <= %d (C=%lld)", who, mrfp::kMaxClasses, (long long)C);
    if (int rc = mrfp::ce_w_check(who, B, C, wstride, smoothing, mode)) return rc;
    mrfp::BilinearRows src;
    if (int rc = mrfp::bilinear_rows(who, P, ld, dlogits, Cd, false, dtype, Hi, Wi, H, W, C, src)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nbx = mrfp::ce_w_blocks_x(B, src.HW);
    return mrfp::by_dtype_class_pad<mrfp::kMaxClasses>(dtype, who, src.C, [&](auto t, auto cp) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((mrfp::upsample_ce_w_bwd_kernel<T, decltype(cp)::value>), dim3(nbx, (unsigned)B), dim3(mrfp::kCeThreads), 0, st,
                           (const T*)P, src.ld, target, loss, gscale, (T*)dlogits, src.Cd, src.Hi, src.Wi, src.H, src.W, src.C, ignore_index,
                           weight, wstride, smoothing, mode);
    });
}

int mrfp_focal_fwd(const void* logits, const int64_t* target, int dtype, int64_t B, int64_t HW, int64_t C, int64_t ignore_index,
                   const float* weight, int64_t wstride, float gamma, int mode, float* ws, float* loss, void* stream) {
    const char* who = "focal_fwd";
    MRFP_CHECK(logits && target && ws && loss && B > 0 && HW > 0, "%s: bad arguments", who);
    if (int rc = mrfp::focal_check(who, B, C, wstride, gamma, mode)) return rc;
    return mrfp::launch_pixel_loss_fwd(who, dtype, B, mrfp::DenseRows{logits, nullptr, HW, (int)C},
                                       mrfp::Focal{target, ignore_index, weight, wstride, gamma, mode}, ws, loss, (hipStream_t)stream);
}

int mrfp_focal_bwd(const void* logits, const int64_t* target, const float* loss, const float* gscale, void* dlogits, int dtype,
                   int64_t B, int64_t HW, int64_t C, int64_t ignore_index, const float* weight, int64_t wstride, float gamma, int mode,
                   void* stream) {
    const char* who = "focal_bwd";
    MRFP_CHECK(logits && target && loss && dlogits && B > 0 && HW > 0, "%s: bad arguments", who);
    if (int rc = mrfp::focal_check(who, B, C, wstride, gamma, mode)) return rc;
    return mrfp::launch_pixel_loss_bwd(who, dtype, B, mrfp::DenseRows{logits, dlogits, HW, (int)C},
                                       mrfp::Focal{target, ignore_index, weight, wstride, gamma, mode}, loss, gscale, (hipStream_t)stream);
}

int mrfp_upsample_focal_fwd(const void* P, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H,
                            int64_t W, int64_t C, int64_t ignore_index, const float* weight, int64_t wstride, float gamma, int mode,
                            float* ws, float* loss, void* stream) {
    const char* who = "upsample_focal_fwd";
    MRFP_CHECK(P && target && ws && loss && B > 0, "%s: bad arguments", who);
    if (int rc = mrfp::focal_check(who, B, C, wstride, gamma, mode)) return rc;
    mrfp::BilinearRows src;
    if (int rc = mrfp::bilinear_rows(who, P, ld, nullptr, 0, false, dtype, Hi, Wi, H, W, C, src)) return rc;
    return mrfp::launch_pixel_loss_fwd(who, dtype, B, src, mrfp::Focal{target, ignore_index, weight, wstride, gamma, mode}, ws, loss,
                                       (hipStream_t)stream);
}

int mrfp_upsample_focal_bwd(const void* P, int64_t ld, const int64_t* target, const float* loss, const float* gscale, void* dlogits,
                            int64_t Cd, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H, int64_t W, int64_t C,
                            int64_t ignore_index, const float* weight, int64_t wstride, float gamma, int mode, void* stream) {
    const char* who = "upsample_focal_bwd";
    MRFP_CHECK(P && target && loss && dlogits && B > 0, "%s: bad arguments", who);
    if (int rc = mrfp::focal_check(who, B, C, wstride, gamma, mode)) return rc;
    mrfp::BilinearRows src;
    if (int rc = mrfp::bilinear_rows(who, P, ld, dlogits, Cd, false, dtype, Hi, Wi, H, W, C, src)) return rc;
    return mrfp::launch_pixel_loss_bwd(who, dtype, B, src, mrfp::Focal{target, ignore_index, weight, wstride, gamma, mode}, loss, gscale,
                                       (hipStream_t)stream);
}

int mrfp_label_class_weights(const int64_t* target, int64_t B, int64_t HW, int64_t C, double upper_bound, int norm, int batch,
                             int64_t* counts_ws, float* weight_out, void* stream) {
    MRFP_CHECK(target && counts_ws && weight_out && B > 0 && B <= 65535 && HW > 0 && C > 0 && C <= mrfp::kHistMaxClasses,
               "label_class_weights: bad arguments (B <= 65535, C <= %d)", mrfp::kHistMaxClasses);
    hipStream_t st = (hipStream_t)stream;
    const int rows = batch ? 1 : (int)B, n = rows * (int)C;
    unsigned long long* counts = (unsigned long long*)counts_ws;
    hipLaunchKernelGGL(mrfp::label_counts_clear_kernel, dim3((n + mrfp::kCeThreads - 1) / mrfp::kCeThreads), dim3(mrfp::kCeThreads), 0, st,
                       counts, n);
    MRFP_LAUNCH_CHECK();
    hipLaunchKernelGGL(mrfp::label_counts_kernel, dim3(mrfp::ce_w_blocks_x(B, HW), (unsigned)B), dim3(mrfp::kCeThreads), 0, st, target, HW,
                       (int)C, batch ? 1 : 0, counts);
    MRFP_LAUNCH_CHECK();
    hipLaunchKernelGGL(mrfp::label_weights_kernel, dim3((n + mrfp::kCeThreads - 1) / mrfp::kCeThreads), dim3(mrfp::kCeThreads), 0, st,
                       counts, rows, (int)C, upper_bound, norm ? 1 : 0, weight_out);
    MRFP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
