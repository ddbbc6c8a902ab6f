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
    __shared__ float sm[2][kCeThreads / 64];
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
    nll = wave_sum(nll);
    cnt = wave_sum(cnt);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[0][w] = nll; sm[1][w] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b = 0.f;
        for (int i = 0; i < kCeThreads / 64; ++i) { a += sm[0][i]; b += sm[1][i]; }
        ws[2 * blockIdx.x] = a;
        ws[2 * blockIdx.x + 1] = b;
    }
}

__global__ void ce_finalize_kernel(const float* ws, int nblk, float* loss) {
    __shared__ double sa[256], sb[256];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) { a += ws[2 * i]; b += ws[2 * i + 1]; }
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { sa[threadIdx.x] += sa[threadIdx.x + s]; sb[threadIdx.x] += sb[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[0] = (float)(sa[0] / sb[0]);   // 0/0 -> NaN, as torch does for an all-ignored batch
        loss[1] = (float)sb[0];
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
    __shared__ float sm[2][kCeThreads / 64];
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
    nll = wave_sum(nll);
    cnt = wave_sum(cnt);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[0][w] = nll; sm[1][w] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, bsum = 0.f;
        for (int i = 0; i < kCeThreads / 64; ++i) { a += sm[0][i]; bsum += sm[1][i]; }
        ws[2 * blockIdx.x] = a;
        ws[2 * blockIdx.x + 1] = bsum;
    }
}

template <typename T, int CP>
__global__ __launch_bounds__(kCeThreads) void upsample_ce_bwd_kernel(const T* __restrict__ P, int ld, const int64_t* __restrict__ target,
                                                                     const float* __restrict__ loss, const float* __restrict__ gscale,
                                                                     T* __restrict__ dlogits, int Cd, int B, int Hi, int Wi, int H,
                                                                     int W, int C, int64_t ignore) {
    constexpr int EPC = 16 / (int)sizeof(T);
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
#pragma unroll
        for (int c0 = 0; c0 < CP; c0 += EPC) {
            if (c0 < Cd) {
                float o[EPC];
#pragma unroll
                for (int i = 0; i < EPC; ++i) o[i] = g[c0 + i];
                store_f<T, EPC>(d + c0, o);
            }
        }
    }
}

// (A backward in gather form over the LOW-resolution pixels -- the full-resolution gradient never written -- was built and
// measured in round 2: 818 us against 276 + 255 us for the two passes at 16 x 768 x 768 x 19; removed, profiles/r02_experiments.md.)

// dispatch on CP = C rounded up to 8 (8 .. kMaxClasses)
struct UpCeArgs {
    const void* P; int ld; const int64_t* target; const float* loss; const float* gscale; void* dlogits; int Cd;
    int B, Hi, Wi, H, W, C; int64_t ignore; float* ws; int nb; hipStream_t st;
};
template <typename T, int CP>
static void launch_up_ce(const UpCeArgs& a, bool bwd) {
    if (!bwd)
        hipLaunchKernelGGL((upsample_ce_fwd_kernel<T, CP>), dim3(a.nb), dim3(kCeThreads), 0, a.st, (const T*)a.P, a.ld, a.target,
                           a.B, a.Hi, a.Wi, a.H, a.W, a.C, a.ignore, a.ws);
    else
        hipLaunchKernelGGL((upsample_ce_bwd_kernel<T, CP>), dim3(a.nb), dim3(kCeThreads), 0, a.st, (const T*)a.P, a.ld, a.target,
                           a.loss, a.gscale, (T*)a.dlogits, a.Cd, a.B, a.Hi, a.Wi, a.H, a.W, a.C, a.ignore);
}
template <typename T>
static void dispatch_up_ce(const UpCeArgs& a, bool bwd) {
    switch ((a.C + 7) / 8) {
        case 1: launch_up_ce<T, 8>(a, bwd); break;
        case 2: launch_up_ce<T, 16>(a, bwd); break;
        case 3: launch_up_ce<T, 24>(a, bwd); break;
        case 4: launch_up_ce<T, 32>(a, bwd); break;
        case 5: launch_up_ce<T, 40>(a, bwd); break;
        case 6: launch_up_ce<T, 48>(a, bwd); break;
        case 7: launch_up_ce<T, 56>(a, bwd); break;
        default: launch_up_ce<T, 64>(a, bwd); break;
    }
}

}  // namespace mrfp

extern "C" {

int mrfp_upsample_ce_fwd(const void* P, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi,
                         int64_t H, int64_t W, int64_t C, int64_t ignore_index, float* ws, float* loss, void* stream) {
    MRFP_CHECK(P && target && ws && loss && B > 0 && Hi > 0 && Wi > 0 && H > 0 && W > 0 && C > 0 && C <= mrfp::kMaxClasses,
               "upsample_ce_fwd: bad arguments");
    MRFP_CHECK(mrfp::dtype_known(dtype), "upsample_ce_fwd: unknown dtype %d", dtype);
    const int epc = 16 / mrfp::dtype_bytes(dtype);
    MRFP_CHECK(ld % epc == 0 && ld >= (C + epc - 1) / epc * epc && mrfp::aligned16(P),
               "upsample_ce_fwd: the score buffer must be channel-padded to 16-byte chunks (ld=%lld)", (long long)ld);
    hipStream_t st = (hipStream_t)stream;
    const int nb = mrfp::ce_blocks(B * H * W);
    mrfp::UpCeArgs a{P, (int)ld, target, nullptr, nullptr, nullptr, 0, (int)B, (int)Hi, (int)Wi, (int)H, (int)W, (int)C,
                     ignore_index, ws, nb, st};
    return mrfp::by_dtype(dtype, "upsample_ce_fwd", [&](auto t) {
        mrfp::dispatch_up_ce<typename decltype(t)::type>(a, false);
        MRFP_LAUNCH_CHECK();
        hipLaunchKernelGGL(mrfp::ce_finalize_kernel, dim3(1), dim3(256), 0, st, ws, nb, loss);
        MRFP_LAUNCH_CHECK();
        return 0;
    });
}

int mrfp_upsample_ce_bwd(const void* P, int64_t ld, const int64_t* target, const float* loss, const float* gscale,
                         void* dlogits, int64_t Cd, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H, int64_t W,
                         int64_t C, int64_t ignore_index, void* stream) {
    MRFP_CHECK(P && target && loss && dlogits && B > 0 && Hi > 0 && Wi > 0 && H > 0 && W > 0 && C > 0 && C <= mrfp::kMaxClasses,
               "upsample_ce_bwd: bad arguments");
    MRFP_CHECK(mrfp::dtype_known(dtype), "upsample_ce_bwd: unknown dtype %d", dtype);
    const int epc = 16 / mrfp::dtype_bytes(dtype);
    MRFP_CHECK(ld % epc == 0 && Cd % epc == 0 && Cd >= C && ld >= Cd && mrfp::aligned16(P) && mrfp::aligned16(dlogits),
               "upsample_ce_bwd: channel pitches must be 16-byte multiples (ld=%lld Cd=%lld)", (long long)ld, (long long)Cd);
    hipStream_t st = (hipStream_t)stream;
    const int nb = mrfp::ce_blocks(B * H * W);
    mrfp::UpCeArgs a{P, (int)ld, target, loss, gscale, dlogits, (int)Cd, (int)B, (int)Hi, (int)Wi, (int)H, (int)W, (int)C,
                     ignore_index, nullptr, nb, st};
    return mrfp::by_dtype(dtype, "upsample_ce_bwd", [&](auto t) {
        mrfp::dispatch_up_ce<typename decltype(t)::type>(a, true);
        MRFP_LAUNCH_CHECK();
        return 0;
    });
}

}  // extern "C"

// =============================================================================================
// Class weights, label smoothing and per-image means (include/mrfp_hip.h: mrfp_ce_w_*, mrfp_upsample_ce_w_*): the criteria a
// caller hands to the reference's DeepV3Plus (network/deepv3.py:111 `criterion`, `criterion_aux`) instead of the plain one of
// main.py:822.  Same streaming as the plain kernels above, which stay as they are; what differs:
//   * the grid is (nbx, B): a workgroup works inside ONE image, stages that image's weight row (and its sum) in LDS once and reads
//     w[t] / w[c] from there -- the run-time index never touches the register-resident class vector -- and its (num, den) partial
//     belongs to one image's denominator;
//   * the finalize kernel reduces the partials in double in a fixed order (no floating-point atomics) and leaves the denominators
//     the backward divides by behind the loss.
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

// one workgroup.  MEAN / SUM: all nbx*B partials are one group; IMAGE_MEAN: the nbx partials of image b are group b.
__global__ void ce_w_finalize_kernel(const float* __restrict__ ws, int nbx, int B, int mode, float* __restrict__ loss) {
    __shared__ double sa[256], sb[256];
    const int groups = mode == MRFP_CE_IMAGE_MEAN ? B : 1;
    const int64_t per = mode == MRFP_CE_IMAGE_MEAN ? nbx : (int64_t)nbx * B;
    double total = 0.0;        // thread 0
    for (int g = 0; g < groups; ++g) {
        const float* w = ws + 2 * (int64_t)g * per;
        double a = 0.0, d = 0.0;
        for (int64_t i = threadIdx.x; i < per; i += 256) { a += w[2 * i]; d += w[2 * i + 1]; }
        sa[threadIdx.x] = a;
        sb[threadIdx.x] = d;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (threadIdx.x < s) { sa[threadIdx.x] += sa[threadIdx.x + s]; sb[threadIdx.x] += sb[threadIdx.x + s]; }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            if (mode == MRFP_CE_SUM) total = sa[0];
            else total += sa[0] / sb[0];          // 0/0 -> NaN: an all-ignored batch (MEAN, as torch) or image (IMAGE_MEAN)
            loss[1 + g] = (float)sb[0];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)total;
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

template <typename T, int CP>
__global__ __launch_bounds__(kCeThreads) void upsample_ce_w_fwd_kernel(const T* __restrict__ P, int ld, const int64_t* __restrict__ target,
                                                                       int Hi, int Wi, int H, int W, int C, int64_t ignore,
                                                                       const float* __restrict__ weight, int64_t wstride, float eps,
                                                                       float* __restrict__ ws) {
    __shared__ float sw[kMaxClasses + 1];
    const int b = blockIdx.y;
    ce_stage_weights(sw, weight, wstride, b, C);
    const float om = 1.f - eps, ec = eps / (float)C;
    const int HW = H * W;
    const int64_t* tb = target + (int64_t)b * HW;
    float num = 0.f, den = 0.f;
    for (int p = blockIdx.x * kCeThreads + threadIdx.x; p < HW; p += gridDim.x * kCeThreads) {
        const int64_t tg = tb[p];
        if (tg == ignore || tg < 0 || tg >= C) continue;
        const int oh = p / W, ow = p - oh * W;
        float z[CP];
        up_logits<T, CP>(P, ld, Hi, Wi, H, W, C, b, oh, ow, z);
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
    ce_w_store_partial(num, den, ws);
}

template <typename T, int CP>
__global__ __launch_bounds__(kCeThreads) void upsample_ce_w_bwd_kernel(const T* __restrict__ P, int ld, const int64_t* __restrict__ target,
                                                                       const float* __restrict__ loss, const float* __restrict__ gscale,
                                                                       T* __restrict__ dlogits, int Cd, int Hi, int Wi, int H, int W,
                                                                       int C, int64_t ignore, const float* __restrict__ weight,
                                                                       int64_t wstride, float eps, int mode) {
    constexpr int EPC = 16 / (int)sizeof(T);
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
#pragma unroll
        for (int c0 = 0; c0 < CP; c0 += EPC) {
            if (c0 < Cd) {
                float o[EPC];
#pragma unroll
                for (int i = 0; i < EPC; ++i) o[i] = g[c0 + i];
                store_f<T, EPC>(d + c0, o);
            }
        }
    }
}

// what the four entries refuse alike, each under its own name
static int ce_w_check(const char* who, int64_t B, int64_t C, int64_t wstride, float eps, int mode) {
    MRFP_CHECK(B <= 65535, "%s: at most 65535 images (B=%lld)", who, (long long)B);
    MRFP_CHECK(wstride == 0 || wstride == C, "%s: wstride must be 0 (one weight row) or C (one per image) (wstride=%lld C=%lld)", who,
               (long long)wstride, (long long)C);
    MRFP_CHECK(eps >= 0.f && eps < 1.f, "%s: label smoothing must be in [0, 1) (got %g)", who, (double)eps);
    MRFP_CHECK(mode == MRFP_CE_MEAN || mode == MRFP_CE_SUM || mode == MRFP_CE_IMAGE_MEAN, "%s: unknown mode %d", who, mode);
    return 0;
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
        hipLaunchKernelGGL(mrfp::ce_w_finalize_kernel, dim3(1), dim3(256), 0, st, ws, nbx, (int)B, mode, loss);
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
    MRFP_CHECK(P && target && ws && loss && B > 0 && Hi > 0 && Wi > 0 && H > 0 && W > 0 && H * W < (1LL << 30),
               "upsample_ce_w_fwd: bad arguments");
    MRFP_CHECK(C >= 1 && C <= mrfp::kMaxClasses, "upsample_ce_w_fwd: 1 <= C <= %d (C=%lld)", mrfp::kMaxClasses, (long long)C);
    MRFP_CHECK(mrfp::dtype_known(dtype), "upsample_ce_w_fwd: unknown dtype %d", dtype);
    if (int rc = mrfp::ce_w_check("upsample_ce_w_fwd", B, C, wstride, smoothing, mode)) return rc;
    const int epc = 16 / mrfp::dtype_bytes(dtype);
    MRFP_CHECK(ld % epc == 0 && ld >= (C + epc - 1) / epc * epc && mrfp::aligned16(P),
               "upsample_ce_w_fwd: the score buffer must be channel-padded to 16-byte chunks (ld=%lld)", (long long)ld);
    hipStream_t st = (hipStream_t)stream;
    const int nbx = mrfp::ce_w_blocks_x(B, H * W);
    return mrfp::by_dtype(dtype, "upsample_ce_w_fwd", [&](auto t) {
        using T = typename decltype(t)::type;
        mrfp::by_class_pad((int)C, [&](auto cp) {
            hipLaunchKernelGGL((mrfp::upsample_ce_w_fwd_kernel<T, decltype(cp)::value>), dim3(nbx, (unsigned)B), dim3(mrfp::kCeThreads), 0, st,
                               (const T*)P, (int)ld, target, (int)Hi, (int)Wi, (int)H, (int)W, (int)C, ignore_index, weight, wstride,
                               smoothing, ws);
        });
        MRFP_LAUNCH_CHECK();
        hipLaunchKernelGGL(mrfp::ce_w_finalize_kernel, dim3(1), dim3(256), 0, st, ws, nbx, (int)B, mode, loss);
        MRFP_LAUNCH_CHECK();
        return 0;
    });
}

int mrfp_upsample_ce_w_bwd(const void* P, int64_t ld, const int64_t* target, const float* loss, const float* gscale, void* dlogits,
                           int64_t Cd, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H, int64_t W, int64_t C,
                           int64_t ignore_index, const float* weight, int64_t wstride, float smoothing, int mode, void* stream) {
    MRFP_CHECK(P && target && loss && dlogits && B > 0 && Hi > 0 && Wi > 0 && H > 0 && W > 0 && H * W < (1LL << 30),
               "upsample_ce_w_bwd: bad arguments");
    MRFP_CHECK(C >= 1 && C <= mrfp::kMaxClasses, "upsample_ce_w_bwd: 1 <= C <= %d (C=%lld)", mrfp::kMaxClasses, (long long)C);
    MRFP_CHECK(mrfp::dtype_known(dtype), "upsample_ce_w_bwd: unknown dtype %d", dtype);
    if (int rc = mrfp::ce_w_check("upsample_ce_w_bwd", B, C, wstride, smoothing, mode)) return rc;
    const int epc = 16 / mrfp::dtype_bytes(dtype);
    MRFP_CHECK(ld % epc == 0 && Cd % epc == 0 && Cd >= C && ld >= Cd && mrfp::aligned16(P) && mrfp::aligned16(dlogits),
               "upsample_ce_w_bwd: channel pitches must be 16-byte multiples (ld=%lld Cd=%lld)", (long long)ld, (long long)Cd);
    hipStream_t st = (hipStream_t)stream;
    const int nbx = mrfp::ce_w_blocks_x(B, H * W);
    return mrfp::by_dtype(dtype, "upsample_ce_w_bwd", [&](auto t) {
        using T = typename decltype(t)::type;
        mrfp::by_class_pad((int)C, [&](auto cp) {
            hipLaunchKernelGGL((mrfp::upsample_ce_w_bwd_kernel<T, decltype(cp)::value>), dim3(nbx, (unsigned)B), dim3(mrfp::kCeThreads), 0, st,
                               (const T*)P, (int)ld, target, loss, gscale, (T*)dlogits, (int)Cd, (int)Hi, (int)Wi, (int)H, (int)W, (int)C,
                               ignore_index, weight, wstride, smoothing, mode);
        });
        MRFP_LAUNCH_CHECK();
        return 0;
    });
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
