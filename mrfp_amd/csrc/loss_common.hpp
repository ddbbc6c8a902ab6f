// loss_common.hpp -- what the loss translation units share (loss.hip: the cross-entropy family; relax.hip: relaxed targets and the
// soft-NLL criterion; predict.hip: the validation loss): the workgroup size, the per-image grid cap, the in-kernel align-corners
// bilinear interpolation of the low-resolution class scores, the per-workgroup (num, den) partial and its reduction, the
// compile-time class-count dispatch, and the pixel-loop skeleton: one forward and one backward kernel over a SOURCE of the
// per-pixel class vector and a CRITERION applied to it.  A new criterion is one struct beside WeightedCe (loss.hip) and SoftNll
// (relax.hip), and two entries that fill it in.
#pragma once
#include "common.hpp"

namespace mrfp {

constexpr int kCeThreads = 256;
constexpr int kMaxClasses = 64;

__device__ __forceinline__ float up_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// CP = class count rounded up to a multiple of 8 (compile time): every loop over classes is fully unrolled with a
// `c < C` predicate, so the per-pixel class vector lives in registers (a run-time bound puts it in scratch memory:
// measured 469 / 1060 us per call at 16x768x768x19 before, see profiles/).
template <typename T, int CP>
__device__ __forceinline__ void up_logits(const T* __restrict__ P, int ld, int Hi, int Wi, int H, int W, int C, int b,
                                          int oh, int ow, float (&z)[CP]) {
    const float sh = up_scale(Hi, H), sw = up_scale(Wi, W);
    const float fh = sh * (float)oh, fw = sw * (float)ow;
    const int h0 = (int)fh, w0 = (int)fw;
    const int h1 = h0 + (h0 < Hi - 1 ? 1 : 0), w1 = w0 + (w0 < Wi - 1 ? 1 : 0);
    const float lh1 = fh - (float)h0, lh0 = 1.f - lh1, lw1 = fw - (float)w0, lw0 = 1.f - lw1;
    const T* p00 = P + (((size_t)b * Hi + h0) * Wi + w0) * ld;
    const T* p01 = P + (((size_t)b * Hi + h0) * Wi + w1) * ld;
    const T* p10 = P + (((size_t)b * Hi + h1) * Wi + w0) * ld;
    const T* p11 = P + (((size_t)b * Hi + h1) * Wi + w1) * ld;
    constexpr int EPC = 16 / (int)sizeof(T);
#pragma unroll
    for (int c0 = 0; c0 < CP; c0 += EPC) {
        float a[EPC], bb[EPC], c[EPC], d[EPC];
#pragma unroll
        for (int i = 0; i < EPC; ++i) { a[i] = 0.f; bb[i] = 0.f; c[i] = 0.f; d[i] = 0.f; }
        if (c0 < C) {        // chunks past the class count are never read (the pitch may be shorter than CP)
            load_f<T, EPC>(p00 + c0, a);
            load_f<T, EPC>(p01 + c0, bb);
            load_f<T, EPC>(p10 + c0, c);
            load_f<T, EPC>(p11 + c0, d);
        }
#pragma unroll
        for (int i = 0; i < EPC; ++i) z[c0 + i] = lh0 * (lw0 * a[i] + lw1 * bb[i]) + lh1 * (lw0 * c[i] + lw1 * d[i]);
    }
}

// the gradient row of one pixel, channel-padded to Cd (a 16-byte multiple), in 16-byte chunks
template <typename T, int CP>
__device__ __forceinline__ void store_class_row(T* __restrict__ d, int Cd, const float (&g)[CP]) {
    constexpr int EPC = 16 / (int)sizeof(T);
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

// workgroups per image of a (nbx, B) grid in which a workgroup stays inside one image: at most 2048 over the launch
static int ce_w_blocks_x(int64_t B, int64_t HW) {
    int64_t n = (HW + kCeThreads - 1) / kCeThreads, cap = 2048 / (B > 0 ? B : 1);
    if (cap < 1) cap = 1;
    if (n > cap) n = cap;
    if (n < 1) n = 1;
    return (int)n;
}

// the workgroup's (num, den) into slot[0], slot[1]
__device__ __forceinline__ void ce_store_partial(float num, float den, float* __restrict__ slot) {
    __shared__ float sm[2][kCeThreads / 64];
    num = wave_sum(num);
    den = wave_sum(den);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[0][w] = num; sm[1][w] = den; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, d = 0.f;
        for (int i = 0; i < kCeThreads / 64; ++i) { a += sm[0][i]; d += sm[1][i]; }
        slot[0] = a;
        slot[1] = d;
    }
}
// on a (nbx, B) grid: the partials of image b are consecutive.  (The flat kernels of loss.hip pass their own slot, ws + 2 *
// blockIdx.x: this form's two extra scalars cost upsample_ce_fwd_kernel<float, 56> its second wave, 256 VGPRs + 1 AGPR.)
__device__ __forceinline__ void ce_w_store_partial(float num, float den, float* __restrict__ ws) {
    ce_store_partial(num, den, ws + 2 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x));
}

// One workgroup of 256 threads: the sums of n (num, den) partials in double in a fixed order (no floating-point atomics), on every
// thread.  Ends behind a barrier, so a kernel may call it once per group.
__device__ __forceinline__ void ce_reduce_partials(const float* __restrict__ w, int64_t n, double& num, double& den) {
    __shared__ double sa[256], sb[256];
    double a = 0.0, d = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) { a += w[2 * i]; d += w[2 * i + 1]; }
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = d;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { sa[threadIdx.x] += sa[threadIdx.x + s]; sb[threadIdx.x] += sb[threadIdx.x + s]; }
        __syncthreads();
    }
    num = sa[0];
    den = sb[0];
    __syncthreads();
}

// The finalize of a (nbx, B) grid.  MEAN / SUM: all nbx*B partials are one group; IMAGE_MEAN: the nbx partials of image b are group b.
// loss[0] = the loss, loss[1 + g] = the denominator of group g + bias, which the backward divides by.  bias: 0 for cross entropy,
// 1 for soft-NLL (the published denominator valid_b + 1: an all-ignored image adds 0 / 1); it is the criterion's kDenBias, and a
// translation unit holds the instance of its criterion only.
template <typename Criterion>
__global__ void ce_w_finalize_kernel(const float* __restrict__ ws, int nbx, int B, int mode, float* __restrict__ loss) {
    constexpr double bias = Criterion::kDenBias;
    const int groups = mode == MRFP_CE_IMAGE_MEAN ? B : 1;
    const int64_t per = mode == MRFP_CE_IMAGE_MEAN ? nbx : (int64_t)nbx * B;
    double total = 0.0;        // thread 0
    for (int g = 0; g < groups; ++g) {
        double a, d;
        ce_reduce_partials(ws + 2 * (int64_t)g * per, per, a, d);
        if (threadIdx.x == 0) {
            if (mode == MRFP_CE_SUM) total = a;
            else total += a / (d + bias);         // 0/0 -> NaN: an all-ignored batch (MEAN, as torch) or image (IMAGE_MEAN)
            loss[1 + g] = (float)(d + bias);
        }
    }
    if (threadIdx.x == 0) loss[0] = (float)total;
}

// CP = C rounded up to 8, as a compile-time value
template <typename F>
static void by_class_pad(int C, F&& f) {
    switch ((C + 7) / 8) {
        case 1: f(Int<8>{}); break;
        case 2: f(Int<16>{}); break;
        case 3: f(Int<24>{}); break;
        case 4: f(Int<32>{}); break;
        case 5: f(Int<40>{}); break;
        case 6: f(Int<48>{}); break;
        case 7: f(Int<56>{}); break;
        default: f(Int<64>{}); break;
    }
}

// ---- the pixel-loop skeleton ----------------------------------------------------------------------------------------------------
// The grid is (nbx, B): a workgroup works inside ONE image, stages what the criterion keeps in LDS for that image once (its weight
// row: a run-time class index never touches the register-resident class vector), walks the image's pixels with the class vector
// of a pixel in registers, and its (num, den) partial belongs to one image's denominator.
//
// A Source supplies the class vector: HW (pixels per image), C, load(b, p, z) and store(b, p, g) for a float (&)[CP], and the index
// type its pixels are counted in.  Pointers are untyped on the host; the kernel's T types them.
struct DenseRows {                 // NHWC rows of pitch C, one scalar conversion per class
    using index_t = int64_t;
    const void* logits; void* dlogits; int64_t HW; int C;
    template <typename T, int CP>
    __device__ __forceinline__ void load(int b, int64_t p, float (&z)[CP]) const {
        const T* l = (const T*)logits + (int64_t)b * HW * C + p * C;
#pragma unroll
        for (int c = 0; c < CP; ++c) z[c] = c < C ? to_f(l[c]) : 0.f;
    }
    template <typename T, int CP>
    __device__ __forceinline__ void store(int b, int64_t p, const float (&g)[CP]) const {
        T* d = (T*)dlogits + (int64_t)b * HW * C + p * C;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) d[c] = from_f<T>(g[c]);
    }
};

struct BilinearRows {              // up_logits of the low-resolution scores P (pitch ld); the gradient row has pitch Cd
    using index_t = int;
    const void* P; void* dlogits; int ld, Cd, Hi, Wi, H, W, HW, C;
    template <typename T, int CP>
    __device__ __forceinline__ void load(int b, int p, float (&z)[CP]) const {
        const int oh = p / W, ow = p - oh * W;
        up_logits<T, CP>((const T*)P, ld, Hi, Wi, H, W, C, b, oh, ow, z);
    }
    template <typename T, int CP>
    __device__ __forceinline__ void store(int b, int p, const float (&g)[CP]) const {
        store_class_row<T, CP>((T*)dlogits + (int64_t)b * HW * Cd + (int64_t)p * Cd, Cd, g);
    }
};

// A Criterion supplies: target (one value per pixel), kLdsFloats and stage(sw, b, C), label(raw target, C) -> the value the rest
// sees, valid(t, C), add_loss(z, C, t, sw, num, den); for the backward bwd_factor(loss, gscale, b) and grad(g, C, t, sw, k), which
// turns the class vector into its gradient in place; on the host kMaxClassPad (the widest CP it is built for), mode and kDenBias
// of its finalize.
template <typename T, int CP, typename Source, typename Criterion>
__global__ __launch_bounds__(kCeThreads) void pixel_loss_fwd_kernel(const Source src, const Criterion crit, float* __restrict__ ws) {
    using index_t = typename Source::index_t;
    __shared__ float sw[Criterion::kLdsFloats];
    const int b = blockIdx.y, C = src.C;
    crit.stage(sw, b, C);
    const auto* tb = crit.target + (int64_t)b * src.HW;
    float num = 0.f, den = 0.f;
    for (index_t p = (index_t)blockIdx.x * kCeThreads + threadIdx.x; p < src.HW; p += (index_t)gridDim.x * kCeThreads) {
        const auto t = crit.label(tb[p], C);
        if (!crit.valid(t, C)) continue;
        float z[CP];
        src.template load<T, CP>(b, p, z);
        crit.template add_loss<CP>(z, C, t, sw, num, den);
    }
    ce_w_store_partial(num, den, ws);
}

// every row is stored: zeros for a pixel that does not count
template <typename T, int CP, typename Source, typename Criterion>
__global__ __launch_bounds__(kCeThreads) void pixel_loss_bwd_kernel(const Source src, const Criterion crit, const float* __restrict__ loss,
                                                                    const float* __restrict__ gscale) {
    using index_t = typename Source::index_t;
    __shared__ float sw[Criterion::kLdsFloats];
    const int b = blockIdx.y, C = src.C;
    crit.stage(sw, b, C);
    const float k = crit.bwd_factor(loss, gscale, b);
    const auto* tb = crit.target + (int64_t)b * src.HW;
    for (index_t p = (index_t)blockIdx.x * kCeThreads + threadIdx.x; p < src.HW; p += (index_t)gridDim.x * kCeThreads) {
        const auto t = crit.label(tb[p], C);
        float g[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) g[c] = 0.f;
        if (crit.valid(t, C)) {
            src.template load<T, CP>(b, p, g);
            crit.template grad<CP>(g, C, t, sw, k);
        }
        src.template store<T, CP>(b, p, g);
    }
}

// ---- host side of the skeleton --------------------------------------------------------------------------------------------------
static int wstride_check(const char* who, int64_t wstride, int64_t C) {
    MRFP_CHECK(wstride == 0 || wstride == C, "%s: wstride must be 0 (one weight row) or C (one per image) (wstride=%lld C=%lld)", who,
               (long long)wstride, (long long)C);
    return 0;
}

// The 16-byte pitches and alignment every entry of a fused kernel (up_logits, store_class_row) needs, refused under the entry's
// name.  dlogits / Cd: null / 0 in a forward.  exact_Cd: the gradient pitch must be C rounded up to a chunk, not merely hold it.
static int class_pitch_check(const char* who, const void* P, int64_t ld, const void* dlogits, int64_t Cd, bool exact_Cd, int dtype,
                             int64_t C) {
    MRFP_CHECK(dtype_known(dtype), "%s: unknown dtype %d", who, dtype);
    const int epc = 16 / dtype_bytes(dtype);
    const int64_t Cr = (C + epc - 1) / epc * epc;
    if (!dlogits)
        MRFP_CHECK(ld % epc == 0 && ld >= Cr && aligned16(P), "%s: the score buffer must be channel-padded to 16-byte chunks (ld=%lld)", who,
                   (long long)ld);
    else if (exact_Cd)
        MRFP_CHECK(ld % epc == 0 && Cd == Cr && ld >= Cd && aligned16(P) && aligned16(dlogits),
                   "%s: ld a 16-byte multiple, Cd = C rounded up to one (ld=%lld Cd=%lld)", who, (long long)ld, (long long)Cd);
    else
        MRFP_CHECK(ld % epc == 0 && Cd % epc == 0 && Cd >= C && ld >= Cd && aligned16(P) && aligned16(dlogits),
                   "%s: channel pitches must be 16-byte multiples (ld=%lld Cd=%lld)", who, (long long)ld, (long long)Cd);
    return 0;
}

// the geometry an entry that launches the skeleton on the fused source refuses, and the source it then launches with
static int bilinear_rows(const char* who, const void* P, int64_t ld, void* dlogits, int64_t Cd, bool exact_Cd, int dtype, int64_t Hi,
                         int64_t Wi, int64_t H, int64_t W, int64_t C, BilinearRows& src) {
    MRFP_CHECK(Hi > 0 && Wi > 0 && H > 0 && W > 0 && H * W < (1LL << 30), "%s: bad size", who);
    if (int rc = class_pitch_check(who, P, ld, dlogits, Cd, exact_Cd, dtype, C)) return rc;
    src = BilinearRows{P, dlogits, (int)ld, (int)Cd, (int)Hi, (int)Wi, (int)H, (int)W, (int)(H * W), (int)C};
    return 0;
}

// by_dtype x by_class_pad: f(Tag<T>, Int<CP>) launches one instance; CP above MaxCP is never built
template <int MaxCP, typename F>
static int by_dtype_class_pad(int dtype, const char* who, int C, F&& f) {
    return by_dtype(dtype, who, [&](auto t) {
        by_class_pad(C, [&](auto cp) {
            if constexpr (decltype(cp)::value <= MaxCP) f(t, cp);
        });
        MRFP_LAUNCH_CHECK();
        return 0;
    });
}

template <typename Source, typename Criterion>
static int launch_pixel_loss_fwd(const char* who, int dtype, int64_t B, const Source& src, const Criterion& crit, float* ws, float* loss,
                                 hipStream_t st) {
    const int nbx = ce_w_blocks_x(B, src.HW);
    if (int rc = by_dtype_class_pad<Criterion::kMaxClassPad>(dtype, who, src.C, [&](auto t, auto cp) {
            hipLaunchKernelGGL((pixel_loss_fwd_kernel<typename decltype(t)::type, decltype(cp)::value, Source, Criterion>), dim3(nbx, (unsigned)B),
                               dim3(kCeThreads), 0, st, src, crit, ws);
        }))
        return rc;
    hipLaunchKernelGGL(ce_w_finalize_kernel<Criterion>, dim3(1), dim3(256), 0, st, ws, nbx, (int)B, crit.mode, loss);
    MRFP_LAUNCH_CHECK();
    return 0;
}

template <typename Source, typename Criterion>
static int launch_pixel_loss_bwd(const char* who, int dtype, int64_t B, const Source& src, const Criterion& crit, const float* loss,
                                 const float* gscale, hipStream_t st) {
    const int nbx = ce_w_blocks_x(B, src.HW);
    return by_dtype_class_pad<Criterion::kMaxClassPad>(dtype, who, src.C, [&](auto t, auto cp) {
        hipLaunchKernelGGL((pixel_loss_bwd_kernel<typename decltype(t)::type, decltype(cp)::value, Source, Criterion>), dim3(nbx, (unsigned)B),
                           dim3(kCeThreads), 0, st, src, crit, loss, gscale);
    });
}

}  // namespace mrfp
