// predict.hip -- the prediction path: bilinear upsample (align_corners) of the low-resolution class scores fused with the arg-max,
// the confusion histogram, the largest soft-max probability and the plain cross entropy of a validation pass, and the colour
// coding of a label map.  The full-resolution logits are never written: every lane re-interpolates the 4 taps of its pixel from
// the (L2-resident) low-resolution scores, as the training loss does (loss.hip).
//
// Replaces (reference):
//   main.py:896-909          outputs = model(inputs); np.argmax of the full-size logits on the host; metrics.fast_hist
//   utils/misc.py:139-156    the evaluation bookkeeping that tracks val_loss beside mIoU (build-defined here: sum nll / valid pixels)
//   utils_main.py:28-103     decode_segmap / get_cityscapes_labels: one masked numpy pass per class and colour channel
// and this build's own eval chain  upsample_bilinear -> .float() -> argmax_hist  (a [B,C,H,W] tensor written twice, read twice).
#include "loss_common.hpp"

namespace mrfp {

// One output pixel: the class vector in registers (up_logits), ROUNDED to the storage type and widened again -- the value
// mrfp_bilinear_fwd stores and .float() reads back, so the arg-max is that of the materialised logits bit for bit -- then the first
// maximum (as np.argmax / argmax_hist_kernel).  SM: also the max-subtracted soft-max sums: conf = 1 / sum exp(z - max) with an fp64
// denominator and quotient (prob_accum_kernel's rule: expf's own error + one rounding), nll = (max + log sum) - z[target].
template <typename T, int CP, bool SM>
__device__ __forceinline__ int predict_pixel(const T* __restrict__ P, int ld, int Hi, int Wi, int H, int W, int C, int b, int oh,
                                             int ow, int tg, float& conf, float& nll) {
    float z[CP];
    up_logits<T, CP>(P, ld, Hi, Wi, H, W, C, b, oh, ow, z);
    if constexpr (!std::is_same<T, float>::value) {
#pragma unroll
        for (int c = 0; c < CP; ++c) z[c] = to_f(from_f<T>(z[c]));
    }
    float m = z[0];
    int am = 0;
#pragma unroll
    for (int c = 1; c < CP; ++c)
        if (c < C && z[c] > m) { m = z[c]; am = c; }      // first maximum; pad channels c >= C never take part
    if constexpr (SM) {
        float s = 0.f, zt = 0.f;
        double den = 0.0;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) {
                const float e = expf(z[c] - m);
                s += e;
                den += (double)e;
                zt = (c == tg) ? z[c] : zt;
            }
        conf = (float)(1.0 / den);
        nll = (m + logf(s)) - zt;
    }
    return am;
}

// Grid (workgroups per image, B): a workgroup stays inside image blockIdx.y, so its LDS histogram is that image's.  A lane owns one
// pixel per trip and stores one prediction byte (a wave: 64 consecutive bytes).  Four pixels of a row per lane with one 4-byte
// store was built and measured: slower at every shape (16 x 768 x 768: 520 against 186 us in fp32, 164 against 152 us in bf16;
// profiles/predict.md), so it is not kept.
template <typename T, int CP, bool SM>
__global__ __launch_bounds__(kCeThreads) void upsample_argmax_kernel(const T* __restrict__ P, int ld, const int64_t* __restrict__ target,
                                                                     int Hi, int Wi, int H, int W, int C, int64_t ignore,
                                                                     uint8_t* __restrict__ pred, float* __restrict__ conf,
                                                                     unsigned long long* __restrict__ hist, int hist_stride,
                                                                     float* __restrict__ ws) {
    __shared__ unsigned int lh[kMaxClasses * kMaxClasses];
    const int b = blockIdx.y, HW = H * W;
    if (hist)
        for (int i = threadIdx.x; i < C * C; i += kCeThreads) lh[i] = 0;
    __syncthreads();
    const size_t base = (size_t)b * HW;
    float nll = 0.f, cnt = 0.f;
    for (int p = blockIdx.x * kCeThreads + threadIdx.x; p < HW; p += gridDim.x * kCeThreads) {
        const int oh = p / W, ow = p - oh * W;
        const int64_t t64 = target ? target[base + p] : -1;
        const bool inside = t64 >= 0 && t64 < C;           // labels outside 0..C-1 count nowhere
        const int tg = inside ? (int)t64 : -1;
        float cf = 0.f, l = 0.f;
        const int am = predict_pixel<T, CP, SM>(P, ld, Hi, Wi, H, W, C, b, oh, ow, tg, cf, l);
        if (pred) pred[base + p] = (uint8_t)am;
        if (hist && inside) atomicAdd(&lh[tg * C + am], 1u);
        if constexpr (SM) {
            if (conf) conf[base + p] = cf;
            if (inside && t64 != ignore) { nll += l; cnt += 1.f; }
        }
    }
    __syncthreads();
    if (hist) {
        unsigned long long* h = hist + (size_t)b * hist_stride;
        for (int i = threadIdx.x; i < C * C; i += kCeThreads)
            if (lh[i]) atomicAdd(&h[i], (unsigned long long)lh[i]);
    }
    if constexpr (SM) {
        if (ws) ce_w_store_partial(nll, cnt, ws);          // (uniform over the workgroup: ws is a kernel argument)
    }
}

// the (sum nll, count) partials of one launch, added in double in a fixed order ONTO the caller's accumulator
__global__ __launch_bounds__(256) void predict_loss_finalize_kernel(const float* __restrict__ ws, int n, double* __restrict__ acc) {
    double a, d;
    ce_reduce_partials(ws, n, a, d);
    if (threadIdx.x == 0) { acc[0] += a; acc[1] += d; }
}

// ---- colour coding ----------------------------------------------------------------------------------------------------------
constexpr int kColPix = 4;        // pixels of one lane in the vector body: 4 prediction bytes in, 12 colour bytes out

struct alignas(4) U32x3 { uint32_t v[3]; };

template <bool BLEND>
__device__ __forceinline__ uint32_t colour_byte(const uint8_t* pal, uint32_t cls, int ch, uint32_t img, int a) {
    const uint32_t c = pal[cls * 3 + ch];
    if constexpr (BLEND) return ((uint32_t)a * c + (uint32_t)(256 - a) * img + 128u) >> 8;
    else return c;
}

// out[i] = palette[pred[i]], or the integer blend with image[i].  The 768 palette bytes are staged in LDS.  VEC (all three
// pointers 4-byte aligned): a lane takes 4 pixels -- one 4-byte load of pred, three of the image, three 4-byte stores -- and the
// npix % 4 pixels behind the body go one per lane; otherwise every pixel goes one per lane, byte by byte.
template <bool BLEND, bool VEC>
__global__ __launch_bounds__(kThreads) void colorize_u8_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ palette,
                                                               const uint8_t* __restrict__ image, uint8_t* __restrict__ out,
                                                               int64_t npix, int a) {
    __shared__ uint8_t pal[768];
    for (int i = threadIdx.x; i < 768; i += kThreads) pal[i] = palette[i];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kThreads, t0 = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int64_t done = 0;
    if constexpr (VEC) {
        const int64_t ngrp = npix / kColPix;
        for (int64_t g = t0; g < ngrp; g += stride) {
            const uint32_t pv = *reinterpret_cast<const uint32_t*>(pred + g * kColPix);
            U32x3 iv = {{0u, 0u, 0u}};
            if constexpr (BLEND) iv = *reinterpret_cast<const U32x3*>(image + g * (kColPix * 3));
            U32x3 ov = {{0u, 0u, 0u}};
#pragma unroll
            for (int k = 0; k < kColPix * 3; ++k) {          // byte k of the 12: pixel k / 3, channel k % 3
                const uint32_t cls = (pv >> (8 * (k / 3))) & 255u;
                const uint32_t img = (iv.v[k >> 2] >> (8 * (k & 3))) & 255u;
                ov.v[k >> 2] |= colour_byte<BLEND>(pal, cls, k % 3, img, a) << (8 * (k & 3));
            }
            *reinterpret_cast<U32x3*>(out + g * (kColPix * 3)) = ov;
        }
        done = ngrp * kColPix;
    }
    for (int64_t i = done + t0; i < npix; i += stride) {
        const uint32_t cls = pred[i];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            out[i * 3 + ch] = (uint8_t)colour_byte<BLEND>(pal, cls, ch, BLEND ? image[i * 3 + ch] : 0u, a);
    }
}

static bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace mrfp

using namespace mrfp;

extern "C" {

int64_t mrfp_upsample_argmax_nblocks(int64_t B, int64_t H, int64_t W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    return B * ce_w_blocks_x(B, H * W);
}

int mrfp_upsample_argmax(const void* P, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H,
                         int64_t W, int64_t C, int64_t ignore_index, uint8_t* pred, float* conf, int64_t* hist, int per_image,
                         float* ws, double* loss_acc, void* stream) {
    MRFP_CHECK(P && B > 0 && Hi > 0 && Wi > 0 && H > 0 && W > 0, "upsample_argmax: bad arguments");
    MRFP_CHECK(C > 0 && C <= kMaxClasses, "upsample_argmax: 1 <= C <= %d (C=%lld)", kMaxClasses, (long long)C);
    MRFP_CHECK(dtype_known(dtype), "upsample_argmax: unknown dtype %d", dtype);
    const int epc = 16 / dtype_bytes(dtype);
    MRFP_CHECK(ld % epc == 0 && ld >= (C + epc - 1) / epc * epc && aligned16(P),
               "upsample_argmax: the score buffer must be channel-padded to 16-byte chunks (ld=%lld)", (long long)ld);
    MRFP_CHECK(B <= 65535 && Hi < (1 << 24) && Wi < (1 << 24) && ld < (1 << 24) && H * W < (1LL << 30),
               "upsample_argmax: sizes out of range");
    MRFP_CHECK(pred || conf || hist || loss_acc, "upsample_argmax: no output requested");
    MRFP_CHECK(target || !hist, "upsample_argmax: hist given without target");
    MRFP_CHECK(target || !loss_acc, "upsample_argmax: loss_acc given without target");
    MRFP_CHECK(ws || !loss_acc, "upsample_argmax: loss_acc given without ws (2 * mrfp_upsample_argmax_nblocks floats)");
    MRFP_CHECK(!conf || aligned4(conf), "upsample_argmax: conf must be 4-byte aligned");
    MRFP_CHECK(!loss_acc || (reinterpret_cast<uintptr_t>(loss_acc) & 7) == 0, "upsample_argmax: loss_acc must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int nbx = ce_w_blocks_x(B, H * W);
    const bool sm = conf || loss_acc;
    float* part = loss_acc ? ws : nullptr;
    const int hist_stride = per_image ? (int)(C * C) : 0;
    return by_dtype(dtype, "upsample_argmax", [&](auto t) {
        using T = typename decltype(t)::type;
        by_class_pad((int)C, [&](auto cp) {
            constexpr int CP = decltype(cp)::value;
            const dim3 grid((unsigned)nbx, (unsigned)B);
#define MRFP_PREDICT_LAUNCH(SM)                                                                                                \
    hipLaunchKernelGGL((upsample_argmax_kernel<T, CP, SM>), grid, dim3(kCeThreads), 0, st, (const T*)P, (int)ld, target, (int)Hi, \
                       (int)Wi, (int)H, (int)W, (int)C, ignore_index, pred, conf, (unsigned long long*)hist, hist_stride, part)
            if (sm) MRFP_PREDICT_LAUNCH(true);
            else MRFP_PREDICT_LAUNCH(false);
#undef MRFP_PREDICT_LAUNCH
        });
        MRFP_LAUNCH_CHECK();
        if (loss_acc) {
            hipLaunchKernelGGL(predict_loss_finalize_kernel, dim3(1), dim3(256), 0, st, ws, (int)(B * nbx), loss_acc);
            MRFP_LAUNCH_CHECK();
        }
        return 0;
    });
}

int mrfp_colorize_u8(const void* pred, const void* palette, const void* image, void* out, int64_t npix, int a, void* stream) {
    MRFP_CHECK(pred && palette && out, "colorize_u8: null argument");
    MRFP_CHECK(npix >= 0, "colorize_u8: negative size %lld", (long long)npix);
    MRFP_CHECK(a >= 0 && a <= 256, "colorize_u8: the blend weight must be in 0..256 (a=%d)", a);
    if (npix == 0) return 0;
    const bool vec = aligned4(pred) && aligned4(out) && (!image || aligned4(image));
    int64_t nb = ((vec ? (npix + kColPix - 1) / kColPix : npix) + kThreads - 1) / kThreads;
    if (nb > 2048) nb = 2048;
    const dim3 grid((unsigned)nb);
    hipStream_t st = (hipStream_t)stream;
    const uint8_t *p = (const uint8_t*)pred, *pal = (const uint8_t*)palette, *img = (const uint8_t*)image;
    uint8_t* o = (uint8_t*)out;
    if (image) {
        if (vec) hipLaunchKernelGGL((colorize_u8_kernel<true, true>), grid, dim3(kThreads), 0, st, p, pal, img, o, npix, a);
        else hipLaunchKernelGGL((colorize_u8_kernel<true, false>), grid, dim3(kThreads), 0, st, p, pal, img, o, npix, a);
    } else {
        if (vec) hipLaunchKernelGGL((colorize_u8_kernel<false, true>), grid, dim3(kThreads), 0, st, p, pal, img, o, npix, a);
        else hipLaunchKernelGGL((colorize_u8_kernel<false, false>), grid, dim3(kThreads), 0, st, p, pal, img, o, npix, a);
    }
    MRFP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
