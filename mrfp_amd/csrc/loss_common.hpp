// loss_common.hpp -- what the loss translation units share (loss.hip: the cross-entropy family; relax.hip: relaxed targets and the
// soft-NLL family): the workgroup size, the per-image grid cap, the in-kernel align-corners bilinear interpolation of the
// low-resolution class scores, the per-workgroup (num, den) partial and the compile-time class-count dispatch.
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

// workgroups per image of a (nbx, B) grid in which a workgroup stays inside one image: at most 2048 over the launch
static int ce_w_blocks_x(int64_t B, int64_t HW) {
    int64_t n = (HW + kCeThreads - 1) / kCeThreads, cap = 2048 / (B > 0 ? B : 1);
    if (cap < 1) cap = 1;
    if (n > cap) n = cap;
    if (n < 1) n = 1;
    return (int)n;
}

__device__ __forceinline__ void ce_w_store_partial(float num, float den, float* __restrict__ ws) {
    __shared__ float sm[2][kCeThreads / 64];
    num = wave_sum(num);
    den = wave_sum(den);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[0][w] = num; sm[1][w] = den; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, d = 0.f;
        for (int i = 0; i < kCeThreads / 64; ++i) { a += sm[0][i]; d += sm[1][i]; }
        const int64_t slot = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        ws[2 * slot] = a;
        ws[2 * slot + 1] = d;
    }
}

// CP = C rounded up to 8, as a compile-time value (the dispatch of dispatch_up_ce, for any body)
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

}  // namespace mrfp
