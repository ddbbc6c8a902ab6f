// relax.hip -- boundary label relaxation and the joint-weighted soft-NLL loss (include/mrfp_hip.h: mrfp_relax_*, mrfp_multihot_pack,
// mrfp_soft_nll_*, mrfp_upsample_soft_nll_*; definitions in DESIGN.md section 8).
//
// Replaces (reference): transforms/transforms.py:75-124 RelaxedBoundaryLossToTensor -- (2 border + 1)^2 scipy.ndimage.shift calls and a
// [C+1,H,W] uint8 multi-hot per sample on the host -- and the criterion that consumes its output, handed to DeepV3Plus as `criterion`
// (network/deepv3.py:111; its source is not in the reference tree).  On the device the relaxed target of a pixel is ONE 32-bit word:
// bit c = "class c occurs in the window", bit C = "ignore / outside the image occurs".  With that word the per-class term of the
// published loss, log max(p_c, q) with q the summed probability of the set, is log q for every class of the set, and the loss is
// the difference of two log-sum-exps -- the same streaming as the cross-entropy kernels of loss.hip, 4 B of target per pixel.
#include "loss_common.hpp"

namespace mrfp {

constexpr int kRelaxMaxC = 31;             // classes 0..C-1 and the ignore bit C share one 32-bit word
constexpr int kRelaxMaxBorder = 8;
constexpr int kRelaxTH = 32, kRelaxTW = 64;        // output tile of one pass of a workgroup
constexpr int kRelaxRH = kRelaxTH + 2 * kRelaxMaxBorder, kRelaxRW = kRelaxTW + 2 * kRelaxMaxBorder;      // tile + halo at the widest border

typedef unsigned __attribute__((ext_vector_type(4))) u32x4;

__device__ __forceinline__ unsigned class_word(int64_t t, int C) { return 1u << ((t >= 0 && t < C) ? (int)t : C); }

// ---- class counts: one ballot + popcount per class per wave, kept per wave, one LDS add per class per wave at the end and one
// integer add per class per workgroup to the image's row ---------------------------------------------------------------------
__device__ __forceinline__ void count_bits(unsigned w, unsigned (&cnt)[32]) {
#pragma unroll
    for (int c = 0; c < 32; ++c)
        cnt[c] += (unsigned)__popcll(__ballot((w >> c) & 1u));      // all 32 bits: skipping those above C behind a branch measured slower
}

__device__ __forceinline__ void flush_counts(const unsigned (&cnt)[32], int C, unsigned long long* __restrict__ row) {
    __shared__ unsigned lc[32];
    if (threadIdx.x < 32) lc[threadIdx.x] = 0u;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 32; ++c)
            if (cnt[c]) atomicAdd(&lc[c], cnt[c]);
    }
    __syncthreads();
    if ((int)threadIdx.x <= C && lc[threadIdx.x]) atomicAdd(&row[threadIdx.x], (unsigned long long)lc[threadIdx.x]);
}

__global__ void relax_counts_clear_kernel(unsigned long long* __restrict__ counts, int n) {
    const int i = blockIdx.x * kCeThreads + threadIdx.x;
    if (i < n) counts[i] = 0ull;
}

// The OR over a square window is separable.  Per tile: the labels of the tile and its halo become class words in LDS (each int64
// label read once, the halo apart), OR along x, then OR along y, four words per thread, written once (16 bytes where `vec4`).
// A workgroup stays inside image blockIdx.y and walks tiles blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(kCeThreads) void relax_labels_kernel(const int64_t* __restrict__ target, int H, int W, int C, int r,
                                                                  unsigned strict, int tilesX, int ntiles, int vec4,
                                                                  int32_t* __restrict__ out, unsigned long long* __restrict__ counts) {
    __shared__ unsigned s_in[kRelaxRH * kRelaxRW];
    __shared__ __attribute__((aligned(16))) unsigned s_h[kRelaxRH * kRelaxTW];
    const int b = blockIdx.y;
    const int64_t* tb = target + (int64_t)b * H * W;
    int32_t* ob = out + (int64_t)b * H * W;
    const int RH = kRelaxTH + 2 * r, RW = kRelaxTW + 2 * r;
    unsigned cnt[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) cnt[c] = 0u;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int ty0 = t / tilesX;
        const int y0 = ty0 * kRelaxTH, x0 = (t - ty0 * tilesX) * kRelaxTW;
        for (int i = threadIdx.x; i < RH * RW; i += kCeThreads) {
            const int ry = i / RW, rx = i - ry * RW;
            const int y = y0 + ry - r, x = x0 + rx - r;
            unsigned w = 1u << C;                  // outside the image: the reference's cval = num_classes
            if (y >= 0 && y < H && x >= 0 && x < W) w = class_word(tb[(int64_t)y * W + x], C);
            s_in[i] = w;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < RH * kRelaxTW; i += kCeThreads) {
            const unsigned* p = s_in + (i / kRelaxTW) * RW + (i % kRelaxTW);
            unsigned w = 0u;
            for (int d = 0; d <= 2 * r; ++d) w |= p[d];
            s_h[i] = w;
        }
        __syncthreads();
        for (int q = threadIdx.x; q < kRelaxTH * kRelaxTW / 4; q += kCeThreads) {
            const int ty = q / (kRelaxTW / 4), tx = (q % (kRelaxTW / 4)) * 4;
            u32x4 w = {0u, 0u, 0u, 0u};
            for (int d = 0; d <= 2 * r; ++d) w |= *reinterpret_cast<const u32x4*>(s_h + (ty + d) * kRelaxTW + tx);
            const int y = y0 + ty, x = x0 + tx;
            unsigned o[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned own = s_in[(ty + r) * RW + tx + r + j];
                if (own & strict) o[j] = own;                      // a strict class keeps its own bit only
                if (y >= H || x + j >= W) o[j] = 0u;               // not a pixel: not stored, not counted
            }
            if (counts) {
#pragma unroll
                for (int j = 0; j < 4; ++j) count_bits(o[j], cnt);
            }
            if (y < H) {
                int32_t* dst = ob + (int64_t)y * W + x;
                if (vec4 && x + 3 < W) {
                    const u32x4 v = {o[0], o[1], o[2], o[3]};
                    *reinterpret_cast<u32x4*>(dst) = v;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x + j < W) dst[j] = (int32_t)o[j];
                }
            }
        }
        __syncthreads();           // the next tile's staging overwrites both arrays
    }
    if (counts) flush_counts(cnt, C, counts + (int64_t)b * (C + 1));
}

static int relax_tiles_x(int64_t W) { return (int)((W + kRelaxTW - 1) / kRelaxTW); }
static int64_t relax_tiles(int64_t H, int64_t W) { return ((H + kRelaxTH - 1) / kRelaxTH) * relax_tiles_x(W); }
// workgroups per image: one per tile up to the cap of the loss kernels (2048 workgroups over the launch)
static int relax_blocks_x(int64_t B, int64_t H, int64_t W) {
    int64_t n = relax_tiles(H, W), cap = 2048 / (B > 0 ? B : 1);
    if (cap < 1) cap = 1;
    if (n > cap) n = cap;
    if (n < 1) n = 1;
    return (int)n;
}

// uint8 [B, C+1, HW] multi-hot (any non-zero byte is set) -> words; V pixels per thread (4: one 32-bit load per plane, one 16-byte store)
template <int V>
__global__ __launch_bounds__(kCeThreads) void multihot_pack_kernel(const uint8_t* __restrict__ mh, int64_t HW, int C,
                                                                   int32_t* __restrict__ out, unsigned long long* __restrict__ counts) {
    const int b = blockIdx.y;
    const uint8_t* mb = mh + (int64_t)b * (C + 1) * HW;
    int32_t* ob = out + (int64_t)b * HW;
    unsigned cnt[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) cnt[c] = 0u;
    const int64_t n = HW / V;
    for (int64_t i = (int64_t)blockIdx.x * kCeThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kCeThreads) {
        unsigned o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = 0u;
        for (int c = 0; c <= C; ++c) {
            if constexpr (V == 4) {
                const unsigned v = *reinterpret_cast<const unsigned*>(mb + (int64_t)c * HW + 4 * i);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] |= ((v >> (8 * j)) & 0xffu) ? (1u << c) : 0u;
            } else {
                o[0] |= mb[(int64_t)c * HW + i] ? (1u << c) : 0u;
            }
        }
        if (counts) {
#pragma unroll
            for (int j = 0; j < V; ++j) count_bits(o[j], cnt);
        }
        if constexpr (V == 4) {
            const u32x4 v = {o[0], o[1], o[2], o[3]};
            *reinterpret_cast<u32x4*>(ob + 4 * i) = v;
        } else {
            ob[i] = (int32_t)o[0];
        }
    }
    if (counts) flush_counts(cnt, C, counts + (int64_t)b * (C + 1));
}

// the counts of words that exist already (a loader that delivers words)
__global__ __launch_bounds__(kCeThreads) void relax_word_counts_kernel(const int32_t* __restrict__ words, int64_t HW, int C,
                                                                       unsigned long long* __restrict__ counts) {
    const int b = blockIdx.y;
    const int32_t* wb = words + (int64_t)b * HW;
    const unsigned all = C >= 31 ? 0xffffffffu : ((2u << C) - 1u);
    unsigned cnt[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) cnt[c] = 0u;
    for (int64_t i = (int64_t)blockIdx.x * kCeThreads + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kCeThreads)
        count_bits((unsigned)wb[i] & all, cnt);
    flush_counts(cnt, C, counts + (int64_t)b * (C + 1));
}

// f_c = n_c / sum_{c=0..C} n_c (the ignore plane counts in the total) and w_c in double, one rounding to float (the translation
// unit is built with -ffp-contract=off: no fused multiply-add).  batch: the rows of all images pooled into one.
__global__ void relax_weights_kernel(const unsigned long long* __restrict__ counts, int B, int C, int batch, double ub, int norm,
                                     float* __restrict__ out) {
    const int i = blockIdx.x * kCeThreads + threadIdx.x;
    if (i >= (batch ? 1 : B) * C) return;
    const int row = i / C, c = i - row * C;
    const int b0 = batch ? 0 : row, b1 = batch ? B : row + 1;
    unsigned long long n = 0ull, total = 0ull;
    for (int b = b0; b < b1; ++b) {
        const unsigned long long* r = counts + (int64_t)b * (C + 1);
        for (int k = 0; k <= C; ++k) total += r[k];
        n += r[c];
    }
    double w = 1.0;
    if (n > 0ull) {
        const double f = (double)n / (double)total;
        w = norm ? 1.0 + ub / f : 1.0 + ub * (1.0 - f);
    }
    out[i] = (float)w;
}

// ---- the loss ------------------------------------------------------------------------------------------------------------------
// sw[0..32): weight row of image b (ones for a null pointer, zeros past C)
__device__ __forceinline__ void soft_stage_weights(float* sw, const float* __restrict__ weight, int64_t wstride, int b, int C) {
    if (threadIdx.x < 32) sw[threadIdx.x] = (int)threadIdx.x < C ? (weight ? weight[(int64_t)b * wstride + threadIdx.x] : 1.f) : 0.f;
    __syncthreads();
}

// W / k of a pixel: the summed weight of its set over the size of the set, one LDS read per set bit.  (The row held in registers
// and summed with CP selects measured slower at the benchmark shape, in two runs: 755 against 735 us forward + backward, 150 against 126 VGPRs;
// profiles/relaxed_loss.md.)
__device__ __forceinline__ float soft_set_weight(const float* sw, unsigned S) {
    const float k = (float)__popc(S);
    float W = 0.f;
    while (S) {
        W += sw[__ffs((int)S) - 1];
        S &= S - 1u;
    }
    return W / k;
}

// The two log-sum-exps, m + log(sa) over all classes and mS + log(sS) over the set.  While the set's maximum is within kSoftShift of
// the overall one, both sums share the exponentials exp(z - m) and mS is returned as m (sS >= exp(-kSoftShift), far above the
// smallest normal float).  A set whose logits lie further below (a confident wrong pixel: exp(z - m) would sum to 0 over the set)
// gets its sum around its own maximum, sS >= 1.
constexpr float kSoftShift = 64.f;

template <int CP>
__device__ __forceinline__ void soft_lse(const float (&z)[CP], int C, unsigned S, float& m, float& sa, float& mS, float& sS) {
    m = -INFINITY;
    mS = -INFINITY;
#pragma unroll
    for (int c = 0; c < CP; ++c)
        if (c < C) {
            m = fmaxf(m, z[c]);
            mS = ((S >> c) & 1u) ? fmaxf(mS, z[c]) : mS;
        }
    sa = 0.f;
    sS = 0.f;
    if (m - mS <= kSoftShift) {
        mS = m;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) {
                const float e = __expf(z[c] - m);
                sa += e;
                sS += ((S >> c) & 1u) ? e : 0.f;
            }
    } else {
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) {
                sa += __expf(z[c] - m);
                sS += ((S >> c) & 1u) ? __expf(z[c] - mS) : 0.f;
            }
    }
}

template <int CP>
__device__ __forceinline__ float soft_pixel_loss(const float (&z)[CP], int C, unsigned S, const float* sw) {
    float m, sa, mS, sS;
    soft_lse<CP>(z, C, S, m, sa, mS, sS);
    return soft_set_weight(sw, S) * ((m - mS) + (__logf(sa) - __logf(sS)));
}

// z -> d(loss)/dz of one valid pixel, k = gscale / (valid_b + 1)
template <int CP>
__device__ __forceinline__ void soft_pixel_grad(float (&z)[CP], int C, unsigned S, const float* sw, float k) {
    float m, sa, mS, sS;
    soft_lse<CP>(z, C, S, m, sa, mS, sS);
    const float f = soft_set_weight(sw, S) * k, ia = 1.f / sa, iS = 1.f / sS;
    if (mS == m) {          // the shared exponentials (also a set that holds the overall maximum)
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            const float e = __expf(z[c] - m);
            z[c] = c < C ? f * (e * ia - (((S >> c) & 1u) ? e * iS : 0.f)) : 0.f;
        }
    } else {
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            const float in_set = ((S >> c) & 1u) ? __expf(z[c] - mS) * iS : 0.f;
            z[c] = c < C ? f * (__expf(z[c] - m) * ia - in_set) : 0.f;
        }
    }
}

// The criterion of the pixel-loop skeleton (loss_common.hpp): the target is a word, its class bits the set S; a pixel counts while S
// is not empty.  One group of partials per image; the finalize adds 1 to each denominator (the published valid_b + 1: an
// all-ignored image adds 0 / 1), and the backward divides by it.  Built for CP <= 32: the class counts a word holds.
struct SoftNll {
    static constexpr int kLdsFloats = 32, kMaxClassPad = 32, mode = MRFP_CE_IMAGE_MEAN;
    static constexpr double kDenBias = 1.0;
    const int32_t* target; const float* weight; int64_t wstride;

    __device__ __forceinline__ void stage(float* sw, int b, int C) const { soft_stage_weights(sw, weight, wstride, b, C); }
    __device__ __forceinline__ unsigned label(int32_t word, int C) const { return (unsigned)word & ((1u << C) - 1u); }
    __device__ __forceinline__ bool valid(unsigned S, int) const { return S != 0u; }
    __device__ __forceinline__ float bwd_factor(const float* __restrict__ loss, const float* __restrict__ gscale, int b) const {
        return (gscale ? gscale[0] : 1.f) / loss[1 + b];
    }
    template <int CP>
    __device__ __forceinline__ void add_loss(const float (&z)[CP], int C, unsigned S, const float* sw, float& num, float& den) const {
        num += soft_pixel_loss<CP>(z, C, S, sw);
        den += 1.f;
    }
    template <int CP>
    __device__ __forceinline__ void grad(float (&g)[CP], int C, unsigned S, const float* sw, float k) const {
        soft_pixel_grad<CP>(g, C, S, sw, k);
    }
};

// what every entry that takes a class count refuses alike, each under its own name
static int relax_check(const char* who, int64_t B, int64_t C) {
    MRFP_CHECK(C >= 1 && C <= kRelaxMaxC, "%s: 1 <= C <= %d (C=%lld)", who, kRelaxMaxC, (long long)C);
    MRFP_CHECK(B >= 1 && B <= 65535, "%s: 1 <= B <= 65535 (B=%lld)", who, (long long)B);
    return 0;
}

static int soft_nll_check(const char* who, int64_t B, int64_t C, int64_t wstride) {
    if (int rc = relax_check(who, B, C)) return rc;
    return wstride_check(who, wstride, C);
}

static int clear_counts(int64_t* counts, int64_t B, int64_t C, hipStream_t st) {
    const int n = (int)(B * (C + 1));
    hipLaunchKernelGGL(relax_counts_clear_kernel, dim3((n + kCeThreads - 1) / kCeThreads), dim3(kCeThreads), 0, st,
                       (unsigned long long*)counts, n);
    MRFP_LAUNCH_CHECK();
    return 0;
}

}  // namespace mrfp

extern "C" {

int64_t mrfp_relax_nblocks(int64_t B, int64_t H, int64_t W) { return (int64_t)mrfp::relax_blocks_x(B, H, W) * (B > 0 ? B : 1); }

int mrfp_relax_labels(const int64_t* target, int64_t B, int64_t H, int64_t W, int64_t C, int64_t border, int strict_mask,
                      int32_t* words, int64_t* counts, void* stream) {
    MRFP_CHECK(target && words, "relax_labels: null pointer");
    MRFP_CHECK(H > 0 && W > 0 && H * W < (1LL << 30), "relax_labels: bad size (H=%lld W=%lld)", (long long)H, (long long)W);
    if (int rc = mrfp::relax_check("relax_labels", B, C)) return rc;
    MRFP_CHECK(border >= 0 && border <= mrfp::kRelaxMaxBorder, "relax_labels: 0 <= border <= %d (border=%lld)", mrfp::kRelaxMaxBorder,
               (long long)border);
    hipStream_t st = (hipStream_t)stream;
    if (counts)
        if (int rc = mrfp::clear_counts(counts, B, C, st)) return rc;
    const int64_t ntiles = mrfp::relax_tiles(H, W);
    const unsigned strict = (unsigned)strict_mask & ((1u << C) - 1u);
    const int vec4 = (W % 4 == 0 && mrfp::aligned16(words)) ? 1 : 0;
    hipLaunchKernelGGL(mrfp::relax_labels_kernel, dim3(mrfp::relax_blocks_x(B, H, W), (unsigned)B), dim3(mrfp::kCeThreads), 0, st, target,
                       (int)H, (int)W, (int)C, (int)border, strict, mrfp::relax_tiles_x(W), (int)ntiles, vec4, words,
                       (unsigned long long*)counts);
    MRFP_LAUNCH_CHECK();
    return 0;
}

int mrfp_multihot_pack(const uint8_t* multihot, int64_t B, int64_t HW, int64_t C, int32_t* words, int64_t* counts, void* stream) {
    MRFP_CHECK(multihot && words, "multihot_pack: null pointer");
    MRFP_CHECK(HW > 0 && HW < (1LL << 30), "multihot_pack: bad size (HW=%lld)", (long long)HW);
    if (int rc = mrfp::relax_check("multihot_pack", B, C)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (counts)
        if (int rc = mrfp::clear_counts(counts, B, C, st)) return rc;
    const bool v4 = HW % 4 == 0 && mrfp::aligned16(words) && (reinterpret_cast<uintptr_t>(multihot) & 3) == 0;
    const dim3 grid(mrfp::ce_w_blocks_x(B, v4 ? HW / 4 : HW), (unsigned)B);
    if (v4)
        hipLaunchKernelGGL(mrfp::multihot_pack_kernel<4>, grid, dim3(mrfp::kCeThreads), 0, st, multihot, HW, (int)C, words,
                           (unsigned long long*)counts);
    else
        hipLaunchKernelGGL(mrfp::multihot_pack_kernel<1>, grid, dim3(mrfp::kCeThreads), 0, st, multihot, HW, (int)C, words,
                           (unsigned long long*)counts);
    MRFP_LAUNCH_CHECK();
    return 0;
}

int mrfp_relax_word_counts(const int32_t* words, int64_t B, int64_t HW, int64_t C, int64_t* counts, void* stream) {
    MRFP_CHECK(words && counts, "relax_word_counts: null pointer");
    MRFP_CHECK(HW > 0 && HW < (1LL << 30), "relax_word_counts: bad size (HW=%lld)", (long long)HW);
    if (int rc = mrfp::relax_check("relax_word_counts", B, C)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = mrfp::clear_counts(counts, B, C, st)) return rc;
    hipLaunchKernelGGL(mrfp::relax_word_counts_kernel, dim3(mrfp::ce_w_blocks_x(B, HW), (unsigned)B), dim3(mrfp::kCeThreads), 0, st, words,
                       HW, (int)C, (unsigned long long*)counts);
    MRFP_LAUNCH_CHECK();
    return 0;
}

int mrfp_relax_class_weights(const int64_t* counts, int64_t B, int64_t C, double upper_bound, int norm, int batch, float* weight_out,
                             void* stream) {
    MRFP_CHECK(counts && weight_out, "relax_class_weights: null pointer");
    if (int rc = mrfp::relax_check("relax_class_weights", B, C)) return rc;
    const int n = (int)((batch ? 1 : B) * C);
    hipLaunchKernelGGL(mrfp::relax_weights_kernel, dim3((n + mrfp::kCeThreads - 1) / mrfp::kCeThreads), dim3(mrfp::kCeThreads), 0,
                       (hipStream_t)stream, (const unsigned long long*)counts, (int)B, (int)C, batch ? 1 : 0, upper_bound, norm ? 1 : 0,
                       weight_out);
    MRFP_LAUNCH_CHECK();
    return 0;
}

int64_t mrfp_soft_nll_nblocks(int64_t B, int64_t HW) { return (int64_t)mrfp::ce_w_blocks_x(B, HW) * (B > 0 ? B : 1); }

int64_t mrfp_soft_nll_loss_floats(int64_t B) { return 1 + (B > 0 ? B : 1); }

int mrfp_soft_nll_fwd(const void* logits, const int32_t* words, int dtype, int64_t B, int64_t HW, int64_t C, const float* weight,
                      int64_t wstride, float* ws, float* loss, void* stream) {
    const char* who = "soft_nll_fwd";
    MRFP_CHECK(logits && words && ws && loss, "%s: null pointer", who);
    MRFP_CHECK(HW > 0, "%s: bad size (HW=%lld)", who, (long long)HW);
    if (int rc = mrfp::soft_nll_check(who, B, C, wstride)) return rc;
    return mrfp::launch_pixel_loss_fwd(who, dtype, B, mrfp::DenseRows{logits, nullptr, HW, (int)C}, mrfp::SoftNll{words, weight, wstride}, ws,
                                       loss, (hipStream_t)stream);
}

int mrfp_soft_nll_bwd(const void* logits, const int32_t* words, const float* loss, const float* gscale, void* dlogits, int dtype,
                      int64_t B, int64_t HW, int64_t C, const float* weight, int64_t wstride, void* stream) {
    const char* who = "soft_nll_bwd";
    MRFP_CHECK(logits && words && loss && dlogits, "%s: null pointer", who);
    MRFP_CHECK(HW > 0, "%s: bad size (HW=%lld)", who, (long long)HW);
    if (int rc = mrfp::soft_nll_check(who, B, C, wstride)) return rc;
    return mrfp::launch_pixel_loss_bwd(who, dtype, B, mrfp::DenseRows{logits, dlogits, HW, (int)C}, mrfp::SoftNll{words, weight, wstride}, loss,
                                       gscale, (hipStream_t)stream);
}

int mrfp_upsample_soft_nll_fwd(const void* P, int64_t ld, const int32_t* words, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H,
                               int64_t W, int64_t C, const float* weight, int64_t wstride, float* ws, float* loss, void* stream) {
    const char* who = "upsample_soft_nll_fwd";
    MRFP_CHECK(P && words && ws && loss, "%s: null pointer", who);
    if (int rc = mrfp::soft_nll_check(who, B, C, wstride)) return rc;
    mrfp::BilinearRows src;
    if (int rc = mrfp::bilinear_rows(who, P, ld, nullptr, 0, true, dtype, Hi, Wi, H, W, C, src)) return rc;
    return mrfp::launch_pixel_loss_fwd(who, dtype, B, src, mrfp::SoftNll{words, weight, wstride}, ws, loss, (hipStream_t)stream);
}

int mrfp_upsample_soft_nll_bwd(const void* P, int64_t ld, const int32_t* words, const float* loss, const float* gscale, void* dlogits,
                               int64_t Cd, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H, int64_t W, int64_t C,
                               const float* weight, int64_t wstride, void* stream) {
    const char* who = "upsample_soft_nll_bwd";
    MRFP_CHECK(P && words && loss && dlogits, "%s: null pointer", who);
    if (int rc = mrfp::soft_nll_check(who, B, C, wstride)) return rc;
    mrfp::BilinearRows src;
    if (int rc = mrfp::bilinear_rows(who, P, ld, dlogits, Cd, true, dtype, Hi, Wi, H, W, C, src)) return rc;
    return mrfp::launch_pixel_loss_bwd(who, dtype, B, src, mrfp::SoftNll{words, weight, wstride}, loss, gscale, (hipStream_t)stream);
}

}  // extern "C"
