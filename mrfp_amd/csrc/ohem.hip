// ohem.hip -- online hard example mining for the cross entropy: the exact kept set of a batch, on the device, with no host wait
// (include/mrfp_hip.h: mrfp_ohem_*, mrfp_upsample_ohem_target, mrfp_select_kth; the definition is in DESIGN.md section 8).
//
// Replaces the criterion a caller hands to the reference's DeepV3Plus as `criterion` / `criterion_aux` (network/deepv3.py:111; the
// published OhemCrossEntropy2dTensor, whose source is not in the reference tree): full-resolution fp32 logits, a soft-max over them,
// a host-visible sort of every probability and a branch on a host value.  Here
//   1. one pass writes p = softmax(z)[t] of every pixel to an fp32 plane (the class vector in registers, from either Source of
//      loss_common.hpp), counts the valid pixels and those with p <= thresh, and fills the first-level histogram of p's bits;
//   2. a radix select (11 + 11 + 10 bits) finds the exact bit pattern of the min_kept-th smallest p: a histogram over the elements
//      that match the prefix so far, then a one-workgroup scan that moves prefix and residual rank along in a small device state;
//   3. one pass writes the int64 masked target (t where kept, ignore_index elsewhere) and counts what it kept.
// The regime (keep all / thresh / k-th) is decided by the first scan from device values; the later select passes leave at once
// when it is settled.  Every count is an integer sum (LDS histogram, integer vector atomics): two runs are bit-identical.  The loss
// and its gradient then run on the existing cross-entropy kernels (loss.hip) over the masked target.
#include "loss_common.hpp"

namespace mrfp {

constexpr unsigned kOhemSentinelBits = 0x40000000u;      // 2.0f: an invalid pixel; above every probability, in no count
constexpr unsigned kOhemNanBits = 0x7fc00000u;           // every NaN p is stored as this one: above +inf in unsigned order, last as in torch.sort
constexpr unsigned kOhemInfBits = 0x7f800000u;
constexpr int kSelBits0 = 11, kSelBits1 = 11, kSelBits2 = 10;
constexpr int kSelBins = 1 << kSelBits0;                 // bins of the widest level
// the device state, 32-bit words at the head of the workspace; the three histograms follow
enum { ST_N = 0, ST_KEPT = 1, ST_THETA = 2, ST_MODE = 3, ST_PREFIX = 4, ST_RANK = 5, ST_DONE = 6, ST_LE = 7, ST_KTH = 8, ST_WORDS = 16 };
constexpr int kOhemWsWords = ST_WORDS + 3 * kSelBins;

__device__ __forceinline__ unsigned* sel_hist(unsigned* ws, int level) { return ws + ST_WORDS + level * kSelBins; }

__device__ __forceinline__ int sel_bin(unsigned bits, int level) {
    return level == 0 ? (int)(bits >> (kSelBits1 + kSelBits2)) : level == 1 ? (int)((bits >> kSelBits2) & ((1u << kSelBits1) - 1u))
                                                                              : (int)(bits & ((1u << kSelBits2) - 1u));
}
// the bits above a level's digit
__device__ __forceinline__ unsigned sel_prefix(unsigned bits, int level) {
    return level == 0 ? 0u : level == 1 ? bits >> (kSelBits1 + kSelBits2) : bits >> kSelBits2;
}

__global__ void ohem_clear_kernel(unsigned* __restrict__ ws) {
    const int i = blockIdx.x * kCeThreads + threadIdx.x;
    if (i < kOhemWsWords) ws[i] = 0u;
}

// the workgroup's LDS histogram into the level's global one, and its two counters into the state
__device__ __forceinline__ void sel_flush(const unsigned* lh, unsigned* __restrict__ hist) {
    for (int i = threadIdx.x; i < kSelBins; i += kCeThreads)
        if (lh[i]) atomicAdd(&hist[i], lh[i]);
}

// p of one valid pixel: exp(z_t - max) over the sum of the exponentials, with the denominator and the quotient in double and one
// rounding to float (the rule of predict.hip's confidence).  Neither source of an error that grows with |ln p| is in it: expf, not
// the scaled-argument __expf; and the numerator's argument x = z_t - max, whose rounding to float (half an ulp of |x|: 8 ulp of p
// at x = -25, measured 16 with fp32 scores) would pass straight into p, is formed in double and split into a float xh and the
// remainder xl: exp(x) = expf(xh) * (1 + xl), xl^2 < 1e-10.  The denominator's terms keep the float argument: those that carry
// weight have a small |x|.
template <int CP>
__device__ __forceinline__ float ohem_prob(const float (&z)[CP], int C, int tg) {
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < CP; ++c) if (c < C) m = fmaxf(m, z[c]);
    double den = 0.0;
    float zt = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c)
        if (c < C) {
            den += (double)expf(z[c] - m);
            zt = (c == tg) ? z[c] : zt;
        }
    const double x = (double)zt - (double)m;
    const float xh = (float)x, xl = xh == -INFINITY ? 0.f : (float)(x - (double)xh);        // z_t = -inf: p = 0, as torch
    const float p = (float)((double)expf(xh) * (1.0 + (double)xl) / den);
    return p != p ? __uint_as_float(kOhemNanBits) : p;
}

// Pass 1 on the (nbx, B) grid of the loss kernels.  The fused Source's class vector is rounded to the storage type and widened
// again: the logits the stock chain (upsample, .float()) hands its soft-max, as predict.hip does.
template <typename T, int CP, typename Source>
__global__ __launch_bounds__(kCeThreads) void ohem_prob_kernel(const Source src, const int64_t* __restrict__ target, int64_t ignore,
                                                               float thresh, float* __restrict__ prob, unsigned* __restrict__ ws) {
    using index_t = typename Source::index_t;
    __shared__ unsigned lh[kSelBins];
    __shared__ unsigned cnt[2];
    for (int i = threadIdx.x; i < kSelBins; i += kCeThreads) lh[i] = 0u;
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0u;
    __syncthreads();
    const int b = blockIdx.y, C = src.C;
    const int64_t* tb = target + (int64_t)b * src.HW;
    float* pb = prob + (int64_t)b * src.HW;
    unsigned nvalid = 0u, nle = 0u;
    for (index_t p = (index_t)blockIdx.x * kCeThreads + threadIdx.x; p < src.HW; p += (index_t)gridDim.x * kCeThreads) {
        const int64_t tg = tb[p];
        if (tg == ignore || tg < 0 || tg >= C) {
            pb[p] = __uint_as_float(kOhemSentinelBits);
            continue;
        }
        float z[CP];
        src.template load<T, CP>(b, p, z);
        if constexpr (std::is_same<Source, BilinearRows>::value && !std::is_same<T, float>::value) {
#pragma unroll
            for (int c = 0; c < CP; ++c) z[c] = to_f(from_f<T>(z[c]));
        }
        const float pr = ohem_prob<CP>(z, C, (int)tg);
        pb[p] = pr;
        nvalid += 1u;
        nle += pr <= thresh ? 1u : 0u;
        atomicAdd(&lh[sel_bin(__float_as_uint(pr), 0)], 1u);
    }
    if (nvalid) atomicAdd(&cnt[0], nvalid);
    if (nle) atomicAdd(&cnt[1], nle);
    __syncthreads();
    sel_flush(lh, sel_hist(ws, 0));
    if (threadIdx.x == 0) {
        if (cnt[0]) atomicAdd(&ws[ST_N], cnt[0]);
        if (cnt[1]) atomicAdd(&ws[ST_LE], cnt[1]);
    }
}

// One level of the select over a plain fp32 array with sentinels: the histogram of the level's digit over the elements whose
// higher bits equal the prefix.  Level 0 also counts the elements (the probability pass does both for the criterion).
__global__ __launch_bounds__(kCeThreads) void sel_hist_kernel(const float* __restrict__ x, int64_t n, int level, unsigned* __restrict__ ws) {
    if (ws[ST_DONE]) return;                 // settled by an earlier scan (uniform over the launch: written by a kernel before this one)
    __shared__ unsigned lh[kSelBins];
    __shared__ unsigned cnt;
    for (int i = threadIdx.x; i < kSelBins; i += kCeThreads) lh[i] = 0u;
    if (threadIdx.x == 0) cnt = 0u;
    __syncthreads();
    const unsigned prefix = ws[ST_PREFIX];
    unsigned mine = 0u;
    for (int64_t i = (int64_t)blockIdx.x * kCeThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kCeThreads) {
        const unsigned bits = __float_as_uint(x[i]);
        if (bits == kOhemSentinelBits || sel_prefix(bits, level) != prefix) continue;
        mine += 1u;
        atomicAdd(&lh[sel_bin(bits, level)], 1u);
    }
    if (level == 0 && mine) atomicAdd(&cnt, mine);
    __syncthreads();
    sel_flush(lh, sel_hist(ws, level));
    if (level == 0 && threadIdx.x == 0 && cnt) atomicAdd(&ws[ST_N], cnt);
}

// One workgroup.  Level 0 first settles the regime: for the criterion (ohem != 0) keep-all (N == 0 or min_kept > N) and thresh
// (min_kept == 0, or at least min_kept probabilities <= thresh, so the min_kept-th smallest is no larger) end the select; for the
// plain select a rank above the element count ends it with NaN.  Otherwise the bin that holds rank k becomes the next digit of the
// prefix and k the rank inside it; after the last level the prefix is the bit pattern of the k-th smallest element.
__global__ __launch_bounds__(kCeThreads) void sel_scan_kernel(int level, int ohem, int64_t k, float thresh, unsigned* __restrict__ ws,
                                                              float* __restrict__ out) {
    __shared__ unsigned part[kCeThreads];
    if (ws[ST_DONE]) return;
    const unsigned N = ws[ST_N];
    if (level == 0) {
        int mode = -1;
        unsigned theta = __float_as_uint(thresh), kth = kOhemNanBits;
        if (ohem) {
            if (N == 0u || k > (int64_t)N) { mode = 0; theta = kOhemInfBits; }
            else if (k == 0 || (int64_t)ws[ST_LE] >= k) mode = 1;
        } else if (k > (int64_t)N) {
            mode = 0;
        }
        if (mode >= 0) {        // uniform: every thread read the same words
            __syncthreads();    // ... before thread 0 changes one of them
            if (threadIdx.x == 0) {
                ws[ST_DONE] = 1u;
                ws[ST_MODE] = (unsigned)mode;
                ws[ST_THETA] = theta;
                ws[ST_KTH] = kth;
                if (out) out[0] = __uint_as_float(kth);
            }
            return;
        }
    }
    const unsigned rank = level == 0 ? (unsigned)k : ws[ST_RANK];        // 1 <= rank <= elements under the prefix
    const unsigned prefix = ws[ST_PREFIX];
    const unsigned* hist = sel_hist(ws, level);
    const int bits = level == 0 ? kSelBits0 : level == 1 ? kSelBits1 : kSelBits2;
    const int per = (1 << bits) / kCeThreads;                            // bins per thread, consecutive
    unsigned s = 0u;
    for (int j = 0; j < per; ++j) s += hist[threadIdx.x * per + j];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned before = 0u;
        int t = 0;
        while (t < kCeThreads - 1 && before + part[t] < rank) before += part[t++];
        int bin = t * per;
        while (bin < t * per + per - 1 && before + hist[bin] < rank) before += hist[bin++];
        const unsigned next = (prefix << bits) | (unsigned)bin;
        ws[ST_PREFIX] = next;
        ws[ST_RANK] = rank - before;
        if (level == 2) {
            const float q = __uint_as_float(next);
            const bool above = q > thresh;                                // false for a NaN q: the threshold stays
            ws[ST_KTH] = next;
            ws[ST_THETA] = above ? next : __float_as_uint(thresh);
            ws[ST_MODE] = above ? 2u : 1u;
            ws[ST_DONE] = 1u;
            if (out) out[0] = q;
        }
    }
}

// Pass 3: the masked target and the kept count.  Mode 0 keeps every valid pixel; otherwise a valid pixel with p <= theta (ties at
// theta kept, a NaN p never).
__global__ __launch_bounds__(kCeThreads) void ohem_mask_kernel(const int64_t* __restrict__ target, const float* __restrict__ prob, int64_t n,
                                                               int C, int64_t ignore, int64_t* __restrict__ masked, unsigned* __restrict__ ws) {
    __shared__ unsigned cnt;
    if (threadIdx.x == 0) cnt = 0u;
    __syncthreads();
    const unsigned mode = ws[ST_MODE];
    const float theta = __uint_as_float(ws[ST_THETA]);
    unsigned mine = 0u;
    for (int64_t i = (int64_t)blockIdx.x * kCeThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kCeThreads) {
        const int64_t tg = target[i];
        const bool valid = !(tg == ignore || tg < 0 || tg >= C);
        const bool kept = valid && (mode == 0u || prob[i] <= theta);
        masked[i] = kept ? tg : ignore;
        mine += kept ? 1u : 0u;
    }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0 && cnt) atomicAdd(&ws[ST_KEPT], cnt);
}

static int sel_blocks(int64_t n) {
    int64_t b = (n + kCeThreads - 1) / kCeThreads;
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (int)b;
}

static int ohem_clear(unsigned* ws, hipStream_t st) {
    hipLaunchKernelGGL(ohem_clear_kernel, dim3((kOhemWsWords + kCeThreads - 1) / kCeThreads), dim3(kCeThreads), 0, st, ws);
    MRFP_LAUNCH_CHECK();
    return 0;
}

// the scans of all levels and the histograms of levels first..2 over x
static int sel_passes(const float* x, int64_t n, int first, int ohem, int64_t k, float thresh, unsigned* ws, float* out, hipStream_t st) {
    for (int level = 0; level < 3; ++level) {
        if (level >= first) {
            hipLaunchKernelGGL(sel_hist_kernel, dim3(sel_blocks(n)), dim3(kCeThreads), 0, st, x, n, level, ws);
            MRFP_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(sel_scan_kernel, dim3(1), dim3(kCeThreads), 0, st, level, ohem, k, thresh, ws, out);
        MRFP_LAUNCH_CHECK();
    }
    return 0;
}

// what the two criterion entries refuse alike, each under its own name
static int ohem_check(const char* who, int dtype, int64_t B, int64_t HW, int64_t C, float thresh, int64_t min_kept) {
    MRFP_CHECK(dtype_known(dtype), "%s: unknown dtype %d", who, dtype);
    MRFP_CHECK(C >= 1 && C <= kMaxClasses, "%s: 1 <= C <= %d (C=%lld)", who, kMaxClasses, (long long)C);
    MRFP_CHECK(min_kept >= 0, "%s: min_kept must not be negative (min_kept=%lld)", who, (long long)min_kept);
    MRFP_CHECK(thresh >= 0.f && thresh <= 1.f, "%s: thresh must be in [0, 1] (got %g)", who, (double)thresh);
    MRFP_CHECK(HW > 0 && HW < (1LL << 30), "%s: bad size (H*W=%lld, below 2^30)", who, (long long)HW);
    MRFP_CHECK(B >= 1 && B <= 65535 && B * HW < (1LL << 31), "%s: 1 <= B <= 65535 and B*H*W below 2^31 (B=%lld)", who, (long long)B);
    return 0;
}

template <typename Source>
static int ohem_launch(const char* who, int dtype, int64_t B, const Source& src, const int64_t* target, int64_t ignore, float thresh,
                       int64_t min_kept, float* prob, int64_t* masked, unsigned* ws, hipStream_t st) {
    if (int rc = ohem_clear(ws, st)) return rc;
    const int nbx = ce_w_blocks_x(B, src.HW);
    if (int rc = by_dtype_class_pad<kMaxClasses>(dtype, who, src.C, [&](auto t, auto cp) {
            hipLaunchKernelGGL((ohem_prob_kernel<typename decltype(t)::type, decltype(cp)::value, Source>), dim3(nbx, (unsigned)B),
                               dim3(kCeThreads), 0, st, src, target, ignore, thresh, prob, ws);
        }))
        return rc;
    const int64_t n = B * (int64_t)src.HW;
    if (int rc = sel_passes(prob, n, 1, 1, min_kept, thresh, ws, nullptr, st)) return rc;
    hipLaunchKernelGGL(ohem_mask_kernel, dim3(sel_blocks(n)), dim3(kCeThreads), 0, st, target, prob, n, src.C, ignore, masked, ws);
    MRFP_LAUNCH_CHECK();
    return 0;
}

}  // namespace mrfp

using namespace mrfp;

extern "C" {

int64_t mrfp_ohem_ws_bytes(int64_t B, int64_t HW) {
    if (B < 1 || B > 65535 || HW < 1 || HW >= (1LL << 30) || B * HW >= (1LL << 31)) return -1;
    return (int64_t)kOhemWsWords * 4;
}

int mrfp_select_kth(const float* x, int64_t n, int64_t k, void* ws, float* out, void* stream) {
    MRFP_CHECK(x && ws && out, "select_kth: null pointer");
    MRFP_CHECK(n >= 1 && n < (1LL << 31), "select_kth: 1 <= n < 2^31 (n=%lld)", (long long)n);
    MRFP_CHECK(k >= 1 && k <= n, "select_kth: 1 <= k <= n (k=%lld n=%lld)", (long long)k, (long long)n);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = ohem_clear((unsigned*)ws, st)) return rc;
    return sel_passes(x, n, 0, 0, k, -1.f, (unsigned*)ws, out, st);
}

int mrfp_ohem_target(const void* logits, const int64_t* target, int dtype, int64_t B, int64_t HW, int64_t C, int64_t ignore_index,
                     float thresh, int64_t min_kept, float* prob, int64_t* masked, void* ws, void* stream) {
    const char* who = "ohem_target";
    MRFP_CHECK(logits && target && prob && masked && ws, "%s: null pointer", who);
    if (int rc = ohem_check(who, dtype, B, HW, C, thresh, min_kept)) return rc;
    return ohem_launch(who, dtype, B, DenseRows{logits, nullptr, HW, (int)C}, target, ignore_index, thresh, min_kept, prob, masked,
                       (unsigned*)ws, (hipStream_t)stream);
}

int mrfp_upsample_ohem_target(const void* P, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H,
                              int64_t W, int64_t C, int64_t ignore_index, float thresh, int64_t min_kept, float* prob, int64_t* masked,
                              void* ws, void* stream) {
    const char* who = "upsample_ohem_target";
    MRFP_CHECK(P && target && prob && masked && ws, "%s: null pointer", who);
    MRFP_CHECK(H > 0 && W > 0 && Hi > 0 && Wi > 0, "%s: bad size", who);
    if (int rc = ohem_check(who, dtype, B, H * W, C, thresh, min_kept)) return rc;
    BilinearRows src;
    if (int rc = bilinear_rows(who, P, ld, nullptr, 0, false, dtype, Hi, Wi, H, W, C, src)) return rc;
    return ohem_launch(who, dtype, B, src, target, ignore_index, thresh, min_kept, prob, masked, (unsigned*)ws, (hipStream_t)stream);
}

}  // extern "C"
