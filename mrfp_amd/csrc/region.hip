// region.hip -- the soft Dice / Jaccard region loss (include/mrfp_hip.h: mrfp_region_*, mrfp_upsample_region_*; DESIGN.md
// section 8): a direct surrogate of the IoU the evaluation reports, used alone or as CE + lambda * Dice.
//
// A region loss is no per-pixel (num, den) partial: it needs per-class sums over the scope first, and a backward that reads
// per-class coefficients.  So it has three kernels of its own on the skeleton's sources (DenseRows, BilinearRows) and grid:
//   region_sums_kernel      (nbx, B) grid of ce_w_blocks_x: I_c, P_c in registers across a thread's pixels, T_c in LDS integer
//                           counters; one partial row [3][CP] per workgroup, written in a fixed lane order
//   region_finalize_kernel  one workgroup (1024 threads): the partials in double in a fixed order, per image or over all; the loss, the
//                           coefficient table (a_c, b_c) per scope group and the sums
//   region_bwd_kernel       the pixel loop with the coefficient row of its image staged in LDS once per workgroup
// No floating-point atomics and no host wait: an empty class set is decided in the finalize; two runs are bit-identical.
#include "loss_common.hpp"

namespace mrfp {

__device__ __forceinline__ bool region_valid(int64_t tg, int64_t ignore, int C) { return !(tg == ignore || tg < 0 || tg >= C); }

// z -> exp(z - max) for c < C (0 beyond), returns the sum
template <int CP>
__device__ __forceinline__ float region_exps(float (&z)[CP], int C) {
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < CP; ++c) if (c < C) m = fmaxf(m, z[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) { z[c] = c < C ? __expf(z[c] - m) : 0.f; s += z[c]; }
    return s;
}

template <typename T, int CP, typename Source>
__global__ __launch_bounds__(kCeThreads) void region_sums_kernel(const Source src, const int64_t* __restrict__ target, int64_t ignore,
                                                                 float* __restrict__ ws) {
    using index_t = typename Source::index_t;
    __shared__ unsigned int lt[CP];
    __shared__ float sm[kCeThreads / 64][2][CP];
    const int b = blockIdx.y, C = src.C;
    for (int c = threadIdx.x; c < CP; c += kCeThreads) lt[c] = 0u;
    __syncthreads();
    const int64_t* tb = target + (int64_t)b * src.HW;
    float I[CP], Pc[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) { I[c] = 0.f; Pc[c] = 0.f; }
    for (index_t p = (index_t)blockIdx.x * kCeThreads + threadIdx.x; p < src.HW; p += (index_t)gridDim.x * kCeThreads) {
        const int64_t tg = tb[p];
        if (!region_valid(tg, ignore, C)) continue;
        float z[CP];
        src.template load<T, CP>(b, p, z);
        const float inv = 1.f / region_exps<CP>(z, C);
#pragma unroll
        for (int c = 0; c < CP; ++c) {        // predicated updates: a run-time index would put the accumulators in scratch memory
            const float pr = z[c] * inv;
            Pc[c] += pr;
            I[c] += (c == (int)tg) ? pr : 0.f;
        }
        atomicAdd(&lt[(int)tg], 1u);          // an integer count: the order of the additions does not matter
    }
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        const float a = wave_sum(I[c]), d = wave_sum(Pc[c]);
        if (lane == 0) { sm[w][0][c] = a; sm[w][1][c] = d; }
    }
    __syncthreads();
    float* row = ws + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (3 * CP);
    for (int j = threadIdx.x; j < 2 * CP; j += kCeThreads) {
        const int q = j / CP, c = j - q * CP;
        float a = 0.f;
        for (int i = 0; i < kCeThreads / 64; ++i) a += sm[i][q][c];
        row[j] = a;
    }
    for (int c = threadIdx.x; c < CP; c += kCeThreads) reinterpret_cast<unsigned int*>(row)[2 * CP + c] = lt[c];
}

// One workgroup of kRegionFinalThreads threads.  Group r (per_image: image r; else the one group) owns `per` consecutive partial
// rows.  A column of the rows ([3][CP]: 3 * CP <= 192 of them) is summed by kRegionFinalThreads / (3 * CP) threads, each over every
// sub-th row in order, then across those threads in order: a fixed order, in double.  The loads of eight rows are issued together
// (the additions keep their order): one load per addition left this single workgroup waiting on memory latency 2 048 times in a row.
constexpr int kRegionFinalThreads = 1024;

__global__ __launch_bounds__(kRegionFinalThreads) void region_finalize_kernel(const float* __restrict__ ws, int nbx, int B, int C, int CP,
                                                                              const float* __restrict__ weight, int kind, float smooth,
                                                                              int present_only, int per_image, float* __restrict__ out) {
    __shared__ double part[kRegionFinalThreads];
    __shared__ double S[3 * kMaxClasses], term[kMaxClasses], wk[kMaxClasses], dsi[kMaxClasses], dsp[kMaxClasses];
    const int rows = per_image ? B : 1;
    const int64_t per = per_image ? nbx : (int64_t)nbx * B;
    const int ncol = 3 * CP, sub = kRegionFinalThreads / ncol;
    const int col = threadIdx.x % ncol, pi = threadIdx.x / ncol;
    float* coef = out + 2;
    double* sums = reinterpret_cast<double*>(out + 2 + (int64_t)rows * 2 * CP);
    const double s = (double)smooth;
    double total = 0.0;          // thread 0
    int counted = 0;
    for (int r = 0; r < rows; ++r) {
        const float* base = ws + (int64_t)r * per * ncol;
        double acc = 0.0;
        if (pi < sub) {
            const unsigned int* ub = reinterpret_cast<const unsigned int*>(base) + col;
            const bool count = col >= 2 * CP;          // the T columns hold integers
            int64_t i = pi;
            for (; i + 7 * (int64_t)sub < per; i += 8 * (int64_t)sub) {
                unsigned int v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = ub[(i + u * (int64_t)sub) * ncol];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += count ? (double)v[u] : (double)__uint_as_float(v[u]);
            }
            for (; i < per; i += sub) {
                const unsigned int v = ub[i * ncol];
                acc += count ? (double)v : (double)__uint_as_float(v);
            }
        }
        part[threadIdx.x] = acc;
        __syncthreads();
        if (threadIdx.x < ncol) {
            double v = 0.0;
            for (int k = 0; k < sub; ++k) v += part[k * ncol + threadIdx.x];
            S[threadIdx.x] = v;
        }
        __syncthreads();
        if (threadIdx.x < C) {
            const int c = threadIdx.x;
            const double Ic = S[c], Pc = S[CP + c], Tc = S[2 * CP + c];
            sums[((int64_t)r * 3 + 0) * C + c] = Ic;
            sums[((int64_t)r * 3 + 1) * C + c] = Pc;
            sums[((int64_t)r * 3 + 2) * C + c] = Tc;
            const double wc = weight ? (double)weight[c] : 1.0;
            const bool inK = !present_only || Tc > 0.0;
            double N, D, dI;
            if (kind == MRFP_REGION_DICE) { N = 2.0 * Ic + s; D = Pc + Tc + s; dI = 2.0 / D; }
            else { N = Ic + s; D = Pc + Tc - Ic + s; dI = (D + N) / (D * D); }
            term[c] = inK ? wc * (1.0 - N / D) : 0.0;
            wk[c] = inK ? wc : 0.0;
            dsi[c] = inK ? wc * dI : 0.0;
            dsp[c] = inK ? wc * (-N / (D * D)) : 0.0;
        }
        __syncthreads();
        double WK = 0.0, L = 0.0;          // every thread, the same order
        for (int c = 0; c < C; ++c) { WK += wk[c]; L += term[c]; }
        const bool counts = WK > 0.0;      // an empty K (every pixel ignored) or all-zero weights on K: loss 0, gradient 0
        if (threadIdx.x < CP) {
            const int c = threadIdx.x;
            float a = 0.f, bq = 0.f;
            if (counts && c < C) { a = (float)(-dsi[c] / WK); bq = (float)(-dsp[c] / WK); }
            coef[((int64_t)r * 2 + 0) * CP + c] = a;
            coef[((int64_t)r * 2 + 1) * CP + c] = bq;
        }
        if (threadIdx.x == 0 && counts) { total += L / WK; ++counted; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = counted ? (float)(total / (double)counted) : 0.f;
        out[1] = counted ? (float)(1.0 / (double)counted) : 0.f;
    }
}

// every row is stored: zeros for a pixel that does not count
template <typename T, int CP, typename Source>
__global__ __launch_bounds__(kCeThreads) void region_bwd_kernel(const Source src, const int64_t* __restrict__ target, int64_t ignore,
                                                                const float* __restrict__ out, const float* __restrict__ gscale,
                                                                int per_image) {
    using index_t = typename Source::index_t;
    __shared__ float sa[CP], sb[CP];
    const int b = blockIdx.y, C = src.C;
    const float* coef = out + 2 + (int64_t)(per_image ? b : 0) * 2 * CP;
    for (int c = threadIdx.x; c < CP; c += kCeThreads) { sa[c] = coef[c]; sb[c] = coef[CP + c]; }
    __syncthreads();
    const float k = (gscale ? gscale[0] : 1.f) * out[1];
    const int64_t* tb = target + (int64_t)b * src.HW;
    for (index_t p = (index_t)blockIdx.x * kCeThreads + threadIdx.x; p < src.HW; p += (index_t)gridDim.x * kCeThreads) {
        const int64_t tg = tb[p];
        float g[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) g[c] = 0.f;
        if (region_valid(tg, ignore, C)) {
            src.template load<T, CP>(b, p, g);
            const float inv = 1.f / region_exps<CP>(g, C);
            float dot = 0.f, pt = 0.f;
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                g[c] *= inv;
                dot += g[c] * sb[c];
                pt = (c == (int)tg) ? g[c] : pt;
            }
            const float at = sa[(int)tg];
            dot += at * pt;
#pragma unroll
            for (int c = 0; c < CP; ++c) g[c] = c < C ? k * g[c] * ((sb[c] + (c == (int)tg ? at : 0.f)) - dot) : 0.f;
        }
        src.template store<T, CP>(b, p, g);
    }
}

static int region_class_pad(int64_t C) { return (int)((C + 7) / 8 * 8); }

static int region_check(const char* who, int64_t B, int64_t HW, int64_t C) {
    MRFP_CHECK(C >= 1 && C <= kMaxClasses, "%s: 1 <= C <= %d (C=%lld)", who, kMaxClasses, (long long)C);
    MRFP_CHECK(B >= 1 && B <= 65535, "%s: 1 <= B <= 65535 (B=%lld)", who, (long long)B);
    MRFP_CHECK(HW > 0 && HW < (1LL << 31), "%s: bad size (HW=%lld)", who, (long long)HW);
    return 0;
}

static int region_fwd_check(const char* who, int kind, float smooth, int present_only) {
    MRFP_CHECK(kind == MRFP_REGION_DICE || kind == MRFP_REGION_JACCARD, "%s: unknown kind %d", who, kind);
    MRFP_CHECK(smooth >= 0.f && smooth <= 3.0e38f, "%s: smooth must be a finite number >= 0 (got %g)", who, (double)smooth);
    MRFP_CHECK(present_only || smooth > 0.f, "%s: present_only == 0 needs smooth > 0 (an absent class has an empty denominator)", who);
    return 0;
}

template <typename Source>
static int launch_region_fwd(const char* who, int dtype, int64_t B, const Source& src, const int64_t* target, int64_t ignore,
                             const float* weight, int kind, float smooth, int present_only, int per_image, float* ws, float* out,
                             hipStream_t st) {
    const int nbx = ce_w_blocks_x(B, src.HW);
    if (int rc = by_dtype_class_pad<kMaxClasses>(dtype, who, src.C, [&](auto t, auto cp) {
            hipLaunchKernelGGL((region_sums_kernel<typename decltype(t)::type, decltype(cp)::value, Source>), dim3(nbx, (unsigned)B),
                               dim3(kCeThreads), 0, st, src, target, ignore, ws);
        }))
        return rc;
    hipLaunchKernelGGL(region_finalize_kernel, dim3(1), dim3(kRegionFinalThreads), 0, st, ws, nbx, (int)B, src.C, region_class_pad(src.C), weight, kind,
                       smooth, present_only ? 1 : 0, per_image ? 1 : 0, out);
    MRFP_LAUNCH_CHECK();
    return 0;
}

template <typename Source>
static int launch_region_bwd(const char* who, int dtype, int64_t B, const Source& src, const int64_t* target, int64_t ignore,
                             const float* out, const float* gscale, int per_image, hipStream_t st) {
    const int nbx = ce_w_blocks_x(B, src.HW);
    return by_dtype_class_pad<kMaxClasses>(dtype, who, src.C, [&](auto t, auto cp) {
        hipLaunchKernelGGL((region_bwd_kernel<typename decltype(t)::type, decltype(cp)::value, Source>), dim3(nbx, (unsigned)B),
                           dim3(kCeThreads), 0, st, src, target, ignore, out, gscale, per_image ? 1 : 0);
    });
}

}  // namespace mrfp

extern "C" {

int64_t mrfp_region_nblocks(int64_t B, int64_t HW) { return (int64_t)mrfp::ce_w_blocks_x(B, HW) * (B > 0 ? B : 1); }

int64_t mrfp_region_ws_floats(int64_t B, int64_t HW, int64_t C) { return mrfp_region_nblocks(B, HW) * 3 * mrfp::region_class_pad(C); }

int64_t mrfp_region_out_floats(int64_t B, int64_t C, int per_image) {
    const int64_t rows = per_image ? (B > 0 ? B : 1) : 1;
    return 2 + rows * 2 * mrfp::region_class_pad(C) + 2 * rows * 3 * C;
}

int mrfp_region_fwd(const void* logits, const int64_t* target, int dtype, int64_t B, int64_t HW, int64_t C, int64_t ignore_index,
                    const float* weight, int kind, float smooth, int present_only, int per_image, float* ws, float* out, void* stream) {
    const char* who = "region_fwd";
    MRFP_CHECK(logits && target && ws && out, "%s: null pointer", who);
    MRFP_CHECK((reinterpret_cast<uintptr_t>(out) & 7) == 0, "%s: out must be 8-byte aligned", who);
    if (int rc = mrfp::region_check(who, B, HW, C)) return rc;
    if (int rc = mrfp::region_fwd_check(who, kind, smooth, present_only)) return rc;
    return mrfp::launch_region_fwd(who, dtype, B, mrfp::DenseRows{logits, nullptr, HW, (int)C}, target, ignore_index, weight, kind, smooth,
                                   present_only, per_image, ws, out, (hipStream_t)stream);
}

int mrfp_region_bwd(const void* logits, const int64_t* target, const float* out, const float* gscale, void* dlogits, int dtype,
                    int64_t B, int64_t HW, int64_t C, int64_t ignore_index, int per_image, void* stream) {
    const char* who = "region_bwd";
    MRFP_CHECK(logits && target && out && dlogits, "%s: null pointer", who);
    if (int rc = mrfp::region_check(who, B, HW, C)) return rc;
    return mrfp::launch_region_bwd(who, dtype, B, mrfp::DenseRows{logits, dlogits, HW, (int)C}, target, ignore_index, out, gscale,
                                   per_image, (hipStream_t)stream);
}

int mrfp_upsample_region_fwd(const void* P, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H,
                             int64_t W, int64_t C, int64_t ignore_index, const float* weight, int kind, float smooth, int present_only,
                             int per_image, float* ws, float* out, void* stream) {
    const char* who = "upsample_region_fwd";
    MRFP_CHECK(P && target && ws && out, "%s: null pointer", who);
    MRFP_CHECK((reinterpret_cast<uintptr_t>(out) & 7) == 0, "%s: out must be 8-byte aligned", who);
    MRFP_CHECK(H > 0 && W > 0, "%s: bad size", who);
    if (int rc = mrfp::region_check(who, B, H * W, C)) return rc;
    if (int rc = mrfp::region_fwd_check(who, kind, smooth, present_only)) return rc;
    mrfp::BilinearRows src;
    if (int rc = mrfp::bilinear_rows(who, P, ld, nullptr, 0, false, dtype, Hi, Wi, H, W, C, src)) return rc;
    return mrfp::launch_region_fwd(who, dtype, B, src, target, ignore_index, weight, kind, smooth, present_only, per_image, ws, out,
                                   (hipStream_t)stream);
}

int mrfp_upsample_region_bwd(const void* P, int64_t ld, const int64_t* target, const float* out, const float* gscale, void* dlogits,
                             int64_t Cd, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H, int64_t W, int64_t C,
                             int64_t ignore_index, int per_image, void* stream) {
    const char* who = "upsample_region_bwd";
    MRFP_CHECK(P && target && out && dlogits, "%s: null pointer", who);
    MRFP_CHECK(H > 0 && W > 0, "%s: bad size", who);
    if (int rc = mrfp::region_check(who, B, H * W, C)) return rc;
    mrfp::BilinearRows src;
    if (int rc = mrfp::bilinear_rows(who, P, ld, dlogits, Cd, false, dtype, Hi, Wi, H, W, C, src)) return rc;
    return mrfp::launch_region_bwd(who, dtype, B, src, target, ignore_index, out, gscale, per_image, (hipStream_t)stream);
}

}  // extern "C"
