// eval.hip -- test-time-augmentation accumulator of the eval path: per (scale, flip, window) variant ONE pass that resizes the
// low-resolution class scores into a rectangle of a full-size probability accumulator, and the closing arg-max + confusion
// histogram over that accumulator.  HBM-bound: the accumulator is read and written once per variant.
//
// Replaces (stock PyTorch; the reference scores single-scale only, main.py:887-913, so there is no reference call site):
//   acc[:, y0:y0+hd, x0:x0+wd] += w * softmax(F.interpolate(flip(logits), (hd, wd), mode='bilinear', align_corners=True), 1)
// -- five or six passes over a [B,NC,hd,wd] fp32 tensor -- and np.argmax + np.bincount of the averaged probabilities.
#include "common.hpp"

namespace mrfp {

constexpr int kAccThreads = 256;       // also the destination pixels of one workgroup (one lane per pixel in the compute phase)
constexpr int kAccMaxClasses = 32;

// ATen's align_corners=True rule, as resize_pool.hip / loss.hip evaluate it
__device__ __forceinline__ float acc_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// One workgroup owns one segment of <= 256 pixels of one destination row, i.e. n*NC CONSECUTIVE floats of `acc`:
//   1. every lane issues the 16-byte loads of its share of that flat range (NC = 19 is 76 bytes per pixel: a lane per pixel
//      would read and write dwords at a 76-byte stride; the flat range is walked in aligned 16-byte chunks instead, with up to
//      3 scalar floats in front and behind);
//   2. lane x computes pixel x: 4 taps x NC low-resolution values (L1 / L2 hits: the source map is (hd*wd)/(hs*ws) times
//      smaller), bilinear, max-subtracted softmax with an fp64 denominator and quotient, w*p into LDS at the pixel's place in the flat range
//      (the LDS copy starts at the range's offset inside its first 16-byte chunk, so chunk k of memory is chunk k of LDS);
//   3. after the barrier the loaded chunks get their LDS chunk added and are stored.
// CP = NC rounded up to 8 (compile time): the class vector and the CP/4 prefetched chunks live in registers.
// VSRC: the source pitch is a multiple of 16 bytes -> 16-byte source loads; otherwise scalar ones (ld = 19).
// LDS pitch = NC: conflict-free writes for odd NC (19); an even NC costs bank conflicts in phase 2, not correctness.
template <typename T, int CP, bool VSRC>
__global__ __launch_bounds__(kAccThreads) void prob_accum_kernel(const T* __restrict__ P, int ld, int hs, int ws,
                                                                 float* __restrict__ acc, float* __restrict__ cnt, int H, int W,
                                                                 int NC, int y0, int x0, int hd, int wd, int nseg, int seg,
                                                                 int flip, float wgt) {
    constexpr int KCH = CP / 4;                     // 16-byte chunks per lane: 256 * NC / 4 / 256 <= CP / 4
    __shared__ __attribute__((aligned(16))) float sm[kAccThreads * CP + 4];
    const int t = threadIdx.x;
    const int s = blockIdx.x % nseg, row = blockIdx.x / nseg;
    const int y = row % hd, b = row / hd;
    const int xs = s * seg, n = min(seg, wd - xs);                       // this workgroup's pixels: xs .. xs + n - 1 of row y
    const size_t pix0 = ((size_t)b * H + (y0 + y)) * W + (x0 + xs);     // first pixel in acc / cnt
    const size_t g0 = pix0 * NC;                                        // flat float range [g0, g0 + n*NC) of acc
    const int total = n * NC;
    const int off = (int)(g0 & 3);                                      // LDS copy starts at sm[off]
    const int head = min((4 - off) & 3, total);                         // scalar floats in front of the first aligned chunk
    const int nch = (total - head) >> 2;                                // aligned chunks
    const int tail = total - head - 4 * nch;                            // scalar floats behind the last one
    float* const ga = acc + g0 + head;                                  // 16-byte aligned (acc is)

    // ---- 1. read-modify-write operands on their way
    float4 r[KCH];
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int c = t + k * kAccThreads;
        if (c < nch) r[k] = *reinterpret_cast<const float4*>(ga + 4 * c);
    }
    float rs = 0.f, rc = 0.f;
    if (t < head) rs = acc[g0 + t];
    else if (t >= 64 && t < 64 + tail) rs = ga[4 * nch + (t - 64)];
    if (t < n) rc = cnt[pix0 + t];

    // ---- 2. one lane per pixel
    if (t < n) {
        const float sh = acc_scale(hs, hd), sw = acc_scale(ws, wd);
        const float fh = sh * (float)y, fw = sw * (float)(xs + t);
        const int h0 = (int)fh, w0 = (int)fw;
        const int h1 = h0 + (h0 < hs - 1 ? 1 : 0), w1 = w0 + (w0 < ws - 1 ? 1 : 0);
        const float lh1 = fh - (float)h0, lh0 = 1.f - lh1, lw1 = fw - (float)w0, lw0 = 1.f - lw1;
        const int c0i = flip ? ws - 1 - w0 : w0, c1i = flip ? ws - 1 - w1 : w1;      // interpolate(flip(logits)): mirrored taps
        const T* p00 = P + (((size_t)b * hs + h0) * ws + c0i) * ld;
        const T* p01 = P + (((size_t)b * hs + h0) * ws + c1i) * ld;
        const T* p10 = P + (((size_t)b * hs + h1) * ws + c0i) * ld;
        const T* p11 = P + (((size_t)b * hs + h1) * ws + c1i) * ld;
        float z[CP];
        if constexpr (VSRC) {
            constexpr int EPC = 16 / (int)sizeof(T);
#pragma unroll
            for (int c0 = 0; c0 < CP; c0 += EPC) {
                float a[EPC], bb[EPC], c[EPC], d[EPC];
#pragma unroll
                for (int i = 0; i < EPC; ++i) { a[i] = 0.f; bb[i] = 0.f; c[i] = 0.f; d[i] = 0.f; }
                if (c0 < NC) {        // chunks past the class count are never read (c0 + EPC <= ld: ld is a chunk multiple >= NC)
                    load_f<T, EPC>(p00 + c0, a);
                    load_f<T, EPC>(p01 + c0, bb);
                    load_f<T, EPC>(p10 + c0, c);
                    load_f<T, EPC>(p11 + c0, d);
                }
#pragma unroll
                for (int i = 0; i < EPC; ++i) z[c0 + i] = lh0 * (lw0 * a[i] + lw1 * bb[i]) + lh1 * (lw0 * c[i] + lw1 * d[i]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                float a = 0.f, bb = 0.f, cc = 0.f, d = 0.f;
                if (c < NC) { a = to_f(p00[c]); bb = to_f(p01[c]); cc = to_f(p10[c]); d = to_f(p11[c]); }
                z[c] = lh0 * (lw0 * a + lw1 * bb) + lh1 * (lw0 * cc + lw1 * d);
            }
        }
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < CP; ++c) if (c < NC) m = fmaxf(m, z[c]);
        double den = 0.0;            // the denominator carries no summation error of its own: p is one expf and one divide from exact
#pragma unroll
        for (int c = 0; c < CP; ++c) { z[c] = c < NC ? expf(z[c] - m) : 0.f; den += (double)z[c]; }
        // p = e / den rounded ONCE: the quotient is formed in fp64 (one reciprocal per pixel) -- rounding the denominator and then
        // the fp32 quotient as well measured 2.2 ulp from the exact softmax, this form stays inside expf's own error + 0.5 ulp
        const double rden = 1.0 / den;
        float* d = sm + off + t * NC;
#pragma unroll
        for (int c = 0; c < CP; ++c) if (c < NC) d[c] = wgt * (float)((double)z[c] * rden);
        cnt[pix0 + t] = rc + wgt;
    }
    __syncthreads();

    // ---- 3. add and store
    const float* sa = sm + off + head;          // 16-byte aligned: off + head is 0 or 4
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int c = t + k * kAccThreads;
        if (c < nch) {
            const float4 v = *reinterpret_cast<const float4*>(sa + 4 * c);
            float4 o = r[k];
            o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
            *reinterpret_cast<float4*>(ga + 4 * c) = o;
        }
    }
    if (t < head) acc[g0 + t] = rs + sm[off + t];
    else if (t >= 64 && t < 64 + tail) ga[4 * nch + (t - 64)] = rs + sa[4 * nch + (t - 64)];
}

struct AccArgs {
    const void* P; int ld, hs, ws; float* acc; float* cnt; int H, W, NC, y0, x0, hd, wd, nseg, seg, flip; float w;
    unsigned grid; hipStream_t st;
};
template <typename T, int CP, bool VSRC>
static void launch_acc(const AccArgs& a) {
    hipLaunchKernelGGL((prob_accum_kernel<T, CP, VSRC>), dim3(a.grid), dim3(kAccThreads), 0, a.st, (const T*)a.P, a.ld, a.hs, a.ws,
                       a.acc, a.cnt, a.H, a.W, a.NC, a.y0, a.x0, a.hd, a.wd, a.nseg, a.seg, a.flip, a.w);
}
template <typename T>
static void dispatch_acc(const AccArgs& a, bool vsrc) {
    switch ((a.NC + 7) / 8) {
        case 1: vsrc ? launch_acc<T, 8, true>(a) : launch_acc<T, 8, false>(a); break;
        case 2: vsrc ? launch_acc<T, 16, true>(a) : launch_acc<T, 16, false>(a); break;
        case 3: vsrc ? launch_acc<T, 24, true>(a) : launch_acc<T, 24, false>(a); break;
        default: vsrc ? launch_acc<T, 32, true>(a) : launch_acc<T, 32, false>(a); break;
    }
}

// Closing pass.  A workgroup stages 256 pixels (256*NC consecutive floats, a 16-byte multiple) in LDS with 16-byte loads, then
// lane x scans pixel x there (pitch NC: conflict-free for NC = 19).  Per-workgroup histogram in LDS, one 64-bit atomic per
// non-empty bin at the end, as argmax_hist_kernel (loss.hip).
__global__ __launch_bounds__(kAccThreads) void acc_argmax_hist_kernel(const float* __restrict__ acc, const float* __restrict__ cnt,
                                                                      const int64_t* __restrict__ target, int64_t npix, int NC,
                                                                      unsigned long long* __restrict__ hist,
                                                                      uint8_t* __restrict__ pred,
                                                                      unsigned long long* __restrict__ uncovered) {
    __shared__ __attribute__((aligned(16))) float sm[kAccThreads * kAccMaxClasses];
    __shared__ unsigned int lh[kAccMaxClasses * kAccMaxClasses];
    __shared__ unsigned int lu;
    const int t = threadIdx.x;
    for (int i = t; i < NC * NC; i += kAccThreads) lh[i] = 0;
    if (t == 0) lu = 0;
    const int64_t nblk = (npix + kAccThreads - 1) / kAccThreads;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t p0 = blk * kAccThreads;
        const int n = (int)min((int64_t)kAccThreads, npix - p0);
        const int total = n * NC, nch = total >> 2;
        const float* g = acc + p0 * NC;
        __syncthreads();                                   // the previous trip's readers are done (and lh / lu are zeroed)
        for (int c = t; c < nch; c += kAccThreads)
            *reinterpret_cast<float4*>(sm + 4 * c) = *reinterpret_cast<const float4*>(g + 4 * c);
        if (t < total - 4 * nch) sm[4 * nch + t] = g[4 * nch + t];
        __syncthreads();
        if (t < n) {
            const float* l = sm + t * NC;
            float m = l[0];
            int am = 0;
            for (int c = 1; c < NC; ++c) {
                const float v = l[c];
                if (v > m) { m = v; am = c; }              // first maximum, as np.argmax
            }
            if (pred) pred[p0 + t] = (uint8_t)am;
            if (target) {
                const int64_t tg = target[p0 + t];
                if (tg >= 0 && tg < NC) atomicAdd(&lh[(int)tg * NC + am], 1u);
            }
            if (cnt && cnt[p0 + t] == 0.f) atomicAdd(&lu, 1u);
        }
    }
    __syncthreads();
    if (target)
        for (int i = t; i < NC * NC; i += kAccThreads)
            if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
    if (uncovered && t == 0 && lu) atomicAdd(uncovered, (unsigned long long)lu);
}

}  // namespace mrfp

using namespace mrfp;

extern "C" {

int mrfp_prob_accum(const void* logits, int dtype, int64_t B, int64_t hs, int64_t ws, int64_t ld, float* acc, float* cnt,
                    int64_t H, int64_t W, int64_t NC, int64_t y0, int64_t x0, int64_t hd, int64_t wd, int flip, float weight,
                    void* stream) {
    MRFP_CHECK(logits && acc && cnt && B > 0 && hs > 0 && ws > 0 && H > 0 && W > 0 && hd > 0 && wd > 0,
               "prob_accum: bad arguments");
    MRFP_CHECK(NC > 0 && NC <= kAccMaxClasses && ld >= NC, "prob_accum: 1 <= NC <= %d and ld >= NC (NC=%lld ld=%lld)",
               kAccMaxClasses, (long long)NC, (long long)ld);
    MRFP_CHECK(y0 >= 0 && x0 >= 0 && y0 + hd <= H && x0 + wd <= W,
               "prob_accum: rectangle (%lld,%lld,%lld,%lld) leaves the %lld x %lld accumulator", (long long)y0, (long long)x0,
               (long long)hd, (long long)wd, (long long)H, (long long)W);
    MRFP_CHECK(dtype_known(dtype), "prob_accum: unknown dtype %d", dtype);
    MRFP_CHECK(aligned16(acc) && (reinterpret_cast<uintptr_t>(cnt) & 3) == 0, "prob_accum: acc must be 16-byte aligned");
    MRFP_CHECK(B < (1 << 24) && H < (1 << 24) && W < (1 << 24) && hs < (1 << 24) && ws < (1 << 24) && ld < (1 << 24),
               "prob_accum: sizes out of range");
    const int64_t nseg = (wd + kAccThreads - 1) / kAccThreads, seg = (wd + nseg - 1) / nseg;    // equal segments of <= 256 pixels
    const int64_t grid = B * hd * nseg;
    MRFP_CHECK(grid < (1LL << 31), "prob_accum: rectangle too large");
    const bool vsrc = (ld * dtype_bytes(dtype)) % 16 == 0 && aligned16(logits);
    AccArgs a{logits, (int)ld, (int)hs, (int)ws, acc, cnt, (int)H, (int)W, (int)NC, (int)y0, (int)x0, (int)hd, (int)wd, (int)nseg,
              (int)seg, flip != 0, weight, (unsigned)grid, (hipStream_t)stream};
    return by_dtype(dtype, "prob_accum", [&](auto t) {
        dispatch_acc<typename decltype(t)::type>(a, vsrc);
        MRFP_LAUNCH_CHECK();
        return 0;
    });
}

int mrfp_acc_argmax_hist(const float* acc, const float* cnt, const int64_t* target, int64_t npix, int64_t NC, int64_t* hist,
                         uint8_t* pred, int64_t* uncovered, void* stream) {
    MRFP_CHECK(acc && npix > 0 && NC > 0 && NC <= kAccMaxClasses, "acc_argmax_hist: bad arguments (NC <= %d)", kAccMaxClasses);
    MRFP_CHECK(!target || hist, "acc_argmax_hist: target given without hist");
    MRFP_CHECK(!uncovered || cnt, "acc_argmax_hist: uncovered given without cnt");
    MRFP_CHECK(aligned16(acc), "acc_argmax_hist: acc must be 16-byte aligned");
    int64_t nb = (npix + kAccThreads - 1) / kAccThreads;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(acc_argmax_hist_kernel, dim3((unsigned)nb), dim3(kAccThreads), 0, (hipStream_t)stream, acc,
                       uncovered ? cnt : nullptr, target, npix, (int)NC, (unsigned long long*)hist, pred,
                       (unsigned long long*)uncovered);
    MRFP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
