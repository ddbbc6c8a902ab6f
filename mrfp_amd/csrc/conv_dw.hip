// conv_dw.hip -- depthwise 3x3 convolution (groups == C_in == C_out) and the ReLU6 apply of the BatchNorm behind it:
// the two layer kinds of MobileNetV2's inverted residual blocks (reference network/Mobilenet.py ConvBNReLU with
// groups = hidden_dim, nn.ReLU6) that the MFMA implicit-GEMM kernels do not cover.
//
// A depthwise 3x3 has an inner product of 9 per output element: nothing for a matrix core, bound by HBM and by how often the
// input rows (halo included) come back from the caches.  Layout: NHWC with the library's channel pitch Cp (the channel count
// rounded up to a 16-byte chunk); pad channels read as zero and are written as zero.
//
// Work split (all three kernels): a workgroup of 256 threads covers CVB channel vectors x PL pixel lanes; each lane owns one
// 16-byte channel vector (8 x 16-bit or 4 x fp32) and keeps its 9 taps (x VEC channels) in registers for every pixel it
// visits.  blockIdx.x = channel chunk, blockIdx.y = (image, row strip); the lanes of a workgroup walk the strip's pixels in
// row-major order, so the 3 (stride 1) input rows a strip row needs are fetched by neighbouring lanes at the same time and
// served from L2 after the first touch.  Every reduction (statistics rows, weight-gradient slabs and their sum) runs in a
// fixed order: results are bitwise reproducible from run to run.
#include "common.hpp"

namespace mrfp {

struct DwGeom {
    int B, H, W, Cp, C, Ho, Wo, stride, dil;    // input [B,H,W,Cp], output [B,Ho,Wo,Cp], logical channels C <= Cp, padding = dil
};

constexpr int kDwCVB = 32;                      // channel vectors per workgroup at most (32 x 16 B = 512 contiguous bytes per pixel)
constexpr int kDwFwdBlocks = 2048;              // workgroups per launch the row strips aim for (8 per CU: 32 waves per CU)
constexpr int kDwWgBlocks = 1024;               // ... for the weight gradient (fewer slabs to sum afterwards)

struct DwSplit {
    int cvb, pl, nchunk;
};
__host__ __device__ inline DwSplit dw_split(int nvec) {
    DwSplit s;
    s.cvb = nvec < kDwCVB ? nvec : kDwCVB;
    s.pl = kThreads / s.cvb;
    s.nchunk = (nvec + s.cvb - 1) / s.cvb;
    return s;
}

// row strips per image: every strip the same number of rows (the last few one less), about `target` workgroups in all
inline int dw_strips(int64_t B, int64_t nchunk, int64_t rows, int target) {
    int64_t cap = target / (B * nchunk > 0 ? B * nchunk : 1);
    if (cap < 1) cap = 1;
    if (rows <= cap) return (int)rows;
    const int64_t per = (rows + cap - 1) / cap;
    return (int)((rows + per - 1) / per);
}

// taps of one channel vector: w is fp32 OIHW [C][1][3][3]; channels >= C read as zero
template <int VEC>
__device__ __forceinline__ void load_taps(const float* __restrict__ w, int c0, int C, float (&tap)[9][VEC]) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        const bool ok = c0 + i < C;
#pragma unroll
        for (int k = 0; k < 9; ++k) tap[k][i] = ok ? w[(size_t)(c0 + i) * 9 + k] : 0.f;
    }
}

template <typename T, int VEC>
__device__ __forceinline__ void load_or_zero(const T* p, bool ok, float (&v)[VEC]) {
    if (ok) {
        load_f<T, VEC>(p, v);
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = 0.f;
    }
}

// Sum over the PL pixel lanes of a workgroup, in lane order, of one float per (channel vector, element): red holds
// kThreads * VEC floats; lane (pl, cvl) stored its VEC values at red[(pl * cvb + cvl) * VEC ...].  Threads t < cvb * VEC
// return the sum for channel element t of the chunk; the others return 0.
template <int VEC>
__device__ __forceinline__ float lane_sum(float* red, const float (&v)[VEC], int t, int cvb, int pl) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) red[t * VEC + i] = v[i];
    __syncthreads();
    float s = 0.f;
    if (t < cvb * VEC) {
        const int cvl = t / VEC, i = t % VEC;
        for (int p = 0; p < pl; ++p) s += red[(p * cvb + cvl) * VEC + i];
    }
    __syncthreads();
    return s;
}

// y = dwconv(x, w) (+ bias); ws (STATS): float [B][nslab][2][Cp], the per-strip sums and sums of squares of the STORED y
// ACT (compile time: 0 none, 1 ReLU, 2 ReLU6 -- conv_common.hpp act_f): the folded inference form y = act(dwconv(x, w) + bias)
template <typename T, int VEC, bool STATS, int ACT = 0>
__global__ __launch_bounds__(kThreads) void dw_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, T* __restrict__ y, DwGeom g, int nslab,
                                                          float* __restrict__ ws) {
    __shared__ float red[STATS ? kThreads * VEC : 1];
    const int nvec = g.Cp / VEC;
    const DwSplit sp = dw_split(nvec);
    const int t = threadIdx.x, cvl = t % sp.cvb, pl = t / sp.cvb;
    const int cv = blockIdx.x * sp.cvb + cvl;
    const bool active = pl < sp.pl && cv < nvec;
    const int b = blockIdx.y / nslab, s = blockIdx.y % nslab;
    const int per = (g.Ho + nslab - 1) / nslab;
    const int r0 = s * per, r1 = min(g.Ho, r0 + per);
    float sum[VEC], sq[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) { sum[i] = 0.f; sq[i] = 0.f; }
    if (active) {
        const int c0 = cv * VEC;
        float tap[9][VEC], b0[VEC];
        load_taps<VEC>(w, c0, g.C, tap);
#pragma unroll
        for (int i = 0; i < VEC; ++i) b0[i] = (bias && c0 + i < g.C) ? bias[c0 + i] : 0.f;
        const T* xb = x + (size_t)b * g.H * g.W * g.Cp + c0;
        const int n = (r1 - r0) * g.Wo;
        for (int p = pl; p < n; p += sp.pl) {
            const int oh = r0 + p / g.Wo, ow = p % g.Wo;
            float acc[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = b0[i];
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int ih = oh * g.stride - g.dil + kh * g.dil;
                const bool hok = ih >= 0 && ih < g.H;
                float xv[3][VEC];
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int iw = ow * g.stride - g.dil + kw * g.dil;
                    const bool ok = hok && iw >= 0 && iw < g.W;
                    load_or_zero<T, VEC>(xb + ((size_t)ih * g.W + iw) * g.Cp, ok, xv[kw]);
                }
#pragma unroll
                for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc[i] += xv[kw][i] * tap[kh * 3 + kw][i];
            }
            if constexpr (ACT != 0) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] = act_f<ACT>(acc[i]);
            }
            store_f<T, VEC>(y + (((size_t)b * g.Ho + oh) * g.Wo + ow) * g.Cp + c0, acc);
            if constexpr (STATS) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const float v = to_f(from_f<T>(acc[i]));     // the statistics of the stored (rounded) output
                    sum[i] += v;
                    sq[i] += v * v;
                }
            }
        }
    }
    if constexpr (STATS) {
        const float s0 = lane_sum<VEC>(red, sum, t, sp.cvb, sp.pl);
        const float s1 = lane_sum<VEC>(red, sq, t, sp.cvb, sp.pl);
        const int c = blockIdx.x * sp.cvb * VEC + t;
        if (t < sp.cvb * VEC && c < g.Cp) {
            float* row = ws + ((size_t)b * nslab + s) * 2 * g.Cp;
            row[c] = s0;
            row[g.Cp + c] = s1;
        }
    }
}

// dx = dwconv^T(dy, w) in gather form: each dx pixel collects the (up to 9) output taps that read it; no atomics
template <typename T, int VEC>
__global__ __launch_bounds__(kThreads) void dw_dgrad_kernel(const T* __restrict__ dy, const float* __restrict__ w, T* __restrict__ dx,
                                                            DwGeom g, int nslab) {
    const int nvec = g.Cp / VEC;
    const DwSplit sp = dw_split(nvec);
    const int t = threadIdx.x, cvl = t % sp.cvb, pl = t / sp.cvb;
    const int cv = blockIdx.x * sp.cvb + cvl;
    if (pl >= sp.pl || cv >= nvec) return;
    const int b = blockIdx.y / nslab, s = blockIdx.y % nslab;
    const int per = (g.H + nslab - 1) / nslab;
    const int r0 = s * per, r1 = min(g.H, r0 + per);
    const int c0 = cv * VEC;
    float tap[9][VEC];
    load_taps<VEC>(w, c0, g.C, tap);
    const T* db = dy + (size_t)b * g.Ho * g.Wo * g.Cp + c0;
    const int n = (r1 - r0) * g.W;
    for (int p = pl; p < n; p += sp.pl) {
        const int ih = r0 + p / g.W, iw = p % g.W;
        float acc[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int th = ih + g.dil - kh * g.dil;            // = oh * stride
            const int oh = th / g.stride;
            const bool hok = th >= 0 && oh * g.stride == th && oh < g.Ho;
            float dv[3][VEC];
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int tw = iw + g.dil - kw * g.dil;
                const int ow = tw / g.stride;
                const bool ok = hok && tw >= 0 && ow * g.stride == tw && ow < g.Wo;
                load_or_zero<T, VEC>(db + ((size_t)oh * g.Wo + ow) * g.Cp, ok, dv[kw]);
            }
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] += dv[kw][i] * tap[kh * 3 + kw][i];
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = c0 + i < g.C ? acc[i] : 0.f;     // pad channels: zero whatever dy holds there
        store_f<T, VEC>(dx + (((size_t)b * g.H + ih) * g.W + iw) * g.Cp + c0, acc);
    }
}

// weight-gradient slabs: slab[b * nslab + s][k][Cp] = sum over the strip's output pixels of dy * x(tap k), per channel;
// per-lane partials in registers, combined across the workgroup's lanes through LDS in lane order
template <typename T, int VEC>
__global__ __launch_bounds__(kThreads) void dw_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ slab,
                                                            DwGeom g, int nslab) {
    __shared__ float red[kThreads * VEC];
    const int nvec = g.Cp / VEC;
    const DwSplit sp = dw_split(nvec);
    const int t = threadIdx.x, cvl = t % sp.cvb, pl = t / sp.cvb;
    const int cv = blockIdx.x * sp.cvb + cvl;
    const bool active = pl < sp.pl && cv < nvec;
    const int b = blockIdx.y / nslab, s = blockIdx.y % nslab;
    const int per = (g.Ho + nslab - 1) / nslab;
    const int r0 = s * per, r1 = min(g.Ho, r0 + per);
    float acc[9][VEC];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[k][i] = 0.f;
    if (active) {
        const int c0 = cv * VEC;
        const T* xb = x + (size_t)b * g.H * g.W * g.Cp + c0;
        const T* db = dy + (size_t)b * g.Ho * g.Wo * g.Cp + c0;
        const int n = (r1 - r0) * g.Wo;
        for (int p = pl; p < n; p += sp.pl) {
            const int oh = r0 + p / g.Wo, ow = p % g.Wo;
            float d[VEC];
            load_f<T, VEC>(db + ((size_t)oh * g.Wo + ow) * g.Cp, d);
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int ih = oh * g.stride - g.dil + kh * g.dil;
                const bool hok = ih >= 0 && ih < g.H;
                float xv[3][VEC];
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int iw = ow * g.stride - g.dil + kw * g.dil;
                    load_or_zero<T, VEC>(xb + ((size_t)ih * g.W + iw) * g.Cp, hok && iw >= 0 && iw < g.W, xv[kw]);
                }
#pragma unroll
                for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc[kh * 3 + kw][i] += d[i] * xv[kw][i];
            }
        }
    }
    const int c = blockIdx.x * sp.cvb * VEC + t;
    float* out = slab + ((size_t)b * nslab + s) * 9 * g.Cp;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float v = lane_sum<VEC>(red, acc[k], t, sp.cvb, sp.pl);
        if (t < sp.cvb * VEC && c < g.Cp) out[(size_t)k * g.Cp + c] = v;
    }
}

// dw[c][k] = sum over the nrows slabs, in slab order, split over 8 lane groups (group j takes slabs j, j+8, ...) whose partials
// are added in group order: a fixed order for a given launch geometry
constexpr int kDwRedOut = 32, kDwRedGroups = kThreads / kDwRedOut;
__global__ __launch_bounds__(kThreads) void dw_wgrad_reduce_kernel(const float* __restrict__ slab, int nrows, int Cp, int C,
                                                                   float* __restrict__ dw) {
    __shared__ float part[kDwRedGroups][kDwRedOut];
    const int o = threadIdx.x % kDwRedOut, gr = threadIdx.x / kDwRedOut;
    const int64_t q = (int64_t)blockIdx.x * kDwRedOut + o;          // q = k * C + c
    const int64_t nq = (int64_t)9 * C;
    float acc = 0.f;
    if (q < nq) {
        const int k = (int)(q / C), c = (int)(q % C);
        const float* base = slab + (size_t)k * Cp + c;
        const size_t rs = (size_t)9 * Cp;
        int r = gr;
        for (; r + 3 * kDwRedGroups < nrows; r += 4 * kDwRedGroups) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = base[(size_t)(r + u * kDwRedGroups) * rs];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc += v[u];
        }
        for (; r < nrows; r += kDwRedGroups) acc += base[(size_t)r * rs];
    }
    part[gr][o] = acc;
    __syncthreads();
    if (gr == 0 && q < nq) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < kDwRedGroups; ++j) s += part[j][o];
        const int k = (int)(q / C), c = (int)(q % C);
        dw[(size_t)c * 9 + k] = s;
    }
}

// ---- ReLU6 apply of a BatchNorm ----------------------------------------------------------------------------------------
// y = clamp(x*A[c] + S[c], 0, 6) over the dense [npix][C] tensor, and the pass mask of the PRE-activation (bit e & 7 of byte e >> 3
// = 0 < x*A + S < 6, torch's hardtanh gate), in the format mrfp_affine_fwd_relu_mask writes.  One thread per mask byte.
template <typename T>
__global__ __launch_bounds__(kThreads) void relu6_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ mask,
                                                             int64_t n, int C, const float* __restrict__ A, const float* __restrict__ S) {
    const int64_t nbytes = (n + 7) >> 3;
    for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < nbytes; j += (int64_t)gridDim.x * kThreads) {
        const int64_t e0 = j << 3;
        unsigned m = 0;
        if (e0 + 8 <= n && C % 8 == 0) {                 // 8 elements of one channel chunk: 16-byte (2 x 16-byte for fp32) accesses
            float v[8];
            const int c0 = (int)(e0 % C);
            if constexpr (sizeof(T) == 2) {
                load_f<T, 8>(x + e0, v);
            } else {
                float lo[4], hi[4];
                load_f<T, 4>(x + e0, lo);
                load_f<T, 4>(x + e0 + 4, hi);
#pragma unroll
                for (int i = 0; i < 4; ++i) { v[i] = lo[i]; v[4 + i] = hi[i]; }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float pre = v[i] * A[c0 + i] + S[c0 + i];
                m |= (pre > 0.f && pre < 6.f ? 1u : 0u) << i;
                v[i] = fminf(fmaxf(pre, 0.f), 6.f);
            }
            if constexpr (sizeof(T) == 2) {
                store_f<T, 8>(y + e0, v);
            } else {
                float lo[4], hi[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { lo[i] = v[i]; hi[i] = v[4 + i]; }
                store_f<T, 4>(y + e0, lo);
                store_f<T, 4>(y + e0 + 4, hi);
            }
        } else {
            for (int i = 0; i < 8 && e0 + i < n; ++i) {
                const int c = (int)((e0 + i) % C);
                const float pre = to_f(x[e0 + i]) * A[c] + S[c];
                m |= (pre > 0.f && pre < 6.f ? 1u : 0u) << i;
                y[e0 + i] = from_f<T>(fminf(fmaxf(pre, 0.f), 6.f));
            }
        }
        mask[j] = (uint8_t)m;
    }
}

// out = dy * bit(e) over n elements: the gated gradient where the masked statistics / apply kernels do not apply (fp32)
template <typename T>
__global__ __launch_bounds__(kThreads) void mask_gate_kernel(const T* __restrict__ dy, const uint8_t* __restrict__ mask, T* __restrict__ out,
                                                             int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads)
        out[e] = ((mask[e >> 3] >> (e & 7)) & 1u) ? dy[e] : from_f<T>(0.f);
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
static bool dw_geom(int dtype, int64_t B, int64_t H, int64_t W, int64_t Cp, int64_t C, int64_t Ho, int64_t Wo, int64_t stride,
                    int64_t dil, DwGeom& g) {
    if (!dtype_known(dtype)) { set_error("dwconv: unsupported dtype %d", dtype); return false; }
    const int vec = 16 / dtype_bytes(dtype);
    if (B < 1 || H < 1 || W < 1 || C < 1 || Cp < C || Cp % vec != 0 || stride < 1 || stride > 2 || dil < 1) {
        set_error("dwconv: bad geometry B=%lld H=%lld W=%lld C=%lld Cp=%lld stride=%lld dil=%lld", (long long)B, (long long)H,
                  (long long)W, (long long)C, (long long)Cp, (long long)stride, (long long)dil);
        return false;
    }
    // 3x3, padding = dilation: Ho = (H + 2d - 2d - 1) / stride + 1
    if (Ho != (H - 1) / stride + 1 || Wo != (W - 1) / stride + 1) {
        set_error("dwconv: output %lldx%lld does not match input %lldx%lld at stride %lld", (long long)Ho, (long long)Wo, (long long)H,
                  (long long)W, (long long)stride);
        return false;
    }
    if (B * H * W * Cp >= ((int64_t)1 << 31) || B * Ho * Wo * Cp >= ((int64_t)1 << 31)) { set_error("dwconv: tensor too large"); return false; }
    g = DwGeom{(int)B, (int)H, (int)W, (int)Cp, (int)C, (int)Ho, (int)Wo, (int)stride, (int)dil};
    return true;
}

static int dw_nchunk(int dtype, int64_t Cp) { return dw_split((int)(Cp / (16 / dtype_bytes(dtype)))).nchunk; }

template <typename T>
static int launch_dw_fwd(const void* x, const float* w, const float* bias, void* y, const DwGeom& g, float* ws, hipStream_t st) {
    constexpr int VEC = FullVec<T>::value;
    const int nchunk = dw_split(g.Cp / VEC).nchunk;
    const int nslab = dw_strips(g.B, nchunk, g.Ho, kDwFwdBlocks);
    dim3 grid((unsigned)nchunk, (unsigned)(g.B * nslab));
    if (ws)
        hipLaunchKernelGGL((dw_fwd_kernel<T, VEC, true>), grid, dim3(kThreads), 0, st, (const T*)x, w, bias, (T*)y, g, nslab, ws);
    else
        hipLaunchKernelGGL((dw_fwd_kernel<T, VEC, false>), grid, dim3(kThreads), 0, st, (const T*)x, w, bias, (T*)y, g, nslab, ws);
    MRFP_LAUNCH_CHECK();
    return 0;
}

template <typename T, int ACT>
static int launch_dw_fwd_act(const void* x, const float* w, const float* bias, void* y, const DwGeom& g, hipStream_t st) {
    constexpr int VEC = FullVec<T>::value;
    const int nchunk = dw_split(g.Cp / VEC).nchunk;
    const int nslab = dw_strips(g.B, nchunk, g.Ho, kDwFwdBlocks);      // (the grid of the plain forward launch)
    hipLaunchKernelGGL((dw_fwd_kernel<T, VEC, false, ACT>), dim3((unsigned)nchunk, (unsigned)(g.B * nslab)), dim3(kThreads), 0, st,
                       (const T*)x, w, bias, (T*)y, g, nslab, (float*)nullptr);
    MRFP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
static int launch_dw_dgrad(const void* dy, const float* w, void* dx, const DwGeom& g, hipStream_t st) {
    constexpr int VEC = FullVec<T>::value;
    const int nchunk = dw_split(g.Cp / VEC).nchunk;
    const int nslab = dw_strips(g.B, nchunk, g.H, kDwFwdBlocks);
    hipLaunchKernelGGL((dw_dgrad_kernel<T, VEC>), dim3((unsigned)nchunk, (unsigned)(g.B * nslab)), dim3(kThreads), 0, st, (const T*)dy,
                       w, (T*)dx, g, nslab);
    MRFP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
static int launch_dw_wgrad(const void* x, const void* dy, float* dw, float* slab, const DwGeom& g, hipStream_t st) {
    constexpr int VEC = FullVec<T>::value;
    const int nchunk = dw_split(g.Cp / VEC).nchunk;
    const int nslab = dw_strips(g.B, nchunk, g.Ho, kDwWgBlocks);
    hipLaunchKernelGGL((dw_wgrad_kernel<T, VEC>), dim3((unsigned)nchunk, (unsigned)(g.B * nslab)), dim3(kThreads), 0, st, (const T*)x,
                       (const T*)dy, slab, g, nslab);
    MRFP_LAUNCH_CHECK();
    const int64_t nq = (int64_t)9 * g.C;
    hipLaunchKernelGGL(dw_wgrad_reduce_kernel, dim3((unsigned)((nq + kDwRedOut - 1) / kDwRedOut)), dim3(kThreads), 0, st,
                       (const float*)slab, g.B * nslab, g.Cp, g.C, dw);
    MRFP_LAUNCH_CHECK();
    return 0;
}

static unsigned elem_blocks(int64_t items) {
    int64_t blocks = (items + kThreads - 1) / kThreads;
    if (blocks > 8192) blocks = 8192;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

}  // namespace mrfp

using namespace mrfp;

extern "C" {

int64_t mrfp_dwconv_nslab(int dtype, int64_t B, int64_t Ho, int64_t Cp) {
    if (B < 1 || Ho < 1 || Cp < 1) return 0;
    return dw_strips(B, dw_nchunk(dtype, Cp), Ho, kDwFwdBlocks);
}

int64_t mrfp_dwconv_wgrad_ws_bytes(int dtype, int64_t B, int64_t Ho, int64_t Cp) {
    if (B < 1 || Ho < 1 || Cp < 1) return 0;
    return (int64_t)B * dw_strips(B, dw_nchunk(dtype, Cp), Ho, kDwWgBlocks) * 9 * Cp * (int64_t)sizeof(float);
}

int mrfp_dwconv_fwd(const void* x, const float* w, const float* bias, void* y, int dtype, int64_t B, int64_t H, int64_t W, int64_t Cp,
                    int64_t C, int64_t Ho, int64_t Wo, int64_t stride, int64_t dil, float* ws, void* stream) {
    MRFP_CHECK(x && w && y, "dwconv_fwd: null pointer");
    MRFP_CHECK(aligned16(x) && aligned16(y) && (!ws || aligned16(ws)), "dwconv_fwd: tensors must be 16-byte aligned");
    DwGeom g;
    if (!dw_geom(dtype, B, H, W, Cp, C, Ho, Wo, stride, dil, g)) return -1;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, "dwconv", [&](auto t) {      // (dw_geom has refused an unknown dtype)
        using T = typename decltype(t)::type;
        return launch_dw_fwd<T>(x, w, bias, y, g, ws, st);
    });
}

int mrfp_dwconv_fwd_act(const void* x, const float* w, const float* bias, void* y, int dtype, int64_t B, int64_t H, int64_t W, int64_t Cp,
                        int64_t C, int64_t Ho, int64_t Wo, int64_t stride, int64_t dil, int act, void* stream) {
    MRFP_CHECK(act >= 0 && act <= 2, "dwconv_fwd_act: act must be 0 (none), 1 (ReLU) or 2 (ReLU6), got %d", act);
    if (act == 0) return mrfp_dwconv_fwd(x, w, bias, y, dtype, B, H, W, Cp, C, Ho, Wo, stride, dil, nullptr, stream);
    MRFP_CHECK(x && w && y, "dwconv_fwd_act: null pointer");
    MRFP_CHECK(aligned16(x) && aligned16(y), "dwconv_fwd_act: tensors must be 16-byte aligned");
    DwGeom g;
    if (!dw_geom(dtype, B, H, W, Cp, C, Ho, Wo, stride, dil, g)) return -1;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, "dwconv", [&](auto t) {      // (dw_geom has refused an unknown dtype)
        using T = typename decltype(t)::type;
        return act == 1 ? launch_dw_fwd_act<T, 1>(x, w, bias, y, g, st) : launch_dw_fwd_act<T, 2>(x, w, bias, y, g, st);
    });
}

int mrfp_dwconv_dgrad(const void* dy, const float* w, void* dx, int dtype, int64_t B, int64_t H, int64_t W, int64_t Cp, int64_t C,
                      int64_t Ho, int64_t Wo, int64_t stride, int64_t dil, void* stream) {
    MRFP_CHECK(dy && w && dx, "dwconv_dgrad: null pointer");
    MRFP_CHECK(aligned16(dy) && aligned16(dx), "dwconv_dgrad: tensors must be 16-byte aligned");
    DwGeom g;
    if (!dw_geom(dtype, B, H, W, Cp, C, Ho, Wo, stride, dil, g)) return -1;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, "dwconv", [&](auto t) {      // (dw_geom has refused an unknown dtype)
        using T = typename decltype(t)::type;
        return launch_dw_dgrad<T>(dy, w, dx, g, st);
    });
}

int mrfp_dwconv_wgrad(const void* x, const void* dy, float* dw, void* ws, int dtype, int64_t B, int64_t H, int64_t W, int64_t Cp,
                      int64_t C, int64_t Ho, int64_t Wo, int64_t stride, int64_t dil, void* stream) {
    MRFP_CHECK(x && dy && dw && ws, "dwconv_wgrad: null pointer");
    MRFP_CHECK(aligned16(x) && aligned16(dy) && aligned16(ws), "dwconv_wgrad: tensors must be 16-byte aligned");
    DwGeom g;
    if (!dw_geom(dtype, B, H, W, Cp, C, Ho, Wo, stride, dil, g)) return -1;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, "dwconv", [&](auto t) {      // (dw_geom has refused an unknown dtype)
        using T = typename decltype(t)::type;
        return launch_dw_wgrad<T>(x, dy, dw, (float*)ws, g, st);
    });
}

int mrfp_affine_fwd_relu6_mask(const void* x, void* y, void* mask, int dtype, int64_t npix, int64_t C, const float* A, const float* S,
                               void* stream) {
    MRFP_CHECK(x && y && mask && A && S && npix > 0 && C > 0, "affine_fwd_relu6_mask: bad arguments");
    MRFP_CHECK(aligned16(x) && aligned16(y), "affine_fwd_relu6_mask: tensors must be 16-byte aligned");
    MRFP_CHECK(dtype_known(dtype), "affine_fwd_relu6_mask: unsupported dtype %d", dtype);
    const int64_t n = npix * C;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = elem_blocks((n + 7) / 8);
    return by_dtype(dtype, "affine_fwd_relu6_mask", [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(relu6_fwd_kernel<T>, dim3(blocks), dim3(kThreads), 0, st, (const T*)x, (T*)y, (uint8_t*)mask, n, (int)C, A, S);
        MRFP_LAUNCH_CHECK();
        return 0;
    });
}

int mrfp_mask_gate(const void* dy, const void* mask, void* out, int dtype, int64_t n, void* stream) {
    MRFP_CHECK(dy && mask && out && n > 0, "mask_gate: bad arguments");
    MRFP_CHECK(dtype_known(dtype), "mask_gate: unsupported dtype %d", dtype);
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = elem_blocks(n);
    return by_dtype(dtype, "mask_gate", [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(mask_gate_kernel<T>, dim3(blocks), dim3(kThreads), 0, st, (const T*)dy, (const uint8_t*)mask, (T*)out, n);
        MRFP_LAUNCH_CHECK();
        return 0;
    });
}

}  // extern "C"
