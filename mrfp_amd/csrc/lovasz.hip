// lovasz.hip -- the Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018; include/mrfp_hip.h: mrfp_lovasz_*, mrfp_upsample_lovasz_*;
// DESIGN.md section 8): the convex surrogate of the Jaccard index, the criterion a caller reaches for when mIoU is the metric.
//
// The gradient of a pixel depends on the RANK of its error among all pixels of the scope, so this is no criterion of the pixel-loop
// skeleton: it needs a device-wide stable sort (sort.hip) and an integer scan.  Classes are processed in groups of kLovaszGroup; per
// group, on the skeleton's sources (DenseRows, BilinearRows) and grid:
//   lovasz_keys_kernel    (nbx, B) grid: soft-max of the pixel, then per class of the group the key 0x3F800000 - bits(e) (e in [0, 1], so
//                         an ascending sort is e descending and 30 key bits take part; an ignored pixel gets kLovaszIgnored, behind every
//                         valid one) and the payload 2 * flat pixel index + foreground bit; segment (class j of the group, scope r) is
//                         items [j * N + r * L, + L) of the group's buffers.  Workgroup (0, 0) also writes the segment offsets.
//   mrfp_sort_pairs       30 bits, in place: four passes of three launches
//   lovasz_count_kernel   per tile of kLovaszTile sorted items: the number of foreground bits
//   lovasz_scan_kernel    one workgroup per segment: the exclusive scan of the tile counts, in place; the segment total is G
//   lovasz_coef_kernel    per tile: F_i from the tile's scanned count and an in-tile scan (which completes the scan: its third launch),
//                         B_i = rank - F_i, g_i in closed form, e_i * g_i into ONE fp32 partial per tile, (1 - 2 f_i) g_i scattered
//                         through the payload into the class-major coefficient plane [C][N]
// and at the end lovasz_finalize_kernel, one workgroup: the tile partials of every (scope, class) in double in a fixed order, class
// presence, the scopes that count, the loss and the per-scope per-class factor table the backward reads.  No floating-point atomics,
// no workgroup waits for another, nothing waits for the host (an absent class costs its launches and a zero factor): two runs are
// bit-identical and the whole forward + backward can be captured in a graph.
//
// g without cancellation: with U = G + B_i the union before pixel i and I = G - F_i the intersection left,
//   f_i = 1:  J_i - J_i^- = 1 / U          f_i = 0:  J_i - J_i^- = I / (U (U + 1))          (first pixel of an absent class: 1)
// which is the published difference of consecutive Jaccard losses, never computed as a difference of two numbers near 1.
#include "loss_common.hpp"

namespace mrfp {

constexpr int kLovaszGroup = 4;                              // classes per group: the sort workspace is 16 B * kLovaszGroup per pixel
constexpr int kLovaszThreads = 256;
constexpr int kLovaszItems = 8;
constexpr int kLovaszTile = kLovaszThreads * kLovaszItems;   // sorted items per workgroup trip of the count and coefficient kernels
constexpr unsigned int kLovaszOne = 0x3F800000u;             // bits(1.0f)
constexpr unsigned int kLovaszIgnored = 0x3FFFFFFFu;         // the largest 30-bit key
constexpr int kLovaszKeyBits = 30;
constexpr float kLovaszSentinel = 2.f;                       // mrfp_lovasz_errors at an invalid pixel
constexpr int kLovaszFinalThreads = 1024;
constexpr int kLovaszMaxGrid = 2048;

__device__ __forceinline__ bool lovasz_valid(int64_t tg, int64_t ignore, int C) { return !(tg == ignore || tg < 0 || tg >= C); }

// z -> p = softmax(z) for c < C (0 beyond), never above 1: the one place the probabilities of the keys pass, of mrfp_lovasz_errors
// and of the backward come from
template <int CP>
__device__ __forceinline__ void lovasz_probs(float (&z)[CP], int C) {
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < CP; ++c) if (c < C) m = fmaxf(m, z[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) { z[c] = c < C ? __expf(z[c] - m) : 0.f; s += z[c]; }
    const float inv = 1.f / s;
#pragma unroll
    for (int c = 0; c < CP; ++c) z[c] = fminf(z[c] * inv, 1.f);
}

__device__ __forceinline__ float lovasz_error(float p, bool fg) { return fg ? 1.f - p : p; }        // |f - p|, p in [0, 1]

// the geometry every kernel of a forward shares
struct LovaszGeom {
    int64_t N, L;          // pixels of the batch; of a scope
    int R, tps;            // scopes; tiles per segment
    int C;
};

template <typename T, int CP, typename Source>
__global__ __launch_bounds__(kCeThreads) void lovasz_keys_kernel(const Source src, const int64_t* __restrict__ target, int64_t ignore,
                                                                 int c0, int ncls, const LovaszGeom geo, unsigned int* __restrict__ keys,
                                                                 unsigned int* __restrict__ pay, int64_t* __restrict__ offsets) {
    using index_t = typename Source::index_t;
    const int b = blockIdx.y, C = src.C;
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int s = threadIdx.x; s <= ncls * geo.R; s += kCeThreads) {
            const int j = s / geo.R, r = s - j * geo.R;
            offsets[s] = (int64_t)j * geo.N + (int64_t)r * geo.L;
        }
    const int64_t* tb = target + (int64_t)b * src.HW;
    for (index_t p = (index_t)blockIdx.x * kCeThreads + threadIdx.x; p < src.HW; p += (index_t)gridDim.x * kCeThreads) {
        const int64_t tg = tb[p];
        const int64_t i = (int64_t)b * src.HW + p;
        const bool valid = lovasz_valid(tg, ignore, C);
        float z[CP];
        if (valid) {
            src.template load<T, CP>(b, p, z);
            lovasz_probs<CP>(z, C);
        }
#pragma unroll
        for (int j = 0; j < kLovaszGroup; ++j) {
            if (j < ncls) {
                float pc = 0.f;
                if (valid) {
#pragma unroll
                    for (int c = 0; c < CP; ++c) pc = (c == c0 + j) ? z[c] : pc;       // predicated: a run-time index would put z in scratch memory
                }
                const bool fg = valid && (int)tg == c0 + j;
                const unsigned int k = valid ? kLovaszOne - __float_as_uint(lovasz_error(pc, fg)) : kLovaszIgnored;
                keys[(int64_t)j * geo.N + i] = k;
                pay[(int64_t)j * geo.N + i] = ((unsigned int)i << 1) | (fg ? 1u : 0u);
            }
        }
    }
}

// tile t (of nseg * tps) -> its segment and item range
__device__ __forceinline__ void lovasz_tile(const LovaszGeom& geo, int64_t t, int& seg, int64_t& seg_begin, int64_t& begin, int64_t& end) {
    seg = (int)(t / geo.tps);
    const int lt = (int)(t - (int64_t)seg * geo.tps), j = seg / geo.R, r = seg - j * geo.R;
    seg_begin = (int64_t)j * geo.N + (int64_t)r * geo.L;
    begin = seg_begin + (int64_t)lt * kLovaszTile;
    const int64_t seg_end = seg_begin + geo.L;
    end = begin + kLovaszTile < seg_end ? begin + kLovaszTile : seg_end;
}

// the sum of one value per thread over the workgroup, on every thread, in a fixed order; and the sum over the threads before this one
__device__ __forceinline__ unsigned int lovasz_block_scan(unsigned int v, unsigned int& total) {
    __shared__ unsigned int wsum[kLovaszThreads / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kLovaszThreads / 64; ++i) {
        const unsigned int t = wsum[i];
        before += i < w ? t : 0u;
        all += t;
    }
    __syncthreads();
    total = all;
    return before + inc - v;
}

// thread k of a tile owns its items k * kLovaszItems ... in order
__global__ __launch_bounds__(kLovaszThreads) void lovasz_count_kernel(const unsigned int* __restrict__ pay, const LovaszGeom geo, int64_t ntiles,
                                                                      unsigned int* __restrict__ tilecnt) {
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int seg;
        int64_t sb, b, e;
        lovasz_tile(geo, t, seg, sb, b, e);
        unsigned int n = 0;
#pragma unroll
        for (int u = 0; u < kLovaszItems; ++u) {
            const int64_t i = b + (int64_t)threadIdx.x * kLovaszItems + u;
            if (i < e) n += pay[i] & 1u;
        }
        unsigned int total;
        lovasz_block_scan(n, total);
        if (threadIdx.x == 0) tilecnt[t] = total;
    }
}

// one workgroup per segment (the grid is capped and walks them): tile counts -> exclusive prefix, in place; the total is G
__global__ __launch_bounds__(kLovaszThreads) void lovasz_scan_kernel(const LovaszGeom geo, int nseg, int c0, unsigned int* __restrict__ tilecnt,
                                                                     unsigned int* __restrict__ gtot) {
    for (int s = blockIdx.x; s < nseg; s += gridDim.x) {
        unsigned int* row = tilecnt + (int64_t)s * geo.tps;
        unsigned int carry = 0u;
        for (int base = 0; base < geo.tps; base += kLovaszThreads) {
            const int t = base + threadIdx.x;
            const unsigned int v = t < geo.tps ? row[t] : 0u;
            unsigned int total;
            const unsigned int ex = lovasz_block_scan(v, total);
            if (t < geo.tps) row[t] = carry + ex;
            carry += total;
        }
        const int j = s / geo.R, r = s - j * geo.R;
        if (threadIdx.x == 0) gtot[(int64_t)(c0 + j) * geo.R + r] = carry;
    }
}

__global__ __launch_bounds__(kLovaszThreads) void lovasz_coef_kernel(const unsigned int* __restrict__ keys, const unsigned int* __restrict__ pay,
                                                                     const LovaszGeom geo, int64_t ntiles, int c0,
                                                                     const unsigned int* __restrict__ tilecnt,
                                                                     const unsigned int* __restrict__ gtot, float* __restrict__ partial,
                                                                     float* __restrict__ coef) {
    __shared__ float sm[kLovaszThreads / 64];
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int seg;
        int64_t sb, b, e;
        lovasz_tile(geo, t, seg, sb, b, e);
        const int j = seg / geo.R, r = seg - j * geo.R, c = c0 + j;
        const unsigned int G = gtot[(int64_t)c * geo.R + r];
        unsigned int k[kLovaszItems], q[kLovaszItems];
        unsigned int n = 0;
#pragma unroll
        for (int u = 0; u < kLovaszItems; ++u) {
            const int64_t i = b + (int64_t)threadIdx.x * kLovaszItems + u;
            k[u] = i < e ? keys[i] : kLovaszIgnored;
            q[u] = i < e ? pay[i] : 0u;
            n += q[u] & 1u;
        }
        unsigned int total;
        unsigned int F = tilecnt[t] + lovasz_block_scan(n, total);          // foreground pixels before this thread's first item
        float acc = 0.f;
#pragma unroll
        for (int u = 0; u < kLovaszItems; ++u) {
            const unsigned int f = q[u] & 1u;
            if (k[u] != kLovaszIgnored) {                                    // ignored pixels are behind every valid one: they count nowhere
                const int64_t rank = b + (int64_t)threadIdx.x * kLovaszItems + u - sb;
                const double U = (double)G + (double)(rank - F);             // G + B_i
                double g;
                if (f) g = 1.0 / U;                                          // G >= 1 here
                else if (G == 0u) g = rank == 0 ? 1.0 : 0.0;
                else g = (double)(G - F) / (U * (U + 1.0));
                const float gf = (float)g, err = __uint_as_float(kLovaszOne - k[u]);
                acc += err * gf;
                const int64_t px = q[u] >> 1;
                if (px < geo.N) coef[(int64_t)c * geo.N + px] = f ? -gf : gf;  // (1 - 2 f) g
            }
            F += f;
        }
        acc = wave_sum(acc);
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            float a = 0.f;
            for (int i = 0; i < kLovaszThreads / 64; ++i) a += sm[i];
            partial[((int64_t)c * geo.R + r) * geo.tps + (t - (int64_t)seg * geo.tps)] = a;
        }
        __syncthreads();
    }
}

// One workgroup of kLovaszFinalThreads threads.  Scope by scope: wave w sums the tile partials of classes w, w + 16, ... in double (lane
// l the tiles l, l + 64, ..., then the fixed butterfly of wave_sum); then every thread walks the classes in order.
//   out[0] the loss; out[1] = 1 / (scopes that count), 0 if none; then the factor table float [R][CP]: 1 / (classes counted in the
//   scope) for a counted class of a scope that counts, else 0.
__global__ __launch_bounds__(kLovaszFinalThreads) void lovasz_finalize_kernel(const float* __restrict__ partial, const unsigned int* __restrict__ gtot,
                                                                              const LovaszGeom geo, int CP, int all_classes,
                                                                              float* __restrict__ out) {
    __shared__ double Lc[kMaxClasses];
    __shared__ unsigned int Gc[kMaxClasses];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, C = geo.C;
    double total = 0.0;          // the same on every thread
    int counted = 0;
    for (int r = 0; r < geo.R; ++r) {
        for (int c = w; c < C; c += kLovaszFinalThreads / 64) {
            const float* row = partial + ((int64_t)c * geo.R + r) * geo.tps;
            double a = 0.0;
            for (int t = lane; t < geo.tps; t += 64) a += (double)row[t];
            a = wave_sum(a);
            if (lane == 0) { Lc[c] = a; Gc[c] = gtot[(int64_t)c * geo.R + r]; }
        }
        __syncthreads();
        unsigned int V = 0;
        for (int c = 0; c < C; ++c) V += Gc[c];          // every valid pixel is the foreground of exactly one class
        int nc = 0;
        double L = 0.0;
        for (int c = 0; c < C; ++c)
            if (V > 0u && (all_classes || Gc[c] > 0u)) { ++nc; L += Lc[c]; }
        if (threadIdx.x < CP) {
            const int c = threadIdx.x;
            const bool in = c < C && V > 0u && (all_classes || Gc[c] > 0u);
            out[2 + (int64_t)r * CP + c] = in ? (float)(1.0 / (double)nc) : 0.f;
        }
        if (nc > 0) { total += L / (double)nc; ++counted; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = counted ? (float)(total / (double)counted) : 0.f;
        out[1] = counted ? (float)(1.0 / (double)counted) : 0.f;
    }
}

// every row is stored: zeros for a pixel that does not count
template <typename T, int CP, typename Source>
__global__ __launch_bounds__(kCeThreads) void lovasz_bwd_kernel(const Source src, const int64_t* __restrict__ target, int64_t ignore,
                                                                const float* __restrict__ out, const float* __restrict__ coef,
                                                                const float* __restrict__ gscale, int per_image, int64_t N) {
    using index_t = typename Source::index_t;
    __shared__ float sf[CP];
    const int b = blockIdx.y, C = src.C;
    const float* fac = out + 2 + (int64_t)(per_image ? b : 0) * CP;
    for (int c = threadIdx.x; c < CP; c += kCeThreads) sf[c] = fac[c];
    __syncthreads();
    const float k = (gscale ? gscale[0] : 1.f) * out[1];
    const int64_t* tb = target + (int64_t)b * src.HW;
    for (index_t p = (index_t)blockIdx.x * kCeThreads + threadIdx.x; p < src.HW; p += (index_t)gridDim.x * kCeThreads) {
        const int64_t tg = tb[p];
        float g[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) g[c] = 0.f;
        if (lovasz_valid(tg, ignore, C)) {
            src.template load<T, CP>(b, p, g);
            lovasz_probs<CP>(g, C);
            const float* row = coef + (int64_t)b * src.HW + p;
            float a[CP];
            float pm = -1.f, am = 0.f;            // the most probable class m and its coefficient
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                a[c] = (c < C && sf[c] != 0.f) ? row[(int64_t)c * N] * sf[c] : 0.f;       // a class that does not count: its plane is not read
                const bool top = c < C && g[c] > pm;
                pm = top ? g[c] : pm;
                am = top ? a[c] : am;
            }
            // p_j (a_j - sum_c a_c p_c) with every coefficient taken relative to a_m (sum_c p_c = 1): class m drops out of the sum, so
            // a pixel with p_m near 1 keeps the digits of 1 - p_m that a_m - sum_c a_c p_c would cancel away in fp32
            float dot = 0.f;
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                a[c] -= am;
                dot += a[c] * g[c];
            }
#pragma unroll
            for (int c = 0; c < CP; ++c) g[c] = c < C ? k * g[c] * (a[c] - dot) : 0.f;
        }
        src.template store<T, CP>(b, p, g);
    }
}

template <typename T, int CP, typename Source>
__global__ __launch_bounds__(kCeThreads) void lovasz_errors_kernel(const Source src, const int64_t* __restrict__ target, int64_t ignore,
                                                                   int64_t N, float* __restrict__ errors) {
    using index_t = typename Source::index_t;
    const int b = blockIdx.y, C = src.C;
    const int64_t* tb = target + (int64_t)b * src.HW;
    for (index_t p = (index_t)blockIdx.x * kCeThreads + threadIdx.x; p < src.HW; p += (index_t)gridDim.x * kCeThreads) {
        const int64_t tg = tb[p];
        const bool valid = lovasz_valid(tg, ignore, C);
        float z[CP];
        if (valid) {
            src.template load<T, CP>(b, p, z);
            lovasz_probs<CP>(z, C);
        }
        float* row = errors + (int64_t)b * src.HW + p;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) row[(int64_t)c * N] = valid ? lovasz_error(z[c], (int)tg == c) : kLovaszSentinel;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
static int lovasz_class_pad(int64_t C) { return (int)((C + 7) / 8 * 8); }

static LovaszGeom lovasz_geom(int64_t B, int64_t HW, int64_t C, int per_image) {
    LovaszGeom g;
    g.N = B * HW;
    g.L = per_image ? HW : g.N;
    g.R = per_image ? (int)B : 1;
    g.tps = (int)((g.L + kLovaszTile - 1) / kLovaszTile);
    g.C = (int)C;
    return g;
}

static int lovasz_check(const char* who, int64_t B, int64_t HW, int64_t C) {
    MRFP_CHECK(C >= 1 && C <= kMaxClasses, "%s: 1 <= C <= %d (C=%lld)", who, kMaxClasses, (long long)C);
    MRFP_CHECK(B >= 1 && B <= 65535, "%s: 1 <= B <= 65535 (B=%lld)", who, (long long)B);
    MRFP_CHECK(HW > 0 && HW < (1LL << 31) && B * HW < (1LL << 31), "%s: B * H * W < 2^31 (B=%lld HW=%lld)", who, (long long)B, (long long)HW);
    return 0;
}

static int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }

// classes per group: kLovaszGroup, fewer where the group's items would not be countable in 31 bits (N >= 2^29)
static int lovasz_group(int64_t N) {
    const int64_t fit = ((1LL << 31) - 1) / (N > 0 ? N : 1);
    return (int)(fit < 1 ? 1 : (fit < kLovaszGroup ? fit : kLovaszGroup));
}

struct LovaszWs {
    int64_t* offsets;
    unsigned int *keys, *pay, *tilecnt, *gtot;
    float* partial;
    void* sort;
    int64_t bytes;
};

static LovaszWs lovasz_ws(void* ws, const LovaszGeom& g) {
    const int64_t grp = lovasz_group(g.N), n = grp * g.N, S = grp * g.R;
    char* p = (char*)ws;
    LovaszWs w;
    int64_t o = 0;
    w.offsets = (int64_t*)(p + o); o += align16(8 * (S + 1));
    w.keys = (unsigned int*)(p + o); o += align16(4 * n);
    w.pay = (unsigned int*)(p + o); o += align16(4 * n);
    w.tilecnt = (unsigned int*)(p + o); o += align16(4 * S * g.tps);
    w.gtot = (unsigned int*)(p + o); o += align16(4 * (int64_t)g.C * g.R);
    w.partial = (float*)(p + o); o += align16(4 * (int64_t)g.C * g.R * g.tps);
    w.sort = (void*)(p + o);
    const int64_t sb = mrfp_sort_pairs_ws_bytes(n, S);
    o += sb > 0 ? align16(sb) : 0;
    w.bytes = sb < 0 ? -1 : o;
    return w;
}

static unsigned int lovasz_grid(int64_t n) { return (unsigned int)(n < kLovaszMaxGrid ? (n < 1 ? 1 : n) : kLovaszMaxGrid); }

template <typename Source>
static int launch_lovasz_fwd(const char* who, int dtype, int64_t B, const Source& src, const int64_t* target, int64_t ignore, int all_classes,
                             int per_image, void* ws, float* out, hipStream_t st) {
    const LovaszGeom geo = lovasz_geom(B, src.HW, src.C, per_image);
    const LovaszWs w = lovasz_ws(ws, geo);
    MRFP_CHECK(w.bytes > 0, "%s: unsupported size", who);
    const int nbx = ce_w_blocks_x(B, src.HW);
    float* coef = out + 2 + (int64_t)geo.R * lovasz_class_pad(src.C);
    const int grp = lovasz_group(geo.N);
    for (int c0 = 0; c0 < src.C; c0 += grp) {
        const int ncls = src.C - c0 < grp ? src.C - c0 : grp;
        const int nseg = ncls * geo.R;
        const int64_t ntiles = (int64_t)nseg * geo.tps;
        if (int rc = by_dtype_class_pad<kMaxClasses>(dtype, who, src.C, [&](auto t, auto cp) {
                hipLaunchKernelGGL((lovasz_keys_kernel<typename decltype(t)::type, decltype(cp)::value, Source>), dim3(nbx, (unsigned)B),
                                   dim3(kCeThreads), 0, st, src, target, ignore, c0, ncls, geo, w.keys, w.pay, w.offsets);
            }))
            return rc;
        // class j of the group is items [j * N, (j + 1) * N): the first ncls * N items, ncls * R segments
        if (int rc = mrfp_sort_pairs(w.keys, w.pay, w.keys, w.pay, (int64_t)ncls * geo.N, w.offsets, nseg, kLovaszKeyBits, w.sort, st)) return rc;
        hipLaunchKernelGGL(lovasz_count_kernel, dim3(lovasz_grid(ntiles)), dim3(kLovaszThreads), 0, st, w.pay, geo, ntiles, w.tilecnt);
        hipLaunchKernelGGL(lovasz_scan_kernel, dim3(lovasz_grid(nseg)), dim3(kLovaszThreads), 0, st, geo, nseg, c0, w.tilecnt, w.gtot);
        hipLaunchKernelGGL(lovasz_coef_kernel, dim3(lovasz_grid(ntiles)), dim3(kLovaszThreads), 0, st, w.keys, w.pay, geo, ntiles, c0, w.tilecnt,
                           w.gtot, w.partial, coef);
        MRFP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(lovasz_finalize_kernel, dim3(1), dim3(kLovaszFinalThreads), 0, st, w.partial, w.gtot, geo, lovasz_class_pad(src.C),
                       all_classes ? 1 : 0, out);
    MRFP_LAUNCH_CHECK();
    return 0;
}

template <typename Source>
static int launch_lovasz_bwd(const char* who, int dtype, int64_t B, const Source& src, const int64_t* target, int64_t ignore, const float* out,
                             const float* gscale, int per_image, hipStream_t st) {
    const int nbx = ce_w_blocks_x(B, src.HW);
    const int64_t N = B * src.HW;
    const float* coef = out + 2 + (int64_t)(per_image ? B : 1) * lovasz_class_pad(src.C);
    return by_dtype_class_pad<kMaxClasses>(dtype, who, src.C, [&](auto t, auto cp) {
        hipLaunchKernelGGL((lovasz_bwd_kernel<typename decltype(t)::type, decltype(cp)::value, Source>), dim3(nbx, (unsigned)B), dim3(kCeThreads),
                           0, st, src, target, ignore, out, coef, gscale, per_image ? 1 : 0, N);
    });
}

template <typename Source>
static int launch_lovasz_errors(const char* who, int dtype, int64_t B, const Source& src, const int64_t* target, int64_t ignore, float* errors,
                                hipStream_t st) {
    const int nbx = ce_w_blocks_x(B, src.HW);
    const int64_t N = B * src.HW;
    return by_dtype_class_pad<kMaxClasses>(dtype, who, src.C, [&](auto t, auto cp) {
        hipLaunchKernelGGL((lovasz_errors_kernel<typename decltype(t)::type, decltype(cp)::value, Source>), dim3(nbx, (unsigned)B),
                           dim3(kCeThreads), 0, st, src, target, ignore, N, errors);
    });
}

}  // namespace mrfp

extern "C" {

int64_t mrfp_lovasz_group_classes(void) { return mrfp::kLovaszGroup; }

int64_t mrfp_lovasz_ws_bytes(int64_t B, int64_t HW, int64_t C, int per_image) {
    if (B < 1 || B > 65535 || HW < 1 || C < 1 || C > mrfp::kMaxClasses || HW >= (1LL << 31) || B * HW >= (1LL << 31)) return -1;
    return mrfp::lovasz_ws(nullptr, mrfp::lovasz_geom(B, HW, C, per_image)).bytes;
}

int64_t mrfp_lovasz_out_floats(int64_t B, int64_t HW, int64_t C, int per_image) {
    if (B < 1 || HW < 1 || C < 1) return -1;
    return 2 + (per_image ? B : 1) * mrfp::lovasz_class_pad(C) + C * B * HW;
}

int mrfp_lovasz_fwd(const void* logits, const int64_t* target, int dtype, int64_t B, int64_t HW, int64_t C, int64_t ignore_index,
                    int all_classes, int per_image, void* ws, float* out, void* stream) {
    const char* who = "lovasz_fwd";
    MRFP_CHECK(logits && target && ws && out, "%s: null pointer", who);
    MRFP_CHECK((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: ws must be 16-byte aligned", who);
    if (int rc = mrfp::lovasz_check(who, B, HW, C)) return rc;
    return mrfp::launch_lovasz_fwd(who, dtype, B, mrfp::DenseRows{logits, nullptr, HW, (int)C}, target, ignore_index, all_classes, per_image, ws,
                                   out, (hipStream_t)stream);
}

int mrfp_lovasz_bwd(const void* logits, const int64_t* target, const float* out, const float* gscale, void* dlogits, int dtype, int64_t B,
                    int64_t HW, int64_t C, int64_t ignore_index, int per_image, void* stream) {
    const char* who = "lovasz_bwd";
    MRFP_CHECK(logits && target && out && dlogits, "%s: null pointer", who);
    if (int rc = mrfp::lovasz_check(who, B, HW, C)) return rc;
    return mrfp::launch_lovasz_bwd(who, dtype, B, mrfp::DenseRows{logits, dlogits, HW, (int)C}, target, ignore_index, out, gscale, per_image,
                                   (hipStream_t)stream);
}

int mrfp_upsample_lovasz_fwd(const void* P, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H,
                             int64_t W, int64_t C, int64_t ignore_index, int all_classes, int per_image, void* ws, float* out, void* stream) {
    const char* who = "upsample_lovasz_fwd";
    MRFP_CHECK(P && target && ws && out, "%s: null pointer", who);
    MRFP_CHECK((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: ws must be 16-byte aligned", who);
    MRFP_CHECK(H > 0 && W > 0, "%s: bad size", who);
    if (int rc = mrfp::lovasz_check(who, B, H * W, C)) return rc;
    mrfp::BilinearRows src;
    if (int rc = mrfp::bilinear_rows(who, P, ld, nullptr, 0, false, dtype, Hi, Wi, H, W, C, src)) return rc;
    return mrfp::launch_lovasz_fwd(who, dtype, B, src, target, ignore_index, all_classes, per_image, ws, out, (hipStream_t)stream);
}

int mrfp_upsample_lovasz_bwd(const void* P, int64_t ld, const int64_t* target, const float* out, const float* gscale, void* dlogits,
                             int64_t Cd, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H, int64_t W, int64_t C,
                             int64_t ignore_index, int per_image, void* stream) {
    const char* who = "upsample_lovasz_bwd";
    MRFP_CHECK(P && target && out && dlogits, "%s: null pointer", who);
    MRFP_CHECK(H > 0 && W > 0, "%s: bad size", who);
    if (int rc = mrfp::lovasz_check(who, B, H * W, C)) return rc;
    mrfp::BilinearRows src;
    if (int rc = mrfp::bilinear_rows(who, P, ld, dlogits, Cd, false, dtype, Hi, Wi, H, W, C, src)) return rc;
    return mrfp::launch_lovasz_bwd(who, dtype, B, src, target, ignore_index, out, gscale, per_image, (hipStream_t)stream);
}

int mrfp_lovasz_errors(const void* scores, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H,
                       int64_t W, int64_t C, int64_t ignore_index, float* errors, void* stream) {
    const char* who = "lovasz_errors";
    MRFP_CHECK(scores && target && errors, "%s: null pointer", who);
    MRFP_CHECK(H > 0 && W > 0, "%s: bad size", who);
    if (int rc = mrfp::lovasz_check(who, B, H * W, C)) return rc;
    if (Hi == 0 && Wi == 0)          // dense logits [B, H, W, C]
        return mrfp::launch_lovasz_errors(who, dtype, B, mrfp::DenseRows{scores, nullptr, H * W, (int)C}, target, ignore_index, errors,
                                          (hipStream_t)stream);
    mrfp::BilinearRows src;
    if (int rc = mrfp::bilinear_rows(who, scores, ld, nullptr, 0, false, dtype, Hi, Wi, H, W, C, src)) return rc;
    return mrfp::launch_lovasz_errors(who, dtype, B, src, target, ignore_index, errors, (hipStream_t)stream);
}

}  // extern "C"
