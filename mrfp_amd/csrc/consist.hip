// consist.hip -- the two-view consistency losses (include/mrfp_hip.h: mrfp_consist_*, mrfp_upsample_consist_*):
// KL(teacher || student) at a temperature, the Jensen-Shannon divergence of the two views, and the pseudo-label cross entropy with
// a confidence threshold.  The "target" of a pixel is a second class vector, so this is no criterion of the pixel-loop skeleton
// (loss_common.hpp: one Source, one value per pixel) but a kernel pair of its own on the skeleton's sources and grid:
//   consist_fwd_kernel       (nbx, B) grid of ce_w_blocks_x; a workgroup stays inside one image.  One partial (sum of the per-pixel
//                            losses, counted pixels, kept pixels) per workgroup, the counts as integers
//   consist_finalize_kernel  one workgroup: the partials in double / 64-bit integers in a fixed order; loss, backward factor, counts
//   consist_bwd_kernel       the same pixel loop; one gradient row per pixel and view that takes a gradient
// Registers.  Two class vectors of CP floats do not fit where one barely does.  The STUDENT's vector is resident (Source::load,
// divided by T in place); the TEACHER is walked in the 16-byte chunks up_logits loads, cache-hot, once for its running maximum /
// sum of exponentials / arg-max, and once more per quantity that needs log q_c beside log p_c (kl: one more walk; js: one for the
// two divergences, in the backward one more for the rows).  Every class index is a compile-time constant of an unrolled loop, so
// no instance uses scratch memory (profiles/consistency.md holds the table).  Gradient rows leave chunk by chunk from the walk.
// Arithmetic is fp32 in log-sum-exp form: log p_c = z^s_c / T - lse_s, log q_c = z^t_c / T - lse_t, q_c log q_c is q_c * (z^t_c / T -
// lse_t), and log m_c = max(log p_c, log q_c) + log(1 + exp(-|log p_c - log q_c|)) - log 2: logits of +-80 give finite values.
// No floating-point atomics (the counts are integer LDS adds) and no host wait: two runs are bit-identical.
#include "loss_common.hpp"

namespace mrfp {

constexpr int kConsistMaxClassPad = 64;        // the widest CP this unit builds: every instance is scratch-free (profiles/consistency.md)
constexpr int kConsistSlot = 4;                // floats per workgroup partial: sum, counted (uint32 bits), kept (uint32 bits), unused
constexpr int kConsistLossFloats = 6;          // loss, backward factor, int64 N_counted, int64 N_kept

template <int K> using Kind = Int<K>;

// ---- the teacher's pixel, chunk by chunk -------------------------------------------------------------------------------------------
// chunk(c0, C, v): the EPC class values from c0 on (EPC = 16 bytes of T; 0 where the class index is >= C).  The arithmetic is the
// source's own load(): DenseRows' conversion, up_logits' interpolation.
template <typename T> struct DenseCursor {
    const T* l;
    __device__ __forceinline__ DenseCursor(const DenseRows& s, int b, int64_t p) : l((const T*)s.logits + (int64_t)b * s.HW * s.C + p * s.C) {}
    template <int N> __device__ __forceinline__ void chunk(int c0, int C, float (&v)[N]) const {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = c0 + i < C ? to_f(l[c0 + i]) : 0.f;
    }
};

template <typename T> struct BilinearCursor {
    const T *p00, *p01, *p10, *p11;
    float lh0, lh1, lw0, lw1;
    __device__ __forceinline__ BilinearCursor(const BilinearRows& s, int b, int p) {
        const int oh = p / s.W, ow = p - oh * s.W;
        const float sh = up_scale(s.Hi, s.H), sw = up_scale(s.Wi, s.W);
        const float fh = sh * (float)oh, fw = sw * (float)ow;
        const int h0 = (int)fh, w0 = (int)fw;
        const int h1 = h0 + (h0 < s.Hi - 1 ? 1 : 0), w1 = w0 + (w0 < s.Wi - 1 ? 1 : 0);
        lh1 = fh - (float)h0; lh0 = 1.f - lh1; lw1 = fw - (float)w0; lw0 = 1.f - lw1;
        const T* P = (const T*)s.P;
        p00 = P + (((size_t)b * s.Hi + h0) * s.Wi + w0) * s.ld;
        p01 = P + (((size_t)b * s.Hi + h0) * s.Wi + w1) * s.ld;
        p10 = P + (((size_t)b * s.Hi + h1) * s.Wi + w0) * s.ld;
        p11 = P + (((size_t)b * s.Hi + h1) * s.Wi + w1) * s.ld;
    }
    template <int N> __device__ __forceinline__ void chunk(int c0, int C, float (&v)[N]) const {
        float a[N], bb[N], c[N], d[N];
#pragma unroll
        for (int i = 0; i < N; ++i) { a[i] = 0.f; bb[i] = 0.f; c[i] = 0.f; d[i] = 0.f; }
        if (c0 < C) {        // chunks past the class count are never read (the pitch may be shorter than CP)
            load_f<T, N>(p00 + c0, a);
            load_f<T, N>(p01 + c0, bb);
            load_f<T, N>(p10 + c0, c);
            load_f<T, N>(p11 + c0, d);
        }
#pragma unroll
        for (int i = 0; i < N; ++i)
            v[i] = c0 + i < C ? lh0 * (lw0 * a[i] + lw1 * bb[i]) + lh1 * (lw0 * c[i] + lw1 * d[i]) : 0.f;
    }
};

template <typename T, typename Source> struct CursorOf;
template <typename T> struct CursorOf<T, DenseRows> { using type = DenseCursor<T>; };
template <typename T> struct CursorOf<T, BilinearRows> { using type = BilinearCursor<T>; };

// one chunk of a gradient row: zeros beyond C are the caller's
template <typename T, int N>
__device__ __forceinline__ void store_chunk(const DenseRows& s, int b, int64_t p, int c0, const float (&g)[N]) {
    T* d = (T*)s.dlogits + (int64_t)b * s.HW * s.C + p * s.C;
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (c0 + i < s.C) d[c0 + i] = from_f<T>(g[i]);
}
template <typename T, int N>
__device__ __forceinline__ void store_chunk(const BilinearRows& s, int b, int p, int c0, const float (&g)[N]) {
    if (c0 < s.Cd) store_f<T, N>((T*)s.dlogits + (int64_t)b * s.HW * s.Cd + (int64_t)p * s.Cd + c0, g);
}

struct ConsistArgs {
    const int64_t* valid;      // NULL: every pixel counts
    float inv_t;               // 1 / T (1 for the pseudo-label kind)
    float threshold;
};

__device__ __forceinline__ bool consist_counts(const int64_t* vb, int64_t p, int C) {
    if (!vb) return true;
    const int64_t v = vb[p];
    return v >= 0 && v < C;
}

// the resident vector: z <- z / T for c < C; returns lse = log sum_c exp(z_c) of the scaled values
template <int CP>
__device__ __forceinline__ float scaled_lse(float (&z)[CP], int C, float inv_t) {
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < CP; ++c) { z[c] *= inv_t; if (c < C) m = fmaxf(m, z[c]); }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) s += c < C ? __expf(z[c] - m) : 0.f;
    return m + __logf(s);
}

// the teacher's first walk: running maximum m, s = sum_c exp(z_c / T - m), and the first arg-max (ascending c, strict >: the first
// maximum wins, as np.argmax and predict.hip).  lse_t = m + log s; softmax(z / T)_k = 1 / s.
template <int CP, int EPC, typename Cursor>
__device__ __forceinline__ void teacher_stats(const Cursor& cur, int C, float inv_t, float& m, float& s, int& k) {
    m = -INFINITY; s = 0.f; k = 0;
#pragma unroll
    for (int c0 = 0; c0 < CP; c0 += EPC) {
        if (c0 < C) {
            float v[EPC];
            cur.template chunk<EPC>(c0, C, v);
            float cm = m;
#pragma unroll
            for (int i = 0; i < EPC; ++i) {
                v[i] *= inv_t;
                if (c0 + i < C && v[i] > cm) { cm = v[i]; k = c0 + i; }
            }
            float add = 0.f;
#pragma unroll
            for (int i = 0; i < EPC; ++i) add += c0 + i < C ? __expf(v[i] - cm) : 0.f;
            s = s * __expf(m - cm) + add;          // (the first chunk: s = 0 * exp(-inf) = 0)
            m = cm;
        }
    }
}

// log m_c - log 2 folded in: log((p + q) / 2) from the two log-probabilities
__device__ __forceinline__ float log_mean(float a, float b) {
    return fmaxf(a, b) + __logf(1.f + __expf(-fabsf(a - b))) - 0.69314718055994531f;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------------
// per counted pixel, in units of the finalize (which multiplies kl / js by T^2): kl: sum_c q_c (log q_c - log p_c); js: (KL(p||m) +
// KL(q||m)) / 2; hard: -log softmax(z^s)_k where the teacher's confidence reaches the threshold
template <typename T, int CP, typename SourceS, typename SourceT, int KIND>
__global__ __launch_bounds__(kCeThreads) void consist_fwd_kernel(const SourceS ss, const SourceT st, const ConsistArgs a,
                                                                 float* __restrict__ ws) {
    using index_t = typename SourceS::index_t;
    using Cursor = typename CursorOf<T, SourceT>::type;
    constexpr int EPC = 16 / (int)sizeof(T);
    __shared__ unsigned int cnt[2];
    __shared__ float sm[kCeThreads / 64];
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0u;
    __syncthreads();
    const int b = blockIdx.y, C = ss.C;
    const int64_t* vb = a.valid ? a.valid + (int64_t)b * ss.HW : nullptr;
    float num = 0.f;
    unsigned int counted = 0u, kept = 0u;
    for (index_t p = (index_t)blockIdx.x * kCeThreads + threadIdx.x; p < ss.HW; p += (index_t)gridDim.x * kCeThreads) {
        if (!consist_counts(vb, p, C)) continue;
        ++counted;
        const Cursor cur(st, b, p);
        float mt, sumt;
        int k;
        teacher_stats<CP, EPC>(cur, C, a.inv_t, mt, sumt, k);
        if constexpr (KIND == MRFP_CONSIST_HARD) {
            if (!(1.f / sumt >= a.threshold)) continue;
        }
        ++kept;
        float z[CP];
        ss.template load<T, CP>(b, p, z);
        const float lse_s = scaled_lse<CP>(z, C, a.inv_t);
        if constexpr (KIND == MRFP_CONSIST_HARD) {
            float zk = 0.f;
#pragma unroll
            for (int c = 0; c < CP; ++c) zk = (c == k) ? z[c] : zk;          // a predicated pick: a run-time index would mean scratch memory
            num += lse_s - zk;
        } else {
            const float lse_t = mt + __logf(sumt);
            float acc = 0.f;
#pragma unroll
            for (int c0 = 0; c0 < CP; c0 += EPC) {
                if (c0 < C) {
                    float v[EPC];
                    cur.template chunk<EPC>(c0, C, v);
#pragma unroll
                    for (int i = 0; i < EPC; ++i) {
                        if (c0 + i < C) {
                            const float lq = v[i] * a.inv_t - lse_t, lp = z[c0 + i] - lse_s;
                            if constexpr (KIND == MRFP_CONSIST_KL) {
                                acc += __expf(lq) * (lq - lp);
                            } else {
                                const float lm = log_mean(lp, lq);
                                acc += 0.5f * (__expf(lp) * (lp - lm) + __expf(lq) * (lq - lm));
                            }
                        }
                    }
                }
            }
            num += acc;
        }
    }
    // the workgroup's partial: the float sum in a fixed order (wave, then waves in order), the counts as integer adds
    num = wave_sum(num);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = num;
    if (counted) atomicAdd(&cnt[0], counted);
    if (kept) atomicAdd(&cnt[1], kept);
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < kCeThreads / 64; ++i) t += sm[i];
        float* slot = ws + kConsistSlot * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x);
        slot[0] = t;
        slot[1] = __uint_as_float(cnt[0]);
        slot[2] = __uint_as_float(cnt[1]);
        slot[3] = 0.f;
    }
}

// One workgroup of 256 threads over n partials, a fixed order.  lscale: T^2 (kl, js) or 1; bscale: T or 1.  D = N_kept (hard,
// normalize "kept"; kl / js: N_kept == N_counted) or N_counted.  D == 0: loss 0 and factor 0, so every gradient row is 0.
__global__ __launch_bounds__(256) void consist_finalize_kernel(const float* __restrict__ ws, int64_t n, double lscale, double bscale,
                                                               int by_counted, float* __restrict__ out) {
    __shared__ double sa[256];
    __shared__ unsigned long long sc[256], sk[256];
    double acc = 0.0;
    unsigned long long nc = 0ull, nk = 0ull;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        acc += (double)ws[kConsistSlot * i];
        nc += __float_as_uint(ws[kConsistSlot * i + 1]);
        nk += __float_as_uint(ws[kConsistSlot * i + 2]);
    }
    sa[threadIdx.x] = acc; sc[threadIdx.x] = nc; sk[threadIdx.x] = nk;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            sa[threadIdx.x] += sa[threadIdx.x + s];
            sc[threadIdx.x] += sc[threadIdx.x + s];
            sk[threadIdx.x] += sk[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long D = by_counted ? sc[0] : sk[0];
        out[0] = D ? (float)(lscale * sa[0] / (double)D) : 0.f;
        out[1] = D ? (float)(bscale / (double)D) : 0.f;
        int64_t* counts = reinterpret_cast<int64_t*>(out + 2);
        counts[0] = (int64_t)sc[0];
        counts[1] = (int64_t)sk[0];
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------------
// k = gscale[0] * out[1].  kl: d z^s_j = k (p_j - q_j).  hard: k (softmax(z^s)_j - [j == arg-max]) at a kept pixel.  js, with
// u_j = (log p_j - log m_j) / 2 and w_j = (log q_j - log m_j) / 2: d z^s_j = k p_j (u_j - sum_c p_c u_c), d z^t_j = k q_j (w_j - sum_c q_c
// w_c).  A view whose dlogits is NULL gets no row; a view that has one gets a row for every pixel: zeros where the pixel does not
// count or is not kept, and in the pad channels.
template <typename T, int CP, typename SourceS, typename SourceT, int KIND>
__global__ __launch_bounds__(kCeThreads) void consist_bwd_kernel(const SourceS ss, const SourceT st, const ConsistArgs a,
                                                                 const float* __restrict__ out, const float* __restrict__ gscale) {
    using index_t = typename SourceS::index_t;
    using Cursor = typename CursorOf<T, SourceT>::type;
    constexpr int EPC = 16 / (int)sizeof(T);
    const int b = blockIdx.y, C = ss.C;
    const int64_t* vb = a.valid ? a.valid + (int64_t)b * ss.HW : nullptr;
    const float kf = (gscale ? gscale[0] : 1.f) * out[1];
    const bool gs = ss.dlogits != nullptr, gt = KIND == MRFP_CONSIST_JS && st.dlogits != nullptr;
    for (index_t p = (index_t)blockIdx.x * kCeThreads + threadIdx.x; p < ss.HW; p += (index_t)gridDim.x * kCeThreads) {
        bool on = consist_counts(vb, p, C);
        float mt = 0.f, sumt = 1.f;
        int k = 0;
        const Cursor cur(st, b, p);
        if (on) {
            teacher_stats<CP, EPC>(cur, C, a.inv_t, mt, sumt, k);
            if constexpr (KIND == MRFP_CONSIST_HARD) on = 1.f / sumt >= a.threshold;
        }
        if (!on) {
            float zero[EPC];
#pragma unroll
            for (int i = 0; i < EPC; ++i) zero[i] = 0.f;
#pragma unroll
            for (int c0 = 0; c0 < CP; c0 += EPC) {
                if (gs) store_chunk<T, EPC>(ss, b, p, c0, zero);
                if (gt) store_chunk<T, EPC>(st, b, p, c0, zero);
            }
            continue;
        }
        float z[CP];
        ss.template load<T, CP>(b, p, z);
        const float lse_s = scaled_lse<CP>(z, C, a.inv_t);
        if constexpr (KIND == MRFP_CONSIST_HARD) {
#pragma unroll
            for (int c0 = 0; c0 < CP; c0 += EPC) {
                float g[EPC];
#pragma unroll
                for (int i = 0; i < EPC; ++i)
                    g[i] = c0 + i < C ? kf * (__expf(z[c0 + i] - lse_s) - (c0 + i == k ? 1.f : 0.f)) : 0.f;
                store_chunk<T, EPC>(ss, b, p, c0, g);
            }
        } else {
            const float lse_t = mt + __logf(sumt);
            float klp = 0.f, klq = 0.f;          // js: sum_c p_c u_c, sum_c q_c w_c
            if constexpr (KIND == MRFP_CONSIST_JS) {
#pragma unroll
                for (int c0 = 0; c0 < CP; c0 += EPC) {
                    if (c0 < C) {
                        float v[EPC];
                        cur.template chunk<EPC>(c0, C, v);
#pragma unroll
                        for (int i = 0; i < EPC; ++i) {
                            if (c0 + i < C) {
                                const float lq = v[i] * a.inv_t - lse_t, lp = z[c0 + i] - lse_s;
                                const float lm = log_mean(lp, lq);
                                klp += __expf(lp) * (0.5f * (lp - lm));
                                klq += __expf(lq) * (0.5f * (lq - lm));
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int c0 = 0; c0 < CP; c0 += EPC) {
                float v[EPC], g[EPC], h[EPC];
                cur.template chunk<EPC>(c0, C, v);
#pragma unroll
                for (int i = 0; i < EPC; ++i) {
                    g[i] = 0.f; h[i] = 0.f;
                    if (c0 + i < C) {
                        const float lq = v[i] * a.inv_t - lse_t, lp = z[c0 + i] - lse_s;
                        if constexpr (KIND == MRFP_CONSIST_KL) {
                            g[i] = kf * (__expf(lp) - __expf(lq));
                        } else {
                            const float lm = log_mean(lp, lq);
                            g[i] = kf * __expf(lp) * (0.5f * (lp - lm) - klp);
                            h[i] = kf * __expf(lq) * (0.5f * (lq - lm) - klq);
                        }
                    }
                }
                if (gs) store_chunk<T, EPC>(ss, b, p, c0, g);
                if (gt) store_chunk<T, EPC>(st, b, p, c0, h);
            }
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
template <typename F>
static void by_consist_kind(int kind, F&& f) {
    switch (kind) {
        case MRFP_CONSIST_KL: f(Kind<MRFP_CONSIST_KL>{}); break;
        case MRFP_CONSIST_JS: f(Kind<MRFP_CONSIST_JS>{}); break;
        default: f(Kind<MRFP_CONSIST_HARD>{}); break;
    }
}

static int consist_check(const char* who, int64_t B, int64_t HW, int64_t C, int kind, float temperature, float threshold) {
    MRFP_CHECK(C >= 1 && C <= kConsistMaxClassPad, "%s: 1 <= C <= %d: the student's class vector lives in registers (C=%lld)", who,
               kConsistMaxClassPad, (long long)C);
    MRFP_CHECK(B >= 1 && B <= 65535, "%s: 1 <= B <= 65535 (B=%lld)", who, (long long)B);
    MRFP_CHECK(HW > 0 && HW < (1LL << 31), "%s: bad size (HW=%lld)", who, (long long)HW);
    MRFP_CHECK(kind == MRFP_CONSIST_KL || kind == MRFP_CONSIST_JS || kind == MRFP_CONSIST_HARD, "%s: unknown kind %d", who, kind);
    MRFP_CHECK(temperature > 0.f && temperature <= 3.0e38f, "%s: the temperature must be a finite number > 0 (got %g)", who,
               (double)temperature);
    MRFP_CHECK(threshold >= 0.f && threshold <= 1.f, "%s: the threshold must be in [0, 1] (got %g)", who, (double)threshold);
    return 0;
}

static ConsistArgs consist_args(const int64_t* valid, int kind, float temperature, float threshold) {
    return ConsistArgs{valid, kind == MRFP_CONSIST_HARD ? 1.f : 1.f / temperature, threshold};
}

template <typename Source>
static int launch_consist_fwd(const char* who, int dtype, int64_t B, const Source& ss, const Source& st, const int64_t* valid, int kind,
                              float temperature, float threshold, int normalize, float* ws, float* loss, hipStream_t stream) {
    MRFP_CHECK(normalize == MRFP_CONSIST_KEPT || normalize == MRFP_CONSIST_VALID, "%s: unknown normalize %d", who, normalize);
    MRFP_CHECK((reinterpret_cast<uintptr_t>(loss) & 7) == 0, "%s: loss must be 8-byte aligned", who);
    const int nbx = ce_w_blocks_x(B, ss.HW);
    const ConsistArgs a = consist_args(valid, kind, temperature, threshold);
    if (int rc = by_dtype_class_pad<kConsistMaxClassPad>(dtype, who, ss.C, [&](auto t, auto cp) {
            by_consist_kind(kind, [&](auto kd) {
                hipLaunchKernelGGL((consist_fwd_kernel<typename decltype(t)::type, decltype(cp)::value, Source, Source, decltype(kd)::value>),
                                   dim3(nbx, (unsigned)B), dim3(kCeThreads), 0, stream, ss, st, a, ws);
            });
        }))
        return rc;
    const bool hard = kind == MRFP_CONSIST_HARD;
    const double T = (double)temperature;
    hipLaunchKernelGGL(consist_finalize_kernel, dim3(1), dim3(256), 0, stream, ws, (int64_t)nbx * B, hard ? 1.0 : T * T, hard ? 1.0 : T,
                       (hard && normalize == MRFP_CONSIST_VALID) ? 1 : 0, loss);
    MRFP_LAUNCH_CHECK();
    return 0;
}

template <typename Source>
static int launch_consist_bwd(const char* who, int dtype, int64_t B, const Source& ss, const Source& st, const int64_t* valid, int kind,
                              float temperature, float threshold, const float* loss, const float* gscale, hipStream_t stream) {
    MRFP_CHECK(ss.dlogits || st.dlogits, "%s: no view takes a gradient", who);
    MRFP_CHECK(kind == MRFP_CONSIST_JS || (ss.dlogits && !st.dlogits), "%s: the teacher is a constant of kinds kl and hard", who);
    const int nbx = ce_w_blocks_x(B, ss.HW);
    const ConsistArgs a = consist_args(valid, kind, temperature, threshold);
    return by_dtype_class_pad<kConsistMaxClassPad>(dtype, who, ss.C, [&](auto t, auto cp) {
        by_consist_kind(kind, [&](auto kd) {
            hipLaunchKernelGGL((consist_bwd_kernel<typename decltype(t)::type, decltype(cp)::value, Source, Source, decltype(kd)::value>),
                               dim3(nbx, (unsigned)B), dim3(kCeThreads), 0, stream, ss, st, a, loss, gscale);
        });
    });
}

// a fused view: the geometry check of bilinear_rows, with the gradient row optional in the backward (dlogits NULL: no row)
static int consist_view(const char* who, const void* P, int64_t ld, void* dlogits, int64_t Cd, int dtype, int64_t Hi, int64_t Wi,
                        int64_t H, int64_t W, int64_t C, BilinearRows& src) {
    return bilinear_rows(who, P, ld, dlogits, dlogits ? Cd : 0, true, dtype, Hi, Wi, H, W, C, src);
}

}  // namespace mrfp

extern "C" {

int64_t mrfp_consist_max_classes(void) { return mrfp::kConsistMaxClassPad; }

int64_t mrfp_consist_nblocks(int64_t B, int64_t HW) { return (int64_t)mrfp::ce_w_blocks_x(B, HW) * (B > 0 ? B : 1); }

int64_t mrfp_consist_ws_floats(int64_t B, int64_t HW) { return mrfp::kConsistSlot * mrfp_consist_nblocks(B, HW); }

int64_t mrfp_consist_loss_floats(void) { return mrfp::kConsistLossFloats; }

int mrfp_consist_fwd(const void* logits_s, const void* logits_t, const int64_t* valid, int dtype, int64_t B, int64_t HW, int64_t C,
                     int kind, float temperature, float threshold, int normalize, float* ws, float* loss, void* stream) {
    const char* who = "consist_fwd";
    MRFP_CHECK(logits_s && logits_t && ws && loss, "%s: null pointer", who);
    if (int rc = mrfp::consist_check(who, B, HW, C, kind, temperature, threshold)) return rc;
    return mrfp::launch_consist_fwd(who, dtype, B, mrfp::DenseRows{logits_s, nullptr, HW, (int)C}, mrfp::DenseRows{logits_t, nullptr, HW, (int)C},
                                    valid, kind, temperature, threshold, normalize, ws, loss, (hipStream_t)stream);
}

int mrfp_consist_bwd(const void* logits_s, const void* logits_t, const int64_t* valid, const float* loss, const float* gscale,
                     void* dlogits_s, void* dlogits_t, int dtype, int64_t B, int64_t HW, int64_t C, int kind, float temperature,
                     float threshold, void* stream) {
    const char* who = "consist_bwd";
    MRFP_CHECK(logits_s && logits_t && loss, "%s: null pointer", who);
    if (int rc = mrfp::consist_check(who, B, HW, C, kind, temperature, threshold)) return rc;
    return mrfp::launch_consist_bwd(who, dtype, B, mrfp::DenseRows{logits_s, dlogits_s, HW, (int)C},
                                    mrfp::DenseRows{logits_t, dlogits_t, HW, (int)C}, valid, kind, temperature, threshold, loss, gscale,
                                    (hipStream_t)stream);
}

int mrfp_upsample_consist_fwd(const void* P_s, int64_t ld_s, int64_t Hi_s, int64_t Wi_s, const void* P_t, int64_t ld_t, int64_t Hi_t,
                              int64_t Wi_t, const int64_t* valid, int dtype, int64_t B, int64_t H, int64_t W, int64_t C, int kind,
                              float temperature, float threshold, int normalize, float* ws, float* loss, void* stream) {
    const char* who = "upsample_consist_fwd";
    MRFP_CHECK(P_s && P_t && ws && loss, "%s: null pointer", who);
    MRFP_CHECK(H > 0 && W > 0, "%s: bad size", who);
    if (int rc = mrfp::consist_check(who, B, H * W, C, kind, temperature, threshold)) return rc;
    mrfp::BilinearRows ss, st;
    if (int rc = mrfp::consist_view(who, P_s, ld_s, nullptr, 0, dtype, Hi_s, Wi_s, H, W, C, ss)) return rc;
    if (int rc = mrfp::consist_view(who, P_t, ld_t, nullptr, 0, dtype, Hi_t, Wi_t, H, W, C, st)) return rc;
    return mrfp::launch_consist_fwd(who, dtype, B, ss, st, valid, kind, temperature, threshold, normalize, ws, loss, (hipStream_t)stream);
}

int mrfp_upsample_consist_bwd(const void* P_s, int64_t ld_s, int64_t Hi_s, int64_t Wi_s, const void* P_t, int64_t ld_t, int64_t Hi_t,
                              int64_t Wi_t, const int64_t* valid, const float* loss, const float* gscale, void* dlogits_s,
                              void* dlogits_t, int64_t Cd, int dtype, int64_t B, int64_t H, int64_t W, int64_t C, int kind,
                              float temperature, float threshold, void* stream) {
    const char* who = "upsample_consist_bwd";
    MRFP_CHECK(P_s && P_t && loss, "%s: null pointer", who);
    MRFP_CHECK(H > 0 && W > 0, "%s: bad size", who);
    if (int rc = mrfp::consist_check(who, B, H * W, C, kind, temperature, threshold)) return rc;
    mrfp::BilinearRows ss, st;
    if (int rc = mrfp::consist_view(who, P_s, ld_s, dlogits_s, Cd, dtype, Hi_s, Wi_s, H, W, C, ss)) return rc;
    if (int rc = mrfp::consist_view(who, P_t, ld_t, dlogits_t, Cd, dtype, Hi_t, Wi_t, H, W, C, st)) return rc;
    return mrfp::launch_consist_bwd(who, dtype, B, ss, st, valid, kind, temperature, threshold, loss, gscale, (hipStream_t)stream);
}

}  // extern "C"
