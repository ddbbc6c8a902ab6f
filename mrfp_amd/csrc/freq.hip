// freq.hip -- the reference's frequency filters on the GPU: HPF, LPF (dataloaders.py:24-45, 59-79) and PHOT (:47-57).
// The reference runs np.fft.fftn over the (H,W,3) PIL image; the operators here take the ToTensor layout float32 [B,3,H,W]
// holding the same integer values (mrfp_amd/input_pipeline.py::hpf / lpf / phot; restated in tests/test_input_freq_cpu.py).
//
// HPF / LPF: the mask is constant along the channel axis, so both are an independent 2-D filter per channel plane:
//   low = Re(IDFT2(F * band)),  band = (fy^2 + fx^2 <= r^2) for HPF, (< r^2) for LPF, with the signed frequencies of the
//   reference's fftshift (f = i - n//2 for shifted index i); HPF = x - low, LPF = low.
// The band fits in a (2R+1)^2 box (R = floor(r)), so it is evaluated as a band-limited DFT, never a full FFT:
//   band_fwd    T[h,k] = sum_w x[h,w] e^{-2 pi i k w/W} for k = 0..K (negative fx by conjugation: x is real), then the
//               partial column DFT of its 64 rows, F_blk[fy,k]; one partial slab per row block, no atomics
//   band_fold   F = the row-block partials summed in a fixed order; the band mask; the +k / -k columns folded into P, Q
//   band_rows   A[h,k], B[h,k]: the inverse column DFT of P, Q per row (1/(HW) folded in)
//   band_out    low[h,w] = sum_k A[h,k] cos(2 pi k w/W) + B[h,k] sin(2 pi k w/W); y = x - low (HPF) or low (LPF)
// fp32 on the VALU (on gfx950 fp32 MFMA runs at the fp32 vector rate: nothing to gain), twiddles from the caller's double-built
// table exp(-2 pi i t/n) indexed by (f t) mod n reduced in integers.  Every sum runs in a fixed order: bitwise reproducible.
//
// PHOT: y = Re(ifftn(F/|F|)) * 5 * 255 over the 3-D (H,W,3) spectrum.  The channel axis has length 3 and the input is real:
//   F0 = DFT2(x0 + x1 + x2), F1 = DFT2(z), z = x0 + w x1 + w^2 x2 (w = -1/2 - i sqrt(3)/2, exact 3-point form), F2 = conj(F1)
//   mirrored, so y[c] = (u0 + 2 Re(e^{2 pi i c/3} u1)) / 3 * 5 * 255 with u = IDFT2(F/|F|).  A bin with |F| == 0 gives NaN as
//   in numpy: a grey image has z == 0 exactly, hence all-NaN output (the reference's behaviour, not "fixed" here).
//   phot_rows_fwd   row FFTs of the channel sum and of z                          (read 12 B/px, write 16)
//   phot_cols       column FFT, F/|F|, inverse column FFT, per spectrum          (read 16, write 16)
//   phot_rows_inv   inverse row FFTs and the channel inverse -> y[3]             (read 16, write 12)
// Line FFTs: Stockham mixed radix 2/3/4/5 in LDS (8192 complex per workgroup), lengths 2^a 3^b 5^c <= 4096.
#include "common.hpp"
#include <math.h>

namespace mrfp {

// ================================= band-limited DFT (HPF / LPF) =================================
constexpr int kBandRows = 64;        // rows per workgroup of band_fwd: one per lane
constexpr int kBandChunk = 64;       // columns per LDS chunk of band_fwd; each of the 4 waves takes 16 of them
constexpr int kOutRows = 32;         // rows per workgroup of band_out

template <int NKM>
struct BandSmem {
    static constexpr int NC = 2 * NKM;                                  // cos sums k = 0..NKM-1, then sin sums
    static constexpr int XS = kBandRows * (kBandChunk + 1);             // x chunk [row][w], rows padded by one word
    static constexpr int CS = kBandChunk * NC;                          // twiddle chunk [w][j]
    static constexpr int RED = 4 * NC * kBandRows;                      // per-wave sums [wave][j][row]
    static constexpr int PH1 = (XS + CS > RED) ? XS + CS : RED;
    static constexpr int TOTAL = PH1 + kBandRows * NC;                  // + the row spectra T [row][j]
};

template <int NKM>
__global__ __launch_bounds__(256) void band_fwd_kernel(const float* __restrict__ x, float2* __restrict__ part,
                                                       const float2* __restrict__ twW, const float2* __restrict__ twH, int H, int W,
                                                       int NK, int fy_lo, int nfy) {
    typedef BandSmem<NKM> S;
    constexpr int NC = S::NC;
    __shared__ float smem[S::TOTAL];
    float* xs = smem;
    float* cs = smem + S::XS;
    float* red = smem;                                                  // reused after the last chunk
    float* Ts = smem + S::PH1;
    const int p = blockIdx.y, blk = blockIdx.x, h0 = blk * kBandRows;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float* xp = x + (int64_t)p * H * W;
    float acc[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = 0.f;
    for (int w0 = 0; w0 < W; w0 += kBandChunk) {
        for (int e = threadIdx.x; e < kBandRows * kBandChunk; e += 256) {
            const int r = e / kBandChunk, c = e % kBandChunk, h = h0 + r, w = w0 + c;
            xs[r * (kBandChunk + 1) + c] = (h < H && w < W) ? xp[(int64_t)h * W + w] : 0.f;
        }
        for (int e = threadIdx.x; e < kBandChunk * NKM; e += 256) {
            const int c = e / NKM, k = e % NKM, w = w0 + c;
            float cv = 0.f, sv = 0.f;
            if (k < NK && w < W) {
                const float2 t = twW[(int)(((int64_t)k * w) % W)];      // exp(-2 pi i k w / W) = cos - i sin
                cv = t.x;
                sv = -t.y;
            }
            cs[c * NC + k] = cv;
            cs[c * NC + NKM + k] = sv;
        }
        __syncthreads();
        for (int c = wv * (kBandChunk / 4); c < (wv + 1) * (kBandChunk / 4); ++c) {
            const float xv = xs[lane * (kBandChunk + 1) + c];
            const float* cc = cs + c * NC;                             // the same address in every lane: broadcast
#pragma unroll
            for (int j = 0; j < NC; ++j) acc[j] = fmaf(xv, cc[j], acc[j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) red[(wv * NC + j) * kBandRows + lane] = acc[j];
    __syncthreads();
    for (int e = threadIdx.x; e < kBandRows * NC; e += 256) {
        const int j = e / kBandRows, r = e % kBandRows;
        float s = red[j * kBandRows + r] + red[(NC + j) * kBandRows + r];
        s += red[(2 * NC + j) * kBandRows + r];
        s += red[(3 * NC + j) * kBandRows + r];
        Ts[r * NC + j] = s;                       // T[h,k] = Ts[k] - i Ts[NKM + k]
    }
    __syncthreads();
    const int rows = min(kBandRows, H - h0);
    const int nblk = gridDim.x;
    for (int o = threadIdx.x; o < nfy * NK; o += 256) {
        const int fi = o / NK, k = o % NK, fy = fy_lo + fi;
        int idx = (int)(((int64_t)fy * h0) % H);
        if (idx < 0) idx += H;
        int step = fy % H;
        if (step < 0) step += H;
        float ar = 0.f, ai = 0.f;
        for (int r = 0; r < rows; ++r) {
            const float2 t = twH[idx];                                 // exp(-2 pi i fy h / H)
            const float tr = Ts[r * NC + k], ti = -Ts[r * NC + NKM + k];
            ar = fmaf(tr, t.x, ar);
            ar = fmaf(-ti, t.y, ar);
            ai = fmaf(tr, t.y, ai);
            ai = fmaf(ti, t.x, ai);
            idx += step;
            if (idx >= H) idx -= H;
        }
        part[(((int64_t)p * nblk + blk) * nfy + fi) * NK + k] = make_float2(ar, ai);
    }
}

// F[fy, k] for k >= 0 from the partials (fixed order); F[fy, -k] = conj(F[-fy, k]) (periodic -fy).  The folded pair
//   P = Fm[fy,k] + Fm[fy,-k],  Q = Fm[fy,k] - Fm[fy,-k]   (Fm = F * band, and a frequency outside the signed range is absent)
// turns the real part of the 2-D inverse into sum_k A cos + B sin (band_rows / band_out).
__global__ __launch_bounds__(256) void band_fold_kernel(const float2* __restrict__ part, float4* __restrict__ pq, int P, int H, int W,
                                                        int NK, int fy_lo, int nfy, int nblk, float radius, int strict) {
    const int64_t n = (int64_t)P * nfy * NK;
    const double rr = (double)radius * (double)radius;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int k = (int)(i % NK), fi = (int)((i / NK) % nfy), p = (int)(i / ((int64_t)NK * nfy));
        const int fy = fy_lo + fi;
        int fyn = -fy;
        if (fyn > fy_lo + nfy - 1) fyn -= H;                            // -H/2 is in the signed range, +H/2 is not
        const int fin = fyn - fy_lo;
        float2 fp = make_float2(0.f, 0.f), fn = make_float2(0.f, 0.f);
        const float2* base = part + (int64_t)p * nblk * nfy * NK;
        for (int b = 0; b < nblk; ++b) {
            const float2 a = base[((int64_t)b * nfy + fi) * NK + k], c = base[((int64_t)b * nfy + fin) * NK + k];
            fp.x += a.x; fp.y += a.y;
            fn.x += c.x; fn.y += c.y;
        }
        const double d2 = (double)(fy * fy + k * k);
        const bool in = strict ? d2 < rr : d2 <= rr;
        const bool pos = k <= W - 1 - W / 2, neg = k > 0 && k <= W / 2;
        const float2 a = pos ? fp : make_float2(0.f, 0.f);
        const float2 b = neg ? make_float2(fn.x, -fn.y) : make_float2(0.f, 0.f);
        pq[i] = in ? make_float4(a.x + b.x, a.y + b.y, a.x - b.x, a.y - b.y) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// A[h,k] = Re sum_fy P e^{+2 pi i fy h/H},  B[h,k] = -Im sum_fy Q e^{+2 pi i fy h/H}, both times 1/(HW); zero for k >= NK.
__global__ __launch_bounds__(256) void band_rows_kernel(const float4* __restrict__ pq, float* __restrict__ ab, const float2* __restrict__ twH,
                                                        int P, int H, int NK, int NKM, int fy_lo, int nfy, float scale) {
    const int64_t n = (int64_t)P * H * NKM;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int k = (int)(i % NKM), h = (int)((i / NKM) % H), p = (int)(i / ((int64_t)NKM * H));
        float A = 0.f, Bq = 0.f;
        if (k < NK) {
            const float4* q = pq + (int64_t)p * nfy * NK + k;
            for (int fi = 0; fi < nfy; ++fi) {
                int idx = (int)(((int64_t)(fy_lo + fi) * h) % H);
                if (idx < 0) idx += H;
                const float2 t = twH[idx];                             // e^{+i phi} = (t.x, -t.y)
                const float4 v = q[(int64_t)fi * NK];
                A = fmaf(v.x, t.x, A);
                A = fmaf(v.y, t.y, A);
                Bq = fmaf(v.w, t.x, Bq);
                Bq = fmaf(-v.z, t.y, Bq);
            }
        }
        float* o = ab + ((int64_t)p * H + h) * 2 * NKM;
        o[k] = A * scale;
        o[NKM + k] = -Bq * scale;
    }
}

template <int NKM>
__global__ __launch_bounds__(256) void band_out_kernel(const float* x, float* y, const float* __restrict__ ab, const float2* __restrict__ twW,
                                                       int H, int W, int NK, int high) {
    const int w = blockIdx.x * 256 + threadIdx.x, h0 = blockIdx.y * kOutRows, p = blockIdx.z;
    const bool valid = w < W;
    float cw[NKM], sw[NKM];
#pragma unroll
    for (int k = 0; k < NKM; ++k) {
        cw[k] = 0.f;
        sw[k] = 0.f;
        if (k < NK && valid) {
            const float2 t = twW[(int)(((int64_t)k * w) % W)];
            cw[k] = t.x;
            sw[k] = -t.y;
        }
    }
    const int h1 = min(H, h0 + kOutRows);
    for (int h = h0; h < h1; ++h) {
        const float* a = ab + ((int64_t)p * H + h) * 2 * NKM;          // uniform across the workgroup
        float low = 0.f;
#pragma unroll
        for (int k = 0; k < NKM; ++k) {
            low = fmaf(a[k], cw[k], low);
            low = fmaf(a[NKM + k], sw[k], low);
        }
        if (valid) {
            const int64_t o = ((int64_t)p * H + h) * W + w;
            y[o] = high ? x[o] - low : low;
        }
    }
}

struct BandDims {
    int R, NK, NKM, fy_lo, nfy, nblk;
    int64_t part_bytes, pq_bytes, ab_bytes;
};

static inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

static bool band_dims(int64_t B, int64_t H, int64_t W, float radius, BandDims* d) {
    if (B <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535 || B * 3 > 65535 || !(radius >= 0.f) || radius >= 33.f) return false;
    d->R = (int)floorf(radius);
    d->NK = (int)(d->R < W / 2 ? d->R : W / 2) + 1;
    d->NKM = d->R <= 16 ? 17 : 33;
    d->fy_lo = -(int)(d->R < H / 2 ? d->R : H / 2);
    const int fy_hi = (int)(d->R < H - 1 - H / 2 ? d->R : H - 1 - H / 2);
    d->nfy = fy_hi - d->fy_lo + 1;
    d->nblk = (int)((H + kBandRows - 1) / kBandRows);
    const int64_t P = 3 * B;
    d->part_bytes = align256(P * d->nblk * d->nfy * d->NK * (int64_t)sizeof(float2));
    d->pq_bytes = align256(P * d->nfy * d->NK * (int64_t)sizeof(float4));
    d->ab_bytes = align256(P * H * 2 * d->NKM * (int64_t)sizeof(float));
    return true;
}

// ================================= Stockham line FFTs (PHOT) =================================
constexpr int kFftElems = 8192;      // complex values per workgroup (64 KiB of LDS)
constexpr int kFftMaxLen = 4096;
constexpr float kSqrt3Half = 0.86602540378443864676f;

struct FftPlan {
    int n, nr;
    int r[16];
};

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }       // -i a

template <int R>
__device__ __forceinline__ void dft_fwd(float2 (&v)[R]) {
    if constexpr (R == 2) {
        const float2 a = v[0], b = v[1];
        v[0] = cadd(a, b);
        v[1] = csub(a, b);
    } else if constexpr (R == 3) {
        const float2 s = cadd(v[1], v[2]), d = csub(v[1], v[2]);
        const float2 t = make_float2(v[0].x - 0.5f * s.x, v[0].y - 0.5f * s.y);
        const float2 m = mul_mi(make_float2(kSqrt3Half * d.x, kSqrt3Half * d.y));
        v[0] = cadd(v[0], s);
        v[1] = cadd(t, m);
        v[2] = csub(t, m);
    } else if constexpr (R == 4) {
        const float2 s02 = cadd(v[0], v[2]), d02 = csub(v[0], v[2]), s13 = cadd(v[1], v[3]), d13 = mul_mi(csub(v[1], v[3]));
        v[0] = cadd(s02, s13);
        v[2] = csub(s02, s13);
        v[1] = cadd(d02, d13);
        v[3] = csub(d02, d13);
    } else {
        static_assert(R == 5, "radix 2, 3, 4 or 5");
        const float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;
        const float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;
        const float2 t1 = cadd(v[1], v[4]), t2 = cadd(v[2], v[3]), d1 = csub(v[1], v[4]), d2 = csub(v[2], v[3]);
        const float2 a1 = make_float2(v[0].x + c1 * t1.x + c2 * t2.x, v[0].y + c1 * t1.y + c2 * t2.y);
        const float2 a2 = make_float2(v[0].x + c2 * t1.x + c1 * t2.x, v[0].y + c2 * t1.y + c1 * t2.y);
        const float2 b1 = mul_mi(make_float2(s1 * d1.x + s2 * d2.x, s1 * d1.y + s2 * d2.y));
        const float2 b2 = mul_mi(make_float2(s2 * d1.x - s1 * d2.x, s2 * d1.y - s1 * d2.y));
        v[0] = cadd(v[0], cadd(t1, t2));
        v[1] = cadd(a1, b1);
        v[4] = csub(a1, b1);
        v[2] = cadd(a2, b2);
        v[3] = csub(a2, b2);
    }
}

// One Stockham pass of radix R over L lines of length N in LDS (line stride N), p = product of the radices before it.
// Every thread reads all of its butterflies into registers before the barrier and writes after it: in place.
template <int R>
__device__ void fft_pass(float2* buf, int N, int L, int p, const float2* __restrict__ tw) {
    constexpr int MAXB = (kFftElems / R + 255) / 256;
    const int nb = N / R, total = nb * L, step = N / (p * R);
    float2 v[MAXB][R];
#pragma unroll
    for (int m = 0; m < MAXB; ++m) {
        const int b = threadIdx.x + m * 256;
        if (b < total) {
            const int line = b / nb, i = b - line * nb, k = i % p;
            const float2* src = buf + line * N;
#pragma unroll
            for (int q = 0; q < R; ++q) v[m][q] = src[i + q * nb];
#pragma unroll
            for (int q = 1; q < R; ++q) v[m][q] = cmul(v[m][q], tw[q * k * step]);
            dft_fwd<R>(v[m]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < MAXB; ++m) {
        const int b = threadIdx.x + m * 256;
        if (b < total) {
            const int line = b / nb, i = b - line * nb, k = i % p;
            float2* dst = buf + line * N + (i - k) * R + k;
#pragma unroll
            for (int q = 0; q < R; ++q) dst[q * p] = v[m][q];
        }
    }
    __syncthreads();
}

// forward DFT (exp(-2 pi i ...)) of L lines of length plan.n in place; tw = exp(-2 pi i t/n), t < n
__device__ void fft_lines(float2* buf, int L, const FftPlan& plan, const float2* __restrict__ tw) {
    int p = 1;
    for (int s = 0; s < plan.nr; ++s) {
        switch (plan.r[s]) {
            case 4: fft_pass<4>(buf, plan.n, L, p, tw); break;
            case 2: fft_pass<2>(buf, plan.n, L, p, tw); break;
            case 3: fft_pass<3>(buf, plan.n, L, p, tw); break;
            default: fft_pass<5>(buf, plan.n, L, p, tw); break;
        }
        p *= plan.r[s];
    }
}

__global__ __launch_bounds__(256) void phot_rows_fwd_kernel(const float* __restrict__ x, float2* __restrict__ gs, float2* __restrict__ gz,
                                                            FftPlan plan, const float2* __restrict__ twW, int B, int H) {
    __shared__ float2 lds[kFftElems];
    const int W = plan.n, L = kFftElems / (2 * W);
    const int64_t nrows_all = (int64_t)B * H, row0 = (int64_t)blockIdx.x * L;
    const int nrows = (int)min((int64_t)L, nrows_all - row0);
    for (int e = threadIdx.x; e < nrows * W; e += 256) {
        const int j = e / W, w = e - j * W;
        const int64_t g = row0 + j, b = g / H, h = g % H;
        const float* px = x + (b * 3 * H + h) * W + w;
        const int64_t plane = (int64_t)H * W;
        const float x0 = px[0], x1 = px[plane], x2 = px[2 * plane];
        // z = x0 + w x1 + w^2 x2 in the exact 3-point form: a grey pixel gives exactly 0 (no contraction: -ffp-contract=off)
        const float s1 = kSqrt3Half * x1, s2 = kSqrt3Half * x2;
        lds[2 * j * W + w] = make_float2((x0 + x1) + x2, 0.f);
        lds[(2 * j + 1) * W + w] = make_float2((x0 - 0.5f * x1) - 0.5f * x2, s2 - s1);
    }
    __syncthreads();
    fft_lines(lds, 2 * nrows, plan, twW);
    for (int e = threadIdx.x; e < nrows * W; e += 256) {
        const int j = e / W, w = e - j * W;
        const int64_t o = (row0 + j) * W + w;
        gs[o] = lds[2 * j * W + w];
        gz[o] = lds[(2 * j + 1) * W + w];
    }
}

// column FFT of one spectrum (blockIdx.z: 0 = channel sum, 1 = z), F/|F|, inverse column FFT (as conj(FFT(conj(.)))), in place
__global__ __launch_bounds__(256) void phot_cols_kernel(float2* __restrict__ g, FftPlan plan, const float2* __restrict__ twH, int B, int W) {
    __shared__ float2 lds[kFftElems];
    const int H = plan.n, C = min(kFftElems / H, W);
    const int c0 = blockIdx.x * C, nc = min(C, W - c0);
    float2* base = g + ((int64_t)blockIdx.z * B + blockIdx.y) * H * W + c0;
    for (int e = threadIdx.x; e < H * nc; e += 256) {
        const int h = e / nc, c = e - h * nc;
        lds[c * H + h] = base[(int64_t)h * W + c];
    }
    __syncthreads();
    fft_lines(lds, nc, plan, twH);
    for (int e = threadIdx.x; e < H * nc; e += 256) {
        const float2 v = lds[e];
        const float amp = sqrtf(v.x * v.x + v.y * v.y);                // 0 -> 0/0 = NaN, as numpy
        lds[e] = make_float2(v.x / amp, -(v.y / amp));                  // conj: the inverse as a forward transform
    }
    __syncthreads();
    fft_lines(lds, nc, plan, twH);
    for (int e = threadIdx.x; e < H * nc; e += 256) {
        const int h = e / nc, c = e - h * nc;
        const float2 v = lds[c * H + h];
        base[(int64_t)h * W + c] = make_float2(v.x, -v.y);
    }
}

// inverse row FFTs of both spectra, then y[c] = k (u0 + 2 Re(e^{2 pi i c/3} u1)), k = 5 * 255 / (3 H W)
__global__ __launch_bounds__(256) void phot_rows_inv_kernel(const float2* __restrict__ gs, const float2* __restrict__ gz, float* __restrict__ y,
                                                            FftPlan plan, const float2* __restrict__ twW, int B, int H, float k) {
    __shared__ float2 lds[kFftElems];
    const int W = plan.n, L = kFftElems / (2 * W);
    const int64_t nrows_all = (int64_t)B * H, row0 = (int64_t)blockIdx.x * L;
    const int nrows = (int)min((int64_t)L, nrows_all - row0);
    for (int e = threadIdx.x; e < nrows * W; e += 256) {
        const int j = e / W, w = e - j * W;
        const int64_t o = (row0 + j) * W + w;
        const float2 a = gs[o], b = gz[o];
        lds[2 * j * W + w] = make_float2(a.x, -a.y);
        lds[(2 * j + 1) * W + w] = make_float2(b.x, -b.y);
    }
    __syncthreads();
    fft_lines(lds, 2 * nrows, plan, twW);
    for (int e = threadIdx.x; e < nrows * W; e += 256) {
        const int j = e / W, w = e - j * W;
        const int64_t g = row0 + j, b = g / H, h = g % H;
        const float u0 = lds[2 * j * W + w].x;
        const float2 r1 = lds[(2 * j + 1) * W + w];
        const float u1r = r1.x, u1i = -r1.y;
        float* py = y + (b * 3 * H + h) * W + w;
        const int64_t plane = (int64_t)H * W;
        py[0] = k * (u0 + 2.f * u1r);
        py[plane] = k * ((u0 - u1r) - 2.f * kSqrt3Half * u1i);
        py[2 * plane] = k * ((u0 - u1r) + 2.f * kSqrt3Half * u1i);
    }
}

static bool fft_plan(int64_t n, FftPlan* plan) {
    if (n < 1 || n > kFftMaxLen) return false;
    plan->n = (int)n;
    plan->nr = 0;
    int64_t m = n;
    while (m % 4 == 0) { plan->r[plan->nr++] = 4; m /= 4; }
    while (m % 2 == 0) { plan->r[plan->nr++] = 2; m /= 2; }
    while (m % 3 == 0) { plan->r[plan->nr++] = 3; m /= 3; }
    while (m % 5 == 0) { plan->r[plan->nr++] = 5; m /= 5; }
    return m == 1;
}

static int64_t grid_cap(int64_t n, int64_t cap) {
    int64_t b = (n + 255) / 256;
    return b < 1 ? 1 : b > cap ? cap : b;
}

}  // namespace mrfp

using namespace mrfp;

extern "C" {

int64_t mrfp_band_filter_ws_bytes(int64_t B, int64_t H, int64_t W, float radius) {
    BandDims d;
    if (!band_dims(B, H, W, radius, &d)) return -1;
    return d.part_bytes + d.pq_bytes + d.ab_bytes;
}

int mrfp_band_filter(const float* x, float* y, void* ws, const void* twH, const void* twW, int64_t B, int64_t H, int64_t W,
                     float radius, int high, void* stream) {
    MRFP_CHECK(x && y && ws && twH && twW, "band_filter: null argument");
    BandDims d;
    MRFP_CHECK(band_dims(B, H, W, radius, &d), "band_filter: bad arguments (B=%lld H=%lld W=%lld radius=%g; H, W < 65536, 0 <= radius < 33)",
               (long long)B, (long long)H, (long long)W, (double)radius);
    hipStream_t st = (hipStream_t)stream;
    const int P = (int)(3 * B);
    float2* part = (float2*)ws;
    float4* pq = (float4*)((char*)ws + d.part_bytes);
    float* ab = (float*)((char*)ws + d.part_bytes + d.pq_bytes);
    const float2 *th = (const float2*)twH, *tw = (const float2*)twW;
    const dim3 gf((unsigned)d.nblk, (unsigned)P), go((unsigned)((W + 255) / 256), (unsigned)((H + kOutRows - 1) / kOutRows), (unsigned)P);
    if (d.NKM == 17) hipLaunchKernelGGL(band_fwd_kernel<17>, gf, dim3(256), 0, st, x, part, tw, th, (int)H, (int)W, d.NK, d.fy_lo, d.nfy);
    else hipLaunchKernelGGL(band_fwd_kernel<33>, gf, dim3(256), 0, st, x, part, tw, th, (int)H, (int)W, d.NK, d.fy_lo, d.nfy);
    const int64_t nf = (int64_t)P * d.nfy * d.NK;
    hipLaunchKernelGGL(band_fold_kernel, dim3((unsigned)grid_cap(nf, 4096)), dim3(256), 0, st, part, pq, P, (int)H, (int)W, d.NK, d.fy_lo,
                       d.nfy, d.nblk, radius, high ? 0 : 1);
    const int64_t nr = (int64_t)P * H * d.NKM;
    hipLaunchKernelGGL(band_rows_kernel, dim3((unsigned)grid_cap(nr, 8192)), dim3(256), 0, st, pq, ab, th, P, (int)H, d.NK, d.NKM, d.fy_lo,
                       d.nfy, (float)(1.0 / ((double)H * (double)W)));
    if (d.NKM == 17) hipLaunchKernelGGL(band_out_kernel<17>, go, dim3(256), 0, st, x, y, ab, tw, (int)H, (int)W, d.NK, high);
    else hipLaunchKernelGGL(band_out_kernel<33>, go, dim3(256), 0, st, x, y, ab, tw, (int)H, (int)W, d.NK, high);
    MRFP_LAUNCH_CHECK();
    return 0;
}

int64_t mrfp_phot_ws_bytes(int64_t B, int64_t H, int64_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return -1;
    return 2 * B * H * W * (int64_t)sizeof(float2);
}

int mrfp_phot(const float* x, float* y, void* ws, const void* twH, const void* twW, int64_t B, int64_t H, int64_t W, void* stream) {
    MRFP_CHECK(x && y && ws && twH && twW && B > 0 && B <= 65535, "phot: bad arguments");
    FftPlan ph, pw;
    MRFP_CHECK(fft_plan(H, &ph), "phot: line length %lld (H) is not of the form 2^a 3^b 5^c <= %d", (long long)H, kFftMaxLen);
    MRFP_CHECK(fft_plan(W, &pw), "phot: line length %lld (W) is not of the form 2^a 3^b 5^c <= %d", (long long)W, kFftMaxLen);
    hipStream_t st = (hipStream_t)stream;
    float2* gs = (float2*)ws;
    float2* gz = gs + B * H * W;
    const int64_t L = kFftElems / (2 * W), C = (kFftElems / H < W) ? kFftElems / H : W;
    const unsigned nrow_blocks = (unsigned)((B * H + L - 1) / L);
    hipLaunchKernelGGL(phot_rows_fwd_kernel, dim3(nrow_blocks), dim3(256), 0, st, x, gs, gz, pw, (const float2*)twW, (int)B, (int)H);
    hipLaunchKernelGGL(phot_cols_kernel, dim3((unsigned)((W + C - 1) / C), (unsigned)B, 2), dim3(256), 0, st, gs, ph, (const float2*)twH, (int)B,
                       (int)W);
    hipLaunchKernelGGL(phot_rows_inv_kernel, dim3(nrow_blocks), dim3(256), 0, st, gs, gz, y, pw, (const float2*)twW, (int)B, (int)H,
                       (float)(5.0 * 255.0 / (3.0 * (double)H * (double)W)));
    MRFP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
