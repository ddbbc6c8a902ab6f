// input.hip -- the training input pipeline (transform_tr) on the GPU, bit-exact with the PIL calls the reference makes
// (main.py:409-419 transform_tr; dataloaders.py:139-150 RandomHorizontalFlip, 398-435 RandomSizeAndCrop -> img.resize(BICUBIC)
// / mask.resize(NEAREST), 257-337 RandomCrop with ImageOps.expand padding, 467-482 Resize, 118-136 ToTensor).
//
// PIL (Pillow 12.2, src/libImaging/Resample.c) resizes 8-bit images in two separable passes with fixed-point
// coefficients: out = clip8((2^21 + sum_x in[xmin + x] * k[x]) >> 22), horizontal pass first, 8-bit intermediate.  The
// coefficient / bounds tables are built on the host in double precision exactly as Pillow does (mrfp_amd/input_pipeline.py,
// oracle/input_oracle.py); the kernels do the integer arithmetic, so the result equals PIL's byte for byte.
//   resample_u8   one separable pass over a [H,W,C] uint8 image (the horizontal pass can read the source mirrored: the
//                 reference flips BEFORE it scales)
//   box_blur3     one pass of ImageFilter.GaussianBlur's box-blur approximation (radius < 1: dataloaders.py:168-177)
//   assemble      pad (ImageOps.expand: image 0, label ignore_index) + crop + ToTensor: float32 [3,Hc,Wc] in 0..255 and the
//                 int64 label map, the label fetched through PIL's nearest-neighbour index tables from the ORIGINAL map
//   affine_u8     Image.rotate of an image / label pair (dataloaders.py:153-165 RandomRotate): PIL's affine transform
//   u8hwc_to_f32chw_norm   Normalize (dataloaders.py:95-115) fused into the ToTensor store
#include "common.hpp"
#include <cmath>

namespace mrfp {

constexpr int kPrecisionBits = 32 - 8 - 2;      // Pillow Resample.c PRECISION_BITS

__global__ __launch_bounds__(256) void resample_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int Hin,
                                                          int Win, int Hout, int Wout, int C, const int32_t* __restrict__ bounds,
                                                          const int32_t* __restrict__ coefs, int ksize, int vertical, int flip) {
    const int64_t n = (int64_t)Hout * Wout * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        const int64_t pix = i / C;
        const int ox = (int)(pix % Wout), oy = (int)(pix / Wout);
        const int o = vertical ? oy : ox;
        const int lo = bounds[2 * o], cnt = bounds[2 * o + 1];
        const int32_t* k = coefs + (int64_t)o * ksize;
        int acc = 1 << (kPrecisionBits - 1);
        if (vertical) {
            for (int t = 0; t < cnt; ++t) acc += (int)src[((int64_t)(lo + t) * Win + ox) * C + c] * k[t];
        } else {
            for (int t = 0; t < cnt; ++t) {
                const int sx = flip ? Win - 1 - (lo + t) : lo + t;
                acc += (int)src[((int64_t)oy * Win + sx) * C + c] * k[t];
            }
        }
        const int v = acc >> kPrecisionBits;                // arithmetic shift, then clip8
        dst[i] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
}

__global__ __launch_bounds__(256) void input_assemble_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lab,
                                                             const int32_t* __restrict__ ytab, const int32_t* __restrict__ xtab,
                                                             int Hs, int Ws, int Hl, int Wl, int flip, int pad_x, int pad_y, int x1,
                                                             int y1, int Hc, int Wc, int ignore, float* __restrict__ out_img,
                                                             uint8_t* __restrict__ out_u8, int64_t* __restrict__ out_lab) {
    const int64_t n = (int64_t)Hc * Wc;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % Wc), oy = (int)(i / Wc);
        const int px = x1 + ox - pad_x, py = y1 + oy - pad_y;       // position in the scaled image
        const bool inside = px >= 0 && px < Ws && py >= 0 && py < Hs;
        uint8_t r = 0, g = 0, b = 0;
        int64_t l = ignore;
        if (inside) {
            const uint8_t* p = img + ((int64_t)py * Ws + px) * 3;
            r = p[0]; g = p[1]; b = p[2];
            const int sy = ytab[py], sx0 = xtab[px];
            if (sy >= 0 && sy < Hl && sx0 >= 0 && sx0 < Wl) l = lab[(int64_t)sy * Wl + (flip ? Wl - 1 - sx0 : sx0)];
            else l = 0;                                               // ImagingScaleAffine leaves such pixels of a new image zero
        }
        if (out_u8) {                                   // uint8 [Hc,Wc,3]: the blur passes come before ToTensor
            out_u8[3 * i] = r; out_u8[3 * i + 1] = g; out_u8[3 * i + 2] = b;
        } else {
            out_img[i] = (float)r;
            out_img[n + i] = (float)g;
            out_img[2 * n + i] = (float)b;
        }
        out_lab[i] = l;
    }
}

// One pass of Pillow's box blur (BoxBlur.c ImagingLineBoxBlur8) for a box radius below 1 -- all ImageFilter.GaussianBlur
// ever asks for when its radius is random.random() (dataloaders.py:172-174): out = (in*ww + (left + right)*fw + 2^23) >> 24
// with the edge pixels replicated; GaussianBlur = 3 horizontal + 3 vertical passes, every pass rounded to 8 bits.
__global__ __launch_bounds__(256) void box_blur3_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W,
                                                           int C, unsigned ww, unsigned fw, int vertical) {
    const int64_t n = (int64_t)H * W * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        const int64_t pix = i / C;
        const int x = (int)(pix % W), y = (int)(pix / W);
        unsigned a, b;
        if (vertical) {
            a = src[((int64_t)(y > 0 ? y - 1 : 0) * W + x) * C + c];
            b = src[((int64_t)(y < H - 1 ? y + 1 : H - 1) * W + x) * C + c];
        } else {
            a = src[((int64_t)y * W + (x > 0 ? x - 1 : 0)) * C + c];
            b = src[((int64_t)y * W + (x < W - 1 ? x + 1 : W - 1)) * C + c];
        }
        const unsigned bulk = (unsigned)src[i] * ww + (a + b) * fw;
        dst[i] = (uint8_t)((bulk + (1u << 23)) >> 24);
    }
}

__global__ __launch_bounds__(256) void u8hwc_to_f32chw_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int64_t npix) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        dst[i] = (float)src[3 * i];
        dst[npix + i] = (float)src[3 * i + 1];
        dst[2 * npix + i] = (float)src[3 * i + 2];
    }
}

// ---- ColorJitter (dataloaders.py:491-660): PIL ImageEnhance blends and the HSV round trip, per pixel ---------------------
// ImageEnhance.X(img).enhance(f) = Image.blend(degenerate, img, f) = clip8((float)d + f * (float)(p - d)) per byte (Blend.c,
// C float arithmetic), with d = 0 (Brightness), the rounded mean of the L image (Contrast) or the pixel's own L (Color);
// L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (Convert.c).  adjust_hue: RGB -> HSV (Convert.c rgb2hsv: float / double
// mix as in the C source), H += shift (uint8 wrap), HSV -> RGB.  Restated in oracle/input_oracle.py and pinned against PIL
// there (the two conversions on all 2^24 triples).
__device__ __forceinline__ int pil_l(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }
__device__ __forceinline__ uint8_t pil_blend(int d, int p, float alpha) {
    const float t = (float)d + alpha * (float)(p - d);
    return (uint8_t)(t <= 0.f ? 0 : t >= 255.f ? 255 : (int)t);
}

__global__ __launch_bounds__(256) void gray_sum_kernel(const uint8_t* __restrict__ src, int64_t npix, unsigned long long* __restrict__ sum) {
    unsigned long long acc = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256)
        acc += (unsigned)pil_l(src[3 * i], src[3 * i + 1], src[3 * i + 2]);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(sum, acc);          // integer sum: exact in any order
}
__global__ void gray_mean_kernel(const unsigned long long* __restrict__ sum, int64_t npix, int* __restrict__ gray) {
    *gray = (int)((double)*sum / (double)npix + 0.5);                  // int(ImageStat.Stat(L).mean[0] + 0.5)
}

// op: 0 brightness, 1 contrast (*gray), 2 saturation (own L), 3 hue (shift)
__global__ __launch_bounds__(256) void jitter_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t npix, int op,
                                                        float alpha, int shift, const int* __restrict__ gray) {
    const int gm = (op == 1) ? *gray : 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const int r = src[3 * i], g = src[3 * i + 1], b = src[3 * i + 2];
        uint8_t o0, o1, o2;
        if (op < 3) {
            const int d = op == 0 ? 0 : op == 1 ? gm : pil_l(r, g, b);
            o0 = pil_blend(d, r, alpha); o1 = pil_blend(d, g, alpha); o2 = pil_blend(d, b, alpha);
        } else {
            const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
            int uh = 0, us = 0;
            const int uv = maxc;
            if (minc != maxc) {
                const float cr = (float)(maxc - minc);
                const float sf = cr / (float)maxc;
                const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
                float h;
                if (r == maxc) h = bc - gc;
                else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
                else h = (float)(4.0 + (double)gc - (double)rc);
                const double hd = (double)h / 6.0 + 1.0;
                h = (float)(hd - floor(hd));                           // fmod(., 1.0) of a positive number
                uh = (int)((double)h * 255.0);
                us = (int)((double)sf * 255.0);
                uh = uh < 0 ? 0 : uh > 255 ? 255 : uh;
                us = us < 0 ? 0 : us > 255 ? 255 : us;
            }
            uh = (uh + shift) & 255;                                   // np_h += np.uint8(hue_factor * 255)
            if (us == 0) {
                o0 = o1 = o2 = (uint8_t)uv;
            } else {
                const float fs = (float)us / 255.0f;
                const double hh = (double)uh * 6.0 / 255.0;
                const int ii = (int)floor(hh);
                const float f = (float)(hh - (double)ii);
                const float vf = (float)uv;
                const double pd = round((double)(vf * (1.0f - fs))), qd = round((double)(vf * (1.0f - fs * f))),
                             td = round((double)(vf * (1.0f - fs * (1.0f - f))));
                const uint8_t pp = (uint8_t)(pd < 0 ? 0 : pd > 255 ? 255 : pd), qq = (uint8_t)(qd < 0 ? 0 : qd > 255 ? 255 : qd),
                              tt = (uint8_t)(td < 0 ? 0 : td > 255 ? 255 : td), vv = (uint8_t)uv;
                switch (ii % 6) {
                    case 0: o0 = vv; o1 = tt; o2 = pp; break;
                    case 1: o0 = qq; o1 = vv; o2 = pp; break;
                    case 2: o0 = pp; o1 = vv; o2 = tt; break;
                    case 3: o0 = pp; o1 = qq; o2 = vv; break;
                    case 4: o0 = tt; o1 = pp; o2 = vv; break;
                    default: o0 = vv; o1 = pp; o2 = qq; break;
                }
            }
        }
        dst[3 * i] = o0; dst[3 * i + 1] = o1; dst[3 * i + 2] = o2;
    }
}

// ---- evaluation input path: label encoding and the validation assemble ------------------------------------------------------
// The reference rewrites every label map on the host with one masked numpy pass per class id (main.py:106-112 encode_segmap,
// :561-563 Synthia, :742-745 Mapillary); whatever order those passes run in, the result is a function of the source byte, i.e. a
// 256-entry table (built on the host by replaying the passes on arange(256): mrfp_amd/input_pipeline.py::LabelEncoder).
// One lane moves 16 bytes, one workgroup a chunk of kThreads * 16 bytes per step of its walk; the table sits in LDS.
constexpr int kLutVec = 16;
constexpr int kLutChunk = kThreads * kLutVec;        // bytes per workgroup and step

__device__ __forceinline__ void load_label_table(uint8_t (&tab)[256], const uint8_t* __restrict__ lut) {
    tab[threadIdx.x] = lut ? lut[threadIdx.x] : (uint8_t)threadIdx.x;       // kThreads == 256 entries; NULL: identity
    __syncthreads();
}
__device__ __forceinline__ uint32_t lut4(const uint8_t (&tab)[256], uint32_t v) {
    return (uint32_t)tab[v & 255] | ((uint32_t)tab[(v >> 8) & 255] << 8) | ((uint32_t)tab[(v >> 16) & 255] << 16) |
           ((uint32_t)tab[v >> 24] << 24);
}

// dst[i] = lut[src[i]], dst == src allowed (no __restrict__: every lane reads its bytes before it writes them).  `head` bytes in
// front of the first 16-byte boundary go one per lane (workgroup 0); VEC: src + head and dst + head are both 16-byte aligned and
// a lane moves one uint4 (the last, partial one byte by byte); !VEC (the two pointers differ modulo 16): the same chunk walk with
// one byte per lane and access, 16 accesses per step.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void label_lut_u8_kernel(const uint8_t* src, uint8_t* dst, int64_t n, int head,
                                                                const uint8_t* __restrict__ lut) {
    __shared__ uint8_t tab[256];
    load_label_table(tab, lut);
    if (blockIdx.x == 0 && (int)threadIdx.x < head) dst[threadIdx.x] = tab[src[threadIdx.x]];
    src += head; dst += head; n -= head;
    const int64_t nchunks = (n + kLutChunk - 1) / kLutChunk;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        if constexpr (VEC) {
            const int64_t o = c * kLutChunk + (int64_t)threadIdx.x * kLutVec;
            if (o + kLutVec <= n) {
                uint4 v = *reinterpret_cast<const uint4*>(src + o);
                v.x = lut4(tab, v.x); v.y = lut4(tab, v.y); v.z = lut4(tab, v.z); v.w = lut4(tab, v.w);
                *reinterpret_cast<uint4*>(dst + o) = v;
            } else {
                for (int64_t i = o; i < n; ++i) dst[i] = tab[src[i]];
            }
        } else {
#pragma unroll 4
            for (int j = 0; j < kLutVec; ++j) {
                const int64_t i = c * kLutChunk + j * kThreads + threadIdx.x;
                if (i < n) dst[i] = tab[src[i]];
            }
        }
    }
}

// dst[i] = (int64)lut[src[i]]: 1 byte read, 8 written.  A lane reads 16 bytes at once (src + head is 16-byte aligned), the
// looked-up bytes cross the wave through LDS so that every store instruction of a wave writes 64 consecutive int64 (512 bytes).
__global__ __launch_bounds__(kThreads) void label_encode_i64_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ lut,
                                                                    int64_t* __restrict__ dst, int64_t n, int head) {
    __shared__ uint8_t tab[256];
    __shared__ __attribute__((aligned(16))) uint8_t stage[kLutChunk];
    load_label_table(tab, lut);
    if (blockIdx.x == 0 && (int)threadIdx.x < head) dst[threadIdx.x] = (int64_t)tab[src[threadIdx.x]];
    src += head; dst += head; n -= head;
    const int64_t nchunks = (n + kLutChunk - 1) / kLutChunk;
    const int wave0 = ((int)threadIdx.x >> 6) * 64 * kLutVec, lane = (int)threadIdx.x & 63;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {          // the same trip count for every lane of the workgroup
        const int64_t base = c * kLutChunk;
        const int64_t o = base + (int64_t)threadIdx.x * kLutVec;
        if (o + kLutVec <= n) {
            uint4 v = *reinterpret_cast<const uint4*>(src + o);
            v.x = lut4(tab, v.x); v.y = lut4(tab, v.y); v.z = lut4(tab, v.z); v.w = lut4(tab, v.w);
            *reinterpret_cast<uint4*>(stage + threadIdx.x * kLutVec) = v;
        } else {
            for (int64_t i = o; i < n; ++i) stage[i - base] = tab[src[i]];
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < kLutVec; ++j) {
            const int e = wave0 + j * 64 + lane;
            if (base + e < n) dst[base + e] = (int64_t)stage[e];
        }
        __syncthreads();                                                  // the next step overwrites the stage
    }
}

// The assemble step of the validation transform (main.py:775-783: dataloaders.py:354-394 CenterCropPad, then ToTensor).  As
// input_assemble_kernel, with: a crop that may leave the padded image (such pixels are 0 in image and label, as Image.crop
// gives); `pad_label` for the pixels of the ImageOps.expand border; the label bytes looked up in `lut` as they are read.
__global__ __launch_bounds__(kThreads) void eval_assemble_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lab,
                                                                 const int32_t* __restrict__ ytab, const int32_t* __restrict__ xtab,
                                                                 int Hs, int Ws, int Hl, int Wl, int pad_x, int pad_y, int x1, int y1,
                                                                 int Hc, int Wc, int pad_label, const uint8_t* __restrict__ lut,
                                                                 float* __restrict__ out_img, int64_t* __restrict__ out_lab) {
    __shared__ uint8_t tab[256];
    load_label_table(tab, lut);
    const int64_t n = (int64_t)Hc * Wc;
    const int Wp = Ws + 2 * pad_x, Hp = Hs + 2 * pad_y;                 // the padded image
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const int ox = (int)(i % Wc), oy = (int)(i / Wc);
        const int qx = x1 + ox, qy = y1 + oy;                           // position in the padded image
        const int px = qx - pad_x, py = qy - pad_y;                     // position in the scaled image
        uint8_t r = 0, g = 0, b = 0;
        int64_t l = 0;                                                  // outside the padded image
        if (px >= 0 && px < Ws && py >= 0 && py < Hs) {
            const uint8_t* p = img + ((int64_t)py * Ws + px) * 3;
            r = p[0]; g = p[1]; b = p[2];
            const int sy = ytab[py], sx = xtab[px];
            if (sy >= 0 && sy < Hl && sx >= 0 && sx < Wl) l = tab[lab[(int64_t)sy * Wl + sx]];
        } else if (qx >= 0 && qx < Wp && qy >= 0 && qy < Hp) {
            l = pad_label;
        }
        out_img[i] = (float)r;
        out_img[n + i] = (float)g;
        out_img[2 * n + i] = (float)b;
        out_lab[i] = l;
    }
}

// ---- RandomRotate (dataloaders.py:153-165): Image.rotate(angle, BILINEAR) / mask.rotate(angle, NEAREST) -------------------
// Pillow (Geometry.c) maps every OUTPUT pixel back into the source with the six-coefficient matrix Image.rotate builds
// (mrfp_amd/input_pipeline.py::rotate_plan restates it).  The image takes ImagingGenericTransform: affine_transform in double at
// the pixel centre, bilinear_filter32RGB (columns x, x + 1 and row y clamped, row y + 1 only when it is inside, else v2 = v1;
// v = a + (b - a) * d in double, first along x, then along y; the result TRUNCATED to 8 bits).  The label takes affine_fixed:
// 16.16 fixed point, xin = (a2 + a1 y + a0 x) >> 16.  Outside pixels are 0 in both (the reference passes no fillcolor: the
// label's corners become class 0).  One lane per output pixel, image and label in one launch; `flip` reads the source mirrored
// (the reference flips before it rotates).  mode 0: the affine path; 1 copy, 2 ROTATE_90, 3 ROTATE_180, 4 ROTATE_270: the exact
// transposes Image.rotate dispatches to (90 / 270 on square images only).
struct AffineCoefs {
    double m[6];        // xin = m0 (x + .5) + m1 (y + .5) + m2, yin = m3 (x + .5) + m4 (y + .5) + m5
    int32_t a[6];       // the same in 16.16, a2 / a5 at the pixel centre
};

__device__ __forceinline__ int pil_floor(double v) { return v < 0.0 ? (int)floor(v) : (int)v; }       // Geometry.c FLOOR
__device__ __forceinline__ int pil_clip(int v, int n) { return v < 0 ? 0 : v < n ? v : n - 1; }          // XCLIP / YCLIP
__device__ __forceinline__ uint8_t pil_bilinear(const uint8_t* __restrict__ r0, const uint8_t* __restrict__ r1, int x0, int x1, int c,
                                                double dx, double dy) {
    const double a = (double)r0[3 * x0 + c], b = (double)r0[3 * x1 + c];
    const double v1 = a + (b - a) * dx;
    double v2 = v1;
    if (r1) {
        const double e = (double)r1[3 * x0 + c], f = (double)r1[3 * x1 + c];
        v2 = e + (f - e) * dx;
    }
    return (uint8_t)(int)(v1 + (v2 - v1) * dy);                  // (UINT8)v: truncation; 0 <= v <= 255
}

__global__ __launch_bounds__(kThreads) void affine_u8_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lab,
                                                             uint8_t* __restrict__ out_img, uint8_t* __restrict__ out_lab, int H, int W,
                                                             int mode, int flip, AffineCoefs A) {
    const int64_t n = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const int x = (int)(i % W), y = (int)(i / W);
        uint8_t r = 0, g = 0, b = 0, l = 0;
        if (mode == 0) {
            const double xc = (double)x + 0.5, yc = (double)y + 0.5;
            double xin = A.m[0] * xc + A.m[1] * yc + A.m[2];
            double yin = A.m[3] * xc + A.m[4] * yc + A.m[5];
            if (!(xin < 0.0 || xin >= (double)W || yin < 0.0 || yin >= (double)H)) {
                xin -= 0.5;
                yin -= 0.5;
                const int fx = pil_floor(xin), fy = pil_floor(yin);
                const double dx = xin - (double)fx, dy = yin - (double)fy;
                int x0 = pil_clip(fx, W), x1 = pil_clip(fx + 1, W);
                if (flip) { x0 = W - 1 - x0; x1 = W - 1 - x1; }
                const uint8_t* r0 = img + (int64_t)pil_clip(fy, H) * W * 3;
                const uint8_t* r1 = (fy + 1 >= 0 && fy + 1 < H) ? img + (int64_t)(fy + 1) * W * 3 : nullptr;
                r = pil_bilinear(r0, r1, x0, x1, 0, dx, dy);
                g = pil_bilinear(r0, r1, x0, x1, 1, dx, dy);
                b = pil_bilinear(r0, r1, x0, x1, 2, dx, dy);
            }
            // |every term| < 2^31 by the entry point's corner check; 64-bit sums keep the intermediate exact
            const int64_t xx = (int64_t)A.a[2] + (int64_t)A.a[1] * y + (int64_t)A.a[0] * x;
            const int64_t yy = (int64_t)A.a[5] + (int64_t)A.a[4] * y + (int64_t)A.a[3] * x;
            const int64_t sx = xx >> 16, sy = yy >> 16;          // arithmetic shifts
            if (sx >= 0 && sx < W && sy >= 0 && sy < H) l = lab[sy * W + (flip ? W - 1 - sx : sx)];
        } else {
            int sx, sy;                                          // Geometry.c ImagingRotate90 / 180 / 270 read backwards
            if (mode == 1) { sx = x; sy = y; }
            else if (mode == 2) { sx = W - 1 - y; sy = x; }
            else if (mode == 3) { sx = W - 1 - x; sy = H - 1 - y; }
            else { sx = y; sy = H - 1 - x; }
            if (flip) sx = W - 1 - sx;
            const uint8_t* p = img + ((int64_t)sy * W + sx) * 3;
            r = p[0]; g = p[1]; b = p[2];
            l = lab[(int64_t)sy * W + sx];
        }
        out_img[3 * i] = r; out_img[3 * i + 1] = g; out_img[3 * i + 2] = b;
        out_lab[i] = l;
    }
}

// Normalize (dataloaders.py:95-115) fused into the ToTensor store.  numpy evaluates `img /= 255.0` in float32 (a Python scalar
// does not widen the array) and `img -= mean`, `img /= std` -- mean and std are tuples, i.e. float64 arrays -- in float64, each
// rounded back to float32 when it is written into the float32 array.
__global__ __launch_bounds__(kThreads) void u8hwc_to_f32chw_norm_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                                        int64_t npix, double m0, double m1, double m2, double s0,
                                                                        double s1, double s2) {
    const double mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < npix; i += (int64_t)gridDim.x * kThreads) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = (float)src[3 * i + c] / 255.0f;
            v = (float)((double)v - mean[c]);
            v = (float)((double)v / sd[c]);
            dst[c * npix + i] = v;
        }
    }
}

// workgroups of a chunk walk: the cap of the row kernels (common.hpp: lines_per_image, MRFP_ROW_BLOCKS), every workgroup the
// same number of chunks; at least one, which moves the head bytes
inline unsigned lut_grid(int64_t nbytes) {
    const int64_t nchunks = (nbytes + kLutChunk - 1) / kLutChunk;
    return nchunks > 0 ? (unsigned)lines_per_image(1, nchunks) : 1u;
}

}  // namespace mrfp

using namespace mrfp;

extern "C" {

int mrfp_resample_u8(const void* src, void* dst, int64_t Hin, int64_t Win, int64_t Hout, int64_t Wout, int64_t C,
                     const int32_t* bounds, const int32_t* coefs, int ksize, int vertical, int flip, void* stream) {
    MRFP_CHECK(src && dst && bounds && coefs && ksize > 0, "resample_u8: null argument");
    MRFP_CHECK(Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && C > 0 && Hin < 65536 && Win < 65536 && Hout < 65536 && Wout < 65536,
               "resample_u8: bad sizes");
    MRFP_CHECK(vertical ? Wout == Win : Hout == Hin, "resample_u8: a pass changes one axis only (%s pass: %lldx%lld -> %lldx%lld)",
               vertical ? "vertical" : "horizontal", (long long)Hin, (long long)Win, (long long)Hout, (long long)Wout);
    MRFP_CHECK(!(vertical && flip), "resample_u8: the mirrored read belongs to the horizontal pass");
    const int64_t n = Hout * Wout * C;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(resample_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src,
                       (uint8_t*)dst, (int)Hin, (int)Win, (int)Hout, (int)Wout, (int)C, bounds, coefs, ksize, vertical, flip);
    MRFP_LAUNCH_CHECK();
    return 0;
}

int mrfp_input_assemble(const void* img, const void* lab, const int32_t* ytab, const int32_t* xtab, int64_t Hs, int64_t Ws,
                        int64_t Hl, int64_t Wl, int flip, int pad_x, int pad_y, int x1, int y1, int64_t Hc, int64_t Wc, int ignore,
                        float* out_img, void* out_u8, int64_t* out_lab, void* stream) {
    MRFP_CHECK(img && lab && ytab && xtab && (out_img || out_u8) && out_lab, "input_assemble: null argument");
    MRFP_CHECK(Hs > 0 && Ws > 0 && Hl > 0 && Wl > 0 && Hc > 0 && Wc > 0 && Hs < 65536 && Ws < 65536 && Hc < 65536 && Wc < 65536,
               "input_assemble: bad sizes");
    MRFP_CHECK(pad_x >= 0 && pad_y >= 0 && x1 >= 0 && y1 >= 0 && x1 + Wc <= Ws + 2 * pad_x && y1 + Hc <= Hs + 2 * pad_y,
               "input_assemble: the crop [%d,%d)+%lldx%lld leaves the padded image %lldx%lld", x1, y1, (long long)Wc, (long long)Hc,
               (long long)(Ws + 2 * pad_x), (long long)(Hs + 2 * pad_y));
    const int64_t n = Hc * Wc;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(input_assemble_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)img,
                       (const uint8_t*)lab, ytab, xtab, (int)Hs, (int)Ws, (int)Hl, (int)Wl, flip, pad_x, pad_y, x1, y1, (int)Hc, (int)Wc,
                       ignore, out_img, (uint8_t*)out_u8, out_lab);
    MRFP_LAUNCH_CHECK();
    return 0;
}

int mrfp_box_blur3_u8(const void* src, void* dst, int64_t H, int64_t W, int64_t C, int64_t ww, int64_t fw, int vertical,
                      void* stream) {
    MRFP_CHECK(src && dst && src != dst && H > 0 && W > 0 && C > 0 && H < 65536 && W < 65536, "box_blur3_u8: bad arguments");
    MRFP_CHECK(ww > 0 && fw >= 0 && ww + 2 * fw <= (1ll << 24), "box_blur3_u8: weights %lld + 2*%lld exceed 2^24 (box radius >= 1?)",
               (long long)ww, (long long)fw);
    const int64_t n = H * W * C;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(box_blur3_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src,
                       (uint8_t*)dst, (int)H, (int)W, (int)C, (unsigned)ww, (unsigned)fw, vertical);
    MRFP_LAUNCH_CHECK();
    return 0;
}

int mrfp_jitter_u8(const void* src, void* dst, int64_t npix, int op, float factor, int shift, void* ws, void* stream) {
    MRFP_CHECK(src && dst && npix > 0 && op >= 0 && op <= 3, "jitter_u8: bad arguments (op 0..3)");
    MRFP_CHECK(op != 1 || ws, "jitter_u8: the contrast op needs 16 bytes of workspace");
    MRFP_CHECK(op != 3 || (shift >= 0 && shift < 256), "jitter_u8: hue shift must be in 0..255");
    hipStream_t st = (hipStream_t)stream;
    int64_t blocks = (npix + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    int* gray = nullptr;
    if (op == 1) {
        unsigned long long* sum = (unsigned long long*)ws;
        gray = (int*)((char*)ws + 8);
        if (hipMemsetAsync(sum, 0, 8, st) != hipSuccess) { set_error("jitter_u8: hipMemsetAsync failed"); return -1; }
        hipLaunchKernelGGL(gray_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const uint8_t*)src, npix, sum);
        hipLaunchKernelGGL(gray_mean_kernel, dim3(1), dim3(1), 0, st, (const unsigned long long*)sum, npix, gray);
    }
    hipLaunchKernelGGL(jitter_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const uint8_t*)src, (uint8_t*)dst, npix, op, factor,
                       shift, (const int*)gray);
    MRFP_LAUNCH_CHECK();
    return 0;
}

int mrfp_u8hwc_to_f32chw(const void* src, float* dst, int64_t H, int64_t W, void* stream) {
    MRFP_CHECK(src && dst && H > 0 && W > 0, "u8hwc_to_f32chw: bad arguments");
    const int64_t n = H * W;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(u8hwc_to_f32chw_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, dst, n);
    MRFP_LAUNCH_CHECK();
    return 0;
}

int mrfp_label_lut_u8(const void* src, void* dst, int64_t n, const void* lut, void* stream) {
    MRFP_CHECK(src && dst && lut, "label_lut_u8: null argument");
    MRFP_CHECK(n >= 0, "label_lut_u8: negative size %lld", (long long)n);
    const uint8_t* s = (const uint8_t*)src;
    uint8_t* d = (uint8_t*)dst;
    const uintptr_t sa = reinterpret_cast<uintptr_t>(s), da = reinterpret_cast<uintptr_t>(d);
    MRFP_CHECK(sa == da || (sa < da ? da - sa : sa - da) >= (uint64_t)n, "label_lut_u8: src and dst overlap (in place means dst == src)");
    if (n == 0) return 0;
    const bool vec = ((reinterpret_cast<uintptr_t>(s) ^ reinterpret_cast<uintptr_t>(d)) & 15) == 0;
    int64_t head = vec ? (int64_t)((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15) : 0;
    if (head > n) head = n;
    const dim3 grid(lut_grid(n - head));
    if (vec) hipLaunchKernelGGL(label_lut_u8_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, s, d, n, (int)head, (const uint8_t*)lut);
    else hipLaunchKernelGGL(label_lut_u8_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, s, d, n, (int)head, (const uint8_t*)lut);
    MRFP_LAUNCH_CHECK();
    return 0;
}

int mrfp_label_encode_i64(const void* src_u8, const void* lut, int64_t* dst_i64, int64_t n, void* stream) {
    MRFP_CHECK(src_u8 && dst_i64, "label_encode_i64: null argument");
    MRFP_CHECK(n >= 0, "label_encode_i64: negative size %lld", (long long)n);
    MRFP_CHECK((reinterpret_cast<uintptr_t>(dst_i64) & 7) == 0, "label_encode_i64: dst_i64 is not 8-byte aligned");
    if (n == 0) return 0;
    int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(src_u8) & 15)) & 15);
    if (head > n) head = n;
    hipLaunchKernelGGL(label_encode_i64_kernel, dim3(lut_grid(n - head)), dim3(kThreads), 0, (hipStream_t)stream, (const uint8_t*)src_u8,
                       (const uint8_t*)lut, dst_i64, n, (int)head);
    MRFP_LAUNCH_CHECK();
    return 0;
}

int mrfp_eval_assemble(const void* img, const void* lab, const int32_t* ytab, const int32_t* xtab, int64_t Hs, int64_t Ws, int64_t Hl,
                       int64_t Wl, int pad_x, int pad_y, int x1, int y1, int64_t Hc, int64_t Wc, int pad_label, const void* lut,
                       float* out_img, int64_t* out_lab, void* stream) {
    MRFP_CHECK(img && lab && ytab && xtab && out_img && out_lab, "eval_assemble: null argument");
    MRFP_CHECK(Hs > 0 && Ws > 0 && Hl > 0 && Wl > 0 && Hc > 0 && Wc > 0 && Hs < 65536 && Ws < 65536 && Hl < 65536 && Wl < 65536 &&
               Hc < 65536 && Wc < 65536, "eval_assemble: bad sizes");
    MRFP_CHECK(pad_x >= 0 && pad_y >= 0, "eval_assemble: negative padding (%d, %d)", pad_x, pad_y);
    MRFP_CHECK(pad_label >= 0 && pad_label <= 255, "eval_assemble: pad_label %d is no uint8 value", pad_label);
    // the kernel's 32-bit positions: the padded extent, the crop's far corner and the crop origin taken back by the padding
    const int64_t lim = 2147483647ll;
    MRFP_CHECK(Ws + 2 * (int64_t)pad_x <= lim && Hs + 2 * (int64_t)pad_y <= lim && (int64_t)x1 + Wc <= lim && (int64_t)y1 + Hc <= lim &&
               (int64_t)x1 - pad_x >= -lim && (int64_t)y1 - pad_y >= -lim,
               "eval_assemble: the crop [%d,%d)+%lldx%lld or the padding (%d, %d) overflows int32", x1, y1, (long long)Wc, (long long)Hc,
               pad_x, pad_y);
    const int64_t n = Hc * Wc;
    int64_t blocks = (n + kThreads - 1) / kThreads;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(eval_assemble_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, (const uint8_t*)img,
                       (const uint8_t*)lab, ytab, xtab, (int)Hs, (int)Ws, (int)Hl, (int)Wl, pad_x, pad_y, x1, y1, (int)Hc, (int)Wc, pad_label,
                       (const uint8_t*)lut, out_img, out_lab);
    MRFP_LAUNCH_CHECK();
    return 0;
}

int mrfp_affine_u8(const void* img, const void* lab, void* out_img, void* out_lab, int64_t H, int64_t W, int mode, int flip,
                   double m0, double m1, double m2, double m3, double m4, double m5, void* stream) {
    MRFP_CHECK(img && lab && out_img && out_lab && img != out_img && lab != out_lab, "affine_u8: null or aliased argument");
    MRFP_CHECK(H > 0 && W > 0 && H < 65536 && W < 65536, "affine_u8: bad sizes %lldx%lld", (long long)H, (long long)W);
    MRFP_CHECK(mode >= 0 && mode <= 4, "affine_u8: mode %d (0 affine, 1 copy, 2 / 3 / 4 the 90 / 180 / 270 degree transposes)", mode);
    MRFP_CHECK(!(mode == 2 || mode == 4) || H == W, "affine_u8: the 90 / 270 degree transposes keep the size of square images only (%lldx%lld)",
               (long long)H, (long long)W);
    AffineCoefs A{};
    if (mode == 0) {
        const double m[6] = {m0, m1, m2, m3, m4, m5};
        // Geometry.c ImagingTransformAffine: the fixed-point path holds while all four corners stay below 32768
        const double w = (double)W, h = (double)H;
        const double cx[4] = {0.0, w, 0.0, w}, cy[4] = {0.0, h, h, 0.0};
        for (int k = 0; k < 4; ++k) {
            const double px = cx[k] * m[0] + cy[k] * m[1] + m[2], py = cx[k] * m[3] + cy[k] * m[4] + m[5];
            MRFP_CHECK(std::isfinite(px) && std::isfinite(py) && fabs(px) < 32768.0 && fabs(py) < 32768.0,
                       "affine_u8: a corner of the %lldx%lld image maps to (%g, %g): outside the 16.16 fixed-point range (< 32768)",
                       (long long)W, (long long)H, px, py);
        }
        const double c[6] = {m[0], m[1], m[2] + m[0] * 0.5 + m[1] * 0.5, m[3], m[4], m[5] + m[3] * 0.5 + m[4] * 0.5};
        for (int k = 0; k < 6; ++k) {
            const double f = floor(c[k] * 65536.0 + 0.5);        // FIX(v): FLOOR(v * 65536 + 0.5)
            MRFP_CHECK(fabs(f) < 2147483648.0, "affine_u8: coefficient %g does not fit 16.16 fixed point", c[k]);
            A.m[k] = m[k];
            A.a[k] = (int32_t)f;
        }
    }
    const int64_t n = H * W;
    int64_t blocks = (n + kThreads - 1) / kThreads;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(affine_u8_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, (const uint8_t*)img,
                       (const uint8_t*)lab, (uint8_t*)out_img, (uint8_t*)out_lab, (int)H, (int)W, mode, flip != 0, A);
    MRFP_LAUNCH_CHECK();
    return 0;
}

int mrfp_u8hwc_to_f32chw_norm(const void* src, float* dst, int64_t H, int64_t W, double mean0, double mean1, double mean2,
                              double std0, double std1, double std2, void* stream) {
    MRFP_CHECK(src && dst && H > 0 && W > 0, "u8hwc_to_f32chw_norm: bad arguments");
    MRFP_CHECK(std::isfinite(mean0) && std::isfinite(mean1) && std::isfinite(mean2) && std::isfinite(std0) && std::isfinite(std1) &&
               std::isfinite(std2) && std0 != 0.0 && std1 != 0.0 && std2 != 0.0,
               "u8hwc_to_f32chw_norm: finite means and finite non-zero standard deviations expected");
    const int64_t n = H * W;
    int64_t blocks = (n + kThreads - 1) / kThreads;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(u8hwc_to_f32chw_norm_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, (const uint8_t*)src, dst, n,
                       mean0, mean1, mean2, std0, std1, std2);
    MRFP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
