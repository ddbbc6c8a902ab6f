#include "conv_common.hpp"

// =============================================================================================
// wgrad:  dW[n, (r,s,c)] = sum_m dY[m, n] * X[pix(m; r,s), c]          (reduction over pixels)
//
// GEMM with M' = output channels, N' = R*S*C, K' = B*Ho*Wo.  Both operands are stored with the
// reduction index (the pixel) as the SLOW dimension, i.e. they are "k-strided": the LDS tiles
// keep the natural [pixel][channel] layout (filled with 16-byte loads along the channels) and the
// MFMA fragments are formed with the gfx950 transposing LDS read ds_read_b64_tr_b16 (bf16) or
// with plain strided ds_read_b32 (fp32).  Row pitch = row bytes + 64 so that the four pixel rows
// of one transposed read fall into four disjoint 16-bank windows.
// K' is split over gridDim.y workgroups; every split writes an fp32 slab, a second kernel sums
// the slabs in a fixed order (bitwise reproducible) and emits the OIHW fp32 gradient.
// =============================================================================================
namespace mrfp {

MRFP_STAMP_DECL(g_stamps_wgrad)
int stamps_wgrad(unsigned long long* out, int n) { return MRFP_STAMP_READ(g_stamps_wgrad, out, n); }

typedef __attribute__((ext_vector_type(4))) short short4v;
typedef __attribute__((address_space(3))) short4v lds_short4v;

struct FastDiv {     // exact n / d for 0 <= n < 2^31:  q = (n * m) >> (31 + l),  m = floor(2^(31+l)/d) + 1
    unsigned m, sh;
};
static FastDiv make_fastdiv(unsigned d) {
    unsigned l = 0;
    while ((1u << l) < d) ++l;
    FastDiv f;
    f.m = (unsigned)(((1ull << (31 + l)) / d) + 1);
    f.sh = 31 + l;
    return f;
}
__device__ __forceinline__ int fdiv(int n, const FastDiv& f) { return (int)(((unsigned long long)(unsigned)n * f.m) >> f.sh); }

struct WgP {
    const char* x;    // [B,H,W,C]
    const char* dy;   // [M][ldn]
    float* slab;      // [splits][N][Q]
    int B, H, W, C;
    int N, ldn;       // logical output channels, physical pitch of dy (elements)
    int R, S, Ho, Wo, stride, pad_h, pad_w, dil;
    int M, Q;         // pixels, R*S*C
    int klen;         // pixels per split (multiple of the K' tile)
    int tiles;        // output tiles per split
    int splits;       // K' splits per problem
    int ngroup;       // problems in this launch (1: x / dy / slab above; > 1: WgGroup below, slabs back to back)
    unsigned xbytes, dybytes;
    FastDiv div_hw, div_w;   // by Ho*Wo and by Wo
};

// GROUPED launch: up to kWgMaxGroup weight-gradient problems of ONE geometry (the repeated blocks of a ResNet stage:
// reference network/Resnet.py:579-585 _make_layer) in one grid.  The operand pointers travel in the kernel arguments (WgGroup,
// conv_common.hpp: no device-side table, no copy, graph-capturable); the work index is problem-major, so with the XCD-chunked order
// the tiles of one problem share one L2.  22x the tiles of a layer-3 launch means 2-3 K' splits instead of 21-32: K' loops of ~190
// tiles per workgroup instead of 12 behind the same prologue, and 1/10 of the fp32 slab traffic.
struct WgOut {
    float* dw[kWgMaxGroup];
};

template <typename T> struct WgFrag;
template <> struct WgFrag<bf16> {
    // 32(rows along the lane) x 16(k) operand from a [pixel][channel] tile; col0 = first channel of
    // the 32-column block, krow0 = first pixel row of this 16-deep k step
    static __device__ __forceinline__ uint4 read(const char* tile, int pitch, int col0, int krow0, int lane) {
        const int g = lane >> 4;
        const int col = col0 + 16 * (g & 1) + 4 * (lane & 3);
        const int row = krow0 + 8 * (g >> 1) + ((lane & 15) >> 2);
        const char* p0 = tile + row * pitch + col * 2;
        const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4v*)(p0));
        const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4v*)(p0 + 4 * pitch));
        uint4 r;
        r.x = (unsigned)(unsigned short)lo[0] | ((unsigned)(unsigned short)lo[1] << 16);
        r.y = (unsigned)(unsigned short)lo[2] | ((unsigned)(unsigned short)lo[3] << 16);
        r.z = (unsigned)(unsigned short)hi[0] | ((unsigned)(unsigned short)hi[1] << 16);
        r.w = (unsigned)(unsigned short)hi[2] | ((unsigned)(unsigned short)hi[3] << 16);
        return r;
    }
    static constexpr int KSTEP = 16;   // pixels consumed per Mma<bf16>::run
};
template <> struct WgFrag<f16> : WgFrag<bf16> {};     // same 16-bit transposing LDS read

// LDS-DMA tile layout of the 16-bit wgrad operands: rows of NB 64-byte blocks with NO padding (a DMA piece is 1 KiB of
// contiguous LDS); block lb of row r sits at physical block lb ^ key(r), key = r & 3 (NB >= 4) or (r >> 1) & 1 (NB == 2),
// so that the four pixel rows of one transposing read still fall into four disjoint 64-byte bank windows.
template <int NB> __device__ __forceinline__ int wg_key(int row) { return NB >= 4 ? (row & 3) : NB == 2 ? ((row >> 1) & 1) : 0; }
template <int NB>
__device__ __forceinline__ uint4 wg_read_sw(const char* tile, int col0, int krow0, int lane) {
    const int g = lane >> 4;
    const int row = krow0 + 8 * (g >> 1) + ((lane & 15) >> 2);
    const char* p0 = tile + row * (NB * 64) + (((col0 >> 5) ^ wg_key<NB>(row)) << 6) + 32 * (g & 1) + 8 * (lane & 3);
    const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4v*)(p0));
    const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4v*)(p0 + 4 * NB * 64));   // row + 4: same key
    uint4 r;
    r.x = (unsigned)(unsigned short)lo[0] | ((unsigned)(unsigned short)lo[1] << 16);
    r.y = (unsigned)(unsigned short)lo[2] | ((unsigned)(unsigned short)lo[3] << 16);
    r.z = (unsigned)(unsigned short)hi[0] | ((unsigned)(unsigned short)hi[1] << 16);
    r.w = (unsigned)(unsigned short)hi[2] | ((unsigned)(unsigned short)hi[3] << 16);
    return r;
}
template <> struct WgFrag<float> {
    // 4 MFMA 32x32x2 per call: element j of lane-half h is pixel krow0 + 2*j + h
    static __device__ __forceinline__ uint4 read(const char* tile, int pitch, int col0, int krow0, int lane) {
        const int c = col0 + (lane & 31), h = lane >> 5;
        uint4 r;
        r.x = *reinterpret_cast<const unsigned*>(tile + (krow0 + 0 + h) * pitch + c * 4);
        r.y = *reinterpret_cast<const unsigned*>(tile + (krow0 + 2 + h) * pitch + c * 4);
        r.z = *reinterpret_cast<const unsigned*>(tile + (krow0 + 4 + h) * pitch + c * 4);
        r.w = *reinterpret_cast<const unsigned*>(tile + (krow0 + 6 + h) * pitch + c * 4);
        return r;
    }
    static constexpr int KSTEP = 8;
};

#ifndef MRFP_WGRAD_HOLD
#define MRFP_WGRAD_HOLD 2      // k steps (of 4 per K' tile) multiplied after the next tile's transfer has been issued
#endif
#ifndef MRFP_WGRAD_HOLD_BIG
#define MRFP_WGRAD_HOLD_BIG 2  // the same for the 256 x 128 tile
#endif
template <typename T> struct WgTile { static constexpr int BKP = 64; };   // pixels per K' tile
template <> struct WgTile<float> { static constexpr int BKP = 32; };

// DENSE: pointwise convolution (1x1, stride 1, no padding): X is a dense [pixel][channel] matrix like dY, so its slots advance
// by a constant and need no (ih, iw) bookkeeping -- 60 of the 85 VALU and 40 of the 64 SALU instructions of a K' tile in
// the general kernel, on layers (M = 36 864 bottleneck 1x1) that are bound by exactly that instruction stream
// (profiles/r02_experiments.md section 4: 31 us with or without any global traffic, MFMA time 11 us).
// TMB: 32-row accumulator blocks per wave along the output channels.  2 = the 128 x 128 workgroup tile (64 FLOP per fill byte, four
// workgroups per CU); 4 = a 256 x 128 tile (85 FLOP per fill byte, 6 fragment reads per 8 MFMAs instead of 4 per 4; 128 accumulator
// registers, two workgroups per CU) for the layers with N % 256 == 0 and long K' loops -- the grouped launches above all.
template <typename T, int WM, int WN, bool DMA, bool DENSE = false, int TMB = 2>
__global__ __launch_bounds__(256, (TMB == 4 ? 2 : DMA ? 4 : 3)) void conv_wgrad_kernel(WgP p, WgGroup grp) {   // 2nd = waves per SIMD
    static_assert(WM * WN == 4, "4 waves");
    static_assert(!DMA || sizeof(T) == 2, "LDS-DMA layout is for the 16-bit types");
    static_assert(TMB == 2 || (TMB == 4 && DMA && WM == 2), "the 256 x 128 tile is an LDS-DMA kernel");
    constexpr int BKP = WgTile<T>::BKP;
    constexpr int EPC = 16 / (int)sizeof(T);                 // elements per 16-byte chunk
    constexpr int BNN = 32 * TMB * WM;                       // output channels per workgroup tile
    constexpr int CY = BNN / EPC, CX = 64 * WN / EPC;        // chunks per tile row
    constexpr int SY = BKP * CY / 256, SX = BKP * CX / 256;  // slots per thread
    constexpr int PY = BNN * (int)sizeof(T) + (DMA ? 0 : 64), PX = 64 * WN * (int)sizeof(T) + (DMA ? 0 : 64);   // row pitches
    constexpr int NBY = BNN * (int)sizeof(T) / 64, NBX = 2 * WN;    // 64-byte blocks per row (DMA layout)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const ty = smem;               // single LDS buffer: the next tile waits in registers
    char* const tx = smem + BKP * PY;
    MRFP_STAMP_BEGIN();

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave / WN, wn = wave % WN;
    typedef __attribute__((address_space(3))) void lds_void;
    const int wave1k = __builtin_amdgcn_readfirstlane(wave) * 1024;      // this wave's first DMA piece (1 KiB each)
    const int ntq = (p.Q + 64 * WN - 1) / (64 * WN);
    // 1-D grid over (split, tile), split-major, dealt to the XCDs in contiguous chunks: the tiles of one split read the
    // same pixel range of x and dy, so they share one L2 instead of pulling those rows into all eight
    int work = xcd_remap(blockIdx.x, gridDim.x);
    const char* xbase = p.x;
    const char* dybase = p.dy;
    int prob = 0;
    if (p.ngroup > 1) {              // (uniform) problem-major work order
        const int per = p.tiles * p.splits;
        prob = work / per;
        work -= prob * per;
        xbase = grp.x[prob];
        dybase = grp.dy[prob];
    }
    const int split = work / p.tiles, tile = work - split * p.tiles;
    const int n0 = (tile / ntq) * BNN, q0 = (tile % ntq) * 64 * WN;
    const int kbeg = split * p.klen;
    const int kend = min(p.M, kbeg + p.klen);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)xbase, 0, (int)p.xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc((void*)dybase, 0, (int)p.dybytes, 0x00020000);

    // dY slots: dense rows; column fixed per thread
    const int yrow = t / CY;
    // DMA: this thread's LDS slot is fixed (piece base + lane * 16); the SOURCE chunk it fetches is the swizzled one
    const int ychunk = DMA ? ((((t % CY) >> 2) ^ wg_key<NBY>(yrow)) << 2) | ((t % CY) & 3) : t % CY;
    const int yn = n0 + ychunk * EPC;
    const unsigned ycol = yn < p.ldn ? (unsigned)yn * (unsigned)sizeof(T) : kOOB;
    const unsigned yrowbytes = (unsigned)p.ldn * (unsigned)sizeof(T);
    // X slots: fixed tap / channel per thread; the pixel moves by one K' tile per trip.  Its source coordinates
    // (ih, iw) and byte offset are advanced incrementally with adds / selects only (no multiply, no divide).
    const int xrow = t / CX;
    const int xchunk = DMA ? ((((t % CX) >> 2) ^ wg_key<NBX>(xrow)) << 2) | ((t % CX) & 3) : t % CX;
    const int q = q0 + xchunk * EPC;
    const int rs = q / p.C, c = q - rs * p.C;
    const int r = rs / p.S, s = rs - r * p.S;
    const int dh = r * p.dil - p.pad_h, dw = s * p.dil - p.pad_w;
    const bool xcol_ok = q < p.Q;
    const int pixbytes = p.C * (int)sizeof(T);
    const int st = p.stride;
    const int qh = BKP / p.Wo, rw = BKP - qh * p.Wo;                       // one K' tile = qh rows + rw pixels
    const int d_iw = rw * st, d_ih = qh * st;
    const unsigned D0 = (unsigned)((d_ih * p.W + d_iw) * pixbytes);        // plain advance
    const unsigned D1 = (unsigned)((st * p.W - p.Wo * st) * pixbytes);     // output-row wrap
    const unsigned D2 = (unsigned)((p.H * p.W - p.Ho * st * p.W) * pixbytes);   // image wrap
    const int iw_lim = p.Wo * st + dw, ih_lim = p.Ho * st + dh, WoSt = p.Wo * st, HoSt = p.Ho * st;
    int x_ih[SX], x_iw[SX];
    unsigned x_off[SX];
#pragma unroll
    for (int i = 0; i < SX; ++i) {
        const int m = kbeg + xrow + i * (256 / CX);
        if constexpr (DENSE) {
            x_ih[i] = 0;
            x_iw[i] = 0;
            x_off[i] = (unsigned)m * (unsigned)pixbytes + (unsigned)c * (unsigned)sizeof(T);
        } else {
            const int b = m / (p.Ho * p.Wo), rem = m - b * (p.Ho * p.Wo);
            const int oh = rem / p.Wo, ow = rem - oh * p.Wo;
            x_ih[i] = oh * st + dh;
            x_iw[i] = ow * st + dw;
            x_off[i] = (unsigned)((b * p.H + x_ih[i]) * p.W + x_iw[i]) * (unsigned)pixbytes + (unsigned)c * (unsigned)sizeof(T);
        }
    }
    const unsigned x_step = (unsigned)BKP * (unsigned)pixbytes;
    unsigned y_off[SY];
#pragma unroll
    for (int i = 0; i < SY; ++i) y_off[i] = (unsigned)(kbeg + yrow + i * (256 / CY)) * yrowbytes + ycol;
    const unsigned y_step = (unsigned)BKP * yrowbytes;

    auto load_tile = [&](int k0, uint4 (&ry)[SY], uint4 (&rx)[SX]) {
#pragma unroll
        for (int i = 0; i < SY; ++i) {
            const int m = k0 + yrow + i * (256 / CY);
            const unsigned voff = (m < kend && ycol < kOOB) ? y_off[i] : kOOB;
            if (DMA)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(yr, (lds_void*)(ty + (wave1k + i * 4096)), 16, (int)voff, 0, 0, 0);
            else
                ry[i] = bload(yr, voff);
            y_off[i] += y_step;
        }
#pragma unroll
        for (int i = 0; i < SX; ++i) {
            const int m = k0 + xrow + i * (256 / CX);
            const bool ok = DENSE ? (xcol_ok && m < kend)
                                  : (xcol_ok && m < kend && (unsigned)x_ih[i] < (unsigned)p.H && (unsigned)x_iw[i] < (unsigned)p.W);
            if (DMA)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_void*)(tx + (wave1k + i * 4096)), 16,
                                                         (int)(ok ? x_off[i] : kOOB), 0, 0, 0);
            else
                rx[i] = bload(xr, ok ? x_off[i] : kOOB);
            // advance this slot by one K' tile
            if constexpr (DENSE) {
                x_off[i] += x_step;
            } else {
                x_iw[i] += d_iw;
                x_ih[i] += d_ih;
                x_off[i] += D0;
                if (x_iw[i] >= iw_lim) { x_iw[i] -= WoSt; x_ih[i] += st; x_off[i] += D1; }
                while (x_ih[i] >= ih_lim) { x_ih[i] -= HoSt; x_off[i] += D2; }
            }
        }
    };
    auto store_tile = [&](const uint4 (&ry)[SY], const uint4 (&rx)[SX]) {
#pragma unroll
        for (int i = 0; i < SY; ++i) *reinterpret_cast<uint4*>(ty + (yrow + i * (256 / CY)) * PY + ychunk * 16) = ry[i];
#pragma unroll
        for (int i = 0; i < SX; ++i) *reinterpret_cast<uint4*>(tx + (xrow + i * (256 / CX)) * PX + xchunk * 16) = rx[i];
    };

    f32x16 acc[TMB][2];
#pragma unroll
    for (int i = 0; i < TMB; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int nkt = (kend - kbeg + BKP - 1) / BKP;
    // one K' tile of register prefetch (a second register set was measured: it costs a wave of occupancy and
    // runs 35 % slower -- three co-resident workgroups per CU hide the load latency better)
    uint4 ry[SY], rx[SX];
    if (DMA) {
        // single LDS buffer filled by LDS-DMA (as the forward kernel, mode 3): no staging registers, no ds_write
        // EARLY ISSUE (as in conv_igemm_kernel): the fragments of the last HOLD k steps go to registers, a barrier frees the
        // buffer, the next tile's transfer is issued and the held k steps are multiplied inside its latency.
        constexpr int KSN = BKP / 16;
        constexpr int HOLD = (!DENSE && WM == 1) ? 1 : TMB == 4 ? MRFP_WGRAD_HOLD_BIG : MRFP_WGRAD_HOLD;     // (the 64x256 gather variant spills with two held k steps)
        if (nkt > 0) load_tile(kbeg, ry, rx);
        for (int kt = 0; kt < nkt; ++kt) {
            dma_wait<0>();            // explicit: across the back edge the compiler's own wait lands behind the barrier
            __syncthreads();          // the tile has landed everywhere
#pragma unroll
            for (int ks = 0; ks < KSN - HOLD; ++ks) {
                uint4 fa[TMB], fb[2];
#pragma unroll
                for (int i = 0; i < TMB; ++i) fa[i] = wg_read_sw<NBY>(ty, wm * 32 * TMB + i * 32, ks * 16, lane);
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[j] = wg_read_sw<NBX>(tx, wn * 64 + j * 32, ks * 16, lane);
#pragma unroll
                for (int i = 0; i < TMB; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) Mma<T>::run(acc[i][j], fa[i], fb[j]);
            }
            uint4 ha[HOLD > 0 ? HOLD : 1][TMB], hb[HOLD > 0 ? HOLD : 1][2];
#pragma unroll
            for (int h = 0; h < HOLD; ++h) {
#pragma unroll
                for (int i = 0; i < TMB; ++i) ha[h][i] = wg_read_sw<NBY>(ty, wm * 32 * TMB + i * 32, (KSN - HOLD + h) * 16, lane);
#pragma unroll
                for (int j = 0; j < 2; ++j) hb[h][j] = wg_read_sw<NBX>(tx, wn * 64 + j * 32, (KSN - HOLD + h) * 16, lane);
            }
            __syncthreads();          // lgkmcnt(0) + barrier: everybody is done reading, the buffer is free
            if (kt + 1 < nkt) load_tile(kbeg + (kt + 1) * BKP, ry, rx);
#pragma unroll
            for (int h = 0; h < HOLD; ++h)
#pragma unroll
                for (int i = 0; i < TMB; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) Mma<T>::run(acc[i][j], ha[h][i], hb[h][j]);
        }
    } else {
    if (nkt > 0) {
        load_tile(kbeg, ry, rx);
        store_tile(ry, rx);
    }
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt + 1 < nkt) load_tile(kbeg + (kt + 1) * BKP, ry, rx);
#pragma unroll
        for (int ks = 0; ks < BKP / WgFrag<T>::KSTEP; ++ks) {
            uint4 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = WgFrag<T>::read(ty, PY, wm * 64 + i * 32, ks * WgFrag<T>::KSTEP, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = WgFrag<T>::read(tx, PX, wn * 64 + j * 32, ks * WgFrag<T>::KSTEP, lane);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) Mma<T>::run(acc[i][j], fa[i], fb[j]);
        }
        __syncthreads();
        if (kt + 1 < nkt) store_tile(ry, rx);
        __syncthreads();
    }
    }

    MRFP_STAMP_END(g_stamps_wgrad);
    float* out = p.slab + ((size_t)prob * p.splits + split) * p.N * p.Q;
    const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int qq = q0 + wn * 64 + j * 32 + lr;
        if (qq >= p.Q) continue;
#pragma unroll
        for (int i = 0; i < TMB; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int n = n0 + wm * 32 * TMB + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (n < p.N) out[(size_t)n * p.Q + qq] = acc[i][j][e];
            }
    }
}

// dW[n][c][r][s] (OIHW fp32, c < Ctrue) = sum_z slab[z][n][(r*S+s)*C + c]
// One workgroup = 64 consecutive float4 of the slab order (1 KB runs: the slabs are ~20-30x the size of dW, so their reads are
// the ones that must coalesce) x 4 slab groups: wave g sums the slabs z = g, g + 4, g + 8, ... in ascending order with eight
// independent 16-byte loads in flight per lane, the four group sums are combined through LDS as (g0 + g1) + (g2 + g3) -- a fixed
// association, so the result is bitwise reproducible.  (Round 2 walked all slabs of an output in ONE thread, four loads in
// flight: 14 us per launch for 30-60 MB that the chip reads in 6; a last-arriving-workgroup reduction inside conv_wgrad_kernel
// was considered and not built -- the arriver of a tile would pull splits x 64 KB through ONE compute unit behind a ~3.5 us
// device-scope fence, MI355X_MICROARCH.md -- DESIGN.md section 4.)  The OIHW stores are 4-byte scattered but few.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slab, int splits, int N, int Q, int C, int Ctrue, int RS,
                                                            float* __restrict__ dw, int accumulate, WgOut outs) {
    __shared__ float4 part[4][64];
    const int o = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int64_t total4 = (int64_t)N * Q / 4, NQ = (int64_t)N * Q;
    if (gridDim.y > 1) {             // grouped launch: problem blockIdx.y, its slabs back to back
        slab += (size_t)blockIdx.y * splits * NQ;
        dw = outs.dw[blockIdx.y];
    }
    const int64_t i = (int64_t)blockIdx.x * 64 + o;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < total4) {
        const float* base = slab + i * 4;
        int z = g;
        for (; z + 28 < splits; z += 32) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(base + (size_t)(z + 4 * u) * NQ);
#pragma unroll
            for (int u = 0; u < 8; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
        }
        for (; z < splits; z += 4) {
            const float4 v = *reinterpret_cast<const float4*>(base + (size_t)z * NQ);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
    }
    part[g][o] = acc;
    __syncthreads();
    if (g != 0 || i >= total4) return;
    const float4 p0 = part[0][o], p1 = part[1][o], p2 = part[2][o], p3 = part[3][o];
    acc.x = (p0.x + p1.x) + (p2.x + p3.x);
    acc.y = (p0.y + p1.y) + (p2.y + p3.y);
    acc.z = (p0.z + p1.z) + (p2.z + p3.z);
    acc.w = (p0.w + p1.w) + (p2.w + p3.w);
    const int64_t j = i * 4;
    const int n = (int)(j / Q), q = (int)(j - (int64_t)n * Q);
    const int rs = q / C, c = q - rs * C;
    if (c >= Ctrue) return;
    float* d = dw + ((size_t)n * Ctrue + c) * RS + rs;
    if (accumulate) {            // a later batch range of an activation that is read in several launches
        acc.x += d[0];
        if (c + 1 < Ctrue) acc.y += d[RS];
        if (c + 2 < Ctrue) acc.z += d[2 * RS];
        if (c + 3 < Ctrue) acc.w += d[3 * RS];
    }
    d[0] = acc.x;
    if (c + 1 < Ctrue) d[RS] = acc.y;
    if (c + 2 < Ctrue) d[2 * RS] = acc.z;
    if (c + 3 < Ctrue) d[3 * RS] = acc.w;
}

template <typename T, int WM, int WN, bool DMA, bool DENSE = false, int TMB = 2>
static int launch_wgrad_v(const WgP& p, const WgradPlan& pl, hipStream_t st, const WgGroup* grp) {
    constexpr int BNN = 32 * TMB * WM;
    constexpr int PY = BNN * (int)sizeof(T) + (DMA ? 0 : 64), PX = 64 * WN * (int)sizeof(T) + (DMA ? 0 : 64);
    // MRFP_WGRAD_LDS=<bytes> (experiments: tools/overlap_micro.py): ask for at least that much LDS per workgroup, i.e. cap the
    // workgroups per CU below what the registers allow (81920: one per CU) -- how much of a concurrent HBM-bound kernel's time
    // a weight-gradient launch can hide in when it leaves register file and wave slots free
    static const int lds_min = env_switch("MRFP_WGRAD_LDS", 0);
    const int lds_need = WgTile<T>::BKP * (PY + PX);
    const int lds = lds_need > lds_min ? lds_need : lds_min;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wgrad_kernel<T, WM, WN, DMA, DENSE, TMB>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        attr_set = true;
    }
    WgP q = p;
    q.tiles = pl.tiles;
    q.splits = pl.splits;
    q.klen = pl.klen;
    hipLaunchKernelGGL((conv_wgrad_kernel<T, WM, WN, DMA, DENSE, TMB>), dim3((unsigned)pl.grid), dim3(256), lds, st, q, *grp);
    MRFP_LAUNCH_CHECK();
    return 0;
}

// the instance of conv_wgrad_kernel a tile plan names (WM = 1: the 64 x 256 tile)
template <typename T, int WM, int WN>
static int launch_wgrad(const WgP& p, const WgradPlan& pl, hipStream_t st, const WgGroup* grp) {
    if (pl.variant & kWgDma) {
        const bool dense = pl.variant & kWgDense;
        if constexpr (WM == 2 && sizeof(T) == 2) {
            if (pl.kind == WgradKernel::t256x128) {
                if (dense) return launch_wgrad_v<T, WM, WN, true, true, 4>(p, pl, st, grp);
                return launch_wgrad_v<T, WM, WN, true, false, 4>(p, pl, st, grp);
            }
        }
        if (dense) return launch_wgrad_v<T, WM, WN, sizeof(T) == 2, true>(p, pl, st, grp);
        return launch_wgrad_v<T, WM, WN, sizeof(T) == 2>(p, pl, st, grp);
    }
    return launch_wgrad_v<T, WM, WN, false>(p, pl, st, grp);
}
template <typename T>
static int launch_wgrad_tiles(const WgP& p, const WgradPlan& pl, hipStream_t st, const WgGroup* grp) {
    return pl.kind == WgradKernel::t64x256 ? launch_wgrad<T, 1, 4>(p, pl, st, grp) : launch_wgrad<T, 2, 2>(p, pl, st, grp);
}

// MRFP_WGRAD_DMA=0 keeps register staging for the 16-bit types (A/B measurements); fp32 always stages in registers
static int wgrad_dma_mode() {
    static const int dma = env_switch("MRFP_WGRAD_DMA", 1);
    return dma;
}
// MRFP_WGRAD_BIG: 0 = never the 256 x 128 tile, 1 (default) = where the cost model prefers it, 2 = wherever it is legal (A/B runs)
static int wgrad_big_mode() {
    // (MRFP_WGRAD_DMA=0: the register-staged A/B path of the 16-bit kernels has no 256 x 128 instance)
    static const int mode = wgrad_dma_mode() == 0 ? 0 : env_switch("MRFP_WGRAD_BIG", 1);
    return mode;
}
static int wgrad_debug_drop() {      // timing-only diagnostics (see mrfp_conv_fwd)
    static const int dbg_drop = env_switch("MRFP_DEBUG_DROP", 0);
    return dbg_drop;
}

// Split count from a small cost model (times in us, constants fitted to the bench workload's per-launch timings):
//   a CU that holds w = ceil(tiles*sp/256) workgroups needs w * (K' tiles per split) tile-steps of `step` us, divided
//   by a latency-hiding efficiency (fewer co-resident workgroups than the kernel's occupancy hide less of each other's fill
//   latency); every split adds an fp32 slab of dW that is written once and read once by the reduction (~3 TB/s).
// MRFP_WGRAD_WGS=<n> replaces the model by "about n workgroups" (A/B measurements).
static int64_t wgrad_cost_splits(int64_t tiles, int64_t nkt, int64_t group, double nq, double step, int occ) {
    static const int target = env_switch("MRFP_WGRAD_WGS", 0);
    if (target > 0) return target / tiles;
    int64_t sp = 1;
    double best = 1e30;
    int64_t smax = 1024 / tiles > 96 ? 1024 / tiles : 96;      // few tiles: enough splits to fill the chip
    if (smax > nkt) smax = nkt;
    for (int64_t c = 1; c <= smax; ++c) {
        const int64_t w = (tiles * c + 255) / 256, iters = (nkt + c - 1) / c;
        const double eff = occ == 4 ? (w >= 3 ? 1.0 : w == 2 ? 0.85 : 0.6) : (w >= 2 ? 1.0 : 0.7);
        const double cost = (double)w * (double)iters * step / eff + (double)c * (double)group * (nq * 8.0 / 3.0e6);
        if (cost < best * 0.999) { best = cost; sp = c; }
    }
    return sp;
}

// The conv_wgrad_kernel arm of wgrad_plan: tile, K' splits and grid for `group` problems of M pixels, N output channels and Q = R*S*C
// columns -- all the workspace queries know of a call, so they read this arm directly.  cap > 0: at most that many splits.
static WgradPlan wgrad_tile_plan(int64_t M, int64_t N, int64_t Q, int esz, bool pointwise, int64_t group, int64_t cap) {
    WgradPlan pl = {};
    const int bkp = esz == 4 ? 32 : 64;          // pixels per K' tile (WgTile)
    const int wm = N <= 64 ? 1 : 2, wn = 4 / wm;
    // (a grouped launch: `group` problems of this geometry fill the chip together; the split count is per problem)
    int64_t tiles = ((N + 64 * wm - 1) / (64 * wm)) * ((Q + 64 * wn - 1) / (64 * wn));
    const int64_t nkt = (M + bkp - 1) / bkp;
    int64_t sp = wgrad_cost_splits(group * tiles, nkt, group, (double)N * (double)Q, 0.84, 4);
    pl.kind = wm == 1 ? WgradKernel::t64x256 : WgradKernel::t128x128;
    // The 256 x 128 tile: 16-bit LDS-DMA kernels (K' tile of 64 pixels), whole 256-channel tiles.  Two workgroups per CU hide less
    // fill latency than four, so it needs LONG K' loops to pay -- measured per launch class of the bench step (tools/wgrad_micro.py,
    // MRFP_WGRAD_BIG=0 / 2, same box): the grouped layer-3 pointwise launches 28.7 -> 26.0 us per problem, 512 <-> 2048 grouped
    // 88 -> 83-86, the 3x3 layers at 192^2 697 -> 634 and 890 -> 802 us; but single pointwise launches with few tiles 37 -> 44 us
    // (every split gets ~10 K' tiles), and the 3x3 layers at 48^2 47.2 -> 49.2 us per problem even grouped.  Rule: enough K' tile-steps
    // per CU (`load`, in 256 x 128 units), and for the gather (non-pointwise) form only the large images.
    if (bkp == 64 && wm == 2 && N % 256 == 0 && wgrad_big_mode() > 0) {
        const int64_t tiles4 = (N / 256) * ((Q + 127) / 128);
        const int64_t load = group * tiles4 * nkt / 256;
        const bool want = load >= 100 && (pointwise || M >= 65536);
        if (wgrad_big_mode() >= 2 || want) {
            sp = wgrad_cost_splits(group * tiles4, nkt, group, (double)N * (double)Q, 1.30, 2);
            tiles = tiles4;
            pl.kind = WgradKernel::t256x128;
        }
    }
    if (esz == 2 && wgrad_dma_mode()) {
        static const int dense = env_switch("MRFP_WGRAD_DENSE", 1);
        pl.variant = kWgDma | (dense && pointwise ? kWgDense : 0);
    }
    if (sp < 1) sp = 1;
    if (sp > nkt) sp = nkt;
    if (cap > 0 && sp > cap) sp = cap;
    const int64_t per = (nkt + sp - 1) / sp;      // K' tiles per split
    pl.splits = (int)((nkt + per - 1) / per);
    pl.klen = (int)(per * bkp);
    pl.tiles = (int)tiles;
    pl.grid = (int)(tiles * pl.splits * group);
    return pl;
}

// The launch plan of one weight-gradient call.  cap > 0: g is a batch range of a larger call whose workspace holds `cap` slots per
// problem (the whole call's own split count) -- the tile kernels only, as the accumulator-stationary ones walk whole activations.
static WgradPlan wgrad_plan(const WgradGeom& g, int64_t cap = 0) {
    WgradPlan pl;
    if (cap == 0 && !wgrad_debug_drop() && (wg3_plan(g, pl) || wg1_plan(g, pl))) return pl;
    return wgrad_tile_plan(g.M(), g.N, g.Q(), g.esz, g.pointwise(), g.count, cap);
}

// slab slots per problem the workspace of a call holds: the maximum over what (M, N, Q, count) leaves open -- the slot bounds of the
// accumulator-stationary kernels, if Q could be 9 * C resp. C, and the element size and pointwise form of the tile arm
static int64_t wgrad_ws_slots(int64_t M, int64_t N, int64_t Q, int64_t count) {
    int64_t slots = wg3_slots(N, Q, count);
    if (wg1_slots(N, Q, count) > slots) slots = wg1_slots(N, Q, count);
    for (int arm = 0; arm < 3; ++arm) {      // 16-bit gather, 16-bit pointwise, fp32 (no pointwise rule)
        const int s = wgrad_tile_plan(M, N, Q, arm < 2 ? 2 : 4, arm == 1, count, 0).splits;
        if (s > slots) slots = s;
    }
    return slots;
}

// The argument checks of a call that its plan depends on (the launch and mrfp_conv_wgrad_plan); fills g with the whole call.
// Both operands are read through 32-bit buffer-descriptor offsets: an activation above kOOB bytes is walked in ranges of `bmax` images
struct WgradCall {
    WgradGeom g;
    int64_t ximg, yimg, bmax;       // bytes of one image of x / dy; images per launch
};
static int wgrad_call(int dtype, int64_t B, int64_t H, int64_t W, int64_t C, int64_t N, int64_t ldn, int64_t R, int64_t S, int64_t Ho,
                      int64_t Wo, int64_t stride, int64_t pad_h, int64_t pad_w, int64_t dil, int64_t count, WgradCall& c) {
    MRFP_CHECK(count > 0 && count <= kWgMaxGroup && B > 0 && H > 0 && W > 0 && C > 0 && N > 0 && R > 0 && S > 0 && Ho > 0 && Wo > 0,
               "conv_wgrad: bad arguments");
    MRFP_CHECK(dtype_known(dtype), "conv_wgrad: unknown dtype %d", dtype);
    const int esz = dtype_bytes(dtype);
    MRFP_CHECK((C * esz) % 16 == 0 && (ldn * esz) % 16 == 0 && ldn >= N,
               "conv_wgrad: channel counts must make 16-byte chunks (C=%lld ldn=%lld)", (long long)C, (long long)ldn);
    MRFP_CHECK(B * Ho * Wo < (1LL << 31), "conv_wgrad: tensor too large");
    c.g = WgradGeom{esz, B, H, W, C, N, ldn, R, S, Ho, Wo, stride, pad_h, pad_w, dil, count};
    c.ximg = H * W * C * esz;
    c.yimg = Ho * Wo * ldn * esz;
    MRFP_CHECK(c.ximg < (int64_t)kOOB && c.yimg < (int64_t)kOOB, "conv_wgrad: one image exceeds the 3.75 GB buffer-descriptor range");
    c.bmax = (int64_t)(kOOB - 1) / (c.ximg > c.yimg ? c.ximg : c.yimg);
    MRFP_CHECK(count == 1 || c.bmax >= B, "conv_wgrad_grouped: the activations of a grouped launch must fit one 3.75 GB buffer range each");
    return 0;
}

}  // namespace mrfp

using namespace mrfp;

extern "C" {

int64_t mrfp_conv_wgrad_grouped_ws_bytes(int64_t M, int64_t N, int64_t Q, int64_t count) {
    return wgrad_ws_slots(M, N, Q, count) * count * N * Q * 4;
}
int64_t mrfp_conv_wgrad_ws_bytes(int64_t M, int64_t N, int64_t Q) { return mrfp_conv_wgrad_grouped_ws_bytes(M, N, Q, 1); }

int mrfp_conv_wgrad_plan(int dtype, int64_t B, int64_t H, int64_t W, int64_t C, int64_t N, int64_t ldn, int64_t R, int64_t S, int64_t Ho,
                         int64_t Wo, int64_t stride, int64_t pad_h, int64_t pad_w, int64_t dil, int64_t count, int64_t* out) {
    MRFP_CHECK(out, "conv_wgrad_plan: null output");
    WgradCall c;
    if (int rc = wgrad_call(dtype, B, H, W, C, N, ldn, R, S, Ho, Wo, stride, pad_h, pad_w, dil, count, c)) return rc;
    WgradPlan pl = wgrad_plan(c.g);
    if (c.bmax < B) {                // (walked in batch ranges: the first one's launch)
        c.g.B = c.bmax;
        pl = wgrad_plan(c.g, pl.splits);
    }
    out[0] = (int64_t)pl.kind; out[1] = pl.variant; out[2] = pl.splits; out[3] = pl.klen; out[4] = pl.grid;
    return 0;
}

static int wgrad_run(const void* const* xs, const void* const* dys, float* const* dws, int64_t count, void* ws, int dtype, int64_t B,
                     int64_t H, int64_t W, int64_t C, int64_t Ctrue, int64_t N, int64_t ldn, int64_t R, int64_t S, int64_t Ho,
                     int64_t Wo, int64_t stride, int64_t pad_h, int64_t pad_w, int64_t dil, void* stream) {
    MRFP_CHECK(xs && dys && dws && ws, "conv_wgrad: bad arguments");
    WgradCall c;
    if (int rc = wgrad_call(dtype, B, H, W, C, N, ldn, R, S, Ho, Wo, stride, pad_h, pad_w, dil, count, c)) return rc;
    MRFP_CHECK(Ctrue <= C, "conv_wgrad: Ctrue=%lld exceeds the channel pitch C=%lld", (long long)Ctrue, (long long)C);
    for (int64_t g = 0; g < count; ++g)
        MRFP_CHECK(xs[g] && dys[g] && dws[g] && aligned16(xs[g]) && aligned16(dys[g]), "conv_wgrad: x / dy must be 16-byte aligned, dw non-null");
    WgP p;
    p.slab = (float*)ws;
    p.H = (int)H; p.W = (int)W; p.C = (int)C; p.N = (int)N; p.ldn = (int)ldn;
    p.R = (int)R; p.S = (int)S; p.Ho = (int)Ho; p.Wo = (int)Wo;
    p.stride = (int)stride; p.pad_h = (int)pad_h; p.pad_w = (int)pad_w; p.dil = (int)dil;
    p.Q = (int)(R * S * C);
    p.ngroup = (int)count;
    p.div_hw = make_fastdiv((unsigned)(Ho * Wo)); p.div_w = make_fastdiv((unsigned)Wo);
    const WgGroup grp = make_wg_group(xs, dys, count);
    WgOut outs;
    for (int g = 0; g < kWgMaxGroup; ++g) outs.dw[g] = dws[g < count ? g : 0];
    hipStream_t st = (hipStream_t)stream;
    // the plan of the whole call: its splits are what `ws` must hold, and the cap of the batch ranges of a call that is walked in several
    const WgradPlan whole = wgrad_plan(c.g);
    // A tile plan is the workspace query's own arm for this element size and form.  The accumulator-stationary kernels plan through
    // class_walk and are granted slots through class_walk_slots, a term of the query's maximum: that pair is checked here.
    if (whole.kind == WgradKernel::wg3 || whole.kind == WgradKernel::wg1) {
        const int64_t slots = whole.kind == WgradKernel::wg3 ? wg3_slots(N, p.Q, count) : wg1_slots(N, p.Q, count);
        MRFP_CHECK(whole.splits <= slots, "conv_wgrad: the launch plan needs %d slab slots per problem, mrfp_conv_wgrad*_ws_bytes grants %lld",
                   whole.splits, (long long)slots);
    }
    const int dbg_drop = wgrad_debug_drop();
    // every range is one wgrad + reduction pair on the stream, the later ones adding to dw (fixed order: reproducible)
    for (int64_t b0 = 0; b0 < B; b0 += c.bmax) {
        WgradGeom g = c.g;
        g.B = B - b0 < c.bmax ? B - b0 : c.bmax;
        const WgradPlan pl = g.B == B ? whole : wgrad_plan(g, whole.splits);
        p.B = (int)g.B;
        p.M = (int)g.M();
        p.x = (const char*)xs[0] + b0 * c.ximg;
        p.dy = (const char*)dys[0] + b0 * c.yimg;
        p.xbytes = (dbg_drop & 1) ? 0u : (unsigned)(g.B * c.ximg);
        p.dybytes = (dbg_drop & 2) ? 0u : (unsigned)(g.B * c.yimg);
        int rc;
        if (pl.kind == WgradKernel::wg3) rc = wg3_run(xs, dys, (float*)ws, dtype == MRFP_F16, g, pl, p.xbytes, p.dybytes, st);
        else if (pl.kind == WgradKernel::wg1) rc = wg1_run(xs, dys, (float*)ws, dtype == MRFP_F16, g, pl, p.xbytes, p.dybytes, st);
        else rc = by_dtype(dtype, "conv_wgrad", [&](auto t) { return launch_wgrad_tiles<typename decltype(t)::type>(p, pl, st, &grp); });
        if (rc) return rc;
        const int64_t total4 = N * (int64_t)p.Q / 4;          // Q = R*S*C and C*esz % 16 == 0  =>  Q % 4 == 0
        const int64_t blocks = (total4 + 63) / 64;
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)blocks, (unsigned)count), dim3(256), 0, st, (const float*)ws, pl.splits, (int)N,
                           p.Q, (int)C, (int)Ctrue, (int)(R * S), dws[0], b0 > 0 ? 1 : 0, outs);
        MRFP_LAUNCH_CHECK();
    }
    return 0;
}

int mrfp_conv_wgrad(const void* x, const void* dy, float* dw, void* ws, int dtype, int64_t B, int64_t H, int64_t W,
                    int64_t C, int64_t Ctrue, int64_t N, int64_t ldn, int64_t R, int64_t S, int64_t Ho, int64_t Wo,
                    int64_t stride, int64_t pad_h, int64_t pad_w, int64_t dil, void* stream) {
    return wgrad_run(&x, &dy, &dw, 1, ws, dtype, B, H, W, C, Ctrue, N, ldn, R, S, Ho, Wo, stride, pad_h, pad_w, dil, stream);
}

int64_t mrfp_conv_wgrad_group_max(void) { return kWgMaxGroup; }

int mrfp_conv_wgrad_grouped(const void* const* xs, const void* const* dys, float* const* dws, int64_t count, void* ws, int dtype,
                            int64_t B, int64_t H, int64_t W, int64_t C, int64_t Ctrue, int64_t N, int64_t ldn, int64_t R, int64_t S,
                            int64_t Ho, int64_t Wo, int64_t stride, int64_t pad_h, int64_t pad_w, int64_t dil, void* stream) {
    return wgrad_run(xs, dys, dws, count, ws, dtype, B, H, W, C, Ctrue, N, ldn, R, S, Ho, Wo, stride, pad_h, pad_w, dil, stream);
}

}  // extern "C"
