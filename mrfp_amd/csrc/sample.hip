// sample.hip -- class-uniform sampling, the producer half: per image tile and class the pixel count, the sums of
// the tile-relative coordinates and the integer centroid, from uint8 label maps that are already on the device.
//
//   tile_sums_clear_kernel   sums <- 0 (the entry clears what it accumulates into)
//   tile_sums_kernel<VEC>    a workgroup takes one CHUNK of one tile at a time -- whole rows of the tile, at most kChunkMax pixels --
//                            and walks further chunks past the grid cap.  A lane reads 16 consecutive labels of one row (one 16-byte
//                            load when base, pitch and tile are multiples of 16, else bytewise) and merges runs of equal labels in
//                            registers, across its units of the chunk, before it touches LDS: label maps are piecewise constant, and
//                            without that step every lane of a wave adds to the same LDS word.  LDS holds unsigned [C][3] = n,
//                            sum(x - x0), sum(y - y0); after a chunk every non-zero word goes to the tile's 64-bit sums with one
//                            integer atomicAdd.  Integer adds commute: two runs give the same bits.
//   tile_centroids_kernel    cx = x0 + floor(sum(x - x0) / n), cy likewise; -1, -1 where n = 0
//
// No floating point, no host wait.
#include "common.hpp"

namespace mrfp {

constexpr int kSampleMaxClasses = 256;
constexpr int kTileMax = 65536;             // tile-relative coordinates are below this
constexpr int kChunkMax = 65536;            // pixels a workgroup adds into its LDS words between two flushes, at most
constexpr int kChunkTarget = 16384;         // ... and what a chunk is cut to where a tile row is shorter than this (more workgroups)
constexpr int kSampleGridCap = 2048;        // workgroups of a launch, as ce_w_blocks_x caps them
// a 32-bit LDS word (and a lane's run sums in registers, which are part of the same chunk) never wraps: at most kChunkMax pixels at
// coordinates of at most kTileMax - 1
static_assert((unsigned long long)kChunkMax * (kTileMax - 1) < (1ull << 32) && kChunkTarget <= kChunkMax, "32-bit chunk sums overflow");
static_assert(kThreads == 256, "one thread per entry of the label table");

// rows of a tile per chunk: whole rows, at least one (a row is at most kTileMax = kChunkMax pixels)
static int chunk_rows(int64_t tw_max) {
    const int64_t r = kChunkTarget / tw_max;
    return (int)(r < 1 ? 1 : r);
}

__global__ void tile_sums_clear_kernel(unsigned long long* __restrict__ sums, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) sums[i] = 0ull;
}

struct LabelRun {
    int raw;                     // the label byte of the run, -1: no run yet
    unsigned cls, n, sx, sy;     // its class (after the table), pixels, sum of x - x0, sum of y - y0
};

__device__ __forceinline__ void run_flush(const LabelRun& r, int C, unsigned* __restrict__ acc) {
    if (r.n != 0u && r.cls < (unsigned)C) {
        atomicAdd(&acc[3 * r.cls], r.n);
        if (r.sx) atomicAdd(&acc[3 * r.cls + 1], r.sx);
        if (r.sy) atomicAdd(&acc[3 * r.cls + 2], r.sy);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void tile_sums_kernel(const uint8_t* __restrict__ lab, const uint8_t* __restrict__ table, int H,
                                                             int W, int C, int tile, int nty, int ntx, int rpc, int cpt, int64_t items,
                                                             unsigned long long* __restrict__ sums) {
    __shared__ unsigned acc[3 * kSampleMaxClasses];
    __shared__ uint8_t tab[256];
    const int tid = threadIdx.x;
    for (int i = tid; i < 3 * C; i += kThreads) acc[i] = 0u;
    tab[tid] = table ? table[tid] : (uint8_t)tid;
    __syncthreads();
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int chunk = (int)(it % cpt);
        const int64_t t = it / cpt;                                  // the tile, over [B][nty][ntx]
        const int tx = (int)(t % ntx), ty = (int)((t / ntx) % nty);
        const int64_t b = t / ((int64_t)ntx * nty);
        const int x0 = tx * tile, y0 = ty * tile;                    // < W, < H
        const int tw = min(tile, W - x0), th = min(tile, H - y0);    // a ragged tile (partial) is narrower / shorter
        const int r0 = chunk * rpc;
        const int nr = min(rpc, th - r0);
        if (nr <= 0) continue;                                       // a chunk below a ragged tile (the same for the whole workgroup)
        const int upr = (tw + 15) >> 4;                              // 16-label units per row
        const int nunits = nr * upr;                                 // nr * tw <= kChunkMax
        const uint8_t* base = lab + ((int64_t)b * H + y0 + r0) * W + x0;
        LabelRun run = {-1, 0u, 0u, 0u, 0u};
        for (int u = tid; u < nunits; u += kThreads) {
            const int r = u / upr;
            const unsigned ux = (unsigned)(u - r * upr) << 4, yr = (unsigned)(r0 + r);      // tile-relative
            const uint8_t* p = base + (int64_t)r * W + ux;
            uint8_t v[16];
            int cnt = 16;
            if constexpr (VEC) {                                     // tw is a multiple of 16 here: every unit is whole
                const uint4 q = *reinterpret_cast<const uint4*>(p);
                const unsigned splat = (unsigned)run.raw * 0x01010101u;
                if (run.raw >= 0 && q.x == splat && q.y == splat && q.z == splat && q.w == splat) {      // the run goes on
                    run.n += 16u;
                    run.sx += 16u * ux + 120u;
                    run.sy += 16u * yr;
                    continue;
                }
                const unsigned w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int i = 0; i < 16; ++i) v[i] = (uint8_t)(w4[i >> 2] >> (8 * (i & 3)));
            } else {
                cnt = min(16, tw - (int)ux);
#pragma unroll
                for (int i = 0; i < 16; ++i) v[i] = i < cnt ? p[i] : (uint8_t)0;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (i < cnt) {
                    const int l = v[i];
                    if (l != run.raw) {
                        run_flush(run, C, acc);
                        run = {l, (unsigned)tab[l], 0u, 0u, 0u};
                    }
                    run.n += 1u;
                    run.sx += ux + (unsigned)i;
                    run.sy += yr;
                }
            }
        }
        run_flush(run, C, acc);
        __syncthreads();
        unsigned long long* dst = sums + t * (3 * (int64_t)C);
        for (int i = tid; i < 3 * C; i += kThreads) {
            const unsigned w = acc[i];
            if (w) {
                atomicAdd(&dst[i], (unsigned long long)w);
                acc[i] = 0u;
            }
        }
        __syncthreads();
    }
}

__global__ void tile_centroids_kernel(const unsigned long long* __restrict__ sums, int64_t n, int C, int tile, int nty, int ntx,
                                      int32_t* __restrict__ cent) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const int64_t t = i / C;
        const int64_t x0 = (t % ntx) * tile, y0 = ((t / ntx) % nty) * tile;
        const unsigned long long cnt = sums[3 * i];
        int32_t cx = -1, cy = -1;
        if (cnt) {
            cx = (int32_t)(x0 + (int64_t)(sums[3 * i + 1] / cnt));
            cy = (int32_t)(y0 + (int64_t)(sums[3 * i + 2] / cnt));
        }
        cent[2 * i] = cx;
        cent[2 * i + 1] = cy;
    }
}

static unsigned flat_grid(int64_t n) {
    int64_t g = (n + kThreads - 1) / kThreads;
    return (unsigned)(g > kSampleGridCap ? kSampleGridCap : (g < 1 ? 1 : g));
}

}  // namespace mrfp

extern "C" {

int64_t mrfp_tile_count(int64_t size, int64_t tile, int partial) {
    if (tile < 1 || size < 0) return -1;
    return partial ? (size + tile - 1) / tile : size / tile;
}

int mrfp_tile_class_sums(const uint8_t* lab, const uint8_t* table, int64_t B, int64_t H, int64_t W, int64_t C, int64_t tile, int partial,
                         int64_t* sums, int32_t* cent, void* stream) {
    using namespace mrfp;
    MRFP_CHECK(C >= 1 && C <= kSampleMaxClasses, "tile_class_sums: C = %lld is outside 1..%d", (long long)C, kSampleMaxClasses);
    MRFP_CHECK(tile >= 1 && tile <= kTileMax, "tile_class_sums: tile = %lld is outside 1..%d", (long long)tile, kTileMax);
    MRFP_CHECK(B >= 1 && H >= 1 && W >= 1 && H < (1ll << 31) && W < (1ll << 31),
               "tile_class_sums: B = %lld, H = %lld, W = %lld: B, H, W >= 1 and H, W < 2^31 expected", (long long)B, (long long)H, (long long)W);
    const int64_t nty = mrfp_tile_count(H, tile, partial), ntx = mrfp_tile_count(W, tile, partial);
    MRFP_CHECK(nty >= 1 && ntx >= 1, "tile_class_sums: no tile: a %lldx%lld map holds no whole tile of %lld (partial = 0)", (long long)H,
               (long long)W, (long long)tile);
    MRFP_CHECK(B < (1ll << 31) && B * nty < (1ll << 31) && B * nty * ntx < (1ll << 31) && B * nty * ntx * C < (1ll << 31),
               "tile_class_sums: B*nty*ntx*C = %lld*%lld*%lld*%lld reaches 2^31", (long long)B, (long long)nty, (long long)ntx, (long long)C);
    MRFP_CHECK(lab && sums && cent, "tile_class_sums: null argument (lab, sums, cent)");      // (behind the sizes: empty outputs have no address)
    const int64_t ntiles = B * nty * ntx, nwords = ntiles * C;
    const int64_t tw_max = tile < W ? tile : W, th_max = tile < H ? tile : H;
    const int rpc = chunk_rows(tw_max);
    MRFP_CHECK((int64_t)rpc * tw_max <= kChunkMax, "tile_class_sums: a chunk of %d rows of %lld pixels exceeds %d", rpc, (long long)tw_max,
               kChunkMax);
    const int cpt = (int)((th_max + rpc - 1) / rpc);
    const int64_t items = ntiles * cpt;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* s = (unsigned long long*)sums;
    hipLaunchKernelGGL(tile_sums_clear_kernel, dim3(flat_grid(3 * nwords)), dim3(kThreads), 0, st, s, 3 * nwords);
    MRFP_LAUNCH_CHECK();
    const bool vec = aligned16(lab) && W % 16 == 0 && tile % 16 == 0;
    const dim3 grid((unsigned)(items > kSampleGridCap ? kSampleGridCap : items));
    if (vec)
        hipLaunchKernelGGL(tile_sums_kernel<true>, grid, dim3(kThreads), 0, st, lab, table, (int)H, (int)W, (int)C, (int)tile, (int)nty,
                           (int)ntx, rpc, cpt, items, s);
    else
        hipLaunchKernelGGL(tile_sums_kernel<false>, grid, dim3(kThreads), 0, st, lab, table, (int)H, (int)W, (int)C, (int)tile, (int)nty,
                           (int)ntx, rpc, cpt, items, s);
    MRFP_LAUNCH_CHECK();
    hipLaunchKernelGGL(tile_centroids_kernel, dim3(flat_grid(nwords)), dim3(kThreads), 0, st, (const unsigned long long*)s, nwords, (int)C,
                       (int)tile, (int)nty, (int)ntx, cent);
    MRFP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
