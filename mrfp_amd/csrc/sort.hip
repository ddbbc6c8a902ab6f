// sort.hip -- mrfp_sort_pairs (include/mrfp_hip.h): a stable least-significant-digit radix sort of (uint32 key, uint32 payload) pairs,
// ascending, over S independent segments of one array, 8 key bits per pass.  It is what the Lovasz-Softmax loss (lovasz.hip) ranks the
// per-class errors of its scope with; OHEM's radix select (ohem.hip) finds one order statistic, not ranks.
//
// A pass is three launches, and no workgroup ever waits for another one inside a launch (no decoupled look-back, no flag that one
// workgroup writes and another polls: the order in which workgroups are scheduled never matters):
//   sort_hist_kernel      per tile of kSortTile consecutive items of ONE segment: the count of each of the 256 digits, LDS integer
//                         counters, stored digit-major: hist[digit][tile]
//   sort_scan_kernel      workgroup (digit, segment): the exclusive scan of that digit's counts over the tiles of that segment, in
//                         place, in sweeps of kSortScanSweep tiles with a running carry; the digit's total of the segment -> totals
//   sort_scatter_kernel   per tile: the 256 digit totals of its segment scanned in LDS (the digit bases), plus the tile's scanned
//                         count, plus the STABLE rank of the item among the tile's items of the same digit -> its destination
// Stable in-tile rank: a tile is contiguous; wave w owns items [w * 64 * kSortItems, ...) of it and walks them in rounds of 64, lane
// l taking item l of the round.  In a round the lanes with the same digit are found with one ballot per digit bit; a lane's rank is
// the wave's running count of that digit (LDS, one row per wave) plus the number of lower lanes among its peers; the lowest peer
// adds the peers to the count.  Rounds, lanes and waves are taken in ascending order, so equal digits keep their order.
// Counts are integers: two runs place every pair identically.  Every loop is bounded by the arguments (n, S); grids are capped at
// kSortMaxGrid workgroups and walk the tiles.
//
// Tiles never straddle a segment: segment s owns the tile ids floor(offsets[s] / kSortTile) + s ... (as many as it needs), which are
// disjoint for non-decreasing offsets, at most n / kSortTile + S + 1 in all -- a bound known on the host, so nothing waits for the
// device.  A workgroup finds the segment of a tile id by bisection over the offsets.  Offsets are clamped to [0, n] and every store
// is bounds-checked: a wrong offsets array gives a wrong order, never a store outside the buffers.
#include "common.hpp"

namespace mrfp {

constexpr int kSortThreads = 256;
constexpr int kSortItems = 16;                               // per thread and pass
constexpr int kSortTile = kSortThreads * kSortItems;         // 4096 items one workgroup ranks per pass
constexpr int kSortRadix = 256;                              // 8 bits per pass
constexpr int kSortScanSweep = kSortThreads;                 // tiles one sweep of a scan workgroup covers
constexpr int kSortMaxGrid = 2048;                           // the cap of the loss kernels (loss_common.hpp: ce_w_blocks_x)
static_assert(kSortRadix == kSortThreads, "thread d owns digit d");

struct SortSegs {
    const int64_t* offsets;          // [S + 1] on the device, or null: one segment [0, n)
    int S;
    int64_t n;
    __device__ __forceinline__ int64_t off(int s) const {
        int64_t o = offsets ? offsets[s] : (s == 0 ? 0 : n);
        return o < 0 ? 0 : (o > n ? n : o);
    }
    __device__ __forceinline__ int64_t tile_base(int s) const { return off(s) / kSortTile + s; }
    // tile id g -> its segment and item range [begin, end) (end - begin <= kSortTile); false for an id no segment uses
    __device__ __forceinline__ bool tile(int64_t g, int& seg, int64_t& seg_begin, int64_t& begin, int64_t& end) const {
        int lo = 0, hi = S - 1;
        for (int it = 0; it < 32 && lo < hi; ++it) {         // the last s with tile_base(s) <= g
            const int mid = (lo + hi + 1) >> 1;
            if (tile_base(mid) <= g) lo = mid; else hi = mid - 1;
        }
        seg = lo;
        seg_begin = off(lo);
        const int64_t local = g - tile_base(lo), seg_end = off(lo + 1);
        if (local < 0) return false;
        begin = seg_begin + local * kSortTile;
        end = begin + kSortTile < seg_end ? begin + kSortTile : seg_end;
        return begin < seg_end;
    }
};

static int64_t sort_max_tiles(int64_t n, int64_t S) { return n / kSortTile + S + 1; }

// exclusive scan of one value per thread over the kSortThreads threads of the workgroup; total: the sum, on every thread.  Ends
// behind a barrier, so it may be called again at once.
__device__ __forceinline__ unsigned int block_exclusive_scan(unsigned int v, unsigned int& total) {
    __shared__ unsigned int wsum[kSortThreads / 64];
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
    for (int i = 0; i < kSortThreads / 64; ++i) {
        const unsigned int t = wsum[i];
        before += i < w ? t : 0u;
        all += t;
    }
    __syncthreads();
    total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(kSortThreads) void sort_hist_kernel(const unsigned int* __restrict__ keys, const SortSegs segs, int64_t ntmax,
                                                                 int shift, unsigned int mask, unsigned int* __restrict__ hist) {
    __shared__ unsigned int cnt[kSortRadix];
    for (int64_t g = blockIdx.x; g < ntmax; g += gridDim.x) {
        cnt[threadIdx.x] = 0u;
        __syncthreads();
        int seg;
        int64_t sb, b, e;
        const bool used = segs.tile(g, seg, sb, b, e);
        if (used) {
#pragma unroll
            for (int u = 0; u < kSortItems; ++u) {
                const int64_t i = b + u * kSortThreads + threadIdx.x;
                if (i < e) atomicAdd(&cnt[(keys[i] >> shift) & mask], 1u);      // an integer count: the order of the additions does not matter
            }
        }
        __syncthreads();
        if (used) hist[(int64_t)threadIdx.x * ntmax + g] = cnt[threadIdx.x];
        __syncthreads();
    }
}

// grid (kSortRadix, min(S, cap)): workgroup (d, y) scans digit d over the tiles of segments y, y + gridDim.y, ...
__global__ __launch_bounds__(kSortThreads) void sort_scan_kernel(const SortSegs segs, int64_t ntmax, unsigned int* __restrict__ hist,
                                                                 unsigned int* __restrict__ totals) {
    const int d = blockIdx.x;
    for (int s = blockIdx.y; s < segs.S; s += gridDim.y) {
        const int64_t b = segs.off(s), e = segs.off(s + 1), tb = segs.tile_base(s);
        int64_t nt = e > b ? (e - b + kSortTile - 1) / kSortTile : 0;
        if (nt > ntmax - tb) nt = ntmax - tb;                 // never past the row, whatever the offsets hold
        unsigned int* row = hist + (int64_t)d * ntmax + tb;
        unsigned int carry = 0u;
        for (int64_t base = 0; base < nt; base += kSortScanSweep) {
            const int64_t t = base + threadIdx.x;
            const unsigned int v = t < nt ? row[t] : 0u;
            unsigned int total;
            const unsigned int ex = block_exclusive_scan(v, total);
            if (t < nt) row[t] = carry + ex;
            carry += total;
        }
        if (threadIdx.x == 0) totals[(int64_t)s * kSortRadix + d] = carry;
    }
}

__global__ __launch_bounds__(kSortThreads) void sort_scatter_kernel(const unsigned int* __restrict__ kin, const unsigned int* __restrict__ pin,
                                                                    unsigned int* __restrict__ kout, unsigned int* __restrict__ pout,
                                                                    const SortSegs segs, int64_t ntmax, int shift, unsigned int mask,
                                                                    const unsigned int* __restrict__ hist,
                                                                    const unsigned int* __restrict__ totals) {
    __shared__ unsigned int cnt[kSortThreads / 64][kSortRadix];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t g = blockIdx.x; g < ntmax; g += gridDim.x) {
        int seg;
        int64_t sb, b, e;
        const bool used = segs.tile(g, seg, sb, b, e);          // the same on every thread
#pragma unroll
        for (int i = 0; i < kSortThreads / 64; ++i) cnt[i][threadIdx.x] = 0u;
        // thread d: where digit d of this tile starts inside the segment
        unsigned int all;
        const unsigned int dbase = block_exclusive_scan(used ? totals[(int64_t)seg * kSortRadix + threadIdx.x] : 0u, all);
        const unsigned int start = dbase + (used ? hist[(int64_t)threadIdx.x * ntmax + g] : 0u);
        // (block_exclusive_scan ended behind a barrier: the zeros are visible)
        unsigned int key[kSortItems], pay[kSortItems], rank[kSortItems];
#pragma unroll
        for (int r = 0; r < kSortItems; ++r) {
            const int64_t i = b + ((int64_t)w * kSortItems + r) * 64 + lane;
            const bool live = used && i < e;
            key[r] = live ? kin[i] : 0u;
            pay[r] = live ? pin[i] : 0u;
        }
#pragma unroll
        for (int r = 0; r < kSortItems; ++r) {
            const int64_t i = b + ((int64_t)w * kSortItems + r) * 64 + lane;
            const bool live = used && i < e;
            const unsigned int d = (key[r] >> shift) & mask;
            unsigned long long peers = __ballot(live);
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool one = (d >> bit) & 1u;
                const unsigned long long m = __ballot(one);
                peers &= one ? m : ~m;
            }
            const unsigned int prev = live ? cnt[w][d] : 0u;     // every peer reads the same word
            __builtin_amdgcn_wave_barrier();
            rank[r] = prev + (unsigned int)__popcll(peers & below);
            if (live && (peers & below) == 0ull) cnt[w][d] = prev + (unsigned int)__popcll(peers);      // the lowest peer
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        {       // thread d: the wave counts of digit d -> where each wave's items of digit d start
            unsigned int run = start;
#pragma unroll
            for (int i = 0; i < kSortThreads / 64; ++i) {
                const unsigned int t = cnt[i][threadIdx.x];
                cnt[i][threadIdx.x] = run;
                run += t;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kSortItems; ++r) {
            const int64_t i = b + ((int64_t)w * kSortItems + r) * 64 + lane;
            if (used && i < e) {
                const unsigned int d = (key[r] >> shift) & mask;
                const int64_t dst = sb + (int64_t)cnt[w][d] + rank[r];
                if (dst >= 0 && dst < segs.n) {
                    kout[dst] = key[r];
                    pout[dst] = pay[r];
                }
            }
        }
        __syncthreads();
    }
}

struct SortWs {
    unsigned int *altk, *altp, *hist, *totals;
    int64_t bytes;
};

static int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }

static SortWs sort_ws(void* ws, int64_t n, int64_t S) {
    char* p = (char*)ws;
    SortWs w;
    int64_t o = 0;
    w.altk = (unsigned int*)(p + o); o += align16(4 * n);
    w.altp = (unsigned int*)(p + o); o += align16(4 * n);
    w.hist = (unsigned int*)(p + o); o += align16(4 * kSortRadix * sort_max_tiles(n, S));
    w.totals = (unsigned int*)(p + o); o += align16(4 * kSortRadix * S);
    w.bytes = o;
    return w;
}

}  // namespace mrfp

extern "C" {

int64_t mrfp_sort_tile_items(void) { return mrfp::kSortTile; }

int64_t mrfp_sort_scan_sweep(void) { return mrfp::kSortScanSweep; }

int64_t mrfp_sort_pairs_ws_bytes(int64_t n, int64_t S) {
    if (n < 0 || n >= (1LL << 31) || S < 1 || S > (1 << 24)) return -1;
    return mrfp::sort_ws(nullptr, n, S).bytes;
}

int mrfp_sort_pairs(const void* keys_in, const void* payload_in, void* keys_out, void* payload_out, int64_t n, const int64_t* offsets,
                    int64_t S, int bits, void* ws, void* stream) {
    using namespace mrfp;
    const char* who = "sort_pairs";
    MRFP_CHECK(n >= 0 && n < (1LL << 31), "%s: 0 <= n < 2^31 (n=%lld)", who, (long long)n);
    MRFP_CHECK(S >= 1 && S <= (1 << 24), "%s: 1 <= S <= 2^24 segments (S=%lld)", who, (long long)S);
    MRFP_CHECK(offsets || S == 1, "%s: S=%lld segments need an offsets array", who, (long long)S);
    MRFP_CHECK(bits >= 1 && bits <= 32, "%s: 1 <= bits <= 32 (bits=%d)", who, bits);
    if (n == 0) return 0;
    MRFP_CHECK(keys_in && payload_in && keys_out && payload_out && ws, "%s: null pointer", who);
    const int passes = (bits + 7) / 8;
    MRFP_CHECK((keys_in != keys_out && payload_in != payload_out) || passes % 2 == 0,
               "%s: sorting in place needs an even number of 8-bit passes (bits=%d)", who, bits);
    hipStream_t st = (hipStream_t)stream;
    const SortWs w = sort_ws(ws, n, S);
    const SortSegs segs{offsets, (int)S, n};
    const int64_t ntmax = sort_max_tiles(n, S);
    const unsigned int grid = (unsigned int)(ntmax < kSortMaxGrid ? ntmax : kSortMaxGrid);
    const unsigned int gy = (unsigned int)(S < kSortMaxGrid / kSortRadix ? S : kSortMaxGrid / kSortRadix);
    const unsigned int* kin = (const unsigned int*)keys_in;
    const unsigned int* pin = (const unsigned int*)payload_in;
    for (int p = 0; p < passes; ++p) {
        // the last pass writes the outputs, the one before it the alternate buffers, and so on backwards
        const bool to_out = (passes - 1 - p) % 2 == 0;
        unsigned int* ko = to_out ? (unsigned int*)keys_out : w.altk;
        unsigned int* po = to_out ? (unsigned int*)payload_out : w.altp;
        const int shift = 8 * p, nb = bits - shift < 8 ? bits - shift : 8;
        const unsigned int mask = (1u << nb) - 1u;
        hipLaunchKernelGGL(sort_hist_kernel, dim3(grid), dim3(kSortThreads), 0, st, kin, segs, ntmax, shift, mask, w.hist);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(kSortRadix, gy), dim3(kSortThreads), 0, st, segs, ntmax, w.hist, w.totals);
        hipLaunchKernelGGL(sort_scatter_kernel, dim3(grid), dim3(kSortThreads), 0, st, kin, pin, ko, po, segs, ntmax, shift, mask, w.hist,
                           w.totals);
        MRFP_LAUNCH_CHECK();
        kin = ko;
        pin = po;
    }
    return 0;
}

}  // extern "C"
