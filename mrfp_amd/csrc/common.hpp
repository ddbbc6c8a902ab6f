// common.hpp -- shared device helpers for libmrfp_hip (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>
#include <type_traits>
#include "../../include/mrfp_hip.h"

namespace mrfp {

void set_error(const char* fmt, ...);

#define MRFP_CHECK(cond, ...)                      \
    do {                                           \
        if (!(cond)) {                             \
            ::mrfp::set_error(__VA_ARGS__);        \
            return -1;                             \
        }                                          \
    } while (0)

#define MRFP_LAUNCH_CHECK()                                                   \
    do {                                                                      \
        hipError_t e__ = hipGetLastError();                                   \
        if (e__ != hipSuccess) {                                              \
            ::mrfp::set_error("%s:%d launch failed: %s", __FILE__, __LINE__,  \
                              hipGetErrorString(e__));                        \
            return -2;                                                        \
        }                                                                     \
    } while (0)

typedef __hip_bfloat16 bf16;
typedef _Float16 f16;        // IEEE half (MRFP_F16): same 16-byte chunks and MFMA rate as bf16, 11-bit mantissa

// ---- element <-> float ----------------------------------------------------------------------
__device__ __forceinline__ float to_f(float v) { return v; }
__device__ __forceinline__ float to_f(bf16 v) { return __bfloat162float(v); }
__device__ __forceinline__ float to_f(f16 v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16 from_f<bf16>(float v) { return __float2bfloat16(v); }
template <> __device__ __forceinline__ f16 from_f<f16>(float v) { return (f16)v; }
// epilogue activation of the folded inference kernels (compile-time ACT: 0 none, 1 ReLU, 2 ReLU6; conv_common.hpp)
template <int ACT> __device__ __forceinline__ float act_f(float v) {
    if constexpr (ACT == 1) return fmaxf(v, 0.f);
    else if constexpr (ACT == 2) return fminf(fmaxf(v, 0.f), 6.f);
    else return v;
}

// ---- 16-byte vectors of VEC elements ---------------------------------------------------------
// VecT<T,VEC>: VEC elements moved with ONE memory instruction when VEC*sizeof(T) == 16
// (float x4, bf16 x8); VEC == 1 is the scalar tail path for odd channel counts (C = 19).
template <typename T, int VEC> struct alignas(sizeof(T) * VEC) VecT { T v[VEC]; };

template <typename T> struct FullVec { static constexpr int value = 16 / sizeof(T); };

template <typename T, int VEC>
__device__ __forceinline__ void load_f(const T* p, float (&out)[VEC]) {
    VecT<T, VEC> t = *reinterpret_cast<const VecT<T, VEC>*>(p);
#pragma unroll
    for (int i = 0; i < VEC; ++i) out[i] = to_f(t.v[i]);
}
template <typename T, int VEC>
__device__ __forceinline__ void store_f(T* p, const float (&in)[VEC]) {
    VecT<T, VEC> t;
#pragma unroll
    for (int i = 0; i < VEC; ++i) t.v[i] = from_f<T>(in[i]);
    *reinterpret_cast<VecT<T, VEC>*>(p) = t;
}
// raw (unconverted) vector loads: keep several 16-byte loads in flight per lane at 4 VGPRs each, convert on use
template <typename T, int VEC>
__device__ __forceinline__ VecT<T, VEC> load_raw(const T* p) { return *reinterpret_cast<const VecT<T, VEC>*>(p); }
// the same with the non-temporal cache policy: for the LAST read of a tensor in a pass sequence (nothing re-reads these
// bytes soon, so they should not displace lines that the next kernel will hit in L2 / the Infinity Cache).  Used by the
// normalisation apply kernels (affine.hip; the statistics pass in front of them keeps the default policy so that the
// apply pass finds the tensor in the caches): bench step 62.4 -> 61.4 ms (tools/ab_lib.sh, same box, 3 alternations;
// `tools/build_variant.sh nont affine -DMRFP_NT=0` builds the default-policy library).
#ifndef MRFP_NT
#define MRFP_NT 1
#endif
template <typename T, int VEC>
__device__ __forceinline__ VecT<T, VEC> load_raw_nt(const T* p) {
    if constexpr (MRFP_NT != 0 && sizeof(T) * VEC == 16) {
        typedef unsigned __attribute__((ext_vector_type(4))) nt_u32x4;
        const nt_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_u32x4*>(p));
        return __builtin_bit_cast(VecT<T, VEC>, v);
    } else {
        return *reinterpret_cast<const VecT<T, VEC>*>(p);
    }
}
template <typename T, int VEC>
__device__ __forceinline__ void cvt_f(const VecT<T, VEC>& t, float (&out)[VEC]) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) out[i] = to_f(t.v[i]);
}

template <int VEC>
__device__ __forceinline__ void load_coef(const float* p, float (&out)[VEC]) {
    VecT<float, VEC> t = *reinterpret_cast<const VecT<float, VEC>*>(p);
#pragma unroll
    for (int i = 0; i < VEC; ++i) out[i] = t.v[i];
}

// ---- reductions -------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Geometry of a "row kernel": one workgroup walks destination lines (b, oh) of a [B,Ho,Wo,C]
// tensor; 256 threads are laid out as (rowthreads x colthreads) over (ow, channel-vector).
struct RowGeom {
    int B, Ho, Wo, C, Hs, Ws;
    const int32_t* tabH;
    const int32_t* tabW;
};

constexpr int kThreads = 256;
constexpr int kCUs = 256;        // compute units of one MI355X (MI355X_MICROARCH.md, chip-level parameters): what "one round of resident
                                 // workgroups" means to the persistent kernels (conv_common.hpp: kGrid1PerCU / kGrid2PerCU; whiten.hip)

struct Lanes {
    int lpr;         // channel vectors per row = C / VEC
    int colthreads;  // threads across the channel dimension
    int rowthreads;  // threads across pixels of a line
};
__host__ __device__ inline Lanes make_lanes(int C, int VEC) {
    Lanes l;
    l.lpr = C / VEC;
    l.colthreads = l.lpr < kThreads ? l.lpr : kThreads;
    l.rowthreads = kThreads / l.colthreads;
    return l;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// A run-time switch (MRFP_*: A/B runs, tests): the integer value of the environment variable `name`, `dflt` where it is unset.
// Callers keep it in a function-local `static const`, so every switch is read once per process (the tests that flip one run a
// child process).
inline int env_switch(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

// choose the vector width for a channel count: full 16-byte vectors when C allows it
template <typename T> inline int pick_vec(int64_t C) {
    const int full = FullVec<T>::value;
    return (C % full == 0) ? full : 1;
}

// ---- host dispatch: element type, vector width ---------------------------------------------------------------------------
// The element type of an entry point, from its run-time `dtype`.  by_dtype(dtype, "name", [&](auto t) { using T = typename
// decltype(t)::type; return launch_x<T>(...); }) calls the body with one of Tag<float> / Tag<bf16> / Tag<f16> and returns its int;
// any other dtype is refused as "name: unknown dtype %d" (-1).  The body is compiled for every type the helper can pass, so a
// 16-bit-only entry point goes through by_dtype16 -- by_dtype would add its float kernels to the code object.
template <typename T> struct Tag { using type = T; };
template <int V> using Int = std::integral_constant<int, V>;      // a compile-time value chosen at run time, passed the same way

inline bool dtype_known(int dtype) { return dtype == MRFP_F32 || dtype == MRFP_BF16 || dtype == MRFP_F16; }
inline int dtype_bytes(int dtype) { return dtype == MRFP_F32 ? 4 : 2; }      // of a known dtype: check dtype_known first

template <typename F> inline int by_dtype16(int dtype, const char* who, F&& f) {
    if (dtype == MRFP_BF16) return f(Tag<bf16>{});
    if (dtype == MRFP_F16) return f(Tag<f16>{});
    MRFP_CHECK(false, "%s: 16-bit activations only (dtype %d)", who, dtype);
}
template <typename F> inline int by_dtype(int dtype, const char* who, F&& f) {
    if (dtype == MRFP_F32) return f(Tag<float>{});
    if (dtype == MRFP_BF16) return f(Tag<bf16>{});
    if (dtype == MRFP_F16) return f(Tag<f16>{});
    MRFP_CHECK(false, "%s: unknown dtype %d", who, dtype);
}

// The vector width of a launch: the full 16-byte instance KFULL when `vec`, else the scalar instance KONE (each a parenthesised
// kernel instance), on kThreads threads; returns -2 from the caller when the launch fails.  MRFP_DISPATCH_VEC is the common case,
// KERNEL<T, FullVec<T>::value> when the channel count makes whole vectors and `ok` (alignment, pitches) holds, else KERNEL<T, 1>.
#define MRFP_LAUNCH_VEC(vec, KFULL, KONE, grid, st, ...)                                \
    do {                                                                                \
        if (vec) hipLaunchKernelGGL(KFULL, grid, dim3(kThreads), 0, st, __VA_ARGS__);   \
        else hipLaunchKernelGGL(KONE, grid, dim3(kThreads), 0, st, __VA_ARGS__);        \
        MRFP_LAUNCH_CHECK();                                                            \
    } while (0)
#define MRFP_DISPATCH_VEC(T, C, ok, KERNEL, grid, st, ...) \
    MRFP_LAUNCH_VEC(pick_vec<T>(C) > 1 && (ok), (KERNEL<T, FullVec<T>::value>), (KERNEL<T, 1>), grid, st, __VA_ARGS__)

inline int lines_per_image(int64_t B, int64_t Ho) {
    // ~1024 workgroups over the chip (4 per CU, 16 waves/CU, 4 independent 16-byte loads per lane in the
    // statistics kernels): enough bytes in flight to cover HBM latency, few enough partial sums that the
    // finalize kernels stay in the microseconds.
    static const int set = env_switch("MRFP_ROW_BLOCKS", 2048);
    const int total = set < 64 ? 2048 : set;
    int64_t cap = total / (B > 0 ? B : 1);
    if (cap < 1) cap = 1;
    if (Ho <= cap) return (int)Ho;
    // every workgroup the same number of lines (the last few one less): 192 lines over 128 workgroups gave half of them two lines and
    // half one -- the launch ran as long as the two-line workgroups (round 4: 96 x 2 lines, normalisation family -0.3 ms per step)
    const int64_t per = (Ho + cap - 1) / cap;
    return (int)((Ho + per - 1) / per);
}

}  // namespace mrfp
