// Internal helpers shared by the libhyres_hip translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <type_traits>

#include "hyres_hip.h"

namespace hyres {

int set_error(int code, const char* fmt, ...);
int ok();

inline hipStream_t as_stream(hyres_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

inline int launch_status(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error((int)e, "%s: %s", what, hipGetErrorString(e));
    return ok();
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
// a 4-element vector of the operand: 8 B as fp16, 16 B as fp32
inline bool aligned_v4(const void* p, bool half) { return half ? aligned8(p) : aligned16(p); }

inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// The kernels that finish per-block partials, one per summation order (pointwise.hip; DESIGN "Reduction orders"). Each
// thread of one 256-thread block walks the partials i = tid, tid + 256, ...; block_sum256 folds the 256 sums.
//   prelu_slope_sum:   dst[0] += sum, one running sum per thread (the conv PReLU-mask epilogues, hyres_se_bwd_prelu)
//   sum_partials8:     out[0] (+)= sum, eight running sums per thread, eight loads in flight, paired at the end
//   sum_partials_cols: one block per column k of part[nb][stride]: (k < n0 ? dst0[k] : dst1[k - n0]) += sum_i part[i][k]
int prelu_slope_sum(const void* partials, int n, const void* dst, hipStream_t st);
int sum_partials8(const float* part, int n, float* out, int accumulate, hipStream_t st, const char* what);
int sum_partials_cols(const float* part, int nb, int stride, float* dst0, int n0, float* dst1, int n1, hipStream_t st,
                      const char* what);

// Operand dtypes of the element-wise and MultiScaleRefine entry points (HYRES_DT_*, hyres_hip.h). The masks that have
// kernels: fp32, fp16 saved activations, fp16 activations with fp16 gradients. dispatch_hg calls f(H, G) with the two
// flags as std::bool_constant values, which serve as template arguments inside f.
inline bool dt_valid(int dt) { return dt == 0 || dt == HYRES_DT_ACT16 || dt == (HYRES_DT_ACT16 | HYRES_DT_GRAD16); }
inline bool f16_valid(int f16) { return f16 == 0 || f16 == 1; }
template <class F>
inline int dispatch_hg(int dt, F&& f) {
    if (dt & HYRES_DT_GRAD16) return f(std::true_type{}, std::true_type{});
    if (dt & HYRES_DT_ACT16) return f(std::true_type{}, std::false_type{});
    return f(std::false_type{}, std::false_type{});
}

// f(A, B) with two independent flags as std::bool_constant values: every combination
template <class F>
inline int dispatch_bool2(bool a, bool b, F&& f) {
    if (a) return b ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    return b ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

typedef float floatx16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }

typedef _Float16 half4_t __attribute__((ext_vector_type(4)));

// activation element / float4 access: fp32, or fp16 storage in HBM (H, autocast inference) with fp32 arithmetic
template <bool H>
__device__ __forceinline__ float ldv(const float* p, long long i) {
    if constexpr (H) return (float)reinterpret_cast<const _Float16*>(p)[i];
    else return p[i];
}
template <bool H>
__device__ __forceinline__ void stv(float* p, long long i, float v) {
    if constexpr (H) reinterpret_cast<_Float16*>(p)[i] = (_Float16)v;
    else p[i] = v;
}
template <bool H>
__device__ __forceinline__ float4 ldv4(const float* p, long long i) {
    if constexpr (H) {
        const half4_t h = *reinterpret_cast<const half4_t*>(reinterpret_cast<const _Float16*>(p) + i);
        return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
    } else {
        return ld4(p + i);
    }
}
template <bool H>
__device__ __forceinline__ void stv4(float* p, long long i, float4 v) {
    if constexpr (H) {
        const half4_t h = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
        *reinterpret_cast<half4_t*>(reinterpret_cast<_Float16*>(p) + i) = h;
    } else {
        *reinterpret_cast<float4*>(p + i) = v;
    }
}

}  // namespace hyres

#define HY_REQUIRE(cond, code, ...)                                  \
    do {                                                             \
        if (!(cond)) return ::hyres::set_error((code), __VA_ARGS__); \
    } while (0)

#define HY_REQUIRE_DT(dt, op)                                                                                         \
    HY_REQUIRE(::hyres::dt_valid(dt), HYRES_E_ARG,                                                                    \
               op ": dt %d: 0, ACT16 or ACT16 | GRAD16 (no fp16 gradients of fp32 activations)", (dt))
#define HY_REQUIRE_F16(f16, op) HY_REQUIRE(::hyres::f16_valid(f16), HYRES_E_ARG, op ": f16 %d: 0 or 1", (f16))

#define HY_LAUNCH_CHECK(name) ::hyres::launch_status(name)
