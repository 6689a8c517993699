// Device code shared by the pointwise / reduction kernels (pointwise.hip, refine.hip, vgg.hip, entropy.hip and conv.hip's
// slope partials): the grid-stride walk and its grid sizes, the 256-thread LDS tree sum and the PReLU backward per
// element. The summation order of every reduction here is part of the contract (DESIGN "Reduction orders"): fused and
// unfused paths give bit-identical losses because they share these definitions.
#pragma once
#include "common.h"

#include <algorithm>

namespace hyres {

#define GRID_STRIDE(i, n) \
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)

// 256-thread blocks over n elements, per_thread elements each, at most 8192 blocks
inline int grid_for(long long n, int per_thread = 1) {
    return (int)std::max<long long>(1, std::min<long long>((n / per_thread + 255) / 256, 8192));
}
// the PW_UNR-unrolled pointwise kernels: each thread takes PW_UNR float4 per pass, 8 blocks of 256 per CU resident
constexpr int PW_UNR = 4;  // float4 per thread in flight
inline int pw_grid(long long n4) {
    return (int)std::max<long long>(1, std::min<long long>((n4 + 256LL * PW_UNR - 1) / (256LL * PW_UNR), 2048));
}

// Sum of v over a 256-thread block: a binary tree over red[256] (128, 64, ..., 1), the result in red[0]. Ends on a
// barrier after the last add; a caller that writes red again adds its own barrier after reading the result.
template <class T>
__device__ __forceinline__ T block_sum256(T v, T* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    return red[0];
}

// PReLU backward of one element: the gradient pre > 0 ? g : a * g; pre * g joins the slope sum s when !(pre > 0).
// An fp16-gradient path rounds g to fp16 before the call (the unfused chain's stored value).
__device__ __forceinline__ float prelu_bwd_elem(float pre, float g, float a, float& s) {
    if (!(pre > 0.f)) s += pre * g;
    return pre > 0.f ? g : a * g;
}

}  // namespace hyres
