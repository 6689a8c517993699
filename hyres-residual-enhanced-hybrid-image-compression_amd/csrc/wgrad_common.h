// Device code shared by the weight-gradient kernels of wgrad.hip: the kernel arguments, the block order and decode,
// the accumulator's slab store, and the bf16x6 / fp16 kernels' staging and transposed-read pieces. Each kernel keeps
// its own load / stage schedule and calls these for the rest.
#pragma once
#include "conv_common.h"

namespace hyres {

struct WgradArgs {
    hyres_wgrad_desc d;
    const float* p;
    const float* q;
    float* slab;  // [nsplit][ntaps][M][N]
    int chunks_per_split;
    int nchunks;
    int mtiles, ntiles, ngroups;
    int nblocks;  // logical blocks (grid padded to a multiple of 8 for the XCD remap)
    int tapn;
    float* bias_slab;  // [nsplit][M] column sums of P (the bias gradient) or NULL
};

template <typename F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
    (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// XCD-aware block order: hardware block b runs on XCD b % 8, so each XCD gets a contiguous range of logical
// blocks and the blocks of one pixel split, which share P/Q rows, hit one XCD's L2. The grid is padded to a
// multiple of 8: a block whose logical index is >= a.nblocks has nothing to do and returns.
__device__ __forceinline__ int wgrad_logical_block() {
    const int bid = blockIdx.x;
    return (bid & 7) * (gridDim.x >> 3) + (bid >> 3);
}

// Logical block lb -> its tile: m tile fastest, then n tile, then tap group, then pixel split.
// GROUPS = false: the kernel has no tap groups (grp = 0).
struct WgradBlock {
    int nt, grp, split, m0, n0;
};
template <int BM, int BN, bool GROUPS>
__device__ __forceinline__ WgradBlock wgrad_block(const WgradArgs& a, int lb) {
    int rr = lb;
    const int mt = rr % a.mtiles; rr /= a.mtiles;
    const int nt = rr % a.ntiles; rr /= a.ntiles;
    const int grp = GROUPS ? rr % a.ngroups : 0;
    const int split = GROUPS ? rr / a.ngroups : rr;
    return {nt, grp, split, mt * BM, nt * BN};
}

// Slab store of one 32x32 MFMA accumulator (v_mfma_f32_32x32x2_f32, and the 32x32x16 f16 / bf16 ones alike): a
// lane holds column lane & 31 of the tile; its 16 registers are four groups of 4 consecutive rows, 8 rows apart,
// the upper lane half (lh = lane >> 5) 4 rows below the lower.
// ``col`` points at (row 0, this lane's column) of one tap's [M][N] slab, ``mb`` is the accumulator's first row.
__device__ __forceinline__ void slab_store_acc(const floatx16& acc, float* col, int mb, int lh, int M, int N) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = mb + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m < M) col[(long long)m * N] = acc[r];
    }
}

typedef __fp16 fp16x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ halfx4_t lds_tr4(const _Float16* p) {
    fp16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)(p));
    return __builtin_bit_cast(halfx4_t, v);
}

// One A / B operand of a 32x32x16 MFMA from a [k][channel] LDS tile of 16-bit values: 8 consecutive k of this
// lane's row / column, as two transposed reads (ds_read_b64_tr_b16) 4 * pitch apart
__device__ __forceinline__ halfx8_t tr_frag(const _Float16* p, int pitch) {
    const halfx4_t lo = lds_tr4(p), hi = lds_tr4(p + 4 * pitch);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ bf16x8_t tr_frag(const __bf16* p, int pitch) {
    return __builtin_bit_cast(bf16x8_t, tr_frag(reinterpret_cast<const _Float16*>(p), pitch));
}

}  // namespace hyres
