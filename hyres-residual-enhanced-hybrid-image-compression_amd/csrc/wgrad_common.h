// Device code shared by the weight-gradient kernels of wgrad.hip: the kernel arguments, the block order and decode,
// a group's chunk share, the halo kernels' tile constants and chunk / element decode, the bias gradient's block
// reduce, the slab stores, and the 16-bit kernels' transposed read and its lane address. Each kernel keeps its own
// load / stage schedule and MFMA loop and calls these for the rest.
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

// lanes per block row of the split reduce (wgrad.hip) for `total` outputs in nsplit partials
int wgrad_reduce_lanes(long long total, int nsplit);

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

// G groups of 4 waves share one pixel split: group gq takes the contiguous chunks [kb, ke) of the split's
// [kb0, ke0); every group runs ``share`` barrier steps (a group with fewer chunks idles through its last ones).
struct GroupShare {
    int share, kb, ke;
};
template <int G>
__device__ __forceinline__ GroupShare group_share(const WgradArgs& a, int split, int gq) {
    const int kb0 = split * a.chunks_per_split;
    const int ke0 = min(a.nchunks, kb0 + a.chunks_per_split);
    const int share = (max(ke0 - kb0, 0) + G - 1) / G;
    const int kb = min(ke0, kb0 + gq * share);
    return {share, kb, min(ke0, kb + share)};
}

// Tile constants of the halo-staged kernels: a 64 x 64 tile, KR x KW taps DIL apart at Q stride SQ, a P chunk of
// KT pixels and one Q halo of KR rows x HC columns per chunk. PAD: row-pitch padding (4 floats for the fp32 image,
// 32 halves for the 16-bit ones). P_V / H_V: float4 of P / of the halo's H_E quads per thread (256 per group).
template <int KR_, int KW_, int SQ_, int DIL_, int PAD>
struct HaloTile {
    static constexpr int KR = KR_, KW = KW_, SQ = SQ_, DIL = DIL_;
    static constexpr int BM = 64, BN = 64, NT = KR * KW;
    static constexpr int HC = 31 * SQ + DIL * (KW - 1) + 1;  // halo columns of a 32-px chunk
    static constexpr int PP = BM + PAD, PQ = BN + PAD;
    static constexpr int PSZ = KT * PP, HSZ = KR * HC * PQ;
    static constexpr int P_V = KT * BM / 4 / 256;
    static constexpr int H_E = KR * HC * (BN / 4);
    static constexpr int H_V = (H_E + 255) / 256;
};

// Chunk kc (rows are cpr = Wq / 32 chunks wide) -> its row segment (b, i, j0 .. j0 + 31) and first P row q0.
struct HaloChunk {
    int b, i, j0;
    long long q0;
};
__device__ __forceinline__ HaloChunk halo_chunk(const hyres_wgrad_desc& d, int cpr, int kc) {
    const int b = kc / (d.Hq * cpr);
    const int rem = kc - b * d.Hq * cpr;
    const int i = rem / cpr;
    return {b, i, (rem - i * cpr) * 32, (long long)kc * 32};
}

// Staged element e (a channel quad of one halo pixel, row-major KR x HC x BN / 4) of chunk ch -> whether it lies
// inside the halo, the image and N, and its element offset into Q. dh0 / dwg: the halo's first row / column offset.
struct HaloElem {
    bool ok;
    long long off;
};
template <typename T>
__device__ __forceinline__ HaloElem halo_elem(const hyres_wgrad_desc& d, int e, const HaloChunk& ch, int dh0, int dwg,
                                              int n0) {
    const int pix = e / (T::BN / 4), c = (e % (T::BN / 4)) * 4;
    const int hr = pix / T::HC, hc = pix - (pix / T::HC) * T::HC;
    const int ih = ch.i * T::SQ + dh0 + T::DIL * hr, iw = ch.j0 * T::SQ + dwg + hc;
    const bool ok = e < T::H_E && (unsigned)ih < (unsigned)d.Hqq && (unsigned)iw < (unsigned)d.Wqq && n0 + c < d.N;
    return {ok, ((long long)(ch.b * d.Hqq + ih) * d.Wqq + iw) * d.ldq + n0 + c};
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

// Slab store [split][t][M][N] of a halo block's NT taps t0 .. t0 + NT - 1: ``n`` is this lane's column, ``mb`` its
// wave's first row.
template <int NT>
__device__ __forceinline__ void slab_store_taps(const floatx16 (&acc)[NT], const WgradArgs& a, int split, int t0, int mb,
                                                int n, int lh) {
    const hyres_wgrad_desc& d = a.d;
    const long long MN = (long long)d.M * d.N;
    static_for<NT>([&](auto J) {
        constexpr int j = decltype(J)::value;
        if (n < d.N) {
            float* out = a.slab + ((long long)split * d.ntaps + t0 + j) * MN + n;
            slab_store_acc(acc[j], out, mb, lh, d.M, d.N);
        }
    });
}

// Bias gradient: each of the block's THREADS threads holds the column sums ``bsum`` of its staged P rows for channel
// quad threadIdx.x % (BM / 4). Sums each quad's partials through ``red`` (LDS the block no longer reads: the main loop
// ended with a barrier) and stores bias_slab[split][m0 ..] up to M. Block-uniform; no barrier after the reads.
template <int BM, int THREADS>
__device__ __forceinline__ void bias_block_reduce(float4* red, const float4& bsum, float* bias_slab, int split, int m0,
                                                  int M) {
    const int t = threadIdx.x;
    red[t] = bsum;
    __syncthreads();
    if (t < BM / 4) {
        float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int r = 0; r < THREADS / (BM / 4); ++r) {
            const float4 v = red[t + r * (BM / 4)];
            s4.x += v.x; s4.y += v.y; s4.z += v.z; s4.w += v.w;
        }
        float* dst = bias_slab + (long long)split * M + m0 + 4 * t;
        const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
        for (int c = 0; c < 4; ++c)
            if (m0 + 4 * t + c < M) dst[c] = sv[c];
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

// Transposed-read address of a lane within a 16-k step of a [k][channel] tile: lane half lh = lane >> 5 takes k rows
// 8 lh .. 8 lh + 7; in its 16-lane group g, lane 4 q + p supplies row (.. + q), columns 16 g + 4 p .. + 3.
struct TrLane {
    int lh, row, col;
};
__device__ __forceinline__ TrLane tr_lane(int lane) {
    const int lh = lane >> 5, lg = (lane >> 4) & 1, lq = (lane >> 2) & 3, lp = lane & 3;
    return {lh, 8 * lh + lq, 16 * lg + 4 * lp};
}

}  // namespace hyres
