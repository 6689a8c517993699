// Device code shared by the halo-tiled 3x3 kernels: conv3x3_halo_f16_kernel, conv3x3_wres_f16_kernel,
// conv3x3_wres_f32_kernel and conv3x3_wres_bf6_kernel (conv.hip) and ru_fused_f16_kernel (ru_fused.hip). All five
// compute 4-row x 64-pixel output tiles from a (4 + 2D) x (64 + 2D) input halo staged in LDS; here are the tile
// geometry, the persistent kernels' tile walk, the halo address, the f16 halo staging, the fp32 kernels'
// fused-operand epilogue and the weight-slice decode. Each kernel keeps its own load / stage / MFMA schedule, its
// launch bounds and its VGPR guard, and calls these for the rest.
#pragma once
#include "conv_common.h"

namespace hyres {

// ---- tile geometry: HALO_R x HALO_TW output pixels, a halo of radius D around them
constexpr int HALO_R = 4, HALO_TW = 64;
constexpr int HALO_PH = 40;  // halves per staged pixel of the f16 kernels (32 channels + 8 pad: 80-B pitch)
constexpr int halo_hw(int D) { return HALO_TW + 2 * D; }                  // halo row length, pixels
constexpr int halo_npx(int D) { return (HALO_R + 2 * D) * halo_hw(D); }  // halo pixels (396 at D = 1)
// 4-channel vectors of one halo chunk of 4 * V4 channels, and the most of them one of NT threads holds
constexpr int halo_elems(int D, int V4) { return halo_npx(D) * V4; }
constexpr int halo_per_thread(int D, int V4, int NT) { return (halo_elems(D, V4) + NT - 1) / NT; }

// xcd_logical_block (the XCD-aware block order): conv_common.h

// ---- tile walk of the persistent kernels: block bg of the nb blocks that share the ntiles tiles (one output-channel
// group). The blocks of one XCD (bg % 8) take one contiguous range of tiles, interleaved, so that vertically adjacent
// tiles (two shared halo rows) run together on it: tile k of this block is tbeg + jx + k * nx, row tiles fastest.
struct HaloTile {
    int b, i0, j0;  // image, first output row and column
};
struct HaloWalk {
    int tbeg, jx, nx, mytiles, nrt, nct;
    __device__ __forceinline__ HaloTile tile(int k) const {
        int l = tbeg + jx + k * nx;
        const int rt = l % nrt; l /= nrt;
        const int ct = l % nct;
        return {l / nct, rt * HALO_R, ct * HALO_TW};
    }
};
__device__ __forceinline__ HaloWalk halo_walk(int bg, int nb, int ntiles, int nrt, int nct) {
    const int xcd = bg & 7, nx = (nb + 7 - xcd) >> 3, jx = bg >> 3;  // blocks of this XCD, index among them
    const int q = ntiles >> 3, r8 = ntiles & 7;
    const int tbeg = xcd * q + min(xcd, r8), tcnt = q + (xcd < r8 ? 1 : 0);
    return {tbeg, jx, nx, jx < tcnt ? (tcnt - 1 - jx) / nx + 1 : 0, nrt, nct};
}

// ---- halo address: element e of a chunk = 4-channel vector e % V4 of halo pixel e / V4 of the tile at (i0, j0);
// its byte offset for a buffer load (elem0: element offset of the image and chunk, ES: element size), or
// 0x80000000 (out of range: the load returns 0) outside the image or past the chunk
template <int D, int V4>
__device__ __forceinline__ int halo_offset(int e, int i0, int j0, int Hi, int Wi, int ldx, int elem0, int ES) {
    static_assert(V4 == 4 || V4 == 8, "16 or 32 channels per chunk");
    const int px = e >> (V4 == 8 ? 3 : 2), c4 = e & (V4 - 1);
    const int hr = px / halo_hw(D), hc = px - hr * halo_hw(D);
    const int ih = i0 - D + hr, iw = j0 - D + hc;
    const bool ok = e < halo_elems(D, V4) && (unsigned)ih < (unsigned)Hi && (unsigned)iw < (unsigned)Wi;
    return ok ? (elem0 + (ih * Wi + iw) * ldx + 4 * c4) * ES : (int)0x80000000;
}

// ---- f16 halo staging (D = 1, 32-channel chunks): thread tid of NT holds elements e0 + NT * v below `end`, e0 = tid
// plus the first element of its staging part. XH: X is fp16 (raw halves until the LDS store), else fp32 (converted at
// the store). The LDS image is [pixel][HALO_PH]. Used by conv3x3_halo_f16_kernel (NT = 256, three parts per chunk) and
// ru_fused_f16_kernel (NT = 512); conv3x3_wres_f16_kernel keeps its own loops over halo_offset (IO 2 spilled through these).
template <bool XH>
using HaloReg = std::conditional_t<XH, half4_t, float4>;

template <bool XH, int NT, int NV>
__device__ __forceinline__ void halo16_load(HaloReg<XH> (&h)[NV], __amdgpu_buffer_rsrc_t xr, int e0, int end, int i0,
                                            int j0, int Hi, int Wi, int ldx, int elem0) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int e = e0 + NT * v;
        const int off = e < end ? halo_offset<1, 8>(e, i0, j0, Hi, Wi, ldx, elem0, XH ? 2 : 4) : (int)0x80000000;
        if constexpr (XH) h[v] = __builtin_bit_cast(half4_t, __builtin_amdgcn_raw_buffer_load_b64(xr, off, 0, 0));
        else h[v] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
    }
}
template <bool XH, int NT, int NV>
__device__ __forceinline__ void halo16_store(_Float16* buf, const HaloReg<XH> (&h)[NV], int e0, int end) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int e = e0 + NT * v;
        if (e < end) {
            half4_t hh;
            if constexpr (XH) hh = h[v];
            else hh = half4_t{(_Float16)h[v].x, (_Float16)h[v].y, (_Float16)h[v].z, (_Float16)h[v].w};
            *reinterpret_cast<half4_t*>(&buf[(e >> 3) * HALO_PH + 4 * (e & 7)]) = hh;
        }
    }
}

// The f16 tap loop (9 taps x 2 k-steps x 2 pixel tiles) of conv3x3_wres_f16_kernel and ru_fused_f16_kernel is NOT
// shared: as one inlined function it made ru_fused_f16_kernel spill (60 B of scratch, 228 -> 256 VGPRs without the
// guard), so both kernels keep their own copy.

// ---- fused-operand epilogue of the fp32 weight-resident kernels (BIAS kind: bias, residual, pre-activation store,
// ReLU / PReLU / ReLU-mask, accumulate; PMASK: also HYRES_ACT_PRELU_MASK). Every operand it reads (bias, residual,
// mask, old y) goes through a buffer resource — an absent operand gets an empty one, so its loads return 0 with no
// branch. request() issues the 16 loads; the caller places it at the START of a tile's last chunk, BEFORE the next
// halo's loads (vmcnt retires loads in issue order, so waiting for these does not wait for that halo too); apply()
// consumes them after that chunk's MFMAs. The generic epi_store4 issued each load behind its own branch and waited
// on it (~8 serialised HBM round trips per tile; +14 % on a 3x3 with a residual).
// A lane holds, per register quad qd, the 4 consecutive channels n0 + 8 qd + 4 lh .. + 3 of output pixel pix.
template <bool PMASK>
struct WresEpi {
    __amdgpu_buffer_rsrc_t r_bias, r_res, r_mask, r_old;
    float slope;
    float pslope;  // PMASK: this thread's share of sum_{pre <= 0} pre * gradient
    float4 bias[4], res[4], mask[4], old[4];

    __device__ __forceinline__ WresEpi(const hyres_epilogue& e, const hyres_conv_geom& g, const float* y) {
        const bool pm = PMASK && e.act == HYRES_ACT_PRELU_MASK;
        slope = (e.act == HYRES_ACT_PRELU || pm) ? e.slope[0] : 0.f;
        pslope = 0.f;
        const long long npix = (long long)g.B * g.Ho * g.Wo;
        r_bias = opnd_rsrc(e.bias, (long long)g.Co * 4);
        r_res = opnd_rsrc(e.res, npix * e.ldres * 4);
        r_mask = opnd_rsrc((e.act == HYRES_ACT_RELU_MASK || pm) ? e.aux0 : nullptr, npix * e.ld0 * 4);
        r_old = opnd_rsrc(e.accumulate ? y : nullptr, npix * g.ldy * 4);
    }
    __device__ __forceinline__ void request(const hyres_epilogue& e, int ldy, long long pix, bool row_ok, int n0, int lh) {
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            const int n = n0 + 8 * qd + 4 * lh;
            const int ob = n * 4;
            const int orr = row_ok ? (int)((pix * e.ldres + n) * 4) : (int)0x80000000;
            const int om = row_ok ? (int)((pix * e.ld0 + n) * 4) : (int)0x80000000;
            const int oy = row_ok ? (int)((pix * ldy + n) * 4) : (int)0x80000000;
            bias[qd] = bload4(r_bias, ob);
            res[qd] = bload4(r_res, orr);
            mask[qd] = bload4(r_mask, om);
            old[qd] = bload4(r_old, oy);
        }
    }
    __device__ __forceinline__ void apply(const floatx16& acc, const hyres_epilogue& e, float* y, int ldy, long long pix,
                                          bool row_ok, int n0, int lh) {
        if (!row_ok) return;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            const int n = n0 + 8 * qd + 4 * lh;
            float o[4] = {acc[4 * qd] + bias[qd].x + res[qd].x, acc[4 * qd + 1] + bias[qd].y + res[qd].y,
                          acc[4 * qd + 2] + bias[qd].z + res[qd].z, acc[4 * qd + 3] + bias[qd].w + res[qd].w};
            if (e.out2) st4(e.out2 + pix * e.ldo2 + n, make_float4(o[0], o[1], o[2], o[3]));
            if (e.act == HYRES_ACT_RELU) {
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = fmaxf(o[k], 0.f);
            } else if (e.act == HYRES_ACT_PRELU) {
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = o[k] >= 0.f ? o[k] : slope * o[k];
            } else if (e.act == HYRES_ACT_RELU_MASK) {
                o[0] = mask[qd].x > 0.f ? o[0] : 0.f;
                o[1] = mask[qd].y > 0.f ? o[1] : 0.f;
                o[2] = mask[qd].z > 0.f ? o[2] : 0.f;
                o[3] = mask[qd].w > 0.f ? o[3] : 0.f;
            } else if (PMASK && e.act == HYRES_ACT_PRELU_MASK) {  // as prelu_bwd4_kernel, per element
                const float pv[4] = {mask[qd].x, mask[qd].y, mask[qd].z, mask[qd].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (!(pv[k] > 0.f)) pslope += pv[k] * o[k];
                    o[k] = pv[k] > 0.f ? o[k] : slope * o[k];
                }
            }
            st4(y + pix * ldy + n, make_float4(o[0] + old[qd].x, o[1] + old[qd].y, o[2] + old[qd].z, o[3] + old[qd].w));
        }
    }
};

// ---- weight-slice decode of the weight-resident kernels' one-time staging: vector f of a slice of W2[co][t][ci]
// (Ci = 64, 16 float4 per tap) -> output channel within the slice, tap, first of its 4 input channels
struct WresWeightIndex {
    int co, t, ci;
};
__device__ __forceinline__ WresWeightIndex wres_weight_index(int f) {
    const int co = f / 144, rem = f - co * 144;
    return {co, rem >> 4, 4 * (rem & 15)};
}

}  // namespace hyres
