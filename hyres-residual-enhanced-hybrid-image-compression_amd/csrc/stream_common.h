// Device code shared by the per-wave streaming 1x1 kernels of conv_stream.hip: conv1x1_stream_kernel,
// conv1x1_stream_h_kernel, conv1x1_stream_hf_kernel and conv1x1_stream_b6_kernel. All four stage W [Co][K] in LDS
// once per persistent block and then let every WAVE stream its own 32-pixel tiles (C^T = W X^T) with no block barrier.
// Here are the lane / tile bookkeeping with its two out-of-range-safe byte offsets (all four), the one-time weight and
// bias staging (all four, one converter each), and what only
// the kernels with streamed epilogue operands use (hf, b6): the accumulator's trip through per-wave LDS scratch from
// the MFMA layout to pixel rows, the per-pixel SA_BWD operand loads, the epilogue arithmetic on a 4-channel group and
// the PReLU-mask block reduction. conv1x1_stream_kernel and conv1x1_stream_h_kernel keep their own bias + activation
// step: through StreamEpi::apply the first one's tile loop came out with a different shape (half the instructions).
// Each kernel keeps its own load / MFMA / prefetch schedule, its register sets, launch bounds, waves_per_eu attribute
// and VGPR guard, and calls these for the rest.
#pragma once
#include "conv_common.h"

namespace hyres {

typedef _Float16 half8s_t __attribute__((ext_vector_type(8)));

constexpr int STREAM_OOR = (int)0x80000000;  // a buffer-load offset past every resource: the load returns 0

// ---- lane and tile bookkeeping. Wave gw of the grid's nw takes tiles gw, gw + nw, ... of the ntile 32-pixel tiles.
// MFMA layout: lane (lr, lh) holds pixel 32 tile + lr, channels ... + 4 lh; row layout (the coalesced epilogues): lane
// (cr, cc) holds pixel 32 tile + cr + 8q, channels ... + cc .. cc + 3 for q < 4, i.e. one instruction covers 8 pixel
// rows x 32 contiguous channels.
struct StreamWalk {
    int lane, wave, lr, lh, cr, cc, gw, nw, ntile;
    const int& M;  // ConvArgs::M itself, read where it is used: a copy held in a register for the whole kernel moved the
                   // VGPR allocation of conv1x1_stream_hf_kernel<2, 8, 5> and <4, 4, 1> by a granule
    // byte offset of element `col` of this lane's pixel row (ld elements of es bytes), STREAM_OOR past the last tile
    // or pixel
    __device__ __forceinline__ int mfma_off(int tile, int ld, int col, int es) const {
        const int p = tile * 32 + lr;
        return (tile < ntile && p < M) ? (p * ld + col) * es : STREAM_OOR;
    }
    __device__ __forceinline__ int row_off(int tile, int q, int ld, int col, int es) const {
        const int p = tile * 32 + cr + 8 * q;
        return (tile < ntile && p < M) ? (p * ld + col) * es : STREAM_OOR;
    }
};
__device__ __forceinline__ StreamWalk stream_walk(const int& M) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    return {lane, wave, lane & 31, lane >> 5, lane >> 3, 4 * (lane & 7), (int)blockIdx.x * 4 + wave, (int)gridDim.x * 4,
            (M + 31) / 32, M};
}

// ---- one-time staging: W [CO][K] -> LDS through put(co, k, the float4 at W[co][k .. k + 3]), the bias -> bs[CO]
template <int CO, int K, class Put>
__device__ __forceinline__ void stream_stage_weights(const float* w2, int ldw, Put put) {
    for (int i = threadIdx.x; i < CO * (K / 4); i += 256) {
        const int co = i / (K / 4), k4 = i - co * (K / 4);
        put(co, 4 * k4, ld4(w2 + (long long)co * ldw + 4 * k4));
    }
}
template <int CO>
__device__ __forceinline__ void stream_stage_bias(float* bs, const hyres_epilogue& e) {
    for (int i = threadIdx.x; i < CO; i += 256) bs[i] = e.bias ? e.bias[i] : 0.f;
}

__device__ __forceinline__ float4 round_f16(float4 v) {
    return make_float4((float)(_Float16)v.x, (float)(_Float16)v.y, (float)(_Float16)v.z, (float)(_Float16)v.w);
}
// the converters, rows of KP elements: fp32 (R16: rounded through fp16), fp16, three bf16 planes WPL apart
template <int KP, bool R16>
struct StreamPutF32 {
    float* Ws;
    __device__ __forceinline__ void operator()(int co, int k, float4 w) const { st4(&Ws[co * KP + k], R16 ? round_f16(w) : w); }
};
template <int KP>
struct StreamPutF16 {
    _Float16* Ws;
    __device__ __forceinline__ void operator()(int co, int k, float4 w) const {
        *reinterpret_cast<half4_t*>(&Ws[co * KP + k]) = half4_t{(_Float16)w.x, (_Float16)w.y, (_Float16)w.z, (_Float16)w.w};
    }
};
template <int KP, int WPL>
struct StreamPutBf6 {
    __bf16* Ws;
    __device__ __forceinline__ void operator()(int co, int k, float4 w) const { bf6_put3<WPL>(Ws, co * KP + k, w); }
};

// ---- accumulator -> pixel rows: a wave's 32 x 32 co tile goes to its scratch es[32 * STREAM_EP] in the MFMA layout
// and comes back as rows (pitch 36 floats: the MFMA-layout float4 writes of 16 lanes land on 16 distinct 4-bank
// groups). LDS instructions of one wave execute in order: the fences only keep the compiler from moving the previous
// co tile's reads past these writes or these writes past the reads that follow
constexpr int STREAM_EP = 36;
__device__ __forceinline__ void stream_rows_put(float* es, const StreamWalk& w, const floatx16& acc) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
    for (int q = 0; q < 4; ++q)
        st4(&es[w.lr * STREAM_EP + 8 * q + 4 * w.lh], make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]));
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ float4 stream_rows_get(const float* es, const StreamWalk& w, int q) {
    return ld4(&es[(w.cr + 8 * q) * STREAM_EP + w.cc]);
}

// ---- SA_BWD's per-pixel operands of one tile in the row layout: (d mean / C, d max) pairs aux0 [P][ld0] and the argmax
// channel aux2 [P]. (ROWSCALE's scale, four 4-byte loads, stays a lambda in each kernel: through a function here
// conv1x1_stream_hf_kernel<2, 12, 16> allocated 128 VGPRs instead of 120.)
__device__ __forceinline__ void stream_load_sab(const StreamWalk& w, __amdgpu_buffer_rsrc_t r_gm, __amdgpu_buffer_rsrc_t r_am,
                                                int ld0, int tile, float2 (&gm)[4], int (&am)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        gm[q] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(r_gm, w.row_off(tile, q, ld0, 0, 4), 0, 0));
        am[q] = __builtin_bit_cast(int, __builtin_amdgcn_raw_buffer_load_b32(r_am, w.row_off(tile, q, 1, 0, 4), 0, 0));
    }
}

// ---- epilogue arithmetic on channels n .. n + 3 of one pixel. F: residual (1) | ReLU mask (2) | accumulate (4) |
// SA_BWD (8) | ROWSCALE (16) | PReLU mask (32); only the operands F names are read, so a caller fills those alone and
// leaves the other members of StreamOpnd unset.
struct StreamOpnd {
    float4 res, mask, old, pre;  // residual, the ReLU mask's y, old y, the PReLU mask's pre-activation
    float2 gm;                   // SA_BWD: d mean / C, d max
    int mi;                      //         argmax channel
    float sc;                    // ROWSCALE
};
struct StreamEpi {
    int act;
    float slope;     // HYRES_ACT_PRELU's
    float pm_slope;  // the PReLU mask's
    float pslope;    // PReLU mask: this thread's share of sum_{pre <= 0} pre * gradient

    // av: the accumulator quad, b4: the bias. In epi_store4's order: SA_BWD (acc + d mean / C) + (channel == argmax ?
    // d max : 0), or ROWSCALE (acc * scale) + bias, or acc + bias; the PReLU mask where pm_on (as prelu_bwd4_kernel on
    // the stored gradient — PM_R16: that gradient is stored as fp16, so it is rounded first); + residual; out2(the
    // pre-activation); ReLU mask / ReLU / PReLU (PRELU: compiled in); + old y.
    template <int F, bool PM_R16, bool PRELU, class Out2>
    __device__ __forceinline__ float4 apply(float4 av, float4 b4, int n, const StreamOpnd& op, bool pm_on, Out2 out2) {
        float o[4];
        if constexpr ((F & 8) != 0) {
            const float a4[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = a4[c] + op.gm.x + (n + c == op.mi ? op.gm.y : 0.f);
        } else if constexpr ((F & 16) != 0) {
            o[0] = av.x * op.sc + b4.x; o[1] = av.y * op.sc + b4.y; o[2] = av.z * op.sc + b4.z; o[3] = av.w * op.sc + b4.w;
        } else {
            o[0] = av.x + b4.x; o[1] = av.y + b4.y; o[2] = av.z + b4.z; o[3] = av.w + b4.w;
        }
        if constexpr ((F & 32) != 0) {
            if (pm_on) {
                const float pv[4] = {op.pre.x, op.pre.y, op.pre.z, op.pre.w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if constexpr (PM_R16) o[c] = (float)(_Float16)o[c];
                    if (!(pv[c] > 0.f)) pslope += pv[c] * o[c];
                    o[c] = pv[c] > 0.f ? o[c] : pm_slope * o[c];
                }
            }
        }
        if constexpr ((F & 1) != 0) { o[0] += op.res.x; o[1] += op.res.y; o[2] += op.res.z; o[3] += op.res.w; }
        out2(make_float4(o[0], o[1], o[2], o[3]));
        if constexpr ((F & 2) != 0) {
            o[0] = op.mask.x > 0.f ? o[0] : 0.f;
            o[1] = op.mask.y > 0.f ? o[1] : 0.f;
            o[2] = op.mask.z > 0.f ? o[2] : 0.f;
            o[3] = op.mask.w > 0.f ? o[3] : 0.f;
        } else if (act == HYRES_ACT_RELU) {
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = fmaxf(o[c], 0.f);
        } else if (PRELU && act == HYRES_ACT_PRELU) {
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = o[c] >= 0.f ? o[c] : slope * o[c];
        }
        if constexpr ((F & 4) != 0) { o[0] += op.old.x; o[1] += op.old.y; o[2] += op.old.z; o[3] += op.old.w; }
        return make_float4(o[0], o[1], o[2], o[3]);
    }

    // the PReLU mask's block partial: wave sums (xor shuffles), then the four waves' in a fixed order -> dst[block]
    __device__ __forceinline__ void reduce_pslope(const StreamWalk& w, float (&pred)[4], float* dst) {
        for (int off = 32; off > 0; off >>= 1) pslope += __shfl_xor(pslope, off);
        if (w.lane == 0) pred[w.wave] = pslope;
        __syncthreads();
        if (threadIdx.x == 0) dst[blockIdx.x] = (pred[0] + pred[1]) + (pred[2] + pred[3]);
    }
};

}  // namespace hyres
