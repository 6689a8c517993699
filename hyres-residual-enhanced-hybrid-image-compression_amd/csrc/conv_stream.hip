// The per-wave streaming 1x1 convolutions (K = Ci short, Co = 32 * NT): conv1x1_stream_kernel (fp32 / fp16-rounded
// operands on the fp32 MFMA), conv1x1_stream_h_kernel (fp16 I/O, f16 MFMA), conv1x1_stream_hf_kernel (fp16 I/O with
// streamed epilogue operands) and conv1x1_stream_b6_kernel (fp32 I/O, bf16x6, the same operand set), with their
// eligibility rules and launchers. route() and hyres_conv_forward (conv.hip) reach them through the declarations in
// conv_common.h; what the four kernels have in common is in stream_common.h.
#include "stream_common.h"
#include "wgrad_common.h"

namespace hyres {

// ------------------------------------------------------------------------------------------------
// Streaming 1x1 conv (K = Ci <= 128, Co = 32*NT): the K-short pointwise layers of the ResidualUnits /
// RBBs at 64^2..256^2 sit at the fp32 ridge (64-128 FLOP per output element against 8-12 bytes), and the
// tiled kernel (conv_gemm.hip) runs them as lock-stepped blocks (load, then MFMA, then epilogue), so their MFMA and
// HBM phases add instead of overlapping. Here each WAVE streams its own 32-pixel tiles with no block
// barrier after the one-time weight staging:
//   * W [Co][K] sits in LDS for the whole (persistent) block, pitch K+4 (conflict-free ds_read_b128);
//   * the wave's A operand goes HBM -> registers directly in the MFMA layout: lane (r, h) holds pixel
//     p0+r, channels 8j+4h..8j+4h+3 (j < K/8), so a float4 feeds 4 MFMA k-steps; each float4 is reloaded
//     for the wave's next tile right after its last MFMA (rolling prefetch);
//   * the product is formed transposed (C^T = W X^T), so each lane's accumulator holds 4 consecutive
//     channels of one pixel per register quad: the results are stored as float4 straight from the
//     accumulator layout — no LDS round trip.
// Exact fp32 (v_mfma_f32_32x32x2f32), epilogue bias + ReLU / PReLU (+ pre-activation copy). Layers whose
// epilogue streams a second operand (residual, ReLU mask, old y) stay on the tiled kernel: prefetching
// that operand per wave tile doubles the registers (2 waves/SIMD) and measured slower than the tiles
// (128^2 64->128 +res 95 vs 92 us, 64^2 27 vs 24 us; profiles/r2_micro_1x1_stream.txt).
// R16 (autocast, f16_operands): both operands are rounded to fp16 as they are loaded, and the products of
// those fp16 values are formed exactly by the fp32 MFMA with fp32 accumulation — the same arithmetic as the
// f16 MFMA (whose products of fp16 inputs are exact in fp32) up to the summation order. These layers are
// HBM-bound (<= 128 FLOP per output element), so the f16 rate buys nothing and the streaming structure does.
template <int NT, int KC, bool R16 = false>
__global__ __launch_bounds__(256, 2) void conv1x1_stream_kernel(const ConvArgs a) {
    constexpr int K = 8 * KC, KP = K + 4, CO = 32 * NT;
    __shared__ __attribute__((aligned(16))) float Ws[CO * KP];
    const hyres_conv_geom& g = a.g;
    const hyres_epilogue& e = a.e;
    const StreamWalk w = stream_walk(a.M);
    const int lr = w.lr, lh = w.lh, nw = w.nw;
    stream_stage_weights<CO, K>(a.w2, a.ldw, StreamPutF32<KP, R16>{Ws});
    __shared__ __attribute__((aligned(16))) float bs[CO];
    stream_stage_bias<CO>(bs, e);
    const float slope = (e.act == HYRES_ACT_PRELU) ? e.slope[0] : 0.f;
    __syncthreads();

    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, a.x_bytes, 0x00020000);
    auto load_a = [&](int tile, int j) -> float4 { return bload4(xr, w.mfma_off(tile, g.ldx, 8 * j + 4 * lh, 4)); };
    float4 av[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) av[j] = load_a(w.gw, j);
    // GEMM as C^T = W X^T (MFMA A operand = weights, B operand = pixels): lane (r, h) ends up holding
    // pixel p0+r, channels 32t + 8q + 4h .. +3 in acc[t][4q .. 4q+3] -> one float4 per (t, q)
    for (int tile = w.gw; tile < w.ntile; tile += nw) {
        const int p = tile * 32 + lr;
        const bool pok = p < a.M;
        floatx16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        if (a.prio) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            float4 bv[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) bv[t] = *reinterpret_cast<const float4*>(&Ws[(32 * t + lr) * KP + 8 * j + 4 * lh]);
            float4 x = av[j];
            if constexpr (R16) x = round_f16(x);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[t].x, x.x, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[t].y, x.y, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[t].z, x.z, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[t].w, x.w, acc[t], 0, 0, 0);
            }
            av[j] = load_a(tile + nw, j);  // rolling prefetch of the wave's next tile
        }
        if (a.prio) __builtin_amdgcn_s_setprio(0);
        if (!pok) continue;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = 32 * t + 8 * q + 4 * lh;
                const float4 b4 = *reinterpret_cast<const float4*>(&bs[n]);
                float o[4] = {acc[t][4 * q] + b4.x, acc[t][4 * q + 1] + b4.y, acc[t][4 * q + 2] + b4.z,
                              acc[t][4 * q + 3] + b4.w};
                if (e.out2) st4(e.out2 + (long long)p * e.ldo2 + n, make_float4(o[0], o[1], o[2], o[3]));
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (e.act == HYRES_ACT_RELU) o[c] = fmaxf(o[c], 0.f);
                    else if (e.act == HYRES_ACT_PRELU) o[c] = o[c] >= 0.f ? o[c] : slope * o[c];
                }
                st4(a.y + (long long)p * g.ldy + n, make_float4(o[0], o[1], o[2], o[3]));
            }
    }
}

// ------------------------------------------------------------------------------------------------
// Streaming 1x1 conv with fp16 activations in HBM (AMP training / autocast, io_f16 = 3: X and Y / residual / mask /
// old y all fp16), K = Ci in {64, 96, 128}, Co = 32 * NT in {64, 96, 128}, on the f16 MFMA. These layers (the
// ResidualUnits' 1x1 convs and their input-gradients with the ReLU mask and the accumulated residual gradient) are
// HBM-latency-bound on the tiled kernel (64-row blocks of 2-4 K chunks, each load then barrier then MFMA: ~0.3 of
// HBM). Here, as conv1x1_stream_kernel, each WAVE streams its own 32-pixel tiles with no barrier after the one-time
// weight staging (W -> fp16 in LDS, pitch K + 8 halves): the wave's X fragments come HBM -> registers in the MFMA
// layout (lane (r, h): pixel p0 + r, channels 16j + 8h .. + 7, one 16-byte load per k-step) with a rolling prefetch
// of the next tile, and the product is formed transposed (C^T = W X^T) so each lane's accumulator holds 4 consecutive
// channels of one pixel. Layers with a streamed epilogue operand (residual, ReLU mask, old y) stay on the tiles
// (measured: stream_h_cfg). Arithmetic: fp16 operands, fp32 accumulation, fp32 epilogue, one rounding at the fp16
// store — the tiled f16 kernel's, in the same K order.
__device__ __forceinline__ half4_t f2h4(float4 v) { return half4_t{(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w}; }

template <int NT, int KC>
__global__ __launch_bounds__(256, 2) void conv1x1_stream_h_kernel(const ConvArgs a) {
    constexpr int K = 16 * KC, KP = K + 8, CO = 32 * NT;
    __shared__ __attribute__((aligned(16))) _Float16 Ws[CO * KP];
    __shared__ __attribute__((aligned(16))) float bs[CO];
    const hyres_conv_geom& g = a.g;
    const hyres_epilogue& e = a.e;
    const StreamWalk w = stream_walk(a.M);
    const int lr = w.lr, lh = w.lh, nw = w.nw;
    stream_stage_weights<CO, K>(a.w2, a.ldw, StreamPutF16<KP>{Ws});
    stream_stage_bias<CO>(bs, e);
    __syncthreads();

    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, a.x_bytes, 0x00020000);
    _Float16* const y = reinterpret_cast<_Float16*>(a.y);
    auto load_x = [&](int tile, int j) -> half8s_t {
        return __builtin_bit_cast(half8s_t, bload4(xr, w.mfma_off(tile, g.ldx, 16 * j + 8 * lh, 2)));
    };
    half8s_t xv[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) xv[j] = load_x(w.gw, j);
    for (int tile = w.gw; tile < w.ntile; tile += nw) {
        const int p = tile * 32 + lr;
        const bool pok = p < a.M;
        floatx16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const half8s_t x = xv[j];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const half8s_t wv = *reinterpret_cast<const half8s_t*>(&Ws[(32 * t + lr) * KP + 16 * j + 8 * lh]);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wv, x, acc[t], 0, 0, 0);
            }
            xv[j] = load_x(tile + nw, j);  // rolling prefetch of the wave's next tile
        }
        if (!pok) continue;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = 32 * t + 8 * q + 4 * lh;
                const float4 b4 = *reinterpret_cast<const float4*>(&bs[n]);
                float o[4] = {acc[t][4 * q] + b4.x, acc[t][4 * q + 1] + b4.y, acc[t][4 * q + 2] + b4.z,
                              acc[t][4 * q + 3] + b4.w};
                if (e.act == HYRES_ACT_RELU) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) o[c] = fmaxf(o[c], 0.f);
                }
                const half4_t h = {(_Float16)o[0], (_Float16)o[1], (_Float16)o[2], (_Float16)o[3]};
                *reinterpret_cast<half4_t*>(y + (long long)p * g.ldy + n) = h;
            }
    }
}

// ------------------------------------------------------------------------------------------------
// Streaming 1x1 conv with fp16 activations AND streamed epilogue operands (round 6, AMP training: the ResidualUnit /
// RBB tails relu(W x + b + residual) and the input-gradients with the ReLU mask and the accumulated gradient; io_f16 =
// 3, every operand fp16), K = Ci in {64, 128}, Co = 32 * NT in {64, 128}, F: residual (1) | ReLU mask (2) |
// accumulate (4). conv1x1_stream_h_kernel's X stream and f16 products (C^T = W X^T: the tiled kernel's products, bit-
// identical), with conv1x1_stream_b6_kernel's two fixes for the streamed operands: co tile t + 1's operands are in
// flight while co tile t multiplies (two register sets), and every operand / store moves as pixel rows — the
// accumulator goes through a per-wave LDS scratch (MFMA layout in, rows out: lane l -> pixel p0 + (l >> 3) + 8q,
// channels 32t + 4 (l & 7) .. + 3), so an instruction covers 8 pixel rows x 64 contiguous bytes instead of the lane
// layout's 32 rows x 8 B (profiles/r5h_access_probe.txt: the narrow pieces cap a read+write stream near 3 TB/s). The
// round-5 version without the row-shaped epilogue measured 2-10 % slower than the tiles (profiles/r5g_stream_hf_ab.txt).
// Arithmetic: fp16 operands, fp32 accumulation and epilogue ((acc + b) + residual, mask, + old y), one fp16 rounding
// at the store — the tiled f16 kernel's (tests/test_stream_h_gpu.py: bit for bit).
// F & 8 (round 6, AMP training with SpatialAttention folded into MultiScaleRefine's fusion 1x1): HYRES_EPI_SA_BWD, the
// fusion's input-gradient 64 -> 192 (NT = 6, KC = 4) with SpatialAttention's mean / max backward added per pixel —
// acc + d mean / C + (channel == argmax ? d max : 0) (+ old y), epi_store4's SA_BWD arithmetic; the per-pixel operands
// (aux0 [P][ld0] fp32 pairs, aux2 int argmax) roll a tile ahead like the others.
template <int NT, int KC, int F>
__global__ __launch_bounds__(256, 2) void conv1x1_stream_hf_kernel(const ConvArgs a) {
    constexpr int K = 16 * KC, KP = K + 8, CO = 32 * NT;
    constexpr bool RES = (F & 1) != 0, MASK = (F & 2) != 0, ACC = (F & 4) != 0, SAB = (F & 8) != 0;
    static_assert(!SAB || (!RES && !MASK), "SA_BWD: no residual / mask");
    // RS (F & 16, round 6, AMP training with SpatialAttention folded): HYRES_EPI_ROWSCALE, the fusion 1x1 forward
    // 192 -> 64 (NT = 2, KC = 12) — o = acc * aux1[p] + bias, the pre-activation copy to out2 (fp16), then ReLU / PReLU
    // (the PReLU only in this form)
    constexpr bool RS = (F & 16) != 0;
    static_assert(!RS || (!RES && !MASK && !ACC && !SAB), "ROWSCALE: no other operand");
    // PM (F & 32, with SAB): conv1x1_stream_b6_kernel's PReLU mask on channels [0, 64), pre fp16; the gradient is
    // rounded to fp16 first (the unfused chain's stored value)
    constexpr bool PM = (F & 32) != 0;
    static_assert(!PM || (SAB && !ACC), "PReLU mask: the SA_BWD form without accumulate");
    static_assert(NT % 2 == 0, "operands alternate between two register sets per co tile");
    __shared__ __attribute__((aligned(16))) _Float16 Ws[CO * KP];
    __shared__ __attribute__((aligned(16))) float bs[CO];
    __shared__ __attribute__((aligned(16))) float Es[4 * 32 * STREAM_EP];
    const hyres_conv_geom& g = a.g;
    const hyres_epilogue& e = a.e;
    const StreamWalk w = stream_walk(a.M);
    const int lr = w.lr, lh = w.lh, nw = w.nw;
    stream_stage_weights<CO, K>(a.w2, a.ldw, StreamPutF16<KP>{Ws});
    stream_stage_bias<CO>(bs, e);
    __syncthreads();
    const long long npix = a.M;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_res = opnd_rsrc(RES ? e.res : nullptr, npix * e.ldres * 2);
    const __amdgpu_buffer_rsrc_t r_mask = opnd_rsrc(MASK ? e.aux0 : nullptr, npix * e.ld0 * 2);
    const __amdgpu_buffer_rsrc_t r_old = opnd_rsrc(ACC ? a.y : nullptr, npix * g.ldy * 2);
    const __amdgpu_buffer_rsrc_t r_gm = opnd_rsrc(SAB ? e.aux0 : nullptr, npix * e.ld0 * 4);
    const __amdgpu_buffer_rsrc_t r_am = opnd_rsrc(SAB ? e.aux2 : nullptr, npix * 4);
    const __amdgpu_buffer_rsrc_t r_rs = opnd_rsrc(RS ? e.aux1 : nullptr, npix * e.ld1 * 4);
    const __amdgpu_buffer_rsrc_t r_pm = opnd_rsrc(PM ? e.aux1 : nullptr, npix * e.ld1 * 2);
    StreamEpi epi{e.act, (RS && e.act == HYRES_ACT_PRELU) ? e.slope[0] : 0.f, PM ? e.slope[0] : 0.f, 0.f};
    _Float16* const o2 = reinterpret_cast<_Float16*>(e.out2);
    _Float16* const y = reinterpret_cast<_Float16*>(a.y);
    auto load_x = [&](int tile, int j) -> half8s_t {
        return __builtin_bit_cast(half8s_t, bload4(xr, w.mfma_off(tile, g.ldx, 16 * j + 8 * lh, 2)));
    };
    half4_t eres[RES ? 2 : 1][4], emask[MASK ? 2 : 1][4], eold[ACC ? 2 : 1][4], epre[PM ? 2 : 1][4];
    auto load_epi = [&](int tile, int t, int set) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if constexpr (RES) eres[set][q] = bload4h(r_res, w.row_off(tile, q, e.ldres, 32 * t + w.cc, 2));
            if constexpr (MASK) emask[set][q] = bload4h(r_mask, w.row_off(tile, q, e.ld0, 32 * t + w.cc, 2));
            if constexpr (ACC) eold[set][q] = bload4h(r_old, w.row_off(tile, q, g.ldy, 32 * t + w.cc, 2));
            if constexpr (PM) epre[set][q] = bload4h(r_pm, t < 2 ? w.row_off(tile, q, e.ld1, 32 * t + w.cc, 2) : STREAM_OOR);
        }
    };
    // SA_BWD's / ROWSCALE's per-pixel operands: one set per tile, two sets (the next tile's are issued with its X)
    float2 sgm[SAB ? 2 : 1][4];
    int sam[SAB ? 2 : 1][4];
    float srs[RS ? 2 : 1][4];
    auto load_rs = [&](int tile, float (&rs)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int p = tile * 32 + w.cr + 8 * q;
            const bool ok = tile < w.ntile && p < a.M;
            rs[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r_rs, ok ? p * e.ld1 * 4 : STREAM_OOR, 0, 0));
        }
    };
    half8s_t xv[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) xv[j] = load_x(w.gw, j);
    load_epi(w.gw, 0, 0);
    if constexpr (SAB) stream_load_sab(w, r_gm, r_am, e.ld0, w.gw, sgm[0], sam[0]);
    if constexpr (RS) load_rs(w.gw, srs[0]);
    float* const es = Es + w.wave * 32 * STREAM_EP;
    int tset = 0;
    for (int tile = w.gw; tile < w.ntile; tile += nw, tset ^= 1) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int cur = t & 1;
            if (t + 1 < NT) load_epi(tile, t + 1, cur ^ 1);
            else load_epi(tile + nw, 0, cur ^ 1);
            if constexpr (SAB) {
                if (t == NT - 1) {  // constant set indices (a dynamic one puts the arrays in scratch)
                    if (tset) stream_load_sab(w, r_gm, r_am, e.ld0, tile + nw, sgm[0], sam[0]);
                    else stream_load_sab(w, r_gm, r_am, e.ld0, tile + nw, sgm[1], sam[1]);
                }
            }
            if constexpr (RS) {
                if (t == NT - 1) {
                    if (tset) load_rs(tile + nw, srs[0]);
                    else load_rs(tile + nw, srs[1]);
                }
            }
            floatx16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const half8s_t wv = *reinterpret_cast<const half8s_t*>(&Ws[(32 * t + lr) * KP + 16 * j + 8 * lh]);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wv, xv[j], acc, 0, 0, 0);
                if (t == NT - 1) xv[j] = load_x(tile + nw, j);  // the next tile's X after its last use
            }
            stream_rows_put(es, w, acc);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = 32 * t + w.cc;
                const int p = tile * 32 + w.cr + 8 * q;
                StreamOpnd op;
                if constexpr (RES) op.res = h2f4(eres[cur][q]);
                if constexpr (MASK) op.mask = h2f4(emask[cur][q]);
                if constexpr (ACC) op.old = h2f4(eold[cur][q]);
                if constexpr (PM) op.pre = h2f4(epre[cur][q]);
                if constexpr (SAB) {
                    op.gm = tset ? sgm[1][q] : sgm[0][q];
                    op.mi = tset ? sam[1][q] : sam[0][q];
                }
                if constexpr (RS) op.sc = tset ? srs[1][q] : srs[0][q];
                const float4 o = epi.apply<F, true, RS>(
                    stream_rows_get(es, w, q), ld4(&bs[n]), n, op, t < 2 && p < a.M, [&](float4 pre) {
                        if constexpr (RS) {  // (PM: out2 holds the slope partials)
                            if (p < a.M) *reinterpret_cast<half4_t*>(o2 + (long long)p * e.ldo2 + n) = f2h4(pre);
                        }
                    });
                if (p < a.M) *reinterpret_cast<half4_t*>(y + (long long)p * g.ldy + n) = f2h4(o);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (PM) {
        __shared__ float pred[4];
        epi.reduce_pslope(w, pred, e.out2);
    }
}

// ------------------------------------------------------------------------------------------------
// Streaming 1x1 conv on the bf16 MFMA with fp32 accuracy (bf16x6, round 5): the fp32 ResidualUnit / RBB 1x1 layers and
// their input-gradients, K = Ci in {64, 128}, Co = 32 * NT in {64, 128}, with the streamed epilogue operands the tiled
// kernel fuses: residual (F & 1), ReLU mask (F & 2), accumulate into y (F & 4). These layers are HBM-bound (at bs 16,
// 128^2: 64->128 + residual moves 335 MB for 17 GFLOP) and ran on the 64-row implicit-GEMM tiles at ~3.3 TB/s: every
// block loads, waits at a barrier, multiplies, then streams its epilogue, so HBM idles while the MFMAs run and the
// other way round. Here, as conv1x1_stream_kernel, each WAVE streams its own 32-pixel tiles with no barrier after the
// one-time weight staging, and EVERY streamed operand rolls a tile ahead in registers:
//   * W [Co][K] is split once per block into three bf16 planes in LDS (pitch K + 8: conflict-free ds_read_b128);
//   * the wave's X tile goes HBM -> registers in the MFMA B layout (lane (r, h): pixel p0 + r, channels 16s + 8h .. +7
//     for k-step s: two float4), is split into its three bf16 pieces in registers (bf6_split4), and each float4 is
//     reloaded for the wave's NEXT tile right after its split;
//   * the epilogue operands (residual, mask, old y: one float4 per (co tile t, quad q)) of co tile t + 1 are issued
//     when co tile t starts (two register sets), so each is in flight during a whole co tile's MFMAs;
//   * the 32-output co tiles are done one at a time (one accumulator; the X pieces re-split per co tile from the
//     raw fp32 registers — a few VALU ops against six MFMAs per k-step): what keeps every operand in flight within
//     the VGPR file without spills;
//   * C^T = W X^T: lane (r, h) holds pixel p0 + r, channels 32t + 8q + 4h .. +3 in acc[t][4q..4q+3] — float4 stores.
// Products: bf6_mfma (six bf16 cross products per 16-deep k-step, fp32 accumulation), the same arithmetic as every
// other bf16x6 kernel. Its waves fill the VGPR file exactly (4 x 128 or 2 x 256; see conv3x3_wres_bf6_kernel: a
// kernel that converts with v_cvt_pk_bf16_f32 and runs bf16 MFMAs must not leave room for other kernels' waves).
// VGPR allocation per wave: 256 (2 waves per SIMD, two epilogue operand sets). Measured (profiles/r5e_stream_b6.txt):
// 128 VGPRs / 4 waves per SIMD with one operand set was slower (256^2 64->64: 153 vs 143 us), and so was prefetching
// X two tiles and the operands a whole tile ahead (128^2 128->64: 50.4 vs 46.7 us, 64^2 64->128 +res 23.9 vs 20.1)

// the forms whose LDS (weight planes + epilogue scratch > 80 KB) admits one block per CU: one wave per SIMD
template <int NT, int KS>
constexpr bool stream_b6_one_block() {
    return NT == 6 || KS == 12 || (NT == 4 && KS == 8);
}
template <int NT, int KS, int F, bool CE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(stream_b6_one_block<NT, KS>() ? 1 : 2)))
void conv1x1_stream_b6_kernel(const ConvArgs a) {
    constexpr int K = 16 * KS, KP = K + 8, CO = 32 * NT;
    constexpr bool RES = (F & 1) != 0, MASK = (F & 2) != 0, ACC = (F & 4) != 0;
    // SAB (F & 8, round 6): the HYRES_EPI_SA_BWD epilogue of MultiScaleRefine's fusion-1x1 input-gradient (64 -> 192 at
    // 256^2): o = (acc + aux0[p][0]) + (n == aux2[p] ? aux0[p][1] : 0), epi_store's order; no bias, no activation.
    // The per-pixel operands are loaded once per 32-pixel tile, the next tile's while this one multiplies
    constexpr bool SAB = (F & 8) != 0;
    static_assert(!SAB || (CE && !RES && !MASK), "SA_BWD: the coalesced epilogue, no residual / mask");
    // RS (F & 16, round 6): HYRES_EPI_ROWSCALE — MultiScaleRefine's fusion 1x1 in training with SpatialAttention folded
    // (192 -> 64 at 256^2, refine_ops.sa_fold_fusion): o = acc * aux1[p] + bias, then out2 (the pre-activation) and the
    // PReLU; the per-pixel scale is loaded once per tile like SAB's operands
    constexpr bool RS = (F & 16) != 0;
    static_assert(!RS || (CE && !RES && !MASK && !ACC && !SAB), "ROWSCALE: the coalesced epilogue, no other operand");
    // PM (F & 32, round 6, with SAB): HYRES_ACT_PRELU_MASK on output channels [0, 64) — MultiScaleRefine's scale-1
    // block writes PReLU(.) into multi[..., 0:64], so d multi's first 64 channels are that PReLU output's whole
    // gradient: o = pre > 0 ? o : slope * o (pre = aux1 [P][ld1]), sum_{pre <= 0} pre * o into this block's partial
    // (out2[block]); the slope gradient (res, ADDED) by prelu_slope_sum() after the launch
    constexpr bool PM = (F & 32) != 0;
    static_assert(!PM || (SAB && !ACC && NT >= 2), "PReLU mask: the SA_BWD form without accumulate");
    constexpr int WPL = CO * KP;  // bf16 per weight plane
    __shared__ __attribute__((aligned(16))) __bf16 Ws[3 * WPL];
    __shared__ __attribute__((aligned(16))) float bs[CO];
    // CE: per-wave epilogue scratch, one 32 x 32 co tile (stream_rows_put / stream_rows_get)
    __shared__ __attribute__((aligned(16))) float Es[CE ? 4 * 32 * STREAM_EP : 4];
    // exactly 2 waves' worth of VGPRs: no room for another kernel's wave on these SIMDs. NT = 6 (the 64 -> 192
    // SA_BWD form, 102 KB of LDS) and KS = 12 (the 192 -> 64 ROWSCALE form, 95 KB) admit one block per CU, i.e. one
    // wave per SIMD — they take all 512 registers
    if constexpr (stream_b6_one_block<NT, KS>()) asm volatile("" ::: "v255", "a255");
    else asm volatile("" ::: "v255");
    const hyres_conv_geom& g = a.g;
    const hyres_epilogue& e = a.e;
    const StreamWalk w = stream_walk(a.M);
    const int lr = w.lr, lh = w.lh, nw = w.nw;
    stream_stage_weights<CO, K>(a.w2, a.ldw, StreamPutBf6<KP, WPL>{Ws});
    stream_stage_bias<CO>(bs, e);
    StreamEpi epi{e.act, (e.act == HYRES_ACT_PRELU) ? e.slope[0] : 0.f, PM ? e.slope[0] : 0.f, 0.f};
    __syncthreads();

    const long long npix = a.M;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_res = opnd_rsrc(RES ? e.res : nullptr, npix * e.ldres * 4);
    const __amdgpu_buffer_rsrc_t r_mask = opnd_rsrc(MASK ? e.aux0 : nullptr, npix * e.ld0 * 4);
    const __amdgpu_buffer_rsrc_t r_old = opnd_rsrc(ACC ? a.y : nullptr, npix * g.ldy * 4);
    const __amdgpu_buffer_rsrc_t r_pm = opnd_rsrc(PM ? e.aux1 : nullptr, npix * e.ld1 * 4);
    const __amdgpu_buffer_rsrc_t r_sg = opnd_rsrc(SAB ? e.aux0 : nullptr, npix * e.ld0 * 4);
    const __amdgpu_buffer_rsrc_t r_si = opnd_rsrc(SAB ? e.aux2 : nullptr, npix * 4);
    const __amdgpu_buffer_rsrc_t r_rs = opnd_rsrc(RS ? e.aux1 : nullptr, npix * e.ld1 * 4);
    auto xoff = [&](int tile, int s, int u) -> int { return w.mfma_off(tile, g.ldx, 16 * s + 8 * lh + 4 * u, 4); };
    // epilogue operand q of co tile t. MFMA layout: lane (r, h) -> pixel p0 + r, channels 32t + 8q + 4h (one wave
    // instruction touches 32 pixel rows x 32 B). CE (coalesced): lane l -> pixel p0 + (l >> 3) + 8q, channels
    // 32t + 4 (l & 7) (one instruction = 8 pixel rows x 128 B contiguous; profiles/r5h_access_probe.txt: the 32-B
    // shape caps a read+write stream at ~3.0-3.5 TB/s, full rows reach 5.3-5.9)
    auto ooff = [&](int tile, int ld, int t, int q) -> int {
        if constexpr (CE) return w.row_off(tile, q, ld, 32 * t + w.cc, 4);
        else return w.mfma_off(tile, ld, 32 * t + 8 * q + 4 * lh, 4);
    };
    static_assert(NT % 2 == 0, "the epilogue operands alternate between two register sets per co tile");
    // epilogue operands, two register sets: co tile t's are in set t & 1 while co tile t + 1's (or the next tile's co
    // tile 0) are in flight in the other, issued when co tile t starts
    float4 xv[KS][2];
    float4 eres[RES ? 2 : 1][4], emask[MASK ? 2 : 1][4], eold[ACC ? 2 : 1][4], epre[PM ? 2 : 1][4];
    // SAB / RS: this tile's (d mean / C, d max) and argmax / scale per epilogue row q, and the next tile's in flight
    // (declared in every form; without SAB / RS nothing touches them and they take no register)
    float2 sg[4], sgn[4];
    int si[4], sin_[4];
    float rsc[4], rscn[4];
    auto load_rs = [&](int tile, float (&rs)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int p = tile * 32 + w.cr + 8 * q;
            const bool ok = tile < w.ntile && p < a.M;
            rs[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r_rs, ok ? p * e.ld1 * 4 : STREAM_OOR, 0, 0));
        }
    };
    auto load_epi = [&](int tile, int t, int set) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if constexpr (RES) eres[set][q] = bload4(r_res, ooff(tile, e.ldres, t, q));
            if constexpr (MASK) emask[set][q] = bload4(r_mask, ooff(tile, e.ld0, t, q));
            if constexpr (ACC) eold[set][q] = bload4(r_old, ooff(tile, g.ldy, t, q));
            if constexpr (PM) epre[set][q] = bload4(r_pm, t < 2 ? ooff(tile, e.ld1, t, q) : STREAM_OOR);
        }
    };
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int u = 0; u < 2; ++u) xv[s][u] = bload4(xr, xoff(w.gw, s, u));
    load_epi(w.gw, 0, 0);
    if constexpr (SAB) stream_load_sab(w, r_sg, r_si, e.ld0, w.gw, sg, si);
    if constexpr (RS) load_rs(w.gw, rsc);
    for (int tile = w.gw; tile < w.ntile; tile += nw) {
        if constexpr (SAB) stream_load_sab(w, r_sg, r_si, e.ld0, tile + nw, sgn, sin_);
        if constexpr (RS) load_rs(tile + nw, rscn);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int cur = t & 1;
            if (t + 1 < NT) load_epi(tile, t + 1, cur ^ 1);
            else load_epi(tile + nw, 0, cur ^ 1);
            floatx16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                // the X pieces are re-split per co tile (a few VALU ops) rather than held for all k-steps
                // (the empty asm makes each co tile's split its own computation: common-subexpression elimination
                // would otherwise keep every k-step's pieces live across all co tiles and spill)
                typedef float f32x4v_t __attribute__((ext_vector_type(4)));
                f32x4v_t v0 = __builtin_bit_cast(f32x4v_t, xv[s][0]), v1 = __builtin_bit_cast(f32x4v_t, xv[s][1]);
                asm volatile("" : "+v"(v0), "+v"(v1));
                const float4 x0 = __builtin_bit_cast(float4, v0), x1 = __builtin_bit_cast(float4, v1);
                bf16x4_t h0, m0, l0, h1, m1, l1;
                bf6_split4(x0, h0, m0, l0);
                bf6_split4(x1, h1, m1, l1);
                const bf16x8_t xb[3] = {__builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7),
                                        __builtin_shufflevector(m0, m1, 0, 1, 2, 3, 4, 5, 6, 7),
                                        __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7)};
                if (t == NT - 1) {
#pragma unroll
                    for (int u = 0; u < 2; ++u) xv[s][u] = bload4(xr, xoff(tile + nw, s, u));  // the next tile's X
                }
                const int o = (32 * t + lr) * KP + 16 * s + 8 * lh;
                const bf16x8_t wb[3] = {*reinterpret_cast<const bf16x8_t*>(&Ws[o]),
                                        *reinterpret_cast<const bf16x8_t*>(&Ws[WPL + o]),
                                        *reinterpret_cast<const bf16x8_t*>(&Ws[2 * WPL + o])};
                acc = bf6_mfma(wb, xb, acc);
            }
            float* const es = Es + w.wave * 32 * STREAM_EP;
            if constexpr (CE) stream_rows_put(es, w, acc);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = CE ? 32 * t + w.cc : 32 * t + 8 * q + 4 * lh;
                float4 av;
                if constexpr (CE) av = stream_rows_get(es, w, q);
                else av = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
                const int p = CE ? tile * 32 + w.cr + 8 * q : tile * 32 + lr;
                const bool pok = p < a.M;
                StreamOpnd op;
                if constexpr (RES) op.res = eres[cur][q];
                if constexpr (MASK) op.mask = emask[cur][q];
                if constexpr (ACC) op.old = eold[cur][q];
                if constexpr (PM) op.pre = epre[cur][q];
                if constexpr (SAB) {
                    op.gm = sg[q];
                    op.mi = si[q];
                }
                if constexpr (RS) op.sc = rsc[q];
                const float4 o = epi.apply<F, false, true>(av, ld4(&bs[n]), n, op, t < 2 && pok, [&](float4 pre) {
                    if constexpr (!PM) {  // (PM: out2 holds the slope partials)
                        if (pok && e.out2) st4(e.out2 + (long long)p * e.ldo2 + n, pre);
                    }
                });
                if (pok) st4(a.y + (long long)p * g.ldy + n, o);
            }
            __builtin_amdgcn_sched_barrier(0);  // keep the next co tile's LDS reads and splits out of this one
        }
        if constexpr (SAB) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                sg[q] = sgn[q];
                si[q] = sin_[q];
            }
        }
        if constexpr (RS) {
#pragma unroll
            for (int q = 0; q < 4; ++q) rsc[q] = rscn[q];
        }
    }
    if constexpr (PM) {
        __shared__ float pred[4];
        epi.reduce_pslope(w, pred, e.out2);
    }
}

// ------------------------------------------------------------------------------------------------
// Fused backward of a plain fp32 1x1 layer (bf16x6): the input gradient conv1x1_stream_b6_kernel computes and the weight
// / bias gradient wgrad1x1_bf6_pf2_kernel computes, in one pass over the output gradient gp [P][KG] (the conv's X, the
// weight gradient's P), which the two kernels each read from HBM and split into bf16 pieces. A persistent block (one
// per CU, 4 waves) takes a contiguous range of 32-pixel chunks; per chunk all four waves stage gp and the saved input
// x [P][CX] as three bf16 planes in LDS (wgrad1x1_bf6_pf2_kernel's transposed-read image, loads two chunks ahead in
// two register sets, two LDS buffers, one barrier per chunk), then
//   * waves 0, 1 form gx [32][CX] = gp W against the LDS-resident split weights (conv1x1_stream_b6_kernel's Ws image)
//     — C^T = W gp^T, the gp fragment of lane (r, h) = row r, channels 16s + 8h .. + 7 of the staged planes, the same
//     pieces (bf6_split4) in the same K order, so gx is bit-identical to the streaming kernel's — and run its coalesced
//     epilogue (stream_rows_put / StreamEpi::apply: residual, ReLU mask, accumulate; operands two chunks ahead);
//   * waves 2, 3 accumulate dW [KG][CX] += gp^T x, KG / 2 rows each (four 32 x 32 accumulators, transposed reads), over
//     all of the block's chunks.
// Both halves issue 48 bf16 MFMAs per chunk (64 <-> 128 channels). At the end a block writes its dW partial to slab
// [block][KG][CX] and its column sums of the unsplit gp to bias_slab [block][KG]: the deterministic wgrad_reduce*
// kernels finish them (no atomics). LDS: weights 51 / 54 KB + 2 x 48 KB of chunk planes + 9 KB of epilogue scratch =
// 156.3 / 159.5 KB, one block per CU, one wave per SIMD: the kernel claims the whole register file (v255, a255).
struct Bwd1x1Args {
    const float* q;    // the saved input [P][ldq]
    int ldq;
    float* slab;       // [blocks][KG][CX]
    float* bias_slab;  // [blocks][KG] or NULL
    int cps, nchunks;  // chunks per block, 32-pixel chunks in all
};

template <int NT, int KS, int F>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1)))
void conv1x1_bwd_fused_b6_kernel(const ConvArgs a, const Bwd1x1Args b) {
    constexpr int KG = 16 * KS, KP = KG + 8, CX = 32 * NT, WPL = CX * KP;
    constexpr bool RES = (F & 1) != 0, MASK = (F & 2) != 0, ACC = (F & 4) != 0;
    constexpr int PP = KG + 32, PQ = CX + 32;  // bf16 row pitches of the chunk planes
    constexpr int PSZ = KT * PP, QSZ = KT * PQ, PLANE = PSZ + QSZ, BUF = 3 * PLANE;
    constexpr int P_V = KT * KG / 4 / 256, Q_V = KT * CX / 4 / 256;
    constexpr int TH = NT / 2;                // co tiles of gx per gx wave
    constexpr int TMW = KG / 64, TNW = NT;    // dW tiles per dW wave
    static_assert(NT % 2 == 0 && KG % 64 == 0 && P_V >= 1 && Q_V >= 1 && PLANE % 8 == 0, "shape");
    __shared__ __attribute__((aligned(16))) __bf16 Ws[3 * WPL];
    __shared__ __attribute__((aligned(16))) __bf16 smem[2 * BUF];
    __shared__ __attribute__((aligned(16))) float Es[2 * 32 * STREAM_EP];
    __shared__ __attribute__((aligned(16))) float bs[CX];
    static_assert((3 * WPL + 2 * BUF) * 2 + (2 * 32 * STREAM_EP + CX) * 4 <= 160 * 1024, "LDS");
    static_assert(2 * BUF * 2 >= 256 * 16, "the bias reduce borrows the chunk planes");
    asm volatile("" ::: "v255", "a255");
    const hyres_conv_geom& g = a.g;
    const hyres_epilogue& e = a.e;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kb = (int)blockIdx.x * b.cps;
    const int ke = min(b.nchunks, kb + b.cps);
    // the gx waves' lane bookkeeping: chunk kc is "tile" kc, chunks from ke on are out of range
    const StreamWalk w{lane, wave & 1, lane & 31, lane >> 5, lane >> 3, 4 * (lane & 7), 0, 0, ke, a.M};
    const int lr = w.lr, lh = w.lh;
    stream_stage_weights<CX, KG>(a.w2, a.ldw, StreamPutBf6<KP, WPL>{Ws});
    stream_stage_bias<CX>(bs, e);
    StreamEpi epi{e.act, 0.f, 0.f, 0.f};

    const long long npix = a.M;
    const __amdgpu_buffer_rsrc_t rp_ = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rq_ = opnd_rsrc(b.q, npix * b.ldq * 4);
    const __amdgpu_buffer_rsrc_t r_res = opnd_rsrc(RES ? e.res : nullptr, npix * e.ldres * 4);
    const __amdgpu_buffer_rsrc_t r_mask = opnd_rsrc(MASK ? e.aux0 : nullptr, npix * e.ld0 * 4);
    const __amdgpu_buffer_rsrc_t r_old = opnd_rsrc(ACC ? a.y : nullptr, npix * g.ldy * 4);
    // staging: fixed per-thread channel quads, rows tid / (C / 4) + i * 256 / (C / 4) of the chunk
    const int pc = (tid % (KG / 4)) * 4, prow0 = tid / (KG / 4);
    const int qc = (tid % (CX / 4)) * 4, qrow0 = tid / (CX / 4);
    constexpr int PRS = 256 / (KG / 4), QRS = 256 / (CX / 4);
    auto load = [&](int kc, float4 (&rp)[P_V], float4 (&rq)[Q_V]) {
#pragma unroll
        for (int i = 0; i < P_V; ++i) {
            const int row = kc * KT + prow0 + i * PRS;
            rp[i] = bload4(rp_, (kc < ke && row < a.M) ? (row * g.ldx + pc) * 4 : STREAM_OOR);
        }
#pragma unroll
        for (int i = 0; i < Q_V; ++i) {
            const int row = kc * KT + qrow0 + i * QRS;
            rq[i] = bload4(rq_, (kc < ke && row < a.M) ? (row * b.ldq + qc) * 4 : STREAM_OOR);
        }
    };
    const bool do_bias = b.bias_slab != nullptr;
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
    auto store = [&](int buf, const float4 (&rp)[P_V], const float4 (&rq)[Q_V]) {
        __bf16* B0 = smem + buf * BUF;
#pragma unroll
        for (int i = 0; i < P_V; ++i) {
            if (do_bias) { bsum.x += rp[i].x; bsum.y += rp[i].y; bsum.z += rp[i].z; bsum.w += rp[i].w; }
            bf6_put3<PLANE>(B0, (prow0 + i * PRS) * PP + pc, rp[i]);
        }
#pragma unroll
        for (int i = 0; i < Q_V; ++i) bf6_put3<PLANE>(B0, PSZ + (qrow0 + i * QRS) * PQ + qc, rq[i]);
    };
    // the gx waves' epilogue operands of a chunk's TH co tiles (row layout), one register set per chunk parity
    const int t0 = (wave & 1) * TH;
    float4 eres[2][RES ? TH : 1][4], emask[2][MASK ? TH : 1][4], eold[2][ACC ? TH : 1][4];
    auto load_epi = [&](int kc, auto SET) {
        constexpr int set = decltype(SET)::value;
#pragma unroll
        for (int tt = 0; tt < TH; ++tt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = 32 * (t0 + tt) + w.cc;
                if constexpr (RES) eres[set][tt][q] = bload4(r_res, w.row_off(kc, q, e.ldres, col, 4));
                if constexpr (MASK) emask[set][tt][q] = bload4(r_mask, w.row_off(kc, q, e.ld0, col, 4));
                if constexpr (ACC) eold[set][tt][q] = bload4(r_old, w.row_off(kc, q, g.ldy, col, 4));
            }
    };
    const TrLane tl = tr_lane(lane);
    floatx16 dacc[TMW][TNW];
#pragma unroll
    for (int i = 0; i < TMW; ++i)
#pragma unroll
        for (int j = 0; j < TNW; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) dacc[i][j][r] = 0.f;
    const bool gxw = wave < 2;  // wave-uniform
    float4 pA[P_V], qA[Q_V], pB[P_V], qB[Q_V];
    load(kb, pA, qA);
    load(kb + 1, pB, qB);
    if (gxw) {
        load_epi(kb, std::integral_constant<int, 0>{});
        load_epi(kb + 1, std::integral_constant<int, 1>{});
    }
    store(0, pA, qA);
    __syncthreads();
    float* const es = Es + (wave & 1) * 32 * STREAM_EP;
    // chunk kc sits in LDS buffer CUR; (pn, qn) hold chunk kc + 1 (in flight), (pl, ql) (stored) receive kc + 2
    auto body = [&](int kc, auto CUR, float4 (&pl)[P_V], float4 (&ql)[Q_V], const float4 (&pn)[P_V],
                    const float4 (&qn)[Q_V]) {
        constexpr int cur = decltype(CUR)::value;
        load(kc + 2, pl, ql);
        const __bf16* Ps = smem + cur * BUF;
        const __bf16* Qs = Ps + PSZ;
        if (gxw) {
#pragma unroll
            for (int tt = 0; tt < TH; ++tt) {
                const int t = t0 + tt;
                floatx16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const int xo = lr * PP + 16 * s + 8 * lh;
                    const bf16x8_t xb[3] = {*reinterpret_cast<const bf16x8_t*>(&Ps[xo]),
                                            *reinterpret_cast<const bf16x8_t*>(&Ps[PLANE + xo]),
                                            *reinterpret_cast<const bf16x8_t*>(&Ps[2 * PLANE + xo])};
                    const int o = (32 * t + lr) * KP + 16 * s + 8 * lh;
                    const bf16x8_t wb[3] = {*reinterpret_cast<const bf16x8_t*>(&Ws[o]),
                                            *reinterpret_cast<const bf16x8_t*>(&Ws[WPL + o]),
                                            *reinterpret_cast<const bf16x8_t*>(&Ws[2 * WPL + o])};
                    acc = bf6_mfma(wb, xb, acc);
                }
                stream_rows_put(es, w, acc);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int n = 32 * t + w.cc;
                    const int p = kc * 32 + w.cr + 8 * q;
                    StreamOpnd op;
                    if constexpr (RES) op.res = eres[cur][tt][q];
                    if constexpr (MASK) op.mask = emask[cur][tt][q];
                    if constexpr (ACC) op.old = eold[cur][tt][q];
                    const float4 o = epi.apply<F, false, false>(stream_rows_get(es, w, q), ld4(&bs[n]), n, op, false,
                                                                 [](float4) {});
                    if (p < a.M) st4(a.y + (long long)p * g.ldy + n, o);
                }
            }
            load_epi(kc + 2, CUR);
        } else {
            const int mw = (wave & 1) * (KG / 2);
#pragma unroll
            for (int s = 0; s < KT / 16; ++s) {
                bf16x8_t af[TMW][3], bf[TNW][3];
#pragma unroll
                for (int tm = 0; tm < TMW; ++tm)
#pragma unroll
                    for (int pl3 = 0; pl3 < 3; ++pl3)
                        af[tm][pl3] = tr_frag(Ps + pl3 * PLANE + (16 * s + tl.row) * PP + mw + tm * 32 + tl.col, PP);
#pragma unroll
                for (int tn = 0; tn < TNW; ++tn)
#pragma unroll
                    for (int pl3 = 0; pl3 < 3; ++pl3)
                        bf[tn][pl3] = tr_frag(Qs + pl3 * PLANE + (16 * s + tl.row) * PQ + tn * 32 + tl.col, PQ);
#pragma unroll
                for (int tm = 0; tm < TMW; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TNW; ++tn) dacc[tm][tn] = bf6_mfma(af[tm], bf[tn], dacc[tm][tn]);
            }
        }
        if (kc + 1 < ke) store(cur ^ 1, pn, qn);  // block-uniform
        __syncthreads();
    };
    for (int kc = kb; kc < ke; kc += 2) {
        body(kc, std::integral_constant<int, 0>{}, pA, qA, pB, qB);
        if (kc + 1 < ke) body(kc + 1, std::integral_constant<int, 1>{}, pB, qB, pA, qA);
    }
    if (do_bias)  // block-uniform; the loop ended with a barrier
        bias_block_reduce<KG, 256>(reinterpret_cast<float4*>(smem), bsum, b.bias_slab, blockIdx.x, 0, KG);
    if (!gxw) {
        float* const out = b.slab + (long long)blockIdx.x * KG * CX;
        const int mw = (wave & 1) * (KG / 2);
#pragma unroll
        for (int tm = 0; tm < TMW; ++tm)
#pragma unroll
            for (int tn = 0; tn < TNW; ++tn) slab_store_acc(dacc[tm][tn], out + tn * 32 + lr, mw + tm * 32, lh, KG, CX);
    }
}

// ------------------------------------------------------------------------------------------------
// eligibility

// the streamed epilogue operands as the streaming kernels' F bits: residual, ReLU mask, old y
static int stream_f(const hyres_epilogue* e) {
    return (e->res ? 1 : 0) | (e->act == HYRES_ACT_RELU_MASK ? 2 : 0) | (e->accumulate ? 4 : 0);
}

// conv1x1_stream_kernel eligibility: single-tap stride-1 fp32 1x1 with K = Ci in {64, 96, 128}, Co in
// {64, 96, 128} (or 192 with K = 64), BIAS epilogue with no streamed operand (residual / ReLU mask /
// old y), grids >= 65536 output pixels. Returns pack_cfg(NT = Co / 32, KC = Ci / 8, 0) or 0.
int stream_cfg(const hyres_conv_geom* g, const hyres_epilogue* e) {
    if ((e->io_f16 & 3) || e->square_input || e->kind != HYRES_EPI_BIAS) return 0;
    if (!pointwise_same_size(g) || gemm_rows(g) < 65536) return 0;
    if (g->Ci != 64 && g->Ci != 96 && g->Ci != 128) return 0;
    if (stream_f(e)) return 0;
    const bool co = g->Co == 64 || g->Co == 96 || g->Co == 128 || (g->Co == 192 && g->Ci == 64);
    return co ? pack_cfg(g->Co / 32, g->Ci / 8, 0) : 0;
}

// conv1x1_stream_h_kernel eligibility: fp16 X and Y (io_f16 = 3), single-tap stride-1 1x1 with Ci and Co in
// {64, 96, 128}, BIAS epilogue with ReLU / none and no streamed operand, grids >= 16384 output pixels, 16-byte X rows.
// Returns pack_cfg(NT = Co / 32, KC = Ci / 16, 0) or 0.
int stream_h_cfg(const hyres_conv_geom* g, const hyres_epilogue* e) {
    if (g_tune[8] == 0 || (e->io_f16 & 3) != 3 || e->square_input || e->kind != HYRES_EPI_BIAS || e->out2) return 0;
    // a streamed epilogue operand (residual, ReLU mask, old y) measured slower than the tiles (128^2 64->128 +res
    // 45.2 vs 43.5 us, 64^2 16.5 vs 13.9 us; without one 24.8 vs 30.7 and 60.3 vs 80.8 us: profiles/r4e_h1x1.txt),
    // as for the fp32 streaming kernel: those layers stay tiled
    if (stream_f(e)) return 0;
    if (e->act != HYRES_ACT_NONE && e->act != HYRES_ACT_RELU) return 0;
    if (!pointwise_same_size(g) || gemm_rows(g) < 16384) return 0;
    if (g->Ci != 64 && g->Ci != 96 && g->Ci != 128) return 0;
    if (g->Co != 64 && g->Co != 96 && g->Co != 128) return 0;
    if (g->ldx % 8 || g->ldy % 4) return 0;
    return pack_cfg(g->Co / 32, g->Ci / 16, 0);
}

// the fusion 1x1's input-gradient 64 -> 192 (HYRES_EPI_SA_BWD, round 6) as conv1x1_stream_b6_kernel /
// conv1x1_stream_hf_kernel run it: plain, accumulating, or with the scale-1 PReLU backward (pm). Returns their F, or 0.
static int sa_bwd_f(const hyres_conv_geom* g, const hyres_epilogue* e) {
    const bool pm = e->act == HYRES_ACT_PRELU_MASK && !e->accumulate;
    if (g_tune[21] == 0 || g->Ci != 64 || g->Co != 192 || (e->act != HYRES_ACT_NONE && !pm) || (e->res && !pm) ||
        (e->out2 && !pm) || (pm && (!e->aux1 || e->ld1 < 64 || e->ld1 % 4 || !e->res)))
        return 0;
    return pm ? 40 : (8 | (e->accumulate ? 4 : 0));
}

// the fusion 1x1 forward 192 -> 64 with SpatialAttention folded (HYRES_EPI_ROWSCALE, round 6) on the same two kernels
static bool rowscale_ok(const hyres_conv_geom* g, const hyres_epilogue* e) {
    return g_tune[21] != 0 && g->Ci == 192 && g->Co == 64 && !e->res && !e->accumulate &&
           (e->act == HYRES_ACT_NONE || e->act == HYRES_ACT_RELU || e->act == HYRES_ACT_PRELU);
}

// conv1x1_stream_hf_kernel eligibility (hyres_conv_tuning key 17 = 1, default): fp16 X and Y / operands (io_f16 = 3),
// f16 operands, single-tap stride-1 1x1, (Ci, Co) in {64, 128}^2, >= 16384 output pixels, BIAS epilogue with none /
// ReLU / ReLU mask and at least one streamed operand (residual, mask, old y; without one: conv1x1_stream_h_kernel),
// no out2, 16-byte X rows / 8-byte Y rows. Returns pack_cfg(NT, KC, F), or 0.
int stream_hf_cfg(const hyres_conv_geom* g, const hyres_epilogue* e) {
    if (g_tune[17] == 0 || (e->io_f16 & 3) != 3 || !e->f16_operands || e->square_input) return 0;
    if (!pointwise_same_size(g) || gemm_rows(g) < 16384 || g->ldx % 8 || g->ldy % 4) return 0;
    if (e->kind == HYRES_EPI_ROWSCALE)  // the fusion 1x1 forward under AMP
        return rowscale_ok(g, e) && e->out2 && e->ldo2 % 4 == 0 ? pack_cfg(2, 12, 16) : 0;
    if (e->kind == HYRES_EPI_SA_BWD) {  // the fusion 1x1's input-gradient under AMP
        const int F = e->ld0 % 2 ? 0 : sa_bwd_f(g, e);
        return F ? pack_cfg(6, 4, F) : 0;
    }
    if (e->out2 || e->kind != HYRES_EPI_BIAS) return 0;
    if (e->act != HYRES_ACT_NONE && e->act != HYRES_ACT_RELU && e->act != HYRES_ACT_RELU_MASK) return 0;
    if ((g->Ci != 64 && g->Ci != 128) || (g->Co != 64 && g->Co != 128)) return 0;
    if ((e->res && e->ldres % 4) || (e->act == HYRES_ACT_RELU_MASK && e->ld0 % 4)) return 0;
    const int F = stream_f(e);
    return F ? pack_cfg(g->Co / 32, g->Ci / 16, F) : 0;
}

// conv1x1_stream_b6_kernel's epilogue: coalesced (hyres_conv_tuning key 11, default) or per-fragment stores
bool stream_b6_ce() { return g_tune[11] != 0; }

// conv1x1_stream_b6_kernel eligibility (bf16x6 fp32 GEMMs, hyres_conv_tuning key 10 = 1): fp32 X / Y, single-tap
// stride-1 1x1 with (Ci, Co) in {(64, 64), (64, 128), (128, 64)}, BIAS epilogue with none / ReLU / PReLU / ReLU mask,
// any of residual / mask / accumulate, grids >= 65536 output pixels. Returns pack_cfg(NT, KS, F), or 0.
int stream_b6_cfg(const hyres_conv_geom* g, const hyres_epilogue* e) {
    if (g_tune[7] != 1 || g_tune[10] == 0) return 0;
    if (e->io_f16 || e->f16_operands || e->square_input) return 0;
    // (hyres_conv_tuning key 24 bit 1 lifts the pixel floor of the BIAS forms: the small-shape tests of the fused backward)
    const bool floor_off = (g_tune[24] & 2) != 0 && e->kind == HYRES_EPI_BIAS;
    if (!pointwise_same_size(g) || (gemm_rows(g) < 65536 && !floor_off)) return 0;
    if (e->kind == HYRES_EPI_SA_BWD) {  // the fusion 1x1's input-gradient (coalesced epilogue only)
        const int F = stream_b6_ce() ? sa_bwd_f(g, e) : 0;
        return F ? pack_cfg(6, 4, F) : 0;
    }
    if (e->kind == HYRES_EPI_ROWSCALE)  // the fusion 1x1 forward (coalesced epilogue only)
        return stream_b6_ce() && rowscale_ok(g, e) ? pack_cfg(2, 12, 16) : 0;
    if (e->kind != HYRES_EPI_BIAS) return 0;
    const bool shape = (g->Ci == 64 && (g->Co == 64 || g->Co == 128)) || (g->Ci == 128 && g->Co == 64) ||
                       (g->Ci == 128 && g->Co == 128);
    if (!shape) return 0;
    const int F = stream_f(e);
    // 128 -> 128 (round 6, the GDN-side 1x1s at 128^2): 122 KB of LDS, one wave per SIMD — built for the operand-free
    // and ReLU-mask forms only
    if (g->Ci == 128 && g->Co == 128 && F != 0 && F != 2) return 0;
    return pack_cfg(g->Co / 32, g->Ci / 16, F);
}

// conv1x1_bwd_fused_b6_kernel eligibility (hyres_conv_tuning key 24 bit 0, default on): the input-gradient conv (g, e) is
// conv1x1_stream_b6_kernel's with the coalesced epilogue, 128 -> 64 channels (64 -> 128 with bit 2), no activation or the ReLU
// mask, no out2; the weight gradient d is the plain fp32 1x1 of the same pixels with P = the conv's X (same stride) and
// Q of the conv's Co channels; every row stride a multiple of 4 and every operand within a buffer resource. Returns
// pack_cfg(NT, KS, F), or 0: the two kernels.
int bwd1x1_fused_cfg(const hyres_conv_geom* g, const hyres_epilogue* e, const hyres_wgrad_desc* d) {
    if ((g_tune[24] & 1) == 0 || !stream_b6_ce() || e->kind != HYRES_EPI_BIAS) return 0;
    const int cfg = stream_b6_cfg(g, e);
    if (!cfg || e->out2 || (e->act != HYRES_ACT_NONE && e->act != HYRES_ACT_RELU_MASK)) return 0;
    // 128 -> 64 (the bottleneck tail's backward: gp is the wide operand). 64 -> 128 shares only the 64-channel operand
    // and measured no faster than its two kernels: built, routed only with key 24 bit 2 (A/B, tests)
    if (!((g->Ci == 128 && g->Co == 64) || (g->Ci == 64 && g->Co == 128 && (g_tune[24] & 4) != 0))) return 0;
    if (d->square_q || d->ntaps != 1 || d->dh[0] != 0 || d->dw[0] != 0 || d->sq != 1 || d->Hqq != d->Hq ||
        d->Wqq != d->Wq || d->f16_operands || d->io_f16)
        return 0;
    const long long rows = gemm_rows(g);
    if (d->M != g->Ci || d->N != g->Co || (long long)d->B * d->Hq * d->Wq != rows || d->ldp != g->ldx) return 0;
    if (g->ldx % 4 || g->ldy % 4 || d->ldq % 4 || (e->res && e->ldres % 4) || (e->aux0 && e->ld0 % 4)) return 0;
    const int ld = std::max(std::max(g->ldx, g->ldy), std::max(d->ldq, std::max(e->res ? e->ldres : 0, e->aux0 ? e->ld0 : 0)));
    if (rows * ld * 4 >= 0x7FFFFFF0LL) return 0;
    return cfg;
}

// its plan: one block per CU, each a contiguous range of cps 32-pixel chunks; one slab row per block
struct Bwd1x1Plan {
    int nchunks, cps, nsplit, lanes;
    long long bias_off, total;  // floats: the slab at 0, the [nsplit][M] bias partials
};
static Bwd1x1Plan bwd1x1_plan(const hyres_wgrad_desc* d) {
    Bwd1x1Plan p{};
    p.nchunks = ceil_div((long long)d->B * d->Hq * d->Wq, KT);
    p.cps = ceil_div(p.nchunks, std::min(p.nchunks, num_cus()));
    p.nsplit = ceil_div(p.nchunks, p.cps);
    p.lanes = wgrad_reduce_lanes((long long)d->M * d->N, p.nsplit);
    p.bias_off = (long long)p.nsplit * d->M * d->N;
    p.total = p.bias_off + (long long)p.nsplit * d->M + 4;
    return p;
}

// ------------------------------------------------------------------------------------------------
// launch

// persistent grid of a streaming kernel: as many blocks as fit on the chip at once (occupancy query, cached per
// instantiation), capped by the 32-pixel tiles available (4 per block)
template <auto Kernel>
static int persistent_blocks(int M) {
    static int occ = -1;
    if (occ < 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, Kernel, 256, 0) != hipSuccess || n < 1) n = 1;
        occ = n;
    }
    return std::max(1, std::min(ceil_div(ceil_div(M, 32), 4), num_cus() * occ));
}

// ... launched; with F & 32 (the PReLU mask) every block leaves a slope partial in out2[blockIdx.x]
template <auto Kernel, int F>
static int launch_persistent(const ConvArgs& a, const char* name, hipStream_t st) {
    const int blocks = persistent_blocks<Kernel>(a.M);
    if constexpr ((F & 32) != 0)
        HY_REQUIRE(blocks <= a.e.ldo2, HYRES_E_ARG, "%s: %d blocks, out2 holds %d slope partials", name, blocks,
                   a.e.ldo2);
    hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(256), 0, st, a);
    const int rc = HY_LAUNCH_CHECK(name);
    if constexpr ((F & 32) != 0) return rc ? rc : prelu_slope_sum(a.e.out2, blocks, a.e.res, st);
    return rc;
}

template <int NT, int KC>
static int launch_stream_one(const ConvArgs& a, hipStream_t st) {
    // (the f16-operand build runs on the fp32 build's block count)
    const dim3 grid(persistent_blocks<conv1x1_stream_kernel<NT, KC>>(a.M));
    if (a.e.f16_operands) hipLaunchKernelGGL((conv1x1_stream_kernel<NT, KC, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((conv1x1_stream_kernel<NT, KC>), grid, dim3(256), 0, st, a);
    return HY_LAUNCH_CHECK("conv1x1_stream_kernel");
}

int launch_stream(const ConvArgs& a, int cfg, hipStream_t st) {
    const int nt = cfg_nt(cfg), kc = cfg_k(cfg);
#define HY_STREAM(NT, KC) \
    if (nt == NT && kc == KC) return launch_stream_one<NT, KC>(a, st);
    HY_STREAM(2, 8) HY_STREAM(2, 12) HY_STREAM(2, 16)
    HY_STREAM(3, 8) HY_STREAM(3, 12) HY_STREAM(3, 16)
    HY_STREAM(4, 8) HY_STREAM(4, 12) HY_STREAM(4, 16)
    HY_STREAM(6, 8)
#undef HY_STREAM
    return set_error(HYRES_E_ARG, "conv1x1_stream: no instantiation for NT=%d KC=%d", nt, kc);
}

int launch_stream_h(const ConvArgs& a, int cfg, hipStream_t st) {
    const int nt = cfg_nt(cfg), kc = cfg_k(cfg);
#define HY_STREAM_H(NT, KC) \
    if (nt == NT && kc == KC) \
        return launch_persistent<conv1x1_stream_h_kernel<NT, KC>, 0>(a, "conv1x1_stream_h_kernel", st);
    HY_STREAM_H(2, 4) HY_STREAM_H(2, 6) HY_STREAM_H(2, 8)
    HY_STREAM_H(3, 4) HY_STREAM_H(3, 6) HY_STREAM_H(3, 8)
    HY_STREAM_H(4, 4) HY_STREAM_H(4, 6) HY_STREAM_H(4, 8)
#undef HY_STREAM_H
    return set_error(HYRES_E_ARG, "conv1x1_stream_h: no instantiation for NT=%d KC=%d", nt, kc);
}

template <int NT, int KS, int F, bool CE>
static int launch_stream_b6_ce(const ConvArgs& a, hipStream_t st) {
    return launch_persistent<conv1x1_stream_b6_kernel<NT, KS, F, CE>, F>(a, "conv1x1_stream_b6_kernel", st);
}
template <int NT, int KS, int F>
static int launch_stream_b6_one(const ConvArgs& a, hipStream_t st) {
    return stream_b6_ce() ? launch_stream_b6_ce<NT, KS, F, true>(a, st) : launch_stream_b6_ce<NT, KS, F, false>(a, st);
}
template <int NT, int KS>
static int launch_stream_b6_f(const ConvArgs& a, int f, hipStream_t st) {
    switch (f) {
        case 0: return launch_stream_b6_one<NT, KS, 0>(a, st);
        case 1: return launch_stream_b6_one<NT, KS, 1>(a, st);
        case 2: return launch_stream_b6_one<NT, KS, 2>(a, st);
        case 3: return launch_stream_b6_one<NT, KS, 3>(a, st);
        case 4: return launch_stream_b6_one<NT, KS, 4>(a, st);
        case 5: return launch_stream_b6_one<NT, KS, 5>(a, st);
        case 6: return launch_stream_b6_one<NT, KS, 6>(a, st);
        default: return launch_stream_b6_one<NT, KS, 7>(a, st);
    }
}

int launch_stream_b6(const ConvArgs& a, int cfg, hipStream_t st) {
    const int nt = cfg_nt(cfg), ks = cfg_k(cfg), f = cfg_f(cfg);
    if (nt == 6 && ks == 4 && f == 8) return launch_stream_b6_ce<6, 4, 8, true>(a, st);
    if (nt == 6 && ks == 4 && f == 12) return launch_stream_b6_ce<6, 4, 12, true>(a, st);
    if (nt == 6 && ks == 4 && f == 40) return launch_stream_b6_ce<6, 4, 40, true>(a, st);
    if (nt == 2 && ks == 12 && f == 16) return launch_stream_b6_ce<2, 12, 16, true>(a, st);
    if (nt == 2 && ks == 4) return launch_stream_b6_f<2, 4>(a, f, st);
    if (nt == 4 && ks == 4) return launch_stream_b6_f<4, 4>(a, f, st);
    if (nt == 2 && ks == 8) return launch_stream_b6_f<2, 8>(a, f, st);
    if (nt == 4 && ks == 8 && f == 0) return launch_stream_b6_one<4, 8, 0>(a, st);
    if (nt == 4 && ks == 8 && f == 2) return launch_stream_b6_one<4, 8, 2>(a, st);
    return set_error(HYRES_E_ARG, "conv1x1_stream_b6: no instantiation for NT=%d KS=%d", nt, ks);
}

template <int NT, int KC, int F>
static int launch_stream_hf_one(const ConvArgs& a, hipStream_t st) {
    return launch_persistent<conv1x1_stream_hf_kernel<NT, KC, F>, F>(a, "conv1x1_stream_hf_kernel", st);
}
template <int NT, int KC>
static int launch_stream_hf_f(const ConvArgs& a, int f, hipStream_t st) {
    switch (f) {  // (no F = 0 form: without a streamed operand the layer is conv1x1_stream_h_kernel's)
        case 1: return launch_stream_hf_one<NT, KC, 1>(a, st);
        case 2: return launch_stream_hf_one<NT, KC, 2>(a, st);
        case 3: return launch_stream_hf_one<NT, KC, 3>(a, st);
        case 4: return launch_stream_hf_one<NT, KC, 4>(a, st);
        case 5: return launch_stream_hf_one<NT, KC, 5>(a, st);
        case 6: return launch_stream_hf_one<NT, KC, 6>(a, st);
        default: return launch_stream_hf_one<NT, KC, 7>(a, st);
    }
}

int launch_stream_hf(const ConvArgs& a, int cfg, hipStream_t st) {
    const int nt = cfg_nt(cfg), kc = cfg_k(cfg), f = cfg_f(cfg);
    if (nt == 6 && kc == 4 && f == 8) return launch_stream_hf_one<6, 4, 8>(a, st);
    if (nt == 6 && kc == 4 && f == 12) return launch_stream_hf_one<6, 4, 12>(a, st);
    if (nt == 6 && kc == 4 && f == 40) return launch_stream_hf_one<6, 4, 40>(a, st);
    if (nt == 2 && kc == 12 && f == 16) return launch_stream_hf_one<2, 12, 16>(a, st);
    if (nt == 2 && kc == 4) return launch_stream_hf_f<2, 4>(a, f, st);
    if (nt == 2 && kc == 8) return launch_stream_hf_f<2, 8>(a, f, st);
    if (nt == 4 && kc == 4) return launch_stream_hf_f<4, 4>(a, f, st);
    if (nt == 4 && kc == 8) return launch_stream_hf_f<4, 8>(a, f, st);
    return set_error(HYRES_E_ARG, "conv1x1_stream_hf: no instantiation for NT=%d KC=%d", nt, kc);
}

template <int NT, int KS>
static int launch_bwd1x1_f(const ConvArgs& a, const Bwd1x1Args& b, int f, int blocks, hipStream_t st) {
#define HY_BWD1X1(FV) \
    case FV: hipLaunchKernelGGL((conv1x1_bwd_fused_b6_kernel<NT, KS, FV>), dim3(blocks), dim3(256), 0, st, a, b); break;
    switch (f) {
        HY_BWD1X1(0) HY_BWD1X1(1) HY_BWD1X1(2) HY_BWD1X1(3) HY_BWD1X1(4) HY_BWD1X1(5) HY_BWD1X1(6)
        default: hipLaunchKernelGGL((conv1x1_bwd_fused_b6_kernel<NT, KS, 7>), dim3(blocks), dim3(256), 0, st, a, b);
    }
#undef HY_BWD1X1
    return HY_LAUNCH_CHECK("conv1x1_bwd_fused_b6_kernel");
}

}  // namespace hyres

using namespace hyres;

extern "C" {

// every pointer may be NULL (then assumed 16-byte aligned: the host-only query)
int hyres_conv1x1_bwd_fused_ok(const hyres_conv_geom* g, const hyres_epilogue* e, const hyres_wgrad_desc* d,
                               const void* gp, const void* q, const void* w2, int ldw, const void* gx) {
    if (!g || !e || !d || !bwd1x1_fused_cfg(g, e, d)) return 0;
    return aligned16(gp) && aligned16(q) && aligned16(w2) && aligned16(gx) && aligned16(e->res) && aligned16(e->aux0) &&
           aligned16(e->bias) && ldw % 4 == 0 && ldw >= g->Ci;
}

long long hyres_conv1x1_bwd_fused_workspace_bytes(const hyres_wgrad_desc* d) {
    return d ? 4 * bwd1x1_plan(d).total : 0;
}

int hyres_conv1x1_bwd_fused_kernel_name(const hyres_conv_geom* g, const hyres_epilogue* e, const hyres_wgrad_desc* d,
                                        char* buf, int n) {
    HY_REQUIRE(g && e && d && buf && n > 0, HYRES_E_ARG, "conv1x1_bwd_fused_kernel_name: bad args");
    const int cfg = bwd1x1_fused_cfg(g, e, d);
    HY_REQUIRE(cfg, HYRES_E_SHAPE, "conv1x1_bwd_fused: not eligible");
    snprintf(buf, n, "conv1x1_bwd_fused_b6_kernel<%d, %d, %d>", cfg_nt(cfg), cfg_k(cfg), cfg_f(cfg));
    return 0;
}

int hyres_conv1x1_bwd_fused(const hyres_conv_geom* g, const float* gp, const float* w2, int ldw, float* gx,
                            const hyres_epilogue* e, const hyres_wgrad_desc* d, const float* q, float* dw, float* dbias,
                            void* ws, long long ws_bytes, hyres_wgrad_job* jobs, int* njobs, hyres_stream_t s) {
    HY_REQUIRE(g && gp && w2 && gx && e && d && q && dw && jobs && njobs, HYRES_E_ARG, "conv1x1_bwd_fused: NULL argument");
    *njobs = 0;
    HY_REQUIRE(hyres_conv1x1_bwd_fused_ok(g, e, d, gp, q, w2, ldw, gx), HYRES_E_SHAPE,
               "conv1x1_bwd_fused: not eligible (shape, epilogue, stride or alignment)");
    const int cfg = bwd1x1_fused_cfg(g, e, d);
    const Bwd1x1Plan p = bwd1x1_plan(d);
    HY_REQUIRE(ws && aligned16(ws) && ws_bytes >= 4 * p.total, HYRES_E_WORKSPACE,
               "conv1x1_bwd_fused: workspace %lld < %lld", ws_bytes, 4 * p.total);
    ConvArgs a{};
    a.g = *g; a.x = gp; a.w2 = w2; a.ldw = ldw; a.y = gx; a.e = *e;
    a.M = g->B * g->Hq * g->Wq;
    a.nsplit = 1;
    a.vec4 = 1;
    a.rsrc_ok = 1;
    a.x_bytes = (int)((long long)a.M * g->ldx * 4);
    a.w_bytes = (int)((long long)g->Co * ldw * 4);
    float* const wsf = (float*)ws;
    Bwd1x1Args b{q, d->ldq, wsf, dbias ? wsf + p.bias_off : nullptr, p.cps, p.nchunks};
    hipStream_t st = as_stream(s);
    const int nt = cfg_nt(cfg), f = cfg_f(cfg);
    const int rc = nt == 2 ? launch_bwd1x1_f<2, 8>(a, b, f, p.nsplit, st) : launch_bwd1x1_f<4, 4>(a, b, f, p.nsplit, st);
    if (rc) return rc;
    jobs[0] = hyres_wgrad_job{wsf, dw, p.nsplit, 1, d->M, d->N, d->sm, d->sn, d->st, d->accumulate, p.lanes, 0};
    *njobs = 1;
    if (dbias) {
        jobs[1] = hyres_wgrad_job{wsf + p.bias_off, dbias, p.nsplit, 1, d->M, 1, 1, 0, 0, d->accumulate, p.lanes, 0};
        *njobs = 2;
    }
    return 0;
}

}  // extern "C"
