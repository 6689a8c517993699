// Convolutions for the HyRES hot path on CDNA4 (gfx950), fp32 in / fp32 accumulate: the kernel choice (route(), the
// tile and split-K planners), the C API, the halo-tiled 3x3 and weight-resident kernels, the narrow-output kernels
// and weight prep.
//
// Every Conv2d / ConvTranspose2d / GDN contraction of the reference (models/checkerboard.py:35-88,
// models/layers/attention.py, models/layers/enhancement.py, compressai GDN / RBB) and their
// input-gradients are one contraction:
//     Y[b, i*osh+oph, j*osw+opw, co] = epi( sum_{t in taps(phase)} sum_ci X[b, i*ish+dh_t, j*isw+dw_t, ci] * W2[co][t][ci] )
// The implicit-GEMM family that runs any of them (conv_fwd_*_kernel, the split-K reduce kernels and launch_tiles) is in
// conv_gemm.hip, the per-wave streaming 1x1 kernels (conv1x1_stream*_kernel) in conv_stream.hip; route() and
// hyres_conv_forward reach both through the declarations in conv_common.h. The generic epilogue (epi_store /
// epi_store4) the kernels here share with the implicit GEMM is in conv_epilogue.h.
// Weight gradients use a second kernel (P^T Q over pixels, split-K slabs + deterministic reduce).
// The halo-tiled 3x3 kernels (conv3x3_halo_f16_kernel, conv3x3_wres_{f16,f32,bf6}_kernel) share their tile geometry,
// tile walk, halo address, f16 halo staging, fused-operand epilogue and weight-slice decode with ru_fused.hip
// through halo_common.h.
#include "conv_epilogue.h"
#include "halo_common.h"
#include <limits>

namespace hyres {

// ------------------------------------------------------------------------------------------------
// Halo-staged f16 3x3 conv (autocast; the dominant AMP kernel).  The implicit-GEMM kernel (conv_gemm.hip) gathers the
// A operand once per tap from L2: for a 3x3 64->64 layer at 128^2 that is ~1 GB of L2->CU traffic per launch
// (PMC: TCC hits+misses ~7.9 M requests, 84 % hit) for 134 MB of HBM traffic, and its one-chunk register
// prefetch cannot cover that latency with the 4 f16 MFMAs a 32-deep chunk gives each wave (SQ_WAIT_ANY 48 %
// of wave-cycles).  Here a block computes a 4-row x 64-pixel x 64-channel output tile: the 6 x 66-pixel
// input halo of one 32-channel chunk is staged ONCE in LDS as fp16 (2 buffers: the next chunk's halo loads
// are issued in three parts between the taps of the current chunk), and all 9 taps read their A fragments
// from it (ds_read_b128, 80-B pixel pitch: conflict-free); the B fragments (weights, fp32 W2 converted in
// registers) come straight from L2 in MFMA layout, one tap ahead.  L2->CU bytes per output pixel drop from
// ~3.4 KB to ~1.5 KB.  Taps: any 9 offsets within [-1, 1]^2 (the conv and its input-gradient), stride 1,
// same-size output, Ci % 32 == 0, Co % 64 == 0, Wo % 64 == 0.  IO: bit 0 X fp16, bit 1 Y/res/aux fp16.
// Tile geometry (HALO_R, HALO_TW, HALO_PH, halo_hw / halo_npx / halo_elems of the radius): halo_common.h
constexpr int HALO_E = halo_elems(1, 8);      // float4 elements of one 32-channel halo chunk (396 px x 8)
constexpr int HALO_PE = (HALO_E + 2) / 3;     // per staging part (3 parts per chunk)
constexpr int HALO_PV = (HALO_PE + 255) / 256;

template <int IO>
__global__ __launch_bounds__(256, 2) void conv3x3_halo_f16_kernel(const ConvArgs a) {
    constexpr bool XH = (IO & 1) != 0, YH = (IO & 2) != 0;
    constexpr int XES = XH ? 2 : 4;
    constexpr int HBUF = halo_npx(1) * HALO_PH;  // halves per buffer
    constexpr int CP = 64 + 4;                // epilogue staging pitch (floats)
    static_assert(2 * 64 * CP * 4 <= 2 * HBUF * 2, "epilogue staging fits in the halo buffers");
    __shared__ __attribute__((aligned(16))) _Float16 hal[2 * HBUF];
    __shared__ int2 tapoff[9];
    typedef _Float16 half8 __attribute__((ext_vector_type(8)));

    const hyres_conv_geom& g = a.g;
    const int tid = threadIdx.x;
    // tile decode, XCD-aware (conv_fwd_body): N tiles fastest, then row tiles (vertical neighbours share
    // two of the six halo rows through one L2), column tiles, images
    const int nnt = g.Co / 64, nrt = (g.Ho + HALO_R - 1) / HALO_R, nct = g.Wo / HALO_TW;
    int l = xcd_logical_block();
    const int nt = l % nnt; l /= nnt;
    const int rt = l % nrt; l /= nrt;
    const int ct = l % nct;
    const int b = l / nct;
    const int n0 = nt * 64, i0 = rt * HALO_R, j0 = ct * HALO_TW;
    const int Ci = g.Ci, nch = Ci / 32;
    if (tid < 9) tapoff[tid] = make_int2(g.dh[tid], g.dw[tid]);

    const long long img = (long long)g.Hi * g.Wi * g.ldx;
    const long long xrem = img * XES;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(reinterpret_cast<const char*>(a.x) + (long long)b * img * XES), (short)0,
        (int)(xrem < 0x7FFFFFF0LL ? xrem : 0x7FFFFFF0LL), 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)a.w2, (short)0, a.w_bytes, 0x00020000);

    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;  // rows 2wm, 2wm+1; channels n0 + 32wn ..
    const int lr = lane & 31, lh = lane >> 5;

    // ---- halo staging (part p of chunk c: elements [p*PE, (p+1)*PE) of the 396 px x 8 float4)
    HaloReg<XH> hreg[HALO_PV];  // fp16 X: raw halves until the LDS store
    auto hload = [&](int part, int c) {
        halo16_load<XH, 256>(hreg, xr, part * HALO_PE + tid, min((part + 1) * HALO_PE, HALO_E), i0, j0, g.Hi, g.Wi,
                             g.ldx, c * 32);
    };
    auto hstore = [&](int part, int buf) {
        halo16_store<XH, 256>(hal + buf * HBUF, hreg, part * HALO_PE + tid, min((part + 1) * HALO_PE, HALO_E));
    };
    // ---- B fragments of one tap (both 16-deep k-steps of the chunk): W2[co][t][ci], fp32 -> fp16
    const int co = n0 + wn * 32 + lr;
    float4 bnx[4];
    auto bload = [&](int t, int c) {
        const int base = (co * a.ldw + t * Ci + c * 32 + 8 * lh) * 4;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bnx[2 * ks] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wr, base + 64 * ks, 0, 0));
            bnx[2 * ks + 1] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wr, base + 64 * ks + 16, 0, 0));
        }
    };

    floatx16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

#pragma unroll
    for (int part = 0; part < 3; ++part) {
        hload(part, 0);
        hstore(part, 0);
    }
    bload(0, 0);
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        const _Float16* H = hal + (c & 1) * HBUF;
        const bool more = c + 1 < nch;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            half8 bf[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const float4 u = bnx[2 * ks], v = bnx[2 * ks + 1];
                bf[ks] = half8{(_Float16)u.x, (_Float16)u.y, (_Float16)u.z, (_Float16)u.w,
                               (_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
            }
            if (t < 8) bload(t + 1, c);
            else if (more) bload(0, c + 1);
            if (more && t % 3 == 0) hload(t / 3, c + 1);
            const int2 o = tapoff[t];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                for (int at = 0; at < 4; ++at) {
                    const int orow = 2 * wm + (at >> 1);  // output row within the tile
                    const int px = (orow + 1 + o.x) * halo_hw(1) + (at & 1) * 32 + lr + 1 + o.y;
                    const half8 af = *reinterpret_cast<const half8*>(&H[px * HALO_PH + 16 * ks + 8 * lh]);
                    acc[at] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf[ks], acc[at], 0, 0, 0);
                }
            }
            if (more && t % 3 == 2) hstore(t / 3, (c + 1) & 1);
        }
        __syncthreads();
    }

    // ---- epilogue in two passes of 2 output rows (rows p and 2 + p), staged through the halo buffers
    float* Cs = reinterpret_cast<float*>(hal);
    const float slope = (a.e.act == HYRES_ACT_PRELU) ? a.e.slope[0] : 0.f;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (p) __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                Cs[(wm * 64 + h * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * CP + wn * 32 + lr] = acc[2 * p + h][r];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int idx = tid + 256 * k;
            const int c4 = idx & 15, px = (idx >> 4) & 63, rr = idx >> 10;
            const int i = i0 + 2 * rr + p, j = j0 + px;
            if (i < g.Ho) {
                const float4 v = *reinterpret_cast<const float4*>(&Cs[(rr * 64 + px) * CP + 4 * c4]);
                const long long pix = ((long long)b * g.Ho + i) * g.Wo + j;
                epi_store4<YH>(a.e, a.y, g.ldy, pix, n0 + 4 * c4, v, slope);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Weight-resident persistent f16 3x3 conv, Ci = 64 (the 64-channel 3x3 convs of every ResidualUnit / RBB
// / MultiScaleRefine scale at 64^2..256^2, forward and input-gradient).  conv3x3_halo_f16_kernel above still
// re-reads the B operand (all 576 x 64 weights, fp32) from L2 once per wave and 256-pixel tile: 147 KB per
// 32-channel chunk per block against 51 KB of halo, ~400 GB/s per CU of L2->CU traffic, 2-3x what a CU gets
// from L2 (MI355X_MICROARCH.md "Indexed rows": 66-73 GB/s per CU from L2) — so it measured no faster than the
// implicit-GEMM kernel.  Here one 512-thread block per CU converts the layer's weights of its 64-channel
// output slice to fp16 ONCE into LDS (9 taps x 64 co x 64 ci, 80-B rows: 92 KB) and then walks its share of
// the 4-row x 64-pixel tiles; per tile and 32-channel chunk only the 6 x 66-pixel halo moves (fp32 -> fp16,
// 7 float4 per thread issued one chunk ahead, 2 LDS buffers: 63 KB), and every A and B fragment is a
// conflict-free ds_read_b128.  Per CU that is ~22 B per cycle at the MFMA rate, below the L2 rate; the
// epilogue is applied from the accumulators directly (per-lane scalar epi_store: the LDS is full).
// 8 waves = 4 output rows x 2 co halves, 2 A tiles (64 px) each; tiles are walked XCD-contiguously.
constexpr int WRES_LDS_B = 2 * 9 * 64 * HALO_PH;  // halves: [chunk][tap][co][40]
constexpr int WRES_HV = halo_per_thread(1, 8, 512);  // halo float4 per thread per chunk (7)

template <int IO>
__global__ __launch_bounds__(512, 2) void conv3x3_wres_f16_kernel(const ConvArgs a, int ntiles, int groups) {
    constexpr bool XH = (IO & 1) != 0, YH = (IO & 2) != 0;
    constexpr int XES = XH ? 2 : 4;
    constexpr int HBUF = halo_npx(1) * HALO_PH;
    __shared__ __attribute__((aligned(16))) _Float16 lds[WRES_LDS_B + 2 * HBUF];
    __shared__ int2 tapoff[9];
    _Float16* const Bs = lds;
    _Float16* const Hs = lds + WRES_LDS_B;
    // whole VGPR file (as conv3x3_wres_bf6_kernel, DESIGN §4 "Cross-kernel interference"): IO 1 allocated 248 and left
    // a 16-VGPR hole beside its two waves per SIMD; the others already allocate 256 (and the clobber made IO 3 spill)
    if constexpr (IO == 1) asm volatile("" ::: "v255");

    const hyres_conv_geom& g = a.g;
    const int tid = threadIdx.x;
    const int nrt = (g.Ho + HALO_R - 1) / HALO_R, nct = g.Wo / HALO_TW;
    // block -> (output-channel group, share of the tiles): the blocks of one XCD (b % 8) take one contiguous
    // range of tiles, interleaved, so that vertically adjacent tiles (two shared halo rows) run together on it
    // group-major block order with nb % 8 == 0 (wres_blocks): hardware XCD = blockIdx.x % 8 = bg % 8, so the
    // blocks of every channel group that walk the same tiles (same bg) sit on one XCD and share its L2 halos
    const int nb = gridDim.x / groups;  // blocks per channel group
    const int grp = blockIdx.x / nb, bg = blockIdx.x - grp * nb;
    const int n0 = grp * 64;
    const HaloWalk walk = halo_walk(bg, nb, ntiles, nrt, nct);
    if (tid < 9) tapoff[tid] = make_int2(g.dh[tid], g.dw[tid]);

    // ---- the 64-channel weight slice, fp32 W2[co][t][ci] -> fp16 Bs[(c*9 + t)*64 + co][k] (ci = 32c + k)
    for (int f = tid; f < 64 * 9 * 16; f += 512) {
        const auto [co, t, ci] = wres_weight_index(f);
        const float4 w = ld4(a.w2 + (long long)(n0 + co) * a.ldw + t * 64 + ci);
        const half4_t h = {(_Float16)w.x, (_Float16)w.y, (_Float16)w.z, (_Float16)w.w};
        *reinterpret_cast<half4_t*>(&Bs[(((ci >> 5) * 9 + t) * 64 + co) * HALO_PH + (ci & 31)]) = h;
    }

    const long long img = (long long)g.Hi * g.Wi * g.ldx;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.x, (short)0, (int)std::min<long long>((long long)g.B * img * XES, 0x7FFFFFF0LL), 0x00020000);
    const int lane = tid & 63, wave = tid >> 6;
    const int orow = wave & 3, wn = wave >> 2;
    const int lr = lane & 31, lh = lane >> 5;

    // halo chunks are prefetched TWO steps ahead (two register sets, alternating): one step of MFMA work
    // (~2.3k cycles per SIMD) does not cover an HBM-bound 50 KB-per-CU chunk load
    using HRT = HaloReg<XH>;  // fp16 X: raw halves until the LDS store
    auto hload = [&](HRT (&h)[WRES_HV], int step) {
        const HaloTile tl = walk.tile(step >> 1);
        const int c = step & 1;
        const int base = tl.b * (int)img;  // element offset of image b (host checks the batch < 2 GB)
        // its own load / store loops, not halo16_load / halo16_store: through those IO 2 spilled (12 B of scratch)
#pragma unroll
        for (int v = 0; v < WRES_HV; ++v) {
            const int off = halo_offset<1, 8>(tid + 512 * v, tl.i0, tl.j0, g.Hi, g.Wi, g.ldx, base + 32 * c, XES);
            if constexpr (XH) {
                h[v] = __builtin_bit_cast(half4_t, __builtin_amdgcn_raw_buffer_load_b64(xr, off, 0, 0));
            } else {
                h[v] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
            }
        }
    };
    auto hstore = [&](const HRT (&h)[WRES_HV], int buf) {
#pragma unroll
        for (int v = 0; v < WRES_HV; ++v) {
            const int e = tid + 512 * v;
            if (e < HALO_E) {
                half4_t hh;
                if constexpr (XH) hh = h[v];
                else hh = half4_t{(_Float16)h[v].x, (_Float16)h[v].y, (_Float16)h[v].z, (_Float16)h[v].w};
                *reinterpret_cast<half4_t*>(&Hs[buf * HBUF + (e >> 3) * HALO_PH + 4 * (e & 7)]) = hh;
            }
        }
    };

    // the product is formed transposed (C^T = W X^T, as conv1x1_stream_kernel): lane (lr, lh) of A tile `at`
    // holds pixel j0 + 32 at + lr and, per register quad qd, the 4 consecutive channels n0 + 32 wn + 8 qd + 4 lh
    // .. + 3 — the epilogue loads / stores float4 straight from the accumulators
    floatx16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const float slope = (a.e.act == HYRES_ACT_PRELU) ? a.e.slope[0] : 0.f;
    const bool pre_res = a.e.kind == HYRES_EPI_BIAS && a.e.res != nullptr;
    float4 rres[2][4];  // the tile's residual operand, prefetched one step before the epilogue
    const int steps = walk.mytiles * 2;  // two 32-channel chunks per tile
    auto tile_pix = [&](int k, int at, int& i, long long& pix) {
        const HaloTile tl = walk.tile(k);
        i = tl.i0 + orow;
        pix = ((long long)tl.b * g.Ho + i) * g.Wo + tl.j0 + 32 * at + lr;
    };
    auto body = [&](int s, HRT (&hl)[WRES_HV], const HRT (&hs)[WRES_HV]) {
        const int k = s >> 1, c = s & 1;
        // the epilogue's residual is loaded BEFORE the halo two steps ahead: vmcnt retires loads in issue
        // order, so waiting for it then does not wait for that halo too (the bias comes from LDS for the same
        // reason)
        if (c == 1 && pre_res) {
#pragma unroll
            for (int at = 0; at < 2; ++at) {
                int i;
                long long pix;
                tile_pix(k, at, i, pix);
#pragma unroll
                for (int qd = 0; qd < 4; ++qd)
                    rres[at][qd] = i < g.Ho ? ldv4<YH>(a.e.res, pix * a.e.ldres + n0 + 32 * wn + 8 * qd + 4 * lh)
                                            : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        if (s + 2 < steps) hload(hl, s + 2);
        const _Float16* H = Hs + (s & 1) * HBUF;
        const _Float16* Bc = Bs + c * 9 * 64 * HALO_PH;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int2 o = tapoff[t];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const halfx8_t bf = *reinterpret_cast<const halfx8_t*>(&Bc[(t * 64 + wn * 32 + lr) * HALO_PH + 16 * ks + 8 * lh]);
#pragma unroll
                for (int at = 0; at < 2; ++at) {
                    const int px = (orow + 1 + o.x) * halo_hw(1) + at * 32 + lr + 1 + o.y;
                    const halfx8_t af = *reinterpret_cast<const halfx8_t*>(&H[px * HALO_PH + 16 * ks + 8 * lh]);
                    acc[at] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bf, af, acc[at], 0, 0, 0);
                }
            }
        }
        if (c == 1) {
#pragma unroll
            for (int at = 0; at < 2; ++at) {
                int i;
                long long pix;
                tile_pix(k, at, i, pix);
                if (i < g.Ho) {
#pragma unroll
                    for (int qd = 0; qd < 4; ++qd) {
                        const int n = n0 + 32 * wn + 8 * qd + 4 * lh;
                        const float4 v = make_float4(acc[at][4 * qd], acc[at][4 * qd + 1], acc[at][4 * qd + 2],
                                                     acc[at][4 * qd + 3]);
                        epi_store4<YH>(a.e, a.y, g.ldy, pix, n, v, slope, pre_res, rres[at][qd]);
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[at][r] = 0.f;
            }
        }
        if (s + 1 < steps) hstore(hs, (s + 1) & 1);
        __syncthreads();
    };
    HRT hA[WRES_HV], hB[WRES_HV];
    if (steps > 0) {
        hload(hA, 0);
        hstore(hA, 0);
    }
    if (steps > 1) hload(hB, 1);
    __syncthreads();
    for (int s = 0; s < steps; s += 2) {
        body(s, hA, hB);
        if (s + 1 < steps) body(s + 1, hB, hA);
    }
}

// ------------------------------------------------------------------------------------------------
// Weight-resident persistent fp32 3x3 conv, Ci = 64 (the fp32 headline path's dominant family: the 64-channel
// 3x3 convs of the ResidualUnits / RBBs / MultiScaleRefine at 64^2..256^2 and their input-gradients, the
// `conv_fwd_kernel<2, 1, 2, 2, 0, false, false>` population). That implicit-GEMM kernel is MFMA-bound at
// ~0.6-0.7 of the fp32 peak isolated: each 32-deep K chunk costs two barriers, a register->LDS store of
// 24 KB and a re-gather of the shifted A rows from L2, against 32 MFMAs per wave. Here one 512-thread block
// per CU holds the fp32 weights of a 32-channel output slice in LDS (9 taps x 32 co x 64 ci, 36-float rows:
// 83 KB) for the whole launch and walks 4-row x 64-pixel tiles; per tile and 32-channel chunk only the
// 6 x 66-pixel fp32 halo moves (7 float4 per thread, loaded during the previous chunk's MFMAs), so a wave
// issues 144 MFMAs (9 taps x 16 k-steps) per barrier pair. Fragments as in conv_fwd_body (k-permuted rows:
// one ds_read_b128 feeds 4 MFMA steps, 36-float pitch conflict-free); the product is formed transposed
// (C^T = W X^T) so the epilogue stores float4 from the accumulators. 8 waves = 4 output rows x 2 pixel
// halves, one 32 x 32 accumulator each. Exact fp32 (v_mfma_f32_32x32x2f32), the same sums per output as
// the implicit-GEMM kernel up to the K order.
constexpr int WF_PK = 36;  // floats per staged row (32 + 4 pad)
constexpr int WF_LDS_W = 2 * 9 * 32 * WF_PK;
constexpr int WF_LDS_H = halo_npx(1) * WF_PK;

// Epilogue (BIAS kind: bias, residual, pre-activation store, ReLU / PReLU / ReLU-mask, accumulate): every operand
// it reads (bias, residual, mask, old y) is requested at the START of the tile's second chunk through buffer
// resources — an absent operand gets an empty resource, so its loads return 0 with no branch — and consumed only
// after that chunk's 144 MFMAs. The generic epi_store4 issued each load behind its own branch and waited on it
// (~8 serialised HBM round trips per tile; +14 % on a 3x3 with a residual).
__global__ __launch_bounds__(512, 1) void conv3x3_wres_f32_kernel(const ConvArgs a, int ntiles, int groups) {
    __shared__ __attribute__((aligned(16))) float lds[WF_LDS_W + WF_LDS_H];
    __shared__ int2 tapoff[9];
    // the whole VGPR file of its SIMDs (2 waves x 256; the code needs 182). Round 5 saw one run-to-run difference in
    // tests/test_bf6_gpu.py::test_bf6_refine_branch_determinism in the subset that runs this kernel (native fp32 GEMM on
    // MultiScaleRefine's scale 1) beside bf16x6 convs on another branch stream; of the kernels in that configuration it
    // is the one 512-thread persistent kernel whose allocation left a hole (144 VGPRs) other waves could share — a mix
    // only tests make (the fp32 GEMM mode is global). Free: its 140 KB of LDS already limits the CU to one block
    asm volatile("" ::: "v255");
    float* const Ws = lds;
    float* const Hs = lds + WF_LDS_W;
    const hyres_conv_geom& g = a.g;
    const int tid = threadIdx.x;
    const int nrt = (g.Ho + HALO_R - 1) / HALO_R, nct = g.Wo / HALO_TW;
    const int nb = gridDim.x / groups;  // group-major, nb % 8 == 0: see conv3x3_wres_f16_kernel
    const int grp = blockIdx.x / nb, bg = blockIdx.x - grp * nb;
    const int n0 = grp * 32;
    const HaloWalk walk = halo_walk(bg, nb, ntiles, nrt, nct);
    if (tid < 9) tapoff[tid] = make_int2(g.dh[tid], g.dw[tid]);
    // weights W2[co][t][ci] -> Ws[((c*9 + t)*32 + co)*36 + k], ci = 32c + k
    for (int f = tid; f < 32 * 9 * 16; f += 512) {
        const auto [co, t, ci] = wres_weight_index(f);
        *reinterpret_cast<float4*>(&Ws[(((ci >> 5) * 9 + t) * 32 + co) * WF_PK + (ci & 31)]) =
            ld4(a.w2 + (long long)(n0 + co) * a.ldw + t * 64 + ci);
    }
    const long long img = (long long)g.Hi * g.Wi * g.ldx;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.x, (short)0, (int)std::min<long long>((long long)g.B * img * 4, 0x7FFFFFF0LL), 0x00020000);
    const int lane = tid & 63, wave = tid >> 6;
    const int orow = wave & 3, ph = wave >> 2;  // output row in the tile, 32-pixel half
    const int lr = lane & 31, lh = lane >> 5;

    float4 hreg[WRES_HV];
    auto hload = [&](int step) {
        const HaloTile tl = walk.tile(step >> 1);
        const int c = step & 1;
        const int base = tl.b * (int)img;
#pragma unroll
        for (int v = 0; v < WRES_HV; ++v)
            hreg[v] = bload4(xr, halo_offset<1, 8>(tid + 512 * v, tl.i0, tl.j0, g.Hi, g.Wi, g.ldx, base + 32 * c, 4));
    };
    auto hstore = [&]() {
#pragma unroll
        for (int v = 0; v < WRES_HV; ++v) {
            const int e = tid + 512 * v;
            if (e < HALO_E) *reinterpret_cast<float4*>(&Hs[(e >> 3) * WF_PK + 4 * (e & 7)]) = hreg[v];
        }
    };
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const hyres_epilogue& e = a.e;
    WresEpi<false> epi(e, g, a.y);  // no PReLU mask: routing gives that activation to the bf16x6 kernel only
    const int steps = walk.mytiles * 2;
    if (steps > 0) {
        hload(0);
        hstore();
    }
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const int k = s >> 1, c = s & 1;
        const HaloTile tl = walk.tile(k);
        const int i = tl.i0 + orow;
        const long long pix = ((long long)tl.b * g.Ho + i) * g.Wo + tl.j0 + 32 * ph + lr;
        // the epilogue's operands, issued before the next halo (vmcnt retires in issue order)
        if (c == 1) epi.request(e, g.ldy, pix, i < g.Ho, n0, lh);
        if (s + 1 < steps) hload(s + 1);
        const float* Wc = Ws + c * 9 * 32 * WF_PK;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int2 o = tapoff[t];
            const float* arow = &Hs[((orow + 1 + o.x) * halo_hw(1) + 32 * ph + lr + 1 + o.y) * WF_PK + lh * 16];
            const float* brow = &Wc[(t * 32 + lr) * WF_PK + lh * 16];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 av = *reinterpret_cast<const float4*>(arow + 4 * u);
                const float4 bv = *reinterpret_cast<const float4*>(brow + 4 * u);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.x, av.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.y, av.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.z, av.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.w, av.w, acc, 0, 0, 0);
            }
        }
        if (c == 1) {
            epi.apply(acc, e, a.y, g.ldy, pix, i < g.Ho, n0, lh);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        }
        __syncthreads();  // every wave is done with this chunk's halo
        if (s + 1 < steps) hstore();
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// fp32-accurate weight-resident 3x3 conv on the bf16 MFMA ("bf16x6", hyres_conv_tuning key 7 = 1, the default).
// conv3x3_wres_f32_kernel above runs at ~0.7 of the fp32 MFMA peak, and that peak (157 TF/s) is 1/16 of the bf16
// MFMA's. Here every fp32 operand is split into three bf16 pieces x = x0 + x1 + x2 (x0 = bf16(x), x1 = bf16(x - x0),
// x2 = bf16(x - x0 - x1): 24 significant bits, |x - x0 - x1 - x2| <= 2^-25 |x|) and each product is formed from the
// six cross products with i + j <= 2 (the dropped ones are below 2^-26 |x y|) with fp32 accumulation on
// v_mfma_f32_32x32x16_bf16 (products of bf16 values are exact in fp32): per product the error is at most about
// 2^-25 relative, below the half-ulp rounding (2^-24) of the fp32 MFMA's own fmaf chain; 6 bf16 MFMAs per 16-deep K
// step against 8 fp32 ones per 2 x 8, i.e. 2.67x fewer MFMA cycles. The weights of the block's 32-channel output
// slice are split once into LDS (3 planes x 4 chunks of 16 input channels x 9 taps x 32 rows of 32 B: 108 KB), the
// halo of each 16-channel chunk is split when staged (3 planes x 396 px x 32 B: 37 KB; 9 taps reuse it). Both
// images swizzle the 16-B half of a 32-B row by bit 3 of the row: every ds_read_b128 lane group then hits 16
// distinct 16-B slots (conflict-free). Same tiles, waves, tile order and epilogue as conv3x3_wres_f32_kernel.
constexpr int BF6_WPL = 4 * 9 * 32 * 16;  // bf16 per weight plane
// 16-B segment (0 / 1) of element k (0..15) of row r in a swizzled [row][16] bf16 image, as an element offset
__device__ __forceinline__ int bf6_off(int r, int k) { return r * 16 + ((((k >> 3) ^ (r >> 3)) & 1) << 3) + (k & 7); }

// V (hyres_conv_tuning key 12, default 1): bit 0 — each tap's six fragments are read one tap ahead into a second
// register set (hand-issued ds_read_b128: the compiler sank its own reads next to their MFMAs, waiting on each) —
// 133 -> 125 us at 128^2, 481 -> 453 us at 256^2 (profiles/r5i_wres_variants_micro.txt); bit 1 — waves 4..7 at static
// priority 1: no effect (kept for the A/B). Every variant forms the same MFMAs in the same order (bit-identical)
// D (round 5): the halo radius = the taps' largest offset, 1 (3x3) or 2 (MultiScaleRefine's dilation-2 3x3s,
// enhancement.py:44-51): (4 + 2D) x (64 + 2D) halo pixels; at D = 2 the three halo planes are 52 KB, 159 KB of LDS in all
template <bool GUARD, int V, int D = 1>
__global__ __launch_bounds__(512, 1) void conv3x3_wres_bf6_kernel(const ConvArgs a, int ntiles, int groups) {
    constexpr int HW = halo_hw(D);  // halo row length
    // bf16 per halo plane, float4 per 16-channel chunk and per thread
    constexpr int HPL = halo_npx(D) * 16, HE = halo_elems(D, 4), HV = halo_per_thread(D, 4, 512);
    __shared__ __attribute__((aligned(16))) __bf16 lds[3 * BF6_WPL + 3 * HPL];
    __shared__ int2 tapoff[9];
    __bf16* const Ws = lds;
    __bf16* const Hs = lds + 3 * BF6_WPL;
    // GUARD: the block takes the whole VGPR file of its SIMDs (2 waves x 256; the code needs 220). With the compiler's
    // 224, waves of OTHER kernels co-resident on those SIMDs (a bilinear on a side stream) computed wrong values while
    // this kernel's own output stayed exact (round 4, tests/test_bf6_gpu.py::test_bf6_kernels_beside_a_bilinear: 0.25
    // off, gone with this line). The error signature and the probes that isolate it: DESIGN §4 "Cross-kernel
    // interference" (scripts/diag_bf6_mechanism.py, scripts/coresidency_probe.hip). No cost to this kernel (its LDS
    // already limits the CU to one block). GUARD = false exists only for that diagnosis (hyres_conv_tuning key 9 = 0).
    if constexpr (GUARD) asm volatile("" ::: "v255");
    const hyres_conv_geom& g = a.g;
    const int tid = threadIdx.x;
    const int nrt = (g.Ho + HALO_R - 1) / HALO_R, nct = g.Wo / HALO_TW;
    const int nb = gridDim.x / groups;  // group-major, nb % 8 == 0: see conv3x3_wres_f16_kernel
    const int grp = blockIdx.x / nb, bg = blockIdx.x - grp * nb;
    const int n0 = grp * 32;
    const HaloWalk walk = halo_walk(bg, nb, ntiles, nrt, nct);
    if (tid < 9) tapoff[tid] = make_int2(g.dh[tid], g.dw[tid]);
    // weights W2[co][t][ci] (fp32) -> three bf16 planes, row (chunk c = ci / 16, tap t, co), element ci % 16
    for (int f = tid; f < 32 * 9 * 16; f += 512) {
        const auto [co, t, ci] = wres_weight_index(f);
        const int row = ((ci >> 4) * 9 + t) * 32 + co;
        bf6_put3<BF6_WPL>(Ws, bf6_off(row, ci & 15), ld4(a.w2 + (long long)(n0 + co) * a.ldw + t * 64 + ci));
    }
    const long long img = (long long)g.Hi * g.Wi * g.ldx;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.x, (short)0, (int)std::min<long long>((long long)g.B * img * 4, 0x7FFFFFF0LL), 0x00020000);
    const int lane = tid & 63, wave = tid >> 6;
    const int orow = wave & 3, ph = wave >> 2;  // output row in the tile, 32-pixel half
    const int lr = lane & 31, lh = lane >> 5;

    // halo chunks are prefetched TWO steps ahead (two register sets, alternating, as conv3x3_wres_f16_kernel): one
    // 16-channel step is 54 MFMAs per wave (~1.7k cycles), too short to cover an HBM load issued one step ahead
    auto hload = [&](float4 (&hreg)[HV], int step) {  // step = 4 * tile + chunk (16 channels)
        const HaloTile tl = walk.tile(step >> 2);
        const int c = step & 3;
        const int base = tl.b * (int)img;
#pragma unroll
        for (int v = 0; v < HV; ++v)
            hreg[v] = bload4(xr, halo_offset<D, 4>(tid + 512 * v, tl.i0, tl.j0, g.Hi, g.Wi, g.ldx, base + 16 * c, 4));
    };
    // the next step's halo is split into its bf16 pieces in registers DURING this step's MFMAs (hsplit, independent
    // VALU work the scheduler interleaves with them); between the two barriers only the LDS stores remain (hput)
    bf16x4_t sp[HV][3];
    auto hsplit = [&](const float4 (&hreg)[HV]) {
#pragma unroll
        for (int v = 0; v < HV; ++v) bf6_split4(hreg[v], sp[v][0], sp[v][1], sp[v][2]);
    };
    auto hput = [&]() {
#pragma unroll
        for (int v = 0; v < HV; ++v) {
            const int e = tid + 512 * v;
            if (e < HE) {
                const int o = bf6_off(e >> 2, 4 * (e & 3));
                *reinterpret_cast<bf16x4_t*>(&Hs[o]) = sp[v][0];
                *reinterpret_cast<bf16x4_t*>(&Hs[HPL + o]) = sp[v][1];
                *reinterpret_cast<bf16x4_t*>(&Hs[2 * HPL + o]) = sp[v][2];
            }
        }
    };
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const hyres_epilogue& e = a.e;
    WresEpi<true> epi(e, g, a.y);
    const int steps = walk.mytiles * 4;
    float4 hA[HV], hB[HV];
    if (steps > 0) {
        hload(hA, 0);
        hsplit(hA);
        hput();
    }
    if (steps > 1) hload(hB, 1);
    __syncthreads();
    // step s: the set that held step s's halo (stored) receives step s + 2; the other holds step s + 1
    auto body = [&](int s, float4 (&hl)[HV], const float4 (&hs)[HV]) {
        const int k = s >> 2, c = s & 3;
        const HaloTile tl = walk.tile(k);
        const int i = tl.i0 + orow;
        const long long pix = ((long long)tl.b * g.Ho + i) * g.Wo + tl.j0 + 32 * ph + lr;
        // the epilogue's operands, issued before the next halo (vmcnt retires in issue order)
        if (c == 3) epi.request(e, g.ldy, pix, i < g.Ho, n0, lh);
        if (s + 2 < steps) hload(hl, s + 2);
        if constexpr ((V & 1) != 0) {
            // explicit software pipeline: tap t + 1's six fragments are read (hand-issued ds_read_b128, so the
            // compiler cannot sink them to their uses) while tap t's MFMAs run; each MFMA pair waits only for its
            // own two reads (the LDS return counter retires in order; any other LGKM op only makes a wait longer)
            typedef __attribute__((address_space(3))) __bf16 lds_bf16;
            const unsigned wbase = (unsigned)(size_t)(lds_bf16*)Ws, hbase = (unsigned)(size_t)(lds_bf16*)Hs;
            auto rd = [&](unsigned addr) -> bf16x8_t {
                bf16x8_t r;
                asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(addr) : "memory");
                return r;
            };
            auto frag = [&](int t, bf16x8_t (&wv)[3], bf16x8_t (&xv)[3]) {
                const int wrow = (c * 9 + t) * 32 + lr;
                const int hrow = (orow + D + g.dh[t]) * HW + 32 * ph + lr + D + g.dw[t];
                const unsigned wo = wbase + 2u * (wrow * 16 + (((lh ^ (wrow >> 3)) & 1) << 3));
                const unsigned ho = hbase + 2u * (hrow * 16 + (((lh ^ (hrow >> 3)) & 1) << 3));
                wv[2] = rd(wo + 4u * BF6_WPL);
                xv[0] = rd(ho);
                wv[1] = rd(wo + 2u * BF6_WPL);
                xv[1] = rd(ho + 2u * HPL);
                wv[0] = rd(wo);
                xv[2] = rd(ho + 4u * HPL);
            };
            bf16x8_t fw[2][3], fx[2][3];
            hsplit(hs);  // unconditional (unused after the last step): no branch inside the tap loop
            frag(0, fw[0], fx[0]);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                bf16x8_t(&w)[3] = fw[t & 1];
                bf16x8_t(&x)[3] = fx[t & 1];
                if (t + 1 < 9) {
                    frag(t + 1, fw[(t + 1) & 1], fx[(t + 1) & 1]);
                    asm volatile("s_waitcnt lgkmcnt(10)" : "+v"(w[2]), "+v"(x[0]));
                } else {
                    asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(w[2]), "+v"(x[0]));
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[2], x[0], acc, 0, 0, 0);
                if (t + 1 < 9) asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(w[1]), "+v"(x[1]));
                else asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(w[1]), "+v"(x[1]));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], x[1], acc, 0, 0, 0);
                if (t + 1 < 9) asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(w[0]), "+v"(x[2]));
                else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w[0]), "+v"(x[2]));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], x[2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], x[0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], x[1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], x[0], acc, 0, 0, 0);
            }
        } else {
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int2 o = tapoff[t];
            const int wrow = (c * 9 + t) * 32 + lr;                                    // A: weights, row = co
            const int hrow = (orow + D + o.x) * HW + 32 * ph + lr + D + o.y;          // B: halo, row = pixel
            const int wo = wrow * 16 + (((lh ^ (wrow >> 3)) & 1) << 3);
            const int ho = hrow * 16 + (((lh ^ (hrow >> 3)) & 1) << 3);
            const bf16x8_t w0 = *reinterpret_cast<const bf16x8_t*>(&Ws[wo]);
            const bf16x8_t w1 = *reinterpret_cast<const bf16x8_t*>(&Ws[BF6_WPL + wo]);
            const bf16x8_t w2 = *reinterpret_cast<const bf16x8_t*>(&Ws[2 * BF6_WPL + wo]);
            const bf16x8_t x0 = *reinterpret_cast<const bf16x8_t*>(&Hs[ho]);
            const bf16x8_t x1 = *reinterpret_cast<const bf16x8_t*>(&Hs[HPL + ho]);
            const bf16x8_t x2 = *reinterpret_cast<const bf16x8_t*>(&Hs[2 * HPL + ho]);
            // the small cross products first, the leading one last
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2, x0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, x1, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, x2, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, x0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, x1, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, x0, acc, 0, 0, 0);
            if (t == 1 && s + 1 < steps) hsplit(hs);  // step s + 1's halo (loaded a step ago) -> bf16 pieces
        }
        }
        if (c == 3) {
            epi.apply(acc, e, a.y, g.ldy, pix, i < g.Ho, n0, lh);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        }
        __syncthreads();  // every wave is done with this chunk's halo
        if (s + 1 < steps) hput();
        __syncthreads();
    };
    if constexpr ((V & 2) != 0) {
        if (wave >= 4) __builtin_amdgcn_s_setprio(1);
    }
    for (int s = 0; s < steps; s += 2) {
        body(s, hA, hB);
        if (s + 1 < steps) body(s + 1, hB, hA);
    }
    if (e.act == HYRES_ACT_PRELU_MASK) {  // block partial of the slope gradient (every body ended with a barrier)
        float* red = reinterpret_cast<float*>(lds);
        red[tid] = epi.pslope;
        __syncthreads();
        for (int k = 256; k > 0; k >>= 1) {
            if (tid < k) red[tid] += red[tid + k];
            __syncthreads();
        }
        if (tid == 0) const_cast<float*>(e.aux2)[blockIdx.x] = red[0];
    }
}

// ------------------------------------------------------------------------------------------------
// Narrow output (Co <= 4: the 3-channel image-side layers — g_s's last deconv 128->3, MultiScaleRefine's
// conv 64->3 and the input-gradient of its conv 3->64). A 32-wide MFMA column tile would be >90% padding,
// so these run on the VALU. Each 16-lane group owns one output pixel: lane l reads channels
// [64s + 4l, +4) of every tap (a wave reads 4 adjacent pixels = contiguous NHWC rows, coalesced), keeps
// CO partial sums, and the group folds them with 4 xor-shuffles. The phase's weights are staged once per
// block in LDS as [tap][co][Ci] (a lane's float4 reads are consecutive across the group: conflict-free).
// HBM traffic = the input once (tap re-reads hit L1/L2) + CO outputs.
// ------------------------------------------------------------------------------------------------
constexpr int NARROW_PIX = 256;      // output pixels per block
constexpr int NARROW_WLDS = 8192;    // floats of staged weights (ntap * CO * Ci)

template <int CO, int S, bool XH = false>
__global__ __launch_bounds__(256) void conv_narrow_kernel(const ConvArgs a) {
    __shared__ __attribute__((aligned(16))) float Ws[NARROW_WLDS];
    __shared__ int2 tapoff[HYRES_MAX_TAPS];
    const hyres_conv_geom& g = a.g;
    const int tid = threadIdx.x;
    const int phase = blockIdx.y;
    const int ntap = g.ntap[phase], tap0 = g.tap0[phase];
    constexpr int CI = 64 * S;
    for (int idx = tid; idx < ntap * CO * (CI / 4); idx += 256) {
        const int c4 = idx % (CI / 4);
        const int r = idx / (CI / 4);
        const int co = r % CO, t = r / CO;
        *reinterpret_cast<float4*>(&Ws[4 * idx]) = ld4(a.w2 + (long long)co * a.ldw + (tap0 + t) * CI + 4 * c4);
    }
    for (int i = tid; i < ntap; i += 256) tapoff[i] = make_int2(g.dh[tap0 + i], g.dw[tap0 + i]);
    __syncthreads();

    const int HqWq = g.Hq * g.Wq;
    // XCD-aware pixel-tile order (as conv_fwd_kernel): neighbouring rows' tiles, which share the 3x3
    // halo, run on one XCD's L2
    int bx = blockIdx.x;
    if (a.xcd) {
        const int nb = gridDim.x, q = nb >> 3, r = nb & 7, x = bx & 7;
        bx = x * q + min(x, r) + (bx >> 3);
    }
    const int b0 = (bx * NARROW_PIX) / HqWq;
    constexpr int XES = XH ? 2 : 4;  // X element bytes (XH: fp16 activations, autocast inference)
    const long long img = (long long)g.Hi * g.Wi * g.ldx;
    const long long xrem = ((long long)g.B - b0) * img * XES;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(reinterpret_cast<const char*>(a.x) + (long long)b0 * img * XES), (short)0,
        (int)(xrem < 0x7FFFFFF0LL ? xrem : 0x7FFFFFF0LL), 0x00020000);
    const int l16 = tid & 15, slot = tid >> 4;  // 16 pixel slots per block pass
    for (int it = 0; it < NARROW_PIX / 16; ++it) {
        const int m = bx * NARROW_PIX + it * 16 + slot;
        const bool ok = m < a.M;
        const int mm = ok ? m : 0;
        const int b = mm / HqWq;
        const int r = mm - b * HqWq;
        const int i = r / g.Wq, j = r - (r / g.Wq) * g.Wq;
        const int base = (int)((b - b0) * img);
        float acc[CO];
#pragma unroll
        for (int c = 0; c < CO; ++c) acc[c] = 0.f;
        // taps in groups of TG: all TG input rows are requested before the first FMA (a loop of one load
        // then its FMAs serialised ~9 memory latencies per output pixel: 254 us -> see DESIGN §4)
        constexpr int TG = 9;
        for (int t0 = 0; t0 < ntap; t0 += TG) {
            std::conditional_t<XH, half4_t, float4> xv[TG][S];  // fp16 X: converted at the FMAs
#pragma unroll
            for (int u = 0; u < TG; ++u) {
                const int t = t0 + u;
                const int2 o = tapoff[t < ntap ? t : 0];
                const int ih = i * g.ish + o.x, iw = j * g.isw + o.y;
                const bool in = ok && t < ntap && (unsigned)ih < (unsigned)g.Hi && (unsigned)iw < (unsigned)g.Wi;
                const int off = in ? (base + (ih * g.Wi + iw) * g.ldx + 4 * l16) * XES : (int)0x80000000;
#pragma unroll
                for (int s2 = 0; s2 < S; ++s2) {
                    if constexpr (XH) {
                        xv[u][s2] = __builtin_bit_cast(
                            half4_t, __builtin_amdgcn_raw_buffer_load_b64(xr, in ? off + 128 * s2 : off, 0, 0));
                    } else {
                        xv[u][s2] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                                                  xr, in ? off + 256 * s2 : off, 0, 0));
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < TG; ++u) {
                const int t = t0 + u;
                if (t >= ntap) break;
#pragma unroll
                for (int s2 = 0; s2 < S; ++s2) {
                    float4 xf;
                    if constexpr (XH) xf = make_float4((float)xv[u][s2].x, (float)xv[u][s2].y, (float)xv[u][s2].z,
                                                       (float)xv[u][s2].w);
                    else xf = xv[u][s2];
#pragma unroll
                    for (int co = 0; co < CO; ++co) {
                        const float4 w =
                            *reinterpret_cast<const float4*>(&Ws[(t * CO + co) * CI + 64 * s2 + 4 * l16]);
                        acc[co] = fmaf(xf.x, w.x, acc[co]);
                        acc[co] = fmaf(xf.y, w.y, acc[co]);
                        acc[co] = fmaf(xf.z, w.z, acc[co]);
                        acc[co] = fmaf(xf.w, w.w, acc[co]);
                    }
                }
            }
        }
#pragma unroll
        for (int co = 0; co < CO; ++co) {
            float v = acc[co];
            v += __shfl_xor(v, 8);
            v += __shfl_xor(v, 4);
            v += __shfl_xor(v, 2);
            v += __shfl_xor(v, 1);
            acc[co] = v;
        }
        float v = acc[0];
#pragma unroll
        for (int co = 1; co < CO; ++co) v = l16 == co ? acc[co] : v;
        if (ok && l16 < CO) {
            const long long pix = (long long)(b * g.Ho + i * g.osh + g.oph[phase]) * g.Wo + j * g.osw + g.opw[phase];
            epi_store(a.e, a.y, g.ldy, pix, l16, v, epi_channel(a.e, l16));
        }
    }
}

// Co <= 4 with register blocking along W (round 5). conv_narrow_kernel is VALU-bound, not memory-bound: on
// MultiScaleRefine's 3x3 64 -> 3 at bs16 256^2 (215 us) the PMC passes read 270 MB (1.0x the input) while each 4-pixel
// wave pass issues ~307 VALU instructions of which 108 are the FMAs — the rest is per-pixel index decode, 9 tap
// addresses and bounds, and the fold (profiles/r5u_narrow_pmc.txt); its per-pixel weight re-reads add 27
// ds_read_b128. Here a lane group (Ci / 4 lanes, 4 channels each) computes a STRIP of 4 consecutive base pixels of
// one row: the phase's taps form a kh x kw grid of consecutive (dh, dw) offsets (every 3x3 conv and every phase of
// the 5x5 stride-2 transposed conv: checked on the host), so the strip needs kh x (kw + 3) input pixels, loaded once
// (<= 18 float4 per lane) and each reused by up to 3 taps; the weights of the phase live in VGPRs (9 taps x Co float4,
// zero for absent taps) for the whole launch; index decode and addressing once per strip; the 4 x Co partial sums
// folded with xor-shuffles and stored by lanes (r, co). Needs Wq % 4 == 0 (strips never cross a row).
// Same products per output as conv_narrow_kernel, different summation order (fp32 FMAs).
constexpr int NSTRIP = 4;
template <int CO, int S, bool XH = false>
__global__ __launch_bounds__(256) void conv_narrow_strip_kernel(const ConvArgs a) {
    constexpr int CI = 64 * S, LP = 16 * S, GROUPS = 256 / LP, XES = XH ? 2 : 4;
    constexpr int STRIPS = NARROW_PIX / NSTRIP, PASSES = STRIPS / GROUPS;
    const hyres_conv_geom& g = a.g;
    const int tid = threadIdx.x, lq = tid % LP, grp = tid / LP;
    const int phase = blockIdx.y;
    const int ntap = g.ntap[phase], tap0 = g.tap0[phase];
    // the phase's taps as a kh x kw grid listed row-major with steps of +-1 in dh and dw (host-checked: the conv's
    // taps ascend, the transposed conv's phases descend); (r, c) below count from the grid's smallest (dh, dw)
    const int da = g.dh[tap0], wa = g.dw[tap0], dz = g.dh[tap0 + ntap - 1], wz = g.dw[tap0 + ntap - 1];
    const int kh = (da > dz ? da - dz : dz - da) + 1, kw = (wa > wz ? wa - wz : wz - wa) + 1;
    const int dh0 = min(da, dz), dw0 = min(wa, wz);
    const bool rh = da > dz, rw = wa > wz;  // descending rows / columns
    float4 w[3][3][CO];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int t = (rh ? kh - 1 - r : r) * kw + (rw ? kw - 1 - c : c);
#pragma unroll
            for (int co = 0; co < CO; ++co)
                w[r][c][co] = (r < kh && c < kw) ? ld4(a.w2 + (long long)co * a.ldw + (tap0 + t) * CI + 4 * lq)
                                                 : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    const int HqWq = g.Hq * g.Wq;
    int bx = blockIdx.x;
    if (a.xcd) {  // XCD-aware pixel-tile order, as conv_narrow_kernel
        const int nb = gridDim.x, q = nb >> 3, r = nb & 7, x = bx & 7;
        bx = x * q + min(x, r) + (bx >> 3);
    }
    const int b0 = (bx * NARROW_PIX) / HqWq;
    const long long img = (long long)g.Hi * g.Wi * g.ldx;
    const long long xrem = ((long long)g.B - b0) * img * XES;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(reinterpret_cast<const char*>(a.x) + (long long)b0 * img * XES), (short)0,
        (int)(xrem < 0x7FFFFFF0LL ? xrem : 0x7FFFFFF0LL), 0x00020000);
    for (int it = 0; it < PASSES; ++it) {
        const int m = bx * NARROW_PIX + (it * GROUPS + grp) * NSTRIP;  // first pixel of the strip
        const bool ok = m < a.M;
        const int mm = ok ? m : 0;
        const int b = mm / HqWq, rr = mm - b * HqWq;
        const int i = rr / g.Wq, j = rr - (rr / g.Wq) * g.Wq;
        const int base = (int)((b - b0) * img);
        const int ih0 = i * g.ish + dh0, iw0 = j * g.isw + dw0;
        std::conditional_t<XH, half4_t, float4> xv[3][NSTRIP + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < NSTRIP + 2; ++c) {
                const int ih = ih0 + r, iw = iw0 + c;
                const bool in = ok && r < kh && c < kw + NSTRIP - 1 && (unsigned)ih < (unsigned)g.Hi &&
                                (unsigned)iw < (unsigned)g.Wi;
                const int off = in ? (base + (ih * g.Wi + iw) * g.ldx + 4 * lq) * XES : (int)0x80000000;
                if constexpr (XH) xv[r][c] = __builtin_bit_cast(half4_t, __builtin_amdgcn_raw_buffer_load_b64(xr, off, 0, 0));
                else xv[r][c] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
            }
        float acc[NSTRIP][CO];
#pragma unroll
        for (int p = 0; p < NSTRIP; ++p)
#pragma unroll
            for (int co = 0; co < CO; ++co) acc[p][co] = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < NSTRIP + 2; ++c) {
                float4 xf;
                if constexpr (XH) xf = make_float4((float)xv[r][c].x, (float)xv[r][c].y, (float)xv[r][c].z, (float)xv[r][c].w);
                else xf = xv[r][c];
#pragma unroll
                for (int p = 0; p < NSTRIP; ++p) {
                    const int t = c - p;  // this input column is tap column t of strip pixel p
                    if (t < 0 || t > 2) continue;
#pragma unroll
                    for (int co = 0; co < CO; ++co) {
                        acc[p][co] = fmaf(xf.x, w[r][t][co].x, acc[p][co]);
                        acc[p][co] = fmaf(xf.y, w[r][t][co].y, acc[p][co]);
                        acc[p][co] = fmaf(xf.z, w[r][t][co].z, acc[p][co]);
                        acc[p][co] = fmaf(xf.w, w[r][t][co].w, acc[p][co]);
                    }
                }
            }
#pragma unroll
        for (int p = 0; p < NSTRIP; ++p)
#pragma unroll
            for (int co = 0; co < CO; ++co) {
                float v = acc[p][co];
#pragma unroll
                for (int off = LP / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
                acc[p][co] = v;
            }
        // lane q < NSTRIP * CO stores pixel q / CO, channel q % CO
        float v = 0.f;
#pragma unroll
        for (int p = 0; p < NSTRIP; ++p)
#pragma unroll
            for (int co = 0; co < CO; ++co) v = lq == p * CO + co ? acc[p][co] : v;
        const int sp = lq / CO, sc = lq - sp * CO;
        if (ok && lq < NSTRIP * CO && m + sp < a.M) {
            const long long pix = (long long)(b * g.Ho + i * g.osh + g.oph[phase]) * g.Wo + (j + sp) * g.osw + g.opw[phase];
            epi_store(a.e, a.y, g.ldy, pix, sc, v, epi_channel(a.e, sc));
        }
    }
}

// the strip kernel's host-side conditions: every phase's taps a row-major grid of consecutive offsets, <= 3 x 3,
// unit input stride along W, strips inside rows
static bool narrow_strip_ok(const hyres_conv_geom* g) {
    if (g_tune[13] == 0 || g->Wq % NSTRIP != 0 || g->isw != 1) return false;
    for (int p = 0; p < g->nphase; ++p) {
        const int n = g->ntap[p], t0 = g->tap0[p];
        if (n < 1) return false;
        const int da = g->dh[t0], wa = g->dw[t0], dz = g->dh[t0 + n - 1], wz = g->dw[t0 + n - 1];
        const int kh = std::abs(da - dz) + 1, kw = std::abs(wa - wz) + 1;
        const int sh = dz >= da ? 1 : -1, sw = wz >= wa ? 1 : -1;
        if (kh > 3 || kw > 3 || kh * kw != n) return false;
        for (int t = 0; t < n; ++t)
            if (g->dh[t0 + t] != da + sh * (t / kw) || g->dw[t0 + t] != wa + sw * (t % kw)) return false;
    }
    return true;
}

static bool narrow_ok(const hyres_conv_geom* g) {
    if (g->Co > 4 || (g->Ci != 64 && g->Ci != 128)) return false;
    int maxtap = 0;
    for (int p = 0; p < g->nphase; ++p) maxtap = std::max(maxtap, g->ntap[p]);
    return maxtap * g->Co * g->Ci <= NARROW_WLDS;
}

template <int CO>
static void launch_narrow(const ConvArgs& a, bool strip, dim3 grid, hipStream_t st) {
    if (strip) {  // narrow_strip_ok: hyres_conv_tuning key 13 (default 1)
        const bool h = (a.e.io_f16 & HYRES_IO_X16) != 0;
        if (a.g.Ci == 64) {
            if (h) hipLaunchKernelGGL((conv_narrow_strip_kernel<CO, 1, true>), grid, dim3(256), 0, st, a);
            else hipLaunchKernelGGL((conv_narrow_strip_kernel<CO, 1>), grid, dim3(256), 0, st, a);
        } else {
            if (h) hipLaunchKernelGGL((conv_narrow_strip_kernel<CO, 2, true>), grid, dim3(256), 0, st, a);
            else hipLaunchKernelGGL((conv_narrow_strip_kernel<CO, 2>), grid, dim3(256), 0, st, a);
        }
        return;
    }
    if (a.e.io_f16 & HYRES_IO_X16) {
        if (a.g.Ci == 64) hipLaunchKernelGGL((conv_narrow_kernel<CO, 1, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((conv_narrow_kernel<CO, 2, true>), grid, dim3(256), 0, st, a);
        return;
    }
    if (a.g.Ci == 64) hipLaunchKernelGGL((conv_narrow_kernel<CO, 1>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((conv_narrow_kernel<CO, 2>), grid, dim3(256), 0, st, a);
}


// ------------------------------------------------------------------------------------------------
// weight re-layout
// ------------------------------------------------------------------------------------------------
struct PrepArgs {
    const float* w;
    float* w2;
    const float* mask;
    int mode, rows, cols, ntaps, KH, KW, Ci, Co;
    int kh[HYRES_MAX_TAPS], kw[HYRES_MAX_TAPS];
};

__device__ __forceinline__ float prep_value(const PrepArgs& a, long long idx) {
    const int c = (int)(idx % a.cols);
    const long long rt = idx / a.cols;
    const int t = (int)(rt % a.ntaps);
    const int r = (int)(rt / a.ntaps);
    const int kh = a.kh[t], kw = a.kw[t];
    long long src;
    switch (a.mode) {
        case HYRES_WPREP_CONV: src = (((long long)r * a.Ci + c) * a.KH + kh) * a.KW + kw; break;
        case HYRES_WPREP_CONV_DGRAD: src = (((long long)c * a.Ci + r) * a.KH + kh) * a.KW + kw; break;
        case HYRES_WPREP_DECONV: src = (((long long)c * a.Co + r) * a.KH + kh) * a.KW + kw; break;
        default: src = (((long long)r * a.Co + c) * a.KH + kh) * a.KW + kw; break;
    }
    float v = a.w[src];
    if (a.mask) v *= a.mask[src];
    return v;
}

struct PrepDesc {
    PrepArgs a;
    long long begin, count;
};

// grid (chunks, n descriptors): blockIdx.y picks the descriptor (block-uniform: its fields are scalar
// loads), blocks stride over its outputs with 32-bit index math
__global__ __launch_bounds__(256) void weight_prep_batch_kernel(const PrepDesc* d, int n, long long total) {
    const PrepArgs& a = d[blockIdx.y].a;
    const int count = (int)d[blockIdx.y].count;
    const int tc = a.ntaps * a.cols;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < count; idx += gridDim.x * 256) {
        const int r = idx / tc;
        const int rem = idx - r * tc;
        const int t = rem / a.cols;
        const int c = rem - t * a.cols;
        const int kh = a.kh[t], kw = a.kw[t];
        int src;
        switch (a.mode) {
            case HYRES_WPREP_CONV: src = ((r * a.Ci + c) * a.KH + kh) * a.KW + kw; break;
            case HYRES_WPREP_CONV_DGRAD: src = ((c * a.Ci + r) * a.KH + kh) * a.KW + kw; break;
            case HYRES_WPREP_DECONV: src = ((c * a.Co + r) * a.KH + kh) * a.KW + kw; break;
            default: src = ((r * a.Co + c) * a.KH + kh) * a.KW + kw; break;
        }
        a.w2[idx] = a.w[src];
    }
}

__global__ void weight_prep_kernel(const PrepArgs a) {
    const long long total = (long long)a.rows * a.ntaps * a.cols;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % a.cols);
        const long long rt = idx / a.cols;
        const int t = (int)(rt % a.ntaps);
        const int r = (int)(rt / a.ntaps);
        const int kh = a.kh[t], kw = a.kw[t];
        long long src;
        switch (a.mode) {
            case HYRES_WPREP_CONV:  // W[Co][Ci][KH][KW]; r = co, c = ci
                src = (((long long)r * a.Ci + c) * a.KH + kh) * a.KW + kw; break;
            case HYRES_WPREP_CONV_DGRAD:  // r = ci, c = co
                src = (((long long)c * a.Ci + r) * a.KH + kh) * a.KW + kw; break;
            case HYRES_WPREP_DECONV:  // W[Ci][Co][K][K]; r = co, c = ci
                src = (((long long)c * a.Co + r) * a.KH + kh) * a.KW + kw; break;
            default:  // DECONV_DGRAD: r = ci, c = co
                src = (((long long)r * a.Co + c) * a.KH + kh) * a.KW + kw; break;
        }
        float v = a.w[src];
        if (a.mask) v *= a.mask[src];
        a.w2[idx] = v;
    }
}



// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------

static void fill_taps(hyres_conv_geom* g, int p, int* tapcount, int K, int pad, int ph, int pw) {
    // sub-pixel phase (ph, pw) of a stride-2 transposed structure: taps kh with (ph+pad-kh) even
    g->tap0[p] = *tapcount;
    int n = 0;
    for (int kh = 0; kh < K; ++kh) {
        if (((ph + pad - kh) & 1) != 0) continue;
        for (int kw = 0; kw < K; ++kw) {
            if (((pw + pad - kw) & 1) != 0) continue;
            int t = *tapcount + n;
            g->dh[t] = (ph + pad - kh) / 2;
            g->dw[t] = (pw + pad - kw) / 2;
            g->kh[t] = kh;
            g->kw[t] = kw;
            ++n;
        }
    }
    g->ntap[p] = n;
    g->oph[p] = ph;
    g->opw[p] = pw;
    *tapcount += n;
}

static void dense_taps(hyres_conv_geom* g, int KH, int KW, int sgn, int dil, int pad) {
    // one phase, taps in (kh, kw) raster order; offset = sgn * (k*dil - pad)
    g->ntap[0] = KH * KW;
    g->tap0[0] = 0;
    g->ntaps = KH * KW;
    for (int kh = 0; kh < KH; ++kh)
        for (int kw = 0; kw < KW; ++kw) {
            int t = kh * KW + kw;
            g->dh[t] = sgn * (kh * dil - pad);
            g->dw[t] = sgn * (kw * dil - pad);
            g->kh[t] = kh;
            g->kw[t] = kw;
        }
}

// keys: HYRES_TUNE_TILE, _SPLIT_BLOCKS, _SPLIT_MINCHUNKS, _WGRAD_BLOCKS, _WGRAD_MINCHUNKS, _WGRAD_NT,
// _WGRAD_MAXSPLIT
// key 7: fp32 GEMMs bf16x6 (0: native fp32 MFMA); key 8: fp16 streaming 1x1; key 9: the bf16x6 weight-resident 3x3's
// whole-VGPR-file guard (0 = diagnostic unguarded build, DESIGN §4 "Cross-kernel interference"); key 10: the bf16x6
// streaming 1x1 kernel (0 = those layers on the tiled implicit GEMM, for A/B)
int g_tune[HYRES_TUNE_KEYS] = {-1, -1, -1, -1, -1, -1, -1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 1, 1, 1, 0, 1, 0, 1, 1};

}  // namespace hyres

using namespace hyres;

extern "C" {

int hyres_geom_conv2d(hyres_conv_geom* g, int B, int H, int W, int Ci, int ldx, int Co, int ldy, int KH,
                      int KW, int stride, int pad, int dil) {
    HY_REQUIRE(g && KH * KW <= HYRES_MAX_TAPS && stride >= 1 && dil >= 1, HYRES_E_ARG, "bad conv args");
    *g = hyres_conv_geom{};
    g->B = B; g->Hi = H; g->Wi = W; g->Ci = Ci; g->ldx = ldx;
    g->Ho = (H + 2 * pad - dil * (KH - 1) - 1) / stride + 1;
    g->Wo = (W + 2 * pad - dil * (KW - 1) - 1) / stride + 1;
    g->Co = Co; g->ldy = ldy;
    g->nphase = 1; g->Hq = g->Ho; g->Wq = g->Wo;
    g->osh = g->osw = 1; g->ish = g->isw = stride;
    dense_taps(g, KH, KW, 1, dil, pad);
    return ok();
}

int hyres_geom_conv2d_dgrad(hyres_conv_geom* g, int B, int H, int W, int Ci, int ld_dx, int Co, int ld_dy,
                            int KH, int KW, int stride, int pad, int dil) {
    HY_REQUIRE(g && KH * KW <= HYRES_MAX_TAPS, HYRES_E_ARG, "bad conv dgrad args");
    *g = hyres_conv_geom{};
    const int Ho = (H + 2 * pad - dil * (KH - 1) - 1) / stride + 1;
    const int Wo = (W + 2 * pad - dil * (KW - 1) - 1) / stride + 1;
    g->B = B; g->Hi = Ho; g->Wi = Wo; g->Ci = Co; g->ldx = ld_dy;
    g->Ho = H; g->Wo = W; g->Co = Ci; g->ldy = ld_dx;
    if (stride == 1) {
        g->nphase = 1; g->Hq = H; g->Wq = W; g->osh = g->osw = 1; g->ish = g->isw = 1;
        dense_taps(g, KH, KW, -1, dil, pad);  // dX[h] += dY[h + pad - k*dil] W[k]
        return ok();
    }
    HY_REQUIRE(stride == 2 && dil == 1 && KH == KW && (H % 2) == 0 && (W % 2) == 0 && Ho * 2 == H &&
                   Wo * 2 == W, HYRES_E_SHAPE, "conv dgrad: only stride 2, dil 1, square K, even H/W");
    g->nphase = 4; g->Hq = H / 2; g->Wq = W / 2; g->osh = g->osw = 2; g->ish = g->isw = 1;
    int cnt = 0;
    for (int p = 0; p < 4; ++p) fill_taps(g, p, &cnt, KH, pad, p >> 1, p & 1);
    g->ntaps = cnt;
    return ok();
}

int hyres_geom_deconv2d(hyres_conv_geom* g, int B, int H, int W, int Ci, int ldx, int Co, int ldy, int K,
                        int pad) {
    HY_REQUIRE(g && K * K <= HYRES_MAX_TAPS, HYRES_E_ARG, "bad deconv args");
    HY_REQUIRE(2 * pad == K - 1, HYRES_E_SHAPE, "deconv: expects padding = K//2, output_padding = 1");
    *g = hyres_conv_geom{};
    g->B = B; g->Hi = H; g->Wi = W; g->Ci = Ci; g->ldx = ldx;
    g->Ho = 2 * H; g->Wo = 2 * W; g->Co = Co; g->ldy = ldy;
    g->nphase = 4; g->Hq = H; g->Wq = W; g->osh = g->osw = 2; g->ish = g->isw = 1;
    int cnt = 0;
    for (int p = 0; p < 4; ++p) fill_taps(g, p, &cnt, K, pad, p >> 1, p & 1);
    g->ntaps = cnt;
    return ok();
}

int hyres_geom_deconv2d_dgrad(hyres_conv_geom* g, int B, int H, int W, int Ci, int ld_dx, int Co, int ld_dy,
                              int K, int pad) {
    HY_REQUIRE(g && K * K <= HYRES_MAX_TAPS, HYRES_E_ARG, "bad deconv dgrad args");
    *g = hyres_conv_geom{};
    g->B = B; g->Hi = 2 * H; g->Wi = 2 * W; g->Ci = Co; g->ldx = ld_dy;
    g->Ho = H; g->Wo = W; g->Co = Ci; g->ldy = ld_dx;
    g->nphase = 1; g->Hq = H; g->Wq = W; g->osh = g->osw = 1; g->ish = g->isw = 2;
    dense_taps(g, K, K, 1, 1, pad);  // dX[i] += dY[2i - pad + k] W[k]
    return ok();
}

int hyres_geom_filter_taps(hyres_conv_geom* g, const unsigned char* keep, int KW) {
    HY_REQUIRE(g && keep && KW > 0, HYRES_E_ARG, "filter_taps: bad args");
    hyres_conv_geom o = *g;
    int cnt = 0;
    for (int p = 0; p < g->nphase; ++p) {
        o.tap0[p] = cnt;
        int n = 0;
        for (int t = g->tap0[p]; t < g->tap0[p] + g->ntap[p]; ++t) {
            if (!keep[g->kh[t] * KW + g->kw[t]]) continue;
            o.dh[cnt] = g->dh[t]; o.dw[cnt] = g->dw[t]; o.kh[cnt] = g->kh[t]; o.kw[cnt] = g->kw[t];
            ++cnt;
            ++n;
        }
        o.ntap[p] = n;
    }
    o.ntaps = cnt;
    *g = o;
    return ok();
}

int hyres_conv_weight_prep(const hyres_conv_geom* g, const float* w, float* w2, int mode, int Ci, int Co,
                           int KH, int KW, int pad, const float* mask, hyres_stream_t s) {
    HY_REQUIRE(g && w && w2, HYRES_E_ARG, "weight_prep: NULL");
    (void)pad;
    PrepArgs a{};
    a.w = w; a.w2 = w2; a.mask = mask; a.mode = mode; a.KH = KH; a.KW = KW; a.Ci = Ci; a.Co = Co;
    a.ntaps = g->ntaps;
    for (int t = 0; t < g->ntaps; ++t) {
        HY_REQUIRE(g->kh[t] < KH && g->kw[t] < KW, HYRES_E_SHAPE, "weight_prep: tap %d outside %dx%d", t, KH, KW);
        a.kh[t] = g->kh[t];
        a.kw[t] = g->kw[t];
    }
    switch (mode) {
        case HYRES_WPREP_CONV: a.rows = Co; a.cols = Ci; break;
        case HYRES_WPREP_CONV_DGRAD: a.rows = Ci; a.cols = Co; break;
        case HYRES_WPREP_DECONV: a.rows = Co; a.cols = Ci; break;
        case HYRES_WPREP_DECONV_DGRAD: a.rows = Ci; a.cols = Co; break;
        default: return set_error(HYRES_E_ARG, "weight_prep: bad mode %d", mode);
    }
    HY_REQUIRE(a.cols == g->Ci && a.rows >= g->Co, HYRES_E_SHAPE,
               "weight_prep: geometry channels (%d->%d) != weight (%d->%d)", g->Ci, g->Co, a.cols, a.rows);
    long long total = (long long)a.rows * a.ntaps * a.cols;
    int blocks = (int)std::min<long long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(weight_prep_kernel, dim3(blocks), dim3(256), 0, as_stream(s), a);
    return HY_LAUNCH_CHECK("weight_prep_kernel");
}

long long hyres_prep_desc_bytes(void) { return (long long)sizeof(PrepDesc); }

int hyres_prep_desc_fill(void* desc, const hyres_conv_geom* g, const float* w, float* w2, int mode, int Ci, int Co,
                         int KH, int KW, long long begin, long long* count) {
    HY_REQUIRE(desc && g && w && w2 && count, HYRES_E_ARG, "prep_desc_fill: NULL");
    PrepDesc d{};
    PrepArgs& a = d.a;
    a.w = w; a.w2 = w2; a.mask = nullptr; a.mode = mode; a.KH = KH; a.KW = KW; a.Ci = Ci; a.Co = Co;
    a.ntaps = g->ntaps;
    for (int t = 0; t < g->ntaps; ++t) {
        HY_REQUIRE(g->kh[t] < KH && g->kw[t] < KW, HYRES_E_SHAPE, "prep_desc: tap %d outside %dx%d", t, KH, KW);
        a.kh[t] = g->kh[t];
        a.kw[t] = g->kw[t];
    }
    switch (mode) {
        case HYRES_WPREP_CONV: case HYRES_WPREP_DECONV: a.rows = Co; a.cols = Ci; break;
        case HYRES_WPREP_CONV_DGRAD: case HYRES_WPREP_DECONV_DGRAD: a.rows = Ci; a.cols = Co; break;
        default: return set_error(HYRES_E_ARG, "prep_desc: bad mode %d", mode);
    }
    d.begin = begin;
    d.count = (long long)a.rows * a.ntaps * a.cols;
    HY_REQUIRE(d.count < (1LL << 31), HYRES_E_SHAPE, "prep_desc: weight too large");
    *count = d.count;
    memcpy(desc, &d, sizeof(d));
    return ok();
}

int hyres_conv_weight_prep_batch(const void* descs, int n, long long total, hyres_stream_t s) {
    HY_REQUIRE(descs && n > 0 && n <= 65535 && total > 0, HYRES_E_ARG, "prep_batch: bad size");
    hipLaunchKernelGGL(weight_prep_batch_kernel, dim3(64, n), dim3(256), 0, as_stream(s), (const PrepDesc*)descs, n,
                       total);
    return HY_LAUNCH_CHECK("weight_prep_batch_kernel");
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// kernel choice: route() decides which kernel family runs; hyres_conv_forward launches what it says,
// hyres_conv_kernel_name / hyres_conv_plan / hyres_conv_workspace_bytes report it
// ------------------------------------------------------------------------------------------------
enum class ConvFamily { NARROW, WRES32, WRES16, HALO16, STREAM_B6, STREAM, STREAM_HF, STREAM_H, TILES };

struct ConvRoute {
    ConvFamily family;
    int mode;         // 0: vector loads (Ci % 32 == 0), 1: + squared input, 2: scalar loads
    int tile;         // TILES (and the split-K plan): index of TILE_BM / TILE_BN
    ConvGemm gemm;    // TILES: the implicit-GEMM kernel (conv_common.h)
    bool strip;       // NARROW: conv_narrow_strip_kernel
    int cfg;          // streaming kernels: pack_cfg(NT, KC or KS, F)
    int nsplit, cps;  // the split-K plan of `tile` ((1, 0) without a usable workspace); only TILES launches it
    int x_bytes;      // streaming kernels: bytes of X (buffer-resource range)
    bool vec4;        // ConvArgs::vec4
};

// What route() needs to know about the operands beyond geometry and epilogue: hyres_conv_forward fills it from the
// real pointers, the host-only queries assume ideal()
struct ConvFacts {
    bool xw16;           // x and w2 16-byte aligned, ldx and ldw % 4 == 0
    bool vec4;           // every epilogue operand 16-byte aligned with ld % 4 == 0, Co % 4 == 0
    bool rsrc_ok;        // every epilogue operand / output spans < 2 GB
    bool y8, opnd8;      // y / each of res, aux0, out2 8-byte aligned
    long long ws_bytes;  // the workspace supplied (0: none)
    bool ws16;           // ... and 16-byte aligned
    static ConvFacts ideal() { return {true, true, true, true, true, std::numeric_limits<long long>::max(), true}; }
};

static bool fits32(long long bytes) { return bytes < 0x7FFFFFF0LL; }

static int max_taps(const hyres_conv_geom* g) {
    int maxtap = 0;
    for (int ph = 0; ph < g->nphase; ++ph) maxtap = std::max(maxtap, g->ntap[ph]);
    return maxtap;
}

// the epilogue operands are addressed with 32-bit byte offsets (buffer resources)
static bool epi_span_ok(const hyres_conv_geom* g, const hyres_epilogue* e) {
    const int ld = std::max(g->ldy, std::max(e->res ? e->ldres : 0, e->aux0 ? e->ld0 : 0));
    return fits32((long long)g->B * g->Ho * g->Wo * ld * 4);
}

// single-phase, stride-1, same-size 3x3 in whole HALO_TW-pixel row tiles: the halo / weight-resident kernels' geometry
static bool halo_geom(const hyres_conv_geom* g) {
    return g->nphase == 1 && g->ntaps == 9 && g->ish == 1 && g->isw == 1 && g->Hi == g->Ho && g->Wi == g->Wo &&
           g->Hq == g->Ho && g->Wq == g->Wo && g->Wo % HALO_TW == 0;
}

// HALO_R x HALO_TW output tiles of that geometry
static long long halo_tiles(const hyres_conv_geom* g) {
    return (long long)g->B * ((g->Ho + HALO_R - 1) / HALO_R) * (g->Wo / HALO_TW);
}

// the 3x3's largest tap offset (the weight-resident halo radius)
static int wres_halo(const hyres_conv_geom* g) {
    int d = 0;
    for (int t = 0; t < 9; ++t) d = std::max(d, std::max(std::abs(g->dh[t]), std::abs(g->dw[t])));
    return d;
}

// conv3x3_halo_f16_kernel applies (see above)
static bool halo16_ok(const hyres_conv_geom* g, const hyres_epilogue* e) {
    return e->f16_operands && halo_geom(g) && g->Ci % 32 == 0 && g->Co % 64 == 0 && !e->square_input &&
           wres_halo(g) <= 1;
}

// weight-resident 3x3s, blocks per output-channel group: one per CU (persistent), a multiple of 8 so that the
// group-major block order keeps block bg of every group on XCD bg % 8
static int wres_blocks(int groups) {
    return std::max(8, (num_cus() / groups) & ~7);
}

// ... and their size conditions: enough tiles per block to amortise the one-time weight staging (>= 2 per block),
// X within a buffer resource
static bool wres_size_ok(const hyres_conv_geom* g, int groups) {
    return halo_tiles(g) >= 2LL * wres_blocks(groups) && fits32((long long)g->B * g->Hi * g->Wi * g->ldx * 4);
}

// conv3x3_wres_f16_kernel: the halo16 geometry with Ci == 64
static bool wres16_ok(const hyres_conv_geom* g) { return g->Ci == 64 && wres_size_ok(g, g->Co / 64); }

// fp32 GEMM mode of the weight-resident 3x3 (hyres_conv_tuning key 7): 0 = native fp32 MFMA, 1 = bf16x6
static bool wres_bf6() { return g_tune[7] == 1; }

// conv3x3_wres_f32_kernel / conv3x3_wres_bf6_kernel: fp32 operands, the halo16 geometry with Ci == 64 and
// Co % 32 == 0, >= 2 tiles per block
static bool wres32_ok(const hyres_conv_geom* g, const hyres_epilogue* e) {
    if (g_tune[14] == 0) return false;  // A/B: the implicit GEMM instead
    if (e->f16_operands || e->io_f16 || e->square_input || e->kind != HYRES_EPI_BIAS || !halo_geom(g) || g->Ci != 64 ||
        g->Co % 32 != 0 || !epi_span_ok(g, e))
        return false;
    // halo radius 1, or 2 for the bf16x6 kernel (dilation-2 3x3s: its D = 2 build)
    if (wres_halo(g) > (wres_bf6() && g_tune[9] != 0 ? 2 : 1)) return false;
    return wres_size_ok(g, g->Co / 32);
}

static int launch_wres16(const ConvArgs& a, hipStream_t st) {
    const int ntiles = (int)halo_tiles(&a.g), groups = a.g.Co / 64;
    const dim3 grid(wres_blocks(groups) * groups);
    switch (a.e.io_f16 & 3) {
        case 0: hipLaunchKernelGGL(conv3x3_wres_f16_kernel<0>, grid, dim3(512), 0, st, a, ntiles, groups); break;
        case 1: hipLaunchKernelGGL(conv3x3_wres_f16_kernel<1>, grid, dim3(512), 0, st, a, ntiles, groups); break;
        case 2: hipLaunchKernelGGL(conv3x3_wres_f16_kernel<2>, grid, dim3(512), 0, st, a, ntiles, groups); break;
        default: hipLaunchKernelGGL(conv3x3_wres_f16_kernel<3>, grid, dim3(512), 0, st, a, ntiles, groups); break;
    }
    return HY_LAUNCH_CHECK("conv3x3_wres_f16_kernel");
}

static int launch_wres32(const ConvArgs& a, hipStream_t st) {
    const int ntiles = (int)halo_tiles(&a.g), groups = a.g.Co / 32;
    const dim3 grid(wres_blocks(groups) * groups);
    if (!wres_bf6()) {
        hipLaunchKernelGGL(conv3x3_wres_f32_kernel, grid, dim3(512), 0, st, a, ntiles, groups);
        return HY_LAUNCH_CHECK("conv3x3_wres_f32_kernel");
    }
    if (wres_halo(&a.g) == 2)  // dilation 2 (wres32_ok admits it only with the guard on): the pipelined build
        hipLaunchKernelGGL((conv3x3_wres_bf6_kernel<true, 1, 2>), grid, dim3(512), 0, st, a, ntiles, groups);
    else if (g_tune[9] == 0)  // diagnostic only: the allocation that let other kernels' waves share its SIMDs
        hipLaunchKernelGGL((conv3x3_wres_bf6_kernel<false, 0>), grid, dim3(512), 0, st, a, ntiles, groups);
    else if (g_tune[12] == 1)
        hipLaunchKernelGGL((conv3x3_wres_bf6_kernel<true, 1>), grid, dim3(512), 0, st, a, ntiles, groups);
    else if (g_tune[12] == 2)
        hipLaunchKernelGGL((conv3x3_wres_bf6_kernel<true, 2>), grid, dim3(512), 0, st, a, ntiles, groups);
    else if (g_tune[12] == 3)
        hipLaunchKernelGGL((conv3x3_wres_bf6_kernel<true, 3>), grid, dim3(512), 0, st, a, ntiles, groups);
    else
        hipLaunchKernelGGL((conv3x3_wres_bf6_kernel<true, 0>), grid, dim3(512), 0, st, a, ntiles, groups);
    const int rc = HY_LAUNCH_CHECK("conv3x3_wres_bf6_kernel");
    if (rc || a.e.act != HYRES_ACT_PRELU_MASK) return rc;
    return prelu_slope_sum(a.e.aux2, (int)grid.x, a.e.aux1, st);
}

static int launch_halo16(const ConvArgs& a, hipStream_t st) {
    const dim3 grid((int)halo_tiles(&a.g) * (a.g.Co / 64));
    switch (a.e.io_f16 & 3) {
        case 0: hipLaunchKernelGGL(conv3x3_halo_f16_kernel<0>, grid, dim3(256), 0, st, a); break;
        case 1: hipLaunchKernelGGL(conv3x3_halo_f16_kernel<1>, grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL(conv3x3_halo_f16_kernel<2>, grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL(conv3x3_halo_f16_kernel<3>, grid, dim3(256), 0, st, a); break;
    }
    return HY_LAUNCH_CHECK("conv3x3_halo_f16_kernel");
}

static const int TILE_BM[5] = {128, 128, 128, 64, 64};
static const int TILE_BN[5] = {128, 64, 32, 128, 64};

// Tile of the implicit GEMM. tile: 0 = <2,2,2,2> (128x128), 1 = <2,1,2,2> (128x64), 2 = <1,1,4,1> (128x32),
// 3 = <1,2,2,2> (64x128), 4 = <1,1,2,2> (64x64).
//   * short-K 1x1 layers (<= 4 K chunks): half-height tiles — the short main loop cannot hide the operand
//     and epilogue latencies, so twice as many blocks go in flight;
//   * small grids (<= 65536 output pixels: the 64^2 and 32^2 regions at bs 16): 64-row tiles, 64 wide up to
//     192 channels (fp32) / below 192 (f16), else 64x128 (fp32) / 128x128 (f16); measured per geometry
//     over every tile and split-K target (scripts/tile_sweep.py, profiles/r2_tile_sweep_*.txt);
//   * the scalar-load path (Ci % 32 != 0: the 3-channel image side) 64-row tiles (3->64 at 256^2: 198 -> 140 us);
//   * otherwise 128-row tiles as wide as Co allows.
// hyres_conv_tuning key HYRES_TUNE_TILE overrides it (tuning sweeps; -1 = these heuristics).
static void choose_tile(const hyres_conv_geom* g, const hyres_epilogue* e, ConvRoute& c) {
    constexpr long long small_px = 65536;
    const bool f16 = e->f16_operands && c.mode != 2;
    const bool short_k = c.mode != 2 && g->nphase == 1 && g->ntaps == 1 && g->Ci <= 4 * KT;
    const long long mtot = (long long)g->B * g->Hq * g->Wq * g->nphase;
    // fp32 small grids (round 6, profiles/r6g_tile32.txt, 32^2 bs16 bf16x6): the 1x1 96 -> 192 (+res) 14.9 -> 13.1 us on
    // 64x64 tiles, 640 -> 512 102 -> 81 us on 128x128
    // (hyres_conv_tuning key 18 = 0: the round-5 rule, A/B)
    const bool r6 = g_tune[18] != 0;
    if (short_k && g->Co > 64 && !(r6 && !f16 && mtot <= small_px && g->Co <= 192)) c.tile = 3;
    else if (short_k && g->Co > 32) c.tile = 4;
    else if (c.mode != 2 && g->Co > 32 && mtot <= small_px) {
        // K depth of the deepest phase: the K-heavy single-phase layers take the bigger tiles (fragment reuse) —
        // 128^2 -> 64^2 5x5 s2 128 -> 128 434 -> 347 us on 128x128, 32^2 3x3 384 -> 192 195 -> 183 us and 64^2 -> 32^2
        // 5x5 s2 128 -> 192 183 -> 172 us on 128x64 (profiles/r6p_tile5.txt)
        int maxtap = 0;
        for (int ph = 0; ph < g->nphase; ++ph) maxtap = std::max(maxtap, g->ntap[ph]);
        const bool kheavy = g->nphase == 1 && (long long)maxtap * g->Ci >= 1024;
        if (f16) c.tile = g->Co >= 192 ? 0 : 4;
        else if (r6 && (g->Co >= 512 || (kheavy && mtot >= small_px && g->Co >= 128))) c.tile = 0;
        else if (r6 && kheavy && g->Co == 192) c.tile = 1;
        else c.tile = g->Co > 192 ? 3 : 4;
    }
    else if (c.mode == 2 && g->Co > 32) c.tile = g->Co > 64 ? 3 : 4;  // scalar-load path: 64-row tiles
    else if (g->Co > 64) c.tile = 0;
    else if (g->Co > 32) c.tile = 1;
    else c.tile = 2;
    if (g_tune[0] >= 0 && g_tune[0] <= 4) c.tile = g_tune[0];
}

// Split-K of the implicit GEMM on r.tile: engages only when the tile leaves fewer than 512 blocks and K has >= 8
// chunks (keys HYRES_TUNE_SPLIT_BLOCKS, _SPLIT_MINCHUNKS)
static void plan_split(const hyres_conv_geom* g, ConvRoute& r) {
    const long long blocks =
        (long long)ceil_div(gemm_rows(g), TILE_BM[r.tile]) * ceil_div(g->Co, TILE_BN[r.tile]) * g->nphase;
    const int maxtap = max_taps(g);
    const int nk = (g->Ci % KT == 0) ? maxtap * (g->Ci / KT) : ceil_div((long long)maxtap * g->Ci, KT);
    r.nsplit = 1;
    r.cps = nk;
    const int sb = g_tune[1] >= 0 ? g_tune[1] : 512;
    const int sc = g_tune[2] > 0 ? g_tune[2] : 4;
    if (blocks < sb && nk >= 2 * sc) {
        // split K so that ~sb blocks are in flight, at least sc chunks per split
        int want = (int)std::min<long long>(ceil_div(sb, blocks), 64);
        int ns = std::max(1, std::min(want, nk / sc));
        r.cps = ceil_div(nk, ns);
        r.nsplit = ceil_div(nk, r.cps);
    }
}

static long long split_ws_bytes(const hyres_conv_geom* g, int nsplit) {
    if (nsplit <= 1) return 0;
    return (long long)nsplit * g->nphase * gemm_rows(g) * g->Co * 4;
}

static ConvGemm choose_gemm(const hyres_conv_geom* g, const hyres_epilogue* e, const ConvRoute& r) {
    if (e->io_f16 & 3) return ConvGemm::H;
    if (r.mode == 2) return ConvGemm::F32;
    if (e->f16_operands) return ConvGemm::F16;
    if (g_tune[7] != 1) return ConvGemm::F32;  // fp32 GEMM on the fp32 MFMA; else on the bf16 MFMA (bf16x6)
    // double-buffered staging (key 20 = 1, or -1: on for the <= 16384-pixel grids). Isolated it wins at 32^2
    // (3x3 96 -> 96 39.6 -> 37.3 us, 1x1 192 -> 96 13.9 -> 13.1 us) and loses on the larger-K 64^2 / 5x5 layers
    // (+2..5 %: the 49 KB of LDS cost the 4th block per CU, profiles/r6m_b6db.txt); in the graphed step the
    // small-grid rule measured 0.2-0.3 ms SLOWER (profiles/r6n_b6db_step_ab.txt: those layers run beside the
    // branch streams' kernels), so the default is off
    const bool db = r.tile == 4 && (g_tune[20] == 1 || (g_tune[20] < 0 && gemm_rows(g) <= 16384));
    return db ? ConvGemm::B6DB : ConvGemm::B6;
}

// The one kernel choice, in this order: narrow, weight-resident fp32 3x3, halo / weight-resident f16 3x3, the four
// streaming 1x1s (bf16x6, fp32, f16 with a streamed operand, f16 without), the implicit-GEMM tiles.
static ConvRoute route(const hyres_conv_geom* g, const hyres_epilogue* e, const ConvFacts& f) {
    ConvRoute r{};
    r.mode = (g->Ci % KT == 0) ? (e->square_input ? 1 : 0) : 2;
    choose_tile(g, e, r);
    r.nsplit = 1;
    r.vec4 = f.vec4;
    if (narrow_ok(g) && !e->square_input && e->kind == HYRES_EPI_BIAS && f.xw16) {
        r.family = ConvFamily::NARROW;
        r.strip = narrow_strip_ok(g);
        return r;
    }
    plan_split(g, r);
    if (r.nsplit > 1 && f.ws_bytes >= split_ws_bytes(g, r.nsplit)) {
        r.vec4 = f.vec4 && f.ws16;  // the slab is read four floats at a time
    } else {  // without workspace: single pass (correct, slower)
        r.nsplit = 1;
        r.cps = 0;
    }
    const bool vec = r.mode == 0 && f.xw16;
    if (vec && r.vec4 && wres32_ok(g, e)) {
        r.family = ConvFamily::WRES32;
        return r;
    }
    if (vec && r.vec4 && halo16_ok(g, e)) {
        r.family = wres16_ok(g) ? ConvFamily::WRES16 : ConvFamily::HALO16;
        return r;
    }
    // a streaming kernel takes the layer if it is eligible (cfg != 0) and X fits a buffer resource
    auto stream = [&](ConvFamily family, int cfg, int x_elem) {
        const long long xb = gemm_rows(g) * g->ldx * x_elem;
        if (!cfg || !fits32(xb)) return false;
        r.family = family;
        r.cfg = cfg;
        r.x_bytes = (int)xb;
        return true;
    };
    if (vec && r.vec4 && f.rsrc_ok && stream(ConvFamily::STREAM_B6, stream_b6_cfg(g, e), 4)) return r;
    if (vec && r.vec4 && stream(ConvFamily::STREAM, stream_cfg(g, e), 4)) return r;
    if (vec && f.rsrc_ok && f.y8 && f.opnd8 && stream(ConvFamily::STREAM_HF, stream_hf_cfg(g, e), 2)) return r;
    if (vec && f.y8 && stream(ConvFamily::STREAM_H, stream_h_cfg(g, e), 2)) return r;
    r.family = ConvFamily::TILES;
    r.gemm = choose_gemm(g, e, r);
    return r;
}

// ConvFacts of a launch from its real operands: only the pointers' alignment is read, never what they point to
static ConvFacts conv_facts(const hyres_conv_geom* g, const hyres_epilogue* e, const void* x, const void* w2, int ldw,
                            const void* y, const void* ws, long long ws_bytes) {
    ConvFacts f;
    f.xw16 = aligned16(x) && aligned16(w2) && g->ldx % 4 == 0 && ldw % 4 == 0;
    {
        auto al = [](const void* p, int ld) { return p == nullptr || (aligned16(p) && ld % 4 == 0); };
        // HYRES_EPI_SA_BWD reads aux0 ([P][2]) and aux2 (argmax), HYRES_EPI_ROWSCALE aux1 (the scale), one scalar per
        // pixel: no alignment needed
        const bool sa = e->kind == HYRES_EPI_SA_BWD, rs = e->kind == HYRES_EPI_ROWSCALE;
        f.vec4 = g->Co % 4 == 0 && al(y, g->ldy) && al(e->bias, 4) && al(e->res, e->ldres) && al(e->out2, e->ldo2) &&
                 (sa || al(e->aux0, e->ld0)) && (rs || al(e->aux1, e->ld1)) && (sa || al(e->aux2, e->ld2));
    }
    f.rsrc_ok = epi_span_ok(g, e);
    f.y8 = aligned8(y);
    f.opnd8 = aligned8(e->res) && aligned8(e->aux0) && aligned8(e->out2);
    f.ws_bytes = ws ? ws_bytes : 0;
    f.ws16 = aligned16(ws);
    return f;
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static int launch_narrow_co(const ConvArgs& a, const ConvRoute& r, hipStream_t st) {
    const dim3 grid(ceil_div(a.M, NARROW_PIX), a.g.nphase);
    switch (a.g.Co) {
        case 1: launch_narrow<1>(a, r.strip, grid, st); break;
        case 2: launch_narrow<2>(a, r.strip, grid, st); break;
        case 3: launch_narrow<3>(a, r.strip, grid, st); break;
        default: launch_narrow<4>(a, r.strip, grid, st); break;
    }
    return HY_LAUNCH_CHECK("conv_narrow_kernel");
}

extern "C" {

int hyres_conv_tuning(int key, int value, int* old) {
    HY_REQUIRE(key >= 0 && key < HYRES_TUNE_KEYS, HYRES_E_ARG, "conv_tuning: key %d", key);
    if (old) *old = g_tune[key];
    g_tune[key] = value;
    return ok();
}

long long hyres_conv_workspace_bytes(const hyres_conv_geom* g) {
    // the larger of the fp32 and fp16-operand plans (the tile, hence the split, depends on the dtype)
    if (!g) return 0;
    long long need = 0;
    for (int f16 = 0; f16 < 2; ++f16) {
        hyres_epilogue e{};
        e.kind = HYRES_EPI_BIAS;
        e.f16_operands = f16;
        need = std::max(need, split_ws_bytes(g, route(g, &e, ConvFacts::ideal()).nsplit));
    }
    return need;
}

int hyres_conv_plan(const hyres_conv_geom* g, const hyres_epilogue* e, int* tile, int* nsplit) {
    HY_REQUIRE(g && e, HYRES_E_ARG, "conv_plan: NULL argument");
    const ConvRoute r = route(g, e, ConvFacts::ideal());
    if (tile) *tile = r.family == ConvFamily::NARROW ? -1 : r.tile;
    if (nsplit) *nsplit = r.nsplit;
    return ok();
}

int hyres_conv_forward(const hyres_conv_geom* g, const float* x, const float* w2, int ldw, float* y,
                       const hyres_epilogue* e, void* ws, long long ws_bytes, hyres_stream_t s) {
    HY_REQUIRE(g && x && w2 && y && e, HYRES_E_ARG, "conv_forward: NULL argument");
    HY_REQUIRE(g->nphase >= 1 && g->nphase <= 4 && g->Ci > 0 && g->Co > 0, HYRES_E_SHAPE, "conv: bad geom");
    HY_REQUIRE(ldw >= g->ntaps * g->Ci, HYRES_E_SHAPE, "conv: ldw %d < ntaps*Ci %d", ldw, g->ntaps * g->Ci);
    const ConvFacts f = conv_facts(g, e, x, w2, ldw, y, ws, ws_bytes);
    const ConvRoute r = route(g, e, f);
    const int mode = r.mode;
    ConvArgs a;
    a.g = *g; a.x = x; a.w2 = w2; a.ldw = ldw; a.y = y; a.e = *e;
    a.M = g->B * g->Hq * g->Wq;
    a.xcd = 1;
    a.prio = 1;
    a.b6sw = g_tune[19] != 0;
    a.vec4 = r.vec4;
    a.rsrc_ok = f.rsrc_ok;
    a.x_bytes = r.x_bytes;
    a.nsplit = r.family == ConvFamily::TILES ? r.nsplit : 1;
    a.cps = r.cps;
    a.slab = r.nsplit > 1 ? (float*)ws : nullptr;
    {
        const long long wb = (long long)g->Co * ldw * 4;
        const long long img_bytes = (long long)g->Hi * g->Wi * g->ldx * 4;
        HY_REQUIRE(fits32(wb) && fits32(3 * img_bytes) && (long long)g->Ho * g->Wo * g->ldy < 0x7FFFFFFFLL,
                   HYRES_E_SHAPE, "conv: per-image tensor too large for 32-bit offsets");
        a.w_bytes = (int)wb;
    }
    if (mode != 2) {
        HY_REQUIRE(f.xw16, HYRES_E_ALIGN, "conv: vector path needs 16B-aligned x/w2 and ldx,ldw %% 4 == 0");
    } else {
        HY_REQUIRE(g->nphase == 1 && !e->square_input, HYRES_E_SHAPE,
                   "conv: Ci %% 32 != 0 supported only single-phase, no square");
    }
    if (e->kind == HYRES_EPI_GDN || e->kind == HYRES_EPI_IGDN)
        HY_REQUIRE(e->aux0 && e->out2, HYRES_E_ARG, "conv: GDN epilogue needs aux0/out2");
    if (e->kind == HYRES_EPI_GDN_BWD || e->kind == HYRES_EPI_IGDN_BWD)
        HY_REQUIRE(e->aux0 && e->aux1 && e->aux2, HYRES_E_ARG, "conv: GDN bwd epilogue needs aux0..2");
    if (e->act == HYRES_ACT_PRELU) HY_REQUIRE(e->slope, HYRES_E_ARG, "conv: PReLU needs slope");
    HY_REQUIRE(e->io_f16 >= 0 && e->io_f16 <= 4, HYRES_E_ARG, "conv: io_f16 %d (fp16 X/Y bits, or AUX16 alone)",
               e->io_f16);
    if (e->io_f16 & 3) {
        HY_REQUIRE(e->io_f16 >= 1 && e->io_f16 <= 3 && (!(e->kind == HYRES_EPI_GDN_BWD || e->kind == HYRES_EPI_IGDN_BWD)
                                                         || (e->io_f16 & 2)),
                   HYRES_E_ARG, "conv: a fp16 GDN-backward epilogue needs fp16 Y (its operands share Y's dtype)");
        HY_REQUIRE(!(e->io_f16 & 1) || mode != 2, HYRES_E_ARG, "conv: fp16 X needs Ci %% 32 == 0");
        HY_REQUIRE(r.family != ConvFamily::NARROW || !(e->io_f16 & 2), HYRES_E_ARG,
                   "conv: the Co <= 4 kernel writes fp32 only");
    }
    if (e->act == HYRES_ACT_RELU_MASK)
        HY_REQUIRE(e->aux0 && e->kind == HYRES_EPI_BIAS, HYRES_E_ARG, "conv: ReLU mask needs aux0, BIAS epilogue");
    if (e->act == HYRES_ACT_PRELU_MASK && e->kind == HYRES_EPI_SA_BWD) {  // round 6: the scale-1 PReLU on SA_BWD
        HY_REQUIRE(e->aux1 && e->ld1 >= 64 && e->slope && e->res && e->out2 && e->ldo2 >= HYRES_PRELU_PARTIALS &&
                       !e->accumulate,
                   HYRES_E_ARG, "conv: SA_BWD + PReLU mask needs aux1 (pre-activation of channels 0..63, ld1 >= 64), "
                   "slope, res (slope gradient), out2 (>= %d partials), no accumulate", HYRES_PRELU_PARTIALS);
    } else if (e->act == HYRES_ACT_PRELU_MASK) {
        HY_REQUIRE(e->aux0 && e->aux1 && e->aux2 && e->slope && e->kind == HYRES_EPI_BIAS && !e->accumulate &&
                       !e->out2 && e->io_f16 == 0 && !e->f16_operands && e->ld2 >= HYRES_PRELU_PARTIALS,
                   HYRES_E_ARG, "conv: PReLU mask needs aux0 (pre-activation), aux1 (slope gradient), aux2 (>= %d "
                   "partials), slope; BIAS, no accumulate / out2, fp32", HYRES_PRELU_PARTIALS);
        HY_REQUIRE(r.family == ConvFamily::WRES32 && wres_bf6() &&
                       wres_blocks(g->Co / 32) * (g->Co / 32) <= HYRES_PRELU_PARTIALS,
                   HYRES_E_ARG, "conv: the PReLU-mask epilogue runs on conv3x3_wres_bf6_kernel only");
    }
    if (e->kind == HYRES_EPI_ROWSCALE)
        HY_REQUIRE(e->aux1 && !e->square_input && !e->accumulate, HYRES_E_ARG,
                   "conv: ROWSCALE needs aux1 (per-pixel scale), no square_input / accumulate");
    if (e->kind == HYRES_EPI_SA_BWD)
        HY_REQUIRE(e->aux0 && e->aux2 && e->ld0 >= 2 && !e->square_input &&
                       ((e->act == HYRES_ACT_NONE && !e->res && !e->out2) || e->act == HYRES_ACT_PRELU_MASK) &&
                       (!(e->io_f16 & 2) || stream_hf_cfg(g, e)),
                   HYRES_E_ARG, "conv: SA_BWD needs aux0 ([P][ld0 >= 2]) and aux2 (argmax), no act / res / out2, fp32 Y "
                   "(fp16 Y: conv1x1_stream_hf_kernel's 64 -> 192 only)");
    // no other kernel implements SA_BWD with an fp16 Y (its epi_store4 instantiations leave the case out)
    if (r.family == ConvFamily::STREAM_H || r.family == ConvFamily::TILES)
        HY_REQUIRE(!(e->kind == HYRES_EPI_SA_BWD && ((e->io_f16 & 2) || e->act == HYRES_ACT_PRELU_MASK)), HYRES_E_ARG,
                   "conv: an fp16-Y or PReLU-mask SA_BWD input-gradient needs the streaming kernels (alignment / size / "
                   "split mode)");
    hipStream_t st = as_stream(s);
    switch (r.family) {
        case ConvFamily::NARROW: return launch_narrow_co(a, r, st);
        case ConvFamily::WRES32: return launch_wres32(a, st);
        case ConvFamily::WRES16: return launch_wres16(a, st);
        case ConvFamily::HALO16: return launch_halo16(a, st);
        case ConvFamily::STREAM_B6: return launch_stream_b6(a, r.cfg, st);
        case ConvFamily::STREAM: return launch_stream(a, r.cfg, st);
        case ConvFamily::STREAM_HF: return launch_stream_hf(a, r.cfg, st);
        case ConvFamily::STREAM_H: return launch_stream_h(a, r.cfg, st);
        case ConvFamily::TILES: break;
    }
    return launch_tiles(a, r.tile, r.mode, r.gemm, st);
}

// the kernel of route r as rocprof prints it (split: the split-K instantiation of the tiles)
static void conv_route_name(const hyres_conv_geom* g, const hyres_epilogue* e, const ConvRoute& r, bool split, char* buf,
                            int n) {
    static const char* tiles[5] = {"2, 2, 2, 2", "2, 1, 2, 2", "1, 1, 4, 1", "1, 2, 2, 2", "1, 1, 2, 2"};
    const int nt = cfg_nt(r.cfg), k = cfg_k(r.cfg), f = cfg_f(r.cfg), io = e->io_f16 & 3;
    const char* sp = split ? "true" : "false";
    switch (r.family) {
        case ConvFamily::NARROW:
            snprintf(buf, n, "%s<%d, %d>", r.strip ? "conv_narrow_strip_kernel" : "conv_narrow_kernel",
                     std::min(g->Co, 4), g->Ci == 64 ? 1 : 2);
            break;
        case ConvFamily::WRES32:
            snprintf(buf, n, wres_bf6() ? "conv3x3_wres_bf6_kernel" : "conv3x3_wres_f32_kernel");
            break;
        case ConvFamily::WRES16: snprintf(buf, n, "conv3x3_wres_f16_kernel<%d>", io); break;
        case ConvFamily::HALO16: snprintf(buf, n, "conv3x3_halo_f16_kernel<%d>", io); break;
        case ConvFamily::STREAM_B6:
            snprintf(buf, n, "conv1x1_stream_b6_kernel<%d, %d, %d, %s>", nt, k, f, stream_b6_ce() ? "true" : "false");
            break;
        case ConvFamily::STREAM:
            snprintf(buf, n, "conv1x1_stream_kernel<%d, %d%s>", nt, k, e->f16_operands ? ", true" : "");
            break;
        case ConvFamily::STREAM_HF: snprintf(buf, n, "conv1x1_stream_hf_kernel<%d, %d, %d>", nt, k, f); break;
        case ConvFamily::STREAM_H: snprintf(buf, n, "conv1x1_stream_h_kernel<%d, %d>", nt, k); break;
        case ConvFamily::TILES:
            switch (r.gemm) {
                case ConvGemm::H:
                    snprintf(buf, n, "conv_fwd_h_kernel<%s, %d, %s, %d>", tiles[r.tile], r.mode, sp, io);
                    break;
                case ConvGemm::B6DB:
                    snprintf(buf, n, "conv_fwd_b6db_kernel<%s, %d, %s>", tiles[r.tile], r.mode, sp);
                    break;
                case ConvGemm::B6: snprintf(buf, n, "conv_fwd_b6_kernel<%s, %d, %s>", tiles[r.tile], r.mode, sp); break;
                default:
                    snprintf(buf, n, "conv_fwd_kernel<%s, %d, %s, %s>", tiles[r.tile], r.mode, sp,
                             r.gemm == ConvGemm::F16 ? "true" : "false");
            }
    }
}

int hyres_conv_kernel_name(const hyres_conv_geom* g, const hyres_epilogue* e, int split, char* buf, int n) {
    HY_REQUIRE(g && e && buf && n > 0, HYRES_E_ARG, "conv_kernel_name: bad args");
    conv_route_name(g, e, route(g, e, ConvFacts::ideal()), split != 0, buf, n);
    return 0;
}

int hyres_conv_kernel_name_at(const hyres_conv_geom* g, const hyres_epilogue* e, const void* x, const void* w2, int ldw,
                              const void* y, const void* ws, long long ws_bytes, int* vec4, char* buf, int n) {
    HY_REQUIRE(g && e && buf && n > 0, HYRES_E_ARG, "conv_kernel_name_at: bad args");
    const ConvRoute r = route(g, e, conv_facts(g, e, x, w2, ldw, y, ws, ws_bytes));
    const bool split = r.family == ConvFamily::TILES && r.nsplit > 1;
    conv_route_name(g, e, r, split, buf, n);
    if (split) {  // launch_tiles' second kernel
        const size_t len = strlen(buf);
        snprintf(buf + len, n - len, "+%s<%s>", r.vec4 ? "conv_splitk_reduce4_kernel" : "conv_splitk_reduce_kernel",
                 (e->io_f16 & 2) ? "true" : "false");
    }
    if (vec4) *vec4 = r.vec4;
    return 0;
}

int hyres_wgrad_desc_conv2d(hyres_wgrad_desc* d, int B, int H, int W, int Ci, int ldx, int Co, int ldy,
                            int KH, int KW, int stride, int pad, int dil) {
    HY_REQUIRE(d && KH * KW <= HYRES_MAX_TAPS, HYRES_E_ARG, "bad wgrad args");
    *d = hyres_wgrad_desc{};
    const int Ho = (H + 2 * pad - dil * (KH - 1) - 1) / stride + 1;
    const int Wo = (W + 2 * pad - dil * (KW - 1) - 1) / stride + 1;
    d->B = B; d->Hq = Ho; d->Wq = Wo;
    d->M = Co; d->ldp = ldy;
    d->N = Ci; d->ldq = ldx; d->Hqq = H; d->Wqq = W; d->sq = stride;
    d->ntaps = KH * KW;
    for (int kh = 0; kh < KH; ++kh)
        for (int kw = 0; kw < KW; ++kw) {
            d->dh[kh * KW + kw] = kh * dil - pad;
            d->dw[kh * KW + kw] = kw * dil - pad;
        }
    d->sm = Ci * KH * KW; d->sn = KH * KW; d->st = 1;
    return ok();
}

int hyres_wgrad_desc_deconv2d(hyres_wgrad_desc* d, int B, int H, int W, int Ci, int ldx, int Co, int ldy,
                              int K, int pad) {
    HY_REQUIRE(d && K * K <= HYRES_MAX_TAPS, HYRES_E_ARG, "bad wgrad args");
    *d = hyres_wgrad_desc{};
    d->B = B; d->Hq = H; d->Wq = W;
    d->M = Ci; d->ldp = ldx;
    d->N = Co; d->ldq = ldy; d->Hqq = 2 * H; d->Wqq = 2 * W; d->sq = 2;
    d->ntaps = K * K;
    for (int kh = 0; kh < K; ++kh)
        for (int kw = 0; kw < K; ++kw) {
            d->dh[kh * K + kw] = kh - pad;
            d->dw[kh * K + kw] = kw - pad;
        }
    d->sm = Co * K * K; d->sn = K * K; d->st = 1;
    return ok();
}

}  // extern "C"
