// The implicit-GEMM convolution family: conv_fwd_kernel (fp32 / f16 MFMA operands), conv_fwd_b6_kernel and
// conv_fwd_b6db_kernel (fp32 operands, bf16x6 products), conv_fwd_h_kernel (fp16 activations in HBM), the split-K
// reduce kernels and their launcher. hyres_conv_forward (conv.hip) reaches them through launch_tiles, declared in
// conv_common.h; the generic epilogue they share with the halo-tiled and narrow kernels is in conv_epilogue.h.
//     Y[b, i*osh+oph, j*osw+opw, co] = epi( sum_{t in taps(phase)} sum_ci X[b, i*ish+dh_t, j*isw+dw_t, ci] * W2[co][t][ci] )
// GEMM view: M = output pixels of one phase (NHWC rows), N = output channels, K = taps x Ci.
//   * operands are staged HBM -> registers -> LDS in 32-deep K chunks (the next chunk's global
//     loads are issued before the current chunk's MFMAs: issue-early / write-late);
//   * the MFMA is v_mfma_f32_32x32x2_f32 (exact fp32, 64 FLOP/clk/SIMD = the fp32 peak);
//   * both LDS tiles are stored K-contiguous ([row][k], +4 float pad) and the K order inside a chunk
//     is permuted so that lane-half h consumes k = 16h + s at MFMA step s: one ds_read_b128 feeds four
//     consecutive MFMA steps (conflict-free with the 36-float row pitch).
#include "conv_epilogue.h"

namespace hyres {

constexpr int PADK = 36;  // LDS row pitch (floats)

// bf16x8_t / bf16x4_t, bf6_split4, bf6_mfma, bf6_put3: conv_common.h (shared with the bf16x6 weight gradients)

// ---- stage to LDS: the four channels k = 4 * c4 .. + 3 of row `row` of an operand's tile T, one store per operand
// format (fp32, f16; bf16x6: bf6_put3). conv_fwd_body calls each once for its A rows and once for its B rows.
__device__ __forceinline__ void put_row_f32(float* T, int row, int c4, const float4& v) {
    *reinterpret_cast<float4*>(&T[row * PADK + 4 * c4]) = v;
}
template <int PADH>
__device__ __forceinline__ void put_row_f16(_Float16* T, int row, int c4, half4_t h) {
    *reinterpret_cast<half4_t*>(&T[row * PADH + 4 * c4]) = h;
}
__device__ __forceinline__ half4_t f2h4(const float4& v) {
    return half4_t{(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
}

// One block of the implicit GEMM, top to bottom: block coordinates, the thread's A rows and the X / W resources, the
// chunk load (load_chunk) and its staging to LDS (store_chunk), one lambda per MFMA flavour, the K loop, the epilogue.
template <int TM, int TN, int WAVES_M, int WAVES_N, int MODE, bool SPLITK, bool F16, int IO, bool B6 = false,
          bool DB = false>
__device__ __forceinline__ void conv_fwd_body(const ConvArgs& a) {
    // MODE 0: Ci % 32 == 0 (float4 loads); 1: same + square A (GDN); 2: generic scalar (small Ci).
    // F16: operands rounded to fp16 when staged into LDS ([row][32 halves], pitch PADH halves) and
    // consumed by v_mfma_f32_32x32x16_f16 (lane r,h holds row r, k = 8h..8h+7), fp32 accumulation.
    // IO (fp16 activations in HBM, autocast inference): bit 0 X is fp16 (8-byte loads of 4 channels),
    // bit 1 Y / res / aux0 / out2 are fp16; arithmetic stays fp32 (F16: fp16 MFMA operands as before).
    // B6: fp32 operands split into three bf16 planes when staged ([plane][row][32], pitch PADH), products to fp32
    // accuracy on v_mfma_f32_32x32x16_bf16 (bf6_mfma; hyres_conv_tuning key 7, conv3x3_wres_bf6_kernel's numerics)
    static_assert(!F16 || MODE != 2, "fp16 operands on the Ci % 32 == 0 paths only");
    static_assert(!B6 || (!F16 && IO == 0 && MODE != 2), "bf16x6: fp32 operands on the vector path");
    static_assert(!(IO & 1) || MODE != 2, "fp16 X on the Ci % 32 == 0 paths only");
    // DB (round 6, bf16x6 only): two LDS buffers of swizzled 64-B rows, one barrier per K chunk — chunk k + 1 is split
    // and stored into the other buffer right after chunk k's MFMAs, while other waves may still read chunk k
    static_assert(!DB || B6, "double-buffered staging: the bf16x6 path");
    constexpr bool XH = (IO & 1) != 0, YH = (IO & 2) != 0;
    constexpr int XES = XH ? 2 : 4;  // X element bytes
    constexpr int PADH = 40;
    constexpr int BM = 32 * TM * WAVES_M;
    constexpr int BN = 32 * TN * WAVES_N;
    constexpr int SOP = DB ? 2 * 3 * (BM + BN) * 32 / 2 : B6 ? 3 * (BM + BN) * PADH / 2 : (BM + BN) * PADK;  // staging (floats)
    constexpr int SMEM = (SOP > BM * (32 * WAVES_N + 8)) ? SOP : BM * (32 * WAVES_N + 8);
    __shared__ __attribute__((aligned(16))) float smem[SMEM];
    float* const As = smem;
    float* const Bs = smem + BM * PADK;
    _Float16* const Ah = reinterpret_cast<_Float16*>(smem);
    _Float16* const Bh = Ah + BM * PADH;
    __bf16* const Pb0 = reinterpret_cast<__bf16*>(smem);  // B6: plane p = Pb0 + p * PLANE, A rows then B (DB: + buffer)
    // B6 row layout (round 6): b6sw = 1 (default) 32-half rows, 16-B slot s of row r stored at slot s ^ ((r >> 2) & 3):
    // the split stores (ds_write_b64, 16-lane groups = two consecutive rows, banks mod 32) then fill complementary
    // halves of the 32 banks, and every ds_read_b128 lane group (16 rows, banks mod 64) meets 16 distinct slots.
    // b6sw = 0: the 40-half padded rows (reads conflict-free, the stores 2-way: SQ_LDS_BANK_CONFLICT 0.33 of the LDS
    // cycles at 32^2, profiles/r6f_pmc_families.txt). Same products in the same order either way.
    const int b6p = (DB || (B6 && a.b6sw)) ? 32 : PADH;
    const int PLANE = (BM + BN) * b6p;

    // ---- block coordinates
    const hyres_conv_geom& g = a.g;
    const int tid = threadIdx.x;
    const int nsplit = SPLITK ? a.nsplit : 1;
    const int phase = blockIdx.z / nsplit;
    const int split = blockIdx.z - phase * nsplit;
    // XCD-aware tile order (a.xcd): hardware block b runs on XCD b % 8, so XCD x gets the contiguous
    // logical range [x*q + min(x, r), ...) of the nb = q*8 + r tiles (a bijection for any nb); within
    // it the N tiles of one M tile are adjacent. Neighbouring pixel tiles (the 3x3/5x5 halo rows) and
    // the N tiles sharing an A tile then hit one L2 instead of being spread over all eight.
    int m0, n0;
    if (a.xcd) {
        const int l = xcd_logical_block();
        const int ntn = (g.Co + BN - 1) / BN;
        m0 = (l / ntn) * BM;
        n0 = (l - (l / ntn) * ntn) * BN;
    } else {
        m0 = blockIdx.x * BM;
        n0 = blockIdx.y * BN;
    }
    const int HqWq = g.Hq * g.Wq;
    const int ntap = g.ntap[phase];
    const int tap0 = g.tap0[phase];
    const int Ci = g.Ci;

    constexpr int A_V = (MODE == 2) ? (BM * KT / 256) : (BM / 32);
    constexpr int B_V = (MODE == 2) ? (BN * KT / 256) : (BN / 32);

    // ---- per-thread A rows (pixel decode once)
    int a_b[A_V], a_i[A_V], a_j[A_V];
    bool a_ok[A_V];
#pragma unroll
    for (int q = 0; q < A_V; ++q) {
        int row = (MODE == 2) ? ((tid + 256 * q) / KT) : (tid / 8 + 32 * q);
        int m = m0 + row;
        a_ok[q] = m < a.M;
        int mm = a_ok[q] ? m : 0;
        a_b[q] = mm / HqWq;
        int r = mm - a_b[q] * HqWq;
        a_i[q] = r / g.Wq;
        a_j[q] = r - a_i[q] * g.Wq;
    }
    const int c4 = tid & 7;

    int nk;
    if constexpr (MODE == 2) nk = (ntap * Ci + KT - 1) / KT;
    else nk = ntap * (Ci / KT);

    float4 ra[MODE == 2 || XH ? 1 : A_V], rb[MODE == 2 ? 1 : B_V];
    // fp16 X: the raw halves stay in registers until the LDS store (converting at the load would make the
    // prefetch of the next chunk wait for its data before this chunk's MFMAs)
    half4_t rah[XH ? A_V : 1];
    float sa[MODE == 2 ? A_V : 1], sb[MODE == 2 ? B_V : 1];
    static_assert(!XH || F16, "fp16 X is staged for the f16 MFMA");

    // vector path: raw buffer loads (out-of-range offset -> 0, no branches). The X resource starts at
    // the block's first image so 32-bit byte offsets suffice (host checks 3 images < 2 GB).
    const int b0 = m0 / HqWq;
    const long long img = (long long)g.Hi * g.Wi * g.ldx;
    const long long xrem = ((long long)g.B - b0) * img * XES;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(reinterpret_cast<const char*>(a.x) + (long long)b0 * img * XES), (short)0,
        (int)(xrem < 0x7FFFFFF0LL ? xrem : 0x7FFFFFF0LL), 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)a.w2, (short)0, a.w_bytes, 0x00020000);
    int a_base[A_V];  // element offset of image row 0 of this row's image, rel. to b0
#pragma unroll
    for (int q = 0; q < A_V; ++q) {
        a_base[q] = (int)((a_b[q] - b0) * img);
        a_i[q] *= g.ish;
        a_j[q] *= g.isw;
    }
    // tap offsets of this phase in LDS (uniform broadcast reads instead of indexed kernarg loads)
    __shared__ int2 tapoff[HYRES_MAX_TAPS];
    for (int i = tid; i < ntap; i += 256) tapoff[i] = make_int2(g.dh[tap0 + i], g.dw[tap0 + i]);
    __syncthreads();
    // (tap, channel) of the next chunk to load, advanced incrementally (no division per chunk)
    int ld_t = 0, ld_c = 0;

    // ---- load one K chunk into registers: the vector path (32 channels of one tap) or the MODE 2 scalar path
    auto load_chunk = [&](int kc) {
        if constexpr (MODE != 2) {
            const int2 o = tapoff[ld_t];
            const int c0 = ld_c + 4 * c4;
            const int gt = tap0 + ld_t;
#pragma unroll
            for (int q = 0; q < A_V; ++q) {
                const int ih = a_i[q] + o.x, iw = a_j[q] + o.y;
                const bool ok = a_ok[q] && (unsigned)ih < (unsigned)g.Hi && (unsigned)iw < (unsigned)g.Wi;
                const int off = ok ? (a_base[q] + (ih * g.Wi + iw) * g.ldx + c0) * XES : (int)0x80000000;
                if constexpr (XH) {
                    rah[q] = __builtin_bit_cast(half4_t, __builtin_amdgcn_raw_buffer_load_b64(xr, off, 0, 0));
                } else {
                    float4 v = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
                    if constexpr (MODE == 1) { v.x *= v.x; v.y *= v.y; v.z *= v.z; v.w *= v.w; }
                    ra[q] = v;
                }
            }
#pragma unroll
            for (int q = 0; q < B_V; ++q) {
                const int co = n0 + tid / 8 + 32 * q;
                const int off = co < g.Co ? (co * a.ldw + gt * Ci + c0) * 4 : (int)0x80000000;
                rb[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wr, off, 0, 0));
            }
            ld_c += KT;
            if (ld_c == Ci) { ld_c = 0; ++ld_t; }
        } else {
            // generic K = ntap*Ci (small Ci): a thread's k is the same for all its rows (256 % KT == 0),
            // so the (tap, channel) decode happens once per chunk; branch-free raw buffer loads
            const int K = ntap * Ci;
            const int k = kc * KT + (tid % KT);
            const bool kok = k < K;
            const int t = kok ? k / Ci : 0;
            const int ci = k - t * Ci;
            const int2 o = tapoff[t];
#pragma unroll
            for (int q = 0; q < A_V; ++q) {
                const int ih = a_i[q] + o.x, iw = a_j[q] + o.y;
                const bool okq = kok && a_ok[q] && (unsigned)ih < (unsigned)g.Hi && (unsigned)iw < (unsigned)g.Wi;
                const int off = okq ? (a_base[q] + (ih * g.Wi + iw) * g.ldx + ci) * 4 : (int)0x80000000;
                sa[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, off, 0, 0));
            }
#pragma unroll
            for (int q = 0; q < B_V; ++q) {
                const int co = n0 + (tid + 256 * q) / KT;
                const int off = (co < g.Co && kok) ? (co * a.ldw + tap0 * Ci + k) * 4 : (int)0x80000000;
                sb[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wr, off, 0, 0));
            }
        }
    };
    // ---- stage the loaded chunk to LDS in the MFMA flavour's operand format: A rows, then B rows
    auto store_chunk = [&](int buf = 0) {
        if constexpr (B6) {
            __bf16* const Pb = Pb0 + buf * 3 * PLANE;
            const int sx = b6p == 32 ? (((c4 >> 1) ^ ((tid >> 5) & 3)) << 3) + 4 * (c4 & 1) : 4 * c4;  // row bits 2..3 = tid bits 5..6
#pragma unroll
            for (int q = 0; q < A_V; ++q) bf6_put3(Pb, PLANE, (tid / 8 + 32 * q) * b6p + sx, ra[q]);
#pragma unroll
            for (int q = 0; q < B_V; ++q) bf6_put3(Pb, PLANE, (BM + tid / 8 + 32 * q) * b6p + sx, rb[q]);
        } else if constexpr (F16) {
#pragma unroll
            for (int q = 0; q < A_V; ++q) {
                half4_t h;
                if constexpr (XH && MODE == 1) {  // GDN norm: x^2 of the fp16 x, rounded for the MFMA
                    const half4_t r = rah[q];
                    h = f2h4(make_float4((float)r.x * (float)r.x, (float)r.y * (float)r.y, (float)r.z * (float)r.z,
                                         (float)r.w * (float)r.w));
                } else if constexpr (XH) {
                    h = rah[q];
                } else {
                    h = f2h4(ra[q]);
                }
                put_row_f16<PADH>(Ah, tid / 8 + 32 * q, c4, h);
            }
#pragma unroll
            for (int q = 0; q < B_V; ++q) put_row_f16<PADH>(Bh, tid / 8 + 32 * q, c4, f2h4(rb[q]));
        } else if constexpr (MODE != 2) {
#pragma unroll
            for (int q = 0; q < A_V; ++q) put_row_f32(As, tid / 8 + 32 * q, c4, ra[q]);
#pragma unroll
            for (int q = 0; q < B_V; ++q) put_row_f32(Bs, tid / 8 + 32 * q, c4, rb[q]);
        } else {
            // MODE 2: element e = tid + 256 q of an operand's chunk is k = e % KT of its row e / KT. Both loops written
            // out: as one function the 128x128 scalar-load kernels took 232-240 VGPRs instead of 216
#pragma unroll
            for (int q = 0; q < A_V; ++q) {
                int e = tid + 256 * q;
                As[(e / KT) * PADK + (e % KT)] = sa[q];
            }
#pragma unroll
            for (int q = 0; q < B_V; ++q) {
                int e = tid + 256 * q;
                Bs[(e / KT) * PADK + (e % KT)] = sb[q];
            }
        }
    };

    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int lr = lane & 31, lh = lane >> 5;

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int kbeg = SPLITK ? min(nk, split * a.cps) : 0;
    const int kend = SPLITK ? min(nk, kbeg + a.cps) : nk;
    if constexpr (MODE != 2) {
        const int cpt = Ci / KT;
        ld_t = kbeg / cpt;
        ld_c = (kbeg - ld_t * cpt) * KT;
    }
    // ---- compute one staged chunk: one lambda per MFMA flavour, its MFMA cluster at raised wave priority
    auto compute_f32 = [&] {
        if (a.prio) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float4 af[TM], bf[TN];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
                af[tm] = *reinterpret_cast<const float4*>(
                    &As[(wm * TM * 32 + tm * 32 + lr) * PADK + lh * 16 + 4 * u]);
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
                bf[tn] = *reinterpret_cast<const float4*>(
                    &Bs[(wn * TN * 32 + tn * 32 + lr) * PADK + lh * 16 + 4 * u]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn) {
                        float av = e == 0 ? af[tm].x : e == 1 ? af[tm].y : e == 2 ? af[tm].z : af[tm].w;
                        float bv = e == 0 ? bf[tn].x : e == 1 ? bf[tn].y : e == 2 ? bf[tn].z : bf[tn].w;
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[tm][tn], 0, 0, 0);
                    }
        }
        if (a.prio) __builtin_amdgcn_s_setprio(0);
    };
    auto compute_f16 = [&] {
        typedef _Float16 half8 __attribute__((ext_vector_type(8)));
        if (a.prio) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s16 = 0; s16 < 2; ++s16) {
            half8 af[TM], bf[TN];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
                af[tm] = *reinterpret_cast<const half8*>(
                    &Ah[(wm * TM * 32 + tm * 32 + lr) * PADH + 16 * s16 + 8 * lh]);
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
                bf[tn] = *reinterpret_cast<const half8*>(
                    &Bh[(wn * TN * 32 + tn * 32 + lr) * PADH + 16 * s16 + 8 * lh]);
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[tm], bf[tn], acc[tm][tn], 0, 0, 0);
        }
        if (a.prio) __builtin_amdgcn_s_setprio(0);
    };
    auto compute_b6 = [&](int buf) {
        const __bf16* const Pb = Pb0 + buf * 3 * PLANE;
        if (a.prio) __builtin_amdgcn_s_setprio(1);
        const int rx = b6p == 32 ? (lr >> 2) & 3 : 0;  // the row's slot swizzle (tile bases are multiples of 32 rows)
#pragma unroll
        for (int s16 = 0; s16 < 2; ++s16) {
            bf16x8_t af[TM][3], bf[TN][3];
            const int ko = ((2 * s16 + lh) ^ rx) << 3;
#pragma unroll
            for (int p = 0; p < 3; ++p) {
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
                    af[tm][p] = *reinterpret_cast<const bf16x8_t*>(
                        &Pb[p * PLANE + (wm * TM * 32 + tm * 32 + lr) * b6p + ko]);
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    bf[tn][p] = *reinterpret_cast<const bf16x8_t*>(
                        &Pb[p * PLANE + (BM + wn * TN * 32 + tn * 32 + lr) * b6p + ko]);
            }
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = bf6_mfma(af[tm], bf[tn], acc[tm][tn]);
        }
        if (a.prio) __builtin_amdgcn_s_setprio(0);
    };
    auto compute_chunk = [&](int buf = 0) {
        if constexpr (B6) compute_b6(buf);
        else if constexpr (F16) compute_f16();
        else compute_f32();
    };

    // ---- the K loop over this block's chunks [kbeg, kend)
    if constexpr (DB) {
        if (kbeg < kend) {
            load_chunk(kbeg);
            store_chunk(0);
        }
        __syncthreads();
        int cur = 0;
        for (int kc = kbeg; kc < kend; ++kc) {
            const bool nxt = kc + 1 < kend;  // block-uniform
            if (nxt) load_chunk(kc + 1);
            compute_chunk(cur);
            if (nxt) store_chunk(cur ^ 1);
            __syncthreads();
            cur ^= 1;
        }
    } else {
        if (kbeg < kend) load_chunk(kbeg);
        for (int kc = kbeg; kc < kend; ++kc) {
            __syncthreads();
            store_chunk();
            __syncthreads();
            if (kc + 1 < kend) load_chunk(kc + 1);
            compute_chunk();
        }
    }

    // ---- epilogue: stage the accumulators through LDS one TN column slice at a time (static register
    // indices), then apply the epilogue row-major: consecutive threads cover consecutive channels of
    // one NHWC pixel row (float4 when every operand is 16B aligned), each row decoded once.
    constexpr int CW = 32 * WAVES_N, CP = CW + 8;  // +8: the two lane halves hit disjoint banks
    float* Cs = smem;
    constexpr bool split_k = SPLITK;
    float* slab = split_k ? a.slab + ((long long)(split * g.nphase + phase) * a.M) * g.Co : nullptr;
    const bool linear = g.nphase == 1 && g.osh == 1 && g.osw == 1 && g.Ho == g.Hq && g.Wo == g.Wq;
    const int oph = g.oph[phase], opw = g.opw[phase];
    const float slope = (a.e.act == HYRES_ACT_PRELU) ? a.e.slope[0] : 0.f;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        __syncthreads();
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                Cs[(wm * TM * 32 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * CP + wn * 32 + lr] = acc[tm][tn][r];
        __syncthreads();
        if constexpr (!split_k) {
            // fast path (BIAS epilogue, float4 operands): the bias / residual / old-y / ReLU-mask loads of U
            // iterations are issued before any of them is consumed. Per-lane validity goes into the buffer offset
            // (out of range -> 0, no divergent branch: a load behind one is waited on where the branches join);
            // an absent operand is skipped by a uniform branch around all U of its loads
            if (a.vec4 && a.rsrc_ok && a.e.kind == HYRES_EPI_BIAS) {
                constexpr int ITER = BM * (CW / 4) / 256;
                constexpr int U = ITER >= 4 ? 4 : ITER;
                static_assert(ITER % U == 0, "epilogue tiling");
                const hyres_epilogue& e = a.e;
                constexpr int ES = YH ? 2 : 4;  // residual / fp16-storage element bytes
                const long long npo = (long long)g.B * g.Ho * g.Wo;
                const bool mask = e.act == HYRES_ACT_RELU_MASK;
                const bool m16 = YH || (e.io_f16 & HYRES_IO_AUX16);
                const __amdgpu_buffer_rsrc_t r_bias = opnd_rsrc(e.bias, (long long)g.Co * 4);
                const __amdgpu_buffer_rsrc_t r_res = opnd_rsrc(e.res, npo * e.ldres * ES);
                const __amdgpu_buffer_rsrc_t r_m32 = opnd_rsrc(mask && !m16 ? e.aux0 : nullptr, npo * e.ld0 * 4);
                const __amdgpu_buffer_rsrc_t r_m16 = opnd_rsrc(mask && m16 ? e.aux0 : nullptr, npo * e.ld0 * 2);
                const __amdgpu_buffer_rsrc_t r_old = opnd_rsrc(e.accumulate ? a.y : nullptr, npo * g.ldy * ES);
                constexpr int OOR = (int)0x80000000;
                for (int it0 = 0; it0 < ITER; it0 += U) {
                    float4 v[U], yo[U], mk[U], bs[U];
                    std::conditional_t<YH, half4_t, float4> rs[U];
                    half4_t mh[U];
                    long long px[U];
                    int nn[U];
                    bool ok[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int idx = tid + 256 * (it0 + u);
                        const int row = idx / (CW / 4);
                        const int col = 4 * (idx - row * (CW / 4));
                        const int m = m0 + row;
                        const int n = n0 + (col >> 5) * TN * 32 + tn * 32 + (col & 31);
                        ok[u] = m < a.M && n < g.Co;
                        nn[u] = n;
                        v[u] = *reinterpret_cast<const float4*>(&Cs[row * CP + col]);
                        long long pix = m;
                        if (!linear) pix = conv_out_pixel(g, HqWq, oph, opw, m);
                        px[u] = pix;
                    }
                    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int u = 0; u < U; ++u) { bs[u] = z4; yo[u] = z4; mk[u] = z4; }
                    if (e.bias) {
#pragma unroll
                        for (int u = 0; u < U; ++u) bs[u] = bload4(r_bias, ok[u] ? nn[u] * 4 : OOR);
                    }
                    if (e.res) {
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const int orr = ok[u] ? (int)((px[u] * e.ldres + nn[u]) * ES) : OOR;
                            if constexpr (YH) rs[u] = bload4h(r_res, orr);
                            else rs[u] = bload4(r_res, orr);
                        }
                    } else {
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            if constexpr (YH) rs[u] = half4_t{(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
                            else rs[u] = z4;
                        }
                    }
                    if (e.accumulate) {  // YH: fp16 gradient accumulation (AMP)
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const int oo = ok[u] ? (int)((px[u] * g.ldy + nn[u]) * ES) : OOR;
                            if constexpr (YH) yo[u] = h2f4(bload4h(r_old, oo));
                            else yo[u] = bload4(r_old, oo);
                        }
                    }
                    if (mask && m16) {
#pragma unroll
                        for (int u = 0; u < U; ++u) mh[u] = bload4h(r_m16, ok[u] ? (int)((px[u] * e.ld0 + nn[u]) * 2) : OOR);
                    } else if (mask) {
#pragma unroll
                        for (int u = 0; u < U; ++u) mk[u] = bload4(r_m32, ok[u] ? (int)((px[u] * e.ld0 + nn[u]) * 4) : OOR);
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (!ok[u]) continue;
                        float4 r4;
                        if constexpr (YH) r4 = h2f4(rs[u]);
                        else r4 = rs[u];
                        float o[4] = {v[u].x + bs[u].x + r4.x, v[u].y + bs[u].y + r4.y,
                                      v[u].z + bs[u].z + r4.z, v[u].w + bs[u].w + r4.w};
                        if (e.out2) stv4<YH>(e.out2, px[u] * e.ldo2 + nn[u], make_float4(o[0], o[1], o[2], o[3]));
                        if (e.act == HYRES_ACT_RELU) {
#pragma unroll
                            for (int c = 0; c < 4; ++c) o[c] = fmaxf(o[c], 0.f);
                        } else if (e.act == HYRES_ACT_PRELU) {
#pragma unroll
                            for (int c = 0; c < 4; ++c) o[c] = o[c] >= 0.f ? o[c] : slope * o[c];
                        } else if (mask) {
                            const float4 q = m16 ? h2f4(mh[u]) : mk[u];
                            o[0] = q.x > 0.f ? o[0] : 0.f;
                            o[1] = q.y > 0.f ? o[1] : 0.f;
                            o[2] = q.z > 0.f ? o[2] : 0.f;
                            o[3] = q.w > 0.f ? o[3] : 0.f;
                        }
                        stv4<YH>(a.y, px[u] * g.ldy + nn[u],
                                 make_float4(o[0] + yo[u].x, o[1] + yo[u].y, o[2] + yo[u].z, o[3] + yo[u].w));
                    }
                }
                continue;
            }
        }
        for (int idx = tid; idx < BM * (CW / 4); idx += 256) {
            const int row = idx / (CW / 4);
            const int col = 4 * (idx - row * (CW / 4));
            const int m = m0 + row;
            const int n = n0 + (col >> 5) * TN * 32 + tn * 32 + (col & 31);
            if (m >= a.M || n >= g.Co) continue;
            const float4 v = *reinterpret_cast<const float4*>(&Cs[row * CP + col]);
            if constexpr (split_k) {
                float* sp = slab + (long long)m * g.Co + n;
                if (a.vec4) {
                    *reinterpret_cast<float4*>(sp) = v;
                } else {
                    sp[0] = v.x;
                    if (n + 1 < g.Co) sp[1] = v.y;
                    if (n + 2 < g.Co) sp[2] = v.z;
                    if (n + 3 < g.Co) sp[3] = v.w;
                }
                continue;
            }
            long long pix = m;
            if (!linear) pix = conv_out_pixel(g, HqWq, oph, opw, m);
            if (a.vec4) {
                epi_store4<YH, true>(a.e, a.y, g.ldy, pix, n, v, slope);
            } else {
                const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (n + c < g.Co) epi_store<YH, true>(a.e, a.y, g.ldy, pix, n + c, vv[c], epi_channel(a.e, n + c));
            }
        }
    }
}

// waves per SIMD the register allocation must allow: 4 (<= 128 VGPRs: 4 blocks per CU) for the vector-load tiles with
// at most two accumulator tiles per wave — left to itself the compiler gave the 64x128 / 128x64 tiles 144 registers
// (3 blocks per CU); with the bound they fit in 109-127 with no spill — and 3 (<= 168) for the 128x128 tiles (176-212
// -> 142-154, 3 blocks per CU instead of 2; AMP step -0.5 %, fp32 neutral: profiles/r3aa_conv_wpe3_ab.txt). The
// scalar-load path (MODE 2, the 3-channel image side) would spill: the compiler's choice there. -DHYRES_CONV_WPE4=0
// builds the unbounded variant (A/B).
#ifndef HYRES_CONV_WPE4
#define HYRES_CONV_WPE4 1
#endif
template <int TM, int TN, int MODE>
constexpr int conv_wpe() { return (HYRES_CONV_WPE4 && MODE != 2) ? (TM * TN <= 2 ? 4 : 3) : 1; }

template <int TM, int TN, int WAVES_M, int WAVES_N, int MODE, bool SPLITK, bool F16 = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(conv_wpe<TM, TN, MODE>())))
void conv_fwd_kernel(const ConvArgs a) {
    conv_fwd_body<TM, TN, WAVES_M, WAVES_N, MODE, SPLITK, F16, 0>(a);
}

// fp32 operands, bf16x6 products (hyres_conv_tuning key 7): the compiler's register allocation (the three-plane
// fragments do not fit the 4-waves-per-SIMD bound of conv_fwd_kernel)
template <int TM, int TN, int WAVES_M, int WAVES_N, int MODE, bool SPLITK>
__global__ __launch_bounds__(256) void conv_fwd_b6_kernel(const ConvArgs a) {
    conv_fwd_body<TM, TN, WAVES_M, WAVES_N, MODE, SPLITK, false, 0, true>(a);
}
// the same with double-buffered staging (conv_fwd_body DB; round 6, the 64x64 tile only: hyres_conv_tuning key 20)
template <int TM, int TN, int WAVES_M, int WAVES_N, int MODE, bool SPLITK>
__global__ __launch_bounds__(256) void conv_fwd_b6db_kernel(const ConvArgs a) {
    conv_fwd_body<TM, TN, WAVES_M, WAVES_N, MODE, SPLITK, false, 0, true, true>(a);
}

// fp16 activations in HBM (IO = 1: X fp16, 2: Y fp16, 3: both); fp16 MFMA operands except on the
// small-Ci scalar path (MODE 2: the fp32 image in, fp16 features out)
template <int TM, int TN, int WAVES_M, int WAVES_N, int MODE, bool SPLITK, int IO>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(conv_wpe<TM, TN, MODE>())))
void conv_fwd_h_kernel(const ConvArgs a) {
    conv_fwd_body<TM, TN, WAVES_M, WAVES_N, MODE, SPLITK, MODE != 2, IO>(a);
}

// split-K reduction + epilogue: one thread per (phase, m, n)
template <bool H>
__global__ void conv_splitk_reduce_kernel(const ConvArgs a) {
    const hyres_conv_geom& g = a.g;
    const long long per_phase = (long long)a.M * g.Co;
    const long long total = per_phase * g.nphase;
    const int HqWq = g.Hq * g.Wq;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int phase = (int)(idx / per_phase);
        const long long r = idx - phase * per_phase;
        const int m = (int)(r / g.Co);
        const int n = (int)(r - (long long)m * g.Co);
        float v = 0.f;
        for (int s = 0; s < a.nsplit; ++s) v += a.slab[((long long)(s * g.nphase + phase) * a.M + m) * g.Co + n];
        const long long pix = conv_out_pixel(g, HqWq, g.oph[phase], g.opw[phase], m);
        epi_store<H, true>(a.e, a.y, g.ldy, pix, n, v, epi_channel(a.e, n));
    }
}

// float4 variant (vec4 launches): 4 channels per thread, split loads unrolled, float4 epilogue
template <bool H>
__global__ __launch_bounds__(256) void conv_splitk_reduce4_kernel(const ConvArgs a) {
    const hyres_conv_geom& g = a.g;
    const int C4 = g.Co >> 2;
    const long long per_phase = (long long)a.M * C4;
    const long long total = per_phase * g.nphase;
    const long long sstride = (long long)g.nphase * a.M * g.Co;
    const int HqWq = g.Hq * g.Wq;
    const float slope = (a.e.act == HYRES_ACT_PRELU) ? a.e.slope[0] : 0.f;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int phase = (int)(idx / per_phase);
        const long long r = idx - phase * per_phase;
        const int m = (int)(r / C4);
        const int n = 4 * (int)(r - (long long)m * C4);
        const float* sp = a.slab + ((long long)phase * a.M + m) * g.Co + n;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
        for (int s = 0; s < a.nsplit; ++s) {
            const float4 u = ld4(sp + s * sstride);
            v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
        }
        const long long pix = conv_out_pixel(g, HqWq, g.oph[phase], g.opw[phase], m);
        epi_store4<H, true>(a.e, a.y, g.ldy, pix, n, v, slope);
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// the implicit GEMM on one tile; split-K launches are a separate instantiation (partials to the slab, no epilogue)
template <int TM, int TN, int WM_, int WN_>
static int launch_fwd(const ConvArgs& a, int mode, ConvGemm gemm, hipStream_t st) {
    constexpr int BM = 32 * TM * WM_, BN = 32 * TN * WN_;
    dim3 grid(ceil_div(a.M, BM), ceil_div(a.g.Co, BN), a.g.nphase * a.nsplit);
    if (a.xcd) grid = dim3(grid.x * grid.y, 1, grid.z);
    // KERNEL<tile, MODE_, split, trailing template arguments>
#define HY_TILES(KERNEL, MODE_, ...)                                                                                   \
    do {                                                                                                               \
        if (a.nsplit > 1)                                                                                              \
            hipLaunchKernelGGL((KERNEL<TM, TN, WM_, WN_, MODE_, true __VA_ARGS__>), grid, dim3(256), 0, st, a);        \
        else                                                                                                           \
            hipLaunchKernelGGL((KERNEL<TM, TN, WM_, WN_, MODE_, false __VA_ARGS__>), grid, dim3(256), 0, st, a);       \
    } while (0)
#define HY_TILES_01(KERNEL, ...)                              \
    do {                                                      \
        if (mode == 0) HY_TILES(KERNEL, 0, __VA_ARGS__);      \
        else HY_TILES(KERNEL, 1, __VA_ARGS__);                \
    } while (0)
    switch (gemm) {
        case ConvGemm::H:
            if (mode == 2) HY_TILES(conv_fwd_h_kernel, 2, , 2);
            else if ((a.e.io_f16 & 3) == 1) HY_TILES_01(conv_fwd_h_kernel, , 1);
            else if ((a.e.io_f16 & 3) == 2) HY_TILES_01(conv_fwd_h_kernel, , 2);
            else HY_TILES_01(conv_fwd_h_kernel, , 3);
            return HY_LAUNCH_CHECK("conv_fwd_h_kernel");
        case ConvGemm::F16:
            HY_TILES_01(conv_fwd_kernel, , true);
            return HY_LAUNCH_CHECK("conv_fwd_kernel(f16)");
        case ConvGemm::B6DB:
            if constexpr (TM == 1 && TN == 1 && WM_ == 2 && WN_ == 2) {  // choose_gemm: tile 4 only
                HY_TILES_01(conv_fwd_b6db_kernel, );
                return HY_LAUNCH_CHECK("conv_fwd_b6db_kernel");
            }
            [[fallthrough]];
        case ConvGemm::B6:
            HY_TILES_01(conv_fwd_b6_kernel, );
            return HY_LAUNCH_CHECK("conv_fwd_b6_kernel");
        case ConvGemm::F32: break;
    }
    if (mode == 2) HY_TILES(conv_fwd_kernel, 2, );
    else HY_TILES_01(conv_fwd_kernel, );
#undef HY_TILES_01
#undef HY_TILES
    return HY_LAUNCH_CHECK("conv_fwd_kernel");
}

int launch_tiles(const ConvArgs& a, int tile, int mode, ConvGemm gemm, hipStream_t st) {
    int rc;
    switch (tile) {
        case 0: rc = launch_fwd<2, 2, 2, 2>(a, mode, gemm, st); break;
        case 1: rc = launch_fwd<2, 1, 2, 2>(a, mode, gemm, st); break;
        case 3: rc = launch_fwd<1, 2, 2, 2>(a, mode, gemm, st); break;
        case 4: rc = launch_fwd<1, 1, 2, 2>(a, mode, gemm, st); break;
        default: rc = launch_fwd<1, 1, 4, 1>(a, mode, gemm, st); break;
    }
    if (rc || a.nsplit == 1) return rc;
    const long long total = (long long)a.M * a.g.Co * a.g.nphase;
    const bool yh = (a.e.io_f16 & 2) != 0;
    if (a.vec4) {
        const dim3 grid((int)std::min<long long>((total / 4 + 255) / 256, 8192));
        if (yh) hipLaunchKernelGGL(conv_splitk_reduce4_kernel<true>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(conv_splitk_reduce4_kernel<false>, grid, dim3(256), 0, st, a);
        return HY_LAUNCH_CHECK("conv_splitk_reduce4_kernel");
    }
    const dim3 grid((int)std::min<long long>((total + 255) / 256, 8192));
    if (yh) hipLaunchKernelGGL(conv_splitk_reduce_kernel<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(conv_splitk_reduce_kernel<false>, grid, dim3(256), 0, st, a);
    return HY_LAUNCH_CHECK("conv_splitk_reduce_kernel");
}

}  // namespace hyres
