// Internal declarations shared by the convolution (conv.hip, conv_gemm.hip through conv_epilogue.h, conv_stream.hip
// through stream_common.h, ru_fused.hip through halo_common.h) and weight-gradient (wgrad.hip) units.
#pragma once
#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

namespace hyres {

constexpr int KT = 32;  // K chunk (floats)

// tile / split-K overrides set through hyres_conv_tuning (conv.hip; -1 = the planners' heuristics)
extern int g_tune[HYRES_TUNE_KEYS];

// fp32 GEMMs on the bf16 MFMA (hyres_conv_tuning key 7 = 1, the default): "bf16x6"
inline bool f32_gemm_bf6() { return g_tune[7] == 1; }

// compute units of the current device (256 on an MI355X, and 256 without a device: the host-only queries)
inline int num_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                     hipSuccess || n < 1)
            n = 256;
        cus = n;
    }
    return cus;
}

// Buffer resource of an epilogue operand: an absent operand (p == NULL) gets an empty resource, so its loads return
// 0 without a branch (a load behind a branch is waited on at the join: the epilogue's loads would serialise)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t opnd_rsrc(const void* p, long long bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, (short)0, p ? (int)std::min<long long>(bytes, 0x7FFFFFF0LL) : 0,
                                             0x00020000);
}
__device__ __forceinline__ float4 bload4(__amdgpu_buffer_rsrc_t r, int off) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ half4_t bload4h(__amdgpu_buffer_rsrc_t r, int off) {
    return __builtin_bit_cast(half4_t, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
}
__device__ __forceinline__ float4 h2f4(half4_t h) { return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w); }

typedef _Float16 halfx4_t __attribute__((ext_vector_type(4)));
typedef _Float16 halfx8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));

// fp32 -> three bf16 pieces h + m + l (24 significant bits, remainder <= 2^-25 |x|): the bf16x6 fp32 GEMM's operands
__device__ __forceinline__ void bf6_split4(float4 v, bf16x4_t& h, bf16x4_t& m, bf16x4_t& l) {
    const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const __bf16 a = (__bf16)x[i];
        const float r1 = x[i] - (float)a;
        const __bf16 b = (__bf16)r1;
        h[i] = a;
        m[i] = b;
        l[i] = (__bf16)(r1 - (float)b);
    }
}

// acc += a * b to fp32 accuracy from the three-piece operands: the six cross products with i + j <= 2, the
// smallest first
__device__ __forceinline__ floatx16 bf6_mfma(const bf16x8_t (&a)[3], const bf16x8_t (&b)[3], floatx16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
}

// bf16x6 staging: four fp32 channels split into their three bf16 pieces, one piece per plane (`plane` apart)
__device__ __forceinline__ void bf6_put3(__bf16* base, int plane, int o, const float4& v) {
    bf16x4_t h, m, l;
    bf6_split4(v, h, m, l);
    *reinterpret_cast<bf16x4_t*>(&base[o]) = h;
    *reinterpret_cast<bf16x4_t*>(&base[plane + o]) = m;
    *reinterpret_cast<bf16x4_t*>(&base[2 * plane + o]) = l;
}
template <int PLANE>
__device__ __forceinline__ void bf6_put3(__bf16* base, int o, const float4& v) { bf6_put3(base, PLANE, o, v); }

// XCD-aware block order: hardware block hw runs on XCD hw % 8, so XCD x gets the contiguous logical range
// [x*q + min(x, r), ...) of the nb = 8q + r blocks (a bijection for any nb)
__device__ __forceinline__ int xcd_logical_block() {
    const int nb = gridDim.x, hw = blockIdx.x;
    const int q = nb >> 3, r = nb & 7, x = hw & 7;
    return x * q + min(x, r) + (hw >> 3);
}

// ---- the forward convolution kernels' argument block (conv.hip, conv_gemm.hip, conv_stream.hip)
struct ConvArgs {
    hyres_conv_geom g;
    const float* x;
    const float* w2;
    int ldw;
    float* y;
    hyres_epilogue e;
    int M;       // B*Hq*Wq
    int nsplit;  // split-K factor (1 = fused epilogue)
    int cps;     // K chunks per split
    float* slab; // [nsplit][nphase][M][Co] partials when nsplit > 1
    int vec4;    // every epilogue operand 16B aligned with ld % 4 == 0 and Co % 4 == 0
    int w_bytes; // bytes of W2 (buffer-resource range)
    int xcd;     // 1: grid.x = M tiles x N tiles in XCD-aware order (grid.y = 1)
    int prio;    // 1: raise the wave priority while it issues its MFMA cluster (s_setprio)
    int x_bytes; // conv1x1_stream_kernel: bytes of X (buffer-resource range)
    int rsrc_ok; // every epilogue operand / output spans < 2 GB: the epilogues may address them by buffer resources
    int b6sw;    // bf16x6 implicit GEMM: 64-B LDS rows with the 16-B slot XOR-swizzled by row bits 2..3 (round 6,
                 // hyres_conv_tuning key 19, default 1) instead of 80-B padded rows
};

// a streaming kernel's instantiation as route() carries it: NT, KC or KS, the epilogue-operand bits F
inline int pack_cfg(int nt, int k, int f) { return nt | (k << 4) | (f << 12); }
inline int cfg_nt(int cfg) { return cfg & 15; }
inline int cfg_k(int cfg) { return (cfg >> 4) & 255; }
inline int cfg_f(int cfg) { return cfg >> 12; }

inline long long gemm_rows(const hyres_conv_geom* g) { return (long long)g->B * g->Hq * g->Wq; }

// single-tap, stride-1, same-size 1x1: the streaming kernels' geometry
inline bool pointwise_same_size(const hyres_conv_geom* g) {
    return g->nphase == 1 && g->ntaps == 1 && g->ish == 1 && g->isw == 1 && g->dh[0] == 0 && g->dw[0] == 0 &&
           g->Hi == g->Hq && g->Wi == g->Wq && g->Ho == g->Hq && g->Wo == g->Wq;
}

// ---- the streaming 1x1 family (conv_stream.hip) as route() and hyres_conv_forward (conv.hip) see it: eligibility
// (pack_cfg(NT, KC or KS, F), or 0) and launch of the instantiation a cfg names
int stream_cfg(const hyres_conv_geom* g, const hyres_epilogue* e);
int stream_h_cfg(const hyres_conv_geom* g, const hyres_epilogue* e);
int stream_hf_cfg(const hyres_conv_geom* g, const hyres_epilogue* e);
int stream_b6_cfg(const hyres_conv_geom* g, const hyres_epilogue* e);
bool stream_b6_ce();
int launch_stream(const ConvArgs& a, int cfg, hipStream_t st);
int launch_stream_h(const ConvArgs& a, int cfg, hipStream_t st);
int launch_stream_hf(const ConvArgs& a, int cfg, hipStream_t st);
int launch_stream_b6(const ConvArgs& a, int cfg, hipStream_t st);

// ---- the implicit-GEMM family (conv_gemm.hip) as route() and hyres_conv_forward (conv.hip) see it: the kernel of
// the tiles — fp16 X / Y, f16 operands, bf16x6 (double-buffered or not), fp32 MFMA / scalar loads — and the launch of
// tile `tile` (the index of TILE_BM / TILE_BN) in load mode `mode` on it, with the split-K reduce when a.nsplit > 1
enum class ConvGemm { H, F16, B6DB, B6, F32 };
int launch_tiles(const ConvArgs& a, int tile, int mode, ConvGemm gemm, hipStream_t st);

}  // namespace hyres
