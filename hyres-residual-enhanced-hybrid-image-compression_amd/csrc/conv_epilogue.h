// The convolution kernels' generic epilogue: epi_store / epi_store4 apply a hyres_epilogue to one GEMM result (or four
// consecutive channels of it) and store it; conv_out_pixel maps a GEMM row to its NHWC output pixel. Used by the
// implicit-GEMM family (conv_gemm.hip) and by the halo-tiled and narrow kernels (conv.hip).
#pragma once
#include "conv_common.h"

namespace hyres {

// ConvArgs, opnd_rsrc, bload4 / bload4h (buffer resources of the epilogue operands), h2f4, st4: conv_common.h

// Output pixel of GEMM row m of one phase: m = (b * Hq + i) * Wq + j (HqWq = Hq * Wq) computes pixel
// (b, i * osh + oph, j * osw + opw)
__device__ __forceinline__ long long conv_out_pixel(const hyres_conv_geom& g, int HqWq, int oph, int opw, int m) {
    const int b = m / HqWq;
    const int rr = m - b * HqWq;
    const int i = rr / g.Wq;
    const int j = rr - i * g.Wq;
    return (long long)(b * g.Ho + i * g.osh + oph) * g.Wo + j * g.osw + opw;
}

struct EpiChannel {
    float bias, slope;
};

__device__ __forceinline__ EpiChannel epi_channel(const hyres_epilogue& e, int n) {
    EpiChannel c;
    c.bias = e.bias ? e.bias[n] : 0.f;
    c.slope = (e.act == HYRES_ACT_PRELU) ? e.slope[0] : 0.f;
    return c;
}

// Saved-activation operand of a backward epilogue (the ReLU mask's y, GDN-backward's x and norm): fp16 when
// the whole epilogue is fp16 (H) or, with fp32 X/Y, when io_f16 carries HYRES_IO_AUX16 (AMP training keeps
// its activations fp16 and its gradients fp32). A uniform kernel-argument branch.
template <bool H>
__device__ __forceinline__ float ld_aux(const hyres_epilogue& e, const float* p, long long i) {
    if constexpr (H) return ldv<true>(p, i);
    else return (e.io_f16 & HYRES_IO_AUX16) ? ldv<true>(p, i) : p[i];
}
template <bool H>
__device__ __forceinline__ float4 ld_aux4(const hyres_epilogue& e, const float* p, long long i) {
    if constexpr (H) return ldv4<true>(p, i);
    else return (e.io_f16 & HYRES_IO_AUX16) ? ldv4<true>(p, i) : ld4(p + i);
}

// Apply the epilogue to one GEMM result v for output pixel ``pix`` / channel n and store it
// (H: y and the activation operands res / aux0 / out2 are fp16 in HBM).
// SAB: the HYRES_EPI_SA_BWD case compiled in (only conv_fwd_body, the one kernel family the launcher routes that
// epilogue to: every other caller keeps its register allocation — the case cost the weight-resident f16 kernels a spill)
template <bool H = false, bool SAB = false>
__device__ __forceinline__ void epi_store(const hyres_epilogue& e, float* y, int ldy, long long pix, int n, float v,
                                          const EpiChannel& c) {
    switch (e.kind) {
        case HYRES_EPI_ROWSCALE:  // the product scaled per output pixel first (aux1[pix * ld1]), then as BIAS
            v *= e.aux1[pix * e.ld1];
            [[fallthrough]];
        case HYRES_EPI_BIAS: {
            v += c.bias;
            if (e.res) v += ldv<H>(e.res, pix * e.ldres + n);
            if (e.out2) stv<H>(e.out2, pix * e.ldo2 + n, v);  // pre-activation (PReLU backward)
            if (e.act == HYRES_ACT_RELU) v = fmaxf(v, 0.f);
            else if (e.act == HYRES_ACT_PRELU) v = v >= 0.f ? v : c.slope * v;
            else if (e.act == HYRES_ACT_RELU_MASK) v = ld_aux<H>(e, e.aux0, pix * e.ld0 + n) > 0.f ? v : 0.f;
            break;
        }
        case HYRES_EPI_GDN:
        case HYRES_EPI_IGDN: {
            const float nv = v + c.bias;
            const float xv = ldv<H>(e.aux0, pix * e.ld0 + n);
            stv<H>(e.out2, pix * e.ldo2 + n, nv);
            v = (e.kind == HYRES_EPI_GDN) ? xv * (1.0f / sqrtf(nv)) : xv * sqrtf(nv);
            break;
        }
        case HYRES_EPI_SA_BWD: {  // SpatialAttention's mean / max backward: + d mean / C, + d max at the argmax
            if constexpr (SAB) {
                const float* gm = e.aux0 + pix * e.ld0;
                v = v + gm[0] + (n == reinterpret_cast<const int*>(e.aux2)[pix] ? gm[1] : 0.f);
            }
            break;
        }
        case HYRES_EPI_GDN_BWD:
        case HYRES_EPI_IGDN_BWD: {  // H (AMP fp16 gradients): x, the incoming gradient and the norm all fp16
            const float xv = ld_aux<H>(e, e.aux0, pix * e.ld0 + n);
            const float gv = ldv<H>(e.aux1, pix * e.ld1 + n);
            const float nv = ld_aux<H>(e, e.aux2, pix * e.ld2 + n);
            const float f = (e.kind == HYRES_EPI_GDN_BWD) ? (1.0f / sqrtf(nv)) : sqrtf(nv);
            v = 2.0f * xv * v + gv * f;
            break;
        }
        default: break;
    }
    if constexpr (H) {
        if (e.accumulate) v += ldv<true>(y, pix * ldy + n);  // fp16 gradient accumulation (AMP): fp32 add
        stv<true>(y, pix * ldy + n, v);
    } else {
        float* yp = y + pix * ldy + n;
        if (e.accumulate) v += *yp;
        *yp = v;
    }
}

// float4 variant of epi_store for channels n..n+3 (all operands 16B aligned).
template <bool H = false, bool SAB = false>
__device__ __forceinline__ void epi_store4(const hyres_epilogue& e, float* y, int ldy, long long pix, int n, float4 v,
                                           float slope, bool use_pre = false,
                                           float4 rpre = make_float4(0.f, 0.f, 0.f, 0.f)) {
    float o[4] = {v.x, v.y, v.z, v.w};
    switch (e.kind) {
        case HYRES_EPI_ROWSCALE: {
            const float sc = e.aux1[pix * e.ld1];
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] *= sc;
        }
            [[fallthrough]];
        case HYRES_EPI_BIAS: {
            if (e.bias) { const float4 b = ld4(e.bias + n); o[0] += b.x; o[1] += b.y; o[2] += b.z; o[3] += b.w; }
            if (e.res) {  // rpre: the residual already loaded by the caller (same value, same order; passed by value:
                          // a pointer into the caller's register array put that array in scratch memory)
                const float4 r = use_pre ? rpre : ldv4<H>(e.res, pix * e.ldres + n);
                o[0] += r.x; o[1] += r.y; o[2] += r.z; o[3] += r.w;
            }
            if (e.out2) stv4<H>(e.out2, pix * e.ldo2 + n, make_float4(o[0], o[1], o[2], o[3]));
            if (e.act == HYRES_ACT_RELU) {
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c] = fmaxf(o[c], 0.f);
            } else if (e.act == HYRES_ACT_PRELU) {
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c] = o[c] >= 0.f ? o[c] : slope * o[c];
            } else if (e.act == HYRES_ACT_RELU_MASK) {
                const float4 y = ld_aux4<H>(e, e.aux0, pix * e.ld0 + n);
                o[0] = y.x > 0.f ? o[0] : 0.f;
                o[1] = y.y > 0.f ? o[1] : 0.f;
                o[2] = y.z > 0.f ? o[2] : 0.f;
                o[3] = y.w > 0.f ? o[3] : 0.f;
            }
            break;
        }
        case HYRES_EPI_GDN:
        case HYRES_EPI_IGDN: {
            const float4 b = e.bias ? ld4(e.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 x = ldv4<H>(e.aux0, pix * e.ld0 + n);
            const float nv[4] = {o[0] + b.x, o[1] + b.y, o[2] + b.z, o[3] + b.w};
            const float xv[4] = {x.x, x.y, x.z, x.w};
            stv4<H>(e.out2, pix * e.ldo2 + n, make_float4(nv[0], nv[1], nv[2], nv[3]));
#pragma unroll
            for (int c = 0; c < 4; ++c)
                o[c] = (e.kind == HYRES_EPI_GDN) ? xv[c] * (1.0f / sqrtf(nv[c])) : xv[c] * sqrtf(nv[c]);
            break;
        }
        case HYRES_EPI_SA_BWD: {  // as in epi_store: (acc + d mean / C) + (channel == argmax ? d max : 0)
            if constexpr (SAB) {
                const float* gm = e.aux0 + pix * e.ld0;
                const float ga = gm[0], gx = gm[1];
                const int mi = reinterpret_cast<const int*>(e.aux2)[pix];
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c] = o[c] + ga + (n + c == mi ? gx : 0.f);
            }
            break;
        }
        case HYRES_EPI_GDN_BWD:
        case HYRES_EPI_IGDN_BWD: {
            const float4 x = ld_aux4<H>(e, e.aux0, pix * e.ld0 + n);
            const float4 gg = ldv4<H>(e.aux1, pix * e.ld1 + n);
            const float4 nn = ld_aux4<H>(e, e.aux2, pix * e.ld2 + n);
            const float xv[4] = {x.x, x.y, x.z, x.w}, gv[4] = {gg.x, gg.y, gg.z, gg.w}, nv[4] = {nn.x, nn.y, nn.z, nn.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float f = (e.kind == HYRES_EPI_GDN_BWD) ? (1.0f / sqrtf(nv[c])) : sqrtf(nv[c]);
                o[c] = 2.0f * xv[c] * o[c] + gv[c] * f;
            }
            break;
        }
        default: break;
    }
    if constexpr (H) {
        if (e.accumulate) {
            const float4 p = ldv4<true>(y, pix * ldy + n);
            o[0] += p.x; o[1] += p.y; o[2] += p.z; o[3] += p.w;
        }
        stv4<true>(y, pix * ldy + n, make_float4(o[0], o[1], o[2], o[3]));
    } else {
        float* yp = y + pix * ldy + n;
        if (e.accumulate) {
            const float4 p = ld4(yp);
            o[0] += p.x; o[1] += p.y; o[2] += p.z; o[3] += p.w;
        }
        st4(yp, make_float4(o[0], o[1], o[2], o[3]));
    }
}

}  // namespace hyres
