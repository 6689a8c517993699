// MS-SSIM arithmetic shared by the HIP kernels (msssim.hip) and the pure-host twin: pytorch_msssim's ms_ssim at its
// defaults (11-tap sigma 1.5 Gaussian, valid filtering, K = (0.01, 0.03), avg_pool2d(2, 2, padding = side % 2,
// count_include_pad) between levels, relu of the per-channel means before the weighted product).
//
// One arithmetic for both sides: every filter sum is a left-to-right fmaf chain over the taps (horizontal pass
// first, vertical pass on its fp32 result), the per-pixel formula is evaluated in fp32 in the order below, the maps
// are summed in fp64, and the level combine runs in fp64. Only the order in which the fp64 sums meet differs between
// the device (per-tile partials, then a fixed tree) and the host loop (row-major).
#pragma once
#include <cmath>

#ifndef __host__
#define __host__
#define __device__
#endif
#define MSSSIM_HD __host__ __device__ inline

namespace hyres {
namespace msssim {

constexpr int kTaps = 11;
constexpr int kHalo = kTaps - 1;
constexpr int kMaxLevels = 5;

// g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) evaluated and normalised to sum 1 in fp32 (the values torch.exp gives
// pytorch_msssim's _fspecial_gauss_1d), as exact hex floats; g[5 + k] == g[5 - k]
struct Window {
    float g[kTaps];
};
MSSSIM_HD constexpr Window window() {
    return Window{{0x1.0d957p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
                   0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d957p-10f}};
}

// the default level weights (Wang, Simoncelli, Bovik 2003)
struct Weights {
    float w[kMaxLevels];
};
MSSSIM_HD constexpr Weights default_weights() { return Weights{{0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f}}; }

struct Consts {
    float C1, C2;
};
// C = (K * L)^2 formed in double and rounded once, as a Python scalar meets an fp32 tensor
MSSSIM_HD Consts make_consts(float data_range) {
    const double a = 0.01 * (double)data_range, b = 0.03 * (double)data_range;
    return Consts{(float)(a * a), (float)(b * b)};
}

// sum_k g[k] * v[k * stride]
MSSSIM_HD float filter11(const Window& w, const float* v, int stride = 1) {
    float acc = w.g[0] * v[0];
#pragma unroll
    for (int k = 1; k < kTaps; ++k) acc = fmaf(w.g[k], v[k * stride], acc);
    return acc;
}

// horizontal pass at one position: the five moment planes x, y, x*x, y*y, x*y of xr[0..10], yr[0..10]
MSSSIM_HD void moments11(const Window& w, const float* xr, const float* yr, float m[5]) {
    float a[5];
    {
        const float x = xr[0], y = yr[0];
        a[0] = w.g[0] * x, a[1] = w.g[0] * y, a[2] = w.g[0] * (x * x), a[3] = w.g[0] * (y * y), a[4] = w.g[0] * (x * y);
    }
#pragma unroll
    for (int k = 1; k < kTaps; ++k) {
        const float x = xr[k], y = yr[k], g = w.g[k];
        a[0] = fmaf(g, x, a[0]);
        a[1] = fmaf(g, y, a[1]);
        a[2] = fmaf(g, x * x, a[2]);
        a[3] = fmaf(g, y * y, a[3]);
        a[4] = fmaf(g, x * y, a[4]);
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) m[i] = a[i];
}

// cs_map and ssim_map at one pixel from the filtered moments (mu1, mu2, E[xx], E[yy], E[xy])
MSSSIM_HD void ssim_pixel(const float m[5], const Consts& c, float& cs, float& ssim) {
    const float mu1 = m[0], mu2 = m[1];
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const float s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu12;
    cs = (2.0f * s12 + c.C2) / (s1 + s2 + c.C2);
    ssim = ((2.0f * mu12 + c.C1) / (mu1_sq + mu2_sq + c.C1)) * cs;
}

// The backward of one filter output p towards the second image: with g the window weight that joins p to the input
// pixel q, d cs(p) / d y(q) = g * (x(q) * a + y(q) * b + c) where a = 2 / B2, b = -cs * a, c = a * (cs * mu2 - mu1)
// and B2 = s1 + s2 + C2. ``last`` gives the same three coefficients for ssim(p) = l * cs: l times the above, plus
// cs * dl / dmu2 = cs * 2 * (mu1 - l * mu2) / B1 in c.
MSSSIM_HD void ssim_pixel_bwd(const float m[5], const Consts& k, bool last, float& a, float& b, float& c) {
    const float mu1 = m[0], mu2 = m[1];
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const float s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu12;
    const float B2 = s1 + s2 + k.C2;
    const float cs = (2.0f * s12 + k.C2) / B2;
    a = 2.0f / B2;
    b = -cs * a;
    c = a * (cs * mu2 - mu1);
    if (last) {
        const float B1 = mu1_sq + mu2_sq + k.C1;
        const float l = (2.0f * mu12 + k.C1) / B1;
        a *= l, b *= l;
        c = fmaf(l, c, cs * (2.0f * (mu1 - l * mu2) / B1));
    }
}

// the level's local gradient at input pixel q from the transposed-filtered coefficient maps, times the upstream
// factor ``u`` of this (level, image, channel); exactly 0 where u is 0
MSSSIM_HD float grad_pixel(float x, float y, float ta, float tb, float tc, float u) {
    return u == 0.0f ? 0.0f : u * fmaf(x, ta, fmaf(y, tb, tc));
}

// avg_pool2d(kernel 2, stride 2, padding = side % 2, count_include_pad): the next level's side
MSSSIM_HD int pooled_size(int s) { return (s + 2 * (s & 1) - 2) / 2 + 1; }

// pooled pixel (j, i) of an H x W plane: rows 2j - (H % 2) and the next, columns 2i - (W % 2) and the next, zeros
// outside, divisor 4. ``at(r, c)`` returns the in-range sample.
template <class At>
MSSSIM_HD float pool_pixel(int H, int W, int j, int i, At at) {
    const int r0 = 2 * j - (H & 1), c0 = 2 * i - (W & 1);
    float acc = 0.0f;
#pragma unroll
    for (int dr = 0; dr < 2; ++dr)
#pragma unroll
        for (int dc = 0; dc < 2; ++dc) {
            const int r = r0 + dr, c = c0 + dc;
            if (r >= 0 && r < H && c >= 0 && c < W) acc += at(r, c);
        }
    return acc * 0.25f;
}

// the transpose of pool_pixel: row / column r of a plane of side ``side`` lies in the window of pooled row / column
// (r + side % 2) / 2, which always exists; the padded positions have no pixel and so receive nothing
MSSSIM_HD int pool_parent(int side, int r) { return (r + (side & 1)) >> 1; }

// prod_l relu(mean[l])^w[l] in fp64; mean[l * stride] = the raw spatial mean of level l (cs, or ssim for the last)
MSSSIM_HD double combine(const double* mean, long long stride, const Weights& w, int levels) {
    double p = 1.0;
    for (int l = 0; l < levels; ++l) {
        const double v = mean[l * stride] > 0.0 ? mean[l * stride] : 0.0;
        p *= pow(v, (double)w.w[l]);
    }
    return p;
}

// d combine / d mean[l] = w[l] * combine / mean[l] in fp64, and exactly 0 for every level as soon as one level's mean
// is <= 0 (what relu's and pow's backward give: never inf or NaN)
MSSSIM_HD void combine_bwd(const double* mean, long long stride, const Weights& w, int levels, double d[kMaxLevels]) {
    bool pos = true;
    for (int l = 0; l < levels; ++l) pos = pos && mean[l * stride] > 0.0;
    const double p = pos ? combine(mean, stride, w, levels) : 0.0;
    for (int l = 0; l < levels; ++l) d[l] = pos ? (double)w.w[l] * p / mean[l * stride] : 0.0;
}

// min(H, W) must exceed this for ``levels`` levels: every level keeps at least one filter output
MSSSIM_HD int min_side_limit(int levels) { return kHalo << (levels - 1); }

}  // namespace msssim
}  // namespace hyres
