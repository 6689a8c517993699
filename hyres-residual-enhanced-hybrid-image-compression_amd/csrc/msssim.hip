// MS-SSIM / SSIM of two [B,C,H,W] fp32 batches on the stream (pytorch_msssim's ms_ssim at its defaults; the arithmetic
// lives in msssim_core.h, shared with the host twin below).
//
//   msssim_level_kernel     one work-group per 16 x 32 tile of filter outputs of one (b, c) plane: the 26 x 42 halo of
//                           X and Y -> LDS, the horizontal 11-tap pass of x, y, xx, yy, xy -> LDS (26 x 32 each), the
//                           vertical pass and cs_map / ssim_map in registers, a fixed-order fp64 reduction to ONE
//                           {sum cs, sum ssim} pair per work-group. The same work-group writes the 2 x 2 average-pooled
//                           pixels of X and Y whose window starts in its tile, straight from the staged halo: the
//                           next level's inputs. No moment plane and no map reaches HBM.
//   msssim_finalize_kernel  one work-group per image: every (level, channel)'s partials summed in a fixed order in
//                           fp64 and divided by the map size -> the raw per-level means; relu, powers, product, mean
//                           over channels -> out[b].
// levels + 1 launches; no atomics, no scratch that needs clearing (every partial is written by its work-group before
// it is read), no host sync / allocation / copy: the call is capture-legal and two calls give the same bits. A
// plane's sums depend on that plane alone, so a batch gives each image the bits it gets alone.
#include "common.h"
#include "msssim_core.h"

#include <vector>

namespace hyres {
namespace msssim {

constexpr int kThreads = 256;
constexpr int kFinalThreads = 1024;                  // 16 waves: an RGB image's 15 (level, channel) sums in one round
constexpr int kTH = 16, kTW = 32;                    // filter outputs per work-group
constexpr int kHH = kTH + kHalo, kHW = kTW + kHalo;  // staged input rows / columns
static_assert(kTH * kTW == 2 * kThreads, "two vertically adjacent outputs per thread");

struct Level {
    int H, W, tx, ty;            // input size, tiles
    long long img, part;         // byte offsets: pooled X of this level (Y follows; level 0: unused), partials
};

struct Layout {
    Level lv[kMaxLevels];
    long long means, chan, end;
};

struct FinalArgs {
    long long part[kMaxLevels];  // byte offsets of the partials
    int nblk[kMaxLevels];        // partials per plane
    double n[kMaxLevels];        // map size
};

static long long align256(long long v) { return (v + 255) & ~255LL; }

static Layout make_layout(int B, int C, int H, int W, int levels) {
    Layout L{};
    long long o = 0;
    for (int l = 0; l < levels; ++l) {
        Level& v = L.lv[l];
        v.H = H, v.W = W;
        v.tx = ceil_div(W - kHalo, kTW), v.ty = ceil_div(H - kHalo, kTH);
        if (l) v.img = o, o = align256(o + 2LL * B * C * H * W * (long long)sizeof(float));
        v.part = o, o = align256(o + (long long)B * C * v.tx * v.ty * (long long)sizeof(double2));
        H = pooled_size(H), W = pooled_size(W);
    }
    L.means = o, o = align256(o + (long long)levels * B * C * (long long)sizeof(double));
    L.chan = o, o = align256(o + (long long)B * C * (long long)sizeof(double));
    L.end = o;
    return L;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;  // lane 0
}

__global__ __launch_bounds__(kThreads) void msssim_level_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                               int H, int W, Consts cst, float* __restrict__ PX,
                                                               float* __restrict__ PY, int Hp, int Wp,
                                                               double2* __restrict__ partials) {
    __shared__ float sx[kHH * kHW], sy[kHH * kHW];
    __shared__ float sm[5][kHH * kTW];
    __shared__ double red[2][kThreads / 64];
    const Window w = window();
    const int tid = threadIdx.x;
    const int plane = blockIdx.z, ty0 = blockIdx.y * kTH, tx0 = blockIdx.x * kTW;
    const long long pofs = (long long)plane * H * W;
    const float* xp = X + pofs;
    const float* yp = Y + pofs;

    // the halo, zero outside the plane; consecutive lanes read consecutive columns
    for (int i = tid; i < kHH * kHW; i += kThreads) {
        const int r = i / kHW, c = i - r * kHW;
        const int gr = ty0 + r, gc = tx0 + c;
        const bool in = gr < H && gc < W;
        const long long o = (long long)gr * W + gc;
        sx[i] = in ? xp[o] : 0.0f;
        sy[i] = in ? yp[o] : 0.0f;
    }
    __syncthreads();

    // the next level's pixels whose window's first in-range sample lies in this tile's rows [ty0, ye) x columns
    // [tx0, xe); the last tile of a row / column owns the remainder up to the edge, which its halo holds
    if (PX) {
        const int ph = H & 1, pw = W & 1;
        const int ye = blockIdx.y == gridDim.y - 1 ? H : ty0 + kTH, xe = blockIdx.x == gridDim.x - 1 ? W : tx0 + kTW;
        const int jlo = ty0 == 0 ? 0 : (ty0 + ph + 1) / 2, ilo = tx0 == 0 ? 0 : (tx0 + pw + 1) / 2;
        const int jhi = min(Hp, (ye + ph + 1) / 2), ihi = min(Wp, (xe + pw + 1) / 2);
        const int ni = max(ihi - ilo, 1), n = ihi > ilo && jhi > jlo ? (jhi - jlo) * ni : 0;
        const long long po = (long long)plane * Hp * Wp;
        for (int k = tid; k < n; k += kThreads) {
            const int j = jlo + k / ni, i = ilo + k % ni;
            const long long o = po + (long long)j * Wp + i;
            PX[o] = pool_pixel(H, W, j, i, [&](int r, int c) { return sx[(r - ty0) * kHW + (c - tx0)]; });
            PY[o] = pool_pixel(H, W, j, i, [&](int r, int c) { return sy[(r - ty0) * kHW + (c - tx0)]; });
        }
    }

    // horizontal pass: 26 rows x 32 columns of the five moment planes
    for (int i = tid; i < kHH * kTW; i += kThreads) {
        const int r = i / kTW, c = i % kTW;
        float m[5];
        moments11(w, sx + r * kHW + c, sy + r * kHW + c, m);
#pragma unroll
        for (int k = 0; k < 5; ++k) sm[k][i] = m[k];
    }
    __syncthreads();

    // vertical pass: outputs (2q, col) and (2q + 1, col) share eleven of their twelve rows
    const int col = tid % kTW, row = 2 * (tid / kTW);
    float m0[5], m1[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        float v[kTaps + 1];
#pragma unroll
        for (int t = 0; t <= kTaps; ++t) v[t] = sm[k][(row + t) * kTW + col];
        m0[k] = filter11(w, v);
        m1[k] = filter11(w, v + 1);
    }
    const int Ho = H - kHalo, Wo = W - kHalo;
    double cs = 0.0, ss = 0.0;
    if (tx0 + col < Wo) {
        float c_, s_;
        if (ty0 + row < Ho) ssim_pixel(m0, cst, c_, s_), cs += (double)c_, ss += (double)s_;
        if (ty0 + row + 1 < Ho) ssim_pixel(m1, cst, c_, s_), cs += (double)c_, ss += (double)s_;
    }
    cs = wave_sum(cs), ss = wave_sum(ss);
    if ((tid & 63) == 0) red[0][tid >> 6] = cs, red[1][tid >> 6] = ss;
    __syncthreads();
    if (tid == 0) {
        double a = red[0][0], b = red[1][0];
#pragma unroll
        for (int k = 1; k < kThreads / 64; ++k) a += red[0][k], b += red[1][k];
        partials[((long long)plane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = make_double2(a, b);
    }
}

__global__ __launch_bounds__(kFinalThreads) void msssim_finalize_kernel(const char* __restrict__ ws, FinalArgs a, int B, int C,
                                                                  Weights wt, int levels, double* __restrict__ means,
                                                                  double* __restrict__ chan, float* __restrict__ per_level,
                                                                  float* __restrict__ out) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
    // one wave per (level, channel): lane i takes partials i, i + 64, ... in order, then a fixed shuffle tree
    for (int q = wave; q < levels * C; q += kFinalThreads / 64) {
        const int l = q / C, c = q % C;
        const double2* p = reinterpret_cast<const double2*>(ws + a.part[l]) + (long long)(b * C + c) * a.nblk[l];
        double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
        for (int i = lane; i < a.nblk[l]; i += 64) {  // independent loads in flight; the adds keep their order
            const double2 d = p[i];
            s0 += d.x, s1 += d.y;
        }
        s0 = wave_sum(s0), s1 = wave_sum(s1);
        if (lane == 0) {
            const double v = (l == levels - 1 ? s1 : s0) / a.n[l];
            const long long o = ((long long)l * B + b) * C + c;
            means[o] = v;
            if (per_level) per_level[o] = (float)v;
        }
    }
    __syncthreads();
    for (int c = tid; c < C; c += kFinalThreads)
        chan[(long long)b * C + c] = combine(means + (long long)b * C + c, (long long)B * C, wt, levels);
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int c = 0; c < C; ++c) s += chan[(long long)b * C + c];
        out[b] = (float)(s / (double)C);
    }
}

static int check_shape(const char* what, int B, int C, int H, int W, int levels) {
    HY_REQUIRE(levels >= 1 && levels <= kMaxLevels, HYRES_E_ARG, "%s: 1 <= levels <= %d (got %d)", what, kMaxLevels,
               levels);
    HY_REQUIRE(B >= 1 && C >= 1 && (long long)B * C <= 65535, HYRES_E_SHAPE, "%s: B, C >= 1, B * C <= 65535 (got %d, %d)",
               what, B, C);
    HY_REQUIRE((H < W ? H : W) > min_side_limit(levels), HYRES_E_SHAPE,
               "%s: min(H, W) must be larger than %d = (11 - 1) * 2^(levels - 1) for %d levels (got %d x %d)", what,
               min_side_limit(levels), levels, H, W);
    HY_REQUIRE(H <= 32768 && W <= 32768 && (long long)B * C * H * W < (1LL << 40), HYRES_E_SHAPE,
               "%s: %d x %d x %d x %d is too large", what, B, C, H, W);
    return ok();
}

// one plane, one level on the host: the raw means, and the pooled planes if px != NULL
static void level_host(const float* x, const float* y, int H, int W, const Consts& cst, double& cs_mean, double& ss_mean,
                       std::vector<float>* px, std::vector<float>* py) {
    const Window w = window();
    const int Ho = H - kHalo, Wo = W - kHalo;
    std::vector<float> hm(5LL * H * Wo);
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < Wo; ++c) {
            float m[5];
            moments11(w, x + (long long)r * W + c, y + (long long)r * W + c, m);
            for (int k = 0; k < 5; ++k) hm[((long long)k * H + r) * Wo + c] = m[k];
        }
    double cs = 0.0, ss = 0.0;
    for (int r = 0; r < Ho; ++r)
        for (int c = 0; c < Wo; ++c) {
            float m[5], c_, s_;
            for (int k = 0; k < 5; ++k) m[k] = filter11(w, &hm[((long long)k * H + r) * Wo + c], Wo);
            ssim_pixel(m, cst, c_, s_);
            cs += (double)c_, ss += (double)s_;
        }
    cs_mean = cs / ((double)Ho * Wo), ss_mean = ss / ((double)Ho * Wo);
    if (px) {
        const int Hp = pooled_size(H), Wp = pooled_size(W);
        px->resize((long long)Hp * Wp), py->resize((long long)Hp * Wp);
        for (int j = 0; j < Hp; ++j)
            for (int i = 0; i < Wp; ++i) {
                (*px)[(long long)j * Wp + i] = pool_pixel(H, W, j, i, [&](int r, int c) { return x[(long long)r * W + c]; });
                (*py)[(long long)j * Wp + i] = pool_pixel(H, W, j, i, [&](int r, int c) { return y[(long long)r * W + c]; });
            }
    }
}

}  // namespace msssim
}  // namespace hyres

using namespace hyres;
using namespace hyres::msssim;

extern "C" {

long long hyres_msssim_workspace_bytes(int B, int C, int H, int W, int levels) {
    if (check_shape("msssim_workspace_bytes", B, C, H, W, levels)) return -1;
    return make_layout(B, C, H, W, levels).end;
}

int hyres_msssim(const float* x, const float* y, int B, int C, int H, int W, int levels, const float* weights,
                 float data_range, float* out, float* per_level, void* ws, long long ws_bytes, hyres_stream_t s) {
    HY_REQUIRE(x && y && weights && out, HYRES_E_ARG, "msssim: NULL");
    int rc = check_shape("msssim", B, C, H, W, levels);
    if (rc) return rc;
    const Layout L = make_layout(B, C, H, W, levels);
    HY_REQUIRE(ws && ws_bytes >= L.end, HYRES_E_WORKSPACE, "msssim: workspace %lld < %lld", ws_bytes, L.end);
    HY_REQUIRE(aligned16(ws), HYRES_E_ALIGN, "msssim: workspace alignment");
    char* base = (char*)ws;
    hipStream_t st = as_stream(s);
    const Consts cst = make_consts(data_range);
    Weights wt{};
    FinalArgs fa{};
    const float *cx = x, *cy = y;
    for (int l = 0; l < levels; ++l) {
        const Level& v = L.lv[l];
        wt.w[l] = weights[l];
        fa.part[l] = v.part, fa.nblk[l] = v.tx * v.ty, fa.n[l] = (double)(v.H - kHalo) * (double)(v.W - kHalo);
        float *px = nullptr, *py = nullptr;
        int Hp = 0, Wp = 0;
        if (l + 1 < levels) {
            const Level& nx = L.lv[l + 1];
            Hp = nx.H, Wp = nx.W;
            px = (float*)(base + nx.img), py = px + (long long)B * C * Hp * Wp;
        }
        hipLaunchKernelGGL(msssim_level_kernel, dim3(v.tx, v.ty, B * C), dim3(kThreads), 0, st, cx, cy, v.H, v.W, cst, px,
                           py, Hp, Wp, (double2*)(base + v.part));
        if ((rc = HY_LAUNCH_CHECK("msssim_level"))) return rc;
        cx = px, cy = py;
    }
    hipLaunchKernelGGL(msssim_finalize_kernel, dim3(B), dim3(kFinalThreads), 0, st, (const char*)base, fa, B, C, wt, levels,
                       (double*)(base + L.means), (double*)(base + L.chan), per_level, out);
    return HY_LAUNCH_CHECK("msssim_finalize");
}

int hyres_msssim_host(const float* x, const float* y, int B, int C, int H, int W, int levels, const float* weights,
                      float data_range, float* out, float* per_level, void* ws, long long ws_bytes, hyres_stream_t s) {
    (void)ws, (void)ws_bytes, (void)s;
    HY_REQUIRE(x && y && weights && out, HYRES_E_ARG, "msssim_host: NULL");
    int rc = check_shape("msssim_host", B, C, H, W, levels);
    if (rc) return rc;
    const Consts cst = make_consts(data_range);
    Weights wt{};
    for (int l = 0; l < levels; ++l) wt.w[l] = weights[l];
    const long long plane = (long long)H * W;
    for (int b = 0; b < B; ++b) {
        double acc = 0.0;
        for (int c = 0; c < C; ++c) {
            const long long p = (long long)b * C + c;
            std::vector<float> bx[2], by[2];
            const float *cx = x + p * plane, *cy = y + p * plane;
            double mean[kMaxLevels];
            int h = H, w = W;
            for (int l = 0; l < levels; ++l) {
                const bool pool = l + 1 < levels;
                double cs, ss;
                level_host(cx, cy, h, w, cst, cs, ss, pool ? &bx[l & 1] : nullptr, pool ? &by[l & 1] : nullptr);
                mean[l] = pool ? cs : ss;
                if (per_level) per_level[((long long)l * B + b) * C + c] = (float)mean[l];
                if (pool) cx = bx[l & 1].data(), cy = by[l & 1].data(), h = pooled_size(h), w = pooled_size(w);
            }
            acc += combine(mean, 1, wt, levels);
        }
        out[b] = (float)(acc / (double)C);
    }
    return ok();
}

}  // extern "C"
