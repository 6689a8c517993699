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
//
// Backward (hyres_msssim_bwd: d sum_b grad_out[b] * out[b] / d y; the function is symmetric in x and y, so the other
// gradient is the same call with the images swapped). Self-contained: the launches above run again into the call's own
// workspace for the pooled pyramids and the fp64 means, then
//   msssim_upstream_kernel  the factor grad_out[b] / C * w_l * prod / mean_l / map size per (level, image, channel) in
//                           fp64; exactly 0 for a channel with any mean <= 0.
//   msssim_coef_kernel      per level, coarsest first: the forward's tile and moments again -> the three coefficient
//                           maps a, b, c of d map(p) / d y(q) = g(p - q) * (x(q) * a + y(q) * b + c), at map size.
//   msssim_grad_kernel      per level: one work-group per 16 x 32 tile of input pixels gathers the transposed 11 x 11
//                           separable filter of a, b, c from an LDS-staged halo, forms the level's gradient and adds a
//                           quarter of the coarser level's gradient at the pooled pixel that holds it.
// 3 * levels + 2 launches; gather only, every pixel written by one thread: the forward's guarantees hold.
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

// the (kTH + 10) x (kTW + 10) halo of X and Y whose first sample is (ty0, tx0), zero outside the plane; consecutive
// lanes read consecutive columns
__device__ __forceinline__ void stage_halo(const float* __restrict__ xp, const float* __restrict__ yp, int H, int W,
                                           int ty0, int tx0, float* sx, float* sy) {
    for (int i = threadIdx.x; i < kHH * kHW; i += kThreads) {
        const int r = i / kHW, c = i - r * kHW;
        const int gr = ty0 + r, gc = tx0 + c;
        const bool in = gr < H && gc < W;
        const long long o = (long long)gr * W + gc;
        sx[i] = in ? xp[o] : 0.0f;
        sy[i] = in ? yp[o] : 0.0f;
    }
}

// the five filtered moments of this thread's two vertically adjacent outputs (2q, col) and (2q + 1, col), which share
// eleven of their twelve rows, from the staged halo: the horizontal pass (26 rows x 32 columns of each plane) -> sm,
// then the vertical pass in registers
__device__ __forceinline__ void filtered_moments(const Window& w, const float* sx, const float* sy, float (*sm)[kHH * kTW],
                                                 float m0[5], float m1[5]) {
    const int tid = threadIdx.x;
    for (int i = tid; i < kHH * kTW; i += kThreads) {
        const int r = i / kTW, c = i % kTW;
        float m[5];
        moments11(w, sx + r * kHW + c, sy + r * kHW + c, m);
#pragma unroll
        for (int k = 0; k < 5; ++k) sm[k][i] = m[k];
    }
    __syncthreads();
    const int col = tid % kTW, row = 2 * (tid / kTW);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        float v[kTaps + 1];
#pragma unroll
        for (int t = 0; t <= kTaps; ++t) v[t] = sm[k][(row + t) * kTW + col];
        m0[k] = filter11(w, v);
        m1[k] = filter11(w, v + 1);
    }
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
    stage_halo(X + pofs, Y + pofs, H, W, ty0, tx0, sx, sy);
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

    const int col = tid % kTW, row = 2 * (tid / kTW);
    float m0[5], m1[5];
    filtered_moments(w, sx, sy, sm, m0, m1);
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

// backward, first kernel of a level: the forward's tile and moments again, and instead of the maps' sums the three
// coefficients of ssim_pixel_bwd per filter output -> A, Bc, Cc [plane][Ho][Wo]
__global__ __launch_bounds__(kThreads) void msssim_coef_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                              int H, int W, Consts cst, int last, float* __restrict__ A,
                                                              float* __restrict__ Bc, float* __restrict__ Cc) {
    __shared__ float sx[kHH * kHW], sy[kHH * kHW];
    __shared__ float sm[5][kHH * kTW];
    const Window w = window();
    const int tid = threadIdx.x;
    const int plane = blockIdx.z, ty0 = blockIdx.y * kTH, tx0 = blockIdx.x * kTW;
    const long long pofs = (long long)plane * H * W;
    stage_halo(X + pofs, Y + pofs, H, W, ty0, tx0, sx, sy);
    __syncthreads();
    const int col = tid % kTW, row = 2 * (tid / kTW);
    float m0[5], m1[5];
    filtered_moments(w, sx, sy, sm, m0, m1);
    const int Ho = H - kHalo, Wo = W - kHalo;
    if (tx0 + col >= Wo) return;
    const long long o = (long long)plane * Ho * Wo + (long long)(ty0 + row) * Wo + tx0 + col;
    float a, b, c;
    if (ty0 + row < Ho) ssim_pixel_bwd(m0, cst, last, a, b, c), A[o] = a, Bc[o] = b, Cc[o] = c;
    if (ty0 + row + 1 < Ho) ssim_pixel_bwd(m1, cst, last, a, b, c), A[o + Wo] = a, Bc[o + Wo] = b, Cc[o + Wo] = c;
}

// backward, second kernel of a level: one work-group per 16 x 32 tile of INPUT pixels q of one plane gathers the
// transposed filter of the three coefficient maps (outputs q - 10 .. q in each direction, zero outside the map; the
// window is symmetric, so it is filter11 over that run): the 26 x 42 halo of A, Bc, Cc -> LDS, the horizontal pass ->
// LDS, the vertical pass in registers; G(q) = up * (x(q) * TA + y(q) * TB + TC) + 0.25 * the coarser level's gradient
// at the pooled pixel whose window holds q. Every q is written by exactly one thread: no scatter, no atomics.
__global__ __launch_bounds__(kThreads) void msssim_grad_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                              int H, int W, const float* __restrict__ A,
                                                              const float* __restrict__ Bc, const float* __restrict__ Cc,
                                                              const float* __restrict__ up, const float* __restrict__ Gc,
                                                              int Hp, int Wp, float* __restrict__ G) {
    __shared__ float sc[3][kHH * kHW];
    __shared__ float sh[3][kHH * kTW];
    const Window w = window();
    const int tid = threadIdx.x;
    const int plane = blockIdx.z, ty0 = blockIdx.y * kTH, tx0 = blockIdx.x * kTW;
    const int Ho = H - kHalo, Wo = W - kHalo;
    const long long cofs = (long long)plane * Ho * Wo;
    for (int i = tid; i < kHH * kHW; i += kThreads) {
        const int r = i / kHW, c = i - r * kHW;
        const int pr = ty0 - kHalo + r, pc = tx0 - kHalo + c;
        const bool in = pr >= 0 && pr < Ho && pc >= 0 && pc < Wo;
        const long long o = cofs + (long long)pr * Wo + pc;
        sc[0][i] = in ? A[o] : 0.0f;
        sc[1][i] = in ? Bc[o] : 0.0f;
        sc[2][i] = in ? Cc[o] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < kHH * kTW; i += kThreads) {
        const int r = i / kTW, c = i % kTW;
#pragma unroll
        for (int k = 0; k < 3; ++k) sh[k][i] = filter11(w, sc[k] + r * kHW + c);
    }
    __syncthreads();
    const int col = tid % kTW, row = 2 * (tid / kTW);
    float t0[3], t1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float v[kTaps + 1];
#pragma unroll
        for (int t = 0; t <= kTaps; ++t) v[t] = sh[k][(row + t) * kTW + col];
        t0[k] = filter11(w, v);
        t1[k] = filter11(w, v + 1);
    }
    const int qc = tx0 + col;
    if (qc >= W) return;
    const float u = up[plane];
    const long long pofs = (long long)plane * H * W;
    const float* gc = Gc ? Gc + (long long)plane * Hp * Wp + pool_parent(W, qc) : nullptr;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const int qr = ty0 + row + d;
        if (qr >= H) break;
        const long long o = pofs + (long long)qr * W + qc;
        const float* t = d ? t1 : t0;
        float g = grad_pixel(X[o], Y[o], t[0], t[1], t[2], u);
        if (gc) g = fmaf(0.25f, gc[(long long)pool_parent(H, qr) * Wp], g);
        G[o] = g;
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

// backward: up[l][b][c] = grad_out[b] / C * d combine / d mean[l] / (map size of level l), formed in fp64 from the
// means msssim_finalize_kernel left; one thread per channel of image blockIdx.x
__global__ void msssim_upstream_kernel(const double* __restrict__ means, const float* __restrict__ grad_out, FinalArgs a,
                                       int B, int C, Weights wt, int levels, float* __restrict__ up) {
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        double d[kMaxLevels];
        combine_bwd(means + (long long)b * C + c, (long long)B * C, wt, levels, d);
        const double go = (double)grad_out[b] / (double)C;
        for (int l = 0; l < levels; ++l) up[((long long)l * B + b) * C + c] = (float)(go * d[l] / a.n[l]);
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

// the horizontal pass of one plane pair on the host: hm[k][r][c], H rows x (W - 10) columns of the five moments
static std::vector<float> hpass_host(const Window& w, const float* x, const float* y, int H, int W) {
    const int Wo = W - kHalo;
    std::vector<float> hm(5LL * H * Wo);
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < Wo; ++c) {
            float m[5];
            moments11(w, x + (long long)r * W + c, y + (long long)r * W + c, m);
            for (int k = 0; k < 5; ++k) hm[((long long)k * H + r) * Wo + c] = m[k];
        }
    return hm;
}

// ... and the vertical pass at output (r, c)
static void vpass_host(const Window& w, const std::vector<float>& hm, int H, int Wo, int r, int c, float m[5]) {
    for (int k = 0; k < 5; ++k) m[k] = filter11(w, &hm[((long long)k * H + r) * Wo + c], Wo);
}

// one plane, one level on the host: the raw means, and the pooled planes if px != NULL
static void level_host(const float* x, const float* y, int H, int W, const Consts& cst, double& cs_mean, double& ss_mean,
                       std::vector<float>* px, std::vector<float>* py) {
    const Window w = window();
    const int Ho = H - kHalo, Wo = W - kHalo;
    const std::vector<float> hm = hpass_host(w, x, y, H, W);
    double cs = 0.0, ss = 0.0;
    for (int r = 0; r < Ho; ++r)
        for (int c = 0; c < Wo; ++c) {
            float m[5], c_, s_;
            vpass_host(w, hm, H, Wo, r, c, m);
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

// one plane, one level of the backward on the host, in the kernels' arithmetic: the coefficient maps, their transposed
// filter (horizontal pass first), g[q] = up * (x * TA + y * TB + TC) + 0.25 * gc[parent of q] (gc may be NULL)
static void level_bwd_host(const float* x, const float* y, int H, int W, const Consts& cst, bool last, float up,
                           const float* gc, float* g) {
    const Window w = window();
    const int Ho = H - kHalo, Wo = W - kHalo, Wp = pooled_size(W);
    const std::vector<float> hm = hpass_host(w, x, y, H, W);
    std::vector<float> co(3LL * Ho * Wo), th(3LL * Ho * W);
    for (int r = 0; r < Ho; ++r)
        for (int c = 0; c < Wo; ++c) {
            float m[5], k[3];
            vpass_host(w, hm, H, Wo, r, c, m);
            ssim_pixel_bwd(m, cst, last, k[0], k[1], k[2]);
            for (int i = 0; i < 3; ++i) co[((long long)i * Ho + r) * Wo + c] = k[i];
        }
    float v[kTaps];
    for (int i = 0; i < 3; ++i)
        for (int r = 0; r < Ho; ++r)
            for (int c = 0; c < W; ++c) {
                for (int t = 0; t < kTaps; ++t) {
                    const int pc = c - kHalo + t;
                    v[t] = pc >= 0 && pc < Wo ? co[((long long)i * Ho + r) * Wo + pc] : 0.0f;
                }
                th[((long long)i * Ho + r) * W + c] = filter11(w, v);
            }
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            float t3[3];
            for (int i = 0; i < 3; ++i) {
                for (int t = 0; t < kTaps; ++t) {
                    const int pr = r - kHalo + t;
                    v[t] = pr >= 0 && pr < Ho ? th[((long long)i * Ho + pr) * W + c] : 0.0f;
                }
                t3[i] = filter11(w, v);
            }
            const long long o = (long long)r * W + c;
            float q = grad_pixel(x[o], y[o], t3[0], t3[1], t3[2], up);
            if (gc) q = fmaf(0.25f, gc[(long long)pool_parent(H, r) * Wp + pool_parent(W, c)], q);
            g[o] = q;
        }
}

// hyres_msssim's launches: one level kernel per level into the workspace laid out by L, then the finalize kernel
static int launch_forward(const char* what, const float* x, const float* y, int B, int C, const Layout& L, int levels,
                          const Weights& wt, const Consts& cst, char* base, hipStream_t st, float* per_level, float* out,
                          FinalArgs& fa) {
    int rc;
    const float *cx = x, *cy = y;
    for (int l = 0; l < levels; ++l) {
        const Level& v = L.lv[l];
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
        if ((rc = HY_LAUNCH_CHECK(what))) return rc;
        cx = px, cy = py;
    }
    hipLaunchKernelGGL(msssim_finalize_kernel, dim3(B), dim3(kFinalThreads), 0, st, (const char*)base, fa, B, C, wt, levels,
                       (double*)(base + L.means), (double*)(base + L.chan), per_level, out);
    return HY_LAUNCH_CHECK(what);
}

// the backward's workspace: the forward's, then out[B] (unused), up[levels][B][C], the three coefficient maps at
// level 0's size (every level reuses them, in stream order) and the gradients of levels 1 .. levels - 1
struct BwdLayout {
    Layout fwd;
    long long out, up, coef, coef_plane, grad[kMaxLevels], end;
};

static BwdLayout make_bwd_layout(int B, int C, int H, int W, int levels) {
    BwdLayout L{};
    L.fwd = make_layout(B, C, H, W, levels);
    long long o = L.fwd.end;
    L.out = o, o = align256(o + (long long)B * (long long)sizeof(float));
    L.up = o, o = align256(o + (long long)levels * B * C * (long long)sizeof(float));
    L.coef_plane = align256((long long)B * C * (H - kHalo) * (W - kHalo) * (long long)sizeof(float));
    L.coef = o, o += 3 * L.coef_plane;
    for (int l = 1; l < levels; ++l)
        L.grad[l] = o, o = align256(o + (long long)B * C * L.fwd.lv[l].H * L.fwd.lv[l].W * (long long)sizeof(float));
    L.end = o;
    return L;
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
    Weights wt{};
    FinalArgs fa{};
    for (int l = 0; l < levels; ++l) wt.w[l] = weights[l];
    return launch_forward("msssim", x, y, B, C, L, levels, wt, make_consts(data_range), base, st, per_level, out, fa);
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

long long hyres_msssim_bwd_workspace_bytes(int B, int C, int H, int W, int levels) {
    if (check_shape("msssim_bwd_workspace_bytes", B, C, H, W, levels)) return -1;
    return make_bwd_layout(B, C, H, W, levels).end;
}

int hyres_msssim_bwd(const float* x, const float* y, int B, int C, int H, int W, int levels, const float* weights,
                     float data_range, const float* grad_out, float* grad_y, void* ws, long long ws_bytes,
                     hyres_stream_t s) {
    HY_REQUIRE(x && y && weights && grad_out && grad_y, HYRES_E_ARG, "msssim_bwd: NULL");
    int rc = check_shape("msssim_bwd", B, C, H, W, levels);
    if (rc) return rc;
    const BwdLayout L = make_bwd_layout(B, C, H, W, levels);
    HY_REQUIRE(ws && ws_bytes >= L.end, HYRES_E_WORKSPACE, "msssim_bwd: workspace %lld < %lld", ws_bytes, L.end);
    HY_REQUIRE(aligned16(ws), HYRES_E_ALIGN, "msssim_bwd: workspace alignment");
    char* base = (char*)ws;
    hipStream_t st = as_stream(s);
    const Consts cst = make_consts(data_range);
    Weights wt{};
    FinalArgs fa{};
    for (int l = 0; l < levels; ++l) wt.w[l] = weights[l];
    // the forward again, into this call's own workspace: the pooled pyramids and the fp64 means
    if ((rc = launch_forward("msssim_bwd_forward", x, y, B, C, L.fwd, levels, wt, cst, base, st, nullptr,
                             (float*)(base + L.out), fa)))
        return rc;
    float* up = (float*)(base + L.up);
    hipLaunchKernelGGL(msssim_upstream_kernel, dim3(B), dim3(64), 0, st, (const double*)(base + L.fwd.means), grad_out, fa,
                       B, C, wt, levels, up);
    if ((rc = HY_LAUNCH_CHECK("msssim_upstream"))) return rc;
    float *ca = (float*)(base + L.coef), *cb = (float*)(base + L.coef + L.coef_plane),
          *cc = (float*)(base + L.coef + 2 * L.coef_plane);
    const float* gc = nullptr;  // the coarser level's gradient
    for (int l = levels - 1; l >= 0; --l) {
        const Level& v = L.fwd.lv[l];
        const float* cx = l ? (const float*)(base + v.img) : x;
        const float* cy = l ? cx + (long long)B * C * v.H * v.W : y;
        float* g = l ? (float*)(base + L.grad[l]) : grad_y;
        hipLaunchKernelGGL(msssim_coef_kernel, dim3(v.tx, v.ty, B * C), dim3(kThreads), 0, st, cx, cy, v.H, v.W, cst,
                           (int)(l == levels - 1), ca, cb, cc);
        if ((rc = HY_LAUNCH_CHECK("msssim_coef"))) return rc;
        hipLaunchKernelGGL(msssim_grad_kernel, dim3(ceil_div(v.W, kTW), ceil_div(v.H, kTH), B * C), dim3(kThreads), 0, st,
                           cx, cy, v.H, v.W, (const float*)ca, (const float*)cb, (const float*)cc,
                           (const float*)(up + (long long)l * B * C), gc, gc ? L.fwd.lv[l + 1].H : 0,
                           gc ? L.fwd.lv[l + 1].W : 0, g);
        if ((rc = HY_LAUNCH_CHECK("msssim_grad"))) return rc;
        gc = g;
    }
    return ok();
}

int hyres_msssim_bwd_host(const float* x, const float* y, int B, int C, int H, int W, int levels, const float* weights,
                          float data_range, const float* grad_out, float* grad_y, void* ws, long long ws_bytes,
                          hyres_stream_t s) {
    (void)ws, (void)ws_bytes, (void)s;
    HY_REQUIRE(x && y && weights && grad_out && grad_y, HYRES_E_ARG, "msssim_bwd_host: NULL");
    int rc = check_shape("msssim_bwd_host", B, C, H, W, levels);
    if (rc) return rc;
    const Consts cst = make_consts(data_range);
    Weights wt{};
    for (int l = 0; l < levels; ++l) wt.w[l] = weights[l];
    const long long plane = (long long)H * W;
    for (long long p = 0; p < (long long)B * C; ++p) {
        // the pyramid and the means of this plane, as hyres_msssim_host forms them
        std::vector<float> px[kMaxLevels], py[kMaxLevels], g[kMaxLevels];
        const float *cx[kMaxLevels], *cy[kMaxLevels];
        int h[kMaxLevels], w[kMaxLevels];
        double mean[kMaxLevels], d[kMaxLevels];
        cx[0] = x + p * plane, cy[0] = y + p * plane, h[0] = H, w[0] = W;
        for (int l = 0; l < levels; ++l) {
            const bool pool = l + 1 < levels;
            double cs, ss;
            level_host(cx[l], cy[l], h[l], w[l], cst, cs, ss, pool ? &px[l + 1] : nullptr, pool ? &py[l + 1] : nullptr);
            mean[l] = pool ? cs : ss;
            if (pool) cx[l + 1] = px[l + 1].data(), cy[l + 1] = py[l + 1].data(), h[l + 1] = pooled_size(h[l]),
                      w[l + 1] = pooled_size(w[l]);
        }
        combine_bwd(mean, 1, wt, levels, d);
        const double go = (double)grad_out[p / C] / (double)C;
        const float* gc = nullptr;
        for (int l = levels - 1; l >= 0; --l) {
            const float up = (float)(go * d[l] / ((double)(h[l] - kHalo) * (double)(w[l] - kHalo)));
            float* gl = grad_y + p * plane;
            if (l) g[l].resize((long long)h[l] * w[l]), gl = g[l].data();
            level_bwd_host(cx[l], cy[l], h[l], w[l], cst, l == levels - 1, up, gc, gl);
            gc = gl;
        }
    }
    return ok();
}

}  // extern "C"
