// Stand-alone host program around hyres_msssim_host / hyres_msssim_bwd_host (csrc/msssim.hip compiled into this one
// translation unit) for a sanitizer run of the host twin on a machine without a GPU: the two smallest legal shapes,
// SSIM at 1x1x12x43 and two levels at 1x2x21x21. No GPU call is made. Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//         scripts/msssim_bwd_host_check.hip -o /tmp/msssim_bwd_host_check && /tmp/msssim_bwd_host_check
#include "../hyres-residual-enhanced-hybrid-image-compression_amd/csrc/msssim.hip"

#include <cstdarg>
#include <cstdio>

namespace hyres {
int ok() { return 0; }  // the library's two live in pointwise.hip
int set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    return code;
}
}  // namespace hyres

static int run(int C, int H, int W, int levels, const float* weights) {
    const long long n = (long long)C * H * W;
    std::vector<float> x(n), y(n), g(n, NAN);
    unsigned s = 12345u;
    for (long long i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        x[i] = (float)(s >> 8) / 16777216.0f;
        s = s * 1664525u + 1013904223u;
        y[i] = 0.9f * x[i] + 0.1f * (float)(s >> 8) / 16777216.0f;
    }
    float out = NAN, go = 1.0f;
    int rc = hyres_msssim_host(x.data(), y.data(), 1, C, H, W, levels, weights, 1.0f, &out, nullptr, nullptr, 0, nullptr);
    if (rc) return rc;
    rc = hyres_msssim_bwd_host(x.data(), y.data(), 1, C, H, W, levels, weights, 1.0f, &go, g.data(), nullptr, 0, nullptr);
    if (rc) return rc;
    float m = 0.0f;
    for (float v : g) {
        if (!std::isfinite(v)) return -1;
        m = fmaxf(m, fabsf(v));
    }
    printf("1x%dx%dx%d levels %d: out %.6f max|grad| %.4e\n", C, H, W, levels, out, m);
    return m > 0.0f && out > 0.0f && out < 1.0f ? 0 : -2;
}

int main() {
    const float w1[1] = {1.0f}, w2[2] = {0.4f, 0.6f};
    int rc = run(1, 12, 43, 1, w1);
    if (!rc) rc = run(2, 21, 21, 2, w2);
    printf(rc ? "FAILED %d\n" : "ok\n", rc);
    return rc ? 1 : 0;
}
