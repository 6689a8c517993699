// Stand-alone check of the device rANS coder's pure-host twins (hyres_wrans_encode_host / _decode_host / _validate,
// csrc/wrans.hip over csrc/wrans_core.h) for a sanitizer build of the HOST code; no GPU call is made.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I include \
//       scripts/wrans_host_check.cpp <pkg>/csrc/wrans.hip <pkg>/csrc/pointwise.hip -o wrans_host_check
//   ./wrans_host_check          # prints one line per case, exit 0 if every round trip and refusal is right
//
// Cases: n in {1, 63, 64, 65, 4097} with all positions owned, 3 x 5 x 7 under parity -1 / 0 / 1, 2 x 1 x 1 under
// parity 1 (n = 0); escapes 5000 and -777 (one in lane 63 of the last row, one row made wholly of them); and the
// strings validate refuses: wrong magic, cut by 4 bytes, another shape, lengths past the end.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hyres_hip.h"

namespace {

constexpr int kNcdf = 8;
struct Tables {
    std::vector<int> cdf, sizes, offsets;
    int stride;
};

// CDF row i: 2 * (i + 2) + 1 symbols centred on 0 with triangular frequencies, plus the escape slot
Tables make_tables() {
    Tables t;
    t.stride = 2 * (kNcdf + 1) + 1 + 2;
    t.cdf.assign((size_t)kNcdf * t.stride, 0);
    for (int i = 0; i < kNcdf; ++i) {
        const int half = i + 2, len = 2 * half + 1;
        std::vector<long long> f(len + 1);
        long long total = 0;
        for (int k = 0; k < len; ++k) total += f[k] = 1 + 50ll * (half + 1 - std::abs(k - half));
        total += f[len] = 1;  // escape slot
        int* row = &t.cdf[(size_t)i * t.stride];
        long long acc = 0, used = 0;
        for (int k = 0; k <= len; ++k) {
            row[k] = (int)used;
            acc += f[k];
            long long next = acc * 65536 / total;
            if (next <= used) next = used + 1;
            used = next;
        }
        row[len + 1] = 65536;
        t.sizes.push_back(len + 2);
        t.offsets.push_back(-half);
    }
    return t;
}

uint32_t rng_state = 12345u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

int failures = 0;
void expect(bool ok, const char* what, const char* name) {
    if (!ok) {
        ++failures;
        std::printf("FAIL %s: %s (%s)\n", name, what, hyres_last_error_string());
    }
}

void run_case(const char* name, const Tables& t, int C, int H, int W, int parity, const std::vector<long long>& esc_k,
              int esc_row) {
    const long long chw = (long long)C * H * W, n = hyres_wrans_count(C, H, W, parity);
    std::vector<int> sym(chw), idx(chw), out(chw, -12345);
    std::vector<float> params((size_t)H * W * 2 * C);
    for (auto& v : params) v = (float)((int)(rnd() % 2001) - 1000) / 100.f;
    long long k = 0;
    for (int c = 0; c < C; ++c)
        for (int h = 0; h < H; ++h)
            for (int w = 0; w < W; ++w) {
                const long long i = ((long long)c * H + h) * W + w;
                idx[i] = (int)(rnd() % kNcdf);
                if (parity >= 0 && ((h + w) & 1) != parity) {
                    sym[i] = (int)rintf(0.f - params[((size_t)h * W + w) * 2 * C + C + c]);
                    continue;
                }
                const int half = idx[i] + 2;
                sym[i] = (int)(rnd() % (2 * half + 1)) - half;
                bool esc = esc_row >= 0 && k / 64 == esc_row;
                for (long long e : esc_k) esc = esc || e == k;
                if (esc) sym[i] = (k & 1) ? -777 : 5000;
                if (k % 97 == 11) sym[i] = half + 1;  // v == max_value: escapes
                ++k;
            }
    expect(k == n, "hyres_wrans_count", name);
    long long len = 0;
    expect(hyres_wrans_encode_host(sym.data(), idx.data(), C, H, W, parity, t.cdf.data(), t.stride, t.sizes.data(),
                                   t.offsets.data(), kNcdf, nullptr, 0, &len) == 0, "size query", name);
    std::vector<unsigned char> s((size_t)len);  // exactly the reported size: an overrun is an ASan error
    expect(hyres_wrans_encode_host(sym.data(), idx.data(), C, H, W, parity, t.cdf.data(), t.stride, t.sizes.data(),
                                   t.offsets.data(), kNcdf, s.data(), len, &len) == 0, "encode", name);
    expect(hyres_wrans_validate(s.data(), len, C, H, W, parity) == 0, "validate", name);
    expect(hyres_wrans_decode_host(s.data(), len, idx.data(), C, H, W, parity, t.cdf.data(), t.stride, t.sizes.data(),
                                   t.offsets.data(), kNcdf, params.data(), 2 * C, C, out.data()) == 0, "decode", name);
    expect(out == sym, "decode(encode(s)) == s", name);
    // refusals
    std::vector<unsigned char> bad = s;
    bad[3] = '2';
    expect(hyres_wrans_validate(bad.data(), len, C, H, W, parity) == HYRES_E_ARG, "wrong magic refused", name);
    expect(hyres_wrans_validate(s.data(), len - 4, C, H, W, parity) == HYRES_E_ARG, "cut string refused", name);
    expect(hyres_wrans_validate(s.data(), len, C, H, W + 2, parity) == HYRES_E_ARG, "other shape refused", name);
    bad = s;
    bad[12] = 0xff, bad[13] = 0xff, bad[14] = 0xff, bad[15] = 0x7f;  // n_words far past the end
    expect(hyres_wrans_decode_host(bad.data(), len, idx.data(), C, H, W, parity, t.cdf.data(), t.stride,
                                   t.sizes.data(), t.offsets.data(), kNcdf, params.data(), 2 * C, C,
                                   out.data()) == HYRES_E_ARG, "bad lengths refused", name);
    // a payload damaged in place still decodes within bounds (wrong symbols are fine)
    if (len > 528 + 8) {
        bad = s;
        for (long long i = 528; i < len; ++i) bad[(size_t)i] ^= (unsigned char)rnd();
        (void)hyres_wrans_decode_host(bad.data(), len, idx.data(), C, H, W, parity, t.cdf.data(), t.stride,
                                      t.sizes.data(), t.offsets.data(), kNcdf, params.data(), 2 * C, C, out.data());
    }
    std::printf("%-22s n = %5lld  %6lld bytes\n", name, n, len);
}

}  // namespace

int main() {
    const Tables t = make_tables();
    run_case("n1", t, 1, 1, 1, -1, {}, -1);
    run_case("n63", t, 1, 1, 63, -1, {0, 62}, -1);
    run_case("n64_lane63_last_row", t, 1, 1, 64, -1, {63}, -1);
    run_case("n65", t, 1, 1, 65, -1, {64}, -1);
    run_case("n4097_esc_row", t, 1, 1, 4097, -1, {4095, 4096}, 3);
    run_case("3x5x7_all", t, 3, 5, 7, -1, {7}, -1);
    run_case("3x5x7_anchor", t, 3, 5, 7, 0, {3, 53}, -1);
    run_case("3x5x7_non_anchor", t, 3, 5, 7, 1, {0, 50}, -1);
    run_case("2x1x1_parity1_n0", t, 2, 1, 1, 1, {}, -1);
    std::printf(failures ? "%d FAILURES\n" : "all cases passed\n", failures);
    return failures ? 1 : 0;
}
