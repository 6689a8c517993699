// Stand-alone check of the segmented device rANS format's pure-host twins (hyres_wrans2_encode_host / _decode_host /
// _validate, csrc/wrans.hip over csrc/wrans_core.h) for a sanitizer build of the HOST code; no GPU call is made.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I include \
//       scripts/wrans2_host_check.cpp <pkg>/csrc/wrans.hip <pkg>/csrc/pointwise.hip -o wrans2_host_check
//   ./wrans2_host_check         # prints one line per case, exit 0 if every round trip and refusal is right
//
// Cases: those of scripts/wrans_host_check.cpp (n in {0, 1, 63, 64, 65, 4097}, 3 x 5 x 7 under the three parities,
// escapes 5000 / -777, one row made wholly of them), each with R in {1, 2, 3, 64, 1 << 21} rows per segment; the
// strings validate refuses; and seeded single-word mutations of the good strings (at least 1000 in all), each sent
// through validate and then decode_host: a mutation is either refused or decoded, and neither reads or writes out of
// bounds.
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
long long mutations = 0, mutations_refused = 0;
void expect(bool ok, const char* what, const char* name, int R) {
    if (!ok) {
        ++failures;
        std::printf("FAIL %s R = %d: %s (%s)\n", name, R, what, hyres_last_error_string());
    }
}

void put32(std::vector<unsigned char>& s, size_t word, uint32_t v) {
    for (int i = 0; i < 4; ++i) s[4 * word + i] = (unsigned char)(v >> (8 * i));
}
uint32_t get32(const std::vector<unsigned char>& s, size_t word) {
    uint32_t v = 0;
    for (int i = 0; i < 4; ++i) v |= (uint32_t)s[4 * word + i] << (8 * i);
    return v;
}

void run_case(const char* name, const Tables& t, int C, int H, int W, int parity, const std::vector<long long>& esc_k,
              int esc_row, int R, int n_mut) {
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
    expect(k == n, "hyres_wrans_count", name, R);
    const long long S = hyres_wrans2_segments(C, H, W, parity, R);
    expect(S == (n <= 64ll * R ? 1 : (n + 64ll * R - 1) / (64ll * R)), "hyres_wrans2_segments", name, R);
    auto encode = [&](unsigned char* dst, long long cap, long long* len) {
        return hyres_wrans2_encode_host(sym.data(), idx.data(), C, H, W, parity, t.cdf.data(), t.stride,
                                        t.sizes.data(), t.offsets.data(), kNcdf, R, dst, cap, len);
    };
    auto decode = [&](const std::vector<unsigned char>& s, long long len) {
        return hyres_wrans2_decode_host(s.data(), len, idx.data(), C, H, W, parity, t.cdf.data(), t.stride,
                                        t.sizes.data(), t.offsets.data(), kNcdf, params.data(), 2 * C, C, out.data());
    };
    long long len = 0;
    expect(encode(nullptr, 0, &len) == 0, "size query", name, R);
    expect(len <= hyres_wrans2_max_string_bytes(C, H, W, parity, R), "within the worst case", name, R);
    std::vector<unsigned char> s((size_t)len);  // exactly the reported size: an overrun is an ASan error
    expect(encode(s.data(), len, &len) == 0, "encode", name, R);
    int rows = -1;
    expect(hyres_wrans2_validate(s.data(), len, C, H, W, parity, &rows) == 0 && rows == R, "validate", name, R);
    expect(hyres_wrans2_validate(s.data(), len, C, H, W, parity, nullptr) == 0, "validate without R", name, R);
    expect(decode(s, len) == 0, "decode", name, R);
    expect(out == sym, "decode(encode(s)) == s", name, R);
    expect(hyres_wrans_validate(s.data(), len, C, H, W, parity) == HYRES_E_ARG, "HRW1 validate refuses HRW2", name, R);
    // refusals
    std::vector<unsigned char> bad = s;
    bad[3] = '1';
    expect(hyres_wrans2_validate(bad.data(), len, C, H, W, parity, &rows) == HYRES_E_ARG, "wrong magic refused", name, R);
    expect(hyres_wrans2_validate(s.data(), len - 4, C, H, W, parity, &rows) == HYRES_E_ARG, "cut string refused", name, R);
    expect(hyres_wrans2_validate(s.data(), 3, C, H, W, parity, &rows) == HYRES_E_ARG, "3 bytes refused", name, R);
    expect(hyres_wrans2_validate(s.data(), len, C, H, W + 2, parity, &rows) == HYRES_E_ARG, "other shape refused", name, R);
    bad = s;
    put32(bad, 2, 0);
    expect(decode(bad, len) == HYRES_E_ARG, "R = 0 refused", name, R);
    bad = s;
    put32(bad, 3, (uint32_t)S + 1);
    expect(decode(bad, len) == HYRES_E_ARG, "S + 1 refused", name, R);
    bad = s;
    put32(bad, 3, 0x7fffffffu);  // a directory far past the end of the string
    expect(decode(bad, len) == HYRES_E_ARG, "huge S refused", name, R);
    bad = s;
    put32(bad, 4, get32(s, 4) + 64u * (uint32_t)(R < 4096 ? R : 4096) + 1u);  // more escapes than segment 0 has symbols
    expect(decode(bad, len) == HYRES_E_ARG, "directory step past its segment refused", name, R);
    // seeded single-word mutations: refused, or decoded within bounds (wrong symbols are fine)
    for (int m = 0; m < n_mut; ++m) {
        bad = s;
        const size_t nw = (size_t)len / 4;
        const uint32_t pick = rnd() % 4;  // half of them in the header and directory, where validate looks
        const size_t fixed = (size_t)(4 + 2 * S) < nw ? (size_t)(4 + 2 * S) : nw;
        const size_t word = pick < 2 ? rnd() % fixed : rnd() % nw;
        const uint32_t old = get32(bad, word);
        const uint32_t kind = rnd() % 4;
        put32(bad, word, kind == 0 ? old ^ (1u << (rnd() % 32)) : kind == 1 ? old + 1 : kind == 2 ? old - 1
                                                                                                   : (rnd() << 8) ^ rnd());
        ++mutations;
        if (hyres_wrans2_validate(bad.data(), len, C, H, W, parity, &rows) != 0) {
            ++mutations_refused;
            expect(decode(bad, len) == HYRES_E_ARG, "decode_host refuses what validate refuses", name, R);
        } else {
            expect(decode(bad, len) == 0, "a string that validates decodes", name, R);
        }
    }
    std::printf("%-22s R = %7d  n = %5lld  S = %3lld  %6lld bytes\n", name, R, n, S, len);
}

}  // namespace

int main() {
    const Tables t = make_tables();
    for (int R : {1, 2, 3, 64, 1 << 21}) {
        const int m = 30;  // 9 cases x 5 R x 30 = 1350 mutations
        run_case("n1", t, 1, 1, 1, -1, {}, -1, R, m);
        run_case("n63", t, 1, 1, 63, -1, {0, 62}, -1, R, m);
        run_case("n64_lane63_last_row", t, 1, 1, 64, -1, {63}, -1, R, m);
        run_case("n65", t, 1, 1, 65, -1, {64}, -1, R, m);
        run_case("n4097_esc_row", t, 1, 1, 4097, -1, {4095, 4096}, 3, R, m);
        run_case("3x5x7_all", t, 3, 5, 7, -1, {7}, -1, R, m);
        run_case("3x5x7_anchor", t, 3, 5, 7, 0, {3, 53}, -1, R, m);
        run_case("3x5x7_non_anchor", t, 3, 5, 7, 1, {0, 50}, -1, R, m);
        run_case("2x1x1_parity1_n0", t, 2, 1, 1, 1, {}, -1, R, m);
    }
    std::printf("%lld mutations, %lld refused, %lld decoded\n", mutations, mutations_refused,
                mutations - mutations_refused);
    if (mutations < 1000) {
        ++failures;
        std::printf("FAIL fewer than 1000 mutations\n");
    }
    std::printf(failures ? "%d FAILURES\n" : "all cases passed\n", failures);
    return failures ? 1 : 0;
}
