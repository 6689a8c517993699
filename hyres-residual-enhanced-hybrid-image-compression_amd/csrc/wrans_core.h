// rANS lane arithmetic and the wave-interleaved string format HRW1, shared by the sequential host coder (rans.hip),
// the device coder's kernels (wrans.hip) and their pure-host twins. Integer work only: both sides of every function
// here give the same bits.
//
// HRW1, one string per image and pass, little endian:
//   header   "HRW1", uint32 n (coded symbols), uint32 n_esc, uint32 n_words
//   states   64 x uint64 final lane states, lane 0 first (a lane that coded nothing holds 1 << 31)
//   escapes  n_esc x int32 raw symbols, in coded-symbol order
//   payload  n_words x uint32, in the order the decoder reads them
// Coded symbol k is the k-th position, in (c, h, w) order, that the checkerboard parity owns (all of them for
// parity -1); it belongs to row k / 64 and lane k % 64. Each lane is one rans64 coder (64-bit state, 32-bit words,
// 16-bit precision, L = 1 << 31); the encoder walks the rows from last to first, the decoder from first to last. The
// words of the lanes that renormalise at a row lie in ascending lane order, the rows in ascending order. A symbol
// outside its CDF's range codes the CDF's last slot and appends its raw value to the escape list: every coded symbol
// is exactly one rANS step, and a lane emits at most one word per step, so n_words <= n.
#pragma once
#include <cstdint>

#ifndef __host__
#define __host__
#define __device__
#endif
#define WRANS_HD __host__ __device__ inline

namespace hyres {
namespace wrans {

constexpr uint64_t kL = 1ull << 31;  // lower bound of the normalisation interval (64-bit state)
constexpr int kPrecision = 16;
constexpr int kLanes = 64;
constexpr uint32_t kMagic = 0x31575248u;                   // "HRW1"
constexpr int kHeaderWords = 4;                            // magic, n, n_esc, n_words
constexpr int kFixedWords = kHeaderWords + 2 * kLanes;     // header + lane states
constexpr long long kFixedBytes = 4ll * kFixedWords;       // 528

// ---------------------------------------------------------------- lane arithmetic (ryg_rans rans64)
// encoder step: returns true if the lane renormalises, with the word it emits BEFORE coding the symbol
WRANS_HD bool enc_put(uint64_t& x, uint32_t start, uint32_t freq, int scale_bits, uint32_t& word) {
    const uint64_t x_max = ((kL >> scale_bits) << 32) * freq;
    const bool emit = x >= x_max;
    if (emit) {
        word = (uint32_t)x;
        x >>= 32;
    }
    x = ((x / freq) << scale_bits) + (x % freq) + start;
    return emit;
}

WRANS_HD uint32_t dec_get(uint64_t x, int scale_bits) { return (uint32_t)(x & ((1u << scale_bits) - 1)); }

// decoder step: returns true if the lane must read one word (dec_refill) AFTER the symbol
WRANS_HD bool dec_advance(uint64_t& x, uint32_t start, uint32_t freq, int scale_bits) {
    const uint64_t mask = (1ull << scale_bits) - 1;
    x = freq * (x >> scale_bits) + (x & mask) - start;
    return x < kL;
}

WRANS_HD void dec_refill(uint64_t& x, uint32_t word) { x = (x << 32) | word; }

// s with cdf[s] <= cum < cdf[s + 1], 0 <= s <= max_value (cdf strictly increasing, cdf[max_value + 1] = 2^16)
WRANS_HD int cdf_search(const int* cdf, int max_value, uint32_t cum) {
    int lo = 0, hi = max_value;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((uint32_t)cdf[mid] <= cum) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---------------------------------------------------------------- symbol -> CDF slot
// v = sym - offset in [0, max_value): slot v; otherwise the escape slot max_value (raw sym goes to the escape list)
WRANS_HD int slot_of(int sym, int offset, int max_value, bool& esc) {
    const long long v = (long long)sym - offset;
    esc = !(v >= 0 && v < max_value);
    return esc ? max_value : (int)v;
}

// ---------------------------------------------------------------- owned positions
WRANS_HD bool keep(int parity, int h, int w) { return parity < 0 || (((h + w) & 1) == parity); }

// positions w < W of a row with w % 2 == q
WRANS_HD int row_count(int W, int q) { return q == 0 ? (W + 1) / 2 : W / 2; }

// owned positions of one H x W plane: row h owns the w with w % 2 == (parity + h) % 2, so two rows own W together
WRANS_HD long long plane_count(int H, int W, int parity) {
    if (parity < 0) return (long long)H * W;
    return (long long)(H / 2) * W + ((H & 1) ? row_count(W, parity) : 0);
}

WRANS_HD long long count(int C, int H, int W, int parity) { return (long long)C * plane_count(H, W, parity); }

struct Pos {
    int c, h, w;
};

// the k-th owned position in (c, h, w) order; ``plane`` = plane_count(H, W, parity) > 0
WRANS_HD Pos owned_pos(long long k, int H, int W, int parity, long long plane) {
    Pos p;
    p.c = (int)(k / plane);
    const long long r = k - (long long)p.c * plane;
    if (parity < 0) {
        p.h = (int)(r / W);
        p.w = (int)(r - (long long)p.h * W);
        return p;
    }
    const int pair = (int)(r / W);
    const int rr = (int)(r - (long long)pair * W);
    const int c0 = row_count(W, parity);  // row 2 * pair owns w % 2 == parity
    if (rr < c0) {
        p.h = 2 * pair;
        p.w = 2 * rr + parity;
    } else {
        p.h = 2 * pair + 1;
        p.w = 2 * (rr - c0) + (parity ^ 1);
    }
    return p;
}

// ---------------------------------------------------------------- header
struct Header {
    uint32_t n, n_esc, n_words;
};

WRANS_HD uint32_t ld32(const unsigned char* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

enum HeaderError {
    kOk = 0, kShort = 1, kBadMagic = 2, kBadCount = 3, kBadLengths = 4, kBadSize = 5,
    kBadMagic2 = 6, kBadSegments = 7, kBadDirectory = 8  // HRW2 (check_header2)
};

// a string of ``len`` bytes that is to hold ``n_expected`` coded symbols
WRANS_HD int check_header(const unsigned char* in, long long len, long long n_expected, Header& h) {
    if (len >= 4 && ld32(in) != kMagic) return kBadMagic;
    if (len < kFixedBytes || (len & 3)) return kShort;
    h.n = ld32(in + 4);
    h.n_esc = ld32(in + 8);
    h.n_words = ld32(in + 12);
    if ((long long)h.n != n_expected) return kBadCount;
    if (h.n_esc > h.n || h.n_words > h.n) return kBadLengths;
    if (kFixedBytes + 4ll * ((long long)h.n_esc + h.n_words) != len) return kBadSize;
    return kOk;
}

inline const char* header_error(int e) {
    switch (e) {
        case kShort: return "shorter than the header and lane states, or not a whole number of words";
        case kBadMagic: return "no HRW1 magic (a host-format string?)";
        case kBadCount: return "symbol count disagrees with the latent shape and parity";
        case kBadLengths: return "more escapes or payload words than coded symbols";
        case kBadSize: return "header lengths disagree with the byte count";
        case kBadMagic2: return "no HRW2 magic (an HRW1 or a host-format string?)";
        case kBadSegments: return "rows per segment is 0 or the segment count disagrees with the symbol count";
        case kBadDirectory: return "segment directory decreases or gives a segment more escapes or words than symbols";
        default: return "ok";
    }
}

// worst case of one string: every symbol an escape and every step a word
WRANS_HD long long max_string_bytes(long long n) { return kFixedBytes + 8 * n; }

// ---------------------------------------------------------------- HRW2: an HRW1-style string cut into segments
// One string per image and pass, little endian:
//   header     "HRW2", uint32 n (coded symbols), uint32 R (rows per segment, >= 1), uint32 S (segments)
//   directory  S x { uint32 esc_end, uint32 words_end }: cumulative escapes / payload words through segment s
//   states     S x 64 x uint64, segment-major, lane 0 first
//   escapes    esc_end[S - 1] x int32, segments ascending (so coded-symbol order overall)
//   payload    words_end[S - 1] x uint32, segments ascending, HRW1's order within a segment
// S = max(1, ceil(n / (64 R))); segment s owns the coded symbols [64 R s, min(n, 64 R (s + 1))) and is coded exactly as
// HRW1 codes a whole string of those symbols: its states, escapes and payload are byte-equal to that string's.
constexpr uint32_t kMagic2 = 0x32575248u;                  // "HRW2"
constexpr int kHeader2Words = 4;                           // magic, n, R, S
constexpr int kSegFixedWords = 2 + 2 * kLanes;             // per segment: directory entry + lane states

WRANS_HD long long seg_symbols(long long R) { return (long long)kLanes * R; }
WRANS_HD long long segments(long long n, long long R) {
    const long long q = seg_symbols(R);
    return n <= q ? 1 : (n + q - 1) / q;
}
// coded symbols of segment s
WRANS_HD long long seg_count(long long n, long long R, long long s) {
    const long long k0 = seg_symbols(R) * s, k1 = k0 + seg_symbols(R);
    return k0 >= n ? 0 : (k1 < n ? k1 : n) - k0;
}
WRANS_HD long long fixed_words2(long long S) { return kHeader2Words + (long long)kSegFixedWords * S; }
WRANS_HD long long max_string_bytes2(long long n, long long S) { return 4 * fixed_words2(S) + 8 * n; }

struct Header2 {
    uint32_t n, R, S, n_esc, n_words;  // n_esc / n_words: the directory's last entry
};

// a string of ``len`` bytes that is to hold ``n_expected`` coded symbols; fails in the order magic, symbol count,
// segment geometry, directory, byte count
WRANS_HD int check_header2(const unsigned char* in, long long len, long long n_expected, Header2& h) {
    if (len < 4 || ld32(in) != kMagic2) return kBadMagic2;
    if (len < 4ll * kHeader2Words || (len & 3)) return kBadSize;
    h.n = ld32(in + 4);
    h.R = ld32(in + 8);
    h.S = ld32(in + 12);
    if ((long long)h.n != n_expected) return kBadCount;
    if (h.R < 1 || (long long)h.S != segments(h.n, h.R)) return kBadSegments;
    if (len < 4 * fixed_words2(h.S)) return kBadSize;
    uint32_t pe = 0, pw = 0;
    for (long long s = 0; s < (long long)h.S; ++s) {
        const uint32_t e = ld32(in + 16 + 8 * s), w = ld32(in + 20 + 8 * s);
        const long long ns = seg_count(h.n, h.R, s);
        if (e < pe || w < pw || (long long)(e - pe) > ns || (long long)(w - pw) > ns) return kBadDirectory;
        pe = e;
        pw = w;
    }
    h.n_esc = pe;
    h.n_words = pw;
    if (4 * (fixed_words2(h.S) + (long long)pe + pw) != len) return kBadSize;
    return kOk;
}

}  // namespace wrans
}  // namespace hyres
