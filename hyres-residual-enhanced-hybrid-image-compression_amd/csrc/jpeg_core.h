// Baseline JPEG 4:2:2 codec core shared by the host round trip and the gfx950 kernels (csrc/jpeg.hip).
//
// It restates libjpeg's baseline pipeline the way libjpeg-turbo runs it for PyTurboJPEG's defaults (BGR input,
// TJSAMP_422, JDCT_ISLOW, the Annex K Huffman tables, fancy upsampling on decode).  Everything is integer
// arithmetic, so host and device produce the same bits as the library:
//   encode: bytes = (clamp(x, 0, 1) * 255) truncated -> YCbCr (16-bit fixed-point tables) -> h2v1 chroma
//           downsample (alternating 0/1 bias) -> -128 -> forward islow DCT (output scaled by 8) -> round-half-away
//           division by 8*q -> zigzag -> DC difference / AC run-size Huffman codes, 0xFF stuffing, 1-bit padding;
//   decode: coefficient * q -> inverse islow DCT with range limiting -> fancy h2v1 upsample ((3a+b+1)>>2,
//           (3a+c+2)>>2) -> YCbCr -> BGR -> float(v) / 255.
// Any H x W: an image that is not whole 16x8 MCUs is coded as libjpeg codes it.  Encode: every component's last real
// row is replicated down to 8 * ceil(H/8) rows and its last real sample to the right (luminance to 8 * ceil(W/8)
// columns, the full-resolution chroma to 16 * ceil(W/16) columns before the h2v1 average), both by clamping the
// pixel coordinates; when ceil(W/8) is odd the second luminance block of a row's last MCU lies outside the
// component and is a dummy block: AC all zero, DC = the quantised DC of the block before it (so its DC difference
// is 0 and it is the predictor of the next luminance block).  Decode: every block of the scan is entropy-decoded
// and inverse-transformed into planes of the padded extents; fancy upsampling applies its last-column rule at the
// last real chroma sample, column ceil(W/2) - 1, and a chroma row of one or two samples (W <= 4) is replicated,
// not interpolated (jdsample.c picks h2v1_upsample for downsampled_width <= 2); samples outside H x W are never
// shown.  Whole-MCU images take none of these paths.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define JC_HD __host__ __device__ __forceinline__
#else
#define JC_HD inline
#endif

namespace hyres {
namespace jpeg {

constexpr int kHeaderBytes = 623;       // SOI, JFIF APP0, 2 DQT, SOF0, 4 DHT, SOS
// Entropy-coded bits of one 8x8 block, worst case: DC 11-bit code + 11 bits, and 63 AC coefficients of a 16-bit
// code + 10 bits each (a ZRL only replaces coefficients that would cost more) = 22 + 63 * 26 = 1660 -> 1664.
constexpr int kMaxBlockBits = 1664;

// ---------------------------------------------------------------------------------------------- tables
// JPEG Annex K.1 quantisation tables in zigzag order (the order of a DQT payload)
constexpr uint8_t kStdQuant[2][64] = {
    {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40,
     26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87,
     95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99},
    {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// natural (row-major) index of zigzag position k
constexpr uint8_t kNatural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// JPEG Annex K.3 Huffman tables: code counts per length 1..16, then the symbols in code order
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
     0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
     0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
     0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
     0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
     0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
     0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
     0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
     0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
     0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
     0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
     0xf9, 0xfa}};

// code word and length per symbol (libjpeg's jpeg_make_c_derived_tbl), index 0 luminance / 1 chrominance.
// The kernels read this from constant memory; the host from a static copy.
struct HuffTables {
    uint16_t dc_code[2][12];
    uint8_t dc_size[2][12];
    uint16_t ac_code[2][256];
    uint8_t ac_size[2][256];
};

constexpr HuffTables make_huff_tables() {
    HuffTables t{};
    for (int c = 0; c < 2; ++c) {
        int code = 0, p = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < kDcBits[c][l - 1]; ++i, ++p, ++code) {
                t.dc_code[c][kDcVals[p]] = (uint16_t)code;
                t.dc_size[c][kDcVals[p]] = (uint8_t)l;
            }
            code <<= 1;
        }
        code = 0;
        p = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < kAcBits[c][l - 1]; ++i, ++p, ++code) {
                t.ac_code[c][kAcVals[c][p]] = (uint16_t)code;
                t.ac_size[c][kAcVals[c][p]] = (uint8_t)l;
            }
            code <<= 1;
        }
    }
    return t;
}

// quantisation steps of both tables in natural order, as the block functions index them
struct QuantTables {
    uint16_t q[2][64];
};

// libjpeg jpeg_quality_scaling + jpeg_add_quant_table(force_baseline): zigzag order, entries in 1..255
inline void quant_tables_zigzag(int quality, uint8_t lum[64], uint8_t chr[64]) {
    if (quality <= 0) quality = 1;
    if (quality > 100) quality = 100;
    const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
    for (int c = 0; c < 2; ++c) {
        uint8_t* out = c ? chr : lum;
        for (int k = 0; k < 64; ++k) {
            long t = ((long)kStdQuant[c][k] * scale + 50L) / 100L;
            if (t <= 0) t = 1;
            if (t > 255) t = 255;
            out[k] = (uint8_t)t;
        }
    }
}

inline QuantTables quant_tables_natural(int quality) {
    uint8_t z[2][64];
    quant_tables_zigzag(quality, z[0], z[1]);
    QuantTables q{};
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 64; ++k) q.q[c][kNatural[k]] = z[c][k];
    return q;
}

// ---------------------------------------------------------------------------------------------- pixels
// (clamp(x, 0, 1) * 255).byte(): one fp32 multiply, then truncation
JC_HD int to_byte(float v) {
    v = v < 0.0f ? 0.0f : v;
    v = v > 1.0f ? 1.0f : v;
    return (int)(v * 255.0f);
}

constexpr int fix16(double x) { return (int)(x * 65536.0 + 0.5); }
constexpr int kHalf16 = 1 << 15;
constexpr int kCOffset = 128 << 16;

// jccolor.c rgb_ycc_convert
JC_HD int rgb_to_y(int r, int g, int b) {
    return (fix16(0.29900) * r + fix16(0.58700) * g + fix16(0.11400) * b + kHalf16) >> 16;
}
JC_HD int rgb_to_cb(int r, int g, int b) {
    return (-fix16(0.16874) * r - fix16(0.33126) * g + fix16(0.50000) * b + kCOffset + kHalf16 - 1) >> 16;
}
JC_HD int rgb_to_cr(int r, int g, int b) {
    return (fix16(0.50000) * r - fix16(0.41869) * g - fix16(0.08131) * b + kCOffset + kHalf16 - 1) >> 16;
}

JC_HD int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// jdcolor.c ycc_rgb_convert (arithmetic right shifts of negative values, as libjpeg's RIGHT_SHIFT)
JC_HD void ycc_to_rgb(int y, int cb, int cr, int& r, int& g, int& b) {
    const int xb = cb - 128, xr = cr - 128;
    r = clamp255(y + ((fix16(1.40200) * xr + kHalf16) >> 16));
    b = clamp255(y + ((fix16(1.77200) * xb + kHalf16) >> 16));
    g = clamp255(y + ((-fix16(0.34414) * xb + kHalf16 - fix16(0.71414) * xr) >> 16));
}

// Level-shifted samples of one block.  x is one image, planar [3][H][W] with plane 0 = B, 1 = G, 2 = R.
// comp 0: luminance block (bx, by) of 8x8 pixels; comp 1 / 2: Cb / Cr block covering 16x8 pixels, downsampled
// 2:1 horizontally with libjpeg's h2v1 bias (0 on even output columns, 1 on odd ones).  EDGE: the block reaches
// past the image; pixel coordinates are clamped to the last real row / column (libjpeg's edge replication).
template <bool EDGE>
JC_HD void sample_block_at(const float* x, int H, int W, int comp, int bx, int by, int* d) {
    const long long plane = (long long)H * W;
    const int x0 = bx * (comp ? 16 : 8);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int y = by * 8 + r;
        const float* p = x + (long long)(EDGE && y > H - 1 ? H - 1 : y) * W + (EDGE ? 0 : x0);
        if (comp == 0) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int i = EDGE ? (x0 + c > W - 1 ? W - 1 : x0 + c) : c;
                d[r * 8 + c] = rgb_to_y(to_byte(p[2 * plane + i]), to_byte(p[plane + i]), to_byte(p[i])) - 128;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                int v[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int i = EDGE ? (x0 + 2 * c + h > W - 1 ? W - 1 : x0 + 2 * c + h) : 2 * c + h;
                    const int R = to_byte(p[2 * plane + i]), G = to_byte(p[plane + i]), B = to_byte(p[i]);
                    v[h] = comp == 1 ? rgb_to_cb(R, G, B) : rgb_to_cr(R, G, B);
                }
                d[r * 8 + c] = ((v[0] + v[1] + (c & 1)) >> 1) - 128;
            }
        }
    }
}

JC_HD void sample_block(const float* x, int H, int W, int comp, int bx, int by, int* d) {
    if (by * 8 + 8 > H || (bx + 1) * (comp ? 16 : 8) > W)
        sample_block_at<true>(x, H, W, comp, bx, by, d);
    else
        sample_block_at<false>(x, H, W, comp, bx, by, d);
}

// ---------------------------------------------------------------------------------------------- DCT
constexpr int kConstBits = 13, kPass1Bits = 2;
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270,
              F_0_899976223 = 7373, F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137,
              F_1_961570560 = 16069, F_2_053119869 = 16819, F_2_562915447 = 20995, F_3_072711026 = 25172;

JC_HD int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c jpeg_fdct_islow: in place on 64 natural-order samples; the output is 8x the true DCT
template <int STRIDE, bool PASS1>
JC_HD void fdct_1d(int* p) {
    const int tmp0 = p[0 * STRIDE] + p[7 * STRIDE], tmp7 = p[0 * STRIDE] - p[7 * STRIDE];
    const int tmp1 = p[1 * STRIDE] + p[6 * STRIDE], tmp6 = p[1 * STRIDE] - p[6 * STRIDE];
    const int tmp2 = p[2 * STRIDE] + p[5 * STRIDE], tmp5 = p[2 * STRIDE] - p[5 * STRIDE];
    const int tmp3 = p[3 * STRIDE] + p[4 * STRIDE], tmp4 = p[3 * STRIDE] - p[4 * STRIDE];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int SH = PASS1 ? kConstBits - kPass1Bits : kConstBits + kPass1Bits;
    if (PASS1) {
        p[0 * STRIDE] = (tmp10 + tmp11) * (1 << kPass1Bits);
        p[4 * STRIDE] = (tmp10 - tmp11) * (1 << kPass1Bits);
    } else {
        p[0 * STRIDE] = descale(tmp10 + tmp11, kPass1Bits);
        p[4 * STRIDE] = descale(tmp10 - tmp11, kPass1Bits);
    }
    int z1 = (tmp12 + tmp13) * F_0_541196100;
    p[2 * STRIDE] = descale(z1 + tmp13 * F_0_765366865, SH);
    p[6 * STRIDE] = descale(z1 + tmp12 * (-F_1_847759065), SH);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * F_1_175875602;
    const int t4 = tmp4 * F_0_298631336, t5 = tmp5 * F_2_053119869, t6 = tmp6 * F_3_072711026,
              t7 = tmp7 * F_1_501321110;
    z1 *= -F_0_899976223;
    z2 *= -F_2_562915447;
    z3 = z3 * (-F_1_961570560) + z5;
    z4 = z4 * (-F_0_390180644) + z5;
    p[7 * STRIDE] = descale(t4 + z1 + z3, SH);
    p[5 * STRIDE] = descale(t5 + z2 + z4, SH);
    p[3 * STRIDE] = descale(t6 + z2 + z3, SH);
    p[1 * STRIDE] = descale(t7 + z1 + z4, SH);
}

JC_HD void fdct_islow(int* d) {
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct_1d<1, true>(d + r * 8);
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct_1d<8, false>(d + c);
}

// jcdctmgr.c: round-half-away division of the 8x-scaled coefficient by 8 * q, in place
JC_HD void quantize(int* d, const uint16_t* q) {
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int qv = (int)q[i] << 3;
        const int v = d[i];
        int t = (v < 0 ? -v : v) + (qv >> 1);
        t = t >= qv ? t / qv : 0;
        d[i] = v < 0 ? -t : t;
    }
}

// libjpeg's IDCT range limit table, centred: index (x & 1023) of sample_range_limit + 128
JC_HD int range_limit(int x) {
    const int i = x & 1023;
    return i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896));
}

// jidctint.c jpeg_idct_islow 1-D pass (its all-zero shortcuts give the same values)
template <int STRIDE, bool PASS1>
JC_HD void idct_1d(int* p) {
    int z2 = p[2 * STRIDE], z3 = p[6 * STRIDE];
    int z1 = (z2 + z3) * F_0_541196100;
    int tmp2 = z1 + z3 * (-F_1_847759065);
    int tmp3 = z1 + z2 * F_0_765366865;
    z2 = p[0 * STRIDE];
    z3 = p[4 * STRIDE];
    int tmp0 = (z2 + z3) * (1 << kConstBits);
    int tmp1 = (z2 - z3) * (1 << kConstBits);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = p[7 * STRIDE];
    tmp1 = p[5 * STRIDE];
    tmp2 = p[3 * STRIDE];
    tmp3 = p[1 * STRIDE];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F_1_175875602;
    tmp0 *= F_0_298631336;
    tmp1 *= F_2_053119869;
    tmp2 *= F_3_072711026;
    tmp3 *= F_1_501321110;
    z1 *= -F_0_899976223;
    z2 *= -F_2_562915447;
    z3 = z3 * (-F_1_961570560) + z5;
    z4 = z4 * (-F_0_390180644) + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    constexpr int SH = PASS1 ? kConstBits - kPass1Bits : kConstBits + kPass1Bits + 3;
    p[0 * STRIDE] = descale(tmp10 + tmp3, SH);
    p[7 * STRIDE] = descale(tmp10 - tmp3, SH);
    p[1 * STRIDE] = descale(tmp11 + tmp2, SH);
    p[6 * STRIDE] = descale(tmp11 - tmp2, SH);
    p[2 * STRIDE] = descale(tmp12 + tmp1, SH);
    p[5 * STRIDE] = descale(tmp12 - tmp1, SH);
    p[3 * STRIDE] = descale(tmp13 + tmp0, SH);
    p[4 * STRIDE] = descale(tmp13 - tmp0, SH);
}

// quantised natural-order coefficients -> 64 samples in 0..255, in place
JC_HD void dequant_idct(int* d, const uint16_t* q) {
#pragma unroll
    for (int i = 0; i < 64; ++i) d[i] *= (int)q[i];
#pragma unroll
    for (int c = 0; c < 8; ++c) idct_1d<8, true>(d + c);
#pragma unroll
    for (int r = 0; r < 8; ++r) idct_1d<1, false>(d + r * 8);
#pragma unroll
    for (int i = 0; i < 64; ++i) d[i] = range_limit(d[i]);
}

// ---------------------------------------------------------------------------------------------- block layout
// Blocks of one image are numbered in scan order: MCU m = my * ceil(W/16) + mx holds blocks 4m .. 4m+3 =
// Y(2mx, my), Y(2mx+1, my), Cb(mx, my), Cr(mx, my); there are ceil(H/8) MCU rows.  The u8 planes between the
// inverse DCT and the upsampling have the padded extents: Y [padded_h][padded_w], Cb / Cr [padded_h][padded_w / 2].
JC_HD int mcus_per_row(int W) { return (W + 15) >> 4; }
JC_HD int block_rows(int H) { return (H + 7) >> 3; }
JC_HD int padded_w(int W) { return mcus_per_row(W) * 16; }
JC_HD int padded_h(int H) { return block_rows(H) * 8; }
JC_HD int blocks_per_image(int H, int W) { return block_rows(H) * mcus_per_row(W) * 4; }
JC_HD bool whole_mcus(int H, int W) { return H % 8 == 0 && W % 16 == 0; }
// luminance block bx of a row lies wholly outside the component: a dummy block
JC_HD bool dummy_block(int comp, int bx, int W) { return comp == 0 && bx * 8 >= W; }

// One block of the encoder: samples -> forward DCT -> quantised natural-order coefficients in d.  A dummy block
// repeats the quantised DC of the luminance block before it and has no AC.
JC_HD void encode_block_coefs(const float* x, int H, int W, int comp, int bx, int by, const uint16_t* q, int* d) {
    const bool dummy = dummy_block(comp, bx, W);
    sample_block(x, H, W, comp, dummy ? bx - 1 : bx, by, d);
    fdct_islow(d);
    quantize(d, q);
    if (dummy) {
#pragma unroll
        for (int i = 1; i < 64; ++i) d[i] = 0;
    }
}
// the previous block of the same component in scan order (its DC is the predictor), or -1 for the first
JC_HD int dc_predecessor(int blk) {
    const int slot = blk & 3;
    if (slot == 1) return blk - 1;
    if (blk < 4) return -1;
    return slot == 0 ? blk - 3 : blk - 4;
}

// jdsample.c h2v1_fancy_upsample: chroma for output columns 2i and 2i+1 from a row of cw real samples; a row of
// one or two samples is replicated (h2v1_upsample, which jinit_upsampler picks for downsampled_width <= 2)
JC_HD void upsample_pair(const uint8_t* c, int cw, int i, int& even, int& odd) {
    const int v = c[i];
    if (cw <= 2) {
        even = odd = v;
        return;
    }
    even = i == 0 ? v : (3 * v + c[i - 1] + 1) >> 2;
    odd = i == cw - 1 ? v : (3 * v + c[i + 1] + 2) >> 2;
}

// ---------------------------------------------------------------------------------------------- entropy coding
JC_HD int bit_length(int v) {  // v >= 0
    int n = 0;
    while (v) {
        ++n;
        v >>= 1;
    }
    return n;
}

// jchuff.c encode_one_block: zz = 64 quantised coefficients in zigzag order, pred = the previous DC of the
// component, tbl = 0 luminance / 1 chrominance.  sink.put(bits, n) appends the low n (<= 27) bits, MSB first.
template <class Sink>
JC_HD void encode_block(const int16_t* zz, int pred, const HuffTables& T, int tbl, Sink& sink) {
    int v = (int)zz[0] - pred;
    int v2 = v;
    if (v < 0) {
        v = -v;
        --v2;
    }
    int n = bit_length(v);
    sink.put(((uint32_t)T.dc_code[tbl][n] << n) | ((uint32_t)v2 & ((1u << n) - 1u)), T.dc_size[tbl][n] + n);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        v = zz[k];
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            sink.put(T.ac_code[tbl][0xF0], T.ac_size[tbl][0xF0]);
            run -= 16;
        }
        v2 = v;
        if (v < 0) {
            v = -v;
            --v2;
        }
        n = bit_length(v);
        const int sym = (run << 4) + n;
        sink.put(((uint32_t)T.ac_code[tbl][sym] << n) | ((uint32_t)v2 & ((1u << n) - 1u)), T.ac_size[tbl][sym] + n);
        run = 0;
    }
    if (run > 0) sink.put(T.ac_code[tbl][0], T.ac_size[tbl][0]);
}

struct CountSink {
    int bits = 0;
    JC_HD void put(uint32_t, int n) { bits += n; }
};

// ---------------------------------------------------------------------------------------------- entropy decoding
// Self-synchronising parallel Huffman decoder (Klein & Wiseman 2003; Weissenberger & Schmidt 2018).  The unstuffed
// entropy segment of an image is cut into subsequences of sub_bits bits; one thread (device) or loop iteration
// (host twin) owns a subsequence.  The decoder state between two symbols is (p, c, z): bit position, block-in-MCU
// 0..3 (0, 1 luminance tables / component Y, 2 Cb, 3 Cr) and the next zigzag index 0..63.
//   round 0   every subsequence i > 0 decodes from its first bit with the guess (c, z) = (0, 0), subsequence 0 from
//             the true start, until the next symbol would start in the following subsequence; it records its exit;
//   round k   subsequence i decodes again from subsequence i-1's exit of round k-1 (two exit buffers, swapped per
//             round) and reports whether its own exit changed.  A subsequence whose entry did not change in the
//             previous round keeps its exit without decoding.  Subsequences 0..k are exact after round k, so at
//             most nsub-1 rounds run; a round in which no exit changed ends the loop early;
//   write     exclusive scan of the blocks completed per subsequence, then one more decode per subsequence from
//             the settled entry that stores every coefficient slot (zeros of runs, EOB fills and ZRLs included)
//             exactly once.  DC slots hold the difference; dc_scan_component turns them into values.
// decode_symbol is total: any 32 bits at any (c, z) give a next state, consume 2..26 bits and index inside the
// tables; an invalid code or a run past index 63 sets the error flag.  Speculative rounds feed it garbage.

// libjpeg's jpeg_make_d_derived_tbl for the Annex K tables: t = 0 DC luminance, 1 DC chrominance, 2 AC luminance,
// 3 AC chrominance.  lut: the next 8 bits -> (code length << 8) | symbol, or 0 where the code is longer than 8 bits.
struct DecTables {
    uint16_t lut[4][256];
    int32_t maxcode[4][17];    // largest code of length l, or -1
    int32_t valoffset[4][17];  // vals index of the first code of length l, minus that code
    uint8_t vals[4][256];      // symbols in code order, zero padded: any 8-bit index is inside
};

constexpr DecTables make_dec_tables() {
    DecTables t{};
    for (int k = 0; k < 4; ++k) {
        const int c = k & 1, ac = k >> 1;
        const uint8_t* bits = ac ? kAcBits[c] : kDcBits[c];
        int code = 0, p = 0;
        for (int l = 1; l <= 16; ++l) {
            t.valoffset[k][l] = p - code;
            for (int i = 0; i < bits[l - 1]; ++i, ++p, ++code) {
                const uint8_t sym = ac ? kAcVals[c][p] : kDcVals[p];
                t.vals[k][p] = sym;
                if (l <= 8)
                    for (int f = 0; f < (1 << (8 - l)); ++f)
                        t.lut[k][(code << (8 - l)) | f] = (uint16_t)((l << 8) | sym);
            }
            t.maxcode[k][l] = bits[l - 1] ? code - 1 : -1;
            code <<= 1;
        }
    }
    return t;
}

// MSB-first reader over the unstuffed segment; bits past the end read as ones (the padding value)
struct BitReader {
    const uint8_t* bytes;
    uint32_t nbytes;
    JC_HD uint32_t word(uint32_t w) const {
        const uint32_t o = w * 4u;
        if (o + 4u <= nbytes) {
            uint32_t v;
            __builtin_memcpy(&v, bytes + o, 4);
            return __builtin_bswap32(v);
        }
        uint32_t v = 0xFFFFFFFFu;
        for (uint32_t j = 0; j < 4u; ++j)
            if (o + j < nbytes) v = (v & ~(0xFFu << (24 - 8 * j))) | ((uint32_t)bytes[o + j] << (24 - 8 * j));
        return v;
    }
    // bits p .. p+31
    JC_HD uint32_t peek(uint32_t p) const {
        const uint32_t w = p >> 5, sh = p & 31u;
        const uint32_t hi = word(w);
        return sh ? (hi << sh) | (word(w + 1u) >> (32u - sh)) : hi;
    }
};

constexpr uint32_t kSymError = 1u, kSymBlockDone = 2u;

// One symbol at bit p in state cz = c * 64 + z.  WRITE: its coefficients go to blk[z ..] (64 zigzag slots of the
// current block; NULL when that block lies past the image).  Returns kSymError | kSymBlockDone flags.
template <bool WRITE>
JC_HD uint32_t decode_symbol(const DecTables& T, const BitReader& R, uint32_t& p, uint32_t& cz, int16_t* blk) {
    const uint32_t c = (cz >> 6) & 3u;
    int z = (int)(cz & 63u);
    const int t = (z ? 2 : 0) + (c >> 1);
    const uint32_t w = R.peek(p);
    uint32_t flags = 0;
    int len, sym;
    const uint32_t e = T.lut[t][w >> 24];
    if (e) {
        len = (int)(e >> 8);
        sym = (int)(e & 255u);
    } else {
        len = 9;
        while (len <= 16 && (int32_t)(w >> (32 - len)) > T.maxcode[t][len]) ++len;
        if (len > 16) {  // no such code
            len = 16;
            sym = 0;
            flags = kSymError;
        } else {
            sym = T.vals[t][((int32_t)(w >> (32 - len)) + T.valoffset[t][len]) & 255];
        }
    }
    const int s = sym & 15;  // magnitude category: <= 11 for DC, <= 10 for AC in the Annex K tables
    int v = 0;
    if (s) {
        v = (int)((w << len) >> (32 - s));
        if (v < (1 << (s - 1))) v -= (1 << s) - 1;
    }
    p += (uint32_t)(len + s);
    if (z == 0) {
        if (WRITE && blk) blk[0] = (int16_t)v;
        z = 1;
    } else if (s == 0) {
        const int end = (sym >> 4) == 15 ? z + 16 : 64;  // ZRL, else EOB
        if (end > 64) flags |= kSymError;
        if (WRITE && blk)
            for (int k = z; k < (end < 64 ? end : 64); ++k) blk[k] = 0;
        z = end;
    } else {
        const int at = z + (sym >> 4);
        if (at > 63) flags |= kSymError;
        if (WRITE && blk) {
            for (int k = z; k < (at < 64 ? at : 64); ++k) blk[k] = 0;
            if (at <= 63) blk[at] = (int16_t)v;
        }
        z = at + 1;
    }
    if (z >= 64) {
        cz = ((c + 1u) & 3u) << 6;
        flags |= kSymBlockDone;
    } else {
        cz = (c << 6) | (uint32_t)z;
    }
    return flags;
}

// exit of a subsequence: p, and w = cz (bits 0..7) | error (8) | exit changed in this round (9) | n << 16, n = the
// blocks completed by symbols that started in the subsequence (<= sub_bits / 4 + 1 < 65536)
struct SubExit {
    uint32_t p, w;
};
constexpr uint32_t kExitError = 1u << 8, kExitChanged = 1u << 9;
constexpr int kMinSubBits = 32, kMaxSubBits = 8192, kDefaultSubBits = 512;

JC_HD int sub_count(uint32_t total_bits, int sub_bits) { return (int)((total_bits + (uint32_t)sub_bits - 1u) / (uint32_t)sub_bits); }

// decodes the symbols that start in subsequence i from the entry (p, cz).  WRITE: first = the index of the block
// open at the entry, coef = the image's [nb][64] coefficients.
template <bool WRITE>
JC_HD SubExit decode_subsequence(const DecTables& T, const BitReader& R, int i, int sub_bits, uint32_t total_bits,
                                 uint32_t p, uint32_t cz, int16_t* coef, int first, int nb) {
    const uint32_t lim = (uint32_t)(i + 1) * (uint32_t)sub_bits;
    const uint32_t end = lim < total_bits ? lim : total_bits;
    uint32_t err = 0, n = 0;
    while (p < end) {
        // fewer than 8 one-bits up to the end of the segment are the padding, not a symbol (no code is all ones)
        const uint32_t left = total_bits - p;
        if (left < 8u && (R.peek(p) >> (32u - left)) == (1u << left) - 1u) break;
        int16_t* blk = nullptr;
        if (WRITE && first + (int)n < nb) blk = coef + (long long)(first + (int)n) * 64;
        const uint32_t f = decode_symbol<WRITE>(T, R, p, cz, blk);
        err |= f & kSymError;
        n += (f >> 1) & 1u;
    }
    return SubExit{p, cz | (err ? kExitError : 0u) | (n << 16)};
}

JC_HD SubExit sync_round0(const DecTables& T, const BitReader& R, int i, int sub_bits, uint32_t total_bits) {
    SubExit e = decode_subsequence<false>(T, R, i, sub_bits, total_bits, (uint32_t)i * (uint32_t)sub_bits, 0u, nullptr,
                                          0, 0);
    e.w |= kExitChanged;
    return e;
}

// round k >= 1 of subsequence i: rd = the exits of round k-1, wr = this round's.  Returns whether the exit changed.
JC_HD bool sync_round(const DecTables& T, const BitReader& R, int i, int sub_bits, uint32_t total_bits,
                      const SubExit* rd, SubExit* wr) {
    SubExit mine = rd[i];
    mine.w &= ~kExitChanged;
    if (i == 0 || !(rd[i - 1].w & kExitChanged)) {  // the same entry as in the previous round
        wr[i] = mine;
        return false;
    }
    const SubExit in = rd[i - 1];
    SubExit e = decode_subsequence<false>(T, R, i, sub_bits, total_bits, in.p, in.w & 255u, nullptr, 0, 0);
    const bool changed = e.p != mine.p || ((e.w ^ mine.w) & 255u);
    if (changed) e.w |= kExitChanged;
    wr[i] = e;
    return changed;
}

JC_HD void write_subsequence(const DecTables& T, const BitReader& R, int i, int sub_bits, uint32_t total_bits,
                             const SubExit* ex, int first, int16_t* coef, int nb) {
    const uint32_t p = i ? ex[i - 1].p : 0u, cz = i ? ex[i - 1].w & 255u : 0u;
    decode_subsequence<true>(T, R, i, sub_bits, total_bits, p, cz, coef, first, nb);
}

constexpr int kStBadMarker = 1, kStBadSymbol = 2, kStBlockCount = 4, kStBadEnd = 8, kStTooLong = 16;

// validity of a decoded image: last = the final subsequence's exit (nsub > 0), blocks = the blocks completed
JC_HD int decode_status(const BitReader& R, uint32_t total_bits, int nsub, SubExit last, int blocks, int nb,
                        bool sym_error, bool marker_error) {
    int st = marker_error ? kStBadMarker : 0;
    if (sym_error) st |= kStBadSymbol;
    if (nsub <= 0) return st | kStBlockCount | kStBadEnd;
    if (blocks != nb || (last.w & 255u) != 0u) st |= kStBlockCount;
    // the final position lies within the last byte and the padding bits up to its end are ones
    if (last.p > total_bits || last.p + 8u <= total_bits) {
        st |= kStBadEnd;
    } else {
        const uint32_t k = total_bits - last.p;
        if (k && (R.peek(last.p) >> (32u - k)) != (1u << k) - 1u) st |= kStBadEnd;
    }
    return st;
}

// Unstuffing: in an entropy segment every 0xFF is followed by a 0x00 that is dropped; anything else after a 0xFF
// (a marker), or a 0xFF as the last byte, is an error.  prev = the byte before cur (0 for the first byte).
JC_HD bool ff_dropped(int prev, int cur) { return prev == 0xFF && cur == 0; }
JC_HD bool ff_error(int prev, int cur, bool last) { return (prev == 0xFF && cur != 0) || (last && cur == 0xFF); }

// inclusive scan of the DC differences of one component in scan order: Y = blocks 4m, 4m+1, Cb 4m+2, Cr 4m+3.
// seq = the block's index within its component.
JC_HD int dc_block_of(int comp, int seq) { return comp == 0 ? (seq >> 1) * 4 + (seq & 1) : seq * 4 + comp + 1; }
JC_HD int dc_blocks_of(int comp, int nb) { return comp == 0 ? nb / 2 : nb / 4; }

// IDCT of one block from its zigzag coefficients: * the file's quantiser (natural order) -> samples 0..255 in d
JC_HD void coef_block_to_samples(const int16_t* zz, const uint16_t* q, int* d) {
#pragma unroll
    for (int k = 0; k < 64; ++k) d[kNatural[k]] = zz[k];
    dequant_idct(d, q);
}

// ---------------------------------------------------------------------------------------------- host side
// the 623-byte header Pillow / libjpeg write for this configuration (quant tables in zigzag order)
inline void build_header(const uint8_t lum[64], const uint8_t chr[64], int H, int W, uint8_t* out) {
    uint8_t* p = out;
    auto put = [&](int v) { *p++ = (uint8_t)v; };
    auto put2 = [&](int v) { put(v >> 8); put(v & 255); };
    put2(0xFFD8);
    put2(0xFFE0); put2(16);
    for (int v : {0x4A, 0x46, 0x49, 0x46, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0}) put(v);  // "JFIF" 1.01, 1:1
    for (int c = 0; c < 2; ++c) {
        put2(0xFFDB); put2(67); put(c);
        for (int k = 0; k < 64; ++k) put((c ? chr : lum)[k]);
    }
    put2(0xFFC0); put2(17); put(8); put2(H); put2(W); put(3);
    put(1); put(0x21); put(0);
    put(2); put(0x11); put(1);
    put(3); put(0x11); put(1);
    for (int c = 0; c < 2; ++c) {
        put2(0xFFC4); put2(2 + 1 + 16 + 12); put(c);
        for (int i = 0; i < 16; ++i) put(kDcBits[c][i]);
        for (int i = 0; i < 12; ++i) put(kDcVals[i]);
        put2(0xFFC4); put2(2 + 1 + 16 + 162); put(0x10 | c);
        for (int i = 0; i < 16; ++i) put(kAcBits[c][i]);
        for (int i = 0; i < 162; ++i) put(kAcVals[c][i]);
    }
    put2(0xFFDA); put2(12); put(3);
    put(1); put(0x00); put(2); put(0x11); put(3); put(0x11);
    put(0); put(63); put(0);
}

// appends entropy-coded bits to a byte vector with 0xFF stuffing (jchuff.c emit_bits / flush_bits)
struct ByteSink {
    std::vector<uint8_t>* out;
    uint64_t acc = 0;
    int fill = 0;
    void emit(int b) {
        out->push_back((uint8_t)b);
        if (b == 0xFF) out->push_back(0);
    }
    void put(uint32_t bits, int n) {
        acc = (acc << n) | bits;
        fill += n;
        while (fill >= 8) {
            emit((int)((acc >> (fill - 8)) & 0xFF));
            fill -= 8;
        }
    }
    void flush() {
        if (fill > 0) put((1u << (8 - fill)) - 1u, 8 - fill);  // pad the last byte with 1-bits
    }
};

// u8 Y [padded_h][padded_w] and Cb / Cr [padded_h][padded_w / 2] planes -> fancy upsample over the ceil(W/2) real
// chroma samples, colour, / 255 into planar [3][H][W] (plane 0 = B); for odd W the last pair's second sample is dropped
inline void planes_to_pixels_host(const uint8_t* yp, const uint8_t* cbp, const uint8_t* crp, int H, int W,
                                  float* decoded) {
    const int cw = (W + 1) / 2, pw = padded_w(W), pcw = pw / 2;
    const size_t plane = (size_t)H * W;
    for (int r = 0; r < H; ++r)
        for (int i = 0; i < cw; ++i) {
            int cb[2], cr[2];
            upsample_pair(cbp + (size_t)r * pcw, cw, i, cb[0], cb[1]);
            upsample_pair(crp + (size_t)r * pcw, cw, i, cr[0], cr[1]);
            for (int h = 0; h < 2 && 2 * i + h < W; ++h) {
                int R, G, B;
                const size_t o = (size_t)r * W + 2 * i + h;
                ycc_to_rgb(yp[(size_t)r * pw + 2 * i + h], cb[h], cr[h], R, G, B);
                decoded[o] = (float)B / 255.0f;
                decoded[plane + o] = (float)G / 255.0f;
                decoded[2 * plane + o] = (float)R / 255.0f;
            }
        }
}

// Encode -> decode of one image on the host.  x planar [3][H][W] (plane 0 = B); decoded the same layout;
// file (optional) receives the complete JPEG file.  Returns the file's byte count.
inline int roundtrip_image_host(const float* x, int H, int W, int quality, float* decoded,
                                std::vector<uint8_t>* file) {
    static const HuffTables T = make_huff_tables();
    const QuantTables Q = quant_tables_natural(quality);
    const int nb = blocks_per_image(H, W), mw = mcus_per_row(W), ph = padded_h(H), ypw = padded_w(W), cw = ypw / 2;
    std::vector<int16_t> coef((size_t)nb * 64);
    std::vector<uint8_t> yp((size_t)ph * ypw), cp[2];
    cp[0].resize((size_t)ph * cw);
    cp[1].resize((size_t)ph * cw);
    int d[64];
    for (int blk = 0; blk < nb; ++blk) {
        const int m = blk >> 2, slot = blk & 3, mx = m % mw, my = m / mw;
        const int comp = slot < 2 ? 0 : slot - 1, bx = slot < 2 ? 2 * mx + slot : mx;
        const uint16_t* q = Q.q[comp ? 1 : 0];
        encode_block_coefs(x, H, W, comp, bx, my, q, d);
        for (int k = 0; k < 64; ++k) coef[(size_t)blk * 64 + k] = (int16_t)d[kNatural[k]];
        dequant_idct(d, q);
        uint8_t* plane = comp ? cp[comp - 1].data() : yp.data();
        const int pw = comp ? cw : ypw;
        for (int r = 0; r < 8; ++r)
            for (int c = 0; c < 8; ++c) plane[(size_t)(my * 8 + r) * pw + bx * 8 + c] = (uint8_t)d[r * 8 + c];
    }
    planes_to_pixels_host(yp.data(), cp[0].data(), cp[1].data(), H, W, decoded);
    std::vector<uint8_t> local;
    std::vector<uint8_t>& f = file ? *file : local;
    f.clear();
    f.resize(kHeaderBytes);
    uint8_t z[2][64];
    quant_tables_zigzag(quality, z[0], z[1]);
    build_header(z[0], z[1], H, W, f.data());
    ByteSink sink{&f};
    for (int blk = 0; blk < nb; ++blk) {
        const int pb = dc_predecessor(blk);
        encode_block(coef.data() + (size_t)blk * 64, pb < 0 ? 0 : coef[(size_t)pb * 64], T, (blk & 3) < 2 ? 0 : 1,
                     sink);
    }
    sink.flush();
    f.push_back(0xFF);
    f.push_back(0xD9);
    return (int)f.size();
}

// What the device decoder needs from a file's marker segments
struct FileInfo {
    int H, W;
    long long scan_off, scan_len;  // the entropy-coded segment: after the SOS header, before the trailing EOI
    uint8_t qtab[2][64];           // luminance / chrominance quantiser, zigzag order
};

// Parses the marker segments of a JPEG file.  Returns NULL when the decoder takes the file (baseline 8-bit 4:2:2,
// three components in one interleaved scan, the Annex K Huffman tables, no restart interval; APPn / COM segments
// anywhere; whole MCUs unless any_size), else the reason it does not.
inline const char* parse_file(const uint8_t* f, size_t n, FileInfo* info, bool any_size = false) {
    if (n < 4 || f[0] != 0xFF || f[1] != 0xD8) return "not a JPEG file (no SOI)";
    uint8_t qt[4][64];
    bool have_qt[4] = {false, false, false, false}, have_ht[2][2] = {{false, false}, {false, false}}, sof = false;
    int ids[3] = {0, 0, 0}, tq[3] = {0, 0, 0};
    size_t i = 2;
    for (;;) {
        if (i + 4 > n) return "truncated before the scan";
        if (f[i] != 0xFF) return "marker expected";
        const int m = f[i + 1];
        if (m == 0xFF) {  // fill byte
            ++i;
            continue;
        }
        const size_t len = ((size_t)f[i + 2] << 8) | f[i + 3];
        if (len < 2 || i + 2 + len > n) return "marker segment runs past the file";
        const uint8_t* p = f + i + 4;
        const size_t body = len - 2;
        if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {
            // APPn / COM
        } else if (m == 0xDB) {
            for (size_t o = 0; o < body; o += 65) {
                if (o + 65 > body) return "malformed DQT";
                if (p[o] >> 4) return "16-bit quantisation table";
                if ((p[o] & 15) > 3) return "malformed DQT";
                for (int k = 0; k < 64; ++k) qt[p[o] & 15][k] = p[o + 1 + k];
                have_qt[p[o] & 15] = true;
            }
        } else if (m == 0xC4) {
            for (size_t o = 0; o < body;) {
                if (o + 17 > body) return "malformed DHT";
                const int tc = p[o] >> 4, th = p[o] & 15;
                size_t cnt = 0;
                for (int k = 0; k < 16; ++k) cnt += p[o + 1 + k];
                if (o + 17 + cnt > body) return "malformed DHT";
                if (tc > 1 || th > 1) return "Huffman table id outside 0..1";
                const uint8_t* bits = tc ? kAcBits[th] : kDcBits[th];
                const uint8_t* vals = tc ? kAcVals[th] : kDcVals;
                if (cnt != (tc ? 162u : 12u)) return "Huffman tables other than Annex K (optimised coding)";
                for (int k = 0; k < 16; ++k)
                    if (p[o + 1 + k] != bits[k]) return "Huffman tables other than Annex K (optimised coding)";
                for (size_t k = 0; k < cnt; ++k)
                    if (p[o + 17 + k] != vals[k]) return "Huffman tables other than Annex K (optimised coding)";
                have_ht[tc][th] = true;
                o += 17 + cnt;
            }
        } else if (m == 0xC0) {
            if (sof) return "two frame headers";
            if (body < 6) return "malformed SOF0";
            if (p[0] != 8) return "sample precision other than 8 bits";
            info->H = (p[1] << 8) | p[2];
            info->W = (p[3] << 8) | p[4];
            if (p[5] != 3) return "not three components (grey or CMYK)";
            if (body != 15) return "malformed SOF0";
            for (int c = 0; c < 3; ++c) {
                ids[c] = p[6 + 3 * c];
                if (p[7 + 3 * c] != (c ? 0x11 : 0x21)) return "chroma subsampling other than 4:2:2 (2x1, 1x1, 1x1)";
                tq[c] = p[8 + 3 * c];
                if (tq[c] > 3) return "malformed SOF0";
            }
            if (info->H <= 0 || info->W <= 0) return "zero height or width";
            if (!any_size && !whole_mcus(info->H, info->W)) return "size is not whole MCUs (H % 8 == 0, W % 16 == 0)";
            sof = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC8) {
            return m == 0xC2 ? "progressive file" : "not a baseline (SOF0) file";
        } else if (m == 0xDD) {
            if (body != 2) return "malformed DRI";
            if (p[0] || p[1]) return "restart interval";
        } else if (m == 0xDA) {
            if (!sof) return "scan before the frame header";
            if (body < 1 || p[0] != 3) return "not one interleaved scan of three components";
            if (body != 10) return "malformed SOS";
            for (int c = 0; c < 3; ++c) {
                if (p[1 + 2 * c] != ids[c]) return "scan components out of frame order";
                if (p[2 + 2 * c] != (c ? 0x11 : 0x00)) return "Huffman table selectors other than 0/0, 1/1, 1/1";
            }
            if (p[7] != 0 || p[8] != 63 || p[9] != 0) return "not a sequential scan (Ss = 0, Se = 63, Ah = Al = 0)";
            if (!(have_ht[0][0] && have_ht[0][1] && have_ht[1][0] && have_ht[1][1])) return "missing Huffman table";
            if (!(have_qt[tq[0]] && have_qt[tq[1]] && have_qt[tq[2]])) return "missing quantisation table";
            for (int k = 0; k < 64; ++k)
                if (qt[tq[1]][k] != qt[tq[2]][k]) return "Cb and Cr use different quantisation tables";
            for (int k = 0; k < 64; ++k) {
                info->qtab[0][k] = qt[tq[0]][k];
                info->qtab[1][k] = qt[tq[1]][k];
                if (!qt[tq[0]][k] || !qt[tq[1]][k]) return "zero quantisation step";
            }
            info->scan_off = (long long)(i + 2 + len);
            if (n < (size_t)info->scan_off + 2 || f[n - 2] != 0xFF || f[n - 1] != 0xD9) return "no EOI at the end of the file";
            info->scan_len = (long long)n - 2 - info->scan_off;
            return nullptr;
        } else {
            return "unexpected marker before the scan";
        }
        i += 2 + len;
    }
}

inline int unstuffed_capacity(long long scan_capacity) { return (int)((scan_capacity + 8 + 255) & ~255LL); }

// The host twin of the device decoder for one image: the same unstuffing rule, symbol step, rounds, write pass, DC
// scan and IDCT, with a plain loop over subsequences where the kernel has threads.  scan = the raw entropy segment.
// Returns the status (0 = valid); decoded planar [3][H][W] (zeros when the status is not 0).
inline int decode_image_host(const uint8_t* scan, long long scan_len, long long capacity, const uint8_t qz[2][64],
                             int H, int W, int sub_bits, float* decoded, int* rounds_out) {
    static const DecTables T = make_dec_tables();
    const int nb = blocks_per_image(H, W), ph = padded_h(H), ypw = padded_w(W), cw = ypw / 2;
    bool marker_error = false;
    int extra = 0;
    if (scan_len < 0) scan_len = 0;
    if (scan_len > capacity) {
        scan_len = capacity;
        extra = kStTooLong;
    }
    std::vector<uint8_t> u;
    u.reserve((size_t)scan_len);
    for (long long k = 0; k < scan_len; ++k) {
        const int prev = k ? scan[k - 1] : 0, cur = scan[k];
        marker_error |= ff_error(prev, cur, k == scan_len - 1);
        if (!ff_dropped(prev, cur)) u.push_back((uint8_t)cur);
    }
    const BitReader R{u.data(), (uint32_t)u.size()};
    const uint32_t total_bits = (uint32_t)u.size() * 8u;
    const int nsub = sub_count(total_bits, sub_bits);
    std::vector<SubExit> a((size_t)nsub), b((size_t)nsub);
    SubExit *cur = a.data(), *nxt = b.data();
    for (int i = 0; i < nsub; ++i) cur[i] = sync_round0(T, R, i, sub_bits, total_bits);
    int rounds = 0;
    for (int r = 1; r < nsub; ++r) {
        bool changed = false;
        for (int i = 0; i < nsub; ++i) changed |= sync_round(T, R, i, sub_bits, total_bits, cur, nxt);
        ++rounds;
        std::swap(cur, nxt);
        if (!changed) break;
    }
    if (rounds_out) *rounds_out = rounds;
    std::vector<int16_t> coef((size_t)nb * 64);
    int blocks = 0;
    bool sym_error = false;
    for (int i = 0; i < nsub; ++i) {
        write_subsequence(T, R, i, sub_bits, total_bits, cur, blocks, coef.data(), nb);
        blocks += (int)(cur[i].w >> 16);
        sym_error |= (cur[i].w & kExitError) != 0;
    }
    const int status = extra | decode_status(R, total_bits, nsub, nsub ? cur[nsub - 1] : SubExit{0, 0}, blocks, nb,
                                             sym_error, marker_error);
    if (status) {
        for (size_t k = 0; k < (size_t)3 * H * W; ++k) decoded[k] = 0.0f;
        return status;
    }
    for (int comp = 0; comp < 3; ++comp) {
        uint32_t dc = 0;
        for (int s = 0; s < dc_blocks_of(comp, nb); ++s) {
            int16_t& slot = coef[(size_t)dc_block_of(comp, s) * 64];
            dc += (uint32_t)(int)slot;
            slot = (int16_t)(uint16_t)dc;
        }
    }
    uint16_t q[2][64];
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 64; ++k) q[c][kNatural[k]] = qz[c][k];
    std::vector<uint8_t> yp((size_t)ph * ypw), cp[2];
    cp[0].resize((size_t)ph * cw);
    cp[1].resize((size_t)ph * cw);
    const int mw = mcus_per_row(W);
    int d[64];
    for (int blk = 0; blk < nb; ++blk) {
        const int m = blk >> 2, slot = blk & 3, mx = m % mw, my = m / mw;
        const int comp = slot < 2 ? 0 : slot - 1, bx = slot < 2 ? 2 * mx + slot : mx;
        coef_block_to_samples(coef.data() + (size_t)blk * 64, q[comp ? 1 : 0], d);
        uint8_t* plane = comp ? cp[comp - 1].data() : yp.data();
        const int pw = comp ? cw : ypw;
        for (int r = 0; r < 8; ++r)
            for (int c = 0; c < 8; ++c) plane[(size_t)(my * 8 + r) * pw + bx * 8 + c] = (uint8_t)d[r * 8 + c];
    }
    planes_to_pixels_host(yp.data(), cp[0].data(), cp[1].data(), H, W, decoded);
    return 0;
}

}  // namespace jpeg
}  // namespace hyres
