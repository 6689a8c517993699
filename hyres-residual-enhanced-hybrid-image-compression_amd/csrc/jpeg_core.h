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
// Images are whole MCUs (H % 8 == 0, W % 16 == 0): no edge replication, no dummy blocks.
#pragma once
#include <stddef.h>
#include <stdint.h>

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
// 2:1 horizontally with libjpeg's h2v1 bias (0 on even output columns, 1 on odd ones).
JC_HD void sample_block(const float* x, int H, int W, int comp, int bx, int by, int* d) {
    const long long plane = (long long)H * W;
    if (comp == 0) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float* p = x + (long long)(by * 8 + r) * W + bx * 8;
#pragma unroll
            for (int c = 0; c < 8; ++c)
                d[r * 8 + c] = rgb_to_y(to_byte(p[2 * plane + c]), to_byte(p[plane + c]), to_byte(p[c])) - 128;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float* p = x + (long long)(by * 8 + r) * W + bx * 16;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                int v[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int i = 2 * c + h;
                    const int R = to_byte(p[2 * plane + i]), G = to_byte(p[plane + i]), B = to_byte(p[i]);
                    v[h] = comp == 1 ? rgb_to_cb(R, G, B) : rgb_to_cr(R, G, B);
                }
                d[r * 8 + c] = ((v[0] + v[1] + (c & 1)) >> 1) - 128;
            }
        }
    }
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
// Blocks of one image are numbered in scan order: MCU m = my * (W/16) + mx holds blocks 4m .. 4m+3 =
// Y(2mx, my), Y(2mx+1, my), Cb(mx, my), Cr(mx, my).
JC_HD int blocks_per_image(int H, int W) { return (H / 8) * (W / 16) * 4; }
// the previous block of the same component in scan order (its DC is the predictor), or -1 for the first
JC_HD int dc_predecessor(int blk) {
    const int slot = blk & 3;
    if (slot == 1) return blk - 1;
    if (blk < 4) return -1;
    return slot == 0 ? blk - 3 : blk - 4;
}

// jdsample.c h2v1_fancy_upsample: chroma for output columns 2i and 2i+1 from a row of cw samples
JC_HD void upsample_pair(const uint8_t* c, int cw, int i, int& even, int& odd) {
    const int v = c[i];
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

// Encode -> decode of one image on the host.  x planar [3][H][W] (plane 0 = B); decoded the same layout;
// file (optional) receives the complete JPEG file.  Returns the file's byte count.
inline int roundtrip_image_host(const float* x, int H, int W, int quality, float* decoded,
                                std::vector<uint8_t>* file) {
    static const HuffTables T = make_huff_tables();
    const QuantTables Q = quant_tables_natural(quality);
    const int nb = blocks_per_image(H, W), mw = W / 16, cw = W / 2;
    std::vector<int16_t> coef((size_t)nb * 64);
    std::vector<uint8_t> yp((size_t)H * W), cp[2];
    cp[0].resize((size_t)H * cw);
    cp[1].resize((size_t)H * cw);
    int d[64];
    for (int blk = 0; blk < nb; ++blk) {
        const int m = blk >> 2, slot = blk & 3, mx = m % mw, my = m / mw;
        const int comp = slot < 2 ? 0 : slot - 1, bx = slot < 2 ? 2 * mx + slot : mx;
        const uint16_t* q = Q.q[comp ? 1 : 0];
        sample_block(x, H, W, comp, bx, my, d);
        fdct_islow(d);
        quantize(d, q);
        for (int k = 0; k < 64; ++k) coef[(size_t)blk * 64 + k] = (int16_t)d[kNatural[k]];
        dequant_idct(d, q);
        uint8_t* plane = comp ? cp[comp - 1].data() : yp.data();
        const int pw = comp ? cw : W;
        for (int r = 0; r < 8; ++r)
            for (int c = 0; c < 8; ++c) plane[(size_t)(my * 8 + r) * pw + bx * 8 + c] = (uint8_t)d[r * 8 + c];
    }
    const size_t plane = (size_t)H * W;
    for (int r = 0; r < H; ++r)
        for (int i = 0; i < cw; ++i) {
            int cb[2], cr[2];
            upsample_pair(cp[0].data() + (size_t)r * cw, cw, i, cb[0], cb[1]);
            upsample_pair(cp[1].data() + (size_t)r * cw, cw, i, cr[0], cr[1]);
            for (int h = 0; h < 2; ++h) {
                int R, G, B;
                const size_t o = (size_t)r * W + 2 * i + h;
                ycc_to_rgb(yp[o], cb[h], cr[h], R, G, B);
                decoded[o] = (float)B / 255.0f;
                decoded[plane + o] = (float)G / 255.0f;
                decoded[2 * plane + o] = (float)R / 255.0f;
            }
        }
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

}  // namespace jpeg
}  // namespace hyres
