// Device JPEG 4:2:2 base layer: encode -> decode round trip of a [B,3,H,W] fp32 batch on the
// stream, bit-exact with libjpeg-turbo (the arithmetic lives in jpeg_core.h, shared with the host round trip).
//
//   jpeg_blocks_kernel    one thread per 8x8 block: pixels -> bytes -> Y / downsampled Cb / Cr -> forward DCT ->
//                         quantise -> int16 zigzag coefficients [B][blocks][64] (scan order), and in the same pass
//                         dequantise -> inverse DCT -> u8 Y / Cb / Cr planes of the padded extents; blocks that reach
//                         past the image gather with clamped coordinates, a dummy block repeats its neighbour's DC
//   jpeg_decode_kernel    fancy h2v1 upsample + YCbCr -> BGR + /255 into the fp32 NCHW output of the true extents
//   jpeg_count_kernel     Huffman bit count per block (DC predicted from the previous block of the component)
//   jpeg_scan_kernel      exclusive scan of the bit counts per image -> every block's bit offset
//   jpeg_pack_kernel      each block's code words at its offset into a big-endian word buffer that
//                         jpeg_clear_kernel zeroed (atomicOr on the two words a block shares with its neighbours,
//                         plain stores between them)
//   jpeg_ff_count/scan/emit   count 0xFF bytes per 1 KiB chunk, scan, and write header + stuffed bytes + EOI and the
//                         per-image byte count
// No kernel syncs the host, allocates or copies to the host; every grid depends on the shape alone, so the round
// trip can be captured into a graph.
#include "common.h"
#include "jpeg_core.h"

#include <cstring>
#include <utility>
#include <vector>

namespace hyres {
namespace jpeg {

__constant__ HuffTables d_huff = make_huff_tables();

struct HeaderArg {
    uint8_t b[kHeaderBytes + 1];
};

constexpr int kThreads = 256;
constexpr int kChunkWords = kThreads;  // one stream word per thread: 1 KiB chunks

struct Layout {
    int nb, nwords, nchunks;
    long long coef, yp, cbp, crp, bits, total, words, ff, end;
};

static long long align256(long long v) { return (v + 255) & ~255LL; }

static Layout make_layout(int B, int H, int W) {
    Layout L;
    L.nb = blocks_per_image(H, W);
    const long long w = ((long long)L.nb * kMaxBlockBits) / 32 + 1;
    L.nchunks = (int)((w + kChunkWords - 1) / kChunkWords);
    L.nwords = L.nchunks * kChunkWords;
    long long o = 0;
    L.coef = o, o = align256(o + (long long)B * L.nb * 64 * 2);
    const long long pix = (long long)B * padded_h(H) * padded_w(W);  // the planes have the padded extents
    L.yp = o, o = align256(o + pix);
    L.cbp = o, o = align256(o + pix / 2);
    L.crp = o, o = align256(o + pix / 2);
    L.bits = o, o = align256(o + (long long)B * L.nb * 4);
    L.total = o, o = align256(o + (long long)B * 4);
    L.words = o, o = align256(o + (long long)B * L.nwords * 4);
    L.ff = o, o = align256(o + (long long)B * L.nchunks * 4);
    L.end = o;
    return L;
}

// exclusive scan of one value per thread over a 256-thread block; total = the block's sum
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int& total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const int t = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const int incl = sh[tid];
    total = sh[kThreads - 1];
    __syncthreads();
    return incl - v;
}

template <size_t... K>
__device__ __forceinline__ void store_zigzag(int16_t* o, const int* d, std::index_sequence<K...>) {
    // 32 packed pairs of zigzag-ordered coefficients, eight 16-byte stores
    const uint32_t w[32] = {((uint32_t)(uint16_t)d[kNatural[2 * K]] | ((uint32_t)(uint16_t)d[kNatural[2 * K + 1]] << 16))...};
#pragma unroll
    for (int g = 0; g < 8; ++g)
        reinterpret_cast<uint4*>(o)[g] = make_uint4(w[4 * g], w[4 * g + 1], w[4 * g + 2], w[4 * g + 3]);
}

// item i of an image: luminance blocks in raster order first (coalesced loads), then Cb, then Cr
__global__ __launch_bounds__(kThreads) void jpeg_blocks_kernel(const float* __restrict__ x, int B, int H, int W,
                                                              QuantTables Q, int16_t* __restrict__ coef,
                                                              uint8_t* __restrict__ yp, uint8_t* __restrict__ cbp,
                                                              uint8_t* __restrict__ crp) {
    __shared__ uint16_t q[128];
    if (threadIdx.x < 128) q[threadIdx.x] = Q.q[threadIdx.x >> 6][threadIdx.x & 63];
    __syncthreads();
    const int mw = mcus_per_row(W), nmcu = mw * block_rows(H), nb = 4 * nmcu;
    const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= (long long)B * nb) return;
    const int b = (int)(gid / nb), i = (int)(gid % nb);
    int comp, bx, by, blk;
    if (i < 2 * nmcu) {
        comp = 0, bx = i % (2 * mw), by = i / (2 * mw);
        blk = (by * mw + (bx >> 1)) * 4 + (bx & 1);
    } else {
        comp = i < 3 * nmcu ? 1 : 2;
        const int m = i - (comp + 1) * nmcu;
        bx = m % mw, by = m / mw;
        blk = m * 4 + comp + 1;
    }
    const uint16_t* qt = q + (comp ? 64 : 0);
    int d[64];
    encode_block_coefs(x + (long long)b * 3 * H * W, H, W, comp, bx, by, qt, d);
    store_zigzag(coef + ((long long)b * nb + blk) * 64, d, std::make_index_sequence<32>());
    dequant_idct(d, qt);
    const int pw = comp ? mw * 8 : mw * 16;
    uint8_t* plane = (comp == 0 ? yp : (comp == 1 ? cbp : crp)) + (long long)b * block_rows(H) * 8 * pw;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        uint32_t u[8];  // samples in 0..255
#pragma unroll
        for (int c = 0; c < 8; ++c) u[c] = (uint32_t)d[r * 8 + c];
        const uint32_t lo = u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24);
        const uint32_t hi = u[4] | (u[5] << 8) | (u[6] << 16) | (u[7] << 24);
        *reinterpret_cast<uint2*>(plane + (long long)(by * 8 + r) * pw + bx * 8) = make_uint2(lo, hi);
    }
}

// one thread per real chroma sample (ceil(W/2) a row): output columns 2i and 2i+1 of the three planes (plane 0 = B).
// The u8 planes have the padded extents ph x pw (= H x W for whole MCUs); column 2i+1 == W of an odd W is dropped.
__global__ __launch_bounds__(kThreads) void jpeg_decode_kernel(const uint8_t* __restrict__ yp,
                                                              const uint8_t* __restrict__ cbp,
                                                              const uint8_t* __restrict__ crp, int B, int H, int W,
                                                              int ph, int pw, float* __restrict__ out) {
    const int cw = (W + 1) / 2, pcw = pw / 2;
    const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= (long long)B * H * cw) return;
    const int i = (int)(gid % cw);
    const long long row = gid / cw;  // b * H + r
    const int b = (int)(row / H), r = (int)(row % H);
    const long long prow = (long long)b * ph + r;
    int cb[2], cr[2];
    upsample_pair(cbp + prow * pcw, cw, i, cb[0], cb[1]);
    upsample_pair(crp + prow * pcw, cw, i, cr[0], cr[1]);
    float v[3][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        int R, G, Bl;
        ycc_to_rgb(yp[prow * pw + 2 * i + h], cb[h], cr[h], R, G, Bl);  // 2i + 1 <= pw - 1: inside the padded row
        v[0][h] = __fdiv_rn((float)Bl, 255.0f);  // a true fp32 division, not a reciprocal multiply
        v[1][h] = __fdiv_rn((float)G, 255.0f);
        v[2][h] = __fdiv_rn((float)R, 255.0f);
    }
    const long long plane = (long long)H * W;
    float* o = out + (long long)b * 3 * plane + (long long)r * W + 2 * i;
    if (!(W & 1)) {  // uniform: every pair is whole and 8-byte aligned
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float2*>(o + c * plane) = make_float2(v[c][0], v[c][1]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[c * plane] = v[c][0];
            if (2 * i + 1 < W) o[c * plane + 1] = v[c][1];
        }
    }
}

__device__ __forceinline__ int pred_dc(const int16_t* coef_img, int blk) {
    const int pb = dc_predecessor(blk);
    return pb < 0 ? 0 : (int)coef_img[(long long)pb * 64];
}

__global__ __launch_bounds__(kThreads) void jpeg_count_kernel(const int16_t* __restrict__ coef, int B, int nb,
                                                             int* __restrict__ bits) {
    const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= (long long)B * nb) return;
    const int blk = (int)(gid % nb);
    const int16_t* img = coef + (gid - blk) * 64;
    CountSink s;
    encode_block(img + (long long)blk * 64, pred_dc(img, blk), d_huff, (blk & 3) < 2 ? 0 : 1, s);
    bits[gid] = s.bits;
}

// one work-group per image: bits[] -> exclusive bit offsets in place, total[b] = the image's bit count
__global__ __launch_bounds__(kThreads) void jpeg_scan_kernel(int* __restrict__ v, int n, int* __restrict__ total) {
    __shared__ int sh[kThreads];
    int* p = v + (long long)blockIdx.x * n;
    int carry = 0;
    for (int base = 0; base < n; base += kThreads) {
        const int i = base + threadIdx.x;
        const int x = i < n ? p[i] : 0;
        int sum;
        const int e = block_excl_scan(x, sh, sum);
        if (i < n) p[i] = carry + e;
        carry += sum;
    }
    if (threadIdx.x == 0) total[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kThreads) void jpeg_clear_kernel(uint4* __restrict__ p, long long n) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// MSB-first bit writer into 32-bit words: bit p of the stream is bit 31 - (p & 31) of word p >> 5
struct WordSink {
    uint32_t* w;
    uint64_t acc = 0;
    int fill;
    bool first = true;
    __device__ __forceinline__ WordSink(uint32_t* words, int bitpos) : w(words + (bitpos >> 5)), fill(bitpos & 31) {}
    __device__ __forceinline__ void put(uint32_t bits, int n) {
        acc |= (uint64_t)bits << (64 - fill - n);  // fill < 32, 1 <= n <= 27
        fill += n;
        if (fill >= 32) {
            const uint32_t word = (uint32_t)(acc >> 32);
            if (first) atomicOr(w, word);  // may share its leading bits with the previous block
            else *w = word;                // all 32 bits are this block's
            first = false;
            ++w;
            acc <<= 32;
            fill -= 32;
        }
    }
    __device__ __forceinline__ void flush() {
        if (fill > 0) atomicOr(w, (uint32_t)(acc >> 32));
    }
};

__global__ __launch_bounds__(kThreads) void jpeg_pack_kernel(const int16_t* __restrict__ coef, int B, int nb,
                                                            const int* __restrict__ offs, uint32_t* __restrict__ words,
                                                            int nwords) {
    const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= (long long)B * nb) return;
    const int blk = (int)(gid % nb);
    const int b = (int)(gid / nb);
    const int16_t* img = coef + (gid - blk) * 64;
    WordSink s(words + (long long)b * nwords, offs[gid]);
    encode_block(img + (long long)blk * 64, pred_dc(img, blk), d_huff, (blk & 3) < 2 ? 0 : 1, s);
    s.flush();
}

// the four stream bytes of word wi as values 0..255, or -1 past the end; the last byte is padded with 1-bits
__device__ __forceinline__ void stream_bytes(const uint32_t* words, int wi, int nbytes, int totalbits, int* by) {
    const uint32_t w = (long long)wi * 4 < nbytes ? words[wi] : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = wi * 4 + j;
        int v = (int)((w >> (24 - 8 * j)) & 255u);
        if (k == nbytes - 1) v |= (1 << (nbytes * 8 - totalbits)) - 1;
        by[j] = k < nbytes ? v : -1;
    }
}

__global__ __launch_bounds__(kThreads) void jpeg_ff_count_kernel(const uint32_t* __restrict__ words, int nwords,
                                                                const int* __restrict__ total, int nchunks,
                                                                int* __restrict__ ff) {
    __shared__ int sh[kThreads];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int totalbits = total[b], nbytes = (totalbits + 7) >> 3;
    if ((long long)chunk * kChunkWords * 4 >= nbytes) {  // uniform over the work-group
        if (threadIdx.x == 0) ff[b * nchunks + chunk] = 0;
        return;
    }
    int by[4];
    stream_bytes(words + (long long)b * nwords, chunk * kChunkWords + threadIdx.x, nbytes, totalbits, by);
    const int c = (by[0] == 255) + (by[1] == 255) + (by[2] == 255) + (by[3] == 255);
    int sum;
    block_excl_scan(c, sh, sum);
    if (threadIdx.x == 0) ff[b * nchunks + chunk] = sum;
}

// one work-group per image: chunk 0xFF counts -> exclusive offsets in place; sizes[b]; header and EOI of the file
__global__ __launch_bounds__(kThreads) void jpeg_ff_scan_kernel(int* __restrict__ ff, int nchunks,
                                                               const int* __restrict__ total, int* __restrict__ sizes,
                                                               uint8_t* __restrict__ files, long long stride,
                                                               HeaderArg hdr) {
    __shared__ int sh[kThreads];
    const int b = blockIdx.x;
    int* p = ff + (long long)b * nchunks;
    int carry = 0;
    for (int base = 0; base < nchunks; base += kThreads) {
        const int i = base + threadIdx.x;
        const int x = i < nchunks ? p[i] : 0;
        int sum;
        const int e = block_excl_scan(x, sh, sum);
        if (i < nchunks) p[i] = carry + e;
        carry += sum;
    }
    const int nbytes = (total[b] + 7) >> 3;
    const int body = nbytes + carry;
    if (threadIdx.x == 0) sizes[b] = kHeaderBytes + body + 2;
    if (files) {
        uint8_t* f = files + (long long)b * stride;
        for (int i = threadIdx.x; i < kHeaderBytes; i += kThreads) f[i] = hdr.b[i];
        if (threadIdx.x == 0) {
            f[kHeaderBytes + body] = 0xFF;
            f[kHeaderBytes + body + 1] = 0xD9;
        }
    }
}

__global__ __launch_bounds__(kThreads) void jpeg_ff_emit_kernel(const uint32_t* __restrict__ words, int nwords,
                                                               const int* __restrict__ total,
                                                               const int* __restrict__ ffoff, int nchunks,
                                                               uint8_t* __restrict__ files, long long stride) {
    __shared__ int sh[kThreads];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int totalbits = total[b], nbytes = (totalbits + 7) >> 3;
    if ((long long)chunk * kChunkWords * 4 >= nbytes) return;  // uniform over the work-group
    const int wi = chunk * kChunkWords + threadIdx.x;
    int by[4];
    stream_bytes(words + (long long)b * nwords, wi, nbytes, totalbits, by);
    const int c = (by[0] == 255) + (by[1] == 255) + (by[2] == 255) + (by[3] == 255);
    int sum;
    int before = ffoff[b * nchunks + chunk] + block_excl_scan(c, sh, sum);
    uint8_t* f = files + (long long)b * stride + kHeaderBytes;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (by[j] < 0) break;
        const long long o = (long long)wi * 4 + j + before;
        f[o] = (uint8_t)by[j];
        if (by[j] == 255) {
            f[o + 1] = 0;
            ++before;
        }
    }
}

// ---------------------------------------------------------------------------------------------- file decode
// Decoding the entropy segments of foreign 4:2:2 files (the schedule is described in jpeg_core.h):
//   jpeg_unstuff_count/scan/emit   the reverse of jpeg_ff_*: count the dropped 0x00 of FF 00 pairs per 1 KiB chunk,
//                         scan, compact into the image's unstuffed bytes; a marker inside the segment sets a flag
//   jpeg_sync_kernel      one work-group per image, threads strided over the subsequences: round 0, the bounded
//                         sync rounds, the block-count scan, the write pass and the validity word
//   jpeg_dc_scan_kernel   inclusive scan of the DC differences per image and component
//   jpeg_idct_kernel      one 8x8 block per thread: zigzag coefficients * the file's quantiser -> IDCT -> u8 planes
// and then jpeg_decode_kernel above.
constexpr int kUnstuffChunk = kThreads * 4;
constexpr int kSyncThreads = 1024;  // default block of jpeg_sync_kernel (sweep: profiles/jpeg_decode.json)
constexpr int kMaxSyncThreads = 1024;

__constant__ DecTables d_dec = make_dec_tables();

struct DecLayout {
    int nb, ucap, nchunks, maxsub;
    long long ubytes, cnt, bad, ulen, exits, first, coef, yp, cbp, crp, end;
};

static DecLayout make_dec_layout(int B, int H, int W, long long capacity) {
    DecLayout L;
    L.nb = blocks_per_image(H, W);
    L.ucap = unstuffed_capacity(capacity);
    L.nchunks = (int)((capacity + kUnstuffChunk - 1) / kUnstuffChunk);
    L.maxsub = (int)((capacity * 8 + kMinSubBits - 1) / kMinSubBits);
    long long o = 0;
    L.ubytes = o, o = align256(o + (long long)B * L.ucap);
    L.cnt = o, o = align256(o + (long long)B * L.nchunks * 4);
    L.bad = o, o = align256(o + (long long)B * L.nchunks * 4);
    L.ulen = o, o = align256(o + (long long)B * 2 * 4);
    L.exits = o, o = align256(o + (long long)B * 2 * L.maxsub * (long long)sizeof(SubExit));
    L.first = o, o = align256(o + (long long)B * L.maxsub * 4);
    L.coef = o, o = align256(o + (long long)B * L.nb * 64 * 2);
    const long long pix = (long long)B * padded_h(H) * padded_w(W);
    L.yp = o, o = align256(o + pix);
    L.cbp = o, o = align256(o + pix / 2);
    L.crp = o, o = align256(o + pix / 2);
    L.end = o;
    return L;
}

// the four segment bytes of thread slot k0 .. k0+3 and the byte before them; -1 past the end
__device__ __forceinline__ void scan_bytes(const uint8_t* seg, int len, int k0, int* by, int& prev) {
    prev = k0 > 0 && k0 - 1 < len ? seg[k0 - 1] : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) by[j] = k0 + j < len ? seg[k0 + j] : -1;
}

__device__ __forceinline__ int clamped_len(const int* scan_len, int b, int capacity) {
    const int n = scan_len[b];
    return n < 0 ? 0 : (n > capacity ? capacity : n);
}

__global__ __launch_bounds__(kThreads) void jpeg_unstuff_count_kernel(const uint8_t* __restrict__ scans,
                                                                     const long long* __restrict__ scan_off,
                                                                     const int* __restrict__ scan_len, int capacity,
                                                                     int nchunks, int* __restrict__ cnt,
                                                                     int* __restrict__ bad) {
    __shared__ int sh[kThreads];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int len = clamped_len(scan_len, b, capacity);
    int by[4], prev, c = 0, e = 0;
    scan_bytes(scans + scan_off[b], len, chunk * kUnstuffChunk + threadIdx.x * 4, by, prev);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (by[j] < 0) break;
        c += ff_dropped(prev, by[j]);
        e |= ff_error(prev, by[j], chunk * kUnstuffChunk + threadIdx.x * 4 + j == len - 1);
        prev = by[j];
    }
    int sum;
    block_excl_scan(c, sh, sum);
    e = __syncthreads_or(e);
    if (threadIdx.x == 0) {
        cnt[b * nchunks + chunk] = sum;
        bad[b * nchunks + chunk] = e;
    }
}

// one work-group per image: dropped-byte counts -> exclusive offsets in place; ulen[2b] = the unstuffed byte
// count, ulen[2b+1] = a marker was seen or the segment is longer than the capacity
__global__ __launch_bounds__(kThreads) void jpeg_unstuff_scan_kernel(int* __restrict__ cnt, const int* __restrict__ bad,
                                                                    int nchunks, const int* __restrict__ scan_len,
                                                                    int capacity, int* __restrict__ ulen) {
    __shared__ int sh[kThreads];
    const int b = blockIdx.x;
    int* p = cnt + (long long)b * nchunks;
    int carry = 0, e = 0;
    for (int base = 0; base < nchunks; base += kThreads) {
        const int i = base + threadIdx.x;
        const int x = i < nchunks ? p[i] : 0;
        e |= i < nchunks ? bad[(long long)b * nchunks + i] : 0;
        int sum;
        const int ex = block_excl_scan(x, sh, sum);
        if (i < nchunks) p[i] = carry + ex;
        carry += sum;
    }
    e = __syncthreads_or(e);
    if (threadIdx.x == 0) {
        ulen[2 * b] = clamped_len(scan_len, b, capacity) - carry;
        ulen[2 * b + 1] = (e ? kStBadMarker : 0) | (scan_len[b] > capacity || scan_len[b] < 0 ? kStTooLong : 0);
    }
}

__global__ __launch_bounds__(kThreads) void jpeg_unstuff_emit_kernel(const uint8_t* __restrict__ scans,
                                                                    const long long* __restrict__ scan_off,
                                                                    const int* __restrict__ scan_len, int capacity,
                                                                    const int* __restrict__ off, int nchunks,
                                                                    uint8_t* __restrict__ ubytes, int ucap) {
    __shared__ int sh[kThreads];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int len = clamped_len(scan_len, b, capacity);
    const int k0 = chunk * kUnstuffChunk + threadIdx.x * 4;
    int by[4], prev, c = 0;
    scan_bytes(scans + scan_off[b], len, k0, by, prev);
    int p = prev;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (by[j] < 0) break;
        c += ff_dropped(p, by[j]);
        p = by[j];
    }
    int sum;
    int before = off[b * nchunks + chunk] + block_excl_scan(c, sh, sum);
    uint8_t* u = ubytes + (long long)b * ucap;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (by[j] < 0) break;
        if (ff_dropped(prev, by[j])) ++before;
        else u[k0 + j - before] = (uint8_t)by[j];  // k0 + j - before < len <= capacity < ucap
        prev = by[j];
    }
}

// exclusive scan over blockDim.x (a multiple of 64, <= 1024) threads; the step count is that of the largest block
// (the steps past blockDim.x add nothing), so that the loop unrolls
__device__ __forceinline__ int block_excl_scan_n(int v, int* sh, int& total) {
    const int tid = threadIdx.x, nt = blockDim.x;
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < kMaxSyncThreads; off <<= 1) {
        const int t = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const int incl = sh[tid];
    total = sh[nt - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kMaxSyncThreads) void jpeg_sync_kernel(const uint8_t* __restrict__ ubytes, int ucap,
                                                                   const int* __restrict__ ulen, int sub_bits,
                                                                   int maxsub, int nb, SubExit* __restrict__ exits,
                                                                   int* __restrict__ first,
                                                                   int16_t* __restrict__ coef,
                                                                   int* __restrict__ status,
                                                                   int* __restrict__ rounds_out) {
    __shared__ DecTables T;
    __shared__ int sh[kMaxSyncThreads];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < (int)(sizeof(DecTables) / 4); i += nt)
        reinterpret_cast<uint32_t*>(&T)[i] = reinterpret_cast<const uint32_t*>(&d_dec)[i];
    __syncthreads();
    const BitReader R{ubytes + (long long)b * ucap, (uint32_t)ulen[2 * b]};
    const uint32_t total_bits = R.nbytes * 8u;
    int nsub = sub_count(total_bits, sub_bits);
    if (nsub > maxsub) nsub = maxsub;  // cannot happen: ulen <= capacity
    SubExit* cur = exits + (long long)b * 2 * maxsub;
    SubExit* nxt = cur + maxsub;
    coef += (long long)b * nb * 64;
    first += (long long)b * maxsub;

    for (int i = tid; i < nsub; i += nt) cur[i] = sync_round0(T, R, i, sub_bits, total_bits);
    __syncthreads();
    int rounds = 0;
    for (int r = 1; r < nsub; ++r) {  // bounded: subsequences 0..r are exact after round r
        int changed = 0;
        for (int i = tid; i < nsub; i += nt) changed |= sync_round(T, R, i, sub_bits, total_bits, cur, nxt);
        ++rounds;
        SubExit* t = cur;
        cur = nxt;
        nxt = t;
        if (!__syncthreads_or(changed)) break;
    }

    int carry = 0, err = 0;
    for (int base = 0; base < nsub; base += nt) {
        const int i = base + tid;
        const int n = i < nsub ? (int)(cur[i].w >> 16) : 0;
        if (i < nsub) err |= (int)(cur[i].w & kExitError);
        int sum;
        const int e = block_excl_scan_n(n, sh, sum);
        if (i < nsub) first[i] = carry + e;
        carry += sum;
    }
    for (int i = tid; i < nsub; i += nt) write_subsequence(T, R, i, sub_bits, total_bits, cur, first[i], coef, nb);
    err = __syncthreads_or(err);
    if (tid == 0) {
        status[b] = ulen[2 * b + 1] |
                    decode_status(R, total_bits, nsub, nsub ? cur[nsub - 1] : SubExit{0u, 0u}, carry, nb, err != 0, false);
        if (rounds_out) rounds_out[b] = rounds;
    }
}

// grid (3, B): component comp of image b, DC differences -> DC values in place
__global__ __launch_bounds__(kThreads) void jpeg_dc_scan_kernel(int16_t* __restrict__ coef, int nb,
                                                               const int* __restrict__ status) {
    __shared__ int sh[kThreads];
    const int comp = blockIdx.x, b = blockIdx.y;
    if (status[b]) return;  // uniform over the work-group
    int16_t* img = coef + (long long)b * nb * 64;
    const int n = dc_blocks_of(comp, nb);
    int carry = 0;
    for (int base = 0; base < n; base += kThreads) {
        const int s = base + threadIdx.x;
        int16_t* slot = img + (long long)dc_block_of(comp, s < n ? s : 0) * 64;
        const int x = s < n ? (int)*slot : 0;
        int sum;
        const int e = block_excl_scan(x, sh, sum);
        if (s < n) *slot = (int16_t)(carry + e + x);
        carry += sum;
    }
}

// grid (ceil(nb / 256), B); item i of an image as in jpeg_blocks_kernel (luminance blocks in raster order first)
__global__ __launch_bounds__(kThreads) void jpeg_idct_kernel(const int16_t* __restrict__ coef,
                                                            const uint8_t* __restrict__ qtabs,
                                                            const int* __restrict__ status, int H, int W,
                                                            uint8_t* __restrict__ yp, uint8_t* __restrict__ cbp,
                                                            uint8_t* __restrict__ crp) {
    __shared__ uint16_t q[128];
    const int b = blockIdx.y;
    if (status[b]) return;  // uniform over the work-group: the image's output stays unspecified
    if (threadIdx.x < 128)
        q[(threadIdx.x & 64) + kNatural[threadIdx.x & 63]] = qtabs[(long long)b * 128 + threadIdx.x];
    __syncthreads();
    const int mw = mcus_per_row(W), nmcu = mw * block_rows(H), nb = 4 * nmcu;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nb) return;
    int comp, bx, by, blk;
    if (i < 2 * nmcu) {
        comp = 0, bx = i % (2 * mw), by = i / (2 * mw);
        blk = (by * mw + (bx >> 1)) * 4 + (bx & 1);
    } else {
        comp = i < 3 * nmcu ? 1 : 2;
        const int m = i - (comp + 1) * nmcu;
        bx = m % mw, by = m / mw;
        blk = m * 4 + comp + 1;
    }
    const uint4* src = reinterpret_cast<const uint4*>(coef + ((long long)b * nb + blk) * 64);
    int16_t zz[64];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const uint4 v = src[g];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            zz[8 * g + 2 * j] = (int16_t)(w[j] & 0xFFFFu);
            zz[8 * g + 2 * j + 1] = (int16_t)(w[j] >> 16);
        }
    }
    int d[64];
    coef_block_to_samples(zz, q + (comp ? 64 : 0), d);
    const int pw = comp ? mw * 8 : mw * 16;
    uint8_t* plane = (comp == 0 ? yp : (comp == 1 ? cbp : crp)) + (long long)b * block_rows(H) * 8 * pw;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        uint32_t u[8];  // samples in 0..255
#pragma unroll
        for (int c = 0; c < 8; ++c) u[c] = (uint32_t)d[r * 8 + c];
        const uint32_t lo = u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24);
        const uint32_t hi = u[4] | (u[5] << 8) | (u[6] << 16) | (u[7] << 24);
        *reinterpret_cast<uint2*>(plane + (long long)(by * 8 + r) * pw + bx * 8) = make_uint2(lo, hi);
    }
}

// any_size: the *_any entry points take every H, W >= 1; the strict ones keep whole MCUs as their contract
static int check_shape(const char* what, int B, int H, int W, bool any_size = false) {
    if (any_size)
        HY_REQUIRE(B >= 1 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535, HYRES_E_SHAPE,
                   "%s: B >= 1, 1 <= H, W < 65536 (got %d x %d x %d)", what, B, H, W);
    else
        HY_REQUIRE(B >= 1 && H >= 8 && W >= 16 && H % 8 == 0 && W % 16 == 0 && H <= 65528 && W <= 65520, HYRES_E_SHAPE,
                   "%s: B >= 1, H %% 8 == 0, W %% 16 == 0, H, W < 65536 (got %d x %d x %d)", what, B, H, W);
    HY_REQUIRE((long long)blocks_per_image(H, W) * kMaxBlockBits < (1LL << 31) &&
                   (long long)B * padded_h(H) * padded_w(W) < (1LL << 31),
               HYRES_E_SHAPE, "%s: %d x %d x %d is too large", what, B, H, W);
    return ok();
}

}  // namespace jpeg
}  // namespace hyres

using namespace hyres;
using namespace hyres::jpeg;

// header + the entropy segment at kMaxBlockBits per block with every byte stuffed + EOI
static long long stream_bytes(int H, int W) { return align256(kHeaderBytes + 2LL * make_layout(1, H, W).nwords * 4 + 2); }

// The entry points come in pairs: the strict one checks for whole MCUs and the *_any one does not; both run the
// one implementation below.
static int roundtrip(const char* what, bool any_size, const float* x, int B, int H, int W, int quality,
                     float* decoded, int* sizes, unsigned char* files, long long file_stride, void* ws,
                     long long ws_bytes, hyres_stream_t s) {
    HY_REQUIRE(x && decoded && sizes, HYRES_E_ARG, "%s: NULL", what);
    int rc = check_shape(what, B, H, W, any_size);
    if (rc) return rc;
    const Layout L = make_layout(B, H, W);
    HY_REQUIRE(ws && ws_bytes >= L.end, HYRES_E_WORKSPACE, "%s: workspace %lld < %lld", what, ws_bytes, L.end);
    HY_REQUIRE(aligned16(ws) && aligned16(decoded), HYRES_E_ALIGN, "%s: alignment", what);
    HY_REQUIRE(!files || file_stride >= stream_bytes(H, W), HYRES_E_WORKSPACE, "%s: file stride %lld < %lld", what,
               file_stride, stream_bytes(H, W));
    char* base = (char*)ws;
    int16_t* coef = (int16_t*)(base + L.coef);
    uint8_t *yp = (uint8_t*)(base + L.yp), *cbp = (uint8_t*)(base + L.cbp), *crp = (uint8_t*)(base + L.crp);
    int *bits = (int*)(base + L.bits), *total = (int*)(base + L.total), *ff = (int*)(base + L.ff);
    uint32_t* words = (uint32_t*)(base + L.words);
    hipStream_t st = as_stream(s);
    const QuantTables Q = quant_tables_natural(quality);
    HeaderArg hdr;
    uint8_t z[2][64];
    quant_tables_zigzag(quality, z[0], z[1]);
    build_header(z[0], z[1], H, W, hdr.b);

    // cleared by a kernel, not hipMemsetAsync: captured into a graph, the memset cleared the buffer for the first
    // replay only, and later replays ORed their bits into the previous stream
    const long long nvec = (long long)B * L.nwords / 4;  // nwords is a multiple of 256
    hipLaunchKernelGGL(jpeg_clear_kernel, dim3(ceil_div(nvec, kThreads)), dim3(kThreads), 0, st, (uint4*)words, nvec);
    if ((rc = HY_LAUNCH_CHECK("jpeg_clear"))) return rc;
    const int gblk = ceil_div((long long)B * L.nb, kThreads);
    hipLaunchKernelGGL(jpeg_blocks_kernel, dim3(gblk), dim3(kThreads), 0, st, x, B, H, W, Q, coef, yp, cbp, crp);
    if ((rc = HY_LAUNCH_CHECK("jpeg_blocks"))) return rc;
    hipLaunchKernelGGL(jpeg_decode_kernel, dim3(ceil_div((long long)B * H * ((W + 1) / 2), kThreads)), dim3(kThreads),
                       0, st, yp, cbp, crp, B, H, W, padded_h(H), padded_w(W), decoded);
    if ((rc = HY_LAUNCH_CHECK("jpeg_decode"))) return rc;
    hipLaunchKernelGGL(jpeg_count_kernel, dim3(gblk), dim3(kThreads), 0, st, coef, B, L.nb, bits);
    if ((rc = HY_LAUNCH_CHECK("jpeg_count"))) return rc;
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(B), dim3(kThreads), 0, st, bits, L.nb, total);
    if ((rc = HY_LAUNCH_CHECK("jpeg_scan"))) return rc;
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3(gblk), dim3(kThreads), 0, st, coef, B, L.nb, bits, words, L.nwords);
    if ((rc = HY_LAUNCH_CHECK("jpeg_pack"))) return rc;
    hipLaunchKernelGGL(jpeg_ff_count_kernel, dim3(L.nchunks, B), dim3(kThreads), 0, st, words, L.nwords, total,
                       L.nchunks, ff);
    if ((rc = HY_LAUNCH_CHECK("jpeg_ff_count"))) return rc;
    hipLaunchKernelGGL(jpeg_ff_scan_kernel, dim3(B), dim3(kThreads), 0, st, ff, L.nchunks, total, sizes, files,
                       file_stride, hdr);
    if ((rc = HY_LAUNCH_CHECK("jpeg_ff_scan"))) return rc;
    if (files) {
        hipLaunchKernelGGL(jpeg_ff_emit_kernel, dim3(L.nchunks, B), dim3(kThreads), 0, st, words, L.nwords, total, ff,
                           L.nchunks, files, file_stride);
        if ((rc = HY_LAUNCH_CHECK("jpeg_ff_emit"))) return rc;
    }
    return ok();
}

static int roundtrip_host(const char* what, bool any_size, const float* x, int B, int H, int W, int quality,
                          float* decoded, int* sizes, unsigned char* files, long long file_stride) {
    HY_REQUIRE(x && decoded && sizes, HYRES_E_ARG, "%s: NULL", what);
    int rc = check_shape(what, B, H, W, any_size);
    if (rc) return rc;
    HY_REQUIRE(!files || file_stride >= stream_bytes(H, W), HYRES_E_WORKSPACE, "%s: file stride %lld < %lld", what,
               file_stride, stream_bytes(H, W));
    std::vector<uint8_t> f;
    const long long img = 3LL * H * W;
    for (int b = 0; b < B; ++b) {
        sizes[b] = roundtrip_image_host(x + b * img, H, W, quality, decoded + b * img, &f);
        if (files) std::memcpy(files + b * file_stride, f.data(), f.size());
    }
    return ok();
}

static int parse(const char* what, bool any_size, const unsigned char* file, long long nbytes, hyres_jpeg_info* info) {
    HY_REQUIRE(file && info && nbytes >= 0, HYRES_E_ARG, "%s: NULL", what);
    FileInfo fi{};
    const char* why = parse_file(file, (size_t)nbytes, &fi, any_size);
    if (!why && check_shape(what, 1, fi.H, fi.W, any_size)) why = "size outside the codec's limits";
    if (!why && fi.scan_len >= (1LL << 28)) why = "entropy segment of 256 MiB or more";
    info->supported = why ? 0 : 1;
    if (why) {
        set_error(HYRES_E_ARG, "%s: %s", what, why);  // the reason, read through hyres_last_error_string
        return ok();  // an unsupported file is an answer, not a failed call
    }
    info->H = fi.H, info->W = fi.W;
    info->scan_off = fi.scan_off, info->scan_len = fi.scan_len;
    std::memcpy(info->qtab, fi.qtab, 128);
    return ok();
}

static int check_decode(const char* what, bool any_size, int B, int H, int W, long long capacity, int& sub_bits) {
    int rc = check_shape(what, B, H, W, any_size);
    if (rc) return rc;
    HY_REQUIRE(capacity >= 1 && capacity < (1LL << 28), HYRES_E_SHAPE, "%s: scan capacity %lld outside 1 .. 2^28 - 1",
               what, capacity);
    if (sub_bits == 0) sub_bits = kDefaultSubBits;
    HY_REQUIRE(sub_bits >= kMinSubBits && sub_bits <= kMaxSubBits && sub_bits % 32 == 0, HYRES_E_ARG,
               "%s: sub_bits %d: 0 or a multiple of 32 in 32 .. 8192", what, sub_bits);
    return ok();
}

static long long decode_workspace_bytes(const char* what, bool any_size, int B, int H, int W, long long scan_capacity) {
    int sub = 0;
    if (check_decode(what, any_size, B, H, W, scan_capacity, sub)) return -1;
    return make_dec_layout(B, H, W, scan_capacity).end;
}

static int decode(const char* what, bool any_size, const unsigned char* scans, const long long* scan_off,
                  const int* scan_len, const unsigned char* qtabs, int B, int H, int W, long long scan_capacity,
                  int sub_bits, int block_threads, float* decoded, int* status, int* rounds, void* ws,
                  long long ws_bytes, hyres_stream_t s) {
    HY_REQUIRE(scans && scan_off && scan_len && qtabs && decoded && status, HYRES_E_ARG, "%s: NULL", what);
    int rc = check_decode(what, any_size, B, H, W, scan_capacity, sub_bits);
    if (rc) return rc;
    if (block_threads == 0) block_threads = kSyncThreads;
    HY_REQUIRE(block_threads >= 64 && block_threads <= kMaxSyncThreads && block_threads % 64 == 0, HYRES_E_ARG,
               "%s: block_threads %d: 0 or a multiple of 64 in 64 .. 1024", what, block_threads);
    const DecLayout L = make_dec_layout(B, H, W, scan_capacity);
    HY_REQUIRE(ws && ws_bytes >= L.end, HYRES_E_WORKSPACE, "%s: workspace %lld < %lld", what, ws_bytes, L.end);
    HY_REQUIRE(aligned16(ws) && aligned16(decoded), HYRES_E_ALIGN, "%s: alignment", what);
    char* base = (char*)ws;
    uint8_t* ubytes = (uint8_t*)(base + L.ubytes);
    int *cnt = (int*)(base + L.cnt), *bad = (int*)(base + L.bad), *ulen = (int*)(base + L.ulen);
    int* first = (int*)(base + L.first);
    SubExit* exits = (SubExit*)(base + L.exits);
    int16_t* coef = (int16_t*)(base + L.coef);
    uint8_t *yp = (uint8_t*)(base + L.yp), *cbp = (uint8_t*)(base + L.cbp), *crp = (uint8_t*)(base + L.crp);
    hipStream_t st = as_stream(s);
    const int cap = (int)scan_capacity;
    // exits are laid out for the smallest sub_bits; this call uses the first maxsub entries of each buffer
    const int maxsub = (int)((scan_capacity * 8 + sub_bits - 1) / sub_bits);

    hipLaunchKernelGGL(jpeg_unstuff_count_kernel, dim3(L.nchunks, B), dim3(kThreads), 0, st, scans, scan_off, scan_len,
                       cap, L.nchunks, cnt, bad);
    if ((rc = HY_LAUNCH_CHECK("jpeg_unstuff_count"))) return rc;
    hipLaunchKernelGGL(jpeg_unstuff_scan_kernel, dim3(B), dim3(kThreads), 0, st, cnt, bad, L.nchunks, scan_len, cap,
                       ulen);
    if ((rc = HY_LAUNCH_CHECK("jpeg_unstuff_scan"))) return rc;
    hipLaunchKernelGGL(jpeg_unstuff_emit_kernel, dim3(L.nchunks, B), dim3(kThreads), 0, st, scans, scan_off, scan_len,
                       cap, cnt, L.nchunks, ubytes, L.ucap);
    if ((rc = HY_LAUNCH_CHECK("jpeg_unstuff_emit"))) return rc;
    hipLaunchKernelGGL(jpeg_sync_kernel, dim3(B), dim3(block_threads), 0, st, ubytes, L.ucap, ulen, sub_bits, maxsub,
                       L.nb, exits, first, coef, status, rounds);
    if ((rc = HY_LAUNCH_CHECK("jpeg_sync"))) return rc;
    hipLaunchKernelGGL(jpeg_dc_scan_kernel, dim3(3, B), dim3(kThreads), 0, st, coef, L.nb, status);
    if ((rc = HY_LAUNCH_CHECK("jpeg_dc_scan"))) return rc;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(ceil_div(L.nb, kThreads), B), dim3(kThreads), 0, st, coef, qtabs, status,
                       H, W, yp, cbp, crp);
    if ((rc = HY_LAUNCH_CHECK("jpeg_idct"))) return rc;
    hipLaunchKernelGGL(jpeg_decode_kernel, dim3(ceil_div((long long)B * H * ((W + 1) / 2), kThreads)), dim3(kThreads),
                       0, st, yp, cbp, crp, B, H, W, padded_h(H), padded_w(W), decoded);
    if ((rc = HY_LAUNCH_CHECK("jpeg_decode"))) return rc;
    return ok();
}

static int decode_host(const char* what, bool any_size, const unsigned char* scans, const long long* scan_off,
                       const int* scan_len, const unsigned char* qtabs, int B, int H, int W, long long scan_capacity,
                       int sub_bits, float* decoded, int* status, int* rounds) {
    HY_REQUIRE(scans && scan_off && scan_len && qtabs && decoded && status, HYRES_E_ARG, "%s: NULL", what);
    int rc = check_decode(what, any_size, B, H, W, scan_capacity, sub_bits);
    if (rc) return rc;
    const long long img = 3LL * H * W;
    for (int b = 0; b < B; ++b) {
        uint8_t qz[2][64];
        std::memcpy(qz, qtabs + (long long)b * 128, 128);
        status[b] = decode_image_host(scans + scan_off[b], scan_len[b], scan_capacity, qz, H, W, sub_bits,
                                      decoded + b * img, rounds ? rounds + b : nullptr);
    }
    return ok();
}

extern "C" {

int hyres_jpeg_quant_tables(int quality, unsigned char* lum, unsigned char* chr) {
    HY_REQUIRE(lum && chr, HYRES_E_ARG, "jpeg_quant_tables: NULL");
    quant_tables_zigzag(quality, lum, chr);
    return ok();
}

long long hyres_jpeg_workspace_bytes(int B, int H, int W) {
    if (check_shape("jpeg_workspace_bytes", B, H, W)) return -1;
    return make_layout(B, H, W).end;
}
long long hyres_jpeg_workspace_bytes_any(int B, int H, int W) {
    if (check_shape("jpeg_workspace_bytes_any", B, H, W, true)) return -1;
    return make_layout(B, H, W).end;
}

long long hyres_jpeg_stream_bytes(int H, int W) {
    if (check_shape("jpeg_stream_bytes", 1, H, W)) return -1;
    return stream_bytes(H, W);
}
long long hyres_jpeg_stream_bytes_any(int H, int W) {
    if (check_shape("jpeg_stream_bytes_any", 1, H, W, true)) return -1;
    return stream_bytes(H, W);
}

int hyres_jpeg_roundtrip(const float* x, int B, int H, int W, int quality, float* decoded, int* sizes,
                         unsigned char* files, long long file_stride, void* ws, long long ws_bytes,
                         hyres_stream_t s) {
    return roundtrip("jpeg_roundtrip", false, x, B, H, W, quality, decoded, sizes, files, file_stride, ws, ws_bytes, s);
}
int hyres_jpeg_roundtrip_any(const float* x, int B, int H, int W, int quality, float* decoded, int* sizes,
                             unsigned char* files, long long file_stride, void* ws, long long ws_bytes,
                             hyres_stream_t s) {
    return roundtrip("jpeg_roundtrip_any", true, x, B, H, W, quality, decoded, sizes, files, file_stride, ws, ws_bytes,
                     s);
}

int hyres_jpeg_roundtrip_host(const float* x, int B, int H, int W, int quality, float* decoded, int* sizes,
                              unsigned char* files, long long file_stride, void* ws, long long ws_bytes,
                              hyres_stream_t s) {
    (void)ws, (void)ws_bytes, (void)s;
    return roundtrip_host("jpeg_roundtrip_host", false, x, B, H, W, quality, decoded, sizes, files, file_stride);
}
int hyres_jpeg_roundtrip_any_host(const float* x, int B, int H, int W, int quality, float* decoded, int* sizes,
                                  unsigned char* files, long long file_stride, void* ws, long long ws_bytes,
                                  hyres_stream_t s) {
    (void)ws, (void)ws_bytes, (void)s;
    return roundtrip_host("jpeg_roundtrip_any_host", true, x, B, H, W, quality, decoded, sizes, files, file_stride);
}

int hyres_jpeg_parse(const unsigned char* file, long long nbytes, hyres_jpeg_info* info) {
    return parse("jpeg_parse", false, file, nbytes, info);
}
int hyres_jpeg_parse_any(const unsigned char* file, long long nbytes, hyres_jpeg_info* info) {
    return parse("jpeg_parse_any", true, file, nbytes, info);
}

long long hyres_jpeg_decode_workspace_bytes(int B, int H, int W, long long scan_capacity) {
    return decode_workspace_bytes("jpeg_decode_workspace_bytes", false, B, H, W, scan_capacity);
}
long long hyres_jpeg_decode_any_workspace_bytes(int B, int H, int W, long long scan_capacity) {
    return decode_workspace_bytes("jpeg_decode_any_workspace_bytes", true, B, H, W, scan_capacity);
}

int hyres_jpeg_decode(const unsigned char* scans, const long long* scan_off, const int* scan_len,
                      const unsigned char* qtabs, int B, int H, int W, long long scan_capacity, int sub_bits,
                      int block_threads, float* decoded, int* status, int* rounds, void* ws, long long ws_bytes,
                      hyres_stream_t s) {
    return decode("jpeg_decode", false, scans, scan_off, scan_len, qtabs, B, H, W, scan_capacity, sub_bits,
                  block_threads, decoded, status, rounds, ws, ws_bytes, s);
}
int hyres_jpeg_decode_any(const unsigned char* scans, const long long* scan_off, const int* scan_len,
                          const unsigned char* qtabs, int B, int H, int W, long long scan_capacity, int sub_bits,
                          int block_threads, float* decoded, int* status, int* rounds, void* ws, long long ws_bytes,
                          hyres_stream_t s) {
    return decode("jpeg_decode_any", true, scans, scan_off, scan_len, qtabs, B, H, W, scan_capacity, sub_bits,
                  block_threads, decoded, status, rounds, ws, ws_bytes, s);
}

int hyres_jpeg_decode_host(const unsigned char* scans, const long long* scan_off, const int* scan_len,
                           const unsigned char* qtabs, int B, int H, int W, long long scan_capacity, int sub_bits,
                           int block_threads, float* decoded, int* status, int* rounds, void* ws, long long ws_bytes,
                           hyres_stream_t s) {
    (void)block_threads, (void)ws, (void)ws_bytes, (void)s;
    return decode_host("jpeg_decode_host", false, scans, scan_off, scan_len, qtabs, B, H, W, scan_capacity, sub_bits,
                       decoded, status, rounds);
}
int hyres_jpeg_decode_any_host(const unsigned char* scans, const long long* scan_off, const int* scan_len,
                               const unsigned char* qtabs, int B, int H, int W, long long scan_capacity, int sub_bits,
                               int block_threads, float* decoded, int* status, int* rounds, void* ws,
                               long long ws_bytes, hyres_stream_t s) {
    (void)block_threads, (void)ws, (void)ws_bytes, (void)s;
    return decode_host("jpeg_decode_any_host", true, scans, scan_off, scan_len, qtabs, B, H, W, scan_capacity,
                       sub_bits, decoded, status, rounds);
}

}  // extern "C"
