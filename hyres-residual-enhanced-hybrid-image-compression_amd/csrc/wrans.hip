// Device rANS coder for compress / decompress (opt-in: HYRES_ENTROPY_CODER=device): the
// wave-interleaved string format HRW1 of wrans_core.h. One wave64 per string (image x pass) in a 64-thread block; each
// lane is one rans64 coder over the coded symbols k with k % 64 == lane, and the lanes' renormalisation words are
// interleaved row by row with a ballot prefix count. Plain C++: no atomics, no LDS, no dynamic allocation.
//
//   encode  wrans_encode_kernel walks the rows from last to first and writes the payload and the escape list
//           backwards into the string's worst-case workspace slot (4 bytes per coded symbol each), then the header and
//           the lane states, and records the string's length; wrans_pack_kernel copies the strings one after the other
//           into the caller's buffer behind an exclusive scan of the lengths (a chained call continues the scan of the
//           previous one, so the z, anchor and non-anchor strings of a batch form one buffer and one offset table).
//   decode  wrans_decode_kernel reads the packed strings and the offset table, binary-searches each lane's CDF in the
//           device-resident table and writes the full symbol array: owned positions from the stream, the others
//           (int)rintf(0.f - mean), which is what the host path's symbols hold there.
// The decoder's loop bounds are kernel arguments the host derived from the latent shape and checked against the
// header (hyres_wrans_validate); every read of the string goes through a clamp to its end, every table index is
// clamped to the table. A damaged string decodes to wrong symbols, never to an out-of-range access.
//
// The pure-host twins (hyres_wrans_encode_host / _decode_host) run the same functions of wrans_core.h in a loop over
// rows and lanes; they produce and accept the same bytes and need no GPU.
//
// HRW2 (hyres_wrans2_*, a second opt-in) cuts a string into segments of R rows, each coded exactly as HRW1 codes a
// whole string, so one wave codes one segment and a string takes S = ceil(n / 64R) waves:
//   encode  wrans2_encode_kernel, grid (S, B): the HRW1 row loop over the segment's rows, backwards into the segment's
//           own part [64 R s, 64 R s + n_s) of the string's escape and payload regions; stores the segment's states and
//           its two counts. wrans2_scan_kernel, one wave per string: the counts become the cumulative directory and the
//           string's length. wrans2_pack_kernel, grid (S, B): every wave adds up the lengths of the strings before its
//           own (as wrans_pack_kernel does, ``chain`` included) and copies its segment's directory entry, states,
//           escapes and words to their final places; segment 0 adds the header and the offset table's entry.
//   decode  wrans2_decode_kernel, grid (S, B): a wave reads its directory entry and the one before it, then runs the
//           HRW1 decode loop over its rows; the unowned-position fill is strided over all waves of the string.
// S, R and every loop bound are kernel arguments the host derived from the shape and R; what a string says about them
// is only ever used through a clamp.
#include "common.h"
#include "wrans_core.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace hyres {
namespace wrans {

constexpr long long kMaxSymbols = 1ll << 27;  // per string: its worst-case byte length stays inside int

inline long long align16(long long v) { return (v + 15) & ~15ll; }
__host__ __device__ inline long long slot_words(long long n) { return kFixedWords + 2 * n; }  // fixed part, escape region, payload region

struct Tables {
    const int* cdfs;
    int stride;
    const int* sizes;
    const int* offsets;
    int ncdf;
};

struct Step {
    long long pos;  // index into the image's [C][H][W] symbol array
    int ci, max_value;
    const int* cdf;
};

// coded symbol k of an image: its position, CDF row and the row's escape slot (indexes clamped to the table)
__host__ __device__ inline Step step_of(long long k, const int* idx, int H, int W, int parity, long long plane,
                                        const Tables& t) {
    const Pos p = owned_pos(k, H, W, parity, plane);
    Step s;
    s.pos = ((long long)p.c * H + p.h) * W + p.w;
    int ci = idx ? idx[s.pos] : p.c;
    ci = ci < 0 ? 0 : (ci >= t.ncdf ? t.ncdf - 1 : ci);
    int mv = t.sizes[ci] - 2;
    mv = mv < 0 ? 0 : (mv > t.stride - 2 ? t.stride - 2 : mv);
    s.ci = ci;
    s.max_value = mv;
    s.cdf = t.cdfs + (long long)ci * t.stride;
    return s;
}

__device__ __forceinline__ int rank_below(unsigned long long mask, int lane) {
    return __popcll(mask & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(64) void wrans_encode_kernel(const int* __restrict__ sym, const int* __restrict__ idx,
                                                          int H, int W, int parity, long long chw, long long plane,
                                                          int n, Tables t, uint32_t* __restrict__ slots,
                                                          int* __restrict__ lens) {
    const int b = blockIdx.x, lane = threadIdx.x;
    sym += (long long)b * chw;
    if (idx) idx += (long long)b * chw;
    uint32_t* slot = slots + (long long)b * slot_words(n);
    uint32_t* esc = slot + kFixedWords;       // [0, n): filled from the back
    uint32_t* pay = slot + kFixedWords + n;   // [0, n): filled from the back
    int ecur = n, pcur = n;
    uint64_t x = kL;
    for (int r = (n + kLanes - 1) / kLanes - 1; r >= 0; --r) {
        const int k = r * kLanes + lane;
        const bool active = k < n;
        bool is_esc = false, emit = false;
        uint32_t word = 0;
        int raw = 0;
        if (active) {
            const Step s = step_of(k, idx, H, W, parity, plane, t);
            raw = sym[s.pos];
            const int v = slot_of(raw, t.offsets[s.ci], s.max_value, is_esc);
            const uint32_t start = (uint32_t)s.cdf[v];
            const uint32_t freq = (uint32_t)s.cdf[v + 1] - start;
            emit = enc_put(x, start, freq, kPrecision, word);
        }
        const unsigned long long em = __ballot(emit), es = __ballot(is_esc);
        const int ne = __popcll(em), ns = __popcll(es);
        const int pw = pcur - ne + rank_below(em, lane), pe = ecur - ns + rank_below(es, lane);
        if (emit && pw >= 0) pay[pw] = word;  // at most one word per step: pw >= 0 always
        if (is_esc && pe >= 0) esc[pe] = (uint32_t)raw;
        pcur -= ne;
        ecur -= ns;
    }
    slot[kHeaderWords + 2 * lane] = (uint32_t)x;
    slot[kHeaderWords + 2 * lane + 1] = (uint32_t)(x >> 32);
    if (lane == 0) {
        slot[0] = kMagic;
        slot[1] = (uint32_t)n;
        slot[2] = (uint32_t)(n - ecur);
        slot[3] = (uint32_t)(n - pcur);
        lens[b] = (int)(kFixedBytes + 4ll * ((n - ecur) + (n - pcur)));
    }
}

// string b goes to out + offs[b], offs = offs[0] + exclusive scan of the lengths; offs[0] is 0, or with ``chain`` the
// end offset an earlier call on the stream left there
__global__ __launch_bounds__(64) void wrans_pack_kernel(const uint32_t* __restrict__ slots, const int* __restrict__ lens,
                                                        int n, int chain, uint32_t* __restrict__ out,
                                                        long long out_words, long long* __restrict__ offs) {
    const int b = blockIdx.x, lane = threadIdx.x;
    long long off = chain ? offs[0] : 0;
    for (int j = 0; j < b; ++j) off += lens[j];
    const uint32_t* slot = slots + (long long)b * slot_words(n);
    const int n_esc = (int)slot[2], n_words = (int)slot[3];
    const uint32_t* esc = slot + kFixedWords + (n - n_esc);
    const uint32_t* pay = slot + kFixedWords + n + (n - n_words);
    const long long o = off >> 2;
    const int total = kFixedWords + n_esc + n_words;
    for (int i = lane; i < total; i += kLanes) {
        const uint32_t v = i < kFixedWords ? slot[i] : (i < kFixedWords + n_esc ? esc[i - kFixedWords]
                                                                               : pay[i - kFixedWords - n_esc]);
        if (o + i < out_words) out[o + i] = v;
    }
    if (lane == 0) {
        offs[b + 1] = off + lens[b];
        if (b == 0 && !chain) offs[0] = 0;
    }
}

__global__ __launch_bounds__(64) void wrans_decode_kernel(const unsigned char* __restrict__ strings,
                                                          const long long* __restrict__ offs,
                                                          const int* __restrict__ idx, int H, int W, int parity,
                                                          long long chw, long long plane, int n, Tables t,
                                                          const float* __restrict__ params, int ldp, int M,
                                                          int* __restrict__ out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (idx) idx += (long long)b * chw;
    out += (long long)b * chw;
    const long long o0 = offs[b], o1 = offs[b + 1];
    // words of this string; a misaligned or empty range reads as zeros
    const long long lw = (o0 >= 0 && o1 > o0 && !(o0 & 3)) ? (o1 - o0) >> 2 : 0;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(strings + (lw ? o0 : 0));
    auto rd = [&](long long i) -> uint32_t { return i < lw ? w[i] : 0u; };
    const long long n_esc = min((long long)rd(2), (long long)n), n_words = min((long long)rd(3), (long long)n);
    const long long esc0 = kFixedWords, pay0 = kFixedWords + n_esc;
    long long ecur = 0, pcur = 0;
    uint64_t x = (uint64_t)rd(kHeaderWords + 2 * lane) | ((uint64_t)rd(kHeaderWords + 2 * lane + 1) << 32);
    for (int r = 0; r * kLanes < n; ++r) {
        const int k = r * kLanes + lane;
        const bool active = k < n;
        bool need = false, is_esc = false;
        Step s{};
        int v = 0;
        if (active) {
            s = step_of(k, idx, H, W, parity, plane, t);
            v = cdf_search(s.cdf, s.max_value, dec_get(x, kPrecision));
            const uint32_t start = (uint32_t)s.cdf[v];
            need = dec_advance(x, start, (uint32_t)s.cdf[v + 1] - start, kPrecision);
            is_esc = v == s.max_value;
        }
        const unsigned long long nm = __ballot(need), es = __ballot(is_esc);
        if (need) {
            const long long i = pcur + rank_below(nm, lane);
            dec_refill(x, i < n_words ? rd(pay0 + i) : 0u);
        }
        if (active) {
            int value = v + t.offsets[s.ci];
            if (is_esc) {
                const long long i = ecur + rank_below(es, lane);
                value = i < n_esc ? (int)rd(esc0 + i) : 0;
            }
            out[s.pos] = value;
        }
        pcur += __popcll(nm);
        ecur += __popcll(es);
    }
    if (parity >= 0) {  // the positions this pass does not own: round(0 - mean), as hyres_gc_symbols writes them
        for (long long i = lane; i < chw; i += kLanes) {
            const int wq = (int)(i % W);
            const long long q = i / W;
            const int h = (int)(q % H), c = (int)(q / H);
            if (!keep(parity, h, wq)) {
                const long long pix = ((long long)b * H + h) * W + wq;
                out[i] = (int)rintf(0.f - params[pix * ldp + M + c]);
            }
        }
    }
}

// ---------------------------------------------------------------- HRW2 kernels: one wave per (segment, string)
// one string's part of the encode workspace: S x 64 lane states, escape region [n], payload region [n]
__host__ __device__ inline long long slot_words2(long long n, long long S) { return 2 * kLanes * S + 2 * n; }

__global__ __launch_bounds__(64) void wrans2_encode_kernel(const int* __restrict__ sym, const int* __restrict__ idx,
                                                           int H, int W, int parity, long long chw, long long plane,
                                                           int n, long long seg, int S, Tables t,
                                                           uint32_t* __restrict__ slots, uint32_t* __restrict__ dir) {
    const int s = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    sym += (long long)b * chw;
    if (idx) idx += (long long)b * chw;
    const long long k0 = seg * s;                                   // < n, or 0 for the one segment of n = 0
    const int ns = (int)(min((long long)n, k0 + seg) - k0);        // this segment's coded symbols
    uint32_t* slot = slots + (long long)b * slot_words2(n, S);
    uint32_t* esc = slot + 2ll * kLanes * S + k0;                   // [0, ns): filled from the back
    uint32_t* pay = slot + 2ll * kLanes * S + n + k0;               // [0, ns): filled from the back
    int ecur = ns, pcur = ns;
    uint64_t x = kL;
    for (int r = (ns + kLanes - 1) / kLanes - 1; r >= 0; --r) {
        const int j = r * kLanes + lane;  // within the segment; k0 is a multiple of 64, so the lane is k % 64
        const bool active = j < ns;
        bool is_esc = false, emit = false;
        uint32_t word = 0;
        int raw = 0;
        if (active) {
            const Step st = step_of(k0 + j, idx, H, W, parity, plane, t);
            raw = sym[st.pos];
            const int v = slot_of(raw, t.offsets[st.ci], st.max_value, is_esc);
            const uint32_t start = (uint32_t)st.cdf[v];
            const uint32_t freq = (uint32_t)st.cdf[v + 1] - start;
            emit = enc_put(x, start, freq, kPrecision, word);
        }
        const unsigned long long em = __ballot(emit), es = __ballot(is_esc);
        const int ne = __popcll(em), nes = __popcll(es);
        const int pw = pcur - ne + rank_below(em, lane), pe = ecur - nes + rank_below(es, lane);
        if (emit && pw >= 0) pay[pw] = word;  // at most one word per step: pw >= 0 always
        if (is_esc && pe >= 0) esc[pe] = (uint32_t)raw;
        pcur -= ne;
        ecur -= nes;
    }
    slot[2ll * kLanes * s + 2 * lane] = (uint32_t)x;
    slot[2ll * kLanes * s + 2 * lane + 1] = (uint32_t)(x >> 32);
    if (lane == 0) {
        dir[2 * ((long long)b * S + s)] = (uint32_t)(ns - ecur);
        dir[2 * ((long long)b * S + s) + 1] = (uint32_t)(ns - pcur);
    }
}

// one wave per string: the per-segment counts become the cumulative directory (in place), and the string's length
__global__ __launch_bounds__(64) void wrans2_scan_kernel(uint32_t* __restrict__ dir, int S,
                                                         long long* __restrict__ lens) {
    const int b = blockIdx.x, lane = threadIdx.x;
    dir += 2ll * b * S;
    uint32_t ce = 0, cw = 0;  // carried over from the chunks before
    for (int s0 = 0; s0 < S; s0 += kLanes) {
        const int s = s0 + lane;
        uint32_t e = s < S ? dir[2ll * s] : 0u, w = s < S ? dir[2ll * s + 1] : 0u;
        for (int d = 1; d < kLanes; d <<= 1) {  // inclusive scan over the wave
            const uint32_t pe = __shfl_up(e, d), pw = __shfl_up(w, d);
            if (lane >= d) {
                e += pe;
                w += pw;
            }
        }
        e += ce;
        w += cw;
        if (s < S) {
            dir[2ll * s] = e;
            dir[2ll * s + 1] = w;
        }
        ce = __shfl(e, kLanes - 1);
        cw = __shfl(w, kLanes - 1);
    }
    if (lane == 0) lens[b] = 4 * (fixed_words2(S) + (long long)ce + cw);
}

// string b goes to out + offs[b] as in wrans_pack_kernel (same ``chain``); wave (s, b) copies segment s's parts
__global__ __launch_bounds__(64) void wrans2_pack_kernel(const uint32_t* __restrict__ slots,
                                                         const uint32_t* __restrict__ dir,
                                                         const long long* __restrict__ lens, int n, int R,
                                                         long long seg, int S, int chain, uint32_t* __restrict__ out,
                                                         long long out_words, long long* __restrict__ offs) {
    const int s = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    long long off = chain ? offs[0] : 0;
    for (int j = 0; j < b; ++j) off += lens[j];
    dir += 2ll * b * S;
    const uint32_t* slot = slots + (long long)b * slot_words2(n, S);
    const long long k0 = seg * s;
    const int ns = (int)(min((long long)n, k0 + seg) - k0);
    const long long e0 = s ? dir[2ll * (s - 1)] : 0, w0 = s ? dir[2ll * (s - 1) + 1] : 0;
    const long long e1 = dir[2ll * s], w1 = dir[2ll * s + 1], n_esc = dir[2ll * (S - 1)];
    const int ce = (int)(e1 - e0), cw = (int)(w1 - w0);  // <= ns each
    const uint32_t* esc = slot + 2ll * kLanes * S + k0 + (ns - ce);
    const uint32_t* pay = slot + 2ll * kLanes * S + n + k0 + (ns - cw);
    const long long o = off >> 2, body = o + fixed_words2(S);
    auto put = [&](long long i, uint32_t v) {
        if (i < out_words) out[i] = v;
    };
    if (s == 0 && lane < kHeader2Words)
        put(o + lane, lane == 0 ? kMagic2 : lane == 1 ? (uint32_t)n : lane == 2 ? (uint32_t)R : (uint32_t)S);
    if (lane < 2) put(o + kHeader2Words + 2ll * s + lane, lane ? (uint32_t)w1 : (uint32_t)e1);
    for (int i = lane; i < 2 * kLanes; i += kLanes)
        put(o + kHeader2Words + 2ll * S + 2ll * kLanes * s + i, slot[2ll * kLanes * s + i]);
    for (int i = lane; i < ce; i += kLanes) put(body + e0 + i, esc[i]);
    for (int i = lane; i < cw; i += kLanes) put(body + n_esc + w0 + i, pay[i]);
    if (s == 0 && lane == 0) {
        offs[b + 1] = off + lens[b];
        if (b == 0 && !chain) offs[0] = 0;
    }
}

__global__ __launch_bounds__(64) void wrans2_decode_kernel(const unsigned char* __restrict__ strings,
                                                           const long long* __restrict__ offs,
                                                           const int* __restrict__ idx, int H, int W, int parity,
                                                           long long chw, long long plane, int n, long long seg, int S,
                                                           Tables t, const float* __restrict__ params, int ldp, int M,
                                                           int* __restrict__ out) {
    const int s = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    if (idx) idx += (long long)b * chw;
    out += (long long)b * chw;
    const long long o0 = offs[b], o1 = offs[b + 1];
    // words of this string; a misaligned or empty range reads as zeros
    const long long lw = (o0 >= 0 && o1 > o0 && !(o0 & 3)) ? (o1 - o0) >> 2 : 0;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(strings + (lw ? o0 : 0));
    auto rd = [&](long long i) -> uint32_t { return i < lw ? w[i] : 0u; };
    const long long k0 = seg * s;
    const int ns = (int)(min((long long)n, k0 + seg) - k0);
    // the directory: this segment's entry, the one before it and the last; every count clamped to the segment
    const long long e0 = s ? rd(kHeader2Words + 2ll * (s - 1)) : 0, w0 = s ? rd(kHeader2Words + 2ll * (s - 1) + 1) : 0;
    const long long e1 = rd(kHeader2Words + 2ll * s), w1 = rd(kHeader2Words + 2ll * s + 1);
    const long long n_esc = max(0ll, min(e1 - e0, (long long)ns)), n_words = max(0ll, min(w1 - w0, (long long)ns));
    const long long esc0 = fixed_words2(S) + e0, pay0 = fixed_words2(S) + rd(kHeader2Words + 2ll * (S - 1)) + w0;
    const long long st0 = kHeader2Words + 2ll * S + 2ll * kLanes * s;
    long long ecur = 0, pcur = 0;
    uint64_t x = (uint64_t)rd(st0 + 2 * lane) | ((uint64_t)rd(st0 + 2 * lane + 1) << 32);
    for (int r = 0; r * kLanes < ns; ++r) {
        const int j = r * kLanes + lane;
        const bool active = j < ns;
        bool need = false, is_esc = false;
        Step st{};
        int v = 0;
        if (active) {
            st = step_of(k0 + j, idx, H, W, parity, plane, t);
            v = cdf_search(st.cdf, st.max_value, dec_get(x, kPrecision));
            const uint32_t start = (uint32_t)st.cdf[v];
            need = dec_advance(x, start, (uint32_t)st.cdf[v + 1] - start, kPrecision);
            is_esc = v == st.max_value;
        }
        const unsigned long long nm = __ballot(need), es = __ballot(is_esc);
        if (need) {
            const long long i = pcur + rank_below(nm, lane);
            dec_refill(x, i < n_words ? rd(pay0 + i) : 0u);
        }
        if (active) {
            int value = v + t.offsets[st.ci];
            if (is_esc) {
                const long long i = ecur + rank_below(es, lane);
                value = i < n_esc ? (int)rd(esc0 + i) : 0;
            }
            out[st.pos] = value;
        }
        pcur += __popcll(nm);
        ecur += __popcll(es);
    }
    if (parity >= 0) {  // the unowned positions, shared among the string's S waves: one thread per position
        for (long long i = (long long)s * kLanes + lane; i < chw; i += (long long)S * kLanes) {
            const int wq = (int)(i % W);
            const long long q = i / W;
            const int h = (int)(q % H), c = (int)(q / H);
            if (!keep(parity, h, wq)) {
                const long long pix = ((long long)b * H + h) * W + wq;
                out[i] = (int)rintf(0.f - params[pix * ldp + M + c]);
            }
        }
    }
}

// ---------------------------------------------------------------- host side
static int check_shape(const char* op, int B, int C, int H, int W, int parity, long long* n) {
    HY_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1 && parity >= -1 && parity <= 1, HYRES_E_ARG,
               "%s: bad shape B=%d C=%d H=%d W=%d parity=%d", op, B, C, H, W, parity);
    *n = count(C, H, W, parity);
    HY_REQUIRE(*n <= kMaxSymbols && (long long)C * H * W <= (1ll << 30), HYRES_E_SHAPE,
               "%s: %lld coded symbols per string (at most %lld)", op, *n, kMaxSymbols);
    return 0;
}

static int check_tables(const char* op, const int* cdfs, int stride, const int* sizes, const int* offsets, int ncdf) {
    HY_REQUIRE(cdfs && sizes && offsets && ncdf >= 1 && stride >= 2, HYRES_E_ARG, "%s: bad CDF tables", op);
    return 0;
}

// HRW2: shape, R and the segment count S they give
static int check_shape2(const char* op, int B, int C, int H, int W, int parity, int seg_rows, long long* n,
                        long long* S) {
    if (int rc = check_shape(op, B, C, H, W, parity, n)) return rc;
    HY_REQUIRE(seg_rows >= 1, HYRES_E_ARG, "%s: seg_rows %d: at least 1 row per segment", op, seg_rows);
    HY_REQUIRE(B <= 65535, HYRES_E_SHAPE, "%s: B = %d strings in one call (at most 65535)", op, B);
    *S = segments(*n, seg_rows);
    return 0;
}

// The coded symbols [k0, k1) (k0 a multiple of 64) coded as HRW1 codes a whole string of them: x[64] receives the final
// lane states, pay_rev / esc_rev the words and escapes in the reverse of the string's order (rows last to first, lanes
// last to first).
static int encode_rows_host(const char* op, const int* sym, const int* idx, long long k0, long long k1, int H, int W,
                            int parity, long long plane, const Tables& t, uint64_t* x, std::vector<uint32_t>& pay_rev,
                            std::vector<uint32_t>& esc_rev) {
    for (int lane = 0; lane < kLanes; ++lane) x[lane] = kL;
    for (long long r = (k1 + kLanes - 1) / kLanes - 1; r >= k0 / kLanes; --r) {
        for (int lane = kLanes - 1; lane >= 0; --lane) {
            const long long k = r * kLanes + lane;
            if (k >= k1) continue;
            const Step st = step_of(k, idx, H, W, parity, plane, t);
            bool is_esc = false;
            const int raw = sym[st.pos];
            const int v = slot_of(raw, t.offsets[st.ci], st.max_value, is_esc);
            const uint32_t start = (uint32_t)st.cdf[v];
            const uint32_t freq = (uint32_t)st.cdf[v + 1] - start;
            HY_REQUIRE(freq > 0 && freq <= (1u << kPrecision), HYRES_E_ARG,
                       "%s: CDF %d is not strictly increasing at slot %d", op, st.ci, v);
            uint32_t word = 0;
            if (enc_put(x[lane], start, freq, kPrecision, word)) pay_rev.push_back(word);
            if (is_esc) esc_rev.push_back((uint32_t)raw);
        }
    }
    return 0;
}

static void push_states(std::vector<uint32_t>& words, const uint64_t* x) {
    for (int lane = 0; lane < kLanes; ++lane) {
        words.push_back((uint32_t)x[lane]);
        words.push_back((uint32_t)(x[lane] >> 32));
    }
}

static void store_le(unsigned char* out, const std::vector<uint32_t>& words) {  // little endian, whatever the host
    for (size_t i = 0; i < words.size(); ++i) {
        const uint32_t w = words[i];
        out[4 * i] = (unsigned char)w;
        out[4 * i + 1] = (unsigned char)(w >> 8);
        out[4 * i + 2] = (unsigned char)(w >> 16);
        out[4 * i + 3] = (unsigned char)(w >> 24);
    }
}

// The decoder of the coded symbols [k0, k1) (k0 a multiple of 64): lane states at word st0 of the string, n_esc escapes
// from word esc0, n_words payload words from word pay0; rows first to last, lanes ascending: the string's order.
template <class Rd>
static void decode_rows_host(Rd rd, const int* idx, long long k0, long long k1, int H, int W, int parity,
                             long long plane, const Tables& t, long long st0, long long esc0, long long n_esc,
                             long long pay0, long long n_words, int* sym_out) {
    long long ecur = 0, pcur = 0;
    uint64_t x[kLanes];
    for (int lane = 0; lane < kLanes; ++lane)
        x[lane] = (uint64_t)rd(st0 + 2 * lane) | ((uint64_t)rd(st0 + 2 * lane + 1) << 32);
    for (long long k = k0; k < k1; ++k) {
        const int lane = (int)(k % kLanes);
        const Step st = step_of(k, idx, H, W, parity, plane, t);
        const int v = cdf_search(st.cdf, st.max_value, dec_get(x[lane], kPrecision));
        const uint32_t start = (uint32_t)st.cdf[v];
        if (dec_advance(x[lane], start, (uint32_t)st.cdf[v + 1] - start, kPrecision)) {
            dec_refill(x[lane], pcur < n_words ? rd(pay0 + pcur) : 0u);
            ++pcur;
        }
        int value = v + t.offsets[st.ci];
        if (v == st.max_value) {
            value = ecur < n_esc ? (int)rd(esc0 + ecur) : 0;
            ++ecur;
        }
        sym_out[st.pos] = value;
    }
}

static void fill_unowned_host(int C, int H, int W, int parity, const float* params, int ldp, int M, int* sym_out) {
    if (parity < 0) return;
    for (int c = 0; c < C; ++c)
        for (int h = 0; h < H; ++h)
            for (int w = 0; w < W; ++w)
                if (!keep(parity, h, w))
                    sym_out[((long long)c * H + h) * W + w] =
                        (int)rintf(0.f - params[((long long)h * W + w) * ldp + M + c]);
}

}  // namespace wrans
}  // namespace hyres

using namespace hyres;

extern "C" {

long long hyres_wrans_count(int C, int H, int W, int parity) {
    if (C < 1 || H < 1 || W < 1 || parity < -1 || parity > 1) return -1;
    return wrans::count(C, H, W, parity);
}

long long hyres_wrans_max_string_bytes(int C, int H, int W, int parity) {
    const long long n = hyres_wrans_count(C, H, W, parity);
    return n < 0 ? -1 : wrans::max_string_bytes(n);
}

long long hyres_wrans_workspace_bytes(int B, int C, int H, int W, int parity) {
    const long long n = hyres_wrans_count(C, H, W, parity);
    if (n < 0 || n > wrans::kMaxSymbols || B < 1) return -1;
    return wrans::align16(4ll * B) + 4ll * B * wrans::slot_words(n);
}

int hyres_wrans_encode(const int* sym, const int* idx, int B, int C, int H, int W, int parity, const int* cdfs,
                       int cdf_stride, const int* cdf_sizes, const int* offsets, int ncdf, unsigned char* out,
                       long long out_cap, long long* offs, int chain, void* ws, long long ws_bytes,
                       hyres_stream_t s) {
    long long n = 0;
    if (int rc = wrans::check_shape("wrans_encode", B, C, H, W, parity, &n)) return rc;
    if (int rc = wrans::check_tables("wrans_encode", cdfs, cdf_stride, cdf_sizes, offsets, ncdf)) return rc;
    HY_REQUIRE(sym && out && offs && ws && (chain == 0 || chain == 1), HYRES_E_ARG, "wrans_encode: NULL or bad chain");
    HY_REQUIRE(idx || C <= ncdf, HYRES_E_ARG, "wrans_encode: no indexes and C = %d > ncdf = %d", C, ncdf);
    HY_REQUIRE(aligned16(ws) && (reinterpret_cast<uintptr_t>(out) & 3u) == 0, HYRES_E_ALIGN,
               "wrans_encode: workspace 16-byte, output 4-byte aligned");
    HY_REQUIRE(ws_bytes >= hyres_wrans_workspace_bytes(B, C, H, W, parity), HYRES_E_WORKSPACE,
               "wrans_encode: workspace %lld < %lld", ws_bytes, hyres_wrans_workspace_bytes(B, C, H, W, parity));
    HY_REQUIRE(out_cap >= 0, HYRES_E_ARG, "wrans_encode: out_cap %lld", out_cap);
    int* lens = static_cast<int*>(ws);
    uint32_t* slots = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(ws) + wrans::align16(4ll * B));
    const wrans::Tables t{cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
    const long long chw = (long long)C * H * W, plane = wrans::plane_count(H, W, parity);
    hipLaunchKernelGGL(wrans::wrans_encode_kernel, dim3(B), dim3(64), 0, as_stream(s), sym, idx, H, W, parity, chw,
                       plane, (int)n, t, slots, lens);
    if (int rc = HY_LAUNCH_CHECK("wrans_encode")) return rc;
    hipLaunchKernelGGL(wrans::wrans_pack_kernel, dim3(B), dim3(64), 0, as_stream(s), slots, lens, (int)n, chain,
                       reinterpret_cast<uint32_t*>(out), out_cap >> 2, offs);
    return HY_LAUNCH_CHECK("wrans_pack");
}

int hyres_wrans_decode(const unsigned char* strings, const long long* offs, const int* idx, int B, int C, int H, int W,
                       int parity, const int* cdfs, int cdf_stride, const int* cdf_sizes, const int* offsets, int ncdf,
                       const float* params, int ldp, int M, int* sym_out, hyres_stream_t s) {
    long long n = 0;
    if (int rc = wrans::check_shape("wrans_decode", B, C, H, W, parity, &n)) return rc;
    if (int rc = wrans::check_tables("wrans_decode", cdfs, cdf_stride, cdf_sizes, offsets, ncdf)) return rc;
    HY_REQUIRE(strings && offs && sym_out, HYRES_E_ARG, "wrans_decode: NULL");
    HY_REQUIRE(idx || C <= ncdf, HYRES_E_ARG, "wrans_decode: no indexes and C = %d > ncdf = %d", C, ncdf);
    HY_REQUIRE(parity < 0 || (params && M == C && ldp >= 2 * M), HYRES_E_ARG,
               "wrans_decode: a checkerboard pass needs params [.., scales(M) | means(M)] with M = C");
    HY_REQUIRE((reinterpret_cast<uintptr_t>(strings) & 3u) == 0, HYRES_E_ALIGN, "wrans_decode: strings 4-byte aligned");
    const wrans::Tables t{cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
    const long long chw = (long long)C * H * W, plane = wrans::plane_count(H, W, parity);
    hipLaunchKernelGGL(wrans::wrans_decode_kernel, dim3(B), dim3(64), 0, as_stream(s), strings, offs, idx, H, W,
                       parity, chw, plane, (int)n, t, params, ldp, M, sym_out);
    return HY_LAUNCH_CHECK("wrans_decode");
}

int hyres_wrans_validate(const unsigned char* in, long long in_len, int C, int H, int W, int parity) {
    long long n = 0;
    if (int rc = wrans::check_shape("wrans_validate", 1, C, H, W, parity, &n)) return rc;
    HY_REQUIRE(in && in_len >= 0, HYRES_E_ARG, "wrans_validate: NULL");
    wrans::Header h{};
    const int e = wrans::check_header(in, in_len, n, h);
    HY_REQUIRE(e == wrans::kOk, HYRES_E_ARG, "wrans_validate: %lld-byte string: %s", in_len, wrans::header_error(e));
    return ok();
}

int hyres_wrans_encode_host(const int* sym, const int* idx, int C, int H, int W, int parity, const int* cdfs,
                            int cdf_stride, const int* cdf_sizes, const int* offsets, int ncdf, unsigned char* out,
                            long long out_cap, long long* out_len) {
    long long n = 0;
    if (int rc = wrans::check_shape("wrans_encode_host", 1, C, H, W, parity, &n)) return rc;
    if (int rc = wrans::check_tables("wrans_encode_host", cdfs, cdf_stride, cdf_sizes, offsets, ncdf)) return rc;
    HY_REQUIRE(sym && out_len, HYRES_E_ARG, "wrans_encode_host: NULL");
    HY_REQUIRE(idx || C <= ncdf, HYRES_E_ARG, "wrans_encode_host: no indexes and C = %d > ncdf = %d", C, ncdf);
    const wrans::Tables t{cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
    const long long plane = wrans::plane_count(H, W, parity);
    uint64_t x[wrans::kLanes];
    std::vector<uint32_t> pay_rev, esc_rev;
    if (int rc = wrans::encode_rows_host("wrans_encode_host", sym, idx, 0, n, H, W, parity, plane, t, x, pay_rev,
                                         esc_rev))
        return rc;
    const long long len = wrans::kFixedBytes + 4ll * (long long)(pay_rev.size() + esc_rev.size());
    *out_len = len;
    if (!out) return ok();  // size query
    HY_REQUIRE(out_cap >= len, HYRES_E_WORKSPACE, "wrans_encode_host: output buffer %lld < %lld", out_cap, len);
    std::vector<uint32_t> words;
    words.reserve((size_t)(len / 4));
    words.push_back(wrans::kMagic);
    words.push_back((uint32_t)n);
    words.push_back((uint32_t)esc_rev.size());
    words.push_back((uint32_t)pay_rev.size());
    wrans::push_states(words, x);
    words.insert(words.end(), esc_rev.rbegin(), esc_rev.rend());
    words.insert(words.end(), pay_rev.rbegin(), pay_rev.rend());
    wrans::store_le(out, words);
    return ok();
}

int hyres_wrans_decode_host(const unsigned char* in, long long in_len, const int* idx, int C, int H, int W, int parity,
                            const int* cdfs, int cdf_stride, const int* cdf_sizes, const int* offsets, int ncdf,
                            const float* params, int ldp, int M, int* sym_out) {
    if (int rc = hyres_wrans_validate(in, in_len, C, H, W, parity)) return rc;
    if (int rc = wrans::check_tables("wrans_decode_host", cdfs, cdf_stride, cdf_sizes, offsets, ncdf)) return rc;
    HY_REQUIRE(sym_out, HYRES_E_ARG, "wrans_decode_host: NULL");
    HY_REQUIRE(idx || C <= ncdf, HYRES_E_ARG, "wrans_decode_host: no indexes and C = %d > ncdf = %d", C, ncdf);
    HY_REQUIRE(parity < 0 || (params && M == C && ldp >= 2 * M), HYRES_E_ARG,
               "wrans_decode_host: a checkerboard pass needs params [.., scales(M) | means(M)] with M = C");
    const wrans::Tables t{cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
    const long long n = wrans::count(C, H, W, parity), plane = wrans::plane_count(H, W, parity);
    const long long lw = in_len / 4;
    auto rd = [&](long long i) -> uint32_t { return i < lw ? wrans::ld32(in + 4 * i) : 0u; };
    const long long n_esc = rd(2), n_words = rd(3);  // validated: the string holds them
    wrans::decode_rows_host(rd, idx, 0, n, H, W, parity, plane, t, wrans::kHeaderWords, wrans::kFixedWords, n_esc,
                            wrans::kFixedWords + n_esc, n_words, sym_out);
    wrans::fill_unowned_host(C, H, W, parity, params, ldp, M, sym_out);
    return ok();
}

// ---------------------------------------------------------------- HRW2
long long hyres_wrans2_segments(int C, int H, int W, int parity, int seg_rows) {
    const long long n = hyres_wrans_count(C, H, W, parity);
    if (n < 0 || seg_rows < 1) return -1;
    return wrans::segments(n, seg_rows);
}

long long hyres_wrans2_max_string_bytes(int C, int H, int W, int parity, int seg_rows) {
    const long long S = hyres_wrans2_segments(C, H, W, parity, seg_rows);
    return S < 0 ? -1 : wrans::max_string_bytes2(hyres_wrans_count(C, H, W, parity), S);
}

long long hyres_wrans2_workspace_bytes(int B, int C, int H, int W, int parity, int seg_rows) {
    const long long n = hyres_wrans_count(C, H, W, parity), S = hyres_wrans2_segments(C, H, W, parity, seg_rows);
    if (S < 0 || n > wrans::kMaxSymbols || B < 1 || B > 65535) return -1;
    return wrans::align16(8ll * B) + wrans::align16(8ll * B * S) + 4ll * B * wrans::slot_words2(n, S);
}

int hyres_wrans2_encode(const int* sym, const int* idx, int B, int C, int H, int W, int parity, const int* cdfs,
                        int cdf_stride, const int* cdf_sizes, const int* offsets, int ncdf, int seg_rows,
                        unsigned char* out, long long out_cap, long long* offs, int chain, void* ws, long long ws_bytes,
                        hyres_stream_t s) {
    long long n = 0, S = 0;
    if (int rc = wrans::check_shape2("wrans2_encode", B, C, H, W, parity, seg_rows, &n, &S)) return rc;
    if (int rc = wrans::check_tables("wrans2_encode", cdfs, cdf_stride, cdf_sizes, offsets, ncdf)) return rc;
    HY_REQUIRE(sym && out && offs && ws && (chain == 0 || chain == 1), HYRES_E_ARG, "wrans2_encode: NULL or bad chain");
    HY_REQUIRE(idx || C <= ncdf, HYRES_E_ARG, "wrans2_encode: no indexes and C = %d > ncdf = %d", C, ncdf);
    HY_REQUIRE(aligned16(ws) && (reinterpret_cast<uintptr_t>(out) & 3u) == 0, HYRES_E_ALIGN,
               "wrans2_encode: workspace 16-byte, output 4-byte aligned");
    const long long need = hyres_wrans2_workspace_bytes(B, C, H, W, parity, seg_rows);
    HY_REQUIRE(ws_bytes >= need, HYRES_E_WORKSPACE, "wrans2_encode: workspace %lld < %lld", ws_bytes, need);
    HY_REQUIRE(out_cap >= 0, HYRES_E_ARG, "wrans2_encode: out_cap %lld", out_cap);
    unsigned char* p = static_cast<unsigned char*>(ws);
    long long* lens = reinterpret_cast<long long*>(p);
    uint32_t* dir = reinterpret_cast<uint32_t*>(p + wrans::align16(8ll * B));
    uint32_t* slots = reinterpret_cast<uint32_t*>(p + wrans::align16(8ll * B) + wrans::align16(8ll * B * S));
    const wrans::Tables t{cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
    const long long chw = (long long)C * H * W, plane = wrans::plane_count(H, W, parity);
    const long long seg = wrans::seg_symbols(seg_rows);
    const dim3 grid((unsigned)S, (unsigned)B);
    hipLaunchKernelGGL(wrans::wrans2_encode_kernel, grid, dim3(64), 0, as_stream(s), sym, idx, H, W, parity, chw, plane,
                       (int)n, seg, (int)S, t, slots, dir);
    if (int rc = HY_LAUNCH_CHECK("wrans2_encode")) return rc;
    hipLaunchKernelGGL(wrans::wrans2_scan_kernel, dim3(B), dim3(64), 0, as_stream(s), dir, (int)S, lens);
    if (int rc = HY_LAUNCH_CHECK("wrans2_scan")) return rc;
    hipLaunchKernelGGL(wrans::wrans2_pack_kernel, grid, dim3(64), 0, as_stream(s), slots, dir, lens, (int)n, seg_rows,
                       seg, (int)S, chain, reinterpret_cast<uint32_t*>(out), out_cap >> 2, offs);
    return HY_LAUNCH_CHECK("wrans2_pack");
}

int hyres_wrans2_decode(const unsigned char* strings, const long long* offs, const int* idx, int B, int C, int H, int W,
                        int parity, int seg_rows, const int* cdfs, int cdf_stride, const int* cdf_sizes,
                        const int* offsets, int ncdf, const float* params, int ldp, int M, int* sym_out,
                        hyres_stream_t s) {
    long long n = 0, S = 0;
    if (int rc = wrans::check_shape2("wrans2_decode", B, C, H, W, parity, seg_rows, &n, &S)) return rc;
    if (int rc = wrans::check_tables("wrans2_decode", cdfs, cdf_stride, cdf_sizes, offsets, ncdf)) return rc;
    HY_REQUIRE(strings && offs && sym_out, HYRES_E_ARG, "wrans2_decode: NULL");
    HY_REQUIRE(idx || C <= ncdf, HYRES_E_ARG, "wrans2_decode: no indexes and C = %d > ncdf = %d", C, ncdf);
    HY_REQUIRE(parity < 0 || (params && M == C && ldp >= 2 * M), HYRES_E_ARG,
               "wrans2_decode: a checkerboard pass needs params [.., scales(M) | means(M)] with M = C");
    HY_REQUIRE((reinterpret_cast<uintptr_t>(strings) & 3u) == 0, HYRES_E_ALIGN, "wrans2_decode: strings 4-byte aligned");
    const wrans::Tables t{cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
    const long long chw = (long long)C * H * W, plane = wrans::plane_count(H, W, parity);
    hipLaunchKernelGGL(wrans::wrans2_decode_kernel, dim3((unsigned)S, (unsigned)B), dim3(64), 0, as_stream(s), strings,
                       offs, idx, H, W, parity, chw, plane, (int)n, wrans::seg_symbols(seg_rows), (int)S, t, params, ldp,
                       M, sym_out);
    return HY_LAUNCH_CHECK("wrans2_decode");
}

int hyres_wrans2_validate(const unsigned char* in, long long in_len, int C, int H, int W, int parity,
                          int* seg_rows_out) {
    long long n = 0;
    if (int rc = wrans::check_shape("wrans2_validate", 1, C, H, W, parity, &n)) return rc;
    HY_REQUIRE(in && in_len >= 0, HYRES_E_ARG, "wrans2_validate: NULL");
    wrans::Header2 h{};
    const int e = wrans::check_header2(in, in_len, n, h);
    HY_REQUIRE(e == wrans::kOk, HYRES_E_ARG, "wrans2_validate: %lld-byte string: %s", in_len, wrans::header_error(e));
    HY_REQUIRE(h.R <= 0x7fffffffu, HYRES_E_ARG, "wrans2_validate: %u rows per segment: more than this interface takes",
               h.R);
    if (seg_rows_out) *seg_rows_out = (int)h.R;
    return ok();
}

int hyres_wrans2_encode_host(const int* sym, const int* idx, int C, int H, int W, int parity, const int* cdfs,
                             int cdf_stride, const int* cdf_sizes, const int* offsets, int ncdf, int seg_rows,
                             unsigned char* out, long long out_cap, long long* out_len) {
    long long n = 0, S = 0;
    if (int rc = wrans::check_shape2("wrans2_encode_host", 1, C, H, W, parity, seg_rows, &n, &S)) return rc;
    if (int rc = wrans::check_tables("wrans2_encode_host", cdfs, cdf_stride, cdf_sizes, offsets, ncdf)) return rc;
    HY_REQUIRE(sym && out_len, HYRES_E_ARG, "wrans2_encode_host: NULL");
    HY_REQUIRE(idx || C <= ncdf, HYRES_E_ARG, "wrans2_encode_host: no indexes and C = %d > ncdf = %d", C, ncdf);
    const wrans::Tables t{cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
    const long long plane = wrans::plane_count(H, W, parity), seg = wrans::seg_symbols(seg_rows);
    std::vector<uint32_t> dir, states, esc, pay, pay_rev, esc_rev;
    for (long long sg = 0; sg < S; ++sg) {
        uint64_t x[wrans::kLanes];
        pay_rev.clear();
        esc_rev.clear();
        const long long k0 = seg * sg, k1 = std::min(n, k0 + seg);
        if (int rc = wrans::encode_rows_host("wrans2_encode_host", sym, idx, k0, k1, H, W, parity, plane, t, x, pay_rev,
                                             esc_rev))
            return rc;
        wrans::push_states(states, x);
        esc.insert(esc.end(), esc_rev.rbegin(), esc_rev.rend());
        pay.insert(pay.end(), pay_rev.rbegin(), pay_rev.rend());
        dir.push_back((uint32_t)esc.size());
        dir.push_back((uint32_t)pay.size());
    }
    const long long len = 4 * (wrans::fixed_words2(S) + (long long)(esc.size() + pay.size()));
    *out_len = len;
    if (!out) return ok();  // size query
    HY_REQUIRE(out_cap >= len, HYRES_E_WORKSPACE, "wrans2_encode_host: output buffer %lld < %lld", out_cap, len);
    std::vector<uint32_t> words{wrans::kMagic2, (uint32_t)n, (uint32_t)seg_rows, (uint32_t)S};
    words.reserve((size_t)(len / 4));
    for (const auto* part : {&dir, &states, &esc, &pay}) words.insert(words.end(), part->begin(), part->end());
    wrans::store_le(out, words);
    return ok();
}

int hyres_wrans2_decode_host(const unsigned char* in, long long in_len, const int* idx, int C, int H, int W,
                             int parity, const int* cdfs, int cdf_stride, const int* cdf_sizes, const int* offsets,
                             int ncdf, const float* params, int ldp, int M, int* sym_out) {
    int R = 0;
    if (int rc = hyres_wrans2_validate(in, in_len, C, H, W, parity, &R)) return rc;
    if (int rc = wrans::check_tables("wrans2_decode_host", cdfs, cdf_stride, cdf_sizes, offsets, ncdf)) return rc;
    HY_REQUIRE(sym_out, HYRES_E_ARG, "wrans2_decode_host: NULL");
    HY_REQUIRE(idx || C <= ncdf, HYRES_E_ARG, "wrans2_decode_host: no indexes and C = %d > ncdf = %d", C, ncdf);
    HY_REQUIRE(parity < 0 || (params && M == C && ldp >= 2 * M), HYRES_E_ARG,
               "wrans2_decode_host: a checkerboard pass needs params [.., scales(M) | means(M)] with M = C");
    const wrans::Tables t{cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
    const long long n = wrans::count(C, H, W, parity), plane = wrans::plane_count(H, W, parity);
    const long long S = wrans::segments(n, R), seg = wrans::seg_symbols(R), lw = in_len / 4;
    auto rd = [&](long long i) -> uint32_t { return i < lw ? wrans::ld32(in + 4 * i) : 0u; };
    const long long body = wrans::fixed_words2(S), n_esc_all = rd(wrans::kHeader2Words + 2 * (S - 1));
    long long e0 = 0, w0 = 0;  // validated: the directory is non-decreasing and the string holds what it counts
    for (long long sg = 0; sg < S; ++sg) {
        const long long e1 = rd(wrans::kHeader2Words + 2 * sg), w1 = rd(wrans::kHeader2Words + 2 * sg + 1);
        const long long k0 = seg * sg, k1 = std::min(n, k0 + seg);
        wrans::decode_rows_host(rd, idx, k0, k1, H, W, parity, plane, t,
                                wrans::kHeader2Words + 2 * S + 2ll * wrans::kLanes * sg, body + e0, e1 - e0,
                                body + n_esc_all + w0, w1 - w0, sym_out);
        e0 = e1;
        w0 = w1;
    }
    wrans::fill_unowned_host(C, H, W, parity, params, ldp, M, sym_out);
    return ok();
}

}  // extern "C"
