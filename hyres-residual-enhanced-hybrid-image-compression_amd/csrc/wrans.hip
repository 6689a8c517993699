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
#include "common.h"
#include "wrans_core.h"

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
    for (auto& v : x) v = wrans::kL;
    std::vector<uint32_t> pay_rev, esc_rev;  // rows last to first, lanes last to first: the reverse of the string's order
    for (long long r = (n + wrans::kLanes - 1) / wrans::kLanes - 1; r >= 0; --r) {
        for (int lane = wrans::kLanes - 1; lane >= 0; --lane) {
            const long long k = r * wrans::kLanes + lane;
            if (k >= n) continue;
            const wrans::Step st = wrans::step_of(k, idx, H, W, parity, plane, t);
            bool is_esc = false;
            const int raw = sym[st.pos];
            const int v = wrans::slot_of(raw, offsets[st.ci], st.max_value, is_esc);
            const uint32_t start = (uint32_t)st.cdf[v];
            const uint32_t freq = (uint32_t)st.cdf[v + 1] - start;
            HY_REQUIRE(freq > 0 && freq <= (1u << wrans::kPrecision), HYRES_E_ARG,
                       "wrans_encode_host: CDF %d is not strictly increasing at slot %d", st.ci, v);
            uint32_t word = 0;
            if (wrans::enc_put(x[lane], start, freq, wrans::kPrecision, word)) pay_rev.push_back(word);
            if (is_esc) esc_rev.push_back((uint32_t)raw);
        }
    }
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
    for (int lane = 0; lane < wrans::kLanes; ++lane) {
        words.push_back((uint32_t)x[lane]);
        words.push_back((uint32_t)(x[lane] >> 32));
    }
    words.insert(words.end(), esc_rev.rbegin(), esc_rev.rend());
    words.insert(words.end(), pay_rev.rbegin(), pay_rev.rend());
    for (size_t i = 0; i < words.size(); ++i) {  // little endian, whatever the host
        const uint32_t w = words[i];
        out[4 * i] = (unsigned char)w;
        out[4 * i + 1] = (unsigned char)(w >> 8);
        out[4 * i + 2] = (unsigned char)(w >> 16);
        out[4 * i + 3] = (unsigned char)(w >> 24);
    }
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
    const long long esc0 = wrans::kFixedWords, pay0 = wrans::kFixedWords + n_esc;
    long long ecur = 0, pcur = 0;
    uint64_t x[wrans::kLanes];
    for (int lane = 0; lane < wrans::kLanes; ++lane)
        x[lane] = (uint64_t)rd(wrans::kHeaderWords + 2 * lane) | ((uint64_t)rd(wrans::kHeaderWords + 2 * lane + 1) << 32);
    for (long long k = 0; k < n; ++k) {  // rows first to last, lanes in ascending order: the string's order
        const int lane = (int)(k % wrans::kLanes);
        const wrans::Step st = wrans::step_of(k, idx, H, W, parity, plane, t);
        const int v = wrans::cdf_search(st.cdf, st.max_value, wrans::dec_get(x[lane], wrans::kPrecision));
        const uint32_t start = (uint32_t)st.cdf[v];
        if (wrans::dec_advance(x[lane], start, (uint32_t)st.cdf[v + 1] - start, wrans::kPrecision)) {
            wrans::dec_refill(x[lane], pcur < n_words ? rd(pay0 + pcur) : 0u);
            ++pcur;
        }
        int value = v + offsets[st.ci];
        if (v == st.max_value) {
            value = ecur < n_esc ? (int)rd(esc0 + ecur) : 0;
            ++ecur;
        }
        sym_out[st.pos] = value;
    }
    if (parity >= 0) {
        for (int c = 0; c < C; ++c)
            for (int h = 0; h < H; ++h)
                for (int w = 0; w < W; ++w)
                    if (!wrans::keep(parity, h, w))
                        sym_out[((long long)c * H + h) * W + w] =
                            (int)rintf(0.f - params[((long long)h * W + w) * ldp + M + c]);
    }
    return ok();
}

}  // extern "C"
