// bpe_lines.hip.h — lines as samples: the corpus helpers of core.ts:55-75 as a device transform on
// UTF-16 units, in front of the ingest and the restore (include/bpe.h "lines as samples").
// Included by bpe_encode.hip (the split on an encoder) and bpe_engine.hip (on a context); everything
// here has internal linkage, like bpe_utf8.hip.h, and uses the scans of bpe_text_front.hip.h.
//
// A batch of texts becomes a batch of samples, exactly texts.flatMap(helper):
//   BPE_LINES_TRIM  linesToCorpus          cut at every U+000A, each piece p -> CR + p.trim() + LF
//   BPE_LINES_KEEP  linesTrimmedToCorpus   the same cut, one trailing CR dropped from p, the same wrap
//   BPE_LINES_FILE  fileContentToCorpus    one sample per text: U+001C + text + U+0004
// A text with m line feeds gives m + 1 samples; sample LF(before b) + k starts at b in text k.
//
// The two ends of a line [b, e) are found independently and never walked: with nw(g)
// "slot g holds a unit that trim() keeps", begin' = the first g >= b with nw(g), end' = 1 + the last
// g < e with nw(g), both unclipped, and length = max(0, end' - begin'): a line without such a unit
// has end' <= b <= e <= begin'.  KEEP takes begin' = b and end' = e - (the unit at e - 1 is CR).
//
// Tiling: tiles of BPE_TEXT_TILE units cut at 16-B addresses of the unit buffer; slot g = t * TILE + s
// holds the flat position g - mis.  All positions below are slots.
//   k_ln_tile    per tile: the lane rule (ln_classify) as two bit planes, LF and nw, LFs before each
//                plane word, the tile's LF count, its words-with-nw mask, its first and last nw slot;
//   k_txt_scan   (bpe_text_front.hip.h) exclusive scan of the tiles' LF counts;
//   k_ln_summ    suffix-min of the first and prefix-max of the last nw slots over the tiles;
//   k_ln_bounds  one thread per LF-plane word and one per text: begin' and end' of every sample;
//   k_ln_len     lengths + 2, scanned by k_txt_scan into the samples' offsets;
//   k_ln_emit    output-centric: 16 B per lane at 16-B addresses of the output (partial head and
//                tail), the lane's sample found by a search in the offsets.
//
// With BPE_LINES_RULE_ONLY defined only the rule is compiled, as plain C++ (a stand-alone host
// program runs it over the fixture: tests/lines_rule_main.cc).
#pragma once

#ifdef BPE_LINES_RULE_ONLY
#include <cstdint>
#define LN_FN inline
#ifndef BPE_TEXT_TILE
#define BPE_TEXT_TILE 2048
#endif
#ifndef BPE_LINES_TRIM
#define BPE_LINES_TRIM 0
#define BPE_LINES_KEEP 1
#define BPE_LINES_FILE 2
#endif
#else
#include "bpe_multi.h"            // bpe_fail
#include "bpe_text_front.hip.h"   // txt_load, txt_valid, k_txt_scan, TS_CHARS
#define LN_FN __host__ __device__ __forceinline__
#endif

namespace {

constexpr int LN_TILE = BPE_TEXT_TILE;
constexpr int LN_RUN = 8;                    // units per lane
constexpr int LN_WORDS = LN_TILE / 32;       // plane words per tile
constexpr long long LN_INF = 0x3FFFFFFFFFFFFFFFll;
static_assert(LN_WORDS == 64, "a tile's words-with-nw mask is one 64-bit word");

struct LnMasks {
    uint32_t lf;   // bit j: slot j of the run holds U+000A
    uint32_t nw;   // bit j: slot j holds a unit of the batch that trim() keeps
};

// The 25 units ECMAScript calls WhiteSpace or LineTerminator: 0009-000D, 0020, 00A0, 1680,
// 2000-200A, 2028, 2029, 202F, 205F, 3000, FEFF.
LN_FN bool ln_is_ws(uint32_t x) {
    return x - 0x9u <= 4u || x == 0x20u || x == 0xA0u || x == 0x1680u || x - 0x2000u <= 0xAu || x - 0x2028u <= 1u ||
           x == 0x202Fu || x == 0x205Fu || x == 0x3000u || x == 0xFEFFu;
}

// u[j]: the unit at slot j of the run; valid: bits of the run's slots inside the batch
LN_FN LnMasks ln_classify(const uint32_t u[LN_RUN], uint32_t valid) {
    LnMasks m{0, 0};
#pragma unroll
    for (int j = 0; j < LN_RUN; ++j) {
        m.lf |= (uint32_t)(u[j] == 0xAu) << j;
        m.nw |= (uint32_t)(!ln_is_ws(u[j])) << j;
    }
    m.lf &= valid;
    m.nw &= valid;
    return m;
}

// What the per-tile pass and the two scans leave behind.
struct LnPlanes {
    const uint32_t *lf, *nw;              // bit b of word w: slot 32 * w + b
    const uint32_t *lfpre;                // LFs of the tile before each word
    const unsigned long long *nwsum;      // per tile, bit w: word w of the tile has a nw bit
    const unsigned long long *tile_base;  // LFs before each tile
    const long long *sfx_first;           // the first nw slot of this tile or a later one (LN_INF)
    const long long *pfx_last;            // the last nw slot of this tile or an earlier one (-1)
    int64_t n_tiles, lf_total;
};

LN_FN int ln_ctz32(uint32_t x) { return __builtin_ctz(x); }
LN_FN int ln_ctz64(unsigned long long x) { return __builtin_ctzll(x); }
LN_FN int ln_top32(uint32_t x) { return 31 - __builtin_clz(x); }
LN_FN int ln_top64(unsigned long long x) { return 63 - __builtin_clzll(x); }

// the first nw slot at or after g (LN_INF: none)
LN_FN long long ln_next_nw(const LnPlanes &P, int64_t g) {
    if (g >= P.n_tiles * LN_TILE) return LN_INF;
    const int64_t t = g / LN_TILE;
    const int w = (int)(g % LN_TILE) >> 5, b = (int)(g & 31);
    const uint32_t x = P.nw[t * LN_WORDS + w] & (~0u << b);
    if (x) return t * LN_TILE + 32 * w + ln_ctz32(x);
    const unsigned long long s = w == LN_WORDS - 1 ? 0ull : P.nwsum[t] & (~0ull << (w + 1));
    if (s) {
        const int w2 = ln_ctz64(s);
        return t * LN_TILE + 32 * w2 + ln_ctz32(P.nw[t * LN_WORDS + w2]);
    }
    return t + 1 < P.n_tiles ? P.sfx_first[t + 1] : LN_INF;
}

// the last nw slot at or before g (-1: none); g < n_tiles * TILE
LN_FN long long ln_prev_nw(const LnPlanes &P, int64_t g) {
    if (g < 0) return -1;
    const int64_t t = g / LN_TILE;
    const int w = (int)(g % LN_TILE) >> 5, b = (int)(g & 31);
    const uint32_t x = P.nw[t * LN_WORDS + w] & (b == 31 ? ~0u : (1u << (b + 1)) - 1u);
    if (x) return t * LN_TILE + 32 * w + ln_top32(x);
    const unsigned long long s = P.nwsum[t] & ((1ull << w) - 1ull);
    if (s) {
        const int w2 = ln_top64(s);
        return t * LN_TILE + 32 * w2 + ln_top32(P.nw[t * LN_WORDS + w2]);
    }
    return t > 0 ? P.pfx_last[t - 1] : -1;
}

// LFs at slots below g
LN_FN int64_t ln_lf_before(const LnPlanes &P, int64_t g) {
    if (g >= P.n_tiles * LN_TILE) return P.lf_total;
    const int64_t t = g / LN_TILE, wi = g >> 5;
    return (int64_t)P.tile_base[t] + P.lfpre[wi] + __builtin_popcount(P.lf[wi] & ((1u << (g & 31)) - 1u));
}

// begin' of a line that starts at slot b, end' of one that ends before slot e (units_al[g]: the
// unit at slot g; no slot below mis is read)
LN_FN long long ln_begin(const LnPlanes &P, int mode, int64_t b) {
    return mode == BPE_LINES_TRIM ? ln_next_nw(P, b) : b;
}

LN_FN long long ln_end(const LnPlanes &P, const uint16_t *units_al, int mis, int mode, int64_t e) {
    if (mode == BPE_LINES_TRIM) return ln_prev_nw(P, e - 1) + 1;
    return e - (int64_t)(e - 1 >= mis && units_al[e - 1] == 0xDu);
}

// the text that holds flat position p (0 <= p < total): the last k with off[k] - base <= p
LN_FN int64_t ln_text_of(const int64_t *off, int64_t n_texts, int64_t base, int64_t p) {
    int64_t lo = 0, hi = n_texts;   // off[lo] - base <= p < off[hi] - base
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (off[mid] - base <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// The LFs of plane word wi: each ends its sample and begins the next one.
LN_FN void ln_word_bounds(const LnPlanes &P, const uint16_t *units_al, int mis, int mode, const int64_t *off,
                          int64_t n_texts, int64_t base, int64_t wi, long long *sb, long long *se) {
    uint32_t x = P.lf[wi];
    if (!x) return;
    int64_t rank = (int64_t)P.tile_base[wi / LN_WORDS] + P.lfpre[wi];
    int64_t k = -1;
    while (x) {   // (at most 32 steps, whatever the lines are)
        const int64_t g = wi * 32 + ln_ctz32(x);
        x &= x - 1;
        if (k < 0 || off[k + 1] - base <= g - mis) k = ln_text_of(off, n_texts, base, g - mis);
        const int64_t idx = rank + k;
        ++rank;
        se[idx] = ln_end(P, units_al, mis, mode, g);
        sb[idx + 1] = ln_begin(P, mode, g + 1);
    }
}

// Text k: its start begins a sample, its end ends one.
LN_FN void ln_text_bounds(const LnPlanes &P, const uint16_t *units_al, int mis, int mode, const int64_t *off,
                          int64_t base, int64_t k, long long *sb, long long *se) {
    const int64_t gb = off[k] - base + mis, ge = off[k + 1] - base + mis;
    sb[ln_lf_before(P, gb) + k] = ln_begin(P, mode, gb);
    se[ln_lf_before(P, ge) + k] = ln_end(P, units_al, mis, mode, ge);
}

LN_FN long long ln_length(long long b, long long e) { return (e > b ? e - b : 0) + 2; }

// Output unit o of the batch, o in sample j = [start, next): a marker at either end, else a unit.
LN_FN uint32_t ln_unit_at(const uint16_t *units_al, int mode, int64_t o, int64_t start, int64_t next, long long b) {
    if (o == start) return mode == BPE_LINES_FILE ? 0x1Cu : 0xDu;
    if (o == next - 1) return mode == BPE_LINES_FILE ? 0x4u : 0xAu;
    return units_al[b + (o - start - 1)];
}

}  // namespace

#ifndef BPE_LINES_RULE_ONLY

namespace {

constexpr int LN_WG = 256;
static_assert(LN_TILE == TXT_TILE && LN_RUN == TXT_RUN && LN_WG == TXT_WG, "the text front's tiles");

__global__ void __launch_bounds__(LN_WG)
k_ln_tile(const uint16_t *__restrict__ units_al, int mis, int64_t total, uint32_t *__restrict__ lf,
          uint32_t *__restrict__ nw, uint32_t *__restrict__ lfpre, unsigned long long *__restrict__ nwsum,
          unsigned long long *__restrict__ tile_cnt, long long *__restrict__ first, long long *__restrict__ last) {
    __shared__ __attribute__((aligned(4))) uint8_t s_lf[LN_WG], s_nw[LN_WG];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    uint32_t u[TXT_RUN + 2];
    int64_t p0;
    txt_load(units_al, tile, mis, total, u, p0);
    const LnMasks m = ln_classify(u + 1, txt_valid(p0, total));
    s_lf[tid] = (uint8_t)m.lf;
    s_nw[tid] = (uint8_t)m.nw;
    __syncthreads();
    if (tid >= LN_WORDS) return;   // (wave 0 goes on, whole)
    const uint32_t wl = reinterpret_cast<const uint32_t *>(s_lf)[tid];
    const uint32_t wn = reinterpret_cast<const uint32_t *>(s_nw)[tid];
    lf[tile * LN_WORDS + tid] = wl;
    nw[tile * LN_WORDS + tid] = wn;
    const int c = __builtin_popcount(wl);
    const int incl = wave_incl(c, tid);
    lfpre[tile * LN_WORDS + tid] = (uint32_t)(incl - c);
    const unsigned long long sum = __ballot(wn != 0);
    if (tid == LN_WORDS - 1) tile_cnt[tile] = (unsigned long long)incl;
    if (tid == 0) {
        nwsum[tile] = sum;
        long long f = LN_INF, l = -1;
        if (sum) {
            const int w0 = ln_ctz64(sum), w1 = ln_top64(sum);
            f = tile * LN_TILE + 32 * w0 + ln_ctz32(reinterpret_cast<const uint32_t *>(s_nw)[w0]);
            l = tile * LN_TILE + 32 * w1 + ln_top32(reinterpret_cast<const uint32_t *>(s_nw)[w1]);
        }
        first[tile] = f;
        last[tile] = l;
    }
}

template <bool MAXOP>
__device__ __forceinline__ long long ln_op(long long a, long long b) {
    return MAXOP ? (a > b ? a : b) : (a < b ? a : b);
}

// inclusive scan by max (forward over `last`) or min (backward over `first`), in place, in rounds
template <bool MAXOP>
__device__ __forceinline__ void ln_summ(long long *__restrict__ v, int64_t n, long long *ws) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long unit = MAXOP ? -1 : LN_INF;
    long long carry = unit;
    for (int64_t b = 0; b < n; b += 1024) {
        const int64_t i = b + threadIdx.x;
        const int64_t at = MAXOP ? i : n - 1 - i;
        long long x = i < n ? v[at] : unit;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long o = __shfl_up(x, d);
            if (lane >= d) x = ln_op<MAXOP>(x, o);
        }
        if (lane == 63) ws[w] = x;
        __syncthreads();
        long long before = carry, all = carry;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const long long y = ws[j];
            if (j < w) before = ln_op<MAXOP>(before, y);
            all = ln_op<MAXOP>(all, y);
        }
        if (i < n) v[at] = ln_op<MAXOP>(before, x);
        carry = all;
        __syncthreads();   // (ws is reused next round)
    }
}

__global__ void __launch_bounds__(1024)
k_ln_summ(long long *__restrict__ first, long long *__restrict__ last, int64_t n_tiles) {
    __shared__ long long ws[16];
    ln_summ<false>(first, n_tiles, ws);
    ln_summ<true>(last, n_tiles, ws);
}

// threads [0, n_words): the LFs of a plane word; threads [n_words, n_words + n_texts): a text
__global__ void __launch_bounds__(256)
k_ln_bounds(LnPlanes P, const uint16_t *__restrict__ units_al, int mis, int mode, const int64_t *__restrict__ off,
            int64_t n_texts, int64_t base, long long *__restrict__ sb, long long *__restrict__ se) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n_words = P.n_tiles * LN_WORDS;
    if (i < n_words) ln_word_bounds(P, units_al, mis, mode, off, n_texts, base, i, sb, se);
    else if (i - n_words < n_texts) ln_text_bounds(P, units_al, mis, mode, off, base, i - n_words, sb, se);
}

// BPE_LINES_FILE: sample k is text k
__global__ void __launch_bounds__(256)
k_ln_file(const int64_t *__restrict__ off, int64_t n_texts, int64_t base, int mis, long long *__restrict__ sb,
          long long *__restrict__ se) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_texts) return;
    sb[k] = off[k] - base + mis;
    se[k] = off[k + 1] - base + mis;
}

__global__ void __launch_bounds__(256)
k_ln_len(const long long *__restrict__ sb, const long long *__restrict__ se, int64_t n_samples,
         unsigned long long *__restrict__ len) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n_samples) len[j] = (unsigned long long)ln_length(sb[j], se[j]);
}

// Chunk c of eight units is one aligned 16-B word at out_al + 8 * c, out_al = out - a (a: the
// output's 16-B phase, 0..7 units); ooff holds n_samples + 1 offsets, ooff[n_samples] = n_out.
__global__ void __launch_bounds__(256)
k_ln_emit(const uint16_t *__restrict__ units_al, int mode, const long long *__restrict__ sb,
          const int64_t *__restrict__ ooff, int64_t n_samples, int64_t n_out, uint16_t *__restrict__ out, int a) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t lo = c * 8 - a;
    if (lo >= n_out) return;
    const int64_t o0 = lo < 0 ? 0 : lo;
    int64_t j = 0, hi = n_samples;   // ooff[j] <= o0 < ooff[hi]
    while (hi - j > 1) {
        const int64_t mid = j + (hi - j) / 2;
        if (ooff[mid] <= o0) j = mid; else hi = mid;
    }
    int64_t start = ooff[j], next = ooff[j + 1];
    long long b = sb[j];
    uint32_t v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t o = lo + i;
        v[i] = 0;
        if (o < 0 || o >= n_out) continue;
        if (o == next) {   // (a sample has at least its two markers: one step is enough)
            ++j;
            start = next, next = ooff[j + 1], b = sb[j];
        }
        v[i] = ln_unit_at(units_al, mode, o, start, next, b);
    }
    if (lo >= 0 && lo + 8 <= n_out) {
        uint4 x;
        x.x = v[0] | (v[1] << 16), x.y = v[2] | (v[3] << 16), x.z = v[4] | (v[5] << 16), x.w = v[6] | (v[7] << 16);
        *reinterpret_cast<uint4 *>(out + lo) = x;
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (lo + i >= 0 && lo + i < n_out) out[lo + i] = (uint16_t)v[i];
    }
}

#define LN_TRY(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return bpe_fail(e_ == hipErrorOutOfMemory ? BPE_ERR_OOM : BPE_ERR_HIP,         \
                            (std::string("bpe native: ") + #expr + ": " +                   \
                             hipGetErrorString(e_)).c_str());                              \
    } while (0)

}  // namespace

// Scratch (three grow-only buffers: the planes and staged input, the samples' bounds and offsets,
// the samples' units), status words, events and counters of the line split of an encoder or context.
struct LinesState {
    char *d_buf[3] = {nullptr, nullptr, nullptr};
    size_t d_cap[3] = {0, 0, 0};
    unsigned long long *d_st = nullptr, *h_st = nullptr;   // (2 x TS_WORDS; h_st pinned)
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bpe_lines_stats st{};
};

// One call's split.  In: the call's arguments.  Out: where the samples and their offsets are on the
// device and the call's numbers, which the caller adds to the counters once its whole pipeline has
// succeeded (ln_commit).
struct LinesCall {
    // in
    int mode = BPE_LINES_TRIM;
    const uint16_t *units = nullptr;   // text k = units[off[k] .. off[k+1])
    const int64_t *off = nullptr;
    int64_t n_texts = 0;
    bool dev = false;                  // units and off are device buffers
    uint16_t *d_out = nullptr;         // the caller's device output, or nullptr: into scratch
    int64_t *d_ooff = nullptr;         // ... its offsets, or nullptr: left in scratch
    int64_t units_cap = -1, off_cap = -1;   // what the caller's buffers hold; -1: whatever is needed
    // out
    int64_t total = 0, samples = 0, units_out = 0;
    double ms = 0;
    bool fits = true;                  // false: a capacity is too small, nothing was written
};

namespace {

inline void ln_free(LinesState &L) {
    for (char *p : L.d_buf)
        if (p) (void)hipFree(p);
    if (L.d_st) (void)hipFree(L.d_st);
    if (L.h_st) (void)hipHostFree(L.h_st);
    for (hipEvent_t &ev : L.ev)
        if (ev) (void)hipEventDestroy(ev);
    L = LinesState{};
}

inline size_t ln_align(size_t x) { return (x + 15) & ~(size_t)15; }

inline int ln_grow(LinesState &L, int which, size_t need, hipStream_t s) {
    if (need <= L.d_cap[which]) return BPE_OK;
    LN_TRY(hipStreamSynchronize(s));
    if (L.d_buf[which]) (void)hipFree(L.d_buf[which]);
    L.d_buf[which] = nullptr;
    L.d_cap[which] = 0;
    const size_t want = need + need / 4 + 4096;
    LN_TRY(hipMalloc((void **)&L.d_buf[which], want));
    L.d_cap[which] = want;
    return BPE_OK;
}

inline int ln_split(LinesState &L, hipStream_t s, LinesCall &J) {
    const int64_t n = J.n_texts;
    const int mode = J.mode;
    if (mode != BPE_LINES_TRIM && mode != BPE_LINES_KEEP && mode != BPE_LINES_FILE)
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad lines mode");
    if (n < 0 || n >= 0x7FFFFFFF || (n && !J.off)) return bpe_fail(BPE_ERR_ARG, "bpe native: bad lines batch arguments");
    std::vector<int64_t> h_off((size_t)n + 1, 0);
    if (n) {
        if (J.dev) {
            LN_TRY(hipMemcpyAsync(h_off.data(), J.off, h_off.size() * 8, hipMemcpyDeviceToHost, s));
            LN_TRY(hipStreamSynchronize(s));
        } else {
            std::copy(J.off, J.off + n + 1, h_off.begin());
        }
    }
    if (n && h_off[0] < 0) return bpe_fail(BPE_ERR_ARG, "bpe native: negative text offset");
    for (int64_t k = 0; k < n; ++k)
        if (h_off[(size_t)k + 1] < h_off[(size_t)k])
            return bpe_fail(BPE_ERR_ARG, "bpe native: text offsets must not decrease");
    const int64_t base0 = n ? h_off[0] : 0, total = n ? h_off[(size_t)n] - base0 : 0;
    if (total && !J.units) return bpe_fail(BPE_ERR_ARG, "bpe native: null unit buffer");
    if (J.dev && total && ((uintptr_t)J.units & 1)) return bpe_fail(BPE_ERR_ARG, "bpe native: misaligned unit buffer");
    J.total = total;
    J.samples = J.units_out = 0;
    J.ms = 0;
    J.fits = true;
    if (!L.d_st) LN_TRY(hipMalloc((void **)&L.d_st, 2 * TS_WORDS * 8));
    if (!L.h_st) LN_TRY(hipHostMalloc((void **)&L.h_st, 2 * TS_WORDS * 8, hipHostMallocDefault));
    for (hipEvent_t &ev : L.ev)
        if (!ev) LN_TRY(hipEventCreate(&ev));
    // the host form stages units and offsets (rebased to the staged units) at a 16-B address
    const int mis = J.dev && total ? (int)(((uintptr_t)(J.units + base0) >> 1) & 7) : 0;
    const bool lines = mode != BPE_LINES_FILE;
    const int64_t n_tiles = lines ? (total + mis + LN_TILE - 1) / LN_TILE : 0;
    if (n_tiles > 0x7FFFFFFF / LN_WORDS) return bpe_fail(BPE_ERR_ARG, "bpe native: lines batch too large");
    // scratch 0: [tile LF counts, then bases | first nw | last nw | nwsum | lf | nw | lfpre | units | off]
    const size_t b_tiles = ln_align((size_t)n_tiles * 8), b_plane = ln_align((size_t)n_tiles * LN_WORDS * 4);
    const size_t b_units = J.dev ? 0 : ln_align((size_t)total * 2), b_off = J.dev ? 0 : ln_align((size_t)(n + 1) * 8);
    int rc = ln_grow(L, 0, 4 * b_tiles + 3 * b_plane + b_units + b_off + 16, s);
    if (rc) return rc;
    char *d = L.d_buf[0];
    unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(d);
    long long *d_first = reinterpret_cast<long long *>(d += b_tiles);
    long long *d_last = reinterpret_cast<long long *>(d += b_tiles);
    unsigned long long *d_nwsum = reinterpret_cast<unsigned long long *>(d += b_tiles);
    uint32_t *d_lf = reinterpret_cast<uint32_t *>(d += b_tiles);
    uint32_t *d_nw = reinterpret_cast<uint32_t *>(d += b_plane);
    uint32_t *d_lfpre = reinterpret_cast<uint32_t *>(d += b_plane);
    uint16_t *s_units = reinterpret_cast<uint16_t *>(d += b_plane);
    int64_t *s_off = reinterpret_cast<int64_t *>(d + b_units);
    const uint16_t *units_al = nullptr;
    const int64_t *k_off = nullptr;
    int64_t base = base0;
    if (J.dev) {
        units_al = J.units ? J.units + base0 - mis : nullptr;
        k_off = J.off;
    } else if (n) {
        std::vector<int64_t> rel((size_t)n + 1);
        for (int64_t k = 0; k <= n; ++k) rel[(size_t)k] = h_off[(size_t)k] - base0;
        if (total) LN_TRY(hipMemcpyAsync(s_units, J.units + base0, (size_t)total * 2, hipMemcpyHostToDevice, s));
        LN_TRY(hipMemcpyAsync(s_off, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        LN_TRY(hipStreamSynchronize(s));   // (rel goes away)
        units_al = s_units;
        k_off = s_off;
        base = 0;
    }
    LN_TRY(hipMemsetAsync(L.d_st, 0, 2 * TS_WORDS * 8, s));
    int64_t lf_total = 0;
    float ms = 0;
    if (n_tiles) {
        LN_TRY(hipEventRecord(L.ev[0], s));
        k_ln_tile<<<(unsigned)n_tiles, LN_WG, 0, s>>>(units_al, mis, total, d_lf, d_nw, d_lfpre, d_nwsum, d_cnt, d_first,
                                                     d_last);
        k_txt_scan<<<1, 1024, 0, s>>>(d_cnt, n_tiles, L.d_st);
        k_ln_summ<<<1, 1024, 0, s>>>(d_first, d_last, n_tiles);
        LN_TRY(hipGetLastError());
        LN_TRY(hipEventRecord(L.ev[1], s));
        LN_TRY(hipMemcpyAsync(L.h_st, L.d_st, TS_WORDS * 8, hipMemcpyDeviceToHost, s));
        LN_TRY(hipStreamSynchronize(s));
        lf_total = (int64_t)L.h_st[TS_CHARS];
        if (lf_total < 0 || lf_total > total) return bpe_fail(BPE_ERR_STATE, "bpe native: bad line feed count");
        LN_TRY(hipEventElapsedTime(&ms, L.ev[0], L.ev[1]));
        J.ms += (double)ms;
    }
    const int64_t n_samples = lf_total + n;
    J.samples = n_samples;
    if (n_samples >= 0x7FFFFFFF) return bpe_fail(BPE_ERR_ARG, "bpe native: too many lines for one batch");
    // scratch 1: [begin' | end' | offsets]
    const size_t b_bound = ln_align((size_t)n_samples * 8);
    if ((rc = ln_grow(L, 1, 2 * b_bound + ln_align((size_t)(n_samples + 1) * 8), s))) return rc;
    long long *d_sb = reinterpret_cast<long long *>(L.d_buf[1]);
    long long *d_se = reinterpret_cast<long long *>(L.d_buf[1] + b_bound);
    int64_t *s_ooff = reinterpret_cast<int64_t *>(L.d_buf[1] + 2 * b_bound);
    if (n_samples) {
        LN_TRY(hipEventRecord(L.ev[2], s));
        if (lines) {
            LnPlanes P{d_lf, d_nw, d_lfpre, d_nwsum, d_cnt, d_first, d_last, n_tiles, lf_total};
            const int64_t threads = n_tiles * LN_WORDS + n;
            k_ln_bounds<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(P, units_al, mis, mode, k_off, n, base, d_sb,
                                                                         d_se);
        } else {
            k_ln_file<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(k_off, n, base, mis, d_sb, d_se);
        }
        k_ln_len<<<(unsigned)((n_samples + 255) / 256), 256, 0, s>>>(d_sb, d_se, n_samples,
                                                                    reinterpret_cast<unsigned long long *>(s_ooff));
        k_txt_scan<<<1, 1024, 0, s>>>(reinterpret_cast<unsigned long long *>(s_ooff), n_samples, L.d_st + TS_WORDS);
        LN_TRY(hipGetLastError());
        LN_TRY(hipEventRecord(L.ev[3], s));
        LN_TRY(hipMemcpyAsync(s_ooff + n_samples, L.d_st + TS_WORDS + TS_CHARS, 8, hipMemcpyDeviceToDevice, s));
        LN_TRY(hipMemcpyAsync(L.h_st + TS_WORDS, L.d_st + TS_WORDS, TS_WORDS * 8, hipMemcpyDeviceToHost, s));
        LN_TRY(hipStreamSynchronize(s));
        J.units_out = (int64_t)L.h_st[TS_WORDS + TS_CHARS];
        if (J.units_out < 2 * n_samples || J.units_out > total + 2 * n_samples)
            return bpe_fail(BPE_ERR_STATE, "bpe native: bad sample unit count");
        LN_TRY(hipEventElapsedTime(&ms, L.ev[2], L.ev[3]));
        J.ms += (double)ms;
    } else {
        LN_TRY(hipMemsetAsync(s_ooff, 0, 8, s));
    }
    J.fits = (J.off_cap < 0 || n_samples + 1 <= J.off_cap) && (J.units_cap < 0 || J.units_out <= J.units_cap);
    if (!J.fits) {
        LN_TRY(hipStreamSynchronize(s));
        return BPE_OK;
    }
    if (!J.d_out) {   // scratch 2: the samples' units
        if ((rc = ln_grow(L, 2, ln_align((size_t)std::max<int64_t>(J.units_out, 1) * 2), s))) return rc;
        J.d_out = reinterpret_cast<uint16_t *>(L.d_buf[2]);
    }
    if (J.units_out) {
        const int a = (int)(((uintptr_t)J.d_out >> 1) & 7);
        const int64_t chunks = (a + J.units_out + 7) / 8;
        LN_TRY(hipEventRecord(L.ev[4], s));
        k_ln_emit<<<(unsigned)((chunks + 255) / 256), 256, 0, s>>>(units_al, mode, d_sb, s_ooff, n_samples, J.units_out,
                                                                  J.d_out, a);
        LN_TRY(hipGetLastError());
        LN_TRY(hipEventRecord(L.ev[5], s));
    }
    if (J.d_ooff)
        LN_TRY(hipMemcpyAsync(J.d_ooff, s_ooff, (size_t)(n_samples + 1) * 8, hipMemcpyDeviceToDevice, s));
    else
        J.d_ooff = s_ooff;
    LN_TRY(hipStreamSynchronize(s));
    if (J.units_out) {
        LN_TRY(hipEventElapsedTime(&ms, L.ev[4], L.ev[5]));
        J.ms += (double)ms;
    }
    return BPE_OK;
}

// the counters of a call whose pipeline succeeded
inline void ln_commit(LinesState &L, const LinesCall &J) {
    L.st.texts += J.n_texts;
    L.st.units_in += J.total;
    L.st.samples += J.samples;
    L.st.units_out += J.units_out;
    L.st.trimmed += J.total - (J.units_out - 2 * J.samples);
    L.st.kernel_ms += J.ms;
}

inline int ln_cap_error(const LinesCall &J) {
    char msg[160];
    std::snprintf(msg, sizeof msg, "bpe native: split_lines needs %lld units and %lld offsets, the buffers hold %lld and %lld",
                  (long long)J.units_out, (long long)J.samples + 1, (long long)J.units_cap, (long long)J.off_cap);
    return bpe_fail(BPE_ERR_ARG, msg);
}

}  // namespace

#endif  // BPE_LINES_RULE_ONLY
