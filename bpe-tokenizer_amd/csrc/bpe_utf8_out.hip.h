// bpe_utf8_out.hip.h — text out as UTF-8: UTF-16 code units -> bytes on the device, behind the
// decoder (bpe_decoder_utf16_to_utf8, bpe_decode_utf8_batch, bpe_export_utf8_batch, include/bpe.h).
// Included by bpe_decode.hip; everything here has internal linkage, like bpe_utf8.hip.h, whose shape
// it follows the other way round, and bpe_text_front.hip.h, whose scans it uses.
//
// The encode is Node's Buffer.from(str, 'utf8') / TextEncoder.encode(str), text by text: the WHATWG
// conversion to a USVString, then UTF-8.  It needs no sequential state: with hi(u) = u in D800-DBFF,
// lo(u) = u in DC00-DFFF and every position clipped to the text that holds unit i, a unit at i is
// absorbed (emits nothing) iff lo(u[i]) and hi(u[i-1]); every other unit starts an output: one byte
// below 0x80, two below 0x800, the four bytes of the pair's code point for hi(u[i]) with lo(u[i+1]),
// EF BF BD for any other surrogate (`replaced`), else three.  So a unit is decided from one unit on
// each side of it.
//
// Tiling: tiles of BPE_UTF16_TILE units cut at 16-B addresses of the unit buffer (slot s of tile t
// holds the flat position t * TILE + s - mis, mis = the buffer's misalignment in units, 0..7), 8
// units (one 16-B load) per lane and one halo unit on each side.
//   k_u16_texts  one pass over the texts' offsets: the first text that starts in each tile, and
//                whether a text starts at a tile's slot 0 (the halo question of the tile before it);
//   k_u16_count  bytes and `replaced` per tile.  A tile without a unit >= 0x80 counts its units and
//                reads neither halo nor texts;
//   k_txt_scan   (bpe_text_front.hip.h) exclusive scan of the tile counts, in rounds;
//   k_u16_map    starts recomputed, their bytes ranked by a workgroup scan, the tile's bytes staged
//                in LDS and written 16 B per lane at 16-B addresses of the output, with partial head
//                and tail; the lane that owns unit off[k] writes out_off[k].
//
// With BPE_UTF8_OUT_CLASSIFY_ONLY defined only the per-lane rule is compiled, as plain C++ (a
// stand-alone host program runs it over the fixture: tests/utf8_out_classify_main.cc).
#pragma once

#ifdef BPE_UTF8_OUT_CLASSIFY_ONLY
#include <cstdint>
#define U16_FN inline
#else
#include "bpe_multi.h"            // bpe_fail
#include "bpe_text_front.hip.h"   // wave_incl, block_scan, k_txt_scan, TS_CHARS
#define U16_FN __host__ __device__ __forceinline__
#endif

namespace {

constexpr int U16_RUN = 8;               // units per lane and load (16 B)
constexpr int U16_N = U16_RUN + 2;       // units a lane looks at: one before its run, one after

// The classes of a lane's units, bit j for the unit at slot j of its run (j in 0..7).
struct U16Masks {
    uint32_t start;   // units of the run that start an output (valid, not absorbed)
    uint32_t one;     // starts below 0x80
    uint32_t two;     // starts in 0x80 .. 0x7FF
    uint32_t four;    // high surrogates with their low one behind them, in the same text
    uint32_t repl;    // lone surrogates: EF BF BD
};                    // (every other start: three bytes)

// u[j + 1] = the unit at slot j of the run (j in -1..8), 0 for a position outside the batch (0 is no
// surrogate); f: bit j + 1 set when a text starts at slot j (j in 0..8); valid: bit j set when slot j
// of the run is inside the batch.
U16_FN U16Masks u16_classify(const uint32_t u[U16_N], uint32_t f, uint32_t valid) {
    uint32_t H = 0, L = 0, A = 0, B = 0;
#pragma unroll
    for (int s = 0; s < U16_N; ++s) {
        const uint32_t x = u[s];
        H |= (uint32_t)((x & 0xFC00u) == 0xD800u) << s;
        L |= (uint32_t)((x & 0xFC00u) == 0xDC00u) << s;
        A |= (uint32_t)(x < 0x80u) << s;
        B |= (uint32_t)(x < 0x800u) << s;
    }
    const uint32_t nb = ~f;                          // the unit before is in the same text
    const uint32_t absorbed = L & (H << 1) & nb;
    const uint32_t pair = H & (L >> 1) & (nb >> 1);  // (a high surrogate is never absorbed itself)
    const uint32_t start = ((valid & 0xFFu) << 1) & ~absorbed;
    U16Masks m;
    m.start = start >> 1;
    m.one = (start & A) >> 1;
    m.two = (start & B & ~A) >> 1;
    m.four = (start & pair) >> 1;
    m.repl = (start & (H | L) & ~pair) >> 1;
    return m;
}

// bytes the starts of `mask`'s slots make (mask: a subset of the run's slots)
U16_FN int u16_bytes_in(const U16Masks &m, uint32_t mask) {
    const uint32_t s = m.start & mask;
    // one byte each for `one`, two for `two`, four for `four`, three for the rest
    return 3 * __builtin_popcount(s) - 2 * __builtin_popcount(m.one & mask) - __builtin_popcount(m.two & mask) +
           __builtin_popcount(m.four & mask);
}

// The bytes of the start at slot j of a lane's run: their number (1..4), into b[0..3].
U16_FN int u16_bytes_at(const uint32_t u[U16_N], const U16Masks &m, int j, uint32_t b[4]) {
    const uint32_t x = u[j + 1];
    if ((m.one >> j) & 1) {
        b[0] = x;
        return 1;
    }
    if ((m.two >> j) & 1) {
        b[0] = 0xC0u | (x >> 6), b[1] = 0x80u | (x & 0x3Fu);
        return 2;
    }
    if ((m.four >> j) & 1) {
        const uint32_t cp = 0x10000u + ((x & 0x3FFu) << 10) + (u[j + 2] & 0x3FFu);
        b[0] = 0xF0u | (cp >> 18), b[1] = 0x80u | ((cp >> 12) & 0x3Fu);
        b[2] = 0x80u | ((cp >> 6) & 0x3Fu), b[3] = 0x80u | (cp & 0x3Fu);
        return 4;
    }
    const uint32_t c = ((m.repl >> j) & 1) ? 0xFFFDu : x;
    b[0] = 0xE0u | (c >> 12), b[1] = 0x80u | ((c >> 6) & 0x3Fu), b[2] = 0x80u | (c & 0x3Fu);
    return 3;
}

}  // namespace

#ifndef BPE_UTF8_OUT_CLASSIFY_ONLY

namespace {

constexpr int U16_TILE = BPE_UTF16_TILE;
constexpr int U16_WG = 256;
constexpr int U16_FWORDS = U16_TILE / 32 + 1;   // text-start bits of slots [0, TILE]
constexpr int U16S_REPLACED = 3;                // status word beside TS_CHARS: lone surrogates replaced
// (a tile makes at most 3 * (TILE - 1) + 4 bytes: its last unit may lead a pair whose low half opens
// the next tile; staged at the output's 16-B phase, 0..15 bytes in)
constexpr int U16_STAGE = 3 * U16_TILE + 32;
static_assert(U16_TILE == U16_WG * U16_RUN, "one 16-B load of units per lane");
static_assert(U16S_REPLACED < TS_WORDS && U16S_REPLACED != TS_CHARS, "status words");

// A lane's 8 units of tile `tile` (u[1..8], flat positions p0 .. p0 + 7); no position outside
// [0, total) is loaded.  units_al is the unit buffer's 16-B aligned base (the flat position -mis).
// any80: some unit of the run is >= 0x80.
__device__ __forceinline__ void u16_load_run(const uint16_t *__restrict__ units_al, int64_t tile, int mis,
                                             int64_t total, uint32_t u[U16_N], int64_t &p0, bool &any80) {
    const int64_t s = tile * U16_TILE + U16_RUN * (int64_t)threadIdx.x;
    p0 = s - mis;
    if (p0 >= 0 && p0 + U16_RUN <= total) {
        const uint4 x = *reinterpret_cast<const uint4 *>(units_al + s);
        u[1] = x.x & 0xFFFFu, u[2] = x.x >> 16, u[3] = x.y & 0xFFFFu, u[4] = x.y >> 16;
        u[5] = x.z & 0xFFFFu, u[6] = x.z >> 16, u[7] = x.w & 0xFFFFu, u[8] = x.w >> 16;
        any80 = ((x.x | x.y | x.z | x.w) & 0xFF80FF80u) != 0;
    } else {
        uint32_t o = 0;
#pragma unroll
        for (int j = 0; j < U16_RUN; ++j) {
            u[j + 1] = (p0 + j >= 0 && p0 + j < total) ? units_al[s + j] : 0u;
            o |= u[j + 1];
        }
        any80 = (o & 0xFF80u) != 0;
    }
}

__device__ __forceinline__ void u16_load_halo(const uint16_t *__restrict__ units_al, int64_t tile, int mis,
                                              int64_t total, uint32_t u[U16_N], int64_t p0) {
    const int64_t s = tile * U16_TILE + U16_RUN * (int64_t)threadIdx.x;
    u[0] = (p0 - 1 >= 0 && p0 - 1 < total) ? units_al[s - 1] : 0u;
    u[U16_RUN + 1] = (p0 + U16_RUN >= 0 && p0 + U16_RUN < total) ? units_al[s + U16_RUN] : 0u;
}

__device__ __forceinline__ uint32_t u16_valid(int64_t p0, int64_t total) {
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < U16_RUN; ++j) v |= (uint32_t)(p0 + j >= 0 && p0 + j < total) << j;
    return v;
}

// A text at the very end of the units belongs to the last tile.
__device__ __forceinline__ int64_t u16_tile_of(int64_t p, int mis, int64_t n_tiles) {
    const int64_t t = (p + mis) / U16_TILE;
    return t < n_tiles ? t : n_tiles - 1;
}

// (the host has checked the offsets' order; tile_first preset to -1, tile_edge to 0)
__global__ void __launch_bounds__(256)
k_u16_texts(int mis, int64_t total, const int64_t *__restrict__ off, int64_t n_texts, int64_t base, int64_t n_tiles,
            long long *__restrict__ tile_first, uint32_t *__restrict__ tile_edge) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k <= n_texts; k += (int64_t)gridDim.x * 256) {
        const int64_t p = off[k] - base;
        const int64_t t = u16_tile_of(p, mis, n_tiles);
        const int64_t q = k ? off[k - 1] - base : -1;
        if (k == 0 || u16_tile_of(q, mis, n_tiles) != t) tile_first[t] = k;
        // the first text that starts at this unit, at a tile's slot 0
        if (p > 0 && p < total && q != p && (p + mis) % U16_TILE == 0) tile_edge[t] = 1u;
    }
}

// The text starts a tile's lanes see, as bits of s_f (bit s of the array: slot s, s in 0..TILE):
// those of the texts that start in the tile (a strided walk from the tile's first text) and, from the
// next tile's edge word, the one right after the tile's last slot.  Ends with the barrier after
// which s_f may be read.
__device__ __forceinline__ void u16_text_bits(uint32_t *s_f, int64_t tile, int64_t n_tiles, int64_t slot0,
                                              int64_t p_lo, int64_t p_hi, const long long *__restrict__ tile_first,
                                              const uint32_t *__restrict__ tile_edge,
                                              const int64_t *__restrict__ off, int64_t n_texts, int64_t base) {
    const int tid = threadIdx.x;
    if (tid < U16_FWORDS) s_f[tid] = (tid == U16_FWORDS - 1 && tile + 1 < n_tiles) ? (tile_edge[tile + 1] & 1u) : 0u;
    __syncthreads();
    const long long k0 = tile_first[tile];
    if (k0 >= 0) {
        for (int64_t k = k0 + tid; k <= n_texts; k += U16_WG) {
            const int64_t p = off[k] - base;
            if (p < p_lo || p >= p_hi) break;   // (an offset at the very end forces nothing)
            const int s = (int)(p - slot0);
            atomicOr(&s_f[s >> 5], 1u << (s & 31));
        }
    }
    __syncthreads();
}

// this lane's text-start bits: bit j + 1 for slot j of its run, j in 0..8
__device__ __forceinline__ uint32_t u16_lane_bits(const uint32_t *s_f) {
    const int b0 = U16_RUN * (int)threadIdx.x;   // the array bit of slot 0 of the run (a multiple of 8)
    const uint32_t lo = s_f[b0 >> 5] >> (b0 & 31);           // slots 0..7 (a run never straddles a word)
    const uint32_t next = (s_f[(b0 + U16_RUN) >> 5] >> ((b0 + U16_RUN) & 31)) & 1u;
    return ((lo & 0xFFu) | (next << U16_RUN)) << 1;
}

__global__ void __launch_bounds__(U16_WG)
k_u16_count(const uint16_t *__restrict__ units_al, int mis, int64_t total, int64_t n_tiles,
            const long long *__restrict__ tile_first, const uint32_t *__restrict__ tile_edge,
            const int64_t *__restrict__ off, int64_t n_texts, int64_t base, unsigned long long *__restrict__ tile_cnt,
            unsigned long long *__restrict__ st) {
    __shared__ uint32_t s_f[U16_FWORDS];
    __shared__ int scn[2][U16_WG / 64];
    const int64_t tile = blockIdx.x;
    const int64_t slot0 = tile * U16_TILE - mis;
    const int64_t p_lo = slot0 < 0 ? 0 : slot0;
    const int64_t p_hi = slot0 + U16_TILE < total ? slot0 + U16_TILE : total;
    uint32_t u[U16_N];
    int64_t p0;
    bool any80;
    u16_load_run(units_al, tile, mis, total, u, p0, any80);
    if (!__syncthreads_or(any80)) {   // pure ASCII: every unit is one byte, whatever the texts are
        if (threadIdx.x == 0) tile_cnt[tile] = (unsigned long long)(p_hi - p_lo);
        return;
    }
    u16_load_halo(units_al, tile, mis, total, u, p0);
    u16_text_bits(s_f, tile, n_tiles, slot0, p_lo, p_hi, tile_first, tile_edge, off, n_texts, base);
    const U16Masks m = u16_classify(u, u16_lane_bits(s_f), u16_valid(p0, total));
    const int bytes = u16_bytes_in(m, 0xFFu);
    const int repl = __builtin_popcount(m.repl);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ib = wave_incl(bytes, lane), ir = wave_incl(repl, lane);
    if (lane == 63) scn[0][w] = ib, scn[1][w] = ir;
    __syncthreads();
    if (threadIdx.x == 0) {
        int ab = 0, ar = 0;
#pragma unroll
        for (int i = 0; i < U16_WG / 64; ++i) ab += scn[0][i], ar += scn[1][i];
        tile_cnt[tile] = (unsigned long long)ab;
        if (ar) atomicAdd(&st[U16S_REPLACED], (unsigned long long)ar);
    }
}

// bytes_out == nullptr: only the offsets are written (the sizing call, and a result past the cap)
__global__ void __launch_bounds__(U16_WG)
k_u16_map(const uint16_t *__restrict__ units_al, int mis, int64_t total, int64_t n_tiles,
          const unsigned long long *__restrict__ tile_base, const long long *__restrict__ tile_first,
          const uint32_t *__restrict__ tile_edge, const int64_t *__restrict__ off, int64_t n_texts, int64_t base,
          uint8_t *__restrict__ bytes_out, int64_t *__restrict__ out_off) {
    __shared__ uint32_t s_f[U16_FWORDS];
    __shared__ int s_pre[U16_WG];           // bytes before each lane's run
    __shared__ uint32_t s_mask[U16_WG];     // each lane's start | one << 8 | two << 16 | four << 24
    __shared__ __attribute__((aligned(16))) uint8_t s_bytes[U16_STAGE];
    __shared__ int scn[U16_WG / 64];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const bool last = tile == n_tiles - 1;
    const int64_t slot0 = tile * U16_TILE - mis;
    const int64_t p_lo = slot0 < 0 ? 0 : slot0;
    const int64_t p_hi = slot0 + U16_TILE < total ? slot0 + U16_TILE : total;
    uint32_t u[U16_N];
    int64_t p0;
    bool any80;
    u16_load_run(units_al, tile, mis, total, u, p0, any80);
    u16_load_halo(units_al, tile, mis, total, u, p0);
    u16_text_bits(s_f, tile, n_tiles, slot0, p_lo, p_hi, tile_first, tile_edge, off, n_texts, base);
    const U16Masks m = u16_classify(u, u16_lane_bits(s_f), u16_valid(p0, total));
    int n_bytes = 0;
    const int before = block_scan<U16_WG>(u16_bytes_in(m, 0xFFu), scn, n_bytes);
    s_pre[tid] = before;
    s_mask[tid] = m.start | (m.one << 8) | (m.two << 16) | (m.four << 24);
    const unsigned long long tb = tile_base[tile];
    // the output's 16-B phase: byte i of the tile sits at s_bytes[a + i], so that chunk c of sixteen
    // bytes is one aligned 16-B word both in LDS and at bytes_out + tb - a
    const int a = bytes_out ? (int)((uintptr_t)(bytes_out + tb) & 15) : 0;
    if (bytes_out) {
        int r = a + before;
        if (!any80) {   // (the lane's units are its bytes)
#pragma unroll
            for (int j = 0; j < U16_RUN; ++j)
                if ((m.start >> j) & 1) s_bytes[r++] = (uint8_t)u[j + 1];
        } else {
#pragma unroll
            for (int j = 0; j < U16_RUN; ++j) {
                if (!((m.start >> j) & 1)) continue;
                uint32_t b[4];
                const int k = u16_bytes_at(u, m, j, b);
                s_bytes[r] = (uint8_t)b[0];
                if (k > 1) s_bytes[r + 1] = (uint8_t)b[1];
                if (k > 2) s_bytes[r + 2] = (uint8_t)b[2];
                if (k > 3) s_bytes[r + 3] = (uint8_t)b[3];
                r += k;
            }
        }
    }
    __syncthreads();
    if (bytes_out) {
        uint8_t *out_al = bytes_out + tb - a;   // (never dereferenced below bytes_out + tb)
        const int end = a + n_bytes;
        for (int c = tid; c * 16 < end; c += U16_WG) {
            if (c * 16 >= a && c * 16 + 16 <= end) {
                *reinterpret_cast<uint4 *>(out_al + c * 16) = *reinterpret_cast<const uint4 *>(s_bytes + c * 16);
            } else {
                for (int i = c * 16 < a ? a : c * 16; i < c * 16 + 16 && i < end; ++i) out_al[i] = s_bytes[i];
            }
        }
    }
    // out_off of the texts that start inside the tile (the last tile: also those at the very end)
    const long long k0 = tile_first[tile];
    if (k0 < 0) return;
    for (int64_t k = k0 + tid; k <= n_texts; k += U16_WG) {
        const int64_t p = off[k] - base;
        if (p < p_lo || p > p_hi || (p == p_hi && !last)) break;
        const int s = (int)(p - slot0);
        int v = n_bytes;
        if (s < U16_TILE) {
            const uint32_t w = s_mask[s / U16_RUN], below = (1u << (s & (U16_RUN - 1))) - 1u;
            U16Masks x;
            x.start = w & 0xFFu, x.one = (w >> 8) & 0xFFu, x.two = (w >> 16) & 0xFFu, x.four = w >> 24, x.repl = 0;
            v = s_pre[s / U16_RUN] + u16_bytes_in(x, below);
        }
        out_off[k] = (int64_t)(tb + (unsigned long long)v);
    }
}

#define U16_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return bpe_fail(e_ == hipErrorOutOfMemory ? BPE_ERR_OOM : BPE_ERR_HIP,         \
                            (std::string("bpe native: ") + #expr + ": " +                   \
                             hipGetErrorString(e_)).c_str());                              \
    } while (0)

}  // namespace

// ---- host side: the transcode of one call on the decoder's device and stream ----------------------

// Scratch (grow-only), status words, events and counters of the UTF-8 back of a decoder.
struct Utf8OutState {
    char *d_buf = nullptr;    // the transcode's tiles, staging and outputs of the host form
    size_t d_cap = 0;
    char *d_dec = nullptr;    // a decode's units (2 B each) and their offsets (8 B per text)
    size_t d_dec_cap = 0;
    unsigned long long *d_st = nullptr, *h_st = nullptr;   // (h_st pinned)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bpe_utf8_stats st{};
};

// One call's transcode.  In: the call's arguments.  Out: where the bytes and their offsets are on
// the device and the call's numbers, which the caller adds to the counters once its whole pipeline
// has succeeded (u16_commit).
struct Utf8OutCall {
    // in
    const uint16_t *units = nullptr;   // text k = units[off[k] .. off[k+1])
    const int64_t *off = nullptr;
    int64_t n_texts = 0;
    bool dev = false;                  // units and off are device buffers
    uint8_t *d_bytes = nullptr;        // the caller's device output, or nullptr: into scratch
    int64_t *d_boff = nullptr;         // ... its n_texts + 1 offsets, or nullptr: into scratch
    int64_t cap = 0;                   // bytes the output may hold
    // out
    int64_t total = 0, bytes = 0, replaced = 0;
    double ms = 0;
    bool fits = true;                  // false: bytes > cap, only the offsets were written
};

namespace {

inline void u16_free(Utf8OutState &U) {
    if (U.d_buf) (void)hipFree(U.d_buf);
    if (U.d_dec) (void)hipFree(U.d_dec);
    if (U.d_st) (void)hipFree(U.d_st);
    if (U.h_st) (void)hipHostFree(U.h_st);
    for (hipEvent_t &ev : U.ev)
        if (ev) (void)hipEventDestroy(ev);
    U = Utf8OutState{};
}

inline size_t u16_align(size_t x) { return (x + 15) & ~(size_t)15; }

// grows one of the state's device buffers, keeping nothing
inline int u16_grow(hipStream_t s, char **p, size_t *have, size_t need) {
    if (need <= *have) return BPE_OK;
    U16_TRY(hipStreamSynchronize(s));
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
    const size_t want = need + need / 4 + 4096;
    U16_TRY(hipMalloc((void **)p, want));
    *have = want;
    return BPE_OK;
}

// On BPE_OK the n_texts + 1 offsets are in J.d_boff and, when J.fits, the bytes in J.d_bytes.
inline int u16_transcode(Utf8OutState &U, hipStream_t s, Utf8OutCall &J) {
    const int64_t n = J.n_texts;
    if (n < 0 || n >= 0x7FFFFFFF || (n && !J.off) || J.cap < 0)
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad utf8 batch arguments");
    std::vector<int64_t> h_off((size_t)n + 1, 0);
    if (n) {
        if (J.dev) {
            U16_TRY(hipMemcpyAsync(h_off.data(), J.off, h_off.size() * 8, hipMemcpyDeviceToHost, s));
            U16_TRY(hipStreamSynchronize(s));
        } else {
            std::copy(J.off, J.off + n + 1, h_off.begin());
        }
    }
    if (n && h_off[0] < 0) return bpe_fail(BPE_ERR_ARG, "bpe native: negative text offset");
    for (int64_t k = 0; k < n; ++k)
        if (h_off[k + 1] < h_off[k]) return bpe_fail(BPE_ERR_ARG, "bpe native: text offsets must not decrease");
    const int64_t base0 = n ? h_off[0] : 0, total = n ? h_off[n] - base0 : 0;
    if (total && !J.units) return bpe_fail(BPE_ERR_ARG, "bpe native: null unit buffer");
    if (total > INT64_MAX / 4) return bpe_fail(BPE_ERR_ARG, "bpe native: utf8 batch too large");
    J.total = total;
    if (!U.d_st) U16_TRY(hipMalloc((void **)&U.d_st, TS_WORDS * 8));
    if (!U.h_st) U16_TRY(hipHostMalloc((void **)&U.h_st, TS_WORDS * 8, hipHostMallocDefault));
    for (hipEvent_t &ev : U.ev)
        if (!ev) U16_TRY(hipEventCreate(&ev));
    // the host form stages units and offsets (rebased to the staged units) at a 16-B address
    const int mis = J.dev && total ? (int)(((uintptr_t)(J.units + base0) >> 1) & 7) : 0;
    const int64_t n_tiles = (total + mis + U16_TILE - 1) / U16_TILE;
    if (n_tiles > 0x7FFFFFFF) return bpe_fail(BPE_ERR_ARG, "bpe native: utf8 batch too large");
    // scratch: [tile counts, then bases | first text of each tile | tile edges | units | off | bytes | boff]
    const size_t b_tiles = u16_align((size_t)n_tiles * 8), b_edge = u16_align((size_t)n_tiles * 4);
    const size_t b_units = J.dev ? 0 : u16_align((size_t)total * 2), b_off = J.dev ? 0 : u16_align((size_t)(n + 1) * 8);
    const size_t b_bytes = J.d_bytes ? 0 : u16_align((size_t)std::min(J.cap, 3 * total));
    const size_t b_boff = J.d_boff ? 0 : u16_align((size_t)(n + 1) * 8);
    int rc;
    if ((rc = u16_grow(s, &U.d_buf, &U.d_cap, 2 * b_tiles + b_edge + b_units + b_off + b_bytes + b_boff + 16))) return rc;
    char *d = U.d_buf;
    unsigned long long *d_tiles = reinterpret_cast<unsigned long long *>(d);
    long long *d_first = reinterpret_cast<long long *>(d += b_tiles);
    uint32_t *d_edge = reinterpret_cast<uint32_t *>(d += b_tiles);
    uint16_t *s_units = reinterpret_cast<uint16_t *>(d += b_edge);
    int64_t *s_off = reinterpret_cast<int64_t *>(d += b_units);
    uint8_t *s_bytes = reinterpret_cast<uint8_t *>(d += b_off);
    int64_t *s_boff = reinterpret_cast<int64_t *>(d + b_bytes);
    if (!J.d_bytes) J.d_bytes = s_bytes;
    if (!J.d_boff) J.d_boff = s_boff;
    J.bytes = J.replaced = 0;
    J.ms = 0;
    J.fits = true;
    if (total == 0) {   // (no text, or every text empty)
        U16_TRY(hipMemsetAsync(J.d_boff, 0, (size_t)(n + 1) * 8, s));
        U16_TRY(hipStreamSynchronize(s));
        return BPE_OK;
    }
    const uint16_t *units_al;
    const int64_t *k_off;
    int64_t base = base0;
    if (J.dev) {
        units_al = J.units + base0 - mis;
        k_off = J.off;
    } else {
        std::vector<int64_t> rel((size_t)n + 1);
        for (int64_t k = 0; k <= n; ++k) rel[(size_t)k] = h_off[(size_t)k] - base0;
        U16_TRY(hipMemcpyAsync(s_units, J.units + base0, (size_t)total * 2, hipMemcpyHostToDevice, s));
        U16_TRY(hipMemcpyAsync(s_off, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        U16_TRY(hipStreamSynchronize(s));   // (rel goes away)
        units_al = s_units;
        k_off = s_off;
        base = 0;
    }
    U16_TRY(hipMemsetAsync(U.d_st, 0, TS_WORDS * 8, s));
    U16_TRY(hipMemsetAsync(d_first, 0xFF, (size_t)n_tiles * 8, s));
    U16_TRY(hipMemsetAsync(d_edge, 0, (size_t)n_tiles * 4, s));
    U16_TRY(hipEventRecord(U.ev[0], s));
    k_u16_texts<<<(unsigned)std::min<int64_t>((n + 256) / 256, 2048), 256, 0, s>>>(mis, total, k_off, n, base, n_tiles,
                                                                                  d_first, d_edge);
    k_u16_count<<<(unsigned)n_tiles, U16_WG, 0, s>>>(units_al, mis, total, n_tiles, d_first, d_edge, k_off, n, base,
                                                    d_tiles, U.d_st);
    k_txt_scan<<<1, 1024, 0, s>>>(d_tiles, n_tiles, U.d_st);
    U16_TRY(hipGetLastError());
    U16_TRY(hipEventRecord(U.ev[1], s));
    U16_TRY(hipMemcpyAsync(U.h_st, U.d_st, TS_WORDS * 8, hipMemcpyDeviceToHost, s));
    U16_TRY(hipStreamSynchronize(s));
    J.bytes = (int64_t)U.h_st[TS_CHARS];
    J.replaced = (int64_t)U.h_st[U16S_REPLACED];
    if (J.bytes < 0 || J.bytes > 3 * total || J.replaced < 0 || J.replaced > total)
        return bpe_fail(BPE_ERR_STATE, "bpe native: bad utf8 byte count");
    J.fits = J.bytes <= J.cap;
    U16_TRY(hipEventRecord(U.ev[2], s));
    k_u16_map<<<(unsigned)n_tiles, U16_WG, 0, s>>>(units_al, mis, total, n_tiles, d_tiles, d_first, d_edge, k_off, n,
                                                  base, J.fits ? J.d_bytes : nullptr, J.d_boff);
    U16_TRY(hipGetLastError());
    U16_TRY(hipEventRecord(U.ev[3], s));
    U16_TRY(hipStreamSynchronize(s));
    float ms0 = 0, ms1 = 0;
    U16_TRY(hipEventElapsedTime(&ms0, U.ev[0], U.ev[1]));
    U16_TRY(hipEventElapsedTime(&ms1, U.ev[2], U.ev[3]));
    J.ms = (double)ms0 + (double)ms1;
    return BPE_OK;
}

// the counters of a call whose pipeline succeeded and wrote its bytes
inline void u16_commit(Utf8OutState &U, const Utf8OutCall &J) {
    U.st.texts += J.n_texts;
    U.st.units += J.total;
    U.st.bytes += J.bytes;
    U.st.replaced += J.replaced;
    U.st.kernel_ms += J.ms;
}

inline int u16_cap_error(const Utf8OutCall &J) {
    char msg[128];
    std::snprintf(msg, sizeof msg, "bpe native: utf16_to_utf8 needs %lld bytes, the buffer holds %lld",
                  (long long)J.bytes, (long long)J.cap);
    return bpe_fail(BPE_ERR_ARG, msg);
}

}  // namespace

#endif  // BPE_UTF8_OUT_CLASSIFY_ONLY
