// bpe_utf8.hip.h — text as UTF-8: bytes -> UTF-16 code units on the device, in front of the three
// text pipelines (bpe_encode_utf8_batch, bpe_add_utf8_batch, bpe_restore_utf8_batch, include/bpe.h).
// Included by bpe_encode.hip (the transcode on an encoder) and bpe_engine.hip (on a context);
// everything here has internal linkage, like bpe_text_front.hip.h, whose scans it uses.
//
// The decode is Node's Buffer.toString() / WHATWG TextDecoder('utf-8', {ignoreBOM: true}), text by
// text: every maximal ill-formed subpart becomes one U+FFFD.  It needs no sequential state: with
//   need(b) = 2 for C2-DF, 3 for E0-EF, 4 for F0-F4, else 0          cont(b) = b in 80-BF
//   r2(L)   = the second-byte range of lead L (E0: A0-BF, ED: 80-9F, F0: 90-BF, F4: 80-8F, else 80-BF)
// and every position clipped to the text that holds byte i, a continuation byte at i is absorbed
// (emits nothing) iff
//   need(b[i-1]) >= 2 and b[i] in r2(b[i-1]),  or  need(b[i-2]) >= 3 and b[i-1] in r2(b[i-2]),  or
//   need(b[i-3]) == 4 and b[i-2] in r2(b[i-3]) and cont(b[i-1]);
// every other byte starts an output: an ASCII byte itself, a lead of need k whose b[i+1] is in
// r2(b[i]) and whose b[i+2 .. i+k-1] are continuation bytes its code point (two units for k == 4),
// anything else U+FFFD.  So a byte is decided from three bytes on each side of it.
//
// Tiling: tiles of BPE_UTF8_TILE bytes cut at 16-B addresses of the byte buffer (slot s of tile t
// holds the flat position t * TILE + s - mis, mis = the buffer's misalignment, 0..15), 16 bytes (one
// 16-B load) per lane and three halo bytes on each side.  A lane keeps its 22 bytes' classes as bit
// masks (bit x + 3: the byte at slot x of its run), so the rule above is a few shifts and ANDs.
//   k_u8_texts  one pass over the texts' offsets: the first text that starts in each tile, and
//               the text starts in a tile's first three and last two slots (the neighbours' halo);
//   k_u8_count  units and U+FFFD made per tile.  A tile without a byte >= 0x80 counts its bytes
//               and reads neither halo nor texts;
//   k_txt_scan  (bpe_text_front.hip.h) exclusive scan of the tile counts, in rounds;
//   k_u8_map    starts recomputed, ranked by a workgroup scan, the tile's units staged in LDS and
//               written 16 B per lane at 16-B addresses of the output, with partial head and tail;
//               the lane that owns byte off[k] writes out_off[k].
#pragma once

#include "bpe_multi.h"            // bpe_fail
#include "bpe_text_front.hip.h"   // wave_incl, block_scan, k_txt_scan, TS_CHARS

namespace {

constexpr int U8_TILE = BPE_UTF8_TILE;
constexpr int U8_WG = 256;
constexpr int U8_RUN = 16;                 // bytes per lane and load
constexpr int U8_HALO = 3;
constexpr int U8_N = U8_RUN + 2 * U8_HALO; // bytes a lane looks at
constexpr int U8_FWORDS = U8_TILE / 32 + 2;   // text-start bits of slots [-32, TILE + 32)
constexpr int U8S_REPLACED = 3;            // status word beside TS_CHARS: U+FFFD made from ill-formed input
static_assert(U8_TILE == U8_WG * U8_RUN, "one 16-B load of bytes per lane");
static_assert(U8S_REPLACED < TS_WORDS && U8S_REPLACED != TS_CHARS, "status words");
// tile_edge bits: a text starts at slot 0, 1, 2 (bits 0..2) or at slot TILE - 2, TILE - 1 (bits 3, 4)
constexpr uint32_t U8_EDGE_LO = 7u, U8_EDGE_HI_SHIFT = 3;

// The classes of a lane's bytes, bit x + U8_HALO for the byte at slot x of its run (x in -3..18).
struct U8Masks {
    uint32_t start;   // bytes of the run that start an output (valid, not absorbed)
    uint32_t four;    // starts that emit a surrogate pair (well-formed 4-byte sequences)
    uint32_t two, three;   // starts that are well-formed 2- and 3-byte sequences
    uint32_t ascii;   // bytes below 0x80
};

// b[x + 3] = the byte at slot x of the run, 0 for a position outside the batch (0 matches nothing);
// f: bit x + 3 set when a text starts at slot x; valid: bits of the run's slots inside the batch.
__host__ __device__ __forceinline__ U8Masks u8_classify(const uint32_t b[U8_N], uint32_t f, uint32_t valid) {
    uint32_t C = 0, N2 = 0, N3 = 0, N4 = 0, A = 0, P = 0;
#pragma unroll
    for (int s = 0; s < U8_N; ++s) {
        const uint32_t x = b[s];
        C |= (uint32_t)((x & 0xC0u) == 0x80u) << s;
        N2 |= (uint32_t)(x - 0xC2u <= 0xDFu - 0xC2u) << s;
        N3 |= (uint32_t)((x & 0xF0u) == 0xE0u) << s;
        N4 |= (uint32_t)(x - 0xF0u <= 4u) << s;
        A |= (uint32_t)(x < 0x80u) << s;
        if (s) {   // P: this byte is in r2 of the byte before it, a lead
            const uint32_t l = b[s - 1];
            const uint32_t lo = l == 0xE0u ? 0xA0u : l == 0xF0u ? 0x90u : 0x80u;
            const uint32_t hi = l == 0xEDu ? 0x9Fu : l == 0xF4u ? 0x8Fu : 0xBFu;
            P |= (uint32_t)(l - 0xC2u <= 0xF4u - 0xC2u && x >= lo && x <= hi) << s;
        }
    }
    const uint32_t nb = ~f;                        // the byte before is in the same text
    const uint32_t back2 = nb & (nb << 1), back3 = back2 & (nb << 2);
    const uint32_t absorbed = C & ((nb & P) | (back2 & ((N3 | N4) << 2) & (P << 1)) |
                                   (back3 & (N4 << 3) & (P << 2) & (C << 1)));
    const uint32_t fwd1 = nb >> 1, fwd2 = fwd1 & (nb >> 2), fwd3 = fwd2 & (nb >> 3);
    U8Masks m;
    m.start = valid & ~absorbed;
    m.two = m.start & N2 & fwd1 & (P >> 1);
    m.three = m.start & N3 & fwd2 & (P >> 1) & (C >> 2);
    m.four = m.start & N4 & fwd3 & (P >> 1) & (C >> 2) & (C >> 3);
    m.ascii = A;
    return m;
}

// The units of the start at bit s of a lane's masks: their number (1 or 2), u0 and u1.
__host__ __device__ __forceinline__ int u8_units_at(const uint32_t b[U8_N], const U8Masks &m, int s, uint32_t &u0,
                                                    uint32_t &u1) {
    const uint32_t b0 = b[s], b1 = b[s + 1] & 0x3Fu, b2 = b[s + 2] & 0x3Fu, b3 = b[s + 3] & 0x3Fu;
    if ((m.four >> s) & 1) {
        const uint32_t cp = (((b0 & 7u) << 18) | (b1 << 12) | (b2 << 6) | b3) - 0x10000u;
        u0 = 0xD800u + (cp >> 10);
        u1 = 0xDC00u + (cp & 0x3FFu);
        return 2;
    }
    u0 = 0xFFFDu;
    if ((m.ascii >> s) & 1) u0 = b0;
    if ((m.two >> s) & 1) u0 = ((b0 & 0x1Fu) << 6) | b1;
    if ((m.three >> s) & 1) u0 = ((b0 & 0xFu) << 12) | (b1 << 6) | b2;
    return 1;
}

// A lane's 16 bytes of tile `tile` (b[3..18], flat positions p0 .. p0 + 15) and the halo on both
// sides; no position outside [0, total) is loaded.  bytes_al is the byte buffer's 16-B aligned base
// (the flat position -mis).  any80: some byte of the run is >= 0x80.
__device__ __forceinline__ void u8_load_run(const uint8_t *__restrict__ bytes_al, int64_t tile, int mis, int64_t total,
                                            uint32_t b[U8_N], int64_t &p0, bool &any80) {
    const int64_t s = tile * U8_TILE + U8_RUN * (int64_t)threadIdx.x;
    p0 = s - mis;
    if (p0 >= 0 && p0 + U8_RUN <= total) {
        const uint4 x = *reinterpret_cast<const uint4 *>(bytes_al + s);
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < U8_RUN; ++j) b[U8_HALO + j] = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        any80 = ((x.x | x.y | x.z | x.w) & 0x80808080u) != 0;
    } else {
        uint32_t o = 0;
#pragma unroll
        for (int j = 0; j < U8_RUN; ++j) {
            b[U8_HALO + j] = (p0 + j >= 0 && p0 + j < total) ? bytes_al[s + j] : 0u;
            o |= b[U8_HALO + j];
        }
        any80 = (o & 0x80u) != 0;
    }
}

__device__ __forceinline__ void u8_load_halo(const uint8_t *__restrict__ bytes_al, int64_t tile, int mis,
                                             int64_t total, uint32_t b[U8_N], int64_t p0) {
    const int64_t s = tile * U8_TILE + U8_RUN * (int64_t)threadIdx.x;
    if (p0 - 4 >= 0 && p0 <= total) {   // one aligned word holds the three bytes before
        const uint32_t w = *reinterpret_cast<const uint32_t *>(bytes_al + s - 4);
        b[0] = (w >> 8) & 0xFFu, b[1] = (w >> 16) & 0xFFu, b[2] = w >> 24;
    } else {
#pragma unroll
        for (int j = 0; j < U8_HALO; ++j) {
            const int64_t p = p0 - U8_HALO + j;
            b[j] = (p >= 0 && p < total) ? bytes_al[s - U8_HALO + j] : 0u;
        }
    }
    if (p0 + U8_RUN >= 0 && p0 + U8_RUN + 4 <= total) {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(bytes_al + s + U8_RUN);
        b[U8_HALO + U8_RUN] = w & 0xFFu, b[U8_HALO + U8_RUN + 1] = (w >> 8) & 0xFFu;
        b[U8_HALO + U8_RUN + 2] = (w >> 16) & 0xFFu;
    } else {
#pragma unroll
        for (int j = 0; j < U8_HALO; ++j) {
            const int64_t p = p0 + U8_RUN + j;
            b[U8_HALO + U8_RUN + j] = (p >= 0 && p < total) ? bytes_al[s + U8_RUN + j] : 0u;
        }
    }
}

__device__ __forceinline__ uint32_t u8_valid(int64_t p0, int64_t total) {
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < U8_RUN; ++j) v |= (uint32_t)(p0 + j >= 0 && p0 + j < total) << (U8_HALO + j);
    return v;
}

// A text at the very end of the bytes belongs to the last tile.
__device__ __forceinline__ int64_t u8_tile_of(int64_t p, int mis, int64_t n_tiles) {
    const int64_t t = (p + mis) / U8_TILE;
    return t < n_tiles ? t : n_tiles - 1;
}

// (the host has checked the offsets' order; tile_first preset to -1, tile_edge to 0)
__global__ void __launch_bounds__(256)
k_u8_texts(int mis, int64_t total, const int64_t *__restrict__ off, int64_t n_texts, int64_t base, int64_t n_tiles,
           long long *__restrict__ tile_first, uint32_t *__restrict__ tile_edge) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k <= n_texts; k += (int64_t)gridDim.x * 256) {
        const int64_t p = off[k] - base;
        const int64_t t = u8_tile_of(p, mis, n_tiles);
        const int64_t q = k ? off[k - 1] - base : -1;
        if (k == 0 || u8_tile_of(q, mis, n_tiles) != t) tile_first[t] = k;
        if (p > 0 && p < total && q != p) {   // the first text that starts at this byte
            const int s = (int)((p + mis) % U8_TILE);
            if (s < U8_HALO) atomicOr(&tile_edge[t], 1u << s);
            if (s >= U8_TILE - 2) atomicOr(&tile_edge[t], 1u << (U8_EDGE_HI_SHIFT + s - (U8_TILE - 2)));
        }
    }
}

// The text starts a tile's lanes see, as bits of s_f (bit 32 + s of the array: slot s): those of the
// texts that start in the tile (a strided walk from the tile's first text) and, from the
// neighbours' edge bits, those in the two slots before the tile and the three after it.
// Ends with the barrier after which s_f may be read.
__device__ __forceinline__ void u8_text_bits(uint32_t *s_f, int64_t tile, int64_t n_tiles, int64_t slot0, int64_t p_lo,
                                             int64_t p_hi, const long long *__restrict__ tile_first,
                                             const uint32_t *__restrict__ tile_edge, const int64_t *__restrict__ off,
                                             int64_t n_texts, int64_t base) {
    const int tid = threadIdx.x;
    if (tid < U8_FWORDS) {
        uint32_t w = 0;
        if (tid == 0 && tile > 0) w = (tile_edge[tile - 1] >> U8_EDGE_HI_SHIFT) << 30;
        if (tid == U8_FWORDS - 1 && tile + 1 < n_tiles) w = tile_edge[tile + 1] & U8_EDGE_LO;
        s_f[tid] = w;
    }
    __syncthreads();
    const long long k0 = tile_first[tile];
    if (k0 >= 0) {
        for (int64_t k = k0 + tid; k <= n_texts; k += U8_WG) {
            const int64_t p = off[k] - base;
            if (p < p_lo || p >= p_hi) break;   // (an offset at the very end forces nothing)
            const int s = (int)(p - slot0) + 32;
            atomicOr(&s_f[s >> 5], 1u << (s & 31));
        }
    }
    __syncthreads();
}

// this lane's text-start bits: bit x + 3 for slot x of its run, x in -2..18 (bit 0, slot -3: unused)
__device__ __forceinline__ uint32_t u8_lane_bits(const uint32_t *s_f) {
    const int b0 = U8_RUN * (int)threadIdx.x + 32 - 2;   // the array bit of slot -2 of the run
    const unsigned long long w = (unsigned long long)s_f[b0 >> 5] | ((unsigned long long)s_f[(b0 >> 5) + 1] << 32);
    return ((uint32_t)(w >> (b0 & 31)) & 0x1FFFFFu) << 1;
}

__global__ void __launch_bounds__(U8_WG)
k_u8_count(const uint8_t *__restrict__ bytes_al, int mis, int64_t total, int64_t n_tiles,
           const long long *__restrict__ tile_first, const uint32_t *__restrict__ tile_edge,
           const int64_t *__restrict__ off, int64_t n_texts, int64_t base, unsigned long long *__restrict__ tile_cnt,
           unsigned long long *__restrict__ st) {
    __shared__ uint32_t s_f[U8_FWORDS];
    __shared__ int scn[2][U8_WG / 64];
    const int64_t tile = blockIdx.x;
    const int64_t slot0 = tile * U8_TILE - mis;
    const int64_t p_lo = slot0 < 0 ? 0 : slot0;
    const int64_t p_hi = slot0 + U8_TILE < total ? slot0 + U8_TILE : total;
    uint32_t b[U8_N];
    int64_t p0;
    bool any80;
    u8_load_run(bytes_al, tile, mis, total, b, p0, any80);
    if (!__syncthreads_or(any80)) {   // pure ASCII: every byte is one unit, whatever the texts are
        if (threadIdx.x == 0) tile_cnt[tile] = (unsigned long long)(p_hi - p_lo);
        return;
    }
    u8_load_halo(bytes_al, tile, mis, total, b, p0);
    u8_text_bits(s_f, tile, n_tiles, slot0, p_lo, p_hi, tile_first, tile_edge, off, n_texts, base);
    const U8Masks m = u8_classify(b, u8_lane_bits(s_f), u8_valid(p0, total));
    const int units = __builtin_popcount(m.start) + __builtin_popcount(m.four);
    const int repl = __builtin_popcount(m.start & ~(m.ascii | m.two | m.three | m.four));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int iu = wave_incl(units, lane), ir = wave_incl(repl, lane);
    if (lane == 63) scn[0][w] = iu, scn[1][w] = ir;
    __syncthreads();
    if (threadIdx.x == 0) {
        int au = 0, ar = 0;
#pragma unroll
        for (int i = 0; i < U8_WG / 64; ++i) au += scn[0][i], ar += scn[1][i];
        tile_cnt[tile] = (unsigned long long)au;
        if (ar) atomicAdd(&st[U8S_REPLACED], (unsigned long long)ar);
    }
}

// units_out == nullptr: only the offsets are written (the sizing call, and a result past the cap)
__global__ void __launch_bounds__(U8_WG)
k_u8_map(const uint8_t *__restrict__ bytes_al, int mis, int64_t total, int64_t n_tiles,
         const unsigned long long *__restrict__ tile_base, const long long *__restrict__ tile_first,
         const uint32_t *__restrict__ tile_edge, const int64_t *__restrict__ off, int64_t n_texts, int64_t base,
         uint16_t *__restrict__ units_out, int64_t *__restrict__ out_off) {
    __shared__ uint32_t s_f[U8_FWORDS];
    __shared__ int s_pre[U8_WG];                // units before each lane's run
    __shared__ uint32_t s_start[U8_WG], s_four[U8_WG];
    // (a tile makes at most TILE + 1 units: its last byte may lead a pair; staged at the output's
    // 16-B phase, 0..7 units in)
    __shared__ __attribute__((aligned(16))) uint16_t s_units[U8_TILE + 16];
    __shared__ int scn[U8_WG / 64];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const bool last = tile == n_tiles - 1;
    const int64_t slot0 = tile * U8_TILE - mis;
    const int64_t p_lo = slot0 < 0 ? 0 : slot0;
    const int64_t p_hi = slot0 + U8_TILE < total ? slot0 + U8_TILE : total;
    uint32_t b[U8_N];
    int64_t p0;
    bool any80;
    u8_load_run(bytes_al, tile, mis, total, b, p0, any80);
    u8_load_halo(bytes_al, tile, mis, total, b, p0);
    u8_text_bits(s_f, tile, n_tiles, slot0, p_lo, p_hi, tile_first, tile_edge, off, n_texts, base);
    const U8Masks m = u8_classify(b, u8_lane_bits(s_f), u8_valid(p0, total));
    int n_units = 0;
    const int before = block_scan<U8_WG>(__builtin_popcount(m.start) + __builtin_popcount(m.four), scn, n_units);
    s_pre[tid] = before;
    s_start[tid] = m.start;
    s_four[tid] = m.four;
    const unsigned long long tb = tile_base[tile];
    // the output's 16-B phase: unit i of the tile sits at s_units[a + i], so that chunk c of eight
    // units is one aligned 16-B word both in LDS and at units_out + tb - a
    const int a = units_out ? (int)(((uintptr_t)(units_out + tb) >> 1) & 7) : 0;
    if (units_out) {
        int r = a + before;
#pragma unroll
        for (int j = 0; j < U8_RUN; ++j) {
            const int s = U8_HALO + j;
            if (!((m.start >> s) & 1)) continue;
            uint32_t u0, u1;
            const int k = u8_units_at(b, m, s, u0, u1);
            s_units[r++] = (uint16_t)u0;
            if (k == 2) s_units[r++] = (uint16_t)u1;
        }
    }
    __syncthreads();
    if (units_out) {
        uint16_t *out_al = units_out + tb - a;   // (never dereferenced below units_out + tb)
        const int end = a + n_units;
        for (int c = tid; c * 8 < end; c += U8_WG) {
            if (c * 8 >= a && c * 8 + 8 <= end) {
                *reinterpret_cast<uint4 *>(out_al + c * 8) = *reinterpret_cast<const uint4 *>(s_units + c * 8);
            } else {
                for (int i = c * 8 < a ? a : c * 8; i < c * 8 + 8 && i < end; ++i) out_al[i] = s_units[i];
            }
        }
    }
    // out_off of the texts that start inside the tile (the last tile: also those at the very end)
    const long long k0 = tile_first[tile];
    if (k0 < 0) return;
    for (int64_t k = k0 + tid; k <= n_texts; k += U8_WG) {
        const int64_t p = off[k] - base;
        if (p < p_lo || p > p_hi || (p == p_hi && !last)) break;
        const int s = (int)(p - slot0);
        int v = n_units;
        if (s < U8_TILE) {
            const uint32_t below = (1u << (U8_HALO + (s & (U8_RUN - 1)))) - 1u;
            v = s_pre[s / U8_RUN] + __builtin_popcount(s_start[s / U8_RUN] & below) +
                __builtin_popcount(s_four[s / U8_RUN] & below);
        }
        out_off[k] = (int64_t)(tb + (unsigned long long)v);
    }
}

#define U8_TRY(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return bpe_fail(e_ == hipErrorOutOfMemory ? BPE_ERR_OOM : BPE_ERR_HIP,         \
                            (std::string("bpe native: ") + #expr + ": " +                   \
                             hipGetErrorString(e_)).c_str());                              \
    } while (0)

// ---- host side: the transcode of one call on one device and stream -------------------------------

}  // namespace

// Scratch (grow-only), status words, events and counters of the UTF-8 front of an encoder or context.
struct Utf8State {
    char *d_buf = nullptr;
    size_t d_cap = 0;
    unsigned long long *d_st = nullptr, *h_st = nullptr;   // (h_st pinned)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bpe_utf8_stats st{};
};

namespace {

inline void u8_free(Utf8State &U) {
    if (U.d_buf) (void)hipFree(U.d_buf);
    if (U.d_st) (void)hipFree(U.d_st);
    if (U.h_st) (void)hipHostFree(U.h_st);
    for (hipEvent_t &ev : U.ev)
        if (ev) (void)hipEventDestroy(ev);
    U = Utf8State{};
}

inline size_t u8_align(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

// One call's transcode.  In: the call's arguments.  Out: where the units and their offsets are on
// the device, scratch for the values of an encode's host form, and the call's numbers, which
// the caller adds to the counters once its whole pipeline has succeeded (u8_commit).
struct Utf8Call {
    // in
    const uint8_t *bytes = nullptr;   // text k = bytes[off[k] .. off[k+1])
    const int64_t *off = nullptr;
    int64_t n_texts = 0;
    bool dev = false;                 // bytes and off are device buffers
    uint16_t *d_units = nullptr;      // the caller's device output, or nullptr: into scratch
    int64_t *d_uoff = nullptr;        // ... its n_texts + 1 offsets, or nullptr: into scratch
    int64_t cap = -1;                 // units the output may hold; -1: as many as there are bytes
    int64_t vals_cap = -1;            // >= 0: scratch for min(vals_cap, bytes) int32 values and n_texts + 1 offsets
    // out
    int32_t *d_vals = nullptr;        // (with vals_cap)
    int64_t *d_ooff = nullptr;
    int64_t s_cap = 0;                // values d_vals holds
    int64_t total = 0, units = 0, replaced = 0;
    double ms = 0;
    bool fits = true;                 // false: units > cap, only the offsets were written
    std::vector<int64_t> h_off;       // the call's offsets on the host, checked
};

namespace {

inline int u8_transcode(Utf8State &U, hipStream_t s, Utf8Call &J) {
    const int64_t n = J.n_texts;
    if (n < 0 || n >= 0x7FFFFFFF || (n && !J.off)) return bpe_fail(BPE_ERR_ARG, "bpe native: bad utf8 batch arguments");
    J.h_off.assign((size_t)n + 1, 0);
    if (n) {
        if (J.dev) {
            U8_TRY(hipMemcpyAsync(J.h_off.data(), J.off, J.h_off.size() * 8, hipMemcpyDeviceToHost, s));
            U8_TRY(hipStreamSynchronize(s));
        } else {
            std::copy(J.off, J.off + n + 1, J.h_off.begin());
        }
    }
    if (n && J.h_off[0] < 0) return bpe_fail(BPE_ERR_ARG, "bpe native: negative text offset");
    for (int64_t k = 0; k < n; ++k)
        if (J.h_off[k + 1] < J.h_off[k]) return bpe_fail(BPE_ERR_ARG, "bpe native: text offsets must not decrease");
    const int64_t base0 = n ? J.h_off[0] : 0, total = n ? J.h_off[n] - base0 : 0;
    if (total && !J.bytes) return bpe_fail(BPE_ERR_ARG, "bpe native: null byte buffer");
    J.total = total;
    if (!U.d_st) U8_TRY(hipMalloc((void **)&U.d_st, TS_WORDS * 8));
    if (!U.h_st) U8_TRY(hipHostMalloc((void **)&U.h_st, TS_WORDS * 8, hipHostMallocDefault));
    for (hipEvent_t &ev : U.ev)
        if (!ev) U8_TRY(hipEventCreate(&ev));
    // the host form stages bytes and offsets (rebased to the staged bytes) at a 16-B address
    const int mis = J.dev && total ? (int)((uintptr_t)(J.bytes + base0) & 15) : 0;
    const int64_t n_tiles = (total + mis + U8_TILE - 1) / U8_TILE;
    if (n_tiles > 0x7FFFFFFF) return bpe_fail(BPE_ERR_ARG, "bpe native: utf8 batch too large");
    const int64_t cap = J.cap < 0 ? total : J.cap;
    // scratch: [tile counts, then bases | first text of each tile | tile edges | bytes | off | units | uoff | vals | ooff]
    const size_t b_tiles = u8_align((size_t)n_tiles * 8), b_edge = u8_align((size_t)n_tiles * 4);
    const size_t b_bytes = J.dev ? 0 : u8_align((size_t)total), b_off = J.dev ? 0 : u8_align((size_t)(n + 1) * 8);
    const size_t b_units = J.d_units ? 0 : u8_align((size_t)std::min(cap, total) * 2);
    const size_t b_uoff = J.d_uoff ? 0 : u8_align((size_t)(n + 1) * 8);
    J.s_cap = std::min(std::max<int64_t>(J.vals_cap, 0), total);
    const size_t b_vals = J.vals_cap < 0 ? 0 : u8_align((size_t)std::max<int64_t>(J.s_cap, 1) * 4);
    const size_t b_ooff = J.vals_cap < 0 ? 0 : u8_align((size_t)(n + 1) * 8);
    const size_t need = 2 * b_tiles + b_edge + b_bytes + b_off + b_units + b_uoff + b_vals + b_ooff;
    if (need > U.d_cap) {
        U8_TRY(hipStreamSynchronize(s));
        if (U.d_buf) (void)hipFree(U.d_buf);
        U.d_buf = nullptr;
        U.d_cap = 0;
        const size_t want = need + need / 4 + 4096;
        U8_TRY(hipMalloc((void **)&U.d_buf, want));
        U.d_cap = want;
    }
    char *d = U.d_buf;
    unsigned long long *d_tiles = reinterpret_cast<unsigned long long *>(d);
    long long *d_first = reinterpret_cast<long long *>(d += b_tiles);
    uint32_t *d_edge = reinterpret_cast<uint32_t *>(d += b_tiles);
    uint8_t *s_bytes = reinterpret_cast<uint8_t *>(d += b_edge);
    int64_t *s_off = reinterpret_cast<int64_t *>(d += b_bytes);
    uint16_t *s_units = reinterpret_cast<uint16_t *>(d += b_off);
    int64_t *s_uoff = reinterpret_cast<int64_t *>(d += b_units);
    J.d_vals = reinterpret_cast<int32_t *>(d += b_uoff);
    J.d_ooff = reinterpret_cast<int64_t *>(d + b_vals);
    if (!J.d_units) J.d_units = s_units;
    if (!J.d_uoff) J.d_uoff = s_uoff;
    J.units = J.replaced = 0;
    J.ms = 0;
    J.fits = true;
    if (total == 0) {   // (no text, or every text empty)
        U8_TRY(hipMemsetAsync(J.d_uoff, 0, (size_t)(n + 1) * 8, s));
        U8_TRY(hipStreamSynchronize(s));
        return BPE_OK;
    }
    const uint8_t *bytes_al;
    const int64_t *k_off;
    int64_t base = base0;
    if (J.dev) {
        bytes_al = J.bytes + base0 - mis;
        k_off = J.off;
    } else {
        std::vector<int64_t> rel((size_t)n + 1);
        for (int64_t k = 0; k <= n; ++k) rel[(size_t)k] = J.h_off[(size_t)k] - base0;
        U8_TRY(hipMemcpyAsync(s_bytes, J.bytes + base0, (size_t)total, hipMemcpyHostToDevice, s));
        U8_TRY(hipMemcpyAsync(s_off, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        U8_TRY(hipStreamSynchronize(s));   // (rel goes away)
        bytes_al = s_bytes;
        k_off = s_off;
        base = 0;
    }
    U8_TRY(hipMemsetAsync(U.d_st, 0, TS_WORDS * 8, s));
    U8_TRY(hipMemsetAsync(d_first, 0xFF, (size_t)n_tiles * 8, s));
    U8_TRY(hipMemsetAsync(d_edge, 0, (size_t)n_tiles * 4, s));
    U8_TRY(hipEventRecord(U.ev[0], s));
    k_u8_texts<<<(unsigned)std::min<int64_t>((n + 256) / 256, 2048), 256, 0, s>>>(mis, total, k_off, n, base, n_tiles,
                                                                                 d_first, d_edge);
    k_u8_count<<<(unsigned)n_tiles, U8_WG, 0, s>>>(bytes_al, mis, total, n_tiles, d_first, d_edge, k_off, n, base,
                                                  d_tiles, U.d_st);
    k_txt_scan<<<1, 1024, 0, s>>>(d_tiles, n_tiles, U.d_st);
    U8_TRY(hipGetLastError());
    U8_TRY(hipEventRecord(U.ev[1], s));
    U8_TRY(hipMemcpyAsync(U.h_st, U.d_st, TS_WORDS * 8, hipMemcpyDeviceToHost, s));
    U8_TRY(hipStreamSynchronize(s));
    J.units = (int64_t)U.h_st[TS_CHARS];
    J.replaced = (int64_t)U.h_st[U8S_REPLACED];
    if (J.units < 0 || J.units > total || J.replaced < 0 || J.replaced > J.units)
        return bpe_fail(BPE_ERR_STATE, "bpe native: bad utf8 unit count");
    J.fits = J.units <= cap;
    U8_TRY(hipEventRecord(U.ev[2], s));
    k_u8_map<<<(unsigned)n_tiles, U8_WG, 0, s>>>(bytes_al, mis, total, n_tiles, d_tiles, d_first, d_edge, k_off, n, base,
                                                J.fits ? J.d_units : nullptr, J.d_uoff);
    U8_TRY(hipGetLastError());
    U8_TRY(hipEventRecord(U.ev[3], s));
    U8_TRY(hipStreamSynchronize(s));
    float ms0 = 0, ms1 = 0;
    U8_TRY(hipEventElapsedTime(&ms0, U.ev[0], U.ev[1]));
    U8_TRY(hipEventElapsedTime(&ms1, U.ev[2], U.ev[3]));
    J.ms = (double)ms0 + (double)ms1;
    return BPE_OK;
}

// the counters of a call whose pipeline succeeded
inline void u8_commit(Utf8State &U, const Utf8Call &J) {
    U.st.texts += J.n_texts;
    U.st.bytes += J.total;
    U.st.units += J.units;
    U.st.replaced += J.replaced;
    U.st.kernel_ms += J.ms;
}

inline int u8_cap_error(const Utf8Call &J) {
    char msg[128];
    std::snprintf(msg, sizeof msg, "bpe native: utf8_to_utf16 needs %lld units, the buffer holds %lld",
                  (long long)J.units, (long long)J.cap);
    return bpe_fail(BPE_ERR_ARG, msg);
}

}  // namespace
