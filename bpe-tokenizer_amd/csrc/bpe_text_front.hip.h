// bpe_text_front.hip.h — the shared part of the text front end: UTF-16 code units -> one char per
// `for (let char of content)` step (core.ts:396, core.ts:184), for the two translation units that
// read text: the encoder (bpe_encode.hip with bpe_text.hip.h: units -> ids of a known char table)
// and the corpus ingest (bpe_engine.hip with bpe_ingest.hip.h: units -> new char tokens, samples
// and counts).  Everything here has internal linkage: each unit compiles its own copy from this
// one source.
//
// Tiling: tiles of BPE_TEXT_TILE units cut at 16-B addresses of the unit buffer (slot s of tile t
// holds the flat position t * TILE + s - mis, mis = the buffer's misalignment in units), 8 units
// (one 16-B load) per lane.
//   k_txt_count  chars per tile by the local rule alone: a unit continues the char before it when
//                it is a low surrogate right after a high one.  Four tiles per workgroup, all loads
//                issued first; one plain store per tile;
//   k_txt_texts  one pass over the texts' offsets: the first text that starts in each tile is
//                noted, a text that starts at a tile's slot 0 marks that tile (the lane holding the
//                unit before it sits in the tile before), and a text boundary that falls between a
//                high and a low surrogate adds the one char the local rule missed to its tile
//                (an atomic per such boundary: rare);
//   k_txt_scan   one workgroup: exclusive scan of the tile counts (BPE_TEXT_SCAN_ROUND per round).
// The per-tile kernels that follow (k_txt_map, k_ing_discover, k_ing_map) rebuild every lane's
// start flags from its units and the texts that start in the tile, and look chars up with
// txt_lookup.
#pragma once

namespace {

// Wave scans on the VALU: DPP row shifts inside each 16-lane row, then the row results through
// v_readlane (no LDS crossbar round trips, unlike __shfl_*).
template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t v, uint32_t old) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, 0xF, 0xF, false);
}

__device__ __forceinline__ int wave_incl(int v, int lane) {
    uint32_t u = (uint32_t)v;
    u += dpp<0x111>(u, 0);   // row_shr:1 (lanes without a source add 0)
    u += dpp<0x112>(u, 0);   // row_shr:2
    u += dpp<0x114>(u, 0);   // row_shr:4
    u += dpp<0x118>(u, 0);   // row_shr:8
    const int r = lane >> 4;
    const int t0 = __builtin_amdgcn_readlane((int)u, 15), t1 = __builtin_amdgcn_readlane((int)u, 31);
    const int t2 = __builtin_amdgcn_readlane((int)u, 47);
    return (int)u + (r >= 1 ? t0 : 0) + (r >= 2 ? t1 : 0) + (r >= 3 ? t2 : 0);
}

// exclusive prefix and total over the workgroup (one barrier; `s` holds one word per wave)
template <int WG>
__device__ __forceinline__ int block_scan(int v, int *s, int &total) {
    const int lane = threadIdx.x & 63;
    const int incl = wave_incl(v, lane);
    if (WG == 64) {
        total = __builtin_amdgcn_readlane(incl, 63);
        __syncthreads();   // (this step's flags, written by other lanes, are read next)
        return incl - v;
    }
    const int w = threadIdx.x >> 6;
    if (lane == 63) s[w] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < WG / 64; ++i) {
        const int x = s[i];
        before += i < w ? x : 0;
        all += x;
    }
    total = all;
    return before + incl - v;
}

constexpr int TXT_TILE = BPE_TEXT_TILE;
constexpr int TXT_WG = 256;
constexpr int TXT_RUN = 8;          // units per lane and load (16 B)
constexpr int TXT_CNT_TILES = 4;    // tiles per workgroup of k_txt_count
constexpr int TXT_SCAN_EACH = 2;    // tile counts per thread and round of k_txt_scan
static_assert(TXT_TILE == TXT_WG * TXT_RUN, "one 16-B load of units per lane");
static_assert(1024 * TXT_SCAN_EACH == BPE_TEXT_SCAN_ROUND, "include/bpe.h");
constexpr unsigned long long TXT_NONE = ~0ull;
// status words of a call on the device
constexpr int TS_BADCHAR = 0;   // least flat unit position of an unknown char (TXT_NONE: none)
constexpr int TS_BADIDX = 1;    // least flat output position of a hole of the vector index
constexpr int TS_CHARS = 2;     // chars of the whole batch
constexpr int TS_WORDS = 4;
constexpr uint32_t PAIR_EMPTY = 0xFFFFFFFFu;
constexpr uint16_t CHAR_UNKNOWN = 0xFFFFu;

struct CharTab {
    const uint16_t *bmp;     // unit value -> id (BMP chars and lone surrogates), CHAR_UNKNOWN
    const uint2 *pairs;      // (code point, id), PAIR_EMPTY; linear probing from pair_home
    uint32_t mask, shift;    // slots = mask + 1 (a power of two >= 2 x the pairs), shift = 32 - log2
};

__host__ __device__ __forceinline__ uint32_t pair_home(uint32_t cp, uint32_t shift) {
    return (cp * 0x9E3779B1u) >> shift;
}

__device__ __forceinline__ bool is_high(uint32_t u) { return (u & 0xFC00u) == 0xD800u; }
__device__ __forceinline__ bool is_low(uint32_t u) { return (u & 0xFC00u) == 0xDC00u; }

// This lane's run of tile `tile`: u[1..8] its units (flat positions p0 .. p0 + 7), u[0] the unit
// before them and u[9] the unit after; every position outside [0, total) reads as 0 (no surrogate)
// and is never loaded.  units_al is the unit buffer's 16-B aligned base (the flat position -mis).
__device__ __forceinline__ void txt_load(const uint16_t *__restrict__ units_al, int64_t tile, int mis,
                                         int64_t total, uint32_t u[TXT_RUN + 2], int64_t &p0) {
    const int64_t s = tile * TXT_TILE + TXT_RUN * (int64_t)threadIdx.x;
    p0 = s - mis;
    if (p0 >= 0 && p0 + TXT_RUN <= total) {
        const uint4 x = *reinterpret_cast<const uint4 *>(units_al + s);
        u[1] = x.x & 0xFFFFu, u[2] = x.x >> 16, u[3] = x.y & 0xFFFFu, u[4] = x.y >> 16;
        u[5] = x.z & 0xFFFFu, u[6] = x.z >> 16, u[7] = x.w & 0xFFFFu, u[8] = x.w >> 16;
    } else {
#pragma unroll
        for (int j = 0; j < TXT_RUN; ++j)
            u[j + 1] = (p0 + j >= 0 && p0 + j < total) ? units_al[s + j] : 0u;
    }
    u[0] = (p0 - 1 >= 0 && p0 - 1 < total) ? units_al[s - 1] : 0u;
    u[TXT_RUN + 1] = (p0 + TXT_RUN >= 0 && p0 + TXT_RUN < total) ? units_al[s + TXT_RUN] : 0u;
}

// bit j: the unit at slot j of the run (j = 8: the unit after it) continues the char before it by
// the local rule
__device__ __forceinline__ uint32_t txt_cont(const uint32_t u[TXT_RUN + 2]) {
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j <= TXT_RUN; ++j) c |= (uint32_t)(is_low(u[j + 1]) && is_high(u[j])) << j;
    return c;
}

// bit j: slot j of the run holds a unit of the batch
__device__ __forceinline__ uint32_t txt_valid(int64_t p0, int64_t total) {
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < TXT_RUN; ++j) v |= (uint32_t)(p0 + j >= 0 && p0 + j < total) << j;
    return v;
}

// The char that starts at slot j of the run (a start by `cont`, the run's continuation bits after
// the texts' boundaries were taken out): its key (the code point; a lone surrogate's unit value)
// and whether it is a surrogate pair.
__device__ __forceinline__ uint32_t txt_key(const uint32_t u[TXT_RUN + 2], uint32_t cont, int j, bool &pair) {
    const uint32_t h = u[j + 1];
    pair = is_high(h) && ((cont >> (j + 1)) & 1);
    return pair ? 0x10000u + ((h - 0xD800u) << 10) + (u[j + 2] - 0xDC00u) : h;
}

// The id of a char in the table, CHAR_UNKNOWN when it is not there (pairs: probed only by the
// lanes that hold one).
__device__ __forceinline__ uint32_t txt_lookup(const CharTab &ct, uint32_t key, bool pair) {
    if (!pair) return ct.bmp[key];
    uint32_t s = pair_home(key, ct.shift);
    for (;;) {
        const uint2 e = ct.pairs[s];
        if (e.x == key) return e.y;
        if (e.x == PAIR_EMPTY) return CHAR_UNKNOWN;
        s = (s + 1) & ct.mask;
    }
}

__device__ __forceinline__ unsigned long long txt_wave_incl64(unsigned long long v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

__global__ void __launch_bounds__(TXT_WG)
k_txt_count(const uint16_t *__restrict__ units_al, int mis, int64_t total, int64_t n_tiles,
            unsigned long long *__restrict__ tile_cnt) {
    __shared__ int ws[TXT_CNT_TILES][TXT_WG / 64];
    const int64_t tile0 = (int64_t)blockIdx.x * TXT_CNT_TILES;
    uint32_t u[TXT_CNT_TILES][TXT_RUN + 2];
    int64_t p0[TXT_CNT_TILES];
#pragma unroll
    for (int g = 0; g < TXT_CNT_TILES; ++g) {
        if (tile0 + g < n_tiles) {
            txt_load(units_al, tile0 + g, mis, total, u[g], p0[g]);
        } else {
#pragma unroll
            for (int j = 0; j < TXT_RUN + 2; ++j) u[g][j] = 0;
            p0[g] = total;   // (no slot valid)
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < TXT_CNT_TILES; ++g) {
        const int cnt = __builtin_popcount(txt_valid(p0[g], total) & ~txt_cont(u[g]));
        const int incl = wave_incl(cnt, lane);
        if (lane == 63) ws[g][w] = incl;
    }
    __syncthreads();
    if (threadIdx.x < TXT_CNT_TILES && tile0 + threadIdx.x < n_tiles) {
        int all = 0;
#pragma unroll
        for (int i = 0; i < TXT_WG / 64; ++i) all += ws[threadIdx.x][i];
        tile_cnt[tile0 + threadIdx.x] = (unsigned long long)all;
    }
}

// A text at the very end of the units belongs to the last tile.
__device__ __forceinline__ int64_t txt_tile_of(int64_t p, int mis, int64_t n_tiles) {
    const int64_t t = (p + mis) / TXT_TILE;
    return t < n_tiles ? t : n_tiles - 1;
}

// (after k_txt_count on the stream: it adds to the counts that kernel stored; the host has checked
// the offsets' order)
__global__ void __launch_bounds__(256)
k_txt_texts(const uint16_t *__restrict__ units_al, int mis, int64_t total, const int64_t *__restrict__ off,
            int64_t n_texts, int64_t base, int64_t n_tiles, long long *__restrict__ tile_first,
            uint32_t *__restrict__ tile_edge, unsigned long long *__restrict__ tile_cnt) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k <= n_texts; k += (int64_t)gridDim.x * 256) {
        const int64_t p = off[k] - base;
        const int64_t t = txt_tile_of(p, mis, n_tiles);
        const int64_t q = k ? off[k - 1] - base : -1;
        if (k == 0 || txt_tile_of(q, mis, n_tiles) != t) tile_first[t] = k;
        if (p > 0 && p < total && q != p) {   // the first text that starts at this unit
            if ((p + mis) % TXT_TILE == 0) tile_edge[t] = 1u;
            if (is_low(units_al[p + mis]) && is_high(units_al[p + mis - 1])) atomicAdd(&tile_cnt[t], 1ull);
        }
    }
}

// tile counts -> each tile's base (in place), and the total
__global__ void __launch_bounds__(1024)
k_txt_scan(unsigned long long *__restrict__ tile_cnt, int64_t n_tiles, unsigned long long *__restrict__ st) {
    __shared__ unsigned long long ws[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (int64_t b = 0; b < n_tiles; b += 1024 * TXT_SCAN_EACH) {
        const int64_t i0 = b + (int64_t)threadIdx.x * TXT_SCAN_EACH;
        unsigned long long v[TXT_SCAN_EACH], mine = 0;
#pragma unroll
        for (int e = 0; e < TXT_SCAN_EACH; ++e) {
            v[e] = i0 + e < n_tiles ? tile_cnt[i0 + e] : 0;
            mine += v[e];
        }
        const unsigned long long incl = txt_wave_incl64(mine, lane);
        if (lane == 63) ws[w] = incl;
        __syncthreads();
        unsigned long long before = 0, all = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const unsigned long long x = ws[i];
            before += i < w ? x : 0;
            all += x;
        }
        unsigned long long pre = carry + before + incl - mine;
#pragma unroll
        for (int e = 0; e < TXT_SCAN_EACH; ++e) {
            if (i0 + e < n_tiles) tile_cnt[i0 + e] = pre;
            pre += v[e];
        }
        carry += all;
        __syncthreads();   // (ws is reused next round)
    }
    if (threadIdx.x == 0) st[TS_CHARS] = carry;
}

}  // namespace
