// bpe_text.hip.h — the text front end and the vector back end of the device encoder
// (bpe_encode_text_batch, include/bpe.h): encodeToVector (core.ts:392-445) from UTF-16 code units.
// Included by bpe_encode.hip, whose merge-rank kernel (k_encode) runs between the two.
//
// Front end: units -> compact token ids (one per char: `for (let char of content)`, core.ts:396)
// and the texts' id offsets, in four kernels over tiles of BPE_TEXT_TILE units cut at 16-B
// addresses of the unit buffer (slot s of tile t holds the flat position t * TILE + s - mis, mis =
// the buffer's misalignment in units), 8 units (one 16-B load) per lane:
//   k_txt_count  chars per tile by the local rule alone: a unit continues the char before it when
//                it is a low surrogate right after a high one.  Four tiles per workgroup, all loads
//                issued first; one plain store per tile;
//   k_txt_texts  one pass over the texts' offsets: the first text that starts in each tile is
//                noted, a text that starts at a tile's slot 0 marks that tile (the lane holding the
//                unit before it sits in the tile before), and a text boundary that falls between a
//                high and a low surrogate adds the one char the local rule missed to its tile
//                (an atomic per such boundary: rare);
//   k_txt_scan   one workgroup: exclusive scan of the tile counts (BPE_TEXT_SCAN_ROUND per round);
//   k_txt_map    one workgroup per tile: the texts that start in the tile set their first unit's
//                bit in an LDS bitmap (a strided walk from the tile's first text: its cost follows
//                the texts), every lane rebuilds its 8 start flags from its units, the unit before
//                and the unit after them and those bits, a workgroup scan ranks the chars, each
//                char is looked up (BMP chars and lone surrogates: a 65 536-entry u16 table, 128 KiB,
//                L2-resident; pairs: an open-addressing hash on the code point, probed only by the
//                lanes that hold one), the ids are gathered in LDS and stored compact, and the same
//                walk over the tile's texts writes their id offsets.  The first unknown char goes
//                into a 64-bit atomicMin of its flat unit position (only such lanes issue it).
// Back end (BPE_ENCODE_VECTORS): the pack kernels' gather with to_vector_index[id] written instead
// of id; a hole or an id past the index goes into an atomicMin of its flat output position.
#pragma once

namespace {

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

__global__ void __launch_bounds__(TXT_WG)
k_txt_map(const uint16_t *__restrict__ units_al, int mis, int64_t total, CharTab ct,
          const unsigned long long *__restrict__ tile_base, const long long *__restrict__ tile_first,
          const uint32_t *__restrict__ tile_edge, const int64_t *__restrict__ off, int64_t n_texts,
          int64_t base, int32_t *__restrict__ ids, int64_t *__restrict__ id_off,
          unsigned long long *__restrict__ st) {
    __shared__ uint32_t s_force[TXT_TILE / 32];   // bit s: a text starts at slot s
    __shared__ int s_pre[TXT_WG + 1];             // chars before each lane's run
    __shared__ uint32_t s_mask[TXT_WG];           // each lane's start flags
    __shared__ int32_t s_ids[TXT_TILE];           // the tile's ids, compact
    __shared__ int scn[TXT_WG / 64];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const bool last = tile == (int64_t)gridDim.x - 1;
    const int64_t slot0 = tile * TXT_TILE - mis;   // flat position of slot 0
    const int64_t p_lo = slot0 < 0 ? 0 : slot0;    // the tile's flat positions: [p_lo, p_hi)
    const int64_t p_hi = slot0 + TXT_TILE < total ? slot0 + TXT_TILE : total;
    const long long k0 = tile_first[tile];
    const uint32_t edge = last ? 0u : tile_edge[tile + 1];
    if (tid < TXT_TILE / 32) s_force[tid] = 0;
    uint32_t u[TXT_RUN + 2];
    int64_t p0;
    txt_load(units_al, tile, mis, total, u, p0);
    __syncthreads();
    if (k0 >= 0) {
        for (int64_t k = k0 + tid; k <= n_texts; k += TXT_WG) {
            const int64_t p = off[k] - base;
            if (p < p_lo || p >= p_hi) break;   // (an offset at the very end forces nothing)
            atomicOr(&s_force[(p - slot0) >> 5], 1u << ((p - slot0) & 31));
        }
    }
    __syncthreads();
    uint32_t f = (s_force[tid >> 2] >> (8 * (tid & 3))) & 0xFFu;
    f |= (tid + 1 < TXT_WG ? (s_force[(tid + 1) >> 2] >> (8 * ((tid + 1) & 3))) & 1u : edge) << TXT_RUN;
    const uint32_t cont = txt_cont(u) & ~f;                  // bits 0..8
    const uint32_t m = txt_valid(p0, total) & ~cont;         // the chars that start in the run
    int n_chars = 0;
    const int before = block_scan<TXT_WG>(__builtin_popcount(m), scn, n_chars);
    s_pre[tid] = before;
    s_mask[tid] = m;
    if (tid == 0) s_pre[TXT_WG] = n_chars;
    int r = before;
#pragma unroll
    for (int j = 0; j < TXT_RUN; ++j) {
        if (!((m >> j) & 1)) continue;
        const uint32_t h = u[j + 1];
        uint32_t id;
        if (is_high(h) && ((cont >> (j + 1)) & 1)) {
            const uint32_t cp = 0x10000u + ((h - 0xD800u) << 10) + (u[j + 2] - 0xDC00u);
            uint32_t s = pair_home(cp, ct.shift);
            for (;;) {
                const uint2 e = ct.pairs[s];
                if (e.x == cp) {
                    id = e.y;
                    break;
                }
                if (e.x == PAIR_EMPTY) {
                    id = CHAR_UNKNOWN;
                    break;
                }
                s = (s + 1) & ct.mask;
            }
        } else {
            id = ct.bmp[h];
        }
        if (id == CHAR_UNKNOWN) {
            atomicMin(&st[TS_BADCHAR], (unsigned long long)(p0 + j));
            id = 0;   // (the call fails: any id the merge kernels take)
        }
        s_ids[r++] = (int32_t)id;
    }
    __syncthreads();
    const unsigned long long tb = tile_base[tile];
    for (int i = tid; i < n_chars; i += TXT_WG) ids[tb + i] = s_ids[i];
    // id_off of the texts that start inside the tile (the last tile: also those at the very end)
    if (k0 < 0) return;
    for (int64_t k = k0 + tid; k <= n_texts; k += TXT_WG) {
        const int64_t p = off[k] - base;
        if (p < p_lo || p > p_hi || (p == p_hi && !last)) break;
        const int s = (int)(p - slot0);
        const int v = s >= TXT_TILE ? n_chars
                                    : s_pre[s >> 3] + __builtin_popcount(s_mask[s >> 3] & ((1u << (s & 7)) - 1u));
        id_off[k] = (int64_t)(tb + (unsigned long long)v);
    }
}

// ---- back end: the pack kernels' map (k_pack_small, k_gather), writing to_vector_index[id] -----

struct VecMap {
    const int32_t *tvi;
    uint32_t n_tvi;
    unsigned long long *st;
    __device__ __forceinline__ int32_t operator()(int32_t id, unsigned long long pos) const {
        const int32_t v = (uint32_t)id < n_tvi ? tvi[id] : -1;
        if (v < 0) atomicMin(&st[TS_BADIDX], pos);
        return v;
    }
};

}  // namespace

// The text side of an encoder: the char table and the vector index (host copies; uploaded when
// dirty), the status words of a call and the events around the front-end and back-end kernels.
struct bpe_text_state {
    std::vector<uint16_t> bmp;
    std::vector<uint2> pairs;
    uint32_t pair_bits = 4;
    bool has_chars = false, chars_dirty = false;
    uint16_t *d_bmp = nullptr;
    uint2 *d_pairs = nullptr;
    size_t d_pairs_n = 0;
    std::vector<int32_t> tvi;
    bool has_tvi = false, tvi_dirty = false;
    int32_t *d_tvi = nullptr;
    size_t d_tvi_n = 0;
    unsigned long long *d_st = nullptr, *h_st = nullptr;   // (h_st pinned)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bpe_text_stats st{};
};
