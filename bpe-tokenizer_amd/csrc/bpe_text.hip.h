// bpe_text.hip.h — the text front end and the vector back end of the device encoder
// (bpe_encode_text_batch, include/bpe.h): encodeToVector (core.ts:392-445) from UTF-16 code units.
// Included by bpe_encode.hip, whose merge-rank kernel (k_encode) runs between the two.
//
// Front end: units -> compact token ids (one per char: `for (let char of content)`, core.ts:396)
// and the texts' id offsets, in four kernels over tiles of BPE_TEXT_TILE units cut at 16-B
// addresses of the unit buffer (slot s of tile t holds the flat position t * TILE + s - mis, mis =
// the buffer's misalignment in units), 8 units (one 16-B load) per lane.  The first three
// (k_txt_count, k_txt_texts, k_txt_scan) and the loads, the surrogate rule and the char lookup are
// bpe_text_front.hip.h's, shared with the corpus ingest; the fourth is here:
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

#include "bpe_text_front.hip.h"   // tiling, loads, surrogate rule, tile counts, scan, char lookup

namespace {

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
        bool pair;
        const uint32_t key = txt_key(u, cont, j, pair);
        uint32_t id = txt_lookup(ct, key, pair);
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
