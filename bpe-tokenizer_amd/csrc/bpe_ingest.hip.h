// bpe_ingest.hip.h — the kernels of the corpus ingest from text (bpe_add_text_batch, include/bpe.h):
// addToCorpus (core.ts:182-207) for a batch of UTF-16 texts.  Included by bpe_engine.hip, which
// launches them around the host's numbering of the new chars.  Tiling, loads, the surrogate rule,
// the tile counts and their scan and the char lookup are bpe_text_front.hip.h's, the encoder's.
//
// After k_txt_count, k_txt_texts and k_txt_scan:
//   k_ing_discover  one workgroup per tile.  Every char is looked up; only a lane that holds a char
//                   the table does not know does more: it lowers that char's least flat unit
//                   position (a plain read first, the atomicMin only when it would win, so a new
//                   char repeated a million times is not a million atomics on one address).  BMP
//                   chars and lone surrogates: a 65 536-entry u64 plane.  Pairs: an open-addressing
//                   insert (atomicCAS on the key word of ING_SUP_SLOTS slots), then the same
//                   atomicMin on the slot's position word.  The lane whose atomic found the entry
//                   empty appends it to the list of new chars, so no pass over the planes is needed.
//                   The insert ends when more than BPE_MAX_VOCAB pairs were claimed (the call has
//                   failed already) or after ING_SUP_SLOTS probes, raising IS_OVER: it never spins.
//   k_ing_collect   the list's (position, code point) pairs, for the host's sort by position.
//   k_ing_map       persistent workgroups over the tiles (the updated table): ids and separators
//                   written straight to the corpus.  A char's slot is its compact rank plus the
//                   index of its text.  The texts that start in the tile COUNT into one LDS word per
//                   slot (several may start at one unit: empty texts), a second workgroup scan over
//                   those counts runs beside the scan of the char flags, and a tile in which no text
//                   starts finds its text by one binary search of the offsets.  The same walk over
//                   the tile's texts writes the separators.
//                   Counts: an LDS histogram of the ids below ING_HOT per workgroup (new ids follow
//                   first appearance, so frequent chars tend to be low), flushed once at the end;
//                   a wave whose chars of one step are all alike adds once; ids at or past ING_HOT
//                   go to 64-bit global atomics, one per distinct id and wave step.  A workgroup
//                   takes at most ING_MAX_TILES_PER_WG tiles, so an LDS counter stays below
//                   2^20 x 2^11 = 2^31: no 32-bit partial can wrap.  The outputs are 64-bit.
#pragma once

#include "bpe_text_front.hip.h"

namespace {

constexpr int ING_SUP_BITS = 17;
constexpr uint32_t ING_SUP_SLOTS = 1u << ING_SUP_BITS;   // >= 2 x BPE_MAX_VOCAB
static_assert(ING_SUP_SLOTS >= 2 * BPE_MAX_VOCAB, "the insert's load factor stays below 1/2 until it fails");
constexpr uint32_t ING_LIST_CAP = 65536u + ING_SUP_SLOTS;   // every plane entry and slot is listed once
constexpr uint32_t ING_LIST_SUP = 0x80000000u;            // list entry: a slot of the pair insert
constexpr int ING_HOT = 8192;                             // ids with an LDS counter (32 KiB)
constexpr int64_t ING_MAX_TILES_PER_WG = 1 << 20;
static_assert(ING_MAX_TILES_PER_WG * TXT_TILE < (1ll << 32), "an LDS counter cannot wrap");
// status words (TS_CHARS is k_txt_scan's)
constexpr int IS_NLIST = 4;   // entries of the list
constexpr int IS_NSUP = 5;    // slots claimed by the pair insert
constexpr int IS_OVER = 6;    // the insert gave up
constexpr int IS_WORDS = 8;

struct IngNew {
    unsigned long long *first;     // [65536] least position per unit value (TXT_NONE)
    uint32_t *sup_keys;            // [ING_SUP_SLOTS] code point (PAIR_EMPTY)
    unsigned long long *sup_pos;   // [ING_SUP_SLOTS] least position (TXT_NONE)
    uint32_t *list;                // [ING_LIST_CAP]
    unsigned long long *st;
};

template <typename T>
__device__ __forceinline__ T ing_peek(const T *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The start flags of this lane's run from the tile's units and the texts that start in the tile
// (s_cnt: texts per slot, zeroed and filled here).  c[j]: texts that start at slot j of the run.
// Ends after a barrier: s_cnt is complete.
__device__ __forceinline__ void ing_tile(const uint16_t *__restrict__ units_al, int64_t tile, bool last, int mis,
                                         int64_t total, const long long *__restrict__ tile_first,
                                         const uint32_t *__restrict__ tile_edge, const int64_t *__restrict__ off,
                                         int64_t n_texts, int64_t base, uint32_t *s_cnt, uint32_t u[TXT_RUN + 2],
                                         int64_t &p0, uint32_t &cont, uint32_t &m, uint32_t c[TXT_RUN]) {
    const int tid = threadIdx.x;
    const int64_t slot0 = tile * TXT_TILE - mis;
    const int64_t p_lo = slot0 < 0 ? 0 : slot0;
    const int64_t p_hi = slot0 + TXT_TILE < total ? slot0 + TXT_TILE : total;
    const long long k0 = tile_first[tile];
    const uint32_t edge = last ? 0u : tile_edge[tile + 1];
#pragma unroll
    for (int j = 0; j < TXT_RUN; ++j) s_cnt[tid + j * TXT_WG] = 0;
    txt_load(units_al, tile, mis, total, u, p0);
    __syncthreads();
    if (k0 >= 0) {
        for (int64_t k = k0 + tid; k <= n_texts; k += TXT_WG) {
            const int64_t p = off[k] - base;
            if (p < p_lo || p >= p_hi) break;   // (an offset at the very end starts nothing)
            atomicAdd(&s_cnt[p - slot0], 1u);
        }
    }
    __syncthreads();
    uint32_t f = 0;
#pragma unroll
    for (int j = 0; j < TXT_RUN; ++j) {
        c[j] = s_cnt[TXT_RUN * tid + j];
        f |= (uint32_t)(c[j] != 0) << j;
    }
    f |= (tid + 1 < TXT_WG ? (uint32_t)(s_cnt[TXT_RUN * (tid + 1)] != 0) : edge) << TXT_RUN;
    cont = txt_cont(u) & ~f;
    m = txt_valid(p0, total) & ~cont;
}

__global__ void __launch_bounds__(TXT_WG)
k_ing_discover(const uint16_t *__restrict__ units_al, int mis, int64_t total, CharTab ct,
               const long long *__restrict__ tile_first, const uint32_t *__restrict__ tile_edge,
               const int64_t *__restrict__ off, int64_t n_texts, int64_t base, IngNew nw) {
    __shared__ uint32_t s_cnt[TXT_TILE];
    const int64_t tile = blockIdx.x;
    uint32_t u[TXT_RUN + 2], c[TXT_RUN], cont, m;
    int64_t p0;
    ing_tile(units_al, tile, tile == (int64_t)gridDim.x - 1, mis, total, tile_first, tile_edge, off, n_texts, base,
             s_cnt, u, p0, cont, m, c);
#pragma unroll
    for (int j = 0; j < TXT_RUN; ++j) {
        if (!((m >> j) & 1)) continue;
        bool pair;
        const uint32_t key = txt_key(u, cont, j, pair);
        if (txt_lookup(ct, key, pair) != CHAR_UNKNOWN) continue;
        const unsigned long long pos = (unsigned long long)(p0 + j);
        if (!pair) {
            if (pos < ing_peek(&nw.first[key])) {
                if (atomicMin(&nw.first[key], pos) == TXT_NONE) {
                    const unsigned long long at = atomicAdd(&nw.st[IS_NLIST], 1ull);
                    if (at < ING_LIST_CAP) nw.list[at] = key;
                }
            }
            continue;
        }
        uint32_t s = pair_home(key, 32 - ING_SUP_BITS);
        uint32_t probes = 0;
        for (; probes < ING_SUP_SLOTS; ++probes) {
            uint32_t k = ing_peek(&nw.sup_keys[s]);
            if (k == PAIR_EMPTY) {
                if (ing_peek(&nw.st[IS_OVER])) break;   // (the call has failed: claim nothing more)
                k = atomicCAS(&nw.sup_keys[s], PAIR_EMPTY, key);
                if (k == PAIR_EMPTY) {
                    k = key;
                    if (atomicAdd(&nw.st[IS_NSUP], 1ull) >= (unsigned long long)BPE_MAX_VOCAB)
                        atomicExch(&nw.st[IS_OVER], 1ull);
                    const unsigned long long at = atomicAdd(&nw.st[IS_NLIST], 1ull);
                    if (at < ING_LIST_CAP) nw.list[at] = ING_LIST_SUP | s;
                }
            }
            if (k == key) {
                if (pos < ing_peek(&nw.sup_pos[s])) atomicMin(&nw.sup_pos[s], pos);
                break;
            }
            s = (s + 1) & (ING_SUP_SLOTS - 1);
        }
        if (probes == ING_SUP_SLOTS) atomicExch(&nw.st[IS_OVER], 1ull);
    }
}

// out[2 i] = the least position, out[2 i + 1] = the code point of list entry i (cap entries)
__global__ void __launch_bounds__(256) k_ing_collect(IngNew nw, unsigned long long *__restrict__ out, uint32_t cap) {
    const unsigned long long n_all = nw.st[IS_NLIST];
    const uint32_t n = n_all < cap ? (uint32_t)n_all : cap;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t e = nw.list[i];
        if (e & ING_LIST_SUP) {
            const uint32_t s = e & (ING_SUP_SLOTS - 1);
            out[2 * (size_t)i] = nw.sup_pos[s];
            out[2 * (size_t)i + 1] = nw.sup_keys[s];
        } else {
            out[2 * (size_t)i] = nw.first[e & 0xFFFFu];
            out[2 * (size_t)i + 1] = e;
        }
    }
}

// dst: the corpus at its first free slot; room for the batch's chars + n_texts slots.  A char the
// table does not know (there is none after the host's update) raises IS_OVER and writes id 0.
__global__ void __launch_bounds__(TXT_WG)
k_ing_map(const uint16_t *__restrict__ units_al, int mis, int64_t total, int64_t n_tiles, CharTab ct,
          const unsigned long long *__restrict__ tile_base, const long long *__restrict__ tile_first,
          const uint32_t *__restrict__ tile_edge, const int64_t *__restrict__ off, int64_t n_texts,
          int64_t base, int32_t sep, int32_t *__restrict__ dst, unsigned long long *__restrict__ hist,
          unsigned long long *__restrict__ st) {
    __shared__ uint32_t s_cnt[TXT_TILE];     // texts that start at each slot
    __shared__ uint32_t s_hist[ING_HOT];     // this workgroup's occurrences of the ids below ING_HOT
    __shared__ int s_pre[TXT_WG + 1];        // chars before each lane's run
    __shared__ uint32_t s_mask[TXT_WG];      // each lane's start flags
    __shared__ int scn[TXT_WG / 64], scn2[TXT_WG / 64];
    __shared__ long long s_prev;             // the text the tile begins in, when none starts in it
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < ING_HOT; i += TXT_WG) s_hist[i] = 0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const bool last = tile == n_tiles - 1;
        const int64_t slot0 = tile * TXT_TILE - mis;
        const int64_t p_lo = slot0 < 0 ? 0 : slot0;
        const int64_t p_hi = slot0 + TXT_TILE < total ? slot0 + TXT_TILE : total;
        const long long k0 = tile_first[tile];
        if (k0 < 0 && tid == 0) {
            // the last text with off[k] - base <= p_lo (it starts in a tile before this one)
            int64_t lo = 0, hi = n_texts;   // off[lo] - base <= p_lo < off[hi] - base
            while (hi - lo > 1) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (off[mid] - base <= p_lo) lo = mid;
                else hi = mid;
            }
            s_prev = lo;
        }
        uint32_t u[TXT_RUN + 2], c[TXT_RUN], cont, m;
        int64_t p0;
        ing_tile(units_al, tile, last, mis, total, tile_first, tile_edge, off, n_texts, base, s_cnt, u, p0, cont, m,
                 c);
        int starts = 0;
#pragma unroll
        for (int j = 0; j < TXT_RUN; ++j) starts += (int)c[j];
        int n_chars = 0, n_starts = 0;
        const int before = block_scan<TXT_WG>(__builtin_popcount(m), scn, n_chars);
        const int starts_before = block_scan<TXT_WG>(starts, scn2, n_starts);
        s_pre[tid] = before;
        s_mask[tid] = m;
        if (tid == 0) s_pre[TXT_WG] = n_chars;
        const unsigned long long tb = tile_base[tile];
        // the text of the char before this lane's run
        int64_t t = (k0 >= 0 ? (int64_t)k0 - 1 : (int64_t)s_prev) + starts_before;
        int r = before;
#pragma unroll
        for (int j = 0; j < TXT_RUN; ++j) {
            t += c[j];
            const bool have = (m >> j) & 1;
            uint32_t id = 0;
            if (have) {
                bool pair;
                const uint32_t key = txt_key(u, cont, j, pair);
                id = txt_lookup(ct, key, pair);
                if (id == CHAR_UNKNOWN) {
                    atomicExch(&st[IS_OVER], 1ull);
                    id = 0;
                }
                dst[tb + (unsigned long long)r + (unsigned long long)t] = (int32_t)id;
                ++r;
            }
            // counts (the whole wave takes every step)
            const unsigned long long all = __ballot(have);
            if (all) {
                const uint32_t lid = (uint32_t)__builtin_amdgcn_readlane((int)id, __builtin_ctzll(all));
                const unsigned long long same = __ballot(have && id == lid);
                if (same == all) {
                    if (lane == __builtin_ctzll(all)) {
                        const uint32_t n = (uint32_t)__builtin_popcountll(all);
                        if (lid < ING_HOT) atomicAdd(&s_hist[lid], n);
                        else atomicAdd(&hist[lid], (unsigned long long)n);
                    }
                } else {
                    if (have && id < ING_HOT) atomicAdd(&s_hist[id], 1u);
                    unsigned long long cold = __ballot(have && id >= ING_HOT);
                    while (cold) {
                        const int lead = __builtin_ctzll(cold);
                        const uint32_t cid = (uint32_t)__builtin_amdgcn_readlane((int)id, lead);
                        const unsigned long long eq = __ballot(have && id == cid);
                        if (lane == lead) atomicAdd(&hist[cid], (unsigned long long)__builtin_popcountll(eq));
                        cold &= ~eq;
                    }
                }
            }
        }
        __syncthreads();   // (s_pre, s_mask)
        // the separators of the texts that end where a text of this tile starts (text k - 1 ends at
        // off[k]); the last tile: also those at the very end
        if (k0 >= 0) {
            for (int64_t k = k0 + tid; k <= n_texts; k += TXT_WG) {
                const int64_t p = off[k] - base;
                if (p < p_lo || p > p_hi || (p == p_hi && !last)) break;
                if (k == 0) continue;
                const int s = (int)(p - slot0);
                const int v = s >= TXT_TILE
                                  ? n_chars
                                  : s_pre[s >> 3] + __builtin_popcount(s_mask[s >> 3] & ((1u << (s & 7)) - 1u));
                dst[tb + (unsigned long long)v + (unsigned long long)(k - 1)] = sep;
            }
        }
        __syncthreads();   // (the next tile reuses the LDS words)
    }
    for (int i = tid; i < ING_HOT; i += TXT_WG) {
        const uint32_t n = s_hist[i];
        if (n) atomicAdd(&hist[i], (unsigned long long)n);
    }
}

}  // namespace
