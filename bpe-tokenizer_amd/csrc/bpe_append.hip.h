// bpe_append.hip.h — the kernel of the corpus append from encoded samples (bpe_add_sample_batch and
// bpe_restore_text_batch, include/bpe.h): bpe_add_sample for a batch, from the encoder's packed
// layout (values back to back, n + 1 offsets) into the corpus layout (each sample's ids, then a
// separator).  Included by bpe_engine.hip, which launches it between append_begin and seal_packed.
//
//   k_smp_append    output-centric: the appended region has total + n slots, and with
//                   g[k] = off[k] - off[0] + k sample k owns the slots [g[k], g[k+1]), the last of
//                   them its separator.  g is strictly increasing even across empty samples, so a
//                   slot s of sample k is either the separator or token s - k of the batch.
//                   A workgroup takes a contiguous range of tiles of BPE_APPEND_TILE slots.  The tiles
//                   are laid on the DESTINATION's 16-byte grid (the corpus's first free slot has any
//                   residue mod 4: the first tile starts up to 3 slots before the region), so every
//                   lane's four slots are one aligned 16-byte store; only the region's head and tail
//                   take single stores.  The sample of the range's first slot comes from one uniform
//                   binary search of g; after that the first sample of the next tile is this tile's
//                   first plus the samples that ended in it.  Those are one bit per slot in an LDS
//                   bitmap (set from off[k + 1], 8 B per sample), a wave scans the bitmap's 64 words,
//                   and a lane's sample is the tile's first plus a popcount prefix: no count plane
//                   and no second scan.  The tile's tokens are one contiguous run of the source: it
//                   is staged through LDS by aligned 16-byte loads (single loads at the batch's ends).
//                   Counts as the ingest's map (bpe_ingest.hip.h): an LDS histogram of the ids below
//                   APP_HOT per workgroup, flushed once as 64-bit atomics; a wave whose ids of one
//                   step are all alike adds once; ids at or past APP_HOT take 64-bit global atomics,
//                   one per distinct id and wave step.  A workgroup takes at most
//                   APP_MAX_TILES_PER_WG tiles, so an LDS counter stays below 2^20 x 2^11 = 2^31.
//                   Ids outside [0, BPE_MAX_VOCAB) are counted (st[APP_BAD]; they are written but not
//                   histogrammed: the host fails the call and seals the corpus again), and
//                   st[APP_MAX] receives the largest id + 1.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bpe.h"

namespace {

constexpr int APP_WG = 256;
constexpr int APP_TILE = BPE_APPEND_TILE;
constexpr int APP_GROUPS = APP_TILE / (4 * APP_WG);   // 16-byte groups per lane and tile
constexpr int APP_BITS = APP_TILE / 32;               // words of the tile's bitmap
constexpr int APP_HOT = 8192;                         // ids with an LDS counter (32 KiB)
constexpr int64_t APP_MAX_TILES_PER_WG = 1 << 20;
static_assert(APP_TILE % (4 * APP_WG) == 0 && APP_BITS == 64, "one wave scans the bitmap's words");
static_assert(APP_MAX_TILES_PER_WG * APP_TILE < (1ll << 32), "an LDS counter cannot wrap");
// status words
constexpr int APP_BAD = 0;   // ids outside [0, BPE_MAX_VOCAB)
constexpr int APP_MAX = 1;   // the largest id + 1
constexpr int APP_WORDS = 2;

// One step of the whole wave: the lanes with `have` count their id.
__device__ __forceinline__ void app_count(bool have, uint32_t id, int lane, uint32_t *s_hist,
                                          unsigned long long *__restrict__ hist) {
    const unsigned long long all = __ballot(have);
    if (!all) return;
    const uint32_t lid = (uint32_t)__builtin_amdgcn_readlane((int)id, __builtin_ctzll(all));
    const unsigned long long same = __ballot(have && id == lid);
    if (same == all) {
        if (lane == __builtin_ctzll(all)) {
            const uint32_t n = (uint32_t)__builtin_popcountll(all);
            if (lid < APP_HOT) atomicAdd(&s_hist[lid], n);
            else atomicAdd(&hist[lid], (unsigned long long)n);
        }
        return;
    }
    if (have && id < APP_HOT) atomicAdd(&s_hist[id], 1u);
    unsigned long long cold = __ballot(have && id >= APP_HOT);
    while (cold) {
        const int lead = __builtin_ctzll(cold);
        const uint32_t cid = (uint32_t)__builtin_amdgcn_readlane((int)id, lead);
        const unsigned long long eq = __ballot(have && id == cid);
        if (lane == lead) atomicAdd(&hist[cid], (unsigned long long)__builtin_popcountll(eq));
        cold &= ~eq;
    }
}

// src: the batch's first token (sample k = src[off[k] - base .. off[k+1] - base), total tokens);
// dst: the corpus at its first free slot, room for total + n slots; dmis: that slot's index mod 4;
// n_tiles tiles cover the slots [-dmis, total + n), per_wg of them per workgroup.
__global__ void __launch_bounds__(APP_WG)
k_smp_append(const int32_t *__restrict__ src, const int64_t *__restrict__ off, int64_t n, int64_t base,
             int64_t total, int dmis, int64_t n_tiles, int64_t per_wg, int32_t sep, int32_t *__restrict__ dst,
             unsigned long long *__restrict__ hist, unsigned long long *__restrict__ st) {
    __shared__ int4 s_stage[APP_TILE / 4 + 2];   // the tile's tokens, from the 16-byte line they start in
    __shared__ uint32_t s_hist[APP_HOT];         // this workgroup's occurrences of the ids below APP_HOT
    __shared__ uint32_t s_bits[APP_BITS];        // slots that hold a separator
    __shared__ int s_pre[APP_BITS + 1];          // separators before each word of the bitmap
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t S = total + n;
    for (int i = tid; i < APP_HOT; i += APP_WG) s_hist[i] = 0;
    const int64_t t_begin = (int64_t)blockIdx.x * per_wg;
    const int64_t t_end = t_begin + per_wg < n_tiles ? t_begin + per_wg : n_tiles;
    // the sample that owns the range's first slot: the last k with g[k] <= that slot (uniform)
    int64_t k_first = 0;
    {
        const int64_t first = t_begin * APP_TILE - dmis;
        const int64_t slot = first < 0 ? 0 : first;
        int64_t lo = 0, hi = n;   // g[lo] <= slot < g[hi]
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (off[mid] - base + mid <= slot) lo = mid;
            else hi = mid;
        }
        k_first = lo;
    }
    unsigned long long bad = 0;
    uint32_t mx = 0;
    const int32_t *stage = reinterpret_cast<const int32_t *>(s_stage);
    for (int64_t tile = t_begin; tile < t_end; ++tile) {
        const int64_t tile0 = tile * APP_TILE - dmis;
        const int64_t slot_lo = tile0 < 0 ? 0 : tile0;
        const int64_t slot_hi = tile0 + APP_TILE < S ? tile0 + APP_TILE : S;
        if (tid < APP_BITS) s_bits[tid] = 0;
        __syncthreads();
        // the samples that end in the tile (sample k's separator is slot g[k+1] - 1)
        for (int64_t k = k_first + tid; k < n; k += APP_WG) {
            const int64_t p = off[k + 1] - base + k;
            if (p >= slot_hi) break;
            if (p < slot_lo) continue;   // (never with increasing offsets; keeps the bitmap's bounds)
            const int b = (int)(p - tile0);
            atomicOr(&s_bits[b >> 5], 1u << (b & 31));
        }
        __syncthreads();
        if (tid < APP_BITS) {   // (the first wave)
            const int c = __builtin_popcount(s_bits[tid]);
            int inc = c;
#pragma unroll
            for (int d = 1; d < APP_BITS; d <<= 1) {
                const int o = __shfl_up(inc, d);
                if (lane >= d) inc += o;
            }
            s_pre[tid] = inc - c;
            if (tid == APP_BITS - 1) s_pre[APP_BITS] = inc;
        }
        __syncthreads();
        const int n_sep = s_pre[APP_BITS];
        // the tile's tokens: tok_lo .. tok_lo + n_tok of the batch, staged from the aligned line below
        const int64_t tok_lo = slot_lo - k_first;
        const int n_tok = (int)(slot_hi - slot_lo) - n_sep;
        const int smis = (int)((((uintptr_t)src >> 2) + (unsigned long long)tok_lo) & 3);
        const int n_quads = (smis + n_tok + 3) >> 2;
        for (int i = tid; i < n_quads; i += APP_WG) {
            const int64_t t0 = tok_lo - smis + 4 * (int64_t)i;
            int4 v;
            if (t0 >= 0 && t0 + 4 <= total) {
                v = *reinterpret_cast<const int4 *>(src + t0);
            } else {
                v.x = t0 >= 0 && t0 < total ? src[t0] : 0;
                v.y = t0 + 1 >= 0 && t0 + 1 < total ? src[t0 + 1] : 0;
                v.z = t0 + 2 >= 0 && t0 + 2 < total ? src[t0 + 2] : 0;
                v.w = t0 + 3 >= 0 && t0 + 3 < total ? src[t0 + 3] : 0;
            }
            s_stage[i] = v;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < APP_GROUPS; ++q) {
            const int b0 = q * 4 * APP_WG + 4 * tid;
            const int64_t r0 = tile0 + b0;
            const uint32_t word = s_bits[b0 >> 5];
            const uint32_t nib = (word >> (b0 & 31)) & 15u;
            // the sample of this lane's first slot
            int64_t k = k_first + s_pre[b0 >> 5] + __builtin_popcount(word & ((1u << (b0 & 31)) - 1u));
            int32_t v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t r = r0 + j;
                const bool is_sep = (nib >> j) & 1;
                const bool tok = r >= slot_lo && r < slot_hi && !is_sep;
                int32_t x = sep;
                if (tok) x = stage[(int)(r - k - tok_lo) + smis];
                v[j] = x;
                const bool have = tok && (uint32_t)x < (uint32_t)BPE_MAX_VOCAB;
                if (tok && !have) ++bad;
                if (have && (uint32_t)x + 1 > mx) mx = (uint32_t)x + 1;
                app_count(have, (uint32_t)x, lane, s_hist, hist);   // (the whole wave takes every step)
                k += is_sep;
            }
            if (r0 >= slot_lo && r0 + 4 <= slot_hi) {
                *reinterpret_cast<int4 *>(dst + r0) = make_int4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (r0 + j >= slot_lo && r0 + j < slot_hi) dst[r0 + j] = v[j];
            }
        }
        k_first += n_sep;
        __syncthreads();   // (the next tile reuses the LDS words)
    }
    for (int i = tid; i < APP_HOT; i += APP_WG) {
        const uint32_t c = s_hist[i];
        if (c) atomicAdd(&hist[i], (unsigned long long)c);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        bad += __shfl_xor(bad, d);
        const uint32_t o = (uint32_t)__shfl_xor((int)mx, d);
        mx = o > mx ? o : mx;
    }
    if (lane == 0) {
        if (bad) atomicAdd(&st[APP_BAD], bad);
        if (mx) atomicMax(&st[APP_MAX], (unsigned long long)mx);
    }
}

}  // namespace
