// bpe_export.hip.h — the kernels of the corpus export (bpe_export_samples, bpe_export_text_batch,
// include/bpe.h "corpus out"): samples out of the chunk layout (chunks of CHUNK slots,
// left-packed, live slots are tokens or SEP at a sample's end) as values back to back, one value per
// token.  Included by bpe_engine.hip after bpe_kernels.hip.h, whose k_census and k_scan_pair give the
// region prefixes (live tokens and separators before every region) both forms start from.
//
//   k_exp_walk   every sample, in corpus order.  The token at live slot j of chunk c is value number
//                (tokens before it) of the output, and separator number k closes sample k at
//                off[k + 1] = (tokens before it): the export of the whole corpus is the compaction
//                of its tokens.  One wave per region, as k_sep_emit: ranks inside a chunk from
//                ballots, the running counts carried from chunk to chunk.  A chunk's values are
//                staged in the wave's own BPE_EXPORT_TILE words of LDS at their ranks and leave as
//                one contiguous run: aligned 16-byte stores (4-byte for codes) with single stores
//                at the run's ends only, so a packed corpus costs about a copy.  The same walk,
//                without values, writes what the selected form needs: every sample's offset and the
//                slot of its separator, and per chunk the tokens before it (8 B per chunk).
//   k_exp_plan   per selected sample: its value count and the chunks its slots touch, both then
//                scanned by k_scan_pair into the output offsets and the prefix of wave items.
//   k_exp_sel    the selected samples.  A wave item is (selected sample, chunk): one uniform binary
//                search in the item prefix finds the sample, the item's rank under it the chunk.
//                The tokens of the sample inside the chunk are those between the separator before
//                the sample and its own; their place in the sample is the chunk's token prefix plus
//                the ballot rank minus the tokens before the sample's start.  Work is cut by
//                chunk, so one sample of 2^30 slots and 10^6 samples of three tokens both spread
//                over the device.  Only the chunks the samples touch are read.
//
// The value of a token id is the id (BPE_EXPORT_IDS), to_vector_index[id] (BPE_EXPORT_VECTORS: a
// gather from the index in global memory, 216 KiB at the most, which the caches hold; it does not fit
// the LDS a workgroup can have beside its stage at full occupancy), or id + 1 narrowed to 16 bits
// (BPE_EXPORT_CODE).  EXP_CHECK writes no value: it looks for tokens that map to a hole and keeps
// the smallest (output position << 16 | id) in st[0], the first failing value in output order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bpe.h"
#include "bpe_kernels.hip.h"

namespace bpe {

constexpr int EXP_WG = 256;
constexpr int EXP_WAVES = EXP_WG / 64;
constexpr int EXP_TILE = BPE_EXPORT_TILE;
static_assert(EXP_TILE == CHUNK, "a wave stages one chunk");
constexpr int EXP_IDS = BPE_EXPORT_IDS, EXP_VEC = BPE_EXPORT_VECTORS, EXP_CODE = BPE_EXPORT_CODE;
constexpr int EXP_NONE = 3;    // no values: offsets, separator slots and chunk prefixes only
constexpr int EXP_CHECK = 4;   // no values: the first token that maps to a hole

// before[e] = the kept slots of the chunk before slot 4 * lane + e; returns the chunk's kept slots.
__device__ __forceinline__ int exp_rank(const bool (&keep)[4], int lane, int (&before)[4]) {
    const unsigned long long below = (1ull << lane) - 1;
    int b = 0, tot = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned long long m = __ballot(keep[e]);
        b += __popcll(m & below);
        tot += __popcll(m);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        before[e] = b;
        b += keep[e];
    }
    return tot;
}

// The kept tokens of one chunk (keep, their ranks in `before`, `tot` of them) go to out[o0 ..
// o0 + tot), never at or past o_end.  stage: this wave's EXP_TILE words of LDS.  (One wave runs its
// LDS accesses in order; the fences keep the compiler from moving them across each other.)
template <int KIND>
__device__ __forceinline__ void exp_emit(const View &w, const bool (&keep)[4], const int (&before)[4], int tot,
                                         int lane, int32_t *stage, const int32_t *__restrict__ map,
                                         int32_t n_index, void *__restrict__ out, int64_t o0, int64_t o_end,
                                         unsigned long long *__restrict__ st) {
    if (KIND == EXP_NONE) return;
    if (KIND == EXP_CHECK) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!keep[e]) continue;
            const int32_t id = w.t[e];
            const bool hole = (uint32_t)id >= (uint32_t)n_index || map[id] < 0;
            if (hole)
                atomicMin(st, ((unsigned long long)(o0 + before[e]) << 16) | (unsigned long long)(id & 0xFFFF));
        }
        return;
    }
    if (o0 + tot > o_end) tot = o_end > o0 ? (int)(o_end - o0) : 0;   // (a layout that lost a separator)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (!keep[e] || before[e] >= tot) continue;
        const int32_t id = w.t[e];
        int32_t v = id;
        if (KIND == EXP_VEC) v = (uint32_t)id < (uint32_t)n_index ? map[id] : -1;
        if (KIND == EXP_CODE) v = id + 1;
        stage[before[e]] = v;
    }
    __threadfence_block();
    if (KIND == EXP_CODE) {
        uint16_t *o = reinterpret_cast<uint16_t *>(out) + o0;
        const int head = tot ? (int)(((uintptr_t)o >> 1) & 1) : 0;   // units before the 4-byte grid
        if (lane == 0 && head) o[0] = (uint16_t)stage[0];
        const int np = (tot - head) >> 1;
        for (int p = lane; p < np; p += 64) {
            const int j = head + 2 * p;
            *reinterpret_cast<uint32_t *>(o + j) = ((uint32_t)stage[j] & 0xFFFFu) | ((uint32_t)stage[j + 1] << 16);
        }
        if (lane == 0 && ((tot - head) & 1)) o[tot - 1] = (uint16_t)stage[tot - 1];
    } else {
        int32_t *o = reinterpret_cast<int32_t *>(out) + o0;
        int head = (int)((4 - (((uintptr_t)o >> 2) & 3)) & 3);   // values before the 16-byte grid
        if (head > tot) head = tot;
        if (lane < head) o[lane] = stage[lane];
        const int nq = (tot - head) >> 2;
        if (lane < nq) {   // (at most EXP_TILE / 4 = 64 groups: one per lane)
            const int j = head + 4 * lane;
            *reinterpret_cast<int4 *>(o + j) = make_int4(stage[j], stage[j + 1], stage[j + 2], stage[j + 3]);
        }
        const int t = head + 4 * nq + lane;
        if (lane < 3 && t < tot) o[t] = stage[t];
    }
    __threadfence_block();
}

// off (n_samples + 1 entries, off[0] is the caller's), slot_end (n_samples) and cpre (n_chunks)
// may each be null.  total: the values the output holds (the corpus's live tokens).
template <int KIND>
__global__ void __launch_bounds__(EXP_WG)
k_exp_walk(const int32_t *__restrict__ ids, int64_t n_chunks, int64_t cpr, int R,
           const int64_t *__restrict__ live_pre, const int64_t *__restrict__ sep_pre, int64_t n_samples,
           int64_t total, const int32_t *__restrict__ map, int32_t n_index, void *__restrict__ out,
           int64_t *__restrict__ off, int64_t *__restrict__ slot_end, int64_t *__restrict__ cpre,
           unsigned long long *__restrict__ st) {
    __shared__ int32_t s_stage[EXP_WAVES][EXP_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * EXP_WAVES + wave;
    if (r >= R) return;
    const int64_t c0 = (int64_t)r * cpr;
    const int64_t c1 = min(c0 + cpr, n_chunks);
    const int4 *v4 = reinterpret_cast<const int4 *>(ids);
    int64_t ol = live_pre[r], os = sep_pre[r];
    for (int64_t c = c0; c < c1; ++c) {
        const View w = make_view(v4[c * 64 + lane]);
        bool T[4], S[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = 4 * lane + e < w.len;
            T[e] = in && w.t[e] >= 0;
            S[e] = in && w.t[e] == SEP;
        }
        int bt[4], bs[4];
        const int tl = exp_rank(T, lane, bt);
        const int ts = exp_rank(S, lane, bs);
        if (cpre && lane == 0) cpre[c] = ol;
        if (off || slot_end) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t k = os + bs[e];
                if (S[e] && k < n_samples) {
                    if (off) off[k + 1] = ol + bt[e];
                    if (slot_end) slot_end[k] = c * CHUNK + 4 * lane + e;
                }
            }
        }
        exp_emit<KIND>(w, T, bt, tl, lane, s_stage[wave], map, n_index, out, ol, total, st);
        ol += tl;
        os += ts;
    }
}

// Sample idx[k] holds len[k] values in nch[k] chunks (none when it is empty); entry n of both is 0,
// so that their exclusive scans (k_scan_pair over n + 1 entries) end in the totals.
// le: n_samples + 1 token offsets of the samples; slot_end: the slots of their separators.
__global__ void __launch_bounds__(256)
k_exp_plan(const int64_t *__restrict__ idx, int64_t n, const int64_t *__restrict__ le,
           const int64_t *__restrict__ slot_end, int64_t *__restrict__ len, int64_t *__restrict__ nch) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > n) return;
    int64_t l = 0, m = 0;
    if (k < n) {
        const int64_t i = idx[k];
        l = le[i + 1] - le[i];
        const int64_t first = i ? slot_end[i - 1] + 1 : 0;
        if (l) m = slot_end[i] / CHUNK - first / CHUNK + 1;
    }
    len[k] = l;
    nch[k] = m;
}

// soff, ipre: the scanned len and nch of k_exp_plan (n + 1 entries each); n_items = ipre[n].
template <int KIND>
__global__ void __launch_bounds__(EXP_WG)
k_exp_sel(const int32_t *__restrict__ ids, const int64_t *__restrict__ idx, int64_t n,
          const int64_t *__restrict__ le, const int64_t *__restrict__ slot_end, const int64_t *__restrict__ cpre,
          const int64_t *__restrict__ soff, const int64_t *__restrict__ ipre, int64_t n_items,
          const int32_t *__restrict__ map, int32_t n_index, void *__restrict__ out,
          unsigned long long *__restrict__ st) {
    __shared__ int32_t s_stage[EXP_WAVES][EXP_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int4 *v4 = reinterpret_cast<const int4 *>(ids);
    for (int64_t item = (int64_t)blockIdx.x * EXP_WAVES + wave; item < n_items;
         item += (int64_t)gridDim.x * EXP_WAVES) {
        // the selected sample of this item: the last k with ipre[k] <= item (uniform; an empty
        // sample shares its prefix with the next one and is never the last)
        int64_t lo = 0, hi = n;   // ipre[lo] <= item < ipre[hi]
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (ipre[mid] <= item) lo = mid;
            else hi = mid;
        }
        const int64_t k = lo, i = idx[k];
        const int64_t first = i ? slot_end[i - 1] + 1 : 0, send = slot_end[i];
        const int64_t c = first / CHUNK + (item - ipre[k]);
        const View w = make_view(v4[c * 64 + lane]);
        bool K[4];
        int n_before = 0;   // the chunk's tokens before the sample's first slot
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t slot = c * CHUNK + 4 * lane + e;
            const bool tok = 4 * lane + e < w.len && w.t[e] >= 0;
            K[e] = tok && slot >= first && slot < send;
            n_before += __popcll(__ballot(tok && slot < first));
        }
        int bk[4];
        const int tot = exp_rank(K, lane, bk);
        const int64_t o0 = soff[k] + (cpre[c] + n_before - le[i]);
        exp_emit<KIND>(w, K, bk, tot, lane, s_stage[wave], map, n_index, out, o0, soff[k + 1], st);
    }
}

}  // namespace bpe
