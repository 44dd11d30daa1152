// bpe_encode.hip — encodeToCode (core.ts:392-409) for many texts at once: a merge-rank encoder
// on the device, behind the bpe_encoder_* / bpe_encode_batch entry
// points of include/bpe.h.
//
// The reference encodes a text by running every merge in order over it:
//     for (let [from_code, to_code] of this.merge_codes)
//       content_in_code = content_in_code.replaceAll(from_code, to_code)        (core.ts:404-406)
// i.e. M sequential leftmost-non-overlapping rewrites.  For a merge list where no merge's new token
// is an input of itself or of an earlier merge (every list findNextMerge / restoreMerge / fromJSON
// of a reference-made JSON produces: c is always a new index, core.ts:315,484), that equals the
// rank-greedy form: repeatedly take the LOWEST-ranked merge whose pair occurs in the text and
// rewrite all of its leftmost non-overlapping occurrences.  Proof sketch: rewriting rank r only
// creates pairs that contain c_r, and every merge taking c_r as input has a rank above r, so ranks
// are taken in increasing order and each one does exactly what its replaceAll does; the ranks the
// greedy skips have no occurrence, where replaceAll is a no-op.  The greedy does work only for
// the merges that fire in this text (at most n - 1 of them), instead of M passes over it.
//
// One workgroup encodes one text held in LDS (u16 token ids + u16 pair ranks, two buffers; ids
// stay below BPE_MAX_VOCAB = 55296).  Per greedy step:
//   1. every thread walks its contiguous segment and flags the counted occurrences of rank r
//      (rule R1 of SURVEY.md Appendix A: for x == y only even offsets inside a run, which needs the
//      run length before the segment: a walk back);
//   2. an exclusive scan of the flag counts gives each segment's destination after the rewrite
//      (position i + 1 of every counted i is deleted);
//   3. the segment is written compacted into the other buffer; only the pairs that now touch c_r
//      are looked up again in the rank table (a hash in HBM, L2-resident: 8 B per merge, load
//      factor <= 1/2), the others keep their rank; the minimum of the written ranks is the next r.
// Two workgroup barriers per step.  Texts longer than an LDS buffer, and merge lists for which the
// greedy would differ, go through the apply-only streaming passes of a scratch engine
// (bpe_apply_merges: the same M replaceAll rewrites, one pass each, all long texts together).
// With BPE_LONG_SPLIT a long text is first cut at boundaries no merge can cross (k_cuts: one wave
// per window of boundaries against the cut set of the list) and its segments are encoded as texts
// are; only a text with a stretch longer than an LDS buffer without such a boundary is replayed.
//
// The text form (bpe_encode_text_batch, at the end of this file) puts bpe_text.hip.h's kernels
// around k_encode: a front end from UTF-16 units to the compact ids and id offsets k_encode reads,
// and a back end that packs its output as vector indices; encodeToVector (core.ts:392-445) of a
// batch then never maps a char or an id on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bpe.h"
#include "bpe_multi.h"   // bpe_fail
#include "bpe_text_front.hip.h"   // wave scans and the text front end shared with the corpus ingest

namespace {

// A pair's rank and the merge's new token in one word, rank << 16 | c: the minimum over a text is
// the next merge together with its c (no dependent load of c), and NO_RANK is above every one.
constexpr uint32_t NO_RANK = 0xFFFFFFFFu;
// tokens per workgroup of each launch shape (LDS: 6 bytes per token, u16 id + u32 rank word)
constexpr int CAP_MAX = 16384;   // 96 KiB (the largest launch shape below)
static_assert(CAP_MAX == BPE_ENCODE_LDS_TOKENS, "include/bpe.h");
constexpr size_t LDS_BYTES = 160 * 1024 - 256;   // per workgroup (the static words aside)

#define ENC_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return bpe_fail(e_ == hipErrorOutOfMemory ? BPE_ERR_OOM : BPE_ERR_HIP,         \
                            (std::string("bpe native: ") + #expr + ": " +                   \
                             hipGetErrorString(e_)).c_str());                              \
    } while (0)

struct RankTab {
    const unsigned long long *slots;   // (a << 16 | b) << 32 | rank << 16 | c; empty = ~0
    uint32_t mask;
    uint32_t shift;                    // 32 - log2(slots)
};

__host__ __device__ __forceinline__ uint32_t rank_home(uint32_t key, uint32_t shift) {
    return (key * 0x9E3779B1u) >> shift;
}

// Wave reductions on the VALU (dpp, wave_incl and block_scan: bpe_text_front.hip.h): DPP row
// rotations inside each 16-lane row, then the four row results through v_readlane.
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    v = min(v, dpp<0x128>(v, v));   // row_ror:8
    v = min(v, dpp<0x124>(v, v));   // row_ror:4
    v = min(v, dpp<0x122>(v, v));   // row_ror:2
    v = min(v, dpp<0x121>(v, v));   // row_ror:1
    const uint32_t a = __builtin_amdgcn_readlane((int)v, 0), b = __builtin_amdgcn_readlane((int)v, 16);
    const uint32_t c = __builtin_amdgcn_readlane((int)v, 32), d = __builtin_amdgcn_readlane((int)v, 48);
    return min(min(a, b), min(c, d));
}

// minimum over the workgroup (one barrier; `m` holds one word per wave)
template <int WG>
__device__ __forceinline__ uint32_t block_min(uint32_t v, uint32_t *m) {
    v = wave_min(v);
    if (WG == 64) return v;
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) m[w] = v;
    __syncthreads();
    uint32_t r = m[0];
#pragma unroll
    for (int i = 1; i < WG / 64; ++i) r = min(r, m[i]);
    return r;
}

// The rank table copied into LDS (the latency form: few texts per call, each on a CU of its own):
// keys[m] u32 (a << 16 | b per rank), cs[m] u16 (c per rank, padded to an even count), slot[S] u32
// (fingerprint << 16 | rank + 1, or 0 = empty; S a power of two >= 2m, linear probing from
// rank_home).  A probe reads one slot; only a fingerprint match reads the key and c (one more LDS
// round).  14 B per merge: 8000 merges take 111 KiB.
struct LdsTab {
    const uint32_t *img;   // the image above in HBM, copied word by word
    uint32_t words;        // its size in u32 words
    uint32_t m;            // merges
    uint32_t mask, shift;  // slot table: S = mask + 1, home = rank_home(key, shift)
};

__host__ __device__ __forceinline__ uint32_t fingerprint(uint32_t key) {
    return (key * 0x85EBCA6Bu) >> 16;
}

template <bool TAB_LDS>
struct Lookup {
    RankTab g;
    const uint32_t *keys, *slot;
    const uint16_t *cs;
    uint32_t mask, shift;
    __device__ __forceinline__ uint32_t operator()(uint32_t key) const {
        if constexpr (!TAB_LDS) {
            uint32_t h = rank_home(key, g.shift);
            for (;;) {
                const unsigned long long e = g.slots[h];
                if ((uint32_t)(e >> 32) == key) return (uint32_t)e;
                if (e == ~0ull) return NO_RANK;
                h = (h + 1) & g.mask;
            }
        } else {
            const uint32_t fp = fingerprint(key);
            uint32_t h = rank_home(key, shift);
            for (;;) {
                const uint32_t e = slot[h];
                if (!e) return NO_RANK;
                if ((e >> 16) == fp) {
                    const uint32_t r = (e & 0xFFFFu) - 1;
                    if (keys[r] == key) return (r << 16) | cs[r];
                }
                h = (h + 1) & mask;
            }
        }
    }
};

// One text per workgroup: which[blockIdx.x] indexes the texts of this launch shape; up to
// WG * (KMAX - 1) tokens, held in LDS as u16 ids + u32 rank words, rewritten in place.  Each greedy step:
//   - every thread loads its segment [s, s + k) (k <= KMAX) plus two tokens of look-ahead and one
//     rank word of look-behind into registers (one batch of LDS reads), and flags the counted
//     occurrences of rank r there (the chain parity comes from the look-behind; a chain crossing
//     into the segment is walked back in LDS, which only x == y runs do);
//   - an exclusive scan of the counts gives the segment's destination (barrier: every read of this
//     step is done before any write);
//   - the segment is written back compacted; the pairs that now touch c get their rank word again,
//     one request per lane per round, so a wave's probes run side by side;
//   - the minimum rank word written is the next step's merge (barrier).
template <int WG, int KMAX, bool TAB_LDS>
__global__ void __launch_bounds__(WG)
k_encode(const int32_t *__restrict__ in, const int64_t *__restrict__ off,
         const int32_t *__restrict__ which, int32_t *__restrict__ out, int32_t *__restrict__ out_len,
         RankTab t, LdsTab lt, unsigned long long *__restrict__ steps_total,
         unsigned long long *__restrict__ err) {
    static_assert(KMAX & 1, "odd segment lengths");
    constexpr int CAP = WG * (KMAX - 1);
    constexpr int H = KMAX + 2;   // segment + look-ahead
    extern __shared__ uint32_t lds32[];
    __shared__ uint32_t red[WG / 64];
    __shared__ int scn[WG / 64];
    uint32_t *rk = lds32;
    uint16_t *tok = reinterpret_cast<uint16_t *>(lds32 + CAP);
    Lookup<TAB_LDS> look;
    look.g = t;
    if constexpr (TAB_LDS) {
        uint32_t *tw = lds32 + CAP + CAP / 2;
        const uint32_t w4 = lt.words & ~3u;
        for (uint32_t w = 4 * threadIdx.x; w < w4; w += 4 * WG)
            *reinterpret_cast<uint4 *>(tw + w) = *reinterpret_cast<const uint4 *>(lt.img + w);
        for (uint32_t w = w4 + threadIdx.x; w < lt.words; w += WG) tw[w] = lt.img[w];
        look.keys = tw;
        look.cs = reinterpret_cast<const uint16_t *>(tw + lt.m);
        look.slot = tw + lt.m + ((lt.m + 1) >> 1);
        look.mask = lt.mask;
        look.shift = lt.shift;
    }

    const int text = which[blockIdx.x];
    const int64_t base = off[text];
    int n = (int)(off[text + 1] - base);
    const int tid = threadIdx.x;

    bool bad = false;
    for (int i = tid; i < n; i += WG) {
        const int32_t v = in[base + i];
        bad |= (uint32_t)v >= (uint32_t)BPE_MAX_VOCAB;
        tok[i] = (uint16_t)v;
    }
    // (an id out of range: counted in *err, the call fails; the text's output is void)
    if (bad) atomicAdd(err, 1ull);
    __syncthreads();
    uint32_t lmin = NO_RANK;
    for (int i = tid; i < n; i += WG) {
        const uint32_t r = i + 1 < n ? look(((uint32_t)tok[i] << 16) | tok[i + 1]) : NO_RANK;
        rk[i] = r;
        lmin = min(lmin, r);
    }
    uint32_t r = block_min<WG>(lmin, red);
    __syncthreads();
    int steps = 0;

    while (r != NO_RANK) {   // (uniform: every thread holds the same r)
        ++steps;
        const uint32_t c = r & 0xFFFFu;
        // segment length: odd, so that lane t's j-th word (t * k + j) falls in a bank of its own
        // (an even stride would put 2..16 lanes on one bank)
        const int k = max(3, (n + WG - 1) / WG) | 1;   // (<= KMAX: n <= WG * (KMAX - 1))
        const int s = tid * k;
        const int len = max(0, min(k, n - s));       // segment [s, s + len)
        uint32_t T[H], R[H];
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const bool in_seg = j < k + 2 && s + j < n;
            T[j] = in_seg ? tok[s + j] : 0u;
            R[j] = in_seg ? rk[s + j] : NO_RANK;
        }
        const uint32_t rb = (len > 0 && s > 0) ? rk[s - 1] : NO_RANK;
        // chain parity at the segment start: d = r-pairs right before s
        int d = 0;
        bool fprev = false;   // is s - 1 counted (s deleted)?
        if (rb == r) {
            for (int j = s - 1; j >= 0 && rk[j] == r; --j) ++d;
            fprev = !((d - 1) & 1);
        }
        uint32_t F = 0;   // counted flags of [s, s + k + 2)
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const bool m = R[j] == r;
            const bool f = m && !(d & 1);
            F |= (uint32_t)f << j;
            cnt += (f && j < len) ? 1 : 0;
            d = m ? d + 1 : 0;
        }
        int total = 0;
        const int before = block_scan<WG>(cnt, scn, total);   // (barrier: all reads done)
        const int p0 = s - before + (fprev ? 1 : 0);
        // live positions of the segment: j is dead when j - 1 is counted
        const uint32_t live = ~((F << 1) | (fprev ? 1u : 0u)) & ((1u << len) - 1u);
        int p = p0;
        lmin = NO_RANK;
        uint32_t K[KMAX];
        uint32_t req = 0;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            K[j] = 0;
            if ((live >> j) & 1) {   // (else: the b of a counted (a, b), or past the segment)
                const bool fi = (F >> j) & 1;
                const uint32_t tv = fi ? c : T[j];
                const int nx = fi ? j + 2 : j + 1;
                uint32_t rv = NO_RANK;
                if (s + nx < n) {
                    const bool fn = (F >> nx) & 1;
                    const uint32_t tn = fi ? T[j + 2] : T[j + 1];
                    if (fi || fn) {
                        K[j] = (tv << 16) | (fn ? c : tn);
                        req |= 1u << j;
                    }
                    rv = R[j];
                }
                tok[p] = (uint16_t)tv;
                if (!((req >> j) & 1)) {
                    rk[p] = rv;
                    lmin = min(lmin, rv);
                }
                ++p;
            }
        }
        // the new pairs' rank words: one request per lane per round (its position: p0 + the live
        // positions before it)
        while (__ballot(req != 0)) {
            if (req) {
                const int j = __builtin_ctz(req);
                uint32_t key = 0;
#pragma unroll
                for (int jj = 0; jj < KMAX; ++jj)
                    if (jj == j) key = K[jj];
                const int pp = p0 + __builtin_popcount(live & ((1u << j) - 1u));
                const uint32_t rv = look(key);
                rk[pp] = rv;
                lmin = min(lmin, rv);
                req &= req - 1;
            }
        }
        n -= total;
        r = block_min<WG>(lmin, red);   // (barrier: the rewritten text visible)
        __syncthreads();
    }

    for (int i = tid; i < n; i += WG) out[base + i] = tok[i];
    if (tid == 0) {
        out_len[text] = n;
        if (steps) atomicAdd(steps_total, (unsigned long long)steps);
    }
}

// launch shapes (WG threads x KMAX tokens each), by text length: the smallest that holds the text,
// so the unrolled segment loops do little masked-off work
constexpr int N_SHAPES = 8;
constexpr int SHAPE_WG[N_SHAPES] = {64, 64, 64, 256, 256, 256, 1024, 1024};
constexpr int SHAPE_K[N_SHAPES] = {3, 5, 9, 5, 9, 17, 9, 17};

constexpr int shape_cap(int i) { return SHAPE_WG[i] * (SHAPE_K[i] - 1); }
constexpr size_t shape_lds(int i) { return (size_t)shape_cap(i) * 6; }
// The packed output of a call on the device: exclusive scan of the encoded lengths (one workgroup,
// 1024 lengths per round) and a gather of every text from its input offset to its output offset
// (one wave per text), so the host copies the result once, with no per-text loop.
// ooff[n + 1] receives the call's bad-id count (*err), so that one copy brings both back.
__global__ void __launch_bounds__(1024)
k_scan_lens(const int32_t *__restrict__ len, int64_t n, int64_t *__restrict__ ooff,
            const unsigned long long *__restrict__ err) {
    __shared__ int scn[16];
    long long carry = 0;
    for (int64_t b = 0; b < n; b += 1024) {
        const int64_t i = b + threadIdx.x;
        const int v = i < n ? len[i] : 0;
        int total = 0;
        const int before = block_scan<1024>(v, scn, total);
        if (i < n) ooff[i] = carry + before;
        carry += total;
        __syncthreads();   // (scn is reused next round)
    }
    if (threadIdx.x == 0) {
        ooff[n] = carry;
        ooff[n + 1] = (long long)*err;
    }
}

// The pack kernels' per-value map: the id itself here, its vector index in bpe_text.hip.h (VecMap).
// `pos` is the value's flat output position.
struct MapId {
    __device__ __forceinline__ int32_t operator()(int32_t id, unsigned long long) const { return id; }
};

// Both in one workgroup, for a call of at most 1024 texts (the one-text-per-call shape): the scan,
// then one wave per text.
template <class Map>
__global__ void __launch_bounds__(1024)
k_pack_small(const int32_t *__restrict__ src, const int64_t *__restrict__ in_off,
             const int32_t *__restrict__ len, int n, int64_t *__restrict__ ooff,
             const unsigned long long *__restrict__ err, int32_t *__restrict__ dst, Map map) {
    __shared__ int scn[16];
    __shared__ int start[1025];
    const int v = (int)threadIdx.x < n ? len[threadIdx.x] : 0;
    int total = 0;
    const int before = block_scan<1024>(v, scn, total);
    if ((int)threadIdx.x < n) {
        start[threadIdx.x] = before;
        ooff[threadIdx.x] = before;
    }
    if (threadIdx.x == 0) {
        ooff[n] = total;
        ooff[n + 1] = (long long)*err;
    }
    __syncthreads();
    for (int t = threadIdx.x >> 6; t < n; t += 16) {
        const int32_t *s = src + in_off[t];
        const int o = start[t];
        int32_t *d = dst + o;
        const int l = len[t];
        for (int i = threadIdx.x & 63; i < l; i += 64) d[i] = map(s[i], (unsigned long long)(o + i));
    }
}

template <class Map>
__global__ void __launch_bounds__(256)
k_gather(const int32_t *__restrict__ src, const int64_t *__restrict__ in_off,
         const int32_t *__restrict__ len, const int64_t *__restrict__ ooff, int64_t n,
         int32_t *__restrict__ dst, Map map) {
    const int64_t text = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (text >= n) return;
    const int32_t *s = src + in_off[text];
    const int64_t o = ooff[text];
    const int l = len[text];
    for (int i = threadIdx.x & 63; i < l; i += 64) dst[o + i] = map(s[i], (unsigned long long)(o + i));
}

// shorter texts take the HBM table even in the few-texts form (the LDS copy costs more than its
// faster probes save over their few steps)
constexpr int LDS_TAB_MIN_TOKENS = 128;

// ---- long texts in segments (BPE_LONG_SPLIT, include/bpe.h) --------------------------------------
// ends[id] = first(id) << 16 | last(id) for the ids below the merges' vocab (an id at or past it
// is its own first and last), and the cut set {last(a) << 16 | first(b)} as an open-addressed u32
// hash (empty = ~0, load factor <= 1/2, home slot rank_home).
constexpr int SPLIT_H = BPE_ENCODE_SPLIT_WINDOW;
static_assert((SPLIT_H & (SPLIT_H - 1)) == 0 && SPLIT_H >= 64 && 2 * SPLIT_H <= CAP_MAX, "include/bpe.h");
constexpr uint32_t CUT_EMPTY = 0xFFFFFFFFu;

struct CutTab {
    const uint32_t *ends;
    uint32_t vocab;
    const uint32_t *slots;
    uint32_t mask, shift;
};

__device__ __forceinline__ long long uniform64(long long v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// One wave per window: win[w] = (lo, hi), the window's boundaries as positions of `ids` (boundary p
// lies between ids[p - 1] and ids[p]; lo <= hi, and both tokens of every boundary belong to the
// window's text).  The wave walks from hi downwards, 64 boundaries per round, lane l testing
// r - l; the first round with a safe boundary ends the walk, and its lowest lane holds the
// largest safe p: cut[w], or -1 when the window has none.  An id outside [0, BPE_MAX_VOCAB) makes
// its boundaries unsafe and indexes nothing (k_encode fails the call for it later).
__global__ void __launch_bounds__(256)
k_cuts(const int32_t *__restrict__ ids, const longlong2 *__restrict__ win, int64_t n_win, CutTab t,
       long long *__restrict__ cut) {
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // (the same in every lane of a wave)
    if (w >= n_win) return;
    const int lane = threadIdx.x & 63;
    const longlong2 lh = win[w];
    const long long lo = uniform64(lh.x), hi = uniform64(lh.y);
    long long found = -1;
    for (long long r = hi; r >= lo; r -= 64) {
        const long long p = r - lane;
        bool safe = false;
        if (p >= lo) {
            const uint32_t x = (uint32_t)ids[p - 1], y = (uint32_t)ids[p];
            if (x < (uint32_t)BPE_MAX_VOCAB && y < (uint32_t)BPE_MAX_VOCAB) {
                const uint32_t lx = x < t.vocab ? t.ends[x] & 0xFFFFu : x;
                const uint32_t fy = y < t.vocab ? t.ends[y] >> 16 : y;
                const uint32_t key = (lx << 16) | fy;
                uint32_t h = rank_home(key, t.shift);
                safe = true;
                for (;;) {
                    const uint32_t e = t.slots[h];
                    if (e == key) safe = false;
                    if (e == key || e == CUT_EMPTY) break;
                    h = (h + 1) & t.mask;
                }
            }
        }
        const unsigned long long b = __ballot(safe);
        if (b) {
            found = r - __builtin_ctzll(b);
            break;
        }
    }
    if (lane == 0) cut[w] = found;
}

// out_off[k] = ooff[seg_of[k]] for k in [0, n]: the texts' packed offsets from their first
// segments' (the device form of a split call)
__global__ void __launch_bounds__(256)
k_text_ooff(const int64_t *__restrict__ ooff, const int64_t *__restrict__ seg_of, int64_t n,
            int64_t *__restrict__ out_off) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k <= n) out_off[k] = ooff[seg_of[k]];
}

}  // namespace

#include "bpe_text.hip.h"   // the text front end and the vector back end (bpe_encode_text_batch)
#include "bpe_utf8.hip.h"   // text as UTF-8: bytes -> units in front of it (bpe_encode_utf8_batch)
#include "bpe_lines.hip.h"  // lines as samples: texts -> samples (bpe_encoder_split_lines)
#include "bpe_skipgram.hip.h"   // skip-gram pairs from the values behind it (bpe_encoder_skipgram)

struct bpe_encoder {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // large calls in groups (encode_groups): copies on cstream, kernels on stream, two slots
    hipStream_t cstream = nullptr;
    hipEvent_t g_in[2] = {nullptr, nullptr}, g_k0[2] = {nullptr, nullptr}, g_k1[2] = {nullptr, nullptr};
    std::vector<int32_t> abc;                 // the merges, in rank order
    bool greedy_ok = true;                    // the rank-greedy form equals the replay (above)
    std::vector<uint8_t> is_input;            // ids used as a or b by the merges so far
    int32_t vocab = 0;                        // 1 + the largest id of the merges
    // rank table (host copy; uploaded when dirty)
    std::vector<unsigned long long> slots;
    uint32_t bits = 0;
    std::vector<uint16_t> c_of;               // rank -> c
    bool dirty = true;
    unsigned long long *d_slots = nullptr;
    size_t d_slots_n = 0;
    // the same merges as the LDS image (LdsTab), for calls of few texts
    std::vector<uint32_t> limg;
    uint32_t *d_limg = nullptr;
    size_t d_limg_n = 0;
    LdsTab lt{};
    unsigned long long *d_steps = nullptr;
    // staging: pinned host and device, grown as needed
    char *h_buf = nullptr, *d_buf = nullptr;
    size_t h_cap = 0, d_cap = 0;
    bpe_ctx *scratch = nullptr;               // the apply-pass route
    int32_t scratch_known = 0;
    bpe_encoder_stats st{};
    bpe_text_state txt;                       // the text form (bpe_encode_text_batch)
    Utf8State u8;                             // text as UTF-8 (bpe_encoder_utf8_to_utf16 and what builds on it)
    Utf8Call u8_pending;                      // a restore's transcode, counted when the restore is done
    LinesState ln;                            // lines as samples (bpe_encoder_split_lines and the restore from lines)
    LinesCall ln_pending;                     // a restore's split, counted when the restore is done
    bool ln_pending_u8 = false;               // ... which had a transcode in front
    SgState sg;                               // skip-gram pairs (bpe_encoder_skipgram and the forms from text)
    // long texts in segments (BPE_LONG_SPLIT): first and last base id of every id (identity until
    // a merge makes it), the ids made so far, and the tables k_cuts reads (built and uploaded
    // with the rank table when dirty)
    int long_mode = BPE_LONG_REPLAY;
    std::vector<uint16_t> first_of, last_of;
    std::vector<uint8_t> is_made;
    bool split_ok = true;                     // greedy_ok, and no id is the c of two merges
    std::vector<uint32_t> ends, cut_slots;
    uint32_t cut_bits = 0;
    uint32_t *d_ends = nullptr, *d_cut_slots = nullptr;
    size_t d_ends_n = 0, d_cut_slots_n = 0;
    longlong2 *d_win = nullptr;               // a call's windows and their cuts
    long long *d_cut = nullptr;
    size_t d_win_n = 0, d_cut_n = 0;
    hipEvent_t ev_p0 = nullptr, ev_p1 = nullptr;
    bpe_split_stats sst{};
};

namespace {

void table_insert(bpe_encoder *E, uint32_t key, uint32_t rank) {
    const uint32_t mask = (1u << E->bits) - 1, shift = 32 - E->bits;
    uint32_t h = rank_home(key, shift);
    for (;;) {
        unsigned long long &s = E->slots[h];
        if (s == ~0ull) {
            s = ((unsigned long long)key << 32) | (rank << 16) | E->c_of[rank];
            return;
        }
        if ((uint32_t)(s >> 32) == key) return;   // a repeated pair: its first rank wins (the
                                                  // later replaceAll finds nothing left)
        h = (h + 1) & mask;
    }
}

void table_rebuild(bpe_encoder *E, uint32_t bits) {
    E->bits = bits;
    E->slots.assign((size_t)1 << bits, ~0ull);
    const int64_t m = (int64_t)E->c_of.size();
    for (int64_t r = 0; r < m; ++r)
        table_insert(E, ((uint32_t)E->abc[3 * r] << 16) | (uint32_t)E->abc[3 * r + 1], (uint32_t)r);
}

template <typename T>
int grow_dev(T **p, size_t *have, size_t want) {
    if (*have >= want) return BPE_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
    const size_t n = std::max<size_t>(want, 1) * 3 / 2 + 64;
    ENC_TRY(hipMalloc((void **)p, n * sizeof(T)));
    *have = n;
    return BPE_OK;
}

// the LDS image of the merges (LdsTab): keys, cs, slots
void build_lds_image(bpe_encoder *E) {
    const uint32_t m = (uint32_t)E->c_of.size();
    uint32_t bits = 1;
    while ((1u << bits) < 2 * m) ++bits;
    const uint32_t S = 1u << bits, m2 = (m + 1) & ~1u;
    E->limg.assign(m + m2 / 2 + S, 0u);
    uint32_t *keys = E->limg.data();
    uint16_t *cs = reinterpret_cast<uint16_t *>(keys + m);
    uint32_t *slot = keys + m + m2 / 2;
    for (uint32_t r = 0; r < m; ++r) {
        const uint32_t key = ((uint32_t)E->abc[3 * r] << 16) | (uint32_t)E->abc[3 * r + 1];
        keys[r] = key;
        cs[r] = E->c_of[r];
        uint32_t h = rank_home(key, 32 - bits);
        while (slot[h] && keys[(slot[h] & 0xFFFFu) - 1] != key) h = (h + 1) & (S - 1);
        if (!slot[h]) slot[h] = (fingerprint(key) << 16) | (r + 1);   // (a repeated pair keeps its first rank)
    }
    E->lt.words = (uint32_t)E->limg.size();
    E->lt.m = m;
    E->lt.mask = S - 1;
    E->lt.shift = 32 - bits;
}

// k_cuts' tables from first_of / last_of (kept by bpe_encoder_add_merges in list order)
void build_split_tables(bpe_encoder *E) {
    const size_t m = E->c_of.size();
    E->ends.resize((size_t)E->vocab);
    for (int32_t i = 0; i < E->vocab; ++i) E->ends[i] = ((uint32_t)E->first_of[i] << 16) | E->last_of[i];
    uint32_t bits = 4;
    while (((size_t)1 << bits) < 2 * m) ++bits;
    E->cut_bits = bits;
    E->cut_slots.assign((size_t)1 << bits, CUT_EMPTY);
    const uint32_t mask = (1u << bits) - 1;
    // (in list order first_of[a] and last_of[b] are final at the merge's turn under greedy_ok,
    // and so they are here; a list that is not split_ok never reads the set)
    for (size_t r = 0; r < m; ++r) {
        const uint32_t key = ((uint32_t)E->last_of[E->abc[3 * r]] << 16) | E->first_of[E->abc[3 * r + 1]];
        uint32_t h = rank_home(key, 32 - bits);
        while (E->cut_slots[h] != CUT_EMPTY && E->cut_slots[h] != key) h = (h + 1) & mask;
        E->cut_slots[h] = key;
    }
}

int upload_table(bpe_encoder *E) {
    if (!E->dirty) return BPE_OK;
    int rc;
    build_split_tables(E);
    if ((rc = grow_dev(&E->d_ends, &E->d_ends_n, E->ends.size())) ||
        (rc = grow_dev(&E->d_cut_slots, &E->d_cut_slots_n, E->cut_slots.size())))
        return rc;
    if (!E->ends.empty())
        ENC_TRY(hipMemcpyAsync(E->d_ends, E->ends.data(), E->ends.size() * 4, hipMemcpyHostToDevice, E->stream));
    ENC_TRY(hipMemcpyAsync(E->d_cut_slots, E->cut_slots.data(), E->cut_slots.size() * 4, hipMemcpyHostToDevice,
                           E->stream));
    if ((rc = grow_dev(&E->d_slots, &E->d_slots_n, E->slots.size()))) return rc;
    ENC_TRY(hipMemcpyAsync(E->d_slots, E->slots.data(), E->slots.size() * 8, hipMemcpyHostToDevice,
                           E->stream));
    build_lds_image(E);
    if ((rc = grow_dev(&E->d_limg, &E->d_limg_n, E->limg.size()))) return rc;
    ENC_TRY(hipMemcpyAsync(E->d_limg, E->limg.data(), E->limg.size() * 4, hipMemcpyHostToDevice,
                           E->stream));
    E->lt.img = E->d_limg;
    E->dirty = false;
    return BPE_OK;
}

// calls of at most this many id bytes go through the pinned staging buffer both ways
constexpr size_t SMALL_CALL_BYTES = 4u << 20;

// texts per call up to which each gets a CU of its own, so the LDS copy of the table pays
constexpr size_t LATENCY_TEXTS = 256;

template <int I, bool TAB_LDS>
hipError_t set_lds_attr() {
    return hipFuncSetAttribute((const void *)k_encode<SHAPE_WG[I], SHAPE_K[I], TAB_LDS>,
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(TAB_LDS ? LDS_BYTES : shape_lds(I)));
}

template <int I>
hipError_t set_lds_attrs() {
    hipError_t e = set_lds_attr<I, true>();
    if (e == hipSuccess) e = set_lds_attr<I, false>();
    if constexpr (I + 1 < N_SHAPES) {
        if (e == hipSuccess) e = set_lds_attrs<I + 1>();
    }
    return e;
}

template <int I>
void launch_one(bpe_encoder *E, unsigned n, bool tab_lds, const int32_t *ids, const int64_t *off,
                const int32_t *which, int32_t *out, int32_t *len, unsigned long long *err) {
    constexpr int WG = SHAPE_WG[I], KM = SHAPE_K[I];
    const RankTab t{E->d_slots, (1u << E->bits) - 1, 32 - E->bits};
    if (tab_lds)
        k_encode<WG, KM, true><<<n, WG, shape_lds(I) + (size_t)E->lt.words * 4, E->stream>>>(
            ids, off, which, out, len, t, E->lt, E->d_steps, err);
    else
        k_encode<WG, KM, false><<<n, WG, shape_lds(I), E->stream>>>(ids, off, which, out, len, t,
                                                                    E->lt, E->d_steps, err);
}

template <int I = 0>
void launch_shape(int i, bpe_encoder *E, unsigned n, bool tab_lds, const int32_t *ids,
                  const int64_t *off, const int32_t *which, int32_t *out, int32_t *len,
                  unsigned long long *err) {
    if (i == I) return launch_one<I>(E, n, tab_lds, ids, off, which, out, len, err);
    if constexpr (I + 1 < N_SHAPES)
        launch_shape<I + 1>(i, E, n, tab_lds, ids, off, which, out, len, err);
}

// Staging buffers of a call: h_bytes of pinned host memory and d_bytes of device memory.  The
// pinned buffer holds only what a call stages through the host (a large call's ids go straight
// from and to the caller's buffers), and one larger than PINNED_KEEP is released at the end of
// the call that needed it (release_stage), so a rare huge call does not pin host memory for the
// encoder's lifetime.
constexpr size_t PINNED_KEEP = size_t(64) << 20;

int grow_stage(bpe_encoder *E, size_t h_bytes, size_t d_bytes) {
    if (E->h_cap < h_bytes) {
        if (E->h_buf) (void)hipHostFree(E->h_buf);
        E->h_buf = nullptr;
        E->h_cap = 0;
        const size_t n = h_bytes * 3 / 2 + 4096;
        ENC_TRY(hipHostMalloc((void **)&E->h_buf, n, hipHostMallocDefault));
        E->h_cap = n;
    }
    if (E->d_cap < d_bytes) {
        if (E->d_buf) (void)hipFree(E->d_buf);
        E->d_buf = nullptr;
        E->d_cap = 0;
        const size_t n = d_bytes * 3 / 2 + 4096;
        ENC_TRY(hipMalloc((void **)&E->d_buf, n));
        E->d_cap = n;
    }
    return BPE_OK;
}

void release_stage(bpe_encoder *E) {
    if (E->h_cap > PINNED_KEEP) {
        // (an early error return may leave a copy from it in flight)
        (void)hipStreamSynchronize(E->stream);
        (void)hipStreamSynchronize(E->cstream);
        (void)hipHostFree(E->h_buf);
        E->h_buf = nullptr;
        E->h_cap = 0;
    }
}

struct Release {
    bpe_encoder *e;
    ~Release() { release_stage(e); }
};

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// ---- the pieces every form of the encoder is made of ----------------------------

// The device staging of one call, or of one slot of a grouped call, sized for n texts of `total`
// ids together:
//     [ooff (n+2) | ids, then the packed output | off (n+2) | which | out | len]
// err, the bad-id counter of k_encode, is word n + 1 of `off`: the id forms zero it through the
// upload of the offsets (rel_offsets), the text form through a memset, because there k_txt_map
// writes the offsets.  The pack kernels copy it to ooff[n + 1], so one copy brings the packed
// offsets and it back (fetch_ooff).  The order [ooff | ids | off | which] is what lets a small id
// call move [ids | off | which] up and [ooff | packed ids] down in one copy each through a pinned
// mirror of the same sizes.  place() returns the end: a form's own regions go there.
struct Stage {
    size_t b_off, b_ids, b_which;   // region sizes in bytes; len is sized like which
    int64_t *ooff = nullptr, *off = nullptr;
    int32_t *ids = nullptr, *which = nullptr, *out = nullptr, *len = nullptr;
    unsigned long long *err = nullptr;
    Stage(int64_t n, int64_t total)
        : b_off(align16((size_t)(n + 2) * 8)), b_ids(align16((size_t)std::max<int64_t>(total, 1) * 4)),
          b_which(align16((size_t)n * 4)) {}
    size_t bytes() const { return 2 * (b_off + b_ids + b_which); }
    // at `d`, for a call of n texts (at most the n it was sized for)
    char *place(char *d, int64_t n) {
        ooff = reinterpret_cast<int64_t *>(d);
        ids = reinterpret_cast<int32_t *>(d += b_off);
        off = reinterpret_cast<int64_t *>(d += b_ids);
        which = reinterpret_cast<int32_t *>(d += b_off);
        out = reinterpret_cast<int32_t *>(d += b_which);
        len = reinterpret_cast<int32_t *>(d += b_ids);
        err = reinterpret_cast<unsigned long long *>(off + n + 1);
        return d + b_which;
    }
};

// the host copy of Stage::off: offsets relative to the first text's, and the zeroed err word
void rel_offsets(int64_t *h_off, const int64_t *off, int64_t n) {
    for (int64_t k = 0; k <= n; ++k) h_off[k] = off[k] - off[0];
    h_off[n + 1] = 0;
}

// The texts of a call by launch shape (the smallest that holds the text), in the order of `which`.
struct ShapeLists {
    std::vector<int32_t> of[N_SHAPES];
    int64_t n = 0;   // texts listed
};

// Can k_encode take a text of l tokens?  Not one longer than an LDS buffer, and none under a merge
// list the greedy would get wrong: those are replayed.
bool kernel_takes(const bpe_encoder *E, int64_t l) { return E->greedy_ok && l <= CAP_MAX; }

// Text k of [0, n) by its length off[k + 1] - off[k] (an upper bound will do): into its shape's
// list, or into `replay`.  What a replayed text means for the call is the form's decision.
void classify(const bpe_encoder *E, const int64_t *off, int64_t n, ShapeLists &lists,
              std::vector<int64_t> &replay) {
    for (int64_t k = 0; k < n; ++k) {
        const int64_t l = off[k + 1] - off[k];
        if (!kernel_takes(E, l)) {
            replay.push_back(k);
        } else {
            int i = 0;
            while (shape_cap(i) < l) ++i;
            lists.of[i].push_back((int32_t)k);
            ++lists.n;
        }
    }
}

void fill_which(const ShapeLists &lists, int32_t *h_which) {
    for (auto &v : lists.of) {
        std::memcpy(h_which, v.data(), v.size() * 4);
        h_which += v.size();
    }
}

// k_encode over every listed text (L.which uploaded from fill_which), one launch per shape in use,
// between the events `before` and `after` (either may be null).  may_few: a call of few texts gives
// each a CU to itself, and the table is read from LDS where it fits beside the text.
int launch_lists(bpe_encoder *E, const ShapeLists &lists, bool may_few, const Stage &L, hipEvent_t before,
                 hipEvent_t after) {
    const size_t tab = (size_t)E->lt.words * 4;
    const bool few = may_few && (size_t)lists.n <= LATENCY_TEXTS;
    if (before) ENC_TRY(hipEventRecord(before, E->stream));
    size_t at = 0;
    for (int i = 0; i < N_SHAPES; ++i) {
        if (lists.of[i].empty()) continue;
        const bool tab_lds = few && shape_cap(i) > LDS_TAB_MIN_TOKENS && shape_lds(i) + tab <= LDS_BYTES;
        launch_shape(i, E, (unsigned)lists.of[i].size(), tab_lds, L.ids, L.off, L.which + at, L.out, L.len, L.err);
        at += lists.of[i].size();
    }
    ENC_TRY(hipGetLastError());
    if (after) ENC_TRY(hipEventRecord(after, E->stream));
    return BPE_OK;
}

// The call's output packed on the device, into the ids region (read by k_encode, free now), every
// value through `map` (MapId, or the text form's VecMap): the scan of the lengths, then the gather.
template <class Map>
int pack_gather(hipStream_t s, const Stage &L, int64_t n, Map map) {
    k_scan_lens<<<1, 1024, 0, s>>>(L.len, n, L.ooff, L.err);
    k_gather<<<(unsigned)((n + 3) / 4), 256, 0, s>>>(L.out, L.off, L.len, L.ooff, n, L.ids, map);
    ENC_TRY(hipGetLastError());
    return BPE_OK;
}

// ... or, for a call one workgroup can copy, both in one launch
template <class Map>
int pack(hipStream_t s, const Stage &L, int64_t n, int64_t total, Map map) {
    if (n > 1024 || total > (1 << 18)) return pack_gather(s, L, n, map);
    k_pack_small<<<1, 1024, 0, s>>>(L.out, L.off, L.len, (int)n, L.ooff, L.err, L.ids, map);
    ENC_TRY(hipGetLastError());
    return BPE_OK;
}

// [ooff (n+1) | bad-id word] of a packed call into the pinned h_ooff, waited for; a count in the
// bad-id word fails the call with the form's own error.  more: bytes of the region after ooff (the
// packed ids) that come with it, for a mirror laid out like the stage and a stage sized for n.
int fetch_ooff(hipStream_t s, const Stage &L, int64_t *h_ooff, int64_t n, size_t more, int bad_rc,
               const char *bad_msg) {
    ENC_TRY(hipMemcpyAsync(h_ooff, L.ooff, align16((size_t)(n + 2) * 8) + more, hipMemcpyDeviceToHost, s));
    ENC_TRY(hipStreamSynchronize(s));
    if (h_ooff[n + 1]) return bpe_fail(bad_rc, bad_msg);
    return BPE_OK;
}

// the packed length of n texts of `total` ids in: checked, and against the caller's capacity
// where there is one (cap >= 0)
int packed_length(const int64_t *h_ooff, int64_t n, int64_t total, int64_t cap, int64_t *n_out) {
    *n_out = h_ooff[n];
    if (*n_out < 0 || *n_out > total) return bpe_fail(BPE_ERR_STATE, "bpe native: bad packed length");
    if (cap >= 0 && *n_out > cap) {
        char msg[128];
        std::snprintf(msg, sizeof msg, "bpe native: encode needs %lld values, the buffer holds %lld",
                      (long long)*n_out, (long long)cap);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    return BPE_OK;
}

// the packed values to the caller's host or device buffer (and everything before it on s done)
int copy_packed(hipStream_t s, int32_t *dst, const int32_t *src, int64_t n_out, hipMemcpyKind kind) {
    if (n_out) ENC_TRY(hipMemcpyAsync(dst, src, (size_t)n_out * 4, kind, s));
    ENC_TRY(hipStreamSynchronize(s));
    return BPE_OK;
}

constexpr const char *BAD_ID = "bpe native: token id out of range in text";

// the apply-pass route: every listed text as one sample of the scratch engine, all M merges
// replayed over them (one streaming pass per merge), the results back into out at the texts'
// own offsets (rel: offsets relative to off[0]) and their lengths into len
int encode_replay(bpe_encoder *E, const int32_t *ids, const int64_t *off, const std::vector<int64_t> &list,
                  int32_t *out, int64_t *len) {
    if (list.empty()) return BPE_OK;
    int rc;
    if (!E->scratch) {
        if ((rc = bpe_create(&E->scratch, E->device))) return rc;
        E->scratch_known = 0;
    }
    struct Clear {
        bpe_ctx *c;
        ~Clear() { bpe_clear_corpus(c); }
    } clear{E->scratch};
    if ((rc = bpe_clear_corpus(E->scratch))) return rc;
    int32_t vocab = E->vocab;
    for (int64_t k : list)
        for (int64_t i = off[k]; i < off[k + 1]; ++i) vocab = std::max(vocab, ids[i] + 1);
    // lengths only matter to the max_length filter of a find, which never runs here
    for (int32_t i = E->scratch_known; i < vocab; ++i)
        if ((rc = bpe_set_token_len16(E->scratch, i, 1))) return rc;
    E->scratch_known = std::max(E->scratch_known, vocab);
    for (int64_t k : list)
        if ((rc = bpe_add_sample(E->scratch, ids + off[k], off[k + 1] - off[k]))) return rc;
    const int64_t m = (int64_t)E->abc.size() / 3;
    if (m && (rc = bpe_apply_merges(E->scratch, E->abc.data(), m, nullptr, 0))) return rc;
    int64_t ns = 0, nt = 0;
    if ((rc = bpe_corpus_size(E->scratch, &ns, &nt))) return rc;
    std::vector<int32_t> got((size_t)std::max<int64_t>(nt, 1));
    std::vector<int64_t> goff((size_t)ns + 1);
    if ((rc = bpe_read_corpus(E->scratch, got.data(), (int64_t)got.size(), goff.data(), ns + 1))) return rc;
    for (size_t j = 0; j < list.size(); ++j) {
        const int64_t k = list[j], l = goff[j + 1] - goff[j];
        std::memcpy(out + (off[k] - off[0]), got.data() + goff[j], (size_t)l * 4);
        len[k] = l;
    }
    E->st.texts_replay += (int64_t)list.size();
    return BPE_OK;
}

// ---- long texts in segments (BPE_LONG_SPLIT) ------------------------------------

// The segments of a call: the texts no longer than CAP_MAX and the replayed ones are one segment
// each, a split text is the segments between its cuts.  Texts lie back to back in the stage's ids,
// so segments do too: seg_off is Stage::off of the segments.
struct SplitPlan {
    std::vector<int64_t> seg_off;    // n_seg + 1 positions in the stage's ids
    std::vector<int64_t> seg_of;     // n_texts + 1: each text's first segment (the last entry: n_seg)
    std::vector<int64_t> fallback;   // the long texts with a stretch over CAP_MAX between cuts, ascending
    bpe_split_stats st{};            // the call's counts: added to the encoder's by the form that
                                     // goes on with the plan (split_commit)
    int64_t n_seg() const { return (int64_t)seg_off.size() - 1; }
};

bool split_route(const bpe_encoder *E) {
    return E->long_mode == BPE_LONG_SPLIT && E->greedy_ok && E->split_ok;
}

// at most this many segments come out of n texts of these lengths (an upper bound will do)
int64_t max_segments(const int64_t *off, int64_t n) {
    int64_t s = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t l = off[k + 1] - off[k];
        s += l > CAP_MAX ? (l - 2) / SPLIT_H + 2 : 1;   // (a cut per window)
    }
    return s;
}

void split_commit(bpe_encoder *E, const SplitPlan &P) {
    if (!P.st.windows) return;
    E->sst.calls++;
    E->sst.texts_split += P.st.texts_split;
    E->sst.texts_fallback += P.st.texts_fallback;
    E->sst.windows += P.st.windows;
    E->sst.segments += P.st.segments;
    E->sst.plan_ms += P.st.plan_ms;
}

// The plan of n texts whose ids are on the device at d_ids, text k at [off[k] - off[0],
// off[k + 1] - off[0]) (off on the host): k_cuts over the windows of every text longer than
// CAP_MAX, the cuts back (8 B per window), and the segments from them.  Waits for the stream.
int plan_split(bpe_encoder *E, const int32_t *d_ids, const int64_t *off, int64_t n, SplitPlan &P) {
    const int64_t base = off[0];
    std::vector<longlong2> win;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t l = off[k + 1] - off[k], t0 = off[k] - base;
        if (l <= CAP_MAX) continue;
        for (int64_t lo = 1; lo <= l - 1; lo += SPLIT_H) {
            longlong2 w;
            w.x = t0 + lo;
            w.y = t0 + std::min<int64_t>(lo + SPLIT_H - 1, l - 1);
            win.push_back(w);
        }
    }
    const int64_t n_win = (int64_t)win.size();
    std::vector<long long> cut((size_t)n_win);
    if (n_win) {
        if (n_win > (int64_t)0x7FFFFFFF) return bpe_fail(BPE_ERR_ARG, "bpe native: encode batch too large");
        int rc;
        if ((rc = grow_dev(&E->d_win, &E->d_win_n, (size_t)n_win)) ||
            (rc = grow_dev(&E->d_cut, &E->d_cut_n, (size_t)n_win)))
            return rc;
        ENC_TRY(hipMemcpyAsync(E->d_win, win.data(), (size_t)n_win * 16, hipMemcpyHostToDevice, E->stream));
        const CutTab t{E->d_ends, (uint32_t)E->vocab, E->d_cut_slots, (1u << E->cut_bits) - 1, 32 - E->cut_bits};
        ENC_TRY(hipEventRecord(E->ev_p0, E->stream));
        k_cuts<<<(unsigned)((n_win + 3) / 4), 256, 0, E->stream>>>(d_ids, E->d_win, n_win, t, E->d_cut);
        ENC_TRY(hipGetLastError());
        ENC_TRY(hipEventRecord(E->ev_p1, E->stream));
        ENC_TRY(hipMemcpyAsync(cut.data(), E->d_cut, (size_t)n_win * 8, hipMemcpyDeviceToHost, E->stream));
        ENC_TRY(hipStreamSynchronize(E->stream));
        float ms = 0;
        ENC_TRY(hipEventElapsedTime(&ms, E->ev_p0, E->ev_p1));
        P.st.plan_ms = ms;
        P.st.windows = n_win;
    }
    P.seg_off.clear();
    P.seg_of.assign((size_t)n + 1, 0);
    int64_t wi = 0;
    std::vector<int64_t> cuts;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t l = off[k + 1] - off[k], t0 = off[k] - base;
        P.seg_of[(size_t)k] = (int64_t)P.seg_off.size();
        P.seg_off.push_back(t0);
        if (l <= CAP_MAX) continue;
        cuts.clear();
        int64_t prev = t0;
        bool ok = true;
        for (int64_t lo = 1; lo <= l - 1; lo += SPLIT_H, ++wi) {
            const int64_t c = cut[(size_t)wi];
            if (c < 0) continue;
            if (c < win[(size_t)wi].x || c > win[(size_t)wi].y)
                return bpe_fail(BPE_ERR_STATE, "bpe native: cut outside its window");
            ok &= c - prev <= CAP_MAX;
            cuts.push_back(c);
            prev = c;
        }
        ok &= t0 + l - prev <= CAP_MAX;
        if (ok) {
            P.seg_off.insert(P.seg_off.end(), cuts.begin(), cuts.end());
            P.st.texts_split++;
            P.st.segments += (int64_t)cuts.size() + 1;
        } else {
            P.fallback.push_back(k);
            P.st.texts_fallback++;
        }
    }
    P.seg_of[(size_t)n] = (int64_t)P.seg_off.size();
    P.seg_off.push_back(off[n] - base);
    return BPE_OK;
}

// The id form of a call with long texts on the split route: the ids go up, the plan is made on
// them, and the kernels and the pack run over segments as they do over texts.  Texts that fall
// back make the call take the host assembly, as a replayed text does on the default route.
int encode_ids_split(bpe_encoder *E, const int32_t *ids, const int64_t *off, int64_t n_texts, int32_t *ids_out,
                     int64_t *out_off) {
    const int64_t base = off[0], total = off[n_texts] - base;
    int rc;
    if ((rc = upload_table(E))) return rc;
    const int64_t n_max = max_segments(off, n_texts);
    if (n_max >= 0x7FFFFFFF) return bpe_fail(BPE_ERR_ARG, "bpe native: encode batch too large");
    Stage L(n_max, total);
    // pinned: [ooff | off | which], sized for n_max segments
    if ((rc = grow_stage(E, 2 * L.b_off + L.b_which, L.bytes()))) return rc;
    Release release{E};
    L.place(E->d_buf, n_max);
    ENC_TRY(hipMemcpyAsync(L.ids, ids + base, (size_t)total * 4, hipMemcpyHostToDevice, E->stream));
    SplitPlan P;
    if ((rc = plan_split(E, L.ids, off, n_texts, P))) return rc;
    split_commit(E, P);
    const int64_t n_seg = P.n_seg();
    L.place(E->d_buf, n_seg);   // (the err word follows the segments' offsets)
    for (int64_t k : P.fallback)
        for (int64_t i = off[k]; i < off[k + 1]; ++i)
            if (ids[i] < 0 || ids[i] >= BPE_MAX_VOCAB) return bpe_fail(BPE_ERR_VOCAB, BAD_ID);
    int64_t *h_ooff = reinterpret_cast<int64_t *>(E->h_buf);
    int64_t *h_off = reinterpret_cast<int64_t *>(E->h_buf + L.b_off);
    int32_t *h_which = reinterpret_cast<int32_t *>(E->h_buf + 2 * L.b_off);
    std::memcpy(h_off, P.seg_off.data(), (size_t)(n_seg + 1) * 8);
    h_off[n_seg + 1] = 0;
    ShapeLists lists;
    std::vector<int64_t> whole;   // (the replayed texts' segments: one each)
    classify(E, h_off, n_seg, lists, whole);
    if (whole.size() != P.fallback.size()) return bpe_fail(BPE_ERR_STATE, "bpe native: split plan mismatch");
    fill_which(lists, h_which);
    ENC_TRY(hipMemcpyAsync(L.off, h_off, L.b_off + (size_t)lists.n * 4, hipMemcpyHostToDevice, E->stream));
    if (!whole.empty()) ENC_TRY(hipMemsetAsync(L.len, 0, (size_t)n_seg * 4, E->stream));
    if ((rc = launch_lists(E, lists, true, L, E->ev0, E->ev1))) return rc;
    if (P.fallback.empty()) {
        int64_t n_out = 0;
        if ((rc = pack(E->stream, L, n_seg, total, MapId{})) ||
            (rc = fetch_ooff(E->stream, L, h_ooff, n_seg, 0, BPE_ERR_VOCAB, BAD_ID)) ||
            (rc = packed_length(h_ooff, n_seg, total, -1, &n_out)) ||
            (rc = copy_packed(E->stream, ids_out, L.ids, n_out, hipMemcpyDeviceToHost)))
            return rc;
        for (int64_t k = 0; k <= n_texts; ++k) out_off[k] = h_ooff[P.seg_of[(size_t)k]];
    } else {
        std::vector<int64_t> tlen((size_t)n_texts, 0);
        std::vector<int32_t> out((size_t)std::max<int64_t>(total, 1));
        std::vector<int32_t> lens((size_t)n_seg);
        unsigned long long err = 0;
        ENC_TRY(hipMemcpyAsync(out.data(), L.out, (size_t)total * 4, hipMemcpyDeviceToHost, E->stream));
        ENC_TRY(hipMemcpyAsync(lens.data(), L.len, (size_t)n_seg * 4, hipMemcpyDeviceToHost, E->stream));
        ENC_TRY(hipMemcpyAsync(&err, L.err, 8, hipMemcpyDeviceToHost, E->stream));
        ENC_TRY(hipStreamSynchronize(E->stream));
        if (err) return bpe_fail(BPE_ERR_VOCAB, BAD_ID);
        if ((rc = encode_replay(E, ids, off, P.fallback, out.data(), tlen.data()))) return rc;
        int64_t o = 0;
        size_t fi = 0;
        out_off[0] = 0;
        for (int64_t k = 0; k < n_texts; ++k) {
            if (fi < P.fallback.size() && P.fallback[fi] == k) {
                ++fi;
                if (tlen[(size_t)k]) std::memcpy(ids_out + o, out.data() + (off[k] - base), (size_t)tlen[(size_t)k] * 4);
                o += tlen[(size_t)k];
            } else {
                for (int64_t g = P.seg_of[(size_t)k]; g < P.seg_of[(size_t)k + 1]; ++g) {
                    if (lens[(size_t)g]) std::memcpy(ids_out + o, out.data() + P.seg_off[(size_t)g], (size_t)lens[(size_t)g] * 4);
                    o += lens[(size_t)g];
                }
            }
            out_off[k + 1] = o;
        }
    }
    float ms = 0;
    ENC_TRY(hipEventElapsedTime(&ms, E->ev0, E->ev1));
    E->st.kernel_ms += ms;
    E->st.texts_rank += n_texts - (int64_t)P.fallback.size();
    E->st.tokens_out += out_off[n_texts];
    return BPE_OK;
}

// A large call (at least 2 x GROUP_TOKENS input tokens) whose texts all take the kernels, in a few
// groups (BPE_ENCODE_GROUPS, default 3) through two slots: the copy stream takes group g's ids up (a pageable copy: the host waits for
// it) while the kernel stream encodes group g - 1, and group g - 1's packed ids come down while
// group g encodes.  Each group is packed on its own; its ids land after the previous groups'.
constexpr int64_t GROUP_TOKENS = int64_t(1) << 23;

int encode_groups_run(bpe_encoder *E, const int32_t *ids, const int64_t *off, int64_t n_texts,
                      int32_t *ids_out, int64_t *out_off) {
    // contiguous text ranges [g0, g1) of >= GROUP_TOKENS tokens (the last one whatever is left)
    // (few groups: each group's longest texts finish alone, so more groups cost kernel time)
    static const int64_t n_groups = [] {
        const char *v = getenv("BPE_ENCODE_GROUPS");
        return v && atoi(v) >= 2 ? (int64_t)atoi(v) : (int64_t)3;
    }();
    const int64_t gt = std::max<int64_t>(GROUP_TOKENS / 2,
                                          (off[n_texts] - off[0] + n_groups - 1) / n_groups);
    std::vector<int64_t> cut{0};
    for (int64_t k = 0; k < n_texts; ++k)
        if (off[k + 1] - off[cut.back()] >= gt && k + 1 < n_texts) cut.push_back(k + 1);
    cut.push_back(n_texts);
    const int ng = (int)cut.size() - 1;
    int64_t max_t = 0, max_n = 0;
    for (int g = 0; g < ng; ++g) {
        max_t = std::max(max_t, off[cut[g + 1]] - off[cut[g]]);
        max_n = std::max(max_n, cut[g + 1] - cut[g]);
    }
    // per slot, device: a Stage for the largest group; pinned: [ooff | off | which] of its sizes
    Stage slot[2] = {Stage(max_n, max_t), Stage(max_n, max_t)};
    const size_t slot_d = slot[0].bytes(), b_off = slot[0].b_off, slot_h = 2 * b_off + slot[0].b_which;
    int rc;
    if ((rc = grow_stage(E, 2 * slot_h, 2 * slot_d))) return rc;
    hipStream_t ks = E->stream, cs = E->cstream;
    int64_t base = 0;
    out_off[0] = 0;
    int64_t n_checked = 0;
    // group g's texts come back: its offsets (small, pinned), then its packed ids
    auto finish = [&](int g) -> int {
        const int sl = g & 1;
        const int64_t k0 = cut[g], n = cut[g + 1] - k0;
        int64_t *h_ooff = reinterpret_cast<int64_t *>(E->h_buf + sl * slot_h);
        int64_t n_out = 0;
        int rc;
        ENC_TRY(hipStreamWaitEvent(cs, E->g_k1[sl], 0));
        if ((rc = fetch_ooff(cs, slot[sl], h_ooff, n, 0, BPE_ERR_VOCAB, BAD_ID)) ||
            (rc = packed_length(h_ooff, n, off[cut[g + 1]] - off[k0], -1, &n_out)) ||
            (rc = copy_packed(cs, ids_out + base, slot[sl].ids, n_out, hipMemcpyDeviceToHost)))
            return rc;
        for (int64_t k = 1; k <= n; ++k) out_off[k0 + k] = base + h_ooff[k];
        base += n_out;
        float ms = 0;
        ENC_TRY(hipEventElapsedTime(&ms, E->g_k0[sl], E->g_k1[sl]));
        E->st.kernel_ms += ms;
        n_checked = cut[g + 1];
        return BPE_OK;
    };
    for (int g = 0; g < ng; ++g) {
        const int sl = g & 1;
        const int64_t k0 = cut[g], n = cut[g + 1] - k0, t0 = off[k0], tn = off[cut[g + 1]] - t0;
        Stage &L = slot[sl];
        L.place(E->d_buf + sl * slot_d, n);
        int64_t *h_off = reinterpret_cast<int64_t *>(E->h_buf + sl * slot_h + b_off);
        int32_t *h_which = reinterpret_cast<int32_t *>(E->h_buf + sl * slot_h + 2 * b_off);
        // (slot sl's pinned staging was last read by group g - 2's upload, complete by now: its
        // kernels, which waited for it, were waited for by finish(g - 2))
        rel_offsets(h_off, off + k0, n);
        ShapeLists lists;
        std::vector<int64_t> none;   // (the caller has seen that no text is replayed)
        classify(E, off + k0, n, lists, none);
        fill_which(lists, h_which);
        ENC_TRY(hipMemcpyAsync(L.ids, ids + t0, (size_t)tn * 4, hipMemcpyHostToDevice, cs));
        ENC_TRY(hipMemcpyAsync(L.off, h_off, b_off + (size_t)n * 4, hipMemcpyHostToDevice, cs));
        ENC_TRY(hipEventRecord(E->g_in[sl], cs));
        ENC_TRY(hipStreamWaitEvent(ks, E->g_in[sl], 0));
        // (not few: a group of GROUP_TOKENS / 2 tokens or more is hundreds of texts)
        if ((rc = launch_lists(E, lists, false, L, E->g_k0[sl], nullptr)) || (rc = pack_gather(ks, L, n, MapId{})))
            return rc;
        ENC_TRY(hipEventRecord(E->g_k1[sl], ks));
        if (g > 0 && (rc = finish(g - 1))) return rc;
    }
    if ((rc = finish(ng - 1))) return rc;
    if (n_checked != n_texts) return bpe_fail(BPE_ERR_STATE, "bpe native: encode groups incomplete");
    E->st.texts_rank += n_texts;
    E->st.tokens_out += out_off[n_texts];
    return BPE_OK;
}

int encode_groups(bpe_encoder *E, const int32_t *ids, const int64_t *off, int64_t n_texts,
                  int32_t *ids_out, int64_t *out_off) {
    // (nothing of an earlier call may still read the staging buffers; a refused call leaves
    // nothing in flight either)
    ENC_TRY(hipStreamSynchronize(E->stream));
    const int rc = encode_groups_run(E, ids, off, n_texts, ids_out, out_off);
    // (every copy of the call is complete on success; a failed call drains both streams)
    (void)hipStreamSynchronize(E->cstream);
    (void)hipStreamSynchronize(E->stream);
    release_stage(E);
    return rc;
}

// The id form (bpe_encode_batch; the text form's replay route enters here too).  It may reallocate
// d_buf and h_buf, and release a large h_buf on return: a caller with staging of its own there has
// brought what it needs to the host first.
int encode_ids(bpe_encoder *E, const int32_t *ids, const int64_t *off, int64_t n_texts, int32_t *ids_out,
               int64_t *out_off) {
    if (n_texts < 0 || (n_texts && (!off || !out_off)))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad encode_batch arguments");
    if (n_texts == 0) {
        if (out_off) out_off[0] = 0;
        return BPE_OK;
    }
    int64_t longest = 0;
    for (int64_t k = 0; k < n_texts; ++k) {
        if (off[k + 1] < off[k]) return bpe_fail(BPE_ERR_ARG, "bpe native: text offsets must not decrease");
        longest = std::max(longest, off[k + 1] - off[k]);
    }
    const int64_t base = off[0], total = off[n_texts] - base;
    if (total && (!ids || !ids_out)) return bpe_fail(BPE_ERR_ARG, "bpe native: null id buffer");
    ENC_TRY(hipSetDevice(E->device));
    E->st.calls++;
    E->st.tokens_in += total;
    int rc;
    // a very large call with no text to replay: in groups, each classifying its own texts
    if (total >= 2 * GROUP_TOKENS && kernel_takes(E, longest) && !getenv("BPE_ENCODE_ONE_GROUP")) {
        if ((rc = upload_table(E))) return rc;
        return encode_groups(E, ids, off, n_texts, ids_out, out_off);
    }
    // long texts in segments, where that route is chosen and the list allows it
    if (longest > CAP_MAX && split_route(E)) return encode_ids_split(E, ids, off, n_texts, ids_out, out_off);
    // per text: the kernels, or the apply-pass route
    ShapeLists lists;
    std::vector<int64_t> replay;
    classify(E, off, n_texts, lists, replay);
    // (only the replay's host route checks ids on the host; the kernels count bad ids)
    for (int64_t k : replay)
        for (int64_t i = off[k]; i < off[k + 1]; ++i)
            if (ids[i] < 0 || ids[i] >= BPE_MAX_VOCAB) return bpe_fail(BPE_ERR_VOCAB, BAD_ID);
    if ((rc = upload_table(E))) return rc;
    // A small call's pinned buffer mirrors the stage's [ooff | ids | off | which]; a large call
    // copies its ids straight from and to the caller's buffers (no host staging pass; a pageable
    // copy costs tens of microseconds of fixed overhead, which a small call cannot hide) and pins
    // only [ooff | off | which].
    Stage L(n_texts, total);
    const bool small = (size_t)total * 4 <= SMALL_CALL_BYTES;
    const size_t h_ids_bytes = small ? L.b_ids : 0;
    if ((rc = grow_stage(E, 2 * L.b_off + h_ids_bytes + L.b_which, L.bytes()))) return rc;
    Release release{E};
    L.place(E->d_buf, n_texts);
    char *h = E->h_buf;
    int64_t *h_ooff = reinterpret_cast<int64_t *>(h);
    int32_t *h_ids = reinterpret_cast<int32_t *>(h + L.b_off);   // (small calls only)
    int64_t *h_off = reinterpret_cast<int64_t *>(h + L.b_off + h_ids_bytes);
    int32_t *h_which = reinterpret_cast<int32_t *>(h + L.b_off + h_ids_bytes + L.b_off);
    rel_offsets(h_off, off, n_texts);
    fill_which(lists, h_which);
    if (small) {
        if (total) std::memcpy(h_ids, ids + base, (size_t)total * 4);
        ENC_TRY(hipMemcpyAsync(L.ids, h_ids, L.b_ids + L.b_off + (size_t)lists.n * 4, hipMemcpyHostToDevice,
                               E->stream));
    } else {
        ENC_TRY(hipMemcpyAsync(L.ids, ids + base, (size_t)total * 4, hipMemcpyHostToDevice, E->stream));
        ENC_TRY(hipMemcpyAsync(L.off, h_off, L.b_off + (size_t)lists.n * 4, hipMemcpyHostToDevice, E->stream));
    }
    // replay texts keep length 0 on the device; they are written on the host below
    if (!replay.empty()) ENC_TRY(hipMemsetAsync(L.len, 0, (size_t)n_texts * 4, E->stream));
    if ((rc = launch_lists(E, lists, true, L, E->ev0, E->ev1))) return rc;
    if (replay.empty()) {
        // [ooff | packed ids] in one copy through the mirror, or the offsets first and then only
        // the packed ids (merges shrink a batch: 5x on zipf words)
        int64_t n_out = 0;
        if ((rc = pack(E->stream, L, n_texts, total, MapId{})) ||
            (rc = fetch_ooff(E->stream, L, h_ooff, n_texts, small ? (size_t)total * 4 : 0, BPE_ERR_VOCAB, BAD_ID)) ||
            (rc = packed_length(h_ooff, n_texts, total, -1, &n_out)))
            return rc;
        if (small) {
            if (n_out) std::memcpy(ids_out, h_ids, (size_t)n_out * 4);
        } else if ((rc = copy_packed(E->stream, ids_out, L.ids, n_out, hipMemcpyDeviceToHost)))
            return rc;
        std::memcpy(out_off, h_ooff, (size_t)(n_texts + 1) * 8);
    } else {
        // host assembly: the kernels' texts come back at their input offsets, the replayed ones
        // from the scratch engine (into the same host buffer: after the copies have landed)
        std::vector<int64_t> len((size_t)n_texts, 0);
        std::vector<int32_t> out((size_t)std::max<int64_t>(total, 1));
        std::vector<int32_t> lens((size_t)n_texts);
        unsigned long long err = 0;
        ENC_TRY(hipMemcpyAsync(out.data(), L.out, (size_t)total * 4, hipMemcpyDeviceToHost, E->stream));
        ENC_TRY(hipMemcpyAsync(lens.data(), L.len, (size_t)n_texts * 4, hipMemcpyDeviceToHost, E->stream));
        ENC_TRY(hipMemcpyAsync(&err, L.err, 8, hipMemcpyDeviceToHost, E->stream));
        ENC_TRY(hipStreamSynchronize(E->stream));
        if (err) return bpe_fail(BPE_ERR_VOCAB, BAD_ID);
        if ((rc = encode_replay(E, ids, off, replay, out.data(), len.data()))) return rc;
        for (auto &v : lists.of)
            for (int32_t k : v) len[k] = lens[k];
        int64_t o = 0;
        out_off[0] = 0;
        for (int64_t k = 0; k < n_texts; ++k) {
            if (len[k]) std::memcpy(ids_out + o, out.data() + (off[k] - base), (size_t)len[k] * 4);
            o += len[k];
            out_off[k + 1] = o;
        }
    }
    float ms = 0;
    ENC_TRY(hipEventElapsedTime(&ms, E->ev0, E->ev1));
    E->st.kernel_ms += ms;
    E->st.texts_rank += lists.n;
    E->st.tokens_out += out_off[n_texts];
    return BPE_OK;
}

// ---- the text form (bpe_encode_text_batch): bpe_text.hip.h's kernels around k_encode -------------

void text_free(bpe_encoder *E) {
    bpe_text_state &T = E->txt;
    if (T.d_bmp) (void)hipFree(T.d_bmp);
    if (T.d_pairs) (void)hipFree(T.d_pairs);
    if (T.d_tvi) (void)hipFree(T.d_tvi);
    if (T.d_st) (void)hipFree(T.d_st);
    if (T.h_st) (void)hipHostFree(T.h_st);
    for (hipEvent_t &ev : T.ev)
        if (ev) (void)hipEventDestroy(ev);
    T = bpe_text_state{};
}

void text_drop_index(bpe_encoder *E) {
    E->txt.tvi.clear();
    E->txt.has_tvi = false;
    E->txt.tvi_dirty = false;
}

// status words and events (made by the first text call), then the tables that changed
int text_upload(bpe_encoder *E) {
    bpe_text_state &T = E->txt;
    if (!T.d_st) ENC_TRY(hipMalloc((void **)&T.d_st, TS_WORDS * 8));
    if (!T.h_st) ENC_TRY(hipHostMalloc((void **)&T.h_st, TS_WORDS * 8, hipHostMallocDefault));
    for (hipEvent_t &ev : T.ev)
        if (!ev) ENC_TRY(hipEventCreate(&ev));
    int rc;
    if (T.has_chars && T.chars_dirty) {
        if (!T.d_bmp) ENC_TRY(hipMalloc((void **)&T.d_bmp, 65536 * 2));
        if ((rc = grow_dev(&T.d_pairs, &T.d_pairs_n, T.pairs.size()))) return rc;
        ENC_TRY(hipMemcpyAsync(T.d_bmp, T.bmp.data(), 65536 * 2, hipMemcpyHostToDevice, E->stream));
        ENC_TRY(hipMemcpyAsync(T.d_pairs, T.pairs.data(), T.pairs.size() * sizeof(uint2),
                               hipMemcpyHostToDevice, E->stream));
        T.chars_dirty = false;
    }
    if (T.has_tvi && T.tvi_dirty) {
        if ((rc = grow_dev(&T.d_tvi, &T.d_tvi_n, T.tvi.size()))) return rc;
        if (!T.tvi.empty())
            ENC_TRY(hipMemcpyAsync(T.d_tvi, T.tvi.data(), T.tvi.size() * 4, hipMemcpyHostToDevice, E->stream));
        T.tvi_dirty = false;
    }
    // (the host vectors may be replaced right after the call returns: the copies must be done)
    ENC_TRY(hipStreamSynchronize(E->stream));
    return BPE_OK;
}

int text_char_error(int64_t k, int64_t unit, uint32_t u0, uint32_t u1, bool has_next) {
    uint32_t cp = u0;
    if ((u0 & 0xFC00u) == 0xD800u && has_next && (u1 & 0xFC00u) == 0xDC00u)
        cp = 0x10000u + ((u0 - 0xD800u) << 10) + (u1 - 0xDC00u);
    char msg[160];
    std::snprintf(msg, sizeof msg, "unknown token, char: U+%04X (text %lld, unit %lld)", cp, (long long)k,
                  (long long)unit);
    return bpe_fail(BPE_ERR_VOCAB, msg);
}

int text_index_error(int32_t id, int64_t k, int64_t pos) {
    char msg[160];
    std::snprintf(msg, sizeof msg, "unknown token index: %d (text %lld, position %lld)", id, (long long)k,
                  (long long)pos);
    return bpe_fail(BPE_ERR_VOCAB, msg);
}

// What every form that ends in the text pipeline checks before any work, in this order and with
// these messages (text_run itself, and the forms that do work in front of it: the UTF-8 transcode,
// the skip-gram forms).  outputs_ok: the caller's capacity and output pointers hold together.
int text_check_call(bpe_encoder *E, int kind, int64_t n_texts, const int64_t *off, bool outputs_ok) {
    if (kind != BPE_ENCODE_IDS && kind != BPE_ENCODE_VECTORS)
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad encode kind");
    if (n_texts < 0 || n_texts >= 0x7FFFFFFF || !outputs_ok || (n_texts && !off))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad encode_text_batch arguments");
    if (kind == BPE_ENCODE_VECTORS && !E->txt.has_tvi)
        return bpe_fail(BPE_ERR_STATE, "bpe native: encode to vectors without a vector index "
                                       "(bpe_encoder_set_vector_index)");
    return BPE_OK;
}

// ... and of the n_texts + 1 offsets once they are on the host
int text_check_offsets(const int64_t *h_off, int64_t n_texts) {
    if (n_texts && h_off[0] < 0) return bpe_fail(BPE_ERR_ARG, "bpe native: negative text offset");
    for (int64_t k = 0; k < n_texts; ++k)
        if (h_off[k + 1] < h_off[k]) return bpe_fail(BPE_ERR_ARG, "bpe native: text offsets must not decrease");
    return BPE_OK;
}

// The pipeline.  dev: units, off, vals_out and out_off are device buffers (the device form);
// otherwise host buffers, staged through the encoder's device buffer.
int text_run(bpe_encoder *E, int kind, const uint16_t *units, const int64_t *off, int64_t n_texts,
             int32_t *vals_out, int64_t cap, int64_t *out_off, bool dev, int64_t *needed) {
    bpe_text_state &T = E->txt;
    *needed = 0;
    int rc0 = text_check_call(E, kind, n_texts, off, !(cap < 0 || !out_off || (cap && !vals_out)));
    if (rc0) return rc0;
    ENC_TRY(hipSetDevice(E->device));
    hipStream_t s = E->stream;
    T.st.calls++;
    // the offsets on the host: checked here, and the launch lists are made from them
    std::vector<int64_t> off_copy;
    const int64_t *h_off = off;
    if (dev && n_texts) {
        off_copy.resize((size_t)n_texts + 1);
        ENC_TRY(hipMemcpyAsync(off_copy.data(), off, off_copy.size() * 8, hipMemcpyDeviceToHost, s));
        ENC_TRY(hipStreamSynchronize(s));
        h_off = off_copy.data();
    }
    if ((rc0 = text_check_offsets(h_off, n_texts))) return rc0;
    const int64_t base = n_texts ? h_off[0] : 0, total = n_texts ? h_off[n_texts] - base : 0;
    if (total && !units) return bpe_fail(BPE_ERR_ARG, "bpe native: null unit buffer");
    if (total && !T.has_chars)
        return bpe_fail(BPE_ERR_STATE, "bpe native: encode of text without a char table (bpe_encoder_set_chars)");
    if (total == 0) {   // (no text, or every text empty)
        if (dev) {
            ENC_TRY(hipMemsetAsync(out_off, 0, (size_t)(n_texts + 1) * 8, s));
            ENC_TRY(hipStreamSynchronize(s));
        } else {
            std::memset(out_off, 0, (size_t)(n_texts + 1) * 8);
        }
        T.st.texts += n_texts;
        return BPE_OK;
    }
    int rc;
    if ((rc = text_upload(E)) || (rc = upload_table(E))) return rc;
    // launch shape of every text by its unit count (its chars are at most that many), or the
    // apply-pass route for the whole call
    ShapeLists lists;
    std::vector<int64_t> no_kernel;
    classify(E, h_off, n_texts, lists, no_kernel);
    // On the split route a text of more than CAP_MAX units is planned after the front end, by its
    // chars: the stage is sized for the segments there can be, and only a text that falls back
    // sends the call through the replay.
    const bool seg = !no_kernel.empty() && split_route(E);
    bool replay = !no_kernel.empty() && !seg;
    const int64_t n_max = seg ? max_segments(h_off, n_texts) : n_texts;
    if (n_max >= 0x7FFFFFFF) return bpe_fail(BPE_ERR_ARG, "bpe native: text batch too large");
    const int mis = dev ? (int)(((uintptr_t)(units + base) >> 1) & (TXT_RUN - 1)) : 0;
    const int64_t n_tiles = (total + mis + TXT_TILE - 1) / TXT_TILE;
    if (n_tiles > 0x7FFFFFFF) return bpe_fail(BPE_ERR_ARG, "bpe native: text batch too large");
    // device: the stage (its ids and off written by k_txt_map: the chars are at most the units), then
    //   [tile counts, then bases | first text of each tile | tile marks | units | off | seg_of]
    // (units and off: the host form's staging; seg_of: the device form's on the split route);
    // pinned: [which | ooff]
    Stage L(n_max, total);
    const size_t b_tiles = align16((size_t)n_tiles * 8), b_edge = align16((size_t)n_tiles * 4);
    const size_t b_units = dev ? 0 : align16((size_t)total * 2);
    const size_t b_uoff = dev ? 0 : L.b_off, b_segof = dev && seg ? align16((size_t)(n_texts + 1) * 8) : 0;
    const size_t bytes = L.bytes() + 2 * b_tiles + b_edge + b_units + b_uoff + b_segof;
    if ((rc = grow_stage(E, L.b_which + L.b_off, bytes))) return rc;
    Release release{E};
    char *d = L.place(E->d_buf, n_texts);
    unsigned long long *d_tiles = reinterpret_cast<unsigned long long *>(d);
    long long *d_first = reinterpret_cast<long long *>(d += b_tiles);
    uint32_t *d_edge = reinterpret_cast<uint32_t *>(d += b_tiles);
    uint16_t *d_units = reinterpret_cast<uint16_t *>(d += b_edge);
    int64_t *d_uoff = reinterpret_cast<int64_t *>(d += b_units);
    int64_t *d_segof = reinterpret_cast<int64_t *>(d += b_uoff);
    int32_t *h_which = reinterpret_cast<int32_t *>(E->h_buf);
    int64_t *h_ooff = reinterpret_cast<int64_t *>(E->h_buf + L.b_which);
    const uint16_t *units_al;
    const int64_t *k_off;
    if (dev) {
        units_al = units + base - mis;
        k_off = off;
    } else {
        ENC_TRY(hipMemcpyAsync(d_units, units + base, (size_t)total * 2, hipMemcpyHostToDevice, s));
        ENC_TRY(hipMemcpyAsync(d_uoff, off, (size_t)(n_texts + 1) * 8, hipMemcpyHostToDevice, s));
        units_al = d_units;
        k_off = d_uoff;
    }
    ENC_TRY(hipMemsetAsync(T.d_st, 0xFF, 16, s));
    ENC_TRY(hipMemsetAsync(T.d_st + 2, 0, (TS_WORDS - 2) * 8, s));
    ENC_TRY(hipMemsetAsync(L.err, 0, 8, s));
    ENC_TRY(hipMemsetAsync(d_first, 0xFF, (size_t)n_tiles * 8, s));
    ENC_TRY(hipMemsetAsync(d_edge, 0, (size_t)n_tiles * 4, s));
    const CharTab ct{T.d_bmp, T.d_pairs, (1u << T.pair_bits) - 1, 32 - T.pair_bits};
    ENC_TRY(hipEventRecord(T.ev[0], s));
    k_txt_count<<<(unsigned)((n_tiles + TXT_CNT_TILES - 1) / TXT_CNT_TILES), TXT_WG, 0, s>>>(units_al, mis, total,
                                                                                          n_tiles, d_tiles);
    k_txt_texts<<<(unsigned)std::min<int64_t>((n_texts + 256) / 256, 2048), 256, 0, s>>>(
        units_al, mis, total, k_off, n_texts, base, n_tiles, d_first, d_edge, d_tiles);
    k_txt_scan<<<1, 1024, 0, s>>>(d_tiles, n_tiles, T.d_st);
    k_txt_map<<<(unsigned)n_tiles, TXT_WG, 0, s>>>(units_al, mis, total, ct, d_tiles, d_first, d_edge, k_off,
                                                  n_texts, base, L.ids, L.off, T.d_st);
    ENC_TRY(hipGetLastError());
    ENC_TRY(hipEventRecord(T.ev[1], s));

    // the unknown char at flat unit `pc`: its text, and the message (two units come back)
    auto text_of_unit = [&](int64_t pc) {
        return (int64_t)(std::upper_bound(h_off, h_off + n_texts + 1, base + pc) - h_off) - 1;
    };
    auto char_error = [&](int64_t pc) -> int {
        const int64_t k = text_of_unit(pc);
        const bool has_next = base + pc + 1 < h_off[k + 1];
        uint16_t u[2] = {0, 0};
        if (dev) {
            ENC_TRY(hipMemcpyAsync(u, units + base + pc, has_next ? 4 : 2, hipMemcpyDeviceToHost, s));
            ENC_TRY(hipStreamSynchronize(s));
        } else {
            u[0] = units[base + pc];
            if (has_next) u[1] = units[base + pc + 1];
        }
        return text_char_error(k, base + pc - h_off[k], u[0], u[1], has_next);
    };
    int64_t n_out = 0;
    float ms = 0;

    // the split route: the texts' id offsets back (8 B per text), the plan on the ids, and from
    // here on the kernels' units are the n_k segments
    SplitPlan P;
    int64_t n_k = n_texts;
    if (seg) {
        std::vector<int64_t> idoff((size_t)n_texts + 1);
        ENC_TRY(hipMemcpyAsync(idoff.data(), L.off, idoff.size() * 8, hipMemcpyDeviceToHost, s));
        ENC_TRY(hipStreamSynchronize(s));
        for (int64_t k = 0; k < n_texts; ++k)
            if (idoff[(size_t)k] < 0 || idoff[(size_t)k + 1] < idoff[(size_t)k] || idoff[(size_t)k + 1] > total)
                return bpe_fail(BPE_ERR_STATE, "bpe native: bad id offsets");
        if (idoff[0] != 0) return bpe_fail(BPE_ERR_STATE, "bpe native: bad id offsets");
        if ((rc = plan_split(E, L.ids, idoff.data(), n_texts, P))) return rc;
        if (!P.fallback.empty()) {
            replay = true;   // (encode_ids makes the plan again, and counts it)
        } else {
            split_commit(E, P);
            n_k = P.n_seg();
            L.place(E->d_buf, n_k);   // (the err word follows the segments' offsets)
            lists = ShapeLists{};
            std::vector<int64_t> none;
            classify(E, P.seg_off.data(), n_k, lists, none);
            if (!none.empty()) return bpe_fail(BPE_ERR_STATE, "bpe native: split plan mismatch");
            ENC_TRY(hipMemcpyAsync(L.off, P.seg_off.data(), (size_t)(n_k + 1) * 8, hipMemcpyHostToDevice, s));
            ENC_TRY(hipMemsetAsync(L.err, 0, 8, s));
            if (dev)
                ENC_TRY(hipMemcpyAsync(d_segof, P.seg_of.data(), (size_t)(n_texts + 1) * 8, hipMemcpyHostToDevice, s));
        }
    }
    // text k's packed offset (h_ooff: one per segment)
    auto text_ooff = [&](int64_t k) { return n_k == n_texts ? h_ooff[k] : h_ooff[P.seg_of[(size_t)k]]; };

    if (replay) {
        // host assembly, as the id form does for these texts: the front end's ids come back (they
        // must: encode_ids lays its own stage over this one), encode_ids replays them, counting
        // its call and tokens as any id call, and the vector index is applied here
        ENC_TRY(hipMemcpyAsync(T.h_st, T.d_st, TS_WORDS * 8, hipMemcpyDeviceToHost, s));
        ENC_TRY(hipStreamSynchronize(s));
        const int64_t n_ids = (int64_t)T.h_st[TS_CHARS];
        if (n_ids < 0 || n_ids > total) return bpe_fail(BPE_ERR_STATE, "bpe native: bad char count");
        std::vector<int32_t> ids((size_t)std::max<int64_t>(n_ids, 1)), vals((size_t)std::max<int64_t>(n_ids, 1));
        std::vector<int64_t> idoff((size_t)n_texts + 1), ooff((size_t)n_texts + 1, 0);
        ENC_TRY(hipMemcpyAsync(ids.data(), L.ids, (size_t)n_ids * 4, hipMemcpyDeviceToHost, s));
        ENC_TRY(hipMemcpyAsync(idoff.data(), L.off, idoff.size() * 8, hipMemcpyDeviceToHost, s));
        ENC_TRY(hipStreamSynchronize(s));
        ENC_TRY(hipEventElapsedTime(&ms, T.ev[0], T.ev[1]));
        T.st.front_ms += ms;
        const bool bad_char = T.h_st[TS_BADCHAR] != TXT_NONE;
        const int64_t pc = (int64_t)T.h_st[TS_BADCHAR];
        // (an unknown char: the texts before its text may still hold a hole, which comes first)
        const int64_t n_use = bad_char ? text_of_unit(pc) : n_texts;
        if (bad_char && kind == BPE_ENCODE_IDS) return char_error(pc);
        if ((rc = encode_ids(E, ids.data(), idoff.data(), n_use, vals.data(), ooff.data()))) return rc;
        if (kind == BPE_ENCODE_VECTORS) {
            const int64_t n_tvi = (int64_t)T.tvi.size();
            for (int64_t k = 0; k < n_use; ++k)
                for (int64_t i = ooff[k]; i < ooff[k + 1]; ++i) {
                    const int32_t id = vals[(size_t)i];
                    const int32_t v = id < n_tvi ? T.tvi[(size_t)id] : -1;
                    if (v < 0) return text_index_error(id, k, i - ooff[k]);
                    vals[(size_t)i] = v;
                }
        }
        if (bad_char) return char_error(pc);
        if ((rc = packed_length(ooff.data(), n_texts, total, cap, needed))) return rc;
        n_out = *needed;
        if (dev) {
            ENC_TRY(hipMemcpyAsync(out_off, ooff.data(), ooff.size() * 8, hipMemcpyHostToDevice, s));
            if ((rc = copy_packed(s, vals_out, vals.data(), n_out, hipMemcpyHostToDevice))) return rc;
        } else {
            if (n_out) std::memcpy(vals_out, vals.data(), (size_t)n_out * 4);
            std::memcpy(out_off, ooff.data(), ooff.size() * 8);
        }
        T.st.chars += n_ids;
    } else {
        fill_which(lists, h_which);
        ENC_TRY(hipMemcpyAsync(L.which, h_which, (size_t)n_k * 4, hipMemcpyHostToDevice, s));
        if ((rc = launch_lists(E, lists, true, L, E->ev0, E->ev1))) return rc;
        const bool vec = kind == BPE_ENCODE_VECTORS;
        ENC_TRY(hipEventRecord(T.ev[2], s));
        if ((rc = vec ? pack(s, L, n_k, total, VecMap{T.d_tvi, (uint32_t)T.tvi.size(), T.d_st})
                      : pack(s, L, n_k, total, MapId{})))
            return rc;
        ENC_TRY(hipEventRecord(T.ev[3], s));
        ENC_TRY(hipMemcpyAsync(T.h_st, T.d_st, TS_WORDS * 8, hipMemcpyDeviceToHost, s));
        // (here the bad-id word counts ids of the char table; the call's times are counted first)
        const int bad_id = fetch_ooff(s, L, h_ooff, n_k, 0, BPE_ERR_STATE, "bpe native: char table id out of range");
        ENC_TRY(hipEventElapsedTime(&ms, T.ev[0], T.ev[1]));
        T.st.front_ms += ms;
        ENC_TRY(hipEventElapsedTime(&ms, T.ev[2], T.ev[3]));
        T.st.back_ms += ms;
        ENC_TRY(hipEventElapsedTime(&ms, E->ev0, E->ev1));
        E->st.kernel_ms += ms;
        if (bad_id) return bad_id;
        // the reference's error order: the first failing text's error, and inside one text the char's
        const bool bad_char = T.h_st[TS_BADCHAR] != TXT_NONE, bad_idx = vec && T.h_st[TS_BADIDX] != TXT_NONE;
        if (bad_char || bad_idx) {
            const int64_t pc = (int64_t)T.h_st[TS_BADCHAR], pi = (int64_t)T.h_st[TS_BADIDX];
            const int64_t kc = bad_char ? text_of_unit(pc) : n_texts;
            // (the hole's segment gi, and the text ki it belongs to: the same without a plan)
            const int64_t gi = bad_idx ? (int64_t)(std::upper_bound(h_ooff, h_ooff + n_k + 1, pi) - h_ooff) - 1 : n_k;
            const int64_t ki = !bad_idx ? n_texts
                               : n_k == n_texts ? gi
                               : (int64_t)(std::upper_bound(P.seg_of.begin(), P.seg_of.end(), gi) - P.seg_of.begin()) - 1;
            if (ki >= kc) return char_error(pc);
            int64_t at_in = 0;
            int32_t id = 0;
            ENC_TRY(hipMemcpyAsync(&at_in, L.off + gi, 8, hipMemcpyDeviceToHost, s));
            ENC_TRY(hipStreamSynchronize(s));
            ENC_TRY(hipMemcpyAsync(&id, L.out + at_in + (pi - h_ooff[gi]), 4, hipMemcpyDeviceToHost, s));
            ENC_TRY(hipStreamSynchronize(s));
            return text_index_error(id, ki, pi - text_ooff(ki));
        }
        if ((rc = packed_length(h_ooff, n_k, total, cap, needed))) return rc;
        n_out = *needed;
        if (dev) {
            if (n_k == n_texts)
                ENC_TRY(hipMemcpyAsync(out_off, L.ooff, (size_t)(n_texts + 1) * 8, hipMemcpyDeviceToDevice, s));
            else {
                k_text_ooff<<<(unsigned)((n_texts + 256) / 256), 256, 0, s>>>(L.ooff, d_segof, n_texts, out_off);
                ENC_TRY(hipGetLastError());
            }
        }
        if ((rc = copy_packed(s, vals_out, L.ids, n_out, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost)))
            return rc;
        if (!dev)
            for (int64_t k = 0; k <= n_texts; ++k) out_off[k] = text_ooff(k);
        E->st.texts_rank += n_texts;
        E->st.tokens_in += (int64_t)T.h_st[TS_CHARS];
        E->st.tokens_out += n_out;
        T.st.chars += (int64_t)T.h_st[TS_CHARS];
    }
    T.st.texts += n_texts;
    T.st.units_in += total;
    T.st.values_out += n_out;
    return BPE_OK;
}

}  // namespace

int encoder_device(bpe_encoder *E, int *device) {
    if (!E || !device) return bpe_fail(BPE_ERR_ARG, "bpe native: null encoder");
    *device = E->device;
    return BPE_OK;
}

// The restore from UTF-8 (bpe_engine.hip): the texts' units and offsets in the encoder's scratch,
// on its device (units == NULL: on the host instead, for a multi-device context); the call's
// numbers are counted by encoder_utf8_done once the restore has succeeded.
int encoder_utf8_units(bpe_encoder *E, const uint8_t *bytes, const int64_t *off, int64_t n_texts, bool dev,
                       const uint16_t **d_units, const int64_t **d_uoff, int64_t *n_units) {
    if (!E || !d_units || !d_uoff || !n_units) return bpe_fail(BPE_ERR_ARG, "bpe native: null encoder");
    ENC_TRY(hipSetDevice(E->device));
    E->u8.st.calls++;
    Utf8Call J;
    J.bytes = bytes, J.off = off, J.n_texts = n_texts, J.dev = dev;
    const int rc = u8_transcode(E->u8, E->stream, J);
    if (rc) return rc;
    *d_units = J.d_units;
    *d_uoff = J.d_uoff;
    *n_units = J.units;
    J.h_off.clear();
    E->u8_pending = J;
    return BPE_OK;
}

void encoder_utf8_done(bpe_encoder *E) { u8_commit(E->u8, E->u8_pending); }

// The restore from lines (bpe_engine.hip): the texts (UTF-16 units, or UTF-8 bytes transcoded first)
// split into samples in the encoder's scratch, on its device; the call's numbers are counted by
// encoder_lines_done once the restore has succeeded.
int encoder_lines_units(bpe_encoder *E, int mode, const void *src, const int64_t *off, int64_t n_texts, bool dev,
                        bool utf8, const uint16_t **d_units, const int64_t **d_uoff, int64_t *n_samples,
                        int64_t *n_units) {
    if (!E || !d_units || !d_uoff || !n_samples || !n_units) return bpe_fail(BPE_ERR_ARG, "bpe native: null encoder");
    ENC_TRY(hipSetDevice(E->device));
    E->ln.st.calls++;
    LinesCall J;
    J.mode = mode, J.n_texts = n_texts;
    E->ln_pending_u8 = utf8;
    if (utf8) {
        E->u8.st.calls++;
        Utf8Call U;
        U.bytes = static_cast<const uint8_t *>(src), U.off = off, U.n_texts = n_texts, U.dev = dev;
        const int rc = u8_transcode(E->u8, E->stream, U);
        if (rc) return rc;
        J.units = U.d_units, J.off = U.d_uoff, J.dev = true;
        U.h_off.clear();
        E->u8_pending = U;
    } else {
        J.units = static_cast<const uint16_t *>(src), J.off = off, J.dev = dev;
    }
    const int rc = ln_split(E->ln, E->stream, J);
    if (rc) return rc;
    *d_units = J.d_out;
    *d_uoff = J.d_ooff;
    *n_samples = J.samples;
    *n_units = J.units_out;
    E->ln_pending = J;
    return BPE_OK;
}

void encoder_lines_done(bpe_encoder *E) {
    if (E->ln_pending_u8) u8_commit(E->u8, E->u8_pending);
    ln_commit(E->ln, E->ln_pending);
}

extern "C" {

int bpe_encoder_create(bpe_encoder **out, int device) {
    if (!out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return bpe_fail(BPE_ERR_HIP, "bpe native: no HIP device available (MI355X required)");
    if (device < 0 || device >= n) return bpe_fail(BPE_ERR_ARG, "bpe native: bad device index");
    bpe_encoder *E = new bpe_encoder();
    E->device = device;
    auto bail = [&](int rc) {
        bpe_encoder_destroy(E);
        return rc;
    };
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&E->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&E->ev0) != hipSuccess || hipEventCreate(&E->ev1) != hipSuccess ||
        hipEventCreate(&E->ev_p0) != hipSuccess || hipEventCreate(&E->ev_p1) != hipSuccess ||
        hipStreamCreateWithFlags(&E->cstream, hipStreamNonBlocking) != hipSuccess)
        return bail(bpe_fail(BPE_ERR_HIP, "bpe native: encoder stream/events"));
    for (int i = 0; i < 2; ++i)
        if (hipEventCreateWithFlags(&E->g_in[i], hipEventDisableTiming) != hipSuccess ||
            hipEventCreate(&E->g_k0[i]) != hipSuccess || hipEventCreate(&E->g_k1[i]) != hipSuccess)
            return bail(bpe_fail(BPE_ERR_HIP, "bpe native: encoder stream/events"));
    if (hipMalloc((void **)&E->d_steps, 64) != hipSuccess ||
        hipMemset(E->d_steps, 0, 64) != hipSuccess)
        return bail(bpe_fail(BPE_ERR_OOM, "bpe native: encoder counters"));
    if (set_lds_attrs<0>() != hipSuccess)
        return bail(bpe_fail(BPE_ERR_HIP, "bpe native: encoder LDS attribute"));
    table_rebuild(E, 10);
    if (const char *v = getenv("BPE_ENCODE_LONG"))
        if (!std::strcmp(v, "split")) E->long_mode = BPE_LONG_SPLIT;
    *out = E;
    return BPE_OK;
}

int bpe_encoder_destroy(bpe_encoder *E) {
    if (!E) return BPE_OK;
    (void)hipSetDevice(E->device);
    if (E->stream) (void)hipStreamSynchronize(E->stream);
    if (E->cstream) (void)hipStreamSynchronize(E->cstream);
    if (E->scratch) bpe_destroy(E->scratch);
    if (E->d_slots) (void)hipFree(E->d_slots);
    if (E->d_limg) (void)hipFree(E->d_limg);
    if (E->d_steps) (void)hipFree(E->d_steps);
    if (E->d_ends) (void)hipFree(E->d_ends);
    if (E->d_cut_slots) (void)hipFree(E->d_cut_slots);
    if (E->d_win) (void)hipFree(E->d_win);
    if (E->d_cut) (void)hipFree(E->d_cut);
    if (E->ev_p0) (void)hipEventDestroy(E->ev_p0);
    if (E->ev_p1) (void)hipEventDestroy(E->ev_p1);
    if (E->d_buf) (void)hipFree(E->d_buf);
    if (E->h_buf) (void)hipHostFree(E->h_buf);
    text_free(E);
    u8_free(E->u8);
    ln_free(E->ln);
    sg_free(E->sg);
    if (E->ev0) (void)hipEventDestroy(E->ev0);
    if (E->ev1) (void)hipEventDestroy(E->ev1);
    for (int i = 0; i < 2; ++i)
        for (hipEvent_t ev : {E->g_in[i], E->g_k0[i], E->g_k1[i]})
            if (ev) (void)hipEventDestroy(ev);
    if (E->cstream) (void)hipStreamDestroy(E->cstream);
    if (E->stream) (void)hipStreamDestroy(E->stream);
    delete E;
    return BPE_OK;
}

int bpe_encoder_clear(bpe_encoder *E) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: null encoder");
    E->abc.clear();
    E->c_of.clear();
    E->is_input.clear();
    E->first_of.clear();
    E->last_of.clear();
    E->is_made.clear();
    E->ends.clear();
    E->cut_slots.clear();
    E->split_ok = true;
    E->greedy_ok = true;
    E->vocab = 0;
    table_rebuild(E, 10);
    E->dirty = true;
    text_drop_index(E);
    return BPE_OK;
}

int bpe_encoder_add_merges(bpe_encoder *E, const int32_t *abc, int64_t n) {
    if (!E || n < 0 || (n && !abc)) return bpe_fail(BPE_ERR_ARG, "bpe native: bad add_merges arguments");
    for (int64_t i = 0; i < 3 * n; ++i)
        if (abc[i] < 0 || abc[i] >= BPE_MAX_VOCAB)
            return bpe_fail(BPE_ERR_VOCAB, "bpe native: merge token id out of range");
    if ((int64_t)E->c_of.size() + n > BPE_MAX_VOCAB)
        return bpe_fail(BPE_ERR_VOCAB, "bpe native: more merges than token ids");
    if (E->is_input.size() < (size_t)BPE_MAX_VOCAB) E->is_input.assign(BPE_MAX_VOCAB, 0);
    if (E->first_of.size() < (size_t)BPE_MAX_VOCAB) {
        E->first_of.resize(BPE_MAX_VOCAB);
        for (int32_t i = 0; i < BPE_MAX_VOCAB; ++i) E->first_of[i] = (uint16_t)i;
        E->last_of = E->first_of;
        E->is_made.assign(BPE_MAX_VOCAB, 0);
    }
    const size_t m = E->c_of.size() + (size_t)n;
    uint32_t bits = E->bits;
    while (((size_t)1 << bits) < 2 * m) ++bits;
    const bool rehash = bits != E->bits;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t a = abc[3 * i], b = abc[3 * i + 1], c = abc[3 * i + 2];
        E->is_input[a] = E->is_input[b] = 1;
        // the greedy needs every new token to be new to the merges up to and including its own
        if (E->is_input[c]) E->greedy_ok = false;
        if (E->is_made[c] || !E->greedy_ok) E->split_ok = false;
        E->is_made[c] = 1;
        E->first_of[c] = E->first_of[a];
        E->last_of[c] = E->last_of[b];
        E->abc.push_back(a);
        E->abc.push_back(b);
        E->abc.push_back(c);
        E->c_of.push_back((uint16_t)c);
        E->vocab = std::max(E->vocab, std::max(a, std::max(b, c)) + 1);
        if (!rehash) table_insert(E, ((uint32_t)a << 16) | (uint32_t)b, (uint32_t)(E->c_of.size() - 1));
    }
    if (rehash) table_rebuild(E, bits);
    E->dirty = true;
    text_drop_index(E);
    return BPE_OK;
}

int bpe_encoder_num_merges(bpe_encoder *E, int64_t *n) {
    if (!E || !n) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *n = (int64_t)E->c_of.size();
    return BPE_OK;
}

int bpe_encode_batch(bpe_encoder *E, const int32_t *ids, const int64_t *off, int64_t n_texts,
                     int32_t *ids_out, int64_t *out_off) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: bad encode_batch arguments");
    return encode_ids(E, ids, off, n_texts, ids_out, out_off);
}

int bpe_encoder_get_stats(bpe_encoder *E, bpe_encoder_stats *out) {
    if (!E || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    ENC_TRY(hipSetDevice(E->device));
    unsigned long long steps[8] = {};
    ENC_TRY(hipMemcpy(steps, E->d_steps, 64, hipMemcpyDeviceToHost));
    E->st.steps = (int64_t)steps[0];
    *out = E->st;
    return BPE_OK;
}

int bpe_encoder_reset_stats(bpe_encoder *E) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    ENC_TRY(hipSetDevice(E->device));
    ENC_TRY(hipMemset(E->d_steps, 0, 64));
    E->st = bpe_encoder_stats{};
    return BPE_OK;
}

int bpe_encoder_set_long_texts(bpe_encoder *E, int mode) {
    if (!E || (mode != BPE_LONG_REPLAY && mode != BPE_LONG_SPLIT))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad set_long_texts arguments");
    E->long_mode = mode;
    return BPE_OK;
}

int bpe_encoder_get_split_stats(bpe_encoder *E, bpe_split_stats *out) {
    if (!E || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = E->sst;
    return BPE_OK;
}

int bpe_encoder_reset_split_stats(bpe_encoder *E) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    E->sst = bpe_split_stats{};
    return BPE_OK;
}

int bpe_encoder_set_chars(bpe_encoder *E, const uint32_t *code_points, const int32_t *ids, int64_t n) {
    if (!E || n < 0 || (n && (!code_points || !ids)))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad set_chars arguments");
    bpe_text_state &T = E->txt;
    if (n == 0) {
        T.bmp.clear();
        T.pairs.clear();
        T.has_chars = false;
        T.chars_dirty = false;
        return BPE_OK;
    }
    // built aside: a failed call changes nothing
    std::vector<uint16_t> bmp(65536, CHAR_UNKNOWN);
    int64_t n_pairs = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (code_points[i] > 0x10FFFFu) return bpe_fail(BPE_ERR_ARG, "bpe native: code point above U+10FFFF");
        if (ids[i] < 0 || ids[i] >= BPE_MAX_VOCAB)
            return bpe_fail(BPE_ERR_VOCAB, "bpe native: char token id out of range");
        n_pairs += code_points[i] > 0xFFFFu;
    }
    uint32_t bits = 4;
    while (((int64_t)1 << bits) < 2 * n_pairs) ++bits;
    std::vector<uint2> pairs((size_t)1 << bits, make_uint2(PAIR_EMPTY, 0u));
    const uint32_t mask = (1u << bits) - 1;
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t cp = code_points[i];
        if (cp <= 0xFFFFu) {
            if (bmp[cp] != CHAR_UNKNOWN) return bpe_fail(BPE_ERR_ARG, "bpe native: duplicate code point");
            bmp[cp] = (uint16_t)ids[i];
        } else {
            uint32_t h = pair_home(cp, 32 - bits);
            while (pairs[h].x != PAIR_EMPTY) {
                if (pairs[h].x == cp) return bpe_fail(BPE_ERR_ARG, "bpe native: duplicate code point");
                h = (h + 1) & mask;
            }
            pairs[h] = make_uint2(cp, (uint32_t)ids[i]);
        }
    }
    T.bmp.swap(bmp);
    T.pairs.swap(pairs);
    T.pair_bits = bits;
    T.has_chars = true;
    T.chars_dirty = true;
    return BPE_OK;
}

int bpe_encoder_set_vector_index(bpe_encoder *E, const int32_t *to_vector_index, int32_t n) {
    if (!E || n < 0 || (n && !to_vector_index))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad set_vector_index arguments");
    if (n == 0 && !to_vector_index) {
        text_drop_index(E);
        return BPE_OK;
    }
    E->txt.tvi.assign(to_vector_index, to_vector_index + n);
    E->txt.has_tvi = true;
    E->txt.tvi_dirty = true;
    return BPE_OK;
}

int bpe_encode_text_batch(bpe_encoder *E, int kind, const uint16_t *units, const int64_t *off, int64_t n_texts,
                          int32_t *vals_out, int64_t vals_cap, int64_t *out_off) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: null encoder");
    int64_t needed = 0;
    return text_run(E, kind, units, off, n_texts, vals_out, vals_cap, out_off, false, &needed);
}

int bpe_encode_text_batch_device(bpe_encoder *E, int kind, const uint16_t *d_units, const int64_t *d_off,
                                 int64_t n_texts, int32_t *d_vals_out, int64_t vals_cap, int64_t *d_out_off,
                                 int64_t *needed) {
    if (!E || !needed) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    return text_run(E, kind, d_units, d_off, n_texts, d_vals_out, vals_cap, d_out_off, true, needed);
}

int bpe_encoder_utf8_to_utf16(bpe_encoder *E, const uint8_t *bytes, const int64_t *off, int64_t n_texts,
                              uint16_t *units_out, int64_t units_cap, int64_t *out_off) {
    if (!E || units_cap < 0 || !out_off || (units_cap && !units_out))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad utf8_to_utf16 arguments");
    ENC_TRY(hipSetDevice(E->device));
    E->u8.st.calls++;
    Utf8Call J;
    J.bytes = bytes, J.off = off, J.n_texts = n_texts, J.dev = false, J.cap = units_cap;
    int rc = u8_transcode(E->u8, E->stream, J);
    if (rc) return rc;
    ENC_TRY(hipMemcpyAsync(out_off, J.d_uoff, (size_t)(n_texts + 1) * 8, hipMemcpyDeviceToHost, E->stream));
    if (J.fits && J.units)
        ENC_TRY(hipMemcpyAsync(units_out, J.d_units, (size_t)J.units * 2, hipMemcpyDeviceToHost, E->stream));
    ENC_TRY(hipStreamSynchronize(E->stream));
    if (!J.fits) return u8_cap_error(J);
    u8_commit(E->u8, J);
    return BPE_OK;
}

int bpe_encoder_utf8_to_utf16_device(bpe_encoder *E, const uint8_t *d_bytes, const int64_t *d_off, int64_t n_texts,
                                     uint16_t *d_units_out, int64_t units_cap, int64_t *d_out_off, int64_t *needed) {
    if (!E || !needed || units_cap < 0 || !d_out_off || (units_cap && !d_units_out))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad utf8_to_utf16 arguments");
    *needed = 0;
    ENC_TRY(hipSetDevice(E->device));
    E->u8.st.calls++;
    Utf8Call J;
    J.bytes = d_bytes, J.off = d_off, J.n_texts = n_texts, J.dev = true, J.cap = units_cap;
    J.d_units = units_cap ? d_units_out : nullptr, J.d_uoff = d_out_off;
    int rc = u8_transcode(E->u8, E->stream, J);
    if (rc) return rc;
    *needed = J.units;
    if (!J.fits) return u8_cap_error(J);
    u8_commit(E->u8, J);
    return BPE_OK;
}

namespace {

// transcode, then the UTF-16 device form on the units; the host form's values and offsets come
// back from scratch
int utf8_encode(bpe_encoder *E, int kind, const uint8_t *bytes, const int64_t *off, int64_t n_texts, int32_t *vals_out,
                int64_t cap, int64_t *out_off, bool dev, int64_t *needed) {
    *needed = 0;
    // (the UTF-16 form's own checks, made before any work here as they are made there)
    int rc = text_check_call(E, kind, n_texts, off, !(cap < 0 || !out_off || (cap && !vals_out)));
    if (rc) return rc;
    ENC_TRY(hipSetDevice(E->device));
    E->u8.st.calls++;
    Utf8Call J;
    J.bytes = bytes, J.off = off, J.n_texts = n_texts, J.dev = dev;
    // the host form's values go through scratch: at most min(cap, bytes) of them (a text never grows)
    if (!dev) J.vals_cap = cap;
    if ((rc = u8_transcode(E->u8, E->stream, J))) return rc;
    if (dev) {
        rc = text_run(E, kind, J.d_units, J.d_uoff, n_texts, vals_out, cap, out_off, true, needed);
    } else {
        rc = text_run(E, kind, J.d_units, J.d_uoff, n_texts, J.d_vals, J.s_cap, J.d_ooff, true, needed);
        if (rc) return rc;
        ENC_TRY(hipMemcpyAsync(out_off, J.d_ooff, (size_t)(n_texts + 1) * 8, hipMemcpyDeviceToHost, E->stream));
        if (*needed) ENC_TRY(hipMemcpyAsync(vals_out, J.d_vals, (size_t)*needed * 4, hipMemcpyDeviceToHost, E->stream));
        ENC_TRY(hipStreamSynchronize(E->stream));
    }
    if (rc) return rc;
    u8_commit(E->u8, J);
    return BPE_OK;
}

}  // namespace

int bpe_encode_utf8_batch(bpe_encoder *E, int kind, const uint8_t *bytes, const int64_t *off, int64_t n_texts,
                          int32_t *vals_out, int64_t vals_cap, int64_t *out_off) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: null encoder");
    int64_t needed = 0;
    return utf8_encode(E, kind, bytes, off, n_texts, vals_out, vals_cap, out_off, false, &needed);
}

int bpe_encode_utf8_batch_device(bpe_encoder *E, int kind, const uint8_t *d_bytes, const int64_t *d_off,
                                 int64_t n_texts, int32_t *d_vals_out, int64_t vals_cap, int64_t *d_out_off,
                                 int64_t *needed) {
    if (!E || !needed) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    return utf8_encode(E, kind, d_bytes, d_off, n_texts, d_vals_out, vals_cap, d_out_off, true, needed);
}

int bpe_encoder_get_utf8_stats(bpe_encoder *E, bpe_utf8_stats *out) {
    if (!E || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = E->u8.st;
    return BPE_OK;
}

int bpe_encoder_reset_utf8_stats(bpe_encoder *E) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    E->u8.st = bpe_utf8_stats{};
    return BPE_OK;
}

int bpe_encoder_split_lines(bpe_encoder *E, int mode, const uint16_t *units, const int64_t *off, int64_t n_texts,
                            uint16_t *units_out, int64_t units_cap, int64_t *out_off, int64_t off_cap,
                            int64_t *n_samples) {
    if (!E || !n_samples || units_cap < 0 || off_cap < 0 || (units_cap && !units_out) || (off_cap && !out_off))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad split_lines arguments");
    *n_samples = 0;
    ENC_TRY(hipSetDevice(E->device));
    E->ln.st.calls++;
    LinesCall J;
    J.mode = mode, J.units = units, J.off = off, J.n_texts = n_texts, J.dev = false;
    J.units_cap = units_cap, J.off_cap = off_cap;
    const int rc = ln_split(E->ln, E->stream, J);
    *n_samples = J.samples;
    if (rc) return rc;
    if (!J.fits) return ln_cap_error(J);
    ENC_TRY(hipMemcpyAsync(out_off, J.d_ooff, (size_t)(J.samples + 1) * 8, hipMemcpyDeviceToHost, E->stream));
    if (J.units_out)
        ENC_TRY(hipMemcpyAsync(units_out, J.d_out, (size_t)J.units_out * 2, hipMemcpyDeviceToHost, E->stream));
    ENC_TRY(hipStreamSynchronize(E->stream));
    ln_commit(E->ln, J);
    return BPE_OK;
}

int bpe_encoder_split_lines_device(bpe_encoder *E, int mode, const uint16_t *d_units, const int64_t *d_off,
                                   int64_t n_texts, uint16_t *d_units_out, int64_t units_cap, int64_t *d_out_off,
                                   int64_t off_cap, int64_t *n_samples, int64_t *needed) {
    if (!E || !n_samples || !needed || units_cap < 0 || off_cap < 0 || (units_cap && !d_units_out) ||
        (off_cap && !d_out_off) || ((uintptr_t)d_units_out & 1))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad split_lines arguments");
    *n_samples = *needed = 0;
    ENC_TRY(hipSetDevice(E->device));
    E->ln.st.calls++;
    LinesCall J;
    J.mode = mode, J.units = d_units, J.off = d_off, J.n_texts = n_texts, J.dev = true;
    J.units_cap = units_cap, J.off_cap = off_cap;
    J.d_out = units_cap ? d_units_out : nullptr, J.d_ooff = off_cap ? d_out_off : nullptr;
    const int rc = ln_split(E->ln, E->stream, J);
    *n_samples = J.samples;
    *needed = J.units_out;
    if (rc) return rc;
    if (!J.fits) return ln_cap_error(J);
    ln_commit(E->ln, J);
    return BPE_OK;
}

int bpe_encoder_get_lines_stats(bpe_encoder *E, bpe_lines_stats *out) {
    if (!E || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = E->ln.st;
    return BPE_OK;
}

int bpe_encoder_reset_lines_stats(bpe_encoder *E) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    E->ln.st = bpe_lines_stats{};
    return BPE_OK;
}

// ---- skip-gram pairs (include/bpe.h; csrc/bpe_skipgram.hip.h) ---------------------------------------

int bpe_encoder_skipgram(bpe_encoder *E, const int32_t *vals, const int64_t *off, int64_t n_texts, int window,
                         int32_t *targets, int32_t *contexts, int64_t pairs_cap, int64_t *pair_off) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: null encoder");
    ENC_TRY(hipSetDevice(E->device));
    E->sg.st.calls++;
    int rc = sg_check_window(window);
    if (rc) return rc;
    if (pairs_cap < 0 || !pair_off || (pairs_cap && (!targets || !contexts)))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram output arguments");
    SgCall J;
    J.window = window;
    if ((rc = sg_stage_host(E->sg, E->stream, vals, off, n_texts, J))) return rc;
    return sg_host_form(E->sg, E->stream, J, targets, contexts, pairs_cap, pair_off);
}

int bpe_encoder_skipgram_device(bpe_encoder *E, const int32_t *d_vals, const int64_t *d_off, int64_t n_texts,
                                int window, int32_t *d_targets, int32_t *d_contexts, int64_t pairs_cap,
                                int64_t *d_pair_off, int64_t *needed) {
    if (!E || !needed) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *needed = 0;
    ENC_TRY(hipSetDevice(E->device));
    E->sg.st.calls++;
    if (pairs_cap < 0 || !d_pair_off || (pairs_cap && (!d_targets || !d_contexts)))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram output arguments");
    SgCall J;
    J.d_vals = d_vals, J.d_off = d_off, J.n_texts = n_texts, J.window = window;
    J.d_t = pairs_cap ? d_targets : nullptr, J.d_c = pairs_cap ? d_contexts : nullptr;
    J.d_poff = d_pair_off, J.cap = pairs_cap;
    return sg_device_form(E->sg, E->stream, J, needed);
}

namespace {

// The texts (UTF-16 units, or UTF-8 bytes transcoded first) through the encoder's device form into
// the skip-gram scratch: J's values and offsets.  A transcode's numbers wait in *U for the commit.
int sg_encode(bpe_encoder *E, int kind, const void *src, const int64_t *off, int64_t n, bool dev, bool utf8,
              SgCall &J, Utf8Call *U) {
    // (the encoder's own checks, made before any work here as they are made there: text_check_call)
    int rc = text_check_call(E, kind, n, off, true);
    if (rc) return rc;
    hipStream_t s = E->stream;
    SgState &S = E->sg;
    const size_t b_off = sg_align((size_t)(n + 1) * 8);
    const uint16_t *d_units = nullptr;
    const int64_t *d_uoff = nullptr;
    int64_t total = 0;   // units the texts have: their values are at most that many
    size_t b_units = 0, b_uoff = 0;
    if (utf8) {
        E->u8.st.calls++;
        U->bytes = static_cast<const uint8_t *>(src), U->off = off, U->n_texts = n, U->dev = dev;
        if ((rc = u8_transcode(E->u8, s, *U))) return rc;
        U->h_off.clear();
        d_units = U->d_units, d_uoff = U->d_uoff, total = U->units;
    } else if (dev) {
        int64_t ends[2] = {0, 0};
        if (n) {
            ENC_TRY(hipMemcpyAsync(&ends[0], off, 8, hipMemcpyDeviceToHost, s));
            ENC_TRY(hipMemcpyAsync(&ends[1], off + n, 8, hipMemcpyDeviceToHost, s));
            ENC_TRY(hipStreamSynchronize(s));
        }
        total = std::max<int64_t>(ends[1] - ends[0], 0);   // (bad offsets: the encoder says so below)
        d_units = static_cast<const uint16_t *>(src), d_uoff = off;
    } else {
        if ((rc = text_check_offsets(off, n))) return rc;   // (before the units they name are staged)
        total = n ? off[n] - off[0] : 0;
        if (total && !src) return bpe_fail(BPE_ERR_ARG, "bpe native: null unit buffer");
        b_units = sg_align((size_t)total * 2), b_uoff = b_off;
    }
    // scratch: [values | their offsets | the host form's units | its offsets]
    const size_t b_vals = sg_align((size_t)total * 4);
    if ((rc = sg_grow(s, &S.d_in, &S.in_cap, b_vals + b_off + b_units + b_uoff))) return rc;
    int32_t *d_vals = reinterpret_cast<int32_t *>(S.d_in);
    int64_t *d_voff = reinterpret_cast<int64_t *>(S.d_in + b_vals);
    if (!utf8 && !dev) {
        uint16_t *s_units = reinterpret_cast<uint16_t *>(S.d_in + b_vals + b_off);
        int64_t *s_uoff = reinterpret_cast<int64_t *>(S.d_in + b_vals + b_off + b_units);
        std::vector<int64_t> rel((size_t)n + 1, 0);
        for (int64_t k = 0; k <= n && n; ++k) rel[(size_t)k] = off[k] - off[0];
        if (total)
            ENC_TRY(hipMemcpyAsync(s_units, static_cast<const uint16_t *>(src) + off[0], (size_t)total * 2,
                                   hipMemcpyHostToDevice, s));
        ENC_TRY(hipMemcpyAsync(s_uoff, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        ENC_TRY(hipStreamSynchronize(s));   // (rel goes away)
        d_units = s_units, d_uoff = s_uoff;
    }
    int64_t n_vals = 0;
    if ((rc = text_run(E, kind, d_units, d_uoff, n, d_vals, total, d_voff, true, &n_vals))) return rc;
    J.d_vals = d_vals, J.d_off = d_voff, J.n_texts = n;
    return BPE_OK;
}

int sg_text(bpe_encoder *E, int kind, const void *src, const int64_t *off, int64_t n, bool utf8, int window,
            int32_t *targets, int32_t *contexts, int64_t cap, int64_t *pair_off, bool dev, int64_t *needed) {
    *needed = 0;
    ENC_TRY(hipSetDevice(E->device));
    E->sg.st.calls++;
    int rc = sg_check_window(window);
    if (rc) return rc;
    if (cap < 0 || !pair_off || (cap && (!targets || !contexts)))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram output arguments");
    SgCall J;
    Utf8Call U;
    J.window = window;
    if ((rc = sg_encode(E, kind, src, off, n, dev, utf8, J, &U))) return rc;
    if (dev) {
        J.d_t = cap ? targets : nullptr, J.d_c = cap ? contexts : nullptr, J.d_poff = pair_off, J.cap = cap;
        rc = sg_device_form(E->sg, E->stream, J, needed);
    } else {
        rc = sg_host_form(E->sg, E->stream, J, targets, contexts, cap, pair_off);
    }
    if (rc) return rc;
    if (utf8) u8_commit(E->u8, U);
    return BPE_OK;
}

}  // namespace

int bpe_skipgram_text_batch(bpe_encoder *E, int kind, const uint16_t *units, const int64_t *off, int64_t n_texts,
                            int window, int32_t *targets, int32_t *contexts, int64_t pairs_cap, int64_t *pair_off) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: null encoder");
    int64_t needed = 0;
    return sg_text(E, kind, units, off, n_texts, false, window, targets, contexts, pairs_cap, pair_off, false, &needed);
}

int bpe_skipgram_text_batch_device(bpe_encoder *E, int kind, const uint16_t *d_units, const int64_t *d_off,
                                   int64_t n_texts, int window, int32_t *d_targets, int32_t *d_contexts,
                                   int64_t pairs_cap, int64_t *d_pair_off, int64_t *needed) {
    if (!E || !needed) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    return sg_text(E, kind, d_units, d_off, n_texts, false, window, d_targets, d_contexts, pairs_cap, d_pair_off, true,
                   needed);
}

int bpe_skipgram_utf8_batch(bpe_encoder *E, int kind, const uint8_t *bytes, const int64_t *off, int64_t n_texts,
                            int window, int32_t *targets, int32_t *contexts, int64_t pairs_cap, int64_t *pair_off) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: null encoder");
    int64_t needed = 0;
    return sg_text(E, kind, bytes, off, n_texts, true, window, targets, contexts, pairs_cap, pair_off, false, &needed);
}

int bpe_skipgram_utf8_batch_device(bpe_encoder *E, int kind, const uint8_t *d_bytes, const int64_t *d_off,
                                   int64_t n_texts, int window, int32_t *d_targets, int32_t *d_contexts,
                                   int64_t pairs_cap, int64_t *d_pair_off, int64_t *needed) {
    if (!E || !needed) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    return sg_text(E, kind, d_bytes, d_off, n_texts, true, window, d_targets, d_contexts, pairs_cap, d_pair_off, true,
                   needed);
}

int bpe_encoder_get_skipgram_stats(bpe_encoder *E, bpe_skipgram_stats *out) {
    if (!E || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = E->sg.st;
    return BPE_OK;
}

int bpe_encoder_reset_skipgram_stats(bpe_encoder *E) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    E->sg.st = bpe_skipgram_stats{};
    return BPE_OK;
}

int bpe_encoder_get_text_stats(bpe_encoder *E, bpe_text_stats *out) {
    if (!E || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = E->txt.st;
    return BPE_OK;
}

int bpe_encoder_reset_text_stats(bpe_encoder *E) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    E->txt.st = bpe_text_stats{};
    return BPE_OK;
}

}  // extern "C"
