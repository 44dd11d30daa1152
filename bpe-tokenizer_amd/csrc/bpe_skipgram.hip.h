// bpe_skipgram.hip.h — skip-gram pairs on the device (include/bpe.h, "skip-gram pairs"): a ragged
// batch of int32 values (vector indices or ids) -> the (target, context) pairs of every text over a
// window of w values on each side, in the order of the loop of example/skip-gram.ts:30-47, as two
// int32 planes and n_texts + 1 int64 pair offsets.  For the two translation units that own such
// values: the encoder (bpe_encode.hip: its own output) and the context (bpe_engine.hip: the corpus
// export).  Everything here has internal linkage.
//
//   k_sg_offsets  one workgroup: the texts' offsets checked (non-negative, non-decreasing), each
//                 text's pairs by the closed form (sg_text_pairs), and their exclusive scan,
//                 BPE_SKIPGRAM_SCAN_ROUND texts per round; the totals go to the status words;
//   k_sg_expand   output-centric: one workgroup per tile of BPE_SKIPGRAM_TILE pairs.  Two lanes find
//                 the texts of the tile's first and last pair by bisection of the pair offsets;
//                 every lane then owns runs of four consecutive pairs at a 16-B address of both
//                 planes, finds the first one's text between the tile's two, inverts its number in
//                 the text to (token, place) by sg_invert (integers only, bpe_skipgram_rule.h) and
//                 steps on from there, bisecting again where a run passes into the next text.  A
//                 text of any length costs what its pairs cost, and texts without pairs cost
//                 nothing.  Values are read straight from the batch: the 2w + 1 neighbours of a run
//                 sit in the same or the next cache line and every value is read by 2w lanes of the
//                 same or the next wave, so the loads hit L1/L2; they are copied, never interpreted.
//                 Stores are 16 B per lane and plane (tiles are cut at 16-B addresses of the planes:
//                 slot s of tile t is pair t * TILE + s - mis); the runs that straddle pair 0 or the
//                 last pair store their valid pairs one by one.  When the two planes sit at
//                 different addresses mod 16 the tile is covered pair by pair (coalesced 4-B
//                 stores).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "bpe.h"
#include "bpe_multi.h"            // bpe_fail
#include "bpe_text_front.hip.h"   // txt_wave_incl64
#include "bpe_skipgram_rule.h"

namespace {

constexpr int SG_TILE = BPE_SKIPGRAM_TILE;
constexpr int SG_WG = 256;
constexpr int SG_RUN = 4;                                // pairs per lane and store (16 B)
constexpr int SG_STEPS = SG_TILE / (SG_WG * SG_RUN);     // runs per lane
constexpr int SG_SCAN_EACH = 8;                          // texts per thread and round of k_sg_offsets
static_assert(SG_TILE == SG_WG * SG_RUN * SG_STEPS && SG_STEPS >= 1, "whole runs per lane");
static_assert(1024 * SG_SCAN_EACH == BPE_SKIPGRAM_SCAN_ROUND, "include/bpe.h");
// status words of a call on the device
constexpr int SGS_PAIRS = 0;    // pairs of the whole batch
constexpr int SGS_BAD = 1;      // nonzero: an offset is negative or smaller than the one before it
constexpr int SGS_VALUES = 2;   // off[n_texts] - off[0]
constexpr int SGS_WORDS = 4;

__global__ void __launch_bounds__(1024)
k_sg_offsets(const int64_t *__restrict__ off, int64_t n_texts, int w, long long *__restrict__ poff,
             unsigned long long *__restrict__ st) {
    __shared__ unsigned long long ws[16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long carry = 0;
    bool bad = false;
    for (int64_t b = 0; b < n_texts; b += 1024 * SG_SCAN_EACH) {
        const int64_t i0 = b + (int64_t)threadIdx.x * SG_SCAN_EACH;
        unsigned long long v[SG_SCAN_EACH], mine = 0;
        int64_t a = i0 < n_texts ? off[i0] : 0;
#pragma unroll
        for (int e = 0; e < SG_SCAN_EACH; ++e) {
            v[e] = 0;
            if (i0 + e < n_texts) {
                const int64_t z = off[i0 + e + 1];
                if (a < 0 || z < a) bad = true;
                else v[e] = (unsigned long long)sg_text_pairs(z - a, w);
                a = z;
            }
            mine += v[e];
        }
        const unsigned long long incl = txt_wave_incl64(mine, lane);
        if (lane == 63) ws[wv] = incl;
        __syncthreads();
        unsigned long long before = 0, all = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const unsigned long long x = ws[i];
            before += i < wv ? x : 0;
            all += x;
        }
        unsigned long long pre = carry + before + incl - mine;
#pragma unroll
        for (int e = 0; e < SG_SCAN_EACH; ++e) {
            if (i0 + e < n_texts) poff[i0 + e] = (long long)pre;
            pre += v[e];
        }
        carry += all;
        __syncthreads();   // (ws is reused next round)
    }
    if (bad) st[SGS_BAD] = 1ull;   // (every writer stores the same word)
    if (threadIdx.x == 0) {
        poff[n_texts] = (long long)carry;
        st[SGS_PAIRS] = carry;
        st[SGS_VALUES] = (unsigned long long)(off[n_texts] - off[0]);
    }
}

// the text of pair q: the largest k in [lo, hi] with poff[k] <= q (poff[lo] <= q; texts without pairs
// share their offset with the text after them and are passed over)
__device__ __forceinline__ int64_t sg_text_of(const long long *__restrict__ poff, int64_t lo, int64_t hi, int64_t q) {
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (poff[mid] <= q) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// where a lane is in the batch: text k = vals[base .. base + n), whose pairs end before pe; token i,
// which has cn pairs, and the place c among them
struct SgCursor {
    int64_t pe, base, n, i, c, cn;
};

__device__ __forceinline__ void sg_locate(const int64_t *__restrict__ off, const long long *__restrict__ poff,
                                          int64_t klo, int64_t khi, int64_t q, int w, SgCursor &u) {
    const int64_t k = sg_text_of(poff, klo, khi, q);
    u.pe = poff[k + 1];
    u.base = off[k];
    u.n = off[k + 1] - u.base;
    sg_invert(q - poff[k], u.n, w, u.i, u.c);
    u.cn = sg_token_pairs(u.i, u.n, w);
}

__device__ __forceinline__ void sg_read(const int32_t *__restrict__ vals, const SgCursor &u, int w, int32_t &t,
                                        int32_t &c) {
    // (both places are inside the text by sg_invert; the clamps keep a load in the batch whatever happens)
    const int64_t last = u.n - 1;
    const int64_t i = u.i < 0 ? 0 : (u.i > last ? last : u.i);
    int64_t j = sg_context(u.i, u.c, w);
    j = j < 0 ? 0 : (j > last ? last : j);
    t = vals[u.base + i];
    c = vals[u.base + j];
}

__device__ __forceinline__ void sg_step(SgCursor &u, int w) {
    if (++u.c == u.cn) {
        u.c = 0;
        ++u.i;
        u.cn = sg_token_pairs(u.i, u.n, w);
    }
}

template <bool VEC>
__global__ void __launch_bounds__(SG_WG)
k_sg_expand(const int32_t *__restrict__ vals, const int64_t *__restrict__ off, const long long *__restrict__ poff,
            int64_t n_texts, int w, int64_t n_pairs, int mis, int32_t *__restrict__ tg, int32_t *__restrict__ cx) {
    __shared__ long long s_k[2];
    const int64_t q_tile = (int64_t)blockIdx.x * SG_TILE - mis;   // the pair at slot 0
    if (threadIdx.x < 2) {
        const int64_t q_lo = q_tile < 0 ? 0 : q_tile;
        const int64_t q_hi = (q_tile + SG_TILE < n_pairs ? q_tile + SG_TILE : n_pairs) - 1;
        s_k[threadIdx.x] = sg_text_of(poff, 0, n_texts - 1, threadIdx.x ? q_hi : q_lo);
    }
    __syncthreads();
    const int64_t klo = s_k[0], khi = s_k[1];
    SgCursor u{};
    if (VEC) {
#pragma unroll
        for (int g = 0; g < SG_STEPS; ++g) {
            const int64_t q0 = q_tile + (int64_t)(g * SG_WG + threadIdx.x) * SG_RUN;
            if (q0 >= n_pairs || q0 + SG_RUN <= 0) continue;
            int32_t t[SG_RUN], c[SG_RUN];
            bool fresh = true;
#pragma unroll
            for (int e = 0; e < SG_RUN; ++e) {
                const int64_t q = q0 + e;
                t[e] = c[e] = 0;
                if (q < 0 || q >= n_pairs) continue;
                if (fresh || q >= u.pe) sg_locate(off, poff, klo, khi, q, w, u);
                fresh = false;
                sg_read(vals, u, w, t[e], c[e]);
                sg_step(u, w);
            }
            if (q0 >= 0 && q0 + SG_RUN <= n_pairs) {
                *reinterpret_cast<int4 *>(tg + q0) = make_int4(t[0], t[1], t[2], t[3]);
                *reinterpret_cast<int4 *>(cx + q0) = make_int4(c[0], c[1], c[2], c[3]);
            } else {
#pragma unroll
                for (int e = 0; e < SG_RUN; ++e)
                    if (q0 + e >= 0 && q0 + e < n_pairs) tg[q0 + e] = t[e], cx[q0 + e] = c[e];
            }
        }
    } else {
        for (int g = 0; g < SG_STEPS * SG_RUN; ++g) {
            const int64_t q = q_tile + g * SG_WG + threadIdx.x;
            if (q < 0 || q >= n_pairs) continue;
            sg_locate(off, poff, klo, khi, q, w, u);
            int32_t t, c;
            sg_read(vals, u, w, t, c);
            tg[q] = t;
            cx[q] = c;
        }
    }
}

#define SG_TRY(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return bpe_fail(e_ == hipErrorOutOfMemory ? BPE_ERR_OOM : BPE_ERR_HIP,         \
                            (std::string("bpe native: ") + #expr + ": " +                   \
                             hipGetErrorString(e_)).c_str());                              \
    } while (0)

}  // namespace

// ---- host side: the expansion of one call on one device and stream ------------------------------

// Scratch (grow-only), status words, events and counters of the skip-gram expansion of an encoder
// or a context.  Three buffers, so that one of them growing leaves the others' contents alone:
// `in` holds what a pipeline or a host form feeds the expansion (units, values, their offsets),
// `work` the pair offsets, `out` a host form's planes.
struct SgState {
    char *d_in = nullptr, *d_work = nullptr, *d_out = nullptr;
    size_t in_cap = 0, work_cap = 0, out_cap = 0;
    unsigned long long *d_st = nullptr, *h_st = nullptr;   // (h_st pinned)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bpe_skipgram_stats st{};
};

// One call's expansion: sg_offsets, then sg_expand (or sg_to_host) with the outputs set.
struct SgCall {
    // in
    const int32_t *d_vals = nullptr;   // text k = d_vals[d_off[k] .. d_off[k+1]), device buffers
    const int64_t *d_off = nullptr;
    int64_t n_texts = 0;
    int window = 0;
    int32_t *d_t = nullptr, *d_c = nullptr;   // the planes on the device (cap pairs each)
    int64_t *d_poff = nullptr;                // where the n_texts + 1 pair offsets go on the device, or nullptr
    int64_t cap = 0;
    // out
    const long long *d_scan = nullptr;        // the pair offsets in scratch
    int64_t pairs = 0, values = 0;
    bool fits = true;                         // false: pairs > cap, only the offsets were written
    double ms = 0;
};

namespace {

inline void sg_free(SgState &S) {
    if (S.d_in) (void)hipFree(S.d_in);
    if (S.d_work) (void)hipFree(S.d_work);
    if (S.d_out) (void)hipFree(S.d_out);
    if (S.d_st) (void)hipFree(S.d_st);
    if (S.h_st) (void)hipHostFree(S.h_st);
    for (hipEvent_t &ev : S.ev)
        if (ev) (void)hipEventDestroy(ev);
    S = SgState{};
}

inline size_t sg_align(size_t x) { return (x + 15) & ~(size_t)15; }

// room for `bytes` in one of the scratch buffers (its contents are not kept)
inline int sg_grow(hipStream_t s, char **buf, size_t *have, size_t bytes) {
    if (bytes <= *have) return BPE_OK;
    SG_TRY(hipStreamSynchronize(s));
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr;
    *have = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    SG_TRY(hipMalloc((void **)buf, want));
    *have = want;
    return BPE_OK;
}

inline int sg_check_window(int window) {
    if (window >= 1 && window <= BPE_SKIPGRAM_MAX_WINDOW) return BPE_OK;
    char msg[96];
    std::snprintf(msg, sizeof msg, "bpe native: skip-gram window %d outside [1, %d]", window, BPE_SKIPGRAM_MAX_WINDOW);
    return bpe_fail(BPE_ERR_ARG, msg);
}

// The texts' offsets checked and turned into pair offsets in scratch; J.pairs and J.values.
inline int sg_offsets(SgState &S, hipStream_t s, SgCall &J) {
    const int64_t n = J.n_texts;
    int rc = sg_check_window(J.window);
    if (rc) return rc;
    if (n < 0 || n >= 0x7FFFFFFF || (n && !J.d_off) || ((uintptr_t)J.d_off & 7) || ((uintptr_t)J.d_vals & 3))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram batch arguments");
    if (!S.d_st) SG_TRY(hipMalloc((void **)&S.d_st, SGS_WORDS * 8));
    if (!S.h_st) SG_TRY(hipHostMalloc((void **)&S.h_st, SGS_WORDS * 8, hipHostMallocDefault));
    for (hipEvent_t &ev : S.ev)
        if (!ev) SG_TRY(hipEventCreate(&ev));
    if ((rc = sg_grow(s, &S.d_work, &S.work_cap, sg_align((size_t)(n + 1) * 8)))) return rc;
    J.d_scan = reinterpret_cast<const long long *>(S.d_work);
    J.pairs = J.values = 0;
    J.ms = 0;
    J.fits = true;
    if (n == 0) {
        SG_TRY(hipMemsetAsync(S.d_work, 0, 8, s));
        SG_TRY(hipStreamSynchronize(s));
        return BPE_OK;
    }
    SG_TRY(hipMemsetAsync(S.d_st, 0, SGS_WORDS * 8, s));
    SG_TRY(hipEventRecord(S.ev[0], s));
    k_sg_offsets<<<1, 1024, 0, s>>>(J.d_off, n, J.window, reinterpret_cast<long long *>(S.d_work), S.d_st);
    SG_TRY(hipGetLastError());
    SG_TRY(hipEventRecord(S.ev[1], s));
    SG_TRY(hipMemcpyAsync(S.h_st, S.d_st, SGS_WORDS * 8, hipMemcpyDeviceToHost, s));
    SG_TRY(hipStreamSynchronize(s));
    if (S.h_st[SGS_BAD])
        return bpe_fail(BPE_ERR_ARG, "bpe native: text offsets must not decrease or be negative");
    J.pairs = (int64_t)S.h_st[SGS_PAIRS];
    J.values = (int64_t)S.h_st[SGS_VALUES];
    if (J.pairs < 0 || J.values < 0) return bpe_fail(BPE_ERR_ARG, "bpe native: skip-gram batch too large");
    if (J.values && !J.d_vals) return bpe_fail(BPE_ERR_ARG, "bpe native: null value buffer");
    float ms = 0;
    SG_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
    J.ms = ms;
    return BPE_OK;
}

// After sg_offsets: the offsets to J.d_poff, and the pairs to J.d_t / J.d_c when J.cap holds them.
inline int sg_expand(SgState &S, hipStream_t s, SgCall &J) {
    const int64_t n = J.n_texts;
    if (J.cap < 0 || (J.cap && (!J.d_t || !J.d_c)) || ((uintptr_t)J.d_t & 3) || ((uintptr_t)J.d_c & 3) ||
        ((uintptr_t)J.d_poff & 7))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram output arguments");
    if (J.d_poff) SG_TRY(hipMemcpyAsync(J.d_poff, J.d_scan, (size_t)(n + 1) * 8, hipMemcpyDeviceToDevice, s));
    J.fits = J.pairs <= J.cap;
    bool timed = false;
    if (J.fits && J.pairs) {
        const bool vec = ((uintptr_t)J.d_t & 15) == ((uintptr_t)J.d_c & 15);
        const int mis = vec ? (int)(((uintptr_t)J.d_t >> 2) & (SG_RUN - 1)) : 0;
        const int64_t n_tiles = (J.pairs + mis + SG_TILE - 1) / SG_TILE;
        if (n_tiles > 0x7FFFFFFF) return bpe_fail(BPE_ERR_ARG, "bpe native: skip-gram batch too large");
        SG_TRY(hipEventRecord(S.ev[2], s));
        if (vec)
            k_sg_expand<true><<<(unsigned)n_tiles, SG_WG, 0, s>>>(J.d_vals, J.d_off, J.d_scan, n, J.window, J.pairs, mis,
                                                                 J.d_t, J.d_c);
        else
            k_sg_expand<false><<<(unsigned)n_tiles, SG_WG, 0, s>>>(J.d_vals, J.d_off, J.d_scan, n, J.window, J.pairs, 0,
                                                                  J.d_t, J.d_c);
        SG_TRY(hipGetLastError());
        SG_TRY(hipEventRecord(S.ev[3], s));
        timed = true;
    }
    SG_TRY(hipStreamSynchronize(s));
    if (timed) {
        float ms = 0;
        SG_TRY(hipEventElapsedTime(&ms, S.ev[2], S.ev[3]));
        J.ms += ms;
    }
    return BPE_OK;
}

// After sg_offsets: the host form's outputs, through S.d_out.
inline int sg_to_host(SgState &S, hipStream_t s, SgCall &J, int32_t *targets, int32_t *contexts, int64_t cap,
                      int64_t *pair_off) {
    if (cap < 0 || !pair_off || (cap && (!targets || !contexts)))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram output arguments");
    const bool fits = J.pairs <= cap;
    const size_t b_plane = sg_align((size_t)(fits ? J.pairs : 0) * 4);
    int rc = sg_grow(s, &S.d_out, &S.out_cap, 2 * b_plane + 16);
    if (rc) return rc;
    J.d_t = reinterpret_cast<int32_t *>(S.d_out);
    J.d_c = reinterpret_cast<int32_t *>(S.d_out + b_plane);
    J.d_poff = nullptr;
    J.cap = fits ? J.pairs : 0;
    if (!fits) J.d_t = J.d_c = nullptr;
    if ((rc = sg_expand(S, s, J))) return rc;
    J.fits = fits;
    SG_TRY(hipMemcpyAsync(pair_off, J.d_scan, (size_t)(J.n_texts + 1) * 8, hipMemcpyDeviceToHost, s));
    if (fits && J.pairs) {
        SG_TRY(hipMemcpyAsync(targets, J.d_t, (size_t)J.pairs * 4, hipMemcpyDeviceToHost, s));
        SG_TRY(hipMemcpyAsync(contexts, J.d_c, (size_t)J.pairs * 4, hipMemcpyDeviceToHost, s));
    }
    SG_TRY(hipStreamSynchronize(s));
    J.cap = cap;
    return BPE_OK;
}

// A host batch into S.d_in: the values of its texts and the offsets rebased to them.  The offsets are
// checked here, before the values they name are read.
inline int sg_stage_host(SgState &S, hipStream_t s, const int32_t *vals, const int64_t *off, int64_t n, SgCall &J) {
    if (n < 0 || n >= 0x7FFFFFFF || (n && !off)) return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram batch arguments");
    if (n && off[0] < 0) return bpe_fail(BPE_ERR_ARG, "bpe native: text offsets must not decrease or be negative");
    for (int64_t k = 0; k < n; ++k)
        if (off[k + 1] < off[k]) return bpe_fail(BPE_ERR_ARG, "bpe native: text offsets must not decrease or be negative");
    const int64_t base = n ? off[0] : 0, total = n ? off[n] - base : 0;
    if (total && !vals) return bpe_fail(BPE_ERR_ARG, "bpe native: null value buffer");
    const size_t b_vals = sg_align((size_t)total * 4);
    int rc = sg_grow(s, &S.d_in, &S.in_cap, b_vals + sg_align((size_t)(n + 1) * 8));
    if (rc) return rc;
    int32_t *d_vals = reinterpret_cast<int32_t *>(S.d_in);
    int64_t *d_off = reinterpret_cast<int64_t *>(S.d_in + b_vals);
    std::vector<int64_t> rel((size_t)n + 1, 0);
    for (int64_t k = 0; k <= n && n; ++k) rel[(size_t)k] = off[k] - base;
    if (total) SG_TRY(hipMemcpyAsync(d_vals, vals + base, (size_t)total * 4, hipMemcpyHostToDevice, s));
    SG_TRY(hipMemcpyAsync(d_off, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
    SG_TRY(hipStreamSynchronize(s));   // (rel goes away)
    J.d_vals = d_vals, J.d_off = d_off, J.n_texts = n;
    return BPE_OK;
}

// the counters of a call that wrote its pairs
inline void sg_commit(SgState &S, const SgCall &J) {
    S.st.texts += J.n_texts;
    S.st.values_in += J.values;
    S.st.pairs_out += J.pairs;
    S.st.kernel_ms += J.ms;
}

inline int sg_cap_error(const SgCall &J) {
    char msg[128];
    std::snprintf(msg, sizeof msg, "bpe native: skip-gram needs %lld pairs, the buffers hold %lld", (long long)J.pairs,
                  (long long)J.cap);
    return bpe_fail(BPE_ERR_ARG, msg);
}

// The two whole forms over values that are already on the device (a pipeline's, or staged).
inline int sg_device_form(SgState &S, hipStream_t s, SgCall &J, int64_t *needed) {
    int rc = sg_offsets(S, s, J);
    if (rc) return rc;
    if ((rc = sg_expand(S, s, J))) return rc;
    *needed = J.pairs;
    if (!J.fits) return sg_cap_error(J);
    sg_commit(S, J);
    return BPE_OK;
}

inline int sg_host_form(SgState &S, hipStream_t s, SgCall &J, int32_t *targets, int32_t *contexts, int64_t cap,
                        int64_t *pair_off) {
    int rc = sg_offsets(S, s, J);
    if (rc) return rc;
    if ((rc = sg_to_host(S, s, J, targets, contexts, cap, pair_off))) return rc;
    if (!J.fits) return sg_cap_error(J);
    sg_commit(S, J);
    return BPE_OK;
}

}  // namespace
