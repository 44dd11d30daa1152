// bpe_skipgram_counts.hip.h — skip-gram pair counts on the device (include/bpe.h, "skip-gram pair
// counts"): a ragged batch of int32 values in [0, dim) -> every distinct (target, context) pair of
// the skip-gram rule (bpe_skipgram.hip.h) with the number of times it occurs, in ascending (target,
// context) order, as two int32 planes and one int64 plane.  For the two translation units that own
// such values (bpe_encode.hip, bpe_engine.hip); everything here has internal linkage.
//
// Input-centric, unlike k_sg_expand: the pairs are never written anywhere.
//
//   k_sg_offsets  (bpe_skipgram.hip.h, as it is) the offsets checked, P and the value span;
//   k_sgc_count   one workgroup per tile of BPE_SKIPGRAM_COUNTS_TILE consecutive positions of the
//                 flat value span plus w halo values to the right, staged into LDS by 16-B loads
//                 (head and tail of a tile whose address is not a multiple of 16 go value by value).
//                 Text starts inside tile and halo are bits of an LDS plane: two lanes bisect the
//                 offsets for the texts of the first and last staged position, the lanes stride over
//                 the texts between them, one bit-set each.  Position i then emits the forward keys
//                 v[i] * dim + v[i + d], d = 1 .. min(w, zeros after bit i of the plane): no loop
//                 over texts, no bisection per pair.  The other direction is the transpose.  Keys go
//                 into an open-addressing LDS table of BPE_SKIPGRAM_COUNTS_SLOTS slots (u32 key
//                 claimed by compare-and-swap, u32 count); a key without a slot within SGC_PROBES
//                 probes goes to its global cell by one 64-bit atomic add.  At the tile's end every
//                 used slot leaves as one 64-bit atomic add into the dense accumulator F[dim * dim].
//                 A value outside [0, dim) raises a flag and the minimum of its flat position; its
//                 pairs are skipped (so no key ever leaves F);
//   k_sgc_sym     C = F + F^T in place, 64 x 64 cells per tile through LDS: one workgroup owns the
//                 tiles (I, J) and (J, I), I <= J, reads both in rows, transposes through LDS and
//                 writes both in rows;
//   k_sgc_census  nonzero cells per block of SGC_BLOCK consecutive row-major cells;
//   k_sgc_scan    one workgroup: the exclusive scan of the block counts, and U;
//   k_sgc_emit    one workgroup per block with nonzeros: ranks them by ballot, packs target, context
//                 and count in LDS, and stores each plane by 16 B from its first 16-B address on
//                 (the elements before it and the rest after the last whole store go one by one).
//                 Row-major cell order is ascending (target, context): nothing is sorted.
#pragma once

#include "bpe_skipgram.hip.h"

namespace {

constexpr int SGC_TILE = BPE_SKIPGRAM_COUNTS_TILE;
constexpr int SGC_SLOTS = BPE_SKIPGRAM_COUNTS_SLOTS;
constexpr int SGC_WG = 256;
constexpr int SGC_STAGE = SGC_TILE + BPE_SKIPGRAM_MAX_WINDOW + 4;       // tile, halo, up to 3 values of misalignment
constexpr int SGC_PLANE_WORDS = (SGC_TILE + BPE_SKIPGRAM_MAX_WINDOW) / 32 + 4;   // ... and the words a 64-bit mask read touches
constexpr int SGC_PROBES = 8;
constexpr uint32_t SGC_EMPTY = 0xFFFFFFFFu;                             // (keys are < 2^28)
constexpr int SGC_SYM = 64;                                             // cells per side of a k_sgc_sym tile
constexpr int SGC_BLOCK = 2048;                                         // cells per block of census and emit
constexpr int SGC_EACH = SGC_BLOCK / SGC_WG;
static_assert(SGC_TILE % SGC_WG == 0 && SGC_TILE % 32 == 0, "whole positions per lane, whole mask words");
static_assert((SGC_SLOTS & (SGC_SLOTS - 1)) == 0, "the table is indexed by a mask");
static_assert((long long)BPE_SKIPGRAM_COUNTS_MAX_DIM * BPE_SKIPGRAM_COUNTS_MAX_DIM <= (1ll << 28), "keys fit 28 bits");
static_assert((long long)SGC_TILE * BPE_SKIPGRAM_MAX_WINDOW < (1ll << 32), "a slot's count fits 32 bits");
static_assert(SGC_STAGE * 4 + SGC_PLANE_WORDS * 4 + SGC_SLOTS * 8 <= 64 * 1024, "LDS of k_sgc_count");
// status words of a call on the device
constexpr int SGCS_BAD = 0;        // nonzero: a value outside [0, dim)
constexpr int SGCS_POS = 1;        // ... the smallest flat position (from off[0]) of one
constexpr int SGCS_OVERFLOW = 2;   // keys that went past the LDS table
constexpr int SGCS_DISTINCT = 3;   // U
constexpr int SGCS_WORDS = 4;

__global__ void k_sgc_init(unsigned long long *__restrict__ st) {
    if (threadIdx.x < SGCS_WORDS) st[threadIdx.x] = threadIdx.x == SGCS_POS ? ~0ull : 0ull;
}

// the largest k in [0, n] with off[k] <= pos (off[0] <= pos)
__device__ __forceinline__ int64_t sgc_text_of(const int64_t *__restrict__ off, int64_t n, int64_t pos) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= pos) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// (the product's top bits: the slot of a key)
__device__ __forceinline__ uint32_t sgc_hash(uint32_t key) {
    return (key * 0x9E3779B1u) >> (32 - __builtin_ctz((unsigned)SGC_SLOTS));
}

__global__ void __launch_bounds__(SGC_WG)
k_sgc_count(const int32_t *__restrict__ vals, const int64_t *__restrict__ off, int64_t n_texts, int w, int dim,
            unsigned long long *__restrict__ F, unsigned long long *__restrict__ st) {
    __shared__ int32_t s_v[SGC_STAGE];
    __shared__ uint32_t s_bits[SGC_PLANE_WORDS];
    __shared__ uint32_t s_key[SGC_SLOTS], s_cnt[SGC_SLOTS];
    __shared__ long long s_k[2];
    const int tid = threadIdx.x;
    const int64_t begin = off[0], end = off[n_texts];
    const int64_t base = begin + (int64_t)blockIdx.x * SGC_TILE;   // the tile's first position in vals
    const int n_tile = (int)(end - base < SGC_TILE ? end - base : SGC_TILE);           // targets
    const int n_stage = (int)(end - base < SGC_TILE + w ? end - base : SGC_TILE + w);  // ... and halo
    // ---- the table and the plane cleared, the two texts found
    for (int i = tid; i < SGC_SLOTS; i += SGC_WG) s_key[i] = SGC_EMPTY, s_cnt[i] = 0;
    for (int i = tid; i < SGC_PLANE_WORDS; i += SGC_WG) s_bits[i] = 0;
    if (tid < 2) s_k[tid] = sgc_text_of(off, n_texts, tid ? base + n_stage - 1 : base);
    // ---- staging: s_v[mis + i] = vals[base + i]; a value outside [0, dim) becomes -1
    const int mis = (int)(((uintptr_t)(vals + base) >> 2) & 3);
    bool bad = false;
    int64_t bad_pos = 0;
    for (int q = tid; q * 4 < mis + n_stage; q += SGC_WG) {
        const int64_t g = base - mis + (int64_t)q * 4;
        int32_t x[4] = {-1, -1, -1, -1};
        if (g >= begin && g + 4 <= end) {
            const int4 v = *reinterpret_cast<const int4 *>(vals + g);
            x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (g + e >= begin && g + e < end) x[e] = vals[g + e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = q * 4 + e - mis;   // the place in the tile
            if (i >= 0 && i < n_stage && (uint32_t)x[e] >= (uint32_t)dim) {
                if (i < n_tile && !bad) bad = true, bad_pos = g + e - begin;   // (every value is one tile's target)
                x[e] = -1;
            }
            s_v[q * 4 + e] = x[e];
        }
    }
    if (bad) {
        st[SGCS_BAD] = 1ull;   // (every writer stores the same word)
        atomicMin(&st[SGCS_POS], (unsigned long long)bad_pos);
    }
    __syncthreads();
    // ---- text starts (and the end of the batch) inside tile and halo
    const int64_t klo = s_k[0], khi = s_k[1] + 1 < n_texts ? s_k[1] + 1 : n_texts;
    for (int64_t k = klo + tid; k <= khi; k += SGC_WG) {
        const int64_t p = off[k] - base;
        if (p >= 0 && p <= n_stage) {
            const uint32_t bit = 1u << (p & 31);
            if (!(*(volatile uint32_t *)&s_bits[p >> 5] & bit)) atomicOr(&s_bits[p >> 5], bit);
        }
    }
    __syncthreads();
    // ---- the forward half into the table
    unsigned int past = 0;
    for (int i = tid; i < n_tile; i += SGC_WG) {
        const int32_t x = s_v[mis + i];
        if (x < 0) continue;
        // bits i + 1 .. i + 64 of the plane: the next text starts after as many zeros
        const int b = i + 1, wd = b >> 5, sh = b & 31;
        unsigned long long m = ((unsigned long long)s_bits[wd] | ((unsigned long long)s_bits[wd + 1] << 32)) >> sh;
        if (sh) m |= (unsigned long long)s_bits[wd + 2] << (64 - sh);
        const int room = m ? __builtin_ctzll(m) : 64;
        const int lim = room < w ? room : w;
        const uint32_t row = (uint32_t)x * (uint32_t)dim;
        for (int d = 1; d <= lim; ++d) {
            const int32_t y = s_v[mis + i + d];
            if (y < 0) continue;
            const uint32_t key = row + (uint32_t)y;
            uint32_t h = sgc_hash(key) & (SGC_SLOTS - 1);
            bool done = false;
            for (int t = 0; t < SGC_PROBES; ++t) {
                uint32_t old = *(volatile uint32_t *)&s_key[h];
                if (old == SGC_EMPTY) old = atomicCAS(&s_key[h], SGC_EMPTY, key);
                if (old == SGC_EMPTY || old == key) {
                    atomicAdd(&s_cnt[h], 1u);
                    done = true;
                    break;
                }
                h = (h + 1) & (SGC_SLOTS - 1);
            }
            if (!done) {
                atomicAdd(&F[key], 1ull);
                ++past;
            }
        }
    }
    if (past) atomicAdd(&st[SGCS_OVERFLOW], (unsigned long long)past);
    __syncthreads();
    // ---- the table out
    for (int i = tid; i < SGC_SLOTS; i += SGC_WG) {
        const uint32_t key = s_key[i];
        if (key != SGC_EMPTY) atomicAdd(&F[key], (unsigned long long)s_cnt[i]);
    }
}

// C = F + F^T in place.  blockIdx (x, y) = tiles (J, I); the blocks below the diagonal have nothing to do.
__global__ void __launch_bounds__(SGC_WG)
k_sgc_sym(unsigned long long *__restrict__ F, int dim) {
    __shared__ unsigned long long s[SGC_SYM][SGC_SYM + 1];
    const int I = blockIdx.y, J = blockIdx.x;
    if (I > J) return;
    constexpr int EACH = SGC_SYM * SGC_SYM / SGC_WG;
    unsigned long long a[EACH], b[EACH];
    const int r0 = I * SGC_SYM, c0 = J * SGC_SYM;
#pragma unroll
    for (int k = 0; k < EACH; ++k) {
        const int e = k * SGC_WG + threadIdx.x, r = e >> 6, c = e & 63;
        // a: cell (r0 + r, c0 + c) of tile (I, J); b: cell (c0 + r, r0 + c) of tile (J, I)
        a[k] = r0 + r < dim && c0 + c < dim ? F[(size_t)(r0 + r) * dim + c0 + c] : 0ull;
        b[k] = c0 + r < dim && r0 + c < dim ? F[(size_t)(c0 + r) * dim + r0 + c] : 0ull;
        s[r][c] = b[k];
    }
    __syncthreads();
    unsigned long long bt[EACH];
#pragma unroll
    for (int k = 0; k < EACH; ++k) {
        const int e = k * SGC_WG + threadIdx.x, r = e >> 6, c = e & 63;
        bt[k] = s[c][r];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EACH; ++k) {
        const int e = k * SGC_WG + threadIdx.x, r = e >> 6, c = e & 63;
        s[r][c] = a[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EACH; ++k) {
        const int e = k * SGC_WG + threadIdx.x, r = e >> 6, c = e & 63;
        const unsigned long long at = s[c][r];
        if (r0 + r < dim && c0 + c < dim) F[(size_t)(r0 + r) * dim + c0 + c] = a[k] + bt[k];
        if (I != J && c0 + r < dim && r0 + c < dim) F[(size_t)(c0 + r) * dim + r0 + c] = b[k] + at;
    }
}

__global__ void __launch_bounds__(SGC_WG)
k_sgc_census(const unsigned long long *__restrict__ F, int64_t cells, uint32_t *__restrict__ blk) {
    __shared__ int ws[SGC_WG / 64];
    const int64_t c0 = (int64_t)blockIdx.x * SGC_BLOCK;
    int mine = 0;
    // (F sits at a 16-B address and blocks hold an even number of cells: two cells per load)
#pragma unroll
    for (int k = 0; k < SGC_EACH / 2; ++k) {
        const int64_t c = c0 + (int64_t)(k * SGC_WG + threadIdx.x) * 2;
        if (c + 2 <= cells) {
            const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(F + c);
            mine += (v.x != 0) + (v.y != 0);
        } else if (c < cells) {
            mine += F[c] != 0;
        }
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) mine += __shfl_down(mine, d);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = (uint32_t)(ws[0] + ws[1] + ws[2] + ws[3]);
}

__global__ void __launch_bounds__(1024)
k_sgc_scan(const uint32_t *__restrict__ blk, int64_t n_blocks, unsigned long long *__restrict__ blk_off,
           unsigned long long *__restrict__ st) {
    __shared__ unsigned long long ws[16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (int64_t b = 0; b < n_blocks; b += 1024) {
        const int64_t i = b + threadIdx.x;
        const unsigned long long mine = i < n_blocks ? blk[i] : 0;
        const unsigned long long incl = txt_wave_incl64(mine, lane);
        if (lane == 63) ws[wv] = incl;
        __syncthreads();
        unsigned long long before = 0, all = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned long long x = ws[j];
            before += j < wv ? x : 0;
            all += x;
        }
        if (i < n_blocks) blk_off[i] = carry + before + incl - mine;
        carry += all;
        __syncthreads();   // (ws is reused next round)
    }
    if (threadIdx.x == 0) st[SGCS_DISTINCT] = carry;
}

// n elements from LDS to dst[0 .. n): 16-B stores from dst's first 16-B address on, the rest one by one
template <typename T>
__device__ __forceinline__ void sgc_store(T *__restrict__ dst, const T *s, int n) {
    constexpr int PER = 16 / (int)sizeof(T);
    int head = (int)(((16 - ((uintptr_t)dst & 15)) & 15) / sizeof(T));
    if (head > n) head = n;
    const int n_vec = (n - head) / PER;
    for (int i = threadIdx.x; i < head; i += SGC_WG) dst[i] = s[i];
    for (int q = threadIdx.x; q < n_vec; q += SGC_WG) {
        T x[PER];
#pragma unroll
        for (int e = 0; e < PER; ++e) x[e] = s[head + q * PER + e];
        int4 v;
        __builtin_memcpy(&v, x, 16);
        *reinterpret_cast<int4 *>(dst + head + q * PER) = v;
    }
    for (int i = head + n_vec * PER + threadIdx.x; i < n; i += SGC_WG) dst[i] = s[i];
}

__global__ void __launch_bounds__(SGC_WG)
k_sgc_emit(const unsigned long long *__restrict__ F, int64_t cells, int dim, const uint32_t *__restrict__ blk,
           const unsigned long long *__restrict__ blk_off, int32_t *__restrict__ tg, int32_t *__restrict__ cx,
           long long *__restrict__ cn) {
    __shared__ int32_t s_t[SGC_BLOCK], s_c[SGC_BLOCK];
    __shared__ long long s_n[SGC_BLOCK];
    __shared__ int s_pre[SGC_EACH * (SGC_WG / 64)];
    const int total = (int)blk[blockIdx.x];
    if (!total) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * SGC_BLOCK;
    unsigned long long v[SGC_EACH];
    unsigned long long ball[SGC_EACH];
#pragma unroll
    for (int k = 0; k < SGC_EACH; ++k) {
        const int64_t c = c0 + k * SGC_WG + threadIdx.x;
        v[k] = c < cells ? F[c] : 0ull;
        ball[k] = __ballot(v[k] != 0);
        if (lane == 0) s_pre[k * (SGC_WG / 64) + wv] = __popcll(ball[k]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int j = 0; j < SGC_EACH * (SGC_WG / 64); ++j) {
            const int x = s_pre[j];
            s_pre[j] = run;
            run += x;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SGC_EACH; ++k) {
        if (!v[k]) continue;
        const int64_t c = c0 + k * SGC_WG + threadIdx.x;
        const int rank = s_pre[k * (SGC_WG / 64) + wv] + __popcll(ball[k] & ((1ull << lane) - 1));
        if (rank < SGC_BLOCK) {   // (always: a block has SGC_BLOCK cells)
            s_t[rank] = (int32_t)(c / dim);
            s_c[rank] = (int32_t)(c % dim);
            s_n[rank] = (long long)v[k];
        }
    }
    __syncthreads();
    const unsigned long long o = blk_off[blockIdx.x];
    sgc_store(tg + o, s_t, total);
    sgc_store(cx + o, s_c, total);
    sgc_store(cn + o, s_n, total);
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------------

// The accumulator, the census' block counts and offsets, status words, events and counters of the
// pair counts of an encoder or a context, beside its SgState (whose `in`, `work` and `out` buffers
// and offsets kernel the counts use as the pairs do).  Grow-only.
struct SgcState {
    char *d_f = nullptr, *d_blk = nullptr;
    size_t f_cap = 0, blk_cap = 0;
    unsigned long long *d_st = nullptr, *h_st = nullptr;   // (h_st pinned)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bpe_skipgram_counts_stats st{};
};

// One call's counts: J (the batch, as for the pairs) plus these.
struct SgcCall {
    int dim = 0;
    int32_t *d_t = nullptr, *d_c = nullptr;   // the planes on the device (cap elements each)
    int64_t *d_n = nullptr;
    int64_t cap = 0;
    // out
    int64_t distinct = 0, overflow = 0;
    bool fits = true;
    double ms = 0;
};

namespace {

inline void sgc_free(SgcState &C) {
    if (C.d_f) (void)hipFree(C.d_f);
    if (C.d_blk) (void)hipFree(C.d_blk);
    if (C.d_st) (void)hipFree(C.d_st);
    if (C.h_st) (void)hipHostFree(C.h_st);
    for (hipEvent_t &ev : C.ev)
        if (ev) (void)hipEventDestroy(ev);
    C = SgcState{};
}

inline int sgc_check_dim(int dim) {
    if (dim >= 1 && dim <= BPE_SKIPGRAM_COUNTS_MAX_DIM) return BPE_OK;
    char msg[96];
    std::snprintf(msg, sizeof msg, "bpe native: skip-gram counts dim %d outside [1, %d]", dim, BPE_SKIPGRAM_COUNTS_MAX_DIM);
    return bpe_fail(BPE_ERR_ARG, msg);
}

inline bool sgc_outputs_ok(const void *t, const void *c, const void *n, int64_t cap, const void *needed) {
    return cap >= 0 && needed && (!cap || (t && c && n));
}

// a value outside [0, dim): the message names it, its text and its place there
inline int sgc_range_error(hipStream_t s, const SgCall &J, int dim, int64_t pos) {
    std::vector<int64_t> off((size_t)J.n_texts + 1);
    int32_t v = 0;
    SG_TRY(hipMemcpyAsync(off.data(), J.d_off, off.size() * 8, hipMemcpyDeviceToHost, s));
    SG_TRY(hipStreamSynchronize(s));
    SG_TRY(hipMemcpyAsync(&v, J.d_vals + off[0] + pos, 4, hipMemcpyDeviceToHost, s));
    SG_TRY(hipStreamSynchronize(s));
    const int64_t k = (std::upper_bound(off.begin(), off.end(), off[0] + pos) - off.begin()) - 1;
    char msg[160];
    std::snprintf(msg, sizeof msg, "bpe native: skip-gram counts value %d outside [0, %d) (text %lld, position %lld)",
                  (int)v, dim, (long long)k, (long long)(off[0] + pos - off[(size_t)k]));
    return bpe_fail(BPE_ERR_ARG, msg);
}

// J.d_vals / J.d_off / J.n_texts / J.window set: the offsets checked, the pairs counted into F, F made
// symmetric, U found; then, when K.cap holds them, the planes written.  Nothing is written to K's
// planes before the range check and the capacity check.
inline int sgc_run(SgState &S, SgcState &C, hipStream_t s, SgCall &J, SgcCall &K) {
    int rc = sg_check_window(J.window);
    if (rc || (rc = sgc_check_dim(K.dim))) return rc;
    if (K.cap < 0 || (K.cap && (!K.d_t || !K.d_c || !K.d_n)) || ((uintptr_t)K.d_t & 3) || ((uintptr_t)K.d_c & 3) ||
        ((uintptr_t)K.d_n & 7))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram counts output arguments");
    if ((rc = sg_offsets(S, s, J))) return rc;
    K.distinct = K.overflow = 0;
    K.fits = true;
    K.ms = J.ms;
    if (!J.values) return BPE_OK;
    if (!C.d_st) SG_TRY(hipMalloc((void **)&C.d_st, SGCS_WORDS * 8));
    if (!C.h_st) SG_TRY(hipHostMalloc((void **)&C.h_st, SGCS_WORDS * 8, hipHostMallocDefault));
    for (hipEvent_t &ev : C.ev)
        if (!ev) SG_TRY(hipEventCreate(&ev));
    const int64_t cells = (int64_t)K.dim * K.dim, n_blocks = (cells + SGC_BLOCK - 1) / SGC_BLOCK;
    const int64_t n_tiles = (J.values + SGC_TILE - 1) / SGC_TILE;
    if (n_tiles > 0x7FFFFFFF) return bpe_fail(BPE_ERR_ARG, "bpe native: skip-gram batch too large");
    const size_t b_cnt = sg_align((size_t)n_blocks * 4);
    if ((rc = sg_grow(s, &C.d_f, &C.f_cap, (size_t)cells * 8))) return rc;
    if ((rc = sg_grow(s, &C.d_blk, &C.blk_cap, b_cnt + (size_t)n_blocks * 8))) return rc;
    unsigned long long *F = reinterpret_cast<unsigned long long *>(C.d_f);
    uint32_t *blk = reinterpret_cast<uint32_t *>(C.d_blk);
    unsigned long long *blk_off = reinterpret_cast<unsigned long long *>(C.d_blk + b_cnt);
    SG_TRY(hipEventRecord(C.ev[0], s));
    SG_TRY(hipMemsetAsync(F, 0, (size_t)cells * 8, s));
    k_sgc_init<<<1, 64, 0, s>>>(C.d_st);
    k_sgc_count<<<(unsigned)n_tiles, SGC_WG, 0, s>>>(J.d_vals, J.d_off, J.n_texts, J.window, K.dim, F, C.d_st);
    SG_TRY(hipGetLastError());
    if (J.pairs) {
        const unsigned nt = (unsigned)((K.dim + SGC_SYM - 1) / SGC_SYM);
        k_sgc_sym<<<dim3(nt, nt), SGC_WG, 0, s>>>(F, K.dim);
        k_sgc_census<<<(unsigned)n_blocks, SGC_WG, 0, s>>>(F, cells, blk);
        k_sgc_scan<<<1, 1024, 0, s>>>(blk, n_blocks, blk_off, C.d_st);
        SG_TRY(hipGetLastError());
    }
    SG_TRY(hipEventRecord(C.ev[1], s));
    SG_TRY(hipMemcpyAsync(C.h_st, C.d_st, SGCS_WORDS * 8, hipMemcpyDeviceToHost, s));
    SG_TRY(hipStreamSynchronize(s));
    if (C.h_st[SGCS_BAD]) return sgc_range_error(s, J, K.dim, (int64_t)C.h_st[SGCS_POS]);
    float ms = 0;
    SG_TRY(hipEventElapsedTime(&ms, C.ev[0], C.ev[1]));
    K.ms += ms;
    K.distinct = (int64_t)C.h_st[SGCS_DISTINCT];
    K.overflow = (int64_t)C.h_st[SGCS_OVERFLOW];
    K.fits = K.distinct <= K.cap;
    if (!K.fits || !K.distinct) return BPE_OK;
    SG_TRY(hipEventRecord(C.ev[2], s));
    k_sgc_emit<<<(unsigned)n_blocks, SGC_WG, 0, s>>>(F, cells, K.dim, blk, blk_off, K.d_t, K.d_c,
                                                    reinterpret_cast<long long *>(K.d_n));
    SG_TRY(hipGetLastError());
    SG_TRY(hipEventRecord(C.ev[3], s));
    SG_TRY(hipStreamSynchronize(s));
    SG_TRY(hipEventElapsedTime(&ms, C.ev[2], C.ev[3]));
    K.ms += ms;
    return BPE_OK;
}

inline int sgc_finish(SgcState &C, const SgCall &J, const SgcCall &K) {
    if (!K.fits) {
        char msg[128];
        std::snprintf(msg, sizeof msg, "bpe native: skip-gram counts need %lld distinct pairs, the buffers hold %lld",
                      (long long)K.distinct, (long long)K.cap);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    C.st.texts += J.n_texts;
    C.st.values_in += J.values;
    C.st.pairs_counted += J.pairs;
    C.st.distinct_out += K.distinct;
    C.st.lds_overflow += K.overflow;
    C.st.kernel_ms += K.ms;
    return BPE_OK;
}

// The two whole forms over values that are already on the device (a pipeline's, or staged).
inline int sgc_device_form(SgState &S, SgcState &C, hipStream_t s, SgCall &J, int dim, int32_t *d_t, int32_t *d_c,
                           int64_t *d_n, int64_t cap, int64_t *needed) {
    SgcCall K;
    K.dim = dim, K.cap = cap;
    if (cap) K.d_t = d_t, K.d_c = d_c, K.d_n = d_n;
    int rc = sgc_run(S, C, s, J, K);
    if (rc) return rc;
    *needed = K.distinct;
    return sgc_finish(C, J, K);
}

inline int sgc_host_form(SgState &S, SgcState &C, hipStream_t s, SgCall &J, int dim, int32_t *targets, int32_t *contexts,
                         int64_t *counts, int64_t cap, int64_t *needed) {
    // the planes in S.d_out: [counts | targets | contexts], cap elements each but no more than dim^2
    const int64_t room = std::min<int64_t>(cap, (int64_t)(dim > 0 ? dim : 0) * dim);
    const size_t b32 = sg_align((size_t)room * 4);
    int rc = sgc_check_dim(dim);
    if (rc || (rc = sg_grow(s, &S.d_out, &S.out_cap, sg_align((size_t)room * 8) + 2 * b32 + 16))) return rc;
    SgcCall K;
    K.dim = dim, K.cap = room;
    if (room) {
        K.d_n = reinterpret_cast<int64_t *>(S.d_out);
        K.d_t = reinterpret_cast<int32_t *>(S.d_out + sg_align((size_t)room * 8));
        K.d_c = reinterpret_cast<int32_t *>(S.d_out + sg_align((size_t)room * 8) + b32);
    }
    if ((rc = sgc_run(S, C, s, J, K))) return rc;
    *needed = K.distinct;
    K.cap = cap;
    if (K.fits && K.distinct) {
        SG_TRY(hipMemcpyAsync(targets, K.d_t, (size_t)K.distinct * 4, hipMemcpyDeviceToHost, s));
        SG_TRY(hipMemcpyAsync(contexts, K.d_c, (size_t)K.distinct * 4, hipMemcpyDeviceToHost, s));
        SG_TRY(hipMemcpyAsync(counts, K.d_n, (size_t)K.distinct * 8, hipMemcpyDeviceToHost, s));
        SG_TRY(hipStreamSynchronize(s));
    }
    return sgc_finish(C, J, K);
}

}  // namespace
