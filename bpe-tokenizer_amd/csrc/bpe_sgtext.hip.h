// bpe_sgtext.hip.h — the skip-gram model over texts (include/bpe.h, "skip-gram model over texts"): one pooled
// embedding per text and the log-likelihood of a text's skip-gram pairs, as ragged reductions over the
// encoder's (vals, off) output with the gathers going into the V x E tables.  Part of bpe_sgmodel.hip's
// translation unit (its struct, SGM_TRY, sgm_grow, sgm_time, sgq_run and the lane-group helpers of
// bpe_glove.hip.h, glv_load4 / glv_store4 / glv_group_sum, are in scope).  DESIGN.md §3v.
//
// The work is split by text, not by flat position: a text is cut into chunks of SGT_CHUNK of its own values
// counted from its start, an item is one (text, chunk), an empty text is one item.  Every sum below is taken
// in an order that depends on the text alone, so a text's answer is the same bytes whatever else is in the
// batch, whatever off[0] is and in both forms.
//
//   k_sgt_items   one workgroup: the offsets checked (non-negative, non-decreasing), each text's items and,
//                 for the texts of more than one chunk, its partial slots, both scanned; the totals, the
//                 value span and the pairs of the batch go to the header words;
//   k_sgt_check   the values against [0, V): the smallest offending flat position by an integer atomicMin.
//                 A pass of its own (4 bytes per value beside the >= 200 a gather costs) in front of the
//                 compute kernels and not part of their staging, because a single-chunk text stores its
//                 result at once and a refused call writes nothing to the caller;
//   k_sgt_pool<EP>   a lane group of EP / 4 lanes owns one item (four groups to a wave at EP = 64, two at 128,
//                 one at 256; a workgroup is four waves: 16, 8 or 4 items).  A wave inverts its items to
//                 (text, chunk) by bisection of the scanned counts, stages their values coalesced into LDS, a
//                 value per lane, each with its weight beside it, and the groups walk their chunks from LDS:
//                 four rows Ein[v] gathered (a lane holds elements 4l .. 4l + 3; 16-, 8- or 4-byte loads by
//                 E's divisibility) before the first is used, acc += w fl32(Ein[v] + b1) and the weight sum
//                 in value order.  A single-chunk text is scaled and stored at once; a chunk of a longer text
//                 goes to its partial slot;
//   k_sgt_score<EP>  the same split.  The staged values have up to `window` halo values on each side, clipped
//                 to the text.  For each target of the chunk X_t stays in registers, the Eout rows of its
//                 contexts are gathered four at a time, each dot is reduced inside the group by DPP, and
//                 fl32(fl32(dot + b2[c]) - lse_t) is added to the item's double in (target, context) order;
//   k_sgt_fold    only when a text has more than SGT_FOLD chunks: the first partial of every SGT_FOLD adds the
//                 ones behind it, in chunk order, into itself;
//   k_sgt_pool_finish / k_sgt_score_finish   a text of several chunks: its partials (every SGT_FOLD-th after
//                 k_sgt_fold, which is the same order of additions) in chunk order, scaled and stored.
// lse comes from the predict forward as it is (sgq_run over the ids 0 .. V - 1, k = 1) once per call.
// No floating-point atomics and no order that depends on the launch: the same bytes on every run.

#include "bpe_skipgram_rule.h"   // sg_text_pairs

namespace {

constexpr int SGT_CHUNK = BPE_SGM_TEXT_CHUNK;   // values of a chunk
constexpr int SGT_WG = 256;
constexpr int SGT_FOLD = BPE_SGM_TEXT_FOLD;                  // partials one wave of k_sgt_fold adds
constexpr int SGT_STAGE = SGT_CHUNK + 2 * BPE_SKIPGRAM_MAX_WINDOW;   // a chunk and its halos
constexpr int SGT_SCAN_EACH = 4;                // texts per thread and round of k_sgt_items
constexpr int SGT_CHECK_BLOCKS = 1024;
// header words of a call on the device
constexpr int SGTH_ERR = 0;      // the smallest flat position (from off[0]) of a value outside [0, V)
constexpr int SGTH_BAD = 1;      // nonzero: an offset is negative or smaller than the one before it
constexpr int SGTH_ITEMS = 2;
constexpr int SGTH_MULTI = 3;    // partial slots: the chunks of the texts that have more than one
constexpr int SGTH_VALUES = 4;   // off[n_texts] - off[0]
constexpr int SGTH_PAIRS = 5;    // the pairs of the batch (score)
constexpr int SGTH_WORDS = 8;
static_assert(SGT_CHUNK % 4 == 0, "values are walked four at a time");

struct sgt_args {
    const float *Ein, *b1, *Eout, *b2, *lse, *w;
    int V, E, pool, window, vm;   // vm: floats per store to the caller's rows (4, 2 or 1)
    const int32_t *vals;
    const int64_t *off;
    int64_t n_texts, n_items, n_multi;
    const long long *ioff, *moff;   // [n_texts + 1]: items and partial slots before a text
    float *out;                     // pool: [n_texts][E]
    double *sum;                    // score: [n_texts]
    int64_t *pairs;
    float *part_row, *part_w;       // [n_multi][E], [n_multi]
    double *part_sum;               // [n_multi]
    long long *slot_text;           // [n_multi]: the text of a partial slot
};

__device__ __forceinline__ unsigned long long sgt_wave_incl(unsigned long long v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long x = __shfl_up(v, o, 64);
        if (lane >= o) v += x;
    }
    return v;
}

__device__ __forceinline__ long long sgt_chunks(int64_t len) { return len <= 0 ? 1 : (len + SGT_CHUNK - 1) / SGT_CHUNK; }

__global__ __launch_bounds__(1024) void k_sgt_items(const int64_t *__restrict__ off, int64_t n_texts, int w,
                                                    long long *__restrict__ ioff, long long *__restrict__ moff,
                                                    unsigned long long *hdr) {
    __shared__ unsigned long long ws[2][16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long carry_i = 0, carry_m = 0, pairs = 0;
    bool bad = false;
    for (int64_t b = 0; b < n_texts; b += 1024 * SGT_SCAN_EACH) {
        const int64_t i0 = b + (int64_t)threadIdx.x * SGT_SCAN_EACH;
        unsigned long long v[SGT_SCAN_EACH], mine_i = 0, mine_m = 0;
        int64_t a = i0 < n_texts ? off[i0] : 0;
#pragma unroll
        for (int e = 0; e < SGT_SCAN_EACH; ++e) {
            v[e] = 0;
            if (i0 + e < n_texts) {
                const int64_t z = off[i0 + e + 1];
                v[e] = 1;
                if (a < 0 || z < a) {
                    bad = true;
                } else {
                    v[e] = (unsigned long long)sgt_chunks(z - a);
                    if (w) pairs += (unsigned long long)sg_text_pairs(z - a, w);
                }
                a = z;
            }
            mine_i += v[e];
            mine_m += v[e] > 1 ? v[e] : 0;
        }
        const unsigned long long incl_i = sgt_wave_incl(mine_i, lane), incl_m = sgt_wave_incl(mine_m, lane);
        if (lane == 63) ws[0][wv] = incl_i, ws[1][wv] = incl_m;
        __syncthreads();
        unsigned long long before_i = 0, before_m = 0, all_i = 0, all_m = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const unsigned long long x = ws[0][i], y = ws[1][i];
            before_i += i < wv ? x : 0;
            before_m += i < wv ? y : 0;
            all_i += x;
            all_m += y;
        }
        unsigned long long pre_i = carry_i + before_i + incl_i - mine_i, pre_m = carry_m + before_m + incl_m - mine_m;
#pragma unroll
        for (int e = 0; e < SGT_SCAN_EACH; ++e) {
            if (i0 + e < n_texts) {
                ioff[i0 + e] = (long long)pre_i;
                moff[i0 + e] = (long long)pre_m;
            }
            pre_i += v[e];
            pre_m += v[e] > 1 ? v[e] : 0;
        }
        carry_i += all_i;
        carry_m += all_m;
        __syncthreads();   // (ws is reused next round)
    }
    if (bad) hdr[SGTH_BAD] = 1ull;   // (every writer stores the same word)
    if (pairs) atomicAdd(&hdr[SGTH_PAIRS], pairs);
    if (threadIdx.x == 0) {
        ioff[n_texts] = (long long)carry_i;
        moff[n_texts] = (long long)carry_m;
        hdr[SGTH_ITEMS] = carry_i;
        hdr[SGTH_MULTI] = carry_m;
        hdr[SGTH_VALUES] = (unsigned long long)(off[n_texts] - off[0]);
    }
}

// (behind k_sgt_items on the stream: offsets that are not in order are never used as a span)
__global__ __launch_bounds__(256) void k_sgt_check(const int32_t *__restrict__ vals, const int64_t *__restrict__ off,
                                                   int64_t n_texts, int V, unsigned long long *hdr) {
    if (hdr[SGTH_BAD] || !vals) return;
    const int64_t begin = off[0], end = off[n_texts], stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < end; i += stride)
        if ((uint32_t)vals[i] >= (uint32_t)V) atomicMin(&hdr[SGTH_ERR], (unsigned long long)(i - begin));
}

// the text of item q: the largest k in [0, n) with ioff[k] <= q (every text has an item, so ioff ascends strictly)
__device__ __forceinline__ int64_t sgt_text_of(const long long *__restrict__ ioff, int64_t n, int64_t q) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (ioff[mid] <= q) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// where a group's item is: text k of nch chunks and len values, chunk `chunk` with n_e values, the first of
// them at t0 of the n_st values staged for the group
struct sgt_item {
    long long k, chunk, nch, len;
    int n_e, t0, n_st, pad;
};

// a wave stages its items' values (the chunk and `halo` values on each side, clipped to the text): a value per
// lane, with its weight beside it when REC is int2
template <class REC, int GW, int ST>
__device__ __forceinline__ void sgt_stage(const sgt_args &a, int64_t item0, int halo, REC *wrec, sgt_item *wit, int lane) {
    for (int g = 0; g < GW; ++g) {
        const int64_t item = item0 + g;
        if (item >= a.n_items) break;   // (uniform)
        sgt_item it;
        it.k = sgt_text_of(a.ioff, a.n_texts, item);
        const int64_t base = a.off[it.k];
        it.len = a.off[it.k + 1] - base;
        it.chunk = item - a.ioff[it.k];
        it.nch = a.ioff[it.k + 1] - a.ioff[it.k];
        const int64_t c0 = it.chunk * SGT_CHUNK;
        const int64_t left = it.len - c0;
        it.n_e = (int)(left < SGT_CHUNK ? left : SGT_CHUNK);
        const int64_t hs = c0 > halo ? c0 - halo : 0;
        const int64_t he = c0 + it.n_e + halo < it.len ? c0 + it.n_e + halo : it.len;
        it.t0 = (int)(c0 - hs);
        it.n_st = (int)(he - hs);
        it.pad = 0;
        for (int x = lane; x < it.n_st; x += 64) {
            int32_t v = a.vals[base + hs + x];
            v = v < 0 ? 0 : (v >= a.V ? a.V - 1 : v);   // (k_sgt_check has passed: this keeps a load in the table whatever happens)
            if constexpr (sizeof(REC) == 8) wrec[g * ST + x] = make_int2(v, __float_as_int(a.w ? a.w[v] : 1.f));
            else wrec[g * ST + x] = v;
        }
        if (lane == 0) wit[g] = it;
    }
}

__device__ __forceinline__ float4 sgt_scale4(float4 x, float s) { return make_float4(x.x * s, x.y * s, x.z * s, x.w * s); }

// s_k from the weight sum or from the sum of squares of the row
__device__ __forceinline__ float sgt_scale(int pool, float ws, float sq) {
    if (pool == BPE_SGM_POOL_MEAN) return ws != 0.f ? 1.f / ws : 0.f;
    if (pool == BPE_SGM_POOL_UNIT) return sq > 0.f ? 1.f / sqrtf(sq) : 0.f;
    return 1.f;
}

template <int VM>
__device__ __forceinline__ void sgt_store_row(const sgt_args &a, float *row, int e, float4 x) {
    if (VM == 4 && a.vm == 4) glv_store4<4>(row, e, a.E, x);
    else if (VM >= 2 && a.vm >= 2) glv_store4<2>(row, e, a.E, x);
    else glv_store4<1>(row, e, a.E, x);
}

template <int EP, int VM>
__device__ __forceinline__ void sgt_pool_walk(const sgt_args &a, const int2 *rec, const sgt_item &it, int l) {
    const int E = a.E, e = 4 * l, n_e = it.n_e;
    const float4 b1r = glv_load4<VM>(a.b1, e, E);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float ws = 0.f;
    for (int j = 0; j < n_e; j += 4) {
        int2 rc[4];
        float4 row[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) rc[k] = rec[min(j + k, n_e - 1)];   // (past the chunk: the last value again, unused)
#pragma unroll
        for (int k = 0; k < 4; ++k) row[k] = glv_load4<VM>(a.Ein + (size_t)rc[k].x * E, e, E);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (j + k < n_e) {
                const float wt = __int_as_float(rc[k].y);
                const float4 x = glv_add4(row[k], b1r);
                acc.x = fmaf(wt, x.x, acc.x), acc.y = fmaf(wt, x.y, acc.y);
                acc.z = fmaf(wt, x.z, acc.z), acc.w = fmaf(wt, x.w, acc.w);
                ws = __fadd_rn(ws, wt);
            }
        }
    }
    if (it.nch == 1) {
        float sq = 0.f;
        if (a.pool == BPE_SGM_POOL_UNIT)
            sq = glv_group_sum<EP / 4>(fmaf(acc.w, acc.w, fmaf(acc.z, acc.z, fmaf(acc.y, acc.y, acc.x * acc.x))));
        sgt_store_row<VM>(a, a.out + (size_t)it.k * E, e, sgt_scale4(acc, sgt_scale(a.pool, ws, sq)));
    } else {
        const int64_t slot = a.moff[it.k] + it.chunk;
        glv_store4<VM>(a.part_row + (size_t)slot * E, e, E, acc);
        if (l == 0) {
            a.part_w[slot] = ws;
            a.slot_text[slot] = it.k;
        }
    }
}

template <int EP>
__global__ __launch_bounds__(SGT_WG) void k_sgt_pool(const sgt_args a) {
    constexpr int G = EP / 4, GW = 64 / G;   // lanes of a group, groups (items) of a wave
    __shared__ int2 recs[4 * GW * SGT_CHUNK];
    __shared__ sgt_item items[4 * GW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t item0 = ((int64_t)blockIdx.x * 4 + w) * GW;
    sgt_stage<int2, GW, SGT_CHUNK>(a, item0, 0, recs + w * GW * SGT_CHUNK, items + w * GW, lane);
    __syncthreads();
    const int gi = lane / G, l = lane % G;
    if (item0 + gi >= a.n_items) return;
    const sgt_item it = items[w * GW + gi];
    const int2 *rec = recs + (w * GW + gi) * SGT_CHUNK;
    if ((a.E & 3) == 0) sgt_pool_walk<EP, 4>(a, rec, it, l);
    else if ((a.E & 1) == 0) sgt_pool_walk<EP, 2>(a, rec, it, l);
    else sgt_pool_walk<EP, 1>(a, rec, it, l);
}

template <int EP, int VM>
__device__ __forceinline__ void sgt_score_walk(const sgt_args &a, const int32_t *sv, const sgt_item &it, int l) {
    const int E = a.E, e = 4 * l, w = a.window;
    const float4 b1r = glv_load4<VM>(a.b1, e, E);
    double sum = 0.0;
    for (int i = 0; i < it.n_e; ++i) {
        const int p = it.t0 + i;   // the target among the staged values; its contexts are lo .. hi without p
        const int vt = sv[p];
        const float4 xt = glv_add4(glv_load4<VM>(a.Ein + (size_t)vt * E, e, E), b1r);
        const float lse = a.lse[vt];
        const int lo = max(p - w, 0), hi = min(p + w, it.n_st - 1), cn = hi - lo;
        for (int c = 0; c < cn; c += 4) {
            int cv[4];
            float4 row[4];
            float cb[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int j = lo + min(c + k, cn - 1);   // (past the last context: it again, unused)
                j += j >= p ? 1 : 0;
                cv[k] = sv[j];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                row[k] = glv_load4<VM>(a.Eout + (size_t)cv[k] * E, e, E);
                cb[k] = a.b2[cv[k]];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (c + k < cn) {
                    const float d = glv_group_sum<EP / 4>(
                        fmaf(xt.w, row[k].w, fmaf(xt.z, row[k].z, fmaf(xt.y, row[k].y, xt.x * row[k].x))));
                    sum += (double)__fsub_rn(__fadd_rn(d, cb[k]), lse);
                }
            }
        }
    }
    if (l != 0) return;
    if (it.nch == 1) {
        a.sum[it.k] = sum;
        a.pairs[it.k] = sg_text_pairs(it.len, w);
    } else {
        const int64_t slot = a.moff[it.k] + it.chunk;
        a.part_sum[slot] = sum;
        a.slot_text[slot] = it.k;
    }
}

template <int EP>
__global__ __launch_bounds__(SGT_WG) void k_sgt_score(const sgt_args a) {
    constexpr int G = EP / 4, GW = 64 / G;
    __shared__ int32_t svals[4 * GW * SGT_STAGE];
    __shared__ sgt_item items[4 * GW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t item0 = ((int64_t)blockIdx.x * 4 + w) * GW;
    sgt_stage<int32_t, GW, SGT_STAGE>(a, item0, a.window, svals + w * GW * SGT_STAGE, items + w * GW, lane);
    __syncthreads();
    const int gi = lane / G, l = lane % G;
    if (item0 + gi >= a.n_items) return;
    const sgt_item it = items[w * GW + gi];
    const int32_t *sv = svals + (w * GW + gi) * SGT_STAGE;
    if ((a.E & 3) == 0) sgt_score_walk<EP, 4>(a, sv, it, l);
    else if ((a.E & 1) == 0) sgt_score_walk<EP, 2>(a, sv, it, l);
    else sgt_score_walk<EP, 1>(a, sv, it, l);
}

constexpr int SGT_NX = BPE_SGM_MAX_EMBED / 64;   // elements of a row per lane of a wave

// a wave per partial slot: the first of every SGT_FOLD chunks of a text adds the ones behind it into itself
__global__ __launch_bounds__(256) void k_sgt_fold(const sgt_args a, int score) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= a.n_multi) return;
    const int64_t k = a.slot_text[m], m0 = a.moff[k], c = m - m0, nch = a.ioff[k + 1] - a.ioff[k];
    if (c % SGT_FOLD || c + 1 >= nch) return;
    const int64_t m1 = m0 + (c + SGT_FOLD < nch ? c + SGT_FOLD : nch);
    if (score) {
        if (lane) return;
        double s = a.part_sum[m];
#pragma unroll 8
        for (int64_t j = m + 1; j < m1; ++j) s += a.part_sum[j];
        a.part_sum[m] = s;
        return;
    }
    const int E = a.E;
    float acc[SGT_NX], ws = a.part_w[m];
#pragma unroll
    for (int x = 0; x < SGT_NX; ++x) acc[x] = lane + 64 * x < E ? a.part_row[(size_t)m * E + lane + 64 * x] : 0.f;
#pragma unroll 4
    for (int64_t j = m + 1; j < m1; ++j) {
#pragma unroll
        for (int x = 0; x < SGT_NX; ++x)
            if (lane + 64 * x < E) acc[x] += a.part_row[(size_t)j * E + lane + 64 * x];
        ws += a.part_w[j];
    }
#pragma unroll
    for (int x = 0; x < SGT_NX; ++x)
        if (lane + 64 * x < E) a.part_row[(size_t)m * E + lane + 64 * x] = acc[x];
    if (lane == 0) a.part_w[m] = ws;
}

// a wave per text of several chunks: its partials, every stride-th, in chunk order; scaled and stored
__global__ __launch_bounds__(256) void k_sgt_pool_finish(const sgt_args a, int stride) {
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= a.n_texts) return;
    const int64_t nch = a.ioff[k + 1] - a.ioff[k], m0 = a.moff[k];
    if (nch == 1) return;
    const int E = a.E;
    float acc[SGT_NX], ws = a.part_w[m0];
#pragma unroll
    for (int x = 0; x < SGT_NX; ++x) acc[x] = lane + 64 * x < E ? a.part_row[(size_t)m0 * E + lane + 64 * x] : 0.f;
#pragma unroll 4
    for (int64_t c = stride; c < nch; c += stride) {
#pragma unroll
        for (int x = 0; x < SGT_NX; ++x)
            if (lane + 64 * x < E) acc[x] += a.part_row[(size_t)(m0 + c) * E + lane + 64 * x];
        ws += a.part_w[m0 + c];
    }
    float sq = 0.f;
    if (a.pool == BPE_SGM_POOL_UNIT) {
#pragma unroll
        for (int x = 0; x < SGT_NX; ++x) sq = fmaf(acc[x], acc[x], sq);
        for (int o = 32; o; o >>= 1) sq += __shfl_xor(sq, o, 64);
    }
    const float s = sgt_scale(a.pool, ws, sq);
#pragma unroll
    for (int x = 0; x < SGT_NX; ++x)
        if (lane + 64 * x < E) a.out[(size_t)k * E + lane + 64 * x] = acc[x] * s;
}

// a thread per text of several chunks: its partial doubles in chunk order, and the closed form of its pairs
__global__ __launch_bounds__(256) void k_sgt_score_finish(const sgt_args a, int stride) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n_texts) return;
    const int64_t nch = a.ioff[k + 1] - a.ioff[k], m0 = a.moff[k];
    if (nch == 1) return;
    double s = a.part_sum[m0];
#pragma unroll 8
    for (int64_t c = stride; c < nch; c += stride) s += a.part_sum[m0 + c];
    a.sum[k] = s;
    a.pairs[k] = sg_text_pairs(a.off[k + 1] - a.off[k], a.window);
}

__global__ __launch_bounds__(256) void k_sgt_iota(int32_t *__restrict__ ids, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ids[i] = i;
}

template <int EP>
void sgt_launch(bpe_sgmodel *M, const sgt_args &a, bool score) {
    constexpr int IPB = 4 * (64 / (EP / 4));   // items of a workgroup
    const unsigned grid = (unsigned)((a.n_items + IPB - 1) / IPB);
    if (score) k_sgt_score<EP><<<grid, SGT_WG, 0, M->stream>>>(a);
    else k_sgt_pool<EP><<<grid, SGT_WG, 0, M->stream>>>(a);
}

const char *const SGT_OFFSETS_MSG = "bpe native: text offsets must not decrease or be negative";

// a value outside [0, V): the message names it, its text and its place there
int sgt_range_error(bpe_sgmodel *M, const int32_t *d_vals, const int64_t *d_off, int64_t n, int64_t pos) {
    std::vector<int64_t> off((size_t)n + 1);
    int32_t v = 0;
    SGM_TRY(hipMemcpy(off.data(), d_off, off.size() * 8, hipMemcpyDeviceToHost));
    SGM_TRY(hipMemcpy(&v, d_vals + off[0] + pos, 4, hipMemcpyDeviceToHost));
    const int64_t k = (std::upper_bound(off.begin(), off.end(), off[0] + pos) - off.begin()) - 1;
    char msg[160];
    snprintf(msg, sizeof msg, "skip-gram model value %d outside [0, %d) (text %lld, value %lld)", (int)v, M->V,
             (long long)k, (long long)(off[0] + pos - off[(size_t)k]));
    return bpe_fail(BPE_ERR_ARG, msg);
}

int sgt_check_args(bpe_sgmodel *M, bool score, const int64_t *off, int64_t n, int pool, int window, const void *o1,
                   const void *o2) {
    char msg[128];
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    M->tstats.calls++;
    if (!score && pool != BPE_SGM_POOL_SUM && pool != BPE_SGM_POOL_MEAN && pool != BPE_SGM_POOL_UNIT) {
        snprintf(msg, sizeof msg, "skip-gram model pool %d is none of BPE_SGM_POOL_SUM, _MEAN, _UNIT", pool);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    if (score && (window < 1 || window > BPE_SKIPGRAM_MAX_WINDOW)) {
        snprintf(msg, sizeof msg, "skip-gram model window %d outside [1, %d]", window, BPE_SKIPGRAM_MAX_WINDOW);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    if (n < 0 || n >= (1ll << 31) || (n && (!off || !o1 || !o2)))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model text arguments");
    return BPE_OK;
}

// the device form of both calls (the arguments have been checked)
int sgt_run(bpe_sgmodel *M, bool score, const int32_t *d_vals, const int64_t *d_off, int64_t n, const float *d_w,
            int pool, int window, float *d_out, double *d_sum, int64_t *d_pairs) {
    if (!n) return BPE_OK;
    SGM_TRY(hipSetDevice(M->device));
    auto up = [](int64_t b) { return (b + 15) / 16 * 16; };
    const int64_t off_bytes = up((n + 1) * 8);
    if (int rc = sgm_grow(&M->d_ts, &M->ts_cap, SGTH_WORDS * 8 + 2 * off_bytes)) return rc;
    unsigned long long *hdr = (unsigned long long *)M->d_ts;
    long long *ioff = (long long *)((char *)M->d_ts + SGTH_WORDS * 8), *moff = (long long *)((char *)ioff + off_bytes);

    unsigned long long h[SGTH_WORDS] = {SGM_NONE, 0, 0, 0, 0, 0, 0, 0};
    SGM_TRY(hipMemcpyAsync(hdr, h, sizeof h, hipMemcpyHostToDevice, M->stream));
    SGM_TRY(hipEventRecord(M->ev0, M->stream));
    k_sgt_items<<<1, 1024, 0, M->stream>>>(d_off, n, score ? window : 0, ioff, moff, hdr);
    k_sgt_check<<<SGT_CHECK_BLOCKS, 256, 0, M->stream>>>(d_vals, d_off, n, M->V, hdr);
    SGM_TRY(hipGetLastError());
    SGM_TRY(hipEventRecord(M->ev1, M->stream));
    SGM_TRY(hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, M->stream));
    SGM_TRY(hipStreamSynchronize(M->stream));
    if (int rc = sgm_time(M, &M->tstats.kernel_ms)) return rc;
    if (h[SGTH_BAD]) return bpe_fail(BPE_ERR_ARG, SGT_OFFSETS_MSG);
    if (h[SGTH_VALUES] && !d_vals) return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model text arguments");
    if (h[SGTH_ERR] != SGM_NONE) return sgt_range_error(M, d_vals, d_off, n, (int64_t)h[SGTH_ERR]);
    if (h[SGTH_ITEMS] >= (1ull << 31)) return bpe_fail(BPE_ERR_ARG, "bpe native: skip-gram model text batch above 2^31 chunks");

    sgt_args a = {};
    a.Ein = M->d_p + M->o_ein, a.b1 = M->d_p + M->o_b1, a.Eout = M->d_p + M->o_eout, a.b2 = M->d_p + M->o_b2;
    a.w = d_w;
    a.V = M->V, a.E = M->E, a.pool = pool, a.window = window;
    a.vm = (M->E % 4 == 0 && (uintptr_t)d_out % 16 == 0) ? 4 : (M->E % 2 == 0 && (uintptr_t)d_out % 8 == 0) ? 2 : 1;
    a.vals = d_vals, a.off = d_off;
    a.n_texts = n, a.n_items = (int64_t)h[SGTH_ITEMS], a.n_multi = (int64_t)h[SGTH_MULTI];
    a.ioff = ioff, a.moff = moff;
    a.out = d_out, a.sum = d_sum, a.pairs = d_pairs;

    // the partials of the texts of several chunks; for the score, lse[V] and what the predict forward writes beside it
    const int64_t vb = up((int64_t)M->V * 4);
    const int64_t sizes[] = {up(a.n_multi * 8), score ? up(a.n_multi * 8) : up(a.n_multi * M->E * 4),
                             score ? 0 : up(a.n_multi * 4), score ? 4 * vb : 0};
    if (int rc = sgm_grow(&M->d_tp, &M->tp_cap, sizes[0] + sizes[1] + sizes[2] + sizes[3] + 16)) return rc;
    char *p = (char *)M->d_tp;
    a.slot_text = (long long *)p;
    p += sizes[0];
    if (score) a.part_sum = (double *)p;
    else a.part_row = (float *)p;
    p += sizes[1];
    a.part_w = (float *)p;
    p += sizes[2];
    if (score) {
        int32_t *ids = (int32_t *)p, *top_id = (int32_t *)(p + vb);
        float *top_p = (float *)(p + 2 * vb), *lse = (float *)(p + 3 * vb);
        k_sgt_iota<<<(M->V + 255) / 256, 256, 0, M->stream>>>(ids, M->V);
        const bpe_sgmodel_query_stats keep = M->qstats;   // (the forward is the query's; its statistics are not)
        const int rc = sgq_run(M, SGQ_PREDICT, ids, nullptr, M->V, 1, BPE_SGM_DOT, top_id, top_p, lse);
        M->tstats.kernel_ms += M->qstats.kernel_ms - keep.kernel_ms;
        M->qstats = keep;
        if (rc) return rc;
        a.lse = lse;
    }

    SGM_TRY(hipEventRecord(M->ev0, M->stream));
    switch (M->EP) {
        case 64: sgt_launch<64>(M, a, score); break;
        case 128: sgt_launch<128>(M, a, score); break;
        default: sgt_launch<256>(M, a, score); break;
    }
    if (a.n_multi) {
        const int stride = a.n_multi > SGT_FOLD ? SGT_FOLD : 1;   // (more than SGT_FOLD chunks in a text need as many slots)
        if (stride > 1) k_sgt_fold<<<(unsigned)((a.n_multi + 3) / 4), 256, 0, M->stream>>>(a, score ? 1 : 0);
        if (score) k_sgt_score_finish<<<(unsigned)((n + 255) / 256), 256, 0, M->stream>>>(a, stride);
        else k_sgt_pool_finish<<<(unsigned)((n + 3) / 4), 256, 0, M->stream>>>(a, stride);
    }
    SGM_TRY(hipGetLastError());
    SGM_TRY(hipEventRecord(M->ev1, M->stream));
    SGM_TRY(hipStreamSynchronize(M->stream));
    if (int rc = sgm_time(M, &M->tstats.kernel_ms)) return rc;
    M->tstats.texts += n;
    M->tstats.values += (int64_t)h[SGTH_VALUES];
    M->tstats.items += a.n_items;
    M->tstats.pairs += (int64_t)h[SGTH_PAIRS];
    return BPE_OK;
}

// a host form: the texts' values, their offsets rebased to them and the weights staged in the model's scratch,
// the device form, the outputs copied back
int sgt_host(bpe_sgmodel *M, bool score, const int32_t *vals, const int64_t *off, int64_t n, const float *w, int pool,
             int window, float *out, double *sum, int64_t *pairs) {
    if (!n) return BPE_OK;
    if (off[0] < 0) return bpe_fail(BPE_ERR_ARG, SGT_OFFSETS_MSG);
    for (int64_t k = 0; k < n; ++k)
        if (off[k + 1] < off[k]) return bpe_fail(BPE_ERR_ARG, SGT_OFFSETS_MSG);
    const int64_t span = off[n] - off[0];
    if (span && !vals) return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model text arguments");
    SGM_TRY(hipSetDevice(M->device));
    auto up = [](int64_t b) { return (b + 15) / 16 * 16; };
    const int64_t out_bytes = score ? up(n * 8) : up(n * M->E * 4), pairs_bytes = score ? up(n * 8) : 0;
    const int64_t off_bytes = up((n + 1) * 8), w_bytes = w ? up((int64_t)M->V * 4) : 0;
    if (int rc = sgm_grow(&M->d_io, &M->io_cap, out_bytes + pairs_bytes + off_bytes + w_bytes + up(span * 4))) return rc;
    char *d_o = (char *)M->d_io, *d_pr = d_o + out_bytes;
    int64_t *d_off = (int64_t *)(d_pr + pairs_bytes);
    float *d_w = (float *)((char *)d_off + off_bytes);
    int32_t *d_vals = (int32_t *)((char *)d_w + w_bytes);
    std::vector<int64_t> rel((size_t)n + 1);
    for (int64_t k = 0; k <= n; ++k) rel[(size_t)k] = off[k] - off[0];
    SGM_TRY(hipMemcpy(d_off, rel.data(), rel.size() * 8, hipMemcpyHostToDevice));
    if (span) SGM_TRY(hipMemcpy(d_vals, vals + off[0], (size_t)span * 4, hipMemcpyHostToDevice));
    if (w) SGM_TRY(hipMemcpy(d_w, w, (size_t)M->V * 4, hipMemcpyHostToDevice));
    if (int rc = sgt_run(M, score, d_vals, d_off, n, w ? d_w : nullptr, pool, window, (float *)d_o, (double *)d_o,
                         (int64_t *)d_pr))
        return rc;
    if (score) {
        SGM_TRY(hipMemcpy(sum, d_o, (size_t)n * 8, hipMemcpyDeviceToHost));
        SGM_TRY(hipMemcpy(pairs, d_pr, (size_t)n * 8, hipMemcpyDeviceToHost));
    } else {
        SGM_TRY(hipMemcpy(out, d_o, (size_t)n * M->E * 4, hipMemcpyDeviceToHost));
    }
    return BPE_OK;
}

}  // namespace

extern "C" {

int bpe_sgmodel_embed_texts_device(bpe_sgmodel *M, const int32_t *d_vals, const int64_t *d_off, int64_t n_texts,
                                   const float *d_weights, int pool, float *d_out) {
    if (int rc = sgt_check_args(M, false, d_off, n_texts, pool, 0, d_out, d_out)) return rc;
    return sgt_run(M, false, d_vals, d_off, n_texts, d_weights, pool, 0, d_out, nullptr, nullptr);
}

int bpe_sgmodel_embed_texts(bpe_sgmodel *M, const int32_t *vals, const int64_t *off, int64_t n_texts, const float *weights,
                            int pool, float *out) {
    if (int rc = sgt_check_args(M, false, off, n_texts, pool, 0, out, out)) return rc;
    return sgt_host(M, false, vals, off, n_texts, weights, pool, 0, out, nullptr, nullptr);
}

int bpe_sgmodel_score_texts_device(bpe_sgmodel *M, const int32_t *d_vals, const int64_t *d_off, int64_t n_texts, int window,
                                   double *d_sum_logp, int64_t *d_pairs) {
    if (int rc = sgt_check_args(M, true, d_off, n_texts, 0, window, d_sum_logp, d_pairs)) return rc;
    return sgt_run(M, true, d_vals, d_off, n_texts, nullptr, 0, window, nullptr, d_sum_logp, d_pairs);
}

int bpe_sgmodel_score_texts(bpe_sgmodel *M, const int32_t *vals, const int64_t *off, int64_t n_texts, int window,
                            double *sum_logp, int64_t *pairs) {
    if (int rc = sgt_check_args(M, true, off, n_texts, 0, window, sum_logp, pairs)) return rc;
    return sgt_host(M, true, vals, off, n_texts, nullptr, 0, window, nullptr, sum_logp, pairs);
}

int bpe_sgmodel_get_text_stats(bpe_sgmodel *M, bpe_sgmodel_text_stats *out) {
    if (!M || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = M->tstats;
    return BPE_OK;
}

int bpe_sgmodel_reset_text_stats(bpe_sgmodel *M) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    M->tstats = {};
    return BPE_OK;
}

}  // extern "C"
