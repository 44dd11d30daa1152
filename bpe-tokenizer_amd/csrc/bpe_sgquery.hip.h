// bpe_sgquery.hip.h — queries of the skip-gram model (include/bpe.h, "skip-gram model queries"): the k
// nearest tokens of an id or of a caller's vector, and the k likeliest contexts of a target, as one
// streamed n x V x E product with the top-k selection fused behind it.  The n x V score matrix is never
// written.  Part of bpe_sgmodel.hip's translation unit (its struct, SGM_TRY, sgm_mfma, sgm_acc_row and
// sgm_grow are in scope).  DESIGN.md §3p.
//
// With X_v = fl32(Ein[v] + b1):  dot s(q, v) = q . X_v;  cosine s(q, v) = fl(fl((q . X_v) r(q)) r(X_v)),
// r(x) = 1 / |x|_2 and 0 for the zero vector;  predict z(t, c) = X_t . Eout[c] + b2[c], p = exp(z - lse_t).
// Order: score descending, then id ascending.  An entry is one 64-bit key, (ordered image of the score)
// << 32 | ~id, so the whole order is one unsigned compare; 0 is below every key and stands for "none".
//
//   k_sgm_ids_check   the smallest id outside [0, V) by an integer atomicMin (nothing is written then);
//   k_sgm_norms       r(X_v) for every v, one wave per row: lanes over e, then a butterfly (one fixed order);
//   k_sgm_topk        grid (query tiles) x (key splits).  A wave owns 32 queries; a workgroup is two waves
//                     (one at EP = 256, where the lists of two would not fit beside the tiles).  The query
//                     tile is staged in LDS (gathered as Ein[id] + b1 for the id forms), the split's
//                     32-row key tiles stream through two LDS buffers behind a register prefetch, and
//                     S^T = K_tile . Q^T leaves a query's 32 scores of a tile in the 16 accumulator
//                     registers of its two lanes.  Each lane tests its 16 keys against the k-th best it
//                     holds in a register; a hit inserts into the lane's sorted list of k keys in LDS
//                     ([k][threads]: a lane's column, no bank shared with another lane's).  Predict also
//                     keeps the running (max, sum) of its logits.  The lists and (max, sum) go to scratch;
//   k_sgm_topk_merge  one wave per query merges its 2 x splits lists (a lane holds the heads of up to 8),
//                     combines the (max, sum) partials in split order and writes the k outputs and padding.
// A score is accumulated over e in one order whatever the tile, the split or the batch, so ids and
// neighbour scores are the same bytes in every call; lse and p depend on the number of splits in the
// last place.  No floating-point atomics.

namespace {

typedef unsigned long long sgq_u64;
constexpr int SGQ_SUB = 32;                 // key rows per streamed tile
constexpr int SGQ_MAX_SPLITS = 256;         // 2 x 256 lists: 8 heads per lane of the merge
constexpr int64_t SGQ_CHUNK = 1 << 16;      // queries per launch (bounds the scratch)
constexpr int SGQ_NEIGH = 0, SGQ_PREDICT = 1;

template <int EP>
constexpr int sgq_waves() { return EP <= 128 ? 2 : 1; }

template <int EP>
constexpr size_t sgq_lds(int k) {
    return (size_t)64 * sgq_waves<EP>() * k * 8 +
           (size_t)((32 * sgq_waves<EP>() + 2 * SGQ_SUB) * (EP + 1) + 2 * SGQ_SUB + EP) * 4;
}
static_assert(sgq_lds<64>(BPE_SGM_MAX_TOPK) <= 160 * 1024 && sgq_lds<128>(BPE_SGM_MAX_TOPK) <= 160 * 1024 &&
              sgq_lds<256>(BPE_SGM_MAX_TOPK) <= 160 * 1024, "LDS of the query kernels at k = 64");

// the order-preserving unsigned image of a float (-0 is +0), and back
__device__ __forceinline__ uint32_t sgq_image(float s) {
    uint32_t b = __float_as_uint(s);
    if (b == 0x80000000u) b = 0;
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float sgq_score(uint32_t im) {
    return __uint_as_float((im & 0x80000000u) ? im & 0x7fffffffu : ~im);
}
__device__ __forceinline__ sgq_u64 sgq_key(float s, int id) { return ((sgq_u64)sgq_image(s) << 32) | (uint32_t)~id; }

// 1 / |x| from the wave's sum of squares: lanes over e, then a butterfly (every lane gets the same bits)
template <class F>
__device__ __forceinline__ float sgq_rnorm_wave(F x, int E, int lane) {
    float s = 0.f;
    for (int e = lane; e < E; e += 64) {
        const float a = x(e);
        s = fmaf(a, a, s);
    }
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
    return s > 0.f ? 1.f / sqrtf(s) : 0.f;
}

__global__ __launch_bounds__(256) void k_sgm_ids_check(const int32_t *__restrict__ ids, int64_t n, int V, sgq_u64 *hdr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (uint32_t)ids[i] >= (uint32_t)V) atomicMin(&hdr[SGMH_ERR], (sgq_u64)i);
}

__global__ __launch_bounds__(256) void k_sgm_norms(const float *__restrict__ Ein, const float *__restrict__ b1, int V, int E,
                                                   float *__restrict__ rnorm) {
    const int lane = threadIdx.x & 63, v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= V) return;
    const float *row = Ein + (size_t)v * E;
    const float r = sgq_rnorm_wave([&](int e) { return row[e] + b1[e]; }, E, lane);
    if (lane == 0) rnorm[v] = r;
}

template <int EP, int MODE>
__global__ __launch_bounds__(64 * sgq_waves<EP>()) void k_sgm_topk(
    const float *__restrict__ Ein, const float *__restrict__ b1, const float *__restrict__ Eout,
    const float *__restrict__ b2, const float *__restrict__ rnorm, int V, int E, const int32_t *__restrict__ ids,
    const float *__restrict__ qv, int n, int k, int metric, int tps, sgq_u64 *__restrict__ part,
    float2 *__restrict__ ml) {
    constexpr int NW = sgq_waves<EP>(), NT = 64 * NW, QT = 32 * NW, LD = EP + 1;
    constexpr int NPRE = SGQ_SUB * EP / NT;
    extern __shared__ sgq_u64 smem64[];
    sgq_u64 *Ls = smem64 + threadIdx.x;                 // [k][NT]: this lane's list, best first
    float *Qs = (float *)(smem64 + (size_t)NT * k);     // [QT][LD]
    float *Ks = Qs + QT * LD;                           // [2][SGQ_SUB][LD]
    float *kvs = Ks + 2 * SGQ_SUB * LD;                 // [2][SGQ_SUB]: r(X_c) or b2[c] of the tile's keys
    float *b1s = kvs + 2 * SGQ_SUB;                     // [EP]
    const float *K = MODE == SGQ_NEIGH ? Ein : Eout;
    const float *kv = MODE == SGQ_NEIGH ? rnorm : b2;
    const bool cosine = MODE == SGQ_NEIGH && metric == BPE_SGM_COSINE;
    const bool use_kv = MODE == SGQ_PREDICT || cosine;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane & 31, half = lane >> 5;
    const int Q0 = blockIdx.x * QT, splits = gridDim.y, split = blockIdx.y;
    const int Ek = (E + 1) & ~1;
    const int n_tiles = (V + SGQ_SUB - 1) / SGQ_SUB;
    const int j0 = split * tps, j1 = min(n_tiles, j0 + tps);

    // the query tile: rows X_id gathered here (an id out of range was reported by k_sgm_ids_check and
    // nothing will be written; its row is zero), or the caller's rows
    for (int idx = tid; idx < QT * EP; idx += NT) {
        const int r = idx / EP, e = idx % EP;
        float x = 0.f;
        if (Q0 + r < n && e < E) {
            if (ids) {
                const int32_t id = ids[Q0 + r];
                if ((uint32_t)id < (uint32_t)V) x = Ein[(size_t)id * E + e] + b1[e];
            } else {
                x = qv[(size_t)(Q0 + r) * E + e];
            }
        }
        Qs[r * LD + e] = x;
    }
    for (int e = tid; e < EP; e += NT) b1s[e] = (MODE == SGQ_NEIGH && e < E) ? b1[e] : 0.f;
    for (int i = 0; i < k; ++i) Ls[i * NT] = 0;
    const int qi = Q0 + w * 32 + q;
    const int excl = (MODE == SGQ_NEIGH && ids && qi < n) ? ids[qi] : -1;
    __syncthreads();

    float rq = 1.f;
    if (cosine) {
        for (int r = 0; r < 32; ++r) {
            const float *row = Qs + (w * 32 + r) * LD;
            const float x = sgq_rnorm_wave([&](int e) { return row[e]; }, E, lane);
            if (q == r) rq = x;
        }
    }

    // EP <= 128: the next tile waits in registers while this one is used; at EP = 256 that would be 128
    // registers per lane (it spilled), so the next tile is staged into the other buffer behind the products
    constexpr bool PRE = EP <= 128;
    float pre[PRE ? NPRE : 1], pre_b = 0.f;
    auto tile_value = [&](int j, int idx) {
        const int e = idx % EP, c = j * SGQ_SUB + idx / EP;
        return (c < V && e < E) ? K[(size_t)c * E + e] : 0.f;
    };
    auto tile_kv = [&](int j) {
        const int c = j * SGQ_SUB + tid;
        return !use_kv ? 0.f : c < V ? kv[c] : (MODE == SGQ_PREDICT ? -INFINITY : 0.f);
    };
    auto load_tile = [&](int j) {
#pragma unroll
        for (int i = 0; i < (PRE ? NPRE : 0); ++i) pre[i] = tile_value(j, tid + i * NT);
        if (tid < SGQ_SUB) pre_b = tile_kv(j);
    };
    // (a padded row becomes b1, not 0: its keys never enter)
    auto put = [&](float *Kb, int idx, float x) {
        Kb[(idx / EP) * LD + idx % EP] = MODE == SGQ_NEIGH ? x + b1s[idx % EP] : x;
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < (PRE ? NPRE : 0); ++i) put(Ks + buf * SGQ_SUB * LD, tid + i * NT, pre[i]);
        if (tid < SGQ_SUB) kvs[buf * SGQ_SUB + tid] = pre_b;
    };
    auto stage_tile = [&](int j, int buf) {
#pragma unroll 8
        for (int i = 0; i < NPRE; ++i) put(Ks + buf * SGQ_SUB * LD, tid + i * NT, tile_value(j, tid + i * NT));
        if (tid < SGQ_SUB) kvs[buf * SGQ_SUB + tid] = tile_kv(j);
    };

    sgq_u64 thr = 0;                       // the k-th best key of this lane so far
    float m_run = -INFINITY, l_run = 0.f;  // predict: of the split's logits of this lane's query
    const float *Qw = Qs + (w * 32 + q) * LD + half;

    if (PRE) load_tile(j0);
    else stage_tile(j0, 0);
    for (int j = j0; j < j1; ++j) {
        const int buf = (j - j0) & 1;
        if (PRE) store_tile(buf);
        __syncthreads();
        if (PRE && j + 1 < j1) load_tile(j + 1);
        const float *Ka = Ks + buf * SGQ_SUB * LD + q * LD + half;
        const float *kb = kvs + buf * SGQ_SUB;
        // S^T[c][t] = sum_e K[c][e] Q[t][e]
        f16v s;
#pragma unroll
        for (int v = 0; v < 16; ++v) s[v] = 0.f;
        for (int e = 0; e < Ek; e += 2) s = sgm_mfma(Ka[e], Qw[e], s);

        sgq_u64 key[16];
        bool any = false;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int row = sgm_acc_row(v, half), c = j * SGQ_SUB + row;
            if (use_kv) s[v] = MODE == SGQ_PREDICT ? s[v] + kb[row] : (s[v] * rq) * kb[row];
            key[v] = (c < V && c != excl) ? sgq_key(s[v], c) : 0;
            any |= key[v] > thr;
        }
        if (MODE == SGQ_PREDICT) {   // (a key past V has the logit -inf)
            float mx = -INFINITY;
#pragma unroll
            for (int v = 0; v < 16; ++v) mx = fmaxf(mx, s[v]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);
            float ps = 0.f;
#pragma unroll
            for (int v = 0; v < 16; ++v) ps += expf(s[v] - m_new);
            ps += __shfl_xor(ps, 32, 64);
            l_run = l_run * expf(m_run - m_new) + ps;
            m_run = m_new;
        }
        if (any) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                if (key[v] > thr) {
                    int i = k - 1;
                    while (i > 0) {
                        const sgq_u64 p = Ls[(i - 1) * NT];
                        if (p > key[v]) break;
                        Ls[i * NT] = p;
                        --i;
                    }
                    Ls[i * NT] = key[v];
                    thr = Ls[(k - 1) * NT];
                }
            }
        }
        // (the other buffer was last read before this iteration's barrier)
        if (!PRE && j + 1 < j1) stage_tile(j + 1, buf ^ 1);
    }

    if (qi < n) {
        sgq_u64 *dst = part + (((size_t)qi * splits + split) * 2 + half) * k;
        for (int i = 0; i < k; ++i) dst[i] = Ls[i * NT];
        if (MODE == SGQ_PREDICT && half == 0) ml[(size_t)qi * splits + split] = make_float2(m_run, l_run);
    }
}

__global__ __launch_bounds__(256) void k_sgm_topk_merge(const sgq_u64 *__restrict__ part, const float2 *__restrict__ ml,
                                                        int n, int k, int splits, int mode, const sgq_u64 *hdr,
                                                        int32_t *__restrict__ out_ids, float *__restrict__ out_vals,
                                                        float *__restrict__ out_lse) {
    const int lane = threadIdx.x & 63, qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= n || hdr[SGMH_ERR] != SGM_NONE) return;
    const int nl = 2 * splits;
    const sgq_u64 *lists = part + (size_t)qi * nl * k;
    // this lane's lists are lane, lane + 64, ..: their read positions, one byte each, and the best head
    sgq_u64 ptrs = 0, best = 0, res = 0;
    int bi = 0;
    auto rescan = [&]() {
        best = 0;
        for (int i = 0; lane + 64 * i < nl; ++i) {
            const int p = (int)((ptrs >> (8 * i)) & 255);
            const sgq_u64 h = p < k ? lists[(size_t)(lane + 64 * i) * k + p] : 0;
            if (h > best) {
                best = h;
                bi = i;
            }
        }
    };
    rescan();
    for (int r = 0; r < k; ++r) {
        sgq_u64 m = best;
        for (int o = 32; o; o >>= 1) {
            const sgq_u64 t = __shfl_xor(m, o, 64);
            m = t > m ? t : m;
        }
        if (!m) break;   // (uniform) the candidates ran out: the rest is padding
        if (lane == r) res = m;
        if (best == m) {   // keys are distinct: one lane
            ptrs += 1ull << (8 * bi);
            rescan();
        }
    }
    float lse = 0.f;
    if (mode == SGQ_PREDICT) {
        const float2 *p = ml + (size_t)qi * splits;
        float mx = -INFINITY, l = 0.f;
        for (int s = 0; s < splits; ++s) mx = fmaxf(mx, p[s].x);
        for (int s = 0; s < splits; ++s) l += p[s].y * expf(p[s].x - mx);
        lse = mx + logf(l);
        if (lane == 0 && out_lse) out_lse[qi] = lse;
    }
    if (lane < k) {
        const float sc = sgq_score((uint32_t)(res >> 32));
        out_ids[(size_t)qi * k + lane] = res ? (int32_t)~(uint32_t)res : -1;
        out_vals[(size_t)qi * k + lane] = mode == SGQ_PREDICT ? (res ? expf(sc - lse) : 0.f) : (res ? sc : -INFINITY);
    }
}

template <int EP, int MODE>
hipError_t sgq_lds_attr() {
    return hipFuncSetAttribute((const void *)k_sgm_topk<EP, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)sgq_lds<EP>(BPE_SGM_MAX_TOPK));
}

hipError_t sgq_lds_attrs() {
    for (hipError_t e : {sgq_lds_attr<64, SGQ_NEIGH>(), sgq_lds_attr<64, SGQ_PREDICT>(), sgq_lds_attr<128, SGQ_NEIGH>(),
                         sgq_lds_attr<128, SGQ_PREDICT>(), sgq_lds_attr<256, SGQ_NEIGH>(),
                         sgq_lds_attr<256, SGQ_PREDICT>()})
        if (e != hipSuccess) return e;
    return hipSuccess;
}

template <int EP, int MODE>
void sgq_launch(bpe_sgmodel *M, const int32_t *ids, const float *qv, int n, int k, int metric, int splits, int tps,
                const float *rnorm, sgq_u64 *part, float2 *ml) {
    constexpr int QT = 32 * sgq_waves<EP>();
    const float *p = M->d_p;
    k_sgm_topk<EP, MODE><<<dim3((unsigned)((n + QT - 1) / QT), (unsigned)splits), 64 * sgq_waves<EP>(), sgq_lds<EP>(k),
                           M->stream>>>(p + M->o_ein, p + M->o_b1, p + M->o_eout, p + M->o_b2, rnorm, M->V, M->E, ids,
                                        qv, n, k, metric, tps, part, ml);
}

int sgq_check_args(bpe_sgmodel *M, const void *in, int64_t n, int k, int metric, int64_t embed, const void *o_ids,
                   const void *o_vals) {
    char msg[160];
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (k < 1 || k > BPE_SGM_MAX_TOPK) {
        snprintf(msg, sizeof msg, "skip-gram model k %d outside [1, %d]", k, BPE_SGM_MAX_TOPK);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    if (metric != BPE_SGM_DOT && metric != BPE_SGM_COSINE) {
        snprintf(msg, sizeof msg, "skip-gram model metric %d is neither BPE_SGM_DOT nor BPE_SGM_COSINE", metric);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    if (embed != M->E) {
        snprintf(msg, sizeof msg, "skip-gram model queries of width %lld given to a model of width %d", (long long)embed,
                 M->E);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    if (n < 0 || (n && (!in || !o_ids || !o_vals)))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model query arguments");
    return BPE_OK;
}

// the device form of every query: ids or rows in, k ids and values (and lse) per query out
int sgq_run(bpe_sgmodel *M, int mode, const int32_t *d_ids, const float *d_q, int64_t n, int k, int metric,
            int32_t *o_ids, float *o_vals, float *o_lse) {
    M->qstats.calls++;
    if (!n) return BPE_OK;
    SGM_TRY(hipSetDevice(M->device));
    // query tiles x key splits cover the machine about twice; one split when the tiles alone cover it
    const int QT = M->EP <= 128 ? 64 : 32;
    const int n_kt = (M->V + SGQ_SUB - 1) / SGQ_SUB;
    const int64_t nc = n < SGQ_CHUNK ? n : SGQ_CHUNK, tiles_q = (nc + QT - 1) / QT;
    int splits = 1;
    if (tiles_q < M->n_cus) {
        splits = (int)((2 * M->n_cus + tiles_q - 1) / tiles_q);
        if (splits > SGQ_MAX_SPLITS) splits = SGQ_MAX_SPLITS;
        if (splits > n_kt) splits = n_kt;
    }
    const int tps = (n_kt + splits - 1) / splits;
    splits = (n_kt + tps - 1) / tps;   // (no split without a tile)
    const int64_t norm_bytes = ((int64_t)M->V * 4 + 15) / 16 * 16, part_bytes = nc * splits * 2 * k * 8,
                  ml_bytes = nc * splits * 8;
    if (int rc = sgm_grow(&M->d_qs, &M->qs_cap, norm_bytes + part_bytes + ml_bytes)) return rc;
    float *rnorm = (float *)M->d_qs;
    sgq_u64 *part = (sgq_u64 *)((char *)M->d_qs + norm_bytes);
    float2 *ml = (float2 *)((char *)part + part_bytes);

    sgq_u64 h[SGMH_WORDS] = {SGM_NONE, 0, 0, 0};
    SGM_TRY(hipMemcpyAsync(M->d_hdr, h, sizeof h, hipMemcpyHostToDevice, M->stream));
    SGM_TRY(hipEventRecord(M->ev0, M->stream));
    if (d_ids) k_sgm_ids_check<<<(unsigned)((n + 255) / 256), 256, 0, M->stream>>>(d_ids, n, M->V, M->d_hdr);
    if (mode == SGQ_NEIGH && metric == BPE_SGM_COSINE)
        k_sgm_norms<<<(M->V + 3) / 4, 256, 0, M->stream>>>(M->d_p + M->o_ein, M->d_p + M->o_b1, M->V, M->E, rnorm);
    for (int64_t at = 0; at < n; at += SGQ_CHUNK) {
        const int m = (int)(n - at < SGQ_CHUNK ? n - at : SGQ_CHUNK);
        const int32_t *ci = d_ids ? d_ids + at : nullptr;
        const float *cq = d_q ? d_q + at * M->E : nullptr;
#define SGQ_GO(EP_) \
    (mode == SGQ_NEIGH ? sgq_launch<EP_, SGQ_NEIGH>(M, ci, cq, m, k, metric, splits, tps, rnorm, part, ml) \
                       : sgq_launch<EP_, SGQ_PREDICT>(M, ci, cq, m, k, metric, splits, tps, rnorm, part, ml))
        switch (M->EP) {
            case 64: SGQ_GO(64); break;
            case 128: SGQ_GO(128); break;
            default: SGQ_GO(256); break;
        }
#undef SGQ_GO
        k_sgm_topk_merge<<<(unsigned)((m + 3) / 4), 256, 0, M->stream>>>(part, ml, m, k, splits, mode, M->d_hdr,
                                                                        o_ids + at * k, o_vals + at * k,
                                                                        o_lse ? o_lse + at : nullptr);
    }
    SGM_TRY(hipGetLastError());
    SGM_TRY(hipEventRecord(M->ev1, M->stream));
    SGM_TRY(hipMemcpyAsync(h, M->d_hdr, sizeof h, hipMemcpyDeviceToHost, M->stream));
    SGM_TRY(hipStreamSynchronize(M->stream));
    float ms = 0.f;
    SGM_TRY(hipEventElapsedTime(&ms, M->ev0, M->ev1));
    M->qstats.kernel_ms += ms;
    if (h[SGMH_ERR] != SGM_NONE) {
        int32_t id = 0;
        SGM_TRY(hipMemcpy(&id, d_ids + h[SGMH_ERR], 4, hipMemcpyDeviceToHost));
        char msg[128];
        snprintf(msg, sizeof msg, "skip-gram model id %d outside [0, %d) (element %lld)", id, M->V,
                 (long long)h[SGMH_ERR]);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    M->qstats.queries += n;
    M->qstats.splits = splits;
    return BPE_OK;
}

// a host form: the input staged in the model's scratch, the device form, the outputs copied back
int sgq_host(bpe_sgmodel *M, int mode, const int32_t *ids, const float *q, int64_t n, int k, int metric,
             int32_t *out_ids, float *out_vals, float *out_lse) {
    if (!n) return sgq_run(M, mode, nullptr, nullptr, 0, k, metric, nullptr, nullptr, nullptr);
    SGM_TRY(hipSetDevice(M->device));
    const int64_t in_bytes = ((ids ? n * 4 : n * M->E * 4) + 15) / 16 * 16, out_bytes = (n * k * 4 + 15) / 16 * 16;
    if (int rc = sgm_grow(&M->d_io, &M->io_cap, in_bytes + 2 * out_bytes + n * 4)) return rc;
    char *d_in = (char *)M->d_io;
    int32_t *d_oi = (int32_t *)(d_in + in_bytes);
    float *d_ov = (float *)(d_in + in_bytes + out_bytes), *d_ol = (float *)(d_in + in_bytes + 2 * out_bytes);
    SGM_TRY(hipMemcpy(d_in, ids ? (const void *)ids : (const void *)q, (size_t)(ids ? n * 4 : n * M->E * 4),
                      hipMemcpyHostToDevice));
    if (int rc = sgq_run(M, mode, ids ? (const int32_t *)d_in : nullptr, ids ? nullptr : (const float *)d_in, n, k, metric,
                         d_oi, d_ov, d_ol))
        return rc;
    SGM_TRY(hipMemcpy(out_ids, d_oi, (size_t)(n * k * 4), hipMemcpyDeviceToHost));
    SGM_TRY(hipMemcpy(out_vals, d_ov, (size_t)(n * k * 4), hipMemcpyDeviceToHost));
    if (out_lse) SGM_TRY(hipMemcpy(out_lse, d_ol, (size_t)(n * 4), hipMemcpyDeviceToHost));
    return BPE_OK;
}

}  // namespace

extern "C" {

int bpe_sgmodel_neighbors_device(bpe_sgmodel *M, const int32_t *d_ids, int64_t n, int k, int metric, int32_t *d_out_ids,
                                 float *d_out_scores) {
    if (int rc = sgq_check_args(M, d_ids, n, k, metric, M ? M->E : 0, d_out_ids, d_out_scores)) return rc;
    return sgq_run(M, SGQ_NEIGH, d_ids, nullptr, n, k, metric, d_out_ids, d_out_scores, nullptr);
}

int bpe_sgmodel_neighbors(bpe_sgmodel *M, const int32_t *ids, int64_t n, int k, int metric, int32_t *out_ids,
                          float *out_scores) {
    if (int rc = sgq_check_args(M, ids, n, k, metric, M ? M->E : 0, out_ids, out_scores)) return rc;
    return sgq_host(M, SGQ_NEIGH, ids, nullptr, n, k, metric, out_ids, out_scores, nullptr);
}

int bpe_sgmodel_neighbors_vectors_device(bpe_sgmodel *M, const float *d_q, int64_t n, int64_t embed, int k, int metric,
                                         int32_t *d_out_ids, float *d_out_scores) {
    if (int rc = sgq_check_args(M, d_q, n, k, metric, embed, d_out_ids, d_out_scores)) return rc;
    return sgq_run(M, SGQ_NEIGH, nullptr, d_q, n, k, metric, d_out_ids, d_out_scores, nullptr);
}

int bpe_sgmodel_neighbors_vectors(bpe_sgmodel *M, const float *q, int64_t n, int64_t embed, int k, int metric,
                                  int32_t *out_ids, float *out_scores) {
    if (int rc = sgq_check_args(M, q, n, k, metric, embed, out_ids, out_scores)) return rc;
    return sgq_host(M, SGQ_NEIGH, nullptr, q, n, k, metric, out_ids, out_scores, nullptr);
}

int bpe_sgmodel_predict_device(bpe_sgmodel *M, const int32_t *d_ids, int64_t n, int k, int32_t *d_out_ids,
                               float *d_out_probs, float *d_out_lse) {
    if (int rc = sgq_check_args(M, d_ids, n, k, BPE_SGM_DOT, M ? M->E : 0, d_out_ids, d_out_probs)) return rc;
    return sgq_run(M, SGQ_PREDICT, d_ids, nullptr, n, k, BPE_SGM_DOT, d_out_ids, d_out_probs, d_out_lse);
}

int bpe_sgmodel_predict(bpe_sgmodel *M, const int32_t *ids, int64_t n, int k, int32_t *out_ids, float *out_probs,
                        float *out_lse) {
    if (int rc = sgq_check_args(M, ids, n, k, BPE_SGM_DOT, M ? M->E : 0, out_ids, out_probs)) return rc;
    return sgq_host(M, SGQ_PREDICT, ids, nullptr, n, k, BPE_SGM_DOT, out_ids, out_probs, out_lse);
}

int bpe_sgmodel_get_query_stats(bpe_sgmodel *M, bpe_sgmodel_query_stats *out) {
    if (!M || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = M->qstats;
    return BPE_OK;
}

int bpe_sgmodel_reset_query_stats(bpe_sgmodel *M) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    M->qstats = {};
    return BPE_OK;
}

}  // extern "C"
