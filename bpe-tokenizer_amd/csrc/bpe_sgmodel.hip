// bpe_sgmodel.hip — the skip-gram model on the device (include/bpe.h, "skip-gram model"): one
// full-softmax step of one-hot -> linear(V, E) -> linear(E, V) -> softmax from the count planes of
// bpe_skipgram_counts.hip.h, with no V x V matrix ever written.  DESIGN.md §3o.
//
//   H_t = Ein[t] + b1, z[t,c] = H_t . Eout[c] + b2[c], lse_t = log sum_c exp z[t,c], n_t = sum_c C[t,c],
//   L = (1/P) (sum_t n_t lse_t - sum C[t,c] z[t,c]),  G[t,c] = (n_t exp(z[t,c] - lse_t) - C[t,c]) / P,
//   dH = G Eout (= dEin; db1 its column sums), dEout = G^T H, db2 = column sums of G.
//
// The three V x V x E products go through v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate).  One
// wave owns 32 x 32 output blocks; of an M x K operand A lane l supplies A[l % 32][k + l / 32], of a
// K x N operand B it supplies B[k + l / 32][l % 32], and of the 32 x 32 result it holds, in register
// v, row 8 (v / 4) + 4 (l / 32) + v % 4 of column l % 32.
//
//   k_sgm_index   the planes checked (range, count >= 0, keys strictly ascending): the smallest
//                 offending element by an integer atomicMin;
//   k_sgm_rowsum  one wave per row: rowptr by lower bound over `targets`, n_t, and P (integer add);
//   k_sgm_rows    one workgroup (two waves) per SGM_TILE target rows, a flash-attention forward with
//                 K = V = Eout.  The block's H tile is staged once in LDS, E zero-padded to EP.  Column
//                 blocks of SGM_SUB rows of Eout (and b2) stream through two LDS buffers, the next one
//                 loaded into registers while this one is used (at EP = 256, where O^T alone takes 128
//                 registers, staged into the other buffer behind the products).  Everything is kept transposed so that
//                 a lane owns ONE target (t = l % 32) in every layout: S^T = Eout_tile . H^T puts a
//                 target's 32 logits into its two lanes' registers (row max and row sum: 16 in-lane
//                 steps and one cross-half shuffle), O^T += Eout_tile^T . P^T takes P^T as its B operand
//                 straight from those registers (the order of the k steps follows the accumulator's
//                 row order, so the P tile never goes through LDS), and the rescale of O^T when the
//                 maximum moves is in-lane as well.  The staged tile serves both products.  Then the
//                 waves walk their rows' CSR entries in order: dH_t = (n_t/P) O_t/l_t - sum_c (C/P)
//                 Eout[c], the loss of the row with sum_c C z[t,c] = H_t . (sum_c C Eout[c]) + sum_c C
//                 b2[c], dEin rows, the block's column sums of dH and its loss partial;
//   k_sgm_cols    one workgroup (four waves) per SGM_TILE context columns, its Eout tile resident in LDS.
//                 Row blocks of H stream through with lse and n_t/P (register prefetch; a block without
//                 count entries is skipped on a uniform branch).  S is recomputed, (n_t/P) exp(S - lse_t)
//                 goes to an LDS tile, behind a barrier one lane per row bisects its CSR row for the
//                 column range and subtracts C/P by plain LDS read-modify-write (keys are distinct),
//                 then dEout_J += tile^T . H_I by matrix instructions and db2_J += the tile's column
//                 sums.  No transposed index, no symmetry assumed;
//   k_sgm_reduce  db1 and the loss from the row blocks' partials, in block order;
//   k_sgm_adam    Adam over the flat parameter array, 16 B per access;
//   k_sgm_embed   rows Ein[id] + b1.
// The queries of a trained model (nearest tokens, top contexts) are in bpe_sgquery.hip.h, and the same
// parameters trained with negative sampling instead of the full softmax in bpe_sgns.hip.h, both included below.
// bpe_sgdense.hip.h, included with them, is the second form of both training steps: the counts as a dense
// V x V tile source instead of CSR entries, chosen per model by bpe_sgmodel_set_counts_form.
// bpe_glove.hip.h (GloVe) and bpe_svd.hip.h (PPMI and a truncated SVD of it, the closed form) come at the end,
// and behind them bpe_sgtext.hip.h: what a trained model says about texts (pooled embeddings, log-likelihood).
// No floating-point atomics; every reduction has a fixed order, so results are the same bytes on
// every run and route.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bpe.h"
#include "bpe_multi.h"   // bpe_fail

namespace {

constexpr int SGM_TILE = BPE_SGM_TILE;   // target rows per k_sgm_rows block, context columns per k_sgm_cols block
constexpr int SGM_SUB = 32;              // Eout rows per streamed tile of k_sgm_rows
constexpr int SGM_ROWS_WG = 64 * (SGM_TILE / 32);
constexpr int SGM_COLS_WG = 256;
constexpr int SGM_GL = SGM_TILE + 1;     // row stride of the G tile
constexpr unsigned long long SGM_NONE = ~0ull;
static_assert(SGM_TILE == 64, "k_sgm_cols splits its tile 2 x 2 over four waves");
static_assert(BPE_SGM_MAX_EMBED == 256, "the widest instantiation");
// header words of a call on the device
constexpr int SGMH_ERR = 0;    // the smallest offending element (SGM_NONE: none)
constexpr int SGMH_P = 1;      // P
constexpr int SGMH_LOSS = 2;   // the loss (a double)
constexpr int SGMH_WORDS = 4;

typedef float f16v __attribute__((ext_vector_type(16)));

#define SGM_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return bpe_fail(e_ == hipErrorOutOfMemory ? BPE_ERR_OOM : BPE_ERR_HIP,         \
                            (std::string("bpe native: ") + #expr + ": " +                   \
                             hipGetErrorString(e_)).c_str());                              \
    } while (0)

__device__ __forceinline__ int sgm_acc_row(int v, int half) { return 8 * (v >> 2) + 4 * half + (v & 3); }

__device__ __forceinline__ f16v sgm_mfma(float a, float b, f16v c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__global__ __launch_bounds__(256) void k_sgm_index(const int32_t *__restrict__ tg, const int32_t *__restrict__ cx,
                                                   const int64_t *__restrict__ cnt, int64_t U, int V,
                                                   unsigned long long *hdr) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < U; i += stride) {
        const int32_t t = tg[i], c = cx[i];
        bool bad = (uint32_t)t >= (uint32_t)V || (uint32_t)c >= (uint32_t)V || cnt[i] < 0;
        if (!bad && i > 0)
            bad = (int64_t)t * V + c <= (int64_t)tg[i - 1] * V + cx[i - 1];
        if (bad) atomicMin(&hdr[SGMH_ERR], (unsigned long long)i);
    }
}

__device__ __forceinline__ int64_t sgm_lower_bound(const int32_t *a, int64_t lo, int64_t hi, int32_t x) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_sgm_rowsum(const int32_t *__restrict__ tg, const int64_t *__restrict__ cnt,
                                                    int64_t U, int V, int64_t *__restrict__ rowptr,
                                                    int64_t *__restrict__ n_t, unsigned long long *hdr) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r > V) return;
    const int64_t lo = sgm_lower_bound(tg, 0, U, r);
    if (r == V) {
        if (lane == 0) rowptr[V] = lo;
        return;
    }
    const int64_t hi = sgm_lower_bound(tg, lo, U, r + 1);
    long long s = 0;
    for (int64_t i = lo + lane; i < hi; i += 64) s += cnt[i];
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
        rowptr[r] = lo;
        n_t[r] = s;
        if (s) atomicAdd(&hdr[SGMH_P], (unsigned long long)s);
    }
}

template <int EP>
constexpr size_t sgm_rows_lds() {
    return (size_t)(2 * SGM_TILE * (EP + 1) + 2 * SGM_SUB + SGM_TILE) * 4 + (SGM_TILE / 32) * 8;
}

template <int EP>
__global__ __launch_bounds__(SGM_ROWS_WG) void k_sgm_rows(
    const float *__restrict__ Ein, const float *__restrict__ b1, const float *__restrict__ Eout,
    const float *__restrict__ b2, int V, int E, const int64_t *__restrict__ rowptr, const int64_t *__restrict__ n_t,
    const unsigned long long *__restrict__ hdr, const int32_t *__restrict__ cx, const int64_t *__restrict__ cnt,
    float *__restrict__ lse_out, float *__restrict__ dEin, float *__restrict__ db1_part,
    double *__restrict__ loss_part) {
    constexpr int LD = EP + 1;                       // odd: a column of 32 rows touches 32 banks
    constexpr int NPRE = SGM_SUB * EP / SGM_ROWS_WG; // staged floats per thread and tile
    constexpr int NEB = EP / 32;
    constexpr int NW = SGM_TILE / 32;
    extern __shared__ float smem[];
    float *Hs = smem;                         // [SGM_TILE][LD]
    float *Es = Hs + SGM_TILE * LD;           // [2][SGM_SUB][LD]; after the stream: O / l, then dH, [SGM_TILE][LD]
    float *b2s = Es + 2 * SGM_SUB * LD;       // [2][SGM_SUB]
    float *lses = b2s + 2 * SGM_SUB;          // [SGM_TILE]
    double *wloss = (double *)(lses + SGM_TILE);   // [NW]
    static_assert((2 * SGM_TILE * LD + 2 * SGM_SUB + SGM_TILE) % 2 == 0, "wloss is 8-byte aligned");

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane & 31, half = lane >> 5;
    const int I0 = blockIdx.x * SGM_TILE;
    const int nrows = min(SGM_TILE, V - I0);
    const int Ek = (E + 1) & ~1;
    const int n_tiles = (V + SGM_SUB - 1) / SGM_SUB;

    for (int idx = tid; idx < SGM_TILE * EP; idx += SGM_ROWS_WG) {
        const int r = idx / EP, e = idx % EP;
        Hs[r * LD + e] = (r < nrows && e < E) ? Ein[(size_t)(I0 + r) * E + e] + b1[e] : 0.f;
    }

    // EP <= 128: the next tile waits in registers while this one is used; EP == 256 has no registers
    // to spare for that (O^T alone is 128) and stages the next tile behind the products instead
    constexpr bool PRE = EP <= 128;
    float pre[PRE ? NPRE : 1], pre_b = 0.f;
    auto tile_value = [&](int j, int idx) {
        const int r = idx / EP, e = idx % EP, c = j * SGM_SUB + r;
        return (c < V && e < E) ? Eout[(size_t)c * E + e] : 0.f;
    };
    auto tile_bias = [&](int j) { return (j * SGM_SUB + tid < V) ? b2[j * SGM_SUB + tid] : -INFINITY; };
    auto load_tile = [&](int j) {
#pragma unroll
        for (int i = 0; i < (PRE ? NPRE : 0); ++i) pre[i] = tile_value(j, tid + i * SGM_ROWS_WG);
        if (tid < SGM_SUB) pre_b = tile_bias(j);
    };
    auto store_tile = [&](int buf) {
        float *Eb = Es + buf * SGM_SUB * LD;
#pragma unroll
        for (int i = 0; i < (PRE ? NPRE : 0); ++i) {
            const int idx = tid + i * SGM_ROWS_WG;
            Eb[(idx / EP) * LD + idx % EP] = pre[i];
        }
        if (tid < SGM_SUB) b2s[buf * SGM_SUB + tid] = pre_b;
    };
    auto stage_tile = [&](int j, int buf) {
        float *Eb = Es + buf * SGM_SUB * LD;
#pragma unroll 8
        for (int i = 0; i < NPRE; ++i) {
            const int idx = tid + i * SGM_ROWS_WG;
            Eb[(idx / EP) * LD + idx % EP] = tile_value(j, idx);
        }
        if (tid < SGM_SUB) b2s[buf * SGM_SUB + tid] = tile_bias(j);
    };

    f16v O[NEB];
#pragma unroll
    for (int eb = 0; eb < NEB; ++eb)
#pragma unroll
        for (int v = 0; v < 16; ++v) O[eb][v] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const float *Hw = Hs + (w * 32 + q) * LD + half;

    if (PRE) load_tile(0);
    else stage_tile(0, 0);
    for (int j = 0; j < n_tiles; ++j) {
        if (PRE) store_tile(j & 1);
        __syncthreads();
        if (PRE && j + 1 < n_tiles) load_tile(j + 1);
        const float *Eb = Es + (j & 1) * SGM_SUB * LD;
        const float *bb = b2s + (j & 1) * SGM_SUB;
        // S^T[c][t] = sum_k Eout[c][k] H[t][k]
        f16v s;
#pragma unroll
        for (int v = 0; v < 16; ++v) s[v] = 0.f;
        const float *Ea = Eb + q * LD + half;
        for (int k = 0; k < Ek; k += 2) s = sgm_mfma(Ea[k], Hw[k], s);
        float mx = -INFINITY;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            s[v] += bb[sgm_acc_row(v, half)];
            mx = fmaxf(mx, s[v]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = expf(m_run - m_new);   // (0 on the first tile: m_run is -inf, m_new is not)
        float ps = 0.f;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            s[v] = expf(s[v] - m_new);
            ps += s[v];
        }
        ps += __shfl_xor(ps, 32, 64);
        l_run = l_run * alpha + ps;
        m_run = m_new;
        // O^T[e][t] = alpha O^T[e][t] + sum_c Eout[c][e] P[t][c]; k step v takes the c of register v
#pragma unroll
        for (int eb = 0; eb < NEB; ++eb) {
            if (eb * 32 < E) {
#pragma unroll
                for (int v = 0; v < 16; ++v) O[eb][v] *= alpha;
#pragma unroll
                for (int v = 0; v < 16; ++v)
                    O[eb] = sgm_mfma(Eb[sgm_acc_row(v, half) * LD + eb * 32 + q], s[v], O[eb]);
            }
        }
        // (the other buffer was last read before this iteration's barrier)
        if (!PRE && j + 1 < n_tiles) stage_tile(j + 1, (j + 1) & 1);
    }
    __syncthreads();   // the last tile has been read by every wave: Es becomes Os

    float *Os = Es;
    {
        const float inv_l = 1.f / l_run;
#pragma unroll
        for (int eb = 0; eb < NEB; ++eb)
#pragma unroll
            for (int v = 0; v < 16; ++v)
                Os[(w * 32 + q) * LD + eb * 32 + sgm_acc_row(v, half)] = O[eb][v] * inv_l;
        if (half == 0) {
            const float lse = m_run + logf(l_run);
            lses[w * 32 + q] = lse;
            if (w * 32 + q < nrows) lse_out[I0 + w * 32 + q] = lse;
        }
    }
    __syncthreads();

    // the rows' count entries, in order; lanes over e
    const double inv_P = 1.0 / (double)(long long)hdr[SGMH_P];
    double wl = 0.0;
    for (int r = w * 32; r < min(nrows, w * 32 + 32); ++r) {
        const int t = I0 + r;
        const int64_t beg = rowptr[t], end = rowptr[t + 1];
        const double wn = (double)n_t[t] * inv_P;
        float acc[(EP + 63) / 64];
#pragma unroll
        for (int x = 0; x < (EP + 63) / 64; ++x) acc[x] = 0.f;
        double bsum = 0.0;
        for (int64_t i = beg; i < end; ++i) {
            const int c = cx[i];
            const double wd = (double)cnt[i] * inv_P;
            const float wc = (float)wd;
            bsum += wd * (double)b2[c];
#pragma unroll
            for (int x = 0; x < (EP + 63) / 64; ++x) {
                const int e = lane + 64 * x;
                if (e < E) acc[x] += wc * Eout[(size_t)c * E + e];
            }
        }
        float dot = 0.f;
#pragma unroll
        for (int x = 0; x < (EP + 63) / 64; ++x) {
            const int e = lane + 64 * x;
            if (e < EP) {
                dot += Hs[r * LD + e] * acc[x];
                const float dh = (float)wn * Os[r * LD + e] - acc[x];
                Os[r * LD + e] = dh;
                if (e < E) dEin[(size_t)t * E + e] = dh;
            }
        }
        for (int o = 32; o; o >>= 1) dot += __shfl_xor(dot, o, 64);
        wl += wn * (double)lses[r] - (double)dot - bsum;
    }
    if (lane == 0) wloss[w] = wl;
    __syncthreads();
    for (int e = tid; e < EP; e += SGM_ROWS_WG) {
        float s = 0.f;
        for (int r = 0; r < nrows; ++r) s += Os[r * LD + e];
        db1_part[(size_t)blockIdx.x * EP + e] = s;
    }
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < NW; ++i) s += wloss[i];
        loss_part[blockIdx.x] = s;
    }
}

template <int EP>
constexpr size_t sgm_cols_lds() {
    return (size_t)(2 * SGM_TILE * (EP + 1) + SGM_TILE * SGM_GL + 3 * SGM_TILE) * 4;
}

template <int EP>
__global__ __launch_bounds__(SGM_COLS_WG) void k_sgm_cols(
    const float *__restrict__ Ein, const float *__restrict__ b1, const float *__restrict__ Eout,
    const float *__restrict__ b2, int V, int E, const int64_t *__restrict__ rowptr, const int64_t *__restrict__ n_t,
    const unsigned long long *__restrict__ hdr, const int32_t *__restrict__ cx, const int64_t *__restrict__ cnt,
    const float *__restrict__ lse, float *__restrict__ dEout, float *__restrict__ db2) {
    constexpr int LD = EP + 1;
    constexpr int NPRE = SGM_TILE * EP / SGM_COLS_WG;
    constexpr int NACC = EP / 64;   // 32-wide e blocks per wave
    extern __shared__ float smem[];
    float *Ecs = smem;                       // [SGM_TILE][LD]: Eout rows J0 ..
    float *Hs = Ecs + SGM_TILE * LD;         // [SGM_TILE][LD]: the row block's H
    float *Gt = Hs + SGM_TILE * LD;          // [SGM_TILE][SGM_GL]: the G tile, [t][c]
    float *lses = Gt + SGM_TILE * SGM_GL;    // [SGM_TILE]
    float *wns = lses + SGM_TILE;            // [SGM_TILE]: n_t / P
    float *b2s = wns + SGM_TILE;             // [SGM_TILE]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane & 31, half = lane >> 5;
    const int J0 = blockIdx.x * SGM_TILE;
    const int Ek = (E + 1) & ~1;
    const int n_blocks = (V + SGM_TILE - 1) / SGM_TILE;
    const double inv_P = 1.0 / (double)(long long)hdr[SGMH_P];

    for (int idx = tid; idx < SGM_TILE * EP; idx += SGM_COLS_WG) {
        const int r = idx / EP, e = idx % EP;
        Ecs[r * LD + e] = (J0 + r < V && e < E) ? Eout[(size_t)(J0 + r) * E + e] : 0.f;
    }
    if (tid < SGM_TILE) b2s[tid] = (J0 + tid < V) ? b2[J0 + tid] : 0.f;

    float pre[NPRE], pre_lse = 0.f, pre_wn = 0.f;
    auto load_block = [&](int ib) {
        const int I0 = ib * SGM_TILE;
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int idx = tid + i * SGM_COLS_WG, r = idx / EP, e = idx % EP;
            pre[i] = (I0 + r < V && e < E) ? Ein[(size_t)(I0 + r) * E + e] + b1[e] : 0.f;
        }
        if (tid < SGM_TILE) {
            const bool in = I0 + tid < V;
            pre_lse = in ? lse[I0 + tid] : 0.f;
            pre_wn = in ? (float)((double)n_t[I0 + tid] * inv_P) : 0.f;
        }
    };
    auto next_block = [&](int ib) {   // the first row block from ib on that has count entries (uniform)
        while (ib < n_blocks && rowptr[min(V, (ib + 1) * SGM_TILE)] == rowptr[ib * SGM_TILE]) ++ib;
        return ib;
    };

    f16v acc[NACC];
#pragma unroll
    for (int x = 0; x < NACC; ++x)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[x][v] = 0.f;
    float db2_acc = 0.f;
    const int th = w & 1, ch = w >> 1;   // the S quadrant of this wave: rows 32 th .., columns 32 ch ..
    const int gc = w & 1, ge = w >> 1;   // of dEout: columns 32 gc .., e blocks ge, ge + 2, ..

    int ib = next_block(0);
    if (ib < n_blocks) load_block(ib);
    while (ib < n_blocks) {
        const int I0 = ib * SGM_TILE;
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int idx = tid + i * SGM_COLS_WG;
            Hs[(idx / EP) * LD + idx % EP] = pre[i];
        }
        if (tid < SGM_TILE) {
            lses[tid] = pre_lse;
            wns[tid] = pre_wn;
        }
        __syncthreads();
        const int nx = next_block(ib + 1);
        if (nx < n_blocks) load_block(nx);

        // S[t][c] = sum_k H[t][k] Eout[c][k]; lane: c = 32 ch + q, rows by register
        {
            f16v s;
#pragma unroll
            for (int v = 0; v < 16; ++v) s[v] = 0.f;
            const float *Ha = Hs + (th * 32 + q) * LD + half;
            const float *Eb = Ecs + (ch * 32 + q) * LD + half;
            for (int k = 0; k < Ek; k += 2) s = sgm_mfma(Ha[k], Eb[k], s);
            const int c = ch * 32 + q;
            const bool c_in = J0 + c < V;
            const float bc = b2s[c];
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int t = th * 32 + sgm_acc_row(v, half);
                const float wn = wns[t];
                Gt[t * SGM_GL + c] = (wn > 0.f && c_in) ? wn * expf(s[v] + bc - lses[t]) : 0.f;
            }
        }
        __syncthreads();
        // the counts that fall into the tile: one lane per row, its CSR row bisected for J0
        if (tid < SGM_TILE && I0 + tid < V) {
            const int64_t end = rowptr[I0 + tid + 1];
            for (int64_t i = sgm_lower_bound(cx, rowptr[I0 + tid], end, J0); i < end; ++i) {
                const int c = cx[i] - J0;
                if (c >= SGM_TILE) break;
                Gt[tid * SGM_GL + c] -= (float)((double)cnt[i] * inv_P);
            }
        }
        __syncthreads();
        // dEout[c][e] += sum_t G[t][c] H[t][e]
        {
            const float *Ga = Gt + half * SGM_GL + gc * 32 + q;
            const float *Hb = Hs + half * LD + q;
            for (int k = 0; k < SGM_TILE; k += 2) {
                const float a = Ga[k * SGM_GL];
#pragma unroll
                for (int x = 0; x < NACC; ++x)
                    if ((ge + 2 * x) * 32 < E) acc[x] = sgm_mfma(a, Hb[k * LD + (ge + 2 * x) * 32], acc[x]);
            }
        }
        if (tid < SGM_TILE) {
            float s = 0.f;
            for (int r = 0; r < SGM_TILE; ++r) s += Gt[r * SGM_GL + tid];
            db2_acc += s;
        }
        __syncthreads();
        ib = nx;
    }

#pragma unroll
    for (int x = 0; x < NACC; ++x) {
        const int e = (ge + 2 * x) * 32 + q;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int c = J0 + gc * 32 + sgm_acc_row(v, half);
            if (c < V && e < E) dEout[(size_t)c * E + e] = acc[x][v];
        }
    }
    if (tid < SGM_TILE && J0 + tid < V) db2[J0 + tid] = db2_acc;
}

// db1[e] and the loss from the row blocks' partials, in block order
__global__ __launch_bounds__(256) void k_sgm_reduce(const float *__restrict__ db1_part, const double *__restrict__ loss_part,
                                                    int n_blocks, int EP, int E, float *__restrict__ db1,
                                                    unsigned long long *hdr) {
    const int e = threadIdx.x;
    if (e < E) {
        float s = 0.f;
        for (int b = 0; b < n_blocks; ++b) s += db1_part[(size_t)b * EP + e];
        db1[e] = s;
    }
    if (e == 255) {
        double s = 0.0;
        for (int b = 0; b < n_blocks; ++b) s += loss_part[b];
        hdr[SGMH_LOSS] = (unsigned long long)__double_as_longlong(s);
    }
}

// Adam (Kingma & Ba) with bias correction: c1 = 1 / (1 - beta1^t), c2 = 1 / (1 - beta2^t).  The pass is
// bound by its 28 bytes per parameter, so the arithmetic is done in double and rounded once per store:
// 1 - beta2 = 0.001 taken in fp32 from fp32 0.999 is already 1.3e-5 off.
__global__ __launch_bounds__(256) void k_sgm_adam(float4 *__restrict__ p, const float4 *__restrict__ g,
                                                  float4 *__restrict__ m, float4 *__restrict__ v, int64_t n4, double lr,
                                                  double beta1, double beta2, double eps, double c1, double c2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 P = p[i], M = m[i], W = v[i];
    const float4 G = g[i];
    auto one = [&](float &pp, float &mm, float &vv, float gg) {
        const double m1 = beta1 * (double)mm + (1.0 - beta1) * (double)gg;
        const double v1 = beta2 * (double)vv + (1.0 - beta2) * (double)gg * (double)gg;
        mm = (float)m1;
        vv = (float)v1;
        pp = (float)((double)pp - lr * (m1 * c1) / (sqrt(v1 * c2) + eps));
    };
    one(P.x, M.x, W.x, G.x);
    one(P.y, M.y, W.y, G.y);
    one(P.z, M.z, W.z, G.z);
    one(P.w, M.w, W.w, G.w);
    p[i] = P;
    m[i] = M;
    v[i] = W;
}

__global__ __launch_bounds__(256) void k_sgm_embed(const float *__restrict__ Ein, const float *__restrict__ b1,
                                                   const int32_t *__restrict__ ids, int64_t n, int V, int E,
                                                   float *__restrict__ out, unsigned long long *hdr) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * E) return;
    const int64_t i = idx / E;
    const int e = (int)(idx % E);
    const int32_t id = ids[i];
    if ((uint32_t)id >= (uint32_t)V) {
        if (e == 0) atomicMin(&hdr[SGMH_ERR], (unsigned long long)i);
        return;
    }
    out[idx] = Ein[(size_t)id * E + e] + b1[e];
}

}  // namespace

struct bpe_sgmodel {
    int device = 0, V = 0, E = 0, EP = 0, n_blocks = 0;
    int64_t n_params = 0, n4 = 0;            // 2VE + V + E, and the float4s that hold them
    int64_t o_ein = 0, o_b1 = 0, o_eout = 0, o_b2 = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float *d_p = nullptr, *d_g = nullptr, *d_m = nullptr, *d_v = nullptr;   // flat: Ein | b1 | Eout | b2
    int64_t *d_rowptr = nullptr, *d_nt = nullptr;
    float *d_lse = nullptr, *d_db1_part = nullptr;
    double *d_loss_part = nullptr;
    unsigned long long *d_hdr = nullptr;
    // grow-only scratch of the host forms
    void *d_planes = nullptr;
    int64_t planes_cap = 0;
    void *d_io = nullptr;
    int64_t io_cap = 0;
    int64_t step = 0;
    bpe_sgmodel_stats stats = {};
    // the queries (bpe_sgquery.hip.h): norms, partial lists and (max, sum) partials, grow-only
    void *d_qs = nullptr;
    int64_t qs_cap = 0;
    int n_cus = 1;
    bpe_sgmodel_query_stats qstats = {};
    // negative sampling (bpe_sgns.hip.h): transposed planes and partials, grow-only
    void *d_ns = nullptr;
    int64_t ns_cap = 0;
    hipEvent_t nev[4] = {nullptr, nullptr, nullptr, nullptr};
    bpe_sgmodel_sgns_stats nstats = {};
    // the dense-count form (bpe_sgdense.hip.h): W and omega, allocated on the first dense call; partials, grow-only
    int form = BPE_SGM_FORM_CSR, form_splits = 0;
    float *d_W = nullptr;
    void *d_ds = nullptr;
    int64_t ds_cap = 0;
    bpe_sgmodel_dense_stats dstats = {};
    // GloVe (bpe_glove.hip.h): the target bias bt[V] with its gradient and Adam moments (bt4 float4s each), in
    // buffers of their own beside the flat array; the call's scratch, grow-only
    int64_t bt4 = 0;
    float *d_bt = nullptr, *d_gbt = nullptr, *d_mbt = nullptr, *d_vbt = nullptr;
    void *d_gs = nullptr;
    int64_t gs_cap = 0;
    bpe_sgmodel_glove_stats gstats = {};
    // PPMI and SVD (bpe_svd.hip.h): the call's scratch, grow-only, and the events between its phases
    void *d_ss = nullptr;
    int64_t ss_cap = 0;
    bool svd_attrs = false;
    std::vector<hipEvent_t> sev;
    bpe_sgmodel_svd_stats sstats = {};
    // texts (bpe_sgtext.hip.h): the scanned item counts and the partials of the long texts, grow-only
    void *d_ts = nullptr, *d_tp = nullptr;
    int64_t ts_cap = 0, tp_cap = 0;
    bpe_sgmodel_text_stats tstats = {};
};

namespace {

template <int EP>
hipError_t sgm_lds_attrs() {
    hipError_t e = hipFuncSetAttribute((const void *)k_sgm_rows<EP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)sgm_rows_lds<EP>());
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void *)k_sgm_cols<EP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)sgm_cols_lds<EP>());
}
static_assert(sgm_rows_lds<256>() <= 160 * 1024 && sgm_cols_lds<256>() <= 160 * 1024, "LDS of the widest kernels");

template <int EP>
void sgm_launch(bpe_sgmodel *M, const int32_t *d_c, const int64_t *d_k) {
    const float *p = M->d_p;
    float *g = M->d_g;
    k_sgm_rows<EP><<<M->n_blocks, SGM_ROWS_WG, sgm_rows_lds<EP>(), M->stream>>>(
        p + M->o_ein, p + M->o_b1, p + M->o_eout, p + M->o_b2, M->V, M->E, M->d_rowptr, M->d_nt, M->d_hdr, d_c, d_k,
        M->d_lse, g + M->o_ein, M->d_db1_part, M->d_loss_part);
    k_sgm_cols<EP><<<M->n_blocks, SGM_COLS_WG, sgm_cols_lds<EP>(), M->stream>>>(
        p + M->o_ein, p + M->o_b1, p + M->o_eout, p + M->o_b2, M->V, M->E, M->d_rowptr, M->d_nt, M->d_hdr, d_c, d_k,
        M->d_lse, g + M->o_eout, g + M->o_b2);
    k_sgm_reduce<<<1, 256, 0, M->stream>>>(M->d_db1_part, M->d_loss_part, M->n_blocks, EP, M->E, g + M->o_b1,
                                          M->d_hdr);
}

int sgm_grow(void **buf, int64_t *cap, int64_t bytes) {
    if (bytes <= *cap) return BPE_OK;
    void *nb = nullptr;
    if (hipMalloc(&nb, (size_t)bytes) != hipSuccess) {
        (void)hipGetLastError();
        return bpe_fail(BPE_ERR_OOM, "bpe native: skip-gram model scratch");
    }
    if (*buf) (void)hipFree(*buf);
    *buf = nb;
    *cap = bytes;
    return BPE_OK;
}

int sgm_time(bpe_sgmodel *M, double *acc) {
    float ms = 0.f;
    SGM_TRY(hipEventElapsedTime(&ms, M->ev0, M->ev1));
    *acc += ms;
    return BPE_OK;
}

// the offending element's message (the kernel's order of checks)
int sgm_bad_element(bpe_sgmodel *M, const int32_t *d_t, const int32_t *d_c, const int64_t *d_k, int64_t i) {
    int32_t t[2] = {0, 0}, c[2] = {0, 0};
    int64_t k = 0;
    const int64_t from = i > 0 ? i - 1 : i;
    SGM_TRY(hipMemcpy(t + (i > 0 ? 0 : 1), d_t + from, (size_t)(i - from + 1) * 4, hipMemcpyDeviceToHost));
    SGM_TRY(hipMemcpy(c + (i > 0 ? 0 : 1), d_c + from, (size_t)(i - from + 1) * 4, hipMemcpyDeviceToHost));
    SGM_TRY(hipMemcpy(&k, d_k + i, 8, hipMemcpyDeviceToHost));
    char msg[160];
    if (t[1] < 0 || t[1] >= M->V)
        snprintf(msg, sizeof msg, "skip-gram model target %d outside [0, %d) (element %lld)", t[1], M->V, (long long)i);
    else if (c[1] < 0 || c[1] >= M->V)
        snprintf(msg, sizeof msg, "skip-gram model context %d outside [0, %d) (element %lld)", c[1], M->V, (long long)i);
    else if (k < 0)
        snprintf(msg, sizeof msg, "skip-gram model count %lld is negative (element %lld)", (long long)k, (long long)i);
    else if (t[0] == t[1] && c[0] == c[1])
        snprintf(msg, sizeof msg, "skip-gram model pair (%d, %d) is given twice (element %lld)", t[1], c[1], (long long)i);
    else
        snprintf(msg, sizeof msg, "skip-gram model pairs must ascend: (%d, %d) after (%d, %d) (element %lld)", t[1], c[1],
                 t[0], c[0], (long long)i);
    return bpe_fail(BPE_ERR_ARG, msg);
}

// the planes checked, rowptr, n_t and P (left in the header on the device too); the kernels' time onto *ms
int sgm_index(bpe_sgmodel *M, const int32_t *d_t, const int32_t *d_c, const int64_t *d_k, int64_t U, int64_t *P,
              double *ms) {
    unsigned long long h[SGMH_WORDS] = {SGM_NONE, 0, 0, 0};
    SGM_TRY(hipMemcpyAsync(M->d_hdr, h, sizeof h, hipMemcpyHostToDevice, M->stream));
    SGM_TRY(hipEventRecord(M->ev0, M->stream));
    if (U) {
        const int64_t nb = (U + 255) / 256;
        k_sgm_index<<<(unsigned)(nb < 4096 ? nb : 4096), 256, 0, M->stream>>>(d_t, d_c, d_k, U, M->V, M->d_hdr);
    }
    k_sgm_rowsum<<<(M->V + 1 + 3) / 4, 256, 0, M->stream>>>(d_t, d_k, U, M->V, M->d_rowptr, M->d_nt, M->d_hdr);
    SGM_TRY(hipGetLastError());
    SGM_TRY(hipEventRecord(M->ev1, M->stream));
    SGM_TRY(hipMemcpyAsync(h, M->d_hdr, sizeof h, hipMemcpyDeviceToHost, M->stream));
    SGM_TRY(hipStreamSynchronize(M->stream));
    if (int rc = sgm_time(M, ms)) return rc;
    if (h[SGMH_ERR] != SGM_NONE) return sgm_bad_element(M, d_t, d_c, d_k, (int64_t)h[SGMH_ERR]);
    *P = (int64_t)h[SGMH_P];
    return BPE_OK;
}

// the dense-count form (bpe_sgdense.hip.h)
bool sgd_wanted(const bpe_sgmodel *M, int64_t U);
int sgd_run(bpe_sgmodel *M, bool sgns, const int32_t *d_t, const int32_t *d_c, const int64_t *d_k, int64_t U,
            const int32_t *d_ids, const float *d_w, int S, double neg_k);

// loss and gradients (into the model's gradient array) from device planes; *loss on the host
int sgm_forward(bpe_sgmodel *M, const int32_t *d_t, const int32_t *d_c, const int64_t *d_k, int64_t U, double *loss) {
    M->stats.calls++;
    M->dstats.calls++;
    if (U < 0 || (U && (!d_t || !d_c || !d_k))) return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model planes");
    SGM_TRY(hipSetDevice(M->device));
    int64_t P = 0;
    if (int rc = sgm_index(M, d_t, d_c, d_k, U, &P, &M->stats.kernel_ms)) return rc;
    unsigned long long h[SGMH_WORDS];
    const bool dense = P && sgd_wanted(M, U);
    SGM_TRY(hipEventRecord(M->ev0, M->stream));
    if (P == 0) {
        SGM_TRY(hipMemsetAsync(M->d_g, 0, (size_t)M->n4 * 16, M->stream));
    } else if (dense) {
        if (int rc = sgd_run(M, false, d_t, d_c, d_k, U, nullptr, nullptr, 0, 0.0)) return rc;
    } else {
        M->dstats.last_form = BPE_SGM_FORM_CSR;
        M->dstats.last_splits = 0;
        switch (M->EP) {
            case 64: sgm_launch<64>(M, d_c, d_k); break;
            case 128: sgm_launch<128>(M, d_c, d_k); break;
            default: sgm_launch<256>(M, d_c, d_k); break;
        }
        SGM_TRY(hipGetLastError());
    }
    SGM_TRY(hipEventRecord(M->ev1, M->stream));
    SGM_TRY(hipMemcpyAsync(h, M->d_hdr, sizeof h, hipMemcpyDeviceToHost, M->stream));
    SGM_TRY(hipStreamSynchronize(M->stream));
    double ms = 0.0;
    if (int rc = sgm_time(M, &ms)) return rc;
    M->stats.kernel_ms += ms;
    if (dense) M->dstats.kernel_ms += ms;
    double L = 0.0;
    std::memcpy(&L, &h[SGMH_LOSS], 8);
    if (loss) *loss = P ? L : 0.0;
    M->stats.elements += U;
    M->stats.pairs += P;
    return BPE_OK;
}

int sgm_adam(bpe_sgmodel *M, double lr, double beta1, double beta2, double eps, double *ms) {
    M->step++;
    const double c1 = 1.0 / (1.0 - std::pow(beta1, (double)M->step));
    const double c2 = 1.0 / (1.0 - std::pow(beta2, (double)M->step));
    SGM_TRY(hipEventRecord(M->ev0, M->stream));
    k_sgm_adam<<<(unsigned)((M->n4 + 255) / 256), 256, 0, M->stream>>>((float4 *)M->d_p, (const float4 *)M->d_g,
                                                                      (float4 *)M->d_m, (float4 *)M->d_v, M->n4, lr, beta1,
                                                                      beta2, eps, c1, c2);
    SGM_TRY(hipGetLastError());
    SGM_TRY(hipEventRecord(M->ev1, M->stream));
    SGM_TRY(hipStreamSynchronize(M->stream));
    return sgm_time(M, ms);
}

// the planes of a host form, in the model's scratch
int sgm_stage(bpe_sgmodel *M, const int32_t *t, const int32_t *c, const int64_t *k, int64_t U, const int32_t **d_t,
              const int32_t **d_c, const int64_t **d_k) {
    *d_t = *d_c = nullptr;
    *d_k = nullptr;
    if (U <= 0 || !t || !c || !k) return BPE_OK;   // (sgm_forward refuses what is wrong)
    SGM_TRY(hipSetDevice(M->device));
    if (int rc = sgm_grow(&M->d_planes, &M->planes_cap, U * 16)) return rc;
    int64_t *dk = (int64_t *)M->d_planes;
    int32_t *dt = (int32_t *)(dk + U), *dc = dt + U;
    SGM_TRY(hipMemcpy(dk, k, (size_t)U * 8, hipMemcpyHostToDevice));
    SGM_TRY(hipMemcpy(dt, t, (size_t)U * 4, hipMemcpyHostToDevice));
    SGM_TRY(hipMemcpy(dc, c, (size_t)U * 4, hipMemcpyHostToDevice));
    *d_t = dt;
    *d_c = dc;
    *d_k = dk;
    return BPE_OK;
}

// the four sections of a flat array to or from the caller's (NULL sections are skipped)
int sgm_copy_sections(bpe_sgmodel *M, float *flat, float *ein, float *b1, float *eout, float *b2, bool to_flat,
                      hipMemcpyKind kind) {
    const int64_t VE = (int64_t)M->V * M->E;
    struct { float *ptr; int64_t off, n; } s[4] = {{ein, M->o_ein, VE}, {b1, M->o_b1, M->E}, {eout, M->o_eout, VE},
                                                   {b2, M->o_b2, M->V}};
    for (auto &x : s) {
        if (!x.ptr) continue;
        if (to_flat) SGM_TRY(hipMemcpyAsync(flat + x.off, x.ptr, (size_t)x.n * 4, kind, M->stream));
        else SGM_TRY(hipMemcpyAsync(x.ptr, flat + x.off, (size_t)x.n * 4, kind, M->stream));
    }
    SGM_TRY(hipStreamSynchronize(M->stream));
    return BPE_OK;
}

int sgm_params(bpe_sgmodel *M, float *ein, float *b1, float *eout, float *b2, int64_t dim, int64_t embed, bool set,
               bool dev) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (dim != M->V || embed != M->E) {
        char msg[160];
        snprintf(msg, sizeof msg, "skip-gram model parameters of %lld x %lld given to a model of %d x %d", (long long)dim,
                 (long long)embed, M->V, M->E);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    if (!ein || !b1 || !eout || !b2) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model parameters");
    SGM_TRY(hipSetDevice(M->device));
    return sgm_copy_sections(M, M->d_p, ein, b1, eout, b2, set,
                             dev ? hipMemcpyDeviceToDevice : set ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost);
}

int sgm_embed(bpe_sgmodel *M, const int32_t *d_ids, int64_t n, float *d_out) {
    unsigned long long h[SGMH_WORDS] = {SGM_NONE, 0, 0, 0};
    SGM_TRY(hipMemcpyAsync(M->d_hdr, h, sizeof h, hipMemcpyHostToDevice, M->stream));
    const int64_t total = n * M->E;
    k_sgm_embed<<<(unsigned)((total + 255) / 256), 256, 0, M->stream>>>(M->d_p + M->o_ein, M->d_p + M->o_b1, d_ids, n,
                                                                       M->V, M->E, d_out, M->d_hdr);
    SGM_TRY(hipGetLastError());
    SGM_TRY(hipMemcpyAsync(h, M->d_hdr, sizeof h, hipMemcpyDeviceToHost, M->stream));
    SGM_TRY(hipStreamSynchronize(M->stream));
    if (h[SGMH_ERR] != SGM_NONE) {
        int32_t id = 0;
        SGM_TRY(hipMemcpy(&id, d_ids + h[SGMH_ERR], 4, hipMemcpyDeviceToHost));
        char msg[128];
        snprintf(msg, sizeof msg, "skip-gram model id %d outside [0, %d) (element %lld)", id, M->V,
                 (long long)h[SGMH_ERR]);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    return BPE_OK;
}

}  // namespace

#include "bpe_sgquery.hip.h"
#include "bpe_sgns.hip.h"
#include "bpe_sgdense.hip.h"

extern "C" {

int bpe_sgmodel_create(int device, int dim, int embed, bpe_sgmodel **out) {
    if (!out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = nullptr;
    char msg[128];
    if (dim < 1 || dim > BPE_SKIPGRAM_COUNTS_MAX_DIM) {
        snprintf(msg, sizeof msg, "skip-gram model dim %d outside [1, %d]", dim, BPE_SKIPGRAM_COUNTS_MAX_DIM);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    if (embed < 1 || embed > BPE_SGM_MAX_EMBED) {
        snprintf(msg, sizeof msg, "skip-gram model embed %d outside [1, %d]", embed, BPE_SGM_MAX_EMBED);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return bpe_fail(BPE_ERR_HIP, "bpe native: no HIP device available (MI355X required)");
    if (device < 0 || device >= n) return bpe_fail(BPE_ERR_ARG, "bpe native: bad device index");
    bpe_sgmodel *M = new bpe_sgmodel();
    M->device = device;
    M->V = dim;
    M->E = embed;
    M->EP = embed <= 64 ? 64 : embed <= 128 ? 128 : 256;
    M->n_blocks = (dim + SGM_TILE - 1) / SGM_TILE;
    const int64_t VE = (int64_t)dim * embed;
    M->o_ein = 0;
    M->o_b1 = VE;
    M->o_eout = VE + embed;
    M->o_b2 = 2 * VE + embed;
    M->n_params = 2 * VE + embed + dim;
    M->n4 = (M->n_params + 3) / 4;
    M->bt4 = ((int64_t)dim + 3) / 4;
    auto bail = [&](int rc) {
        bpe_sgmodel_destroy(M);
        return rc;
    };
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&M->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&M->ev0) != hipSuccess || hipEventCreate(&M->ev1) != hipSuccess ||
        hipEventCreate(&M->nev[0]) != hipSuccess || hipEventCreate(&M->nev[1]) != hipSuccess ||
        hipEventCreate(&M->nev[2]) != hipSuccess || hipEventCreate(&M->nev[3]) != hipSuccess)
        return bail(bpe_fail(BPE_ERR_HIP, "bpe native: skip-gram model stream/events"));
    const size_t flat = (size_t)M->n4 * 16;
    bool ok = true;
    for (float **p : {&M->d_p, &M->d_g, &M->d_m, &M->d_v})
        ok = ok && hipMalloc((void **)p, flat) == hipSuccess && hipMemset(*p, 0, flat) == hipSuccess;
    for (float **p : {&M->d_bt, &M->d_gbt, &M->d_mbt, &M->d_vbt})
        ok = ok && hipMalloc((void **)p, (size_t)M->bt4 * 16) == hipSuccess &&
             hipMemset(*p, 0, (size_t)M->bt4 * 16) == hipSuccess;
    ok = ok && hipMalloc((void **)&M->d_rowptr, (size_t)(dim + 1) * 8) == hipSuccess &&
         hipMalloc((void **)&M->d_nt, (size_t)dim * 8) == hipSuccess &&
         hipMalloc((void **)&M->d_lse, (size_t)dim * 4) == hipSuccess &&
         hipMalloc((void **)&M->d_db1_part, (size_t)M->n_blocks * M->EP * 4) == hipSuccess &&
         hipMalloc((void **)&M->d_loss_part, (size_t)M->n_blocks * 8) == hipSuccess &&
         hipMalloc((void **)&M->d_hdr, SGMH_WORDS * 8) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        return bail(bpe_fail(BPE_ERR_OOM, "bpe native: skip-gram model arrays"));
    }
    if (sgm_lds_attrs<64>() != hipSuccess || sgm_lds_attrs<128>() != hipSuccess || sgm_lds_attrs<256>() != hipSuccess)
        return bail(bpe_fail(BPE_ERR_HIP, "bpe native: skip-gram model LDS attribute"));
    if (sgq_lds_attrs() != hipSuccess || hipDeviceGetAttribute(&M->n_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess)
        return bail(bpe_fail(BPE_ERR_HIP, "bpe native: skip-gram model query attributes"));
    if (sgn_lds_attrs_all() != hipSuccess)
        return bail(bpe_fail(BPE_ERR_HIP, "bpe native: skip-gram model negative-sampling LDS attribute"));
    *out = M;
    return BPE_OK;
}

int bpe_sgmodel_destroy(bpe_sgmodel *M) {
    if (!M) return BPE_OK;
    (void)hipSetDevice(M->device);
    if (M->stream) (void)hipStreamSynchronize(M->stream);
    for (void *p : {(void *)M->d_p, (void *)M->d_g, (void *)M->d_m, (void *)M->d_v, (void *)M->d_rowptr, (void *)M->d_nt,
                    (void *)M->d_lse, (void *)M->d_db1_part, (void *)M->d_loss_part, (void *)M->d_hdr, M->d_planes,
                    M->d_io, M->d_qs, M->d_ns, (void *)M->d_W, M->d_ds, (void *)M->d_bt, (void *)M->d_gbt,
                    (void *)M->d_mbt, (void *)M->d_vbt, M->d_gs, M->d_ss, M->d_ts, M->d_tp})
        if (p) (void)hipFree(p);
    if (M->ev0) (void)hipEventDestroy(M->ev0);
    if (M->ev1) (void)hipEventDestroy(M->ev1);
    for (hipEvent_t e : M->nev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : M->sev) (void)hipEventDestroy(e);
    if (M->stream) (void)hipStreamDestroy(M->stream);
    delete M;
    return BPE_OK;
}

int bpe_sgmodel_set_params(bpe_sgmodel *M, const float *Ein, const float *b1, const float *Eout, const float *b2,
                           int64_t dim, int64_t embed) {
    return sgm_params(M, (float *)Ein, (float *)b1, (float *)Eout, (float *)b2, dim, embed, true, false);
}

int bpe_sgmodel_set_params_device(bpe_sgmodel *M, const float *d_Ein, const float *d_b1, const float *d_Eout,
                                  const float *d_b2, int64_t dim, int64_t embed) {
    return sgm_params(M, (float *)d_Ein, (float *)d_b1, (float *)d_Eout, (float *)d_b2, dim, embed, true, true);
}

int bpe_sgmodel_get_params(bpe_sgmodel *M, float *Ein, float *b1, float *Eout, float *b2, int64_t dim, int64_t embed) {
    return sgm_params(M, Ein, b1, Eout, b2, dim, embed, false, false);
}

int bpe_sgmodel_get_params_device(bpe_sgmodel *M, float *d_Ein, float *d_b1, float *d_Eout, float *d_b2, int64_t dim,
                                  int64_t embed) {
    return sgm_params(M, d_Ein, d_b1, d_Eout, d_b2, dim, embed, false, true);
}

int bpe_sgmodel_loss_grad_device(bpe_sgmodel *M, const int32_t *d_targets, const int32_t *d_contexts,
                                 const int64_t *d_counts, int64_t U, double *loss, float *d_dEin, float *d_db1,
                                 float *d_dEout, float *d_db2) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (int rc = sgm_forward(M, d_targets, d_contexts, d_counts, U, loss)) return rc;
    return sgm_copy_sections(M, M->d_g, d_dEin, d_db1, d_dEout, d_db2, false, hipMemcpyDeviceToDevice);
}

int bpe_sgmodel_loss_grad(bpe_sgmodel *M, const int32_t *targets, const int32_t *contexts, const int64_t *counts,
                          int64_t U, double *loss, float *dEin, float *db1, float *dEout, float *db2) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (U > 0 && (!targets || !contexts || !counts))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model planes");
    const int32_t *d_t, *d_c;
    const int64_t *d_k;
    if (int rc = sgm_stage(M, targets, contexts, counts, U, &d_t, &d_c, &d_k)) return rc;
    if (int rc = sgm_forward(M, d_t, d_c, d_k, U, loss)) return rc;
    return sgm_copy_sections(M, M->d_g, dEin, db1, dEout, db2, false, hipMemcpyDeviceToHost);
}

int bpe_sgmodel_adam_step_device(bpe_sgmodel *M, const int32_t *d_targets, const int32_t *d_contexts,
                                 const int64_t *d_counts, int64_t U, double lr, double beta1, double beta2, double eps,
                                 double *loss) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (!(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1))
        return bpe_fail(BPE_ERR_ARG, "bpe native: skip-gram model betas outside [0, 1)");
    if (int rc = sgm_forward(M, d_targets, d_contexts, d_counts, U, loss)) return rc;
    return sgm_adam(M, lr, beta1, beta2, eps, &M->stats.kernel_ms);
}

int bpe_sgmodel_adam_step(bpe_sgmodel *M, const int32_t *targets, const int32_t *contexts, const int64_t *counts,
                          int64_t U, double lr, double beta1, double beta2, double eps, double *loss) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (U > 0 && (!targets || !contexts || !counts))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model planes");
    const int32_t *d_t, *d_c;
    const int64_t *d_k;
    if (int rc = sgm_stage(M, targets, contexts, counts, U, &d_t, &d_c, &d_k)) return rc;
    return bpe_sgmodel_adam_step_device(M, d_t, d_c, d_k, U, lr, beta1, beta2, eps, loss);
}

int bpe_sgmodel_reset_optimizer(bpe_sgmodel *M) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    SGM_TRY(hipSetDevice(M->device));
    SGM_TRY(hipMemsetAsync(M->d_m, 0, (size_t)M->n4 * 16, M->stream));
    SGM_TRY(hipMemsetAsync(M->d_v, 0, (size_t)M->n4 * 16, M->stream));
    SGM_TRY(hipMemsetAsync(M->d_mbt, 0, (size_t)M->bt4 * 16, M->stream));
    SGM_TRY(hipMemsetAsync(M->d_vbt, 0, (size_t)M->bt4 * 16, M->stream));
    SGM_TRY(hipStreamSynchronize(M->stream));
    M->step = 0;
    return BPE_OK;
}

int bpe_sgmodel_embed_device(bpe_sgmodel *M, const int32_t *d_ids, int64_t n, float *d_out) {
    if (!M || n < 0 || (n && (!d_ids || !d_out))) return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model embed arguments");
    if (!n) return BPE_OK;
    SGM_TRY(hipSetDevice(M->device));
    return sgm_embed(M, d_ids, n, d_out);
}

int bpe_sgmodel_embed(bpe_sgmodel *M, const int32_t *ids, int64_t n, float *out) {
    if (!M || n < 0 || (n && (!ids || !out))) return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model embed arguments");
    if (!n) return BPE_OK;
    SGM_TRY(hipSetDevice(M->device));
    const int64_t out_bytes = n * M->E * 4, id_bytes = (n * 4 + 15) / 16 * 16;
    if (int rc = sgm_grow(&M->d_io, &M->io_cap, out_bytes + id_bytes)) return rc;
    float *d_out = (float *)M->d_io;
    int32_t *d_ids = (int32_t *)((char *)M->d_io + out_bytes);
    SGM_TRY(hipMemcpy(d_ids, ids, (size_t)n * 4, hipMemcpyHostToDevice));
    if (int rc = sgm_embed(M, d_ids, n, d_out)) return rc;
    SGM_TRY(hipMemcpy(out, d_out, (size_t)out_bytes, hipMemcpyDeviceToHost));
    return BPE_OK;
}

int bpe_sgmodel_get_stats(bpe_sgmodel *M, bpe_sgmodel_stats *out) {
    if (!M || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = M->stats;
    out->steps = M->step;
    return BPE_OK;
}

int bpe_sgmodel_reset_stats(bpe_sgmodel *M) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    M->stats = {};
    return BPE_OK;
}

}  // extern "C"

#include "bpe_glove.hip.h"
#include "bpe_svd.hip.h"
#include "bpe_sgtext.hip.h"
