// bpe_svd.hip.h — PPMI and a truncated SVD of it into the skip-gram model's parameters (include/bpe.h,
// "skip-gram model, PPMI and SVD"): the closed-form consumer of the count planes.  Part of bpe_sgmodel.hip's
// translation unit (its struct, SGM_TRY, sgm_grow, sgm_index, sgm_stage, the k_glv_count / k_glv_scan /
// k_glv_compact / k_glv_rowptr compaction, glv_load4 / glv_store4 and the k_sgns_col* / k_sgns_place
// transposition are in scope).  DESIGN.md §3u.
//
//   r_t = sum_c C[t,c] (k_sgm_rowsum's n_t), k_c = sum_t C[t,c], Z = sum_c k_c^cds,
//   a_t = log r_t, b_c = cds log k_c - log Z + log shift, m(t,c) = fl32(max(0, (log C - a_t) - b_c)) on the
//   cells; M is never stored.  Randomized subspace iteration (Halko, Martinsson & Tropp) with L columns:
//   Q = orth(M Omega); power_iters x { W = orth(M^T Q); Q = orth(M W) }; B = M^T Q; T = B^T B = W^ Lambda W^^T;
//   U = Q W^, Vm = B W^ Sigma^-1; Ein = U[:, :E] Sigma^gamma, Eout = Vm[:, :E] Sigma^(1 - gamma), b1 = b2 = 0.
//   orth(Y): G = Y^T Y in double, G = R^T R (Cholesky, no pivoting, small pivots dropped), Y R^-1.
//
//   k_svd_colsum   k_c by integer atomics; k_svd_tables (one workgroup) Z in a fixed order, then a and b;
//   k_svd_ppmi     m of every element of the planes (the ppmi calls only);
//   k_svd_omega    the seeded start matrix: Box-Muller from the 64-bit mix on (seed, row, column);
//   k_svd_spmm<LP, SIDE>  Y = M X on the planes, Y = M^T X on the transposed planes.  The cell range is cut
//                  into runs of SVD_RUN cells whatever the row lengths; a lane group of LP / 4 lanes owns a run
//                  and holds a row of Y in registers, four floats a lane.  A wave first stages its runs: one
//                  cell per lane and pass, the double log at full occupancy, (row id, key id, m) to LDS.
//                  Then the groups walk their runs from LDS, the X rows of four cells gathered with one
//                  16-byte load per lane before the first is used; a cell with m == 0 skips its gather.  A
//                  row that begins and ends inside a run is stored straight; the first and the last row of a
//                  run go to the run's two carry records;
//   k_svd_carry    a wave per carry record: the first record of a row adds the row's records in order;
//   k_svd_gram<LP> partial G = Y^T Y of a block of rows in double on v_mfma_f64_16x16x4_f64: 64 rows at a time
//                  through LDS as fp32 (converted as they are read), the 16 x 16 tiles of the upper triangle
//                  dealt round-robin to the four waves (9 tiles = 36 accumulator doubles a lane at L = 128);
//   k_svd_gram_sum the blocks' partials in block order, the lower triangle mirrored;
//   k_svd_chol     one workgroup, G in LDS: right-looking Cholesky with the drop rule, R^-1 by back
//                  substitution into the lower triangle (transposed), one thread per column;
//   k_svd_apply<LP>  out = Y X for an L x L double X in LDS, on the same matrix instruction; a wave owns 16
//                  rows and all L columns (32 accumulator doubles at L = 128), its A operands read once as
//                  16-byte loads (lane (i, q) takes k = q L / 4 ..), rounded to fp32 once, on the store;
//   k_svd_eig      one workgroup of 1024: cyclic Jacobi in double on T, round-robin order, L / 2 disjoint
//                  rotations at once; T in LDS, the rotation product beside it where both fit (L <= 96), in
//                  memory otherwise; the sorted, scaled right-hand matrices of the finish and sigma;
//   k_svd_sign / k_svd_store  the sign rule and the store into the flat parameter array, b1 = b2 = 0.
// No floating-point atomics; every reduction is an integer reduction or has a fixed order.
#include "bpe_dropout_rule.h"   // drop_mix64, drop_stream

namespace {

constexpr int SVD_RUN = 64;          // cells of a run
constexpr int SVD_STAGE = 64;        // rows of Y in LDS at a time (k_svd_gram)
constexpr int SVD_GRAM_ROWS = 128;   // rows per workgroup of k_svd_gram
constexpr int SVD_SIGN_ROWS = 128;   // rows per workgroup of k_svd_sign and k_svd_store
constexpr int SVD_W_LDS_MAX_L = 96;  // the largest L at which T and the rotation product both fit in LDS
constexpr int SVD_MAX_SWEEPS = 30;
constexpr int SVD_TGT = 0, SVD_CTX = 1;
// header words of a call, in its scratch
constexpr int SVH_POS = 0, SVH_CELLS = 1, SVH_DROPPED = 2, SVH_SWEEPS = 3, SVH_WORDS = 8;
static_assert(BPE_SVD_MAX_L == 128, "the widest instantiation");
static_assert(SVD_RUN % 4 == 0, "cells are walked four at a time");
static_assert((size_t)BPE_SVD_MAX_L * BPE_SVD_MAX_L * 8 + 1024 * 8 <= 160 * 1024, "T and the small arrays in LDS");
static_assert((size_t)2 * SVD_W_LDS_MAX_L * SVD_W_LDS_MAX_L * 8 + 1024 * 8 <= 160 * 1024, "T and the product in LDS");

typedef double d4v __attribute__((ext_vector_type(4)));

// D += A B, A 16 x 4, B 4 x 16: lane l supplies A[l % 16][l / 16] and B[l / 16][l % 16] and holds, in
// element v, D[4 v + l / 16][l % 16]
__device__ __forceinline__ d4v svd_mfma(double a, double b, d4v c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float svd_m(int64_t c, double at, double bc) {
    return (float)fmax(0.0, (log((double)c) - at) - bc);
}

// ---- marginals and log tables ----
__global__ __launch_bounds__(256) void k_svd_colsum(const int32_t *__restrict__ cx, const int64_t *__restrict__ cnt,
                                                    int64_t U, unsigned long long *kc) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < U; i += stride)
        if (cnt[i] > 0) atomicAdd(&kc[cx[i]], (unsigned long long)cnt[i]);
}

// Z: a thread's slice in ascending c, the slices in order
__global__ __launch_bounds__(1024) void k_svd_tables(const int64_t *__restrict__ n_t, const unsigned long long *__restrict__ kc,
                                                     int V, double cds, double log_shift, double *__restrict__ a,
                                                     double *__restrict__ b) {
    __shared__ double sh[1024];
    const int tid = threadIdx.x, per = (V + 1023) / 1024, c0 = tid * per;
    double s = 0.0;
    for (int i = 0; i < per; ++i)
        if (c0 + i < V && kc[c0 + i] > 0) s += pow((double)kc[c0 + i], cds);
    sh[tid] = s;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < 1024; ++i) t += sh[i];
        sh[0] = log(t);
    }
    __syncthreads();
    const double log_z = sh[0];
    for (int c = tid; c < V; c += 1024) {
        a[c] = n_t[c] > 0 ? log((double)n_t[c]) : 0.0;
        b[c] = kc[c] > 0 ? cds * log((double)kc[c]) - log_z + log_shift : 0.0;
    }
}

__global__ __launch_bounds__(256) void k_svd_ppmi(const int32_t *__restrict__ tg, const int32_t *__restrict__ cx,
                                                  const int64_t *__restrict__ cnt, int64_t U, const double *__restrict__ a,
                                                  const double *__restrict__ b, float *__restrict__ out,
                                                  unsigned long long *hdr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t c = i < U ? cnt[i] : 0;
    const float m = c > 0 ? svd_m(c, a[tg[i]], b[cx[i]]) : 0.f;
    if (i < U) out[i] = m;
    const int n_cell = __popcll(__ballot(c > 0)), n_pos = __popcll(__ballot(m > 0.f));
    if ((threadIdx.x & 63) == 0) {
        if (n_cell) atomicAdd(&hdr[SVH_CELLS], (unsigned long long)n_cell);
        if (n_pos) atomicAdd(&hdr[SVH_POS], (unsigned long long)n_pos);
    }
}

// standard normal values, a function of (seed, row, column) alone
__global__ __launch_bounds__(256) void k_svd_omega(float *__restrict__ X, int V, int L, uint64_t seed) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)V * L) return;
    const uint64_t row = (uint64_t)(idx / L), col = (uint64_t)(idx % L);
    const uint64_t z = drop_mix64(drop_stream(seed, row, 0, 1) ^ col);
    const double u1 = ((double)(z >> 32) + 1.0) * (1.0 / 4294967296.0);   // (0, 1]
    const double u2 = (double)(z & 0xFFFFFFFFull) * (1.0 / 4294967296.0);
    X[idx] = (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925 * u2));
}

// ---- the sparse product ----
struct svd_spmm_args {
    const int32_t *rid, *kid;   // SVD_TGT: targets, contexts; SVD_CTX: the transposed planes' contexts, targets
    const int64_t *cnt;
    int64_t N, nruns;
    const double *a, *b;        // the log tables, by target and by context
    const float *X;             // [V][L]
    float *Y;                   // [V][L], zeroed
    int L;
    int32_t *carry_id;          // [2 nruns]: the row of a carry record, -1: none
    float *carry_row;           // [2 nruns][L]
    unsigned long long *pos;    // the cells with m > 0 are counted here (NULL: not counted)
};

template <int LP, int SIDE>
__global__ __launch_bounds__(256) void k_svd_spmm(const svd_spmm_args a) {
    constexpr int G = LP / 4, GW = 64 / G, WR = GW * SVD_RUN;   // lanes of a group, groups and cells of a wave
    __shared__ int4 recs[4 * WR];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t run0 = ((int64_t)blockIdx.x * 4 + w) * GW;
    const int64_t cell0 = run0 * SVD_RUN;
    int4 *wrec = recs + w * WR;
    int n_pos = 0;
    for (int x = lane; x < WR; x += 64) {
        const int64_t i = cell0 + x;
        float m = 0.f;
        if (i < a.N) {
            int4 r;
            r.x = a.rid[i];
            r.y = a.kid[i];
            m = svd_m(a.cnt[i], a.a[SIDE == SVD_TGT ? r.x : r.y], a.b[SIDE == SVD_TGT ? r.y : r.x]);
            r.z = __float_as_int(m);
            r.w = 0;
            wrec[x] = r;
        }
        n_pos += __popcll(__ballot(m > 0.f));
    }
    if (a.pos && lane == 0 && n_pos) atomicAdd(a.pos, (unsigned long long)n_pos);
    __syncthreads();
    const int gi = lane / G, l = lane % G;
    const int64_t run = run0 + gi;
    if (run >= a.nruns) return;
    const int64_t left = a.N - run * SVD_RUN;
    const int n_e = left < SVD_RUN ? (int)left : SVD_RUN;
    const int4 *rec = wrec + gi * SVD_RUN;
    const int L = a.L, e = 4 * l;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int cur = -1, n_rows = 0;

    // the row `cur` is complete as far as this run goes: to its row of Y, or to a carry record
    auto flush = [&](bool last) {
        const bool first = n_rows == 0;
        if (first || last) {
            const int64_t ci = 2 * run + (first ? 0 : 1);
            glv_store4<4>(a.carry_row + (size_t)ci * L, e, L, acc);
            if (l == 0) {
                a.carry_id[ci] = cur;
                if (first && last) a.carry_id[ci + 1] = -1;
            }
        } else {
            glv_store4<4>(a.Y + (size_t)cur * L, e, L, acc);
        }
        ++n_rows;
    };

    for (int j = 0; j < n_e; j += 4) {
        int4 rc[4];
        float4 key[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) rc[k] = rec[min(j + k, n_e - 1)];   // (past the run: the last cell again, unused)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            key[k] = rc[k].z ? glv_load4<4>(a.X + (size_t)rc[k].y * L, e, L) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (j + k < n_e) {
                if (rc[k].x != cur) {
                    if (cur >= 0) flush(false);
                    cur = rc[k].x;
                    acc = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                const float m = __int_as_float(rc[k].z);
                acc.x = fmaf(m, key[k].x, acc.x), acc.y = fmaf(m, key[k].y, acc.y);
                acc.z = fmaf(m, key[k].z, acc.z), acc.w = fmaf(m, key[k].w, acc.w);
            }
        }
    }
    flush(true);
}

// a wave per carry record: the first record of a row sums the row's records in record order
__global__ __launch_bounds__(256) void k_svd_carry(const int32_t *__restrict__ id, const float *__restrict__ rows,
                                                   int64_t n_rec, int L, float *__restrict__ Y) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_rec) return;
    const int row = id[i];
    if (row < 0) return;
    int64_t p = i - 1;
    while (p >= 0 && id[p] < 0) --p;
    if (p >= 0 && id[p] == row) return;
    constexpr int NX = BPE_SVD_MAX_L / 64;
    float acc[NX];
#pragma unroll
    for (int x = 0; x < NX; ++x) acc[x] = lane + 64 * x < L ? rows[(size_t)i * L + lane + 64 * x] : 0.f;
    for (int64_t j = i + 1; j < n_rec; ++j) {
        const int rj = id[j];
        if (rj < 0) continue;
        if (rj != row) break;
#pragma unroll
        for (int x = 0; x < NX; ++x)
            if (lane + 64 * x < L) acc[x] += rows[(size_t)j * L + lane + 64 * x];
    }
#pragma unroll
    for (int x = 0; x < NX; ++x)
        if (lane + 64 * x < L) Y[(size_t)row * L + lane + 64 * x] = acc[x];
}

// ---- the Gram ----
template <int LP>
__global__ __launch_bounds__(256) void k_svd_gram(const float *__restrict__ Y, int V, int L, double *__restrict__ part) {
    constexpr int NT = LP / 16, NTILES = NT * (NT + 1) / 2, MAXS = (NTILES + 3) / 4;
    constexpr int LD = LP + 16;   // the four rows of a step fall into four different groups of 16 banks
    __shared__ float Ys[SVD_STAGE * LD];
    const int tid = threadIdx.x, lane = tid & 63, q = lane >> 4, j = lane & 15;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt = L / 16, l4 = L / 4;
    // tile w + 4 s of the upper triangle, row by row
    int tI[MAXS], tJ[MAXS];
    bool on[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        int I = 0, rem = w + 4 * s;
        while (I < nt && rem >= nt - I) rem -= nt - I, ++I;
        on[s] = I < nt;
        tI[s] = 16 * I, tJ[s] = 16 * (I + rem);
    }
    d4v acc[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) acc[s] = (d4v){0.0, 0.0, 0.0, 0.0};
    const int r_end = min(V, ((int)blockIdx.x + 1) * SVD_GRAM_ROWS);
    for (int r0 = blockIdx.x * SVD_GRAM_ROWS; r0 < r_end; r0 += SVD_STAGE) {
        for (int idx = tid; idx < SVD_STAGE * l4; idx += 256) {
            const int r = idx / l4, c4 = idx % l4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r0 + r < r_end) v = *(const float4 *)(Y + (size_t)(r0 + r) * L + 4 * c4);
            *(float4 *)(Ys + r * LD + 4 * c4) = v;
        }
        __syncthreads();
        for (int kk = 0; kk < SVD_STAGE; kk += 4) {
            const float *row = Ys + (kk + q) * LD + j;
#pragma unroll
            for (int s = 0; s < MAXS; ++s)
                if (on[s]) acc[s] = svd_mfma((double)row[tI[s]], (double)row[tJ[s]], acc[s]);
        }
        __syncthreads();
    }
    double *mine = part + (size_t)blockIdx.x * L * L;
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (on[s])
#pragma unroll
            for (int v = 0; v < 4; ++v) mine[(size_t)(tI[s] + 4 * v + q) * L + tJ[s] + j] = acc[s][v];
}

__global__ __launch_bounds__(256) void k_svd_gram_sum(const double *__restrict__ part, int n_blocks, int L,
                                                      double *__restrict__ G) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= L * L) return;
    int i = idx / L, j = idx % L;
    if (i / 16 > j / 16) {
        const int x = i;
        i = j, j = x;
    }
    double s = 0.0;
    for (int b = 0; b < n_blocks; ++b) s += part[((size_t)b * L + i) * L + j];
    G[idx] = s;
}

// ---- Cholesky and inverse ----
__global__ __launch_bounds__(256) void k_svd_chol(const double *__restrict__ G, int L, double *__restrict__ Rinv,
                                                  unsigned long long *hdr) {
    extern __shared__ double svd_sm[];
    double *A = svd_sm, *invd = A + L * L;   // R in the upper triangle (its diagonal as invd = 1 / R_kk)
    __shared__ double s_thr;
    const int tid = threadIdx.x;
    for (int idx = tid; idx < L * L; idx += 256) A[idx] = G[idx];
    __syncthreads();
    if (tid == 0) {
        double mx = 0.0;
        for (int k = 0; k < L; ++k) mx = fmax(mx, A[k * L + k]);
        s_thr = 1e-12 * mx;
    }
    __syncthreads();
    const double thr = s_thr;
    int n_drop = 0;
    for (int k = 0; k < L; ++k) {
        const double piv = A[k * L + k];   // (never written: the update touches rows below k only)
        if (piv > thr) {                   // (false for a NaN)
            const double rk = sqrt(piv);
            for (int jj = k + 1 + tid; jj < L; jj += 256) A[k * L + jj] /= rk;
            if (tid == 0) invd[k] = 1.0 / rk;
            __syncthreads();
            const int n = L - k - 1;
            for (int idx = tid; idx < n * n; idx += 256) {
                const int i = k + 1 + idx / n, jj = k + 1 + idx % n;
                if (jj >= i) A[i * L + jj] -= A[k * L + i] * A[k * L + jj];
            }
        } else {
            for (int jj = k + 1 + tid; jj < L; jj += 256) A[k * L + jj] = 0.0;
            if (tid == 0) invd[k] = 0.0;
            ++n_drop;
        }
        __syncthreads();
    }
    // X = R^-1, column jj by thread jj: x_ij (i < jj) is kept at A[jj][i]
    if (tid < L) {
        const int jj = tid;
        const double xjj = invd[jj];
        for (int i = jj - 1; i >= 0; --i) {
            double s = A[i * L + jj] * xjj;
            for (int k = i + 1; k < jj; ++k) s += A[i * L + k] * A[jj * L + k];
            A[jj * L + i] = -s * invd[i];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < L * L; idx += 256) {
        const int i = idx / L, jj = idx % L;
        Rinv[idx] = i < jj ? A[jj * L + i] : i == jj ? invd[i] : 0.0;
    }
    if (tid == 0) hdr[SVH_DROPPED] += (unsigned long long)n_drop;
}

// ---- out = Y X ----
template <int LP>
__global__ __launch_bounds__(256) void k_svd_apply(const float *__restrict__ Y, int V, int L, const double *__restrict__ X,
                                                   float *__restrict__ out) {
    constexpr int NT = LP / 16, NS = LP / 4;
    extern __shared__ double svd_sm[];
    double *Xs = svd_sm;   // [L][L]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane >> 4, j = lane & 15;
    const int nt = L / 16, ns = L / 4;
    for (int idx = tid; idx < L * L; idx += 256) Xs[idx] = X[idx];
    __syncthreads();
    for (int tile = blockIdx.x * 4 + w; tile * 16 < V; tile += gridDim.x * 4) {
        // lane (i = j, q) takes k = q ns + st at step st: its A operands are ns consecutive floats of row i
        const int row = tile * 16 + j;
        float av[NS];
#pragma unroll
        for (int m4 = 0; m4 < NS / 4; ++m4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (4 * m4 < ns && row < V) v = *(const float4 *)(Y + (size_t)row * L + q * ns + 4 * m4);
            av[4 * m4] = v.x, av[4 * m4 + 1] = v.y, av[4 * m4 + 2] = v.z, av[4 * m4 + 3] = v.w;
        }
        d4v acc[NT];
#pragma unroll
        for (int J = 0; J < NT; ++J) acc[J] = (d4v){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int st = 0; st < NS; ++st) {
            if (st < ns) {
                const double *xr = Xs + (q * ns + st) * L + j;
                const double av_d = (double)av[st];
#pragma unroll
                for (int J = 0; J < NT; ++J)
                    if (J < nt) acc[J] = svd_mfma(av_d, xr[16 * J], acc[J]);
            }
        }
#pragma unroll
        for (int J = 0; J < NT; ++J)
            if (J < nt)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int r = tile * 16 + 4 * v + q;
                    if (r < V) out[(size_t)r * L + 16 * J + j] = (float)acc[J][v];
                }
    }
}

// ---- the eigenproblem ----
__global__ __launch_bounds__(1024) void k_svd_eig(const double *__restrict__ Tg, int L, int w_in_lds, double *Wg, double gamma,
                                                  double *__restrict__ Wu, double *__restrict__ Wv,
                                                  double *__restrict__ sigma, unsigned long long *hdr) {
    extern __shared__ double svd_sm[];
    double *T = svd_sm;
    double *W = w_in_lds ? T + L * L : Wg;
    double *cs = w_in_lds ? W + L * L : T + L * L;   // [L / 2][2]
    double *lam = cs + L;                            // [L]
    int *perm = (int *)(lam + L);                    // [L]
    int *pp = perm + L, *pq = pp + L / 2;            // [L / 2] each
    __shared__ double red[16];
    __shared__ double s_off, s_tr;
    const int tid = threadIdx.x, half = L / 2, n1 = L - 1;
    for (int idx = tid; idx < L * L; idx += 1024) {
        T[idx] = Tg[idx];
        W[idx] = idx / L == idx % L ? 1.0 : 0.0;
    }
    __syncthreads();
    int sweeps = 0;
    for (int sweep = 0; sweep < SVD_MAX_SWEEPS; ++sweep) {
        double s = 0.0;
        for (int idx = tid; idx < L * L; idx += 1024)
            if (idx / L != idx % L) s += T[idx] * T[idx];
        for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((tid & 63) == 0) red[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0, tr = 0.0;
            for (int i = 0; i < 16; ++i) t += red[i];
            for (int i = 0; i < L; ++i) tr += T[i * L + i];
            s_off = sqrt(t), s_tr = tr;
        }
        __syncthreads();
        if (!(s_off > 1e-14 * s_tr)) break;
        ++sweeps;
        for (int r = 0; r < n1; ++r) {
            if (tid < half) {
                int p = tid == 0 ? n1 : (r + tid) % n1, qq = tid == 0 ? r : (r - tid + n1) % n1;
                if (p > qq) {
                    const int x = p;
                    p = qq, qq = x;
                }
                const double app = T[p * L + p], aqq = T[qq * L + qq], apq = T[p * L + qq];
                double c = 1.0, sn = 0.0;
                if (apq != 0.0) {
                    const double tau = (aqq - app) / (2.0 * apq);
                    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + t * t);
                    sn = t * c;
                }
                pp[tid] = p, pq[tid] = qq;
                cs[2 * tid] = c, cs[2 * tid + 1] = sn;
            }
            __syncthreads();
            for (int idx = tid; idx < half * L; idx += 1024) {   // columns p and q of T and of W
                const int i = idx / half, k = idx % half, p = pp[k], qq = pq[k];
                const double c = cs[2 * k], sn = cs[2 * k + 1];
                double x = T[i * L + p], y = T[i * L + qq];
                T[i * L + p] = c * x - sn * y, T[i * L + qq] = sn * x + c * y;
                x = W[i * L + p], y = W[i * L + qq];
                W[i * L + p] = c * x - sn * y, W[i * L + qq] = sn * x + c * y;
            }
            __syncthreads();
            for (int idx = tid; idx < half * L; idx += 1024) {   // rows p and q of T
                const int k = idx / L, jj = idx % L, p = pp[k], qq = pq[k];
                const double c = cs[2 * k], sn = cs[2 * k + 1];
                const double x = T[p * L + jj], y = T[qq * L + jj];
                T[p * L + jj] = c * x - sn * y, T[qq * L + jj] = sn * x + c * y;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid < L) lam[tid] = T[tid * L + tid];
    __syncthreads();
    if (tid < L) {   // descending, ties to the lower index
        int rank = 0;
        for (int x = 0; x < L; ++x) rank += (lam[x] > lam[tid] || (lam[x] == lam[tid] && x < tid)) ? 1 : 0;
        perm[rank] = tid;
    }
    __syncthreads();
    const double s1 = sqrt(fmax(lam[perm[0]], 0.0));
    for (int idx = tid; idx < L * L; idx += 1024) {
        const int k = idx / L, src = perm[idx % L];
        const double sg = sqrt(fmax(lam[src], 0.0)), wv = W[k * L + src];
        Wu[idx] = wv * pow(sg, gamma);
        Wv[idx] = sg > 1e-7 * s1 ? wv * pow(sg, -gamma) : 0.0;
    }
    if (tid < L) sigma[tid] = sqrt(fmax(lam[perm[tid]], 0.0));
    if (tid == 0) hdr[SVH_SWEEPS] += (unsigned long long)sweeps;
}

// ---- the finish ----
// part[b][c]: the entry of largest magnitude of column c among the block's rows (the lowest row on a tie)
__global__ __launch_bounds__(128) void k_svd_sign(const float *__restrict__ Ut, int V, int L, float *__restrict__ part) {
    const int c = threadIdx.x;
    if (c >= L) return;
    const int r1 = min(V, ((int)blockIdx.x + 1) * SVD_SIGN_ROWS);
    float best = 0.f;
    for (int r = blockIdx.x * SVD_SIGN_ROWS; r < r1; ++r) {
        const float v = Ut[(size_t)r * L + c];
        if (fabsf(v) > fabsf(best)) best = v;
    }
    part[(size_t)blockIdx.x * L + c] = best;
}

__global__ __launch_bounds__(128) void k_svd_store(const float *__restrict__ Ut, const float *__restrict__ Vt,
                                                   const float *__restrict__ part, int n_blocks, int V, int L, int E,
                                                   float *__restrict__ Ein, float *__restrict__ b1, float *__restrict__ Eout,
                                                   float *__restrict__ b2) {
    const int c = threadIdx.x;
    const int r0 = blockIdx.x * SVD_SIGN_ROWS, r1 = min(V, r0 + SVD_SIGN_ROWS);
    for (int r = r0 + c; r < r1; r += 128) b2[r] = 0.f;
    if (c >= E) return;
    if (blockIdx.x == 0) b1[c] = 0.f;
    float best = 0.f;
    for (int b = 0; b < n_blocks; ++b) {
        const float v = part[(size_t)b * L + c];
        if (fabsf(v) > fabsf(best)) best = v;
    }
    const float sg = best < 0.f ? -1.f : 1.f;
    for (int r = r0; r < r1; ++r) {
        Ein[(size_t)r * E + c] = sg * Ut[(size_t)r * L + c];
        Eout[(size_t)r * E + c] = sg * Vt[(size_t)r * L + c];
    }
}

// ---- the host side ----
enum { SVP_PREP = 0, SVP_SPMM, SVP_GRAM, SVP_CHOL, SVP_APPLY, SVP_EIG, SVP_FINISH, SVP_N };

struct svd_timer {
    bpe_sgmodel *M;
    size_t n = 0;
    std::vector<int> phase;   // (as many events as the call has stretches: 8 + 8 power_iters + 7)
    // an event at the end of a stretch of kernels of one kind
    int mark(int ph) {
        if (n == M->sev.size()) {
            hipEvent_t e = nullptr;
            SGM_TRY(hipEventCreate(&e));
            M->sev.push_back(e);
        }
        SGM_TRY(hipEventRecord(M->sev[n], M->stream));
        phase.push_back(ph);
        ++n;
        return BPE_OK;
    }
    int collect(double *ms) {
        for (size_t i = 1; i < n; ++i) {
            float t = 0.f;
            SGM_TRY(hipEventElapsedTime(&t, M->sev[i - 1], M->sev[i]));
            ms[phase[i]] += t;
        }
        return BPE_OK;
    }
};

int svd_add_times(bpe_sgmodel *M, svd_timer &tm) {
    double ms[SVP_N] = {0, 0, 0, 0, 0, 0, 0};
    if (int rc = tm.collect(ms)) return rc;
    bpe_sgmodel_svd_stats &st = M->sstats;
    st.prep_ms += ms[SVP_PREP], st.spmm_ms += ms[SVP_SPMM], st.gram_ms += ms[SVP_GRAM], st.chol_ms += ms[SVP_CHOL];
    st.apply_ms += ms[SVP_APPLY], st.eig_ms += ms[SVP_EIG], st.finish_ms += ms[SVP_FINISH];
    for (double x : ms) st.kernel_ms += x;
    return BPE_OK;
}

int svd_check_ppmi(double shift, double cds) {
    char msg[128];
    if (!(shift > 0 && std::isfinite(shift))) {
        snprintf(msg, sizeof msg, "skip-gram model shift %g is not positive or not finite", shift);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    if (!(cds > 0 && cds <= 1)) {
        snprintf(msg, sizeof msg, "skip-gram model cds %g outside (0, 1]", cds);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    return BPE_OK;
}

// k_c and the two log tables from planes on the device (rowptr and n_t are sgm_index's)
void svd_tables(bpe_sgmodel *M, const int32_t *d_c, const int64_t *d_k, int64_t n, double shift, double cds,
                unsigned long long *kc, double *ta, double *tb) {
    (void)hipMemsetAsync(kc, 0, (size_t)M->V * 8, M->stream);
    if (n) {
        const int64_t nb = (n + 255) / 256;
        k_svd_colsum<<<(unsigned)(nb < 4096 ? nb : 4096), 256, 0, M->stream>>>(d_c, d_k, n, kc);
    }
    k_svd_tables<<<1, 1024, 0, M->stream>>>(M->d_nt, kc, M->V, cds, std::log(shift), ta, tb);
}

int svd_ppmi(bpe_sgmodel *M, const int32_t *d_t, const int32_t *d_c, const int64_t *d_k, int64_t U, double shift,
             double cds, float *d_out) {
    bpe_sgmodel_svd_stats &st = M->sstats;
    st.calls++;
    if (U < 0 || (U && (!d_t || !d_c || !d_k || !d_out)))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model planes");
    if (int rc = svd_check_ppmi(shift, cds)) return rc;
    SGM_TRY(hipSetDevice(M->device));
    int64_t P = 0;
    if (int rc = sgm_index(M, d_t, d_c, d_k, U, &P, &st.kernel_ms)) return rc;
    if (!U) return BPE_OK;
    const size_t vb = ((size_t)M->V * 8 + 15) / 16 * 16;
    if (int rc = sgm_grow(&M->d_ss, &M->ss_cap, (int64_t)(3 * vb + SVH_WORDS * 8))) return rc;
    char *p = (char *)M->d_ss;
    unsigned long long *kc = (unsigned long long *)p, *shdr = (unsigned long long *)(p + 3 * vb);
    double *ta = (double *)(p + vb), *tb = (double *)(p + 2 * vb);
    svd_timer tm{M};
    SGM_TRY(hipMemsetAsync(shdr, 0, SVH_WORDS * 8, M->stream));
    if (int rc = tm.mark(SVP_PREP)) return rc;
    svd_tables(M, d_c, d_k, U, shift, cds, kc, ta, tb);
    k_svd_ppmi<<<(unsigned)((U + 255) / 256), 256, 0, M->stream>>>(d_t, d_c, d_k, U, ta, tb, d_out, shdr);
    SGM_TRY(hipGetLastError());
    if (int rc = tm.mark(SVP_PREP)) return rc;
    unsigned long long h[SVH_WORDS];
    SGM_TRY(hipMemcpyAsync(h, shdr, sizeof h, hipMemcpyDeviceToHost, M->stream));
    SGM_TRY(hipStreamSynchronize(M->stream));
    st.cells += (int64_t)h[SVH_CELLS];
    st.positive_cells += (int64_t)h[SVH_POS];
    return svd_add_times(M, tm);
}

struct svd_bufs {
    float *A, *Y, *Q, *B;   // [V][L] each
    int32_t *carry_id;
    float *carry_row;
    double *gpart, *G, *R, *Wu, *Wv, *Wg, *sigma;
    float *sign_part;
    unsigned long long *shdr;
    const double *ta, *tb;
};

template <int LP>
void svd_spmm_launch(bpe_sgmodel *M, int side, svd_spmm_args a) {
    constexpr int RPB = 4 * (64 / (LP / 4));   // runs of a workgroup
    const unsigned grid = (unsigned)((a.nruns + RPB - 1) / RPB);
    (void)hipMemsetAsync(a.Y, 0, (size_t)M->V * a.L * 4, M->stream);
    if (side == SVD_TGT) k_svd_spmm<LP, SVD_TGT><<<grid, 256, 0, M->stream>>>(a);
    else k_svd_spmm<LP, SVD_CTX><<<grid, 256, 0, M->stream>>>(a);
    k_svd_carry<<<(unsigned)((2 * a.nruns + 3) / 4), 256, 0, M->stream>>>(a.carry_id, a.carry_row, 2 * a.nruns, a.L, a.Y);
}

void svd_spmm(bpe_sgmodel *M, int LP, int side, const svd_spmm_args &a) {
    if (LP == 32) svd_spmm_launch<32>(M, side, a);
    else if (LP == 64) svd_spmm_launch<64>(M, side, a);
    else svd_spmm_launch<128>(M, side, a);
}

void svd_gram(bpe_sgmodel *M, int LP, int L, const float *Y, const svd_bufs &w, double *G) {
    const int nb = (M->V + SVD_GRAM_ROWS - 1) / SVD_GRAM_ROWS;
    if (LP == 32) k_svd_gram<32><<<nb, 256, 0, M->stream>>>(Y, M->V, L, w.gpart);
    else if (LP == 64) k_svd_gram<64><<<nb, 256, 0, M->stream>>>(Y, M->V, L, w.gpart);
    else k_svd_gram<128><<<nb, 256, 0, M->stream>>>(Y, M->V, L, w.gpart);
    k_svd_gram_sum<<<(L * L + 255) / 256, 256, 0, M->stream>>>(w.gpart, nb, L, G);
}

void svd_apply(bpe_sgmodel *M, int LP, int L, const float *Y, const double *X, float *out) {
    const int tiles = (M->V + 63) / 64;
    const unsigned grid = (unsigned)std::min(tiles, std::max(1, M->n_cus));
    const size_t lds = (size_t)L * L * 8;
    if (LP == 32) k_svd_apply<32><<<grid, 256, lds, M->stream>>>(Y, M->V, L, X, out);
    else if (LP == 64) k_svd_apply<64><<<grid, 256, lds, M->stream>>>(Y, M->V, L, X, out);
    else k_svd_apply<128><<<grid, 256, lds, M->stream>>>(Y, M->V, L, X, out);
}


constexpr size_t svd_eig_lds(int L, bool w_in_lds) {
    return (size_t)(w_in_lds ? 2 : 1) * L * L * 8 + (size_t)2 * L * 8 + (size_t)2 * L * 4;
}

hipError_t svd_lds_attrs() {
    constexpr int big = BPE_SVD_MAX_L * BPE_SVD_MAX_L * 8;
    hipError_t e = hipFuncSetAttribute((const void *)k_svd_chol, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       big + BPE_SVD_MAX_L * 8);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_svd_apply<32>, hipFuncAttributeMaxDynamicSharedMemorySize, big);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_svd_apply<64>, hipFuncAttributeMaxDynamicSharedMemorySize, big);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_svd_apply<128>, hipFuncAttributeMaxDynamicSharedMemorySize, big);
    const size_t eig = std::max(svd_eig_lds(BPE_SVD_MAX_L, false), svd_eig_lds(SVD_W_LDS_MAX_L, true));
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_svd_eig, hipFuncAttributeMaxDynamicSharedMemorySize, (int)eig);
    return e;
}
static_assert(svd_eig_lds(BPE_SVD_MAX_L, false) + 256 <= 160 * 1024 && svd_eig_lds(SVD_W_LDS_MAX_L, true) + 256 <= 160 * 1024,
              "LDS of k_svd_eig");

// the defaults, the checks and L; `o` may be NULL
int svd_options(const bpe_sgmodel *M, const bpe_sgmodel_svd_opts *o, bpe_sgmodel_svd_opts *eff, int *L_out) {
    bpe_sgmodel_svd_opts d = {1.0, 1.0, 0.5, 16, 4, 0, nullptr};
    if (o) d = *o;
    char msg[160];
    if (int rc = svd_check_ppmi(d.shift, d.cds)) return rc;
    if (!(d.gamma >= 0 && d.gamma <= 1)) {
        snprintf(msg, sizeof msg, "skip-gram model gamma %g outside [0, 1]", d.gamma);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    if (d.oversample < 0 || d.power_iters < 0) {
        snprintf(msg, sizeof msg, "skip-gram model %s %d is negative", d.oversample < 0 ? "oversample" : "power_iters",
                 d.oversample < 0 ? d.oversample : d.power_iters);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    const int64_t L = ((int64_t)M->E + d.oversample + 15) / 16 * 16;
    if (L > BPE_SVD_MAX_L || L > M->V) {
        snprintf(msg, sizeof msg, "skip-gram model svd width %lld (embed %d + oversample %d, in sixteens) above %s %d",
                 (long long)L, M->E, d.oversample, L > BPE_SVD_MAX_L ? "the limit" : "dim",
                 L > BPE_SVD_MAX_L ? BPE_SVD_MAX_L : M->V);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    *eff = d;
    *L_out = (int)L;
    return BPE_OK;
}

// the optimizer as bpe_sgmodel_reset_optimizer leaves it (on the stream, not waited for)
int svd_reset_optimizer(bpe_sgmodel *M) {
    SGM_TRY(hipMemsetAsync(M->d_m, 0, (size_t)M->n4 * 16, M->stream));
    SGM_TRY(hipMemsetAsync(M->d_v, 0, (size_t)M->n4 * 16, M->stream));
    SGM_TRY(hipMemsetAsync(M->d_mbt, 0, (size_t)M->bt4 * 16, M->stream));
    SGM_TRY(hipMemsetAsync(M->d_vbt, 0, (size_t)M->bt4 * 16, M->stream));
    M->step = 0;
    return BPE_OK;
}

// the whole call from device planes; opts->omega is a host pointer (omega_kind hipMemcpyHostToDevice) or a
// device pointer; sigma[E] on the host
int svd_run(bpe_sgmodel *M, const int32_t *d_t, const int32_t *d_c, const int64_t *d_k, int64_t U,
            const bpe_sgmodel_svd_opts *opts, hipMemcpyKind omega_kind, double *sigma) {
    bpe_sgmodel_svd_stats &st = M->sstats;
    st.calls++;
    if (U < 0 || (U && (!d_t || !d_c || !d_k))) return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model planes");
    bpe_sgmodel_svd_opts o;
    int L = 0;
    if (int rc = svd_options(M, opts, &o, &L)) return rc;
    SGM_TRY(hipSetDevice(M->device));
    int64_t P = 0;
    if (int rc = sgm_index(M, d_t, d_c, d_k, U, &P, &st.kernel_ms)) return rc;
    const int V = M->V, E = M->E, LP = L <= 32 ? 32 : L <= 64 ? 64 : 128;
    if (!M->svd_attrs) {
        SGM_TRY(svd_lds_attrs());
        M->svd_attrs = true;
    }

    // the scratch, sized for N = U
    const int64_t n_chunks_u = (U + GLV_CHUNK - 1) / GLV_CHUNK, max_runs = (U + SVD_RUN - 1) / SVD_RUN;
    const int rpc = (V + SGN_MAX_CHUNKS - 1) / SGN_MAX_CHUNKS, n_chunks = (V + rpc - 1) / rpc;
    const int n_gb = (V + SVD_GRAM_ROWS - 1) / SVD_GRAM_ROWS, n_sb = (V + SVD_SIGN_ROWS - 1) / SVD_SIGN_ROWS;
    auto up = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t VL = up((size_t)V * L * 4), LL = up((size_t)L * L * 8);
    const size_t sizes[] = {up((size_t)n_chunks_u * 8), up((size_t)U * 8), up((size_t)U * 4), up((size_t)U * 4),
                            up((size_t)(V + 1) * 8), up((size_t)U * 8), up((size_t)U * 4), up((size_t)U * 4),
                            up((size_t)(V + 1) * 8), up((size_t)n_chunks * V * 4), up((size_t)V * 4),
                            up((size_t)V * 8), up((size_t)V * 8), up((size_t)V * 8), VL, VL, VL, VL,
                            up((size_t)max_runs * 8), up((size_t)max_runs * 2 * L * 4), (size_t)n_gb * LL, LL, LL, LL, LL, LL,
                            up((size_t)L * 8), up((size_t)n_sb * L * 4), SVH_WORDS * 8};
    size_t total = 0;
    for (size_t b : sizes) total += b;
    if (int rc = sgm_grow(&M->d_ss, &M->ss_cap, (int64_t)total)) return rc;
    char *p = (char *)M->d_ss;
    auto take = [&](int i) { char *r = p; p += sizes[i]; return r; };
    int64_t *part = (int64_t *)take(0), *k2 = (int64_t *)take(1);
    int32_t *t2 = (int32_t *)take(2), *c2 = (int32_t *)take(3);
    int64_t *rowptr2 = (int64_t *)take(4), *kT = (int64_t *)take(5);
    int32_t *tT = (int32_t *)take(6), *cT = (int32_t *)take(7);
    int64_t *colptr = (int64_t *)take(8);
    int32_t *cc = (int32_t *)take(9), *tot = (int32_t *)take(10);
    unsigned long long *kc = (unsigned long long *)take(11);
    double *ta = (double *)take(12), *tb = (double *)take(13);
    svd_bufs w;
    w.A = (float *)take(14), w.Y = (float *)take(15), w.Q = (float *)take(16), w.B = (float *)take(17);
    w.carry_id = (int32_t *)take(18), w.carry_row = (float *)take(19);
    w.gpart = (double *)take(20), w.G = (double *)take(21), w.R = (double *)take(22), w.Wu = (double *)take(23);
    w.Wv = (double *)take(24), w.Wg = (double *)take(25), w.sigma = (double *)take(26);
    w.sign_part = (float *)take(27), w.shdr = (unsigned long long *)take(28);
    w.ta = ta, w.tb = tb;

    svd_timer tm{M};
    unsigned long long h[SGMH_WORDS] = {SGM_NONE, (unsigned long long)P, 0, 0};
    SGM_TRY(hipMemsetAsync(w.shdr, 0, SVH_WORDS * 8, M->stream));
    if (int rc = tm.mark(SVP_PREP)) return rc;
    if (U) {
        k_glv_count<<<(unsigned)n_chunks_u, 256, 0, M->stream>>>(d_k, U, part, M->d_hdr);
        SGM_TRY(hipGetLastError());
        SGM_TRY(hipMemcpyAsync(h, M->d_hdr, sizeof h, hipMemcpyDeviceToHost, M->stream));
    }
    SGM_TRY(hipStreamSynchronize(M->stream));
    const int64_t N = U ? (int64_t)h[GLVH_N] : 0;
    st.cells += N;
    st.L = L;
    float *prm = M->d_p;
    if (N == 0) {   // no cells: zero embeddings and biases, every sigma 0
        SGM_TRY(hipMemsetAsync(prm, 0, (size_t)M->n4 * 16, M->stream));
        if (int rc = svd_reset_optimizer(M)) return rc;
        SGM_TRY(hipStreamSynchronize(M->stream));
        if (sigma) std::fill(sigma, sigma + E, 0.0);
        return BPE_OK;
    }

    const int64_t *rowptr = M->d_rowptr;
    if (N < U) {   // some elements have no count: the cells alone, as planes of their own
        k_glv_scan<<<1, 1024, 0, M->stream>>>(part, n_chunks_u);
        k_glv_compact<<<(unsigned)n_chunks_u, 256, 0, M->stream>>>(d_t, d_c, d_k, U, part, t2, c2, k2);
        k_glv_rowptr<<<(V + 1 + 255) / 256, 256, 0, M->stream>>>(t2, N, V, rowptr2);
        d_t = t2, d_c = c2, d_k = k2, rowptr = rowptr2;
    }
    // the transposed planes (bpe_sgns.hip.h)
    SGM_TRY(hipMemsetAsync(cc, 0, sizes[9], M->stream));
    const int64_t ub = (N + 255) / 256;
    k_sgns_colcount<<<(unsigned)(ub < 4096 ? ub : 4096), 256, 0, M->stream>>>(d_t, d_c, N, V, rpc, cc);
    k_sgns_coloffs<<<(V + 255) / 256, 256, 0, M->stream>>>(cc, V, n_chunks, tot);
    k_sgns_colscan<<<1, 1024, 0, M->stream>>>(tot, V, colptr);
    k_sgns_place<<<n_chunks, 256, 0, M->stream>>>(rowptr, d_c, d_k, V, rpc, cc, colptr, tT, cT, kT);
    svd_tables(M, d_c, d_k, N, o.shift, o.cds, kc, ta, tb);
    if (o.omega) {
        SGM_TRY(hipMemcpyAsync(w.A, o.omega, (size_t)V * L * 4, omega_kind, M->stream));
    } else {
        const int64_t n = (int64_t)V * L;
        k_svd_omega<<<(unsigned)((n + 255) / 256), 256, 0, M->stream>>>(w.A, V, L, o.seed);
    }
    SGM_TRY(hipGetLastError());
    if (int rc = tm.mark(SVP_PREP)) return rc;

    svd_spmm_args a = {};
    a.N = N, a.nruns = (N + SVD_RUN - 1) / SVD_RUN;
    a.a = ta, a.b = tb, a.L = L;
    a.carry_id = w.carry_id, a.carry_row = w.carry_row;
    auto product = [&](int side, const float *X, float *Y, bool count) {   // Y = M X or M^T X
        svd_spmm_args s = a;
        if (side == SVD_TGT) s.rid = d_t, s.kid = d_c, s.cnt = d_k;
        else s.rid = cT, s.kid = tT, s.cnt = kT;
        s.X = X, s.Y = Y, s.pos = count ? w.shdr + SVH_POS : nullptr;
        svd_spmm(M, LP, side, s);
        return tm.mark(SVP_SPMM);
    };
    auto orth = [&](const float *Y, float *out) {   // out = orth(Y)
        svd_gram(M, LP, L, Y, w, w.G);
        if (int rc = tm.mark(SVP_GRAM)) return rc;
        k_svd_chol<<<1, 256, (size_t)(L * L + L) * 8, M->stream>>>(w.G, L, w.R, w.shdr);
        if (int rc = tm.mark(SVP_CHOL)) return rc;
        svd_apply(M, LP, L, Y, w.R, out);
        return tm.mark(SVP_APPLY);
    };
    if (int rc = product(SVD_TGT, w.A, w.Y, true)) return rc;
    if (int rc = orth(w.Y, w.Q)) return rc;
    for (int it = 0; it < o.power_iters; ++it) {
        if (int rc = product(SVD_CTX, w.Q, w.Y, false)) return rc;
        if (int rc = orth(w.Y, w.A)) return rc;
        if (int rc = product(SVD_TGT, w.A, w.Y, false)) return rc;
        if (int rc = orth(w.Y, w.Q)) return rc;
    }
    if (int rc = product(SVD_CTX, w.Q, w.B, false)) return rc;
    SGM_TRY(hipGetLastError());

    const bool w_in_lds = L <= SVD_W_LDS_MAX_L;
    svd_gram(M, LP, L, w.B, w, w.G);
    if (int rc = tm.mark(SVP_GRAM)) return rc;
    k_svd_eig<<<1, 1024, svd_eig_lds(L, w_in_lds), M->stream>>>(w.G, L, w_in_lds ? 1 : 0, w.Wg, o.gamma, w.Wu, w.Wv,
                                                               w.sigma, w.shdr);
    SGM_TRY(hipGetLastError());
    if (int rc = tm.mark(SVP_EIG)) return rc;

    svd_apply(M, LP, L, w.Q, w.Wu, w.A);   // U Sigma^gamma
    svd_apply(M, LP, L, w.B, w.Wv, w.Y);   // Vm Sigma^(1 - gamma)
    if (int rc = tm.mark(SVP_APPLY)) return rc;
    k_svd_sign<<<n_sb, 128, 0, M->stream>>>(w.A, V, L, w.sign_part);
    k_svd_store<<<n_sb, 128, 0, M->stream>>>(w.A, w.Y, w.sign_part, n_sb, V, L, E, prm + M->o_ein, prm + M->o_b1,
                                            prm + M->o_eout, prm + M->o_b2);
    SGM_TRY(hipGetLastError());
    if (int rc = svd_reset_optimizer(M)) return rc;
    if (int rc = tm.mark(SVP_FINISH)) return rc;

    unsigned long long sh[SVH_WORDS];
    double sg[BPE_SVD_MAX_L];
    SGM_TRY(hipMemcpyAsync(sh, w.shdr, sizeof sh, hipMemcpyDeviceToHost, M->stream));
    SGM_TRY(hipMemcpyAsync(sg, w.sigma, (size_t)L * 8, hipMemcpyDeviceToHost, M->stream));
    SGM_TRY(hipStreamSynchronize(M->stream));
    if (sigma) std::copy(sg, sg + E, sigma);
    st.positive_cells += (int64_t)sh[SVH_POS];
    st.dropped_columns += (int64_t)sh[SVH_DROPPED];
    st.sweeps += (int64_t)sh[SVH_SWEEPS];
    return svd_add_times(M, tm);
}

}  // namespace

extern "C" {

int bpe_sgmodel_ppmi_device(bpe_sgmodel *M, const int32_t *d_targets, const int32_t *d_contexts, const int64_t *d_counts,
                            int64_t U, double shift, double cds, float *d_out) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    return svd_ppmi(M, d_targets, d_contexts, d_counts, U, shift, cds, d_out);
}

int bpe_sgmodel_ppmi(bpe_sgmodel *M, const int32_t *targets, const int32_t *contexts, const int64_t *counts, int64_t U,
                     double shift, double cds, float *out) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (U > 0 && (!targets || !contexts || !counts || !out))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model planes");
    const int32_t *d_t, *d_c;
    const int64_t *d_k;
    if (int rc = sgm_stage(M, targets, contexts, counts, U, &d_t, &d_c, &d_k)) return rc;
    if (U > 0)
        if (int rc = sgm_grow(&M->d_io, &M->io_cap, U * 4)) return rc;
    if (int rc = svd_ppmi(M, d_t, d_c, d_k, U, shift, cds, (float *)M->d_io)) return rc;
    if (U > 0) SGM_TRY(hipMemcpy(out, M->d_io, (size_t)U * 4, hipMemcpyDeviceToHost));
    return BPE_OK;
}

int bpe_sgmodel_ppmi_svd_device(bpe_sgmodel *M, const int32_t *d_targets, const int32_t *d_contexts,
                                const int64_t *d_counts, int64_t U, const bpe_sgmodel_svd_opts *opts, double *sigma) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    return svd_run(M, d_targets, d_contexts, d_counts, U, opts, hipMemcpyDeviceToDevice, sigma);
}

int bpe_sgmodel_ppmi_svd(bpe_sgmodel *M, const int32_t *targets, const int32_t *contexts, const int64_t *counts,
                         int64_t U, const bpe_sgmodel_svd_opts *opts, double *sigma) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (U > 0 && (!targets || !contexts || !counts))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model planes");
    const int32_t *d_t, *d_c;
    const int64_t *d_k;
    if (int rc = sgm_stage(M, targets, contexts, counts, U, &d_t, &d_c, &d_k)) return rc;
    return svd_run(M, d_t, d_c, d_k, U, opts, hipMemcpyHostToDevice, sigma);
}

int bpe_sgmodel_get_svd_stats(bpe_sgmodel *M, bpe_sgmodel_svd_stats *out) {
    if (!M || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = M->sstats;
    return BPE_OK;
}

int bpe_sgmodel_reset_svd_stats(bpe_sgmodel *M) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    M->sstats = {};
    return BPE_OK;
}

}  // extern "C"
