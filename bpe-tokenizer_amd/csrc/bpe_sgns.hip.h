// bpe_sgns.hip.h — skip-gram with negative sampling on the skip-gram model's parameters (include/bpe.h,
// "skip-gram model, negative sampling"): loss, gradients and Adam from the count planes and one negative
// set shared by all targets of a step.  Part of bpe_sgmodel.hip's translation unit (its struct, SGM_TRY,
// sgm_mfma, sgm_acc_row, sgm_grow, sgm_index, sgm_adam and k_sgm_reduce are in scope).  DESIGN.md §3q.
//
//   H_t = Ein[t] + b1, z(t,c) = H_t . Eout[c] + b2[c], n_t = sum_c C[t,c], P = sum_t n_t, ls = log sigma,
//   L = -(1/P) [ sum C[t,c] ls(z(t,c)) + k sum_t n_t sum_s w_s ls(-z(t,a_s)) ],
//   G[t,c] = (1/P) [ C[t,c] (sigma(z) - 1) + k n_t W_c sigma(z) ],  W_c = w_s where c = a_s, else 0,
//   dEin = G Eout, db1 its column sums, dEout = G^T H, db2 the column sums of G.
// G is nonzero on the U count cells and on the V x S block of the set only, and that is all that is
// touched: a step costs about 32 U E (the masked product below) + 4 V S E flops, not 4 V^2 E.
//
// One tile loop, k_sgns<EP, MODE>, serves three ways.  A workgroup is one wave that owns 32 resident rows,
// staged in LDS and zero-padded to EP.  32-row key tiles stream through two LDS buffers behind a register
// prefetch (at EP = 256, where O^T alone takes 128 registers, staged behind the products), gathered with
// 16-byte loads where E % 4 == 0.  Beside each key sit its bias, its weight and its row-in-tile.
// S^T = K . R^T by v_mfma_f32_32x32x2_f32 leaves a resident row's 32 logits in the accumulators of its
// two lanes; the weight g is formed there in-lane (e = exp(-|z|), sigma and log sigma in the forms that
// do not cancel); O^T += K^T . G^T takes G from those registers as its B operand.  No softmax statistic,
// no rescale.
//   SGN_TGT   resident: 32 rows of H.  Keys: first the block's CSR entries, 32 consecutive ones per tile
//             (Eout[c_i], b2[c_i], C_i / P, row t_i - I0): a lane's weight is -(C_i/P) sigma(-z) where the
//             entry's row is its own and 0 elsewhere.  Then the set, 32 entries per tile (Eout[a_s],
//             b2[a_s], k w_s; every row): weight (n_t/P) k w_s sigma(z).  Out: dEin rows, the block's
//             column sums for db1, its loss partial (double).
//   SGN_CTXP  the same loop with roles swapped over the transposed planes: resident 32 rows of Eout with
//             b2 as the lane's bias, keys the gathered H_{t_i}.  Out: dEout rows and db2 (in-lane: a lane
//             owns a column); rows that nothing touches are written as zeros.
//   SGN_CTXN  resident: 32 set entries gathered by id.  Keys: contiguous 32-row blocks of H with n_t / P;
//             blocks without counts are skipped on a uniform branch.  grid.y splits the row range; the
//             partials go to scratch and k_sgns_add sums them in split order onto dEout[a_s], db2[a_s].
// The transposed planes (c, t, C) by (c, t) are built per call with integers only: k_sgns_colcount counts
// every (row chunk, column) cell by integer atomics, k_sgns_coloffs turns a column's chunk counts into
// offsets and its total, k_sgns_colscan scans the totals into colptr, and k_sgns_place walks each chunk's
// rows in order, a row's entries in parallel (its columns are distinct, so no two lanes share a counter).
// The same bytes on every run.  No floating-point atomics; every sum has a fixed order.

namespace {

constexpr int SGN_ROWS = BPE_SGNS_ROWS;   // resident rows of a wave, rows of a key tile
constexpr int SGN_TGT = 0, SGN_CTXP = 1, SGN_CTXN = 2;
constexpr int SGN_MAX_CHUNKS = 256;       // row chunks of the transposition
constexpr int SGN_MAX_SPLITS = 64;        // row-range splits of SGN_CTXN
constexpr int SGN_ALL = -1, SGN_NO_ROW = -2;   // a key's row-in-tile: every resident row / none
static_assert(SGN_ROWS == 32, "the matrix instruction's tile");

struct sgn_args {
    const float *Ein, *b1, *Eout, *b2;
    int V, E;
    const int64_t *rowptr, *n_t;
    const unsigned long long *hdr;
    const int64_t *ptr;        // SGN_TGT: rowptr; SGN_CTXP: colptr
    const int32_t *key_ids;    // SGN_TGT: contexts; SGN_CTXP: the transposed planes' targets
    const int32_t *row_ids;    // SGN_TGT: targets;  SGN_CTXP: the transposed planes' contexts
    const int64_t *cnt;        // ... and their counts
    const int32_t *neg_ids;
    const float *neg_w;        // NULL: 1 / S each
    int S;
    double neg_k;
    int bps;                   // SGN_CTXN: key blocks per split
    float *out;                // dEin / dEout / partial rows [splits][SP][E]
    float *out_b;              // db1 partials [blocks][EP] / db2 / partial db2 [splits][SP]
    double *loss_part;         // SGN_TGT
};

__global__ __launch_bounds__(256) void k_sgns_set_check(const int32_t *__restrict__ ids, const float *__restrict__ w, int S,
                                                        int V, unsigned long long *hdr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    bool bad = (uint32_t)ids[i] >= (uint32_t)V || (i > 0 && ids[i] <= ids[i - 1]);
    if (!bad && w) bad = !(w[i] >= 0.f && w[i] <= 3.402823466e38f);   // (false for a NaN)
    if (bad) atomicMin(&hdr[SGMH_ERR], (unsigned long long)i);
}

// ---- the transposed planes ----
__global__ __launch_bounds__(256) void k_sgns_colcount(const int32_t *__restrict__ tg, const int32_t *__restrict__ cx, int64_t U,
                                                       int V, int rpc, int32_t *cc) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < U; i += stride)
        atomicAdd(&cc[(size_t)(tg[i] / rpc) * V + cx[i]], 1);
}

__global__ __launch_bounds__(256) void k_sgns_coloffs(int32_t *__restrict__ cc, int V, int n_chunks, int32_t *__restrict__ tot) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= V) return;
    int32_t run = 0;
    for (int k = 0; k < n_chunks; ++k) {
        const int32_t x = cc[(size_t)k * V + c];
        cc[(size_t)k * V + c] = run;
        run += x;
    }
    tot[c] = run;
}

__global__ __launch_bounds__(1024) void k_sgns_colscan(const int32_t *__restrict__ tot, int V, int64_t *__restrict__ colptr) {
    __shared__ int64_t sh[1024];
    const int tid = threadIdx.x, per = (V + 1023) / 1024, c0 = tid * per;
    int64_t s = 0;
    for (int i = 0; i < per; ++i)
        if (c0 + i < V) s += tot[c0 + i];
    sh[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t x = tid >= o ? sh[tid - o] : 0;
        __syncthreads();
        sh[tid] += x;
        __syncthreads();
    }
    int64_t run = sh[tid] - s;
    for (int i = 0; i < per; ++i)
        if (c0 + i < V) {
            colptr[c0 + i] = run;
            run += tot[c0 + i];
        }
    if (tid == 1023) colptr[V] = sh[1023];
}

// one workgroup per row chunk, its rows in order: the placement is stable, so a column's entries ascend in t
__global__ __launch_bounds__(256) void k_sgns_place(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ cx,
                                                    const int64_t *__restrict__ cnt, int V, int rpc, int32_t *cc,
                                                    const int64_t *__restrict__ colptr, int32_t *__restrict__ tT,
                                                    int32_t *__restrict__ cT, int64_t *__restrict__ kT) {
    int32_t *mine = cc + (size_t)blockIdx.x * V;
    const int t1 = min(V, (int)(blockIdx.x + 1) * rpc);
    for (int t = blockIdx.x * rpc; t < t1; ++t) {
        const int64_t beg = rowptr[t], end = rowptr[t + 1];
        if (beg == end) continue;
        for (int64_t i = beg + threadIdx.x; i < end; i += blockDim.x) {
            const int32_t c = cx[i];
            const int32_t o = mine[c];
            mine[c] = o + 1;
            const int64_t pos = colptr[c] + o;
            tT[pos] = t;
            cT[pos] = c;
            kT[pos] = cnt[i];
        }
        __syncthreads();   // (uniform: the next row may meet this row's columns)
    }
}

// ---- the tile loop ----
template <int EP>
constexpr size_t sgn_lds() {
    return (size_t)64 * 8 + (size_t)(3 * SGN_ROWS * (EP + 1) + 6 * SGN_ROWS) * 4;
}
static_assert(sgn_lds<256>() <= 160 * 1024, "LDS of the widest instantiation");

template <int EP, int MODE>
__global__ __launch_bounds__(64) void k_sgns(const sgn_args a) {
    constexpr int LD = EP + 1;                // odd: a column of 32 rows touches 32 banks
    constexpr int NEB = EP / 32;
    constexpr int N4 = SGN_ROWS * EP / 4 / 64;   // staged float4s per lane and tile
    constexpr bool PRE = EP <= 128;
    extern __shared__ double smem_d[];
    double *red = smem_d;                     // [64]
    float *Rs = (float *)(red + 64);          // [32][LD]: the resident rows
    float *Ks = Rs + SGN_ROWS * LD;           // [2][32][LD]: key tiles; after the stream: O, [32][LD]
    float *kbs = Ks + 2 * SGN_ROWS * LD;      // [2][32]: a key's bias
    float *kws = kbs + 2 * SGN_ROWS;          // [2][32]: ... weight
    int *krs = (int *)(kws + 2 * SGN_ROWS);   // [2][32]: ... row-in-tile, SGN_ALL or SGN_NO_ROW

    const int lane = threadIdx.x, q = lane & 31, half = lane >> 5;
    const int V = a.V, E = a.E, S = a.S;
    const int Ek = (E + 1) & ~1;
    const bool vec4 = (E & 3) == 0;           // rows start on 16 bytes
    const int R0 = blockIdx.x * SGN_ROWS;     // the first resident row: a target, a context or a set index
    const double inv_P = 1.0 / (double)(long long)a.hdr[SGMH_P];
    const float *rbase = MODE == SGN_TGT ? a.Ein : a.Eout;
    const float *kbase = MODE == SGN_TGT ? a.Eout : a.Ein;
    auto neg_weight = [&](int s) { return (float)(a.neg_k * (a.neg_w ? (double)a.neg_w[s] : 1.0 / S)); };

    // four values of row `id` from column e (zeros past E or for no row); add: + b1
    auto row4 = [&](const float *base, bool add, int id, int e) {
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (id < 0 || e >= E) return x;
        const float *p = base + (size_t)id * E + e;
        if (vec4) {
            x = *(const float4 *)p;
            if (add) {
                const float4 b = *(const float4 *)(a.b1 + e);
                x.x += b.x, x.y += b.y, x.z += b.z, x.w += b.w;
            }
        } else {
            x.x = p[0] + (add ? a.b1[e] : 0.f);
            if (e + 1 < E) x.y = p[1] + (add ? a.b1[e + 1] : 0.f);
            if (e + 2 < E) x.z = p[2] + (add ? a.b1[e + 2] : 0.f);
            if (e + 3 < E) x.w = p[3] + (add ? a.b1[e + 3] : 0.f);
        }
        return x;
    };
    auto put4 = [&](float *dst, float4 x) { dst[0] = x.x, dst[1] = x.y, dst[2] = x.z, dst[3] = x.w; };

    // the resident rows, the lane's bias rb and its row weight wn
    const int n_res = MODE == SGN_CTXN ? S : V;
    auto res_id = [&](int r) { return R0 + r >= n_res ? -1 : MODE == SGN_CTXN ? a.neg_ids[R0 + r] : R0 + r; };
    for (int i = lane; i < SGN_ROWS * EP / 4; i += 64) {
        const int r = i / (EP / 4), e = (i % (EP / 4)) * 4;
        put4(Rs + r * LD + e, row4(rbase, MODE == SGN_TGT, res_id(r), e));
    }
    const int my = res_id(q);
    float rb = 0.f, wn = 0.f;
    if (my >= 0) {
        if (MODE == SGN_TGT) wn = (float)((double)a.n_t[my] * inv_P);
        else rb = a.b2[my];
        if (MODE == SGN_CTXN) wn = neg_weight(R0 + q);
    }

    // the key tiles j0 <= j < j1
    int64_t beg = 0, end = 0;
    int npos = 0, j0 = 0, j1 = 0;
    if (MODE == SGN_CTXN) {
        j0 = blockIdx.y * a.bps;
        j1 = min((V + SGN_ROWS - 1) / SGN_ROWS, j0 + a.bps);
    } else {
        beg = a.ptr[R0];
        end = a.ptr[min(V, R0 + SGN_ROWS)];
        npos = (int)((end - beg + SGN_ROWS - 1) / SGN_ROWS);
        j1 = npos + (MODE == SGN_TGT ? (S + SGN_ROWS - 1) / SGN_ROWS : 0);
    }
    // key r of tile j: its row id (-1: none), and for lanes < 32 its bias, weight and row-in-tile
    auto key_id = [&](int j, int r) -> int {
        if (MODE == SGN_CTXN) return j * SGN_ROWS + r < V ? j * SGN_ROWS + r : -1;
        if (j < npos) {
            const int64_t i = beg + (int64_t)j * SGN_ROWS + r;
            return i < end ? a.key_ids[i] : -1;
        }
        const int s = (j - npos) * SGN_ROWS + r;
        return s < S ? a.neg_ids[s] : -1;
    };
    auto key_meta = [&](int j, int r, float &kb, float &kw, int &kr) {
        const int id = key_id(j, r);
        kb = 0.f, kw = 0.f, kr = SGN_NO_ROW;
        if (id < 0) return;
        if (MODE == SGN_CTXN) {
            kw = (float)((double)a.n_t[id] * inv_P);
            kr = kw > 0.f ? SGN_ALL : SGN_NO_ROW;
        } else if (j < npos) {
            const int64_t i = beg + (int64_t)j * SGN_ROWS + r;
            kw = (float)((double)a.cnt[i] * inv_P);
            kr = a.row_ids[i] - R0;
            if (MODE == SGN_TGT) kb = a.b2[id];
        } else {
            kw = neg_weight((j - npos) * SGN_ROWS + r);
            kr = SGN_ALL;
            kb = a.b2[id];
        }
    };
    auto next_tile = [&](int j) {   // SGN_CTXN: the first block from j on that has count entries (uniform)
        if (MODE == SGN_CTXN)
            while (j < j1 && a.rowptr[min(V, (j + 1) * SGN_ROWS)] == a.rowptr[j * SGN_ROWS]) ++j;
        return j;
    };

    float4 pre[PRE ? N4 : 1];
    float pre_kb = 0.f, pre_kw = 0.f;
    int pre_kr = SGN_NO_ROW;
    auto load_tile = [&](int j) {
#pragma unroll
        for (int i = 0; i < (PRE ? N4 : 0); ++i) {
            const int x = lane + i * 64;
            pre[i] = row4(kbase, MODE != SGN_TGT, key_id(j, x / (EP / 4)), (x % (EP / 4)) * 4);
        }
        if (lane < SGN_ROWS) key_meta(j, lane, pre_kb, pre_kw, pre_kr);
    };
    auto store_meta = [&](int buf) {
        if (lane < SGN_ROWS) {
            kbs[buf * SGN_ROWS + lane] = pre_kb;
            kws[buf * SGN_ROWS + lane] = pre_kw;
            krs[buf * SGN_ROWS + lane] = pre_kr;
        }
    };
    auto store_tile = [&](int buf) {
        float *Kb = Ks + buf * SGN_ROWS * LD;
#pragma unroll
        for (int i = 0; i < (PRE ? N4 : 0); ++i) {
            const int x = lane + i * 64;
            put4(Kb + (x / (EP / 4)) * LD + (x % (EP / 4)) * 4, pre[i]);
        }
        store_meta(buf);
    };
    auto stage_tile = [&](int j, int buf) {
        float *Kb = Ks + buf * SGN_ROWS * LD;
#pragma unroll 4
        for (int i = 0; i < N4; ++i) {
            const int x = lane + i * 64;
            put4(Kb + (x / (EP / 4)) * LD + (x % (EP / 4)) * 4,
                 row4(kbase, MODE != SGN_TGT, key_id(j, x / (EP / 4)), (x % (EP / 4)) * 4));
        }
        if (lane < SGN_ROWS) key_meta(j, lane, pre_kb, pre_kw, pre_kr);
        store_meta(buf);
    };

    f16v O[NEB];
#pragma unroll
    for (int eb = 0; eb < NEB; ++eb)
#pragma unroll
        for (int v = 0; v < 16; ++v) O[eb][v] = 0.f;
    double loss = 0.0;
    float gsum = 0.f;
    const float *Rw = Rs + q * LD + half;

    int j = next_tile(j0), it = 0;
    if (j < j1) {
        if (PRE) load_tile(j);
        else stage_tile(j, 0);
    }
    while (j < j1) {
        const int buf = it & 1;
        if (PRE) store_tile(buf);
        __syncthreads();
        const int nx = next_tile(j + 1);
        if (PRE && nx < j1) load_tile(nx);
        const float *Kb = Ks + buf * SGN_ROWS * LD;
        // S^T[key][row] = sum_k K[key][k] R[row][k]
        f16v s;
#pragma unroll
        for (int v = 0; v < 16; ++v) s[v] = 0.f;
        const float *Ka = Kb + q * LD + half;
        for (int k = 0; k < Ek; k += 2) s = sgm_mfma(Ka[k], Rw[k], s);
        float lt = 0.f;   // this tile's share of the lane's loss (at most 16 terms), then on in double
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int slot = buf * SGN_ROWS + sgm_acc_row(v, half);
            const int kr = krs[slot];
            const float kw = kws[slot];
            const float z = s[v] + kbs[slot] + rb;
            const float e = expf(-fabsf(z));
            const float hi = 1.f / (1.f + e), lo = e * hi;   // sigma(|z|), sigma(-|z|)
            float g = 0.f;
            if (kr == q) {                                   // a count cell of this row: (C/P) (sigma(z) - 1)
                g = -kw * (z >= 0.f ? lo : hi);
                if (MODE == SGN_TGT) lt -= kw * (fminf(z, 0.f) - log1pf(e));
            } else if (kr == SGN_ALL) {                      // a negative: k w_s (n_t/P) sigma(z)
                const float ww = wn * kw;
                g = ww * (z >= 0.f ? hi : lo);
                if (MODE == SGN_TGT) lt -= ww * (fminf(-z, 0.f) - log1pf(e));
            }
            s[v] = g;
            gsum += g;
        }
        loss += (double)lt;
        // O^T[e][row] += sum_key K[key][e] G[row][key]; k step v takes the key of register v
#pragma unroll
        for (int eb = 0; eb < NEB; ++eb) {
            if (eb * 32 < E) {
#pragma unroll
                for (int v = 0; v < 16; ++v)
                    O[eb] = sgm_mfma(Kb[sgm_acc_row(v, half) * LD + eb * 32 + q], s[v], O[eb]);
            }
        }
        // (the other buffer was last read before this iteration's barrier)
        if (!PRE && nx < j1) stage_tile(nx, buf ^ 1);
        j = nx;
        ++it;
    }
    __syncthreads();   // the last tile has been read: Ks becomes Os

    float *Os = Ks;
#pragma unroll
    for (int eb = 0; eb < NEB; ++eb)
#pragma unroll
        for (int v = 0; v < 16; ++v) Os[q * LD + eb * 32 + sgm_acc_row(v, half)] = O[eb][v];
    if (MODE == SGN_TGT) red[lane] = loss;
    __syncthreads();

    const int nrows = min(SGN_ROWS, n_res - R0);
    const int SP = (S + SGN_ROWS - 1) / SGN_ROWS * SGN_ROWS;
    float *out = a.out + (MODE == SGN_CTXN ? ((size_t)blockIdx.y * SP + R0) * E : (size_t)R0 * E);
    for (int i = lane; i < nrows * E; i += 64) out[i] = Os[(i / E) * LD + i % E];
    if (MODE == SGN_TGT) {
        for (int e = lane; e < EP; e += 64) {
            float c = 0.f;
            for (int r = 0; r < SGN_ROWS; ++r) c += Os[r * LD + e];   // (rows past V are zero)
            a.out_b[(size_t)blockIdx.x * EP + e] = c;
        }
        if (lane == 0) {
            double c = 0.0;
            for (int i = 0; i < 64; ++i) c += red[i];
            a.loss_part[blockIdx.x] = c;
        }
    } else {
        gsum += __shfl_xor(gsum, 32, 64);
        if (half == 0 && q < nrows) a.out_b[MODE == SGN_CTXN ? (size_t)blockIdx.y * SP + R0 + q : (size_t)R0 + q] = gsum;
    }
}

// the set's partial rows and db2 partials summed in split order onto dEout[a_s] and db2[a_s] (ids are unique)
__global__ __launch_bounds__(256) void k_sgns_add(const float *__restrict__ part, const float *__restrict__ part_b,
                                                  const int32_t *__restrict__ neg_ids, int S, int E, int splits,
                                                  float *__restrict__ dEout, float *__restrict__ db2) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t SP = (size_t)(S + SGN_ROWS - 1) / SGN_ROWS * SGN_ROWS;
    if (idx < (int64_t)S * E) {
        float c = 0.f;
        for (int sp = 0; sp < splits; ++sp) c += part[sp * SP * E + idx];
        dEout[(size_t)neg_ids[idx / E] * E + idx % E] += c;
    }
    if (idx < S) {
        float c = 0.f;
        for (int sp = 0; sp < splits; ++sp) c += part_b[sp * SP + idx];
        db2[neg_ids[idx]] += c;
    }
}

template <int EP>
hipError_t sgn_lds_attrs() {
    for (const void *f : {(const void *)k_sgns<EP, SGN_TGT>, (const void *)k_sgns<EP, SGN_CTXP>, (const void *)k_sgns<EP, SGN_CTXN>}) {
        hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sgn_lds<EP>());
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t sgn_lds_attrs_all() {
    hipError_t e = sgn_lds_attrs<64>();
    if (e == hipSuccess) e = sgn_lds_attrs<128>();
    if (e == hipSuccess) e = sgn_lds_attrs<256>();
    return e;
}

// the call's scratch, carved from one grow-only buffer
struct sgn_scratch {
    int64_t *kT, *colptr;
    int32_t *tT, *cT, *cc, *tot;
    float *db1_part, *part, *part_b;
    double *loss_part;
};

template <int EP>
void sgn_launch(bpe_sgmodel *M, const sgn_args &base, const sgn_scratch &w, int splits, hipEvent_t mid) {
    const int nb = (M->V + SGN_ROWS - 1) / SGN_ROWS;
    float *g = M->d_g;
    sgn_args a = base;
    a.out = g + M->o_ein;
    a.out_b = w.db1_part;
    a.loss_part = w.loss_part;
    k_sgns<EP, SGN_TGT><<<nb, 64, sgn_lds<EP>(), M->stream>>>(a);
    k_sgm_reduce<<<1, 256, 0, M->stream>>>(w.db1_part, w.loss_part, nb, EP, M->E, g + M->o_b1, M->d_hdr);
    (void)hipEventRecord(mid, M->stream);
    a.ptr = w.colptr;
    a.key_ids = w.tT;
    a.row_ids = w.cT;
    a.cnt = w.kT;
    a.out = g + M->o_eout;
    a.out_b = g + M->o_b2;
    k_sgns<EP, SGN_CTXP><<<nb, 64, sgn_lds<EP>(), M->stream>>>(a);
    if (a.S) {
        a.out = w.part;
        a.out_b = w.part_b;
        k_sgns<EP, SGN_CTXN><<<dim3((a.S + SGN_ROWS - 1) / SGN_ROWS, splits), 64, sgn_lds<EP>(), M->stream>>>(a);
        const int64_t n = (int64_t)a.S * M->E;
        k_sgns_add<<<(unsigned)((n + 255) / 256), 256, 0, M->stream>>>(w.part, w.part_b, a.neg_ids, a.S, M->E, splits,
                                                                     g + M->o_eout, g + M->o_b2);
    }
}

int sgn_bad_set(bpe_sgmodel *M, const int32_t *d_ids, const float *d_w, int64_t i) {
    int32_t id[2] = {0, 0};
    float w = 0.f;
    const int64_t from = i > 0 ? i - 1 : i;
    SGM_TRY(hipMemcpy(id + (i > 0 ? 0 : 1), d_ids + from, (size_t)(i - from + 1) * 4, hipMemcpyDeviceToHost));
    if (d_w) SGM_TRY(hipMemcpy(&w, d_w + i, 4, hipMemcpyDeviceToHost));
    char msg[160];
    if (id[1] < 0 || id[1] >= M->V)
        snprintf(msg, sizeof msg, "skip-gram model negative id %d outside [0, %d) (element %lld)", id[1], M->V, (long long)i);
    else if (i > 0 && id[1] <= id[0])
        snprintf(msg, sizeof msg, "skip-gram model negative ids must ascend: %d after %d (element %lld)", id[1], id[0],
                 (long long)i);
    else
        snprintf(msg, sizeof msg, "skip-gram model negative weight %g is negative or not finite (element %lld)", (double)w,
                 (long long)i);
    return bpe_fail(BPE_ERR_ARG, msg);
}

// loss and gradients (into the model's gradient array) from device planes and a device set; *loss on the host
int sgn_forward(bpe_sgmodel *M, const int32_t *d_t, const int32_t *d_c, const int64_t *d_k, int64_t U,
                const int32_t *d_ids, const float *d_w, int64_t S, double neg_k, double *loss) {
    bpe_sgmodel_sgns_stats &st = M->nstats;
    st.calls++;
    M->dstats.calls++;
    char msg[128];
    if (U < 0 || (U && (!d_t || !d_c || !d_k))) return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model planes");
    if (S < 0 || S > M->V) {
        snprintf(msg, sizeof msg, "skip-gram model negatives %lld outside [0, %d]", (long long)S, M->V);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    if (!(neg_k >= 0 && std::isfinite(neg_k))) {
        snprintf(msg, sizeof msg, "skip-gram model neg_k %g is negative or not finite", neg_k);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    if (S && !d_ids) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model negative ids");
    SGM_TRY(hipSetDevice(M->device));
    int64_t P = 0;
    if (int rc = sgm_index(M, d_t, d_c, d_k, U, &P, &st.kernel_ms)) return rc;
    unsigned long long h[SGMH_WORDS] = {SGM_NONE, (unsigned long long)P, 0, 0};
    if (S) {
        SGM_TRY(hipMemcpyAsync(M->d_hdr, h, sizeof h, hipMemcpyHostToDevice, M->stream));
        k_sgns_set_check<<<(unsigned)((S + 255) / 256), 256, 0, M->stream>>>(d_ids, d_w, (int)S, M->V, M->d_hdr);
        SGM_TRY(hipGetLastError());
        SGM_TRY(hipMemcpyAsync(h, M->d_hdr, sizeof h, hipMemcpyDeviceToHost, M->stream));
        SGM_TRY(hipStreamSynchronize(M->stream));
        if (h[SGMH_ERR] != SGM_NONE) return sgn_bad_set(M, d_ids, d_w, (int64_t)h[SGMH_ERR]);
    }
    st.elements += U;
    st.pairs += P;
    if (loss) *loss = 0.0;
    if (P == 0) {
        SGM_TRY(hipMemsetAsync(M->d_g, 0, (size_t)M->n4 * 16, M->stream));
        SGM_TRY(hipStreamSynchronize(M->stream));
        return BPE_OK;
    }
    const int V = M->V, E = M->E;
    const int Sn = neg_k > 0 ? (int)S : 0;   // (k = 0: the positive term alone)
    st.negatives += Sn;
    if (sgd_wanted(M, U)) {   // the dense-count form (bpe_sgdense.hip.h): no transposed planes
        SGM_TRY(hipEventRecord(M->ev0, M->stream));
        if (int rc = sgd_run(M, true, d_t, d_c, d_k, U, d_ids, d_w, Sn, neg_k)) return rc;
        SGM_TRY(hipEventRecord(M->ev1, M->stream));
        SGM_TRY(hipMemcpyAsync(h, M->d_hdr, sizeof h, hipMemcpyDeviceToHost, M->stream));
        SGM_TRY(hipStreamSynchronize(M->stream));
        double ms = 0.0;
        if (int rc = sgm_time(M, &ms)) return rc;
        st.kernel_ms += ms;
        M->dstats.kernel_ms += ms;
        if (loss) std::memcpy(loss, &h[SGMH_LOSS], 8);
        return BPE_OK;
    }
    M->dstats.last_form = BPE_SGM_FORM_CSR;
    M->dstats.last_splits = 0;
    const int nb = (V + SGN_ROWS - 1) / SGN_ROWS;
    const int rpc = (V + SGN_MAX_CHUNKS - 1) / SGN_MAX_CHUNKS, n_chunks = (V + rpc - 1) / rpc;
    int splits = 1, bps = nb;
    if (Sn) {
        const int n_res = (Sn + SGN_ROWS - 1) / SGN_ROWS;
        splits = std::min(std::min(nb, SGN_MAX_SPLITS), std::max(1, (2 * M->n_cus + n_res - 1) / n_res));
        bps = (nb + splits - 1) / splits;
        splits = (nb + bps - 1) / bps;
    }
    const size_t SP = (size_t)(Sn + SGN_ROWS - 1) / SGN_ROWS * SGN_ROWS;
    auto up = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t sizes[] = {up((size_t)U * 8), up((size_t)(V + 1) * 8), up((size_t)nb * 8), up((size_t)U * 4), up((size_t)U * 4),
                            up((size_t)n_chunks * V * 4), up((size_t)V * 4), up((size_t)nb * M->EP * 4),
                            up(splits * SP * E * 4), up(splits * SP * 4)};
    size_t total = 0;
    for (size_t b : sizes) total += b;
    if (int rc = sgm_grow(&M->d_ns, &M->ns_cap, (int64_t)total)) return rc;
    char *p = (char *)M->d_ns;
    auto take = [&](int i) { char *r = p; p += sizes[i]; return r; };
    sgn_scratch w;
    w.kT = (int64_t *)take(0), w.colptr = (int64_t *)take(1), w.loss_part = (double *)take(2);
    w.tT = (int32_t *)take(3), w.cT = (int32_t *)take(4), w.cc = (int32_t *)take(5), w.tot = (int32_t *)take(6);
    w.db1_part = (float *)take(7), w.part = (float *)take(8), w.part_b = (float *)take(9);

    // the transposed planes
    SGM_TRY(hipEventRecord(M->nev[0], M->stream));
    SGM_TRY(hipMemsetAsync(w.cc, 0, sizes[5], M->stream));
    const int64_t ub = (U + 255) / 256;
    k_sgns_colcount<<<(unsigned)(ub < 4096 ? ub : 4096), 256, 0, M->stream>>>(d_t, d_c, U, V, rpc, w.cc);
    k_sgns_coloffs<<<(V + 255) / 256, 256, 0, M->stream>>>(w.cc, V, n_chunks, w.tot);
    k_sgns_colscan<<<1, 1024, 0, M->stream>>>(w.tot, V, w.colptr);
    k_sgns_place<<<n_chunks, 256, 0, M->stream>>>(M->d_rowptr, d_c, d_k, V, rpc, w.cc, w.colptr, w.tT, w.cT, w.kT);
    SGM_TRY(hipGetLastError());
    SGM_TRY(hipEventRecord(M->nev[1], M->stream));

    sgn_args a = {};
    a.Ein = M->d_p + M->o_ein, a.b1 = M->d_p + M->o_b1, a.Eout = M->d_p + M->o_eout, a.b2 = M->d_p + M->o_b2;
    a.V = V, a.E = E;
    a.rowptr = M->d_rowptr, a.n_t = M->d_nt, a.hdr = M->d_hdr;
    a.ptr = M->d_rowptr, a.key_ids = d_c, a.row_ids = d_t, a.cnt = d_k;
    a.neg_ids = d_ids, a.neg_w = d_w, a.S = Sn, a.neg_k = neg_k, a.bps = bps;
    switch (M->EP) {
        case 64: sgn_launch<64>(M, a, w, splits, M->nev[2]); break;
        case 128: sgn_launch<128>(M, a, w, splits, M->nev[2]); break;
        default: sgn_launch<256>(M, a, w, splits, M->nev[2]); break;
    }
    SGM_TRY(hipGetLastError());
    SGM_TRY(hipEventRecord(M->nev[3], M->stream));
    SGM_TRY(hipMemcpyAsync(h, M->d_hdr, sizeof h, hipMemcpyDeviceToHost, M->stream));
    SGM_TRY(hipStreamSynchronize(M->stream));
    float ms[3] = {0.f, 0.f, 0.f};
    for (int i = 0; i < 3; ++i) SGM_TRY(hipEventElapsedTime(&ms[i], M->nev[i], M->nev[i + 1]));
    st.transpose_ms += ms[0];
    st.target_ms += ms[1];
    st.context_ms += ms[2];
    st.kernel_ms += ms[0] + ms[1] + ms[2];
    double L = 0.0;
    std::memcpy(&L, &h[SGMH_LOSS], 8);
    if (loss) *loss = L;
    return BPE_OK;
}

// the negative set of a host form, in the model's io scratch
int sgn_stage_set(bpe_sgmodel *M, const int32_t *ids, const float *w, int64_t S, const int32_t **d_ids, const float **d_w) {
    *d_ids = nullptr;
    *d_w = nullptr;
    if (S <= 0 || S > M->V || !ids) return BPE_OK;   // (sgn_forward refuses what is wrong)
    SGM_TRY(hipSetDevice(M->device));
    const int64_t ib = (S * 4 + 15) / 16 * 16;
    if (int rc = sgm_grow(&M->d_io, &M->io_cap, 2 * ib)) return rc;
    SGM_TRY(hipMemcpy(M->d_io, ids, (size_t)S * 4, hipMemcpyHostToDevice));
    *d_ids = (const int32_t *)M->d_io;
    if (w) {
        SGM_TRY(hipMemcpy((char *)M->d_io + ib, w, (size_t)S * 4, hipMemcpyHostToDevice));
        *d_w = (const float *)((char *)M->d_io + ib);
    }
    return BPE_OK;
}

}  // namespace

extern "C" {

int bpe_sgmodel_sgns_loss_grad_device(bpe_sgmodel *M, const int32_t *d_targets, const int32_t *d_contexts,
                                      const int64_t *d_counts, int64_t U, const int32_t *d_neg_ids,
                                      const float *d_neg_weights, int64_t S, double neg_k, double *loss, float *d_dEin,
                                      float *d_db1, float *d_dEout, float *d_db2) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (int rc = sgn_forward(M, d_targets, d_contexts, d_counts, U, d_neg_ids, d_neg_weights, S, neg_k, loss)) return rc;
    return sgm_copy_sections(M, M->d_g, d_dEin, d_db1, d_dEout, d_db2, false, hipMemcpyDeviceToDevice);
}

int bpe_sgmodel_sgns_loss_grad(bpe_sgmodel *M, const int32_t *targets, const int32_t *contexts, const int64_t *counts,
                               int64_t U, const int32_t *neg_ids, const float *neg_weights, int64_t S, double neg_k,
                               double *loss, float *dEin, float *db1, float *dEout, float *db2) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (U > 0 && (!targets || !contexts || !counts))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model planes");
    const int32_t *d_t, *d_c, *d_ids;
    const int64_t *d_k;
    const float *d_w;
    if (int rc = sgm_stage(M, targets, contexts, counts, U, &d_t, &d_c, &d_k)) return rc;
    if (int rc = sgn_stage_set(M, neg_ids, neg_weights, S, &d_ids, &d_w)) return rc;
    if (int rc = sgn_forward(M, d_t, d_c, d_k, U, d_ids, d_w, S, neg_k, loss)) return rc;
    return sgm_copy_sections(M, M->d_g, dEin, db1, dEout, db2, false, hipMemcpyDeviceToHost);
}

int bpe_sgmodel_sgns_adam_step_device(bpe_sgmodel *M, const int32_t *d_targets, const int32_t *d_contexts,
                                      const int64_t *d_counts, int64_t U, const int32_t *d_neg_ids,
                                      const float *d_neg_weights, int64_t S, double neg_k, double lr, double beta1,
                                      double beta2, double eps, double *loss) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (!(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1))
        return bpe_fail(BPE_ERR_ARG, "bpe native: skip-gram model betas outside [0, 1)");
    if (int rc = sgn_forward(M, d_targets, d_contexts, d_counts, U, d_neg_ids, d_neg_weights, S, neg_k, loss)) return rc;
    return sgm_adam(M, lr, beta1, beta2, eps, &M->nstats.kernel_ms);
}

int bpe_sgmodel_sgns_adam_step(bpe_sgmodel *M, const int32_t *targets, const int32_t *contexts, const int64_t *counts,
                               int64_t U, const int32_t *neg_ids, const float *neg_weights, int64_t S, double neg_k,
                               double lr, double beta1, double beta2, double eps, double *loss) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (U > 0 && (!targets || !contexts || !counts))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model planes");
    const int32_t *d_t, *d_c, *d_ids;
    const int64_t *d_k;
    const float *d_w;
    if (int rc = sgm_stage(M, targets, contexts, counts, U, &d_t, &d_c, &d_k)) return rc;
    if (int rc = sgn_stage_set(M, neg_ids, neg_weights, S, &d_ids, &d_w)) return rc;
    return bpe_sgmodel_sgns_adam_step_device(M, d_t, d_c, d_k, U, d_ids, d_w, S, neg_k, lr, beta1, beta2, eps, loss);
}

int bpe_sgmodel_get_sgns_stats(bpe_sgmodel *M, bpe_sgmodel_sgns_stats *out) {
    if (!M || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = M->nstats;
    return BPE_OK;
}

int bpe_sgmodel_reset_sgns_stats(bpe_sgmodel *M) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    M->nstats = {};
    return BPE_OK;
}

}  // extern "C"
