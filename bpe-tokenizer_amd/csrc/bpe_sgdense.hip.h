// bpe_sgdense.hip.h — the dense-count form of the skip-gram model's training step (include/bpe.h,
// "skip-gram model, dense counts"): the rules of bpe_sgmodel.hip (full softmax) and bpe_sgns.hip.h (negative
// sampling) with the counts read from a V x V fp32 tile source instead of walked as CSR entries.  Part of
// bpe_sgmodel.hip's translation unit (its struct, SGM_TRY, sgm_mfma, sgm_acc_row, sgm_grow and k_sgm_reduce
// are in scope).  DESIGN.md §3r.
//
//   W[Vp][Vp]  fl32(C[t,c] / P), Vp = V rounded up to 64, zero elsewhere; omega[Vp] = fl32(k w_s) at a_s, zero
//              elsewhere.  Zeroed and scattered from the checked planes on every call (keys are distinct:
//              plain stores); the buffer is the model's, allocated on its first dense call.
//
// One tile loop, k_sgd<EP, MODE, SIDE>.  A workgroup is two waves that own 64 resident rows (a wave 32),
// staged in LDS and zero-padded to EP; grid.y splits the streamed axis in units of 64.  32-row key tiles
// stream through two LDS buffers behind a register prefetch (at EP = 256, where O^T alone takes 128
// registers, staged behind the products).  S^T = K . R^T by v_mfma_f32_32x32x2_f32 leaves a resident row's
// 32 logits of the tile in the accumulators of its two lanes; the matching cells of W are loaded straight
// into the same lanes; G is formed there and O^T += K^T . G^T takes it as its B operand from those
// registers.  z and G never leave registers.
//   SGD_TGT  resident: rows of H = Ein + b1 with lse_t and n_t / P.  Keys: rows of Eout with b2 (and omega).
//            A lane's 16 cells of W are four runs of four: 16-byte loads.  Out: a dEin partial per split,
//            the block's column sums for db1, its loss partial (fp32 within a tile, then double).
//   SGD_CTX  resident: rows of Eout with b2 (and omega).  Keys: rows of H with lse_t and n_t / P; tiles
//            whose rows have no counts are skipped on a uniform branch.  For one register the wave's lanes
//            read two runs of 32 consecutive cells of W: coalesced, no LDS pass.  Out: a dEout partial per
//            split and db2 in-lane behind it.
//   SGD_STAT (full softmax, before the others) the SGD_TGT stream with no W and no O: the running
//            (max, sum) of a row's logits per split; k_sgd_lse merges them in split order into lse_t.
// k_sgm_reduce sums the blocks' db1 and loss partials in block order, k_sgd_sum the splits' rows in split
// order.  No floating-point atomics, every sum in a fixed order: for one form and one split count the same
// bytes on every run and route.  The bytes differ from the CSR form's and between split counts.

namespace {

constexpr int SGD_RES = 64;                 // resident rows of a workgroup, the unit of a split
constexpr int SGD_SUB = 32;                 // rows of a key tile
constexpr int SGD_WG = 128;
constexpr int SGD_STAT = 0, SGD_SOFT = 1, SGD_SGNS = 2;
constexpr int SGD_TGT = 0, SGD_CTX = 1;
static_assert(SGD_RES == BPE_SGM_TILE, "the tests place sizes around it");

struct sgd_args {
    const float *Ein, *b1, *Eout, *b2;
    int V, E, Vp;
    const int64_t *rowptr, *n_t;
    const unsigned long long *hdr;
    const float *W, *omega;
    float *lse;                // SGD_STAT: unused; the others read it
    int tps;                   // units of SGD_RES streamed rows per split
    float *out;                // SGD_TGT: [splits][V][E]; SGD_CTX: [splits][V E + V] (rows, then db2)
    float *db1_part;           // SGD_TGT: [blocks][EP]
    double *loss_part;         // SGD_TGT: [blocks]
    float2 *ml;                // SGD_STAT: [V][splits]
};

__global__ __launch_bounds__(256) void k_sgd_fill(const int32_t *__restrict__ tg, const int32_t *__restrict__ cx,
                                                  const int64_t *__restrict__ cnt, int64_t U, int Vp,
                                                  const unsigned long long *__restrict__ hdr, float *__restrict__ W) {
    const double inv_P = 1.0 / (double)(long long)hdr[SGMH_P];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < U; i += stride)
        W[(size_t)tg[i] * Vp + cx[i]] = (float)((double)cnt[i] * inv_P);
}

__global__ __launch_bounds__(256) void k_sgd_omega(const int32_t *__restrict__ ids, const float *__restrict__ w, int S,
                                                   double neg_k, float *__restrict__ omega) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S) omega[ids[s]] = (float)(neg_k * (w ? (double)w[s] : 1.0 / S));
}

// a tile's 32 logits of one row (16 in this lane, 16 in lane ^ 32) folded into the row's running (max, sum)
__device__ __forceinline__ void sgd_ml_tile(const f16v &s, float &m_run, float &l_run) {
    float mx = -INFINITY;
#pragma unroll
    for (int v = 0; v < 16; ++v) mx = fmaxf(mx, s[v]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    float ps = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) ps += expf(s[v] - m_new);
    ps += __shfl_xor(ps, 32, 64);
    l_run = l_run * expf(m_run - m_new) + ps;   // (0 on the first tile: m_run is -inf, m_new is not)
    m_run = m_new;
}

__global__ __launch_bounds__(256) void k_sgd_lse(const float2 *__restrict__ ml, int V, int splits, float *__restrict__ lse) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= V) return;
    const float2 *p = ml + (size_t)t * splits;
    float mx = -INFINITY, l = 0.f;
    for (int s = 0; s < splits; ++s) mx = fmaxf(mx, p[s].x);
    for (int s = 0; s < splits; ++s) l += p[s].y * expf(p[s].x - mx);
    lse[t] = mx + logf(l);
}

template <int EP>
constexpr size_t sgd_lds() {
    return (size_t)SGD_WG * 8 + (size_t)((SGD_RES + 2 * SGD_SUB) * (EP + 1) + 4 * SGD_SUB) * 4;
}
static_assert(sgd_lds<256>() <= 160 * 1024, "LDS of the widest instantiation");

template <int EP, int MODE, int SIDE>
__global__ __launch_bounds__(SGD_WG) void k_sgd(const sgd_args a) {
    static_assert(MODE != SGD_STAT || SIDE == SGD_TGT, "the statistic streams Eout");
    constexpr int LD = EP + 1;                    // odd: a column of 32 rows touches 32 banks
    constexpr int NEB = EP / 32;
    constexpr int NPRE = SGD_SUB * EP / SGD_WG;   // staged floats per thread and tile
    constexpr bool PRE = EP <= 128 || MODE == SGD_STAT;   // (the statistic keeps no O^T)
    extern __shared__ double smem_d[];
    double *red = smem_d;                         // [SGD_WG]
    float *Rs = (float *)(red + SGD_WG);          // [64][LD]: the resident rows
    float *Ks = Rs + SGD_RES * LD;                // [2][32][LD]: key tiles; after the stream: O, [64][LD]
    float *kbs = Ks + 2 * SGD_SUB * LD;           // [2][32]: a key's b2 (SGD_TGT) or lse_t (SGD_CTX)
    float *kws = kbs + 2 * SGD_SUB;               // [2][32]: ... omega or n_t / P

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane & 31, half = lane >> 5;
    const int V = a.V, E = a.E, Vp = a.Vp;
    const int Ek = (E + 1) & ~1;
    const int R0 = blockIdx.x * SGD_RES, split = blockIdx.y;
    const int my = R0 + w * 32 + q;               // this lane's resident row
    const bool in = my < V;
    const double inv_P = 1.0 / (double)(long long)a.hdr[SGMH_P];
    const float *rbase = SIDE == SGD_TGT ? a.Ein : a.Eout;
    const float *kbase = SIDE == SGD_TGT ? a.Eout : a.Ein;

    for (int idx = tid; idx < SGD_RES * EP; idx += SGD_WG) {
        const int r = idx / EP, e = idx % EP;
        float x = 0.f;
        if (R0 + r < V && e < E) x = rbase[(size_t)(R0 + r) * E + e] + (SIDE == SGD_TGT ? a.b1[e] : 0.f);
        Rs[r * LD + e] = x;
    }
    // the lane's row: n_t / P and lse_t of a target, b2 and omega of a context (a padded context's logits
    // are -inf under the softmax, and 0 with no weight under negative sampling)
    double r_wnd = 0.0;
    float r_wn = 0.f, r_lse = 0.f, r_b = MODE == SGD_SOFT ? -INFINITY : 0.f, r_om = 0.f;
    if (in) {
        if (SIDE == SGD_TGT) {
            r_wnd = (double)a.n_t[my] * inv_P;
            r_wn = (float)r_wnd;
            if (MODE == SGD_SOFT) r_lse = a.lse[my];
        } else {
            r_b = a.b2[my];
            if (MODE == SGD_SGNS) r_om = a.omega[my];
        }
    }

    const int n_kt = (V + SGD_SUB - 1) / SGD_SUB;
    const int j0 = split * a.tps * (SGD_RES / SGD_SUB), j1 = min(n_kt, j0 + a.tps * (SGD_RES / SGD_SUB));
    auto next_tile = [&](int j) {   // SGD_CTX: the first tile from j on whose rows have count entries (uniform)
        if (SIDE == SGD_CTX)
            while (j < j1 && a.rowptr[min(V, (j + 1) * SGD_SUB)] == a.rowptr[j * SGD_SUB]) ++j;
        return j;
    };
    auto tile_value = [&](int j, int idx) {
        const int e = idx % EP, c = j * SGD_SUB + idx / EP;
        if (c >= V || e >= E) return 0.f;
        return kbase[(size_t)c * E + e] + (SIDE == SGD_CTX ? a.b1[e] : 0.f);
    };
    auto tile_meta = [&](int j, float &kb, float &kw) {   // (threads < 32; omega is padded to Vp)
        const int c = j * SGD_SUB + tid;
        if (SIDE == SGD_TGT) {
            kb = c < V ? a.b2[c] : (MODE == SGD_SGNS ? 0.f : -INFINITY);
            kw = MODE == SGD_SGNS ? a.omega[c] : 0.f;
        } else {
            kb = (MODE == SGD_SOFT && c < V) ? a.lse[c] : 0.f;
            kw = c < V ? (float)((double)a.n_t[c] * inv_P) : 0.f;
        }
    };
    float pre[PRE ? NPRE : 1], pre_kb = 0.f, pre_kw = 0.f;
    auto load_tile = [&](int j) {
#pragma unroll
        for (int i = 0; i < (PRE ? NPRE : 0); ++i) pre[i] = tile_value(j, tid + i * SGD_WG);
        if (tid < SGD_SUB) tile_meta(j, pre_kb, pre_kw);
    };
    auto store_meta = [&](int buf) {
        if (tid < SGD_SUB) {
            kbs[buf * SGD_SUB + tid] = pre_kb;
            kws[buf * SGD_SUB + tid] = pre_kw;
        }
    };
    auto store_tile = [&](int buf) {
        float *Kb = Ks + buf * SGD_SUB * LD;
#pragma unroll
        for (int i = 0; i < (PRE ? NPRE : 0); ++i) {
            const int idx = tid + i * SGD_WG;
            Kb[(idx / EP) * LD + idx % EP] = pre[i];
        }
        store_meta(buf);
    };
    auto stage_tile = [&](int j, int buf) {
        float *Kb = Ks + buf * SGD_SUB * LD;
#pragma unroll 8
        for (int i = 0; i < NPRE; ++i) {
            const int idx = tid + i * SGD_WG;
            Kb[(idx / EP) * LD + idx % EP] = tile_value(j, idx);
        }
        if (tid < SGD_SUB) tile_meta(j, pre_kb, pre_kw);
        store_meta(buf);
    };

    f16v O[MODE == SGD_STAT ? 1 : NEB];
#pragma unroll
    for (int eb = 0; eb < (MODE == SGD_STAT ? 1 : NEB); ++eb)
#pragma unroll
        for (int v = 0; v < 16; ++v) O[eb][v] = 0.f;
    double loss = 0.0;
    float gsum = 0.f, m_run = -INFINITY, l_run = 0.f;
    const float *Rw = Rs + (w * 32 + q) * LD + half;

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
        // the lane's 16 cells of W: rows and columns below Vp, where the padding is zero
        float wv[16];
        if (MODE != SGD_STAT) {
            if (SIDE == SGD_TGT) {
                const float4 *wp = (const float4 *)(a.W + (size_t)my * Vp + j * SGD_SUB + 4 * half);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 x = wp[2 * g];
                    wv[4 * g] = x.x, wv[4 * g + 1] = x.y, wv[4 * g + 2] = x.z, wv[4 * g + 3] = x.w;
                }
            } else {
#pragma unroll
                for (int v = 0; v < 16; ++v) wv[v] = a.W[(size_t)(j * SGD_SUB + sgm_acc_row(v, half)) * Vp + my];
            }
        }
        const float *Kb = Ks + buf * SGD_SUB * LD;
        // S^T[key][row] = sum_k K[key][k] R[row][k]
        f16v s;
#pragma unroll
        for (int v = 0; v < 16; ++v) s[v] = 0.f;
        const float *Ka = Kb + q * LD + half;
        for (int k = 0; k < Ek; k += 2) s = sgm_mfma(Ka[k], Rw[k], s);
        if (MODE == SGD_STAT) {
#pragma unroll
            for (int v = 0; v < 16; ++v) s[v] += kbs[buf * SGD_SUB + sgm_acc_row(v, half)];
            sgd_ml_tile(s, m_run, l_run);
        } else {
            float lt = 0.f;   // this tile's share of the lane's loss (16 terms), then on in double
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int slot = buf * SGD_SUB + sgm_acc_row(v, half);
                const float z = s[v] + (SIDE == SGD_TGT ? kbs[slot] : r_b);
                const float wn = SIDE == SGD_TGT ? r_wn : kws[slot];
                float g;
                if (MODE == SGD_SOFT) {
                    const float lse = SIDE == SGD_TGT ? r_lse : kbs[slot];
                    g = (wn > 0.f ? wn * expf(z - lse) : 0.f) - wv[v];
                    if (SIDE == SGD_TGT) lt -= wv[v] > 0.f ? wv[v] * z : 0.f;
                } else {
                    const float ww = wn * (SIDE == SGD_TGT ? kws[slot] : r_om);
                    const float e = expf(-fabsf(z));
                    const float hi = 1.f / (1.f + e), lo = e * hi;   // sigma(|z|), sigma(-|z|)
                    g = ww * (z >= 0.f ? hi : lo) - wv[v] * (z >= 0.f ? lo : hi);
                    if (SIDE == SGD_TGT) {
                        const float l1p = log1pf(e);
                        lt -= wv[v] * (fminf(z, 0.f) - l1p) + ww * (fminf(-z, 0.f) - l1p);
                    }
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
        }
        // (the other buffer was last read before this iteration's barrier)
        if (!PRE && nx < j1) stage_tile(nx, buf ^ 1);
        j = nx;
        ++it;
    }

    if (MODE == SGD_STAT) {
        if (in && half == 0) a.ml[(size_t)my * gridDim.y + split] = make_float2(m_run, l_run);
        return;
    }
    __syncthreads();   // the last tile has been read by both waves: Ks becomes Os

    float *Os = Ks;
#pragma unroll
    for (int eb = 0; eb < NEB; ++eb)
#pragma unroll
        for (int v = 0; v < 16; ++v) Os[(w * 32 + q) * LD + eb * 32 + sgm_acc_row(v, half)] = O[eb][v];
    if (SIDE == SGD_TGT) {
        if (MODE == SGD_SOFT && split == 0 && half == 0) loss += r_wnd * (double)r_lse;   // n_t lse_t / P, once
        red[tid] = loss;
    }
    __syncthreads();

    const int nrows = min(SGD_RES, V - R0);
    const size_t VE = (size_t)V * E;
    float *out = a.out + (size_t)split * (SIDE == SGD_TGT ? VE : VE + V);
    for (int i = tid; i < nrows * E; i += SGD_WG) out[(size_t)R0 * E + i] = Os[(i / E) * LD + i % E];
    if (SIDE == SGD_TGT) {
        const size_t b = (size_t)split * gridDim.x + blockIdx.x;
        for (int e = tid; e < EP; e += SGD_WG) {
            float c = 0.f;
            for (int r = 0; r < SGD_RES; ++r) c += Os[r * LD + e];   // (rows past V are zero)
            a.db1_part[b * EP + e] = c;
        }
        if (tid == 0) {
            double c = 0.0;
            for (int i = 0; i < SGD_WG; ++i) c += red[i];
            a.loss_part[b] = c;
        }
    } else {
        gsum += __shfl_xor(gsum, 32, 64);
        if (half == 0 && in) out[VE + my] = gsum;
    }
}

// dst[i] = the splits' part[sp][i] in split order
__global__ __launch_bounds__(256) void k_sgd_sum(const float *__restrict__ part, int64_t n, int splits,
                                                 float *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float c = 0.f;
    for (int sp = 0; sp < splits; ++sp) c += part[(size_t)sp * n + i];
    dst[i] = c;
}

template <int EP, int MODE, int SIDE>
hipError_t sgd_lds_attr() {
    return hipFuncSetAttribute((const void *)k_sgd<EP, MODE, SIDE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)sgd_lds<EP>());
}

template <int EP>
hipError_t sgd_lds_attrs() {
    for (hipError_t e : {sgd_lds_attr<EP, SGD_STAT, SGD_TGT>(), sgd_lds_attr<EP, SGD_SOFT, SGD_TGT>(),
                         sgd_lds_attr<EP, SGD_SOFT, SGD_CTX>(), sgd_lds_attr<EP, SGD_SGNS, SGD_TGT>(),
                         sgd_lds_attr<EP, SGD_SGNS, SGD_CTX>()})
        if (e != hipSuccess) return e;
    return hipSuccess;
}

template <int EP>
void sgd_launch(bpe_sgmodel *M, sgd_args a, bool sgns, int tiles, int splits, float *part_t, float *part_c) {
    const dim3 grid((unsigned)tiles, (unsigned)splits);
    const int64_t VE = (int64_t)M->V * M->E;
    float *g = M->d_g;
    if (!sgns) {
        k_sgd<EP, SGD_STAT, SGD_TGT><<<grid, SGD_WG, sgd_lds<EP>(), M->stream>>>(a);
        k_sgd_lse<<<(M->V + 255) / 256, 256, 0, M->stream>>>(a.ml, M->V, splits, a.lse);
    }
    a.out = part_t;
    if (sgns) k_sgd<EP, SGD_SGNS, SGD_TGT><<<grid, SGD_WG, sgd_lds<EP>(), M->stream>>>(a);
    else k_sgd<EP, SGD_SOFT, SGD_TGT><<<grid, SGD_WG, sgd_lds<EP>(), M->stream>>>(a);
    k_sgm_reduce<<<1, 256, 0, M->stream>>>(a.db1_part, a.loss_part, tiles * splits, EP, M->E, g + M->o_b1, M->d_hdr);
    k_sgd_sum<<<(unsigned)((VE + 255) / 256), 256, 0, M->stream>>>(part_t, VE, splits, g + M->o_ein);
    a.out = part_c;
    if (sgns) k_sgd<EP, SGD_SGNS, SGD_CTX><<<grid, SGD_WG, sgd_lds<EP>(), M->stream>>>(a);
    else k_sgd<EP, SGD_SOFT, SGD_CTX><<<grid, SGD_WG, sgd_lds<EP>(), M->stream>>>(a);
    k_sgd_sum<<<(unsigned)((VE + M->V + 255) / 256), 256, 0, M->stream>>>(part_c, VE + M->V, splits, g + M->o_eout);
}

// what a call with U elements runs under the model's form
bool sgd_wanted(const bpe_sgmodel *M, int64_t U) {
    if (M->form == BPE_SGM_FORM_AUTO) return (double)U >= BPE_SGM_DENSE_THETA * (double)M->V * (double)M->V;
    return M->form == BPE_SGM_FORM_DENSE;
}

// the gradients of checked planes (P > 0, left in the header) into the model's gradient array and the loss
// into the header, all on the model's stream between ev0 and ev1; the caller synchronises
int sgd_run(bpe_sgmodel *M, bool sgns, const int32_t *d_t, const int32_t *d_c, const int64_t *d_k, int64_t U,
            const int32_t *d_ids, const float *d_w, int S, double neg_k) {
    const int V = M->V, E = M->E, Vp = (V + SGD_RES - 1) / SGD_RES * SGD_RES, tiles = Vp / SGD_RES;
    // tiles x splits cover the machine about twice (the queries' rule); a split is at least one unit of 64
    int splits = M->form_splits ? M->form_splits : tiles >= 2 * M->n_cus ? 1 : (2 * M->n_cus + tiles - 1) / tiles;
    splits = std::min(splits, tiles);
    const int tps = (tiles + splits - 1) / splits;
    splits = (tiles + tps - 1) / tps;   // (no split without a tile)
    const size_t w_bytes = ((size_t)Vp * Vp + Vp) * 4;
    if (!M->d_W) {
        if (sgd_lds_attrs<64>() != hipSuccess || sgd_lds_attrs<128>() != hipSuccess || sgd_lds_attrs<256>() != hipSuccess)
            return bpe_fail(BPE_ERR_HIP, "bpe native: skip-gram model dense-count LDS attribute");
        if (hipMalloc((void **)&M->d_W, w_bytes) != hipSuccess) {
            (void)hipGetLastError();
            M->d_W = nullptr;
            return bpe_fail(BPE_ERR_OOM, "bpe native: skip-gram model dense count tiles");
        }
    }
    const size_t VE = (size_t)V * E;
    auto up = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t sizes[] = {up((size_t)tiles * splits * 8), up((size_t)V * splits * 8), up(splits * VE * 4),
                            up(splits * (VE + V) * 4), up((size_t)tiles * splits * M->EP * 4)};
    size_t total = 0;
    for (size_t b : sizes) total += b;
    if (int rc = sgm_grow(&M->d_ds, &M->ds_cap, (int64_t)total)) return rc;
    char *p = (char *)M->d_ds;
    auto take = [&](int i) { char *r = p; p += sizes[i]; return r; };
    sgd_args a = {};
    a.Ein = M->d_p + M->o_ein, a.b1 = M->d_p + M->o_b1, a.Eout = M->d_p + M->o_eout, a.b2 = M->d_p + M->o_b2;
    a.V = V, a.E = E, a.Vp = Vp;
    a.rowptr = M->d_rowptr, a.n_t = M->d_nt, a.hdr = M->d_hdr;
    a.W = M->d_W, a.omega = M->d_W + (size_t)Vp * Vp, a.lse = M->d_lse, a.tps = tps;
    a.loss_part = (double *)take(0), a.ml = (float2 *)take(1);
    float *part_t = (float *)take(2), *part_c = (float *)take(3);
    a.db1_part = (float *)take(4);

    SGM_TRY(hipMemsetAsync(M->d_W, 0, w_bytes, M->stream));
    const int64_t ub = (U + 255) / 256;
    k_sgd_fill<<<(unsigned)(ub < 4096 ? ub : 4096), 256, 0, M->stream>>>(d_t, d_c, d_k, U, Vp, M->d_hdr, M->d_W);
    if (sgns && S)
        k_sgd_omega<<<(unsigned)((S + 255) / 256), 256, 0, M->stream>>>(d_ids, d_w, S, neg_k, M->d_W + (size_t)Vp * Vp);
    switch (M->EP) {
        case 64: sgd_launch<64>(M, a, sgns, tiles, splits, part_t, part_c); break;
        case 128: sgd_launch<128>(M, a, sgns, tiles, splits, part_t, part_c); break;
        default: sgd_launch<256>(M, a, sgns, tiles, splits, part_t, part_c); break;
    }
    SGM_TRY(hipGetLastError());
    M->dstats.dense_calls++;
    M->dstats.last_form = BPE_SGM_FORM_DENSE;
    M->dstats.last_splits = splits;
    return BPE_OK;
}

}  // namespace

extern "C" {

int bpe_sgmodel_set_counts_form(bpe_sgmodel *M, int form, int splits) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    char msg[160];
    if (form != BPE_SGM_FORM_CSR && form != BPE_SGM_FORM_DENSE && form != BPE_SGM_FORM_AUTO) {
        snprintf(msg, sizeof msg, "skip-gram model counts form %d is none of BPE_SGM_FORM_CSR, _DENSE, _AUTO", form);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    if (splits < 0 || splits > BPE_SGM_MAX_SPLITS) {
        snprintf(msg, sizeof msg, "skip-gram model splits %d outside [0, %d]", splits, BPE_SGM_MAX_SPLITS);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    M->form = form;
    M->form_splits = splits;
    return BPE_OK;
}

int bpe_sgmodel_get_dense_stats(bpe_sgmodel *M, bpe_sgmodel_dense_stats *out) {
    if (!M || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = M->dstats;
    return BPE_OK;
}

int bpe_sgmodel_reset_dense_stats(bpe_sgmodel *M) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    M->dstats = {};
    return BPE_OK;
}

}  // extern "C"
