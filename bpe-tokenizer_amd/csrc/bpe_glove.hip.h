// bpe_glove.hip.h — GloVe on the skip-gram model's parameters (include/bpe.h, "skip-gram model, GloVe"):
// loss, gradients and Adam from the count planes, with one more parameter array, the target bias bt[V].
// Part of bpe_sgmodel.hip's translation unit (its struct, SGM_TRY, sgm_grow, sgm_index, sgm_stage,
// sgm_copy_sections, k_sgm_adam and the k_sgns_col* / k_sgns_place kernels are in scope).  DESIGN.md §3s.
//
//   cells: the elements with C > 0, N of them.  H_t = Ein[t] + b1, z(t,c) = H_t . Eout[c] + b2[c] + bt[t],
//   l = fl32(log C), f = fl32(min(1, (C / x_max)^alpha)) (both in double from the int64 count), r = z - l,
//   L = (1/(2N)) sum f r^2,  G[t,c] = (1/N) f r on the cells,
//   dEin = G Eout, db1 its column sums, dbt the row sums of G, dEout = G^T H, db2 the column sums of G.
// The work is exactly the N cells: an SDDMM and an SpMM at about half a flop per gathered byte, so there
// is no matrix instruction here; the kernel is built around gather width, loads in flight and a split
// that does not depend on row lengths.
//
//   k_glv_count    the cells counted (integer atomics) and, per GLV_CHUNK elements, for the compaction;
//   k_glv_scan / k_glv_compact / k_glv_rowptr   only when some element has C == 0: the cells alone, in
//                  order, as planes of their own with their row pointers.  Everything below runs over the
//                  cells, so zero-count elements change no byte of the result;
//   k_sgns_col* / k_sgns_place (bpe_sgns.hip.h)  the transposed planes (c, t, C) for the context side;
//   k_glv<EP, SIDE>  one walk for both sides.  The cell range [0, N) is cut into runs of GLV_RUN consecutive
//                  cells; a lane group of EP / 4 lanes owns one run (four groups to a wave at EP = 64, two
//                  at 128, one at 256), a workgroup is four waves, the grid depends on N only.  A wave
//                  first loads its runs' row ids, key ids and counts coalesced, one cell per lane and
//                  pass; each lane takes its cells' l and f (the double log and pow at full occupancy) and
//                  writes (row id, key id, l, f) as a 16-byte record to LDS.  Then the groups walk their
//                  runs from LDS.  A lane holds elements 4l .. 4l + 3 of a row (one 16-byte load where
//                  E % 4 == 0, two 8-byte loads where E % 2 == 0, four 4-byte loads otherwise; zeros past
//                  E).  The resident row (H_t on the target side, Eout[c] on the context side) is reloaded
//                  only when the row id changes; the key rows of four cells are gathered before the first
//                  dot is reduced.  The dot is reduced inside the group by DPP row operations (a group of
//                  16 is one DPP row; the wider groups add one or two cross-row steps), every lane ends
//                  with the same z, g = f r / N, acc += g key in its four registers and the sum of g
//                  beside them.  When the row id changes, a row that began and ended inside the run is
//                  stored straight to its output row; the first and the last row of a run always go to the
//                  run's two carry records;
//   k_glv_carry    a wave per carry record: the first record of a row (the record before it has another
//                  row) adds the row's records in record order and stores the row once.  A row is written
//                  by a group or by this kernel, never both; rows that nothing touches are zeroed by the
//                  memset of the gradient arrays up front;
//   k_glv_colsum   db1 as fixed-order column sums of dEin, in two levels;
//   k_glv_loss     the runs' loss partials (fp32 within four cells, double from there on) in run order.
// No floating-point atomics; every reduction has a fixed order: the same bytes on every run and route.
// The calls always read the planes as entries: bpe_sgmodel_set_counts_form does not apply to them and
// they do not touch the dense statistics.

namespace {

constexpr int GLV_RUN = BPE_GLOVE_RUN;   // cells of a run
constexpr int GLV_WG = 256;
constexpr int GLV_TGT = 0, GLV_CTX = 1;
constexpr int GLV_CHUNK = 1024;          // elements per workgroup of the count and the compaction
constexpr int GLV_COLROWS = 128;         // rows per workgroup of the first level of k_glv_colsum
constexpr int GLVH_N = 3;                // the header word of N (SGMH_WORDS' spare)
static_assert(GLV_RUN % 4 == 0 && GLV_RUN >= 4, "cells are walked four at a time");
static_assert(GLV_CHUNK % 256 == 0, "passes of one workgroup");
static_assert(BPE_SKIPGRAM_COUNTS_MAX_DIM <= GLV_COLROWS * GLV_COLROWS, "two levels of column sums");
static_assert(SGMH_WORDS > GLVH_N, "a header word for N");

struct glv_args {
    const float *Ein, *b1, *Eout, *b2, *bt;
    int V, E;
    const int32_t *rid, *kid;   // GLV_TGT: targets, contexts; GLV_CTX: the transposed planes' contexts, targets
    const int64_t *cnt;
    int64_t N, nruns;
    double x_max, alpha;
    float inv_n;
    float *out, *out_b;         // dEin, dbt / dEout, db2
    int32_t *carry_id;          // [2 nruns]: the row of a carry record, -1: none
    float *carry_s, *carry_row; // [2 nruns], [2 nruns][E]
    double *loss_part;          // [nruns], GLV_TGT
};

// ---- the cells ----
__global__ __launch_bounds__(256) void k_glv_count(const int64_t *__restrict__ cnt, int64_t U, int64_t *__restrict__ part,
                                                   unsigned long long *hdr) {
    __shared__ int wtot[4];
    const int64_t base = (int64_t)blockIdx.x * GLV_CHUNK;
    int n = 0;
    for (int p = 0; p < GLV_CHUNK / 256; ++p) {
        const int64_t i = base + p * 256 + threadIdx.x;
        n += (i < U && cnt[i] > 0) ? 1 : 0;
    }
    for (int o = 32; o; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = wtot[0] + wtot[1] + wtot[2] + wtot[3];
        part[blockIdx.x] = t;
        if (t) atomicAdd(&hdr[GLVH_N], (unsigned long long)t);
    }
}

// part[nb] -> its exclusive prefix sums, in place
__global__ __launch_bounds__(1024) void k_glv_scan(int64_t *__restrict__ part, int64_t nb) {
    __shared__ int64_t sh[1024];
    const int tid = threadIdx.x;
    const int64_t per = (nb + 1023) / 1024, b0 = tid * per;
    int64_t s = 0;
    for (int64_t i = 0; i < per; ++i)
        if (b0 + i < nb) s += part[b0 + i];
    sh[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t x = tid >= o ? sh[tid - o] : 0;
        __syncthreads();
        sh[tid] += x;
        __syncthreads();
    }
    int64_t run = sh[tid] - s;
    for (int64_t i = 0; i < per; ++i)
        if (b0 + i < nb) {
            const int64_t x = part[b0 + i];
            part[b0 + i] = run;
            run += x;
        }
}

__global__ __launch_bounds__(256) void k_glv_compact(const int32_t *__restrict__ tg, const int32_t *__restrict__ cx,
                                                     const int64_t *__restrict__ cnt, int64_t U,
                                                     const int64_t *__restrict__ offs, int32_t *__restrict__ tg2,
                                                     int32_t *__restrict__ cx2, int64_t *__restrict__ cnt2) {
    __shared__ int wtot[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * GLV_CHUNK;
    int64_t o = offs[blockIdx.x];
    for (int p = 0; p < GLV_CHUNK / 256; ++p) {
        const int64_t i = base + p * 256 + threadIdx.x;
        const bool keep = i < U && cnt[i] > 0;
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wtot[w] = __popcll(b);
        __syncthreads();
        int before = __popcll(b & ((1ull << lane) - 1ull));
        for (int x = 0; x < w; ++x) before += wtot[x];
        if (keep) {
            tg2[o + before] = tg[i];
            cx2[o + before] = cx[i];
            cnt2[o + before] = cnt[i];
        }
        o += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_glv_rowptr(const int32_t *__restrict__ tg, int64_t N, int V,
                                                    int64_t *__restrict__ rowptr) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= V) rowptr[r] = sgm_lower_bound(tg, 0, N, r);
}

// ---- the walk ----
template <int CTRL>
__device__ __forceinline__ float glv_dpp(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, false));
}

// the sum of x over a lane group of G, the same bits in every lane (a butterfly: both partners add the same pair)
template <int G>
__device__ __forceinline__ float glv_group_sum(float x) {
    x += glv_dpp<0xB1>(x);    // quad_perm [1, 0, 3, 2]
    x += glv_dpp<0x4E>(x);    // quad_perm [2, 3, 0, 1]
    x += glv_dpp<0x141>(x);   // row_half_mirror: the other quad of eight
    x += glv_dpp<0x140>(x);   // row_mirror: the other half of the row
    if (G >= 32) x += __shfl_xor(x, 16, 64);
    if (G >= 64) x += __shfl_xor(x, 32, 64);
    return x;
}

// elements e .. e + 3 of the row at p (zeros past E), VM floats per load
template <int VM>
__device__ __forceinline__ float4 glv_load4(const float *__restrict__ p, int e, int E) {
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e >= E) return x;
    p += e;
    if (VM == 4) {
        x = *(const float4 *)p;
    } else if (VM == 2) {
        const float2 lo = *(const float2 *)p;
        x.x = lo.x, x.y = lo.y;
        if (e + 2 < E) {
            const float2 hi = *(const float2 *)(p + 2);
            x.z = hi.x, x.w = hi.y;
        }
    } else {
        x.x = p[0];
        if (e + 1 < E) x.y = p[1];
        if (e + 2 < E) x.z = p[2];
        if (e + 3 < E) x.w = p[3];
    }
    return x;
}

template <int VM>
__device__ __forceinline__ void glv_store4(float *__restrict__ p, int e, int E, float4 x) {
    if (e >= E) return;
    p += e;
    if (VM == 4) {
        *(float4 *)p = x;
    } else if (VM == 2) {
        *(float2 *)p = make_float2(x.x, x.y);
        if (e + 2 < E) *(float2 *)(p + 2) = make_float2(x.z, x.w);
    } else {
        p[0] = x.x;
        if (e + 1 < E) p[1] = x.y;
        if (e + 2 < E) p[2] = x.z;
        if (e + 3 < E) p[3] = x.w;
    }
}

__device__ __forceinline__ float4 glv_add4(float4 a, float4 b) {
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// one group's run: rec[n_e] in LDS, lane l of the group
template <int EP, int SIDE, int VM>
__device__ __forceinline__ void glv_walk(const glv_args &a, const int4 *rec, int n_e, int64_t run, int l) {
    const int E = a.E, e = 4 * l;
    const float *rbase = SIDE == GLV_TGT ? a.Ein : a.Eout;
    const float *kbase = SIDE == GLV_TGT ? a.Eout : a.Ein;
    const float *rbias = SIDE == GLV_TGT ? a.bt : a.b2;   // the scalar of a resident row, of a key row
    const float *kbias = SIDE == GLV_TGT ? a.b2 : a.bt;
    const float4 b1r = glv_load4<VM>(a.b1, e, E);
    float4 res = make_float4(0.f, 0.f, 0.f, 0.f), acc = res;
    float rb = 0.f, s = 0.f;
    int cur = -1, n_rows = 0;
    double loss = 0.0;

    // the row `cur` is complete as far as this run goes: to its output row, or to a carry record
    auto flush = [&](bool last) {
        const bool first = n_rows == 0;
        if (first || last) {
            const int64_t ci = 2 * run + (first ? 0 : 1);
            glv_store4<VM>(a.carry_row + (size_t)ci * E, e, E, acc);
            if (l == 0) {
                a.carry_id[ci] = cur;
                a.carry_s[ci] = s;
                if (first && last) a.carry_id[ci + 1] = -1;
            }
        } else {
            glv_store4<VM>(a.out + (size_t)cur * E, e, E, acc);
            if (l == 0) a.out_b[cur] = s;
        }
        ++n_rows;
    };

    for (int j = 0; j < n_e; j += 4) {
        int4 rc[4];
        float4 key[4];
        float kb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) rc[k] = rec[min(j + k, n_e - 1)];   // (past the run: the last cell again, unused)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            key[k] = glv_load4<VM>(kbase + (size_t)rc[k].y * E, e, E);
            kb[k] = kbias[rc[k].y];
        }
        float lt = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (j + k < n_e) {
                const int row = rc[k].x;
                if (row != cur) {
                    if (cur >= 0) flush(false);
                    cur = row;
                    res = glv_load4<VM>(rbase + (size_t)row * E, e, E);
                    if (SIDE == GLV_TGT) res = glv_add4(res, b1r);
                    rb = rbias[row];
                    acc = make_float4(0.f, 0.f, 0.f, 0.f);
                    s = 0.f;
                }
                const float4 kk = SIDE == GLV_CTX ? glv_add4(key[k], b1r) : key[k];
                const float d = glv_group_sum<EP / 4>(fmaf(res.w, kk.w, fmaf(res.z, kk.z, fmaf(res.y, kk.y, res.x * kk.x))));
                // z = (H_t . Eout[c] + b2[c]) + bt[t] on both sides
                const float z = SIDE == GLV_TGT ? __fadd_rn(__fadd_rn(d, kb[k]), rb) : __fadd_rn(__fadd_rn(d, rb), kb[k]);
                const float r = z - __int_as_float(rc[k].z);
                const float fr = __fmul_rn(__int_as_float(rc[k].w), r);
                const float g = __fmul_rn(fr, a.inv_n);
                acc.x = fmaf(g, kk.x, acc.x), acc.y = fmaf(g, kk.y, acc.y);
                acc.z = fmaf(g, kk.z, acc.z), acc.w = fmaf(g, kk.w, acc.w);
                s = __fadd_rn(s, g);
                if (SIDE == GLV_TGT) lt = __fadd_rn(lt, __fmul_rn(fr, r));
            }
        }
        loss += (double)lt;
    }
    flush(true);
    if (SIDE == GLV_TGT && l == 0) a.loss_part[run] = loss;
}

template <int EP, int SIDE>
__global__ __launch_bounds__(GLV_WG) void k_glv(const glv_args a) {
    constexpr int G = EP / 4, GW = 64 / G, WR = GW * GLV_RUN;   // lanes of a group, groups and cells of a wave
    __shared__ int4 recs[4 * WR];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t run0 = ((int64_t)blockIdx.x * 4 + w) * GW;
    const int64_t cell0 = run0 * GLV_RUN;
    int4 *wrec = recs + w * WR;
    for (int x = lane; x < WR; x += 64) {
        const int64_t i = cell0 + x;
        if (i < a.N) {
            const double c = (double)a.cnt[i];   // (> 0: the planes hold cells only)
            int4 r;
            r.x = a.rid[i];
            r.y = a.kid[i];
            r.z = __float_as_int((float)log(c));
            r.w = __float_as_int((float)fmin(1.0, pow(c / a.x_max, a.alpha)));
            wrec[x] = r;
        }
    }
    __syncthreads();
    const int gi = lane / G, l = lane % G;
    const int64_t run = run0 + gi;
    if (run >= a.nruns) return;
    const int64_t left = a.N - run * GLV_RUN;
    const int n_e = left < GLV_RUN ? (int)left : GLV_RUN;
    const int4 *rec = wrec + gi * GLV_RUN;
    if ((a.E & 3) == 0) glv_walk<EP, SIDE, 4>(a, rec, n_e, run, l);
    else if ((a.E & 1) == 0) glv_walk<EP, SIDE, 2>(a, rec, n_e, run, l);
    else glv_walk<EP, SIDE, 1>(a, rec, n_e, run, l);
}

// a wave per carry record: the first record of a row sums the row's records in record order
__global__ __launch_bounds__(256) void k_glv_carry(const int32_t *__restrict__ id, const float *__restrict__ cs,
                                                   const float *__restrict__ rows, int64_t n_rec, int E,
                                                   float *__restrict__ out, float *__restrict__ out_b) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_rec) return;
    const int row = id[i];
    if (row < 0) return;
    int64_t p = i - 1;
    while (p >= 0 && id[p] < 0) --p;
    if (p >= 0 && id[p] == row) return;
    constexpr int NX = BPE_SGM_MAX_EMBED / 64;
    float acc[NX], s = cs[i];
#pragma unroll
    for (int x = 0; x < NX; ++x) acc[x] = lane + 64 * x < E ? rows[(size_t)i * E + lane + 64 * x] : 0.f;
    for (int64_t j = i + 1; j < n_rec; ++j) {
        const int rj = id[j];
        if (rj < 0) continue;
        if (rj != row) break;
#pragma unroll
        for (int x = 0; x < NX; ++x)
            if (lane + 64 * x < E) acc[x] += rows[(size_t)j * E + lane + 64 * x];
        s += cs[j];
    }
#pragma unroll
    for (int x = 0; x < NX; ++x)
        if (lane + 64 * x < E) out[(size_t)row * E + lane + 64 * x] = acc[x];
    if (lane == 0) out_b[row] = s;
}

// out[b][e] = the sum of in[r][e] over the block's rows, in row order
__global__ __launch_bounds__(256) void k_glv_colsum(const float *__restrict__ in, int rows, int E, int rpb,
                                                    float *__restrict__ out) {
    const int e = threadIdx.x;
    if (e >= E) return;
    const int r1 = min(rows, ((int)blockIdx.x + 1) * rpb);
    float s = 0.f;
    for (int r = blockIdx.x * rpb; r < r1; ++r) s += in[(size_t)r * E + e];
    out[(size_t)blockIdx.x * E + e] = s;
}

// the loss from the runs' partials: a thread's slice in run order, the slices in order
__global__ __launch_bounds__(256) void k_glv_loss(const double *__restrict__ part, int64_t nruns, int64_t N,
                                                  unsigned long long *hdr) {
    __shared__ double sh[256];
    const int64_t per = (nruns + 255) / 256, r0 = threadIdx.x * per;
    double s = 0.0;
    for (int64_t i = r0; i < r0 + per && i < nruns; ++i) s += part[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 256; ++i) t += sh[i];
        hdr[SGMH_LOSS] = (unsigned long long)__double_as_longlong(t / (2.0 * (double)N));
    }
}

template <int EP>
void glv_launch(bpe_sgmodel *M, glv_args a, const int32_t *d_tT, const int32_t *d_cT, const int64_t *d_kT,
                float *colsum_part, hipEvent_t mid) {
    constexpr int RPB = 4 * (64 / (EP / 4));   // runs of a workgroup
    const unsigned grid = (unsigned)((a.nruns + RPB - 1) / RPB);
    const int64_t n_rec = 2 * a.nruns;
    const unsigned cgrid = (unsigned)((n_rec + 3) / 4);
    float *g = M->d_g;
    a.out = g + M->o_ein;
    a.out_b = M->d_gbt;
    k_glv<EP, GLV_TGT><<<grid, GLV_WG, 0, M->stream>>>(a);
    k_glv_carry<<<cgrid, 256, 0, M->stream>>>(a.carry_id, a.carry_s, a.carry_row, n_rec, a.E, a.out, a.out_b);
    const int nb = (a.V + GLV_COLROWS - 1) / GLV_COLROWS;
    k_glv_colsum<<<nb, 256, 0, M->stream>>>(a.out, a.V, a.E, GLV_COLROWS, nb == 1 ? g + M->o_b1 : colsum_part);
    if (nb > 1) k_glv_colsum<<<1, 256, 0, M->stream>>>(colsum_part, nb, a.E, nb, g + M->o_b1);
    k_glv_loss<<<1, 256, 0, M->stream>>>(a.loss_part, a.nruns, a.N, M->d_hdr);
    (void)hipEventRecord(mid, M->stream);
    a.rid = d_cT, a.kid = d_tT, a.cnt = d_kT;
    a.out = g + M->o_eout;
    a.out_b = g + M->o_b2;
    k_glv<EP, GLV_CTX><<<grid, GLV_WG, 0, M->stream>>>(a);
    k_glv_carry<<<cgrid, 256, 0, M->stream>>>(a.carry_id, a.carry_s, a.carry_row, n_rec, a.E, a.out, a.out_b);
}

// loss and gradients (into the model's gradient arrays) from device planes; *loss on the host
int glv_forward(bpe_sgmodel *M, const int32_t *d_t, const int32_t *d_c, const int64_t *d_k, int64_t U, double x_max,
                double alpha, double *loss) {
    bpe_sgmodel_glove_stats &st = M->gstats;
    st.calls++;
    char msg[128];
    if (U < 0 || (U && (!d_t || !d_c || !d_k))) return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model planes");
    if (!(x_max > 0 && std::isfinite(x_max))) {
        snprintf(msg, sizeof msg, "skip-gram model x_max %g is not positive or not finite", x_max);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    if (!(alpha >= 0 && std::isfinite(alpha))) {
        snprintf(msg, sizeof msg, "skip-gram model alpha %g is negative or not finite", alpha);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    SGM_TRY(hipSetDevice(M->device));
    int64_t P = 0;
    if (int rc = sgm_index(M, d_t, d_c, d_k, U, &P, &st.kernel_ms)) return rc;
    const int V = M->V, E = M->E;

    // the scratch, sized for N = U
    const int64_t n_chunks_u = (U + GLV_CHUNK - 1) / GLV_CHUNK, max_runs = (U + GLV_RUN - 1) / GLV_RUN;
    const int rpc = (V + SGN_MAX_CHUNKS - 1) / SGN_MAX_CHUNKS, n_chunks = (V + rpc - 1) / rpc;
    auto up = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t sizes[] = {up((size_t)n_chunks_u * 8), up((size_t)U * 8), up((size_t)U * 4), up((size_t)U * 4),
                            up((size_t)(V + 1) * 8), up((size_t)U * 8), up((size_t)U * 4), up((size_t)U * 4),
                            up((size_t)(V + 1) * 8), up((size_t)n_chunks * V * 4), up((size_t)V * 4),
                            up((size_t)max_runs * 8), up((size_t)max_runs * 8), up((size_t)max_runs * 8),
                            up((size_t)max_runs * 2 * E * 4), up((size_t)GLV_COLROWS * E * 4)};
    size_t total = 0;
    for (size_t b : sizes) total += b;
    if (int rc = sgm_grow(&M->d_gs, &M->gs_cap, (int64_t)total)) return rc;
    char *p = (char *)M->d_gs;
    auto take = [&](int i) { char *r = p; p += sizes[i]; return r; };
    int64_t *part = (int64_t *)take(0), *k2 = (int64_t *)take(1);
    int32_t *t2 = (int32_t *)take(2), *c2 = (int32_t *)take(3);
    int64_t *rowptr2 = (int64_t *)take(4), *kT = (int64_t *)take(5);
    int32_t *tT = (int32_t *)take(6), *cT = (int32_t *)take(7);
    int64_t *colptr = (int64_t *)take(8);
    int32_t *cc = (int32_t *)take(9), *tot = (int32_t *)take(10);
    double *loss_part = (double *)take(11);
    int32_t *carry_id = (int32_t *)take(12);
    float *carry_s = (float *)take(13), *carry_row = (float *)take(14), *colsum_part = (float *)take(15);

    unsigned long long h[SGMH_WORDS] = {SGM_NONE, (unsigned long long)P, 0, 0};
    SGM_TRY(hipEventRecord(M->nev[0], M->stream));
    SGM_TRY(hipMemsetAsync(M->d_g, 0, (size_t)M->n4 * 16, M->stream));
    SGM_TRY(hipMemsetAsync(M->d_gbt, 0, (size_t)M->bt4 * 16, M->stream));
    if (U) {
        k_glv_count<<<(unsigned)n_chunks_u, 256, 0, M->stream>>>(d_k, U, part, M->d_hdr);
        SGM_TRY(hipGetLastError());
        SGM_TRY(hipMemcpyAsync(h, M->d_hdr, sizeof h, hipMemcpyDeviceToHost, M->stream));
    }
    SGM_TRY(hipStreamSynchronize(M->stream));
    const int64_t N = U ? (int64_t)h[GLVH_N] : 0;
    st.elements += U;
    st.cells += N;
    if (loss) *loss = 0.0;
    if (N == 0) return BPE_OK;

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
    SGM_TRY(hipGetLastError());
    SGM_TRY(hipEventRecord(M->nev[1], M->stream));

    glv_args a = {};
    a.Ein = M->d_p + M->o_ein, a.b1 = M->d_p + M->o_b1, a.Eout = M->d_p + M->o_eout, a.b2 = M->d_p + M->o_b2;
    a.bt = M->d_bt;
    a.V = V, a.E = E;
    a.rid = d_t, a.kid = d_c, a.cnt = d_k;
    a.N = N, a.nruns = (N + GLV_RUN - 1) / GLV_RUN;
    a.x_max = x_max, a.alpha = alpha, a.inv_n = (float)(1.0 / (double)N);
    a.carry_id = carry_id, a.carry_s = carry_s, a.carry_row = carry_row, a.loss_part = loss_part;
    switch (M->EP) {
        case 64: glv_launch<64>(M, a, tT, cT, kT, colsum_part, M->nev[2]); break;
        case 128: glv_launch<128>(M, a, tT, cT, kT, colsum_part, M->nev[2]); break;
        default: glv_launch<256>(M, a, tT, cT, kT, colsum_part, M->nev[2]); break;
    }
    SGM_TRY(hipGetLastError());
    SGM_TRY(hipEventRecord(M->nev[3], M->stream));
    SGM_TRY(hipMemcpyAsync(h, M->d_hdr, sizeof h, hipMemcpyDeviceToHost, M->stream));
    SGM_TRY(hipStreamSynchronize(M->stream));
    float ms[3] = {0.f, 0.f, 0.f};
    for (int i = 0; i < 3; ++i) SGM_TRY(hipEventElapsedTime(&ms[i], M->nev[i], M->nev[i + 1]));
    st.runs += a.nruns;
    st.carry_records += 4 * a.nruns;
    st.transpose_ms += ms[0];
    st.target_ms += ms[1];
    st.context_ms += ms[2];
    st.kernel_ms += ms[0] + ms[1] + ms[2];
    if (loss) std::memcpy(loss, &h[SGMH_LOSS], 8);
    return BPE_OK;
}

// Adam over the flat array and over bt: one step counter, the same bias corrections
int glv_adam(bpe_sgmodel *M, double lr, double beta1, double beta2, double eps) {
    M->step++;
    const double c1 = 1.0 / (1.0 - std::pow(beta1, (double)M->step));
    const double c2 = 1.0 / (1.0 - std::pow(beta2, (double)M->step));
    SGM_TRY(hipEventRecord(M->ev0, M->stream));
    k_sgm_adam<<<(unsigned)((M->n4 + 255) / 256), 256, 0, M->stream>>>((float4 *)M->d_p, (const float4 *)M->d_g,
                                                                      (float4 *)M->d_m, (float4 *)M->d_v, M->n4, lr, beta1,
                                                                      beta2, eps, c1, c2);
    k_sgm_adam<<<(unsigned)((M->bt4 + 255) / 256), 256, 0, M->stream>>>((float4 *)M->d_bt, (const float4 *)M->d_gbt,
                                                                       (float4 *)M->d_mbt, (float4 *)M->d_vbt, M->bt4, lr,
                                                                       beta1, beta2, eps, c1, c2);
    SGM_TRY(hipGetLastError());
    SGM_TRY(hipEventRecord(M->ev1, M->stream));
    SGM_TRY(hipStreamSynchronize(M->stream));
    return sgm_time(M, &M->gstats.kernel_ms);
}

// the five gradient arrays to the caller's (NULL ones are skipped)
int glv_copy_out(bpe_sgmodel *M, float *dEin, float *db1, float *dEout, float *db2, float *dbt, hipMemcpyKind kind) {
    if (dbt) SGM_TRY(hipMemcpyAsync(dbt, M->d_gbt, (size_t)M->V * 4, kind, M->stream));
    return sgm_copy_sections(M, M->d_g, dEin, db1, dEout, db2, false, kind);
}

int glv_target_bias(bpe_sgmodel *M, float *bt, int64_t dim, bool set, bool dev) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (dim != M->V) {
        char msg[128];
        snprintf(msg, sizeof msg, "skip-gram model target bias of %lld given to a model of %d", (long long)dim, M->V);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    if (!bt) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model target bias");
    SGM_TRY(hipSetDevice(M->device));
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : set ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    if (set) SGM_TRY(hipMemcpyAsync(M->d_bt, bt, (size_t)M->V * 4, kind, M->stream));
    else SGM_TRY(hipMemcpyAsync(bt, M->d_bt, (size_t)M->V * 4, kind, M->stream));
    SGM_TRY(hipStreamSynchronize(M->stream));
    return BPE_OK;
}

bool glv_betas_ok(double beta1, double beta2) { return beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1; }

}  // namespace

extern "C" {

int bpe_sgmodel_glove_loss_grad_device(bpe_sgmodel *M, const int32_t *d_targets, const int32_t *d_contexts,
                                       const int64_t *d_counts, int64_t U, double x_max, double alpha, double *loss,
                                       float *d_dEin, float *d_db1, float *d_dEout, float *d_db2, float *d_dbt) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (int rc = glv_forward(M, d_targets, d_contexts, d_counts, U, x_max, alpha, loss)) return rc;
    return glv_copy_out(M, d_dEin, d_db1, d_dEout, d_db2, d_dbt, hipMemcpyDeviceToDevice);
}

int bpe_sgmodel_glove_loss_grad(bpe_sgmodel *M, const int32_t *targets, const int32_t *contexts, const int64_t *counts,
                                int64_t U, double x_max, double alpha, double *loss, float *dEin, float *db1,
                                float *dEout, float *db2, float *dbt) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (U > 0 && (!targets || !contexts || !counts))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model planes");
    const int32_t *d_t, *d_c;
    const int64_t *d_k;
    if (int rc = sgm_stage(M, targets, contexts, counts, U, &d_t, &d_c, &d_k)) return rc;
    if (int rc = glv_forward(M, d_t, d_c, d_k, U, x_max, alpha, loss)) return rc;
    return glv_copy_out(M, dEin, db1, dEout, db2, dbt, hipMemcpyDeviceToHost);
}

int bpe_sgmodel_glove_adam_step_device(bpe_sgmodel *M, const int32_t *d_targets, const int32_t *d_contexts,
                                       const int64_t *d_counts, int64_t U, double x_max, double alpha, double lr,
                                       double beta1, double beta2, double eps, double *loss) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (!glv_betas_ok(beta1, beta2)) return bpe_fail(BPE_ERR_ARG, "bpe native: skip-gram model betas outside [0, 1)");
    if (int rc = glv_forward(M, d_targets, d_contexts, d_counts, U, x_max, alpha, loss)) return rc;
    return glv_adam(M, lr, beta1, beta2, eps);
}

int bpe_sgmodel_glove_adam_step(bpe_sgmodel *M, const int32_t *targets, const int32_t *contexts, const int64_t *counts,
                                int64_t U, double x_max, double alpha, double lr, double beta1, double beta2, double eps,
                                double *loss) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null skip-gram model");
    if (U > 0 && (!targets || !contexts || !counts))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad skip-gram model planes");
    const int32_t *d_t, *d_c;
    const int64_t *d_k;
    if (int rc = sgm_stage(M, targets, contexts, counts, U, &d_t, &d_c, &d_k)) return rc;
    return bpe_sgmodel_glove_adam_step_device(M, d_t, d_c, d_k, U, x_max, alpha, lr, beta1, beta2, eps, loss);
}

int bpe_sgmodel_set_target_bias(bpe_sgmodel *M, const float *bt, int64_t dim) {
    return glv_target_bias(M, (float *)bt, dim, true, false);
}

int bpe_sgmodel_set_target_bias_device(bpe_sgmodel *M, const float *d_bt, int64_t dim) {
    return glv_target_bias(M, (float *)d_bt, dim, true, true);
}

int bpe_sgmodel_get_target_bias(bpe_sgmodel *M, float *bt, int64_t dim) { return glv_target_bias(M, bt, dim, false, false); }

int bpe_sgmodel_get_target_bias_device(bpe_sgmodel *M, float *d_bt, int64_t dim) {
    return glv_target_bias(M, d_bt, dim, false, true);
}

int bpe_sgmodel_get_glove_stats(bpe_sgmodel *M, bpe_sgmodel_glove_stats *out) {
    if (!M || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = M->gstats;
    return BPE_OK;
}

int bpe_sgmodel_reset_glove_stats(bpe_sgmodel *M) {
    if (!M) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    M->gstats = {};
    return BPE_OK;
}

}  // extern "C"
