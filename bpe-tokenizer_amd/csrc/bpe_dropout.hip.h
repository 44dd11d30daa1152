// bpe_dropout.hip.h — BPE-dropout (Provilkov et al. 2020) on the device: S sampled segmentations of
// every text of a batch (bpe_encode_dropout_batch and the text forms, include/bpe.h).
// Included by bpe_encode.hip, whose lookup, scan, minimum, cut and pack kernels it shares.
//
// The rule (csrc/bpe_dropout_rule.h) is encodeToCode's M scans with one change: a site whose coin
// falls below the threshold is left alone.  Under a list the greedy can take it equals the
// rank-greedy form of k_encode with every dropped site's rank word stored as NO_RANK at the moment
// it is looked up: the word then never wins the minimum, and it never enters the parity chain of an
// x == x run, which is then the run of consecutive kept sites, as the sequential scan has it.  A
// site (i, r) is looked up at most once while its two tokens stand, and its coin depends on (i, r)
// alone, so the stored word is the coin the scan of merge r would draw there.
//
// k_encode_drop: one workgroup per (segment, sample), the S samples of a segment side by side in
// the grid so that they read the same input from L2.  LDS per token: one u32 word start << 16 | id
// (start: where the token begins in the segment before any merge) and one u32 rank word, 8 B.  Id
// and start share a word so that they move together on compaction with one store, and the word
// plane has the rank plane's banking under the odd segment stride.  The stream key, the segment's
// base in its text and the threshold are uniform (scalar registers).
#pragma once

#include "bpe_dropout_rule.h"

namespace {

struct DropSeg {
    long long base;    // position of the segment's first token in its text
    long long res0;    // result index of its sample 0; sample s is res0 + s * stride
    int32_t text;      // its text's index in the call
    int32_t stride;    // segments of its text
};

struct DropKey {
    unsigned long long seed, thr;
    long long text_base;
    int32_t S;
};

constexpr size_t drop_lds(int i) { return (size_t)shape_cap(i) * 8; }
static_assert(drop_lds(N_SHAPES - 1) + 256 <= LDS_BYTES, "the largest shape fits an LDS allocation");

// which[b / S] is the segment, b % S the sample; res_off[res] is where the result goes in `out`,
// out_len[res] its length.  A segment that does not fit the shape (the host never lists one) is
// counted in *err and left empty.
template <int WG, int KMAX, bool TAB_LDS>
__global__ void __launch_bounds__(WG)
k_encode_drop(const int32_t *__restrict__ in, const int64_t *__restrict__ off, const int32_t *__restrict__ which,
              const DropSeg *__restrict__ seg, const int64_t *__restrict__ res_off, int32_t *__restrict__ out,
              int32_t *__restrict__ out_len, RankTab t, LdsTab lt, DropKey dk,
              unsigned long long *__restrict__ steps_total, unsigned long long *__restrict__ err) {
    static_assert(KMAX & 1, "odd segment lengths");
    constexpr int CAP = WG * (KMAX - 1);
    constexpr int H = KMAX + 2;   // segment + look-ahead
    extern __shared__ uint32_t lds32[];
    __shared__ uint32_t red[WG / 64];
    __shared__ int scn[WG / 64];
    uint32_t *rk = lds32;
    uint32_t *tp = lds32 + CAP;   // start << 16 | id
    const int tid = threadIdx.x;
    const int sample = (int)(blockIdx.x % (unsigned)dk.S);
    const int g = which[blockIdx.x / (unsigned)dk.S];
    const DropSeg sg = seg[g];
    const int64_t base = off[g];
    const int64_t n64 = off[g + 1] - base;
    const int64_t res = sg.res0 + (int64_t)sample * sg.stride;
    if (n64 < 0 || n64 > CAP) {   // (uniform)
        if (tid == 0) {
            atomicAdd(err, 1ull);
            out_len[res] = 0;
        }
        return;
    }
    int n = (int)n64;
    const int64_t obase = res_off[res];
    const uint64_t stream = drop_stream(dk.seed, (uint64_t)(dk.text_base + sg.text), (uint64_t)sample, (uint64_t)dk.S);
    const uint64_t seg_base = (uint64_t)sg.base, thr = dk.thr;

    Lookup<TAB_LDS> look;
    look.g = t;
    if constexpr (TAB_LDS) {
        uint32_t *tw = lds32 + 2 * CAP;
        const uint32_t w4 = lt.words & ~3u;
        for (uint32_t w = 4 * tid; w < w4; w += 4 * WG)
            *reinterpret_cast<uint4 *>(tw + w) = *reinterpret_cast<const uint4 *>(lt.img + w);
        for (uint32_t w = w4 + tid; w < lt.words; w += WG) tw[w] = lt.img[w];
        look.keys = tw;
        look.cs = reinterpret_cast<const uint16_t *>(tw + lt.m);
        look.slot = tw + lt.m + ((lt.m + 1) >> 1);
        look.mask = lt.mask;
        look.shift = lt.shift;
    }
    // the rank word of the pair `key` whose left token starts at `start`: the coin is drawn here
    auto coined = [&](uint32_t key, uint32_t start) -> uint32_t {
        const uint32_t rv = look(key);
        if (rv != NO_RANK && drop_dropped(stream, seg_base + start, rv >> 16, thr)) return NO_RANK;
        return rv;
    };

    bool bad = false;
    for (int i = tid; i < n; i += WG) {
        const int32_t v = in[base + i];
        bad |= (uint32_t)v >= (uint32_t)BPE_MAX_VOCAB;
        tp[i] = ((uint32_t)i << 16) | (uint16_t)v;
    }
    if (bad) atomicAdd(err, 1ull);
    __syncthreads();
    uint32_t lmin = NO_RANK;
    for (int i = tid; i < n; i += WG) {
        const uint32_t r = i + 1 < n ? coined((tp[i] << 16) | (tp[i + 1] & 0xFFFFu), (uint32_t)i) : NO_RANK;
        rk[i] = r;
        lmin = min(lmin, r);
    }
    uint32_t r = block_min<WG>(lmin, red);
    __syncthreads();
    int steps = 0;

    // k_encode's step, with the word plane in place of its id plane
    while (r != NO_RANK) {   // (uniform)
        ++steps;
        const uint32_t c = r & 0xFFFFu;
        const int k = max(3, (n + WG - 1) / WG) | 1;   // (odd: a bank per lane; <= KMAX)
        const int s = tid * k;
        const int len = max(0, min(k, n - s));
        uint32_t T[H], R[H];
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const bool in_seg = j < k + 2 && s + j < n;
            T[j] = in_seg ? tp[s + j] : 0u;
            R[j] = in_seg ? rk[s + j] : NO_RANK;
        }
        const uint32_t rb = (len > 0 && s > 0) ? rk[s - 1] : NO_RANK;
        // chain parity at the segment start: d = kept r-sites right before s (a dropped one, being
        // NO_RANK, ends the chain)
        int d = 0;
        bool fprev = false;
        if (rb == r) {
            for (int j = s - 1; j >= 0 && rk[j] == r; --j) ++d;
            fprev = !((d - 1) & 1);
        }
        uint32_t F = 0;
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
        const uint32_t live = ~((F << 1) | (fprev ? 1u : 0u)) & ((1u << len) - 1u);
        int p = p0;
        lmin = NO_RANK;
        uint32_t K[KMAX];
        uint32_t req = 0;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            K[j] = 0;
            if ((live >> j) & 1) {
                const bool fi = (F >> j) & 1;
                const uint32_t tv = fi ? c : (T[j] & 0xFFFFu);
                const int nx = fi ? j + 2 : j + 1;
                uint32_t rv = NO_RANK;
                if (s + nx < n) {
                    const bool fn = (F >> nx) & 1;
                    const uint32_t tn = (fi ? T[j + 2] : T[j + 1]) & 0xFFFFu;
                    if (fi || fn) {
                        K[j] = (tv << 16) | (fn ? c : tn);
                        req |= 1u << j;
                    }
                    rv = R[j];
                }
                tp[p] = (T[j] & 0xFFFF0000u) | tv;   // (a counted site keeps its left token's start)
                if (!((req >> j) & 1)) {
                    rk[p] = rv;
                    lmin = min(lmin, rv);
                }
                ++p;
            }
        }
        // the pairs that now touch c: their rank words and their coins, one request per lane per round
        while (__ballot(req != 0)) {
            if (req) {
                const int j = __builtin_ctz(req);
                uint32_t key = 0, start = 0;
#pragma unroll
                for (int jj = 0; jj < KMAX; ++jj)
                    if (jj == j) {
                        key = K[jj];
                        start = T[jj] >> 16;
                    }
                const int pp = p0 + __builtin_popcount(live & ((1u << j) - 1u));
                const uint32_t rv = coined(key, start);
                rk[pp] = rv;
                lmin = min(lmin, rv);
                req &= req - 1;
            }
        }
        n -= total;
        r = block_min<WG>(lmin, red);   // (barrier: the rewritten text visible)
        __syncthreads();
    }

    for (int i = tid; i < n; i += WG) out[obase + i] = (int32_t)(tp[i] & 0xFFFFu);
    if (tid == 0) {
        out_len[res] = n;
        if (steps) atomicAdd(steps_total, (unsigned long long)steps);
    }
}

template <int I, bool TAB_LDS>
hipError_t drop_set_attr() {
    return hipFuncSetAttribute((const void *)k_encode_drop<SHAPE_WG[I], SHAPE_K[I], TAB_LDS>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)(TAB_LDS ? LDS_BYTES : drop_lds(I)));
}

template <int I = 0>
hipError_t drop_set_attrs() {
    hipError_t e = drop_set_attr<I, true>();
    if (e == hipSuccess) e = drop_set_attr<I, false>();
    if constexpr (I + 1 < N_SHAPES) {
        if (e == hipSuccess) e = drop_set_attrs<I + 1>();
    }
    return e;
}

// The device regions of a call of n_texts texts in at most n_max segments, `total` ids in, S
// samples: the results' stage R (Stage's layout over the n_max * S results: R.off is where each
// result lies in R.out, R.ids receives the packed values), then
//     [seg_off (n_max + 2) | which | seg | res_of (n_texts * S + 1)]
// mirrored in pinned memory behind [ooff | res_off].
struct DropStage {
    Stage R;
    size_t b_soff, b_which, b_seg, b_resof;
    int64_t *seg_off = nullptr, *res_of = nullptr;
    int32_t *which = nullptr;
    DropSeg *seg = nullptr;
    DropStage(int64_t n_max, int64_t n_texts, int64_t total, int64_t S)
        : R(n_max * S, total * S), b_soff(align16((size_t)(n_max + 2) * 8)), b_which(align16((size_t)n_max * 4)),
          b_seg(align16((size_t)n_max * sizeof(DropSeg))), b_resof(align16((size_t)(n_texts * S + 1) * 8)) {}
    size_t lists_bytes() const { return b_soff + b_which + b_seg + b_resof; }
    size_t bytes() const { return R.bytes() + lists_bytes(); }
    size_t host_bytes() const { return 2 * R.b_off + lists_bytes(); }
    char *place(char *d, int64_t n_res) {
        d = R.place(d, n_res);
        seg_off = reinterpret_cast<int64_t *>(d);
        which = reinterpret_cast<int32_t *>(d += b_soff);
        seg = reinterpret_cast<DropSeg *>(d += b_which);
        res_of = reinterpret_cast<int64_t *>(d += b_seg);
        return d + b_resof;
    }
};

template <int I>
void drop_launch_one(bpe_encoder *E, unsigned n_wg, bool tab_lds, const int32_t *ids, const DropStage &D,
                     const int32_t *which, const DropKey &dk) {
    constexpr int WG = SHAPE_WG[I], KM = SHAPE_K[I];
    const RankTab t{E->d_slots, (1u << E->bits) - 1, 32 - E->bits};
    if (tab_lds)
        k_encode_drop<WG, KM, true><<<n_wg, WG, drop_lds(I) + (size_t)E->lt.words * 4, E->stream>>>(
            ids, D.seg_off, which, D.seg, D.R.off, D.R.out, D.R.len, t, E->lt, dk, E->d_drop_steps, D.R.err);
    else
        k_encode_drop<WG, KM, false><<<n_wg, WG, drop_lds(I), E->stream>>>(
            ids, D.seg_off, which, D.seg, D.R.off, D.R.out, D.R.len, t, E->lt, dk, E->d_drop_steps, D.R.err);
}

template <int I = 0>
void drop_launch_shape(int i, bpe_encoder *E, unsigned n_wg, bool tab_lds, const int32_t *ids, const DropStage &D,
                       const int32_t *which, const DropKey &dk) {
    if (i == I) return drop_launch_one<I>(E, n_wg, tab_lds, ids, D, which, dk);
    if constexpr (I + 1 < N_SHAPES) drop_launch_shape<I + 1>(i, E, n_wg, tab_lds, ids, D, which, dk);
}

int drop_no_form(int64_t k, const char *why) {
    char msg[200];
    std::snprintf(msg, sizeof msg, "bpe native: no dropout form for text %lld: %s", (long long)k, why);
    return bpe_fail(BPE_ERR_STATE, msg);
}

// what a merge list needs (checked before any work; text 0 is the first text of any call)
int drop_check_list(const bpe_encoder *E) {
    if (!E->greedy_ok) return drop_no_form(0, "the merge list is not one the rank-greedy form takes");
    if (E->pair_twice) return drop_no_form(0, "the merge list holds a pair twice");
    return BPE_OK;
}

int drop_check_args(int32_t samples, double p, int64_t text_base, uint64_t seed, DropKey &dk) {
    unsigned long long thr = 0;
    uint64_t t64 = 0;
    if (samples < 1 || text_base < 0 || !drop_threshold(p, &t64))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad dropout arguments (samples >= 1, 0 <= p <= 1, text_base >= 0)");
    thr = t64;
    dk = DropKey{seed, thr, text_base, samples};
    return BPE_OK;
}

int drop_init(bpe_encoder *E) {
    if (E->d_drop_steps) return BPE_OK;
    if (drop_set_attrs() != hipSuccess) return bpe_fail(BPE_ERR_HIP, "bpe native: dropout LDS attribute");
    ENC_TRY(hipMalloc((void **)&E->d_drop_steps, 8));
    ENC_TRY(hipMemset(E->d_drop_steps, 0, 8));
    return BPE_OK;
}

// sizes of a call by its texts' lengths (an upper bound will do): the most segments, and that the
// results can be indexed
int drop_sizes(const int64_t *off, int64_t n, int64_t total, int64_t S, int64_t *n_max) {
    *n_max = max_segments(off, n);
    if (*n_max >= 0x7FFFFFFF / S || total > (int64_t(1) << 40) / S)
        return bpe_fail(BPE_ERR_ARG, "bpe native: dropout batch too large");
    return BPE_OK;
}

// What a finished run leaves: on the device the packed values in D.R.ids, on the host (pinned) the
// results' packed offsets and where each lies in D.R.out; the plan; result res_of(k, s) is sample s
// of text k.
struct DropDone {
    SplitPlan P;
    int64_t n_res = 0, S = 1;
    const int64_t *h_ooff = nullptr, *h_res_off = nullptr, *h_res_of = nullptr;
    int64_t res_of(int64_t k, int64_t s) const {
        const int64_t g0 = P.seg_of[(size_t)k];
        return g0 * S + s * (P.seg_of[(size_t)k + 1] - g0);
    }
    bool split(int64_t n_texts) const { return P.n_seg() != n_texts; }
};

// n texts whose ids lie back to back on the device at d_ids, text k at [idoff[k], idoff[k + 1])
// (idoff on the host, idoff[0] == 0), placed stage D, pinned mirror at E->h_buf: the plan, the
// lists, k_encode_drop over every (segment, sample), the pack through `vec` or as ids, and the
// packed offsets back.  Waits for the stream.  A text with no dropout form fails the call here.
int drop_run(bpe_encoder *E, const DropKey &dk, DropStage &D, const int32_t *d_ids, const int64_t *idoff, int64_t n,
             const VecMap *vec, int bad_rc, const char *bad_msg, DropDone &O) {
    const int64_t S = dk.S, total = idoff[n];
    hipStream_t s = E->stream;
    int rc;
    SplitPlan &P = O.P;
    int64_t first_long = -1;
    for (int64_t k = 0; k < n && first_long < 0; ++k)
        if (idoff[k + 1] - idoff[k] > CAP_MAX) first_long = k;
    if (first_long >= 0) {
        if (!split_route(E))
            return drop_no_form(first_long, "longer than BPE_ENCODE_LDS_TOKENS tokens on the replay route "
                                            "(bpe_encoder_set_long_texts)");
        if ((rc = plan_split(E, d_ids, idoff, n, P))) return rc;
        if (!P.fallback.empty())
            return drop_no_form(P.fallback[0], "no safe boundary within BPE_ENCODE_LDS_TOKENS tokens");
        split_commit(E, P);
    } else {
        P.seg_off.assign(idoff, idoff + n + 1);
        P.seg_of.resize((size_t)n + 1);
        for (int64_t k = 0; k <= n; ++k) P.seg_of[(size_t)k] = k;
    }
    const int64_t n_seg = P.n_seg(), n_res = n_seg * S;
    O.n_res = n_res, O.S = S;
    D.place(E->d_buf, n_res);   // (the err word follows the results' offsets)
    char *h = E->h_buf;
    int64_t *h_ooff = reinterpret_cast<int64_t *>(h);
    int64_t *h_res_off = reinterpret_cast<int64_t *>(h += D.R.b_off);
    int64_t *h_soff = reinterpret_cast<int64_t *>(h += D.R.b_off);
    int32_t *h_which = reinterpret_cast<int32_t *>(h += D.b_soff);
    DropSeg *h_seg = reinterpret_cast<DropSeg *>(h += D.b_which);
    int64_t *h_res_of = reinterpret_cast<int64_t *>(h += D.b_seg);
    O.h_ooff = h_ooff, O.h_res_off = h_res_off, O.h_res_of = h_res_of;
    std::memcpy(h_soff, P.seg_off.data(), (size_t)(n_seg + 1) * 8);
    // results in order of text, then sample, then segment: text k's S samples lie back to back in
    // R.out, each laid out like the text
    for (int64_t k = 0; k < n; ++k) {
        const int64_t g0 = P.seg_of[(size_t)k], ns = P.seg_of[(size_t)k + 1] - g0, t0 = idoff[k], l = idoff[k + 1] - t0;
        for (int64_t g = g0; g < g0 + ns; ++g)
            h_seg[g] = DropSeg{(long long)(h_soff[g] - t0), (long long)(g0 * S + (g - g0)), (int32_t)k, (int32_t)ns};
        for (int64_t sm = 0; sm < S; ++sm) {
            h_res_of[k * S + sm] = g0 * S + sm * ns;
            for (int64_t g = g0; g < g0 + ns; ++g) h_res_off[g0 * S + sm * ns + (g - g0)] = S * t0 + sm * l + (h_soff[g] - t0);
        }
    }
    h_res_of[n * S] = n_res;
    h_res_off[n_res] = S * total;
    h_res_off[n_res + 1] = 0;   // (the err word)
    ShapeLists lists;
    std::vector<int64_t> none;
    classify(E, h_soff, n_seg, lists, none);
    if (!none.empty()) return bpe_fail(BPE_ERR_STATE, "bpe native: split plan mismatch");
    fill_which(lists, h_which);
    ENC_TRY(hipMemcpyAsync(D.R.off, h_res_off, (size_t)(n_res + 2) * 8, hipMemcpyHostToDevice, s));
    ENC_TRY(hipMemcpyAsync(D.seg_off, h_soff, D.lists_bytes(), hipMemcpyHostToDevice, s));
    // a call of few workgroups gives each a CU to itself: the table in LDS where it fits beside the text
    const size_t tab = (size_t)E->lt.words * 4;
    const bool few = (size_t)(lists.n * S) <= LATENCY_TEXTS;
    ENC_TRY(hipEventRecord(E->ev0, s));
    size_t at = 0;
    for (int i = 0; i < N_SHAPES; ++i) {
        if (lists.of[i].empty()) continue;
        const bool tab_lds = few && shape_cap(i) > LDS_TAB_MIN_TOKENS && drop_lds(i) + tab <= LDS_BYTES;
        drop_launch_shape(i, E, (unsigned)(lists.of[i].size() * (size_t)S), tab_lds, d_ids, D, D.which + at, dk);
        at += lists.of[i].size();
    }
    ENC_TRY(hipGetLastError());
    ENC_TRY(hipEventRecord(E->ev1, s));
    if ((rc = vec ? pack(s, D.R, n_res, S * total, *vec) : pack(s, D.R, n_res, S * total, MapId{}))) return rc;
    const int bad = fetch_ooff(s, D.R, h_ooff, n_res, 0, bad_rc, bad_msg);
    float ms = 0;
    ENC_TRY(hipEventElapsedTime(&ms, E->ev0, E->ev1));
    E->dst.kernel_ms += ms;
    return bad;
}

void drop_count(bpe_encoder *E, int64_t n_texts, int64_t S, int64_t tokens_in, int64_t n_out) {
    E->dst.texts += n_texts;
    E->dst.samples += n_texts * S;
    E->dst.tokens_in += tokens_in;
    E->dst.tokens_out += n_out;
}

// ---- the id form (bpe_encode_dropout_batch) --------------------------------------------------------

int drop_ids(bpe_encoder *E, const int32_t *ids, const int64_t *off, int64_t n_texts, const DropKey &dk,
             int32_t *ids_out, int64_t *out_off) {
    const int64_t S = dk.S;
    if (n_texts < 0 || !out_off || (n_texts && !off))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad encode_dropout_batch arguments");
    for (int64_t k = 0; k < n_texts; ++k)
        if (off[k + 1] < off[k]) return bpe_fail(BPE_ERR_ARG, "bpe native: text offsets must not decrease");
    const int64_t base = n_texts ? off[0] : 0, total = n_texts ? off[n_texts] - base : 0;
    if (total && (!ids || !ids_out)) return bpe_fail(BPE_ERR_ARG, "bpe native: null id buffer");
    ENC_TRY(hipSetDevice(E->device));
    E->dst.calls++;
    if (n_texts == 0) {
        out_off[0] = 0;
        return BPE_OK;
    }
    int rc;
    int64_t n_max = 0;
    if ((rc = drop_check_list(E)) || (rc = drop_sizes(off, n_texts, total, S, &n_max)) || (rc = drop_init(E)) ||
        (rc = upload_table(E)))
        return rc;
    DropStage D(n_max, n_texts, total, S);
    const size_t b_in = align16((size_t)std::max<int64_t>(total, 1) * 4);
    if ((rc = grow_stage(E, D.host_bytes(), D.bytes() + b_in))) return rc;
    Release release{E};
    int32_t *d_ids = reinterpret_cast<int32_t *>(D.place(E->d_buf, n_max * S));
    if (total) ENC_TRY(hipMemcpyAsync(d_ids, ids + base, (size_t)total * 4, hipMemcpyHostToDevice, E->stream));
    std::vector<int64_t> idoff((size_t)n_texts + 1);
    for (int64_t k = 0; k <= n_texts; ++k) idoff[(size_t)k] = off[k] - base;
    DropDone O;
    int64_t n_out = 0;
    if ((rc = drop_run(E, dk, D, d_ids, idoff.data(), n_texts, nullptr, BPE_ERR_VOCAB, BAD_ID, O)) ||
        (rc = packed_length(O.h_ooff, O.n_res, S * total, -1, &n_out)) ||
        (rc = copy_packed(E->stream, ids_out, D.R.ids, n_out, hipMemcpyDeviceToHost)))
        return rc;
    for (int64_t j = 0; j <= n_texts * S; ++j) out_off[j] = O.h_ooff[O.h_res_of[j]];
    drop_count(E, n_texts, S, total, n_out);
    return BPE_OK;
}

// ---- the text forms (bpe_encode_dropout_text_batch and its device form) ----------------------------
// text_run's front end, checks and messages in their order; then the run above on the ids it made.

int drop_text(bpe_encoder *E, int kind, const uint16_t *units, const int64_t *off, int64_t n_texts, const DropKey &dk,
              int32_t *vals_out, int64_t cap, int64_t *out_off, bool dev, int64_t *needed) {
    bpe_text_state &T = E->txt;
    const int64_t S = dk.S;
    *needed = 0;
    int rc = text_check_call(E, kind, n_texts, off, !(cap < 0 || !out_off || (cap && !vals_out)));
    if (rc) return rc;
    ENC_TRY(hipSetDevice(E->device));
    hipStream_t s = E->stream;
    E->dst.calls++;
    std::vector<int64_t> off_copy;
    const int64_t *h_off = off;
    if (dev && n_texts) {
        off_copy.resize((size_t)n_texts + 1);
        ENC_TRY(hipMemcpyAsync(off_copy.data(), off, off_copy.size() * 8, hipMemcpyDeviceToHost, s));
        ENC_TRY(hipStreamSynchronize(s));
        h_off = off_copy.data();
    }
    if ((rc = text_check_offsets(h_off, n_texts))) return rc;
    const int64_t base = n_texts ? h_off[0] : 0, total = n_texts ? h_off[n_texts] - base : 0;
    if (total && !units) return bpe_fail(BPE_ERR_ARG, "bpe native: null unit buffer");
    if (total && !T.has_chars)
        return bpe_fail(BPE_ERR_STATE, "bpe native: encode of text without a char table (bpe_encoder_set_chars)");
    if (n_texts && (rc = drop_check_list(E))) return rc;
    if (total == 0) {   // (no text, or every text empty)
        if (dev) {
            ENC_TRY(hipMemsetAsync(out_off, 0, (size_t)(n_texts * S + 1) * 8, s));
            ENC_TRY(hipStreamSynchronize(s));
        } else {
            std::memset(out_off, 0, (size_t)(n_texts * S + 1) * 8);
        }
        drop_count(E, n_texts, S, 0, 0);
        return BPE_OK;
    }
    int64_t n_max = 0;
    if ((rc = drop_sizes(h_off, n_texts, total, S, &n_max)) || (rc = drop_init(E)) || (rc = text_upload(E)) ||
        (rc = upload_table(E)))
        return rc;
    const int mis = dev ? (int)(((uintptr_t)(units + base) >> 1) & (TXT_RUN - 1)) : 0;
    const int64_t n_tiles = (total + mis + TXT_TILE - 1) / TXT_TILE;
    if (n_tiles > 0x7FFFFFFF) return bpe_fail(BPE_ERR_ARG, "bpe native: text batch too large");
    // device: the dropout stage, then the front end's
    //   [ids | id offsets | tile counts, then bases | first text of each tile | tile marks | units | off]
    DropStage D(n_max, n_texts, total, S);
    const size_t b_ids = align16((size_t)total * 4), b_idoff = align16((size_t)(n_texts + 2) * 8);
    const size_t b_tiles = align16((size_t)n_tiles * 8), b_edge = align16((size_t)n_tiles * 4);
    const size_t b_units = dev ? 0 : align16((size_t)total * 2), b_uoff = dev ? 0 : b_idoff;
    if ((rc = grow_stage(E, D.host_bytes(), D.bytes() + b_ids + b_idoff + 2 * b_tiles + b_edge + b_units + b_uoff)))
        return rc;
    Release release{E};
    char *d = D.place(E->d_buf, n_max * S);
    int32_t *d_ids = reinterpret_cast<int32_t *>(d);
    int64_t *d_idoff = reinterpret_cast<int64_t *>(d += b_ids);
    unsigned long long *d_tiles = reinterpret_cast<unsigned long long *>(d += b_idoff);
    long long *d_first = reinterpret_cast<long long *>(d += b_tiles);
    uint32_t *d_edge = reinterpret_cast<uint32_t *>(d += b_tiles);
    uint16_t *d_units = reinterpret_cast<uint16_t *>(d += b_edge);
    int64_t *d_uoff = reinterpret_cast<int64_t *>(d += b_units);
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
    ENC_TRY(hipMemsetAsync(d_first, 0xFF, (size_t)n_tiles * 8, s));
    ENC_TRY(hipMemsetAsync(d_edge, 0, (size_t)n_tiles * 4, s));
    const CharTab ct{T.d_bmp, T.d_pairs, (1u << T.pair_bits) - 1, 32 - T.pair_bits};
    k_txt_count<<<(unsigned)((n_tiles + TXT_CNT_TILES - 1) / TXT_CNT_TILES), TXT_WG, 0, s>>>(units_al, mis, total,
                                                                                          n_tiles, d_tiles);
    k_txt_texts<<<(unsigned)std::min<int64_t>((n_texts + 256) / 256, 2048), 256, 0, s>>>(
        units_al, mis, total, k_off, n_texts, base, n_tiles, d_first, d_edge, d_tiles);
    k_txt_scan<<<1, 1024, 0, s>>>(d_tiles, n_tiles, T.d_st);
    k_txt_map<<<(unsigned)n_tiles, TXT_WG, 0, s>>>(units_al, mis, total, ct, d_tiles, d_first, d_edge, k_off, n_texts,
                                                  base, d_ids, d_idoff, T.d_st);
    ENC_TRY(hipGetLastError());
    // the texts' id offsets and the front end's status back (8 B per text): the plan and the lists
    // are made from the char counts
    std::vector<int64_t> idoff((size_t)n_texts + 1);
    ENC_TRY(hipMemcpyAsync(idoff.data(), d_idoff, idoff.size() * 8, hipMemcpyDeviceToHost, s));
    ENC_TRY(hipMemcpyAsync(T.h_st, T.d_st, TS_WORDS * 8, hipMemcpyDeviceToHost, s));
    ENC_TRY(hipStreamSynchronize(s));
    const int64_t n_ids = (int64_t)T.h_st[TS_CHARS];
    if (idoff[0] != 0 || n_ids < 0 || n_ids > total || idoff[(size_t)n_texts] != n_ids)
        return bpe_fail(BPE_ERR_STATE, "bpe native: bad id offsets");
    for (int64_t k = 0; k < n_texts; ++k)
        if (idoff[(size_t)k + 1] < idoff[(size_t)k]) return bpe_fail(BPE_ERR_STATE, "bpe native: bad id offsets");
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
    // the reference's error order: the first failing text's error, and inside one text the char's.
    // An unknown char: the texts before its text may still hold a hole of the index, which comes first.
    const bool vec = kind == BPE_ENCODE_VECTORS, bad_char = T.h_st[TS_BADCHAR] != TXT_NONE;
    const int64_t pc = (int64_t)T.h_st[TS_BADCHAR];
    const int64_t n_use = bad_char ? text_of_unit(pc) : n_texts;
    if (bad_char && (!vec || n_use == 0)) return char_error(pc);
    const VecMap vmap{T.d_tvi, (uint32_t)T.tvi.size(), T.d_st};
    DropDone O;
    if ((rc = drop_run(E, dk, D, d_ids, idoff.data(), n_use, vec ? &vmap : nullptr, BPE_ERR_STATE,
                       "bpe native: char table id out of range", O)))
        return rc;
    if (vec) {
        ENC_TRY(hipMemcpyAsync(T.h_st, T.d_st, TS_WORDS * 8, hipMemcpyDeviceToHost, s));
        ENC_TRY(hipStreamSynchronize(s));
        if (T.h_st[TS_BADIDX] != TXT_NONE) {
            // the hole's result j, its text ki and the sample's first result j0
            const int64_t pi = (int64_t)T.h_st[TS_BADIDX];
            const int64_t j = (int64_t)(std::upper_bound(O.h_ooff, O.h_ooff + O.n_res + 1, pi) - O.h_ooff) - 1;
            const int64_t ki = (int64_t)(std::upper_bound(O.P.seg_of.begin(), O.P.seg_of.end(), j / S) - O.P.seg_of.begin()) - 1;
            const int64_t g0 = O.P.seg_of[(size_t)ki], ns = O.P.seg_of[(size_t)ki + 1] - g0;
            const int64_t j0 = g0 * S + (j - g0 * S) / ns * ns;
            int32_t id = 0;
            ENC_TRY(hipMemcpyAsync(&id, D.R.out + O.h_res_off[j] + (pi - O.h_ooff[j]), 4, hipMemcpyDeviceToHost, s));
            ENC_TRY(hipStreamSynchronize(s));
            return text_index_error(id, ki, pi - O.h_ooff[j0]);
        }
    }
    if (bad_char) return char_error(pc);
    if ((rc = packed_length(O.h_ooff, O.n_res, S * n_ids, cap, needed))) return rc;
    const int64_t n_out = *needed;
    if (dev) {
        if (!O.split(n_texts))
            ENC_TRY(hipMemcpyAsync(out_off, D.R.ooff, (size_t)(n_texts * S + 1) * 8, hipMemcpyDeviceToDevice, s));
        else {
            k_text_ooff<<<(unsigned)((n_texts * S + 256) / 256), 256, 0, s>>>(D.R.ooff, D.res_of, n_texts * S, out_off);
            ENC_TRY(hipGetLastError());
        }
    }
    if ((rc = copy_packed(s, vals_out, D.R.ids, n_out, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost))) return rc;
    if (!dev)
        for (int64_t j = 0; j <= n_texts * S; ++j) out_off[j] = O.h_ooff[O.h_res_of[j]];
    drop_count(E, n_texts, S, n_ids, n_out);
    return BPE_OK;
}

}  // namespace

extern "C" {

int bpe_encode_dropout_batch(bpe_encoder *E, const int32_t *ids, const int64_t *off, int64_t n_texts, int32_t samples,
                             double p, uint64_t seed, int64_t text_base, int32_t *ids_out, int64_t *out_off) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: null encoder");
    DropKey dk;
    const int rc = drop_check_args(samples, p, text_base, seed, dk);
    return rc ? rc : drop_ids(E, ids, off, n_texts, dk, ids_out, out_off);
}

int bpe_encode_dropout_text_batch(bpe_encoder *E, int kind, const uint16_t *units, const int64_t *off, int64_t n_texts,
                                  int32_t samples, double p, uint64_t seed, int64_t text_base, int32_t *vals_out,
                                  int64_t vals_cap, int64_t *out_off) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: null encoder");
    DropKey dk;
    int64_t needed = 0;
    const int rc = drop_check_args(samples, p, text_base, seed, dk);
    return rc ? rc : drop_text(E, kind, units, off, n_texts, dk, vals_out, vals_cap, out_off, false, &needed);
}

int bpe_encode_dropout_text_batch_device(bpe_encoder *E, int kind, const uint16_t *d_units, const int64_t *d_off,
                                         int64_t n_texts, int32_t samples, double p, uint64_t seed, int64_t text_base,
                                         int32_t *d_vals_out, int64_t vals_cap, int64_t *d_out_off, int64_t *needed) {
    if (!E || !needed) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    DropKey dk;
    const int rc = drop_check_args(samples, p, text_base, seed, dk);
    return rc ? rc : drop_text(E, kind, d_units, d_off, n_texts, dk, d_vals_out, vals_cap, d_out_off, true, needed);
}

int bpe_encoder_get_dropout_stats(bpe_encoder *E, bpe_dropout_stats *out) {
    if (!E || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    ENC_TRY(hipSetDevice(E->device));
    unsigned long long steps = 0;
    if (E->d_drop_steps) ENC_TRY(hipMemcpy(&steps, E->d_drop_steps, 8, hipMemcpyDeviceToHost));
    E->dst.steps = (int64_t)steps;
    *out = E->dst;
    return BPE_OK;
}

int bpe_encoder_reset_dropout_stats(bpe_encoder *E) {
    if (!E) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    ENC_TRY(hipSetDevice(E->device));
    if (E->d_drop_steps) ENC_TRY(hipMemset(E->d_drop_steps, 0, 8));
    E->dst = bpe_dropout_stats{};
    return BPE_OK;
}

}  // extern "C"
