// bpe_kernels.hip.h — CDNA4 (gfx950) kernels of the BPE merge-training hot path: everything the
// engine launches.  The constants, the layout structs, the streaming pass and the digest stream
// are in bpe_pass.hip.h (the part csrc/bpe_step.hip compiles with its own flags); this header adds
// the delta form's site kernel, the stitch and the reduces, the selection and the decision, and
// the kernels of ingest, compaction and read-back.
#pragma once
#include "bpe_pass.hip.h"

namespace bpe {

// ---- the delta form's site kernel -----------------------------------------------------------
// A live slot of the corpus as (chunk, slot, the chunk's live length), walked one live slot at a
// time by a single lane: over dead tails and empty chunks, across chunk and region boundaries.
struct Cursor {
    int64_t q;
    int k, len;
};

__device__ __forceinline__ int chunk_live_len(const int32_t *ids, int64_t q) {
    const int32_t v = ids[q * CHUNK + (CHUNK - 1)];
    return v >= SEP ? CHUNK : ((LEN_TAG - v) & 255);
}

// The live slot before p (p moves there); SEP before the corpus start.
__device__ __forceinline__ int32_t live_prev(const int32_t *ids, Cursor &p) {
    for (;;) {
        if (p.k > 0) {
            --p.k;
            return ids[p.q * CHUNK + p.k];
        }
        if (p.q == 0) return SEP;
        --p.q;
        p.len = chunk_live_len(ids, p.q);
        p.k = p.len;
    }
}

// The live slot after p (p moves there); SEP past the corpus end.
__device__ __forceinline__ int32_t live_next(const int32_t *ids, int64_t n_chunks, Cursor &p) {
    for (;;) {
        if (p.k + 1 < p.len) {
            ++p.k;
            return ids[p.q * CHUNK + p.k];
        }
        if (p.q + 1 >= n_chunks) return SEP;
        ++p.q;
        p.len = chunk_live_len(ids, p.q);
        p.k = -1;
    }
}

// The table's deltas of one site of the merge (a, b) -> c, a != b, from the post-merge corpus: the
// site is the token c at p (c is a fresh id, so every c is a site).  x, y = the live tokens before
// and after it (SEP ends a sample: no pair across it).  Before the merge the site read a b, so:
//  - left, removed: (x, a); when x == c the site before ended in b, so (b, a); when x == a the
//    site's a ended a run of M + 1 a's that is now M long, and a run of L counts floor(L / 2):
//    one (a, a) less iff M is odd;
//  - left, added: (x, c); when x == c the sites form a chain, counted floor(n / 2) once, by the
//    chain's last site (n = the c's up to and including this one);
//  - right, only when y != c (the next site's left side covers that adjacency): removed (b, y),
//    or, y == b, one (b, b) less iff the M' b's that follow are odd in number; added (c, y).
// The pair (a, b) itself loses W, once for the whole merge (k_site_delta).
__device__ void site_deltas(const int32_t *ids, int64_t n_chunks, const Cursor &p, int32_t a,
                            int32_t b, int32_t c, unsigned long long *table) {
    auto add = [&](int32_t x, int32_t y, long long d) {
        atomicAdd(&table[table_index(x, y)], (unsigned long long)d);
    };
    Cursor l = p, r = p;
    const int32_t x = live_prev(ids, l);
    const int32_t y = live_next(ids, n_chunks, r);
    if (x >= 0) {
        if (x == c) {
            add(b, a, -1);
        } else if (x == a) {
            long long m = 1;
            for (Cursor t = l; live_prev(ids, t) == a;) ++m;
            if (m & 1) add(a, a, -1);
            add(a, c, 1);
        } else {
            add(x, a, -1);
            add(x, c, 1);
        }
    }
    if (y == c) return;
    if (x == c) {
        long long n = 2;
        for (Cursor t = l; live_prev(ids, t) == c;) ++n;
        add(c, c, n >> 1);
    }
    if (y >= 0) {
        if (y == b) {
            long long m = 1;
            for (Cursor t = r; live_next(ids, n_chunks, t) == b;) ++m;
            if (m & 1) add(b, b, -1);
        } else {
            add(b, y, -1);
        }
        add(c, y, 1);
    }
}

// After a delta iteration's apply-only stream, on the consistent post-merge corpus: one workgroup
// per region, one wave per listed chunk (k_apply_loop's site list), every token c of the chunk a
// site (a site across two chunks lists both; the chunk holding the c owns it).  The deltas go
// into the u64 table with 64-bit atomic adds (negative ones as two's complement), bins from
// table_index: hot bins and sketch buckets alike.  The bin of (a, b) loses W; a hot bin must have
// held exactly W, a sketch bucket at least W (it sums every pair it holds), else LOOP_ERROR.
__global__ void __launch_bounds__(256)
k_site_delta(const int32_t *__restrict__ ids, int64_t n_chunks, int64_t cpr, int R,
             const uint32_t *__restrict__ site_list, const uint32_t *__restrict__ site_n,
             unsigned long long *__restrict__ table, LoopCtl *ctl) {
    if (ctl->status != LOOP_RUN || !ctl->delta) return;
    const int32_t a = ctl->a, b = ctl->b, c = ctl->c;
    const unsigned long long W = (unsigned long long)ctl->w;
    const int r = blockIdx.x;
    if (r >= R) return;
    if (r == 0 && threadIdx.x == 0) {
        const int bin = table_index(a, b);
        const unsigned long long old = atomicAdd(&table[bin], 0ull - W);
        if (bin < HOT_BINS ? old != W : old < W) {
            ctl->status = LOOP_ERROR;
            ctl->err = 3;
            ctl->err_got = old;
            ctl->err_want = W;
        }
    }
    const int lane = threadIdx.x & 63;
    const uint32_t n = min(site_n[r], (uint32_t)cpr);
    const uint32_t *seg = site_list + (int64_t)r * cpr;
    for (uint32_t i = threadIdx.x >> 6; i < n; i += 4) {
        const int64_t q = seg[i];
        if (q >= n_chunks) continue;
        const int4 v = reinterpret_cast<const int4 *>(ids)[q * (CHUNK / 4) + lane];
        const int32_t l3 = bcast(v.w, 63);
        Cursor p;
        p.q = q;
        p.len = l3 >= SEP ? CHUNK : ((LEN_TAG - l3) & 255);
        const int32_t t[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (t[e] == c) {
                p.k = 4 * lane + e;
                site_deltas(ids, n_chunks, p, a, b, c, table);
            }
    }
}

__device__ __forceinline__ int prev_nonempty(const RegionSum *s, int q) {
    while (q >= 0 && s[q].n_live == 0) --q;
    return q;
}

__device__ __forceinline__ int next_nonempty(const RegionSum *s, int q, int R) {
    while (q < R && s[q].n_live == 0) ++q;
    return q;
}

// Stitches the regions after a pass.  The waves counted every pair inside their region, with the
// X X pairs of each region's first run counted from the region start; here, per region:
//  - the pair straddling its left boundary (unless both sides belong to one run);
//  - for the run that starts in the region and continues into later regions (segments of lengths
//    L_1..L_n, the waves having counted sum floor(L_i / 2)): floor(sum L_i / 2) - sum floor(L_i / 2)
//    = floor(#odd segments / 2) more X X pairs;
//  - the RegionCarry the next pass needs (neighbour tokens, run-offset parity of the first token).
template <int MODE>
__device__ __forceinline__ void runs_body(const RegionSum *__restrict__ s, int R,
                                          RegionCarry *__restrict__ carry,
                                          unsigned long long *__restrict__ spill, ColdTable ct,
                                          const uint32_t *__restrict__ heavy, const LoopCtl *ctl,
                                          int32_t ma, int32_t mb, int32_t mc,
                                          unsigned long long *hot, unsigned long long *delta,
                                          const uint32_t *__restrict__ site_n = nullptr,
                                          unsigned long long *n_listed = nullptr) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (site_n && !loop_off(ctl)) {
        // the delta form's statistic: chunks listed by the pass, one atomic per wave
        unsigned n = r < R ? site_n[r] : 0u;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(n_listed, (unsigned long long)n);
    }
    if (r >= R) return;
    // the region and its two neighbours, loaded together before anything else (the loop's state
    // included): one memory latency for the common case, where both neighbours are non-empty and
    // no run crosses a boundary.  (Walking to the neighbours first made a chain of four dependent
    // loads, each a round trip to memory for sums another XCD's L2 wrote: 4.9 us per launch.)
    RegionSum empty;
    empty.n_live = 0;
    empty.lead_len = 0;
    empty.first_tok = NONE;
    empty.last_tok = NONE;
    empty.uniform = 0;
    empty.trail_odd = 0;
    const RegionSum me = s[r];
    const RegionSum sl = r > 0 ? s[r - 1] : empty;
    const RegionSum sr = r + 1 < R ? s[r + 1] : empty;
    if (loop_off(ctl)) return;
    if ((MODE == MODE_FUSED || MODE == MODE_INCR) && ctl) {   // (device loop: the merge applied)
        ma = ctl->a;
        mb = ctl->b;
        mc = ctl->c;
    }
    Sink k;
    k.hist = nullptr;
    k.spill = spill;
    k.ct = ct;
    k.heavy = heavy;
    k.ma = MODE == MODE_FUSED || MODE == MODE_INCR ? ma : -1;
    k.mb = mb;
    k.mc = mc;
    k.hot = hot;
    k.rspill = nullptr;
    k.delta = delta;
    // the nearest non-empty regions before and after (rarely past the immediate neighbours)
    int p = r - 1;
    RegionSum P = sl;
    if (p >= 0 && P.n_live == 0) {
        p = prev_nonempty(s, p - 1);
        P = p >= 0 ? s[p] : empty;
    }
    int nx = r + 1;
    RegionSum N = sr;
    if (nx < R && N.n_live == 0) {
        nx = next_nonempty(s, nx + 1, R);
        N = nx < R ? s[nx] : empty;
    }
    RegionCarry rc;
    rc.prev_tok = p >= 0 ? P.last_tok : SEP;
    rc.next_tok = nx < R ? N.first_tok : SEP;
    rc.carry_off = 0;
    if (me.n_live == 0) {
        carry[r] = rc;
        return;
    }
    const int32_t x0 = me.first_tok;
    const bool linked = p >= 0 && x0 >= 0 && P.last_tok == x0;
    if (linked) {
        // parity of the number of x0 tokens of the run before this region
        int64_t par = 0;
        for (int q = p; q >= 0;) {
            const RegionSum Q = q == p ? P : s[q];
            if (Q.uniform) {
                par ^= Q.n_live & 1;
                const int q2 = prev_nonempty(s, q - 1);
                if (q2 >= 0 && s[q2].last_tok == x0) q = q2;
                else break;
            } else {
                par ^= Q.trail_odd;
                break;
            }
        }
        rc.carry_off = par;
    } else if (p >= 0 && x0 >= 0 && P.last_tok >= 0) {
        add_pairs_global<MODE>(k, P.last_tok, x0, 1);            // the boundary pair
    }
    carry[r] = rc;
    // the run that starts in this region and reaches its end
    if (me.uniform && linked) return;
    const int32_t x = me.uniform ? x0 : me.last_tok;
    if (x < 0) return;
    int64_t odd = me.uniform ? (me.n_live & 1) : me.trail_odd;
    int segs = 1;
    for (int q = nx; q < R;) {
        const RegionSum Q = q == nx ? N : s[q];
        if (Q.first_tok != x) break;
        ++segs;
        if (Q.uniform) {
            odd += Q.n_live & 1;
            q = next_nonempty(s, q + 1, R);
        } else {
            odd += Q.lead_len & 1;
            break;
        }
    }
    if (segs > 1 && odd >= 2) add_pairs_global<MODE>(k, x, x, (unsigned long long)(odd >> 1));
}

template <int MODE>
__global__ void k_runs(const RegionSum *__restrict__ s, int R, RegionCarry *__restrict__ carry,
                       unsigned long long *__restrict__ spill, ColdTable ct,
                       const uint32_t *__restrict__ heavy, const LoopCtl *ctl, int32_t ma = -1,
                       int32_t mb = -1, int32_t mc = -1, unsigned long long *hot = nullptr,
                       unsigned long long *delta = nullptr) {
    runs_body<MODE>(s, R, carry, spill, ct, heavy, ctl, ma, mb, mc, hot, delta);
}

// The table state's stitch when the delta form is allowed, one launch for either form of the
// iteration: after a full pass k_runs<MODE_TABLE>; after the apply-only stream the carries alone
// (k_runs<MODE_NONE>) and the count of the chunks it listed (LoopCtl::delta_chunks).
__global__ void k_runs_loop(const RegionSum *__restrict__ s, int R, RegionCarry *__restrict__ carry,
                            unsigned long long *__restrict__ spill, ColdTable ct,
                            const uint32_t *__restrict__ heavy, LoopCtl *ctl,
                            const uint32_t *__restrict__ site_n) {
    if (ctl->delta)
        runs_body<MODE_NONE>(s, R, carry, nullptr, ct, nullptr, ctl, -1, -1, -1, nullptr, nullptr,
                             site_n, &ctl->delta_chunks);
    else
        runs_body<MODE_TABLE>(s, R, carry, spill, ct, heavy, ctl, -1, -1, -1, nullptr, nullptr);
}

// Sums the per-workgroup 16-bit LDS partials and the spill table into the u64 table (hot bins
// [0, 64K), sketch buckets [64K, TABLE_BINS)), zeroes the spill for the next pass, and leaves the
// best hot key (max_length filter applied) in res->best.  A block owns 128 words (256 bins):
// 32 lanes x 4 words, each of its 8 lane groups sums every 8th slab, so each thread keeps 32
// independent uint4 loads in flight instead of walking all G slabs.
constexpr int REDUCE_WORDS_PER_BLOCK = 128;
static_assert(HIST_WORDS % REDUCE_WORDS_PER_BLOCK == 0, "reduce tiling");

__device__ __forceinline__ bool pair_ok(int32_t a, int32_t b, const int32_t *len16,
                                        int64_t max_length);

// A block owns 128 dwords (256 bins): 32 lanes x 4 dwords (512 contiguous bytes of a slab per
// lane group), each of its REDUCE_GROUPS lane groups summing every REDUCE_GROUPS-th slab with up to
// 16 16-B loads in flight.  (Narrower column tiles, reading many slabs per wave-instruction, ran
// 2-3x slower.)  The slabs were just written (MALL-resident): the kernel is latency-bound, so the
// lane groups are many (more waves per CU hiding the loads' latency) rather than few with deep
// chains of loads.
#ifndef BPE_REDUCE_GROUPS
#define BPE_REDUCE_GROUPS 8
#endif
constexpr int REDUCE_GROUPS = BPE_REDUCE_GROUPS;
constexpr int REDUCE_THREADS = 32 * REDUCE_GROUPS;
static_assert(REDUCE_THREADS >= 256 && REDUCE_THREADS <= 1024, "reduce block");
__global__ void __launch_bounds__(REDUCE_THREADS)
k_reduce_table(const uint32_t *__restrict__ partials, int G, unsigned long long *__restrict__ spill,
               unsigned long long *__restrict__ table, const int32_t *__restrict__ len16,
               int64_t max_length, Result *res, const LoopCtl *ctl,
               unsigned long long *__restrict__ hdr = nullptr,
               const unsigned long long *__restrict__ rep = nullptr,
               unsigned long long *__restrict__ bin_max = nullptr,
               unsigned long long *__restrict__ bkey = nullptr) {
    __shared__ uint32_t s_sum[REDUCE_GROUPS][32][8];
    // A delta iteration of the device loop (LoopCtl::delta, uniform over the grid): the table is
    // already current (k_site_delta), so nothing is summed or written; the block only scans its
    // 256 bins for the best hot key and the largest bin, as after a reduce.  (Both words loaded
    // before either is tested: one memory latency.)
    const int32_t status = ctl ? ctl->status : LOOP_RUN;
    const bool scan = ctl && ctl->delta;
    if (status != LOOP_RUN) return;
    const int t = threadIdx.x;
    // (sharded: the exchange header carries this shard's replacement count, summed with the table)
    if (hdr && rep && blockIdx.x == 0 && t == 0) hdr[0] = *rep;
    const int wl = t & 31, grp = t >> 5;
    const int w0 = blockIdx.x * REDUCE_WORDS_PER_BLOCK + 4 * wl;   // first of my 4 words
    uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // < 2^24 each: G <= 256 slabs x halves < 2^16
    const uint4 *p4 = reinterpret_cast<const uint4 *>(partials + w0);
    auto add = [&](const uint4 p) {
        acc[0] += p.x & 0xFFFFu;
        acc[1] += p.x >> 16;
        acc[2] += p.y & 0xFFFFu;
        acc[3] += p.y >> 16;
        acc[4] += p.z & 0xFFFFu;
        acc[5] += p.z >> 16;
        acc[6] += p.w & 0xFFFFu;
        acc[7] += p.w >> 16;
    };
    constexpr int RG = REDUCE_GROUPS;
    int g = scan ? G : grp;
    for (; g + 15 * RG < G; g += 16 * RG) {
        uint4 p[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) p[q] = p4[(size_t)(g + RG * q) * (HIST_WORDS / 4)];
#pragma unroll
        for (int q = 0; q < 16; ++q) add(p[q]);
    }
    for (; g + 7 * RG < G; g += 8 * RG) {
        uint4 p[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) p[q] = p4[(size_t)(g + RG * q) * (HIST_WORDS / 4)];
#pragma unroll
        for (int q = 0; q < 8; ++q) add(p[q]);
    }
    for (; g < G; g += RG) add(p4[(size_t)g * (HIST_WORDS / 4)]);
#pragma unroll
    for (int i = 0; i < 8; ++i) s_sum[grp][wl][i] = acc[i];
    __syncthreads();
    // thread t < 256 finalises bin 2*w0' + i for one (word-lane, i) pair: 256 bins
    unsigned long long k = 0, vm = 0;
    if (t < 256) {
        const int bl = t >> 3, bi = t & 7;
        uint32_t sum = 0;
#pragma unroll
        for (int q = 0; q < RG; ++q) sum += s_sum[q][bl][bi];
        // dword w holds bins 2w and 2w + 1 (hot pairs and sketch buckets alike): contiguous writes
        const int bin = blockIdx.x * (2 * REDUCE_WORDS_PER_BLOCK) + t;
        unsigned long long v;
        if (scan) {
            v = table[bin];
        } else {
            v = (unsigned long long)sum + spill[bin];
            table[bin] = v;
            spill[bin] = 0;
        }
        if (bin < HOT_BINS && v && pair_ok(bin_a(bin), bin_b(bin), len16, max_length))
            k = pack_key(v, bin_a(bin), bin_b(bin));
        vm = v;
    }
    // one atomic per workgroup (a wave each would queue over a thousand on one address); and the
    // largest bin of all, hot and sketch alike: the next decision's bound, LoopCtl::unscreened
    k = wave_max_u64(k);
    vm = wave_max_u64(vm);
    __shared__ unsigned long long s_best[4], s_vmax[4];
    if ((t & 63) == 0 && t < 256) {
        s_best[t >> 6] = k;
        s_vmax[t >> 6] = vm;
    }
    __syncthreads();
    // (bin_max: where the largest bin goes, res->bin_max by default; a sharded rank's reduce has no
    // Result to select from, but its own largest bin bounds its own next pass alike)
    if (!bin_max && res) bin_max = &res->bin_max;
    if (t == 0 && (res || bin_max)) {
        for (int w = 1; w < 4; ++w) {
            k = s_best[w] > k ? s_best[w] : k;
            vm = s_vmax[w] > vm ? s_vmax[w] : vm;
        }
        // (a hot block's own best key: what the digest stream predicts the next merges from,
        // DigestLists::bkey)
        if (bkey && blockIdx.x < HOT) bkey[blockIdx.x] = k;
        if (k && res) atomicMax(&res->best, k);
        if (bin_max) atomicMax(bin_max, vm + 1);
    }
}

// Marks the sketch buckets whose (global) sum reaches the best hot count: only cold pairs there
// can still reach W, so only they need exact counts.  T = max(W_hot, 1).
__global__ void k_heavy(const unsigned long long *__restrict__ table, Result *res,
                        uint32_t *__restrict__ heavy) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;   // one thread per bucket
    const unsigned long long w_hot = res->best >> 17;
    const unsigned long long T = w_hot ? w_hot : 1;
    const bool h = b < SKETCH_BINS && table[HOT_BINS + b] >= T;
    const unsigned long long m = __ballot(h);
    if ((threadIdx.x & 31) == 0 && b < SKETCH_BINS) {
        const uint32_t word = (uint32_t)(m >> (threadIdx.x & 32));
        heavy[b >> 5] = word;
        if (word) atomicAdd(&res->n_heavy, (unsigned)__popc(word));
    }
}

// max_length filter (core.ts:270-273) applied at selection time: it depends only on the pair,
// so excluding a pair here is equivalent to never counting it.
__device__ __forceinline__ bool pair_ok(int32_t a, int32_t b, const int32_t *len16,
                                        int64_t max_length) {
    return !max_length || (int64_t)len16[a] + len16[b] <= max_length;
}

// argmax over the dense hot table: best = max packed key.  One atomic per block of 256 (an atomic
// per wave queued a thousand on one address: 12 us per launch).
__global__ void __launch_bounds__(256)
k_argmax_hot(const unsigned long long *__restrict__ hot_counts, const int32_t *__restrict__ len16,
             int64_t max_length, Result *res, const LoopCtl *ctl = nullptr) {
    __shared__ unsigned long long s_best[4];
    if (loop_off(ctl)) return;
    unsigned long long k = 0;
    for (int bin = blockIdx.x * blockDim.x + threadIdx.x; bin < HOT_BINS;
         bin += gridDim.x * blockDim.x)
        if (pair_ok(bin_a(bin), bin_b(bin), len16, max_length)) {
            const unsigned long long v = pack_key(hot_counts[bin], bin_a(bin), bin_b(bin));
            k = v > k ? v : k;
        }
    k = wave_max_u64(k);
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) k = s_best[w] > k ? s_best[w] : k;
        if (k) atomicMax(&res->best, k);
    }
}

// argmax over the claimed cold slots (dense view, coalesced).
// Also counts the claims whose pair is gone (res->cold_dead, zero on entry: a real key whose count a
// merge zeroed and no pass counted again): they stay in the dense view, and every scan streams
// them, until the table is rebuilt.  (Holes, key EMPTY, are claims that lost a race.)
__global__ void k_argmax_cold(ColdTable ct, const int32_t *__restrict__ len16, int64_t max_length,
                              Result *res, const LoopCtl *ctl = nullptr) {
    __shared__ unsigned long long s_best[4];
    __shared__ unsigned s_live;
    if (loop_off(ctl)) return;
    const uint32_t n = cold_used(ct);
    if (blockIdx.x == 0 && threadIdx.x == 0)   // (rides along with the Result's copy to the host)
        res->cold_flags = ((unsigned long long)*ct.overflow << 32) | n;
    if (threadIdx.x == 0) s_live = 0;
    __syncthreads();
    unsigned long long best = 0;
    unsigned dead = 0;
    // COLD_ILP entries per thread and sweep, their loads issued together (one dependent load per
    // thread at a time left the scan latency-bound at about a third of the stream rate)
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += COLD_ILP * stride) {
        unsigned long long v[COLD_ILP];
        uint32_t kk[COLD_ILP];
#pragma unroll
        for (int q = 0; q < COLD_ILP; ++q) {
            const uint32_t i = i0 + q * stride;
            v[q] = i < n ? ct.dcounts[i] : 0ull;
            kk[q] = i < n ? ct.dkeys[i] : EMPTY;
        }
#pragma unroll
        for (int q = 0; q < COLD_ILP; ++q) {
            const unsigned long long n_ab = v[q];
            dead += (n_ab == 0) & (kk[q] != EMPTY);
            const int32_t a = (int32_t)(kk[q] >> 16), b = (int32_t)(kk[q] & 0xFFFFu);
            if (n_ab && pair_ok(a, b, len16, max_length)) {
                const unsigned long long k = pack_key(n_ab, a, b);
                best = k > best ? k : best;
            }
        }
    }
    // one atomic per workgroup (a wave each would queue thousands on one address)
    best = wave_max_u64(best);
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
    if (dead) atomicAdd(&s_live, dead);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) best = s_best[w] > best ? s_best[w] : best;
        if (best) atomicMax(&res->best, best);
        if (s_live) atomicAdd(&res->cold_dead, (unsigned long long)s_live);
    }
}

// Last-block detection over a whole grid.  Thread 0 of each block calls it after its block's
// writes and a __threadfence; it returns true in the one block that finishes last.  Same-address
// atomics are serialised by the memory side (a device-wide ticket of 1024 blocks took ~60 us), so
// blocks count in groups of TK_GROUP, one counter per group on its own 128-byte line, and only
// each group's last block takes the top ticket.  Counters are zero between launches (each last
// block resets the counter it completed).
constexpr int TK_STRIDE = 32, TK_GROUP = 32, TK_MAX_GROUPS = 64;
constexpr int TICKET_WORDS = TK_STRIDE * (1 + TK_MAX_GROUPS);
__device__ bool grid_last(unsigned int *ticket) {
    const unsigned G = gridDim.x, g = blockIdx.x / TK_GROUP;
    const unsigned ng = (G + TK_GROUP - 1) / TK_GROUP;
    const unsigned size = min((unsigned)TK_GROUP, G - g * TK_GROUP);
    unsigned int *gc = ticket + TK_STRIDE * (1 + g);
    if (atomicAdd(gc, 1u) != size - 1) return false;
    *gc = 0;
    __threadfence();
    if (atomicAdd(ticket, 1u) != ng - 1) return false;
    *ticket = 0;
    return true;
}

// The maintained state's selection in one launch (the single-corpus device loop; was k_argmax_hot
// + k_argmax_cold + k_collect): the best key over the hot bins and the cold table's dense entries,
// and every pair holding it.  res->best and res->n_cand are zero on entry (k_decide / k_tie_fused
// clear them).  Two forms, the same for every block of the launch:
//  - full (full_req: the first selection of a batch, every SEL_FULL_EVERY-th, and always in
//    MODE_FUSED; launched on the full grid): every dense entry.  Workgroup w takes the CB-entry blocks w, w + G, ...; each
//    thread keeps its best key, its first entry holding it and how many of its entries hold it;
//    each workgroup its best and the entries holding it (a rescan only by the threads with
//    several).  Every block's max is written (ct.bmax), the dirty flags cleared, and the dead
//    claims (count 0, key set) counted: they decide when the table is rebuilt.
//  - incremental: a merge (a, b) -> c changes only the pairs with a side in {a, b, c}.  Those with
//    a or b were zeroed (k_incr_invalidate flagged the blocks whose max they may have been) and
//    recounted to at most their old count; those with c are new claims, at the end of the dense
//    view.  So only the flagged blocks and the blocks of claims made since the last selection are
//    recomputed; the other blocks' maxima are still exact.  The hot bins are scanned in full.
//    (Launched on HOT_BINS / 256 workgroups: zipf C3 recomputes ~24 of ~7700 blocks per merge,
//    so the grid's tickets and the last workgroup's record scan were most of the cost.)
// A ticket picks the last workgroup, which settles the global best from the workgroups' records
// (and, incremental, from the block maxima: the entries of the blocks holding it are the cold
// candidates).  The dead-claim count of the last full scan stands for the incremental ones.
constexpr int SEL_MAX = MAX_CAND + 1;   // (more than MAX_CAND candidates: the host path)
constexpr int SEL_FULL_EVERY = 16;
constexpr uint32_t SEL_MAX_BLOCKS = 1u << 16;   // (more blocks: always the full scan)
struct BlockBest {
    unsigned long long key;
    uint32_t n;
    uint32_t dead;   // the block's dead claims
    int2 cand[SEL_MAX];
};

__device__ __forceinline__ unsigned long long cold_entry_key(const ColdTable &ct, uint32_t i,
                                                             uint32_t n, const int32_t *len16,
                                                             int64_t max_length, int2 &ab,
                                                             unsigned &dead) {
    if (i >= n) return 0;
    const unsigned long long v = ct.dcounts[i];
    const uint32_t kk = ct.dkeys[i];
    dead += (v == 0) & (kk != EMPTY);
    ab = make_int2((int32_t)(kk >> 16), (int32_t)(kk & 0xFFFFu));
    return v && pair_ok(ab.x, ab.y, len16, max_length) ? pack_key(v, ab.x, ab.y) : 0ull;
}

// max over a 256-thread workgroup (s: 4 words of LDS); every thread gets it
__device__ __forceinline__ unsigned long long wg_max_u64(unsigned long long v, unsigned long long *s) {
    v = wave_max_u64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    return max(max(s[0], s[1]), max(s[2], s[3]));
}

__global__ void __launch_bounds__(256) k_select_maint(const unsigned long long *__restrict__ hot,
                                                      ColdTable ct, const int32_t *__restrict__ len16,
                                                      int64_t max_length, Result *res, int2 *cand,
                                                      BlockBest *rec, unsigned int *ticket,
                                                      const LoopCtl *ctl, int full_req) {
    __shared__ unsigned long long s_best[4], s_red[4];
    __shared__ unsigned s_dead, s_n;
    __shared__ int2 s_c[SEL_MAX];
    __shared__ bool s_last;
    __shared__ int s_full;
    __shared__ uint32_t s_nl, s_b0, s_b1, s_ncb;
    __shared__ uint32_t s_cb[64];
    if (loop_off(ctl)) return;
    const uint32_t n_cold = cold_used(ct);
    const uint32_t nblk = (n_cold + CB - 1) / CB;
    if (threadIdx.x == 0) {
        // (read once and broadcast: every branch around a barrier below is uniform)
        const uint32_t n0 = *ct.sel_n0;
        s_full = full_req || nblk > SEL_MAX_BLOCKS || n0 > n_cold;
        s_nl = min(*ct.n_blist, ct.mask / CB + 1);
        s_b0 = n0 / CB;              // blocks holding claims made since the last selection
        s_b1 = nblk;
        s_dead = s_n = 0;
    }
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    if (tid == 0) res->cold_flags = ((unsigned long long)*ct.overflow << 32) | n_cold;
    __syncthreads();
    const bool full = s_full;
    unsigned long long best = 0;
    int2 first = make_int2(-1, -1);
    uint32_t cnt = 0;
    unsigned dead = 0;
    auto see = [&](unsigned long long k, int2 ab) {
        if (k > best) {
            best = k;
            first = ab;
            cnt = 1;
        } else if (k && k == best) {
            ++cnt;
        }
    };
    for (uint32_t bin = tid; bin < (uint32_t)HOT_BINS; bin += stride) {
        const int32_t a = bin_a(bin), b = bin_b(bin);
        if (pair_ok(a, b, len16, max_length)) see(pack_key(hot[bin], a, b), make_int2(a, b));
    }
    // one CB-entry block: every thread its 4 entries (coalesced); the block's max to ct.bmax
    auto block = [&](uint32_t blk, bool keep) {
        unsigned long long m = 0;
#pragma unroll
        for (int q = 0; q < (int)(CB / 256); ++q) {
            int2 ab;
            const unsigned long long k =
                cold_entry_key(ct, blk * CB + threadIdx.x + 256 * q, n_cold, len16, max_length, ab, dead);
            if (keep) see(k, ab);
            m = max(m, k);
        }
        m = wg_max_u64(m, s_red);
        if (threadIdx.x == 0) {
            ct.bmax[blk] = m;
            ct.bdirty[blk] = 0;
        }
    };
    if (full) {
        for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) block(blk, true);
    } else {
        // the flagged blocks, then the blocks of the new claims
        const uint32_t nl = s_nl, nn = s_b1 - min(s_b0, s_b1);
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(ct.n_recomputed, nl + nn);
        for (uint32_t j = blockIdx.x; j < nl + nn; j += gridDim.x) {
            // (blist holds blocks of entries below n_used: always < nblk, so every thread of
            // the workgroup calls block() with the same blk)
            block(j < nl ? ct.blist[j] : s_b0 + (j - nl), false);
        }
        dead = 0;
    }
    unsigned long long bb = wave_max_u64(best);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = bb;
    if (dead) atomicAdd(&s_dead, dead);
    __syncthreads();
    bb = max(max(s_best[0], s_best[1]), max(s_best[2], s_best[3]));
    if (bb && best == bb) {
        if (cnt == 1) {
            const unsigned k = atomicAdd(&s_n, 1u);
            if (k < SEL_MAX) s_c[k] = first;
        } else {
            // (rare: several entries of this thread hold the block's best) the thread's elements again
            for (uint32_t bin = tid; bin < (uint32_t)HOT_BINS; bin += stride) {
                const int32_t a = bin_a(bin), b = bin_b(bin);
                if (pair_ok(a, b, len16, max_length) && pack_key(hot[bin], a, b) == bb) {
                    const unsigned k = atomicAdd(&s_n, 1u);
                    if (k < SEL_MAX) s_c[k] = make_int2(a, b);
                }
            }
            if (full)
                for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x)
                    for (int q = 0; q < (int)(CB / 256); ++q) {
                        int2 ab;
                        unsigned dd = 0;
                        if (cold_entry_key(ct, blk * CB + threadIdx.x + 256 * q, n_cold, len16,
                                           max_length, ab, dd) == bb) {
                            const unsigned k = atomicAdd(&s_n, 1u);
                            if (k < SEL_MAX) s_c[k] = ab;
                        }
                    }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        BlockBest &r = rec[blockIdx.x];
        r.key = bb;
        r.n = s_n;
        r.dead = s_dead;
        for (unsigned k = 0; k < min(s_n, (unsigned)SEL_MAX); ++k) r.cand[k] = s_c[k];
        __threadfence();
        s_last = grid_last(ticket);
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    // the last block: the global best, the dead claims and the candidates from every block's
    // record, read by all its threads (one thread alone waited on ~1000 dependent loads)
    unsigned long long g = 0, dsum = 0;
    for (unsigned q = threadIdx.x; q < gridDim.x; q += blockDim.x) {
        g = max(g, rec[q].key);
        dsum += rec[q].dead;
    }
    // incremental: the best block max; per thread its best, its first block holding it and how
    // many (16 loads in flight per thread: one at a time left this scan latency-bound)
    unsigned long long gc = 0;
    uint32_t gfirst = 0, gcnt = 0;
    if (!full)
        for (uint32_t b0 = threadIdx.x; b0 < nblk; b0 += 16 * 256) {
            unsigned long long v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) v[q] = b0 + 256 * q < nblk ? ct.bmax[b0 + 256 * q] : 0ull;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if (v[q] > gc) {
                    gc = v[q];
                    gfirst = b0 + 256 * q;
                    gcnt = 1;
                } else if (v[q] && v[q] == gc) {
                    ++gcnt;
                }
            }
        }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) dsum += __shfl_xor(dsum, d);
    __shared__ unsigned long long s_dsum[4];
    if ((threadIdx.x & 63) == 0) s_dsum[threadIdx.x >> 6] = dsum;
    g = wg_max_u64(max(g, gc), s_best);
    if (threadIdx.x == 0) {
        s_n = 0;
        s_ncb = 0;
    }
    __syncthreads();
    if (g)
        for (unsigned q = threadIdx.x; q < gridDim.x; q += blockDim.x) {
            const BlockBest &r = rec[q];
            if (r.key != g) continue;
            const unsigned k0 = atomicAdd(&s_n, r.n);
            for (unsigned k = 0; k < min(r.n, (unsigned)SEL_MAX) && k0 + k < (unsigned)SEL_MAX; ++k)
                cand[k0 + k] = r.cand[k];
        }
    if (!full && g) {
        // the cold blocks holding the best key, then their entries holding it
        if (gc == g && gcnt == 1) {
            const unsigned k = atomicAdd(&s_ncb, 1u);
            if (k < 64) s_cb[k] = gfirst;
        } else if (gc == g) {
            // (rare: several of this thread's blocks hold it) its blocks again
            for (uint32_t blk = threadIdx.x; blk < nblk; blk += blockDim.x)
                if (ct.bmax[blk] == g) {
                    const unsigned k = atomicAdd(&s_ncb, 1u);
                    if (k < 64) s_cb[k] = blk;
                }
        }
        __syncthreads();
        const uint32_t ncb = s_ncb;
        if (ncb > 64) {
            if (threadIdx.x == 0) s_n = SEL_MAX;   // (too many: the host path)
        } else {
            for (uint32_t j = 0; j < ncb; ++j)
#pragma unroll
                for (int q = 0; q < (int)(CB / 256); ++q) {
                    int2 ab;
                    unsigned dd = 0;
                    if (cold_entry_key(ct, s_cb[j] * CB + threadIdx.x + 256 * q, n_cold, len16,
                                       max_length, ab, dd) == g) {
                        const unsigned k = atomicAdd(&s_n, 1u);
                        if (k < SEL_MAX) cand[k] = ab;
                    }
                }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        res->best = g;
        res->n_cand = s_n;
        if (full) *ct.dead = (uint32_t)(s_dsum[0] + s_dsum[1] + s_dsum[2] + s_dsum[3]);
        res->cold_dead = *ct.dead;
        *ct.n_blist = 0;
        *ct.sel_n0 = n_cold;
    }
}

// One workgroup: best hot key (wave + LDS max), the hot pairs sharing it, and the heavy sketch
// buckets (sum >= max(W_hot, 1)).  Replaces three launches and their atomics on the fast path.
__global__ void __launch_bounds__(1024) k_select(const unsigned long long *__restrict__ table,
                                                 const int32_t *__restrict__ len16,
                                                 int64_t max_length, Result *res, int2 *cand,
                                                 uint32_t *__restrict__ heavy) {
    __shared__ unsigned long long s_best[16];
    __shared__ unsigned int s_n, s_heavy;
    const int t = threadIdx.x;
    unsigned long long best = 0;
    for (int bin = t; bin < HOT_BINS; bin += 1024) {
        const int32_t a = bin_a(bin), b = bin_b(bin);
        if (!pair_ok(a, b, len16, max_length)) continue;
        const unsigned long long k = pack_key(table[bin], a, b);
        best = k > best ? k : best;
    }
    best = wave_max_u64(best);
    if ((t & 63) == 0) s_best[t >> 6] = best;
    if (t == 0) s_n = s_heavy = 0;
    __syncthreads();
    best = 0;
    for (int i = 0; i < 16; ++i) best = s_best[i] > best ? s_best[i] : best;
    if (best)
        for (int bin = t; bin < HOT_BINS; bin += 1024) {
            const int32_t a = bin_a(bin), b = bin_b(bin);
            if (pair_ok(a, b, len16, max_length) && pack_key(table[bin], a, b) == best) {
                const unsigned i = atomicAdd(&s_n, 1u);
                if (i < CAND_CAP) cand[i] = make_int2(a, b);
            }
        }
    const unsigned long long w_hot = best >> 17;
    const unsigned long long T = w_hot ? w_hot : 1;
    for (int b0 = 0; b0 < SKETCH_BINS; b0 += 1024) {
        const int b = b0 + t;
        const unsigned long long m = __ballot(table[HOT_BINS + b] >= T);
        if ((t & 31) == 0) {
            const uint32_t word = (uint32_t)(m >> (t & 32));
            heavy[b >> 5] = word;
            if (word) atomicAdd(&s_heavy, (unsigned)__popc(word));
        }
    }
    __syncthreads();
    if (t == 0) {
        res->best = best;
        res->n_cand = s_n;
        res->n_heavy = s_heavy;
    }
}

// Multi-workgroup selection once res->best holds the best hot key (k_reduce_table): every hot
// pair sharing it (unordered: the tie rule does not depend on the order) and the heavy sketch
// buckets (sum >= max(W_hot, 1)).  res->n_cand / n_heavy must be zero on entry.
__global__ void __launch_bounds__(256) k_select_multi(const unsigned long long *__restrict__ table,
                                                      const int32_t *__restrict__ len16,
                                                      int64_t max_length, Result *res, int2 *cand,
                                                      uint32_t *__restrict__ heavy,
                                                      const LoopCtl *ctl) {
    if (loop_off(ctl)) return;
    const int idx = blockIdx.x * 256 + threadIdx.x;   // grid covers TABLE_BINS exactly
    const unsigned long long best = res->best;
    if (idx < HOT_BINS) {
        const int32_t a = bin_a(idx), b = bin_b(idx);
        if (best && pack_key(table[idx], a, b) == best && pair_ok(a, b, len16, max_length)) {
            const unsigned i = atomicAdd(&res->n_cand, 1u);
            if (i < CAND_CAP) cand[i] = make_int2(a, b);
        }
    } else {
        const unsigned long long w_hot = best >> 17;
        const unsigned long long T = w_hot ? w_hot : 1;
        const int bk = idx - HOT_BINS;
        const unsigned long long m = __ballot(table[idx] >= T);
        if ((threadIdx.x & 31) == 0) {
            const uint32_t word = (uint32_t)(m >> (threadIdx.x & 32));
            heavy[bk >> 5] = word;
            if (word) atomicAdd(&res->n_heavy, (unsigned)__popc(word));
        }
    }
}

// The device loop's decision: do_find's selection tail (core.ts:294-318) without leaving the GPU.
// phase 0, after the selection kernels: checks the previous merge's replacement count against its
// W, then ends the batch (no pair or W < min_weight: LOOP_DONE; heavy sketch buckets or more than
// MAX_CAND candidates: LOOP_HOST, the host path takes that iteration), waits for the tie pass
// (several candidates), or decides.  phase 1, after k_tie: the candidate whose last counted
// occurrence is earliest (rule R3).  A decision logs (a, b, W), registers the new token's UTF-16
// length (core.ts:318) and clears the Result for the next pass.  One thread.
//
// With a maintained cold table (ctl->maintained) the selection read that table, not the sketch:
// the batch hands over to the host when the table overflowed, is 3/4 full, is more than half dead
// claims (it is then rebuilt), or when the refresh of the chosen merge might not fit (2 claims
// per replacement at most).
//
// One rank of a sharded corpus (ctl->sharded): the replacement count checked is the SUM over the
// ranks (the exchange header `hdr`, all-reduced with the table or the delta rows).  Phase 0 only
// proposes (ctl->tie: 1 / 2 tie pass in the tail window / over the whole shard, 3 one candidate,
// 4 no merge, 5 the host path) and votes: the reasons above that depend on this rank's copy of the
// maintained tables (fill, dead claims, room) differ between ranks, so they ride in the tie
// all-reduce(MAX) (tie_pos[MAX_CAND]) and phase 1 decides on every rank alike.
// ---- the decision's parts (k_decide, and k_tie_fused's last block) ----
// Room in the maintained table for the refresh of the merge: every pair the merge creates has
// the new token c as a side, and c occurs W times, so it claims at most 2 W new slots.
__device__ __forceinline__ bool decide_room(const LoopCtl &C, const Result &R) {
    if (!C.maintained) return true;
    const long long W = (long long)(R.best >> 17);
    const unsigned long long V = (unsigned long long)C.next_id + 1;
    const unsigned long long claims = 2 * (unsigned long long)W < V * V ? 2 * W : V * V;
    return (R.cold_flags & 0xFFFFFFFFull) + claims + 64 <= C.cold_cap / 4 * 3;
}

// Phase 0's proposal from the snapshots: 4 no merge (LOOP_DONE), 5 the host path, 1 / 2 a tie
// pass over the corpus tail window / the whole corpus, 3 one candidate.  *vote: this corpus's
// own reasons for the host path (a sharded rank votes; one corpus proposes 5).  Sorts
// cand[0 .. n) by (a, b) when tied (the same order on every rank).
__device__ int decide_propose(const LoopCtl &C, const Result &R, int2 *cand, int &vote) {
    const unsigned long long best = R.best;
    const long long W = (long long)(best >> 17);
    const unsigned n = R.n_cand;
    vote = 0;
    if (C.maintained) {
        const unsigned long long used = R.cold_flags & 0xFFFFFFFFull;
        if ((R.cold_flags >> 32) || used * 4 > C.cold_cap * 3 || 2 * R.cold_dead > used + 65536)
            vote = 1;
    }
    if (!decide_room(C, R)) vote = 1;
    if (vote && !C.sharded) return 5;
    // a heavy sketch bucket may hold a cold pair above the best hot one (even when no hot pair
    // exists at all): only the host path's exact counts can tell
    if (!C.maintained && R.n_heavy) return 5;
    if (best == 0 || W < C.min_weight) return 4;                     // core.ts:312-313
    if (n == 0 || n > (unsigned)MAX_CAND || C.next_id >= C.max_id) return 5;
    if (n == 1) return 3;
    for (unsigned j = 1; j < n; ++j) {
        const int2 v = cand[j];
        unsigned i = j;
        for (; i > 0 && (cand[i - 1].x > v.x || (cand[i - 1].x == v.x && cand[i - 1].y > v.y)); --i)
            cand[i] = cand[i - 1];
        cand[i] = v;
    }
    // X Y candidates only: the corpus tail window first (a sharded corpus's tail is the last
    // rank's); else the full pass
    int all_xy = 1;
    for (unsigned j = 0; j < n; ++j) all_xy &= cand[j].x != cand[j].y;
    return all_xy ? 1 : 2;
}

// Rule R3 from the last positions (0: none): the candidate whose last counted occurrence comes
// first.  Tail window (tie == 1): one candidate missing there occurs only earlier, so it wins;
// two or more missing need the host path's full pass.  Returns 0 (a, b set), 1 (host), 2 (no
// occurrence at all: an error).
__device__ int decide_r3(int tie, unsigned n, const unsigned long long *pos, const int2 *cand,
                         int32_t &a, int32_t &b, int &lone) {
    unsigned long long bp = ~0ull;
    unsigned missing = 0;
    a = b = -1;
    lone = 0;
    for (unsigned j = 0; j < n; ++j) {
        const unsigned long long p = pos[j];
        if (p && p < bp) {
            bp = p;
            a = cand[j].x;
            b = cand[j].y;
        }
        missing += p == 0;
    }
    if (tie == 1 && missing) {
        if (missing > 1) return 1;
        for (unsigned j = 0; j < n; ++j)
            if (pos[j] == 0) {
                a = cand[j].x;
                b = cand[j].y;
            }
        lone = 1;
    }
    return a < 0 ? 2 : 0;
}

// The decision's writes: the log entry (a, b, W), the new token's UTF-16 length (core.ts:318),
// the merge the next pass applies, and a Result cleared for the next selection.
// n_chunks (the single-context loop only; 0: never the delta form): the iteration takes the delta
// form when the host allows it (the table state), a != b, and the merge's W sites lie in fewer
// than 1/16 of the chunks, the rule k_step_loop uses for a heavy merge.
__device__ void decide_commit(LoopCtl *ctl, Result *res, const LoopCtl &C, long long W, int32_t a,
                              int32_t b, int32_t *len16, long long *log, int64_t n_chunks = 0,
                              DigestLists *lists = nullptr) {
    const int32_t c = C.next_id;
    len16[c] = len16[a] + len16[b];
    const long long i = C.n_done;
    log[LOG_WORDS * i] = a;
    log[LOG_WORDS * i + 1] = b;
    log[LOG_WORDS * i + 2] = W;
    log[LOG_WORDS * i + 3] = -1;   // (filled in by the next decision or at the batch end)
    ctl->a = a;
    ctl->b = b;
    ctl->c = c;
    ctl->w = W;
    ctl->next_id = c + 1;
    ctl->n_done = i + 1;
    const unsigned long long bm = res->bin_max;
    const int32_t dl = C.allow_delta && !C.maintained && a != b && (int64_t)W * 16 < n_chunks;
    ctl->delta = dl;
    ctl->n_delta = C.n_delta + dl;
    // (the plane goes stale with the first full pass that rewrites a chunk)
    const int32_t dg = C.digest_ok && (dl || W <= 0);
    ctl->digest_ok = dg;
    ctl->n_digest = C.n_digest + (dl && dg);
    // The hit lists (the single-context loop): a delta iteration on the plane applies (a, b) from
    // the row a scan cached for it, and the slot is free again; without one the stream scans the
    // plane, which refills every slot.  The decision that clears digest_ok drops every list.
    if (lists) {
        int32_t use = -1;
        if (dl && dg)
            for (int j = 1; j < DIGEST_CAND; ++j)
                if (j < C.digest_cand && lists->pa[j] == a && lists->pb[j] == b) use = j;
        if (use >= 0) lists->pa[use] = -1;
        if (C.digest_ok && !dg)
            for (int j = 0; j < DIGEST_CAND; ++j) lists->pa[j] = -1;
        lists->use = use;
        ctl->n_scan = C.n_scan + (dl && dg && use < 0);
    }
    // (a delta iteration counts nothing: unscreened describes the full passes only)
    const int32_t uns = !dl && !C.maintained && bm &&
                        (bm - 1) + 2 * (unsigned long long)W < 0x10000ull;
    ctl->unscreened = uns;
    ctl->n_unscreened = C.n_unscreened + uns;
    res->bin_max = 0;
    res->best = 0;
    res->n_cand = 0;
    res->n_heavy = 0;
    res->replaced = 0;
    res->cold_dead = 0;
}

// Phase 0's check of the previous merge's replacement count: == W on the whole corpus (sharded:
// summed over the ranks in the exchange header); this corpus's own count is logged.
__device__ bool decide_check_replaced(LoopCtl *ctl, const LoopCtl &C, const Result &R,
                                      const unsigned long long *hdr, long long *log) {
    if (C.w < 0) return true;
    const unsigned long long total = C.sharded && hdr ? hdr[0] : R.replaced;
    if ((C.sharded && !hdr) || total != (unsigned long long)C.w) {
        ctl->status = LOOP_ERROR;
        ctl->err = 1;
        ctl->err_got = total;
        ctl->err_want = (unsigned long long)C.w;
        return false;
    }
    // (a sharded batch may open on the last batch's last merge: not in this log)
    if (C.n_done > 0) log[LOG_WORDS * (C.n_done - 1) + 3] = (long long)R.replaced;
    return true;
}

__global__ void k_decide(LoopCtl *ctl, Result *res, int2 *__restrict__ cand, int32_t *len16,
                         long long *log, int phase, const unsigned long long *__restrict__ tie_pos,
                         const unsigned long long *__restrict__ hdr = nullptr) {
    if (threadIdx.x != 0) return;
    // Snapshots of the control block and the Result (their loads issue together: one memory
    // latency instead of a chain of dependent ones); the fields are written back one by one.
    const LoopCtl C = *ctl;
    const Result R = *res;
    if (C.status != LOOP_RUN) return;
    const long long W = (long long)(R.best >> 17);
    const unsigned n = R.n_cand;
    auto to_host = [&]() {
        ctl->status = LOOP_HOST;
        ctl->n_host = C.n_host + 1;
    };
    int32_t a = -1, b = -1;
    if (phase == 0) {
        if (!decide_check_replaced(ctl, C, R, hdr, log)) return;
        ctl->w = -1;
        int vote = 0;
        const int prop = decide_propose(C, R, cand, vote);
        if (prop == 1 || prop == 2) {
            for (int j = 0; j < MAX_CAND; ++j) res->last[j] = 0;
            ctl->n_tie = C.n_tie + 1;
        }
        if (C.sharded) {
            ctl->tie = prop;
            ctl->vote = vote;
            ctl->pend_a = cand[0].x;
            ctl->pend_b = cand[0].y;
            return;
        }
        if (prop == 4) {
            ctl->status = LOOP_DONE;
            return;
        }
        if (prop == 5) {
            to_host();
            return;
        }
        if (prop != 3) {
            ctl->tie = prop;
            return;
        }
        a = cand[0].x;
        b = cand[0].y;
    } else {
        if (!C.tie) return;
        if (C.sharded) {
            ctl->tie = 0;
            if (tie_pos[MAX_CAND] || C.tie == 5) {   // some rank voted for the host path
                to_host();
                return;
            }
            if (C.tie == 4) {
                ctl->status = LOOP_DONE;
                return;
            }
        }
        if (C.tie == 3) {
            a = C.pend_a;
            b = C.pend_b;
        } else {
            unsigned long long pos[MAX_CAND];
            for (unsigned j = 0; j < n && j < (unsigned)MAX_CAND; ++j) pos[j] = tie_pos ? tie_pos[j] : R.last[j];
            int lone = 0;
            const int r3 = decide_r3(C.tie, n, pos, cand, a, b, lone);
            if (r3 == 1) {
                to_host();
                return;
            }
            if (lone) ctl->n_lone = C.n_lone + 1;
            if (C.tie == 1) ctl->n_tail = C.n_tail + 1;
            if (r3 == 2) {
                ctl->status = LOOP_ERROR;
                ctl->err = 2;
                return;
            }
            if (!C.sharded && !decide_room(C, R)) {
                to_host();
                return;
            }
        }
        ctl->tie = 0;
    }
    decide_commit(ctl, res, C, W, a, b, len16, log);
}

__device__ __forceinline__ void push_cand(Result *res, int2 *cand, int32_t a, int32_t b) {
    const unsigned int i = atomicAdd(&res->n_cand, 1u);
    if (i < CAND_CAP) cand[i] = make_int2(a, b);
}

// Collects every pair whose packed key equals the best (same W and same a+b).
__global__ void k_collect(const unsigned long long *__restrict__ hot_counts, ColdTable ct,
                          const int32_t *__restrict__ len16, int64_t max_length, Result *res,
                          int2 *cand, const LoopCtl *ctl = nullptr) {
    if (loop_off(ctl)) return;
    const unsigned long long best = res->best;
    if (best == 0) return;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < HOT_BINS) {
        const int32_t a = bin_a(tid), b = bin_b(tid);
        if (pair_ok(a, b, len16, max_length) && pack_key(hot_counts[tid], a, b) == best)
            push_cand(res, cand, a, b);
    }
    const uint32_t n = cold_used(ct);
    const unsigned long long w = best >> 17;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i0 = tid; i0 < n; i0 += COLD_ILP * stride) {
        unsigned long long v[COLD_ILP];   // (loads issued together, as in k_argmax_cold)
#pragma unroll
        for (int q = 0; q < COLD_ILP; ++q) {
            const uint32_t i = i0 + q * stride;
            v[q] = i < n ? ct.dcounts[i] : 0ull;
        }
#pragma unroll
        for (int q = 0; q < COLD_ILP; ++q) {
            if (v[q] != w) continue;   // (dense view; the key only for count matches)
            const uint32_t key = ct.dkeys[i0 + q * stride];
            const int32_t a = (int32_t)(key >> 16), b = (int32_t)(key & 0xFFFFu);
            if (pair_ok(a, b, len16, max_length) && pack_key(w, a, b) == best)
                push_cand(res, cand, a, b);
        }
    }
}

// ---- sharded selection over caller-provided (global) tables ----------------------------------
__global__ void k_export_cold(ColdTable ct, uint32_t *keys, unsigned long long *counts) {
    const uint32_t n = cold_used(ct);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        keys[i] = ct.dkeys[i];
        counts[i] = ct.dcounts[i];   // (a hole exports count 0)
    }
}

__global__ void k_argmax_list(const uint32_t *__restrict__ keys,
                              const unsigned long long *__restrict__ counts, int64_t n,
                              const int32_t *__restrict__ len16, int64_t max_length, Result *res) {
    unsigned long long best = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (!counts[i]) continue;   // (holes: count 0, key EMPTY)
        const int32_t a = (int32_t)(keys[i] >> 16), b = (int32_t)(keys[i] & 0xFFFFu);
        if (!pair_ok(a, b, len16, max_length)) continue;
        const unsigned long long k = pack_key(counts[i], a, b);
        best = k > best ? k : best;
    }
    best = wave_max_u64(best);
    if ((threadIdx.x & 63) == 0 && best) atomicMax(&res->best, best);
}

__global__ void k_collect_list(const unsigned long long *__restrict__ hot,
                               const uint32_t *__restrict__ keys,
                               const unsigned long long *__restrict__ counts, int64_t n,
                               const int32_t *__restrict__ len16, int64_t max_length, Result *res,
                               int2 *cand) {
    const unsigned long long best = res->best;
    if (best == 0) return;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (tid < HOT_BINS) {
        const int32_t a = bin_a((uint32_t)tid), b = bin_b((uint32_t)tid);
        if (pair_ok(a, b, len16, max_length) && pack_key(hot[tid], a, b) == best)
            push_cand(res, cand, a, b);
    }
    for (int64_t i = tid; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (counts[i] != (best >> 17)) continue;   // (holes: count 0)
        const int32_t a = (int32_t)(keys[i] >> 16), b = (int32_t)(keys[i] & 0xFFFFu);
        if (pair_ok(a, b, len16, max_length) && pack_key(counts[i], a, b) == best)
            push_cand(res, cand, a, b);
    }
}

// The maintained cold table before its refresh after the merge (a, b) -> c: the pairs with a side
// a or b lose their count (the refresh pass counts them again on the merged corpus; every other
// pair's count is unchanged by the merge).
// (device loop: the merge the next pass applies, from the LoopCtl)
__global__ void k_cold_invalidate(ColdTable ct, int32_t a, int32_t b, const LoopCtl *ctl = nullptr) {
    if (loop_off(ctl)) return;
    if (ctl) {
        a = ctl->a;
        b = ctl->b;
    }
    const uint32_t n = cold_used(ct);
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += COLD_ILP * stride) {
        uint32_t kk[COLD_ILP];   // (loads issued together, as in k_argmax_cold)
#pragma unroll
        for (int q = 0; q < COLD_ILP; ++q) {
            const uint32_t i = i0 + q * stride;
            kk[q] = i < n ? ct.dkeys[i] : EMPTY;
        }
#pragma unroll
        for (int q = 0; q < COLD_ILP; ++q) {
            const int32_t x = (int32_t)(kk[q] >> 16), y = (int32_t)(kk[q] & 0xFFFFu);
            if ((kk[q] != EMPTY) & ((x == a) | (x == b) | (y == a) | (y == b)))
                ct.dcounts[i0 + q * stride] = 0;   // (MODE_FUSED: its selections are full scans)
        }
    }
}


// MODE_INCR before the pass of the merge (a, b) -> c: every pair with a side a or b loses its
// count, in the maintained hot table (rows and columns a, b) and in the cold table.
__global__ void k_incr_invalidate(ColdTable ct, unsigned long long *__restrict__ hot, int32_t a,
                                  int32_t b, const LoopCtl *ctl = nullptr,
                                  const int32_t *__restrict__ len16 = nullptr,
                                  int64_t max_length = 0) {
    if (loop_off(ctl)) return;
    if (ctl) {
        a = ctl->a;
        b = ctl->b;
    }
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 4 * HOT) {   // hot bin (x, y) = y * 256 + x: column x = a / b, row y = a / b
        const int32_t m = (t >> 8) & 1 ? b : a, o = t & 255;
        if (m < HOT) hot[(t >> 9) ? hot_bin((uint32_t)m, (uint32_t)o) : hot_bin((uint32_t)o, (uint32_t)m)] = 0;
    }
    const uint32_t n = cold_used(ct);
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i0 = t; i0 < n; i0 += COLD_ILP * stride) {
        uint32_t kk[COLD_ILP];
#pragma unroll
        for (int q = 0; q < COLD_ILP; ++q) {
            const uint32_t i = i0 + q * stride;
            kk[q] = i < n ? ct.dkeys[i] : EMPTY;
        }
#pragma unroll
        for (int q = 0; q < COLD_ILP; ++q) {
            const int32_t x = (int32_t)(kk[q] >> 16), y = (int32_t)(kk[q] & 0xFFFFu);
            if ((kk[q] != EMPTY) & ((x == a) | (x == b) | (y == a) | (y == b))) {
                const uint32_t i = i0 + q * stride;
                const unsigned long long old = ct.dcounts[i];
                ct.dcounts[i] = 0;
                // a fall matters to the block maxima only where the entry may have been its
                // block's max (W at least the max's): that block is recomputed before the next
                // selection (the recount after this merge can only give it back less)
                const uint32_t blk = i / CB;
                const unsigned long long ko =
                    old && pair_ok(x, y, len16, max_length) ? pack_key(old, x, y) : 0ull;
                if (ko && ko >= ct.bmax[blk] && atomicExch(&ct.bdirty[blk], 1u) == 0u) {
                    const uint32_t k = atomicAdd(ct.n_blist, 1u);
                    if (k <= ct.mask / CB) ct.blist[k] = blk;
                }
            }
        }
    }
}

// Sharded maintained state, at the start of the next selection: the delta rows summed over the
// ranks (the recount of every pair the last merge (a, b) -> c touched, which k_incr_invalidate
// zeroed before the pass) into this rank's copy of the global tables, and the rows zeroed for the
// next merge.  Each touched pair has exactly one slot (delta_slot), so a hot bin gets one add.
__global__ void __launch_bounds__(256) k_apply_delta(unsigned long long *__restrict__ xchg,
                                                     unsigned long long *__restrict__ hot,
                                                     ColdTable ct, const LoopCtl *ctl) {
    if (loop_off(ctl) || ctl->w < 0) return;   // (w < 0: no merge applied yet in this batch)
    const int32_t a = ctl->a, b = ctl->b, c = ctl->c;
    const uint32_t n = (uint32_t)DELTA_ROWS * (uint32_t)(c + 1);   // other tokens <= c
    unsigned long long *d = xchg + XCHG_HDR;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned long long v = d[i];
        if (!v) continue;
        d[i] = 0;
        const uint32_t row = i % DELTA_ROWS;
        const int32_t o = (int32_t)(i / DELTA_ROWS);
        const int32_t m = row == 0 || row == 2 ? a : row == 1 || row == 3 ? b : c;
        const bool left = row == 0 || row == 1 || row == 4;   // (m, o), else (o, m)
        const int32_t x = left ? m : o, y = left ? o : m;
        if (((uint32_t)x | (uint32_t)y) < (uint32_t)HOT) hot[hot_bin((uint32_t)x, (uint32_t)y)] += v;
        else cold_add(ct, pair_key(x, y), v);
    }
}

// bpe_set_global_counts: (key, count) entries of every shard, duplicates summed, into the cleared
// cold table (holes, key EMPTY or count 0, skipped).
// The live claims of the cold table (a key, a count > 0) into dense arrays, in any order: the
// maintained table rebuilt from itself (bpe_engine.hip cold_rebuild) instead of from the corpus.
// (A wave-uniform loop: one atomic per wave for the output slots.)
__global__ void __launch_bounds__(256) k_cold_gather(ColdTable ct, uint32_t *__restrict__ keys,
                                                     unsigned long long *__restrict__ counts,
                                                     uint32_t *__restrict__ n_out) {
    const uint32_t n = cold_used(ct), lane = threadIdx.x & 63;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
        const uint32_t i = i0 + lane;
        uint32_t k = EMPTY;
        unsigned long long v = 0;
        if (i < n) {
            k = ct.dkeys[i];
            v = ct.dcounts[i];
        }
        const bool live = k != EMPTY && v != 0ull;
        const unsigned long long m = __ballot(live);
        if (!m) continue;
        uint32_t b = 0;
        if (lane == 0) b = atomicAdd(n_out, (uint32_t)__popcll(m));
        b = __shfl(b, 0);
        if (live) {
            const uint32_t j = b + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            keys[j] = k;
            counts[j] = v;
        }
    }
}

__global__ void k_load_cold(ColdTable ct, const uint32_t *__restrict__ keys,
                            const unsigned long long *__restrict__ counts, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        if (counts[i] && keys[i] != EMPTY) cold_add(ct, keys[i], counts[i]);
}

// MODE_INCR after the pass: sums the G slabs' rows (+ their spill, zeroed here) and adds each
// nonzero count to its pair in the maintained tables.  A block owns 32 row dwords (64 counters):
// its 8 lane groups each sum every 8th slab, eight loads in flight, then combine in LDS.
constexpr int RR_COLS = 32;
__global__ void __launch_bounds__(256)
k_reduce_rows(const uint32_t *__restrict__ partials, int G, unsigned long long *__restrict__ rspill,
              unsigned long long *__restrict__ hot, ColdTable ct, int32_t a, int32_t b, int32_t c,
              const LoopCtl *ctl = nullptr, unsigned long long *__restrict__ delta = nullptr,
              const unsigned long long *__restrict__ rep = nullptr) {
    __shared__ uint32_t s_lo[8][RR_COLS], s_hi[8][RR_COLS];
    if (loop_off(ctl)) return;
    if (ctl) {
        a = ctl->a;
        b = ctl->b;
        c = ctl->c;
    }
    // (sharded: the exchange header carries this shard's replacement count, summed with the rows)
    if (delta && rep && blockIdx.x == 0 && threadIdx.x == 0) delta[0] = *rep;
    const int vl = incr_vlim(c);
    const int d0 = blockIdx.x * RR_COLS;   // first of the block's dwords (4 rows x INCR_RLIM / 2)
    const int row = d0 / (INCR_RLIM / 2);
    if (row >= 4 || 2 * (d0 % (INCR_RLIM / 2)) >= vl || (a == b && (row & 1))) return;
    const int col = threadIdx.x & (RR_COLS - 1), grp = threadIdx.x / RR_COLS;
    uint32_t lo = 0, hi = 0;
    const uint32_t *p = partials + d0 + col;
    int g = grp;
    for (; g + 56 < G; g += 64) {
        uint32_t v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = p[(size_t)(g + 8 * q) * HIST_WORDS];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            lo += v[q] & 0xFFFFu;
            hi += v[q] >> 16;
        }
    }
    for (; g < G; g += 8) {
        const uint32_t v = p[(size_t)g * HIST_WORDS];
        lo += v & 0xFFFFu;
        hi += v >> 16;
    }
    s_lo[grp][col] = lo;
    s_hi[grp][col] = hi;
    __syncthreads();
    if (grp != 0) return;
    for (int q = 1; q < 8; ++q) {
        lo += s_lo[q][col];
        hi += s_hi[q][col];
    }
    const int wi = (d0 + col) % (INCR_RLIM / 2);
    if (2 * wi >= vl) return;
    const int32_t m = (row & 1) ? b : a;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int idx = 2 * wi + h;
        const uint32_t ci = (uint32_t)(row * INCR_RLIM + idx);
        const unsigned long long n = (unsigned long long)(h ? hi : lo) + rspill[ci];
        rspill[ci] = 0;
        if (!n) continue;
        const int32_t x = row < 2 ? m : idx, y = row < 2 ? idx : m;
        Sink k;
        k.hot = hot;
        k.ct = ct;
        k.delta = delta;
        k.ma = a;
        k.mb = b;
        k.mc = c;
        incr_global_add(k, x, y, n);
    }
}

// ---------------------------------------------------------------------------------------------
// K3 tie pass (rule R3): last counted occurrence (slot + 1) of up to MAX_CAND tied pairs on the
// current corpus, with exact X X parity (carry from k_runs).  Same streaming structure as k_step:
// a 6-slot register ring, each chunk checked once the next chunk's first token (its last slot's
// right-hand neighbour) has arrived.  Per chunk and candidate: four compares of a packed
// (token, right neighbour) word; the positions are worked out only in chunks that match.
// ---------------------------------------------------------------------------------------------
struct TieArgs {
    const int32_t *ids;
    int64_t n_chunks, cpr;
    int R;
    int n_cand;                  // host-driven passes (the device loop reads res->n_cand)
    const RegionCarry *carry;
    const int2 *cand;            // the candidates (a, b), at most MAX_CAND
    Result *res;
    const LoopCtl *ctl;          // device loop: run only when ctl->tie is set
};

struct TieState {
    int32_t prev;     // last live token before the chunk
    int32_t par;      // its run-offset parity (valid when it is an X X candidate's token)
    int32_t n;        // candidates
    uint32_t xx;      // bit j: candidate j is an X X pair
    uint32_t key[MAX_CAND];   // candidate j as a packed (a, b) word (wave-uniform registers)
    int32_t pos[MAX_CAND];    // region slot + 1 of the last counted occurrence (0: none)
};

// Checks one chunk (w.len > 0) at chunk index c of the region; nxt = the first live token after it.
// Every candidate costs four compares per chunk (the loops are unrolled, so keys and positions
// stay in registers); only chunks that hold a candidate work out positions.
__device__ __forceinline__ void tie_chunk(const Chunk &w, int32_t nxt, int c, int lane,
                                          TieState &ts) {
    const int32_t r3 = from_next(w.t[0], nxt);
    const uint32_t k0 = pack_pair(w.t[0], w.t[1]), k1 = pack_pair(w.t[1], w.t[2]),
                   k2 = pack_pair(w.t[2], w.t[3]), k3 = pack_pair(w.t[3], r3);
    const uint32_t kl_key = pack_pair_s(w.last, nxt);   // the last live slot's pair
    const int kl = w.len - 1;
    uint32_t hit = 0;
#pragma unroll
    for (int j = 0; j < MAX_CAND; ++j) {
        if (j < ts.n) {
            const uint32_t key = ts.key[j];
            const unsigned long long m = __ballot(k0 == key) | __ballot(k1 == key) |
                                         __ballot(k2 == key) | __ballot(k3 == key);
            hit |= (uint32_t)((m != 0ull) | (kl_key == key)) << j;
        }
    }
    int par[4] = {0, 0, 0, 0};
    int have_par = 0;
    if (hit) {
        // rare: the chunk holds a candidate.  Partial chunks keep the pairs whose right-hand slot
        // is live (slot < kl) and add the last slot's pair; X X candidates keep even run offsets.
        const int part = w.len < CHUNK;
        const unsigned long long L0 = part ? lanes_upto(kl, 0) : ~0ull,
                                 L1 = part ? lanes_upto(kl, 1) : ~0ull,
                                 L2 = part ? lanes_upto(kl, 2) : ~0ull,
                                 L3 = part ? lanes_upto(kl, 3) : ~0ull;
        unsigned long long Q0 = ~0ull, Q1 = ~0ull, Q2 = ~0ull, Q3 = ~0ull;
        if (hit & ts.xx) {
            bool start[4];
            run_parity(w.t, w.len, ts.prev, ts.par, lane, par, start);
            have_par = 1;
            Q0 = __ballot(par[0] == 0);
            Q1 = __ballot(par[1] == 0);
            Q2 = __ballot(par[2] == 0);
            Q3 = __ballot(par[3] == 0);
        }
        const unsigned long long bit = 1ull << (kl >> 2);
#pragma unroll
        for (int j = 0; j < MAX_CAND; ++j) {
            if ((hit >> j) & 1u) {
                const uint32_t key = ts.key[j];
                unsigned long long M0 = __ballot(k0 == key) & L0, M1 = __ballot(k1 == key) & L1,
                                   M2 = __ballot(k2 == key) & L2, M3 = __ballot(k3 == key) & L3;
                if (part & (kl_key == key)) {
                    switch (kl & 3) {
                    case 0: M0 |= bit; break;
                    case 1: M1 |= bit; break;
                    case 2: M2 |= bit; break;
                    default: M3 |= bit; break;
                    }
                }
                if ((ts.xx >> j) & 1u) {
                    // X X: only even run offsets count (core.ts:285-290)
                    M0 &= Q0;
                    M1 &= Q1;
                    M2 &= Q2;
                    M3 &= Q3;
                }
                // highest matching slot of the chunk
                int best = -1;
                if (M0) best = max(best, 4 * (63 - __builtin_clzll(M0)) + 0);
                if (M1) best = max(best, 4 * (63 - __builtin_clzll(M1)) + 1);
                if (M2) best = max(best, 4 * (63 - __builtin_clzll(M2)) + 2);
                if (M3) best = max(best, 4 * (63 - __builtin_clzll(M3)) + 3);
                ts.pos[j] = best >= 0 ? c * CHUNK + best + 1 : ts.pos[j];
            }
        }
    }
    // the parity of the last token matters only while it continues an X X candidate's run
    int par_last = 0;
    if (ts.xx) {
        uint32_t need = 0;
#pragma unroll
        for (int j = 0; j < MAX_CAND; ++j)
            need |= (uint32_t)((ts.key[j] >> 16) == (uint32_t)w.last) << j;
        if (need & ts.xx) {
            if (!have_par) {
                bool start[4];
                run_parity(w.t, w.len, ts.prev, ts.par, lane, par, start);
            }
            par_last = bcast(pick4(par, kl & 3), kl >> 2);
        }
    }
    ts.prev = w.last;
    ts.par = par_last;
}

// Tail mode of the tie pass (device loop, no X X candidate): the last TIE_TAIL_CHUNKS chunks, two
// per wave, each chunk on its own (an X Y pair needs no run context, only the next live token).
// The last occurrence of a candidate found there is its last occurrence in the corpus; a candidate
// not found there occurs only earlier, so it wins if it is the only one missing (k_decide).
constexpr int TIE_TAIL_PER_WAVE = 2;

// One wave's share of the tie pass: n candidates cand[0 .. n) (any memory), over the corpus tail
// window (tail) or the wave's region; the last positions go to A.res->last[j] (atomicMax).
__device__ __forceinline__ void tie_body(const TieArgs &A, int n, int tail, const int2 *cand) {
    const int lane = threadIdx.x & 63;
    const int r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    TieState ts;
    ts.n = min(n, MAX_CAND);
    ts.xx = 0;
#pragma unroll
    for (int j = 0; j < MAX_CAND; ++j) {
        ts.pos[j] = 0;
        // unused slots get a key no chunk word has (slot values >= 0xFF01 in both halves)
        const int2 cj = j < ts.n ? cand[j] : make_int2(-1, -1);
        ts.key[j] = __builtin_amdgcn_readfirstlane(pack_pair_s(cj.x, cj.y));
        ts.xx |= (uint32_t)((j < ts.n) & (cj.x == cj.y)) << j;
    }
    ts.xx = __builtin_amdgcn_readfirstlane(ts.xx);
    if (tail) {
        const int64_t win = (int64_t)gridDim.x * 4 * TIE_TAIL_PER_WAVE;
        const int64_t cw = max((int64_t)0, A.n_chunks - win) + (int64_t)r * TIE_TAIL_PER_WAVE;
        if (cw >= A.n_chunks) return;
        ts.prev = NONE;
        ts.par = 0;
        const int4 *v4 = reinterpret_cast<const int4 *>(A.ids);
        for (int q = 0; q < TIE_TAIL_PER_WAVE; ++q) {
            const int64_t c = cw + q;
            if (c >= A.n_chunks) break;
            const int4 v = v4[c * 64 + lane];
            Chunk w;
            w.t[0] = v.x;
            w.t[1] = v.y;
            w.t[2] = v.z;
            w.t[3] = v.w;
            finish_load(w);
            if (w.len == 0) continue;
            // the first live token after the chunk (SEP past the corpus end)
            int32_t nxt = SEP;
            for (int64_t q2 = c + 1; q2 < A.n_chunks; ++q2) {
                const int32_t f = __builtin_amdgcn_readfirstlane(A.ids[q2 * CHUNK]);
                if (f >= SEP) {
                    nxt = f;
                    break;
                }
            }
            tie_chunk(w, nxt, q, lane, ts);
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < MAX_CAND; ++j)
                if (j < ts.n && ts.pos[j])
                    atomicMax(&A.res->last[j], (unsigned long long)(cw * CHUNK + ts.pos[j]));
        }
        return;
    }
    if (r >= A.R) return;
    const int64_t c0 = (int64_t)r * A.cpr;
    const int64_t c1 = min(c0 + A.cpr, A.n_chunks);
    const int nc = (int)(c1 > c0 ? c1 - c0 : 0);
    if (nc == 0) return;
    const RegionCarry rc = A.carry[r];
    ts.prev = rc.prev_tok;
    ts.par = (int32_t)(rc.carry_off & 1) ^ 1;   // the token before the region (if linked)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<int32_t *>(A.ids) + c0 * CHUNK, 0, nc * CHUNK * 4, 0x00020000);
    const int lo = lane * 16;
    auto load = [&](Chunk &q, int c) __attribute__((always_inline)) {
        const auto x = __builtin_amdgcn_raw_buffer_load_b128(rs, lo, c * (CHUNK * 4), BPE_LOAD_AUX);
        q.t[0] = (int)x[0];
        q.t[1] = (int)x[1];
        q.t[2] = (int)x[2];
        q.t[3] = (int)x[3];
    };
    int pc = 0;   // chunk index of the pending chunk
    // the ring of k_step: chunk c+RING-2 loads into the slot chunk c-2 freed
    auto stage = [&](Chunk &cur, Chunk &prv, Chunk &fre, int c) __attribute__((always_inline)) {
        load(fre, c + RING - 2);
        if (c < nc) {
            finish_load(cur);
        } else {
            cur.first = TOMB;
            cur.len = 0;
            cur.last = NONE;
        }
        if (cur.len) {
            if (prv.len) tie_chunk(prv, cur.first, pc, lane, ts);
            pc = c;
        } else {
            cur = prv;   // rare: hand the pending chunk on
        }
    };
    Chunk S[RING];
    static_for<0, RING - 2>([&](auto i) __attribute__((always_inline)) { load(S[i], i); });
    S[RING - 1].len = 0;
    for (int c = 0; c < nc; c += RING) {
        static_for<0, RING>([&](auto I) __attribute__((always_inline)) {
            constexpr int i = decltype(I)::value;
            stage(S[i], S[(i + RING - 1) % RING], S[(i + RING - 2) % RING], c + i);
        });
    }
    if (S[RING - 1].len) tie_chunk(S[RING - 1], rc.next_tok, pc, lane, ts);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < MAX_CAND; ++j)
            if (j < ts.n && ts.pos[j])
                atomicMax(&A.res->last[j], (unsigned long long)(c0 * CHUNK + ts.pos[j]));
    }
}

__global__ void __launch_bounds__(256) k_tie(TieArgs A) {
    int n = A.n_cand;
    int tail = 0;
    if (A.ctl) {
        const int tie = A.ctl->tie;
        if (A.ctl->status != LOOP_RUN || (tie != 1 && tie != 2)) return;
        n = (int)A.res->n_cand;
        tail = tie == 1;
        // (a sharded corpus's tail window lies on the last rank: the others find nothing there)
        if (tail && A.ctl->sharded && !A.ctl->last_rank) return;
    }
    tie_body(A, n, tail, A.cand);
}

// The single-corpus device loop's selection tail in one launch (k_decide phase 0, k_tie, k_decide
// phase 1).  Without a tie, block 0 decides alone and the other blocks return at once: a
// device-wide ticket costs one same-address atomic per block, which the memory side serialises
// (1024 of them took 62 us, an iteration's whole selection budget).  With a tie (2 to MAX_CAND
// candidates and an R3 proposal), every block takes the same proposal from the same snapshot of
// the control block, the Result and the candidates (nothing writes them until every block has
// taken its ticket), scans for rule R3, and the last block to finish (the ticket) commits the
// decision with the positions every block left.  `ticket` is zero between launches.
// (the kernel's argument block is not passed on by reference: that pinned it to the stack and cost
// k_tie_fused 45 registers and 64 bytes of scratch)
__device__ void fused_commit(LoopCtl *ctl, Result *res, int64_t n_chunks, const LoopCtl &C,
                             const Result &R, const int2 *sc, int prop, int32_t *len16,
                             long long *log, DigestLists *lists) {
    if (!decide_check_replaced(ctl, C, R, nullptr, log)) return;
    ctl->w = -1;
    if (prop == 4) {
        ctl->status = LOOP_DONE;
        return;
    }
    if (prop == 5) {
        ctl->status = LOOP_HOST;
        ctl->n_host = C.n_host + 1;
        return;
    }
    int32_t a = sc[0].x, b = sc[0].y;
    if (prop != 3) {
        const unsigned n = R.n_cand;
        unsigned long long pos[MAX_CAND];
        for (unsigned j = 0; j < n; ++j) {
            pos[j] = __hip_atomic_load(&res->last[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            res->last[j] = 0;   // (for the next tie)
        }
        ctl->n_tie = C.n_tie + 1;
        int lone = 0;
        const int r3 = decide_r3(prop, n, pos, sc, a, b, lone);
        if (r3 == 1) {
            ctl->status = LOOP_HOST;
            ctl->n_host = C.n_host + 1;
            return;
        }
        if (lone) ctl->n_lone = C.n_lone + 1;
        if (prop == 1) ctl->n_tail = C.n_tail + 1;
        if (r3 == 2) {
            ctl->status = LOOP_ERROR;
            ctl->err = 2;
            return;
        }
    }
    decide_commit(ctl, res, C, (long long)(R.best >> 17), a, b, len16, log, n_chunks, lists);
}

__global__ void __launch_bounds__(256) k_tie_fused(TieArgs A, int32_t *len16, long long *log,
                                                   unsigned int *ticket, DigestLists *lists) {
    __shared__ LoopCtl sC;
    __shared__ Result sR;
    __shared__ int2 sc[MAX_CAND];
    __shared__ int s_prop;
    __shared__ bool s_last;
    if (threadIdx.x == 0) {
        int prop = 0;
        // (blocks other than 0 look further only when a tie pass is possible; a late block that
        // finds block 0's decision already made returns here too: the status or n_cand changed)
        const unsigned nc = blockIdx.x ? __hip_atomic_load(&A.res->n_cand, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT) : 2u;
        if (nc >= 2 && nc <= (unsigned)MAX_CAND) {
            sC = *A.ctl;
            sR = *A.res;
            const unsigned n = min(sR.n_cand, (unsigned)MAX_CAND);
            for (unsigned j = 0; j < n; ++j) sc[j] = A.cand[j];
            int vote = 0;
            prop = sC.status == LOOP_RUN ? decide_propose(sC, sR, sc, vote) : 0;
            if (blockIdx.x && prop != 1 && prop != 2) prop = 0;
        }
        s_prop = prop;
    }
    __syncthreads();
    const int prop = s_prop;
    if (prop == 0) return;   // (the batch has ended, or block 0 decides alone)
    if (prop != 1 && prop != 2) {
        if (threadIdx.x == 0) fused_commit(const_cast<LoopCtl *>(A.ctl), A.res, A.n_chunks, sC, sR, sc, prop, len16, log, lists);   // (block 0 only)
        return;
    }
    tie_body(A, (int)sR.n_cand, prop == 1, sc);
    // (every wave's position atomics complete at agent scope before the block takes its ticket)
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) s_last = grid_last(ticket);
    __syncthreads();
    if (!s_last || threadIdx.x != 0) return;
    __threadfence();
    fused_commit(const_cast<LoopCtl *>(A.ctl), A.res, A.n_chunks, sC, sR, sc, prop, len16, log, lists);
}

// Sharded loop: this shard's last tie positions as corpus-wide ones (rank << 40 | position; 0:
// none), and this rank's vote for the host path at [MAX_CAND], for the all-reduce(MAX) that
// follows.  One thread per slot.
constexpr int RANK_SHIFT = 40;
constexpr int TIE_WORDS = 32;   // include/bpe.h BPE_TIE_WORDS
static_assert(TIE_WORDS > MAX_CAND, "tie exchange: positions + vote");
__global__ void k_tie_export(const LoopCtl *ctl, const Result *res, unsigned long long *tie_pos,
                             int rank) {
    const int j = threadIdx.x;
    if (j >= TIE_WORDS) return;
    const bool run = ctl->status == LOOP_RUN;
    const int tie = ctl->tie;
    unsigned long long v = 0;
    if (j < MAX_CAND) {
        if (run && (tie == 1 || tie == 2) && res->last[j])
            v = ((unsigned long long)rank << RANK_SHIFT) | res->last[j];
    } else if (j == MAX_CAND) {
        v = run && ctl->vote ? 1 : 0;
    }
    tie_pos[j] = v;
}

// ---------------------------------------------------------------------------------------------
// Compaction (rare): moves every region's live slots to a dense prefix of a fresh buffer.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) k_scan_live(const RegionSum *__restrict__ s, int R,
                                                    int64_t *__restrict__ out_off,
                                                    unsigned long long *total) {
    __shared__ int64_t part[1024];
    const int per = (R + 1023) / 1024;
    const int t = threadIdx.x;
    int64_t acc = 0;
    for (int i = 0; i < per; ++i) {
        const int r = t * per + i;
        if (r < R) acc += s[r].n_live;
    }
    part[t] = acc;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        int64_t o = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += o;
        __syncthreads();
    }
    int64_t run = part[t] - acc;
    for (int i = 0; i < per; ++i) {
        const int r = t * per + i;
        if (r < R) {
            out_off[r] = run;
            run += s[r].n_live;
        }
    }
    if (t == 1023) *total = (unsigned long long)part[1023];
}

__global__ void __launch_bounds__(256) k_compact(const int32_t *__restrict__ ids, int64_t n_chunks,
                                                 int64_t cpr, int R,
                                                 const int64_t *__restrict__ out_off,
                                                 int32_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int64_t c0 = (int64_t)r * cpr;
    const int64_t c1 = min(c0 + cpr, n_chunks);
    const int4 *v4 = reinterpret_cast<const int4 *>(ids);
    int64_t o = out_off[r];
    for (int64_t c = c0; c < c1; ++c) {
        const View w = make_view(v4[c * 64 + lane]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * lane + e < w.len) out[o + 4 * lane + e] = w.t[e];
        o += w.len;
    }
}

// ---------------------------------------------------------------------------------------------
// Sample index: where every sample ends, for reading back single samples (the rows a merge
// changed, db/core.ts:399-417).  One wave per region, as k_compact.  k_census counts a region's
// live tokens and sample terminators, k_scan_pair turns both into region offsets, and k_sep_emit
// writes, per terminator in corpus order, its slot and the live tokens before it.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t wave_sum64(int64_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ void __launch_bounds__(256) k_census(const int32_t *__restrict__ ids, int64_t n_chunks,
                                                int64_t cpr, int R, int64_t *__restrict__ live,
                                                int64_t *__restrict__ seps) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int64_t c0 = (int64_t)r * cpr;
    const int64_t c1 = min(c0 + cpr, n_chunks);
    const int4 *v4 = reinterpret_cast<const int4 *>(ids);
    int64_t nl = 0, ns = 0;
    for (int64_t c = c0; c < c1; ++c) {
        const View w = make_view(v4[c * 64 + lane]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = 4 * lane + e < w.len;
            nl += in && w.t[e] >= 0;
            ns += in && w.t[e] == SEP;
        }
    }
    nl = wave_sum64(nl);
    ns = wave_sum64(ns);
    if (lane == 0) {
        live[r] = nl;
        seps[r] = ns;
    }
}

// Exclusive prefix sums of two arrays of R <= 1024 * k entries, in place.  One block of 1024.
__global__ void __launch_bounds__(1024) k_scan_pair(int R, int64_t *__restrict__ a,
                                                    int64_t *__restrict__ b) {
    __shared__ int64_t pa[1024], pb[1024];
    const int per = (R + 1023) / 1024;
    const int t = threadIdx.x;
    int64_t sa = 0, sb = 0;
    for (int i = 0; i < per; ++i) {
        const int r = t * per + i;
        if (r < R) {
            sa += a[r];
            sb += b[r];
        }
    }
    pa[t] = sa;
    pb[t] = sb;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int64_t oa = t >= d ? pa[t - d] : 0, ob = t >= d ? pb[t - d] : 0;
        __syncthreads();
        pa[t] += oa;
        pb[t] += ob;
        __syncthreads();
    }
    int64_t ra = pa[t] - sa, rb = pb[t] - sb;
    for (int i = 0; i < per; ++i) {
        const int r = t * per + i;
        if (r < R) {
            const int64_t va = a[r], vb = b[r];
            a[r] = ra;
            b[r] = rb;
            ra += va;
            rb += vb;
        }
    }
}

__global__ void __launch_bounds__(256) k_sep_emit(const int32_t *__restrict__ ids, int64_t n_chunks,
                                                  int64_t cpr, int R,
                                                  const int64_t *__restrict__ live_pre,
                                                  const int64_t *__restrict__ sep_pre,
                                                  int64_t n_samples,
                                                  int64_t *__restrict__ slot_end,
                                                  int64_t *__restrict__ live_end) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int64_t c0 = (int64_t)r * cpr;
    const int64_t c1 = min(c0 + cpr, n_chunks);
    const int4 *v4 = reinterpret_cast<const int4 *>(ids);
    const unsigned long long below = (1ull << lane) - 1;
    int64_t ol = live_pre[r], os = sep_pre[r];
    for (int64_t c = c0; c < c1; ++c) {
        const View w = make_view(v4[c * 64 + lane]);
        bool L[4], S[4];
        int bl = 0, bs = 0, tl = 0, ts = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = 4 * lane + e < w.len;
            L[e] = in && w.t[e] >= 0;
            S[e] = in && w.t[e] == SEP;
            const unsigned long long ml = __ballot(L[e]), ms = __ballot(S[e]);
            bl += __popcll(ml & below);
            bs += __popcll(ms & below);
            tl += __popcll(ml);
            ts += __popcll(ms);
        }
        // slots of lane l precede those of lane l+1: live tokens / terminators before (lane, e)
        // are those of the lanes below plus this lane's slots 0..e-1
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (S[e]) {
                const int64_t k = os + bs;
                if (k < n_samples) {
                    slot_end[k] = c * CHUNK + 4 * lane + e;
                    live_end[k] = ol + bl;
                }
            }
            bl += L[e];
            bs += S[e];
        }
        ol += tl;
        os += ts;
    }
}

// Packs slot ranges [src[k], src[k] + len[k]) to dst + dst_off[k], for reading chosen samples
// back in one copy.  One block per range.
__global__ void __launch_bounds__(256) k_gather_ranges(const int32_t *__restrict__ ids,
                                                       const int64_t *__restrict__ src,
                                                       const int64_t *__restrict__ len,
                                                       const int64_t *__restrict__ dst_off,
                                                       int64_t n, int32_t *__restrict__ dst) {
    for (int64_t k = blockIdx.x; k < n; k += gridDim.x) {
        const int32_t *s = ids + src[k];
        int32_t *d = dst + dst_off[k];
        for (int64_t i = threadIdx.x; i < len[k]; i += 256) d[i] = s[i];
    }
}

// Dead tail + tail tags of the last chunk after a dense write of live_slots slots.  One block of
// CHUNK threads.
__global__ void __launch_bounds__(CHUNK) k_seal(int32_t *__restrict__ ids, int64_t live_slots) {
    const int len = (int)(live_slots % CHUNK);
    if (len == 0) return;
    int32_t *p = ids + (live_slots / CHUNK) * CHUNK;
    const int t = threadIdx.x;
    const int32_t last = p[len - 1];
    if (t >= len) p[t] = (t & 1) ? TOMB_ODD : TOMB;
    __syncthreads();
    if (t == 0) p[CHUNK - 1] = tail_tag(len, last);
}

// ---------------------------------------------------------------------------------------------
// K5 ingest: latin1 bytes -> first-appearance positions + histogram, then expansion to slots.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_byte_stats(const uint8_t *__restrict__ bytes, int64_t n,
                                                    unsigned long long *__restrict__ first,
                                                    unsigned long long *__restrict__ hist) {
    __shared__ unsigned long long s_first[256];
    __shared__ unsigned int s_hist[256];
    s_first[threadIdx.x] = ~0ull;
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t per_block = 1 << 16;
    for (int64_t base = (int64_t)blockIdx.x * per_block; base < n;
         base += (int64_t)gridDim.x * per_block) {
        const int64_t end = min(base + per_block, n);
        for (int64_t i = base + threadIdx.x; i < end; i += 256) {
            const uint8_t b = bytes[i];
            atomicAdd(&s_hist[b], 1u);
            if ((unsigned long long)i < s_first[b]) atomicMin(&s_first[b], (unsigned long long)i);
        }
        __syncthreads();
        if (s_hist[threadIdx.x]) {
            atomicAdd(&hist[threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);
            s_hist[threadIdx.x] = 0;
        }
        __syncthreads();
    }
    if (s_first[threadIdx.x] != ~0ull) atomicMin(&first[threadIdx.x], s_first[threadIdx.x]);
}

__global__ void k_expand_latin1(const uint8_t *__restrict__ bytes, int64_t n, int64_t sample_bytes,
                                const int32_t *__restrict__ map, int32_t *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / sample_bytes;
        out[i + s] = map[bytes[i]];
        if ((i + 1) % sample_bytes == 0 || i + 1 == n) out[i + s + 1] = SEP;
    }
}

}  // namespace bpe
