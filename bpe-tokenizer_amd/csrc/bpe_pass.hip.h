// bpe_pass.hip.h — CDNA4 (gfx950) kernels of the BPE merge-training hot path: the constants, the
// layout structs, the streaming pass and the digest stream (bpe_kernels.hip.h holds the rest).
//
// Reference semantics: /root/reference/core.ts findNextMerge (247-326) and applyMerge (332-360);
// order-free restatement in SURVEY.md Appendix A (R1-R5).
//
// Corpus layout in HBM: one int32 slot array cut into 256-slot *chunks*.  Every sample (one
// `corpus_in_code` element, core.ts:106) is its token ids followed by one SEP (-1).  Every chunk is
// LEFT-PACKED: its live slots (tokens and SEPs) come first, dead slots (TOMB, -2) fill the tail.
// The logical corpus is the concatenation of the chunks' live prefixes.  A merge therefore never
// moves data between chunks: it rewrites only the chunks that contain a match (1 KiB each).  A
// spare all-SEP chunk follows the last chunk so "first slot of the next chunk" loads stay in range.
//
// Work decomposition: the chunks are cut into R contiguous *regions*; one wave (64 lanes) owns one
// region and streams it chunk by chunk (lane L holds slots 4L..4L+3 as one int4: a 1 KiB fully
// coalesced load per wave-instruction).  Inside a region the state that crosses chunks (the open
// run of equal tokens behind the `X X X` skip rule, core.ts:285-290) lives in wave-uniform
// registers.  Across regions nothing is shared during a pass: each wave writes a RegionSum and
// k_runs stitches the boundaries (the pair straddling each boundary, runs crossing regions, and
// the carries the next pass needs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace bpe {

constexpr int32_t SEP = -1;                 // sample separator (live slot, never in a pair)
constexpr int32_t TOMB = -2;                // dead slot in a chunk tail
constexpr int32_t NONE = -3;                // "no token" (register sentinel only)
// Tail tag of a partial chunk (every stored value < SEP is a dead slot): slot 255 holds
// LEN_TAG - len - ((last + 3) << 8), i.e. its live length and its last live slot (NONE when empty)
// in one value, read with one v_readlane.
constexpr int32_t LEN_TAG = -16;
// Dead slots alternate TOMB (even slots) and TOMB_ODD (odd slots), so no dead slot equals its
// neighbour: equal-neighbour masks need no liveness masking.
constexpr int32_t TOMB_ODD = -4;

__host__ __device__ __forceinline__ int32_t tail_tag(int len, int32_t last) {
    return LEN_TAG - len - (int32_t)((uint32_t)(last + 3) << 8);
}
constexpr int CHUNK = 256;                  // slots per wave-chunk (64 lanes x int4)
#ifndef BPE_WAVES
#define BPE_WAVES 16
#endif
constexpr int WAVES_PER_WG = BPE_WAVES;
// Register ring of the streaming passes: RING chunks per wave (k_step: loads issued RING - 3
// chunks ahead, k_tie: RING - 2).  Depth 2 already streams at 5.8 TB/s and 12 at 6.06
// (tools/probe/stream_probe.hip).  With the round-end overflow screen, depth 6 times best over
// the full C3 run: k_step 0.760 ms against 0.767 (5), 0.795 (7), 0.83 (8, 9).
#ifndef BPE_RING
#define BPE_RING 6
#endif
constexpr int RING = BPE_RING;
static_assert(RING >= 5, "ring depth");
// (the overflow screen runs once per ring round: 16 waves x RING chunks x 256 adds must stay
// below the 49152 adds of headroom above 0x4000, see lds_sweep)
static_assert(WAVES_PER_WG * RING * 256 < 49152,
              "ring depth vs the LDS overflow screen");
// How far ahead k_step loads: chunk c + LEAD at stage c, into the slot of chunk c + LEAD - RING.
// At stage c the wave holds chunks c - 1 (count), c (apply) and c + 1 (its first token), so every
// slot of a chunk <= c - 2 is free: LEAD <= RING - 2.
#ifndef BPE_LEAD
#define BPE_LEAD (BPE_RING - 3)
#endif
constexpr int LEAD = BPE_LEAD;
static_assert(LEAD >= 2 && LEAD <= RING - 2, "load lead");

// Cache-policy bits of the streaming passes' corpus loads (buffer_load aux: 0 plain, 2 nt).  A
// pass streams 4 GB, far past the caches, so the loads are non-temporal: 6.15 -> 7.0 TB/s for
// this access pattern (tools/probe/stream_probe2.hip), k_step 2.6 % faster.
#ifndef BPE_LOAD_AUX
#define BPE_LOAD_AUX 2
#endif
// f(integral_constant<I>) for I = 0 .. N-1, unrolled in the source (the ring's slot indices must be
// compile-time constants, or the ring is moved to scratch memory)
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}
constexpr int WG = WAVES_PER_WG * 64;       // one workgroup per CU (LDS-bound)
constexpr int MAX_WG = 256;                 // one per CU on MI355X
constexpr int MAX_REGIONS = MAX_WG * WAVES_PER_WG;
constexpr int HOT = 256;                    // ids < HOT form the dense LDS histogram
constexpr int HOT_BINS = HOT * HOT;
constexpr int SKETCH_BINS = 16384;          // count sketch of the cold pairs (an id >= HOT)
constexpr int TABLE_BINS = HOT_BINS + SKETCH_BINS;   // [0, 64K) exact hot pairs, then the sketch
// Hot pair (a, b) sits at table bin b * 256 + a: the order of the LDS table's 16-bit counters
// (dword (b << 7) | (a >> 1), half a & 1), so the reduction writes the table contiguously.
__host__ __device__ constexpr uint32_t hot_bin(uint32_t a, uint32_t b) { return (b << 8) | a; }
__host__ __device__ constexpr int32_t bin_a(uint32_t bin) { return (int32_t)(bin & 255); }
__host__ __device__ constexpr int32_t bin_b(uint32_t bin) { return (int32_t)(bin >> 8); }
constexpr int HIST_WORDS = TABLE_BINS / 2;  // two 16-bit counters per LDS dword: 160 KiB, all of it
constexpr int HEAVY_WORDS = SKETCH_BINS / 32;        // bitmap of sketch buckets needing exact counts
// What a streaming pass does with the pairs it sees: the pair table, exact counts of the cold
// pairs in heavy sketch buckets, or nothing (apply-only replay: restoreMerge, batch encoding).
// MODE_FUSED: a merge pass that also refreshes the maintained cold table (the table counts plus
// MODE_EXACT's refresh of the pairs with a side in {ma, mb, mc}, in one stream of the corpus)
// MODE_INCR: incremental counts.  Both tables are maintained: the merge
// (ma, mb) -> mc changes only the counts of the pairs with a side in {ma, mb, mc} (every other pair
// keeps its occurrences and its run parity), so those are zeroed before the pass and the pass
// counts only them, into dense per-token LDS rows (no 128 KiB histogram of every pair).
enum CountMode { MODE_TABLE = 0, MODE_EXACT = 1, MODE_NONE = 2, MODE_FUSED = 3, MODE_INCR = 4 };
constexpr int MAX_CAND = 16;                // candidates resolved per tie pass
constexpr int CAND_CAP = 65536;             // candidates collected per iteration
constexpr uint32_t EMPTY = 0xFFFFFFFFu;

// What one pass learned about its region of the (post-merge) corpus.  Live slots only.
struct RegionSum {
    int64_t n_live;      // live slots (tokens + SEPs)
    int64_t lead_len;    // length of the first run (the whole region when uniform)
    int32_t first_tok;   // first live slot value (NONE when the region is empty)
    int32_t last_tok;    // last live slot value
    int32_t uniform;     // the region is one single run
    int32_t trail_odd;   // the last run's length is odd (meaningful when not uniform)
};

// Boundary facts k_runs derives for the NEXT pass over the same corpus.
struct RegionCarry {
    int64_t carry_off;   // parity of the run offset of the region's first live token (0 unless
                         // its run began in an earlier region)
    int32_t prev_tok;    // last live slot before the region (SEP at the corpus start)
    int32_t next_tok;    // first live slot after the region (SEP at the corpus end)
};

// Sparse pair table for pairs with an id >= HOT: open addressing on key = a << 16 | b.
struct ColdTable {
    // open-addressing hash of the claimed pairs: slot = (key << 32) | dense index, EMPTY64 = free
    unsigned long long *slots;
    // the dense arrays, entry i = the i-th claimed index (claim order): every scan (argmax,
    // collect, invalidate, export) streams these coalesced, and the counts live here, so a scan
    // never gathers hashed slots.  A claim that loses its slot race leaves a hole (key EMPTY,
    // count 0).  dcounts[i] == 0 for every i >= *n_used (zeroed with the table).  Counts are
    // 64-bit: one pair of a 16 GiB shard can occur more than 2^32 times (JS numbers in the
    // reference's Map are exact to 2^53, core.ts:280-292).
    uint32_t *dkeys;
    unsigned long long *dcounts;
    uint32_t *n_used;
    uint32_t *overflow;  // set when a probe sequence wraps the table or the dense arrays fill up
    uint32_t mask;       // slots - 1 (= dense capacity - 1)
    uint32_t shift;
    // Block maxima of the dense view (the device loop's maintained selection, k_select_maint):
    // per CB entries the best packed key, exact except in the blocks flagged dirty (listed in
    // blist, n_blist entries); sel_n0 = n_used at the last selection, dead = the dead claims
    // found by the last full scan.  n_blist, sel_n0 and dead follow n_used and overflow in the
    // same flags array.
    unsigned long long *bmax;
    uint32_t *bdirty, *blist;
    uint32_t *n_blist, *sel_n0, *dead;
    uint32_t *n_recomputed;   // block maxima recomputed by incremental selections (a statistic)
};
// entries per block of the cold table's block maxima
constexpr uint32_t CB = 1024;

struct Result {
    unsigned long long best;             // packed (W << 17) | (0x1FFFF - c_index), 0 = none
    unsigned int n_cand;                 // pairs sharing the best packed key (list in `cand`)
    unsigned int n_heavy;                // sketch buckets that need exact cold counts
    unsigned long long last[MAX_CAND];   // R3: slot + 1 of the last counted occurrence
    unsigned long long replaced;         // apply: replacement count
    unsigned long long cold_flags;       // k_argmax_cold: (overflow << 32) | n_used of the cold table
    unsigned long long cold_dead;        // k_argmax_cold: claims whose pair is gone (count 0, key set)
    // k_reduce_table: the largest bin of the table it wrote, plus one (0: unknown); consumed and
    // cleared by the next decision (LoopCtl::unscreened)
    unsigned long long bin_max;
};

// Device-resident mergeUntil loop (core.ts:367-384): the decision of each iteration stays in HBM and
// the next pass reads it from there, so a batch of iterations runs without a host round trip.
// Every kernel of the loop returns at once when status != LOOP_RUN (the batch has ended early).
enum LoopStatus { LOOP_RUN = 0, LOOP_DONE = 1, LOOP_HOST = 2, LOOP_ERROR = 3 };

struct LoopCtl {
    int32_t status;
    int32_t tie;          // the candidates wait for the tie pass (rule R3)
    int32_t a, b, c;      // the merge the next pass applies
    int32_t next_id;      // id of the next new token (token_table.length, core.ts:315)
    int64_t w;            // its weight (-1: no merge applied yet in this batch)
    int64_t n_done;       // merges decided in this batch (entries of the log)
    int64_t min_weight;   // after the core.ts:256 default
    int32_t n_tie;        // tie passes run in this batch
    // one rank of a sharded corpus: W is global (this shard's replacement count is logged, not
    // checked), ties take the full pass and their positions come from the all-reduced tie table
    int32_t sharded;
    int32_t max_id;       // ids below it fit the vocabulary (BPE_MAX_VOCAB): at it the batch ends
    int32_t n_tail;       // ties decided from the tail window alone (k_tie tail mode)
    int32_t n_lone;       // ... of which by the lone candidate missing from the window
    int32_t n_host;       // iterations handed to the host path (LOOP_HOST: 0 or 1 per batch)
    // the maintained cold-pair table (skewed corpora): selection reads it instead of the sketch,
    // each merge pass refreshes it (MODE_FUSED); cold_cap = its capacity (for the fill limits)
    int32_t maintained;
    // sharded: this rank holds the corpus tail (the tie pass's tail window scans it alone)
    int32_t last_rank;
    unsigned long long cold_cap;
    // sharded: this rank asks the others to hand the iteration to the host (its copy of the
    // maintained tables is too full, or dead, or the merge's refresh might not fit: facts that
    // differ between ranks, so they travel through the tie all-reduce(MAX) before any decision)
    int32_t vote;
    // sharded: the single candidate chosen before the vote (tie == 3)
    int32_t pend_a, pend_b;
    // LOOP_ERROR: 1 the replacement count (sum) != W, 2 a tie pass found no occurrence
    int32_t err;
    // (err 1: the count found and the W expected)
    unsigned long long err_got, err_want;
    // The pass applying this merge cannot take any LDS counter of any workgroup to 16 bits, so it
    // counts with adds that return nothing and no overflow screen (k_step_loop<MODE_TABLE>).  Set
    // by the decision when (largest bin of the pre-merge table) + 2 W < 2^16: a pair's count never
    // grows by a merge (a b -> c only removes occurrences of pairs next to a or b, and runs of X
    // only shrink), the new pairs (x, c) and (c, y) number W each at most, and a workgroup's LDS
    // count of a bin is at most the bin's count over the whole corpus (pairs across regions go
    // to the spill; a run's segments count at most the run's floor(L / 2)).  A sharded rank bounds
    // its own shard's counts with its own largest bin and the global W (W >= the shard's count of
    // the pair).  0 (screened) in the maintained state and for the first pass of a batch.
    int32_t unscreened;
    int32_t n_unscreened;   // decisions that set it, in this batch
    // The delta form of a table-state iteration (single-context loop): the merge is applied by an
    // apply-only stream (k_apply_loop) that lists the chunks it rewrites, and the table is kept by
    // the deltas of the merge's sites (k_site_delta) instead of a recount.  Set by the decision
    // for a merge of two distinct ids in fewer than 1/16 of the chunks, when the host allows it
    // (allow_delta: the table state, BPE_DELTA != 0); every kernel of the form not taken returns
    // at once.  err 3: the table's bin of (a, b) did not hold W.
    int32_t delta;
    int32_t allow_delta;
    int32_t n_delta;        // decisions that set it, in this batch
    // The digest plane (one byte per slot, digest_of) matches the corpus: a delta iteration then
    // finds its sites through the plane (digest_body) instead of streaming the int32 slots.  Set
    // by the host at the batch start, cleared by the decision that commits a merge with W > 0 in
    // the full form (the full pass rewrites chunks without the plane): stale for the rest of the
    // batch.
    int32_t digest_ok;
    unsigned long long delta_chunks;   // chunks listed by the delta iterations of this batch
    unsigned long long digest_hits;    // chunks the digest stream took to the exact path
    int32_t n_digest;       // delta iterations on the plane, in this batch
    int32_t n_scan;         // ... of which streamed the plane (the others took a cached hit list)
    // candidate pairs a stream of the plane answers for, 1 .. DIGEST_CAND (the host's, per batch:
    // BPE_DIGEST_CAND); at 1 every delta iteration on the plane scans
    int32_t digest_cand;
    int32_t pad_;
};

// The hit lists of the digest stream (include/bpe.h BPE_DIGEST_CAND: candidate slots).  One
// stream of the plane answers "can this chunk hold a site?" for the decided pair (slot 0, applied
// at once, never stored) and for up to DIGEST_CAND - 1 predicted pairs, whose answers are kept:
// one bit per chunk, region r's row of slot j at rows[(r * DIGEST_CAND + j) * wpr], wpr =
// ceil(cpr / 32) words.  A merge only replaces two adjacent tokens by a fresh id and never moves
// a token to another chunk, so the chunks that hold a site of (p, q) after any number of merges
// are among those flagged for (p, q) at the scan: a cached row stays a superset (a chunk with no
// site left is one more false hit) while the plane stays valid and the geometry unchanged.
// The state lives outside the LoopCtl (re-sent at every batch start) and survives a batch exactly
// when the plane does (digest_begin_batch clears it with every build).
constexpr int DIGEST_CAND = 8;
static_assert(DIGEST_CAND >= 1 && DIGEST_CAND <= 8, "candidate slots of a plane stream");
struct DigestLists {
    int32_t pa[DIGEST_CAND], pb[DIGEST_CAND];   // slot j holds the row of (pa, pb); pa < 0: free
    // this iteration (set by the decision): the slot whose row the merge is applied from, or -1:
    // stream the plane
    int32_t use;
    int32_t pad_;
    // the best key of each block of 256 hot bins (bins b * 256 + a of one b), left by the last
    // k_reduce_table: the scan predicts the next merges from the largest of them
    unsigned long long bkey[HOT];
};



// Merge log entry of the device loop: (a, b, W, this corpus's replacement count).
constexpr int LOG_WORDS = 4;

__device__ __forceinline__ bool loop_off(const LoopCtl *ctl) {
    return ctl && ctl->status != LOOP_RUN;
}

__device__ __forceinline__ unsigned long long pack_key(unsigned long long w, int32_t a, int32_t b) {
    return w ? ((w << 17) | (unsigned long long)(0x1FFFF - (a + b))) : 0ull;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        unsigned long long o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ int wave_incl_sum(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// DPP wavefront shifts by one lane (a VALU modifier: no LDS crossbar round trip, unlike
// __shfl_*).  from_next: lane i gets lane i+1's x, lane 63 gets fill.  from_prev: lane i gets lane
// i-1's x, lane 0 gets fill.
__device__ __forceinline__ int32_t from_next(int32_t x, int32_t fill) {
    return __builtin_amdgcn_update_dpp(fill, x, 0x130, 0xF, 0xF, false);   // wave_shl:1
}

__device__ __forceinline__ int32_t from_prev(int32_t x, int32_t fill) {
    return __builtin_amdgcn_update_dpp(fill, x, 0x138, 0xF, 0xF, false);   // wave_shr:1
}

// A (token, right neighbour) pair as one word: (low 16 bits of x) << 16 | (low 16 bits of y), one
// v_perm.  Token ids are < 55296; SEP, TOMB and TOMB_ODD have low halves >= 0xFFFC, so they never
// alias one.  A tail tag (slot 255 of a partial chunk) can: code comparing packed pairs must not
// trust a match involving slot 255 of a partial chunk.
__device__ __forceinline__ uint32_t pack_pair(int32_t x, int32_t y) {
    return __builtin_amdgcn_perm((uint32_t)x, (uint32_t)y, 0x05040100u);
}

// The same packing on wave-uniform values, as scalar arithmetic.
__device__ __forceinline__ uint32_t pack_pair_s(int32_t x, int32_t y) {
    return ((uint32_t)x << 16) | ((uint32_t)y & 0xFFFFu);
}

constexpr unsigned long long EMPTY64 = ~0ull;

__device__ __forceinline__ void cold_add(const ColdTable &ct, uint32_t key, unsigned long long inc) {
    uint32_t h = (key * 0x9E3779B1u) >> ct.shift;
    uint32_t mine = EMPTY;   // the dense index this call reserved (at its first free slot)
    for (uint32_t probes = 0; probes <= ct.mask; ++probes) {
        unsigned long long v =
            __hip_atomic_load(&ct.slots[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v == EMPTY64) {
            if (mine == EMPTY) {
                mine = atomicAdd(ct.n_used, 1u);
                if (mine > ct.mask) {
                    atomicOr(ct.overflow, 1u);
                    return;
                }
                ct.dkeys[mine] = key;
            }
            v = atomicCAS(&ct.slots[h], EMPTY64, ((unsigned long long)key << 32) | mine);
            if (v == EMPTY64) {
                atomicAdd(&ct.dcounts[mine], inc);
                return;
            }
        }
        if ((uint32_t)(v >> 32) == key) {
            atomicAdd(&ct.dcounts[(uint32_t)v], inc);
            if (mine != EMPTY) ct.dkeys[mine] = EMPTY;   // (lost the race for this key: a hole)
            return;
        }
        h = (h + 1) & ct.mask;
    }
    atomicOr(ct.overflow, 1u);
}

// Claimed dense entries to scan: a claim past the capacity bumps n_used before it sees the
// overflow, so n_used alone can point past the dense arrays.
__device__ __forceinline__ uint32_t cold_used(const ColdTable &ct) {
    const uint32_t n = *ct.n_used;
    return n <= ct.mask ? n : ct.mask + 1;
}

// entries per thread and sweep of the cold-table scans (their loads in flight together)
constexpr int COLD_ILP = 8;

__device__ __forceinline__ uint32_t pair_key(int32_t x, int32_t y) {
    return ((uint32_t)x << 16) | (uint32_t)y;
}

// Sketch hash of a cold pair: h = y * SKETCH_K + (x >> 1) (one v_mad_u32_u24), sketch dword
// h & 0x1FFF = (y * K + x / 2) mod 8192 (K odd), its half x & 1.  Consecutive ids land in
// consecutive bins, so the merged tokens (allocated in sequence) spread evenly.  (Round 5: y
// multiplied, x halved, so that the fast path forms 4 h from the x << 1 its hot address uses and
// the sketch address in one more bit operation, pair_slot.  Round 4's x * K + y; a bucket of the
// ids' low bits alone, with no multiply, collided: profiles/r05_ab_sketch_low.txt.)
constexpr uint32_t SKETCH_K = 0x19B1u;
__device__ __forceinline__ uint32_t sketch_hash(int32_t x, int32_t y) {
    // (written out: left to itself the compiler may widen this to a 64-bit multiply-add)
    uint32_t h;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(h) : "v"(y), "s"(SKETCH_K), "v"((uint32_t)x >> 1));
    return h;
}

// Sketch bucket: the dword from the hash, the half from x (as for hot pairs, see below).
__device__ __forceinline__ uint32_t sketch_bucket(int32_t x, int32_t y) {
    return ((sketch_hash(x, y) & 0x1FFFu) << 1) | ((uint32_t)x & 1u);
}

// Table index of a pair: its exact bin when both ids are hot, else its sketch bucket.
// Branch-free: both forms are computed and selected.
__device__ __forceinline__ int table_index(int32_t x, int32_t y) {
    const uint32_t hot = hot_bin((uint32_t)x, (uint32_t)y);
    const uint32_t cold = HOT_BINS + sketch_bucket(x, y);
    return ((uint32_t)x | (uint32_t)y) < (uint32_t)HOT ? (int)hot : (int)cold;
}

// Where a pass's pair occurrences go.  MODE_TABLE: the per-workgroup LDS table (exact hot bins +
// cold sketch buckets, 16-bit counters) with a global u64 spill.  MODE_EXACT: exact counts of the
// cold pairs whose sketch bucket is marked heavy, into the sparse table; the rest is ignored.
// MODE_FUSED: the hot bins (no sketch: the maintained cold table counts the cold pairs) plus the
// cold pairs with a side in {ma, mb, mc}.
struct Sink {
    uint32_t *hist;                  // LDS table (MODE_TABLE)
    unsigned long long *spill;       // global u64 [TABLE_BINS]
    ColdTable ct;
    const uint32_t *heavy;           // LDS bitmap [HEAVY_WORDS] (MODE_EXACT)
    // MODE_FUSED (ma >= 0): the maintained cold table's refresh after the merge (ma, mb) -> mc,
    // every cold pair with a side in {ma, mb, mc}, whatever its bucket (heavy is then unused)
    int32_t ma, mb, mc;
    // MODE_INCR: the maintained hot table (global u64 [HOT_BINS]) and the rows' spill
    // (global u64 [4 * INCR_RLIM])
    unsigned long long *hot;
    unsigned long long *rspill;
    // MODE_INCR on a rank of a sharded corpus: the touched pairs' counts go to this shard's delta
    // rows (summed over the ranks, then added to every rank's copy of the global tables by
    // k_apply_delta) instead of straight into the tables
    unsigned long long *delta;
    // HOT_BYTES in a VGPR: the third operand of the fast path's sketch address (pair_slot)
    uint32_t hot_bytes_v;
};

// Delta rows of the sharded maintained state (include/bpe.h BPE_XCHG_*): the pairs a merge
// (a, b) -> c can change, at HDR + 6 * other + row, rows in precedence order (a, .) (b, .)
// (., a) (., b) (c, .) (., c).  Every touched pair has a side in {a, b, c}: each maps to one slot.
constexpr int XCHG_HDR = 8;
constexpr int DELTA_ROWS = 6;
constexpr int XCHG_WORDS = XCHG_HDR + DELTA_ROWS * 55296;   // BPE_MAX_VOCAB
static_assert(XCHG_WORDS >= XCHG_HDR + TABLE_BINS, "exchange buffer holds the table too");

__device__ __forceinline__ uint32_t delta_slot(int32_t x, int32_t y, int32_t a, int32_t b,
                                                int32_t c) {
    int row, other;
    if (x == a) { row = 0; other = y; }
    else if (x == b) { row = 1; other = y; }
    else if (y == a) { row = 2; other = x; }
    else if (y == b) { row = 3; other = x; }
    else if (x == c) { row = 4; other = y; }
    else { row = 5; other = x; }
    return (uint32_t)(XCHG_HDR + DELTA_ROWS * other + row);
}

template <int MODE>
__device__ __forceinline__ bool exact_wanted(const Sink &k, int32_t x, int32_t y) {
    const int idx = table_index(x, y);
    if (idx < HOT_BINS) return false;
    if (k.ma >= 0)
        return (x == k.ma) | (x == k.mb) | (x == k.mc) | (y == k.ma) | (y == k.mb) | (y == k.mc);
    const int b = idx - HOT_BINS;
    return (k.heavy[b >> 5] >> (b & 31)) & 1u;
}

// MODE_INCR: is (x, y) a valid pair with a side in {ma, mb, mc}?
__device__ __forceinline__ bool incr_touched(const Sink &k, int32_t x, int32_t y) {
    return ((x | y) >= 0) & ((x == k.ma) | (x == k.mb) | (x == k.mc) | (y == k.ma) | (y == k.mb) |
                             (y == k.mc));
}

// MODE_INCR: n occurrences of a touched pair straight into the maintained tables.
__device__ __forceinline__ void incr_global_add(const Sink &k, int32_t x, int32_t y,
                                                unsigned long long n) {
    if (k.delta) {
        atomicAdd(&k.delta[delta_slot(x, y, k.ma, k.mb, k.mc)], n);
        return;
    }
    if (((uint32_t)x | (uint32_t)y) < (uint32_t)HOT)
        atomicAdd(&k.hot[hot_bin((uint32_t)x, (uint32_t)y)], n);
    else
        cold_add(k.ct, ((uint32_t)x << 16) | (uint32_t)y, n);
}

// Adds n occurrences of (x, y) from outside the LDS table (boundary pairs, resolved runs).
template <int MODE>
__device__ __forceinline__ void add_pairs_global(const Sink &k, int32_t x, int32_t y,
                                                 unsigned long long n) {
    if (n == 0 || MODE == MODE_NONE) return;
    if (MODE == MODE_INCR) {
        if (incr_touched(k, x, y)) incr_global_add(k, x, y, n);
        return;
    }
    if (MODE == MODE_TABLE || MODE == MODE_FUSED) atomicAdd(&k.spill[table_index(x, y)], n);
    if (MODE != MODE_TABLE && exact_wanted<MODE>(k, x, y))
        cold_add(k.ct, pair_key(x, y), n);
}

// The LDS table: 16-bit counters, two per dword.
//  - hot pair (x, y), both < 256: dword (y << 7) | (x >> 1), half x & 1, i.e. byte address
//    ((x << 1) & 0x1FC) | (y << 9) and increment 1 << ((x << 4) & 16): five VALU operations, the
//    half chosen by a bit the shift amount already carries;
//  - sketch bucket b of a cold pair: dword HOT_BINS / 2 + (b >> 1), half b & 1, with
//    b = ((hash & 0x1FFF) << 1) | (x & 1): the dword from the hash, the half from x, so both
//    classes share the increment.
// Overflow: the adds return the dword they found.  Each wave ORs the returns of a ring round
// (RING chunks) together and, at the round's end, when some half it touched stood at >= 0x4000,
// sweeps the table (lds_sweep): every half >= 0x4000 gives its top two bits to the global u64
// spill (indexed by the bin, 2 * dword + half) with one atomic AND, race-free against the other
// waves' adds and sweeps.  No half can pass 0xFFFF: it receives at most 49152 adds between
// reaching 0x4000 and the first sweep, and every one of those adds comes from a wave that saw
// it at >= 0x4000 and sweeps at the end of its round, after at most RING chunks of at most 256
// adds to any one counter: 16 waves x 7 x 256 = 28672.
constexpr uint32_t HOT_BYTES = HOT_BINS * 2;   // 128 KiB

__device__ __forceinline__ uint32_t hot_addr(int32_t x, int32_t y) {
    return (((uint32_t)x << 1) & 0x1FCu) | ((uint32_t)y << 9);
}

// 1 << ((x & 1) * 16): the shift operand's low five bits of x << 4 are exactly that
__device__ __forceinline__ uint32_t hot_inc(int32_t x) {
    return 1u << (((uint32_t)x << 4) & 31u);
}

// byte address of sketch dword HOT_BINS / 2 + (h & 0x1FFF)
__device__ __forceinline__ uint32_t cold_addr(uint32_t h) { return HOT_BYTES | ((h & 0x1FFFu) << 2); }


__device__ __forceinline__ uint32_t *lds_word(const Sink &k, uint32_t addr) {
    return reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(k.hist) + addr);
}

// The halves a sweep moves: bits 14 and 15 of each.
constexpr uint32_t SWEEP_BITS = 0xC000C000u;

__device__ __forceinline__ void sweep_word(uint32_t *hist, unsigned long long *spill, int i,
                                           uint32_t w) {
    if (!(w & SWEEP_BITS)) return;
    const uint32_t old = atomicAnd(&hist[i], ~SWEEP_BITS);
    const uint32_t lo = old & 0xC000u, hi = (old >> 16) & 0xC000u;
    if (lo) atomicAdd(&spill[2 * i], (unsigned long long)lo);
    if (hi) atomicAdd(&spill[2 * i + 1], (unsigned long long)hi);
}

// One wave's sweep of LDS dwords [begin, end) (begin a multiple of 4): each half >= 0x4000 moves
// its top two bits to spill[2 * dword + half].  (Rare: no counter of the uniform C3 corpus ever
// reaches 0x4000 in a workgroup.)
__device__ __attribute__((noinline)) void lds_sweep(uint32_t *hist, unsigned long long *spill,
                                                    int lane, int begin, int end) {
    const int end4 = begin + ((end - begin) & ~3);
    for (int i = begin + 4 * lane; i < end4; i += 4 * 64) {
        const uint4 v = *reinterpret_cast<const uint4 *>(hist + i);
        sweep_word(hist, spill, i, v.x);
        sweep_word(hist, spill, i + 1, v.y);
        sweep_word(hist, spill, i + 2, v.z);
        sweep_word(hist, spill, i + 3, v.w);
    }
    for (int i = end4 + lane; i < end; i += 64) sweep_word(hist, spill, i, hist[i]);
}

// MODE_EXACT: each workgroup first sums its cold-pair counts in an LDS hash (open addressing,
// after the heavy bitmap; the table's LDS is free in that mode) and adds each distinct key to the
// global sparse table once at the end, so a skewed corpus's frequent cold pairs do not serialise
// on one global counter.  A key that finds no slot within LH_PROBES goes to the global table.
constexpr int LH_BITS = 14;
constexpr int LH_SLOTS = 1 << LH_BITS;   // (key, count) dword pairs: 128 KiB
constexpr int LH_PROBES = 8;
static_assert(HEAVY_WORDS + 2 * LH_SLOTS <= HIST_WORDS, "LDS cold hash does not fit");

__device__ __forceinline__ void lds_cold_add(const Sink &k, uint32_t key, uint32_t inc) {
    uint32_t *keys = k.hist + HEAVY_WORDS;
    uint32_t *cnt = keys + LH_SLOTS;
    uint32_t h = (key * 0x9E3779B1u) >> (32 - LH_BITS);
    for (int p = 0; p < LH_PROBES; ++p) {
        uint32_t kk = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (kk == EMPTY) kk = atomicCAS(&keys[h], EMPTY, key);   // (EMPTY: this lane claimed it)
        if (kk == EMPTY || kk == key) {
            atomicAdd(&cnt[h], inc);
            return;
        }
        h = (h + 1) & (LH_SLOTS - 1);
    }
    cold_add(k.ct, key, inc);
}

// MODE_FUSED's LDS hash: all of the sketch dwords (the sketch is not kept while the cold table is
// maintained), (key, count) x 4096.
constexpr int FH_BITS = 12;
constexpr int FH_SLOTS = 1 << FH_BITS;
constexpr int FH_BASE = HOT_BINS / 2;   // dword index of the first key
static_assert(FH_BASE + 2 * FH_SLOTS == HIST_WORDS, "fused LDS hash = the sketch's dwords");

__device__ __forceinline__ void lds_fused_add(const Sink &k, uint32_t key, uint32_t inc) {
    uint32_t *keys = k.hist + FH_BASE;
    uint32_t *cnt = keys + FH_SLOTS;
    uint32_t h = (key * 0x9E3779B1u) >> (32 - FH_BITS);
    for (int p = 0; p < LH_PROBES; ++p) {
        uint32_t kk = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (kk == EMPTY) kk = atomicCAS(&keys[h], EMPTY, key);
        if (kk == EMPTY || kk == key) {
            atomicAdd(&cnt[h], inc);
            return;
        }
        h = (h + 1) & (FH_SLOTS - 1);
    }
    cold_add(k.ct, key, inc);
}

// MODE_INCR's LDS: four rows of 16-bit counters indexed by the pair's other token, for the pairs
// (ma, y), (mb, y), (x, ma), (x, mb) in this order of precedence (each pair counts once), the
// other token below INCR_RLIM; then a hash of (key, count) dwords for everything else touched
// (the pairs of mc, and other tokens >= INCR_RLIM).  Overflow as in the hot table: the round's
// screen and lds_sweep over the rows' used part, to the global rspill rows.
constexpr int INCR_RLIM = 18432;                       // counters per row
constexpr int IH_SLOTS = 2048;
constexpr int IH_BASE = 4 * INCR_RLIM / 2;             // dword index of the hash keys
static_assert(IH_BASE + 2 * IH_SLOTS == HIST_WORDS, "MODE_INCR LDS layout");

// counters of a row in use: other tokens below the vocabulary size after the merge (mc + 1)
static_assert(INCR_RLIM % 2 == 0, "a row's counters pair up in dwords");
__device__ __forceinline__ int incr_vlim(int32_t mc) {
    const int v = (mc + 2) & ~1;
    return v < INCR_RLIM ? v : INCR_RLIM;
}

__device__ __forceinline__ void incr_hash_add(const Sink &k, uint32_t key, uint32_t inc) {
    uint32_t *keys = k.hist + IH_BASE;
    uint32_t *cnt = keys + IH_SLOTS;
    uint32_t h = (key * 0x9E3779B1u) >> (32 - 11);
    for (int p = 0; p < LH_PROBES; ++p) {
        uint32_t kk = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (kk == EMPTY) kk = atomicCAS(&keys[h], EMPTY, key);
        if (kk == EMPTY || kk == key) {
            atomicAdd(&cnt[h], inc);
            return;
        }
        h = (h + 1) & (IH_SLOTS - 1);
    }
    incr_global_add(k, (int32_t)(key >> 16), (int32_t)(key & 0xFFFFu), inc);
}

// One occurrence of a pair touched by the merge (incr_touched) into MODE_INCR's LDS.
__device__ __forceinline__ void incr_add(const Sink &k, int32_t x, int32_t y, uint32_t &seen) {
    int row, idx;
    if (x == k.ma) {
        row = 0;
        idx = y;
    } else if (x == k.mb) {
        row = 1;
        idx = y;
    } else if (y == k.ma) {
        row = 2;
        idx = x;
    } else if (y == k.mb) {
        row = 3;
        idx = x;
    } else {
        row = 4;
        idx = INCR_RLIM;
    }
    if (idx >= INCR_RLIM) {
        incr_hash_add(k, ((uint32_t)x << 16) | (uint32_t)y, 1u);
        return;
    }
    const uint32_t c = (uint32_t)(row * INCR_RLIM + idx);
    const uint32_t sh = (c & 1u) << 4;
    // (the round's overflow screen, as for the hot table: consumed at once, see count_pair)
    uint32_t old = atomicAdd(&k.hist[c >> 1], 1u << sh);
    asm volatile("" : "+v"(old));
    seen |= old;
}

// One counted occurrence of (x, y) (outside the streaming fast paths).
// (MODE_TABLE / MODE_FUSED: the dword the add found is ORed into `seen`, the wave's overflow
// screen; see lds_sweep)
template <int MODE, bool SCREEN = true>
__device__ __forceinline__ void count_pair(const Sink &k, int32_t x, int32_t y, uint32_t &seen) {
    if (MODE == MODE_NONE) return;
    if (MODE == MODE_INCR) {
        if (incr_touched(k, x, y)) incr_add(k, x, y, seen);
        return;
    }
    if (MODE == MODE_TABLE || MODE == MODE_FUSED) {
        const bool hot = ((uint32_t)x | (uint32_t)y) < (uint32_t)HOT;
        const uint32_t addr = hot ? hot_addr(x, y) : cold_addr(sketch_hash(x, y));
        // (MODE_FUSED keeps no sketch: its cold pairs go to the maintained table only)
        if (MODE == MODE_TABLE && !SCREEN) {
            atomicAdd(lds_word(k, addr), hot_inc(x));
        } else if (MODE == MODE_TABLE || hot) {
            // (consumed at once: a `seen` still in flight would make every later join wait for
            // all of the wave's LDS adds, the fast path's deferred ones included)
            uint32_t old = atomicAdd(lds_word(k, addr), hot_inc(x));
            asm volatile("" : "+v"(old));
            seen |= old;
        }
        if (MODE == MODE_FUSED && exact_wanted<MODE>(k, x, y)) lds_fused_add(k, pair_key(x, y), 1u);
    } else if (exact_wanted<MODE>(k, x, y)) {
        lds_cold_add(k, pair_key(x, y), 1u);
    }
}

// ---------------------------------------------------------------------------------------------
// A left-packed chunk as seen by one lane: slots k = 4*lane + e, live iff k < len.
// ---------------------------------------------------------------------------------------------
struct View {
    int32_t t[4];
    int len;
};

__device__ __forceinline__ View make_view(const int4 v) {
    View w;
    w.t[0] = v.x;
    w.t[1] = v.y;
    w.t[2] = v.z;
    w.t[3] = v.w;
    // chunks are left-packed, so len = number of non-TOMB slots (256 iff the last slot is live)
    if (__builtin_amdgcn_readlane(v.w, 63) >= SEP) {
        w.len = CHUNK;
    } else {
        w.len = (LEN_TAG - __builtin_amdgcn_readlane(v.w, 63)) & 255;
    }
    return w;
}

template <typename T>
__device__ __forceinline__ T pick4(const T (&a)[4], int e) {
    const T a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
    return e == 0 ? a0 : e == 1 ? a1 : e == 2 ? a2 : a3;
}

// c ? a : b on values (a conditional over two lvalues compiles to a select of their addresses,
// which pins arrays and structs in registers to scratch)
template <typename T>
__device__ __forceinline__ T sel(bool c, T a, T b) { return c ? a : b; }

// Broadcast of lane `src` (wave-uniform) through v_readlane.
__device__ __forceinline__ int32_t bcast(int32_t v, int src) {
    return __builtin_amdgcn_readlane(v, src);
}

__device__ __forceinline__ int64_t bcast64(int64_t v, int src) {
    const int32_t lo = __builtin_amdgcn_readlane((int32_t)(v & 0xFFFFFFFF), src);
    const int32_t hi = __builtin_amdgcn_readlane((int32_t)(v >> 32), src);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// Token at chunk index k (wave-uniform k), broadcast.
__device__ __forceinline__ int32_t view_at(const View &w, int k) {
    return bcast(pick4(w.t, k & 3), k >> 2);
}

// Neighbourhood of each live slot: partner = next live token (the pair's right side), prev.
struct Nbr {
    int32_t partner[4];
    bool live[4];
    bool eqn[4];   // live, non-SEP, equal to partner  (an X X pair starts here)
    bool eqp[4];   // live, non-SEP, equal to the previous live token (continues a run)
};

__device__ __forceinline__ void neighbours(const View &w, int32_t prev, int32_t nxt, int lane,
                                           Nbr &n) {
    const int32_t dn = from_next(w.t[0], nxt);
    const int32_t pm = from_prev(w.t[3], prev);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = 4 * lane + e;
        n.live[e] = k < w.len;
        const int32_t right = sel(e < 3, w.t[e < 3 ? e + 1 : 0], dn);
        n.partner[e] = (k + 1 < w.len) ? right : nxt;
        const int32_t left = sel(e == 0, pm, w.t[e > 0 ? e - 1 : 0]);
        n.eqp[e] = n.live[e] && w.t[e] >= 0 && w.t[e] == left;
        n.eqn[e] = n.live[e] && w.t[e] >= 0 && w.t[e] == n.partner[e];
    }
}

// Run-start scan over the live prefix: rs[e] = chunk index of the start of the run containing
// slot 4*lane+e, or -1 when that run began before the chunk.
__device__ __forceinline__ void run_starts(const Nbr &n, int lane, int rs[4]) {
    int lmax = -1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (n.live[e] && !n.eqp[e]) lmax = 4 * lane + e;
        rs[e] = lmax;
    }
    int incl = lmax;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int o = __shfl_up(incl, d);
        if (lane >= d) incl = o > incl ? o : incl;
    }
    int excl = __shfl_up(incl, 1);
    if (lane == 0) excl = -1;
#pragma unroll
    for (int e = 0; e < 4; ++e) rs[e] = max(rs[e], excl);
}

// Exact run offsets of the live slots (needed where X X pairs are matched / located exactly).
// prev_off = offset of the live token before the chunk (valid when slot 0 continues its run).
// Returns the offset of the last live slot (the next chunk's prev_off).
__device__ __forceinline__ int64_t run_offsets(const View &w, const Nbr &n, int lane,
                                               int64_t prev_off, int64_t (&off)[4]) {
    bool slow = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) slow |= n.eqn[e] && n.eqp[e];
    if (__ballot(slow) == 0ull) {
        // every X X slot starts its run (offset 0); a run reaching the next chunk starts at the
        // last live slot, so the carried offset is 0 whenever it is used
#pragma unroll
        for (int e = 0; e < 4; ++e) off[e] = 0;
        return 0;
    }
    int rs[4];
    run_starts(n, lane, rs);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = 4 * lane + e;
        off[e] = rs[e] >= 0 ? (int64_t)(k - rs[e]) : prev_off + 1 + k;
    }
    const int kl = w.len - 1;
    return bcast64(pick4(off, kl & 3), kl >> 2);
}

// ---------------------------------------------------------------------------------------------
// Chunk re-packing in registers (no LDS: it is all pair table).  Each kept slot moves left by
// D = the number of dropped slots before it, one binary digit of D per step, least significant
// first; that order never lands two slots on one position.  A slot travels as one dword:
// value+1 (17 bits) | D << 17 (8 bits) | kept << 25.  Returns the new live length.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int compact_chunk(int32_t (&val)[4], const bool (&keep)[4], int len,
                                             int lane) {
    const unsigned long long K0 = __ballot(keep[0]), K1 = __ballot(keep[1]),
                             K2 = __ballot(keep[2]), K3 = __ballot(keep[3]);
    const int total = __popcll(K0) + __popcll(K1) + __popcll(K2) + __popcll(K3);
    int kb = (int)(__builtin_amdgcn_mbcnt_hi((uint32_t)(K0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)K0, 0)) +
                   __builtin_amdgcn_mbcnt_hi((uint32_t)(K1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)K1, 0)) +
                   __builtin_amdgcn_mbcnt_hi((uint32_t)(K2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)K2, 0)) +
                   __builtin_amdgcn_mbcnt_hi((uint32_t)(K3 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)K3, 0)));
    constexpr uint32_t KEPT = 1u << 25;
    uint32_t pk[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t d = (uint32_t)(4 * lane + e - kb);
        pk[e] = keep[e] ? ((uint32_t)(val[e] + 1) | (d << 17) | KEPT) : 0u;
        kb += keep[e];
    }
    const int dmax = len - total;   // dropped live slots; dead slots all follow the live ones
    for (int sh = 1; sh <= dmax; sh <<= 1) {
        uint32_t nb[4];   // the slot sh positions to the right
        if (sh == 1) {
            nb[0] = pk[1];
            nb[1] = pk[2];
            nb[2] = pk[3];
            nb[3] = (uint32_t)from_next((int32_t)pk[0], 0);
        } else if (sh == 2) {
            nb[0] = pk[2];
            nb[1] = pk[3];
            nb[2] = (uint32_t)from_next((int32_t)pk[0], 0);
            nb[3] = (uint32_t)from_next((int32_t)pk[1], 0);
        } else {
            const int dl = sh >> 2;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t x = __shfl_down(pk[e], dl);
                nb[e] = sel(lane < 64 - dl, x, 0u);
            }
        }
        const uint32_t bit = (uint32_t)sh << 17;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool mv = (nb[e] & KEPT) && (nb[e] & bit);
            const bool stay = (pk[e] & KEPT) && !(pk[e] & bit);
            pk[e] = sel(mv, nb[e], sel(stay, pk[e], 0u));
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        val[e] = sel(4 * lane < total - e, (int32_t)(pk[e] & 0x1FFFFu) - 1, (e & 1) ? TOMB_ODD : TOMB);
    return total;
}

// ---------------------------------------------------------------------------------------------
// K1 (fused with K4): the streaming pass.
//
// One wave streams one region chunk by chunk through a 6-slot register ring (the loop is unrolled
// by 6, so every slot is a fixed set of registers and nothing is ever copied):
//   - the current chunk j is applied in place (merge passes), its right-hand neighbour being the
//     first live token of chunk j+1, already in the ring;
//   - the post-merge chunk before it (the ring slot of j-1) is counted, its right-hand neighbour
//     being the first post-merge token of chunk j;
//   - that slot is then refilled with chunk j+5.
// Empty chunks (rare: every token deleted) hand the pending chunk on to the next slot.
//
// Per-slot tests are vector compares whose results are wave masks (SGPR pairs); everything
// derived from them is scalar work.  Only the pair-table address arithmetic and the compares are
// vector instructions on the common path.
//
// X X pairs follow the reference's skip rule (core.ts:285-290): an X X pair counts iff its left
// slot sits at an even offset of its maximal run of X.  The wave carries the offset parity of the
// last token from chunk to chunk, and measures the region's first run from the region start as if
// nothing preceded it; k_runs adds what that assumption missed for runs that cross regions.  A
// chunk with no slot in the middle of a run of three or more (the common case) needs no parity:
// then every valid pair counts.
// ---------------------------------------------------------------------------------------------

// Registers of one ring slot: the lane's four slots + wave-uniform facts.
struct Chunk {
    int32_t t[4];
    int len;         // live slots (left-packed)
    int32_t first;   // slot 0 (dead when empty)
    int32_t last;    // last live slot (NONE when empty)
};

// Slot k (wave-uniform) broadcast from its lane.
__device__ __forceinline__ int32_t slot_at(const int32_t (&t)[4], int k) {
    const int l = k >> 2;
    switch (k & 3) {
    case 0: return bcast(t[0], l);
    case 1: return bcast(t[1], l);
    case 2: return bcast(t[2], l);
    default: return bcast(t[3], l);
    }
}

__device__ __forceinline__ bool lane_in(unsigned long long m) {
    return __builtin_amdgcn_inverse_ballot_w64(m);
}

// Lanes whose plane-e slot 4*lane + e lies below n.
__device__ __forceinline__ unsigned long long lanes_upto(int n, int e) {
    const int m = (n - e + 3) >> 2;
    return m >= 64 ? ~0ull : m <= 0 ? 0ull : ((1ull << m) - 1ull);
}

// Lanes whose t is one of ma, mb, mc: three compares straight into lane masks, OR'ed on the scalar
// unit.  (A ballot of the OR of the three compares made the compiler materialise the OR as a 0/1
// vector value and compare it again: two more VALU per token.)
__device__ __forceinline__ unsigned long long member3(int32_t t, int32_t ma, int32_t mb, int32_t mc) {
    return __ballot(t == ma) | __ballot(t == mb) | __ballot(t == mc);
}

// Wave-uniform facts of a freshly loaded chunk, from slot 255 (a live token, or the tail tag).
__device__ __forceinline__ void finish_load(Chunk &c, int32_t first) {
    c.first = first;
    const int32_t l3 = bcast(c.t[3], 63);
    const int32_t v = LEN_TAG - l3;
    const int live = l3 >= SEP;
    c.len = live ? CHUNK : (v & 255);
    c.last = live ? l3 : (v >> 8) - 3;
}
__device__ __forceinline__ void finish_load(Chunk &c) { finish_load(c, bcast(c.t[0], 0)); }

// Exact run-offset parity of every live slot (SEPs are runs of their own), and the run starts.
// prev = the live token before slot 0 (NONE: none), prev_par = the parity of its offset.
__device__ __forceinline__ void run_parity(const int32_t (&t)[4], int len, int32_t prev,
                                           int prev_par, int lane, int (&par)[4],
                                           bool (&start)[4]) {
    const int32_t l0 = from_prev(t[3], prev);
    int lmax = -1;
    int rs[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = 4 * lane + e;
        const int32_t left = sel(e == 0, l0, t[e > 0 ? e - 1 : 0]);
        start[e] = k < len && !(t[e] >= 0 && t[e] == left);
        if (start[e]) lmax = k;
        rs[e] = lmax;
    }
    int incl = lmax;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if (lane >= d) incl = o > incl ? o : incl;
    }
    int excl = __shfl_up(incl, 1);
    if (lane == 0) excl = -1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = 4 * lane + e;
        const int s = max(rs[e], excl);
        par[e] = s >= 0 ? ((k - s) & 1) : ((prev_par + 1 + k) & 1);
    }
}

// Count-side state of one region (wave-uniform).
struct Tally {
    int32_t n_live;      // live slots counted so far
    int32_t lead_len;    // length of the region's first run (once it has ended)
    int32_t prev;        // last live token counted (NONE before the first)
    int32_t par;         // run-offset parity of prev (the first run counts from the region start)
    int32_t first_tok;   // the region's first live token
    int32_t in_lead;     // every live token so far belongs to the region's first run
    uint32_t seen;       // (per lane) OR of the words the exact path's LDS adds returned
};

// LDS adds of one chunk's pairs (x[e], y[e]), then the overflow screen.  Per pair (11 VALU): the
// hot address (three operations: x << 1, y << 9, one bit operation), the sketch address (two:
// a multiply-add on x << 1, one bit operation), u = ~(x | y) (one, opaque to the compiler so both
// uses below read it as is), the class select (two), and the increment (three): hot_inc(x) for a
// valid pair, 0 when a side is negative (SEP, dead), with the validity bit (u's sign) as the value
// shifted.  Pairs with a cold side go to their sketch bucket (its half is also x & 1).
// FUSED (the maintained cold table counts the cold pairs): a cold pair adds 0 to a hot dword (its
// address masked into the hot table) instead of going to the sketch.
template <bool FUSED = false>
__device__ __forceinline__ void pair_slot(const Sink &k, int32_t x, int32_t y, uint32_t &addr,
                                          uint32_t &inc) {
    uint32_t u = ~((uint32_t)x | (uint32_t)y);
    asm("" : "+v"(u));
    if (FUSED) {
        const uint32_t hot = (((uint32_t)x << 1) & 0x1FCu) | ((uint32_t)y << 9);
        addr = hot & (HOT_BYTES - 4);
        inc = (uint32_t)(u >= 0xFFFFFF00u) << (((uint32_t)x << 4) & 31u);   // both ids < 256
    } else {
        // both addresses as (a & b) | c (v_bitop3 table 0xEA): the hot one from x << 1 and
        // y << 9; the sketch one from 4 h = y * 4K + (x << 1) (the sketch hash times 4: its
        // dword's byte offset in bits 2..14) and HOT_BYTES
        const uint32_t x2 = (uint32_t)x << 1;
        uint32_t hot, h4, cold;
        asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xea"
            : "=v"(hot) : "v"(x2), "s"(0x1FCu), "v"((uint32_t)y << 9));
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(h4) : "v"(y), "s"(4u * SKETCH_K), "v"(x2));
        asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xea" : "=v"(cold) : "v"(h4), "s"(0x7FFCu), "v"(k.hot_bytes_v));
        addr = sel(u >= 0xFFFFFF00u, hot, cold);   // both ids < 256
        inc = (u >> 31) << (((uint32_t)x << 4) & 31u);
    }
}

// The words a fast-path count's LDS adds returned (0 when the chunk took another path), and their
// byte addresses.  Each stage of a ring round keeps its own, and they are all screened together at
// the round's end, so the waves wait on LDS returns once per RING chunks, not once per chunk.
// (Screening each chunk's returns one stage later left the compiler a wait for every add still
// in flight at each stage: 5 % of the pass.)  The addresses let the screen sweep just the words
// its adds saw at >= 0x4000 (round 5; see screen_round).
struct Defer {
    uint32_t o[4];
    uint32_t a[4];
};

// The LDS adds of a fast-path chunk; their returned words and
// addresses go to df, screened at the end of the
// ring round (Returns), so no wave waits on its LDS atomics' return before then.
// SCREEN false (MODE_TABLE, when no LDS counter can reach 16 bits in this pass: see LoopCtl::
// unscreened): the adds return nothing, and no word is kept for a screen.
template <bool FUSED = false, bool SCREEN = true>
__device__ __forceinline__ void add_pairs(const int32_t (&x)[4], const int32_t (&y)[4],
                                          const Sink &k, Defer &df) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint32_t addr, inc;
        pair_slot<FUSED>(k, x[e], y[e], addr, inc);
        if (SCREEN) {
            df.o[e] = atomicAdd(lds_word(k, addr), inc);
            df.a[e] = addr;
        } else {
            atomicAdd(lds_word(k, addr), inc);   // (ds_add_u32: no return to wait for)
        }
    }
}


// MODE_TABLE merge passes: a chunk's pair-table slots (pair_slot) made at apply time, from the
// chunk before the merge, and counted by the next stage's count of the same chunk whenever the
// merge left it as it was (no rewrite: nearly every chunk).  The apply test then compares the
// slots with the merge's own slot (4 VALU, where packing the pairs cost 8), and the count makes no
// slot again.  A slot stands for two hot pairs (x, y) and (x ^ 1, y) (the counter's half is in
// inc), and for a sketch dword's cold pairs: such a false hit only sends the chunk to the exact
// apply test, which finds no match.
struct Prep {
    uint32_t addr[4], inc[4];
    int32_t x3, r3;   // plane 3's pair: lane 63 of a partial chunk holds (last live slot, nx)
    int32_t nx;       // the first live token after the chunk that r3 was made with
    int32_t ok;       // the slots hold the chunk's current pairs (0: rewritten, or not made)
};

__device__ __forceinline__ void prep_pairs(const int32_t (&t)[4], int len, int32_t last,
                                           int32_t nxt, const Sink &k, Prep &p) {
    const unsigned long long P63 = (unsigned long long)((int64_t)len - CHUNK) & (1ull << 63);
    p.x3 = sel(lane_in(P63), last, t[3]);
    p.r3 = from_next(t[0], nxt);
    const int32_t x[4] = {t[0], t[1], t[2], p.x3}, y[4] = {t[1], t[2], t[3], p.r3};
#pragma unroll
    for (int e = 0; e < 4; ++e) pair_slot<false>(k, x[e], y[e], p.addr[e], p.inc[e]);
    p.nx = nxt;
    p.ok = 1;
}

// The fast-path pairs (x[e], y[e]) of a chunk with a side in {ma, mb, mc} (MODE_FUSED's refresh
// of the maintained cold table): per-token membership masks (compares into lane masks,
// combined on the scalar unit), one wave-wide test, and the LDS hash only in chunks that hold
// such a cold pair.  (t3 differs from x3 only in lane 63 of a partial chunk, where pair 2's right
// side is the tail tag, negative: that pair is not live either way.)
template <int MODE>
__device__ __forceinline__ void refresh_pairs(const Sink &k, int32_t t0, int32_t t1, int32_t t2,
                                              int32_t x3, int32_t r3, const int32_t (&x)[4],
                                              const int32_t (&y)[4]) {
    const int32_t ma = k.ma, mb = k.mb, mc = k.mc;
    const unsigned long long M0 = member3(t0, ma, mb, mc), M1 = member3(t1, ma, mb, mc),
                             M2 = member3(t2, ma, mb, mc), M3 = member3(x3, ma, mb, mc),
                             M4 = member3(r3, ma, mb, mc);
    const unsigned long long W0 = M0 | M1, W1 = M1 | M2, W2 = M2 | M3, W3 = M3 | M4;
    if ((W0 | W1 | W2 | W3) == 0ull) return;
    const unsigned long long Wm[4] = {W0, W1, W2, W3};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (lane_in(Wm[e]) & ((x[e] | y[e]) >= HOT)) {
            lds_fused_add(k, pair_key(x[e], y[e]), 1u);
        }
}

// Counts the pairs of one post-merge chunk (len > 0) whose right side lies inside the region:
// nxt = the first live token of the next non-empty chunk, NONE past the region's end.
//
// Fast path: no slot inside a run of >= 3 and, for a partial chunk, a last token that differs
// from nxt.  A partial chunk's last pair (last, nxt) is moved to lane 63's slot 3 (dead in a
// partial chunk), so no lane-dependent fix-up is needed.  Everything else (runs of >= 3, the
// region's first run, a partial chunk ending in an X X pair) takes the exact path.
//
// Per-slot conditions are wave masks combined with 64-bit bitwise operations and uniform
// conditions are integers: no short-circuit operators on the common path (they become control
// flow whose booleans round-trip through vector registers).
// TAIL: the region's last chunk (nxt = NONE).  It always takes the exact path: the parity of its
// last token's run offset feeds RegionSum::trail_odd, which k_runs needs whenever that run goes on
// in the next region, and the fast path does not work that parity out.
// Fast-path counts of MODE_TABLE / MODE_FUSED leave the words their adds returned in `df`, and the
// other paths OR theirs into s.seen: the overflow screen of the ring round (screen_round).
template <int MODE, bool TAIL = false, bool SCREEN = true, bool PREP = false>
__device__ __forceinline__ void count_chunk(const Chunk &w, int32_t nxt, int lane, Tally &s,
                                            const Sink &k, Defer &df, Prep &pp) {
    const int len = w.len;
    if (MODE == MODE_NONE && !TAIL) {
        // apply-only passes keep only the region sums: the chunk needs work only in the region's
        // first run, or when its last token's run goes on in the next chunk (its parity)
        const uint32_t lead0 = (uint32_t)__builtin_amdgcn_readfirstlane(s.in_lead);
        if ((lead0 | (uint32_t)(w.last == nxt)) == 0u) {
            s.first_tok = s.n_live ? s.first_tok : w.first;
            s.par = 0;
            s.prev = w.last;
            s.n_live += len;
            return;
        }
    }
#ifdef BPE_PROBE_NOCOUNT
    if (MODE == MODE_TABLE) {   // (timing probe only: the ring and its bookkeeping, no counting)
        s.first_tok = s.n_live ? s.first_tok : w.first;
        s.par = 0;
        s.prev = w.last;
        s.n_live += len;
        s.in_lead = 0;
        return;
    }
#endif
    const int32_t t0 = w.t[0], t1 = w.t[1], t2 = w.t[2], t3 = w.t[3];
    // lane 63's bit when the chunk is partial (an integer mask, not a boolean: uniform booleans
    // cost a lane-mask round trip per use)
    const unsigned long long P63 = (unsigned long long)((int64_t)len - CHUNK) & (1ull << 63);
    if (PREP && !TAIL) {
        // the slots made at apply time (Prep): made now if the merge rewrote the chunk, plane 3
        // made again if the first token after it changed (a merge at the next chunk's start)
        if (!pp.ok) {
            prep_pairs(w.t, len, w.last, nxt, k, pp);
        } else if (pp.nx != nxt) {
            pp.r3 = from_next(t0, nxt);
            pair_slot<false>(k, pp.x3, pp.r3, pp.addr[3], pp.inc[3]);
            pp.nx = nxt;
        }
    }
    // slot 3 of lane 63 holds the last live slot (a partial chunk's slot 255 is its tail tag)
    const int32_t x3 = PREP && !TAIL ? pp.x3 : sel(lane_in(P63), w.last, t3);
    const int32_t r3 = PREP && !TAIL ? pp.r3 : from_next(t0, nxt);
    const int32_t l0 = from_prev(t3, s.prev);
    // E*: slot equals its right-hand neighbour (Em1: slot 0 equals the token before it).  No
    // dead slot equals its neighbour and slot 0 is live (an SEP next to an SEP only sends the chunk
    // to the exact path); E3's lane-63 bit compares the last live slot with nxt.
    const unsigned long long Em1 = __ballot(t0 == l0), E0 = __ballot(t0 == t1),
                             E1 = __ballot(t1 == t2), E2 = __ballot(t2 == t3), E3 = __ballot(x3 == r3);
    const unsigned long long trip = (E0 & (Em1 | E1)) | (E2 & (E1 | E3));
    // fast: no run of three, not in the region's first run, and a partial chunk does not end in
    // an X X pair
    // (readfirstlane: the compiler cannot see that in_lead is wave-uniform, and would branch on it
    // per lane)
    const unsigned long long lead = (uint32_t)__builtin_amdgcn_readfirstlane(s.in_lead);
    if (!TAIL && (trip | (E3 & P63) | lead) == 0ull) {
        // every X X pair starts its run, so every valid pair counts
        const int32_t x[4] = {t0, t1, t2, x3}, y[4] = {t1, t2, t3, r3};
        if (MODE == MODE_TABLE || MODE == MODE_FUSED) {
            // one form for every chunk: 11 VALU per pair, both classes (a separate 5-VALU form
            // for chunks of hot tokens only paid off only on a fresh corpus; telling the two
            // apart cost more over a whole run: dropping it timed the C3 run 3 % faster)
            if (PREP) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (SCREEN) {
                        df.o[e] = atomicAdd(lds_word(k, pp.addr[e]), pp.inc[e]);
                        df.a[e] = pp.addr[e];
                    } else {
                        atomicAdd(lds_word(k, pp.addr[e]), pp.inc[e]);
                    }
                }
            } else {
                add_pairs<MODE == MODE_FUSED, SCREEN>(x, y, k, df);
            }
            if (MODE == MODE_FUSED) refresh_pairs<MODE>(k, t0, t1, t2, x3, r3, x, y);
        } else if (MODE == MODE_EXACT) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if ((x[e] | y[e]) >= HOT) count_pair<MODE>(k, x[e], y[e], s.seen);
        } else if (MODE == MODE_INCR) {
            // only the pairs with a side in {ma, mb, mc}: membership masks per slot (compares into
            // lane masks, combined on the scalar unit), the LDS only for chunks that hold one
            const int32_t ma = k.ma, mb = k.mb, mc = k.mc;
            const unsigned long long M0 = member3(t0, ma, mb, mc), M1 = member3(t1, ma, mb, mc),
                                     M2 = member3(t2, ma, mb, mc), M3 = member3(x3, ma, mb, mc),
                                     M4 = member3(r3, ma, mb, mc);
            const unsigned long long Wm[4] = {M0 | M1, M1 | M2, M2 | M3, M3 | M4};
            if ((Wm[0] | Wm[1] | Wm[2] | Wm[3]) != 0ull) {
                // branch-free on the common route (a row counter): every lane adds, 0 when its
                // pair is not touched (to a counter of its own: no two lanes on one address);
                // pairs of mc, and other tokens past the rows, take the hash (rare)
                unsigned long long hsh = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // a plane with no touched pair adds nothing (its df.o[e] stays 0): 3 % of
                    // the skewed corpus's pass (profiles/r05_ab_zipf_plane_skip.txt)
                    if (Wm[e] == 0ull) continue;
                    const int32_t xx = x[e], yy = y[e];
                    const bool act = lane_in(Wm[e]);
                    const bool xa = xx == ma, xb = xx == mb, ya = yy == ma, yb = yy == mb;
                    const int row = xa ? 0 : xb ? 1 : ya ? 2 : 3;
                    const int idx = (xa | xb) ? yy : xx;
                    // (an unsigned bound: a pair with a negative side (SEP, dead) never has both a
                    // member side and idx >= 0, so it never lands in a row; the rare branch below
                    // drops such pairs from the hash)
                    const bool inrow = act & (xa | xb | ya | yb) & ((uint32_t)idx < (uint32_t)INCR_RLIM);
                    // counter cc = row * INCR_RLIM + idx: byte address of its dword (cc >> 1) * 4,
                    // made as (2 cc) & ~3; its half (cc & 1) = (idx & 1) (INCR_RLIM is even)
                    const uint32_t cc2 = (uint32_t)(row * (2 * INCR_RLIM)) + 2u * (uint32_t)idx;
                    const uint32_t ba = inrow ? (cc2 & ~3u) : 4u * (uint32_t)lane;
                    // (the returns wait for the round's overflow screen; a lane's own dword
                    // `lane` is a row 0 counter, so its return can only raise a false alarm)
                    df.o[e] = atomicAdd(reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(k.hist) + ba),
                                        (uint32_t)inrow << (((uint32_t)idx & 1u) << 4));
                    df.a[e] = ba;
                    hsh |= (unsigned long long)(act & !inrow) << e;
                }
                if (__ballot(hsh != 0ull) != 0ull) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (((hsh >> e) & 1ull) && (x[e] | y[e]) >= 0)
                            incr_hash_add(k, ((uint32_t)x[e] << 16) | (uint32_t)y[e], 1u);
                }
            }
        }
        // the last token starts its run here (a run continuing into the next chunk would be a run
        // of three, or a partial chunk's X X end), so its offset parity is 0
        s.first_tok = s.n_live ? s.first_tok : w.first;
        s.par = 0;
        s.prev = w.last;
        s.n_live += len;
        return;
    }
    const int full = len == CHUNK;
    // exact path
#ifdef BPE_PROBE_COMMON
    s.in_lead = 0;   // (static instruction-count probe only: drop the exact path)
    return;
#endif
    const int kl = len - 1, ll = kl >> 2, el = kl & 3;
    int32_t rr[4] = {t1, t2, t3, r3};
    if (!full) {
        const bool me = lane_in(1ull << ll);
        switch (el) {
        case 0: rr[0] = sel(me, nxt, rr[0]); break;
        case 1: rr[1] = sel(me, nxt, rr[1]); break;
        case 2: rr[2] = sel(me, nxt, rr[2]); break;
        default: rr[3] = sel(me, nxt, rr[3]); break;
        }
    }
    int par[4];
    bool start[4];
    run_parity(w.t, len, s.prev, s.par, lane, par, start);
    bool cnt[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool valid = ((w.t[e] | rr[e]) >= 0) & (4 * lane + e < len);
        cnt[e] = valid & !((w.t[e] == rr[e]) & (par[e] != 0));
    }
    const int par_last = bcast(pick4(par, el), ll);
    if (s.in_lead) {
        // the first run ends at the first run start at region position >= 1
        int f = len;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned long long m = __ballot(start[e] & ((s.n_live + 4 * lane + e) > 0));
            if (m) {
                const int q = 4 * __builtin_ctzll(m) + e;
                f = q < f ? q : f;
            }
        }
        if (f < len) {
            s.lead_len = s.n_live + f;
            s.in_lead = 0;
        }
        // (MODE_TABLE: kept a scalar; as a select the compiler made it a vector value, read back
        // with a readfirstlane in every chunk's fast-path test: C3 pass 0.7249 -> 0.7207 ms.  The
        // maintained state's pass timed 4 % slower with it; profiles/r05_ab_in_lead.txt)
        if (MODE == MODE_TABLE) s.in_lead = __builtin_amdgcn_readfirstlane(s.in_lead);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (cnt[e]) count_pair<MODE, SCREEN>(k, w.t[e], rr[e], s.seen);
    s.first_tok = s.n_live ? s.first_tok : w.first;
    s.prev = w.last;
    s.par = par_last;
    s.n_live += len;
}

// Apply-side state of one region (wave-uniform).
struct Apply {
    int32_t prev;        // last pre-merge live token before the chunk
    int32_t par;         // its run-offset parity (X X merges only)
    int32_t match;       // it is an `a` matched with the chunk's first live token
    uint32_t n_match;
    // SITES (the delta form's apply-only stream): the region's segment of the site list, the
    // entries written so far, and the region's first chunk (entries are corpus chunk indices)
    uint32_t *sites;
    uint32_t n_sites;
    uint32_t c0;
};

// What a k_step pass does before counting: nothing, a merge of two distinct ids, or an X X merge
// (the only kind whose matches depend on run parity, so the only one carrying that code).
enum MergeKind { NO_MERGE = 0, MERGE_XY = 1, MERGE_XX = 2 };

// Writes the tail tag of a re-packed chunk (slot 255 lives on lane 63).
__device__ __forceinline__ void tag_tail(int32_t (&y)[4], int total, int32_t last) {
    if (total < CHUNK) y[3] = sel(lane_in(1ull << 63), tail_tag(total, last), y[3]);
}

// Applies the merge (a, b) -> c to one pre-merge chunk (w.len > 0) at chunk index c of the region,
// in place: nxt = the first pre-merge live token after it (the next region's first for the last
// chunk).  A touched chunk is re-packed and written back.
// SITES: every chunk written back is appended to the wave's own segment of the site list.
template <int MERGE, bool PREP = false, bool SITES = false>
__device__ __forceinline__ void apply_chunk(Chunk &w, int32_t nxt, int32_t ma, int32_t mb,
                                            int32_t mc,
                                            const __amdgpu_buffer_rsrc_t rs, int c, int lane,
                                            Apply &ap, Prep &pp, uint32_t akey) {
#ifdef BPE_PROBE_NOAPPLY
    if (lane >= 0) {   // (timing probe only: no merge detection or rewrite)
        ap.prev = w.last;
        ap.par = 0;
        ap.match = 0;
        return;
    }
#endif
    // The common case, no (a, b) in the chunk: four packed (slot, right neighbour) compares.  In a
    // partial chunk lane 63's slot 3 (dead) stands in for the last live slot, paired with nxt.
    // (A tail tag can alias a token in its low half; such a false hit only takes the exact path.)
    // (Testing for `a` alone, four compares instead of eight VALU, timed 2 % slower on C3 and zipf
    // C3: a chunk holding `a` without (a, b) then pays the full test; profiles/r05_ab_acheck.txt.)
    {
        unsigned long long H;
        if (PREP) {
            // (the chunk's pair-table slots, made by prep_pairs: a slot equal to the merge's own)
            H = __ballot(pp.addr[0] == akey) | __ballot(pp.addr[1] == akey) |
                __ballot(pp.addr[2] == akey) | __ballot(pp.addr[3] == akey);
        } else {
            const int32_t r3 = from_next(w.t[0], nxt);
            const unsigned long long P63 = (unsigned long long)((int64_t)w.len - CHUNK) & (1ull << 63);
            const int32_t x3 = sel(lane_in(P63), w.last, w.t[3]);
            const uint32_t key = pack_pair_s(ma, mb);
            H = __ballot(pack_pair(w.t[0], w.t[1]) == key) | __ballot(pack_pair(w.t[1], w.t[2]) == key) |
                __ballot(pack_pair(w.t[2], w.t[3]) == key) | __ballot(pack_pair(x3, r3) == key);
        }
        unsigned long long T = H | (unsigned long long)(uint32_t)ap.match;
        // (X X merges also carry the run parity while the chunk ends in `a`)
        if (MERGE == MERGE_XX) T |= (unsigned long long)(uint32_t)(w.last == ma);
        if (T == 0ull) {
            ap.prev = w.last;
            ap.par = 0;
            ap.match = 0;
            return;
        }
    }
    // M[e]: slot e is `a` and its in-register right-hand neighbour is `b`
    const unsigned long long A0 = __ballot(w.t[0] == ma), A1 = __ballot(w.t[1] == ma),
                             A2 = __ballot(w.t[2] == ma), A3 = __ballot(w.t[3] == ma);
    const unsigned long long B0 = __ballot(w.t[0] == mb), B1 = __ballot(w.t[1] == mb),
                             B2 = __ballot(w.t[2] == mb), B3 = __ballot(w.t[3] == mb);
    unsigned long long M0 = A0 & B1, M1 = A1 & B2, M2 = A2 & B3, M3 = A3 & (B0 >> 1);
    // the last live slot's neighbour is nxt
    int m_last = ((uint32_t)(w.last ^ ma) | (uint32_t)(nxt ^ mb)) == 0u;
    int par_last = 0;
    if (MERGE == MERGE_XX) {
        // only even run offsets match (core.ts:285-290 == replaceAll's leftmost rule); the
        // parity is carried only while the chunk ends in `a`
        if (((M0 | M1 | M2 | M3) != 0ull) | (w.last == ma)) {
            const int kl = w.len - 1;
            int par[4];
            bool start[4];
            run_parity(w.t, w.len, ap.prev, ap.par, lane, par, start);
            M0 &= __ballot(par[0] == 0);
            M1 &= __ballot(par[1] == 0);
            M2 &= __ballot(par[2] == 0);
            M3 &= __ballot(par[3] == 0);
            par_last = bcast(pick4(par, kl & 3), kl >> 2);
            m_last &= par_last == 0;
        }
    }
    const int32_t t_last = w.last;
    if (((M0 | M1 | M2 | M3) != 0ull) | ((ap.match | m_last) != 0)) {
#ifdef BPE_PROBE_COMMON
        if (lane < 0) {   // (static instruction-count probe only: drop the rewrite)
#endif
        const int kl = w.len - 1;
        if (m_last) {
            const unsigned long long bit = 1ull << (kl >> 2);
            switch (kl & 3) {
            case 0: M0 |= bit; break;
            case 1: M1 |= bit; break;
            case 2: M2 |= bit; break;
            default: M3 |= bit; break;
            }
        }
        const bool m[4] = {lane_in(M0), lane_in(M1), lane_in(M2), lane_in(M3)};
        const bool up = lane_in((M3 << 1) | (unsigned long long)(ap.match != 0));
        const int l4 = 4 * lane;
        bool keep[4];
        keep[0] = (l4 < w.len) & !up;
        keep[1] = (l4 < w.len - 1) & !m[0];
        keep[2] = (l4 < w.len - 2) & !m[1];
        keep[3] = (l4 < w.len - 3) & !m[2];
        int32_t y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = sel(m[e], mc, w.t[e]);
        const int total = compact_chunk(y, keep, w.len, lane);
        const int32_t last = total ? slot_at(y, total - 1) : NONE;
        w.first = total ? bcast(y[0], 0) : TOMB;
#pragma unroll
        for (int e = 0; e < 4; ++e) w.t[e] = y[e];
        tag_tail(y, total, last);
        __builtin_amdgcn_raw_buffer_store_b128(
            __builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned,
                               make_uint4((unsigned)y[0], (unsigned)y[1], (unsigned)y[2], (unsigned)y[3])),
            rs, lane * 16, c * (CHUNK * 4), 0);
        ap.n_match += (uint32_t)(__popcll(M0) + __popcll(M1) + __popcll(M2) + __popcll(M3));
        if (SITES) {
            // (a chunk is rewritten at most once per pass, so the segment of cpr entries holds)
            if (lane == 0) ap.sites[ap.n_sites] = ap.c0 + (uint32_t)c;
            ++ap.n_sites;
        }
        w.len = total;
        w.last = last;
        pp.ok = 0;   // (the count makes the rewritten chunk's slots)
#ifdef BPE_PROBE_COMMON
        }
#endif
    }
    ap.prev = t_last;
    ap.par = par_last;
    ap.match = m_last;
}

// hist: the kernel's static LDS table (so, once inlined, LDS addresses are plain constants with no
// symbol base to add per access)
template <int MERGE, int MODE, bool SCREEN = true, bool SLOTS = true, bool SITES = false>
__device__ __forceinline__ void step_body(uint32_t *hist, int32_t *__restrict__ ids,
                                          int64_t n_chunks, int64_t cpr, int R,
                                          const RegionCarry *__restrict__ carry, int32_t ma,
                                          int32_t mb, int32_t mc, uint32_t *__restrict__ partials,
                                          unsigned long long *__restrict__ spill, ColdTable ct,
                                          const uint32_t *__restrict__ heavy_g,
                                          RegionSum *__restrict__ sums,
                                          unsigned long long *__restrict__ replaced,
                                          unsigned long long *__restrict__ hot_g = nullptr,
                                          unsigned long long *__restrict__ delta = nullptr,
                                          uint32_t *__restrict__ site_list = nullptr,
                                          uint32_t *__restrict__ site_n = nullptr) {
    // (SITES: site_list holds a segment of cpr entries per region, site_n the entries written)
    // (MODE_INCR: `spill` holds the rows' spill, 4 * INCR_RLIM u64; hot_g the maintained table;
    // delta: a sharded rank's delta rows, which then take the touched pairs instead of the tables)
    unsigned long long *rspill = spill;
    if (MODE == MODE_TABLE || MODE == MODE_FUSED) {
        // (MODE_FUSED: the LDS hash's keys start EMPTY; one store per dword, so no two threads
        // write the same dword before the barrier)
        uint4 *h4 = reinterpret_cast<uint4 *>(hist);
        for (int i = threadIdx.x; i < HIST_WORDS / 4; i += WG) {
            const bool key = MODE == MODE_FUSED && i >= FH_BASE / 4 && i < (FH_BASE + FH_SLOTS) / 4;
            const uint32_t v = key ? EMPTY : 0u;
            h4[i] = make_uint4(v, v, v, v);
        }
    } else if (MODE == MODE_EXACT) {
        for (int i = threadIdx.x; i < HEAVY_WORDS; i += WG) hist[i] = heavy_g[i];
        for (int i = threadIdx.x; i < LH_SLOTS; i += WG) {
            hist[HEAVY_WORDS + i] = EMPTY;
            hist[HEAVY_WORDS + LH_SLOTS + i] = 0;
        }
    } else if (MODE == MODE_INCR) {
        // the rows' used part (other tokens < min(vocabulary, INCR_RLIM)) and the hash
        const int vl = incr_vlim(mc);
        for (int r = 0; r < 4; ++r)
            for (int i = threadIdx.x; i < vl / 2; i += WG) hist[r * (INCR_RLIM / 2) + i] = 0;
        for (int i = threadIdx.x; i < IH_SLOTS; i += WG) {
            hist[IH_BASE + i] = EMPTY;
            hist[IH_BASE + IH_SLOTS + i] = 0;
        }
    }
    if (MODE != MODE_NONE) __syncthreads();
    Sink k;
    k.hist = hist;
    k.spill = spill;
    k.ct = ct;
    k.heavy = hist;
    k.ma = MODE == MODE_FUSED || MODE == MODE_INCR ? ma : -1;
    k.mb = mb;
    k.mc = mc;
    k.hot = hot_g;
    k.rspill = rspill;
    k.delta = delta;
    k.hot_bytes_v = HOT_BYTES;
    asm volatile("" : "+v"(k.hot_bytes_v));   // (kept in a VGPR for the whole pass)
    const int lane = threadIdx.x & 63;
    const int r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES_PER_WG + (threadIdx.x >> 6)));
    if (r < R) {
        const int64_t c0 = (int64_t)r * cpr;
        const int64_t c1 = min(c0 + cpr, n_chunks);
        const int nc = (int)(c1 > c0 ? c1 - c0 : 0);
        const RegionCarry rc = carry[r];
        Tally s;
        s.n_live = 0;
        s.lead_len = 0;
        s.prev = NONE;
        s.par = 0;
        s.first_tok = NONE;
        s.in_lead = 1;
        s.seen = 0;
        Apply ap;
        ap.prev = rc.prev_tok;
        ap.par = (int32_t)(rc.carry_off & 1) ^ 1;   // the token before the region (if linked)
        ap.match = 0;
        ap.n_match = 0;
        ap.sites = SITES ? site_list + c0 : nullptr;
        ap.n_sites = 0;
        ap.c0 = (uint32_t)c0;
        // the region through a range-checked buffer descriptor (loads past its end return 0 and
        // are never consumed)
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            ids + c0 * CHUNK, 0, nc * CHUNK * 4, 0x00020000);
        const int lo = lane * 16;
        auto load = [&](Chunk &q, int c) __attribute__((always_inline)) {
            const auto x = __builtin_amdgcn_raw_buffer_load_b128(rs, lo, c * (CHUNK * 4), BPE_LOAD_AUX);
            q.t[0] = (int)x[0];
            q.t[1] = (int)x[1];
            q.t[2] = (int)x[2];
            q.t[3] = (int)x[3];
        };
        // first pre-merge live token at or after chunk c (whose slot 0 is f0)
        auto live_from = [&](int c, int32_t f0) -> int32_t {
            int32_t v = c < nc ? f0 : rc.next_tok;
            if (__builtin_expect(v < SEP, 0)) {
                // rare: empty chunks; scan their slot 0s
                int q = c + 1;
                for (; q < nc; ++q) {
                    v = __builtin_amdgcn_readfirstlane(
                        (int)__builtin_amdgcn_raw_buffer_load_b32(rs, 0, q * (CHUNK * 4), 0));
                    if (v >= SEP) break;
                }
                if (q >= nc) v = rc.next_tok;
            }
            return v;
        };
        // Ring of RING slots: stage c applies chunk c (cur), counts chunk c-1 (prv) and loads chunk
        // c+RING-3 into the slot of chunk c-3 (fre), which the previous stage freed, so the load
        // can issue at once without its registers overlapping a chunk still in use.  Stage i of a
        // round keeps its count's LDS returns in D[i] until the round's overflow screen.
        Defer D[RING];
        static_for<0, RING>([&](auto i) __attribute__((always_inline)) {
            D[i].o[0] = D[i].o[1] = D[i].o[2] = D[i].o[3] = 0u;
            D[i].a[0] = D[i].a[1] = D[i].a[2] = D[i].a[3] = 0u;
        });
        // The overflow screen of a round (MODE_TABLE / MODE_FUSED / MODE_INCR): every word the
        // wave's adds returned since the last screen; where a half stood at >= 0x4000, a sweep.
        // The fast path's adds kept their addresses: each lane sweeps just the words its adds saw
        // high (sweep_word: an atomic AND, so lanes and waves sweeping one word take its bits
        // once).  The next add to a half that crossed 0x4000 sees it high, and its wave sweeps it
        // at the end of that round: the bound of the whole-table sweep, 0x4000 + the adds of one
        // round of every wave (the static_assert on RING).  The exact path's adds (s.seen) kept
        // no address: the whole table then, as before round 5.  (Early on a skewed corpus a few
        // pairs hold most of a workgroup's counts: every round swept all 40960 words, and a pass
        // took 4 ms instead of 0.6.)
        auto screen_round = [&]() __attribute__((always_inline)) {
            if (MODE != MODE_TABLE && MODE != MODE_FUSED && MODE != MODE_INCR) return;
            if (!SCREEN) return;
            const bool whole = __ballot((s.seen & SWEEP_BITS) != 0u) != 0ull;
            s.seen = 0;
            uint32_t acc = 0;
            static_for<0, RING>([&](auto i) __attribute__((always_inline)) {
                acc |= D[i].o[0] | D[i].o[1] | D[i].o[2] | D[i].o[3];
            });
            if (!whole && __ballot((acc & SWEEP_BITS) != 0u) != 0ull) {
                unsigned long long *sp = MODE == MODE_INCR ? rspill : spill;
                static_for<0, RING>([&](auto i) __attribute__((always_inline)) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) sweep_word(hist, sp, (int)(D[i].a[e] >> 2), D[i].o[e]);
                });
            }
            static_for<0, RING>([&](auto i) __attribute__((always_inline)) {
                D[i].o[0] = D[i].o[1] = D[i].o[2] = D[i].o[3] = 0u;
            });
            if (whole) {
                if (MODE == MODE_INCR) {
                    const int vl = incr_vlim(mc);
                    for (int rw = 0; rw < 4; ++rw)
                        lds_sweep(hist, rspill, lane, rw * (INCR_RLIM / 2),
                                  rw * (INCR_RLIM / 2) + vl / 2);
                } else {
                    lds_sweep(hist, spill, lane, 0, MODE == MODE_FUSED ? HOT_BINS / 2 : HIST_WORDS);
                }
            }
        };
        // pf (MODE_TABLE): slot 0 of the chunk the next stage takes up, read (a lane read, one
        // VALU) by the stage before it for its merge test's right-hand neighbour, and handed on
        // rather than read again when that chunk's own stage begins: C3 pass -0.2 %; the other
        // modes read it again (the maintained state's pass timed 2.6 % slower with the hand-on;
        // profiles/r05_ab_first_handon.txt)
        int32_t pf = 0;
        // MODE_TABLE merge passes: each chunk's pair-table slots made at apply time (Prep), and the
        // merge's own slot, to test against them
        constexpr bool PREP = MODE == MODE_TABLE && MERGE != NO_MERGE && SLOTS;
        uint32_t akey = 0;
        if (PREP) {
            uint32_t a0, i0;
            pair_slot<false>(k, ma, mb, a0, i0);
            akey = (uint32_t)__builtin_amdgcn_readfirstlane((int)a0);
        }
        // (the stage waits for chunk c + 1's load at its start: chunk c's merge test needs its
        // first token.  Loading slot 0 of every chunk on its own a stage earlier, so that a stage
        // waits only for loads issued two stages back, timed the same: profiles/r06_ab_early.txt)
        auto stage = [&](Chunk &cur, const Chunk &nxt_slot, Chunk &prv, Chunk &fre, int c,
                         Defer &df, Prep &pcur, Prep &pprv) __attribute__((always_inline)) {
            load(fre, c + LEAD);
            const int32_t f_next = bcast(nxt_slot.t[0], 0);
            if (c < nc) {
                finish_load(cur, MODE == MODE_TABLE ? pf : bcast(cur.t[0], 0));
            } else {
                // past the region: an empty chunk hands the pending one on (every field stored on
                // both sides, so the stores merge as values, not as a select of addresses)
                cur.first = TOMB;
                cur.len = 0;
                cur.last = NONE;
            }
            if (MERGE && cur.len) {
                const int32_t nx = live_from(c + 1, MODE == MODE_TABLE ? f_next : bcast(nxt_slot.t[0], 0));
                if (PREP) prep_pairs(cur.t, cur.len, cur.last, nx, k, pcur);
                apply_chunk<MERGE, PREP, SITES>(cur, nx, ma, mb, mc, rs, c, lane, ap, pcur, akey);
            }
            if (cur.len) {
                if (prv.len) count_chunk<MODE, false, SCREEN, PREP>(prv, cur.first, lane, s, k, df, pprv);
            } else {
                cur = prv;   // rare: hand the pending chunk on
                if (PREP) pcur = pprv;
            }
            // (prv kept live past the hand-on's merge of two register sets, so the register
            // allocator gives the merged chunk cur's registers and puts the copies on the rare
            // path: 7 -> 2 register moves per stage, C3 pass -0.9 %; in the other modes it timed
            // 2 % slower on the skewed corpus; profiles/r05_ab_handon_live.txt)
            if (MODE == MODE_TABLE)
                asm volatile("" ::"v"(prv.t[0]), "v"(prv.t[1]), "v"(prv.t[2]), "v"(prv.t[3]),
                             "s"(prv.last), "s"(prv.first), "s"(prv.len));
            pf = f_next;
        };
        if (nc > 0) {
            Chunk S[RING];   // (constant indices only: the ring stays in registers)
            Prep P[RING];
            static_for<0, RING>([&](auto i) __attribute__((always_inline)) { P[i].ok = 0; });
            static_for<0, LEAD>([&](auto i) __attribute__((always_inline)) { load(S[i], i); });
            S[RING - 1].len = 0;
            pf = bcast(S[0].t[0], 0);
            if (MERGE) {
                // does the token before the region match the region's first live token?
                const int32_t f = live_from(0, pf);
                // (integer arithmetic: a short-circuit && here makes the flag a vector value)
                ap.match = (((uint32_t)(ap.prev ^ ma) | (uint32_t)(f ^ mb)) == 0u) &
                           ((MERGE == MERGE_XY) | (ap.par == 0));
            }
            // whole rounds of RING stages; stages past the region see empty chunks, so the
            // pending chunk always ends in the last slot
            for (int c = 0; c < nc; c += RING) {
                static_for<0, RING>([&](auto I) __attribute__((always_inline)) {
                    constexpr int i = decltype(I)::value;
                    stage(S[i], S[(i + 1) % RING], S[(i + RING - 1) % RING],
                          S[(i + LEAD) % RING], c + i, D[i], P[i], P[(i + RING - 1) % RING]);
                });
                screen_round();
            }
            Defer dt;   // (the region's last chunk takes the exact path: s.seen)
            if (S[RING - 1].len)
                count_chunk<MODE, true, SCREEN>(S[RING - 1], NONE, lane, s, k, dt, P[RING - 1]);
            screen_round();
        }
        if (lane == 0) {
            RegionSum o;
            o.n_live = s.n_live;
            o.first_tok = s.n_live ? s.first_tok : NONE;
            o.last_tok = s.n_live ? s.prev : NONE;
            o.uniform = s.n_live && s.in_lead ? 1 : 0;
            o.lead_len = s.in_lead ? s.n_live : s.lead_len;
            o.trail_odd = s.par ^ 1;   // trail run length = offset of the last token + 1
            sums[r] = o;
            if (MERGE && ap.n_match) atomicAdd(replaced, (unsigned long long)ap.n_match);
            if (SITES) site_n[r] = ap.n_sites;
        }
    }
    if (MODE == MODE_TABLE || MODE == MODE_FUSED) {
        __syncthreads();
        uint4 *out = reinterpret_cast<uint4 *>(partials + (size_t)blockIdx.x * HIST_WORDS);
        const uint4 *h4 = reinterpret_cast<const uint4 *>(hist);
        for (int i = threadIdx.x; i < HIST_WORDS / 4; i += WG) out[i] = h4[i];
        if (MODE == MODE_FUSED)   // (the slab's sketch dwords are then garbage: unused)
            for (int j = threadIdx.x; j < FH_SLOTS; j += WG) {
                // (each workgroup starts its flush elsewhere: workgroups adding one new key at
                // the same moment each reserve a dense index, and all but one become holes)
                const int i = (j + (int)blockIdx.x * 97 * 64) & (FH_SLOTS - 1);
                const uint32_t key = hist[FH_BASE + i];
                if (key != EMPTY) cold_add(ct, key, hist[FH_BASE + FH_SLOTS + i]);
            }
    } else if (MODE == MODE_INCR) {
        // the rows' used part to this workgroup's slab (k_reduce_rows sums the slabs), the hash's
        // keys straight into the maintained tables
        __syncthreads();
        const int vl = incr_vlim(mc);
        uint32_t *out = partials + (size_t)blockIdx.x * HIST_WORDS;
        for (int r = 0; r < 4; ++r)
            for (int i = threadIdx.x; i < vl / 2; i += WG)
                out[r * (INCR_RLIM / 2) + i] = hist[r * (INCR_RLIM / 2) + i];
        for (int j = threadIdx.x; j < IH_SLOTS; j += WG) {
            const int i = (j + (int)blockIdx.x * 97 * 64) & (IH_SLOTS - 1);
            const uint32_t key = hist[IH_BASE + i];
            if (key != EMPTY)
                incr_global_add(k, (int32_t)(key >> 16), (int32_t)(key & 0xFFFFu),
                                hist[IH_BASE + IH_SLOTS + i]);
        }
    } else if (MODE == MODE_EXACT) {
        __syncthreads();
        for (int j = threadIdx.x; j < LH_SLOTS; j += WG) {
            const int i = (j + (int)blockIdx.x * 97 * 64) & (LH_SLOTS - 1);   // (as above)
            const uint32_t key = hist[HEAVY_WORDS + i];
            if (key != EMPTY) cold_add(ct, key, hist[HEAVY_WORDS + LH_SLOTS + i]);
        }
    }
}

template <int MERGE, int MODE>
__global__ void __launch_bounds__(WG)
k_step(int32_t *__restrict__ ids, int64_t n_chunks, int64_t cpr, int R,
       const RegionCarry *__restrict__ carry, int32_t ma, int32_t mb, int32_t mc,
       uint32_t *__restrict__ partials, unsigned long long *__restrict__ spill, ColdTable ct,
       const uint32_t *__restrict__ heavy_g, RegionSum *__restrict__ sums,
       unsigned long long *__restrict__ replaced, unsigned long long *__restrict__ hot_g = nullptr) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[HIST_WORDS];
    step_body<MERGE, MODE>(hist, ids, n_chunks, cpr, R, carry, ma, mb, mc, partials, spill, ct,
                           heavy_g, sums, replaced, hot_g);
}

// Apply-only pass (restoreMerge replay, batch encoding, core.ts:477-494 / 392-409): the merge is
// applied exactly as by k_step, and the region sums are kept (k_runs<MODE_NONE> turns them into the
// carries of the next pass), but no pair is counted: no LDS table, no slab.
template <int MERGE>
__global__ void __launch_bounds__(WG)
k_apply(int32_t *__restrict__ ids, int64_t n_chunks, int64_t cpr, int R,
        const RegionCarry *__restrict__ carry, int32_t ma, int32_t mb, int32_t mc,
        RegionSum *__restrict__ sums, unsigned long long *__restrict__ replaced) {
    step_body<MERGE, MODE_NONE>(nullptr, ids, n_chunks, cpr, R, carry, ma, mb, mc, nullptr, nullptr,
                                ColdTable{}, nullptr, sums, replaced);
}

// The device loop's pass: the merge to apply is the one k_decide left in the LoopCtl.
// MODE_FUSED: the maintained cold table's refresh rides along (k_cold_invalidate ran before).
template <int MODE = MODE_TABLE>
__global__ void __launch_bounds__(WG)
k_step_loop(int32_t *__restrict__ ids, int64_t n_chunks, int64_t cpr, int R,
            const RegionCarry *__restrict__ carry, const LoopCtl *__restrict__ ctl,
            uint32_t *__restrict__ partials, unsigned long long *__restrict__ spill, ColdTable ct,
            RegionSum *__restrict__ sums, unsigned long long *__restrict__ replaced,
            unsigned long long *__restrict__ hot_g = nullptr,
            unsigned long long *__restrict__ delta = nullptr) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[HIST_WORDS];
    // (a delta iteration is k_apply_loop's; both words loaded before either is tested: one
    // memory latency)
    const int32_t status = ctl->status, form = MODE == MODE_TABLE ? ctl->delta : 0;
    if ((status != LOOP_RUN) | (form != 0)) return;
    const int32_t ma = ctl->a, mb = ctl->b, mc = ctl->c;
    if (ma == mb)
        step_body<MERGE_XX, MODE>(hist, ids, n_chunks, cpr, R, carry, ma, mb, mc, partials, spill,
                                  ct, nullptr, sums, replaced, hot_g, delta);
    else if (MODE == MODE_TABLE && ctl->unscreened)
        step_body<MERGE_XY, MODE, false>(hist, ids, n_chunks, cpr, R, carry, ma, mb, mc, partials,
                                         spill, ct, nullptr, sums, replaced, hot_g, delta);
    else if (MODE == MODE_TABLE && (int64_t)ctl->w * 16 >= n_chunks)
        // a heavy merge (a skewed corpus's first merges: W in the millions, always screened)
        // rewrites too many chunks for the apply-time slots to pay: the packed-pair test
        step_body<MERGE_XY, MODE, true, false>(hist, ids, n_chunks, cpr, R, carry, ma, mb, mc,
                                               partials, spill, ct, nullptr, sums, replaced, hot_g,
                                               delta);
    else
        step_body<MERGE_XY, MODE>(hist, ids, n_chunks, cpr, R, carry, ma, mb, mc, partials, spill,
                                  ct, nullptr, sums, replaced, hot_g, delta);
}

// ---- the digest plane -----------------------------------------------------------------------
// One byte per corpus slot, in the chunk geometry (chunk j's 256 digests are bytes [256 j,
// 256 j + 256) of the plane): a token id t >= 0 maps to t % DIGEST_MOD (merged ids are allocated
// in sequence, so the codes fill evenly), SEP to DIGEST_SEP, every dead slot (TOMB, TOMB_ODD, a
// tail tag: anything below SEP) to DIGEST_DEAD.  The int32 corpus stays the record; only the delta
// form's stream reads the plane, to find the few chunks that can hold a site of the merge.
// (include/bpe.h BPE_DIGEST_*, mirrored by the package's DIGEST_* and digest())
constexpr uint32_t DIGEST_MOD = 254, DIGEST_SEP = 254, DIGEST_DEAD = 255;

__host__ __device__ __forceinline__ uint32_t digest_of(int32_t t) {
    return t >= 0 ? (uint32_t)t % DIGEST_MOD : t == SEP ? DIGEST_SEP : DIGEST_DEAD;
}

__device__ __forceinline__ uint32_t digest4(const int32_t (&t)[4]) {
    return digest_of(t[0]) | (digest_of(t[1]) << 8) | (digest_of(t[2]) << 16) |
           (digest_of(t[3]) << 24);
}

// The plane of the whole corpus in one pass: 4 B read and 1 B written per slot.
__global__ void __launch_bounds__(256)
k_digest_build(const int32_t *__restrict__ ids, int64_t n_chunks, uint32_t *__restrict__ plane) {
    const int64_t n = n_chunks * (CHUNK / 4);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int4 v = reinterpret_cast<const int4 *>(ids)[i];
        const int32_t t[4] = {v.x, v.y, v.z, v.w};
        plane[i] = digest4(t);
    }
}

// The digest stream's ring: wave-loads of 16 B per lane (1 KiB: the digests of four chunks, lane L
// holding bytes 16 (L & 15) .. + 15 of chunk L >> 4), DG_RING of them per round, loaded DG_LEAD
// ahead.  A round covers 32 chunks: one bit each in the round's hit mask.
constexpr int DG_RING = 8;
constexpr int DG_LEAD = 6;
static_assert(DG_LEAD >= 2 && DG_LEAD <= DG_RING - 1, "digest ring lead");
static_assert(4 * DG_RING == 32, "a round's chunks fill a 32-bit hit mask");
// Chunks the region sums' walks read from either end of a rewritten region before its wave
// tallies the whole region instead (region_tally).
constexpr int DG_WALK = 2;
// Hit chunks whose loads are in flight while the exact path applies the first of them.
constexpr int DG_PF = 4;

// The scan's candidate-mask table, in dynamic LDS (k_apply_loop is launched with DG_TABLE bytes):
// one byte per byte pair lo | hi << 8, bit j set when the pair is a key of candidate j.  The
// pair test of a scan is then one byte read per pair, whatever the number of candidates.
constexpr int DG_TABLE = 65536;
static_assert(DG_TABLE % (16 * WG) == 0, "the workgroup zeroes the table in 16-byte stores");

// The sums of one region tallied from its int32 slots (the apply-only pass's count, chunk by
// chunk with synchronous loads): the digest stream's slow path, for a region whose first or last
// run is longer than the walks below read.
__device__ __forceinline__ RegionSum region_tally(const __amdgpu_buffer_rsrc_t rs, int nc, int lane) {
    Sink k{};
    k.ma = -1;
    Tally s;
    s.n_live = 0;
    s.lead_len = 0;
    s.prev = NONE;
    s.par = 0;
    s.first_tok = NONE;
    s.in_lead = 1;
    s.seen = 0;
    Defer df;
    Prep pp;
    pp.ok = 0;
    Chunk prv;
    prv.len = 0;
    for (int c = 0; c < nc; ++c) {
        Chunk cur;
        const auto x = __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, c * (CHUNK * 4), 0);
        cur.t[0] = (int)x[0];
        cur.t[1] = (int)x[1];
        cur.t[2] = (int)x[2];
        cur.t[3] = (int)x[3];
        finish_load(cur);
        if (cur.len == 0) continue;
        if (prv.len) count_chunk<MODE_NONE, false>(prv, cur.first, lane, s, k, df, pp);
        prv = cur;
    }
    if (prv.len) count_chunk<MODE_NONE, true>(prv, NONE, lane, s, k, df, pp);
    RegionSum o;
    o.n_live = s.n_live;
    o.first_tok = s.n_live ? s.first_tok : NONE;
    o.last_tok = s.n_live ? s.prev : NONE;
    o.uniform = s.n_live && s.in_lead ? 1 : 0;
    o.lead_len = s.in_lead ? s.n_live : s.lead_len;
    o.trail_odd = s.par ^ 1;
    return o;
}

// The sums of a region the digest stream rewrote (n_live = its live slots now): the first run from
// the first non-empty chunk on, the last run from the last non-empty chunk back, each walk reading
// at most DG_WALK non-empty chunks; past that, the whole region's tally.  Field for field what the
// int32 stream's count leaves (step_body).
__device__ __forceinline__ RegionSum region_resum(const __amdgpu_buffer_rsrc_t rs, int nc, int lane,
                                                  int64_t n_live) {
    RegionSum o;
    o.n_live = n_live;
    o.lead_len = 0;
    o.first_tok = NONE;
    o.last_tok = NONE;
    o.uniform = 0;
    o.trail_odd = 1;
    if (n_live <= 0) return o;
    auto load = [&](Chunk &q, int c) __attribute__((always_inline)) {
        const auto x = __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, c * (CHUNK * 4), 0);
        q.t[0] = (int)x[0];
        q.t[1] = (int)x[1];
        q.t[2] = (int)x[2];
        q.t[3] = (int)x[3];
        finish_load(q);
    };
    // live slots of q that differ from t, per plane e
    auto differ = [&](const Chunk &q, int32_t t, unsigned long long (&m)[4]) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = __ballot(q.t[e] != t) & lanes_upto(q.len, e);
    };
    // forward: the first live token and the length of its run
    int64_t lead = 0;
    bool open = true, slow = false;
    int walked = 0;
    for (int c = 0; c < nc && open; ++c) {
        Chunk q;
        load(q, c);
        if (q.len == 0) continue;
        if (walked == DG_WALK) {
            slow = true;
            break;
        }
        ++walked;
        if (lead == 0) o.first_tok = q.first;
        if (o.first_tok < 0) {   // (a separator is a run of its own)
            lead = 1;
            break;
        }
        unsigned long long m[4];
        differ(q, o.first_tok, m);
        int f = q.len;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (m[e]) f = min(f, 4 * (int)__builtin_ctzll(m[e]) + e);
        lead += f;
        if (f < q.len) open = false;
        if (lead == n_live) break;
    }
    o.lead_len = lead;
    if (!slow && lead == n_live) {   // one single run
        o.last_tok = o.first_tok;
        o.uniform = 1;
        o.trail_odd = (int32_t)(n_live & 1);
        return o;
    }
    // backward: the last live token and the length of its run (it starts inside the region)
    int64_t trail = 0;
    walked = 0;
    for (int c = nc - 1; c >= 0 && !slow; --c) {
        Chunk q;
        load(q, c);
        if (q.len == 0) continue;
        if (walked == DG_WALK) {
            slow = true;
            break;
        }
        ++walked;
        if (trail == 0) o.last_tok = q.last;
        if (o.last_tok < 0) {
            trail = 1;
            break;
        }
        unsigned long long m[4];
        differ(q, o.last_tok, m);
        int kmax = -1;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (m[e]) kmax = max(kmax, 4 * (63 - (int)__builtin_clzll(m[e])) + e);
        trail += q.len - 1 - kmax;
        if (kmax >= 0) break;
    }
    o.trail_odd = (int32_t)(trail & 1);
    if (slow) return region_tally(rs, nc, lane);
    return o;
}

// The delta form's stream over the digest plane: the structure of step_body<MERGE_XY, MODE_NONE,
// .., SITES> (one wave per region, its chunks in order, RegionCarry for the region's edges) with
// digest words in the ring.  With (da, db) the digests of (a, b), a chunk goes to the exact path
// (its 1 KiB of int32 slots loaded, apply_chunk as in the int32 stream) when
//  - some byte equals da and the byte to its right equals db (the right of a chunk's byte 255 is
//    byte 0 of the next chunk, already in the ring; of the region's last byte, next_tok's digest);
//  - some byte equals da and the byte to its right is DIGEST_DEAD: that a-alike is the chunk's
//    last live token, its true neighbour lies beyond a dead tail or an empty chunk;
//  - a match is pending (ap.match): the chunk before ended in a real `a` whose neighbour, a real
//    `b`, is this chunk's first live token and has to go (an empty chunk hands the match on).
// Complete for a != b: a site is a live `a` whose next live token is `b`, and that `b` is either
// the next byte of the same chunk or `a` is its chunk's last live token.  A false hit (a digest
// alias) costs one chunk load.  The test is a lookup: a scan first fills a table in LDS (`tab`,
// DG_TABLE bytes, one per byte pair lo | hi << 8) with bit j set at the two keys of candidate j,
// (da, db) and (da, DIGEST_DEAD); a lane then reads the byte of each of its 16 pairs and ors them,
// and a wave-load whose lanes all read zero is done with one ballot.  Two candidates may share a
// byte (digests alias, and the second key depends on `a` alone): each keeps its own bit.  The
// table is the workgroup's: every wave zeroes a part, wave 0 derives the candidates, sets their
// entries and publishes the set of slots in use (wg_acc[3]); waves without a region take part
// up to the second barrier and leave.
// A rewritten chunk's digests are stored with it and the chunk is listed for k_site_delta.  The
// region's sums are left as the last pass wrote them unless a chunk was rewritten; then n_live
// loses the removed slots and the edge fields are read again (region_resum).
// A scan (use < 0) streams the plane once and answers the first two conditions for up to `ncand`
// pairs: the decided one, whose hit chunks are applied at once, and the predicted next ones, whose
// answers are stored as rows of bits (DigestLists).  With use >= 0 nothing is streamed: the decided
// pair's hit chunks are those of its cached row `use`.  Either way the hit chunks are applied in
// order by one copy of the exact path, the loads of the next DG_PF of them in flight (apply_words).
__device__ __forceinline__ void digest_body(int32_t *__restrict__ ids, uint32_t *__restrict__ plane,
                                            int64_t n_chunks, int64_t cpr, int R,
                                            const RegionCarry *__restrict__ carry, int32_t ma,
                                            int32_t mb, int32_t mc, RegionSum *__restrict__ sums,
                                            unsigned long long *__restrict__ replaced,
                                            uint32_t *__restrict__ site_list,
                                            uint32_t *__restrict__ site_n,
                                            unsigned long long *__restrict__ n_hits,
                                            DigestLists *__restrict__ dl,
                                            uint32_t *__restrict__ rows, int ncand, int use,
                                            uint32_t *wg_acc, uint4 *tab) {
    const int lane = threadIdx.x & 63;
    const int r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES_PER_WG + (threadIdx.x >> 6)));
    const bool scan = use < 0;   // (the same in every wave of the grid)
    uint32_t cmask = 1u;         // the candidate slots in use: bit j
    if (scan) {
        // (both barriers are met by every wave of the workgroup, with a region or without)
#pragma unroll
        for (int i = 0; i < DG_TABLE / 16 / WG; ++i) tab[i * WG + threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        if (threadIdx.x < 64) {
            // The candidates of a scan: the decided pair in slot 0, and in slots 1 .. ncand - 1
            // the pairs of the largest block keys the last k_reduce_table left
            // (DigestLists::bkey), the table's order by pack_key being the order of the next
            // merges unless a merge between disturbs it.  Only a guess: a != b, 16 W < n_chunks
            // (the delta form's rule), not the decided pair itself; wave 0 of every workgroup
            // derives the same ones, that of workgroup 0 records them.
            int32_t ca[DIGEST_CAND], cb[DIGEST_CAND];
            static_for<0, DIGEST_CAND>([&](auto J) __attribute__((always_inline)) {
                ca[decltype(J)::value] = -1;
                cb[decltype(J)::value] = -1;
            });
            ca[0] = ma;
            cb[0] = mb;
            if (ncand > 1) {
                // (key << 8 | 255 - block: one owner per value)
                unsigned long long s[HOT / 64];
#pragma unroll
                for (int q = 0; q < HOT / 64; ++q) {
                    const unsigned long long k = dl->bkey[q * 64 + lane];
                    s[q] = k ? (k << 8) | (unsigned long long)(255 - (q * 64 + lane)) : 0ull;
                }
                static_for<1, DIGEST_CAND>([&](auto J) __attribute__((always_inline)) {
                    constexpr int j = decltype(J)::value;
                    if (j >= ncand) return;
                    for (int t = 0; t < 3 && ca[j] < 0; ++t) {
                        unsigned long long m = 0;
#pragma unroll
                        for (int q = 0; q < HOT / 64; ++q) m = s[q] > m ? s[q] : m;
                        m = wave_max_u64(m);
                        if (m == 0ull) break;
#pragma unroll
                        for (int q = 0; q < HOT / 64; ++q) s[q] = s[q] == m ? 0ull : s[q];
                        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m);
                        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32));
                        const unsigned long long key = (((unsigned long long)hi << 32) | lo) >> 8;
                        const int32_t pb = 255 - (int32_t)(lo & 255u);
                        const int32_t pa = (int32_t)(0x1FFFFu - (uint32_t)(key & 0x1FFFFu)) - pb;
                        const bool ok = pa >= 0 && pa < HOT && pa != pb && !(pa == ma && pb == mb) &&
                                        (int64_t)(key >> 17) * 16 < n_chunks;
                        ca[j] = ok ? pa : -1;
                        cb[j] = ok ? pb : -1;
                    }
                });
            }
            uint32_t *const tabw = reinterpret_cast<uint32_t *>(tab);
            static_for<0, DIGEST_CAND>([&](auto J) __attribute__((always_inline)) {
                constexpr int j = decltype(J)::value;
                if (blockIdx.x == 0 && lane == 0) {
                    dl->pa[j] = j ? ca[j] : -1;   // (slot 0 is applied now and never cached)
                    dl->pb[j] = j ? cb[j] : -1;
                }
                if (ca[j] < 0) return;
                cmask |= 1u << j;
                // lane 0 sets the entry of (da, db), lane 1 that of (da, DIGEST_DEAD)
                const uint32_t k = digest_of(ca[j]) | ((lane ? DIGEST_DEAD : digest_of(cb[j])) << 8);
                if (lane < 2)
                    __hip_atomic_fetch_or(&tabw[k >> 2], (1u << j) << (8 * (k & 3u)), __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_WORKGROUP);
            });
            if (lane == 0) wg_acc[3] = cmask;
        }
        __syncthreads();
        cmask = (uint32_t)__builtin_amdgcn_readfirstlane((int)wg_acc[3]);
    }
    if (r >= R) return;
    const int64_t c0 = (int64_t)r * cpr;
    const int64_t c1 = min(c0 + cpr, n_chunks);
    const int nc = (int)(c1 > c0 ? c1 - c0 : 0);
    const RegionCarry rc = carry[r];
    Apply ap;
    ap.prev = rc.prev_tok;
    ap.par = 0;
    ap.match = 0;
    ap.n_match = 0;
    ap.sites = site_list + c0;
    ap.n_sites = 0;
    ap.c0 = (uint32_t)c0;
    Prep pp;
    pp.ok = 0;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        ids + c0 * CHUNK, 0, nc * CHUNK * 4, 0x00020000);
    // (the plane's loads past the region return 0 and are masked off below)
    const __amdgpu_buffer_rsrc_t ps = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<uint8_t *>(plane) + c0 * CHUNK, 0, nc * CHUNK, 0x00020000);
    auto live_from = [&](int c, int32_t f0) -> int32_t {
        int32_t v = c < nc ? f0 : rc.next_tok;
        if (__builtin_expect(v < SEP, 0)) {
            int q = c + 1;
            for (; q < nc; ++q) {
                v = __builtin_amdgcn_readfirstlane(
                    (int)__builtin_amdgcn_raw_buffer_load_b32(rs, 0, q * (CHUNK * 4), 0));
                if (v >= SEP) break;
            }
            if (q >= nc) v = rc.next_tok;
        }
        return v;
    };
    auto slot0 = [&](int c) -> int32_t {
        return __builtin_amdgcn_readfirstlane(
            (int)__builtin_amdgcn_raw_buffer_load_b32(rs, 0, c * (CHUNK * 4), 0));
    };
    uint32_t hits = 0;
    int32_t removed = 0;
    // A chunk's 1 KiB of slots, and slot 0 of its successor in the same round trip (of the
    // region's last chunk live_from takes next_tok instead).
    auto load_chunk = [&](int c) __attribute__((always_inline)) {
        return __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, c * (CHUNK * 4), 0);
    };
    auto load_slot0 = [&](int c) __attribute__((always_inline)) {
        return (int32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, 0, c * (CHUNK * 4), 0);
    };
    using Slots = decltype(load_chunk(0));
    // the exact path of chunk c, its slots x and its successor's slot 0 loaded: what the int32
    // stream's stage does for it
    auto exact = [&](int c, const Slots x, const int32_t f1) __attribute__((always_inline)) {
        Chunk q;
        q.t[0] = (int)x[0];
        q.t[1] = (int)x[1];
        q.t[2] = (int)x[2];
        q.t[3] = (int)x[3];
        finish_load(q);
        ++hits;
        if (q.len == 0) return;   // (an empty chunk hands the pending match on)
        const int32_t nx = live_from(c + 1, f1);
        const int len0 = q.len;
        const uint32_t ns0 = ap.n_sites;
        apply_chunk<MERGE_XY, false, true>(q, nx, ma, mb, mc, rs, c, lane, ap, pp, 0u);
        if (ap.n_sites != ns0) {
            removed += len0 - q.len;
            __builtin_amdgcn_raw_buffer_store_b32(digest4(q.t), ps, lane * 4, c * CHUNK, 0);
        }
    };
    if (nc > 0) {
        // does the token before the region match the region's first live token?
        const int32_t f = live_from(0, slot0(0));
        ap.match = ((uint32_t)(ap.prev ^ ma) | (uint32_t)(f ^ mb)) == 0u;
        const uint8_t *const tb = reinterpret_cast<const uint8_t *>(tab);
        // the rows of this region's slots: words [j * wpr, j * wpr + nw) of its block, the index
        // in the bounds-checked offset (a word past the block reads 0 and is never written)
        const int wpr = (int)((cpr + 31) >> 5), nw = (nc + 31) >> 5;
        const __amdgpu_buffer_rsrc_t rws = __builtin_amdgcn_make_buffer_rsrc(
            rows + (int64_t)r * DIGEST_CAND * wpr, 0, DIGEST_CAND * wpr * 4, 0x00020000);
        // the byte after the region's last: the digest of the first live token after the region,
        // in byte 0 of lane lp of wave-load gp
        const uint32_t dnext = digest_of(rc.next_tok);
        const int gp = nc >> 2, lp = (nc & 3) * 16;
        auto load = [&](uint4 &q, int g) __attribute__((always_inline)) {
            const auto x = __builtin_amdgcn_raw_buffer_load_b128(ps, lane * 16, g * (4 * CHUNK), BPE_LOAD_AUX);
            q.x = x[0];
            q.y = x[1];
            q.z = x[2];
            q.w = x[3];
        };
        uint32_t rm[DIGEST_CAND];   // the round's hit chunks, per candidate
        auto stage = [&](const uint4 &cur, const uint4 &nxt, uint4 &fre, int g, int i)
                         __attribute__((always_inline)) {
            load(fre, g + DG_LEAD);
            uint32_t d0 = cur.x;
            if (g == gp) d0 = lane == lp ? dnext : d0;
            const uint32_t fill = (g + 1 == gp && lp == 0) ? dnext
                                                           : (uint32_t)bcast((int32_t)nxt.x, 0);
            const uint32_t d[5] = {d0, cur.y, cur.z, cur.w,
                                   (uint32_t)from_next((int32_t)d0, (int32_t)fill)};
            // the table bytes of the lane's 16 pairs (byte k with the byte to its right), ored:
            // the candidates some pair of the lane is a key of
            uint32_t m = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                m |= tb[d[e] & 0xFFFFu];
                m |= tb[(d[e] >> 8) & 0xFFFFu];
                m |= tb[d[e] >> 16];
                m |= tb[__builtin_amdgcn_alignbyte(d[e + 1], d[e], 3) & 0xFFFFu];
            }
            // (the chunks of the wave-load that lie in the region)
            const int v = nc - 4 * g;
            const unsigned long long valid = v >= 4 ? ~0ull : v <= 0 ? 0ull : ((1ull << (16 * v)) - 1ull);
            // (nearly every wave-load ends here)
            if ((__ballot(m != 0u) & valid) == 0ull) return;
            static_for<0, DIGEST_CAND>([&](auto J) __attribute__((always_inline)) {
                constexpr int j = decltype(J)::value;
                if (!(cmask >> j & 1u)) return;
                const unsigned long long H = __ballot((m >> j & 1u) != 0u) & valid;
                if (H != 0ull) {
                    const uint32_t lo = (uint32_t)H, hi = (uint32_t)(H >> 32);
                    const uint32_t b = (uint32_t)((lo & 0xFFFFu) != 0u) | ((uint32_t)((lo >> 16) != 0u) << 1) |
                                       ((uint32_t)((hi & 0xFFFFu) != 0u) << 2) | ((uint32_t)((hi >> 16) != 0u) << 3);
                    rm[j] |= b << (4 * i);
                }
            });
        };
        // The hit chunks of row words [wb, wb + n) (word wb + L in lane L of v) in order, the
        // loads of the next DG_PF of them in flight: a chunk's content changes only when the
        // chunk itself is processed, and the wave goes forward, so a chunk loaded early is the
        // chunk as it will be met.  A pending match takes the chunks from `nextc` on as they are
        // (synchronous loads), listed or not; `last`: after the region's last word, up to its end.
        int nextc = 0;   // every chunk before it is done
        auto apply_words = [&](const uint32_t v, const int wb, const int n, const bool last)
                               __attribute__((always_inline)) {
            unsigned long long nz = __ballot(v != 0u);
            if (n < 64) nz &= (1ull << n) - 1ull;
            uint32_t bits = 0;
            int wj = 0;
            bool fin = !last;   // (the end of the region is met once, as the hit `nc`)
            auto next_hit = [&]() __attribute__((always_inline)) -> int {
                if (bits == 0u && nz != 0ull) {
                    wj = (int)__builtin_ctzll(nz);
                    nz &= nz - 1ull;
                    bits = (uint32_t)bcast((int32_t)v, wj);
                }
                if (bits != 0u) {
                    const int c = 32 * (wb + wj) + (int)__builtin_ctz(bits);
                    bits &= bits - 1u;
                    if (c < nc) return c;
                    bits = 0u;   // (no row holds a bit past the region: the scan masks them)
                    nz = 0ull;
                }
                if (fin) return -1;
                fin = true;
                return nc;
            };
            int cs[DG_PF];
            Slots X[DG_PF];
            int32_t F[DG_PF];
            auto fetch = [&](auto I) __attribute__((always_inline)) {
                constexpr int i = decltype(I)::value;
                cs[i] = next_hit();
                if (cs[i] >= 0 && cs[i] < nc) {
                    X[i] = load_chunk(cs[i]);
                    F[i] = load_slot0(cs[i] + 1);
                }
            };
            static_for<0, DG_PF>(fetch);
            while (cs[0] >= 0) {
                const int c = cs[0];
                for (;;) {
                    const bool pre = ap.match && nextc < c;
                    if (!pre && c >= nc) break;
                    const int cc = pre ? nextc : c;
                    Slots x = X[0];
                    int32_t f1 = F[0];
                    if (pre) {
                        x = load_chunk(cc);
                        f1 = load_slot0(cc + 1);
                    }
                    exact(cc, x, __builtin_amdgcn_readfirstlane(f1));
                    nextc = cc + 1;
                    if (!pre) break;
                }
                static_for<1, DG_PF>([&](auto I) __attribute__((always_inline)) {
                    constexpr int i = decltype(I)::value;
                    cs[i - 1] = cs[i];
                    X[i - 1] = X[i];
                    F[i - 1] = F[i];
                });
                fetch(std::integral_constant<int, DG_PF - 1>{});
            }
        };
        uint4 S[DG_RING];   // (constant indices only: the ring stays in registers)
        if (scan) static_for<0, DG_LEAD>([&](auto i) __attribute__((always_inline)) { load(S[i], i); });
        for (int wb = 0; wb < nw; wb += 64) {
            const int n = min(64, nw - wb);
            uint32_t v = 0;
            if (!scan) {
                // the decided pair's cached row
                if (lane < n)
                    v = __builtin_amdgcn_raw_buffer_load_b32(rws, (use * wpr + wb + lane) * 4, 0, 0);
            } else {
                // the plane streamed once: a round's masks are a word of each candidate's row
                uint32_t row[DIGEST_CAND];
                static_for<0, DIGEST_CAND>([&](auto J) __attribute__((always_inline)) { row[decltype(J)::value] = 0; });
                for (int w = 0; w < n; ++w) {
                    const int g0 = (wb + w) * DG_RING;
                    static_for<0, DIGEST_CAND>([&](auto J) __attribute__((always_inline)) { rm[decltype(J)::value] = 0; });
                    static_for<0, DG_RING>([&](auto I) __attribute__((always_inline)) {
                        constexpr int i = decltype(I)::value;
                        stage(S[i], S[(i + 1) % DG_RING], S[(i + DG_LEAD) % DG_RING], g0 + i, i);
                    });
                    static_for<0, DIGEST_CAND>([&](auto J) __attribute__((always_inline)) {
                        constexpr int j = decltype(J)::value;
                        row[j] = lane == w ? rm[j] : row[j];
                    });
                }
                static_for<1, DIGEST_CAND>([&](auto J) __attribute__((always_inline)) {
                    constexpr int j = decltype(J)::value;
                    if ((cmask >> j & 1u) && lane < n)
                        __builtin_amdgcn_raw_buffer_store_b32(row[j], rws, (j * wpr + wb + lane) * 4, 0, 0);
                });
                v = row[0];
            }
            apply_words(v, wb, n, wb + 64 >= nw);
        }
    }
    if (ap.n_sites) {
        const RegionSum o = region_resum(rs, nc, lane, sums[r].n_live - removed);
        if (lane == 0) sums[r] = o;
    }
    if (lane == 0) {
        site_n[r] = ap.n_sites;
        // The two counters go through the workgroup (wg_acc: replaced, hits, waves done, and the
        // scan's candidate slots; zero at the start): a list iteration's waves all end within microseconds of each other, and
        // thousands of atomics on one address would then be the launch's critical path.  The
        // wave that finds itself last adds the workgroup's sums.
        if (ap.n_match) __hip_atomic_fetch_add(&wg_acc[0], (uint32_t)ap.n_match, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (hits) __hip_atomic_fetch_add(&wg_acc[1], hits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const int active = min(WAVES_PER_WG, R - (int)blockIdx.x * WAVES_PER_WG);
        const uint32_t done = __hip_atomic_fetch_add(&wg_acc[2], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        if ((int)done + 1 == active) {
            const uint32_t m = __hip_atomic_load(&wg_acc[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint32_t h = __hip_atomic_load(&wg_acc[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (m) atomicAdd(replaced, (unsigned long long)m);
            if (h) atomicAdd(n_hits, (unsigned long long)h);
        }
    }
}

// The delta form's apply-only stream: the merge in the LoopCtl applied as by k_apply<MERGE_XY> (no
// LDS table, no slab, no pair counted; the region sums kept, so k_runs<MODE_NONE> rebuilds the
// carries and a full pass can follow), every rewritten chunk listed for k_site_delta.  With a
// fresh digest plane (LoopCtl::digest_ok) the sites are found through it (digest_body), else by
// streaming the int32 slots: one launch, a uniform branch between the two bodies.
__global__ void __launch_bounds__(WG)
k_apply_loop(int32_t *__restrict__ ids, int64_t n_chunks, int64_t cpr, int R,
             const RegionCarry *__restrict__ carry, LoopCtl *__restrict__ ctl,
             RegionSum *__restrict__ sums, unsigned long long *__restrict__ replaced,
             uint32_t *__restrict__ site_list, uint32_t *__restrict__ site_n,
             uint32_t *__restrict__ plane, DigestLists *__restrict__ dl,
             uint32_t *__restrict__ rows) {
    if (ctl->status != LOOP_RUN || !ctl->delta) return;
    if (ctl->digest_ok) {
        // (from the decided pair's cached row when the decision found one, DigestLists::use; else
        // the plane streamed for it and the predicted pairs)
        // (dg_table: the scan's DG_TABLE bytes of dynamic LDS, which only a scan touches)
        extern __shared__ uint4 dg_table[];
        __shared__ uint32_t wg_acc[4];
        if (threadIdx.x < 4) wg_acc[threadIdx.x] = 0;
        __syncthreads();
        digest_body(ids, plane, n_chunks, cpr, R, carry, ctl->a, ctl->b, ctl->c, sums, replaced,
                    site_list, site_n, &ctl->digest_hits, dl, rows, ctl->digest_cand, dl->use, wg_acc,
                    dg_table);
    } else
        step_body<MERGE_XY, MODE_NONE, true, true, true>(
            nullptr, ids, n_chunks, cpr, R, carry, ctl->a, ctl->b, ctl->c, nullptr, nullptr,
            ColdTable{}, nullptr, sums, replaced, nullptr, nullptr, site_list, site_n);
}

}  // namespace bpe
