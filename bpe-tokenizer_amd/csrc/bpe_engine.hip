// bpe_engine.hip — libbpe: host side of the MI355X BPE merge-training engine + the C ABI of
// include/bpe.h.  One context = one HIP device + one stream + one corpus shard in HBM.
//
// The corpus is never compacted per merge: chunks stay left-packed and a merge rewrites only the
// chunks it touches.  One streaming kernel (k_step) does both halves of an iteration:
//   applyMerge(a, b, c)   (core.ts:332-360)  -> k_step<MERGE>: apply to every chunk, then count the
//                                               post-merge pairs, k_runs, k_reduce_hot
//   findNextMerge(opts)   (core.ts:247-326)  -> (k_step<plain> only if no counts are cached)
//                                               k_argmax_hot/cold, k_collect, [k_tie (rule R3)]
// so a mergeUntil iteration streams the corpus exactly once.
#include "bpe_kernels.hip.h"
#include "bpe_pix.hip.h"
#include "bpe.h"
#include "bpe_ingest.hip.h"   // the corpus ingest from text (with bpe_text_front.hip.h, the encoder's front end)
#include "bpe_append.hip.h"   // the corpus append from encoded samples (bpe_add_sample_batch, the restore)
#include "bpe_export.hip.h"   // the corpus export (bpe_export_samples, bpe_export_text_batch)
#include "bpe_multi.h"
#include "bpe_utf8.hip.h"     // text as UTF-8: bytes -> units in front of the ingest (bpe_add_utf8_batch)
#include "bpe_lines.hip.h"    // lines as samples: texts -> samples in front of the ingest (bpe_add_lines_batch)
#include "bpe_skipgram.hip.h" // skip-gram pairs behind the export (bpe_export_skipgram)
#include "bpe_tools.h"

namespace bpe_step {
// (csrc/bpe_step.hip: the C3 hot path's pass, compiled with its own flags; the structures are
// the ones of bpe_kernels.hip.h, passed untyped)
hipError_t launch_step_loop_table(unsigned grid, hipStream_t s, int32_t *ids, int64_t n_chunks,
                                  int64_t cpr, int R, const void *carry, const void *ctl,
                                  uint32_t *partials, unsigned long long *spill, const void *ct,
                                  void *sums, unsigned long long *replaced);
hipError_t launch_apply_loop(unsigned grid, hipStream_t s, int32_t *ids, int64_t n_chunks,
                             int64_t cpr, int R, const void *carry, void *ctl, void *sums,
                             unsigned long long *replaced, uint32_t *site_list, uint32_t *site_n,
                             uint32_t *plane, void *lists, uint32_t *rows);
hipError_t launch_digest_build(hipStream_t s, const int32_t *ids, int64_t n_chunks, uint32_t *plane);
hipError_t launch_step_table(int merge, unsigned grid, hipStream_t s, int32_t *ids, int64_t n_chunks,
                             int64_t cpr, int R, const void *carry, int32_t ma, int32_t mb,
                             int32_t mc, uint32_t *partials, unsigned long long *spill,
                             const void *ct, const uint32_t *heavy, void *sums,
                             unsigned long long *replaced);
}

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace bpe;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(e_ == hipErrorOutOfMemory ? BPE_ERR_OOM : BPE_ERR_HIP,             \
                        std::string("bpe native: ") + #expr + ": " + hipGetErrorString(e_)); \
    } while (0)

inline void dfree(void *p) {
    if (p) (void)hipFree(p);
}

// mergeUntil iterations the device runs per host round trip (each ends in one sync)
constexpr int64_t LOOP_BATCH = 64;
// apply-only replay: merges per host round trip (their replacement counts come back together)
constexpr int64_t REPLAY_BATCH = 256;
// a digest plane that went stale inside a batch is rebuilt for the next one only if that batch
// took the delta form in at least this many iterations, and in at least half of its iterations
constexpr int64_t DIGEST_REBUILD_MIN = 4;

static_assert(TABLE_BINS == BPE_TABLE_BINS && HOT_BINS == BPE_HOT_BINS, "include/bpe.h table layout");
static_assert(MAX_CAND == BPE_MAX_CAND && LOOP_BATCH == BPE_LOOP_BATCH, "include/bpe.h rank loop sizes");
static_assert(XCHG_HDR == BPE_XCHG_HDR && XCHG_WORDS == BPE_XCHG_WORDS && TIE_WORDS == BPE_TIE_WORDS &&
                  DELTA_ROWS == BPE_DELTA_ROWS,
              "include/bpe.h exchange layout");
static_assert(DIGEST_MOD == BPE_DIGEST_MOD && DIGEST_SEP == BPE_DIGEST_SEP &&
                  DIGEST_DEAD == BPE_DIGEST_DEAD && DIGEST_CAND == BPE_DIGEST_CAND,
              "include/bpe.h digest plane");

template <typename T>
int dev_alloc(T **p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    hipError_t e = hipMalloc((void **)p, n * sizeof(T));
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? BPE_ERR_OOM : BPE_ERR_HIP,
                    std::string("bpe native: hipMalloc: ") + hipGetErrorString(e));
    return BPE_OK;
}

}  // namespace

struct bpe_ctx {
    // a corpus sharded over several devices (bpe_create_multi): every entry point forwards to
    // csrc/bpe_multi.cpp, which drives one single-device context per shard
    bpe_multi *multi = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    // corpus: n_chunks left-packed chunks + one all-SEP spare chunk
    int32_t *d_ids = nullptr, *d_tmp = nullptr;
    int64_t cap_slots = 0;
    int64_t n_chunks = 0;
    int64_t live_slots = 0;    // live slots (tokens + SEPs)
    int64_t n_samples = 0;
    int64_t n_live = 0;        // live tokens
    bool packed = true;        // live slots are a dense prefix (only the last chunk has a tail)
    // vocabulary
    std::vector<int32_t> h_len16;
    std::vector<int64_t> h_count;      // occurrences per token in the corpus (exact)
    int32_t *d_len16 = nullptr;
    int64_t cap_vocab = 0;
    int64_t len16_lo = 0;      // h_len16[len16_lo:] is not yet on the device
    // pass state
    uint32_t *d_partials = nullptr;
    int partials_wg = 0;         // workgroups the partial slab can hold
    unsigned long long *d_spill = nullptr, *d_hot = nullptr, *d_total = nullptr;   // d_hot: TABLE_BINS
    uint32_t *d_heavy = nullptr;
    RegionSum *d_sums = nullptr;
    RegionCarry *d_carry = nullptr;
    int64_t *d_outoff = nullptr;
    Result *d_res = nullptr, *h_res = nullptr;
    int2 *d_cand = nullptr;
    ColdTable cold{};
    // [0] n_used, [1] overflow, [2] n_blist, [3] sel_n0, [4] dead, [5] n_recomputed (ColdTable)
    uint32_t *d_cold_flags = nullptr;
    uint64_t cold_cap = 0;
    // an applied merge whose replacement count is still on the device (settled at the next sync)
    bool pending = false;
    int32_t pend_a = 0, pend_b = 0, pend_c = 0;
    int64_t pend_expect = -1;    // W the replacement count must equal (mergeUntil), -1 = any
    int2 *h_cand = nullptr;      // pinned: first MAX_CAND candidates come back with the Result
    bool counts_valid = false;   // d_hot + cold table describe the current corpus
    // d_hot's sketch half is an upper bound of the cold pairs' counts.  A MODE_FUSED pass leaves
    // it garbage (its LDS half holds the refresh hash there): every reader of the sketch recounts
    // first (table_ok)
    bool sketch_valid = false;
    uint64_t cold_used = 0;      // n_used of the cold table last reported to the host
    // The cold table holds the exact count of EVERY cold pair and is kept so merge by merge
    // (cold_refresh) instead of being rebuilt by exact passes: entered after consecutive exact
    // passes (a corpus whose winners are pairs of merged tokens, e.g. Zipf words)
    bool cold_exact = false;
    int exact_streak = 0;
    // with the cold table maintained, merge passes count incrementally (MODE_INCR: the hot bins are
    // maintained too, and a pass counts only the pairs the merge can change); BPE_FUSED=1 keeps
    // the full hot recount with the cold refresh riding along (MODE_FUSED) instead
    bool use_incr = true;
    // mergeUntil on the position index (bpe_set_mode BPE_MODE_INCREMENTAL, BPE_PIX=1): O(W) work
    // per merge instead of a pass (bpe_pix.hip.h)
    bool use_pix = false;
    struct PixState *pix = nullptr;
    bool carry_valid = false;    // d_sums / d_carry describe the current corpus and geometry
    int64_t cpr = 0;
    int R = 0, G = 0;
    int64_t last_replaced = 0;
    // best hot key of d_hot computed by the last k_reduce_table (valid for best_ml)
    bool best_ready = false;
    int64_t best_ml = 0;
    int64_t opt_max_length = 0;   // max_length of the last find (the reduce's filter)
    // stats: kernel spans are timed with events read back lazily (no sync in the merge loop)
    bool stats_on = false;
    bool span_mute = false;   // the device loop's untimed iterations (events cost ~µs each)
    uint64_t span_tick = 0;
    bpe_stats stats{};
    struct Span {
        hipEvent_t a, b;
        int kind;   // 0 stream pass, 1 selection, 2 tie pass
    };
    std::vector<Span> spans;
    std::vector<hipEvent_t> ev_pool;
    // device-resident mergeUntil loop: control block + merge log (pinned host mirrors)
    LoopCtl *d_ctl = nullptr, *h_ctl = nullptr;
    long long *d_log = nullptr, *h_log = nullptr;
    // the delta form of the table-state loop: the chunks a pass rewrote, a segment of cpr entries
    // per region (d_sites, sites_cap entries) and each region's count (d_site_n)
    uint32_t *d_sites = nullptr, *d_site_n = nullptr;
    int64_t sites_cap = 0;
    // the digest plane of the delta form's stream: one byte per slot of d_ids (digest_cap bytes).
    // Stale unless proven fresh: digest_valid says it matches d_ids.  Every function that enqueues
    // a write of d_ids clears it (digest_stale, with the writer's class: DigestWriter below); the
    // only proof of freshness is a build, or a batch's control block that comes back with
    // digest_ok still set (digest_end_batch).  digest_changed: stale by a write from outside the
    // merge loop since the last batch (the next batch rebuilds); otherwise a stale plane is
    // rebuilt only after a batch that took the delta form in at least DIGEST_REBUILD_MIN and at
    // least half of its iterations (last_delta of last_done).
    uint32_t *d_digest = nullptr;
    int64_t digest_cap = 0;
    bool digest_valid = false, digest_changed = true;
    // the hit lists of the digest stream (DigestLists: the cached pairs and the block keys the
    // scan predicts from) and their rows (lists_cap words: R x DIGEST_CAND x ceil(cpr / 32)).
    // They live and die with the plane: digest_stale drops them with it (lists_valid), and the
    // batch that finds them dropped, or the geometry or the candidate cap changed, clears the
    // device's copy before its first iteration (digest_begin_batch).
    DigestLists *d_lists = nullptr;
    uint32_t *d_rows = nullptr;
    int64_t lists_cap = 0, lists_cpr = 0;
    int lists_R = 0, lists_cand = 0;
    bool lists_valid = false;
    int64_t last_delta = 0, last_done = 0;
    unsigned int *d_ticket = nullptr;   // last-block tickets (k_tie_fused, k_select_maint; zero between launches)
    BlockBest *d_brec = nullptr;        // k_select_maint's per-block bests
    // apply-only replay: per-merge replacement counts
    unsigned long long *d_repl = nullptr, *h_repl = nullptr;
    // sharded device loop (one rank): the caller's all-reduced exchange buffer (include/bpe.h
    // BPE_XCHG_*: header + this shard's table, or + the delta rows) and tie positions
    unsigned long long *rl_table = nullptr, *rl_tie = nullptr;
    int rl_rank = 0, rl_world = 1;
    int64_t rl_base = 0, rl_enqueued = 0, rl_max_length = 0;
    int64_t rl_words = 0;   // words of the exchange all-reduced per iteration (this batch)
    bool rl_open = false;
    // d_hot and the cold table hold the GLOBAL counts of a sharded corpus, replicated on every
    // rank (bpe_set_global_counts): the rank loop keeps them merge by merge from the all-reduced
    // delta rows.  Anything that needs this shard's own counts leaves that state first.
    bool rl_global = false;
    // the last batch's last merge left its delta rows in rl_table, not yet all-reduced: the next
    // batch's first exchange carries them (same buffer)
    bool rl_delta_pending = false;
    int32_t rl_last_a = 0, rl_last_b = 0, rl_last_c = 0;
    int64_t rl_last_w = -1;
    // the cold table holds this shard's exact count of every cold pair (bpe_cold_counts)
    bool cold_list = false;
    // the global state of a sharded corpus lives in the position index (bpe_set_mode
    // BPE_MODE_INCREMENTAL, bpe_pix.hip.h): c->pix holds this shard's lists and the GLOBAL counts
    // between rank loop batches, and the corpus is in the index's slot layout until it is dropped
    bool rl_pix = false;
    uint64_t pix_min_cap = 0;    // (the next index build's least table size)
    // sharded incremental mode, compact exchange: entries of L and of R the next batch's exchange
    // holds (0: not known yet, every token id; sized from the largest need of the batches before)
    // the lane layout of the sharded incremental exchange: the last merge's count (0: unknown),
    // the layout {bits, lanes per word, right side's first word} of this batch and of the batch
    // whose last merge's lanes are pending
    unsigned long long pix_w_last = 0;
    uint32_t pix_lane[3] = {0, 0, 0}, pix_lane_prev[3] = {0, 0, 0};
    int64_t pix_nw_last = 0;   // words the last rank-loop batch all-reduced (its pending merge's)
    bool pix_first_pending = false;
    // checking (bpe_tools.h bpe_debug_pix_hook): called by pix_merge_until while its index is live,
    // and the merges per host round trip it then makes (0: PIX_BATCH)
    void (*pix_hook)(void *user, int where) = nullptr;
    void *pix_hook_user = nullptr;
    int64_t pix_dbg_batch = 0;
    // the corpus ingest from text: char table, scratch and counters (made by its first call)
    struct IngestState *ing = nullptr;
    // the corpus append from encoded samples: scratch and counters (made by its first call)
    struct AppendState *app = nullptr;
    // the corpus export: scratch and counters (made by its first call)
    struct ExportState *exp = nullptr;
    // text as UTF-8: the transcode's scratch and counters (made by its first call)
    Utf8State *u8 = nullptr;
    LinesState *ln = nullptr;
    SgState *sg = nullptr;    // skip-gram pairs of exported samples (made by its first call)
};

void ingest_free(bpe_ctx *c);
void append_free(bpe_ctx *c);
void export_free(bpe_ctx *c);

namespace {

int set_device(bpe_ctx *c) {
    HIP_TRY(hipSetDevice(c->device));
    return BPE_OK;
}

}  // namespace
int pix_finish(bpe_ctx *c);
namespace {

// Before anything that reads or updates this shard's own counts: global tables (the sharded
// maintained state) are dropped, and the next use recounts.  A sharded position index is dropped
// too: the corpus goes back to the chunk layout.
int leave_global(bpe_ctx *c) {
    if (!c->rl_global) return BPE_OK;
    c->rl_global = false;
    c->rl_delta_pending = false;
    c->counts_valid = c->sketch_valid = c->best_ready = false;
    c->cold_exact = false;
    c->cold_list = false;
    if (c->rl_pix) {
        c->rl_pix = false;
        return pix_finish(c);
    }
    return BPE_OK;
}
#define LEAVE_GLOBAL(c)                   \
    do {                                  \
        const int lg_ = leave_global(c);  \
        if (lg_) return lg_;              \
    } while (0)

// ---- the digest plane's freshness (bpe_ctx::d_digest) ------------------------------------------
// Who writes d_ids, by what the write means for a stale plane:
//  WRITER_LOOP     the merge loop itself: a host-path merge (enqueue_pass), a pass of the device
//                  loop (enqueue_loop_pass: the full form, or a batch without the plane) and a
//                  compaction.  The loop goes on as before, so whether the next batch rebuilds is
//                  left to the last batch's delta share.
//  WRITER_OUTSIDE  everything else: ingest and a replaced corpus (seal_packed), a replay
//                  (enqueue_apply), the position index (its build merges in place, pix_finish
//                  writes the corpus back) and the rank loop's passes.  The next batch rebuilds.
enum DigestWriter { WRITER_LOOP, WRITER_OUTSIDE };

// d_ids is about to be written (or replaced) by something that does not keep the digest plane.
void digest_stale(bpe_ctx *c, DigestWriter w) {
    c->digest_valid = false;
    c->lists_valid = false;   // (a list is a view of the plane: compaction even moves its chunks)
    if (w == WRITER_OUTSIDE) c->digest_changed = true;
}

// Before a batch of the device loop whose iterations may take the delta form: whether their
// stream reads the digest plane (BPE_DIGEST=0 keeps the int32 stream everywhere, for A/B and
// checking; read per batch).  A stale plane is rebuilt here when the corpus was written from
// outside the merge loop since the last batch (the first batch after such a change always
// builds), and otherwise only if the last batch took the delta form in at least
// DIGEST_REBUILD_MIN and at least half of its iterations: a build costs about 1.3 int32 streams,
// and a batch of heavy merges would clear the plane again at once.  If the plane cannot be
// allocated the batch runs on the int32 stream.
int digest_begin_batch(bpe_ctx *c, bool *fresh, int *cand) {
    *fresh = false;
    // (BPE_DIGEST_CAND=n caps the candidates of a plane stream, 1 .. the constant; read per batch;
    // at 1 every delta iteration scans: the A/B and checking knob)
    const char *cknob = getenv("BPE_DIGEST_CAND");
    *cand = cknob ? std::min(std::max(atoi(cknob), 1), DIGEST_CAND) : DIGEST_CAND;
    const char *gknob = getenv("BPE_DIGEST");
    if ((gknob && atoi(gknob) == 0) || c->n_chunks <= 0) return BPE_OK;
    if (c->digest_cap < c->n_chunks * CHUNK) {
        dfree(c->d_digest);
        c->d_digest = nullptr;
        c->digest_cap = 0;
        c->digest_valid = false;
        const int64_t cap = (c->cap_slots > 0 ? c->cap_slots : c->n_chunks * CHUNK);
        void *p = nullptr;
        if (hipMalloc(&p, (size_t)cap) != hipSuccess) {
            (void)hipGetLastError();
            return BPE_OK;
        }
        c->d_digest = static_cast<uint32_t *>(p);
        c->digest_cap = cap;
    }
    if (!c->digest_valid) {
        if (c->digest_changed ||
            (c->last_delta >= DIGEST_REBUILD_MIN && 2 * c->last_delta >= c->last_done)) {
            HIP_TRY(bpe_step::launch_digest_build(c->stream, c->d_ids, c->n_chunks, c->d_digest));
            c->digest_valid = true;
            if (c->stats_on) c->stats.digest_builds += 1;
        }
        c->digest_changed = false;
    }
    *fresh = c->digest_valid;
    if (!c->digest_valid) return BPE_OK;
    const int64_t words = (int64_t)c->R * DIGEST_CAND * ((c->cpr + 31) / 32);
    if (c->lists_cap < words) {
        dfree(c->d_rows);
        c->d_rows = nullptr;
        c->lists_cap = 0;
        c->lists_valid = false;
        if (dev_alloc(&c->d_rows, (size_t)words)) {
            // (no room for the rows: the batch scans for the decided pair alone)
            (void)hipGetLastError();
            *cand = 1;
            return BPE_OK;
        }
        c->lists_cap = words;
    }
    // the device's lists outlive a batch only with the plane they were read from (kept by
    // digest_end_batch, nothing written since), in the same geometry and under the same cap
    if (!c->lists_valid || c->lists_cpr != c->cpr || c->lists_R != c->R || c->lists_cand != *cand) {
        HIP_TRY(hipMemsetAsync(c->d_lists, 0xFF, offsetof(DigestLists, bkey), c->stream));
        c->lists_cpr = c->cpr;
        c->lists_R = c->R;
        c->lists_cand = *cand;
    }
    return BPE_OK;
}

// After a batch, from its control block: fresh only if the batch began on a fresh plane and every
// merge took its stream (a full-form merge clears digest_ok on the device); and the delta share.
void digest_end_batch(bpe_ctx *c, const LoopCtl *h) {
    c->digest_valid = h->digest_ok != 0;
    c->lists_valid = c->digest_valid;   // (the decision that clears digest_ok drops them too)
    c->last_delta = h->n_delta;
    c->last_done = h->n_done;
}

void geometry(bpe_ctx *c) {
    const int64_t nc = std::max<int64_t>(1, c->n_chunks);
    c->cpr = (nc + MAX_REGIONS - 1) / MAX_REGIONS;
    c->R = (int)((nc + c->cpr - 1) / c->cpr);
    c->G = (c->R + WAVES_PER_WG - 1) / WAVES_PER_WG;
}

// Capacity for `chunks` data chunks + the spare chunk, in both buffers.  Preserves the data.
int ensure_chunks(bpe_ctx *c, int64_t chunks) {
    const int64_t want = (chunks + 1) * CHUNK;
    if (want <= c->cap_slots) return BPE_OK;
    int64_t cap = std::max<int64_t>(want, c->cap_slots * 3 / 2);
    cap = (cap + CHUNK - 1) / CHUNK * CHUNK;
    int32_t *ids, *tmp;
    int rc;
    if ((rc = dev_alloc(&ids, cap))) return rc;
    if ((rc = dev_alloc(&tmp, cap))) {
        dfree(ids);
        return rc;
    }
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)ids, SEP, cap, c->stream));
    if (c->d_ids && c->n_chunks)
        HIP_TRY(hipMemcpyAsync(ids, c->d_ids, c->n_chunks * CHUNK * sizeof(int32_t),
                               hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    dfree(c->d_ids);
    dfree(c->d_tmp);
    c->d_ids = ids;
    c->d_tmp = tmp;
    c->cap_slots = cap;
    return BPE_OK;
}

// After writing live slots [0, live_slots) densely: TOMB to the end of the last chunk, SEP spare.
// The layout is new (the carries go with it); what the corpus holds is the caller's matter.
int seal_tail(bpe_ctx *c) {
    c->n_chunks = (c->live_slots + CHUNK - 1) / CHUNK;
    const int64_t end = c->n_chunks * CHUNK;
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(c->d_ids + end), SEP, CHUNK, c->stream));
    if (end > c->live_slots) {
        k_seal<<<1, CHUNK, 0, c->stream>>>(c->d_ids, c->live_slots);
        HIP_TRY(hipGetLastError());
    }
    c->packed = true;
    c->carry_valid = false;
    geometry(c);
    return BPE_OK;
}

// A corpus with other contents (ingest, add, clear, the index's write-back): nothing counted holds.
int seal_packed(bpe_ctx *c) {
    c->counts_valid = false;
    digest_stale(c, WRITER_OUTSIDE);
    c->cold_exact = false;
    c->rl_global = c->rl_delta_pending = false;
    c->cold_list = false;
    return seal_tail(c);
}

void mark_len16(bpe_ctx *c, int64_t i) { c->len16_lo = std::min(c->len16_lo, i); }

// Room for ids [0, n) in the device length table (the host tables are not extended).
int ensure_len16_cap(bpe_ctx *c, int64_t n) {
    if (n > c->cap_vocab) {
        int64_t cap = std::max<int64_t>(n, std::max<int64_t>(1024, c->cap_vocab * 2));
        dfree(c->d_len16);
        int rc = dev_alloc(&c->d_len16, cap);
        if (rc) return rc;
        c->cap_vocab = cap;
        c->len16_lo = 0;   // a fresh device buffer
    }
    return BPE_OK;
}

int ensure_vocab(bpe_ctx *c, int64_t n) {
    if ((int64_t)c->h_len16.size() < n) {
        mark_len16(c, (int64_t)c->h_len16.size());
        c->h_len16.resize(n, 1);
        c->h_count.resize(n, 0);
    }
    return ensure_len16_cap(c, n);
}

// The UTF-16 length table is read on the device only by the max_length filter (core.ts:270-273),
// so it is brought up to date lazily and incrementally (a merge adds one entry).
int sync_len16(bpe_ctx *c, int64_t max_length) {
    const int64_t n = (int64_t)c->h_len16.size();
    if (!max_length || c->len16_lo >= n) return BPE_OK;
    if (c->h_len16.empty()) return BPE_OK;
    HIP_TRY(hipMemcpyAsync(c->d_len16 + c->len16_lo, c->h_len16.data() + c->len16_lo,
                           (n - c->len16_lo) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    c->len16_lo = n;
    return BPE_OK;
}

// Upper bound on distinct cold pairs in the next pass: every counted pair with an id >= HOT
// involves a cold-token occurrence, and each occurrence sits in at most two pairs.  `extra` bounds
// the occurrences of a token created by the pass itself.
// grid of the scans over the cold table's dense view (>= HOT_BINS / 256 for k_collect)
constexpr int COLD_GRID = 1024;
static_assert(COLD_GRID * 256 >= HOT_BINS, "k_collect covers the hot bins");
static_assert(COLD_GRID <= TK_GROUP * TK_MAX_GROUPS && (MAX_REGIONS + 3) / 4 <= TK_GROUP * TK_MAX_GROUPS,
              "grid_last's counters cover k_select_maint's and k_tie_fused's grids");

// Empties the cold table: free slots, zero dense counts (the invariant past n_used), n_used = 0.
int cold_clear(bpe_ctx *c) {
    c->cold_list = false;
    HIP_TRY(hipMemsetAsync(c->cold.slots, 0xFF, c->cold_cap * sizeof(unsigned long long), c->stream));
    HIP_TRY(hipMemsetAsync(c->cold.dcounts, 0, c->cold_cap * sizeof(unsigned long long), c->stream));
    HIP_TRY(hipMemsetAsync(c->d_cold_flags, 0, 5 * sizeof(uint32_t), c->stream));
    // (the block maxima: no block flagged; the next selection of a batch is a full scan)
    HIP_TRY(hipMemsetAsync(c->cold.bdirty, 0, (c->cold_cap / CB + 1) * sizeof(uint32_t), c->stream));
    c->cold_used = 0;
    return BPE_OK;
}

// the cold table's capacity for a pass that creates at most `extra` cold-token occurrences
uint64_t cold_cap_for(const bpe_ctx *c, uint64_t extra, uint64_t min_cap = 0) {
    uint64_t s = extra;
    for (size_t t = HOT; t < c->h_count.size(); ++t) s += (uint64_t)std::max<int64_t>(0, c->h_count[t]);
    uint64_t need = 2 * s + 16;
    const uint64_t V = c->h_len16.size() + 1;
    need = std::min<uint64_t>(need, V * V);
    need = std::min<uint64_t>(need, (uint64_t)c->n_live + 16);
    uint64_t cap = 1024;
    while (cap < 2 * need || cap < min_cap) cap <<= 1;
    return cap;
}

// (reallocates empty when it grows: the contents are lost, cold_rebuild keeps them)
int ensure_cold(bpe_ctx *c, uint64_t extra, uint64_t min_cap = 0) {
    const uint64_t cap = cold_cap_for(c, extra, min_cap);
    if (cap <= c->cold_cap) return BPE_OK;
    if (cap > (1ull << 31)) return fail(BPE_ERR_OOM, "bpe native: cold pair table too large");
    HIP_TRY(hipStreamSynchronize(c->stream));
    dfree(c->cold.slots);
    dfree(c->cold.dkeys);
    dfree(c->cold.dcounts);
    dfree(c->cold.bmax);
    dfree(c->cold.bdirty);
    dfree(c->cold.blist);
    int rc;
    if ((rc = dev_alloc(&c->cold.slots, cap))) return rc;
    if ((rc = dev_alloc(&c->cold.dkeys, cap))) return rc;
    if ((rc = dev_alloc(&c->cold.dcounts, cap))) return rc;
    if ((rc = dev_alloc(&c->cold.bmax, cap / CB + 1))) return rc;
    if ((rc = dev_alloc(&c->cold.bdirty, cap / CB + 1))) return rc;
    if ((rc = dev_alloc(&c->cold.blist, cap / CB + 1))) return rc;
    c->cold_cap = cap;
    c->cold.mask = (uint32_t)(cap - 1);
    int lg = 0;
    while ((1ull << lg) < cap) ++lg;
    c->cold.shift = 32 - lg;
    c->cold.n_used = c->d_cold_flags;
    c->cold.overflow = c->d_cold_flags + 1;
    c->cold.n_blist = c->d_cold_flags + 2;
    c->cold.sel_n0 = c->d_cold_flags + 3;
    c->cold.dead = c->d_cold_flags + 4;
    c->cold.n_recomputed = c->d_cold_flags + 5;
    c->counts_valid = false;
    c->cold_exact = false;
    return cold_clear(c);
}

// The maintained cold table rebuilt from itself (round 5): its live claims (a count > 0: every
// cold pair of the corpus, the table being exact) gathered out, then loaded into a cleared table
// of at least min_cap slots and four times their number, so that the dead claims and the holes go
// and the fill drops to a quarter.  The exact pass over the corpus it replaces took 8 ms on 1 GiB
// of zipf words, plus the table-state iterations until the maintained state was entered again.
// BPE_COLD_REBUILD=0: the exact pass instead (A/B; read per call).  (Rebuilding also ahead of a
// batch at half fill, so that the batch hands no iteration over for it, timed 0.2 % slower on
// zipf C3: profiles/r05_ab_cold_rebuild.txt)
bool cold_rebuild_on() {
    const char *e = getenv("BPE_COLD_REBUILD");
    return !e || atoi(e) != 0;
}

int cold_rebuild(bpe_ctx *c, uint64_t min_cap) {
    hipStream_t s = c->stream;
    uint32_t flags[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(flags, c->d_cold_flags, sizeof flags, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (flags[1]) return fail(BPE_ERR_STATE, "bpe native: cold pair table overflow");
    const uint64_t n = std::min<uint64_t>(flags[0], c->cold_cap);
    // (the temporary lists are freed on every way out, HIP_TRY's early returns included)
    struct Scratch {
        hipStream_t s;
        uint32_t *keys = nullptr, *d_m = nullptr;
        unsigned long long *counts = nullptr;
        ~Scratch() {
            (void)hipStreamSynchronize(s);
            dfree(keys);
            dfree(counts);
            dfree(d_m);
        }
    } t{s};
    int rc;
    if ((rc = dev_alloc(&t.keys, std::max<uint64_t>(n, 1))) ||
        (rc = dev_alloc(&t.counts, std::max<uint64_t>(n, 1))) || (rc = dev_alloc(&t.d_m, 1)))
        return rc;
    HIP_TRY(hipMemsetAsync(t.d_m, 0, sizeof(uint32_t), s));
    k_cold_gather<<<COLD_GRID, 256, 0, s>>>(c->cold, t.keys, t.counts, t.d_m);
    HIP_TRY(hipGetLastError());
    uint32_t m = 0;
    HIP_TRY(hipMemcpyAsync(&m, t.d_m, sizeof m, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // (a table that grows is reallocated empty, which drops the maintained state: restored once
    // the live claims are back)
    const bool counts_valid = c->counts_valid, cold_exact = c->cold_exact;
    for (int attempt = 0;; ++attempt) {
        if ((rc = ensure_cold(c, 0, std::max<uint64_t>(min_cap, 4 * (uint64_t)m + 4096)))) return rc;
        if ((rc = cold_clear(c))) return rc;
        if (m) k_load_cold<<<COLD_GRID, 256, 0, s>>>(c->cold, t.keys, t.counts, m);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(flags, c->d_cold_flags, sizeof flags, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (!flags[1]) break;
        if (attempt == 2) return fail(BPE_ERR_STATE, "bpe native: cold pair table overflow");
        min_cap = 2 * c->cold_cap;
    }
    c->cold_used = flags[0];
    c->counts_valid = counts_valid;
    c->cold_exact = cold_exact;
    if (c->stats_on) c->stats.cold_rebuilds += 1;
    return BPE_OK;
}

float ev_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms;
}

hipEvent_t take_event(bpe_ctx *c) {
    hipEvent_t e = nullptr;
    if (!c->ev_pool.empty()) {
        e = c->ev_pool.back();
        c->ev_pool.pop_back();
    } else if (hipEventCreate(&e) != hipSuccess) {
        e = nullptr;
    }
    return e;
}

// Starts a timed span on the stream (nullptr when stats are off).
constexpr uint64_t SPAN_EVERY = 8;

hipEvent_t span_begin(bpe_ctx *c) {
    if (!c->stats_on || c->span_mute) return nullptr;
    hipEvent_t e = take_event(c);
    if (e) (void)hipEventRecord(e, c->stream);
    return e;
}

// Reads every finished span into the stats and recycles the events.
int flush_spans(bpe_ctx *c) {
    if (c->spans.empty()) return BPE_OK;
    HIP_TRY(hipEventSynchronize(c->spans.back().b));
    for (auto &sp : c->spans) {
        const double ms = ev_ms(sp.a, sp.b);
        if (sp.kind == 0 || sp.kind == 2) {   // (2: a maintained-state pass, MODE_INCR)
            c->stats.step_ms += ms;
            c->stats.step_timed += 1;
            if (sp.kind == 2) {
                c->stats.incr_ms += ms;
                c->stats.incr_timed += 1;
            }
        }
        else c->stats.select_ms += ms;
        c->ev_pool.push_back(sp.a);
        c->ev_pool.push_back(sp.b);
    }
    c->spans.clear();
    return BPE_OK;
}

int span_end(bpe_ctx *c, hipEvent_t a, int kind) {
    if (!a) return BPE_OK;
    hipEvent_t b = take_event(c);
    if (!b) return fail(BPE_ERR_HIP, "bpe native: event");
    HIP_TRY(hipEventRecord(b, c->stream));
    c->spans.push_back({a, b, kind});
    if (c->spans.size() >= 1024) return flush_spans(c);
    return BPE_OK;
}

// One streaming pass: (optionally apply the merge a,b -> cc, then) count every pair, stitch the
// region boundaries and reduce the hot table.  Leaves counts + carries valid for the new corpus.
// With a merge, *replaced receives the number of replacements.
int settle(bpe_ctx *c);
int settle_with(bpe_ctx *c, unsigned long long R);
int maybe_compact(bpe_ctx *c);

// One 160 KiB slab per workgroup of a counting pass (for the current geometry).
int ensure_partials(bpe_ctx *c) {
    geometry(c);
    if (c->G > c->partials_wg) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        dfree(c->d_partials);
        c->d_partials = nullptr;
        c->partials_wg = 0;
        int rc = dev_alloc(&c->d_partials, (size_t)c->G * HIST_WORDS);
        if (rc) return rc;
        c->partials_wg = c->G;
    }
    return BPE_OK;
}

// ---- the launch list of each pass form, once: enqueued on c->stream for the current geometry,
// with its kernels' grid shapes, its spans and, where it rewrites d_ids, the plane marked stale
constexpr unsigned REDUCE_ROWS_GRID = 4 * INCR_RLIM / 2 / RR_COLS;
constexpr unsigned REDUCE_TABLE_GRID = HIST_WORDS / REDUCE_WORDS_PER_BLOCK;
unsigned runs_grid(const bpe_ctx *c) { return (c->R + 255) / 256; }
unsigned regions_grid(const bpe_ctx *c) { return (c->R + 3) / 4; }   // (one wave per region)

// (The code object lays the kernel templates out in the order the unit first names them: named
// here in the order they have always had, rearranging the host code below moves no device code.)
[[maybe_unused]] const void *const KERNEL_ORDER[] = {
    (void *)k_step<MERGE_XX, MODE_INCR>, (void *)k_step<MERGE_XY, MODE_INCR>,
    (void *)k_step<MERGE_XX, MODE_FUSED>, (void *)k_step<MERGE_XY, MODE_FUSED>,
    (void *)k_runs<MODE_INCR>, (void *)k_runs<MODE_FUSED>, (void *)k_runs<MODE_TABLE>,
    (void *)k_step<NO_MERGE, MODE_EXACT>, (void *)k_runs<MODE_EXACT>,
    (void *)k_step_loop<MODE_INCR>, (void *)k_step_loop<MODE_FUSED>,
    (void *)k_apply<NO_MERGE>, (void *)k_runs<MODE_NONE>, (void *)k_apply<MERGE_XX>,
    (void *)k_apply<MERGE_XY>};

// The form of a counting pass: the table state (MODE_TABLE: every pair counted into d_hot, which
// the reduce also scans for the best hot key) or refreshing the maintained tables, MODE_INCR (the
// pairs touching a or b lose their count first, the pass recounts the pairs with a side in
// {a, b, c}) or MODE_FUSED (the full hot recount with the cold refresh riding along).
struct Pass {
    int mode;
    // the merge: the host path's ids (ctl == nullptr), or the LoopCtl's, which every kernel of the
    // device loop reads itself (the ids are -1; the form is fixed for a batch)
    int32_t a, b, c;
    LoopCtl *ctl;
    int64_t max_length;
    bool delta;   // device loop, MODE_TABLE: the delta form's launches ride along (allow_delta)
    // one rank of a sharded corpus: the exchange buffer the pass leaves this shard's table (or
    // delta rows) and replacement count in; nullptr in a single context
    unsigned long long *xchg;
};

// Either pass's second half: the stitch of the region boundaries and the reduce, one span.
int enqueue_stitch_reduce(bpe_ctx *c, const Pass &p) {
    hipStream_t s = c->stream;
    unsigned long long *x = p.xchg, *rep = &c->d_res->replaced;
    hipEvent_t e_red = span_begin(c);
    if (p.mode == MODE_INCR) {
        // the touched pairs into the maintained tables (a rank: into its delta rows)
        k_runs<MODE_INCR><<<runs_grid(c), 256, 0, s>>>(c->d_sums, c->R, c->d_carry, c->d_spill,
                                                       c->cold, c->d_heavy, p.ctl, p.a, p.b, p.c,
                                                       c->d_hot, x);
        k_reduce_rows<<<REDUCE_ROWS_GRID, 256, 0, s>>>(c->d_partials, c->G, c->d_spill, c->d_hot,
                                                       c->cold, p.a, p.b, p.c, p.ctl, x,
                                                       x ? rep : nullptr);
        // (the host path's best hot key; the device loop's selection takes it itself)
        if (!p.ctl)
            k_argmax_hot<<<HOT_BINS / 256, 256, 0, s>>>(c->d_hot, c->d_len16, p.max_length, c->d_res);
    } else {
        if (p.mode == MODE_FUSED)
            k_runs<MODE_FUSED><<<runs_grid(c), 256, 0, s>>>(c->d_sums, c->R, c->d_carry, c->d_spill,
                                                            c->cold, c->d_heavy, p.ctl, p.a, p.b, p.c);
        else if (!p.delta)
            k_runs<MODE_TABLE><<<runs_grid(c), 256, 0, s>>>(c->d_sums, c->R, c->d_carry, c->d_spill,
                                                            c->cold, c->d_heavy, p.ctl);
        else {
            // either form's stitch in one launch; after the apply-only stream the sites' deltas
            // into the table (after a full pass k_site_delta returns at once)
            k_runs_loop<<<runs_grid(c), 256, 0, s>>>(c->d_sums, c->R, c->d_carry, c->d_spill,
                                                     c->cold, c->d_heavy, p.ctl, c->d_site_n);
            k_site_delta<<<c->R, 256, 0, s>>>(c->d_ids, c->n_chunks, c->cpr, c->R, c->d_sites,
                                              c->d_site_n, c->d_hot, p.ctl);
        }
        // (after a delta iteration it sums nothing: the scan of the table alone.  A rank: this
        // shard's table, replacement count and largest bin into the exchange buffer, no best key)
        k_reduce_table<<<REDUCE_TABLE_GRID, REDUCE_THREADS, 0, s>>>(
            c->d_partials, c->G, c->d_spill, x ? x + XCHG_HDR : c->d_hot, c->d_len16, p.max_length,
            x ? nullptr : c->d_res, p.ctl, x, x ? rep : nullptr, x ? &c->d_res->bin_max : nullptr,
            x ? nullptr : c->d_lists->bkey);
    }
    HIP_TRY(hipGetLastError());
    return span_end(c, e_red, 1);
}

// The host path's pass: the merge (p.a, p.b) -> p.c applied and every pair counted, or counting
// only (!merge).  A MODE_FUSED pass has had its k_cold_invalidate (do_apply).  The Result is the
// caller's to clear.
int enqueue_pass(bpe_ctx *c, const Pass &p, bool merge) {
    int rc;
    hipStream_t s = c->stream;
    const int mode = p.mode;
    const int32_t a = p.a, b = p.b, cc = p.c;
    unsigned long long *rep = &c->d_res->replaced;
    if (merge) digest_stale(c, WRITER_LOOP);   // (a host-path merge)
    hipEvent_t e_step = span_begin(c);
    if (mode == MODE_INCR) k_incr_invalidate<<<COLD_GRID, 256, 0, s>>>(c->cold, c->d_hot, a, b);
    if (mode != MODE_TABLE) {
        const auto k = mode == MODE_INCR
                           ? (a == b ? k_step<MERGE_XX, MODE_INCR> : k_step<MERGE_XY, MODE_INCR>)
                           : (a == b ? k_step<MERGE_XX, MODE_FUSED> : k_step<MERGE_XY, MODE_FUSED>);
        k<<<c->G, WG, 0, s>>>(c->d_ids, c->n_chunks, c->cpr, c->R, c->d_carry, a, b, cc,
                              c->d_partials, c->d_spill, c->cold, c->d_heavy, c->d_sums, rep,
                              mode == MODE_INCR ? c->d_hot : nullptr);
    } else   // (built in the step unit, with the flags of the device loop's pass)
        HIP_TRY(bpe_step::launch_step_table(!merge ? NO_MERGE : a == b ? MERGE_XX : MERGE_XY, c->G,
                                            s, c->d_ids, c->n_chunks, c->cpr, c->R, c->d_carry,
                                            merge ? a : -1, merge ? b : -1, merge ? cc : -1,
                                            c->d_partials, c->d_spill, &c->cold, c->d_heavy,
                                            c->d_sums, rep));
    HIP_TRY(hipGetLastError());
    if ((rc = span_end(c, e_step, 0))) return rc;
    return enqueue_stitch_reduce(c, p);
}

// The exact pass: the cold pairs of the sketch buckets marked in d_heavy, counted into the cold
// table (no span: exact_pass reads the table's flags back at once).
int enqueue_exact(bpe_ctx *c) {
    hipStream_t s = c->stream;
    k_step<NO_MERGE, MODE_EXACT><<<c->G, WG, 0, s>>>(
        c->d_ids, c->n_chunks, c->cpr, c->R, c->d_carry, -1, -1, -1, c->d_partials, c->d_spill,
        c->cold, c->d_heavy, c->d_sums, &c->d_res->replaced);
    k_runs<MODE_EXACT><<<runs_grid(c), 256, 0, s>>>(c->d_sums, c->R, c->d_carry, c->d_spill, c->cold,
                                                    c->d_heavy, nullptr);
    HIP_TRY(hipGetLastError());
    return BPE_OK;
}

// The apply-only pass: the merge m = (a, b, c) streamed in without counting a pair (its
// replacement count added to *replaced), or with m == nullptr nothing rewritten, and the carries
// (RegionCarry) rebuilt for the corpus it leaves.  No span.
int enqueue_apply(bpe_ctx *c, const int32_t *m, unsigned long long *replaced) {
    hipStream_t s = c->stream;
    if (m) digest_stale(c, WRITER_OUTSIDE);   // (a replay: k_apply rewrites chunks without the plane)
    const auto k = !m ? k_apply<NO_MERGE> : m[0] == m[1] ? k_apply<MERGE_XX> : k_apply<MERGE_XY>;
    k<<<c->G, WG, 0, s>>>(c->d_ids, c->n_chunks, c->cpr, c->R, c->d_carry, m ? m[0] : -1,
                          m ? m[1] : -1, m ? m[2] : -1, c->d_sums, replaced);
    k_runs<MODE_NONE><<<runs_grid(c), 256, 0, s>>>(c->d_sums, c->R, c->d_carry, nullptr, c->cold,
                                                   nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    return BPE_OK;
}

// The maintained tables' entries touching the LoopCtl's merge, zeroed for the pass to recount.
int enqueue_loop_invalidate(bpe_ctx *c, const Pass &p) {
    if (p.mode == MODE_INCR)
        k_incr_invalidate<<<COLD_GRID, 256, 0, c->stream>>>(c->cold, c->d_hot, -1, -1, c->d_ctl,
                                                            c->d_len16, p.max_length);
    else if (p.mode == MODE_FUSED)
        k_cold_invalidate<<<COLD_GRID, 256, 0, c->stream>>>(c->cold, -1, -1, c->d_ctl);
    HIP_TRY(hipGetLastError());
    return BPE_OK;
}

// MODE_TABLE with p.delta: the launch list is fixed and holds both forms of the iteration, the
// full pass and the delta form (k_apply_loop streams the merge in without counting and lists the
// rewritten chunks, k_runs_loop stitches either form, k_site_delta adds the sites' deltas to the
// table, and k_reduce_table then only scans it); the kernels of the form the decision did not
// take return on LoopCtl::delta.
int enqueue_loop_pass(bpe_ctx *c, const Pass &p) {
    int rc;
    hipStream_t s = c->stream;
    unsigned long long *x = p.xchg, *rep = &c->d_res->replaced;
    digest_stale(c, x ? WRITER_OUTSIDE : WRITER_LOOP);   // (fresh again: digest_end_batch)
    hipEvent_t e_step = span_begin(c);
    // (a rank's selection is another call, the all-reduce between: its invalidate is timed here;
    // the single context's went with its selection, loop_enqueue)
    if (x && (rc = enqueue_loop_invalidate(c, p))) return rc;
    if (p.mode != MODE_TABLE) {
        const auto k = p.mode == MODE_INCR ? k_step_loop<MODE_INCR> : k_step_loop<MODE_FUSED>;
        k<<<c->G, WG, 0, s>>>(c->d_ids, c->n_chunks, c->cpr, c->R, c->d_carry, c->d_ctl,
                              c->d_partials, c->d_spill, c->cold, c->d_sums, rep,
                              p.mode == MODE_INCR ? c->d_hot : nullptr, x);
    } else {
        HIP_TRY(bpe_step::launch_step_loop_table(c->G, s, c->d_ids, c->n_chunks, c->cpr, c->R,
                                                 c->d_carry, c->d_ctl, c->d_partials, c->d_spill,
                                                 &c->cold, c->d_sums, rep));
        if (p.delta)
            HIP_TRY(bpe_step::launch_apply_loop(c->G, s, c->d_ids, c->n_chunks, c->cpr, c->R,
                                                c->d_carry, c->d_ctl, c->d_sums, rep, c->d_sites,
                                                c->d_site_n, c->d_digest, c->d_lists, c->d_rows));
    }
    HIP_TRY(hipGetLastError());
    // (span kind 2, the incr_* statistics: the single context's maintained passes only)
    if ((rc = span_end(c, e_step, p.mode == MODE_INCR && !x ? 2 : 0))) return rc;
    return enqueue_stitch_reduce(c, p);
}

// The arguments of a tie pass (k_tie, k_tie_fused) over the current corpus: n_cand candidates at
// `cand` for a host-driven pass, or with a LoopCtl the device loop's (it reads res->n_cand).
TieArgs tie_args(const bpe_ctx *c, const int2 *cand, int n_cand, const LoopCtl *ctl) {
    return {c->d_ids, c->n_chunks, c->cpr, c->R, n_cand, c->d_carry, cand, c->d_res, ctl};
}

// One streaming pass of the host path: (optionally apply the merge a,b -> cc, then) count every
// pair.  fused: a merge pass that also refreshes the maintained cold table (the caller
// invalidates the pairs with a side a or b before a MODE_FUSED one).
int run_pass(bpe_ctx *c, bool merge, int32_t a, int32_t b, int32_t cc, int64_t *replaced,
             bool fused = false) {
    int rc;
    if (merge && c->pending)
        if ((rc = settle(c))) return rc;
    if ((rc = ensure_partials(c))) return rc;
    c->cold_list = false;   // (fused and incremental passes update the cold table)
    if ((rc = sync_len16(c, c->opt_max_length))) return rc;   // the reduce's max_length filter
    // the spill is zero here: zeroed once at create, then by every k_reduce_table
    HIP_TRY(hipMemsetAsync(c->d_res, 0, sizeof(Result), c->stream));
    const int mode = !(merge && fused) ? MODE_TABLE : c->use_incr ? MODE_INCR : MODE_FUSED;
    const Pass p = {mode, a, b, cc, nullptr, c->opt_max_length, false, nullptr};
    if ((rc = enqueue_pass(c, p, merge))) return rc;
    c->best_ready = true;
    c->best_ml = c->opt_max_length;
    if (c->stats_on) {
        c->stats.step_launches += 1;
        c->stats.step_slots += c->n_chunks * CHUNK;
        c->stats.step_live += c->n_live;
    }
    if (merge) {
        // the replacement count stays on the device until the next sync point (settle)
        c->pending = true;
        c->pend_a = a;
        c->pend_b = b;
        c->pend_c = cc;
        c->pend_expect = -1;
        if (replaced) {
            int rc2 = settle(c);
            if (rc2) return rc2;
            *replaced = c->last_replaced;
        }
    }
    c->counts_valid = true;
    c->carry_valid = true;
    c->sketch_valid = !(merge && fused);
    if (merge && fused && c->stats_on) c->stats.fused_passes += 1;
    return BPE_OK;
}

// d_hot holds this corpus's counts with a usable sketch (the hot bins and the sketch bound)
bool table_ok(const bpe_ctx *c) { return c->counts_valid && c->sketch_valid; }

// The host's accounting of an applied merge (a, b) -> cc that replaced R occurrences in this
// corpus (a shard's own R, not the global W).  `what`: the statistics the site counts per merge.
enum MergeAcct : unsigned {
    ACCT_ITER = 1,    // a mergeUntil iteration decided on the device (iterations, live_tokens)
    ACCT_PASS = 2,    // ... applied by a streaming pass of the device loop (step_*)
    ACCT_INCR = 4,    // ... a MODE_INCR pass of the single context (incr_*)
    ACCT_FUSED = 8,   // ... a pass that kept the maintained tables (fused_passes)
    // ... on the position index (pix_merges).  `packed` is left alone: the slots are the index's,
    ACCT_PIX = 16,    // merged in place, and pix_finish writes the corpus back packed anyway
};

void account_merge(bpe_ctx *c, int32_t a, int32_t b, int32_t cc, int64_t R, unsigned what) {
    if (c->stats_on && (what & ACCT_ITER)) {
        c->stats.iterations += 1;
        c->stats.live_tokens += c->n_live;   // (the tokens the iteration selected over: before R)
        if (what & ACCT_PIX) c->stats.pix_merges += 1;
    }
    c->n_live -= R;
    c->live_slots -= R;
    c->h_count[a] -= R;
    c->h_count[b] -= R;
    c->h_count[cc] += R;
    if (R && !(what & ACCT_PIX)) c->packed = false;
    if (c->stats_on && (what & ACCT_PASS)) {
        c->stats.step_launches += 1;
        c->stats.step_slots += c->n_chunks * CHUNK;
        c->stats.step_live += c->n_live;
        if (what & ACCT_INCR) {
            c->stats.incr_launches += 1;
            c->stats.incr_live += c->n_live;
        }
        if (what & ACCT_FUSED) c->stats.fused_passes += 1;
    }
}

// A pending merge's accounting once its replacement count R is known.  (Its pass and its
// iteration were counted when they were enqueued: run_pass, do_find.)
int settle_with(bpe_ctx *c, unsigned long long Ru) {
    if (!c->pending) return BPE_OK;
    c->pending = false;
    const int64_t R = (int64_t)Ru;
    c->last_replaced = R;   // (what bpe_apply_merge reports)
    account_merge(c, c->pend_a, c->pend_b, c->pend_c, R, 0);
    if (c->pend_expect >= 0 && R != c->pend_expect)
        return fail(BPE_ERR_STATE, "bpe native: replacement count != W");
    return BPE_OK;
}

int settle(bpe_ctx *c) {
    // (a sharded position index between rank loop batches: anything else reads the chunk layout)
    if (c->rl_pix && !c->rl_open) LEAVE_GLOBAL(c);
    if (!c->pending) return BPE_OK;
    unsigned long long R = 0;
    HIP_TRY(hipMemcpyAsync(&R, &c->d_res->replaced, sizeof R, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return settle_with(c, R);
}

// Moves the live slots to a dense prefix (when dead slots waste too much of the stream, and
// before appending to a merged corpus).  Needs valid region sums; leaves counts valid (they do
// not depend on the layout) but invalidates the carries (the geometry changes).
int compact(bpe_ctx *c) {
    int rc;
    if (c->packed) return BPE_OK;
    if (!c->carry_valid)
        if ((rc = run_pass(c, false, 0, 0, 0, nullptr))) return rc;
    hipStream_t s = c->stream;
    k_scan_live<<<1, 1024, 0, s>>>(c->d_sums, c->R, c->d_outoff, c->d_total);
    // (no fill of the target first: k_compact writes the live prefix and seal_tail the last
    // chunk's tail and the spare chunk, the only slots past the prefix that anything reads.  A
    // fill of the whole buffer cost ~0.7 ms per compaction, 58 of them on zipf C3)
    k_compact<<<(c->R + 3) / 4, 256, 0, s>>>(c->d_ids, c->n_chunks, c->cpr, c->R, c->d_outoff,
                                             c->d_tmp);
    HIP_TRY(hipGetLastError());
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, c->d_total, sizeof total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((int64_t)total != c->live_slots)
        return fail(BPE_ERR_STATE, "bpe native: compaction lost slots");
    std::swap(c->d_ids, c->d_tmp);
    // (the plane goes stale, but the merge loop goes on as before: whether the next batch
    // rebuilds it is up to the last batch's delta share, as after a host-path merge.  The tokens
    // are the same: every count and every table of the old layout still holds)
    digest_stale(c, WRITER_LOOP);
    if ((rc = seal_tail(c))) return rc;
    if (c->stats_on) c->stats.compactions += 1;
    return BPE_OK;
}

// Dead slots past the compaction threshold.
bool compaction_due(const bpe_ctx *c);

int maybe_compact(bpe_ctx *c) {
    if (!compaction_due(c)) return BPE_OK;
    int rc = compact(c);
    if (rc) return rc;
    return run_pass(c, false, 0, 0, 0, nullptr);         // rebuild carries for the new layout
}

bool compaction_due(const bpe_ctx *c) {
    const int64_t slots = c->n_chunks * CHUNK;
    if (c->packed || slots < (1 << 20)) return false;
    // dead slots cost a pass as much as live ones: re-pack once they are 1% of the stream (a
    // compaction costs about three passes; at C3 merge rates that is every ~700 merges; 3% timed
    // 0.8% slower per pass over the full C3 run)
    static const int keep_pct = [] {
        const char *v = getenv("BPE_COMPACT_LIVE_PCT");   // (A/B knob: live share kept, 90..99)
        const int p = v ? atoi(v) : 99;
        return p >= 90 && p <= 99 ? p : 99;
    }();
    return c->live_slots * 100 < slots * keep_pct;
}

// Exact counts of the cold pairs in the sketch buckets marked in d_heavy, into the sparse table
// (one more streaming pass; only when some bucket could still reach the best hot count).
int exact_pass(bpe_ctx *c) {
    int rc;
    c->cold_exact = false;   // (the table is rebuilt for the marked buckets only)
    if ((rc = ensure_cold(c, 0))) return rc;
    if (!c->carry_valid)
        if ((rc = run_pass(c, false, 0, 0, 0, nullptr))) return rc;
    geometry(c);
    hipStream_t s = c->stream;
    uint32_t flags[2] = {0, 0};
    for (int attempt = 0;; ++attempt) {
        if ((rc = cold_clear(c))) return rc;
        if ((rc = enqueue_exact(c))) return rc;
        HIP_TRY(hipMemcpyAsync(flags, c->d_cold_flags, sizeof flags, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (!flags[1]) break;
        // the distinct pairs fit by construction; claims that lost a race (holes) did not:
        // a table twice as large, and the pass again
        if (attempt == 2) return fail(BPE_ERR_STATE, "bpe native: cold pair table overflow");
        if ((rc = ensure_cold(c, 0, 2 * c->cold_cap))) return rc;
    }
    c->cold_used = flags[0];
    if (c->stats_on) c->stats.exact_passes += 1;
    return BPE_OK;
}

// select_from_table: the maintained cold table overflowed, select again after a recount
constexpr int SELECT_RETRY = 100;

// Best hot pair + heavy sketch buckets for `table` (a [TABLE_BINS] u64 table on the device);
// then, when some bucket is heavy, the exact pass; then every pair sharing the best key.
// Leaves the Result in h_res and the candidates in `cand`.
int select_from_table(bpe_ctx *c, const unsigned long long *table, int64_t max_length,
                      bool local, std::vector<int2> &cand, hipEvent_t e_sel) {
    int rc;
    if ((rc = sync_len16(c, max_length))) return rc;
    hipStream_t s = c->stream;
    const bool maintained = local && c->cold_exact;
    if (maintained) {
        // the maintained cold table holds every cold pair exactly (the sketch is not consulted):
        // best hot key, then the cold argmax and every pair sharing the best, one host round trip
        if (table == c->d_hot && c->best_ready && c->best_ml == max_length) {
            HIP_TRY(hipMemsetAsync(&c->d_res->n_cand, 0, 2 * sizeof(unsigned), s));
        } else {
            k_select<<<1, 1024, 0, s>>>(table, c->d_len16, max_length, c->d_res, c->d_cand,
                                       c->d_heavy);
            HIP_TRY(hipMemsetAsync(&c->d_res->n_cand, 0, sizeof(unsigned), s));
        }
        c->best_ready = false;
        HIP_TRY(hipMemsetAsync(&c->d_res->cold_dead, 0, sizeof(unsigned long long), s));
        k_argmax_cold<<<COLD_GRID, 256, 0, s>>>(c->cold, c->d_len16, max_length, c->d_res);
        k_collect<<<COLD_GRID, 256, 0, s>>>(table, c->cold, c->d_len16, max_length, c->d_res,
                                            c->d_cand);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c->h_res, c->d_res, sizeof(Result), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(c->h_cand, c->d_cand, MAX_CAND * sizeof(int2), hipMemcpyDeviceToHost, s));
        if ((rc = span_end(c, e_sel, 1))) return rc;
        HIP_TRY(hipStreamSynchronize(s));
        if ((rc = settle_with(c, c->h_res->replaced))) return rc;
        const uint64_t flags = c->h_res->cold_flags;
        c->cold_used = flags & 0xFFFFFFFFu;
        if (flags >> 32) {
            // a refresh claimed more slots than the table has: this selection cannot be
            // trusted.  Leave the maintained state; the caller recounts and selects again (plain
            // pass, then exact passes that rebuild the table)
            c->cold_exact = false;
            c->counts_valid = false;
            c->exact_streak = 1;
            return SELECT_RETRY;
        }
        if ((flags & 0xFFFFFFFFu) * 4 > c->cold_cap * 3 ||
            2 * c->h_res->cold_dead > (flags & 0xFFFFFFFFu) + 65536) {
            // too full to probe well, or mostly claims whose pair is gone (every scan streams
            // them): this selection has read it (its result is on the host); rebuilt from its
            // own live claims, it stays the maintained table (BPE_COLD_REBUILD=0: the exact pass
            // over the corpus at the next selection, as before round 5)
            if (cold_rebuild_on()) {
                if ((rc = cold_rebuild(c, 0))) return rc;
            } else {
                c->cold_exact = false;
                c->exact_streak = 1;
            }
        }
    } else if (local && table == c->d_hot && c->best_ready && c->best_ml == max_length) {
        // the reduce already left the best hot key in the Result: collect its pairs and the
        // heavy sketch buckets with the whole chip
        HIP_TRY(hipMemsetAsync(&c->d_res->n_cand, 0, 2 * sizeof(unsigned), s));
        k_select_multi<<<TABLE_BINS / 256, 256, 0, s>>>(table, c->d_len16, max_length, c->d_res,
                                                        c->d_cand, c->d_heavy, nullptr);
    } else {
        k_select<<<1, 1024, 0, s>>>(table, c->d_len16, max_length, c->d_res, c->d_cand, c->d_heavy);
    }
    if (!maintained) {
    c->best_ready = false;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_res, c->d_res, sizeof(Result), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(c->h_cand, c->d_cand, MAX_CAND * sizeof(int2), hipMemcpyDeviceToHost, s));
    if ((rc = span_end(c, e_sel, 1))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = settle_with(c, c->h_res->replaced))) return rc;   // a pending apply's R came along
    if (local && !c->h_res->n_heavy && !c->cold_exact) c->exact_streak = 0;
    if (local && (c->h_res->n_heavy || c->cold_exact)) {
        // some cold pair may still reach W: count those exactly (or read the maintained table),
        // then recollect hot + cold
        if (!c->cold_exact) {
            // the second exact pass in a row counts every cold pair and keeps the table
            const bool full = ++c->exact_streak >= 2;
            if (full) HIP_TRY(hipMemsetAsync(c->d_heavy, 0xFF, HEAVY_WORDS * sizeof(uint32_t), s));
            if ((rc = exact_pass(c))) return rc;
            c->cold_exact = full;
        } else {
            uint32_t flags[2] = {0, 0};
            HIP_TRY(hipMemcpyAsync(flags, c->d_cold_flags, sizeof flags, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (flags[1]) return fail(BPE_ERR_STATE, "bpe native: cold pair table overflow");
            if ((uint64_t)flags[0] * 4 > c->cold_cap * 3) {
                // too full to probe well: this selection still reads it, the next one rebuilds it
                c->cold_exact = false;
                c->exact_streak = 1;
            }
        }
        HIP_TRY(hipMemsetAsync(&c->d_res->n_cand, 0, sizeof(unsigned), s));
        k_argmax_cold<<<COLD_GRID, 256, 0, s>>>(c->cold, c->d_len16, max_length, c->d_res);
        k_collect<<<COLD_GRID, 256, 0, s>>>(table, c->cold, c->d_len16, max_length, c->d_res,
                                                 c->d_cand);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c->h_res, c->d_res, sizeof(Result), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(c->h_cand, c->d_cand, MAX_CAND * sizeof(int2), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    }
    const unsigned n_cand = std::min<unsigned>(c->h_res->n_cand, CAND_CAP);
    cand.assign(c->h_cand, c->h_cand + std::min<unsigned>(n_cand, MAX_CAND));
    if (n_cand > (unsigned)MAX_CAND) {
        cand.resize(n_cand);
        HIP_TRY(hipMemcpy(cand.data(), c->d_cand, n_cand * sizeof(int2), hipMemcpyDeviceToHost));
    }
    return BPE_OK;
}

// R3 pass(es): last counted occurrence (slot + 1, 0 = none) of each candidate on this corpus.
// cand: the candidate list in device memory.
int tie_positions(bpe_ctx *c, const int2 *cand, unsigned n_cand, unsigned long long *last) {
    int rc;
    if (!c->carry_valid)
        if ((rc = run_pass(c, false, 0, 0, 0, nullptr))) return rc;
    hipStream_t s = c->stream;
    for (unsigned j0 = 0; j0 < n_cand; j0 += MAX_CAND) {
        const unsigned nb = std::min<unsigned>(MAX_CAND, n_cand - j0);
        HIP_TRY(hipMemsetAsync(c->d_res, 0, sizeof(Result), s));
        c->best_ready = false;   // the Result is reused
        hipEvent_t e_tie = span_begin(c);
        if (c->n_live > 0)
            k_tie<<<regions_grid(c), 256, 0, s>>>(tie_args(c, cand + j0, (int)nb, nullptr));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c->h_res, c->d_res, sizeof(Result), hipMemcpyDeviceToHost, s));
        if ((rc = span_end(c, e_tie, 2))) return rc;
        HIP_TRY(hipStreamSynchronize(s));
        if (c->stats_on) c->stats.tie_passes += 1;
        for (unsigned j = 0; j < nb; ++j) last[j0 + j] = c->h_res->last[j];
    }
    return BPE_OK;
}

int do_find(bpe_ctx *c, int64_t max_length, int64_t min_weight, int32_t *a, int32_t *b,
            int64_t *w) {
    if (min_weight == 0) min_weight = 2;                              // core.ts:256
    int rc;
    LEAVE_GLOBAL(c);
    // with a maintained cold table the selection settles a pending merge from the Result it
    // copies back anyway, so the host does not wait for the merge pass before enqueueing it
    const bool deferred = c->pending && c->cold_exact && c->counts_valid;
    if (!deferred) {
        if ((rc = settle(c))) return rc;
        if (c->n_live < 2) return BPE_NO_MERGE;
    }
    // (the maintained cold table does not read the sketch; every other selection does)
    if (!(c->cold_exact ? c->counts_valid : table_ok(c)))
        if ((rc = run_pass(c, false, 0, 0, 0, nullptr))) return rc;
    c->opt_max_length = max_length;
    hipEvent_t e_sel = span_begin(c);
    std::vector<int2> cand;
    rc = select_from_table(c, c->d_hot, max_length, true, cand, e_sel);
    if (rc == SELECT_RETRY) {
        if ((rc = run_pass(c, false, 0, 0, 0, nullptr))) return rc;
        rc = select_from_table(c, c->d_hot, max_length, true, cand, nullptr);
    }
    if (rc) return rc;
    if (c->stats_on) {
        c->stats.iterations += 1;
        c->stats.live_tokens += c->n_live;
    }
    const Result res = *c->h_res;
    if (res.best == 0) return BPE_NO_MERGE;                            // core.ts:312
    const int64_t W = (int64_t)(res.best >> 17);
    if (W < min_weight) return BPE_NO_MERGE;                           // core.ts:313
    const unsigned n_cand = (unsigned)cand.size();
    if (n_cand == 0 || res.n_cand > (unsigned)CAND_CAP)
        return fail(BPE_ERR_STATE, "bpe native: bad candidate count");
    int32_t ba = cand[0].x, bb = cand[0].y;
    if (n_cand > 1) {
        // R3: several pairs share W and a+b -> the one whose last counted occurrence is earliest
        // (the pair that reached W first in the reference's scan, core.ts:296-305)
        std::vector<unsigned long long> last(n_cand);
        if ((rc = tie_positions(c, c->d_cand, n_cand, last.data()))) return rc;
        unsigned long long best_pos = ~0ull;
        for (unsigned j = 0; j < n_cand; ++j) {
            if (last[j] && last[j] < best_pos) {
                best_pos = last[j];
                ba = cand[j].x;
                bb = cand[j].y;
            }
        }
        if (best_pos == ~0ull) return fail(BPE_ERR_STATE, "bpe native: tie pass found no occurrence");
    }
    *a = ba;
    *b = bb;
    *w = W;
    return BPE_OK;
}

int register_merge(bpe_ctx *c, int32_t a, int32_t b, int32_t cc);

int do_apply(bpe_ctx *c, int32_t a, int32_t b, int32_t cc, int64_t *replaced) {
    int rc;
    LEAVE_GLOBAL(c);
    if ((rc = register_merge(c, a, b, cc))) return rc;                 // core.ts:315-318
    if (replaced) *replaced = 0;
    if ((rc = settle(c))) return rc;
    if ((rc = maybe_compact(c))) return rc;
    if (c->n_live < 2) return BPE_OK;
    if (!c->carry_valid)
        if ((rc = run_pass(c, false, 0, 0, 0, nullptr))) return rc;
    // a maintained cold table is refreshed by the merge pass itself: the pairs with a side in
    // {a, b, cc} are the only ones whose count the merge changes (every other pair keeps its
    // occurrences and its run parity), so those lose their count before the pass and the pass
    // counts them again on the merged corpus.  A table that has to grow is rebuilt by a full
    // exact pass at the next selection instead.
    bool fused = false;
    if (c->cold_exact) {
        const int64_t na = c->h_count[a], nb = c->h_count[b];
        const uint64_t bound = (uint64_t)std::max<int64_t>(0, a == b ? na / 2 : std::min(na, nb));
        // the refresh claims at most 2 * bound new slots (holes included): it must fit the
        // table's 3/4 fill limit, which counts every claim made since the last rebuild
        const uint64_t V = c->h_len16.size() + 1;
        const uint64_t claims = std::min<uint64_t>(2 * bound, V * V) + 64;
        if (cold_rebuild_on() &&
            (cold_cap_for(c, bound) > c->cold_cap || c->cold_used + claims > c->cold_cap / 4 * 3)) {
            // a table that has to grow, or has no room for the refresh: rebuilt from its own
            // live claims, with room for both
            if ((rc = cold_rebuild(c, std::max(cold_cap_for(c, bound), 2 * claims)))) return rc;
        }
        const uint64_t cap1 = c->cold_cap;
        if ((rc = ensure_cold(c, bound))) return rc;
        const bool room = c->cold_used + claims <= c->cold_cap / 4 * 3 && c->cold_cap == cap1;
        fused = c->cold_exact && room && !getenv("BPE_DEBUG_NO_FUSED");
        if (!fused) {
            c->cold_exact = false;
            c->exact_streak = 1;   // (the next exact pass rebuilds the whole table)
        }
    }
    if (fused && !c->use_incr) k_cold_invalidate<<<COLD_GRID, 256, 0, c->stream>>>(c->cold, a, b);
    if ((rc = run_pass(c, true, a, b, cc, replaced, fused))) return rc;
    return BPE_OK;
}

// ---- the device loop: up to n mergeUntil iterations decided on the device (core.ts:367-384) ----
// Per iteration the selection (k_select_multi; with a maintained cold table, skewed corpora,
// k_select_maint), the decision with the R3 tie pass when tied (k_tie_fused) and the pass
// (enqueue_loop_pass), every kernel reading the merge from the LoopCtl; one host sync per batch.

// Before a batch of up to n merges decided on the device: room for their ids in the device length
// table, which must be exact below the first of them (k_decide extends it from there).
int len16_for_batch(bpe_ctx *c, int64_t n) {
    int rc;
    if ((rc = ensure_len16_cap(c, (int64_t)c->h_len16.size() + n))) return rc;
    return sync_len16(c, 1);
}

// A batch's control block in its pinned mirror: the fields every form of the device loop sets
// (min_weight: after the core.ts:256 default).  The caller adds its own and uploads it.
LoopCtl *ctl_begin(bpe_ctx *c, int64_t min_weight, bool maintained) {
    LoopCtl *h = c->h_ctl;
    memset(h, 0, sizeof *h);
    h->status = LOOP_RUN;
    h->next_id = (int32_t)c->h_len16.size();
    h->w = -1;
    h->min_weight = min_weight;
    h->max_id = BPE_MAX_VOCAB;
    h->maintained = maintained ? 1 : 0;
    h->cold_cap = c->cold_cap;
    return h;
}

// A batch's first part: the tables and carries a batch starts from, its buffers, the digest plane,
// the Result and the control block.  *p: the form of the batch's passes.
int loop_prepare(bpe_ctx *c, int64_t max_length, int64_t min_weight, int64_t n, Pass *p) {
    int rc;
    LEAVE_GLOBAL(c);
    if ((rc = settle(c))) return rc;
    c->cold_list = false;
    c->opt_max_length = max_length;
    const bool maint = c->cold_exact && c->counts_valid && c->carry_valid &&
                       !getenv("BPE_DEBUG_NO_FUSED");
    if (!maint) c->cold_exact = false;
    if (!maint && (!table_ok(c) || !c->carry_valid))
        if ((rc = run_pass(c, false, 0, 0, 0, nullptr))) return rc;
    if ((rc = len16_for_batch(c, n))) return rc;
    geometry(c);
    // The table state may take the delta form (LoopCtl::delta; BPE_DELTA=0 turns it off, for A/B
    // and checking; read per batch): the site list holds a segment of cpr entries per region.
    const char *dknob = getenv("BPE_DELTA");
    *p = {!maint ? MODE_TABLE : c->use_incr ? MODE_INCR : MODE_FUSED, -1, -1, -1, c->d_ctl, max_length,
          !maint && !(dknob && atoi(dknob) == 0), nullptr};
    if (p->delta && c->sites_cap < (int64_t)c->R * c->cpr) {
        dfree(c->d_sites);
        c->d_sites = nullptr;
        c->sites_cap = 0;
        const int64_t cap = (int64_t)c->R * c->cpr;
        if ((rc = dev_alloc(&c->d_sites, (size_t)cap))) return rc;
        c->sites_cap = cap;
    }
    bool digest = false;   // the delta form's stream reads the digest plane
    int cand = 1;          // ... for this many candidate pairs per stream
    if (p->delta && (rc = digest_begin_batch(c, &digest, &cand))) return rc;
    hipStream_t s = c->stream;
    if (maint) {
        // (k_select_maint takes the best over the hot bins itself)
        HIP_TRY(hipMemsetAsync(c->d_res, 0, sizeof(Result), s));
    } else if (c->best_ready && c->best_ml == max_length) {
        // keep the reduce's best key, clear the rest of the Result
        HIP_TRY(hipMemsetAsync(&c->d_res->n_cand, 0, sizeof(Result) - offsetof(Result, n_cand), s));
    } else {
        HIP_TRY(hipMemsetAsync(c->d_res, 0, sizeof(Result), s));
        k_argmax_hot<<<HOT_BINS / 256, 256, 0, s>>>(c->d_hot, c->d_len16, max_length, c->d_res);
        // (no block keys of this table: the first scan has nothing to predict from)
        HIP_TRY(hipMemsetAsync(c->d_lists->bkey, 0, sizeof c->d_lists->bkey, s));
    }
    LoopCtl *h = ctl_begin(c, min_weight, maint);
    h->allow_delta = p->delta ? 1 : 0;
    h->digest_ok = digest ? 1 : 0;
    h->digest_cand = cand;
    HIP_TRY(hipMemcpyAsync(c->d_ctl, h, sizeof *h, hipMemcpyHostToDevice, s));
    return BPE_OK;
}

// A batch's second part: n iterations enqueued, nothing waited for.
int loop_enqueue(bpe_ctx *c, const Pass &p, int64_t n) {
    int rc;
    hipStream_t s = c->stream;
    // (A/B and checking knob: every maintained selection a full scan of the cold table)
    static const bool sel_full = getenv("BPE_SEL_FULL") != nullptr;
    const TieArgs tie = tie_args(c, c->d_cand, 0, c->d_ctl);
    for (int64_t i = 0; i < n; ++i) {
        // the spans of every SPAN_EVERY-th iteration only: each event record costs the stream
        // a few microseconds, about 3% of an iteration with all six
        c->span_mute = (c->span_tick++ % SPAN_EVERY) != 0;
        hipEvent_t e_sel = span_begin(c);
        if (p.mode != MODE_TABLE) {
            // best key over the hot bins and the cold table, its pairs, the table's flags
            // a full scan of the cold table on the first selection of the batch and every
            // SEL_FULL_EVERY-th (its dead claims), else the block maxima on a grid of one
            // workgroup per 256 hot bins
            const bool full = p.mode == MODE_FUSED || sel_full || i % SEL_FULL_EVERY == 0;
            k_select_maint<<<full ? COLD_GRID : HOT_BINS / 256, 256, 0, s>>>(
                c->d_hot, c->cold, c->d_len16, p.max_length, c->d_res, c->d_cand, c->d_brec,
                c->d_ticket, c->d_ctl, full ? 1 : 0);
        } else {
            k_select_multi<<<TABLE_BINS / 256, 256, 0, s>>>(c->d_hot, c->d_len16, p.max_length,
                                                            c->d_res, c->d_cand, c->d_heavy,
                                                            c->d_ctl);
        }
        // the decision, the R3 tie pass when tied, and its commit: one launch
        k_tie_fused<<<regions_grid(c), 256, 0, s>>>(tie, c->d_len16, c->d_log, c->d_ticket,
                                                    c->d_lists);
        HIP_TRY(hipGetLastError());
        // (timed with the selection, so that the pass's span is the pass kernel alone)
        if ((rc = enqueue_loop_invalidate(c, p))) return rc;
        if ((rc = span_end(c, e_sel, 1))) return rc;
        if ((rc = enqueue_loop_pass(c, p))) return rc;
    }
    c->span_mute = false;
    return BPE_OK;
}

// The one host sync of a batch (single context or rank): its control block, the Result and the
// log of n merges into their pinned mirrors.
int loop_read_back(bpe_ctx *c, int64_t n) {
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(c->h_ctl, c->d_ctl, sizeof(LoopCtl), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(c->h_res, c->d_res, sizeof(Result), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(c->h_log, c->d_log, LOG_WORDS * n * sizeof(long long),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return BPE_OK;
}

// A finished batch's counters (a rank's batch takes no delta form: those counters are zero).
void loop_stats(bpe_ctx *c, const LoopCtl *h) {
    if (!c->stats_on) return;
    c->stats.tie_passes += h->n_tie;
    c->stats.unscreened_passes += h->n_unscreened;
    c->stats.tie_tail += h->n_tail;
    c->stats.tie_lone += h->n_lone;
    c->stats.loop_host += h->n_host;
    c->stats.delta_passes += h->n_delta;
    c->stats.delta_chunks += (int64_t)h->delta_chunks;
    c->stats.digest_passes += h->n_digest;
    c->stats.digest_hits += (int64_t)h->digest_hits;
    c->stats.digest_scans += h->n_scan;
}

// A batch's third part: the one host sync, then the host tables brought up to date from the log.
// The merges go to out_abw[3 * i ...]; *status is the LoopStatus the batch ended with (LOOP_RUN:
// all n done; LOOP_HOST: the next iteration needs the host path).
int loop_finish(bpe_ctx *c, const Pass &p, int64_t n, int64_t *out_abw, int64_t *n_done,
                int *status) {
    int rc;
    LoopCtl *h = c->h_ctl;
    const bool maint = p.mode != MODE_TABLE;
    const int64_t base = (int64_t)c->h_len16.size();   // (the batch's first new id)
    if ((rc = loop_read_back(c, n))) return rc;
    digest_end_batch(c, h);
    const int64_t nd = h->n_done;
    if (h->status == LOOP_ERROR)
        return fail(BPE_ERR_STATE,
                    h->err == 3 ? "bpe native: device loop: the table's bin of the merged pair != W"
                                : "bpe native: device loop: replacement count != W, or a tie "
                                  "pass found no occurrence");
    if (nd < 0 || nd > n) return fail(BPE_ERR_STATE, "bpe native: device loop: bad merge count");
    // the last merge's replacement count is checked here (the others were, on the device)
    if (h->status == LOOP_RUN && nd > 0 && c->h_res->replaced != (unsigned long long)h->w)
        return fail(BPE_ERR_STATE, "bpe native: replacement count != W");
    c->h_len16.resize(base + nd, 1);
    c->h_count.resize(base + nd, 0);
    const unsigned acct = ACCT_ITER | ACCT_PASS | (p.mode == MODE_INCR ? ACCT_INCR : 0) |
                          (maint ? ACCT_FUSED : 0);
    for (int64_t i = 0; i < nd; ++i) {
        const int32_t a = (int32_t)c->h_log[LOG_WORDS * i], b = (int32_t)c->h_log[LOG_WORDS * i + 1];
        const int64_t W = c->h_log[LOG_WORDS * i + 2];
        const int64_t cc = base + i;
        c->h_len16[cc] = c->h_len16[a] + c->h_len16[b];                // core.ts:318
        account_merge(c, a, b, (int32_t)cc, W, acct);   // (one corpus: W is its replacement count)
        c->last_replaced = W;
        out_abw[3 * i] = a;
        out_abw[3 * i + 1] = b;
        out_abw[3 * i + 2] = W;
    }
    c->len16_lo = base + nd;   // k_decide wrote the new lengths on the device
    if (maint) {
        c->cold_used = c->h_res->cold_flags & 0xFFFFFFFFu;   // (as of the last selection)
        if (c->stats_on) {
            c->stats.cold_used = std::max<int64_t>(c->stats.cold_used, (int64_t)c->cold_used);
            uint32_t nr = 0;
            HIP_TRY(hipMemcpy(&nr, c->cold.n_recomputed, sizeof nr, hipMemcpyDeviceToHost));
            c->stats.sel_blocks = nr;   // (cumulative since the context was made)
        }
        if (nd) c->sketch_valid = false;                     // (fused passes)
    }
    loop_stats(c, h);
    // every early-ended batch of the table state leaves the last reduce's best key in the Result
    // (the maintained state selects with k_select_maint: nothing is left ready)
    c->best_ready = !maint;
    c->best_ml = p.max_length;
    c->counts_valid = c->carry_valid = true;
    if (!maint) c->sketch_valid = true;
    *n_done = nd;
    *status = h->status;
    return BPE_OK;
}

int loop_batch(bpe_ctx *c, int64_t max_length, int64_t min_weight, int64_t n, int64_t *out_abw,
               int64_t *n_done, int *status) {
    int rc;
    *n_done = 0;
    *status = LOOP_DONE;
    Pass p;
    if ((rc = loop_prepare(c, max_length, min_weight, n, &p))) return rc;
    if ((rc = loop_enqueue(c, p, n))) return rc;
    return loop_finish(c, p, n, out_abw, n_done, status);
}

// ---- the device loop on one rank of a sharded corpus ------------------------
// Per iteration the caller enqueues, on this context's stream: all-reduce(SUM) of the exchange
// buffer's first *n_words words, rank_loop_select, all-reduce(MAX) of the BPE_TIE_WORDS tie words,
// rank_loop_decide, rank_loop_count.  Nothing syncs the host until rank_loop_end, which reads the
// batch's merges back.  Two states, the same on every rank:
//  - table (the streaming pass's full recount): the exchange is the header + this shard's 81920-bin
//    table, summed into the global table every rank selects from;
//  - maintained (after bpe_set_global_counts: skewed corpora, large vocabularies): every rank
//    holds the global hot and cold tables; a merge (a, b) -> c zeroes the pairs touching a or b
//    in them, each shard recounts the pairs with a side in {a, b, c} on its own corpus (MODE_INCR)
//    into delta rows, and the summed rows are added to every rank's tables (k_apply_delta).
// The header's first word is this shard's replacement count of the merge just applied: summed,
// it must equal W (checked on the device by the next decision, and for the batch's last merge by
// the host from the log).
int carry_pass(bpe_ctx *c);
}  // namespace
int pix_rank_begin(bpe_ctx *c, int64_t max_length, int64_t min_weight, unsigned long long *xchg,
                   unsigned long long *tie, int rank, int world, int64_t *n_words);
int pix_rank_select(bpe_ctx *c);
int pix_rank_decide(bpe_ctx *c);
int pix_rank_count(bpe_ctx *c);
int pix_rank_end(bpe_ctx *c, int64_t *out, int64_t cap, int64_t *n_done, int *status);
int pix_set_global(bpe_ctx *c, const unsigned long long *table, const uint32_t *keys,
                   const unsigned long long *counts, int64_t n);
namespace {

int rank_loop_begin(bpe_ctx *c, int64_t max_length, int64_t min_weight, unsigned long long *xchg,
                    unsigned long long *tie, int rank, int world, int64_t *n_words) {
    int rc;
    if (c->rl_pix && c->rl_global) {
        if (!c->rl_delta_pending || xchg == c->rl_table)
            return pix_rank_begin(c, max_length, min_weight, xchg, tie, rank, world, n_words);
        LEAVE_GLOBAL(c);   // (another exchange buffer: the last merge's delta rows are not in it)
    }
    if ((rc = settle(c))) return rc;
    const bool glob = c->rl_global;
    c->opt_max_length = max_length;
    if (glob) {
        // the global tables stay: a compaction keeps every count, and the carries are rebuilt
        // without a counting pass (it would write this shard's counts over the global table)
        if (compaction_due(c)) {
            if (!c->carry_valid)
                if ((rc = carry_pass(c))) return rc;
            if ((rc = compact(c))) return rc;
        }
        if (!c->carry_valid)
            if ((rc = carry_pass(c))) return rc;
        if (c->rl_delta_pending && xchg != c->rl_table) {
            // (another exchange buffer: the last merge's delta rows are not in it)
            LEAVE_GLOBAL(c);
            return rank_loop_begin(c, max_length, min_weight, xchg, tie, rank, world, n_words);
        }
    } else {
        c->cold_exact = false;
        if ((rc = maybe_compact(c))) return rc;
        if (!table_ok(c) || !c->carry_valid)
            if ((rc = run_pass(c, false, 0, 0, 0, nullptr))) return rc;
    }
    if ((rc = ensure_partials(c))) return rc;
    const int64_t base = (int64_t)c->h_len16.size();
    if ((rc = len16_for_batch(c, LOOP_BATCH))) return rc;
    hipStream_t s = c->stream;
    HIP_TRY(hipMemsetAsync(c->d_res, 0, sizeof(Result), s));
    LoopCtl *h = ctl_begin(c, min_weight == 0 ? 2 : min_weight, glob);   // core.ts:256
    h->sharded = 1;
    h->last_rank = rank == world - 1;
    int64_t nw;
    if (glob) {
        // the delta rows of every token id a merge of this batch can see (<= base + LOOP_BATCH)
        nw = XCHG_HDR + DELTA_ROWS * std::min<int64_t>(BPE_MAX_VOCAB, base + LOOP_BATCH + 1);
        if (c->rl_delta_pending) {
            // the last batch's last merge: its rows go into this batch's first exchange
            h->a = c->rl_last_a;
            h->b = c->rl_last_b;
            h->c = c->rl_last_c;
            h->w = c->rl_last_w;
        } else {
            // all of it: the rows past this batch's words must be zero when later batches reach
            // them (k_apply_delta only zeroes the rows it consumes; the buffer may hold anything)
            HIP_TRY(hipMemsetAsync(xchg, 0, XCHG_WORDS * sizeof(unsigned long long), s));
        }
    } else {
        nw = XCHG_HDR + TABLE_BINS;
        HIP_TRY(hipMemsetAsync(xchg, 0, XCHG_HDR * sizeof(unsigned long long), s));
        HIP_TRY(hipMemcpyAsync(xchg + XCHG_HDR, c->d_hot, TABLE_BINS * sizeof(unsigned long long),
                               hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(c->d_ctl, h, sizeof *h, hipMemcpyHostToDevice, s));
    c->rl_delta_pending = false;
    c->cold_list = false;
    c->rl_table = xchg;
    c->rl_tie = tie;
    c->rl_rank = rank;
    c->rl_world = world;
    c->rl_base = base;
    c->rl_enqueued = 0;
    c->rl_max_length = max_length;
    c->rl_open = true;
    c->best_ready = false;
    *n_words = nw;
    return BPE_OK;
}

// From the all-reduced exchange: the global table (or the maintained tables after the delta),
// the best key, its pairs, the proposal (or the tie pass, whose positions go to `tie` with this
// rank's vote for the all-reduce(MAX)).
int rank_loop_select(bpe_ctx *c) {
    if (!c->rl_open || c->rl_enqueued >= LOOP_BATCH)
        return fail(BPE_ERR_STATE, "bpe native: rank loop not begun, or its batch is full");
    if (c->rl_pix) return pix_rank_select(c);
    hipStream_t s = c->stream;
    const int64_t ml = c->rl_max_length;
    hipEvent_t e_sel = span_begin(c);
    if (c->rl_global) {
        k_apply_delta<<<COLD_GRID, 256, 0, s>>>(c->rl_table, c->d_hot, c->cold, c->d_ctl);
        // the block maxima of the cold table, as in the single-corpus device loop (round 5: was
        // k_argmax_hot + k_argmax_cold + k_collect, two scans of every claimed cold pair per merge,
        // which grew with the vocabulary).  The summed delta rows re-add the pairs of a and b that
        // k_incr_invalidate zeroed (to at most their old count: their blocks were flagged when the
        // zeroed entry may have been the max) and claim the pairs of c (new claims at the end of
        // the dense view), exactly the changes the incremental form recomputes.  A full scan on the
        // first selection of a batch and every SEL_FULL_EVERY-th (its dead claims).
        static const bool sel_full = getenv("BPE_SEL_FULL") != nullptr;
        const bool full = sel_full || c->rl_enqueued % SEL_FULL_EVERY == 0;
        k_select_maint<<<full ? COLD_GRID : HOT_BINS / 256, 256, 0, s>>>(
            c->d_hot, c->cold, c->d_len16, ml, c->d_res, c->d_cand, c->d_brec, c->d_ticket,
            c->d_ctl, full ? 1 : 0);
    } else {
        const unsigned long long *table = c->rl_table + XCHG_HDR;
        k_argmax_hot<<<HOT_BINS / 256, 256, 0, s>>>(table, c->d_len16, ml, c->d_res, c->d_ctl);
        k_select_multi<<<TABLE_BINS / 256, 256, 0, s>>>(table, c->d_len16, ml, c->d_res, c->d_cand,
                                                        c->d_heavy, c->d_ctl);
    }
    k_decide<<<1, 64, 0, s>>>(c->d_ctl, c->d_res, c->d_cand, c->d_len16, c->d_log, 0, nullptr,
                              c->rl_table);
    k_tie<<<regions_grid(c), 256, 0, s>>>(tie_args(c, c->d_cand, 0, c->d_ctl));
    k_tie_export<<<1, 64, 0, s>>>(c->d_ctl, c->d_res, c->rl_tie, c->rl_rank);
    HIP_TRY(hipGetLastError());
    return span_end(c, e_sel, 1);
}

// After the all-reduce(MAX) of `tie`: the decision, the same on every rank.
int rank_loop_decide(bpe_ctx *c) {
    if (!c->rl_open) return fail(BPE_ERR_STATE, "bpe native: rank loop not begun");
    if (c->rl_pix) return pix_rank_decide(c);
    k_decide<<<1, 64, 0, c->stream>>>(c->d_ctl, c->d_res, c->d_cand, c->d_len16, c->d_log, 1,
                                      c->rl_tie, c->rl_table);
    HIP_TRY(hipGetLastError());
    return BPE_OK;
}

// Applies the decided merge to this shard and counts it: this shard's table (or delta rows) and
// its replacement count into the exchange buffer.
int rank_loop_count(bpe_ctx *c) {
    if (!c->rl_open) return fail(BPE_ERR_STATE, "bpe native: rank loop not begun");
    if (c->rl_pix) return pix_rank_count(c);
    // (the global state's pass is MODE_INCR; the table state's the full pass, never the delta form)
    const Pass p = {c->rl_global ? MODE_INCR : MODE_TABLE, -1, -1, -1, c->d_ctl, c->rl_max_length,
                    false, c->rl_table};
    const int rc = enqueue_loop_pass(c, p);
    if (rc) return rc;
    c->rl_enqueued += 1;
    return BPE_OK;
}

// Syncs, reads the batch's merges back (out_abwr: (a, b, W, this shard's replacement count)
// quadruples) and updates the host tables with this shard's counts.  *status: LOOP_RUN (every
// enqueued iteration merged), LOOP_DONE (no pair qualifies), LOOP_HOST (the next iteration needs
// the host protocol).
int rank_loop_end(bpe_ctx *c, int64_t *out, int64_t cap, int64_t *n_done, int *status) {
    if (!c->rl_open) return fail(BPE_ERR_STATE, "bpe native: rank loop not begun");
    if (c->rl_pix) return pix_rank_end(c, out, cap, n_done, status);
    c->rl_open = false;
    hipStream_t s = c->stream;
    LoopCtl *h = c->h_ctl;
    const int rc = loop_read_back(c, LOOP_BATCH);
    if (rc) return rc;
    const bool glob = c->rl_global;
    if (h->status == LOOP_ERROR) {
        const bool was_global = glob;
        static const bool dbg = getenv("BPE_DEBUG_GLOBAL") != nullptr;
        if (dbg) {
            HIP_TRY(hipMemcpy(c->h_log, c->d_log, LOG_WORDS * LOOP_BATCH * sizeof(long long),
                              hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < h->n_done && i < LOOP_BATCH; ++i)
                fprintf(stderr, "[bpe debug] rank %d batch merge %lld: (%lld, %lld) W %lld rep %lld\n",
                        c->rl_rank, (long long)i, c->h_log[4 * i], c->h_log[4 * i + 1],
                        c->h_log[4 * i + 2], c->h_log[4 * i + 3]);
            fprintf(stderr, "[bpe debug] rank %d ctl: a %d b %d c %d w %lld tie %d vote %d base %lld\n",
                    c->rl_rank, h->a, h->b, h->c, (long long)h->w, h->tie, h->vote, (long long)c->rl_base);
        }
        LEAVE_GLOBAL(c);
        c->counts_valid = false;
        char msg[256];
        if (h->err == 1)
            snprintf(msg, sizeof msg, "bpe native: rank loop: the shards' replacement counts sum to "
                     "%llu, not W = %llu (merge %lld of the batch, %s state)", h->err_got, h->err_want,
                     (long long)h->n_done, was_global ? "maintained" : "table");
        else
            snprintf(msg, sizeof msg, "bpe native: rank loop: a tie pass found no occurrence (merge "
                     "%lld of the batch, %s state)", (long long)h->n_done, was_global ? "maintained" : "table");
        return fail(BPE_ERR_STATE, msg);
    }
    const int64_t nd = h->n_done;
    if (nd < 0 || nd > c->rl_enqueued) return fail(BPE_ERR_STATE, "bpe native: rank loop: bad merge count");
    const int64_t base = c->rl_base;
    c->h_len16.resize(base + nd, 1);
    c->h_count.resize(base + nd, 0);
    for (int64_t i = 0; i < nd; ++i) {
        const long long *m = c->h_log + LOG_WORDS * i;
        const int32_t a = (int32_t)m[0], b = (int32_t)m[1];
        const int64_t W = m[2];
        // this shard's replacement count (the last merge's is still in the Result)
        const int64_t R = m[3] >= 0 ? m[3] : (int64_t)c->h_res->replaced;
        const int64_t cc = base + i;
        c->h_len16[cc] = c->h_len16[a] + c->h_len16[b];                // core.ts:318
        // (the global state's passes count as fused ones, not in the incr_* statistics)
        account_merge(c, a, b, (int32_t)cc, R, ACCT_ITER | ACCT_PASS | (glob ? ACCT_FUSED : 0));
        if (i < cap) {
            out[4 * i] = a;
            out[4 * i + 1] = b;
            out[4 * i + 2] = W;
            out[4 * i + 3] = R;
        }
    }
    c->len16_lo = base + nd;
    loop_stats(c, h);
    c->carry_valid = true;   // (the last pass's carries)
    c->best_ready = false;
    const bool all = h->status == LOOP_RUN && nd == c->rl_enqueued;
    if (glob) {
        if (all && nd > 0) {
            // the last merge's delta rows wait in the exchange buffer for the next batch's first
            // all-reduce
            const long long *m = c->h_log + LOG_WORDS * (nd - 1);
            c->rl_delta_pending = true;
            c->rl_last_a = (int32_t)m[0];
            c->rl_last_b = (int32_t)m[1];
            c->rl_last_c = (int32_t)(base + nd - 1);
            c->rl_last_w = m[2];
        } else if (!all) {
            LEAVE_GLOBAL(c);   // (the host path takes over: this shard's counts are recounted)
        }
    } else if (all && nd > 0) {
        // the last count left this shard's table in the exchange buffer, not summed since
        HIP_TRY(hipMemcpyAsync(c->d_hot, c->rl_table + XCHG_HDR, TABLE_BINS * sizeof(unsigned long long),
                               hipMemcpyDeviceToDevice, s));
        c->counts_valid = c->sketch_valid = true;
    } else if (nd > 0 || !all) {
        // (the exchange buffer was summed again after the batch ended: recount when needed)
        c->counts_valid = false;
    }
    *n_done = nd;
    *status = h->status;
    return BPE_OK;
}

// This shard's exact count of every cold pair (an id >= 256), for the global tables of the
// sharded maintained state: one exact streaming pass (kept: a second call with a bigger buffer
// exports the same list without another pass).
int cold_counts(bpe_ctx *c, uint32_t *keys, unsigned long long *counts, int64_t cap, int64_t *n) {
    int rc;
    LEAVE_GLOBAL(c);
    if ((rc = settle(c))) return rc;
    if (!c->cold_list) {
        hipStream_t s = c->stream;
        if (c->n_live >= 2) {
            HIP_TRY(hipMemsetAsync(c->d_heavy, 0xFF, HEAVY_WORDS * sizeof(uint32_t), s));
            if ((rc = exact_pass(c))) return rc;
        } else {
            if ((rc = cold_clear(c))) return rc;
            c->cold_used = 0;
        }
        c->cold_list = true;
    }
    *n = (int64_t)c->cold_used;
    if (*n > cap) return BPE_OK;
    if (*n) {
        if (!keys || !counts) return fail(BPE_ERR_ARG, "bpe native: null cold buffers");
        k_export_cold<<<256, 256, 0, c->stream>>>(c->cold, keys, counts);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return BPE_OK;
}

// Loads the global maintained state of a sharded corpus: the hot bins of the global table and
// the cold pairs of every shard (duplicates summed).  The next rank loop batch keeps them.
int set_global_counts(bpe_ctx *c, const unsigned long long *table, const uint32_t *keys,
                      const unsigned long long *counts, int64_t n) {
    int rc;
    LEAVE_GLOBAL(c);
    if ((rc = settle(c))) return rc;
    if (n < 0 || (n && (!keys || !counts))) return fail(BPE_ERR_ARG, "bpe native: bad global counts");
    if (c->use_pix) return pix_set_global(c, table, keys, counts, n);   // (the incremental mode)
    hipStream_t s = c->stream;
    // room for every distinct pair at half fill, and for the claims of the merges to come (the
    // decisions hand over to the host before 3/4 fill)
    if ((rc = ensure_cold(c, 0, 4 * (uint64_t)n + 4096))) return rc;
    for (int attempt = 0;; ++attempt) {
        if ((rc = cold_clear(c))) return rc;
        HIP_TRY(hipMemcpyAsync(c->d_hot, table, HOT_BINS * sizeof(unsigned long long),
                               hipMemcpyDeviceToDevice, s));
        if (n) k_load_cold<<<1024, 256, 0, s>>>(c->cold, keys, counts, n);
        HIP_TRY(hipGetLastError());
        uint32_t flags[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(flags, c->d_cold_flags, sizeof flags, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (!flags[1] && (uint64_t)flags[0] * 4 <= c->cold_cap) {
            c->cold_used = flags[0];
            break;
        }
        if (attempt == 2) return fail(BPE_ERR_STATE, "bpe native: global cold table overflow");
        if ((rc = ensure_cold(c, 0, 2 * c->cold_cap))) return rc;
    }
    c->rl_global = true;
    c->rl_delta_pending = false;
    c->rl_table = nullptr;   // (no batch of this state was begun yet: bpe_debug_global reads none)
    c->counts_valid = true;
    c->sketch_valid = false;
    c->cold_exact = false;   // (the single-context maintained state is not this one)
    c->best_ready = false;
    return BPE_OK;
}

// Carries (RegionCarry) for the current corpus and geometry without counting pairs.
int carry_pass(bpe_ctx *c) {
    geometry(c);
    const int rc = enqueue_apply(c, nullptr, nullptr);
    if (rc) return rc;
    c->carry_valid = true;
    return BPE_OK;
}

// Checks a merge (a, b) -> cc against the vocabulary and registers cc (core.ts:315-318).
int register_merge(bpe_ctx *c, int32_t a, int32_t b, int32_t cc) {
    if (a < 0 || b < 0 || cc < 0 || cc >= BPE_MAX_VOCAB)
        return fail(cc >= BPE_MAX_VOCAB ? BPE_ERR_VOCAB : BPE_ERR_ARG,
                    "bpe native: token id out of range (vocab is limited to 55295 tokens)");
    if (a >= (int64_t)c->h_len16.size() || b >= (int64_t)c->h_len16.size())
        return fail(BPE_ERR_ARG, "bpe native: apply_merge with an unregistered token");
    int rc;
    if ((rc = ensure_vocab(c, (int64_t)cc + 1))) return rc;
    c->h_len16[cc] = c->h_len16[a] + c->h_len16[b];
    mark_len16(c, cc);
    return BPE_OK;
}

// applyMerge without counting, for a run of merges (restoreMerge replay, core.ts:477-494; batch
// encoding, core.ts:392-409): one apply-only streaming pass per merge (k_apply + k_runs for the
// carries), their replacement counts read back once per REPLAY_BATCH merges.  With count_after
// the last merge is applied by the fused apply + count pass, so a find that follows needs no
// extra pass.  replaced (may be null) receives each merge's replacement count.
int replay(bpe_ctx *c, const int32_t *abc, int64_t n, int64_t *replaced, bool count_after) {
    int rc;
    LEAVE_GLOBAL(c);
    if ((rc = settle(c))) return rc;
    const int64_t n_plain = count_after ? n - 1 : n;
    for (int64_t i0 = 0; i0 < n_plain;) {
        if ((rc = maybe_compact(c))) return rc;
        if (!c->carry_valid)
            if ((rc = carry_pass(c))) return rc;
        const int64_t nb = std::min<int64_t>(REPLAY_BATCH, n_plain - i0);
        for (int64_t j = 0; j < nb; ++j) {
            const int32_t *m = abc + 3 * (i0 + j);
            if ((rc = register_merge(c, m[0], m[1], m[2]))) return rc;
        }
        geometry(c);
        hipStream_t s = c->stream;
        HIP_TRY(hipMemsetAsync(c->d_repl, 0, nb * sizeof(unsigned long long), s));
        for (int64_t j = 0; j < nb; ++j)
            if ((rc = enqueue_apply(c, abc + 3 * (i0 + j), c->d_repl + j))) return rc;
        HIP_TRY(hipMemcpyAsync(c->h_repl, c->d_repl, nb * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int64_t j = 0; j < nb; ++j) {
            const int32_t *m = abc + 3 * (i0 + j);
            const int64_t R = (int64_t)c->h_repl[j];
            account_merge(c, m[0], m[1], m[2], R, 0);   // (a replay is no iteration and no pass)
            if (replaced) replaced[i0 + j] = R;
        }
        c->counts_valid = false;
        c->cold_exact = false;
        c->best_ready = false;
        i0 += nb;
    }
    if (count_after && n > 0) {
        const int32_t *m = abc + 3 * (n - 1);
        int64_t R = 0;
        if ((rc = do_apply(c, m[0], m[1], m[2], &R))) return rc;
        if (replaced) replaced[n - 1] = R;
    }
    return BPE_OK;
}

int append_begin(bpe_ctx *c, int64_t extra_slots) {
    int rc;
    if ((rc = settle(c))) return rc;
    if (!c->packed)
        if ((rc = compact(c))) return rc;
    return ensure_chunks(c, (c->live_slots + extra_slots + CHUNK - 1) / CHUNK);
}

}  // namespace

int bpe_fail(int code, const char *msg) { return fail(code, msg); }

// a multi-device context forwards the call; per-shard entry points refuse it
// Device scratch freed on scope exit (the sample index is a rare, host-facing operation).
struct Scratch {
    std::vector<void *> p;
    template <typename T>
    int get(T **out, size_t n) {
        int rc = dev_alloc(out, n);
        if (!rc) p.push_back(*out);
        return rc;
    }
    ~Scratch() {
        for (void *q : p) dfree(q);
    }
};

// Where every sample ends: slot_end[i] = the slot of sample i's terminator, live_end[i] = the
// live tokens of samples 0..i.  Two reads of the corpus (k_census, k_sep_emit), one host sync.
int sample_ends(bpe_ctx *c, std::vector<int64_t> &slot_end, std::vector<int64_t> &live_end) {
    int rc;
    if ((rc = settle(c))) return rc;
    const int64_t ns = c->n_samples;
    slot_end.assign(ns, 0);
    live_end.assign(ns, 0);
    if (!ns) return BPE_OK;
    geometry(c);
    Scratch t;
    int64_t *d_live, *d_seps, *d_slot, *d_lend;
    if ((rc = t.get(&d_live, c->R)) || (rc = t.get(&d_seps, c->R)) || (rc = t.get(&d_slot, ns)) ||
        (rc = t.get(&d_lend, ns)))
        return rc;
    hipStream_t s = c->stream;
    const int blocks = (c->R + 3) / 4;
    k_census<<<blocks, 256, 0, s>>>(c->d_ids, c->n_chunks, c->cpr, c->R, d_live, d_seps);
    k_scan_pair<<<1, 1024, 0, s>>>(c->R, d_live, d_seps);
    k_sep_emit<<<blocks, 256, 0, s>>>(c->d_ids, c->n_chunks, c->cpr, c->R, d_live, d_seps, ns,
                                      d_slot, d_lend);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(slot_end.data(), d_slot, ns * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(live_end.data(), d_lend, ns * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (live_end[ns - 1] != c->n_live)
        return fail(BPE_ERR_STATE, "bpe native: corpus layout mismatch (sample index)");
    return BPE_OK;
}

int sample_lengths(bpe_ctx *c, int64_t *lens, int64_t cap) {
    if (cap < c->n_samples || (c->n_samples && !lens))
        return fail(BPE_ERR_ARG, "bpe native: sample_lengths buffer too small");
    std::vector<int64_t> se, le;
    int rc = sample_ends(c, se, le);
    if (rc) return rc;
    for (int64_t i = 0; i < c->n_samples; ++i) lens[i] = le[i] - (i ? le[i - 1] : 0);
    return BPE_OK;
}

// Live ids of samples idx[0..n), packed in that order: one gather of their slot ranges on the
// device, one copy back, the dead slots dropped on the host.
int read_samples(bpe_ctx *c, const int64_t *idx, int64_t n, int32_t *ids_out, int64_t ids_cap,
                 int64_t *off) {
    if (n < 0 || (n && !idx) || !off) return fail(BPE_ERR_ARG, "bpe native: bad read_samples arguments");
    off[0] = 0;
    if (!n) return BPE_OK;
    std::vector<int64_t> se, le;
    int rc = sample_ends(c, se, le);
    if (rc) return rc;
    std::vector<int64_t> src(n), len(n), dst(n + 1);
    int64_t need = 0;
    dst[0] = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t i = idx[k];
        if (i < 0 || i >= c->n_samples) return fail(BPE_ERR_ARG, "bpe native: sample index out of range");
        src[k] = i ? se[i - 1] + 1 : 0;
        len[k] = se[i] - src[k];
        dst[k + 1] = dst[k] + len[k];
        need += le[i] - (i ? le[i - 1] : 0);
    }
    if (ids_cap < need || (need && !ids_out))
        return fail(BPE_ERR_ARG, "bpe native: read_samples buffer too small");
    const int64_t total = dst[n];
    std::vector<int32_t> buf(total);
    if (total) {
        Scratch t;
        int64_t *d_src, *d_len, *d_dst;
        int32_t *d_out;
        if ((rc = t.get(&d_src, n)) || (rc = t.get(&d_len, n)) || (rc = t.get(&d_dst, n)) ||
            (rc = t.get(&d_out, total)))
            return rc;
        hipStream_t s = c->stream;
        HIP_TRY(hipMemcpyAsync(d_src, src.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_len, len.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_dst, dst.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, s));
        k_gather_ranges<<<(unsigned)std::min<int64_t>(n, 1 << 16), 256, 0, s>>>(c->d_ids, d_src, d_len,
                                                                                d_dst, n, d_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(buf.data(), d_out, total * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    int64_t o = 0;
    for (int64_t k = 0; k < n; ++k) {
        for (int64_t j = dst[k]; j < dst[k + 1]; ++j)
            if (buf[j] >= 0) ids_out[o++] = buf[j];
        off[k + 1] = o;
    }
    if (o != need) return fail(BPE_ERR_STATE, "bpe native: corpus layout mismatch (read_samples)");
    return BPE_OK;
}

// ================================================================================================
// The incremental mergeUntil on the position index (bpe_pix.hip.h)
// ================================================================================================
struct PixState {
    PixCorpus C{};
    PixTable T{};
    PixBufs B{};
    PixCtl *d_ctl = nullptr, *h_ctl = nullptr;
    long long *d_log = nullptr, *h_log = nullptr;
    uint64_t cap = 0;
    int64_t max_length = 0;
    std::vector<void *> owned;
};
constexpr int64_t PIX_BATCH = 256;      // merges per host round trip
constexpr int PIX_NOT_ELIGIBLE = 100;   // (internal) the corpus does not fit the index

void pix_free(bpe_ctx *c) {
    PixState *P = c->pix;
    if (!P) return;
    for (void *q : P->owned) dfree(q);
    if (P->h_ctl) (void)hipHostFree(P->h_ctl);
    if (P->h_log) (void)hipHostFree(P->h_log);
    delete P;
    c->pix = nullptr;
}

template <typename T>
int pix_alloc(PixState *P, T **out, size_t n) {
    int rc = dev_alloc(out, n);
    if (!rc) P->owned.push_back(*out);
    return rc;
}

// The index of the current corpus: the slot array is the compacted corpus itself (d_ids, n live
// slots), links i -> i +- 1, and every pair's list from a counting scatter into the pair table
// (bpe_pix.hip.h, index build): run starts per block and their carries, then per position its
// pair's slot, list length and count, a pool segment per pair, and the positions into the
// segments.  A table that fills past a quarter is built again four times larger.
int pix_build_timed(bpe_ctx *c, int64_t max_length);

int pix_build(bpe_ctx *c, int64_t max_length) {
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = pix_build_timed(c, max_length);
    if (c->stats_on && rc == BPE_OK)
        c->stats.pix_build_ms +=
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

// A size knob of the index build and of pix_reserve, read from the environment where the size is
// used (once per build or reserve): `dflt` when unset or not a positive number, never below `least`.
static uint64_t pix_knob(const char *name, uint64_t dflt, uint64_t least) {
    const char *v = getenv(name);
    const long long x = v ? atoll(v) : 0;
    return x > 0 ? std::max<uint64_t>((uint64_t)x, least) : dflt;
}
// BPE_PIX_TABLE_FLOOR=n (tests): the pair table's least capacity in slots (default 2^20, at least
// 2^10; the build rounds it up to a power of two), so that a small corpus fills its table and
// pix_reserve's rehash is reached.
static uint64_t pix_table_floor() { return pix_knob("BPE_PIX_TABLE_FLOOR", 1u << 20, 1u << 10); }
// BPE_PIX_POOL_SLACK=n (tests): the floor, in entries, of the pool's room beyond the corpus at the
// build (default 2^22) and of the free room below which pix_reserve grows it (default 2^20), so
// that a small corpus reaches the pool's growth.
static uint64_t pix_pool_slack(uint64_t dflt) { return pix_knob("BPE_PIX_POOL_SLACK", dflt, 1); }

int pix_build_timed(bpe_ctx *c, int64_t max_length) {
    int rc;
    if ((rc = settle(c))) return rc;
    if (!c->packed)
        if ((rc = compact(c))) return rc;
    const int64_t n = c->live_slots;
    // positions and pool offsets are 32-bit (PIX_NONE = 2^32 - 1 is no position; the margin keeps
    // a block's end, block * PB + PB, below 2^32); the vocabulary key is two 16-bit ids
    // (a shard of a sharded corpus may hold fewer than two slots: its index is just empty)
    if (n > (int64_t)PIX_MAX_SLOTS || c->h_len16.size() > 0xFFFF) return PIX_NOT_ELIGIBLE;
    if ((rc = ensure_vocab(c, (int64_t)c->h_len16.size()))) return rc;
    if ((rc = sync_len16(c, 1))) return rc;
    pix_free(c);
    PixState *P = c->pix = new PixState();
    P->max_length = max_length;
    hipStream_t s = c->stream;
    const uint32_t N = (uint32_t)n;
    PixCorpus &C = P->C;
    C.tok = c->d_ids;
    digest_stale(c, WRITER_OUTSIDE);   // (the index merges in place in d_ids)
    C.n = N;
    if ((rc = pix_alloc(P, &C.nxt, N)) || (rc = pix_alloc(P, &C.prv, N))) return rc;
    const uint64_t pool_cap = std::min<uint64_t>(0xFFFFFFF0ull, (uint64_t)N + std::max<uint64_t>(N / 2, pix_pool_slack(1u << 22)));
    PixBufs &B = P->B;
    if ((rc = pix_alloc(P, &B.pool, pool_cap))) return rc;
    const uint32_t nblk = (N + PB - 1) / PB;
    uint32_t *carry;
    if ((rc = pix_alloc(P, &carry, nblk))) return rc;
    k_pix_build_links<<<4096, 256, 0, s>>>(C, carry);
    k_pix_scan_max<<<1, 1024, 0, s>>>(carry, nblk);
    HIP_TRY(hipGetLastError());
    if ((rc = pix_alloc(P, &P->d_ctl, 1)) || (rc = pix_alloc(P, &P->d_log, PIX_LOG * PIX_BATCH))) return rc;
    HIP_TRY(hipHostMalloc((void **)&P->h_ctl, sizeof(PixCtl), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void **)&P->h_log, PIX_LOG * PIX_BATCH * sizeof(long long), hipHostMallocDefault));
    // the hot passes' scratch: per workgroup and half a slab of 32768 counts (then offsets), the
    // hot pairs' totals, slots and uncounted (x, x) occurrences
    Scratch hs;
    const int G = (int)std::max<uint32_t>(1, std::min<uint32_t>(PH_WG_MAX, nblk));
    uint32_t *slab, *htot, *hslot, *hseg, *bucket, *xoff;
    unsigned long long *oddxx;
    if ((rc = hs.get(&slab, (size_t)2 * G * PH_HALF)) || (rc = hs.get(&htot, 65536)) ||
        (rc = hs.get(&hslot, 65536)) || (rc = hs.get(&oddxx, 256)) || (rc = hs.get(&hseg, 65536)) ||
        (rc = hs.get(&bucket, 257)) || (rc = hs.get(&xoff, (size_t)G * 256)))
        return rc;
    // the pair table: room for the current pairs and the ones merges will add (a shard of a
    // sharded corpus: also every pair of the other shards, pix_min_cap)
    uint64_t cap = 1u << 10;
    const uint64_t floor_cap = pix_table_floor();
    while (cap < floor_cap || cap < (uint64_t)N / 8 || cap < c->pix_min_cap) cap <<= 1;
    PixTable &T = P->T;
    for (int attempt = 0;; ++attempt) {
        if (cap >= (1ull << 31)) return PIX_NOT_ELIGIBLE;   // (slot numbers keep PIX_OWNER free)
        P->cap = cap;
        T = PixTable{};
        T.mask = (uint32_t)(cap - 1);
        T.len16 = c->d_len16;
        T.ml = max_length;
        T.nblocks = (uint32_t)(cap / PIX_B);
        T.nsuper = (T.nblocks + PIX_SB - 1) / PIX_SB;
        if ((rc = pix_alloc(P, &T.keys, cap)) || (rc = pix_alloc(P, &T.cnt, cap)) ||
            (rc = pix_alloc(P, &T.off, cap)) || (rc = pix_alloc(P, &T.len, cap)) ||
            (rc = pix_alloc(P, &T.fill, cap)) || (rc = pix_alloc(P, &T.bmax, T.nblocks)) ||
            (rc = pix_alloc(P, &T.sbmax, T.nsuper)) || (rc = pix_alloc(P, &T.bdirty, T.nblocks)) ||
            (rc = pix_alloc(P, &T.sbdirty, T.nsuper)))
            return rc;
        HIP_TRY(hipMemsetAsync(T.keys, 0xFF, cap * sizeof(uint32_t), s));
        HIP_TRY(hipMemsetAsync(T.cnt, 0, cap * sizeof(unsigned long long), s));
        HIP_TRY(hipMemsetAsync(T.len, 0, cap * sizeof(uint32_t), s));
        HIP_TRY(hipMemsetAsync(T.bdirty, 0, T.nblocks * sizeof(uint32_t), s));
        HIP_TRY(hipMemsetAsync(T.sbdirty, 0, T.nsuper * sizeof(uint32_t), s));
        HIP_TRY(hipMemsetAsync(oddxx, 0, 256 * sizeof(unsigned long long), s));
        PixCtl *h = P->h_ctl;
        memset(h, 0, sizeof *h);
        h->status = PIX_RUN;
        h->max_length = max_length;
        h->max_id = BPE_MAX_VOCAB;
        h->next_id = (int32_t)c->h_len16.size();
        h->pool_cap = pool_cap;
        h->used_cap = cap / 10 * 7;
        HIP_TRY(hipMemcpyAsync(P->d_ctl, h, sizeof *h, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(slab, 0, (size_t)2 * G * PH_HALF * sizeof(uint32_t), s));
        k_pix_hot_count<<<G, PH_T, 0, s>>>(C, T, P->d_ctl, carry, slab, oddxx);
        k_pix_hot_xoff<<<256, 256, 0, s>>>(slab, G, xoff);
        k_pix_hot_scan<<<2 * PH_HALF / 256, 256, 0, s>>>(slab, G, htot);
        k_pix_hot_claim<<<65536 / 256, 256, 0, s>>>(T, P->d_ctl, htot, oddxx, hslot);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, P->d_ctl, sizeof *h, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (!h->err && h->used * 4 <= cap) break;
        // too full to probe well: a table four times larger
        for (void *q : {(void *)T.keys, (void *)T.cnt, (void *)T.off, (void *)T.len, (void *)T.fill,
                        (void *)T.bmax, (void *)T.sbmax, (void *)T.bdirty, (void *)T.sbdirty}) {
            P->owned.erase(std::find(P->owned.begin(), P->owned.end(), q));
            dfree(q);
        }
        cap <<= 2;
        if (attempt == 3) return PIX_NOT_ELIGIBLE;
    }
    // the hot pairs' segments in (x, y) order (buckets by first token), then the cold pairs'
    k_pix_hot_seg<<<1, 1024, 0, s>>>(T, P->d_ctl, htot, hslot, hseg, bucket);
    k_pix_build_alloc<<<4096, 256, 0, s>>>(T, P->d_ctl, (uint32_t)cap, 1);
    HIP_TRY(hipGetLastError());
    // The two-level fill when no first token holds more than 1/32 of the hot positions (a
    // workgroup per bucket does the second level); else the per-pair cursors (k_pix_hot_fill)
    uint32_t hb[257];
    HIP_TRY(hipMemcpyAsync(hb, bucket, sizeof hb, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint32_t bmax = 0;
    for (int x = 0; x < 256; ++x) bmax = std::max(bmax, hb[x + 1] - hb[x]);
    uint2 *stage = nullptr;
    const bool two_level = hb[256] > 0 && (uint64_t)bmax * 32 <= (uint64_t)hb[256] + (1u << 20) &&
                           !getenv("BPE_PIX_FILL_PAIRS") && hs.get(&stage, hb[256]) == BPE_OK;
    if (!two_level) (void)hipGetLastError();   // (a failed staging allocation is not an error)
    if (two_level) {
        k_pix_fill_x<<<G, PH_T, 0, s>>>(C, T, B, xoff, bucket, stage);
        k_pix_fill_y<<<256, 1024, 0, s>>>(B, hseg, bucket, stage);
    } else {
        for (int half = 0; half < 2; ++half)
            k_pix_hot_fill<<<G, PH_T, 0, s>>>(C, T, B, half, slab, hslot);
    }
    HIP_TRY(hipGetLastError());
    // per-merge buffers
    B.site_cap = (uint32_t)std::min<uint64_t>(N / 2 + 16, 1u << 26);
    B.ent_cap = 2 * B.site_cap + 16;
    if ((rc = pix_alloc(P, &B.sites, B.site_cap)) || (rc = pix_alloc(P, &B.ent, B.ent_cap)) ||
        (rc = pix_alloc(P, &B.dblocks, T.nblocks)) || (rc = pix_alloc(P, &B.dsuper, T.nsuper)))
        return rc;
    k_pix_bmax_all<<<4096, 256, 0, s>>>(T);
    k_pix_sbmax<<<1024, 256, 0, s>>>(T, B, P->d_ctl, 1);
    HIP_TRY(hipGetLastError());
    PixCtl *h = P->h_ctl;
    HIP_TRY(hipMemcpyAsync(h, P->d_ctl, sizeof *h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h->status != PIX_RUN) return fail(BPE_ERR_STATE, "bpe native: position index: pair table full");
    if (h->pool_top > (uint64_t)N) return fail(BPE_ERR_STATE, "bpe native: position index: bad pair lists");
    c->counts_valid = c->carry_valid = c->best_ready = false;
    c->cold_exact = false;
    if (c->stats_on) c->stats.pix_builds += 1;
    return BPE_OK;
}

// The corpus back into the chunk layout: the live slots of the slot array, in order, as a dense
// prefix (then the streaming path's state is rebuilt on its next use).
int pix_finish(bpe_ctx *c) {
    PixState *P = c->pix;
    if (!P) return BPE_OK;
    hipStream_t s = c->stream;
    const uint32_t N = P->C.n;
    {
        Scratch t;
        uint32_t *cnt, *d_total;
        const uint32_t nblk = (N + PB - 1) / PB;
        int rc;
        if ((rc = t.get(&cnt, nblk)) || (rc = t.get(&d_total, 1))) return rc;
        // (no fill first: the scatter writes the live prefix, seal_packed the rest that is read)
        k_pix_live_count<<<4096, 256, 0, s>>>(c->d_ids, N, cnt);
        k_pix_scan_sum<<<1, 1024, 0, s>>>(cnt, nblk, d_total);
        k_pix_live_scatter<<<4096, 256, 0, s>>>(c->d_ids, N, cnt, c->d_tmp);
        HIP_TRY(hipGetLastError());
        uint32_t nsel = 0;
        HIP_TRY(hipMemcpyAsync(&nsel, d_total, sizeof nsel, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if ((int64_t)nsel != c->live_slots)
            return fail(BPE_ERR_STATE, "bpe native: position index: live slots lost");
    }
    std::swap(c->d_ids, c->d_tmp);
    pix_free(c);
    return seal_packed(c);   // (a corpus written from outside the merge loop)
}

int pix_reserve(bpe_ctx *c);

// The n-th merge of a mergeUntil call into the caller's list, while it has room.
static void put_merge(int64_t *out_abw, int64_t cap, int64_t n, int64_t a, int64_t b, int64_t w) {
    if (n >= cap) return;
    out_abw[3 * n] = a;
    out_abw[3 * n + 1] = b;
    out_abw[3 * n + 2] = w;
}

// mergeUntil on the index: batches of PIX_BATCH merges, one host round trip each.  An iteration
// the index cannot take (PIX_HOST) runs on the streaming path, and the index is rebuilt after it.
int pix_merge_until(bpe_ctx *c, int64_t max_length, int64_t min_weight, int64_t max_iterations,
                    int64_t *out_abw, int64_t cap, int64_t *n_merges) {
    int rc;
    int64_t n = 0;
    const int64_t mw = min_weight == 0 ? 2 : min_weight;                  // core.ts:256
    int builds = 0;
    bool just_built = false;
    LEAVE_GLOBAL(c);
    // Heavy merges first on the stream: a merge costs the index O(W) (plus contention on the
    // new pairs' slots when W is large), the stream one pass whatever W.  While the next merge's
    // W exceeds max(2^16, n_live / 8192) (C3: 131 K against W = 16 K, so never; a skewed corpus's
    // first merges replace millions), the streaming path takes it (findNextMerge + applyMerge),
    // and the index is built once the merges get light.  Zipf C3, incremental mode: 1.34 ms/merge
    // without the prefix; 0.585 / 0.363 / 0.309 / 0.432 with n_live / 512 / 2048 / 8192 / 32768
    // (tools/pix_wdiv.sh), against 0.394 for the stream alone.
    static const int64_t w_div = [] {
        const char *v = getenv("BPE_PIX_WDIV");   // (A/B knob)
        const long long d = v ? atoll(v) : 8192;
        return (int64_t)(d > 0 ? d : 8192);
    }();
    while (!c->pix && (!max_iterations || n < max_iterations)) {
        if ((rc = settle(c))) return rc;
        if (c->n_live < 2) break;
        int32_t a, b;
        int64_t w;
        rc = do_find(c, max_length, min_weight, &a, &b, &w);
        if (rc == BPE_NO_MERGE) {
            *n_merges = n;
            return settle(c);
        }
        if (rc) return rc;
        if (w <= (int64_t)1 << 16 || w * w_div <= c->n_live) break;   // light: the index from here
        const int32_t cc = (int32_t)c->h_len16.size();
        if ((rc = do_apply(c, a, b, cc, nullptr))) return rc;
        if (c->pending) c->pend_expect = w;
        if ((rc = settle(c))) return rc;
        put_merge(out_abw, cap, n, a, b, w);
        ++n;
    }
    while (!max_iterations || n < max_iterations) {                      // core.ts:374-378
        if (!c->pix || c->pix->max_length != max_length) {
            if ((rc = pix_finish(c))) return rc;
            if ((rc = settle(c))) return rc;
            if (c->n_live < 2) break;
            rc = pix_build(c, max_length);
            ++builds;
            just_built = true;
            if (rc == BPE_ERR_OOM) {
                // (the index does not fit next to the corpus: the stream needs no extra memory)
                if (c->pix) {
                    (void)hipStreamSynchronize(c->stream);
                    pix_free(c);
                }
                rc = PIX_NOT_ELIGIBLE;
            }
            if (rc == PIX_NOT_ELIGIBLE) {
                pix_free(c);
                *n_merges = n;
                return PIX_NOT_ELIGIBLE;   // the caller goes on with the streaming loop
            }
            if (rc) return rc;
        }
        if (builds && !just_built)
            if ((rc = pix_reserve(c))) return rc;   // (grow the pool / table in place)
        just_built = false;
        if (c->pix_hook) c->pix_hook(c->pix_hook_user, 0);   // (checking: the index before a batch)
        PixState *P = c->pix;
        hipStream_t s = c->stream;
        const int64_t base = (int64_t)c->h_len16.size();
        const int64_t batch = c->pix_dbg_batch > 0 ? c->pix_dbg_batch : PIX_BATCH;
        int64_t want = std::min<int64_t>(batch, BPE_MAX_VOCAB - base);
        if (max_iterations) want = std::min<int64_t>(want, max_iterations - n);
        if ((rc = len16_for_batch(c, std::max<int64_t>(want, 1)))) return rc;
        int status = PIX_HOST;
        int64_t nd = 0;
        if (want > 0) {
            P->T.len16 = c->d_len16;   // (ensure_len16_cap may have moved it)
            k_pix_begin<<<1, 1, 0, s>>>(P->d_ctl, want, (int32_t)base, mw);
            for (int64_t i = 0; i < want; ++i) {
                k_pix_select<<<1, 1024, 0, s>>>(P->T, P->B, P->d_ctl);
                k_pix_sites<<<PIX_GRID, 256, 0, s>>>(P->C, P->T, P->B, P->d_ctl);
                k_pix_alloc<<<PIX_GRID, 256, 0, s>>>(P->T, P->B, P->d_ctl);
                k_pix_apply<<<PIX_GRID, 256, 0, s>>>(P->C, P->T, P->B, P->d_ctl, P->d_log);
            }
            HIP_TRY(hipGetLastError());
            PixCtl *h = P->h_ctl;
            HIP_TRY(hipMemcpyAsync(h, P->d_ctl, sizeof *h, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(P->h_log, P->d_log, PIX_LOG * want * sizeof(long long),
                                   hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            status = h->status;
            nd = h->n_done;
            if (status == PIX_ERROR) {
                char msg[160];
                snprintf(msg, sizeof msg, "bpe native: position index inconsistent (code %d)", h->err);
                return fail(BPE_ERR_STATE, msg);
            }
            if (nd < 0 || nd > want) return fail(BPE_ERR_STATE, "bpe native: position index: bad merge count");
            c->h_len16.resize(base + nd, 1);
            c->h_count.resize(base + nd, 0);
            for (int64_t i = 0; i < nd; ++i, ++n) {
                const int32_t a = (int32_t)P->h_log[PIX_LOG * i], b = (int32_t)P->h_log[PIX_LOG * i + 1];
                const int64_t W = P->h_log[PIX_LOG * i + 2];
                const int64_t cc = base + i;
                c->h_len16[cc] = c->h_len16[a] + c->h_len16[b];            // core.ts:318
                account_merge(c, a, b, (int32_t)cc, W, ACCT_ITER | ACCT_PIX);
                put_merge(out_abw, cap, n, a, b, W);
            }
            c->len16_lo = base + nd;   // pix_commit wrote the new lengths on the device
            if (c->pix_hook) c->pix_hook(c->pix_hook_user, 1);   // (checking: the index after a batch)
            if (status == PIX_DONE) break;
            if (status == PIX_RUN || status == PIX_PAUSE) continue;
            if (c->stats_on) c->stats.pix_host += 1;
        }
        if (max_iterations && n >= max_iterations) break;
        // PIX_HOST: this iteration on the streaming path, then a fresh index
        if ((rc = pix_finish(c))) return rc;
        if (builds > 64 && builds > n / 16) {
            *n_merges = n;
            return PIX_NOT_ELIGIBLE;   // (the index keeps failing here: stay on the stream)
        }
        int32_t a, b;
        int64_t w;
        rc = do_find(c, max_length, min_weight, &a, &b, &w);
        if (rc == BPE_NO_MERGE) break;
        if (rc) return rc;
        const int32_t cc = (int32_t)c->h_len16.size();
        if ((rc = do_apply(c, a, b, cc, nullptr))) return rc;
        if (c->pending) c->pend_expect = w;
        if ((rc = settle(c))) return rc;
        put_merge(out_abw, cap, n, a, b, w);
        ++n;
    }
    if ((rc = pix_finish(c))) return rc;
    *n_merges = n;
    return settle(c);
}

// ================================================================================================
// A shard of a sharded corpus in the incremental mode: the position index inside the rank loop
// (bpe_pix.hip.h, "a shard of a sharded corpus").  The index holds this shard's lists and every
// pair's GLOBAL count; each merge's count changes travel as delta rows.
// ================================================================================================

// bpe_set_global_counts in the incremental mode: this shard's index, then the global counts (the
// summed table's hot bins, every shard's cold pairs) in place of its own.
int pix_set_global(bpe_ctx *c, const unsigned long long *table, const uint32_t *keys,
                   const unsigned long long *counts, int64_t n) {
    int rc;
    // every pair of the corpus at most half the table (n counts a pair once per shard holding it;
    // pix_reserve grows the table in place as merges add pairs)
    c->pix_min_cap = 2 * (uint64_t)(HOT_BINS + n);
    // (BPE_PIX_FORCE_OOM=1, tests: the build fails as if out of device memory)
    rc = getenv("BPE_PIX_FORCE_OOM") ? BPE_ERR_OOM : pix_build(c, c->opt_max_length);
    c->pix_min_cap = 0;
    if (rc == PIX_NOT_ELIGIBLE || rc == BPE_ERR_OOM) {
        if (c->pix) {
            (void)hipStreamSynchronize(c->stream);
            pix_free(c);
        }
        return fail(BPE_ERR_NOFIT, "bpe native: the position index does not fit this shard "
                                   "(use the streaming mode)");
    }
    if (rc) return rc;
    PixState *P = c->pix;
    hipStream_t s = c->stream;
    HIP_TRY(hipMemsetAsync(P->T.cnt, 0, P->cap * sizeof(unsigned long long), s));
    k_pix_load_global<<<1024, 256, 0, s>>>(P->T, P->d_ctl, table, keys, counts, n);
    k_pix_bmax_all<<<4096, 256, 0, s>>>(P->T);
    k_pix_sbmax<<<1024, 256, 0, s>>>(P->T, P->B, P->d_ctl, 1);
    HIP_TRY(hipGetLastError());
    PixCtl *h = P->h_ctl;
    HIP_TRY(hipMemcpyAsync(h, P->d_ctl, sizeof *h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h->err || h->used * 2 > P->cap) {
        pix_free(c);
        return fail(BPE_ERR_STATE, "bpe native: position index: the global pairs overflow the table");
    }
    c->rl_global = true;
    c->rl_pix = true;
    c->rl_delta_pending = false;
    c->pix_w_last = 0;   // (the first batch's lanes: full words)
    c->counts_valid = c->sketch_valid = c->best_ready = false;
    c->cold_exact = false;
    return BPE_OK;
}

// Room for the next batch, grown in place (no hand-off, no rebuild): the pool when less than an
// eighth of the corpus is left of it (the new segments of a merge take two entries per site), the
// pair table (rehashed twice as large) past 45 % fill.  Between batches, with no tie pending (a
// decided tie names its pair by slot).  A shard of a sharded corpus grows its own index alone.
int pix_reserve(bpe_ctx *c) {
    PixState *P = c->pix;
    hipStream_t s = c->stream;
    PixCtl *h = P->h_ctl;
    HIP_TRY(hipMemcpyAsync(h, P->d_ctl, sizeof *h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h->status != PIX_RUN && h->status != PIX_PAUSE) return BPE_OK;
    const uint64_t N = P->C.n;
    const uint64_t slack = std::max<uint64_t>(N / 8, pix_pool_slack(1u << 20));
    if (h->pool_top + slack > h->pool_cap && h->pool_cap < 0xFFFFFFF0ull) {
        const uint64_t ncap = std::min<uint64_t>(0xFFFFFFF0ull, h->pool_cap + std::max<uint64_t>(N / 2, 4 * slack));
        uint32_t *np = nullptr;
        int rc = dev_alloc(&np, ncap);
        if (rc == BPE_OK) {
            HIP_TRY(hipMemcpyAsync(np, P->B.pool, h->pool_top * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipStreamSynchronize(s));
            P->owned.erase(std::find(P->owned.begin(), P->owned.end(), (void *)P->B.pool));
            dfree(P->B.pool);
            P->B.pool = np;
            P->owned.push_back(np);
            h->pool_cap = ncap;
            HIP_TRY(hipMemcpyAsync(&P->d_ctl->pool_cap, &h->pool_cap, sizeof h->pool_cap,
                                   hipMemcpyHostToDevice, s));
        } else {
            (void)hipGetLastError();   // (no memory: the pool fills, and the batch hands over)
        }
    }
    if (h->used * 20 > P->cap * 9 && h->tie == PIX_TIE_NONE && P->cap * 2 < (1ull << 31)) {
        const uint64_t ncap = P->cap * 2;
        PixTable T = P->T;
        T.mask = (uint32_t)(ncap - 1);
        T.nblocks = (uint32_t)(ncap / PIX_B);
        T.nsuper = (T.nblocks + PIX_SB - 1) / PIX_SB;
        std::vector<void *> fresh;
        auto get = [&](auto **q, size_t n) {
            const int r = dev_alloc(q, n);
            if (r == BPE_OK) fresh.push_back(*q);
            return r;
        };
        uint32_t *dblocks = nullptr, *dsuper = nullptr;
        if (get(&T.keys, ncap) || get(&T.cnt, ncap) || get(&T.off, ncap) || get(&T.len, ncap) ||
            get(&T.fill, ncap) || get(&T.bmax, T.nblocks) || get(&T.sbmax, T.nsuper) ||
            get(&T.bdirty, T.nblocks) || get(&T.sbdirty, T.nsuper) || get(&dblocks, T.nblocks) ||
            get(&dsuper, T.nsuper)) {
            for (void *q : fresh) dfree(q);
            (void)hipGetLastError();
            return BPE_OK;   // (no memory: the table fills, and the batch hands over)
        }
        HIP_TRY(hipMemsetAsync(T.keys, 0xFF, ncap * sizeof(uint32_t), s));
        // (as in the build: a pair claimed later counts and lists from 0; k_pix_rehash writes only
        // the slots of the pairs it moves, and fresh device memory is not always zero)
        HIP_TRY(hipMemsetAsync(T.cnt, 0, ncap * sizeof(unsigned long long), s));
        HIP_TRY(hipMemsetAsync(T.len, 0, ncap * sizeof(uint32_t), s));
        HIP_TRY(hipMemsetAsync(T.bdirty, 0, T.nblocks * sizeof(uint32_t), s));
        HIP_TRY(hipMemsetAsync(T.sbdirty, 0, T.nsuper * sizeof(uint32_t), s));
        k_pix_rehash<<<4096, 256, 0, s>>>(P->T, T, P->d_ctl, (uint32_t)P->cap);
        // (the old table's dirty lists name its blocks: every block max is recomputed instead)
        h->n_dblocks = h->n_dsuper = 0;
        h->used_cap = ncap / 10 * 7;
        HIP_TRY(hipMemcpyAsync(&P->d_ctl->n_dblocks, &h->n_dblocks, 2 * sizeof(uint32_t),
                               hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(&P->d_ctl->used_cap, &h->used_cap, sizeof h->used_cap,
                               hipMemcpyHostToDevice, s));
        PixBufs B = P->B;
        B.dblocks = dblocks;
        B.dsuper = dsuper;
        k_pix_bmax_all<<<4096, 256, 0, s>>>(T);
        k_pix_sbmax<<<1024, 256, 0, s>>>(T, B, P->d_ctl, 1);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, P->d_ctl, sizeof *h, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (h->err) return fail(BPE_ERR_STATE, "bpe native: position index: rehash overflow");
        for (void *q : {(void *)P->T.keys, (void *)P->T.cnt, (void *)P->T.off, (void *)P->T.len,
                        (void *)P->T.fill, (void *)P->T.bmax, (void *)P->T.sbmax, (void *)P->T.bdirty,
                        (void *)P->T.sbdirty, (void *)P->B.dblocks, (void *)P->B.dsuper}) {
            P->owned.erase(std::find(P->owned.begin(), P->owned.end(), q));
            dfree(q);
        }
        for (void *q : fresh) P->owned.push_back(q);
        P->T = T;
        P->B = B;
        P->cap = ncap;
    }
    return BPE_OK;
}

int pix_rank_begin(bpe_ctx *c, int64_t max_length, int64_t min_weight, unsigned long long *xchg,
                   unsigned long long *tie, int rank, int world, int64_t *n_words) {
    int rc;
    PixState *P = c->pix;
    hipStream_t s = c->stream;
    if ((rc = pix_reserve(c))) return rc;
    const int64_t base = (int64_t)c->h_len16.size();
    if ((rc = len16_for_batch(c, LOOP_BATCH))) return rc;
    P->T.len16 = c->d_len16;
    if (P->max_length != max_length) {
        // (the selection keys filter on max_length: every block max again)
        P->max_length = max_length;
        P->T.ml = max_length;
        c->pix_w_last = 0;   // (pairs the filter held back may now count more than the last W)
        k_pix_bmax_all<<<4096, 256, 0, s>>>(P->T);
        k_pix_sbmax<<<1024, 256, 0, s>>>(P->T, P->B, P->d_ctl, 1);
    }
    P->T.delta = xchg;
    // the exchange: the lane layout (a count per token id and side, in lanes as wide as the last
    // merge's count needs, bpe_pix.hip.h), or (BPE_XCHG_DENSE=1, A/B and checks) six dense rows per
    // token id
    const bool dense = getenv("BPE_XCHG_DENSE") != nullptr;   // (read per batch: tests switch it)
    const int64_t ids = std::min<int64_t>(BPE_MAX_VOCAB, base + LOOP_BATCH + 1);
    int64_t nw;
    // (the last batch's pending merge keeps its own layout for its decode, and its words)
    c->pix_first_pending = c->rl_delta_pending;
    for (int i = 0; i < 3; ++i) c->pix_lane_prev[i] = c->pix_lane[i];
    // (a pending merge's rows span the words of its own batch's layout, lanes or dense rows: this
    // batch all-reduces at least those, whatever layout it takes itself)
    const int64_t prev_words = c->rl_delta_pending ? c->pix_nw_last : 0;
    if (dense) {
        P->T.lane_w = P->T.lane_q = P->T.lane_base = 0;
        nw = std::max<int64_t>(XCHG_HDR + DELTA_ROWS * ids, prev_words);
    } else {
        uint32_t w = c->pix_w_last ? 64u - (uint32_t)__builtin_clzll(c->pix_w_last) : 64u;
        // (BPE_XCHG_LANE_BITS=n, tests: lanes of at most n bits after a known count, so that
        // counts outgrow them, pause the batch and the next one takes full words)
        if (const char *lb = getenv("BPE_XCHG_LANE_BITS"))
            if (c->pix_w_last) w = std::max(1u, std::min<uint32_t>(w, (uint32_t)atoi(lb)));
        const uint32_t q = 64u / w;
        P->T.lane_w = w;
        P->T.lane_q = q;
        P->T.lane_base = (uint32_t)((ids + q - 1) / q);
        nw = std::max<int64_t>(XCHG_HDR + PIX_XCHG_SPECIAL + 2 * (int64_t)P->T.lane_base, prev_words);
    }
    c->pix_nw_last = nw;
    c->pix_lane[0] = P->T.lane_w;
    c->pix_lane[1] = P->T.lane_q;
    c->pix_lane[2] = P->T.lane_base;
    // (delta pending: the last batch's last merge's rows are in xchg, for this batch's first
    // all-reduce; else all of it zero: the rows past this batch's words are read by later ones)
    if (!c->rl_delta_pending)
        HIP_TRY(hipMemsetAsync(xchg, 0, XCHG_WORDS * sizeof(unsigned long long), s));
    k_pix_rank_begin<<<1, 1, 0, s>>>(P->d_ctl, LOOP_BATCH, (int32_t)base,
                                     min_weight == 0 ? 2 : min_weight);   // core.ts:256
    HIP_TRY(hipGetLastError());
    c->opt_max_length = max_length;
    c->rl_table = xchg;
    c->rl_tie = tie;
    c->rl_rank = rank;
    c->rl_world = world;
    c->rl_base = base;
    c->rl_enqueued = 0;
    c->rl_max_length = max_length;
    c->rl_open = true;
    *n_words = nw;
    return BPE_OK;
}

int pix_rank_select(bpe_ctx *c) {
    PixState *P = c->pix;
    hipStream_t s = c->stream;
    hipEvent_t e = span_begin(c);
    // (the batch's first iteration decodes the last batch's pending merge in its layout)
    PixTable T = P->T;
    if (c->rl_enqueued == 0 && c->pix_first_pending) {
        T.lane_w = c->pix_lane_prev[0];
        T.lane_q = c->pix_lane_prev[1];
        T.lane_base = c->pix_lane_prev[2];
    }
    k_pix_apply_delta<<<PIX_GRID, 256, 0, s>>>(T, P->B, P->d_ctl, c->rl_table);
    k_pix_dirty<<<PIX_GRID, 256, 0, s>>>(P->T, P->B, P->d_ctl);
    k_pix_select<<<1, 1024, 0, s>>>(P->T, P->B, P->d_ctl);
    k_pix_sites<<<PIX_GRID, 256, 0, s>>>(P->C, P->T, P->B, P->d_ctl);
    k_pix_export<<<1, 64, 0, s>>>(P->d_ctl, c->rl_table, c->rl_tie, c->rl_rank);
    HIP_TRY(hipGetLastError());
    return span_end(c, e, 1);
}

int pix_rank_decide(bpe_ctx *c) {
    (void)c;   // (the decision is made by k_pix_alloc's block 0 in pix_rank_count)
    return BPE_OK;
}

int pix_rank_count(bpe_ctx *c) {
    PixState *P = c->pix;
    hipStream_t s = c->stream;
    hipEvent_t e = span_begin(c);
    k_pix_alloc<<<PIX_GRID, 256, 0, s>>>(P->T, P->B, P->d_ctl, c->rl_tie);   // (+ k_pix_decide)
    k_pix_apply<<<PIX_GRID, 256, 0, s>>>(P->C, P->T, P->B, P->d_ctl, P->d_log);
    HIP_TRY(hipGetLastError());
    c->rl_enqueued += 1;
    return span_end(c, e, 0);
}

int pix_rank_end(bpe_ctx *c, int64_t *out, int64_t cap, int64_t *n_done, int *status) {
    c->rl_open = false;
    PixState *P = c->pix;
    hipStream_t s = c->stream;
    PixCtl *h = P->h_ctl;
    HIP_TRY(hipMemcpyAsync(h, P->d_ctl, sizeof *h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(P->h_log, P->d_log, PIX_LOG * std::max<int64_t>(1, c->rl_enqueued) * sizeof(long long),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h->status == PIX_ERROR) {
        const int err = h->err;
        const unsigned long long got = h->n_check, W = h->W;
        LEAVE_GLOBAL(c);
        char msg[200];
        if (err == 21)
            snprintf(msg, sizeof msg, "bpe native: rank loop (incremental): the shards' replacement "
                     "counts sum to %llu, not W = %llu", got, W);
        else
            snprintf(msg, sizeof msg, "bpe native: rank loop (incremental): position index "
                     "inconsistent (code %d)", err);
        return fail(BPE_ERR_STATE, msg);
    }
    const int64_t nd = h->n_done;
    if (nd < 0 || nd > c->rl_enqueued) return fail(BPE_ERR_STATE, "bpe native: rank loop: bad merge count");
    const int64_t base = c->rl_base;
    c->h_len16.resize(base + nd, 1);
    c->h_count.resize(base + nd, 0);
    for (int64_t i = 0; i < nd; ++i) {
        const long long *m = P->h_log + PIX_LOG * i;
        const int32_t a = (int32_t)m[0], b = (int32_t)m[1];
        const int64_t W = m[2], R = m[3];
        const int64_t cc = base + i;
        c->h_len16[cc] = c->h_len16[a] + c->h_len16[b];                // core.ts:318
        account_merge(c, a, b, (int32_t)cc, R, ACCT_ITER | ACCT_PIX);
        if (i < cap) {
            out[4 * i] = a;
            out[4 * i + 1] = b;
            out[4 * i + 2] = W;
            out[4 * i + 3] = R;
        }
    }
    c->len16_lo = base + nd;   // (pix_commit wrote the new lengths on the device)
    const int st = h->status == PIX_DONE ? LOOP_DONE : h->status == PIX_HOST ? LOOP_HOST : LOOP_RUN;
    // the next batch's lanes: the last merge's count bounds every later one's (and each of its
    // per-neighbour counts); a count past the lanes (lane_over) takes full words once
    if (nd > 0) c->pix_w_last = (unsigned long long)P->h_log[PIX_LOG * (nd - 1) + 2];
    if (h->lane_over) {
        c->pix_w_last = 0;
        HIP_TRY(hipMemsetAsync(&P->d_ctl->lane_over, 0, sizeof(uint32_t), s));
    }
    if (st != LOOP_RUN) {
        static const bool dbg = getenv("BPE_DEBUG_PIX") != nullptr;
        if (dbg)
            fprintf(stderr, "[bpe debug] rank %d: incremental rank loop hands over after %lld merges "
                    "(status %d, code %d, used %llu of %llu, pool %llu of %llu, candidates %u)\n",
                    c->rl_rank, (long long)nd, h->status, h->err, h->used, h->used_cap, h->pool_top,
                    h->pool_cap, h->n_cand);
        if (c->stats_on && st == LOOP_HOST) c->stats.pix_host += 1;
        LEAVE_GLOBAL(c);   // (the host takes over: the corpus back to the chunk layout)
    } else {
        c->rl_delta_pending = h->merged != 0;
    }
    *n_done = nd;
    *status = st;
    return BPE_OK;
}

#define MULTI(call) \
    if (c && c->multi) return multi_##call
#define NOT_MULTI                                                                          \
    if (c && c->multi)                                                                     \
        return fail(BPE_ERR_STATE, "bpe native: a per-shard entry point on a multi-device " \
                                   "context (drive its shards through bpe_create instead)")

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

int bpe_version(void) { return 201; }

int bpe_digest(const int32_t *ids, int64_t n, uint8_t *out) {
    if (n < 0 || (n > 0 && (!ids || !out))) return fail(BPE_ERR_ARG, "bpe native: bad digest arguments");
    for (int64_t i = 0; i < n; ++i) out[i] = (uint8_t)digest_of(ids[i]);
    return BPE_OK;
}

int bpe_last_error(char *buf, size_t cap) {
    if (!buf || !cap) return BPE_ERR_ARG;
    snprintf(buf, cap, "%s", g_err.c_str());
    return BPE_OK;
}

int bpe_device_count(int *n) {
    if (!n) return fail(BPE_ERR_ARG, "bpe native: null argument");
    int k = 0;
    if (hipGetDeviceCount(&k) != hipSuccess) k = 0;
    *n = k;
    return BPE_OK;
}

int bpe_create(bpe_ctx **out, int device) {
    if (!out) return fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return fail(BPE_ERR_HIP, "bpe native: no HIP device available (MI355X required)");
    if (device < 0 || device >= n) return fail(BPE_ERR_ARG, "bpe native: bad device index");
    bpe_ctx *c = new bpe_ctx();
    c->device = device;
    c->use_incr = !getenv("BPE_FUSED");
    c->use_pix = getenv("BPE_PIX") && atoi(getenv("BPE_PIX")) > 0;
    int rc;
    auto bail = [&](int code) {
        bpe_destroy(c);
        return code;
    };
    if ((rc = set_device(c))) return bail(rc);
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
        return bail(fail(BPE_ERR_HIP, "bpe native: hipStreamCreate failed"));
    if ((rc = dev_alloc(&c->d_spill, TABLE_BINS))) return bail(rc);
    if (hipMemset(c->d_spill, 0, TABLE_BINS * sizeof(unsigned long long)) != hipSuccess)
        return bail(fail(BPE_ERR_HIP, "bpe native: hipMemset failed"));
    if ((rc = dev_alloc(&c->d_hot, TABLE_BINS))) return bail(rc);
    if ((rc = dev_alloc(&c->d_heavy, HEAVY_WORDS))) return bail(rc);
    if ((rc = dev_alloc(&c->d_total, 2))) return bail(rc);
    if ((rc = dev_alloc(&c->d_sums, MAX_REGIONS))) return bail(rc);
    if ((rc = dev_alloc(&c->d_carry, MAX_REGIONS))) return bail(rc);
    if ((rc = dev_alloc(&c->d_outoff, MAX_REGIONS))) return bail(rc);
    if ((rc = dev_alloc(&c->d_res, 1))) return bail(rc);
    if ((rc = dev_alloc(&c->d_cand, CAND_CAP))) return bail(rc);
    if ((rc = dev_alloc(&c->d_cold_flags, 8))) return bail(rc);
    if (hipHostMalloc((void **)&c->h_cand, MAX_CAND * sizeof(int2), hipHostMallocDefault) != hipSuccess)
        return bail(fail(BPE_ERR_HIP, "bpe native: hipHostMalloc failed"));
    if (hipHostMalloc((void **)&c->h_res, sizeof(Result), hipHostMallocDefault) != hipSuccess)
        return bail(fail(BPE_ERR_HIP, "bpe native: hipHostMalloc failed"));
    if ((rc = dev_alloc(&c->d_ctl, 1))) return bail(rc);
    if ((rc = dev_alloc(&c->d_ticket, TICKET_WORDS))) return bail(rc);
    if ((rc = dev_alloc(&c->d_brec, COLD_GRID))) return bail(rc);
    if ((rc = dev_alloc(&c->d_site_n, MAX_REGIONS))) return bail(rc);
    if ((rc = dev_alloc(&c->d_lists, 1))) return bail(rc);
    // (no pair cached, no row to apply from, no block keys)
    if (hipMemset(c->d_lists, 0, sizeof(DigestLists)) != hipSuccess ||
        hipMemset(c->d_lists, 0xFF, offsetof(DigestLists, bkey)) != hipSuccess ||
        hipMemset(c->d_ticket, 0, TICKET_WORDS * sizeof(unsigned int)) != hipSuccess)
        return bail(fail(BPE_ERR_HIP, "bpe native: memset failed"));
    if ((rc = dev_alloc(&c->d_repl, REPLAY_BATCH))) return bail(rc);
    if (hipHostMalloc((void **)&c->h_repl, REPLAY_BATCH * sizeof(unsigned long long),
                      hipHostMallocDefault) != hipSuccess)
        return bail(fail(BPE_ERR_HIP, "bpe native: hipHostMalloc failed"));
    if ((rc = dev_alloc(&c->d_log, LOG_WORDS * LOOP_BATCH))) return bail(rc);
    if (hipHostMalloc((void **)&c->h_ctl, sizeof(LoopCtl), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&c->h_log, LOG_WORDS * LOOP_BATCH * sizeof(long long), hipHostMallocDefault) !=
            hipSuccess)
        return bail(fail(BPE_ERR_HIP, "bpe native: hipHostMalloc failed"));
    if (hipMemset(c->d_cold_flags, 0, 32) != hipSuccess)
        return bail(fail(BPE_ERR_HIP, "bpe native: memset failed"));
    if ((rc = ensure_chunks(c, 1))) return bail(rc);
    if ((rc = ensure_vocab(c, 0))) return bail(rc);
    if ((rc = ensure_cold(c, 0))) return bail(rc);
    if ((rc = seal_packed(c))) return bail(rc);
    *out = c;
    return BPE_OK;
}

int bpe_create_multi(bpe_ctx **out, int n_shards, const int *devices, int reduce) {
    if (!out) return fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = nullptr;
    bpe_multi *m = nullptr;
    int rc = multi_create(&m, n_shards, devices, reduce);
    if (rc) return rc;
    bpe_ctx *c = new bpe_ctx();
    c->multi = m;
    *out = c;
    return BPE_OK;
}

int bpe_shard_count(bpe_ctx *c, int *n) {
    if (!c || !n) return fail(BPE_ERR_ARG, "bpe native: null argument");
    MULTI(shard_count(c->multi, n));
    *n = 1;
    return BPE_OK;
}

int bpe_destroy(bpe_ctx *c) {
    if (!c) return BPE_OK;
    if (c->multi) {
        multi_destroy(c->multi);
        delete c;
        return BPE_OK;
    }
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    rank_rccl_forget(c);
    pix_free(c);
    ingest_free(c);
    append_free(c);
    export_free(c);
    if (c->u8) {
        u8_free(*c->u8);
        delete c->u8;
    }
    if (c->ln) {
        ln_free(*c->ln);
        delete c->ln;
    }
    if (c->sg) {
        sg_free(*c->sg);
        delete c->sg;
    }
    void *ptrs[] = {c->d_ids, c->d_tmp, c->d_len16, c->d_partials, c->d_spill, c->d_hot,
                    c->d_total, c->d_sums, c->d_carry, c->d_outoff, c->d_res, c->d_cand,
                    c->d_heavy, c->d_cold_flags, c->cold.slots, c->cold.dkeys, c->cold.dcounts,
                    c->cold.bmax, c->cold.bdirty, c->cold.blist,
                    c->d_ctl, c->d_log, c->d_repl, c->d_ticket, c->d_brec, c->d_sites,
                    c->d_site_n, c->d_digest, c->d_lists, c->d_rows};
    for (void *p : ptrs) dfree(p);
    if (c->h_res) (void)hipHostFree(c->h_res);
    if (c->h_cand) (void)hipHostFree(c->h_cand);
    if (c->h_ctl) (void)hipHostFree(c->h_ctl);
    if (c->h_log) (void)hipHostFree(c->h_log);
    if (c->h_repl) (void)hipHostFree(c->h_repl);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto &sp : c->spans) c->ev_pool.insert(c->ev_pool.end(), {sp.a, sp.b});
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return BPE_OK;
}

int bpe_set_token_len16(bpe_ctx *c, int32_t id, int32_t len16) {
    MULTI(set_token_len16(c->multi, id, len16));
    if (!c || id < 0 || len16 < 0) return fail(BPE_ERR_ARG, "bpe native: bad token registration");
    if (id >= BPE_MAX_VOCAB)
        return fail(BPE_ERR_VOCAB, "bpe native: vocab is limited to 55295 tokens (UTF-16 surrogates)");
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = ensure_vocab(c, (int64_t)id + 1))) return rc;
    if (c->h_len16[id] != len16) {
        c->h_len16[id] = len16;
        mark_len16(c, id);
    }
    return BPE_OK;
}

int bpe_num_tokens(bpe_ctx *c, int32_t *n) {
    if (c && n) MULTI(num_tokens(c->multi, n));
    if (!c || !n) return fail(BPE_ERR_ARG, "bpe native: null argument");
    *n = (int32_t)c->h_len16.size();
    return BPE_OK;
}

int bpe_add_sample(bpe_ctx *c, const int32_t *ids, int64_t n) {
    if (n >= 0 && (n == 0 || ids)) MULTI(add_sample(c->multi, ids, n));
    if (!c || n < 0 || (n > 0 && !ids)) return fail(BPE_ERR_ARG, "bpe native: bad sample");
    int rc = set_device(c);
    if (rc) return rc;
    int32_t mx = -1;
    for (int64_t i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= BPE_MAX_VOCAB)
            return fail(BPE_ERR_ARG, "bpe native: token id out of range in sample");
        mx = std::max(mx, ids[i]);
    }
    if ((rc = ensure_vocab(c, (int64_t)mx + 1))) return rc;
    if ((rc = append_begin(c, n + 1))) return rc;
    std::vector<int32_t> buf(ids, ids + n);
    buf.push_back(SEP);
    HIP_TRY(hipMemcpyAsync(c->d_ids + c->live_slots, buf.data(), buf.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice, c->stream));
    for (int64_t i = 0; i < n; ++i) c->h_count[ids[i]] += 1;
    c->live_slots += n + 1;
    c->n_samples += 1;
    c->n_live += n;
    if ((rc = seal_packed(c))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BPE_OK;
}

int bpe_add_latin1(bpe_ctx *c, const uint8_t *bytes, int64_t n, int64_t sample_bytes,
                   int32_t char_to_id[256], int32_t *n_tokens_io, int64_t char_hist[256]) {
    if (!c || n < 0 || (n > 0 && !bytes) || !char_to_id || !n_tokens_io || sample_bytes < 0)
        return fail(BPE_ERR_ARG, "bpe native: bad latin1 ingest arguments");
    MULTI(add_latin1(c->multi, bytes, n, sample_bytes, char_to_id, n_tokens_io, char_hist));
    int rc = set_device(c);
    if (rc) return rc;
    if (n == 0) {
        if (char_hist) memset(char_hist, 0, 256 * sizeof(int64_t));
        return bpe_add_sample(c, nullptr, 0);
    }
    if (sample_bytes == 0 || sample_bytes > n) sample_bytes = n;
    const int64_t n_smp = (n + sample_bytes - 1) / sample_bytes;
    if ((rc = append_begin(c, n + n_smp))) return rc;
    hipStream_t s = c->stream;
    uint8_t *d_bytes = nullptr;
    unsigned long long *d_stats = nullptr;   // first[256] + hist[256]
    int32_t *d_map = nullptr;
    if ((rc = dev_alloc(&d_bytes, n))) return rc;
    if ((rc = dev_alloc(&d_stats, 512)) || (rc = dev_alloc(&d_map, 256))) {
        dfree(d_bytes);
        dfree(d_stats);
        return rc;
    }
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(s);
        dfree(d_bytes);
        dfree(d_stats);
        dfree(d_map);
    };
    std::vector<unsigned long long> st(512);
    if (hipMemcpyAsync(d_bytes, bytes, n, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(d_stats, 0xFF, 256 * sizeof(unsigned long long), s) != hipSuccess ||
        hipMemsetAsync(d_stats + 256, 0, 256 * sizeof(unsigned long long), s) != hipSuccess) {
        cleanup();
        return fail(BPE_ERR_HIP, "bpe native: latin1 upload failed");
    }
    const int blocks = (int)std::min<int64_t>(2048, (n + 65535) / 65536);
    k_byte_stats<<<blocks, 256, 0, s>>>(d_bytes, n, d_stats, d_stats + 256);
    if (hipMemcpyAsync(st.data(), d_stats, 512 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                       s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        cleanup();
        return fail(BPE_ERR_HIP, "bpe native: latin1 stats failed");
    }
    // first-appearance order for unseen chars (core.ts:186-199)
    std::vector<std::pair<unsigned long long, int>> fresh;
    for (int ch = 0; ch < 256; ++ch)
        if (st[256 + ch] && char_to_id[ch] < 0) fresh.push_back({st[ch], ch});
    std::sort(fresh.begin(), fresh.end());
    int32_t next = *n_tokens_io;
    for (auto &p : fresh) {
        if (next >= BPE_MAX_VOCAB) {
            cleanup();
            return fail(BPE_ERR_VOCAB, "bpe native: vocab limit");
        }
        char_to_id[p.second] = next++;
    }
    if ((rc = ensure_vocab(c, next))) {
        cleanup();
        return rc;
    }
    for (int ch = 0; ch < 256; ++ch) {
        if (st[256 + ch] == 0) continue;
        const int32_t id = char_to_id[ch];
        c->h_count[id] += (int64_t)st[256 + ch];
        if (id >= *n_tokens_io) {
            c->h_len16[id] = 1;
            mark_len16(c, id);
        }
    }
    *n_tokens_io = next;
    if (char_hist)
        for (int ch = 0; ch < 256; ++ch) char_hist[ch] = (int64_t)st[256 + ch];
    if (hipMemcpyAsync(d_map, char_to_id, 256 * sizeof(int32_t), hipMemcpyHostToDevice, s) !=
        hipSuccess) {
        cleanup();
        return fail(BPE_ERR_HIP, "bpe native: map upload failed");
    }
    k_expand_latin1<<<4096, 256, 0, s>>>(d_bytes, n, sample_bytes, d_map,
                                         c->d_ids + c->live_slots);
    hipError_t e = hipGetLastError();
    cleanup();
    if (e != hipSuccess) return fail(BPE_ERR_HIP, "bpe native: latin1 expand failed");
    c->live_slots += n + n_smp;
    c->n_samples += n_smp;
    c->n_live += n;
    if ((rc = seal_packed(c))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return BPE_OK;
}

int bpe_clear_corpus(bpe_ctx *c) {
    MULTI(clear_corpus(c->multi));
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = settle(c))) return rc;
    c->live_slots = c->n_samples = c->n_live = 0;
    std::fill(c->h_count.begin(), c->h_count.end(), 0);
    if ((rc = seal_packed(c))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BPE_OK;
}

int bpe_corpus_size(bpe_ctx *c, int64_t *n_samples, int64_t *n_tokens) {
    MULTI(corpus_size(c->multi, n_samples, n_tokens));
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = settle(c))) return rc;
    if (n_samples) *n_samples = c->n_samples;
    if (n_tokens) *n_tokens = c->n_live;
    return BPE_OK;
}

int bpe_read_corpus(bpe_ctx *c, int32_t *ids_out, int64_t ids_cap, int64_t *sample_off,
                    int64_t off_cap) {
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    MULTI(read_corpus(c->multi, ids_out, ids_cap, sample_off, off_cap));
    if (ids_cap < c->n_live || off_cap < c->n_samples + 1 || (c->n_live && !ids_out) || !sample_off)
        return fail(BPE_ERR_ARG, "bpe native: read_corpus buffers too small");
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = settle(c))) return rc;
    const int64_t slots = c->n_chunks * CHUNK;
    std::vector<int32_t> buf(slots);
    if (slots)
        HIP_TRY(hipMemcpy(buf.data(), c->d_ids, slots * sizeof(int32_t), hipMemcpyDeviceToHost));
    int64_t o = 0, sidx = 0;
    sample_off[0] = 0;
    for (int64_t i = 0; i < slots; ++i) {
        const int32_t v = buf[i];
        if (v < SEP) continue;   // dead slot (TOMB or a tail tag)
        if (v == SEP) {
            if (sidx >= c->n_samples) return fail(BPE_ERR_STATE, "bpe native: corpus layout mismatch");
            sample_off[++sidx] = o;
        } else {
            if (o >= c->n_live) return fail(BPE_ERR_STATE, "bpe native: corpus layout mismatch");
            ids_out[o++] = v;
        }
    }
    if (sidx != c->n_samples || o != c->n_live)
        return fail(BPE_ERR_STATE, "bpe native: corpus layout mismatch");
    return BPE_OK;
}

int bpe_sample_lengths(bpe_ctx *c, int64_t *lens, int64_t cap) {
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    MULTI(sample_lengths(c->multi, lens, cap));
    int rc = set_device(c);
    if (rc) return rc;
    return sample_lengths(c, lens, cap);
}

int bpe_read_samples(bpe_ctx *c, const int64_t *idx, int64_t n, int32_t *ids_out, int64_t ids_cap,
                     int64_t *sample_off) {
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    MULTI(read_samples(c->multi, idx, n, ids_out, ids_cap, sample_off));
    int rc = set_device(c);
    if (rc) return rc;
    return read_samples(c, idx, n, ids_out, ids_cap, sample_off);
}

int bpe_find_next_merge(bpe_ctx *c, int64_t max_length, int64_t min_weight, int32_t *a,
                        int32_t *b, int64_t *w) {
    if (a && b && w) MULTI(find_next_merge(c->multi, max_length, min_weight, a, b, w));
    if (!c || !a || !b || !w) return fail(BPE_ERR_ARG, "bpe native: null argument");
    int rc = set_device(c);
    if (rc) return rc;
    return do_find(c, max_length, min_weight, a, b, w);
}

int bpe_apply_merge(bpe_ctx *c, int32_t a, int32_t b, int32_t cc, int64_t *replaced) {
    MULTI(apply_merge(c->multi, a, b, cc, replaced));
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    int rc = set_device(c);
    if (rc) return rc;
    return do_apply(c, a, b, cc, replaced);
}

int bpe_rank_loop_begin(bpe_ctx *c, int64_t max_length, int64_t min_weight, uint64_t *xchg,
                        uint64_t *tie, int rank, int world, int64_t *xchg_words) {
    NOT_MULTI;
    if (!c || !xchg || !tie || rank < 0 || world < 1 || rank >= world || !xchg_words)
        return fail(BPE_ERR_ARG, "bpe native: bad rank loop arguments");
    int rc = set_device(c);
    if (rc) return rc;
    rc = rank_loop_begin(c, max_length, min_weight, (unsigned long long *)xchg,
                         (unsigned long long *)tie, rank, world, xchg_words);
    if (rc == BPE_OK) c->rl_words = *xchg_words;
    return rc;
}

int bpe_cold_counts(bpe_ctx *c, uint32_t *keys, uint64_t *counts, int64_t cap, int64_t *n) {
    NOT_MULTI;
    if (!c || !n || cap < 0) return fail(BPE_ERR_ARG, "bpe native: null argument");
    int rc = set_device(c);
    if (rc) return rc;
    return cold_counts(c, keys, (unsigned long long *)counts, cap, n);
}

int bpe_set_global_counts(bpe_ctx *c, const uint64_t *table, const uint32_t *keys,
                          const uint64_t *counts, int64_t n) {
    NOT_MULTI;
    if (!c || !table) return fail(BPE_ERR_ARG, "bpe native: null argument");
    int rc = set_device(c);
    if (rc) return rc;
    return set_global_counts(c, (const unsigned long long *)table, keys,
                             (const unsigned long long *)counts, n);
}

int bpe_rank_loop_select(bpe_ctx *c) {
    NOT_MULTI;
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    int rc = set_device(c);
    if (rc == BPE_OK && c->stats_on && c->rl_open) {
        // (every iteration's exchange: one all-reduce(SUM) of rl_words words before this call)
        c->stats.xchg_bytes += c->rl_words * 8;
        c->stats.xchg_iters += 1;
    }
    return rc ? rc : rank_loop_select(c);
}

}  // extern "C"

// (internal, bpe_multi.cpp bpe_rank_loop_rccl) the buffers and size of the open batch: the
// all-reduces a caller issues must be over exactly these
int rank_loop_buffers(bpe_ctx *c, unsigned long long **xchg, unsigned long long **tie, int64_t *words) {
    if (!c || !c->rl_open) return fail(BPE_ERR_STATE, "bpe native: rank loop not begun");
    *xchg = c->rl_table;
    *tie = c->rl_tie;
    *words = c->rl_words;
    return BPE_OK;
}

extern "C" {

int bpe_rank_loop_decide(bpe_ctx *c) {
    NOT_MULTI;
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    int rc = set_device(c);
    return rc ? rc : rank_loop_decide(c);
}

int bpe_rank_loop_count(bpe_ctx *c) {
    NOT_MULTI;
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    int rc = set_device(c);
    return rc ? rc : rank_loop_count(c);
}

int bpe_rank_loop_end(bpe_ctx *c, int64_t *out_abwr, int64_t cap, int64_t *n_merges, int *status) {
    NOT_MULTI;
    if (!c || !n_merges || !status || (cap > 0 && !out_abwr))
        return fail(BPE_ERR_ARG, "bpe native: null argument");
    int rc = set_device(c);
    return rc ? rc : rank_loop_end(c, out_abwr, cap, n_merges, status);
}

int bpe_apply_merges(bpe_ctx *c, const int32_t *abc, int64_t n, int64_t *replaced, int count_after) {
    if (n >= 0 && (n == 0 || abc)) MULTI(apply_merges(c->multi, abc, n, replaced, count_after));
    if (!c || n < 0 || (n > 0 && !abc)) return fail(BPE_ERR_ARG, "bpe native: bad apply_merges arguments");
    int rc = set_device(c);
    if (rc) return rc;
    return replay(c, abc, n, replaced, count_after != 0);
}

// The streaming mergeUntil: batches on the device-resident loop, host iterations between them.
static int merge_until_stream(bpe_ctx *c, int64_t max_length, int64_t min_weight, int64_t max_iterations,
                       int64_t *out_abw, int64_t cap, int64_t *n_merges) {
    int rc;
    int64_t n = 0;
    const int64_t mw = min_weight == 0 ? 2 : min_weight;                  // core.ts:256
    int64_t abw[3 * LOOP_BATCH];
    // Batch size adapts to how often the host path is needed: a batch that ends early leaves its
    // remaining iterations' launches as no-ops, so after an early end the next batch is sized to
    // about twice the merges that one finished; after a batch that finished none, the device loop
    // rests for a few host iterations (backing off up to 16) before it is tried again.
    int64_t batch = LOOP_BATCH, rest = 0, backoff = 0;
    while (!max_iterations || n < max_iterations) {                      // core.ts:374-378
        // (a maintained cold table: do_find settles the pending merge with its selection, and
        // do_apply compacts)
        if (!(c->pending && c->cold_exact)) {
            if ((rc = settle(c))) return rc;
            if (c->n_live < 2) break;
            if ((rc = maybe_compact(c))) return rc;
        }
        // batches on the device while the vocabulary has room (the host path reports the limit)
        int64_t want = std::min<int64_t>(batch, BPE_MAX_VOCAB - (int64_t)c->h_len16.size());
        if (max_iterations) want = std::min<int64_t>(want, max_iterations - n);
        if (rest > 0) {
            --rest;
            want = 0;
        }
        if (want > 0) {
            int64_t nd = 0;
            int st = LOOP_DONE;
            if ((rc = loop_batch(c, max_length, mw, want, abw, &nd, &st))) return rc;
            for (int64_t i = 0; i < nd; ++i, ++n)
                if (n < cap)
                    for (int q = 0; q < 3; ++q) out_abw[3 * n + q] = abw[3 * i + q];
            if (st == LOOP_DONE) break;
            if (st == LOOP_RUN) {
                batch = std::min<int64_t>(LOOP_BATCH, 2 * batch);
                backoff = 0;
                continue;
            }
            batch = std::max<int64_t>(1, std::min<int64_t>(LOOP_BATCH, 2 * nd));
            if (nd == 0) rest = backoff = std::min<int64_t>(16, 2 * backoff + 1);
            else backoff = 0;
            if (max_iterations && n >= max_iterations) break;
        }
        // LOOP_HOST (heavy sketch buckets, many tied candidates) or no vocabulary room: one
        // host-driven iteration
        int32_t a, b;
        int64_t w;
        rc = do_find(c, max_length, min_weight, &a, &b, &w);
        if (rc == BPE_NO_MERGE) break;
        if (rc) return rc;
        const int32_t cc = (int32_t)c->h_len16.size();
        if ((rc = do_apply(c, a, b, cc, nullptr))) return rc;
        if (c->pending) c->pend_expect = w;    // checked when the count comes back
        put_merge(out_abw, cap, n, a, b, w);
        ++n;
    }
    *n_merges = n;
    return settle(c);
}

int bpe_merge_until(bpe_ctx *c, int64_t max_length, int64_t min_weight, int64_t max_iterations,
                    int64_t *out_abw, int64_t cap, int64_t *n_merges) {
    if (n_merges && (cap <= 0 || out_abw)) MULTI(merge_until(c->multi, max_length, min_weight, max_iterations, out_abw, cap, n_merges));
    if (!c || !n_merges || (cap > 0 && !out_abw))
        return fail(BPE_ERR_ARG, "bpe native: null argument");
    int rc = set_device(c);
    if (rc) return rc;
    if (!c->use_pix) return merge_until_stream(c, max_length, min_weight, max_iterations, out_abw, cap, n_merges);
    int64_t n = 0;
    rc = pix_merge_until(c, max_length, min_weight, max_iterations, out_abw, cap, &n);
    *n_merges = n;
    if (rc != PIX_NOT_ELIGIBLE) return rc;
    // the corpus does not fit the index (or keeps failing it): the stream takes the rest
    if (max_iterations && n >= max_iterations) return settle(c);
    int64_t m = 0;
    rc = merge_until_stream(c, max_length, min_weight, max_iterations ? max_iterations - n : 0,
                            cap > n ? out_abw + 3 * n : out_abw, cap - n, &m);
    *n_merges = n + m;
    return rc;
}

int bpe_set_mode(bpe_ctx *c, int mode) {
    if (mode == BPE_MODE_STREAM || mode == BPE_MODE_INCREMENTAL) MULTI(set_mode(c->multi, mode));
    if (!c || (mode != BPE_MODE_STREAM && mode != BPE_MODE_INCREMENTAL))
        return fail(BPE_ERR_ARG, "bpe native: bad mode");
    c->use_pix = mode == BPE_MODE_INCREMENTAL;
    return BPE_OK;
}

int bpe_export_counts(bpe_ctx *c, uint64_t *table) {
    NOT_MULTI;
    if (!c || !table) return fail(BPE_ERR_ARG, "bpe native: null argument");
    int rc = set_device(c);
    if (rc) return rc;
    LEAVE_GLOBAL(c);
    if ((rc = settle(c))) return rc;
    if (!table_ok(c))
        if ((rc = run_pass(c, false, 0, 0, 0, nullptr))) return rc;
    HIP_TRY(hipMemcpyAsync(table, c->d_hot, TABLE_BINS * sizeof(uint64_t), hipMemcpyDeviceToDevice,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BPE_OK;
}

int bpe_heavy_counts(bpe_ctx *c, const uint64_t *table, int64_t max_length, uint32_t *cold_keys,
                     uint64_t *cold_counts, int64_t cap, int64_t *n_cold) {
    NOT_MULTI;
    if (!c || !table || !n_cold || cap < 0) return fail(BPE_ERR_ARG, "bpe native: null argument");
    int rc = set_device(c);
    if (rc) return rc;
    LEAVE_GLOBAL(c);
    if ((rc = settle(c))) return rc;
    if ((rc = sync_len16(c, max_length))) return rc;
    hipStream_t s = c->stream;
    const auto *t = (const unsigned long long *)table;
    HIP_TRY(hipMemsetAsync(c->d_res, 0, sizeof(Result), s));
    k_argmax_hot<<<HOT_BINS / 256, 256, 0, s>>>(t, c->d_len16, max_length, c->d_res);
    k_heavy<<<SKETCH_BINS / 256, 256, 0, s>>>(t, c->d_res, c->d_heavy);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_res, c->d_res, sizeof(Result), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n_cold = -1;   // no heavy bucket: the same on every rank (bpe.h)
    if (!c->h_res->n_heavy) return BPE_OK;
    *n_cold = 0;
    if ((rc = exact_pass(c))) return rc;
    uint32_t nu = 0;
    HIP_TRY(hipMemcpy(&nu, c->cold.n_used, sizeof nu, hipMemcpyDeviceToHost));
    nu = std::min<uint32_t>(nu, c->cold.mask + 1);
    *n_cold = nu;
    if ((int64_t)nu > cap) return fail(BPE_ERR_ARG, "bpe native: export buffer too small");
    if (nu) {
        if (!cold_keys || !cold_counts) return fail(BPE_ERR_ARG, "bpe native: null cold buffers");
        k_export_cold<<<256, 256, 0, s>>>(c->cold, cold_keys, (unsigned long long *)cold_counts);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
    }
    return BPE_OK;
}

int bpe_select_counts(bpe_ctx *c, const uint64_t *table, const uint32_t *cold_keys,
                      const uint64_t *cold_counts, int64_t n_cold, int64_t max_length,
                      int64_t min_weight, int32_t *cand, int64_t cap, int64_t *n_cand,
                      int64_t *w) {
    NOT_MULTI;
    const uint64_t *hot = table;
    if (!c || !hot || !n_cand || !w || n_cold < 0 || (n_cold && (!cold_keys || !cold_counts)) ||
        (cap > 0 && !cand))
        return fail(BPE_ERR_ARG, "bpe native: bad select arguments");
    int rc = set_device(c);
    if (rc) return rc;
    if (min_weight == 0) min_weight = 2;                               // core.ts:256
    if ((rc = sync_len16(c, max_length))) return rc;
    hipStream_t s = c->stream;
    HIP_TRY(hipMemsetAsync(c->d_res, 0, sizeof(Result), s));
    const auto *h = (const unsigned long long *)hot;
    const auto *cc = (const unsigned long long *)cold_counts;
    k_argmax_hot<<<HOT_BINS / 256, 256, 0, s>>>(h, c->d_len16, max_length, c->d_res);
    if (n_cold)
        k_argmax_list<<<256, 256, 0, s>>>(cold_keys, cc, n_cold, c->d_len16, max_length, c->d_res);
    k_collect_list<<<HOT_BINS / 256, 256, 0, s>>>(h, cold_keys, cc, n_cold, c->d_len16, max_length,
                                                  c->d_res, c->d_cand);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_res, c->d_res, sizeof(Result), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const Result res = *c->h_res;
    *n_cand = 0;
    if (res.best == 0) return BPE_NO_MERGE;                            // core.ts:312
    const int64_t W = (int64_t)(res.best >> 17);
    if (W < min_weight) return BPE_NO_MERGE;                           // core.ts:313
    const int64_t nc = std::min<int64_t>(res.n_cand, CAND_CAP);
    std::vector<int2> buf(nc);
    HIP_TRY(hipMemcpy(buf.data(), c->d_cand, nc * sizeof(int2), hipMemcpyDeviceToHost));
    std::sort(buf.begin(), buf.end(), [](const int2 &x, const int2 &y) {
        return x.x != y.x ? x.x < y.x : x.y < y.y;
    });
    for (int64_t i = 0; i < std::min(nc, cap); ++i) {
        cand[2 * i] = buf[i].x;
        cand[2 * i + 1] = buf[i].y;
    }
    *n_cand = res.n_cand;
    *w = W;
    return BPE_OK;
}

int bpe_tie_positions(bpe_ctx *c, const int32_t *cand, int64_t n, uint64_t *last) {
    NOT_MULTI;
    if (!c || n < 0 || (n > 0 && (!cand || !last)))
        return fail(BPE_ERR_ARG, "bpe native: bad tie arguments");
    int rc = set_device(c);
    if (rc) return rc;
    if (n > CAND_CAP) return fail(BPE_ERR_ARG, "bpe native: too many tie candidates");
    if (n == 0) return BPE_OK;
    std::vector<int2> cv(n);
    for (int64_t i = 0; i < n; ++i) cv[i] = make_int2(cand[2 * i], cand[2 * i + 1]);
    if ((rc = settle(c))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_cand, cv.data(), n * sizeof(int2), hipMemcpyHostToDevice, c->stream));
    return tie_positions(c, c->d_cand, (unsigned)n, (unsigned long long *)last);
}

int bpe_stats_enable(bpe_ctx *c, int on) {
    MULTI(stats_enable(c->multi, on));
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    c->stats_on = on != 0;
    return BPE_OK;
}

int bpe_get_stats(bpe_ctx *c, bpe_stats *out) {
    if (out) MULTI(get_stats(c->multi, out));
    if (!c || !out) return fail(BPE_ERR_ARG, "bpe native: null argument");
    int rc = flush_spans(c);
    if (rc) return rc;
    *out = c->stats;
    return BPE_OK;
}

int bpe_reset_stats(bpe_ctx *c) {
    MULTI(reset_stats(c->multi));
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    int rc = flush_spans(c);
    if (rc) return rc;
    memset(&c->stats, 0, sizeof c->stats);
    return BPE_OK;
}

int bpe_recount(bpe_ctx *c) {
    NOT_MULTI;
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    int rc = set_device(c);
    if (rc) return rc;
    LEAVE_GLOBAL(c);
    if ((rc = settle(c))) return rc;
    return run_pass(c, false, 0, 0, 0, nullptr);
}

// (internal, bpe_multi.cpp) the exchange of shards that share one device: the sum (or max) of the
// shards' buffers written back to every one of them, on `stream` (which the caller orders after
// every shard's producer and before every shard's consumer with events).  No host copies.
}  // extern "C"
namespace {
struct ShardBufs {
    unsigned long long *p[BPE_MAX_SHARDS_ONE_DEVICE];
};
__global__ void __launch_bounds__(256) k_sum_shards(ShardBufs b, int n, size_t count, int take_max) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count;
         i += (size_t)gridDim.x * blockDim.x) {
        unsigned long long v = b.p[0][i];
        for (int r = 1; r < n; ++r) {
            const unsigned long long x = b.p[r][i];
            v = take_max ? (x > v ? x : v) : v + x;
        }
        for (int r = 0; r < n; ++r) b.p[r][i] = v;
    }
}
}  // namespace
extern "C" {
int bpe_sum_shards(unsigned long long *const *bufs, int n, size_t count, int take_max, void *stream) {
    if (n < 1 || n > BPE_MAX_SHARDS_ONE_DEVICE) return fail(BPE_ERR_ARG, "bpe native: too many shards on one device");
    ShardBufs b{};
    for (int r = 0; r < n; ++r) b.p[r] = bufs[r];
    const unsigned grid = (unsigned)std::min<size_t>(1024, (count + 255) / 256 + 1);
    k_sum_shards<<<grid, 256, 0, (hipStream_t)stream>>>(b, n, count, take_max);
    HIP_TRY(hipGetLastError());
    return BPE_OK;
}

// (internal, bpe_multi.cpp) the corpus of one shard changed outside the rank loop: every shard
// leaves the replicated global tables, so the next batch starts from the table state on all alike
int bpe_leave_global(bpe_ctx *c) {
    if (!c || c->multi) return fail(BPE_ERR_ARG, "bpe native: bad shard context");
    const int rc = set_device(c);
    if (rc) return rc;
    LEAVE_GLOBAL(c);
    return BPE_OK;
}

// (internal, bpe_multi.cpp) whether this shard still holds the global state it entered: anything
// that reads its corpus between two batches makes it leave (settle)
int bpe_holds_global(bpe_ctx *c, int *yes) {
    if (!c || c->multi || !yes) return fail(BPE_ERR_ARG, "bpe native: bad shard context");
    *yes = c->rl_global ? 1 : 0;
    return BPE_OK;
}

// (bpe_tools.h; BPE_DEBUG_GLOBAL in bpe_multi.cpp, and the tests) this context's maintained
// tables: the hot bins (HOT_BINS u64 into hot) and the cold table's dense entries (up to cap;
// *n = n_used)
int bpe_debug_tables(bpe_ctx *c, uint64_t *hot, uint32_t *keys, uint64_t *counts, int64_t cap,
                     int64_t *n) {
    if (!c || c->multi || !hot || !n || cap < 0 || (cap > 0 && (!keys || !counts)))
        return fail(BPE_ERR_ARG, "bpe native: bad debug_tables arguments");
    int rc = set_device(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(hot, c->d_hot, HOT_BINS * sizeof(uint64_t), hipMemcpyDeviceToHost));
    *n = 0;
    if (!c->cold_cap) return BPE_OK;   // (no cold table yet)
    uint32_t nu = 0;
    HIP_TRY(hipMemcpy(&nu, c->cold.n_used, sizeof nu, hipMemcpyDeviceToHost));
    uint32_t of = 0;
    HIP_TRY(hipMemcpy(&of, c->cold.overflow, sizeof of, hipMemcpyDeviceToHost));
    if (of) fprintf(stderr, "[bpe debug] cold table overflow (n_used %u, capacity %u)\n", nu, c->cold.mask + 1);
    nu = std::min<uint32_t>(nu, c->cold.mask + 1);
    *n = nu;
    const int64_t k = std::min<int64_t>(nu, cap);
    if (k) {
        HIP_TRY(hipMemcpy(keys, c->cold.dkeys, k * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(counts, c->cold.dcounts, k * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    return BPE_OK;
}

int bpe_debug_tables_shard(bpe_ctx *c, int shard, uint64_t *hot, uint32_t *keys, uint64_t *counts,
                           int64_t cap, int64_t *n) {
    if (!c || !c->multi || !hot || !n || cap < 0 || (cap > 0 && (!keys || !counts)))
        return fail(BPE_ERR_ARG, "bpe native: bad debug_tables_shard arguments");
    return multi_debug_tables_shard(c->multi, shard, hot, keys, counts, cap, n);
}

// (bpe_tools.h) what this context holds of the sharded maintained state of the streaming mode,
// and the exchange buffer it last began a batch with, copied out; nothing is launched or changed
int bpe_debug_global(bpe_ctx *c, int shard, int64_t *info, uint64_t *xchg, int64_t cap) {
    if (!c || !info || cap < 0 || (cap > 0 && !xchg) || (!c->multi && shard != -1))
        return fail(BPE_ERR_ARG, "bpe native: bad debug_global arguments");
    if (c->multi) return multi_debug_global(c->multi, shard, info, xchg, cap);
    int rc = set_device(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const bool held = c->rl_global && !c->rl_pix;
    const bool pending = held && c->rl_delta_pending;
    // (the buffer is the caller's: it is read only while the state that was begun with it is held)
    const int64_t words = held && c->rl_table ? (int64_t)XCHG_WORDS : 0;
    for (int i = 0; i < BPE_GLOBAL_INFO_WORDS; ++i) info[i] = 0;
    info[BPE_GLOBAL_INFO_HELD] = held ? 1 : 0;
    info[BPE_GLOBAL_INFO_PENDING] = pending ? 1 : 0;
    info[BPE_GLOBAL_INFO_A] = pending ? c->rl_last_a : -1;
    info[BPE_GLOBAL_INFO_B] = pending ? c->rl_last_b : -1;
    info[BPE_GLOBAL_INFO_C] = pending ? c->rl_last_c : -1;
    info[BPE_GLOBAL_INFO_W] = pending ? c->rl_last_w : -1;
    info[BPE_GLOBAL_INFO_MULTI] = -1;
    info[BPE_GLOBAL_INFO_XCHG] = words;
    if (cap == 0 || words == 0) return BPE_OK;
    if (cap < words) return fail(BPE_ERR_ARG, "bpe native: debug_global: the buffer is smaller than the sizing call said");
    HIP_TRY(hipMemcpy(xchg, c->rl_table, (size_t)words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return BPE_OK;
}

// (bpe_tools.h) the live position index of a single-device context, copied out
int bpe_debug_pix(bpe_ctx *c, int64_t *info, void *const *arrays) {
    if (!c || c->multi || !info) return fail(BPE_ERR_ARG, "bpe native: bad debug_pix arguments");
    int rc = set_device(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    PixState *P = c->pix;
    if (!P || !P->d_ctl) {
        if (arrays) return fail(BPE_ERR_ARG, "bpe native: debug_pix: no index to copy");
        for (int i = 0; i < BPE_PIX_INFO_WORDS; ++i) info[i] = 0;
        return BPE_OK;
    }
    PixCtl h;
    HIP_TRY(hipMemcpy(&h, P->d_ctl, sizeof h, hipMemcpyDeviceToHost));
    const PixTable &T = P->T;
    int64_t now[BPE_PIX_INFO_WORDS] = {0};
    now[0] = 1;
    now[1] = P->C.n;
    now[2] = (int64_t)P->cap;
    now[3] = T.nblocks;
    now[4] = T.nsuper;
    now[5] = T.ml;
    now[6] = h.status;
    now[7] = h.tie;
    now[8] = h.err;
    now[9] = (int64_t)h.used;
    now[10] = (int64_t)h.used_cap;
    now[11] = (int64_t)h.pool_top;
    now[12] = (int64_t)h.pool_cap;
    now[13] = std::min<uint32_t>(h.n_dblocks, T.nblocks);
    now[14] = std::min<uint32_t>(h.n_dsuper, T.nsuper);
    now[15] = h.next_id;
    now[16] = h.merged;
    now[17] = h.n_done;
    now[18] = c->rl_pix ? 1 : 0;
    now[19] = c->rl_pix && c->rl_delta_pending ? 1 : 0;
    now[20] = h.pair_slot;
    now[21] = h.max_id;
    if (!arrays) {
        for (int i = 0; i < BPE_PIX_INFO_WORDS; ++i) info[i] = now[i];
        return BPE_OK;
    }
    // (the arrays were sized by the first call: nothing may have changed since)
    for (int i = 0; i < BPE_PIX_INFO_WORDS; ++i)
        if (info[i] != now[i]) return fail(BPE_ERR_ARG, "bpe native: debug_pix: the index changed since the sizing call");
    for (int i = 0; i < BPE_PIX_ARRAYS; ++i)
        if (!arrays[i]) return fail(BPE_ERR_ARG, "bpe native: bad debug_pix arguments");
    const size_t n = P->C.n, cap = (size_t)P->cap;
    const size_t top = (size_t)std::min<unsigned long long>(h.pool_top, h.pool_cap);
    const struct { const void *src; size_t bytes; } cp[BPE_PIX_ARRAYS] = {
        {P->C.tok, n * sizeof(int32_t)},       {P->C.nxt, n * sizeof(uint32_t)},
        {P->C.prv, n * sizeof(uint32_t)},      {T.keys, cap * sizeof(uint32_t)},
        {T.cnt, cap * sizeof(uint64_t)},       {T.off, cap * sizeof(uint32_t)},
        {T.len, cap * sizeof(uint32_t)},       {T.fill, cap * sizeof(uint32_t)},
        {T.bmax, T.nblocks * sizeof(uint64_t)}, {T.sbmax, T.nsuper * sizeof(uint64_t)},
        {T.bdirty, T.nblocks * sizeof(uint32_t)}, {T.sbdirty, T.nsuper * sizeof(uint32_t)},
        {P->B.pool, top * sizeof(uint32_t)},   {P->B.dblocks, (size_t)now[13] * sizeof(uint32_t)},
        {P->B.dsuper, (size_t)now[14] * sizeof(uint32_t)},
    };
    for (int i = 0; i < BPE_PIX_ARRAYS; ++i)
        if (cp[i].bytes) HIP_TRY(hipMemcpy(arrays[i], cp[i].src, cp[i].bytes, hipMemcpyDeviceToHost));
    return BPE_OK;
}

int bpe_debug_pix_shard(bpe_ctx *c, int shard, int64_t *info, void *const *arrays) {
    if (!c || !c->multi || !info) return fail(BPE_ERR_ARG, "bpe native: bad debug_pix_shard arguments");
    return multi_debug_pix_shard(c->multi, shard, info, arrays);
}

int bpe_debug_pix_hook(bpe_ctx *c, void (*hook)(void *user, int where), void *user, int64_t batch) {
    if (!c || c->multi || batch < 0 || batch > PIX_BATCH)
        return fail(BPE_ERR_ARG, "bpe native: bad debug_pix_hook arguments");
    c->pix_hook = hook;
    c->pix_hook_user = user;
    c->pix_dbg_batch = batch;
    return BPE_OK;
}

int bpe_table_state(bpe_ctx *c, int *maintained) {
    if (!c || c->multi || !maintained) return fail(BPE_ERR_ARG, "bpe native: bad table_state arguments");
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = settle(c))) return rc;
    *maintained = c->cold_exact && c->counts_valid ? 1 : 0;
    return BPE_OK;
}

int bpe_get_stream(bpe_ctx *c, void **stream) {
    if (stream) MULTI(get_stream(c->multi, stream));
    if (!c || !stream) return fail(BPE_ERR_ARG, "bpe native: null argument");
    *stream = (void *)c->stream;
    return BPE_OK;
}

}  // extern "C"

// ---- corpus from text (bpe_add_text_batch, include/bpe.h): bpe_ingest.hip.h's kernels around the
// host's numbering of the new chars, appended through append_begin / seal_packed ------------------
struct IngestState {
    // the char table (host copy; uploaded when dirty): an empty one knows no char
    std::vector<uint16_t> bmp;
    std::vector<uint2> pairs;
    uint32_t pair_bits = 4;
    int64_t n_pairs = 0;
    bool dirty = true;
    uint16_t *d_bmp = nullptr;
    uint2 *d_pairs = nullptr;
    size_t d_pairs_n = 0;
    // a call's device words: the new chars' planes and list, the counts, the status words
    unsigned long long *d_first = nullptr, *d_sup_pos = nullptr, *d_hist = nullptr, *d_st = nullptr, *d_out = nullptr;
    uint32_t *d_sup_keys = nullptr, *d_list = nullptr;
    char *d_buf = nullptr;   // tile counts, first texts, tile marks, and the host form's units and offsets
    size_t buf_bytes = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bpe_ingest_stats st{};
    IngestState() : bmp(65536, CHAR_UNKNOWN), pairs(16, make_uint2(PAIR_EMPTY, 0u)) {}
};

void ingest_free(bpe_ctx *c) {
    IngestState *I = c->ing;
    if (!I) return;
    void *ptrs[] = {I->d_bmp, I->d_pairs, I->d_first, I->d_sup_pos, I->d_hist, I->d_st,
                    I->d_out, I->d_sup_keys, I->d_list, I->d_buf};
    for (void *p : ptrs) dfree(p);
    for (hipEvent_t ev : I->ev)
        if (ev) (void)hipEventDestroy(ev);
    delete I;
    c->ing = nullptr;
}

namespace {

constexpr size_t ING_OUT_CAP = BPE_MAX_VOCAB;   // (more new chars than that: the call fails first)

// The context's ingest state, with its fixed device words (made by the first call that needs them).
int ingest_state(bpe_ctx *c, IngestState **out, bool device) {
    if (!c->ing) c->ing = new IngestState();
    IngestState *I = *out = c->ing;
    if (!device || I->d_st) return BPE_OK;
    int rc;
    if ((rc = dev_alloc(&I->d_bmp, 65536)) || (rc = dev_alloc(&I->d_first, 65536)) ||
        (rc = dev_alloc(&I->d_sup_pos, ING_SUP_SLOTS)) || (rc = dev_alloc(&I->d_sup_keys, ING_SUP_SLOTS)) ||
        (rc = dev_alloc(&I->d_list, ING_LIST_CAP)) || (rc = dev_alloc(&I->d_hist, BPE_MAX_VOCAB)) ||
        (rc = dev_alloc(&I->d_out, 2 * ING_OUT_CAP)))
        return rc;
    for (hipEvent_t &ev : I->ev)
        if (!ev) HIP_TRY(hipEventCreate(&ev));
    if ((rc = dev_alloc(&I->d_st, IS_WORDS))) return rc;   // (last: marks the state complete)
    return BPE_OK;
}

void ingest_table_put(IngestState *I, uint32_t cp, uint32_t id) {
    I->dirty = true;
    if (cp <= 0xFFFFu) {
        I->bmp[cp] = (uint16_t)id;
        return;
    }
    if (2 * (I->n_pairs + 1) > (int64_t)I->pairs.size()) {   // grow: load factor <= 1/2
        std::vector<uint2> old;
        old.swap(I->pairs);
        I->pair_bits += 1;
        I->pairs.assign((size_t)1 << I->pair_bits, make_uint2(PAIR_EMPTY, 0u));
        I->n_pairs = 0;
        for (const uint2 &e : old)
            if (e.x != PAIR_EMPTY) ingest_table_put(I, e.x, e.y);
    }
    const uint32_t mask = (1u << I->pair_bits) - 1;
    uint32_t h = pair_home(cp, 32 - I->pair_bits);
    while (I->pairs[h].x != PAIR_EMPTY && I->pairs[h].x != cp) h = (h + 1) & mask;
    if (I->pairs[h].x == PAIR_EMPTY) I->n_pairs += 1;
    I->pairs[h] = make_uint2(cp, id);
}

int ingest_table_upload(bpe_ctx *c, IngestState *I) {
    if (!I->dirty) return BPE_OK;
    if (I->pairs.size() > I->d_pairs_n) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        dfree(I->d_pairs);
        I->d_pairs_n = 0;
        int rc = dev_alloc(&I->d_pairs, I->pairs.size());
        if (rc) return rc;
        I->d_pairs_n = I->pairs.size();
    }
    HIP_TRY(hipMemcpyAsync(I->d_bmp, I->bmp.data(), 65536 * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(I->d_pairs, I->pairs.data(), I->pairs.size() * sizeof(uint2), hipMemcpyHostToDevice,
                           c->stream));
    // (the host vectors may change right after: the copies must be done)
    HIP_TRY(hipStreamSynchronize(c->stream));
    I->dirty = false;
    return BPE_OK;
}

size_t ing_align(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

// New char tokens nt, nt + 1, ... for the code points cps[0 .. n) (nt = the token count): registered
// with their len16 and put into the char table.  (bpe_multi.cpp: every shard learns every token.)
int ingest_learn(bpe_ctx *c, const uint32_t *cps, int64_t n) {
    if (!c || c->multi || n < 0 || (n && !cps)) return fail(BPE_ERR_ARG, "bpe native: bad ingest_learn arguments");
    int rc = set_device(c);
    if (rc) return rc;
    IngestState *I;
    if ((rc = ingest_state(c, &I, false))) return rc;
    const int64_t nt0 = (int64_t)c->h_len16.size();
    if (nt0 + n > BPE_MAX_VOCAB) return fail(BPE_ERR_VOCAB, "bpe native: vocab limit");
    if ((rc = ensure_vocab(c, nt0 + n))) return rc;
    for (int64_t i = 0; i < n; ++i) {
        ingest_table_put(I, cps[i], (uint32_t)(nt0 + i));
        c->h_len16[nt0 + i] = cps[i] > 0xFFFFu ? 2 : 1;
    }
    if (n) mark_len16(c, nt0);
    return BPE_OK;
}

// The pipeline.  dev: units and off are device buffers.  number_only: the new chars are numbered
// and reported (every check made) and nothing is changed (bpe_multi.cpp numbers a whole batch on
// one shard before its shards take their parts).
int ingest_text(bpe_ctx *c, const uint16_t *units, const int64_t *off, int64_t n_texts, bool dev, bool number_only,
                uint32_t *new_chars, int64_t new_cap, int64_t *n_new, int64_t *id_hist, int64_t hist_cap) {
    if (!c || c->multi || !n_new || n_texts < 0 || n_texts >= 0x7FFFFFFF || new_cap < 0 || hist_cap < 0 ||
        (n_texts && !off) || (new_cap && !new_chars) || (hist_cap && !id_hist))
        return fail(BPE_ERR_ARG, "bpe native: bad add_text_batch arguments");
    *n_new = 0;
    int rc = set_device(c);
    if (rc) return rc;
    IngestState *I;
    if ((rc = ingest_state(c, &I, true))) return rc;
    hipStream_t s = c->stream;
    if (!number_only) I->st.calls++;
    std::vector<int64_t> off_copy;
    const int64_t *h_off = off;
    if (dev && n_texts) {
        off_copy.resize((size_t)n_texts + 1);
        HIP_TRY(hipMemcpyAsync(off_copy.data(), off, off_copy.size() * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        h_off = off_copy.data();
    }
    if (n_texts && h_off[0] < 0) return fail(BPE_ERR_ARG, "bpe native: negative text offset");
    for (int64_t k = 0; k < n_texts; ++k)
        if (h_off[k + 1] < h_off[k]) return fail(BPE_ERR_ARG, "bpe native: text offsets must not decrease");
    const int64_t base = n_texts ? h_off[0] : 0, total = n_texts ? h_off[n_texts] - base : 0;
    if (total && !units) return fail(BPE_ERR_ARG, "bpe native: null unit buffer");
    const int64_t nt0 = (int64_t)c->h_len16.size();
    const int mis = dev && total ? (int)(((uintptr_t)(units + base) >> 1) & (TXT_RUN - 1)) : 0;
    const int64_t n_tiles = (total + mis + TXT_TILE - 1) / TXT_TILE;
    if (n_tiles > 0x7FFFFFFF) return fail(BPE_ERR_ARG, "bpe native: text batch too large");

    // device: [tile counts, then bases | first text of each tile | tile marks | units | off]
    // (the last two: the host form's staging)
    const uint16_t *units_al = nullptr;
    const int64_t *k_off = nullptr;
    unsigned long long *d_tiles = nullptr;
    long long *d_tfirst = nullptr;
    uint32_t *d_edge = nullptr;
    int64_t chars = 0, n_list = 0;
    std::vector<unsigned long long> fresh;   // (position, code point) pairs
    std::vector<unsigned long long> h_st(IS_WORDS, 0);
    float ms = 0, ms2 = 0;
    if (total) {
        if ((rc = ingest_table_upload(c, I))) return rc;
        const size_t b_tiles = ing_align((size_t)n_tiles * 8), b_edge = ing_align((size_t)n_tiles * 4);
        const size_t b_units = dev ? 0 : ing_align((size_t)total * 2), b_off = dev ? 0 : (size_t)(n_texts + 1) * 8;
        const size_t bytes = 2 * b_tiles + b_edge + b_units + b_off;
        if (bytes > I->buf_bytes) {
            HIP_TRY(hipStreamSynchronize(s));
            dfree(I->d_buf);
            I->buf_bytes = 0;
            if ((rc = dev_alloc(&I->d_buf, bytes + bytes / 4))) return rc;
            I->buf_bytes = bytes + bytes / 4;
        }
        char *d = I->d_buf;
        d_tiles = reinterpret_cast<unsigned long long *>(d);
        d_tfirst = reinterpret_cast<long long *>(d += b_tiles);
        d_edge = reinterpret_cast<uint32_t *>(d += b_tiles);
        uint16_t *d_units = reinterpret_cast<uint16_t *>(d += b_edge);
        int64_t *d_uoff = reinterpret_cast<int64_t *>(d += b_units);
        if (dev) {
            units_al = units + base - mis;
            k_off = off;
        } else {
            HIP_TRY(hipMemcpyAsync(d_units, units + base, (size_t)total * 2, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_uoff, off, (size_t)(n_texts + 1) * 8, hipMemcpyHostToDevice, s));
            units_al = d_units;
            k_off = d_uoff;
        }
        HIP_TRY(hipMemsetAsync(I->d_st, 0, IS_WORDS * 8, s));
        HIP_TRY(hipMemsetAsync(I->d_first, 0xFF, 65536 * 8, s));
        HIP_TRY(hipMemsetAsync(I->d_sup_pos, 0xFF, (size_t)ING_SUP_SLOTS * 8, s));
        HIP_TRY(hipMemsetAsync(I->d_sup_keys, 0xFF, (size_t)ING_SUP_SLOTS * 4, s));
        HIP_TRY(hipMemsetAsync(d_tfirst, 0xFF, (size_t)n_tiles * 8, s));
        HIP_TRY(hipMemsetAsync(d_edge, 0, (size_t)n_tiles * 4, s));
        const CharTab ct{I->d_bmp, I->d_pairs, (1u << I->pair_bits) - 1, 32 - I->pair_bits};
        const IngNew nw{I->d_first, I->d_sup_keys, I->d_sup_pos, I->d_list, I->d_st};
        HIP_TRY(hipEventRecord(I->ev[0], s));
        k_txt_count<<<(unsigned)((n_tiles + TXT_CNT_TILES - 1) / TXT_CNT_TILES), TXT_WG, 0, s>>>(units_al, mis, total,
                                                                                              n_tiles, d_tiles);
        k_txt_texts<<<(unsigned)std::min<int64_t>((n_texts + 256) / 256, 2048), 256, 0, s>>>(
            units_al, mis, total, k_off, n_texts, base, n_tiles, d_tfirst, d_edge, d_tiles);
        k_txt_scan<<<1, 1024, 0, s>>>(d_tiles, n_tiles, I->d_st);
        k_ing_discover<<<(unsigned)n_tiles, TXT_WG, 0, s>>>(units_al, mis, total, ct, d_tfirst, d_edge, k_off, n_texts,
                                                           base, nw);
        k_ing_collect<<<64, 256, 0, s>>>(nw, I->d_out, (uint32_t)ING_OUT_CAP);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(I->ev[1], s));
        HIP_TRY(hipMemcpyAsync(h_st.data(), I->d_st, IS_WORDS * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipEventElapsedTime(&ms, I->ev[0], I->ev[1]));
        I->st.kernel_ms += ms;
        chars = (int64_t)h_st[TS_CHARS];
        n_list = (int64_t)h_st[IS_NLIST];
        if (chars < 0 || chars > total) return fail(BPE_ERR_STATE, "bpe native: bad char count");
        if (h_st[IS_OVER] || nt0 + n_list > BPE_MAX_VOCAB) {
            if (!h_st[IS_OVER]) *n_new = n_list;
            return fail(BPE_ERR_VOCAB, "bpe native: vocab is limited to 55295 tokens (UTF-16 surrogates)");
        }
        if (n_list) {
            // first-appearance order for unseen chars (core.ts:186-199)
            fresh.resize(2 * (size_t)n_list);
            HIP_TRY(hipMemcpyAsync(fresh.data(), I->d_out, fresh.size() * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            std::vector<std::pair<unsigned long long, uint32_t>> order((size_t)n_list);
            for (int64_t i = 0; i < n_list; ++i) order[i] = {fresh[2 * i], (uint32_t)fresh[2 * i + 1]};
            std::sort(order.begin(), order.end());
            for (int64_t i = 0; i < n_list; ++i) fresh[i] = order[i].second;
        }
    }
    const int64_t nt1 = nt0 + n_list;
    *n_new = n_list;
    if (n_list > new_cap) return fail(BPE_ERR_ARG, "bpe native: new_chars too small (see *n_new)");
    if (hist_cap < nt1) return fail(BPE_ERR_ARG, "bpe native: id_hist too small for the token count after the call");
    if (number_only) {
        for (int64_t i = 0; i < n_list; ++i) new_chars[i] = (uint32_t)fresh[i];
        return BPE_OK;
    }
    if (n_texts == 0) {
        std::fill(id_hist, id_hist + nt1, (int64_t)0);
        return BPE_OK;
    }
    // from here on the call succeeds (device failures aside)
    const int64_t extra = chars + n_texts;
    if ((rc = append_begin(c, extra))) return rc;
    if (n_list) {
        std::vector<uint32_t> cps((size_t)n_list);
        for (int64_t i = 0; i < n_list; ++i) cps[i] = (uint32_t)fresh[i];
        if ((rc = ingest_learn(c, cps.data(), n_list))) return rc;
        for (int64_t i = 0; i < n_list; ++i) new_chars[i] = cps[i];
    }
    int32_t *dst = c->d_ids + c->live_slots;
    std::vector<unsigned long long> hist((size_t)nt1, 0);
    if (total) {
        if ((rc = ingest_table_upload(c, I))) return rc;   // (a batch with no new char uploads nothing)
        const CharTab ct{I->d_bmp, I->d_pairs, (1u << I->pair_bits) - 1, 32 - I->pair_bits};
        if (nt1) HIP_TRY(hipMemsetAsync(I->d_hist, 0, (size_t)nt1 * 8, s));
        int64_t grid = std::min<int64_t>(n_tiles, 1024);
        grid = std::max(grid, (n_tiles + ING_MAX_TILES_PER_WG - 1) / ING_MAX_TILES_PER_WG);
        HIP_TRY(hipEventRecord(I->ev[2], s));
        k_ing_map<<<(unsigned)grid, TXT_WG, 0, s>>>(units_al, mis, total, n_tiles, ct, d_tiles, d_tfirst, d_edge, k_off,
                                                    n_texts, base, SEP, dst, I->d_hist, I->d_st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(I->ev[3], s));
        if (nt1) HIP_TRY(hipMemcpyAsync(hist.data(), I->d_hist, (size_t)nt1 * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h_st.data(), I->d_st, IS_WORDS * 8, hipMemcpyDeviceToHost, s));
    } else {
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)dst, SEP, (size_t)n_texts, s));
    }
    c->live_slots += extra;
    c->n_samples += n_texts;
    c->n_live += chars;
    if ((rc = seal_packed(c))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    if (total) {
        HIP_TRY(hipEventElapsedTime(&ms2, I->ev[2], I->ev[3]));
        I->st.kernel_ms += ms2;
        if (h_st[IS_OVER]) return fail(BPE_ERR_STATE, "bpe native: the char table lost a char of the batch");
    }
    for (int64_t id = 0; id < nt1; ++id) {
        c->h_count[id] += (int64_t)hist[id];
        id_hist[id] = (int64_t)hist[id];
    }
    I->st.texts += n_texts;
    I->st.units += total;
    I->st.chars += chars;
    I->st.new_chars += n_list;
    return BPE_OK;
}

int ingest_kernel_ms(bpe_ctx *c, double *ms, bool reset) {
    if (!c || c->multi || !ms) return fail(BPE_ERR_ARG, "bpe native: bad shard context");
    *ms = c->ing ? c->ing->st.kernel_ms : 0.0;
    if (reset && c->ing) c->ing->st = bpe_ingest_stats{};
    return BPE_OK;
}

extern "C" {

int bpe_set_chars(bpe_ctx *c, const uint32_t *code_points, const int32_t *ids, int64_t n) {
    if (!c || n < 0 || (n && (!code_points || !ids))) return fail(BPE_ERR_ARG, "bpe native: bad set_chars arguments");
    MULTI(set_chars(c->multi, code_points, ids, n));
    int rc = set_device(c);
    if (rc) return rc;
    IngestState *I;
    if ((rc = ingest_state(c, &I, false))) return rc;
    // checked and built aside: a failed call changes nothing
    int32_t mx = -1;
    for (int64_t i = 0; i < n; ++i) {
        if (code_points[i] > 0x10FFFFu) return fail(BPE_ERR_ARG, "bpe native: code point above U+10FFFF");
        if (ids[i] < 0 || ids[i] >= BPE_MAX_VOCAB) return fail(BPE_ERR_VOCAB, "bpe native: char token id out of range");
        mx = std::max(mx, ids[i]);
    }
    IngestState T;
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t cp = code_points[i];
        const int64_t before = T.n_pairs;
        if (cp <= 0xFFFFu && T.bmp[cp] != CHAR_UNKNOWN) return fail(BPE_ERR_ARG, "bpe native: duplicate code point");
        ingest_table_put(&T, cp, (uint32_t)ids[i]);
        if (cp > 0xFFFFu && T.n_pairs == before) return fail(BPE_ERR_ARG, "bpe native: duplicate code point");
    }
    const int64_t nt0 = (int64_t)c->h_len16.size();
    if ((rc = ensure_vocab(c, (int64_t)mx + 1))) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (ids[i] >= nt0) c->h_len16[ids[i]] = code_points[i] > 0xFFFFu ? 2 : 1;
    I->bmp.swap(T.bmp);
    I->pairs.swap(T.pairs);
    I->pair_bits = T.pair_bits;
    I->n_pairs = T.n_pairs;
    I->dirty = true;
    return BPE_OK;
}

int bpe_add_text_batch(bpe_ctx *c, const uint16_t *units, const int64_t *off, int64_t n_texts, uint32_t *new_chars,
                       int64_t new_cap, int64_t *n_new, int64_t *id_hist, int64_t hist_cap) {
    if (c && c->multi && n_new)
        return multi_add_text_batch(c->multi, units, off, n_texts, false, new_chars, new_cap, n_new, id_hist, hist_cap);
    return ingest_text(c, units, off, n_texts, false, false, new_chars, new_cap, n_new, id_hist, hist_cap);
}

int bpe_add_text_batch_device(bpe_ctx *c, const uint16_t *d_units, const int64_t *d_off, int64_t n_texts,
                              uint32_t *new_chars, int64_t new_cap, int64_t *n_new, int64_t *id_hist,
                              int64_t hist_cap) {
    if (c && c->multi && n_new)
        return multi_add_text_batch(c->multi, d_units, d_off, n_texts, true, new_chars, new_cap, n_new, id_hist,
                                    hist_cap);
    return ingest_text(c, d_units, d_off, n_texts, true, false, new_chars, new_cap, n_new, id_hist, hist_cap);
}

int bpe_get_ingest_stats(bpe_ctx *c, bpe_ingest_stats *out) {
    if (out) MULTI(get_ingest_stats(c->multi, out));
    if (!c || !out) return fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = c->ing ? c->ing->st : bpe_ingest_stats{};
    return BPE_OK;
}

int bpe_reset_ingest_stats(bpe_ctx *c) {
    MULTI(reset_ingest_stats(c->multi));
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    if (c->ing) c->ing->st = bpe_ingest_stats{};
    return BPE_OK;
}

}  // extern "C"

// ---- corpus from encoded samples / restore (bpe_add_sample_batch, bpe_restore_text_batch,
// include/bpe.h): bpe_append.hip.h's kernel between append_begin and seal_packed --------------------
struct AppendState {
    unsigned long long *d_hist = nullptr, *d_st = nullptr;   // BPE_MAX_VOCAB counts, APP_WORDS status words
    char *d_buf = nullptr;   // grow-only: the host forms' staging, the restore's encoded values and offsets
    size_t buf_bytes = 0;
    int64_t max_wgs = 1024;   // workgroups of the append kernel the device holds at once
    hipEvent_t ev[2] = {nullptr, nullptr};
    bpe_append_stats st{};
};

void append_free(bpe_ctx *c) {
    AppendState *A = c->app;
    if (!A) return;
    dfree(A->d_hist);
    dfree(A->d_st);
    dfree(A->d_buf);
    for (hipEvent_t ev : A->ev)
        if (ev) (void)hipEventDestroy(ev);
    delete A;
    c->app = nullptr;
}

namespace {

static_assert(APP_TILE == BPE_APPEND_TILE, "include/bpe.h append tile");

int append_state(bpe_ctx *c, AppendState **out) {
    if (!c->app) c->app = new AppendState();
    AppendState *A = *out = c->app;
    if (A->d_st) return BPE_OK;
    int rc;
    if ((rc = dev_alloc(&A->d_hist, BPE_MAX_VOCAB))) return rc;
    // one resident round of persistent workgroups: a second, partly filled round would idle CUs
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_smp_append, APP_WG, 0) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && per_cu > 0 &&
        cus > 0)
        A->max_wgs = (int64_t)per_cu * cus;
    for (hipEvent_t &ev : A->ev)
        if (!ev) HIP_TRY(hipEventCreate(&ev));
    if ((rc = dev_alloc(&A->d_st, APP_WORDS))) return rc;   // (last: marks the state complete)
    return BPE_OK;
}

// Room for `bytes` in the scratch buffer (nothing in it is kept between calls).
int append_scratch(bpe_ctx *c, AppendState *A, size_t bytes) {
    if (bytes <= A->buf_bytes) return BPE_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    dfree(A->d_buf);
    A->d_buf = nullptr;
    A->buf_bytes = 0;
    int rc = dev_alloc(&A->d_buf, bytes + bytes / 4);
    if (rc) return rc;
    A->buf_bytes = bytes + bytes / 4;
    return BPE_OK;
}

size_t app_align(size_t n) { return (n + 15) & ~(size_t)15; }

int check_offsets(const int64_t *h_off, int64_t n, const char *what) {
    if (n && h_off[0] < 0) return fail(BPE_ERR_ARG, std::string("bpe native: negative ") + what + " offset");
    for (int64_t k = 0; k < n; ++k)
        if (h_off[k + 1] < h_off[k])
            return fail(BPE_ERR_ARG, std::string("bpe native: ") + what + " offsets must not decrease");
    return BPE_OK;
}

// The append: n samples, sample k = d_vals[h_off[k] .. h_off[k+1]) (device values and offsets; h_off
// the host's checked copy of d_off).  The kernel writes past live_slots before the host knows that
// every id is good, over the sealed tail of the last chunk (which the passes read): a failed call
// does not advance and seals the tail again, so nothing observable has changed.
int append_samples(bpe_ctx *c, AppendState *A, const int32_t *d_vals, const int64_t *d_off, const int64_t *h_off,
                   int64_t n) {
    if (n == 0) return BPE_OK;
    const int64_t base = h_off[0], total = h_off[n] - base, S = total + n;
    hipStream_t s = c->stream;
    int rc;
    if ((rc = append_begin(c, S))) return rc;
    const int64_t nt0 = (int64_t)c->h_len16.size();
    const int dmis = (int)(c->live_slots & 3);
    const int64_t n_tiles = (S + dmis + APP_TILE - 1) / APP_TILE;
    int64_t per_wg = (n_tiles + A->max_wgs - 1) / A->max_wgs;
    if (per_wg > APP_MAX_TILES_PER_WG) per_wg = APP_MAX_TILES_PER_WG;
    const int64_t grid = (n_tiles + per_wg - 1) / per_wg;
    if (grid > 0x7FFFFFFF) return fail(BPE_ERR_ARG, "bpe native: sample batch too large");
    HIP_TRY(hipMemsetAsync(A->d_hist, 0, (size_t)BPE_MAX_VOCAB * 8, s));
    HIP_TRY(hipMemsetAsync(A->d_st, 0, APP_WORDS * 8, s));
    HIP_TRY(hipEventRecord(A->ev[0], s));
    k_smp_append<<<(unsigned)grid, APP_WG, 0, s>>>(d_vals + base, d_off, n, base, total, dmis, n_tiles, per_wg, SEP,
                                                   c->d_ids + c->live_slots, A->d_hist, A->d_st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(A->ev[1], s));
    // one sync: the status words and the counts of the ids the context knows already
    unsigned long long h_st[APP_WORDS] = {0, 0};
    std::vector<unsigned long long> hist((size_t)nt0, 0);
    HIP_TRY(hipMemcpyAsync(h_st, A->d_st, sizeof h_st, hipMemcpyDeviceToHost, s));
    if (nt0) HIP_TRY(hipMemcpyAsync(hist.data(), A->d_hist, (size_t)nt0 * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, A->ev[0], A->ev[1]));
    A->st.kernel_ms += ms;
    const int64_t nt1 = std::max<int64_t>(nt0, (int64_t)h_st[APP_MAX]);
    rc = BPE_OK;
    if (h_st[APP_BAD] || nt1 > BPE_MAX_VOCAB) rc = fail(BPE_ERR_ARG, "bpe native: token id out of range in sample");
    if (!rc && nt1 > nt0) {   // (ids the call registers, as bpe_add_sample does: their counts too)
        hist.resize((size_t)nt1, 0);
        hipError_t e = hipMemcpyAsync(hist.data() + nt0, A->d_hist + nt0, (size_t)(nt1 - nt0) * 8,
                                      hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = fail(BPE_ERR_HIP, std::string("bpe native: append counts: ") + hipGetErrorString(e));
        if (!rc) rc = ensure_vocab(c, nt1);
    }
    if (rc) {
        const std::string msg = g_err;
        const int rc2 = seal_tail(c);
        if (rc2) return rc2;
        HIP_TRY(hipStreamSynchronize(s));
        return fail(rc, msg);
    }
    for (int64_t id = 0; id < nt1; ++id) c->h_count[id] += (int64_t)hist[id];
    c->live_slots += S;
    c->n_samples += n;
    c->n_live += total;
    if ((rc = seal_packed(c))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    A->st.samples += n;
    A->st.tokens += total;
    return BPE_OK;
}

int add_sample_batch(bpe_ctx *c, const int32_t *ids, const int64_t *off, int64_t n, bool dev) {
    if (!c || n < 0 || n >= 0x7FFFFFFF || (n && !off)) return fail(BPE_ERR_ARG, "bpe native: bad add_sample_batch arguments");
    int rc = set_device(c);
    if (rc) return rc;
    AppendState *A;
    if ((rc = append_state(c, &A))) return rc;
    A->st.calls++;
    if (n == 0) return BPE_OK;
    hipStream_t s = c->stream;
    std::vector<int64_t> off_copy;
    const int64_t *h_off = off;
    if (dev) {
        off_copy.resize((size_t)n + 1);
        HIP_TRY(hipMemcpyAsync(off_copy.data(), off, off_copy.size() * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        h_off = off_copy.data();
    }
    if ((rc = check_offsets(h_off, n, "sample"))) return rc;
    const int64_t base = h_off[0], total = h_off[n] - base;
    if (total && !ids) return fail(BPE_ERR_ARG, "bpe native: null id buffer");
    if (dev) return append_samples(c, A, ids, off, h_off, n);
    // the host form: ids and offsets staged, the offsets rebased to the staged ids
    const size_t b_ids = app_align((size_t)total * 4);
    if ((rc = append_scratch(c, A, b_ids + (size_t)(n + 1) * 8))) return rc;
    int32_t *d_ids = reinterpret_cast<int32_t *>(A->d_buf);
    int64_t *d_off = reinterpret_cast<int64_t *>(A->d_buf + b_ids);
    if (total) HIP_TRY(hipMemcpyAsync(d_ids, ids + base, (size_t)total * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_off, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
    // (the kernel subtracts off[0] itself: d_ids - base is never dereferenced below d_ids)
    return append_samples(c, A, d_ids - base, d_off, h_off, n);
}

int restore_text(bpe_ctx *c, bpe_encoder *E, const uint16_t *units, const int64_t *off, int64_t n, bool dev) {
    if (!c || n < 0 || n >= 0x7FFFFFFF || (n && !off))
        return fail(BPE_ERR_ARG, "bpe native: bad restore_text_batch arguments");
    if (!E) return fail(BPE_ERR_ARG, "bpe native: null encoder");
    int enc_device = -1;
    int rc = encoder_device(E, &enc_device);
    if (rc) return rc;
    if (enc_device != c->device) return fail(BPE_ERR_ARG, "bpe native: the encoder is on another device than the context");
    if ((rc = set_device(c))) return rc;
    AppendState *A;
    if ((rc = append_state(c, &A))) return rc;
    A->st.calls++;
    hipStream_t s = c->stream;
    std::vector<int64_t> h_off((size_t)n + 1, 0);
    if (n) {
        if (dev) {
            HIP_TRY(hipMemcpyAsync(h_off.data(), off, h_off.size() * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        } else {
            std::copy(off, off + n + 1, h_off.begin());
        }
    }
    if ((rc = check_offsets(h_off.data(), n, "text"))) return rc;
    const int64_t base = n ? h_off[0] : 0, total = n ? h_off[n] - base : 0;
    if (total && !units) return fail(BPE_ERR_ARG, "bpe native: null unit buffer");
    // scratch: [encoded values: 4 B per unit (a text never grows) | their n + 1 offsets |
    //           the host form's units and offsets]
    const size_t b_vals = app_align((size_t)std::max<int64_t>(total, 1) * 4), b_ooff = app_align((size_t)(n + 1) * 8);
    const size_t b_units = dev ? 0 : app_align((size_t)total * 2), b_uoff = dev ? 0 : (size_t)(n + 1) * 8;
    if ((rc = append_scratch(c, A, b_vals + b_ooff + b_units + b_uoff))) return rc;
    int32_t *d_vals = reinterpret_cast<int32_t *>(A->d_buf);
    int64_t *d_ooff = reinterpret_cast<int64_t *>(A->d_buf + b_vals);
    const uint16_t *d_units = units;
    const int64_t *d_uoff = off;
    if (!dev) {
        uint16_t *su = reinterpret_cast<uint16_t *>(A->d_buf + b_vals + b_ooff);
        int64_t *so = reinterpret_cast<int64_t *>(A->d_buf + b_vals + b_ooff + b_units);
        if (total) HIP_TRY(hipMemcpyAsync(su, units + base, (size_t)total * 2, hipMemcpyHostToDevice, s));
        for (int64_t k = 0; k <= n; ++k) h_off[k] -= base;
        HIP_TRY(hipMemcpyAsync(so, h_off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        d_units = su;
        d_uoff = so;
    }
    // Two streams, no events: the staging above is complete before the encoder starts (this sync),
    // and the encoder's device form synchronises its own stream before it returns, so its values
    // and offsets are complete before the append kernel is enqueued on the context's stream.
    HIP_TRY(hipStreamSynchronize(s));
    int64_t needed = 0;
    if ((rc = bpe_encode_text_batch_device(E, BPE_ENCODE_IDS, d_units, d_uoff, n, d_vals, total, d_ooff, &needed)))
        return rc;   // (the encoder's own code and message)
    if ((rc = set_device(c))) return rc;
    if (n == 0) return BPE_OK;
    std::vector<int64_t> h_ooff((size_t)n + 1);
    HIP_TRY(hipMemcpyAsync(h_ooff.data(), d_ooff, h_ooff.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = check_offsets(h_ooff.data(), n, "sample"))) return rc;
    if (h_ooff[n] - h_ooff[0] != needed || needed > total)
        return fail(BPE_ERR_STATE, "bpe native: the encoder's offsets do not match its value count");
    return append_samples(c, A, d_vals, d_ooff, h_ooff.data(), n);
}

}  // namespace

extern "C" {

int bpe_add_sample_batch(bpe_ctx *c, const int32_t *ids, const int64_t *off, int64_t n) {
    if (n >= 0 && (n == 0 || off)) MULTI(add_sample_batch(c->multi, ids, off, n, false));
    return add_sample_batch(c, ids, off, n, false);
}

int bpe_add_sample_batch_device(bpe_ctx *c, const int32_t *d_ids, const int64_t *d_off, int64_t n) {
    if (n >= 0 && (n == 0 || d_off)) MULTI(add_sample_batch(c->multi, d_ids, d_off, n, true));
    return add_sample_batch(c, d_ids, d_off, n, true);
}

int bpe_restore_text_batch(bpe_ctx *c, bpe_encoder *enc, const uint16_t *units, const int64_t *off, int64_t n_texts) {
    if (enc && n_texts >= 0 && (n_texts == 0 || off)) MULTI(restore_text_batch(c->multi, enc, units, off, n_texts, false));
    return restore_text(c, enc, units, off, n_texts, false);
}

int bpe_restore_text_batch_device(bpe_ctx *c, bpe_encoder *enc, const uint16_t *d_units, const int64_t *d_off,
                                  int64_t n_texts) {
    if (enc && n_texts >= 0 && (n_texts == 0 || d_off))
        MULTI(restore_text_batch(c->multi, enc, d_units, d_off, n_texts, true));
    return restore_text(c, enc, d_units, d_off, n_texts, true);
}

}  // extern "C"

// ---- text as UTF-8 (include/bpe.h): the transcode of bpe_utf8.hip.h, then the UTF-16 device forms ----

namespace {

// the units of a transcode on the host (a multi-device context takes its UTF-16 host forms)
int utf8_units_to_host(hipStream_t s, const uint16_t *d_units, const int64_t *d_uoff, int64_t n, int64_t n_units,
                       std::vector<uint16_t> &units, std::vector<int64_t> &uoff) {
    units.resize((size_t)std::max<int64_t>(n_units, 1));
    uoff.resize((size_t)n + 1);
    if (n_units) HIP_TRY(hipMemcpyAsync(units.data(), d_units, (size_t)n_units * 2, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(uoff.data(), d_uoff, uoff.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return BPE_OK;
}

int add_utf8(bpe_ctx *c, const uint8_t *bytes, const int64_t *off, int64_t n_texts, bool dev, uint32_t *new_chars,
             int64_t new_cap, int64_t *n_new, int64_t *id_hist, int64_t hist_cap) {
    // (the UTF-16 form's own argument check, made before any work here as it is made there)
    if (!c || !n_new || n_texts < 0 || n_texts >= 0x7FFFFFFF || new_cap < 0 || hist_cap < 0 || (n_texts && !off) ||
        (new_cap && !new_chars) || (hist_cap && !id_hist))
        return fail(BPE_ERR_ARG, "bpe native: bad add_text_batch arguments");
    *n_new = 0;
    bpe_ctx *t = c->multi ? multi_first_shard(c->multi) : c;   // the context that transcodes
    int rc = set_device(t);
    if (rc) return rc;
    if (!t->u8) t->u8 = new Utf8State();
    t->u8->st.calls++;
    Utf8Call J;
    J.bytes = bytes, J.off = off, J.n_texts = n_texts, J.dev = dev;
    if ((rc = u8_transcode(*t->u8, t->stream, J))) return rc;
    if (c->multi) {
        std::vector<uint16_t> units;
        std::vector<int64_t> uoff;
        if ((rc = utf8_units_to_host(t->stream, J.d_units, J.d_uoff, n_texts, J.units, units, uoff))) return rc;
        rc = multi_add_text_batch(c->multi, units.data(), uoff.data(), n_texts, false, new_chars, new_cap, n_new,
                                  id_hist, hist_cap);
    } else {
        rc = ingest_text(c, J.d_units, J.d_uoff, n_texts, true, false, new_chars, new_cap, n_new, id_hist, hist_cap);
    }
    if (rc) return rc;
    u8_commit(*t->u8, J);
    return BPE_OK;
}

int restore_utf8(bpe_ctx *c, bpe_encoder *E, const uint8_t *bytes, const int64_t *off, int64_t n, bool dev) {
    // (the UTF-16 form's own checks, made before any work here as they are made there)
    if (!c || n < 0 || n >= 0x7FFFFFFF || (n && !off))
        return fail(BPE_ERR_ARG, "bpe native: bad restore_text_batch arguments");
    if (!E) return fail(BPE_ERR_ARG, "bpe native: null encoder");
    int enc_device = -1;
    int rc = encoder_device(E, &enc_device);
    if (rc) return rc;
    if (!c->multi && enc_device != c->device)
        return fail(BPE_ERR_ARG, "bpe native: the encoder is on another device than the context");
    const uint16_t *d_units = nullptr;
    const int64_t *d_uoff = nullptr;
    int64_t n_units = 0;
    if ((rc = encoder_utf8_units(E, bytes, off, n, dev, &d_units, &d_uoff, &n_units))) return rc;
    if (c->multi) {
        std::vector<uint16_t> units;
        std::vector<int64_t> uoff;
        HIP_TRY(hipSetDevice(enc_device));
        // (the encoder's transcode has synchronised its stream: a plain copy follows it)
        if ((rc = utf8_units_to_host(nullptr, d_units, d_uoff, n, n_units, units, uoff))) return rc;
        rc = multi_restore_text_batch(c->multi, E, units.data(), uoff.data(), n, false);
    } else {
        rc = restore_text(c, E, d_units, d_uoff, n, true);
    }
    if (rc) return rc;
    encoder_utf8_done(E);
    return BPE_OK;
}

}  // namespace

extern "C" {

int bpe_add_utf8_batch(bpe_ctx *c, const uint8_t *bytes, const int64_t *off, int64_t n_texts, uint32_t *new_chars,
                       int64_t new_cap, int64_t *n_new, int64_t *id_hist, int64_t hist_cap) {
    return add_utf8(c, bytes, off, n_texts, false, new_chars, new_cap, n_new, id_hist, hist_cap);
}

int bpe_add_utf8_batch_device(bpe_ctx *c, const uint8_t *d_bytes, const int64_t *d_off, int64_t n_texts,
                              uint32_t *new_chars, int64_t new_cap, int64_t *n_new, int64_t *id_hist,
                              int64_t hist_cap) {
    return add_utf8(c, d_bytes, d_off, n_texts, true, new_chars, new_cap, n_new, id_hist, hist_cap);
}

int bpe_restore_utf8_batch(bpe_ctx *c, bpe_encoder *enc, const uint8_t *bytes, const int64_t *off, int64_t n_texts) {
    return restore_utf8(c, enc, bytes, off, n_texts, false);
}

int bpe_restore_utf8_batch_device(bpe_ctx *c, bpe_encoder *enc, const uint8_t *d_bytes, const int64_t *d_off,
                                  int64_t n_texts) {
    return restore_utf8(c, enc, d_bytes, d_off, n_texts, true);
}

int bpe_get_utf8_stats(bpe_ctx *c, bpe_utf8_stats *out) {
    if (!c || !out) return fail(BPE_ERR_ARG, "bpe native: null argument");
    const bpe_ctx *t = c->multi ? multi_first_shard(c->multi) : c;
    *out = t->u8 ? t->u8->st : bpe_utf8_stats{};
    return BPE_OK;
}

int bpe_reset_utf8_stats(bpe_ctx *c) {
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    bpe_ctx *t = c->multi ? multi_first_shard(c->multi) : c;
    if (t->u8) t->u8->st = bpe_utf8_stats{};
    return BPE_OK;
}

}  // extern "C"

// ---- lines as samples (include/bpe.h): the split of bpe_lines.hip.h, then the UTF-16 device forms ----

namespace {

int add_lines(bpe_ctx *c, int mode, const void *src, const int64_t *off, int64_t n_texts, bool dev, bool utf8,
              uint32_t *new_chars, int64_t new_cap, int64_t *n_new, int64_t *id_hist, int64_t hist_cap) {
    // (the UTF-16 form's own argument check, made before any work here as it is made there)
    if (!c || !n_new || n_texts < 0 || n_texts >= 0x7FFFFFFF || new_cap < 0 || hist_cap < 0 || (n_texts && !off) ||
        (new_cap && !new_chars) || (hist_cap && !id_hist))
        return fail(BPE_ERR_ARG, "bpe native: bad add_text_batch arguments");
    *n_new = 0;
    bpe_ctx *t = c->multi ? multi_first_shard(c->multi) : c;   // the context that splits
    int rc = set_device(t);
    if (rc) return rc;
    if (!t->ln) t->ln = new LinesState();
    t->ln->st.calls++;
    LinesCall J;
    J.mode = mode, J.n_texts = n_texts;
    Utf8Call U;
    if (utf8) {
        if (!t->u8) t->u8 = new Utf8State();
        t->u8->st.calls++;
        U.bytes = static_cast<const uint8_t *>(src), U.off = off, U.n_texts = n_texts, U.dev = dev;
        if ((rc = u8_transcode(*t->u8, t->stream, U))) return rc;
        J.units = U.d_units, J.off = U.d_uoff, J.dev = true;
    } else {
        J.units = static_cast<const uint16_t *>(src), J.off = off, J.dev = dev;
    }
    if ((rc = ln_split(*t->ln, t->stream, J))) return rc;
    if (c->multi) {
        std::vector<uint16_t> units;
        std::vector<int64_t> uoff;
        if ((rc = utf8_units_to_host(t->stream, J.d_out, J.d_ooff, J.samples, J.units_out, units, uoff))) return rc;
        rc = multi_add_text_batch(c->multi, units.data(), uoff.data(), J.samples, false, new_chars, new_cap, n_new,
                                  id_hist, hist_cap);
    } else {
        rc = ingest_text(c, J.d_out, J.d_ooff, J.samples, true, false, new_chars, new_cap, n_new, id_hist, hist_cap);
    }
    if (rc) return rc;
    if (utf8) u8_commit(*t->u8, U);
    ln_commit(*t->ln, J);
    return BPE_OK;
}

int restore_lines(bpe_ctx *c, bpe_encoder *E, int mode, const void *src, const int64_t *off, int64_t n, bool dev,
                  bool utf8) {
    // (the UTF-16 form's own checks, made before any work here as they are made there)
    if (!c || n < 0 || n >= 0x7FFFFFFF || (n && !off))
        return fail(BPE_ERR_ARG, "bpe native: bad restore_text_batch arguments");
    if (!E) return fail(BPE_ERR_ARG, "bpe native: null encoder");
    int enc_device = -1;
    int rc = encoder_device(E, &enc_device);
    if (rc) return rc;
    if (!c->multi && enc_device != c->device)
        return fail(BPE_ERR_ARG, "bpe native: the encoder is on another device than the context");
    const uint16_t *d_units = nullptr;
    const int64_t *d_uoff = nullptr;
    int64_t n_samples = 0, n_units = 0;
    if ((rc = encoder_lines_units(E, mode, src, off, n, dev, utf8, &d_units, &d_uoff, &n_samples, &n_units))) return rc;
    if (c->multi) {
        std::vector<uint16_t> units;
        std::vector<int64_t> uoff;
        HIP_TRY(hipSetDevice(enc_device));
        // (the encoder's split has synchronised its stream: a plain copy follows it)
        if ((rc = utf8_units_to_host(nullptr, d_units, d_uoff, n_samples, n_units, units, uoff))) return rc;
        rc = multi_restore_text_batch(c->multi, E, units.data(), uoff.data(), n_samples, false);
    } else {
        rc = restore_text(c, E, d_units, d_uoff, n_samples, true);
    }
    if (rc) return rc;
    encoder_lines_done(E);
    return BPE_OK;
}

}  // namespace

extern "C" {

int bpe_add_lines_batch(bpe_ctx *c, int mode, const uint16_t *units, const int64_t *off, int64_t n_texts,
                        uint32_t *new_chars, int64_t new_cap, int64_t *n_new, int64_t *id_hist, int64_t hist_cap) {
    return add_lines(c, mode, units, off, n_texts, false, false, new_chars, new_cap, n_new, id_hist, hist_cap);
}

int bpe_add_lines_batch_device(bpe_ctx *c, int mode, const uint16_t *d_units, const int64_t *d_off, int64_t n_texts,
                               uint32_t *new_chars, int64_t new_cap, int64_t *n_new, int64_t *id_hist,
                               int64_t hist_cap) {
    return add_lines(c, mode, d_units, d_off, n_texts, true, false, new_chars, new_cap, n_new, id_hist, hist_cap);
}

int bpe_add_lines_utf8_batch(bpe_ctx *c, int mode, const uint8_t *bytes, const int64_t *off, int64_t n_texts,
                             uint32_t *new_chars, int64_t new_cap, int64_t *n_new, int64_t *id_hist,
                             int64_t hist_cap) {
    return add_lines(c, mode, bytes, off, n_texts, false, true, new_chars, new_cap, n_new, id_hist, hist_cap);
}

int bpe_add_lines_utf8_batch_device(bpe_ctx *c, int mode, const uint8_t *d_bytes, const int64_t *d_off,
                                    int64_t n_texts, uint32_t *new_chars, int64_t new_cap, int64_t *n_new,
                                    int64_t *id_hist, int64_t hist_cap) {
    return add_lines(c, mode, d_bytes, d_off, n_texts, true, true, new_chars, new_cap, n_new, id_hist, hist_cap);
}

int bpe_restore_lines_batch(bpe_ctx *c, bpe_encoder *enc, int mode, const uint16_t *units, const int64_t *off,
                            int64_t n_texts) {
    return restore_lines(c, enc, mode, units, off, n_texts, false, false);
}

int bpe_restore_lines_batch_device(bpe_ctx *c, bpe_encoder *enc, int mode, const uint16_t *d_units,
                                   const int64_t *d_off, int64_t n_texts) {
    return restore_lines(c, enc, mode, d_units, d_off, n_texts, true, false);
}

int bpe_restore_lines_utf8_batch(bpe_ctx *c, bpe_encoder *enc, int mode, const uint8_t *bytes, const int64_t *off,
                                 int64_t n_texts) {
    return restore_lines(c, enc, mode, bytes, off, n_texts, false, true);
}

int bpe_restore_lines_utf8_batch_device(bpe_ctx *c, bpe_encoder *enc, int mode, const uint8_t *d_bytes,
                                        const int64_t *d_off, int64_t n_texts) {
    return restore_lines(c, enc, mode, d_bytes, d_off, n_texts, true, true);
}

int bpe_get_lines_stats(bpe_ctx *c, bpe_lines_stats *out) {
    if (!c || !out) return fail(BPE_ERR_ARG, "bpe native: null argument");
    const bpe_ctx *t = c->multi ? multi_first_shard(c->multi) : c;
    *out = t->ln ? t->ln->st : bpe_lines_stats{};
    return BPE_OK;
}

int bpe_reset_lines_stats(bpe_ctx *c) {
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    bpe_ctx *t = c->multi ? multi_first_shard(c->multi) : c;
    if (t->ln) t->ln->st = bpe_lines_stats{};
    return BPE_OK;
}

}  // extern "C"

extern "C" {

int bpe_token_counts(bpe_ctx *c, int64_t *counts, int64_t cap) {
    if (counts && cap >= 0) MULTI(token_counts(c->multi, counts, cap));
    if (!c || cap < 0 || (cap && !counts)) return fail(BPE_ERR_ARG, "bpe native: bad token_counts arguments");
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = settle(c))) return rc;
    const int64_t nt = (int64_t)c->h_count.size();
    if (cap < nt) return fail(BPE_ERR_ARG, "bpe native: token_counts buffer below the token count");
    std::copy(c->h_count.begin(), c->h_count.end(), counts);
    return BPE_OK;
}

int bpe_get_append_stats(bpe_ctx *c, bpe_append_stats *out) {
    if (out) MULTI(get_append_stats(c->multi, out));
    if (!c || !out) return fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = c->app ? c->app->st : bpe_append_stats{};
    return BPE_OK;
}

int bpe_reset_append_stats(bpe_ctx *c) {
    MULTI(reset_append_stats(c->multi));
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    if (c->app) c->app->st = bpe_append_stats{};
    return BPE_OK;
}

}  // extern "C"

// ---- corpus out (bpe_export_samples, bpe_export_text_batch, include/bpe.h): bpe_export.hip.h's
// kernels after k_census and k_scan_pair; nothing here writes the corpus or any state of the passes --
struct ExportState {
    char *d_buf = nullptr;    // grow-only: region prefixes, sample index, chunk prefixes, plan, vector index
    size_t buf_bytes = 0;
    char *d_vals = nullptr;   // grow-only: the host forms' values; the text export's ids, offsets and units
    size_t vals_bytes = 0;
    unsigned long long *d_st = nullptr;   // EXP_CHECK's first failing value
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // the index / check span, the emit span
    bpe_export_stats st{};
    // the call in flight, between export_prepare and export_emit (pointers into d_buf)
    bool all = false, le_done = false, emit_timed = false;
    int64_t n = 0, needed = 0, n_items = 0;
    int64_t *d_live = nullptr, *d_seps = nullptr, *d_le = nullptr, *d_se = nullptr, *d_cpre = nullptr;
    int64_t *d_idx = nullptr, *d_soff = nullptr, *d_ipre = nullptr;
    int32_t *d_map = nullptr;
    int32_t n_index = 0;
    const int64_t *d_off = nullptr;   // the call's n + 1 offsets
};

void export_free(bpe_ctx *c) {
    ExportState *X = c->exp;
    if (!X) return;
    dfree(X->d_buf);
    dfree(X->d_vals);
    dfree(X->d_st);
    for (hipEvent_t ev : X->ev)
        if (ev) (void)hipEventDestroy(ev);
    delete X;
    c->exp = nullptr;
}

namespace {

static_assert(EXP_TILE == BPE_EXPORT_TILE && BPE_EXPORT_SCAN_THREADS == 1024, "include/bpe.h export constants");

int export_state(bpe_ctx *c, ExportState **out) {
    if (!c->exp) c->exp = new ExportState();
    ExportState *X = *out = c->exp;
    if (X->d_st) return BPE_OK;
    for (hipEvent_t &ev : X->ev)
        if (!ev) HIP_TRY(hipEventCreate(&ev));
    return dev_alloc(&X->d_st, 1);   // (last: marks the state complete)
}

// Room for `bytes` in one of the scratch buffers (nothing in them is kept between calls).
int export_grow(bpe_ctx *c, char **buf, size_t *have, size_t bytes) {
    if (bytes <= *have) return BPE_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    dfree(*buf);
    *buf = nullptr;
    *have = 0;
    int rc = dev_alloc(buf, bytes + bytes / 4);
    if (rc) return rc;
    *have = bytes + bytes / 4;
    return BPE_OK;
}

// Every way out of an export call waits for the copies it enqueued from and to the caller's buffers.
struct ExportSync {
    hipStream_t s;
    ~ExportSync() { (void)hipStreamSynchronize(s); }
};

template <int KIND>
void export_walk(bpe_ctx *c, ExportState *X, void *d_out, int64_t *off, int64_t *se, int64_t *cpre) {
    k_exp_walk<KIND><<<(c->R + EXP_WAVES - 1) / EXP_WAVES, EXP_WG, 0, c->stream>>>(
        c->d_ids, c->n_chunks, c->cpr, c->R, X->d_live, X->d_seps, c->n_samples, c->n_live, X->d_map, X->n_index,
        d_out, off, se, cpre, X->d_st);
}

template <int KIND>
void export_sel(bpe_ctx *c, ExportState *X, void *d_out) {
    const int64_t grid = std::min<int64_t>((X->n_items + EXP_WAVES - 1) / EXP_WAVES, 1 << 16);
    k_exp_sel<KIND><<<(unsigned)grid, EXP_WG, 0, c->stream>>>(c->d_ids, X->d_idx, X->n, X->d_le, X->d_se, X->d_cpre,
                                                              X->d_soff, X->d_ipre, X->n_items, X->d_map, X->n_index,
                                                              d_out, X->d_st);
}

// The values (kind: BPE_EXPORT_*, or EXP_NONE for the offsets alone) of the prepared call into d_out;
// X->d_off holds the call's offsets afterwards.
int export_emit(bpe_ctx *c, ExportState *X, int kind, void *d_out) {
    hipStream_t s = c->stream;
    X->emit_timed = false;
    if (X->all ? (kind == EXP_NONE && X->le_done) : (kind == EXP_NONE || X->n_items == 0)) return BPE_OK;
    HIP_TRY(hipEventRecord(X->ev[2], s));
    if (X->all) {
        if (kind == EXP_IDS) export_walk<EXP_IDS>(c, X, d_out, X->d_le, nullptr, nullptr);
        else if (kind == EXP_VEC) export_walk<EXP_VEC>(c, X, d_out, X->d_le, nullptr, nullptr);
        else if (kind == EXP_CODE) export_walk<EXP_CODE>(c, X, d_out, X->d_le, nullptr, nullptr);
        else export_walk<EXP_NONE>(c, X, nullptr, X->d_le, nullptr, nullptr);
        X->le_done = true;
    } else {
        if (kind == EXP_IDS) export_sel<EXP_IDS>(c, X, d_out);
        else if (kind == EXP_VEC) export_sel<EXP_VEC>(c, X, d_out);
        else export_sel<EXP_CODE>(c, X, d_out);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(X->ev[3], s));
    X->emit_timed = true;
    return BPE_OK;
}

// The kernels' time of a call, after its last sync.
int export_timing(ExportState *X) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, X->ev[0], X->ev[1]));
    X->st.kernel_ms += ms;
    if (X->emit_timed) {
        HIP_TRY(hipEventElapsedTime(&ms, X->ev[2], X->ev[3]));
        X->st.kernel_ms += ms;
    }
    return BPE_OK;
}

size_t exp_align(size_t n) { return (n + 15) & ~(size_t)15; }

// Everything of a call before its values: the arguments, the region prefixes, for the selected
// form the sample index, the chunk prefixes and the plan (the call's offsets and wave items), and
// the hole check of the vectors where the host's counts cannot rule a hole out.  Sets X->needed.
int export_prepare(bpe_ctx *c, ExportState *X, int kind, const int64_t *idx, int64_t n, const int32_t *tvi,
                   int32_t n_index) {
    if (kind != EXP_IDS && kind != EXP_VEC && kind != EXP_CODE) return fail(BPE_ERR_ARG, "bpe native: unknown export kind");
    if (n < 0 || n >= 0x7FFFFFFE) return fail(BPE_ERR_ARG, "bpe native: bad export arguments");
    if (kind == EXP_VEC && !tvi) return fail(BPE_ERR_STATE, "bpe native: no vector index (compactVectorIndex first)");
    if (kind == EXP_VEC && n_index < 0) return fail(BPE_ERR_ARG, "bpe native: bad export arguments");
    int rc;
    if ((rc = settle(c))) return rc;
    const int64_t ns = c->n_samples;
    if (!idx && n != ns)
        return fail(BPE_ERR_ARG, "bpe native: an export of every sample (idx NULL) takes n = the sample count");
    for (int64_t k = 0; idx && k < n; ++k)
        if (idx[k] < 0 || idx[k] >= ns) return fail(BPE_ERR_ARG, "bpe native: sample index out of range");
    hipStream_t s = c->stream;
    const bool all = !idx, vec = kind == EXP_VEC;
    X->all = all;
    X->le_done = false;
    X->n = n;
    X->n_items = 0;
    X->n_index = vec ? n_index : 0;
    // the engine's per-token counts are exact: a hole no present id maps to cannot be met
    bool check = false;
    for (size_t id = 0; vec && id < c->h_count.size() && !check; ++id)
        check = c->h_count[id] > 0 && ((int64_t)id >= n_index || tvi[id] < 0);
    geometry(c);
    const size_t b_reg = exp_align((size_t)c->R * 8), b_le = exp_align((size_t)(ns + 1) * 8);
    const size_t b_se = all ? 0 : exp_align((size_t)std::max<int64_t>(ns, 1) * 8);
    const size_t b_cpre = all ? 0 : exp_align((size_t)std::max<int64_t>(c->n_chunks, 1) * 8);
    const size_t b_n = all ? 0 : exp_align((size_t)(n + 1) * 8);
    const size_t b_map = vec ? exp_align((size_t)std::max<int32_t>(n_index, 1) * 4) : 0;
    if ((rc = export_grow(c, &X->d_buf, &X->buf_bytes, 2 * b_reg + b_le + b_se + b_cpre + 3 * b_n + b_map))) return rc;
    char *p = X->d_buf;
    auto take = [&p](size_t bytes) {
        char *q = p;
        p += bytes;
        return q;
    };
    X->d_live = reinterpret_cast<int64_t *>(take(b_reg));
    X->d_seps = reinterpret_cast<int64_t *>(take(b_reg));
    X->d_le = reinterpret_cast<int64_t *>(take(b_le));
    X->d_se = reinterpret_cast<int64_t *>(take(b_se));
    X->d_cpre = reinterpret_cast<int64_t *>(take(b_cpre));
    X->d_idx = reinterpret_cast<int64_t *>(take(b_n));
    X->d_soff = reinterpret_cast<int64_t *>(take(b_n));
    X->d_ipre = reinterpret_cast<int64_t *>(take(b_n));
    X->d_map = vec ? reinterpret_cast<int32_t *>(take(b_map)) : nullptr;
    X->d_off = all ? X->d_le : X->d_soff;
    if (vec && n_index) HIP_TRY(hipMemcpyAsync(X->d_map, tvi, (size_t)n_index * 4, hipMemcpyHostToDevice, s));
    if (!all && n) HIP_TRY(hipMemcpyAsync(X->d_idx, idx, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(X->d_le, 0, 8, s));
    HIP_TRY(hipMemsetAsync(X->d_st, 0xFF, 8, s));
    HIP_TRY(hipEventRecord(X->ev[0], s));
    const bool empty = !all && n == 0;   // (nothing selected: off[0] = 0 is the whole answer)
    if (empty) HIP_TRY(hipMemsetAsync(X->d_soff, 0, 8, s));
    if (!empty) {
        k_census<<<(c->R + 3) / 4, 256, 0, s>>>(c->d_ids, c->n_chunks, c->cpr, c->R, X->d_live, X->d_seps);
        k_scan_pair<<<1, 1024, 0, s>>>(c->R, X->d_live, X->d_seps);
    }
    X->needed = all ? c->n_live : 0;
    if (!all && n) {
        export_walk<EXP_NONE>(c, X, nullptr, X->d_le, X->d_se, X->d_cpre);
        k_exp_plan<<<(unsigned)((n + 1 + 255) / 256), 256, 0, s>>>(X->d_idx, n, X->d_le, X->d_se, X->d_soff, X->d_ipre);
        k_scan_pair<<<1, 1024, 0, s>>>((int)(n + 1), X->d_soff, X->d_ipre);
        HIP_TRY(hipGetLastError());
        int64_t tot[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(&tot[0], X->d_soff + n, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&tot[1], X->d_ipre + n, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        X->needed = tot[0];
        X->n_items = tot[1];
    }
    if (check && !empty) {
        if (all) {
            export_walk<EXP_CHECK>(c, X, nullptr, X->d_le, nullptr, nullptr);
            X->le_done = true;
        } else if (X->n_items) {
            export_sel<EXP_CHECK>(c, X, nullptr);
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(X->ev[1], s));
    if (check && !empty) {
        unsigned long long key = ~0ull;
        HIP_TRY(hipMemcpyAsync(&key, X->d_st, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (key != ~0ull) {
            const int64_t pos = (int64_t)(key >> 16);
            std::vector<int64_t> off((size_t)n + 1);
            HIP_TRY(hipMemcpyAsync(off.data(), X->d_off, off.size() * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            const int64_t k = (int64_t)(std::upper_bound(off.begin(), off.end(), pos) - off.begin()) - 1;
            char msg[128];
            std::snprintf(msg, sizeof msg, "unknown token index: %lld (sample %lld, position %lld)",
                          (long long)(key & 0xFFFF), (long long)k, (long long)(pos - off[(size_t)std::max<int64_t>(k, 0)]));
            return fail(BPE_ERR_VOCAB, msg);
        }
    }
    return BPE_OK;
}

int export_samples(bpe_ctx *c, int kind, const int64_t *idx, int64_t n, const int32_t *tvi, int32_t n_index,
                   void *out, int64_t cap, int64_t *off_out, int64_t *needed_out, bool dev) {
    if (!c || cap < 0 || !off_out || (cap && !out) || (dev && !needed_out))
        return fail(BPE_ERR_ARG, "bpe native: bad export_samples arguments");
    const size_t esize = kind == EXP_CODE ? 2 : 4;
    if (dev && (((uintptr_t)out & (esize - 1)) || ((uintptr_t)off_out & 7)))
        return fail(BPE_ERR_ARG, "bpe native: misaligned export buffer");
    int rc = set_device(c);
    if (rc) return rc;
    ExportState *X;
    if ((rc = export_state(c, &X))) return rc;
    X->st.calls++;
    hipStream_t s = c->stream;
    ExportSync guard{s};
    if ((rc = export_prepare(c, X, kind, idx, n, tvi, n_index))) return rc;
    const int64_t needed = X->needed;
    const bool fits = needed <= cap;
    void *d_out = out;
    if (!dev && fits && needed) {
        if ((rc = export_grow(c, &X->d_vals, &X->vals_bytes, (size_t)needed * esize))) return rc;
        d_out = X->d_vals;
    }
    if ((rc = export_emit(c, X, fits ? kind : EXP_NONE, d_out))) return rc;
    HIP_TRY(hipMemcpyAsync(off_out, X->d_off, (size_t)(n + 1) * 8, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (!dev && fits && needed)
        HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)needed * esize, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = export_timing(X))) return rc;
    if (needed_out) *needed_out = needed;
    if (!fits) {
        char msg[128];
        std::snprintf(msg, sizeof msg, "bpe native: export needs %lld values, the buffer holds %lld",
                      (long long)needed, (long long)cap);
        return fail(BPE_ERR_ARG, msg);
    }
    X->st.samples += n;
    X->st.values += needed;
    return BPE_OK;
}

// (utf8: bytes through bpe_decode_utf8_batch_device instead of units; `units` and cap count bytes then)
int export_text(bpe_ctx *c, bpe_decoder *D, const int64_t *idx, int64_t n, void *units, int64_t cap,
                int64_t *off_out, int64_t *needed_out, bool dev, bool utf8 = false) {
    if (!c || cap < 0 || !off_out || (cap && !units) || (dev && !needed_out))
        return fail(BPE_ERR_ARG, utf8 ? "bpe native: bad export_utf8_batch arguments"
                                      : "bpe native: bad export_text_batch arguments");
    const size_t esize = utf8 ? 1 : 2;
    if (!D) return fail(BPE_ERR_ARG, "bpe native: null decoder");
    int dec_device = -1;
    int rc = decoder_device(D, &dec_device);
    if (rc) return rc;
    if (dec_device != c->device) return fail(BPE_ERR_ARG, "bpe native: the decoder is on another device than the context");
    if ((rc = set_device(c))) return rc;
    ExportState *X;
    if ((rc = export_state(c, &X))) return rc;
    X->st.calls++;
    hipStream_t s = c->stream;
    ExportSync guard{s};
    if ((rc = export_prepare(c, X, EXP_IDS, idx, n, nullptr, 0))) return rc;
    const int64_t n_ids = X->needed;
    // scratch: [ids: 4 B per token | the host form's n + 1 unit offsets and units_cap units]
    const size_t b_ids = exp_align((size_t)std::max<int64_t>(n_ids, 1) * 4), b_ooff = dev ? 0 : exp_align((size_t)(n + 1) * 8);
    if ((rc = export_grow(c, &X->d_vals, &X->vals_bytes, b_ids + b_ooff + (dev ? 0 : (size_t)cap * esize)))) return rc;
    int32_t *d_ids = reinterpret_cast<int32_t *>(X->d_vals);
    int64_t *d_ooff = dev ? off_out : reinterpret_cast<int64_t *>(X->d_vals + b_ids);
    void *d_units = dev ? units : (cap ? static_cast<void *>(X->d_vals + b_ids + b_ooff) : nullptr);
    if ((rc = export_emit(c, X, EXP_IDS, d_ids))) return rc;
    // Two streams, no events: the ids and their offsets are complete before the decoder starts (this
    // sync), and the decoder's device form synchronises its own stream before it returns.
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = export_timing(X))) return rc;
    int64_t dneed = -1;   // (set by the decoder once its offsets are written)
    const int drc = utf8 ? bpe_decode_utf8_batch_device(D, BPE_DECODE_IDS, d_ids, X->d_off, n,
                                                        static_cast<uint8_t *>(d_units), cap, d_ooff, &dneed)
                         : bpe_decode_batch_device(D, BPE_DECODE_IDS, d_ids, X->d_off, n,
                                                   static_cast<uint16_t *>(d_units), cap, d_ooff, &dneed);
    const std::string dmsg = g_err;
    if ((rc = set_device(c))) return rc;
    if (!dev && dneed >= 0) {
        HIP_TRY(hipMemcpyAsync(off_out, d_ooff, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s));
        if (drc == BPE_OK && dneed)
            HIP_TRY(hipMemcpyAsync(units, d_units, (size_t)dneed * esize, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (needed_out && dneed >= 0) *needed_out = dneed;
    if (drc) return drc < 0 ? fail(drc, dmsg) : drc;   // (the decoder's own code and message)
    X->st.samples += n;
    X->st.values += n_ids;
    return BPE_OK;
}

// ---- skip-gram pairs of corpus samples (bpe_export_skipgram, include/bpe.h): the export above into
// scratch, then bpe_skipgram.hip.h's expansion on the context's stream ---------------------------------
int skipgram_state(bpe_ctx *c, SgState **out) {
    if (!c->sg) c->sg = new SgState();
    *out = c->sg;
    return BPE_OK;
}

int skipgram_kind(int kind) {
    if (kind == EXP_IDS || kind == EXP_VEC) return BPE_OK;
    return fail(BPE_ERR_ARG, "bpe native: a skip-gram export takes BPE_EXPORT_IDS or BPE_EXPORT_VECTORS");
}

int export_skipgram(bpe_ctx *c, int kind, const int64_t *idx, int64_t n, const int32_t *tvi, int32_t n_index,
                    int window, int32_t *targets, int32_t *contexts, int64_t cap, int64_t *pair_off,
                    int64_t *needed_out, bool dev) {
    if (!c || cap < 0 || !pair_off || (cap && (!targets || !contexts)) || (dev && !needed_out))
        return fail(BPE_ERR_ARG, "bpe native: bad export_skipgram arguments");
    int rc = set_device(c);
    if (rc) return rc;
    SgState *S;
    if ((rc = skipgram_state(c, &S))) return rc;
    S->st.calls++;
    if ((rc = sg_check_window(window)) || (rc = skipgram_kind(kind))) return rc;
    ExportState *X;
    if ((rc = export_state(c, &X))) return rc;
    X->st.calls++;
    hipStream_t s = c->stream;
    ExportSync guard{s};
    if ((rc = export_prepare(c, X, kind, idx, n, tvi, n_index))) return rc;
    const int64_t n_vals = X->needed;
    if ((rc = export_grow(c, &X->d_vals, &X->vals_bytes, exp_align((size_t)std::max<int64_t>(n_vals, 1) * 4)))) return rc;
    if ((rc = export_emit(c, X, kind, X->d_vals))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = export_timing(X))) return rc;
    X->st.samples += n;
    X->st.values += n_vals;
    SgCall J;
    J.d_vals = reinterpret_cast<const int32_t *>(X->d_vals), J.d_off = X->d_off, J.n_texts = n, J.window = window;
    if (!dev) return sg_host_form(*S, s, J, targets, contexts, cap, pair_off);
    J.d_t = cap ? targets : nullptr, J.d_c = cap ? contexts : nullptr, J.d_poff = pair_off, J.cap = cap;
    return sg_device_form(*S, s, J, needed_out);
}

// A multi-device context: the samples through its host export, shard by shard, and the expansion of
// the assembled batch on its first shard's device.
int multi_skipgram(bpe_ctx *c, int kind, const int64_t *idx, int64_t n, const int32_t *tvi, int32_t n_index,
                   int window, int32_t *targets, int32_t *contexts, int64_t cap, int64_t *pair_off) {
    bpe_ctx *t = multi_first_shard(c->multi);
    int rc = set_device(t);
    if (rc) return rc;
    SgState *S;
    if ((rc = skipgram_state(t, &S))) return rc;
    S->st.calls++;
    if ((rc = sg_check_window(window)) || (rc = skipgram_kind(kind))) return rc;
    std::vector<int64_t> off;
    std::vector<int32_t> vals;
    if ((rc = multi_export_values(c->multi, kind, idx, n, tvi, n_index, vals, off))) return rc;
    if ((rc = set_device(t))) return rc;
    SgCall J;
    J.window = window;
    if ((rc = sg_stage_host(*S, t->stream, vals.data(), off.data(), n, J))) return rc;
    return sg_host_form(*S, t->stream, J, targets, contexts, cap, pair_off);
}

}  // namespace

extern "C" {

int bpe_export_samples(bpe_ctx *c, int kind, const int64_t *idx, int64_t n, const int32_t *to_vector_index,
                       int32_t n_index, void *vals_out, int64_t vals_cap, int64_t *out_off) {
    if (n >= 0 && vals_cap >= 0 && out_off && (!vals_cap || vals_out))
        MULTI(export_samples(c->multi, kind, idx, n, to_vector_index, n_index, vals_out, vals_cap, out_off));
    return export_samples(c, kind, idx, n, to_vector_index, n_index, vals_out, vals_cap, out_off, nullptr, false);
}

int bpe_export_samples_device(bpe_ctx *c, int kind, const int64_t *idx, int64_t n, const int32_t *to_vector_index,
                              int32_t n_index, void *d_vals_out, int64_t vals_cap, int64_t *d_out_off,
                              int64_t *needed) {
    if (c && c->multi)
        return fail(BPE_ERR_ARG, "bpe native: the device form of an export on a multi-device context "
                                 "(its shards sit on different devices: take the host form)");
    return export_samples(c, kind, idx, n, to_vector_index, n_index, d_vals_out, vals_cap, d_out_off, needed, true);
}

int bpe_export_text_batch(bpe_ctx *c, bpe_decoder *dec, const int64_t *idx, int64_t n, uint16_t *units_out,
                          int64_t units_cap, int64_t *out_off) {
    if (dec && n >= 0 && units_cap >= 0 && out_off && (!units_cap || units_out))
        MULTI(export_text_batch(c->multi, dec, idx, n, units_out, units_cap, out_off));
    return export_text(c, dec, idx, n, units_out, units_cap, out_off, nullptr, false);
}

int bpe_export_text_batch_device(bpe_ctx *c, bpe_decoder *dec, const int64_t *idx, int64_t n, uint16_t *d_units_out,
                                 int64_t units_cap, int64_t *d_out_off, int64_t *needed) {
    if (c && c->multi)
        return fail(BPE_ERR_ARG, "bpe native: the device form of an export on a multi-device context "
                                 "(its shards sit on different devices: take the host form)");
    return export_text(c, dec, idx, n, d_units_out, units_cap, d_out_off, needed, true);
}

int bpe_export_utf8_batch(bpe_ctx *c, bpe_decoder *dec, const int64_t *idx, int64_t n, uint8_t *bytes_out,
                          int64_t bytes_cap, int64_t *out_off) {
    if (dec && n >= 0 && bytes_cap >= 0 && out_off && (!bytes_cap || bytes_out))
        MULTI(export_utf8_batch(c->multi, dec, idx, n, bytes_out, bytes_cap, out_off));
    return export_text(c, dec, idx, n, bytes_out, bytes_cap, out_off, nullptr, false, true);
}

int bpe_export_utf8_batch_device(bpe_ctx *c, bpe_decoder *dec, const int64_t *idx, int64_t n, uint8_t *d_bytes_out,
                                 int64_t bytes_cap, int64_t *d_out_off, int64_t *needed) {
    if (c && c->multi)
        return fail(BPE_ERR_ARG, "bpe native: the device form of an export on a multi-device context "
                                 "(its shards sit on different devices: take the host form)");
    return export_text(c, dec, idx, n, d_bytes_out, bytes_cap, d_out_off, needed, true, true);
}

int bpe_get_export_stats(bpe_ctx *c, bpe_export_stats *out) {
    if (out) MULTI(get_export_stats(c->multi, out));
    if (!c || !out) return fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = c->exp ? c->exp->st : bpe_export_stats{};
    return BPE_OK;
}

int bpe_reset_export_stats(bpe_ctx *c) {
    MULTI(reset_export_stats(c->multi));
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    if (c->exp) c->exp->st = bpe_export_stats{};
    return BPE_OK;
}

int bpe_export_skipgram(bpe_ctx *c, int kind, const int64_t *idx, int64_t n, const int32_t *to_vector_index,
                        int32_t n_index, int window, int32_t *targets, int32_t *contexts, int64_t pairs_cap,
                        int64_t *pair_off) {
    if (c && c->multi && n >= 0 && pairs_cap >= 0 && pair_off && (!pairs_cap || (targets && contexts)))
        return multi_skipgram(c, kind, idx, n, to_vector_index, n_index, window, targets, contexts, pairs_cap, pair_off);
    return export_skipgram(c, kind, idx, n, to_vector_index, n_index, window, targets, contexts, pairs_cap, pair_off,
                           nullptr, false);
}

int bpe_export_skipgram_device(bpe_ctx *c, int kind, const int64_t *idx, int64_t n, const int32_t *to_vector_index,
                               int32_t n_index, int window, int32_t *d_targets, int32_t *d_contexts,
                               int64_t pairs_cap, int64_t *d_pair_off, int64_t *needed) {
    if (c && c->multi)
        return fail(BPE_ERR_ARG, "bpe native: the device form of an export on a multi-device context "
                                 "(its shards sit on different devices: take the host form)");
    return export_skipgram(c, kind, idx, n, to_vector_index, n_index, window, d_targets, d_contexts, pairs_cap,
                           d_pair_off, needed, true);
}

int bpe_get_skipgram_stats(bpe_ctx *c, bpe_skipgram_stats *out) {
    if (!c || !out) return fail(BPE_ERR_ARG, "bpe native: null argument");
    const bpe_ctx *t = c->multi ? multi_first_shard(c->multi) : c;
    *out = t->sg ? t->sg->st : bpe_skipgram_stats{};
    return BPE_OK;
}

int bpe_reset_skipgram_stats(bpe_ctx *c) {
    if (!c) return fail(BPE_ERR_ARG, "bpe native: null context");
    bpe_ctx *t = c->multi ? multi_first_shard(c->multi) : c;
    if (t->sg) t->sg->st = bpe_skipgram_stats{};
    return BPE_OK;
}

}  // extern "C"
