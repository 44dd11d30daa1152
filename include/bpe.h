/*
 * bpe.h — C ABI of libbpe: the MI355X (gfx950) engine for the BPE merge-training hot path of
 * beenotung/bpe-tokenizer (reference: /root/reference/core.ts, v2.2.0).
 *
 * The reference has no FFI layer: its drop-in boundary is the public `BPETokenizer` class
 * (core.ts:77).  These entry points are exactly what that class's corpus-touching methods need;
 * the host side (bpe-tokenizer_amd/js/core.js over the N-API addon, or any ctypes/cgo binding —
 * see INTEGRATION.md) keeps the token table, codes, JSON and encode/decode bookkeeping and calls
 * down here for every pass over the corpus.
 *
 * Conventions
 *   - Every function returns an int status: BPE_OK (0), BPE_NO_MERGE (1, "findNextMerge returned
 *     null"), or a negative error code; bpe_last_error() returns the message of the last error
 *     raised on the calling thread.
 *   - Token ids are the reference's `token.index` (code point of `token.code` minus one,
 *     core.ts:149,189,316,485).  Ids must stay below BPE_MAX_VOCAB (55 296): above it the
 *     reference's codes become lone UTF-16 surrogates (hard part 8).
 *   - Caller-owned host buffers are copied in/out; the library never retains host pointers.
 *   - A context owns one HIP device, one stream and all device memory of one corpus shard.
 *   - There is no CPU fallback: without a usable HIP device bpe_create() fails with BPE_ERR_HIP.
 */
#ifndef BPE_H
#define BPE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BPE_OK 0
#define BPE_NO_MERGE 1
#define BPE_ERR_ARG (-1)
#define BPE_ERR_HIP (-2)
#define BPE_ERR_OOM (-3)
#define BPE_ERR_STATE (-4)
#define BPE_ERR_VOCAB (-5)
/* The incremental mode's position index does not fit beside this shard's corpus in device memory
 * (bpe_set_global_counts on a shard in BPE_MODE_INCREMENTAL).  Nothing was changed: the streaming
 * mode, which needs no index, can go on.  Drivers fall back to it on this code only. */
#define BPE_ERR_NOFIT (-6)

#define BPE_MAX_VOCAB 55296

typedef struct bpe_ctx bpe_ctx;

/* Library version (major*10000 + minor*100 + patch). */
int bpe_version(void);

/* Copies the last error message of this thread (NUL-terminated, truncated to cap). */
int bpe_last_error(char *buf, size_t cap);

/* Number of visible HIP devices (0 when none). */
int bpe_device_count(int *n);

/* `new BPETokenizer()` (core.ts:77-106): an empty corpus shard on HIP device `device`. */
int bpe_create(bpe_ctx **out, int device);
int bpe_destroy(bpe_ctx *ctx);

/* One corpus sharded over n_shards HIP devices behind one context (the drop-in's BPE_NUM_GPUS;
 * SURVEY.md §5, §8(e)).  devices: n_shards device indices (NULL: 0 .. n_shards-1).  Every entry
 * point below works on it as on a single-device context, with identical results: the shards hold
 * contiguous runs of whole samples (pairs never cross samples, core.ts:265-267), samples added
 * before the first pass are cut into runs of about equal size, later ones go to the last shard.
 * Per merge iteration the shards all-reduce their pair tables and tie positions:
 *   BPE_REDUCE_RCCL — RCCL communicators over the devices (ncclCommInitAll, grouped calls on the
 *                     shards' streams; one shard per device);
 *   BPE_REDUCE_HOST — host copies (any placement, e.g. several shards on one device: tests).
 * The per-shard entry points (bpe_export_counts ... bpe_rank_loop_*, bpe_recount) refuse a
 * multi-device context. */
#define BPE_REDUCE_RCCL 0
#define BPE_REDUCE_HOST 1
int bpe_create_multi(bpe_ctx **out, int n_shards, const int *devices, int reduce);
int bpe_shard_count(bpe_ctx *ctx, int *n_shards);

/* ---- vocabulary ------------------------------------------------------------------------------
 * Registers token `id` with the UTF-16 length of its chars (`token.chars.length`, used by the
 * max_length filter, core.ts:270-273).  Grows the table when id >= current size.  Called by the
 * host for every new char token (core.ts:186-199) and on fromJSON (core.ts:147-162); merged tokens
 * are registered by bpe_apply_merge itself (len16[c] = len16[a] + len16[b], core.ts:318). */
int bpe_set_token_len16(bpe_ctx *ctx, int32_t id, int32_t len16);
int bpe_num_tokens(bpe_ctx *ctx, int32_t *n_tokens);

/* ---- corpus ----------------------------------------------------------------------------------
 * addToCorpus (core.ts:182-207) / restoreToCorpus (core.ts:213-216): appends ONE sample whose
 * chars the host has already mapped to token ids.  n may be 0 (an empty sample). */
int bpe_add_sample(bpe_ctx *ctx, const int32_t *ids, int64_t n);

/* Bulk native ingest for corpora JS strings cannot hold: `n` latin1 bytes
 * (byte b == code point b), split into samples of `sample_bytes` (last one shorter; 0 = one
 * sample).  char_to_id[256] is in/out: -1 marks an unseen char; unseen chars get ids
 * *n_tokens_io, *n_tokens_io+1, ... in first-appearance order (core.ts:186-199).  char_hist[256]
 * receives the per-char occurrence counts of this call (the weight/original_weight increments of
 * core.ts:192-202).  Each new char is registered with len16 = 1. */
int bpe_add_latin1(bpe_ctx *ctx, const uint8_t *bytes, int64_t n, int64_t sample_bytes,
                   int32_t char_to_id[256], int32_t *n_tokens_io, int64_t char_hist[256]);

/* `corpus_in_code = []` (example/import-merge-log-to-ram.ts:21-22): drops every sample. */
int bpe_clear_corpus(bpe_ctx *ctx);

/* Sample count and live token count (excluding sample separators). */
int bpe_corpus_size(bpe_ctx *ctx, int64_t *n_samples, int64_t *n_tokens);

/* Materialises `corpus_in_code` (core.ts:106): all samples' ids back to back into ids_out
 * (capacity ids_cap) and n_samples+1 offsets into sample_off (capacity off_cap). */
int bpe_read_corpus(bpe_ctx *ctx, int32_t *ids_out, int64_t ids_cap, int64_t *sample_off,
                    int64_t off_cap);

/* Live token count of every sample, in corpus order (cap >= n_samples).  A merge shortens
 * exactly the samples it rewrites, so comparing lengths before and after finds the rows
 * BPETokenizerDB.applyMerge selects and updates (db/core.ts:399-417: `like '%from_code%'` +
 * `update corpus`).  Two reads of the corpus on the device; n_samples x 8 B come back. */
int bpe_sample_lengths(bpe_ctx *ctx, int64_t *lens, int64_t cap);

/* Reads back the samples idx[0..n) (any order, repeats allowed): their ids packed in that order
 * into ids_out (capacity ids_cap), sample k at [sample_off[k], sample_off[k+1]) (n+1 offsets).
 * The db twin's row write-back (db/core.ts:414-417) without materialising the whole corpus. */
int bpe_read_samples(bpe_ctx *ctx, const int64_t *idx, int64_t n, int32_t *ids_out, int64_t ids_cap,
                     int64_t *sample_off);

/* ---- hot path ----------------------------------------------------------------------------------
 * findNextMerge (core.ts:247-326).  max_length: 0 = falsy = unlimited (core.ts:255,272);
 * min_weight: 0 = falsy = 2 (core.ts:256).  On BPE_OK writes the chosen pair (a, b) and its count
 * W (== c.weight == c.original_weight, core.ts:317-323); BPE_NO_MERGE when the reference returns
 * null (core.ts:312-313).  The selection is bit-identical to the reference's running argmax
 * (max W, then min a+b, then earliest W-th counted occurrence — SURVEY.md Appendix A). */
int bpe_find_next_merge(bpe_ctx *ctx, int64_t max_length, int64_t min_weight, int32_t *a,
                        int32_t *b, int64_t *w);

/* applyMerge corpus rewrite (core.ts:356-359, `replaceAll(a.code+b.code, c.code)`): every
 * leftmost non-overlapping occurrence of (a, b) becomes c.  Also registers c (len16 sum).
 * `replaced` (may be NULL) receives the replacement count (== W for a merge from findNextMerge). */
int bpe_apply_merge(bpe_ctx *ctx, int32_t a, int32_t b, int32_t c, int64_t *replaced);

/* A run of applyMerge rewrites without counting pairs: restoreMerge replay (core.ts:477-494,
 * `example/import-merge-log-to-ram.ts`) and batch encoding of a corpus with a trained merge list
 * (encodeToCode, core.ts:392-409, applies the merges in order with replaceAll).  abc holds n
 * triples (a, b, c), applied in order, each registering c as bpe_apply_merge does.  One
 * apply-only streaming pass per merge.  count_after != 0: the last merge is applied by the fused
 * apply + count pass, so a findNextMerge that follows streams nothing extra.  replaced (may be
 * NULL) receives n replacement counts. */
int bpe_apply_merges(bpe_ctx *ctx, const int32_t *abc, int64_t n, int64_t *replaced,
                     int count_after);

/* mergeUntil (core.ts:365-383).  max_iterations 0 = unlimited.  New tokens get ids
 * bpe_num_tokens(), bpe_num_tokens()+1, ...  (core.ts:315).  Writes (a, b, W) int64 triples into
 * out_abw (capacity `cap` triples) and the number of merges into *n_merges. */
int bpe_merge_until(bpe_ctx *ctx, int64_t max_length, int64_t min_weight, int64_t max_iterations,
                    int64_t *out_abw, int64_t cap, int64_t *n_merges);

/* ---- sharded corpus (one process per GPU) ------------------------------------------------------
 * Pairs never cross samples (core.ts:265-267), so a corpus split at sample boundaries is counted
 * shard by shard; the caller sums the shards' tables (all-reduce / all-gather over RCCL) and
 * selects from the global table.  All table pointers below are DEVICE pointers on this context's
 * device (e.g. torch tensors); host pointers are marked.
 *
 * The pair-count table has BPE_TABLE_BINS u64 entries: [0, 65536) exact counts of the pairs with
 * both ids < 256 at b*256+a, [65536, 81920) a count sketch of every other pair (bucket =
 * ((b * 0x19B1 + a / 2) mod 8192) * 2 + (a & 1)): an upper bound of each such pair's count. */
#define BPE_HOT_BINS 65536
#define BPE_TABLE_BINS 81920

/* The digest plane of the device loop's delta form: one byte per corpus slot.  A token id t >= 0
 * has the digest t % BPE_DIGEST_MOD, a sample separator BPE_DIGEST_SEP, every dead slot
 * BPE_DIGEST_DEAD; ids with equal digests alias (an alias costs a chunk load, never a result). */
#define BPE_DIGEST_MOD 254
#define BPE_DIGEST_SEP 254
#define BPE_DIGEST_DEAD 255
/* Candidate pairs one stream of the plane answers for: the decided merge and the predicted next
 * ones, whose hit lists (one bit per chunk) are kept and applied from without another stream.
 * The stream tests a byte pair by one lookup in a 64 KiB table of candidate masks, a bit per
 * candidate in a byte per pair, so its cost does not grow with the candidates and eight, the bits
 * of the byte, is the most there can be.
 * BPE_DIGEST_CAND=n in the environment caps the candidates in use (1 .. this constant, read per
 * batch); at 1 every delta iteration streams the plane. */
#define BPE_DIGEST_CAND 8
/* out[i] = the digest of the slot value ids[i] (host arrays; needs no context and no device). */
int bpe_digest(const int32_t *ids, int64_t n, uint8_t *out);

/* This shard's table for the current corpus (one streaming pass if none is cached). */
int bpe_export_counts(bpe_ctx *ctx, uint64_t *table);

/* Given the GLOBAL (summed) table: the cold pairs whose sketch bucket reaches the best hot count
 * (the only ones that can still win) are counted exactly on this shard (one streaming pass) and
 * written as cold_keys[i] = a<<16|b (u32), cold_counts[i] (u64).  *n_cold = entries; -1 (and no
 * pass) when no bucket qualifies, a decision every rank reaches alike from the same global table,
 * so the cold-list exchange can be skipped; when *n_cold > cap nothing is written and
 * BPE_ERR_ARG is returned (retry with a bigger buffer). */
int bpe_heavy_counts(bpe_ctx *ctx, const uint64_t *table, int64_t max_length, uint32_t *cold_keys,
                     uint64_t *cold_counts, int64_t cap, int64_t *n_cold);

/* findNextMerge's selection (core.ts:294-313) over the GLOBAL table's exact hot bins plus the
 * GLOBAL exact cold entries (distinct keys).  Writes W and the candidate pairs sharing the best
 * (W, a+b) as host int32 (a, b) pairs into cand (capacity cap pairs); *n_cand may exceed cap
 * (then only cap written).  BPE_NO_MERGE when the reference would return null. */
int bpe_select_counts(bpe_ctx *ctx, const uint64_t *table, const uint32_t *cold_keys,
                      const uint64_t *cold_counts, int64_t n_cold, int64_t max_length,
                      int64_t min_weight, int32_t *cand, int64_t cap, int64_t *n_cand,
                      int64_t *w);

/* Rule R3 on this shard: for each host (a, b) pair in cand, the shard-local position + 1 of its
 * last counted occurrence (0 when none) into host last[n].  Positions grow in corpus order. */
int bpe_tie_positions(bpe_ctx *ctx, const int32_t *cand, int64_t n, uint64_t *last);

/* ---- the device-resident loop on one rank of a sharded corpus ---------------------------------
 * mergeUntil (core.ts:365-383) over shards with no host sync per iteration.  `xchg`
 * (BPE_XCHG_WORDS u64) and `tie` (BPE_TIE_WORDS u64) are DEVICE buffers the caller all-reduces IN
 * ORDER on this context's stream (bpe_get_stream; e.g. RCCL on that stream).  Per iteration:
 *   all-reduce(SUM, xchg[0 .. *xchg_words)); bpe_rank_loop_select;
 *   all-reduce(MAX, tie[0 .. BPE_TIE_WORDS)); bpe_rank_loop_decide; bpe_rank_loop_count
 * at most BPE_LOOP_BATCH times between bpe_rank_loop_begin and bpe_rank_loop_end.  Every rank takes
 * the same decisions from the same global tables, so all ranks run the same collectives; an
 * iteration after the batch has ended is a no-op (its collectives still run).
 * The exchange holds a header (BPE_XCHG_HDR words; word 0: this shard's replacement count of the
 * merge just applied, so that the sum checked against W covers every shard) and either
 *   - this shard's pair table (BPE_TABLE_BINS words), summed into the global table, or
 *   - after bpe_set_global_counts (the maintained state: every rank holds the GLOBAL hot and cold
 *     tables and keeps them merge by merge), BPE_DELTA_ROWS delta rows per token id: this shard's
 *     recount of every pair the merge (a, b) -> c touched, at HDR + 6 * other + row, rows
 *     (a, .) (b, .) (., a) (., b) (c, .) (., c) in this order of precedence.  In the
 *     incremental mode (bpe_set_mode) the global state lives in the shard's position index instead
 *     (every pair's global count beside this shard's own lists) and the exchange carries each
 *     merge's count CHANGES: 16 words for the pairs of two of {a, b, c} (signed, two's complement
 *     u64), then per token id and side the sites with that neighbour (left: (x, a) -> (x, c);
 *     right: (b, y) -> (c, y)) in unsigned lanes as wide as the last merge's count, packed in the
 *     u64 words (their u64 sum adds the lanes without carries).  *xchg_words is
 *     then 8 + 16 + 2 ceil(ids / lanes per word) for the batch's ids.
 *     A tie there takes one iteration of its own: the scan's positions cross in `tie`, and the
 *     next iteration commits the winner, so a batch may merge fewer times than it iterates.
 * tie: the tied candidates' last positions (rank << 40 | position, rule R3: rank r's occurrences
 * come after rank r-1's) in words 0..15, and word 16 this rank's vote for the host path (facts of
 * its own copy of the maintained tables: fill, dead claims, room).  A tie between pairs X Y is
 * decided from the corpus tail, which only the last rank (world - 1) scans.
 * bpe_rank_loop_begin writes this shard's part of the first exchange and *xchg_words (the words to
 * all-reduce per iteration of this batch: the same on every rank).  bpe_rank_loop_end syncs and
 * writes the batch's merges as (a, b, W, this shard's replacement count) quadruples into host
 * out_abwr (capacity cap quadruples; sum the counts over the shards: == W), *status:
 * 0 = every enqueued iteration merged, 1 = no pair qualifies (stop), 2 = the next iteration needs
 * the host protocol (heavy sketch buckets, more than BPE_MAX_CAND tied pairs, a vote: export /
 * heavy / select / tie_positions above).  A batch of the maintained state that ran to its end
 * leaves its last merge's delta rows in xchg for the next batch's first exchange: pass the same
 * buffer again. */
#define BPE_MAX_CAND 16
#define BPE_LOOP_BATCH 64
#define BPE_XCHG_HDR 8
#define BPE_DELTA_ROWS 6
#define BPE_XCHG_WORDS (BPE_XCHG_HDR + BPE_DELTA_ROWS * BPE_MAX_VOCAB)
#define BPE_TIE_WORDS 32
int bpe_rank_loop_begin(bpe_ctx *ctx, int64_t max_length, int64_t min_weight, uint64_t *xchg,
                        uint64_t *tie, int rank, int world, int64_t *xchg_words);
int bpe_rank_loop_select(bpe_ctx *ctx);
int bpe_rank_loop_decide(bpe_ctx *ctx);
int bpe_rank_loop_count(bpe_ctx *ctx);
int bpe_rank_loop_end(bpe_ctx *ctx, int64_t *out_abwr, int64_t cap, int64_t *n_merges, int *status);

/* The maintained state of a sharded corpus (skewed corpora, large vocabularies: the cold pairs
 * outgrow the sketch).  Every rank: bpe_cold_counts (its exact count of every pair with an id >=
 * 256, one streaming pass; *n > cap: nothing written, call again with room, no second pass), then
 * the lists of ALL ranks gathered (e.g. all-gather) and bpe_set_global_counts with the global table
 * (all-reduced bpe_export_counts) and the gathered lists (device pointers; duplicate keys summed).
 * The next rank loop batches keep those global tables up to date with delta rows (above); any
 * per-shard entry point (find/apply/export/...) drops the state.  In the incremental mode
 * bpe_set_global_counts builds the shard's position index and loads the global counts into it
 * (enter at once: a driver need not wait for the cold pairs to outgrow the sketch). */
int bpe_cold_counts(bpe_ctx *ctx, uint32_t *keys, uint64_t *counts, int64_t cap, int64_t *n);

/* The rank loop's collectives from C++ (one process per GPU): an RCCL
 * communicator per context, and a batch's iterations enqueued by one call.  Rank 0 makes the id
 * (bpe_rccl_unique_id, 128 bytes: NCCL_UNIQUE_ID_BYTES), the caller broadcasts it (e.g.
 * torch.distributed), then every rank calls bpe_rank_rccl_init (collective).  Between
 * bpe_rank_loop_begin and bpe_rank_loop_end, bpe_rank_loop_rccl(ctx, xchg, xchg_words, tie, k) runs
 * k iterations of: ncclAllReduce(SUM, xchg[0 .. xchg_words)); bpe_rank_loop_select;
 * ncclAllReduce(MAX, tie); bpe_rank_loop_decide; bpe_rank_loop_count — all on the context's
 * stream (no host sync, no cross-stream events).  The RCCL is the one beside the HIP runtime libbpe
 * runs on.  bpe_destroy frees the communicator; bpe_rank_rccl_destroy frees it earlier. */
int bpe_rccl_unique_id(void *id, size_t cap);
int bpe_rank_rccl_init(bpe_ctx *ctx, const void *id, int rank, int world);
int bpe_rank_loop_rccl(bpe_ctx *ctx, uint64_t *xchg, int64_t xchg_words, uint64_t *tie, int iterations);
int bpe_rank_rccl_destroy(bpe_ctx *ctx);
int bpe_set_global_counts(bpe_ctx *ctx, const uint64_t *table, const uint32_t *keys,
                          const uint64_t *counts, int64_t n);

/* ---- modes -------------------------------------------------------------------------------------
 * BPE_MODE_STREAM (default): every merge is one fused streaming pass over the corpus (apply the
 * merge, recount every pair): the reference's own full recount (core.ts:265-310), at HBM rate.
 * BPE_MODE_INCREMENTAL: bpe_merge_until works on a position index: per
 * merge only the W match sites and their neighbours are touched, O(W) instead of O(N).  Same
 * merges, counts and corpus; it changes what pair-scans/s measures, so it is reported apart.
 * Built per call by a hand-written counting scatter of the corpus's positions into per-pair lists
 * (one count pass, one exclusive scan, two fill passes; no sort); 32-bit positions, so up to
 * 0xFFFF0000 live slots per context or shard.  Env BPE_PIX=1 selects it for new contexts.  On a
 * multi-device context (bpe_create_multi) the mode applies to every shard: each shard indexes its
 * own samples inside the rank loop (above). */
#define BPE_MODE_STREAM 0
#define BPE_MODE_INCREMENTAL 1
int bpe_set_mode(bpe_ctx *ctx, int mode);

/* ---- measurement -------------------------------------------------------------------------------
 * HIP-event timings of the kernels, recorded on the context's own stream. */
typedef struct {
    double step_ms;           /* fused streaming pass (K1 count + K4 apply of the pending merge) */
    int64_t step_launches;
    int64_t step_slots;       /* int32 slots streamed by those passes (live + dead) */
    int64_t step_live;        /* live corpus tokens at those passes (pair-scans) */
    double select_ms;         /* boundary stitch + reduce + argmax + collect + R3 tie passes */
    int64_t tie_passes;       /* R3 tie-break passes */
    int64_t iterations;       /* findNextMerge calls */
    int64_t live_tokens;      /* sum over those calls of live corpus tokens (pair-scans) */
    int64_t compactions;      /* dead-slot compactions */
    int64_t exact_passes;     /* extra streaming passes for cold pairs whose sketch bucket could win */
    int64_t step_timed;       /* streaming passes whose duration step_ms sums (the device loop times
                                 every SPAN_EVERY-th iteration, all of its spans; select_ms covers
                                 those same iterations) */
    int64_t tie_tail;         /* device loop: R3 ties decided from the corpus-tail window alone */
    int64_t tie_lone;         /* ... of which the lone candidate missing from the window won */
    int64_t loop_host;        /* device loop: iterations handed to the host path (heavy sketch
                                 buckets, > BPE_MAX_CAND tied pairs, >= 2 tied pairs missing from
                                 the tail window, the vocabulary limit) */
    int64_t fused_passes;     /* merge passes that also refreshed the maintained cold-pair table */
    int64_t pix_builds;       /* incremental mode: position-index builds (one counting scatter of
                                 the corpus's positions) */
    int64_t pix_merges;       /* incremental mode: merges made on the index (O(W) each) */
    int64_t pix_host;         /* incremental mode: iterations the index handed to the stream */
    double pix_build_ms;      /* incremental mode: wall time of those builds (host clock, synced) */
    int64_t cold_used;        /* maintained state: claimed entries of the cold-pair table (largest seen) */
    int64_t sel_blocks;       /* maintained state: block maxima recomputed by incremental selections
                                 (cumulative since the context was made) */
    int64_t xchg_bytes;       /* rank loop: bytes of the per-iteration exchange all-reduced (SUM leg;
                                 the table, or the maintained state's delta rows), summed over the
                                 iterations (a multi-device context: over its shards) */
    int64_t xchg_iters;       /* rank loop: iterations those bytes cover */
    int64_t pix_fallbacks;    /* multi-device context, incremental mode: times the shards' index kept
                                 handing over and the run went on in the streaming mode */
    int64_t cold_rebuilds;    /* maintained state: cold pair tables rebuilt from their own live
                                 claims (instead of an exact pass over the corpus) */
    double incr_ms;           /* the device loop's maintained-state passes (k_step_loop<MODE_INCR>)
                                 among the timed step spans: their durations, */
    int64_t incr_timed;       /* ... their number, */
    int64_t incr_launches;    /* ... all such passes, */
    int64_t incr_live;        /* ... and the live corpus tokens summed over them (pair-scans) */
    int64_t unscreened_passes;/* device loop, table state: merge passes whose LDS adds return nothing
                                 and skip the overflow screen (no counter can reach 16 bits: the
                                 largest table bin + 2 W < 2^16); full passes only */
    int64_t delta_passes;     /* device loop, table state: iterations in the delta form (an apply-only
                                 stream, then the table kept by the deltas of the merge's sites
                                 instead of a recount; BPE_DELTA=0 turns the form off) */
    int64_t delta_chunks;     /* ... and the rewritten chunks those streams listed for the site kernel */
    int64_t digest_passes;    /* ... of the delta iterations, those whose stream read the digest plane
                                 (one byte per slot) instead of the int32 slots; BPE_DIGEST=0 keeps
                                 the int32 stream everywhere */
    int64_t digest_hits;      /* ... the chunks those streams took to the exact path (true sites,
                                 digest aliases, an a-alike last in its chunk, pending matches) */
    int64_t digest_builds;    /* builds of the digest plane (one pass over the int32 corpus each) */
    int64_t digest_scans;     /* ... of the digest_passes, those that streamed the plane (and filled the
                                 hit lists of up to BPE_DIGEST_CAND pairs); the others applied their
                                 merge from a cached list */
} bpe_stats;

int bpe_stats_enable(bpe_ctx *ctx, int on);
int bpe_get_stats(bpe_ctx *ctx, bpe_stats *out);
int bpe_reset_stats(bpe_ctx *ctx);

/* Raw device pointer of the context's HIP stream (hipStream_t), for callers that order their own
 * work (collectives, events) against the engine. */
int bpe_get_stream(bpe_ctx *ctx, void **stream);

/* ---- encoding ----------------------------------------------------------------------------------
 * encodeToCode (core.ts:392-409) for a batch of texts with a trained merge list, apart from any
 * corpus: `for (let [from_code, to_code] of this.merge_codes) content_in_code =
 * content_in_code.replaceAll(from_code, to_code)` (core.ts:404-406) on every text.  An encoder
 * holds the merge list as a rank table on one device.  A text of up to
 * BPE_ENCODE_LDS_TOKENS tokens is encoded by one workgroup in LDS: the lowest-ranked merge present is rewritten
 * (all its leftmost non-overlapping occurrences) until none is, which equals the in-order replay
 * whenever no merge's new token c is an input (a or b) of itself or an earlier merge — every list
 * the reference makes (c is a fresh index, core.ts:315,484).  Longer texts, and lists that break
 * that rule (checked as merges are added), are replayed merge by merge by apply-only streaming
 * passes (bpe_apply_merges on a scratch engine of the encoder).  Output is identical either way. */
#define BPE_ENCODE_LDS_TOKENS 16384
typedef struct bpe_encoder bpe_encoder;
typedef struct {
    double kernel_ms;         /* HIP-event time of the merge-rank kernels (per call: launch to end) */
    int64_t calls;            /* bpe_encode_batch calls */
    int64_t texts_rank;       /* texts encoded by the merge-rank kernels */
    int64_t texts_replay;     /* texts replayed by apply-only passes (long, or a non-greedy list) */
    int64_t tokens_in;        /* ids in */
    int64_t tokens_out;       /* ids out */
    int64_t steps;            /* merge-rank kernels: greedy steps (ranks rewritten), all texts */
} bpe_encoder_stats;

/* An encoder with no merges on HIP device `device` (fails with BPE_ERR_HIP without one). */
int bpe_encoder_create(bpe_encoder **out, int device);
int bpe_encoder_destroy(bpe_encoder *enc);
/* Appends n merges (a, b, c) in list order (`merge_codes`, core.ts:91,352; restoreMerge
 * core.ts:477-494 and fromJSON core.ts:163-169 append the same way).  Ids < BPE_MAX_VOCAB. */
int bpe_encoder_add_merges(bpe_encoder *enc, const int32_t *abc, int64_t n);
/* Drops every merge (fromJSON of another tokenizer, core.ts:140-145). */
int bpe_encoder_clear(bpe_encoder *enc);
int bpe_encoder_num_merges(bpe_encoder *enc, int64_t *n);
/* Encodes n_texts texts: text k = ids[off[k] .. off[k+1]) (token ids, `token.index`).  Writes the
 * encoded texts back to back into ids_out (capacity off[n_texts] - off[0]: a text never grows) and
 * n_texts + 1 offsets into out_off (out_off[0] = 0). */
int bpe_encode_batch(bpe_encoder *enc, const int32_t *ids, const int64_t *off, int64_t n_texts,
                     int32_t *ids_out, int64_t *out_off);
int bpe_encoder_get_stats(bpe_encoder *enc, bpe_encoder_stats *out);
int bpe_encoder_reset_stats(bpe_encoder *enc);

/* Long texts (more than BPE_ENCODE_LDS_TOKENS tokens).  BPE_LONG_REPLAY, the default, replays them
 * as described above.  BPE_LONG_SPLIT cuts them into segments at boundaries no merge can cross
 * and encodes the segments with the merge-rank kernels like any other text.  With first(x) and
 * last(x) the first and last base id a token id expands to (an id no merge makes is itself; for
 * (a, b) -> c, first(c) = first(a) and last(c) = last(b)), the boundary between tokens x | y is
 * safe iff (last(x), first(y)) differs from (last(a), first(b)) of every merge: the last base id
 * left of it and the first one right of it never change, so no merge can ever join across it, and
 * the replay of the whole text is the concatenation of the replays of both sides.  The text's
 * boundaries p (between tokens p - 1 and p) are searched in windows of BPE_ENCODE_SPLIT_WINDOW,
 * window j being [j * H + 1, min((j + 1) * H, n - 1)]; each window's cut is its largest safe p.
 * A text with a stretch of more than BPE_ENCODE_LDS_TOKENS tokens between cuts is replayed, and so
 * is every long text under a list the greedy cannot take or one that makes an id twice.  Output is
 * identical either way.  A split text counts in bpe_encoder_stats.texts_rank, a replayed one in
 * texts_replay.  BPE_ENCODE_LONG=split in the environment of bpe_encoder_create selects
 * BPE_LONG_SPLIT for the new encoder. */
#define BPE_LONG_REPLAY 0
#define BPE_LONG_SPLIT 1
#ifndef BPE_ENCODE_SPLIT_WINDOW   /* (-D at build time: tools/encode_long_bench.py compares windows) */
#define BPE_ENCODE_SPLIT_WINDOW 1024   /* H: a power of two, at most BPE_ENCODE_LDS_TOKENS / 2; the fastest of 1024, 2048, 4096, 8192 (profiles/encode_long_bench.jsonl) */
#endif
int bpe_encoder_set_long_texts(bpe_encoder *enc, int mode);   /* other values: BPE_ERR_ARG */
typedef struct {
    int64_t calls;          /* calls that planned at least one long text */
    int64_t texts_split;    /* long texts encoded as segments by the merge-rank kernels */
    int64_t texts_fallback; /* long texts with a stretch > BPE_ENCODE_LDS_TOKENS without a safe boundary: replayed */
    int64_t windows;        /* windows searched */
    int64_t segments;       /* segments of the texts_split texts */
    double plan_ms;         /* HIP-event time of the cut kernel */
} bpe_split_stats;
int bpe_encoder_get_split_stats(bpe_encoder *enc, bpe_split_stats *out);
int bpe_encoder_reset_split_stats(bpe_encoder *enc);

/* ---- encoding from text ------------------------------------------------------------------------
 * encodeToVector (core.ts:392-445) for a batch of UTF-16 texts, all three of its stages on the
 * device: chars -> token ids (`for (let char of content)` + char_to_token, core.ts:396-402), the
 * merges (bpe_encode_batch's kernels and routes), and ids -> vector indices (to_vector_index,
 * core.ts:434-444).  A unit continues the char before it when it is a low surrogate (0xDC00-0xDFFF),
 * not its text's first unit, and the unit before it is a high surrogate (0xD800-0xDBFF); every
 * other unit starts a char.  A char's key is its code point; a lone surrogate's its unit value.
 *
 * bpe_encoder_set_chars replaces the whole char table (char_to_token): n (code point, id) entries;
 * n == 0 drops it.  A code point above 0x10FFFF or a duplicate gives BPE_ERR_ARG, an id outside
 * [0, BPE_MAX_VOCAB) BPE_ERR_VOCAB; a failed call changes nothing.  bpe_encoder_clear keeps the
 * table (it drops merges).
 * bpe_encoder_set_vector_index takes to_vector_index of compactVectorIndex (core.ts:222-241): one
 * entry per token id, -1 for a hole (a token of weight 0); ids at or past n are holes.  NULL with
 * n == 0 drops the index; bpe_encoder_add_merges and bpe_encoder_clear drop it too
 * (invalidateVectorIndex, core.ts:348).
 *
 * bpe_encode_text_batch: text k is units[off[k] .. off[k+1]); off[0] need not be 0 and units before
 * it are never read; offsets must not decrease or be negative (BPE_ERR_ARG); n_texts == 0 is fine.
 * It writes the texts' values (token ids, or vector indices) back to back into vals_out and
 * n_texts + 1 offsets into out_off (out_off[0] = 0).  A text never grows, so vals_cap >=
 * off[n_texts] - off[0] always suffices; a smaller cap that the result does not fit gives
 * BPE_ERR_ARG with nothing written.  BPE_ENCODE_VECTORS without an index, and a call with at least
 * one unit without a char table, give BPE_ERR_STATE.
 * A char that is not in the table, or (vectors) a resulting id that is a hole, fails the whole
 * call with BPE_ERR_VOCAB; nothing is written to either output, the encoder stays usable, and the
 * message is
 *   unknown token, char: U+XXXX (text K, unit I)         (I: the char's first unit in its text)
 *   unknown token index: N (text K, position I)          (I: the position in the encoded text)
 * for the error the reference's `texts.map(t => encodeToVector(t))` throws: the first failing
 * text's, and inside one text the char's (core.ts:398-401 runs before any merge).
 * Launch shapes and the replay route are chosen by a text's unit count (its char count is at most
 * that); texts longer than BPE_ENCODE_LDS_TOKENS units and lists the greedy cannot take make the
 * call assemble on the host, as bpe_encode_batch does.  Output is identical either way.
 * With BPE_LONG_SPLIT a text longer than that is planned on its char count after the front end
 * and stays on the device, segment by segment; only a text that falls back to the replay makes
 * the call assemble on the host.  Error places stay relative to the text.
 * bpe_encode_text_batch_device is the same pipeline on buffers already on the encoder's device
 * (any 2-byte aligned unit pointer); values and offsets stay there; it reads the offsets back
 * (8 B per text) for the launch lists, runs on the encoder's stream and synchronises before
 * returning.  *needed (a host int64) receives the number of values.
 * The front end works on tiles of BPE_TEXT_TILE units and scans BPE_TEXT_SCAN_ROUND tile counts per
 * round (csrc/bpe_text.hip.h; exported for the tests). */
#define BPE_TEXT_TILE 2048
#define BPE_TEXT_SCAN_ROUND 2048
#define BPE_ENCODE_IDS 0       /* values out are token ids (encodeToCode's tokens) */
#define BPE_ENCODE_VECTORS 1   /* values out are vector indices (encodeToVector) */
typedef struct {
    int64_t calls;            /* text calls */
    int64_t texts;            /* texts of the calls that succeeded */
    int64_t units_in;         /* ... their UTF-16 units */
    int64_t chars;            /* ... their chars (token ids before the merges) */
    int64_t values_out;       /* ... the values written */
    double front_ms;          /* HIP-event time of the front-end kernels (units -> ids) */
    double back_ms;           /* ... of the back-end kernels (pack, vector index); the merge-rank
                                 kernels' time stays in bpe_encoder_stats.kernel_ms */
} bpe_text_stats;
int bpe_encoder_set_chars(bpe_encoder *enc, const uint32_t *code_points, const int32_t *ids, int64_t n);
int bpe_encoder_set_vector_index(bpe_encoder *enc, const int32_t *to_vector_index, int32_t n);
int bpe_encode_text_batch(bpe_encoder *enc, int kind, const uint16_t *units, const int64_t *off,
                          int64_t n_texts, int32_t *vals_out, int64_t vals_cap, int64_t *out_off);
int bpe_encode_text_batch_device(bpe_encoder *enc, int kind, const uint16_t *d_units, const int64_t *d_off,
                                 int64_t n_texts, int32_t *d_vals_out, int64_t vals_cap,
                                 int64_t *d_out_off, int64_t *needed);
int bpe_encoder_get_text_stats(bpe_encoder *enc, bpe_text_stats *out);
int bpe_encoder_reset_text_stats(bpe_encoder *enc);

/* ---- corpus from text --------------------------------------------------------------------------
 * addToCorpus (core.ts:182-207) for a batch of UTF-16 texts, on the device: the call leaves the
 * context exactly as `for (t of texts) addToCorpus(t)` would.  Chars follow bpe_encode_text_batch's
 * rule (above): a low surrogate right after a high one inside the same text continues the char, every
 * other unit starts one; a char's key is its code point, a lone surrogate's its unit value.
 *
 * The context owns a char table (char_to_token: code point -> id).  bpe_set_chars replaces it, with
 * bpe_encoder_set_chars's argument rules and error codes (a code point above 0x10FFFF or a duplicate:
 * BPE_ERR_ARG; an id outside [0, BPE_MAX_VOCAB): BPE_ERR_VOCAB; a failed call changes nothing);
 * n == 0 drops the table.  An id at or past bpe_num_tokens() is registered by the call (len16 2 for
 * a supplementary code point, else 1; ids between get len16 1, as bpe_add_sample registers them), so
 * new chars are never numbered into the table's ids.  Use it after fromJSON, and whenever chars were
 * added some other way: the table knows only what this call and the text ingest put into it.
 * bpe_add_sample and bpe_add_latin1 do not feed it, and bpe_clear_corpus keeps it.
 *
 * bpe_add_text_batch: text k is units[off[k] .. off[k+1]) (host buffers; any 2-byte aligned unit
 * pointer); off[0] need not be 0 and units before it are never read; offsets must not decrease or be
 * negative (BPE_ERR_ARG); n_texts == 0 is fine.  A char that is not in the table becomes a new token:
 * new tokens get the ids bpe_num_tokens(), +1, ... (after any merged tokens) in order of first
 * appearance over the whole batch (text 0 before text 1; inside a text by unit position), are
 * registered with len16 2 for a supplementary code point and 1 otherwise, and enter the table.
 * new_chars[i] receives the code point (or lone unit value) of token bpe_num_tokens() + i, *n_new
 * their number.  Every text becomes one sample, its ids then the separator; an empty text is an empty
 * sample.  id_hist[id] receives the char occurrences of this call for every id below the token count
 * after the call (the weight / original_weight increments of core.ts:192-202; the engine's own
 * per-token counts take them too); hist_cap = BPE_MAX_VOCAB always suffices.
 * A failed call changes nothing (corpus, sample count, char table, vocabulary, counts, maintained
 * state) and the context stays usable: new_cap < the new chars gives BPE_ERR_ARG with *n_new written
 * (retry with room), hist_cap below the token count after the call BPE_ERR_ARG, new chars that would
 * pass BPE_MAX_VOCAB BPE_ERR_VOCAB.
 * bpe_add_text_batch_device is the same with units and offsets already on the context's device; the
 * small outputs (new_chars, id_hist) stay host-side; it runs on the context's stream and synchronises
 * before returning.  (A multi-device context copies them to the host and takes the host form.)
 * A multi-device context takes the call as it takes bpe_add_latin1: on a fresh corpus the texts are
 * cut into contiguous runs of whole texts of about equal units, one per shard; otherwise all go to
 * the last shard.  Numbering, counts, corpus and merges equal a single context's.
 * The kernels work on bpe_encode_text_batch's tiles (BPE_TEXT_TILE, BPE_TEXT_SCAN_ROUND;
 * csrc/bpe_ingest.hip.h). */
typedef struct {
    int64_t calls;            /* text ingest calls */
    int64_t texts;            /* texts of the calls that succeeded */
    int64_t units;            /* ... their UTF-16 units */
    int64_t chars;            /* ... their chars (corpus tokens added) */
    int64_t new_chars;        /* ... the char tokens they created */
    double kernel_ms;         /* HIP-event time of the ingest kernels (discover and map spans) */
} bpe_ingest_stats;
int bpe_set_chars(bpe_ctx *ctx, const uint32_t *code_points, const int32_t *ids, int64_t n);
int bpe_add_text_batch(bpe_ctx *ctx, const uint16_t *units, const int64_t *off, int64_t n_texts,
                       uint32_t *new_chars, int64_t new_cap, int64_t *n_new, int64_t *id_hist,
                       int64_t hist_cap);
int bpe_add_text_batch_device(bpe_ctx *ctx, const uint16_t *d_units, const int64_t *d_off, int64_t n_texts,
                              uint32_t *new_chars, int64_t new_cap, int64_t *n_new, int64_t *id_hist,
                              int64_t hist_cap);
int bpe_get_ingest_stats(bpe_ctx *ctx, bpe_ingest_stats *out);
int bpe_reset_ingest_stats(bpe_ctx *ctx);

/* ---- corpus from encoded samples / restore -----------------------------------------------------
 * bpe_add_sample for a batch, and on top of it restoreToCorpus (core.ts:213-216:
 * `corpus_in_code.push(encodeToCode(content))`) for a batch of UTF-16 texts, on the device.
 *
 * bpe_add_sample_batch: sample k is ids[off[k] .. off[k+1]) (host buffers); off[0] need not be 0 and
 * ids before it are never read; offsets must not decrease or be negative (BPE_ERR_ARG); n == 0 and
 * empty samples are fine.  The call leaves the context exactly as
 * `for k: bpe_add_sample(ids + off[k], off[k+1] - off[k])` would: corpus, sample count, live count,
 * the engine's per-token counts, and the vocabulary (ids at or past bpe_num_tokens() are registered
 * with len16 1).  An id outside [0, BPE_MAX_VOCAB) gives BPE_ERR_ARG with bpe_add_sample's message.
 * A failed call changes nothing (the loop would have kept the samples before the bad one; the batch
 * is atomic) and the context stays usable.
 * bpe_add_sample_batch_device is the same with ids and offsets already on the context's device (any
 * 4-byte aligned id pointer); it reads the n + 1 offsets back (8 B per sample) for validation and
 * sizing, runs on the context's stream and synchronises before returning.
 *
 * bpe_restore_text_batch: text k is units[off[k] .. off[k+1]), with bpe_encode_text_batch's offset
 * rules.  The texts go through `enc` (its char table, its merges, its long-text mode and all its
 * routes: bpe_encode_text_batch_device with BPE_ENCODE_IDS, into scratch on the device) and the
 * result is appended as samples, one per text, by the code above: no id comes to the host unless the
 * encoder itself assembles there (a replayed long text).  enc must be on the context's device
 * (BPE_ERR_ARG).  No token weight, char table or vocabulary entry changes beyond what bpe_add_sample
 * does for those ids ("Token weights are not updated when restoring content").
 * The encoder's errors come back as they are: `unknown token, char: U+XXXX (text K, unit I)` with
 * BPE_ERR_VOCAB, texts with at least one unit and no char table BPE_ERR_STATE, offset errors
 * BPE_ERR_ARG.  The batch is atomic: on any error no text has been added, where the reference's
 * `for (t of texts) restoreToCorpus(t)` would have added the texts before the failing one.
 * Scratch beside the corpus: 4 B per unit and 8 B per text (the host form: 2 B per unit and 8 B per
 * text more), kept by the context and only ever grown; BPE_ERR_OOM changes nothing.
 * bpe_restore_text_batch_device is the same with units and offsets already on the context's device;
 * it runs on the encoder's stream, then the context's, and synchronises before returning.
 *
 * A multi-device context takes both as it takes bpe_add_text_batch: on a fresh corpus the samples are
 * cut into contiguous runs of whole samples of about equal tokens, one per shard; otherwise all go to
 * the last shard.  Its restore encodes through the encoder's host form (any device), and its device
 * forms copy to the host.  Corpus, counts and merges equal a single context's.
 *
 * bpe_token_counts: the occurrences of every token id in the corpus (the engine's own exact counts,
 * after any pending merge is settled); cap >= bpe_num_tokens(), else BPE_ERR_ARG.  A multi-device
 * context sums its shards.
 * The append kernel works on tiles of BPE_APPEND_TILE corpus slots (csrc/bpe_append.hip.h; exported
 * for the tests, which place sample ends around the tile edges). */
#define BPE_APPEND_TILE 2048   /* corpus slots per tile of the append kernel */
typedef struct {
    int64_t calls;            /* sample-batch and restore calls */
    int64_t samples;          /* samples of the calls that succeeded */
    int64_t tokens;           /* ... their tokens */
    double kernel_ms;         /* HIP-event time of the append kernel only */
} bpe_append_stats;
int bpe_add_sample_batch(bpe_ctx *ctx, const int32_t *ids, const int64_t *off, int64_t n);
int bpe_add_sample_batch_device(bpe_ctx *ctx, const int32_t *d_ids, const int64_t *d_off, int64_t n);
int bpe_restore_text_batch(bpe_ctx *ctx, bpe_encoder *enc, const uint16_t *units, const int64_t *off,
                           int64_t n_texts);
int bpe_restore_text_batch_device(bpe_ctx *ctx, bpe_encoder *enc, const uint16_t *d_units, const int64_t *d_off,
                                  int64_t n_texts);
int bpe_token_counts(bpe_ctx *ctx, int64_t *counts, int64_t cap);
int bpe_get_append_stats(bpe_ctx *ctx, bpe_append_stats *out);
int bpe_reset_append_stats(bpe_ctx *ctx);

/* ---- decoding ----------------------------------------------------------------------------------
 * decodeVector / decodeTokens (core.ts:447-471) for a batch of texts: `content += token.chars` for
 * every value of a text (core.ts:462-468), the values being vector indices (mapped through
 * from_vector_index first) or token ids.  A decoder holds the vocabulary on one device: a blob of
 * UTF-16 code units (`token.chars` is a JS string: a unit is a uint16_t, lone surrogates included)
 * and one (offset, length) record per token id, with 32-bit offsets: a vocabulary whose chars would
 * pass 2^32 units is refused with BPE_ERR_VOCAB.  Ids stay below BPE_MAX_VOCAB.
 *
 * Token order: ids are given in the order the tokens are added; char tokens (bpe_decoder_add_tokens)
 * and merged tokens (bpe_decoder_add_merges) interleave freely, as they do in the reference when
 * addToCorpus runs after merges.
 * bpe_decoder_add_tokens appends n char tokens with ids count, count + 1, ...: token k's chars are
 * units[off[k] .. off[k+1]) (any length >= 0; the reference makes 1 or 2).
 * bpe_decoder_add_merges appends n merged tokens, chars[c] = chars[a] + chars[b] (core.ts:318,487),
 * from the (a, b, c) triples the encoder takes.  Each c must equal the token count at its turn
 * (core.ts:315,484), else BPE_ERR_ARG; a and b must be below that count (they may name tokens added
 * earlier in the same call), else BPE_ERR_VOCAB.  A failed call adds nothing.
 * bpe_decoder_set_vector_index takes from_vector_index of compactVectorIndex (core.ts:222-241): n
 * token ids, each below the token count, else BPE_ERR_VOCAB; n == 0 with NULL drops the index.
 * add_tokens, add_merges and clear drop the index too (invalidateVectorIndex, core.ts:348), and
 * BPE_DECODE_VECTORS without an index returns BPE_ERR_STATE.
 *
 * bpe_decode_batch: text k is vals[off[k] .. off[k+1]); off[0] need not be 0, offsets must not
 * decrease, n_texts == 0 is fine (out_off[0] = 0).  It writes n_texts + 1 offsets with
 * out_off[0] = 0, so out_off[n_texts] is the number of units needed; if that exceeds units_cap no
 * unit is written and BPE_ERR_ARG comes back (units_out == NULL with units_cap 0 is the sizing
 * call); otherwise the texts' units are written back to back.
 * A value outside [0, n_live) for vectors, or [0, n_tokens) for ids, fails the whole call with
 * BPE_ERR_VOCAB; nothing is written to units_out or out_off, and the message is
 *   unknown vector index: V (text K, position I)      /      unknown token index: V (text K, position I)
 * for the first offending value in flat order, the one the reference's loop throws on
 * (core.ts:462-468).  The decoder stays usable.
 * bpe_decode_batch_device is the same pipeline on buffers already on the decoder's device (e.g.
 * torch tensors holding a model's output); it runs on the decoder's stream and synchronises before
 * returning; *needed is a host int64.  The host form is this function plus the copies.
 * Offsets must not be negative (BPE_ERR_ARG).
 * The kernels work on tiles of BPE_DECODE_TILE values, and the scan of the tiles' sums takes
 * BPE_DECODE_SCAN_ROUND of them per round (csrc/bpe_decode.hip; exported for the tests, which
 * place texts around the first and size a batch past the second). */
#define BPE_DECODE_TILE 1024
#define BPE_DECODE_SCAN_ROUND 8192
#define BPE_DECODE_IDS 0       /* decodeTokens: values are token ids */
#define BPE_DECODE_VECTORS 1   /* decodeVector: values are vector indices */
typedef struct bpe_decoder bpe_decoder;
typedef struct {
    double kernel_ms;         /* HIP-event time of the decode kernels (per call: first launch to last) */
    int64_t calls;            /* decode calls (the sizing call counts) */
    int64_t texts;            /* texts of the calls whose values were all known */
    int64_t values_in;        /* ... their values */
    int64_t units_out;        /* UTF-16 units written */
} bpe_decoder_stats;

/* A decoder with no tokens on HIP device `device` (fails with BPE_ERR_HIP without one). */
int bpe_decoder_create(bpe_decoder **out, int device);
int bpe_decoder_destroy(bpe_decoder *dec);
/* Drops every token (fromJSON of another tokenizer, core.ts:140-145). */
int bpe_decoder_clear(bpe_decoder *dec);
int bpe_decoder_add_tokens(bpe_decoder *dec, const uint16_t *units, const int64_t *off, int64_t n);
int bpe_decoder_add_merges(bpe_decoder *dec, const int32_t *abc, int64_t n);
int bpe_decoder_num_tokens(bpe_decoder *dec, int32_t *n_tokens, int64_t *n_units);
int bpe_decoder_set_vector_index(bpe_decoder *dec, const int32_t *from_vector_index, int32_t n);
int bpe_decode_batch(bpe_decoder *dec, int kind, const int32_t *vals, const int64_t *off,
                     int64_t n_texts, uint16_t *units_out, int64_t units_cap, int64_t *out_off);
int bpe_decode_batch_device(bpe_decoder *dec, int kind, const int32_t *d_vals, const int64_t *d_off,
                            int64_t n_texts, uint16_t *d_units_out, int64_t units_cap,
                            int64_t *d_out_off, int64_t *needed);
int bpe_decoder_get_stats(bpe_decoder *dec, bpe_decoder_stats *out);
int bpe_decoder_reset_stats(bpe_decoder *dec);

/* ---- corpus out ----------------------------------------------------------------------------------
 * The trained corpus back out of the device layout: samples as token ids (`corpus_in_code` as ids,
 * core.ts:106), as vector indices (encodeToVector of every sample, core.ts:434-444, without encoding
 * the raw text again: what example/skip-gram.ts consumes), as code units (the `corpus_in_code` /
 * `content_code` strings themselves: unit = id + 1, at most BPE_MAX_VOCAB, so 16 bits hold it), or,
 * through a decoder, as UTF-16 text (the opposite of bpe_restore_text_batch).
 *
 * bpe_export_samples: idx is a host array of n sample indices, in any order, repeats allowed,
 * n == 0 fine; idx == NULL means every sample in corpus order, and n must then be the context's
 * sample count (BPE_ERR_ARG).  An index outside [0, n_samples) gives BPE_ERR_ARG with nothing
 * written.  The samples' values go back to back into vals_out (int32_t, or uint16_t for
 * BPE_EXPORT_CODE; vals_cap counts values) and n + 1 offsets into out_off (out_off[0] = 0).
 * Capacity follows bpe_decode_batch: when out_off[n] exceeds vals_cap the offsets are written, no
 * value is, and BPE_ERR_ARG comes back (vals_out == NULL with vals_cap 0 is the sizing call).
 * BPE_EXPORT_VECTORS takes to_vector_index of compactVectorIndex (core.ts:222-241) as a host array
 * with bpe_encoder_set_vector_index's rules: n_index entries, -1 for a hole, ids at or past n_index
 * are holes; NULL gives BPE_ERR_STATE (the other kinds ignore both arguments).  A token that maps to
 * a hole fails the whole call with BPE_ERR_VOCAB, nothing written to either output, and the message
 *   unknown token index: N (sample K, position I)     (K: the place in idx; I: the place in the sample)
 * for the first failing value in output order.  The engine's exact per-token counts rule that out on
 * the host when no id with a nonzero count is a hole; only otherwise does a check pass over the
 * samples run before anything is written.
 * An export only reads: it settles a pending merge as bpe_sample_lengths does and leaves the corpus,
 * the counts, the mode, the digest plane, the hit lists and every other stat as they were, so a
 * bpe_merge_until after it gives the merges it would have given without it.
 * bpe_export_samples_device is the same with the outputs on the context's device (any 4-byte aligned
 * value pointer, 2-byte for BPE_EXPORT_CODE; idx and to_vector_index stay host arrays): no value
 * touches the host.  *needed (a host int64) receives the number of values.  It runs on the context's
 * stream and synchronises before returning.
 *
 * bpe_export_text_batch: the samples' ids go into scratch on the context (4 B per token and 8 B per
 * sample, grow-only) and through `dec` (bpe_decode_batch_device with BPE_DECODE_IDS): units_out and
 * out_off as bpe_decode_batch fills them, the decoder's errors, messages and sizing behaviour as
 * they are (a decoder that knows fewer tokens than the corpus holds: `unknown token index: V (text K,
 * position I)`).  dec must be on the context's device (BPE_ERR_ARG; NULL too).  In the device form no
 * id and no unit touches the host; it runs on the context's stream, then the decoder's.
 *
 * A multi-device context takes the host forms shard by shard into the caller's buffer (the indices
 * routed to the shards that hold them, as bpe_read_samples routes them; its text export decodes
 * through the decoder's host form); the device forms refuse it with BPE_ERR_ARG, since the shards
 * sit on different devices.
 * The kernels stage one chunk of BPE_EXPORT_TILE corpus slots per wave (csrc/bpe_export.hip.h;
 * exported for the tests); the prefixes come from the scan of bpe_sample_lengths, one block of
 * BPE_EXPORT_SCAN_THREADS threads, each owning a run of consecutive entries. */
#define BPE_EXPORT_TILE 256           /* corpus slots per wave step of the export kernels */
#define BPE_EXPORT_SCAN_THREADS 1024  /* threads of the one-block scan of the prefixes */
#define BPE_EXPORT_IDS     0   /* int32 token ids (what bpe_read_samples returns) */
#define BPE_EXPORT_VECTORS 1   /* int32 to_vector_index[id]: encodeToVector of the sample, core.ts:434-444 */
#define BPE_EXPORT_CODE    2   /* uint16 units id + 1: the sample's corpus_in_code / content_code string */
typedef struct {
    int64_t calls;            /* export calls (sizing calls and failed calls count) */
    int64_t samples;          /* samples of the calls that wrote their values */
    int64_t values;           /* ... the values they wrote (tokens; for the text export too) */
    double kernel_ms;         /* HIP-event time of the export's kernels (index, check and emit spans) */
} bpe_export_stats;
int bpe_export_samples(bpe_ctx *ctx, int kind, const int64_t *idx, int64_t n,
                       const int32_t *to_vector_index, int32_t n_index,
                       void *vals_out, int64_t vals_cap, int64_t *out_off);
int bpe_export_samples_device(bpe_ctx *ctx, int kind, const int64_t *idx, int64_t n,
                              const int32_t *to_vector_index, int32_t n_index,
                              void *d_vals_out, int64_t vals_cap, int64_t *d_out_off, int64_t *needed);
int bpe_export_text_batch(bpe_ctx *ctx, bpe_decoder *dec, const int64_t *idx, int64_t n,
                          uint16_t *units_out, int64_t units_cap, int64_t *out_off);
int bpe_export_text_batch_device(bpe_ctx *ctx, bpe_decoder *dec, const int64_t *idx, int64_t n,
                                 uint16_t *d_units_out, int64_t units_cap, int64_t *d_out_off, int64_t *needed);
int bpe_get_export_stats(bpe_ctx *ctx, bpe_export_stats *out);
int bpe_reset_export_stats(bpe_ctx *ctx);

/* ---- text as UTF-8 -------------------------------------------------------------------------------
 * The three text pipelines above from UTF-8 bytes (files, datasets, byte tensors) instead of UTF-16
 * units: the bytes are transcoded to units on the device and the UTF-16 `_device` form takes them
 * there, so a host form ships 1 B per byte and no char is touched on the host.
 *
 * Text k is bytes[off[k] .. off[k+1]) and decodes on its own, exactly as Node's
 * Buffer.prototype.toString() and WHATWG TextDecoder('utf-8', {ignoreBOM: true}) decode it (what
 * fileContentToCorpus does to a Buffer, core.ts:55-58; CPython's bytes.decode('utf-8', 'replace')
 * gives the same): every maximal ill-formed subpart becomes one U+FFFD, a sequence cut by the end
 * of its text is ill-formed, a BOM stays U+FEFF, a 4-byte sequence becomes a surrogate pair.
 * Ill-formed input is not an error: U+FFFD is then a char like any other (new to the ingest; to the
 * encoder unknown unless its table has it).
 *
 * bpe_encoder_utf8_to_utf16 is the transcode alone, on the encoder's device and stream and in its
 * own grow-only scratch.  Offsets follow bpe_encode_text_batch's rules (off[0] need not be 0 and
 * bytes before it are never read; decreasing or negative offsets give BPE_ERR_ARG; n_texts == 0 is
 * fine), capacity follows bpe_decode_batch's: out_off receives n_texts + 1 offsets with
 * out_off[0] = 0; when out_off[n_texts] exceeds units_cap the offsets are written, no unit is, and
 * BPE_ERR_ARG comes back (units_out == NULL with units_cap 0 is the sizing call).  units_cap >=
 * off[n_texts] - off[0] always suffices.  The `_device` form takes and fills buffers on the
 * encoder's device (any byte pointer, any 2-byte aligned unit pointer), reads the offsets back
 * (8 B per text) and synchronises before returning; *needed (a host int64) receives the units.
 *
 * bpe_encode_utf8_batch, bpe_add_utf8_batch and bpe_restore_utf8_batch are that transcode (on the
 * encoder for the encode and the restore, on the context for the ingest) followed by
 * bpe_encode_text_batch_device, bpe_add_text_batch_device and bpe_restore_text_batch_device on the
 * units and their offsets: outputs, error codes, messages, atomicity and the long-text routes are
 * those of the UTF-16 form given the decoded texts, and error places stay (text K, unit I) with I a
 * unit of the decoded text.  The host forms copy the bytes in and only the existing outputs out;
 * the `_device` forms change their arguments as the UTF-16 `_device` forms do.
 * A multi-device context transcodes on its first shard's device, brings the units to the host and
 * takes its UTF-16 host form (the restore: on the encoder's device); its device forms do the same
 * from device buffers.
 *
 * bpe_utf8_stats counts the calls and, for those whose whole pipeline succeeded, their texts,
 * bytes, units and `replaced`: the U+FFFD made from ill-formed input (a U+FFFD spelled EF BF BD is
 * not counted), which is how a caller learns that a file was not clean.  The encoder's counters
 * take the transcode, the encode and the restore, the context's the ingest (a multi-device
 * context's: its first shard's).
 * The kernels work on tiles of BPE_UTF8_TILE bytes and scan BPE_TEXT_SCAN_ROUND tile counts per
 * round (csrc/bpe_utf8.hip.h; exported for the tests). */
#define BPE_UTF8_TILE 4096
typedef struct {
    int64_t calls;            /* UTF-8 calls */
    int64_t texts;            /* texts of the calls that succeeded */
    int64_t bytes;            /* ... their bytes */
    int64_t units;            /* ... the UTF-16 units they decoded to */
    int64_t replaced;         /* ... the U+FFFD among them made from ill-formed input */
    double kernel_ms;         /* HIP-event time of the transcode kernels */
} bpe_utf8_stats;
int bpe_encoder_utf8_to_utf16(bpe_encoder *enc, const uint8_t *bytes, const int64_t *off, int64_t n_texts,
                              uint16_t *units_out, int64_t units_cap, int64_t *out_off);
int bpe_encoder_utf8_to_utf16_device(bpe_encoder *enc, const uint8_t *d_bytes, const int64_t *d_off,
                                     int64_t n_texts, uint16_t *d_units_out, int64_t units_cap,
                                     int64_t *d_out_off, int64_t *needed);
int bpe_encode_utf8_batch(bpe_encoder *enc, int kind, const uint8_t *bytes, const int64_t *off, int64_t n_texts,
                          int32_t *vals_out, int64_t vals_cap, int64_t *out_off);
int bpe_encode_utf8_batch_device(bpe_encoder *enc, int kind, const uint8_t *d_bytes, const int64_t *d_off,
                                 int64_t n_texts, int32_t *d_vals_out, int64_t vals_cap, int64_t *d_out_off,
                                 int64_t *needed);
int bpe_add_utf8_batch(bpe_ctx *ctx, const uint8_t *bytes, const int64_t *off, int64_t n_texts,
                       uint32_t *new_chars, int64_t new_cap, int64_t *n_new, int64_t *id_hist, int64_t hist_cap);
int bpe_add_utf8_batch_device(bpe_ctx *ctx, const uint8_t *d_bytes, const int64_t *d_off, int64_t n_texts,
                              uint32_t *new_chars, int64_t new_cap, int64_t *n_new, int64_t *id_hist,
                              int64_t hist_cap);
int bpe_restore_utf8_batch(bpe_ctx *ctx, bpe_encoder *enc, const uint8_t *bytes, const int64_t *off,
                           int64_t n_texts);
int bpe_restore_utf8_batch_device(bpe_ctx *ctx, bpe_encoder *enc, const uint8_t *d_bytes, const int64_t *d_off,
                                  int64_t n_texts);
int bpe_encoder_get_utf8_stats(bpe_encoder *enc, bpe_utf8_stats *out);
int bpe_encoder_reset_utf8_stats(bpe_encoder *enc);
int bpe_get_utf8_stats(bpe_ctx *ctx, bpe_utf8_stats *out);
int bpe_reset_utf8_stats(bpe_ctx *ctx);

/* ---- lines as samples ----------------------------------------------------------------------------
 * The corpus helpers (core.ts:35-75) on the device: a batch of texts becomes a batch of samples,
 * exactly texts.flatMap(helper), so that a file's bytes reach the corpus without a host loop over
 * chars or lines.
 *   BPE_LINES_TRIM  linesToCorpus (core.ts:61-64): the text cut at every U+000A; each piece p becomes
 *                   U+000D + p.trim() + U+000A.  trim() removes, at both ends, the 25 units ECMAScript
 *                   calls WhiteSpace or LineTerminator: 0009-000D, 0020, 00A0, 1680, 2000-200A, 2028,
 *                   2029, 202F, 205F, 3000, FEFF (not 001C-001F, 0085, 180E or 200B);
 *   BPE_LINES_KEEP  linesTrimmedToCorpus (core.ts:67-75): the same cut; from each piece exactly one
 *                   trailing U+000D is dropped if present, nothing else; the same wrap;
 *   BPE_LINES_FILE  fileContentToCorpus (core.ts:55-58): one sample per text, U+001C + text + U+0004.
 * (The reference's doc comments of the two line helpers are swapped relative to their code; this
 * follows the code.)  A text with m line feeds gives m + 1 samples, the empty text one (CR LF); a
 * text boundary always ends a line and nothing is trimmed across it.  No cut or trim separates a
 * surrogate pair: all 25 units are BMP non-surrogates.
 *
 * bpe_encoder_split_lines is the split alone, on the encoder's device and stream and in its own
 * grow-only scratch.  Text k is units[off[k] .. off[k+1]) with bpe_encode_text_batch's offset rules.
 * Sizing follows bpe_decode_batch: *n_samples (and *needed, the units of all samples, in the
 * `_device` form) are always written once the arguments are valid; off_cap counts offsets, so
 * n_samples + 1 suffice; when off_cap or units_cap is too small nothing else is written and
 * BPE_ERR_ARG comes back (NULL outputs with zero capacities are the sizing call).  units_cap >=
 * 3 * (off[n_texts] - off[0]) + 2 * n_texts always suffices.  n_samples at or past 0x7FFFFFFF and an
 * unknown mode give BPE_ERR_ARG.  The `_device` form takes and fills buffers on the encoder's device
 * (any 2-byte aligned unit pointers), reads the offsets back (8 B per text) and synchronises before
 * returning.
 *
 * bpe_add_lines_batch and bpe_restore_lines_batch are that split (on the context for the ingest, on
 * the encoder for the restore) followed by bpe_add_text_batch_device / bpe_restore_text_batch_device
 * on the samples; the `_utf8_` forms run the UTF-8 transcode ("text as UTF-8") in front of the
 * split.  The context is left exactly as `for (t of texts) for (s of helper(t)) addToCorpus(s)`
 * leaves it: new_chars and id_hist are the ingest's own, and outputs, error codes, messages and
 * atomicity are those of the UTF-16 form given the produced samples (a failed call changes
 * nothing).  Error places (text K, unit I) refer to the produced sample K and its units, markers
 * included, not to the input text.  A multi-device context splits on its first shard's device,
 * brings the samples to the host and takes its UTF-16 host form (the restore: on the encoder's
 * device).  There is no encode-from-lines form: bpe_encoder_split_lines_device followed by
 * bpe_encode_text_batch_device composes it.
 *
 * bpe_lines_stats counts the calls and, for those whose whole pipeline succeeded, their texts,
 * units in, samples, units out (markers included) and `trimmed`: the units the mode dropped
 * (whitespace, the line feeds themselves, a CR in KEEP).  The kernels work on
 * bpe_encode_text_batch's tiles (BPE_TEXT_TILE, BPE_TEXT_SCAN_ROUND; csrc/bpe_lines.hip.h). */
#define BPE_LINES_TRIM 0
#define BPE_LINES_KEEP 1
#define BPE_LINES_FILE 2
typedef struct {
    int64_t calls;            /* line-split calls */
    int64_t texts;            /* texts of the calls that succeeded */
    int64_t units_in;         /* ... their UTF-16 units */
    int64_t samples;          /* ... the samples they gave */
    int64_t units_out;        /* ... the samples' units, markers included */
    int64_t trimmed;          /* ... the units the mode dropped */
    double kernel_ms;         /* HIP-event time of the split kernels */
} bpe_lines_stats;
int bpe_encoder_split_lines(bpe_encoder *enc, int mode, const uint16_t *units, const int64_t *off, int64_t n_texts,
                            uint16_t *units_out, int64_t units_cap, int64_t *out_off, int64_t off_cap,
                            int64_t *n_samples);
int bpe_encoder_split_lines_device(bpe_encoder *enc, int mode, const uint16_t *d_units, const int64_t *d_off,
                                   int64_t n_texts, uint16_t *d_units_out, int64_t units_cap, int64_t *d_out_off,
                                   int64_t off_cap, int64_t *n_samples, int64_t *needed);
int bpe_add_lines_batch(bpe_ctx *ctx, int mode, const uint16_t *units, const int64_t *off, int64_t n_texts,
                        uint32_t *new_chars, int64_t new_cap, int64_t *n_new, int64_t *id_hist, int64_t hist_cap);
int bpe_add_lines_batch_device(bpe_ctx *ctx, int mode, const uint16_t *d_units, const int64_t *d_off,
                               int64_t n_texts, uint32_t *new_chars, int64_t new_cap, int64_t *n_new,
                               int64_t *id_hist, int64_t hist_cap);
int bpe_add_lines_utf8_batch(bpe_ctx *ctx, int mode, const uint8_t *bytes, const int64_t *off, int64_t n_texts,
                             uint32_t *new_chars, int64_t new_cap, int64_t *n_new, int64_t *id_hist,
                             int64_t hist_cap);
int bpe_add_lines_utf8_batch_device(bpe_ctx *ctx, int mode, const uint8_t *d_bytes, const int64_t *d_off,
                                    int64_t n_texts, uint32_t *new_chars, int64_t new_cap, int64_t *n_new,
                                    int64_t *id_hist, int64_t hist_cap);
int bpe_restore_lines_batch(bpe_ctx *ctx, bpe_encoder *enc, int mode, const uint16_t *units, const int64_t *off,
                            int64_t n_texts);
int bpe_restore_lines_batch_device(bpe_ctx *ctx, bpe_encoder *enc, int mode, const uint16_t *d_units,
                                   const int64_t *d_off, int64_t n_texts);
int bpe_restore_lines_utf8_batch(bpe_ctx *ctx, bpe_encoder *enc, int mode, const uint8_t *bytes, const int64_t *off,
                                 int64_t n_texts);
int bpe_restore_lines_utf8_batch_device(bpe_ctx *ctx, bpe_encoder *enc, int mode, const uint8_t *d_bytes,
                                        const int64_t *d_off, int64_t n_texts);
int bpe_encoder_get_lines_stats(bpe_encoder *enc, bpe_lines_stats *out);
int bpe_encoder_reset_lines_stats(bpe_encoder *enc);
int bpe_get_lines_stats(bpe_ctx *ctx, bpe_lines_stats *out);
int bpe_reset_lines_stats(bpe_ctx *ctx);

/* ---- text out as UTF-8 ---------------------------------------------------------------------------
 * The ways out of the device that end in text (bpe_decode_batch, bpe_export_text_batch) as UTF-8
 * bytes (files, dataset shards, sockets, byte tensors) instead of UTF-16 units: the units are
 * transcoded to bytes on the device, so a host form brings back 1-3 B per unit already encoded, and
 * with the forms of "text as UTF-8" above bytes -> corpus -> merges -> bytes and bytes -> vectors ->
 * bytes cross PCIe as bytes and offsets only.  Everything here sits on a decoder, its device and
 * stream, and keeps grow-only scratch there (2 B per decoded unit and 8 B per text, besides the
 * transcode's tiles); BPE_ERR_OOM changes nothing.
 *
 * Text k is units[off[k] .. off[k+1]) and encodes on its own, exactly as Node's
 * Buffer.from(str, 'utf8'), TextEncoder.encode(str) and fs.writeFileSync(path, str) encode a JS
 * string (the WHATWG conversion to a USVString, then UTF-8): a high surrogate followed in its text by
 * a low one becomes the four bytes of their code point, any other surrogate EF BF BD (U+FFFD), every
 * other unit one, two or three bytes.  A high surrogate that ends text k and a low one that starts
 * text k + 1 are both lone; U+FEFF is a char like any other (no BOM is added or dropped); a text
 * never makes more than 3 bytes per unit.  On well-formed text this is the inverse of
 * bpe_encoder_utf8_to_utf16.  Lone surrogates are not an error.
 *
 * bpe_decoder_utf16_to_utf8 is the transcode alone.  Offsets follow bpe_encode_text_batch's rules
 * (off[0] need not be 0 and units before it are never read; decreasing or negative offsets give
 * BPE_ERR_ARG with nothing written; n_texts == 0 is fine), capacity follows bpe_decode_batch's:
 * out_off receives n_texts + 1 offsets with out_off[0] = 0; when out_off[n_texts] exceeds bytes_cap
 * the offsets are written, no byte is, and BPE_ERR_ARG comes back (bytes_out == NULL with bytes_cap 0
 * is the sizing call).  bytes_cap >= 3 * (off[n_texts] - off[0]) always suffices.  The `_device`
 * form takes and fills buffers on the decoder's device (any 2-byte aligned unit pointer, any byte
 * pointer), reads the offsets back (8 B per text) and synchronises before returning; *needed (a host
 * int64) receives the bytes.
 *
 * bpe_decode_utf8_batch is bpe_decode_batch_device into the scratch, then that transcode: the
 * decoder's errors and messages come back as they are, with nothing written (`unknown vector index:
 * V (text K, position I)`, `unknown token index: ...`, BPE_ERR_STATE without a vector index).
 * Surrogates pair on the decoded text, as in the reference's `content += token.chars` (core.ts:462-
 * 468): a token that is a lone high surrogate followed by one that is a lone low surrogate becomes one
 * 4-byte sequence.
 *
 * bpe_export_utf8_batch is bpe_export_text_batch's route with bpe_decode_utf8_batch_device in place
 * of the UTF-16 decode: the same idx rules, the same "an export only reads" guarantee, the same
 * decoder-device check.  A multi-device context takes the host form as bpe_export_text_batch does,
 * shard by shard (through the decoder's host form); the device form refuses it with BPE_ERR_ARG.
 *
 * bpe_decoder_get_utf8_stats fills a bpe_utf8_stats read the other way round: calls, and for the
 * calls whose whole pipeline succeeded and wrote its bytes their texts, `units` taken in, `bytes`
 * written, `replaced` (lone surrogates turned into EF BF BD; a U+FFFD unit is not counted) and the
 * HIP-event time of the transcode kernels alone (the decode's is in bpe_decoder_stats).
 * The kernels work on tiles of BPE_UTF16_TILE units and scan BPE_TEXT_SCAN_ROUND tile counts per
 * round (csrc/bpe_utf8_out.hip.h; exported for the tests). */
#define BPE_UTF16_TILE 2048
int bpe_decoder_utf16_to_utf8(bpe_decoder *dec, const uint16_t *units, const int64_t *off, int64_t n_texts,
                              uint8_t *bytes_out, int64_t bytes_cap, int64_t *out_off);
int bpe_decoder_utf16_to_utf8_device(bpe_decoder *dec, const uint16_t *d_units, const int64_t *d_off,
                                     int64_t n_texts, uint8_t *d_bytes_out, int64_t bytes_cap,
                                     int64_t *d_out_off, int64_t *needed);
int bpe_decode_utf8_batch(bpe_decoder *dec, int kind, const int32_t *vals, const int64_t *off, int64_t n_texts,
                          uint8_t *bytes_out, int64_t bytes_cap, int64_t *out_off);
int bpe_decode_utf8_batch_device(bpe_decoder *dec, int kind, const int32_t *d_vals, const int64_t *d_off,
                                 int64_t n_texts, uint8_t *d_bytes_out, int64_t bytes_cap, int64_t *d_out_off,
                                 int64_t *needed);
int bpe_export_utf8_batch(bpe_ctx *ctx, bpe_decoder *dec, const int64_t *idx, int64_t n,
                          uint8_t *bytes_out, int64_t bytes_cap, int64_t *out_off);
int bpe_export_utf8_batch_device(bpe_ctx *ctx, bpe_decoder *dec, const int64_t *idx, int64_t n,
                                 uint8_t *d_bytes_out, int64_t bytes_cap, int64_t *d_out_off, int64_t *needed);
int bpe_decoder_get_utf8_stats(bpe_decoder *dec, bpe_utf8_stats *out);
int bpe_decoder_reset_utf8_stats(bpe_decoder *dec);

/* ---- skip-gram pairs -----------------------------------------------------------------------------
 * What the reference's own consumer of vectors does with them (example/skip-gram.ts:28-47): every text
 * is expanded into (target, context) pairs over a window of `window` values on each side, on the
 * device, so that bytes -> vectors -> training pairs and corpus -> training pairs cross PCIe as nothing
 * or as bytes only, and a framework gets two int32 arrays it can feed to an embedding.
 *
 * For one text with values v[0 .. n) and window w >= 1: for i = 0 .. n - 1 ascending, and for
 * j = i - w .. i + w ascending, skipping j < 0, j == i and j >= n, the pair (target = v[i], context =
 * v[j]).  Token i emits min(i, w) + min(n - 1 - i, w) pairs; a text n (n - 1) pairs if n <= w + 1, else
 * w (2n - w - 1); n = 0 and n = 1 emit nothing; pairs never cross texts.  Values are copied as given
 * (vector indices or ids): the expansion knows no vocabulary.
 * The output is two int32 planes, targets[P] and contexts[P], and n_texts + 1 int64 pair offsets
 * (pair_off[0] = 0, P = pair_off[n_texts]).  Counts and offsets are 64-bit everywhere.  A window outside
 * [1, BPE_SKIPGRAM_MAX_WINDOW] gives BPE_ERR_ARG.
 *
 * Capacity and sizing follow bpe_decode_batch: the offsets are always written; when pair_off[n_texts]
 * exceeds pairs_cap (the pairs each plane holds) no pair is written and BPE_ERR_ARG comes back; NULL
 * planes with pairs_cap 0 are the sizing call.  The `_device` forms take and fill buffers on the
 * owner's device (4-byte aligned values and planes, 8-byte aligned offsets; the planes are stored
 * 16 B per lane when both sit at the same address mod 16, pair by pair otherwise), report *needed (a
 * host int64: P), run on the owner's stream and synchronise before returning.  The host forms are the
 * device forms plus the copies.
 *
 * bpe_encoder_skipgram is the expansion alone: text k is vals[off[k] .. off[k+1]); off[0] need not be 0
 * and values before it are never read; decreasing or negative offsets give BPE_ERR_ARG with nothing
 * written; n_texts == 0 is fine.
 * bpe_skipgram_text_batch and bpe_skipgram_utf8_batch run bpe_encode_text_batch_device /
 * bpe_encode_utf8_batch_device (`kind`: BPE_ENCODE_IDS or BPE_ENCODE_VECTORS) into grow-only scratch of
 * the encoder and expand from there: in the device form no value touches the host.  The encoder's
 * errors, messages and long-text mode are its own (`unknown token, char: U+XXXX (text K, unit I)`,
 * BPE_ERR_STATE without a char table or a vector index, ...), with nothing written.
 * bpe_export_skipgram sends corpus samples through bpe_export_samples_device (kind BPE_EXPORT_IDS or
 * BPE_EXPORT_VECTORS with to_vector_index; idx NULL for every sample) into scratch of the context and
 * expands from there.  It has the export's errors and its read-only guarantee: a bpe_merge_until after
 * it gives the merges it would have given without it.  A multi-device context takes the host form
 * shard by shard (the samples through its host export, the expansion on its first shard's device);
 * the device form refuses it with BPE_ERR_ARG.
 *
 * bpe_skipgram_stats: `calls` counts every call (sizing and failed ones too); the other fields count
 * the calls that wrote their pairs: their texts, the values they read, the pairs they wrote, and the
 * HIP-event time of the two kernels alone (the encode's and the export's stay in their own stats).  A
 * multi-device context reports its first shard's.
 * The expand kernel works on tiles of BPE_SKIPGRAM_TILE pairs, and the scan of the texts' pair counts
 * takes BPE_SKIPGRAM_SCAN_ROUND texts per round (csrc/bpe_skipgram.hip.h; exported for the tests, which
 * place texts around the first and size a batch past the second). */
#define BPE_SKIPGRAM_MAX_WINDOW 64
#define BPE_SKIPGRAM_TILE 2048
#define BPE_SKIPGRAM_SCAN_ROUND 8192
typedef struct {
    int64_t calls;            /* skip-gram calls */
    int64_t texts;            /* texts of the calls that wrote their pairs */
    int64_t values_in;        /* ... their values */
    int64_t pairs_out;        /* ... the pairs written (to each plane) */
    double kernel_ms;         /* HIP-event time of the offsets and expand kernels */
} bpe_skipgram_stats;
int bpe_encoder_skipgram(bpe_encoder *enc, const int32_t *vals, const int64_t *off, int64_t n_texts, int window,
                         int32_t *targets, int32_t *contexts, int64_t pairs_cap, int64_t *pair_off);
int bpe_encoder_skipgram_device(bpe_encoder *enc, const int32_t *d_vals, const int64_t *d_off, int64_t n_texts,
                                int window, int32_t *d_targets, int32_t *d_contexts, int64_t pairs_cap,
                                int64_t *d_pair_off, int64_t *needed);
int bpe_skipgram_text_batch(bpe_encoder *enc, int kind, const uint16_t *units, const int64_t *off, int64_t n_texts,
                            int window, int32_t *targets, int32_t *contexts, int64_t pairs_cap, int64_t *pair_off);
int bpe_skipgram_text_batch_device(bpe_encoder *enc, int kind, const uint16_t *d_units, const int64_t *d_off,
                                   int64_t n_texts, int window, int32_t *d_targets, int32_t *d_contexts,
                                   int64_t pairs_cap, int64_t *d_pair_off, int64_t *needed);
int bpe_skipgram_utf8_batch(bpe_encoder *enc, int kind, const uint8_t *bytes, const int64_t *off, int64_t n_texts,
                            int window, int32_t *targets, int32_t *contexts, int64_t pairs_cap, int64_t *pair_off);
int bpe_skipgram_utf8_batch_device(bpe_encoder *enc, int kind, const uint8_t *d_bytes, const int64_t *d_off,
                                   int64_t n_texts, int window, int32_t *d_targets, int32_t *d_contexts,
                                   int64_t pairs_cap, int64_t *d_pair_off, int64_t *needed);
int bpe_export_skipgram(bpe_ctx *ctx, int kind, const int64_t *idx, int64_t n, const int32_t *to_vector_index,
                        int32_t n_index, int window, int32_t *targets, int32_t *contexts, int64_t pairs_cap,
                        int64_t *pair_off);
int bpe_export_skipgram_device(bpe_ctx *ctx, int kind, const int64_t *idx, int64_t n, const int32_t *to_vector_index,
                               int32_t n_index, int window, int32_t *d_targets, int32_t *d_contexts,
                               int64_t pairs_cap, int64_t *d_pair_off, int64_t *needed);
int bpe_encoder_get_skipgram_stats(bpe_encoder *enc, bpe_skipgram_stats *out);
int bpe_encoder_reset_skipgram_stats(bpe_encoder *enc);
int bpe_get_skipgram_stats(bpe_ctx *ctx, bpe_skipgram_stats *out);
int bpe_reset_skipgram_stats(bpe_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* BPE_H */
