/*
 * bpe_tools.h — benchmark/test utilities exported by libbpe (not part of the reference boundary).
 */
#ifndef BPE_TOOLS_H
#define BPE_TOOLS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Synthetic corpus of SURVEY.md §8(d): xorshift32 (x ^= x<<13; x ^= x>>17; x ^= x<<5) from
 * `seed`, skipping the first `skip` outputs (GF(2) jump-ahead, so a shard can be generated
 * without its prefix), byte = base + floor(x * A / 2^32).  Writes n bytes. */
int bpe_synth_latin1(uint32_t seed, uint32_t A, uint32_t base, uint64_t skip, uint8_t *out,
                     int64_t n);

/* Skewed variant of the synthetic corpus (Zipf s=1.1 words, the worst case for
 * counter contention and for pairs of merged tokens): a list of n_words words, word w of 2..8
 * letters a-z from its own xorshift32 stream; each sample of sample_bytes bytes is a stream of
 * words drawn with P(rank r) ∝ r^-s, each followed by '\n' (1 in 16) or ' ', cut at the sample
 * end.  Sample k depends only on (seed, k), so a shard starting at sample `first_sample` is
 * generated without its prefix.  Writes n bytes (samples first_sample, first_sample + 1, ...). */
int bpe_synth_zipf(uint32_t seed, double s, uint32_t n_words, uint64_t first_sample,
                   int64_t sample_bytes, uint8_t *out, int64_t n);

/* Forces one plain streaming count pass over the current corpus (no merge applied): what
 * findNextMerge does when no counts are cached.  For measuring K1 alone. */
struct bpe_ctx;
int bpe_recount(struct bpe_ctx *ctx);

/* The maintained tables of a single-device context, copied out for checking: the HOT_BINS (65536)
 * u64 hot bins into `hot` (pair (a, b) with both ids below 256 at b * 256 + a) and the cold
 * table's dense entries into keys / counts (key a << 16 | b, 0xFFFFFFFF = a hole; a count of 0 =
 * a claim whose pair is gone), up to `cap` of them; *n = the entries in use.  Two calls: cap 0
 * (keys and counts may be null) for *n, then with room.  BPE_ERR_ARG for a multi-device context
 * and for null arguments.  What the tables mean is bpe_table_state's matter. */
int bpe_debug_tables(struct bpe_ctx *ctx, uint64_t *hot, uint32_t *keys, uint64_t *counts,
                     int64_t cap, int64_t *n);

/* *maintained = 1 while the context holds the single-context maintained state (the hot bins and
 * the cold table hold the exact count of every pair of the corpus and are kept so merge by
 * merge), else 0.  A pending merge's replacement count is settled first; nothing else changes.
 * BPE_ERR_ARG for a multi-device context and for null arguments. */
int bpe_table_state(struct bpe_ctx *ctx, int *maintained);

/* bpe_debug_tables for shard `shard` of a multi-device context: that shard's own copy of the
 * tables (in the streaming mode's sharded maintained state every shard holds a copy of the global
 * tables; what they hold between two batches is bpe_debug_global's matter).  The same two calls.
 * The call synchronises the shard's stream, launches nothing and changes nothing.  BPE_ERR_ARG for
 * a single-device context, a bad shard and null arguments. */
int bpe_debug_tables_shard(struct bpe_ctx *ctx, int shard, uint64_t *hot, uint32_t *keys,
                           uint64_t *counts, int64_t cap, int64_t *n);

/* What a context holds of the sharded maintained state of the streaming mode (the "global state":
 * bpe_set_global_counts, then the rank loop keeps the tables with delta rows), for shard `shard` of
 * a multi-device context or, with shard == -1, for a single-device context used as one rank
 * (bpe_rank_loop_*).  info receives BPE_GLOBAL_INFO_WORDS int64 words:
 *   HELD      1 while the context holds the global tables of the streaming mode, else 0 (the
 *             incremental mode's global state, a shard's position index, is bpe_debug_pix's)
 *   PENDING   1 while the last batch's last merge is applied to the corpus and zeroed in the tables
 *             (every pair with a side a or b), but its recount, this shard's delta rows, still
 *             waits in the exchange buffer for the next batch's first all-reduce
 *   A B C W   that merge (a, b) -> c and its weight; -1 each when none is pending
 *   MULTI     the multi-device context's own flag that its batches run in the maintained state
 *             (either mode); -1 for a single-device context
 *   XCHG      the words of the exchange buffer that can be copied: BPE_XCHG_WORDS while HELD and a
 *             batch was begun, else 0
 * and xchg a copy of the exchange buffer the context last began a batch with, word for word
 * (include/bpe.h BPE_XCHG_*: word 0 this shard's replacement count of the pending merge, the delta
 * rows from BPE_XCHG_HDR on).  Two calls, like bpe_debug_tables: cap 0 (xchg may be null) for
 * info, then with cap >= info[XCHG].  The call synchronises the context's stream, launches nothing
 * and changes nothing.  BPE_ERR_ARG for null arguments, a bad shard, a shard other than -1 with a
 * single-device context, and a cap between 1 and info[XCHG] - 1. */
enum {
    BPE_GLOBAL_INFO_HELD = 0, BPE_GLOBAL_INFO_PENDING = 1, BPE_GLOBAL_INFO_A = 2,
    BPE_GLOBAL_INFO_B = 3, BPE_GLOBAL_INFO_C = 4, BPE_GLOBAL_INFO_W = 5, BPE_GLOBAL_INFO_MULTI = 6,
    BPE_GLOBAL_INFO_XCHG = 7, BPE_GLOBAL_INFO_WORDS = 8
};
int bpe_debug_global(struct bpe_ctx *ctx, int shard, int64_t *info, uint64_t *xchg, int64_t cap);

/* The live position index of the incremental mode (csrc/bpe_pix.hip.h), copied out for checking.
 * Two calls, like bpe_debug_tables: with arrays == NULL the sizes and scalars into info
 * (BPE_PIX_INFO_WORDS int64 words, BPE_PIX_INFO_* below; info[BPE_PIX_INFO_PRESENT] = 0 and the
 * rest zero when the context holds no index), then with the same info and BPE_PIX_ARRAYS host
 * pointers, in this order and of these element counts:
 *   tok (int32, n)  nxt, prv (uint32, n)                          the slot array and its links
 *   keys (uint32, cap)  cnt (uint64, cap)  off, len, fill (uint32, cap)   the pair table
 *   bmax (uint64, nblocks)  sbmax (uint64, nsuper)  bdirty (uint32, nblocks)  sbdirty (uint32, nsuper)
 *   pool (uint32, pool_top)  dblocks (uint32, n_dblocks)  dsuper (uint32, n_dsuper)
 * The second call fails with BPE_ERR_ARG when the index is gone or no longer has the sizes and
 * scalars of info.  The call synchronises the context's stream and launches nothing.  BPE_ERR_ARG
 * for null arguments and for a multi-device context.  In a single context the index lives only
 * inside bpe_merge_until: see bpe_debug_pix_hook. */
enum {
    BPE_PIX_INFO_PRESENT = 0, BPE_PIX_INFO_N = 1, BPE_PIX_INFO_CAP = 2, BPE_PIX_INFO_NBLOCKS = 3,
    BPE_PIX_INFO_NSUPER = 4, BPE_PIX_INFO_ML = 5, BPE_PIX_INFO_STATUS = 6, BPE_PIX_INFO_TIE = 7,
    BPE_PIX_INFO_ERR = 8, BPE_PIX_INFO_USED = 9, BPE_PIX_INFO_USED_CAP = 10,
    BPE_PIX_INFO_POOL_TOP = 11, BPE_PIX_INFO_POOL_CAP = 12, BPE_PIX_INFO_N_DBLOCKS = 13,
    BPE_PIX_INFO_N_DSUPER = 14, BPE_PIX_INFO_NEXT_ID = 15, BPE_PIX_INFO_MERGED = 16,
    BPE_PIX_INFO_N_DONE = 17,
    BPE_PIX_INFO_SHARDED = 18,        /* a shard's index: cnt holds the global counts */
    BPE_PIX_INFO_DELTA_PENDING = 19,  /* ... whose last merge's delta rows are not added yet */
    BPE_PIX_INFO_PAIR_SLOT = 20, BPE_PIX_INFO_MAX_ID = 21,
    BPE_PIX_INFO_WORDS = 24, BPE_PIX_ARRAYS = 15
};
int bpe_debug_pix(struct bpe_ctx *ctx, int64_t *info, void *const *arrays);

/* The same for shard `shard` of a multi-device context, whose shards keep their indices between
 * the batches and the calls of bpe_merge_until in the incremental mode, until something reads or
 * changes the corpus.  BPE_ERR_ARG for a single-device context, a bad shard and null arguments. */
int bpe_debug_pix_shard(struct bpe_ctx *ctx, int shard, int64_t *info, void *const *arrays);

/* Checking a single context's index while it lives: bpe_merge_until in the incremental mode calls
 * hook(user, 0) after an index build or after the room for the next batch was reserved (the pool
 * grown, the table rehashed), before the batch starts, and hook(user, 1) after a batch's host
 * synchronisation and merge accounting; the hook may call bpe_debug_pix and must change nothing.
 * batch (1 to 256; 0: the default, 256) is the number of iterations per batch for this context:
 * with 1 the index is seen after every merge, and between a tie's scan and its commit.
 * hook == NULL removes the hook.  BPE_ERR_ARG for a multi-device context and a bad batch. */
int bpe_debug_pix_hook(struct bpe_ctx *ctx, void (*hook)(void *user, int where), void *user,
                       int64_t batch);

#ifdef __cplusplus
}
#endif
#endif
