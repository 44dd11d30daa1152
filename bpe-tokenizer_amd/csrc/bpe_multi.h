// bpe_multi.h — internal: one corpus sharded over several HIP devices behind one bpe_ctx
// (bpe_create_multi, include/bpe.h).  bpe_engine.hip forwards every C-ABI call made on such a
// context here; the shards are ordinary single-device contexts driven through the same C ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "bpe.h"

struct bpe_multi;

int multi_create(bpe_multi **out, int n_shards, const int *devices, int reduce);
int multi_destroy(bpe_multi *m);
int multi_set_token_len16(bpe_multi *m, int32_t id, int32_t len16);
int multi_num_tokens(bpe_multi *m, int32_t *n);
int multi_add_sample(bpe_multi *m, const int32_t *ids, int64_t n);
int multi_add_latin1(bpe_multi *m, const uint8_t *bytes, int64_t n, int64_t sample_bytes,
                     int32_t char_to_id[256], int32_t *n_tokens_io, int64_t char_hist[256]);
int multi_set_chars(bpe_multi *m, const uint32_t *code_points, const int32_t *ids, int64_t n);
int multi_add_text_batch(bpe_multi *m, const uint16_t *units, const int64_t *off, int64_t n_texts, bool dev,
                         uint32_t *new_chars, int64_t new_cap, int64_t *n_new, int64_t *id_hist,
                         int64_t hist_cap);
int multi_get_ingest_stats(bpe_multi *m, bpe_ingest_stats *out);
int multi_reset_ingest_stats(bpe_multi *m);
int multi_add_sample_batch(bpe_multi *m, const int32_t *ids, const int64_t *off, int64_t n, bool dev);
int multi_restore_text_batch(bpe_multi *m, bpe_encoder *enc, const uint16_t *units, const int64_t *off,
                             int64_t n_texts, bool dev);
int multi_token_counts(bpe_multi *m, int64_t *counts, int64_t cap);
int multi_get_append_stats(bpe_multi *m, bpe_append_stats *out);
int multi_reset_append_stats(bpe_multi *m);
int multi_export_samples(bpe_multi *m, int kind, const int64_t *idx, int64_t n, const int32_t *to_vector_index,
                         int32_t n_index, void *vals_out, int64_t vals_cap, int64_t *out_off);
int multi_export_text_batch(bpe_multi *m, bpe_decoder *dec, const int64_t *idx, int64_t n, uint16_t *units_out,
                            int64_t units_cap, int64_t *out_off);
int multi_export_utf8_batch(bpe_multi *m, bpe_decoder *dec, const int64_t *idx, int64_t n, uint8_t *bytes_out,
                            int64_t bytes_cap, int64_t *out_off);
// the samples' ids or vector indices assembled on the host (sized, then filled: one export call),
// for the skip-gram expansion of a multi-device context (bpe_engine.hip)
int multi_export_values(bpe_multi *m, int kind, const int64_t *idx, int64_t n, const int32_t *to_vector_index,
                        int32_t n_index, std::vector<int32_t> &vals, std::vector<int64_t> &off);
int multi_get_export_stats(bpe_multi *m, bpe_export_stats *out);
int multi_reset_export_stats(bpe_multi *m);
int multi_clear_corpus(bpe_multi *m);
int multi_corpus_size(bpe_multi *m, int64_t *n_samples, int64_t *n_tokens);
int multi_read_corpus(bpe_multi *m, int32_t *ids_out, int64_t ids_cap, int64_t *sample_off,
                      int64_t off_cap);
int multi_sample_lengths(bpe_multi *m, int64_t *lens, int64_t cap);
int multi_read_samples(bpe_multi *m, const int64_t *idx, int64_t n, int32_t *ids_out,
                       int64_t ids_cap, int64_t *off);
int multi_find_next_merge(bpe_multi *m, int64_t max_length, int64_t min_weight, int32_t *a,
                          int32_t *b, int64_t *w);
int multi_apply_merge(bpe_multi *m, int32_t a, int32_t b, int32_t c, int64_t *replaced);
int multi_apply_merges(bpe_multi *m, const int32_t *abc, int64_t n, int64_t *replaced,
                       int count_after);
int multi_merge_until(bpe_multi *m, int64_t max_length, int64_t min_weight,
                      int64_t max_iterations, int64_t *out_abw, int64_t cap, int64_t *n_merges);
int multi_stats_enable(bpe_multi *m, int on);
int multi_get_stats(bpe_multi *m, bpe_stats *out);
int multi_reset_stats(bpe_multi *m);
int multi_get_stream(bpe_multi *m, void **stream);
int multi_shard_count(bpe_multi *m, int *n);
// (bpe_tools.h bpe_debug_pix_shard) the position index of one shard, for checking
int multi_debug_pix_shard(bpe_multi *m, int shard, int64_t *info, void *const *arrays);
// (bpe_tools.h bpe_debug_tables_shard, bpe_debug_global) one shard's copy of the global tables and
// what it holds of the streaming mode's maintained state, for checking
int multi_debug_tables_shard(bpe_multi *m, int shard, uint64_t *hot, uint32_t *keys,
                             uint64_t *counts, int64_t cap, int64_t *n);
int multi_debug_global(bpe_multi *m, int shard, int64_t *info, uint64_t *xchg, int64_t cap);
// the shard whose device and stream a multi-device context's UTF-8 ingest transcodes on
bpe_ctx *multi_first_shard(bpe_multi *m);
// explicit_choice: the caller's bpe_set_mode (false: the automatic switch past AUTO_PIX_VOCAB ids)
int multi_set_mode(bpe_multi *m, int mode, bool explicit_choice = true);

// shards that share one device exchange through a device kernel (bpe_engine.hip)
constexpr int BPE_MAX_SHARDS_ONE_DEVICE = 16;
extern "C" int bpe_sum_shards(unsigned long long *const *bufs, int n, size_t count, int take_max,
                              void *stream);

// (bpe_multi.cpp) a context going away frees its rank communicator (bpe_rank_rccl_init)
void rank_rccl_forget(bpe_ctx *ctx);

// (bpe_engine.hip) the exchange and tie buffers and the exchange's word count of the context's
// open rank-loop batch (bpe_rank_loop_begin); BPE_ERR_STATE when no batch is open
int rank_loop_buffers(bpe_ctx *c, unsigned long long **xchg, unsigned long long **tie, int64_t *words);

// (bpe_engine.hip) the text ingest of one shard (bpe_add_text_batch): the whole pipeline, or with
// number_only the new chars numbered and reported, every check made and nothing changed;
// ingest_learn registers new char tokens (ids from the token count on) and puts them into the
// shard's char table; ingest_kernel_ms reads (and with reset clears) the shard's counters
int ingest_text(bpe_ctx *c, const uint16_t *units, const int64_t *off, int64_t n_texts, bool dev, bool number_only,
                uint32_t *new_chars, int64_t new_cap, int64_t *n_new, int64_t *id_hist, int64_t hist_cap);
int ingest_learn(bpe_ctx *c, const uint32_t *code_points, int64_t n);
int ingest_kernel_ms(bpe_ctx *c, double *ms, bool reset);

// (bpe_encode.hip) the device an encoder lives on (the restore checks it against the context's; the
// encoder's struct stays private)
int encoder_device(bpe_encoder *enc, int *device);
// (bpe_encode.hip) the restore from UTF-8: the texts transcoded on the encoder, their units and
// offsets left in its scratch on its device; encoder_utf8_done counts that transcode in the
// encoder's bpe_utf8_stats once the restore has succeeded
int encoder_utf8_units(bpe_encoder *enc, const uint8_t *bytes, const int64_t *off, int64_t n_texts, bool dev,
                       const uint16_t **d_units, const int64_t **d_uoff, int64_t *n_units);
void encoder_utf8_done(bpe_encoder *enc);
// (bpe_encode.hip) the restore from lines: the texts (units, or with utf8 bytes transcoded first)
// split into samples on the encoder, their units and offsets left in its scratch on its device;
// encoder_lines_done counts the call in the encoder's counters once the restore has succeeded
int encoder_lines_units(bpe_encoder *enc, int mode, const void *src, const int64_t *off, int64_t n_texts, bool dev,
                        bool utf8, const uint16_t **d_units, const int64_t **d_uoff, int64_t *n_samples,
                        int64_t *n_units);
void encoder_lines_done(bpe_encoder *enc);
// (bpe_decode.hip) the same for a decoder (the text export checks it)
int decoder_device(bpe_decoder *dec, int *device);

// error reporting shared with bpe_engine.hip
int bpe_fail(int code, const char *msg);
